"""Checks of the crop sampler and the `-tf fast` chain (csrc/sampler_crop.h, sampler_crop_adjoint.h, sampler_warp.h: aph_sample_fwd / aph_sample_bwd)
shared by the interpreter tests (test_emu_sampler.py) and the GPU tests (test_gpu_sampler.py).  `lib` = a loaded C-ABI library (the interpreter
build) or None (the product), `dev` = where its tensors live.

Truth: tests/sampler_ref.py -- float32 source coordinates (they are part of the operation), everything after them float64.  Tolerance, per case
and per quantity (raw image, normalised image, the gradient of each): max |kernel - reference| <= MARGIN x max |fp32 oracle - reference|, the
oracle being the untouched R.slice_imgs / augment_ref of oracle/, run in float32 with autograd; measured here, never taken from the kernel and
never a literal.  Both are float32 evaluations of one map on shared coordinates, and both maps are continuous in them: EVERY element is compared.
The f16 layouts are held to the f16 rounding of the reference value plus one f16 ulp plus that bound.  Every output, gradient and workspace
buffer sits between NaN guard bands and is pre-filled with NaN.  A dropped tap of weight 5e-5, a clamp or a search box off by one, a missing
mask factor do not fit in the bound (the mutation table in DESIGN.md section 2 a-8b, `PYTHONPATH=. python tests/sampler_checks.py`)."""
import math

import numpy as np
import torch

from aphantasia_amd import _ffi, ops
from aphantasia_amd import transforms as T
from oracle import augment_ref
from oracle import reference_path as R
import sampler_ref
from tf_checks import MARGIN, banded, bands_intact, f16_ulp, from_patch_rows, to_patch_rows

FWD_MODES = {'nchw_raw': _ffi.APH_OUT_NCHW_RAW, 'nchw_norm': _ffi.APH_OUT_NCHW_NORM, 'patch_f16': _ffi.APH_OUT_PATCH_F16,
             'patch_f32': _ffi.APH_OUT_PATCH_F32, 'patch_f16_hilo': _ffi.APH_OUT_PATCH_F16_HILO}
BWD_MODES = {'nchw_raw': _ffi.APH_OUT_NCHW_RAW, 'nchw_norm': _ffi.APH_OUT_NCHW_NORM, 'patch_f16': _ffi.APH_OUT_PATCH_F16,
             'patch_f32': _ffi.APH_OUT_PATCH_F32, 'grad_patch_f16': _ffi.APH_GRAD_PATCH_F16}
PATCH_ONLY = ('patch_f16', 'patch_f32', 'patch_f16_hilo', 'grad_patch_f16')
# (rb, cpt, nbc, nseg, order) of aph_crop_adjoint_set_shape, as kernel_checks.CROP_ADJOINT_SHAPES lists them (the first there is the automatic shape)
CROP_ADJOINT_SHAPES = ((4, 2, 12, 1, 0), (16, 3, 5, 1, 1), (13, 2, 1, 2, 1), (9, 3, 12, 3, 0), (16, 2, 3, 1, 1))
GSCALE = 0.375        # the second gradient scale (the first is 1)
RATIOS = []           # (case, quantity, layout, kernel path, max |kernel - reference|, max |fp32 oracle - reference|) of every check run in this process


# ---------------------------------------------------------------------------- cases
def _base(H, W, size, Hp, Wp, table):
    """one up-sampling cut, one of scale exactly 1, one of cs == size + 1, one of cs == min(H, W) flush against the right and bottom edges"""
    m = min(H, W)
    table[0] = (size - 3, 1, 2)
    table[1] = (size, 5, 3)
    table[2] = (size + 1, Wp - size - 2, 4)
    table[3] = (m, Wp - m, Hp - m)


def _segments(H, W, size, Hp, Wp, table):
    """column segments of 152 (nseg 2) and 100 (nseg 3) pixels: cuts that straddle the boundaries at 100, 152 and 200, one flush right; every
    cut (<= 40 wide) misses at least one segment"""
    table[0] = (36, 90, 2)
    table[1] = (34, 140, 3)
    table[2] = (40, 260, 0)
    table[3] = (33, 180, 7)


def _tiny9(H, W, size, Hp, Wp, table):
    """9 rows leave the draw one cut size, 8 = the output's (an exact copy: nothing to bound): every other cut takes all 9 rows"""
    for k in range(0, len(table), 2):
        table[k] = (9, int(table[k][1]) % (Wp - 8), k % (Hp - 8))


# name -> (H, W, S, size, patch, align, image, adjoint shapes, hand cuts, layouts or None = all)
CROP_CASES = {
    'base-uniform': (40, 56, 6, 16, 8, 'uniform', 'noise', CROP_ADJOINT_SHAPES, _base, None),
    'base-central': (40, 56, 6, 16, 8, 'central', 'smooth', CROP_ADJOINT_SHAPES[:2], _base, None),
    'base-overscan': (40, 56, 6, 16, 8, 'overscan', 'noise', (), _base, None),
    'base-overmax': (40, 56, 6, 16, 8, 'overmax', 'noise', (), _base, None),
    'tiny-23x37': (23, 37, 14, 8, 4, 'overmax', 'noise', (), None, None),
    'tiny-9x72': (9, 72, 14, 8, 4, 'overscan', 'noise', (), _tiny9, None),
    'tiny-13x72': (13, 72, 14, 8, 4, 'overscan', 'noise', (), None, None),
    'many_rows': (20, 24, 530, 8, 4, 'uniform', 'noise', (), None, None),           # > 512 cuts: the row kernel's list chunks; 1060 strip units
    'many_aliases': (20, 24, 300, 8, 4, 'overmax', 'noise', (), None, None),        # 1200 aliases: the gather kernel's list chunks
    'trips-72': (80, 90, 4, 72, 8, 'uniform', 'noise', (), None, None),             # column trips 2 .. 4 of the row kernel's column pass
    'trips-136': (140, 150, 4, 136, 8, 'uniform', 'noise', (), None, None),
    'trips-200': (210, 216, 4, 200, 8, 'uniform', 'noise', (), None, None),
    'lds-224': (232, 250, 14, 224, 32, 'uniform', 'noise', (), None, None),         # nbc lowered to 11: two batches
    'lds-256': (260, 270, 14, 256, 32, 'uniform', 'noise', ((16, 2, 0, 1, 1),), None, None),
    'fallback': (270, 280, 3, 264, 8, 'uniform', 'noise', (), None, None),          # size > 256: the gather kernel
    'segments': (40, 300, 8, 32, 16, 'uniform', 'noise', ((0, 0, 0, 1, -1), (0, 0, 0, 2, -1), (0, 0, 0, 3, -1)), _segments, None),
    'patches-1': (70, 76, 3, 64, 1, 'uniform', 'noise', (), None, PATCH_ONLY),      # the extremes of Layout::col_of's multiply-shift division
    'patches-2': (70, 76, 3, 64, 2, 'uniform', 'noise', (), None, PATCH_ONLY),
    'patches-32': (70, 76, 3, 64, 32, 'uniform', 'noise', (), None, PATCH_ONLY),
    'patches-64': (70, 76, 3, 64, 64, 'uniform', 'noise', (), None, PATCH_ONLY),
    'patches-96x2': (100, 104, 3, 96, 2, 'uniform', 'noise', (), None, PATCH_ONLY),
}


def _persp(n, corners):
    """end points at the extremes of perspective_get_params' ranges (distortion 0.33): 'in' = the corner pulled in as far as a draw can, 'out' = left"""
    d = int(0.33 * (n // 2))
    lo, hi = {'in': d, 'out': 0}, {'in': n - d - 1, 'out': n - 1}
    tl, tr, br, bl = corners
    end = [[lo[tl[0]], lo[tl[1]]], [hi[tr[0]], lo[tr[1]]], [hi[br[0]], hi[br[1]]], [lo[bl[0]], hi[bl[1]]]]
    start = [[0, 0], [n - 1, 0], [n - 1, n - 1], [0, n - 1]]
    return augment_ref.perspective_coeffs(start, end)


IN, OUT = ('in', 'in'), ('out', 'out')
KEYSTONE = (IN, OUT, OUT, ('in', 'out'))                             # the left side shrunk to its shortest
TWIST = (('in', 'out'), ('out', 'in'), ('in', 'out'), ('out', 'in'))   # every corner moved along one side only, in turn


def _fast_hand_a(n):
    return [dict(persp=_persp(n, KEYSTONE), erase=None, angle=None),                                  # the largest distortions a draw can give
            dict(persp=_persp(n, (IN, IN, IN, IN)), erase=None, angle=None),
            dict(persp=_persp(n, (OUT, OUT, OUT, OUT)), erase=None, angle=None),                      # the identity homography
            dict(persp=None, erase=None, angle=-30.0),
            dict(persp=None, erase=None, angle=30.0),
            dict(persp=None, erase=None, angle=45.0),                                                 # the adjoint's 3 x 3 box at its widest
            dict(persp=None, erase=None, angle=90.0),
            dict(persp=None, erase=None, angle=None)]                                                 # no stage at all


def _fast_hand_b(n):
    return [dict(persp=None, erase=None, angle=0.0),                                                  # the identity resample
            dict(persp=None, erase=(0, 0, n // 3, n // 2), angle=None),
            dict(persp=None, erase=(n - n // 3, n - n // 4, n // 3, n // 4), angle=None),             # flush against the far corner
            dict(persp=None, erase=(n // 2, 3, 1, n - 5), angle=None),                                # height 1
            dict(persp=None, erase=(2, n - 1, n - 4, 1), angle=None),                                 # width 1, the last column
            dict(persp=_persp(n, TWIST), erase=(n // 4, n // 3, n // 3, n // 2), angle=-30.0),        # all three stages
            dict(persp=_persp(n, KEYSTONE), erase=(0, 0, 1, n - 1), angle=17.0),
            dict(persp=_persp(n, TWIST), erase=None, angle=45.0)]


def _fast_drawn(n):
    """draws of oracle.augment_ref.draw_fast_params under a fixed seed (the reference's own stream)"""
    st_t, st_n = torch.get_rng_state(), np.random.get_state()
    torch.manual_seed(41)
    np.random.seed(41)
    prms = [augment_ref.draw_fast_params(n) for _ in range(8)]
    torch.set_rng_state(st_t)
    np.random.set_state(st_n)
    return prms


def _fast_224(n):
    return [dict(persp=_persp(n, KEYSTONE), erase=(50, 0, 60, 90), angle=-30.0),
            dict(persp=None, erase=(n - 40, n - 70, 40, 70), angle=45.0),
            dict(persp=_persp(n, TWIST), erase=None, angle=0.0)]


# name -> (H, W, S, size, patch, align, image, parameters)
FAST_CASES = {
    'fast_a-uniform': (40, 56, 8, 32, 16, 'uniform', 'smooth', _fast_hand_a),
    'fast_b-uniform': (40, 56, 8, 32, 16, 'uniform', 'smooth', _fast_hand_b),
    'fast_drawn-uniform': (40, 56, 8, 32, 16, 'uniform', 'smooth', _fast_drawn),
    'fast_a-overscan': (40, 56, 8, 32, 16, 'overscan', 'smooth', _fast_hand_a),
    'fast_b-overscan': (40, 56, 8, 32, 16, 'overscan', 'smooth', _fast_hand_b),
    'fast_drawn-overscan': (40, 56, 8, 32, 16, 'overscan', 'smooth', _fast_drawn),
    'fast-224': (232, 250, 3, 224, 32, 'uniform', 'smooth', _fast_224),
}


def smooth_image(H, W, seed):
    """a few low-frequency sinusoids, different per channel, values in [0.2, 0.8]"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
    img = np.zeros((3, H, W))
    for c in range(3):
        for _ in range(3):
            fy, fx, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 2 * math.pi)
            img[c] += np.sin(2 * math.pi * (fy * y + fx * x) + ph) / 3.0
    return torch.from_numpy(0.5 + 0.3 * img).float()


class Case:
    """inputs of one case, the float64 reference and the float32 oracle of its four quantities, computed once and left unchanged"""
    _cache = {}

    @classmethod
    def get(cls, name):
        if name not in cls._cache:
            cls._cache[name] = cls(name)
        return cls._cache[name]

    def __init__(self, name):
        self.name = name
        if name in CROP_CASES:
            self.H, self.W, self.S, self.n, self.patch, self.align, image, self.shapes, hand, self.layouts = CROP_CASES[name]
            make_prms = None
        else:
            self.H, self.W, self.S, self.n, self.patch, self.align, image, make_prms = FAST_CASES[name]
            self.shapes, hand, self.layouts = (), None, None
        H, W, S, n = self.H, self.W, self.S, self.n
        seed = 100 + sorted(list(CROP_CASES) + list(FAST_CASES)).index(name)
        gen = torch.Generator().manual_seed(seed)
        self.img = smooth_image(H, W, seed) if image == 'smooth' else torch.rand(3, H, W, generator=gen)
        st = torch.get_rng_state()
        torch.manual_seed(seed)
        self.table = R.draw_crop_table(S, n, H, W, self.align, 0.4)
        torch.set_rng_state(st)
        self.geom = ops.make_geom(H, W, S, n, self.patch, self.align)
        if hand is not None:
            hand(H, W, n, self.geom.Hp, self.geom.Wp, self.table)
        assert all(cs <= min(H, W) and ox >= 0 and oy >= 0 and ox + cs <= self.geom.Wp and oy + cs <= self.geom.Hp for cs, ox, oy in self.table)
        self.prms, self.aug = None, None
        if make_prms is not None:
            self.prms = make_prms(n)
            assert len(self.prms) == S
            prev = T._EXACT_ZERO_ROT
            T._EXACT_ZERO_ROT = True            # a 0-degree cut is resampled through the identity grid, as the oracle (and torchvision) does
            try:
                self.aug = T.pack_aug([dict(p) for p in self.prms])
            finally:
                T._EXACT_ZERO_ROT = prev
        # gradient of the output: f16-representable, so the f16 gradient layout carries the same values
        self.g = torch.randn(S, 3, n, n, generator=gen).half().float()
        self.ref = self._reference()
        self.oracle = self._oracle()

    def sampler(self):
        return sampler_ref.Sampler(self.H, self.W, self.table, self.n, self.align, self.prms)

    def _reference(self):
        smp, g = self.sampler(), self.g.double().numpy()
        raw = smp.forward(self.img.double().numpy())
        out = dict(raw=raw, norm=sampler_ref.normalise(raw), d_raw=smp.adjoint(g), d_norm=smp.adjoint(sampler_ref.normalise_adjoint(g)))
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def _oracle(self):
        """the untouched float32 oracle and autograd through it, as float64"""
        img = self.img[None].clone().requires_grad_(True)
        prms = self.prms

        def per_cut(c, cut):
            p = prms[c]
            if p['angle'] is not None:
                return augment_ref.apply_fast(cut, p, lambda x: x)
            if p['persp'] is not None:
                cut = augment_ref.perspective(cut, p['persp'])
            return augment_ref.erase(cut, p['erase']) if p['erase'] is not None else cut
        raw = R.slice_imgs(img, self.table, self.n, self.align, transform=None, per_cut=per_cut if prms is not None else None)
        norm = R.normalize(raw)
        out = dict(raw=raw.detach().double(), norm=norm.detach().double())
        for key, y in (('d_raw', raw), ('d_norm', norm)):
            out[key] = torch.autograd.grad((y * self.g).sum(), img, retain_graph=True)[0][0].double()
        return out

    def bound(self, key):
        gap = (self.oracle[key] - self.ref[key]).abs().max().item()
        assert gap > 0, 'the float32 oracle equals the float64 reference: no bound to take'
        return gap


def cases():
    """every case runs under the interpreter and on the GPU (the largest adjoint check, lds-256, takes 25 s under the interpreter)"""
    return list(CROP_CASES) + list(FAST_CASES)


def mode_cases():
    """(case, forward layout) and (case, gradient layout)"""
    def lay(c, modes):
        only = CROP_CASES[c][9] if c in CROP_CASES else None
        return [m for m in modes if only is None or m in only]
    fwd = [(c, m) for c in cases() for m in lay(c, FWD_MODES)]
    bwd = [(c, m) for c in cases() for m in lay(c, BWD_MODES)]
    return fwd, bwd


def case_id(c):
    return '-'.join(str(v) for v in c)


# ---------------------------------------------------------------------------- running the kernels between guard bands
def run_fwd(lib, dev, case, mode):
    shape, dtype = ops.sample_out_shape(case.geom, mode)
    big, flat = banded(int(np.prod(shape)), dtype, dev)
    ws = ops.sample_ws(case.geom, case.aug is not None, dev, lib)
    wbig, wflat = banded(ws.numel(), torch.float32, dev)
    out = ops.sample_fwd(case.geom, case.img.contiguous().to(dev), torch.from_numpy(case.table).to(dev), None if case.aug is None else case.aug.to(dev),
                         wflat, flat.view(shape), mode, lib=lib)
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bands_intact(big) and bands_intact(wbig), 'a write outside the output or the workspace'
    assert not torch.isnan(out.float()).any(), 'an output element was not written'
    return out.cpu()


def run_bwd(lib, dev, case, mode, gout, gscale):
    big, flat = banded(3 * case.H * case.W, torch.float32, dev)
    ws = ops.sample_ws(case.geom, case.aug is not None, dev, lib)
    wbig, wflat = banded(ws.numel(), torch.float32, dev)
    out = ops.sample_bwd(case.geom, gout.contiguous().to(dev), torch.from_numpy(case.table).to(dev), None if case.aug is None else case.aug.to(dev),
                         wflat, flat.view(3, case.H, case.W), mode, gscale=gscale, lib=lib)
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bands_intact(big) and bands_intact(wbig), 'a write outside the gradient or the workspace'
    assert not torch.isnan(out).any(), 'a gradient element was not written'
    return out.cpu()


def _note(dev, case, quantity, layout, path, err, gap):
    RATIOS.append((case.name, quantity, layout, path, err, gap))
    print('sampler_fp64 %s %s %s %s %s: kernel %.3e oracle %.3e ratio %.2f' % ('emu' if dev == 'cpu' else 'gpu', case.name, quantity, layout, path, err, gap, err / gap))


# ---------------------------------------------------------------------------- parity
def check_forward(lib, dev, name, mode_name):
    case = Case.get(name)
    mode, n, S, p = FWD_MODES[mode_name], case.n, case.S, case.patch
    out = run_fwd(lib, dev, case, mode)
    key = 'raw' if mode == _ffi.APH_OUT_NCHW_RAW else 'norm'
    want, gap = case.ref[key], case.bound(key)
    if mode in (_ffi.APH_OUT_NCHW_RAW, _ffi.APH_OUT_NCHW_NORM, _ffi.APH_OUT_PATCH_F32):
        got = (from_patch_rows(out, S, n, p) if mode == _ffi.APH_OUT_PATCH_F32 else out).double()
        assert tuple(got.shape) == (S, 3, n, n)
        err = (got - want).abs().max().item()
        _note(dev, case, key, mode_name, 'fwd', err, gap)
        assert err <= MARGIN * gap, (err, gap)
        return
    # f16 layouts: the f16 rounding of the reference value plus one f16 ulp plus the f32 bound
    kp = 3 * p * p
    hi = from_patch_rows(out[:, :kp], S, n, p).double()
    w16 = want.half().double()
    excess = ((hi - w16).abs() - f16_ulp(w16)).max().item()
    _note(dev, case, key, mode_name, 'fwd', max(excess, 0.0), gap)
    assert excess <= MARGIN * gap, (excess, gap)
    if mode == _ffi.APH_OUT_PATCH_F16_HILO:         # hi + lo: the f32 value again, up to the rounding of lo (2^-10 of an f16 ulp of the value)
        assert out.shape[1] == 2 * kp
        both = hi + from_patch_rows(out[:, kp:], S, n, p).double()
        excess = ((both - want).abs() - f16_ulp(w16) * 2.0 ** -10).max().item()
        _note(dev, case, key, mode_name, 'fwd-hi+lo', max(excess, 0.0), gap)
        assert excess <= MARGIN * gap, (excess, gap)


def adjoint_paths(case):
    """(name, gather flag, launch shape or None, gscale): the automatic choice at both scales, the gather kernel, the listed row-kernel shapes"""
    paths = [('auto', 0, None, 1.0), ('auto-gscale', 0, None, GSCALE), ('gather', 1, None, GSCALE)]
    return paths + [('shape' + '.'.join(str(v) for v in s), 0, s, 1.0) for s in case.shapes]


def check_adjoint(lib, dev, name, mode_name):
    case = Case.get(name)
    mode, p = BWD_MODES[mode_name], case.patch
    L = lib if lib is not None else _ffi.lib()
    if mode in (_ffi.APH_OUT_NCHW_RAW, _ffi.APH_OUT_NCHW_NORM):
        gout = case.g
    else:
        gout = to_patch_rows(case.g, p)
        if mode == _ffi.APH_GRAD_PATCH_F16:
            gout = gout.half()                      # (exact: the values are f16-representable)
    key = 'd_raw' if mode == _ffi.APH_OUT_NCHW_RAW else 'd_norm'
    fails = []
    for path, gather, shape, gscale in adjoint_paths(case):
        prev = L.cdll.aph_crop_adjoint_set_gather(gather)
        try:
            if shape is not None:
                L.call('aph_crop_adjoint_set_shape', *shape)
            got = run_bwd(lib, dev, case, mode, gout, gscale).double()
        finally:
            L.cdll.aph_crop_adjoint_set_gather(prev)
            L.call('aph_crop_adjoint_set_shape', 0, 0, 0, 0, -1)
        want, gap = case.ref[key] * gscale, case.bound(key) * gscale
        err = (got - want).abs().max().item()
        _note(dev, case, key, mode_name, path, err, gap)
        if not err <= MARGIN * gap:
            fails.append((path, err, gap))
    assert not fails, fails


# ---------------------------------------------------------------------------- the restatement's own pins (no kernel involved)
def check_reference_vs_golden(g, align):
    """tests/golden/slice_48x80.npz: the reference's own slice_imgs (float32, normalised) at the seeded table of check_sampler_golden"""
    img = torch.from_numpy(g['img'])[0]
    st = torch.get_rng_state()
    torch.manual_seed(7)
    table = R.draw_crop_table(6, 16, 48, 80, align, 0.4)
    torch.set_rng_state(st)
    smp = sampler_ref.Sampler(48, 80, table, 16, align)
    x = img.double().numpy()
    got = sampler_ref.normalise(smp.forward(x))
    bound = (sampler_ref.rounding_bound(smp, x, False) + 4 * sampler_ref.EPS32 * (smp.forward(np.abs(x), mode='abs') + 1.0)) / sampler_ref.STD
    err = np.abs(got - g['cuts_' + align].astype(np.float64))
    print('reference vs golden %s: max %.3e, a-priori float32 bound there %.3e' % (align, err.max(), bound.reshape(-1)[err.argmax()]))
    assert (err <= bound).all(), (err.max(), bound.max())


def check_reference_vs_oracle(name):
    """the float64 restatement against the float32 oracle, forward and autograd gradient, element by element inside the oracle's a-priori
    float32 rounding error (sampler_ref.rounding_bound)"""
    case = Case.get(name)
    smp, x, g = case.sampler(), case.img.double().numpy(), case.g.double().numpy()
    fb = sampler_ref.rounding_bound(smp, x, False)
    bounds = dict(raw=fb, norm=(fb + 4 * sampler_ref.EPS32 * (smp.forward(np.abs(x), mode='abs') + 1.0)) / sampler_ref.STD,
                  d_raw=sampler_ref.rounding_bound(smp, g, True), d_norm=sampler_ref.rounding_bound(smp, g / sampler_ref.STD, True))
    for key, b in bounds.items():
        err = (case.oracle[key] - case.ref[key]).abs().numpy()
        print('reference vs fp32 oracle %s %s: max gap %.3e (max |value| %.3e), a-priori float32 bound there %.3e'
              % (name, key, err.max(), case.ref[key].abs().max().item(), b.reshape(-1)[err.argmax()]))
        assert err.max() > 0 and (err <= b).all(), (name, key, err.max(), (err / np.maximum(b, 1e-300)).max())


def check_reference_vs_tv_fixture(fx):
    """where tests/golden/tf_fast_224.npz exists: the restated warps against torchvision's own outputs (explicit perspectives and rotations
    of oracle/make_tv_fixture.py), each cut fed with the identity crop"""
    from oracle import make_tv_fixture as F
    cuts, _ = F.inputs()
    n = F.SIZE
    delta = 10 * 12 * n * sampler_ref.EPS32

    def one(x, prm, want):
        v = x.double().numpy().reshape(3, n * n)
        (m, _), = sampler_ref.chain_maps(prm, n)             # one warp: its float32 roundings plus the grid's (sampler_ref.rounding_bound)
        bound = 64 * sampler_ref.EPS32 * m.absolute().fwd(np.abs(v)) + delta * m.ones().fwd(np.abs(v))
        assert (np.abs(m.fwd(v) - want.reshape(3, n * n)) <= bound).all()
    for i, (sp, ep) in enumerate(F.PERSP_CASES):
        one(cuts[i], dict(persp=augment_ref.perspective_coeffs(sp, ep)), fx['persp_out'][i])
    for i, (a, t, sc, sh) in enumerate(F.AFFINE_CASES):
        one(cuts[i % F.STREAM_CUTS], dict(angle=a), fx['rotate_out'][i])


# ---------------------------------------------------------------------------- mutation table (not a test: `python tests/sampler_checks.py`)
MUTANTS = [
    ('tap_weight / bicubic3 skip taps of |weight| < 5e-5',
     [('sampler_crop_adjoint.h', '    if (yy == q) w += wv[k];', '    if (yy == q && fabsf(wv[k]) >= 5e-5f) w += wv[k];'),
      ('sampler_crop.h', '  cubic_w(sx - (float)x0, wx);\n', '  cubic_w(sx - (float)x0, wx);\n  for (int k = 0; k < 4; ++k) { if (fabsf(wy[k]) < 5e-5f) wy[k] = 0.f; if (fabsf(wx[k]) < 5e-5f) wx[k] = 0.f; }\n')]),
    ('tap_table_kernel: hi loses its + 1', [('sampler_crop_adjoint.h', 'hi = (int)floorf((float)(q + 2) * inv) + 1;', 'hi = (int)floorf((float)(q + 2) * inv);')]),
    ('phase0 keeps 7 of the 8 union rows', [('sampler_crop_adjoint.h', '              if (any && i < g.size) qr.off = L.rowpart(i);', '              if (any && i < g.size && r < 7) qr.off = L.rowpart(i);')]),
    ('rotate_emit_adjoint_kernel: rad - 0.3', [('sampler_warp.h', 'const float rad = fabsf(cs) + fabsf(sn) + 0.02f;', 'const float rad = fabsf(cs) + fabsf(sn) - 0.3f;')]),
    ('tent weight: mask factors mx, my = 1', [('sampler_warp.h', 'wm[d] = (iok[a3] && jok[b3]) ? (wx * wy) * (mx * my) : 0.f;', 'wm[d] = (iok[a3] && jok[b3]) ? (wx * wy) : 0.f;')]),
    ('persp_adjoint_kernel: 1.01 -> 0.6', [('sampler_warp.h', '((k & 1) ? 1.01f : -1.01f), v = (float)py + 0.5f + ((k & 2) ? 1.01f : -1.01f);',
                                            '((k & 1) ? 0.6f : -0.6f), v = (float)py + 0.5f + ((k & 2) ? 0.6f : -0.6f);')]),
    ('in_rect: <= at the far edge', [('sampler_warp.h', 'return y >= ei && y < ei + eh && x >= ej && x < ej + ew;', 'return y >= ei && y <= ei + eh && x >= ej && x <= ej + ew;')]),
    ('warp_gather3: the mask only where every tap is in range', [('sampler_warp.h', '  v[0] *= m; v[1] *= m; v[2] *= m;\n',
                                                           '  if (t.x0 >= 0 && t.x0 + 1 < n && t.y0 >= 0 && t.y0 + 1 < n) { v[0] *= m; v[1] *= m; v[2] *= m; }\n')]),
    # (the float32 quotient (cs - 1) / (size - 1) IS the double quotient rounded once, and so is a float32 product: what differs is carrying
    #  the scale in double into scale * i -- in the forward, which knows the cut's size)
    ('cut_scale in double: scale * i rounded once (forward)',
     [('sampler_crop.h', 'const float sy = src_index(b.scale, i), sx = src_index(b.scale, j);',
       'const double sd = g.size > 1 ? (double)(b.cs - 1) / (double)(g.size - 1) : 0.0; const float sy = (float)(sd * i), sx = (float)(sd * j);')]),
    # neighbours of the two table mutants above, which fail no check at any case
    ('tap_table_kernel: hi = floor((q + 1) * inv), one output short', [('sampler_crop_adjoint.h', 'hi = (int)floorf((float)(q + 2) * inv) + 1;', 'hi = (int)floorf((float)(q + 1) * inv);')]),
    ('phase0 keeps 6 of the 8 union rows', [('sampler_crop_adjoint.h', '              if (any && i < g.size) qr.off = L.rowpart(i);', '              if (any && i < g.size && r < 6) qr.off = L.rowpart(i);')]),
]


# the cases the mutants are run against (every crop-adjoint kernel and path, the up-sampling cut, wrap padding, > 64 columns, every warp stage)
MUTATION_CASES = ('base-uniform', 'base-overscan', 'tiny-23x37', 'trips-136', 'fast_a-uniform', 'fast_b-uniform', 'fast_drawn-overscan')


def mutation_table(old_checks=True, which=None, cases=MUTATION_CASES):
    """Each mutant of the sampler's headers (a textual patch on a scratch copy, built for the interpreter beside the real objects; none moves
    an address out of bounds) must FAIL at least one check here that the real kernels pass.  Prints one line per mutant: the checks of this
    file it fails, and whether the sampler tests from before this file (kernel_checks: golden, adjoint, augment, crop-adjoint paths, fuzz)
    notice it.

    The closing assertion FAILS and is left failing: `tap_table_kernel: hi loses its + 1` and `phase0 keeps 7 of the 8 union rows` fail 0 of the
    49 checks here and 0 of 196 over all 28 cases (`--all`); the other nine fail 7 to 28 (DESIGN.md section 2 a-8b has the table and why)."""
    import os
    import shutil
    import subprocess
    import sys
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, 'emu'))
    import build_emu
    import kernel_checks as KC
    build_emu.build()
    csrc, bdir = build_emu.CSRC, os.path.join(build_emu.HERE, 'build')
    modes = ('nchw_raw', 'nchw_norm', 'patch_f16', 'grad_patch_f16')
    checks = [(check_forward, (c, m)) for c in cases for m in modes if m in FWD_MODES]
    checks += [(check_adjoint, (c, m)) for c in cases for m in modes if m in BWD_MODES]
    golden = dict(np.load(os.path.join(here, 'golden', 'slice_48x80.npz')))

    def failures(lib):
        bad = []
        for fn, chk in checks:
            try:
                fn(lib, 'cpu', *chk)
            except AssertionError:
                bad.append(fn.__name__[6:] + ':' + case_id(chk))
        return bad

    def old_failures(lib):
        prev, T._EXACT_ZERO_ROT = T._EXACT_ZERO_ROT, True
        bad = []
        old = [lambda: [KC.check_sampler_golden(lib, 'cpu', golden, a) for a in ('uniform', 'central', 'overscan', 'overmax')],
               lambda: [KC.check_sampler_adjoint(lib, 'cpu', a, m) for a in ('uniform', 'overscan', 'overmax') for m in (0, 1, 2)],
               lambda: KC.check_sampler_augment(lib, 'cpu'), lambda: KC.check_crop_adjoint_paths(lib, 'cpu'),
               lambda: KC.check_sampler_f16_gradient(lib, 'cpu'), lambda: KC.check_augment_invariants(lib, 'cpu'),
               lambda: KC.check_sampler_fuzz(lib, 'cpu', 1, 12)]
        names = ['golden', 'adjoint', 'augment', 'crop_adjoint_paths', 'f16_gradient', 'augment_invariants', 'fuzz']
        try:
            for nm, f in zip(names, old):
                try:
                    f()
                except AssertionError:
                    bad.append(nm)
        finally:
            T._EXACT_ZERO_ROT = prev
        return bad
    assert not failures(_ffi.Library(build_emu.OUT)), 'the unmutated kernels fail'
    rows = []
    for name, patches in (MUTANTS if which is None else [MUTANTS[i] for i in which]):
        with tempfile.TemporaryDirectory() as tmp:
            for f_ in os.listdir(csrc):          # the whole stage family: the headers include each other by name
                if f_.startswith('sampler'):
                    shutil.copy(os.path.join(csrc, f_), tmp)
            for fname in sorted({p[0] for p in patches}):
                src = open(os.path.join(csrc, fname)).read()
                for f_, old, new in patches:
                    if f_ == fname:
                        assert old in src, (name, old)
                        src = src.replace(old, new)
                open(os.path.join(tmp, fname), 'w').write(src)
            obj, so = os.path.join(tmp, 'sampler.o'), os.path.join(tmp, 'libmutant.so')
            subprocess.check_call([build_emu.CLANG, '-x', 'c++', '-std=c++17', '-O2', '-fPIC', '-DAPH_EMU', '-Wno-unused-value', '-I', build_emu.HERE, '-I', tmp,
                                   '-I', csrc, '-I', os.path.join(build_emu.ROOT, 'include'), '-c', os.path.join(tmp, 'sampler.hip'), '-o', obj])
            others = [os.path.join(bdir, s + '.emu.o') for s in build_emu.SOURCES if s != 'sampler.hip']
            subprocess.check_call([build_emu.CLANG, '-shared', '-fPIC', '-o', so, obj] + others)
            lib = _ffi.Library(so)
            bad = failures(lib)
            was = old_failures(lib) if old_checks else []
        rows.append((name, len(bad), bad[:3], was))
    print('\nmutant -> failed checks of sampler_checks.py (of %d) | the earlier sampler checks that fail' % len(checks))
    for name, nbad, some, was in rows:
        print('  %-52s %3d   e.g. %s | %s' % (name, nbad, ', '.join(some), ', '.join(was) or 'none'))
    assert all(r[1] > 0 for r in rows), 'a mutant passes every check'


if __name__ == '__main__':
    import sys
    everywhere = '--all' in sys.argv          # every case instead of MUTATION_CASES (slow), without the earlier checks
    mutation_table(old_checks=not everywhere, which=[int(v) for v in sys.argv[1:] if v != '--all'] or None, cases=list(CROP_CASES) + list(FAST_CASES) if everywhere else MUTATION_CASES)
