"""Checks of the `-tf custom` / `-tf elastic` augment chains (csrc/sampler_kornia.h: aph_sample_fwd_tf / aph_sample_bwd_tf) shared by the
interpreter tests (test_emu_tf.py) and the GPU tests (test_gpu_tf.py).  `lib` = a loaded C-ABI library (the interpreter build) or None (the
product), `dev` = where its tensors live.

Truth: tests/tf_ref.py -- kornia's call chains restated literally on torch -- in float64, through the untouched oracle's slice_imgs; autograd
through it is the adjoint's truth.  Tolerance, per case and per quantity (image, gradient): max |kernel - fp64| <= MARGIN x max |the same
restatement run in float32 - fp64|, measured here, not hard-coded.  Both are f32 evaluations of one map; they differ in where they round
(the restatement in normalised grids and 3x3 matrix products, the kernels in pixel space).  The f16 layouts are held to the f16 rounding of the
fp64 value plus that bound plus one f16 ulp.  EVERY element is compared: a bilinear chain is continuous in its coordinates, there is no
breakpoint to excuse.  A wrong sign, tap, ring value or window does not fit in the bound (the mutation table in DESIGN.md section 2 a-8)."""
import math

import numpy as np
import torch

from aphantasia_amd import _ffi, ops
from aphantasia_amd.transforms import pack_aug, transforms_custom, transforms_elastic
from oracle import reference_path as R
import tf_ref

MARGIN = 4.0
BAND = 1024          # canary elements on either side of every output and of the workspace
CHAINS = {'custom': transforms_custom, 'elastic': transforms_elastic}
FWD_MODES = {'nchw_raw': _ffi.APH_OUT_NCHW_RAW, 'nchw_norm': _ffi.APH_OUT_NCHW_NORM, 'patch_f16': _ffi.APH_OUT_PATCH_F16,
             'patch_f16_hilo': _ffi.APH_OUT_PATCH_F16_HILO, 'patch_f32': _ffi.APH_OUT_PATCH_F32}
BWD_MODES = {'nchw_raw': _ffi.APH_OUT_NCHW_RAW, 'nchw_norm': _ffi.APH_OUT_NCHW_NORM, 'patch_f16': _ffi.APH_OUT_PATCH_F16,
             'patch_f32': _ffi.APH_OUT_PATCH_F32, 'grad_patch_f16': _ffi.APH_GRAD_PATCH_F16}
RATIOS = []          # (case, chain, quantity, mode, max |kernel - fp64|, max |fp32 restatement - fp64|) of every check run in this process


def hand_cuts(n):
    """six hand-written cuts on the P = n + 8 canvas: the copy path (angle 0), +30 and -30 degrees, the jitter corners (0,0) (7,7) (7,0),
    an erase rectangle over the pad ring and the canvas corner, one of height 1, and none"""
    P = n + 8
    return [dict(angle=0.0, erase=None, shift=(0, 0)),
            dict(angle=30.0, erase=(0, 0, P // 4, P // 3), shift=(7, 7)),                       # over the ring and the canvas corner
            dict(angle=-30.0, erase=(P // 2, 5, 1, P - 10), shift=(7, 0)),                      # height 1
            dict(angle=0.0, erase=(P - P // 4, P - P // 3 - 1, P // 4 - 1, P // 3), shift=(7, 7)),   # copy path, erased to one short of the far corner
            dict(angle=17.0, erase=None, shift=(0, 0)),
            dict(angle=-30.0, erase=None, shift=(3, 5))]


# name -> (image H, W, size n, patch, cuts)
CASES = {'hand': (40, 56, 32, 16, 6), 'drawn': (40, 56, 32, 16, 6), 'vit_b32': (232, 250, 224, 32, 3)}


class Case:
    """inputs of one (case, chain) and its fp64 / fp32 references, computed once and left unchanged"""
    _cache = {}

    @classmethod
    def get(cls, name, chain):
        key = (name, chain)
        if key not in cls._cache:
            cls._cache[key] = cls(name, chain)
        return cls._cache[key]

    def __init__(self, name, chain):
        self.name, self.chain = name, chain
        self.tf = CHAINS[chain]
        self.elastic = chain == 'elastic'
        self.H, self.W, self.n, self.patch, self.S = CASES[name]
        n, S = self.n, self.S
        self.P = n + 8
        gen = torch.Generator().manual_seed(17 + len(name))
        self.img = torch.rand(1, 3, self.H, self.W, generator=gen)
        st_t, st_n = torch.get_rng_state(), np.random.get_state()
        torch.manual_seed(31)
        np.random.seed(31)
        if name == 'hand':
            self.prms = hand_cuts(n)
            lo, hi = n, min(self.H, self.W)
            self.table = np.array([(lo, 0, 0), (hi, self.W - hi, 0), ((lo + hi) // 2, 3, self.H - (lo + hi) // 2), (lo + 1, 20, 7), (hi, 0, 0), (hi - 2, 10, 1)], dtype=np.int32)
        else:
            self.prms = []
            self.table = R.draw_crop_table(S, n, self.H, self.W, 'uniform', 0.4, per_cut_hook=lambda c: self.prms.append(self.tf.draw(n)))
            if name == 'vit_b32':          # the real layout: make sure a rotation, an erase and a copy are all in it
                self.prms[0].update(angle=-30.0, shift=(7, 3), erase=(50, 0, 60, 90))
                self.prms[1].update(angle=0.0, shift=(0, 7), erase=None)
                self.prms[2].update(angle=23.0, shift=(5, 0), erase=(200, 180, 31, 51))
        torch.set_rng_state(st_t)
        np.random.set_state(st_n)
        if not self.elastic:
            self.prms = [dict(p, erase=None) for p in self.prms]
        self.aug = pack_aug([dict(p) for p in self.prms])
        # gradient of the output: f16-representable, so the f16 gradient layout carries the same values
        self.g = torch.randn(S, 3, self.P, self.P, generator=gen).half().float()
        self.gwin = torch.zeros_like(self.g)
        self.gwin[:, :, :n, :n] = self.g[:, :, :n, :n]
        self.ref = {dt: self._reference(dt) for dt in (torch.float64, torch.float32)}

    def _reference(self, dtype):
        """-> dict: raw / norm canvases [S,3,P,P] and the image gradients of <raw, g>, <norm, g>, <norm, gwin>, all as float64"""
        img = self.img.to(dtype).requires_grad_(True)
        raw = R.slice_imgs(img, self.table, self.n, 'uniform', per_cut=tf_ref.per_cut(self.prms, self.elastic, normalise=False))
        norm = R.normalize(raw)
        out = dict(raw=raw.detach().double(), norm=norm.detach().double())
        for key, y, g in (('d_raw', raw, self.g), ('d_norm', norm, self.g), ('d_win', norm, self.gwin)):
            out[key] = torch.autograd.grad((y * g.to(dtype)).sum(), img, retain_graph=True)[0][0].double()
        return out

    def bound(self, key):
        gap = (self.ref[torch.float32][key] - self.ref[torch.float64][key]).abs().max().item()
        assert gap > 0, 'the float32 restatement equals the float64 one: no bound to take'
        return gap


def case_id(c):
    return '-'.join(str(v) for v in c)


# ---------------------------------------------------------------------------- layouts
def from_patch_rows(rows, S, n, p):
    """patch-major [S (n/p)^2, 3 p^2], column (iy p + ix) 3 + c  ->  [S,3,n,n]"""
    g = n // p
    return rows.reshape(S, g, g, p, p, 3).permute(0, 5, 1, 3, 2, 4).reshape(S, 3, n, n)


def to_patch_rows(x, p):
    S, _, n, _ = x.shape
    g = n // p
    return x.reshape(S, 3, g, p, g, p).permute(0, 2, 4, 3, 5, 1).reshape(S * g * g, 3 * p * p).contiguous()


def f16_ulp(v):
    """one unit in the last place of the f16 nearest to v (float64 tensor)"""
    a = v.abs().clamp_min(2.0 ** -14)                # below the smallest normal the spacing stays 2^-24
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 10)


def banded(numel, dtype, dev):
    big = torch.full((numel + 2 * BAND,), float('nan'), dtype=dtype, device=dev)
    return big, big[BAND:BAND + numel]


def bands_intact(big):
    return bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[-BAND:]).all())


def geom_of(case):
    return ops.make_geom(case.H, case.W, case.S, case.n, case.patch, 'uniform')


def run_fwd(lib, dev, case, mode, geom=None, aug=None):
    geom = geom_of(case) if geom is None else geom
    kind = case.tf.kind
    shape, dtype = ops.sample_out_shape(geom, mode, kind)
    big, flat = banded(int(np.prod(shape)), dtype, dev)
    ws = ops.sample_ws(geom, True, dev, lib, kind)
    wbig, wflat = banded(ws.numel(), torch.float32, dev)
    aug_h = case.aug if aug is None else aug
    out = ops.sample_fwd(geom, case.img[0].contiguous().to(dev), torch.from_numpy(case.table).to(dev), aug_h.to(dev), wflat, flat.view(shape), mode,
                         lib=lib, tf=kind, h_aug=aug_h)
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bands_intact(big) and bands_intact(wbig), 'a write outside the output or the workspace'
    assert not torch.isnan(out.float()).any(), 'an output element was not written'
    return out.cpu()


def run_bwd(lib, dev, case, mode, gout, gscale=1.0):
    geom, kind = geom_of(case), case.tf.kind
    big, flat = banded(3 * case.H * case.W, torch.float32, dev)
    ws = ops.sample_ws(geom, True, dev, lib, kind)
    wbig, wflat = banded(ws.numel(), torch.float32, dev)
    out = ops.sample_bwd(geom, gout.contiguous().to(dev), torch.from_numpy(case.table).to(dev), case.aug.to(dev), wflat, flat.view(3, case.H, case.W), mode,
                         gscale=gscale, lib=lib, tf=kind, h_aug=case.aug)
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bands_intact(big) and bands_intact(wbig), 'a write outside the gradient or the workspace'
    assert not torch.isnan(out).any(), 'a gradient element was not written'
    return out.cpu()


def _note(case, quantity, mode, err, gap):
    RATIOS.append((case.name, case.chain, quantity, mode, err, gap))


# ---------------------------------------------------------------------------- parity
def check_forward(lib, dev, name, chain, mode_name):
    case = Case.get(name, chain)
    mode, n, P, S, p = FWD_MODES[mode_name], case.n, case.P, case.S, case.patch
    out = run_fwd(lib, dev, case, mode)
    key = 'raw' if mode == _ffi.APH_OUT_NCHW_RAW else 'norm'
    want, gap = case.ref[torch.float64][key], case.bound(key)
    if mode in (_ffi.APH_OUT_NCHW_RAW, _ffi.APH_OUT_NCHW_NORM):
        assert tuple(out.shape) == (S, 3, P, P)
        err = (out.double() - want).abs().max().item()
        print('%s %s fwd %s: max |kernel - fp64| %.3e, fp32 restatement %.3e, ratio %.2f' % (name, chain, mode_name, err, gap, err / gap))
        _note(case, 'fwd', mode_name, err, gap)
        assert err <= MARGIN * gap, (err, gap)
        return
    want = want[:, :, :n, :n]                       # the window the patch embedding reads
    if mode == _ffi.APH_OUT_PATCH_F32:
        got = from_patch_rows(out, S, n, p).double()
        err = (got - want).abs().max().item()
        print('%s %s fwd %s: max |kernel - fp64| %.3e, fp32 restatement %.3e, ratio %.2f' % (name, chain, mode_name, err, gap, err / gap))
        _note(case, 'fwd', mode_name, err, gap)
        assert err <= MARGIN * gap, (err, gap)
        return
    # f16 layouts: the f16 rounding of the fp64 value plus one f16 ulp -- PLUS the f32 bound above, which the literal wording leaves out and
    # small values need: near zero an f16 ulp (down to 2^-24) is smaller than the f32 chain's own error, which the rounding does not remove
    kp = 3 * p * p
    hi = from_patch_rows(out[:, :kp], S, n, p).double()
    w16 = want.half().double()                      # the f16 rounding of the fp64 value
    excess = ((hi - w16).abs() - f16_ulp(w16)).max().item()
    print('%s %s fwd %s: max (|kernel - f16(fp64)| - 1 f16 ulp) %.3e, fp32 restatement %.3e' % (name, chain, mode_name, excess, gap))
    _note(case, 'fwd', mode_name, max(excess, 0.0), gap)
    assert excess <= MARGIN * gap, (excess, gap)
    if mode == _ffi.APH_OUT_PATCH_F16_HILO:         # hi + lo: the f32 value again, up to the rounding of lo (2^-11 of an f16 ulp of the value)
        assert out.shape[1] == 2 * kp
        both = hi + from_patch_rows(out[:, kp:], S, n, p).double()
        excess = ((both - want).abs() - f16_ulp(w16) * 2.0 ** -10).max().item()
        print('%s %s fwd %s: hi + lo, max excess %.3e' % (name, chain, mode_name, excess))
        assert excess <= MARGIN * gap, (excess, gap)


def check_adjoint(lib, dev, name, chain, mode_name, gscale=1.0):
    case = Case.get(name, chain)
    mode, n, p = BWD_MODES[mode_name], case.n, case.patch
    if mode == _ffi.APH_OUT_NCHW_RAW:
        gout, key = case.g, 'd_raw'
    elif mode == _ffi.APH_OUT_NCHW_NORM:
        gout, key = case.g, 'd_norm'
    else:
        gout, key = to_patch_rows(case.g[:, :, :n, :n].contiguous(), p), 'd_win'
        if mode == _ffi.APH_GRAD_PATCH_F16:
            gout = gout.half()                      # (exact: the values are f16-representable)
    got = run_bwd(lib, dev, case, mode, gout, gscale).double()
    want, gap = case.ref[torch.float64][key] * gscale, case.bound(key) * gscale
    err = (got - want).abs().max().item()
    print('%s %s bwd %s: max |kernel - fp64| %.3e, fp32 restatement %.3e, ratio %.2f (max |grad| %.3e)' % (name, chain, mode_name, err, gap, err / gap, want.abs().max().item()))
    _note(case, 'bwd', mode_name, err, gap)
    assert err <= MARGIN * gap, (err, gap)


# ---------------------------------------------------------------------------- properties
def check_dot_product(lib, dev, name, chain):
    """<A x1 - A x0, g> == <x1 - x0, A^T g> (A is affine: the ring and the shifted-in zeros are constants) to fp32 summation accuracy:
    every product term carries a few f32 roundings, so the two sums agree to 16 eps of the sum of their absolute terms"""
    case = Case.get(name, chain)
    other = Case.__new__(Case)
    other.__dict__.update(case.__dict__)
    other.img = torch.rand(case.img.shape, generator=torch.Generator().manual_seed(5))
    y1, y0 = run_fwd(lib, dev, case, _ffi.APH_OUT_NCHW_RAW).double(), run_fwd(lib, dev, other, _ffi.APH_OUT_NCHW_RAW).double()
    atg = run_bwd(lib, dev, case, _ffi.APH_OUT_NCHW_RAW, case.g).double()
    dxv = (case.img[0] - other.img[0]).double()
    lhs, rhs = ((y1 - y0) * case.g.double()).sum().item(), (dxv * atg).sum().item()
    scale = ((y1.abs() + y0.abs()) * case.g.double().abs()).sum().item() + (dxv.abs() * atg.abs()).sum().item()
    print('%s %s <Ax,g> %.9e  <x,A^T g> %.9e  |d| / sum|terms| %.2e' % (name, chain, lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 16 * 2.0 ** -24 * scale, (lhs, rhs, scale)


def check_window_gradient(lib, dev, name, chain):
    """the patch-major layouts hold the top-left n x n window: canvas rows / columns >= n get EXACTLY no gradient -- the patch-mode adjoint
    equals, bit for bit, the planar adjoint of the same gradient with zeros outside the window"""
    case = Case.get(name, chain)
    n, p = case.n, case.patch
    a = run_bwd(lib, dev, case, _ffi.APH_OUT_PATCH_F16, to_patch_rows(case.g[:, :, :n, :n].contiguous(), p))
    b = run_bwd(lib, dev, case, _ffi.APH_OUT_NCHW_NORM, case.gwin)
    assert torch.equal(a, b)
    only_outside = case.g - case.gwin
    c = run_bwd(lib, dev, case, _ffi.APH_OUT_NCHW_NORM, only_outside)
    assert c.abs().max().item() > 0                 # (the planar layout does carry gradient there: the check above is not vacuous)


def check_erase_preimage(lib, dev, chain):
    """one cut of exactly n x n pixels (the bicubic resize is then the identity: weights 0, 1, 0, 0), erase rectangle over it: the image
    pixels under the rectangle, and those outside the cut, get EXACTLY zero gradient"""
    base = Case.get('hand', chain)
    one = Case.__new__(Case)
    one.__dict__.update(base.__dict__)
    n, P = base.n, base.P
    one.S = 1
    ox, oy = 11, 5
    one.table = np.array([(n, ox, oy)], dtype=np.int32)
    rect = (P // 2 - 3, 2, 9, P // 2) if chain == 'elastic' else None
    one.prms = [dict(angle=-30.0, erase=rect, shift=(2, 1))]
    one.aug = pack_aug([dict(one.prms[0])])
    one.g = base.g[:1].abs() + 0.5                   # positive: no cancellation can fake a zero
    got = run_bwd(lib, dev, one, _ffi.APH_OUT_NCHW_RAW, one.g)
    inside = torch.zeros(base.H, base.W, dtype=torch.bool)
    inside[oy:oy + n, ox:ox + n] = True
    assert got[:, ~inside].abs().max().item() == 0.0
    erased = torch.zeros_like(inside)
    if rect is not None:
        i, j, h, w = rect
        i0, i1, j0, j1 = max(i - 4, 0), min(i + h - 4, n), max(j - 4, 0), min(j + w - 4, n)
        erased[oy + i0:oy + i1, ox + j0:ox + j1] = True
        assert erased.sum().item() > 0 and got[:, erased].abs().max().item() == 0.0
    # every other cut pixel within 14 pixels of the cut's centre stays on the canvas under the rotation (the corners of the cut leave it)
    # and under the jitter, so it lies in some footprint and gets a strictly positive gradient
    yy, xx = torch.meshgrid(torch.arange(base.H, dtype=torch.float64), torch.arange(base.W, dtype=torch.float64), indexing='ij')
    disc = (yy - (oy + (n - 1) / 2)) ** 2 + (xx - (ox + (n - 1) / 2)) ** 2 < 14.0 ** 2
    live = inside & ~erased & disc
    assert (got[:, live] > 0).all()


def check_bitwise_repeat(lib, dev, name, chain):
    case = Case.get(name, chain)
    n, p = case.n, case.patch
    for mode in (_ffi.APH_OUT_NCHW_NORM, _ffi.APH_OUT_PATCH_F16):
        assert torch.equal(run_fwd(lib, dev, case, mode), run_fwd(lib, dev, case, mode))
    gout = to_patch_rows(case.g[:, :, :n, :n].contiguous(), p)
    assert torch.equal(run_bwd(lib, dev, case, _ffi.APH_OUT_PATCH_F16, gout), run_bwd(lib, dev, case, _ffi.APH_OUT_PATCH_F16, gout))


def check_refusals(lib, dev):
    """bad arguments return APH_ERR_ARG (-1) with a message, before any launch (the outputs keep their NaN prefill)"""
    import ctypes
    import pytest
    case = Case.get('hand', 'custom')
    L = lib if lib is not None else _ffi.lib()
    img, table, aug = case.img[0].contiguous().to(dev), torch.from_numpy(case.table).to(dev), case.aug.to(dev)

    def fwd(geom, tf, aug_d, aug_h, mode):
        shape, dtype = ops.sample_out_shape(geom, mode, _ffi.APH_TF_CUSTOM)
        out = torch.full(shape, float('nan'), dtype=dtype, device=dev)
        ws = ops.sample_ws(geom, True, dev, L, _ffi.APH_TF_ELASTIC)
        rc = L.cdll.aph_sample_fwd_tf(ctypes.byref(geom), tf, ops.ptr(img), ops.ptr(table), ops.ptr(aug_d), ops.ptr(aug_h), ops.ptr(ws), ops.ptr(out), mode, None)
        assert torch.isnan(out.float()).all(), 'a refused call launched'
        return rc, L.last_error()
    geom = geom_of(case)
    for tf in (-1, 3):
        rc, msg = fwd(geom, tf, aug, None, _ffi.APH_OUT_NCHW_NORM)
        assert rc == -1 and 'chain kind' in msg, (rc, msg)
    rc, msg = fwd(geom, _ffi.APH_TF_CUSTOM, None, None, _ffi.APH_OUT_NCHW_NORM)
    assert rc == -1 and 'null augment table' in msg, (rc, msg)
    small = ops.make_geom(case.H, case.W, case.S, case.n, 8, 'uniform')
    for mode in (_ffi.APH_OUT_PATCH_F16, _ffi.APH_OUT_PATCH_F32, _ffi.APH_OUT_PATCH_F16_HILO):
        rc, msg = fwd(small, _ffi.APH_TF_ELASTIC, aug, None, mode)
        assert rc == -1 and 'patch 8 <= 8' in msg, (rc, msg)
    for col, val in ((0, 8.0), (1, -1.0), (0, 2.5)):
        bad = case.aug.clone()
        bad[2, col] = val
        rc, msg = fwd(geom, _ffi.APH_TF_CUSTOM, bad.to(dev), bad, _ffi.APH_OUT_NCHW_NORM)
        assert rc == -1 and 'cut 2: jitter' in msg, (rc, msg)
    gr = torch.full((3, case.H, case.W), float('nan'), device=dev)
    ws = ops.sample_ws(geom, True, dev, L, _ffi.APH_TF_ELASTIC)
    rc = L.cdll.aph_sample_bwd_tf(ctypes.byref(geom), 7, ops.ptr(case.g.to(dev)), 1.0, ops.ptr(table), ops.ptr(aug), None, ops.ptr(ws), ops.ptr(gr),
                                  _ffi.APH_OUT_NCHW_NORM, None)
    assert rc == -1 and 'chain kind' in L.last_error() and torch.isnan(gr).all()
    assert L.cdll.aph_sample_ws_bytes_tf(ctypes.byref(geom), 5) == 0
    assert L.cdll.aph_sample_ws_bytes_tf(ctypes.byref(geom), _ffi.APH_TF_FAST) == L.cdll.aph_sample_ws_bytes(ctypes.byref(geom), 1)
    P2 = (case.n + 8) ** 2
    assert (L.cdll.aph_sample_ws_bytes_tf(ctypes.byref(geom), _ffi.APH_TF_ELASTIC) - L.cdll.aph_sample_ws_bytes_tf(ctypes.byref(geom), _ffi.APH_TF_CUSTOM)
            == case.S * 4 * P2 * 4)                  # the elastic scratch is a P x P canvas per cut, not n x n
    with pytest.raises(ValueError):
        pack_aug([dict(angle=0.0, shift=(8, 0))])


def check_fast_forwarding(lib, dev):
    """tf = APH_TF_FAST is today's chain, bit for bit"""
    import ctypes
    from aphantasia_amd.transforms import draw_fast_bulk
    case = Case.get('drawn', 'custom')
    L = lib if lib is not None else _ffi.lib()
    geom = geom_of(case)
    aug = torch.from_numpy(draw_fast_bulk(case.S, case.n, np.random.default_rng(3))).to(dev)
    img, table = case.img[0].contiguous().to(dev), torch.from_numpy(case.table).to(dev)
    a = ops.sample_fwd(geom, img, table, aug, lib=L)
    ws = ops.sample_ws(geom, True, dev, L)
    b = torch.empty_like(a)
    L.call('aph_sample_fwd_tf', ctypes.byref(geom), _ffi.APH_TF_FAST, ops.ptr(img), ops.ptr(table), ops.ptr(aug), None, ops.ptr(ws), ops.ptr(b), _ffi.APH_OUT_NCHW_NORM, ops._stream(img))
    ga = ops.sample_bwd(geom, case.g[:, :, :case.n, :case.n].contiguous().to(dev), table, aug, lib=L)
    gb = torch.empty_like(ga)
    L.call('aph_sample_bwd_tf', ctypes.byref(geom), _ffi.APH_TF_FAST, ops.ptr(case.g[:, :, :case.n, :case.n].contiguous().to(dev)), 1.0, ops.ptr(table), ops.ptr(aug), None,
           ops.ptr(ws), ops.ptr(gb), _ffi.APH_OUT_NCHW_NORM, ops._stream(img))
    assert torch.equal(a, b) and torch.equal(ga, gb)


# ---------------------------------------------------------------------------- the whole step
def check_engine(lib, dev, model, weights, cfg, chain, h, w, S, steps, use_graph, **engine_kw):
    """`steps` free-running optimisation steps of Engine(transform = the chain) against the oracle's ReferenceRun with the tf_ref per-cut
    transform (its ViT restatement takes n x n cuts: the window the conv reads), the reference's draw order; tolerances of the `-tf fast` /
    `-tf none` runs of tests/test_engine_emu.py: per-step |d loss| < 1e-3, final image RMS < 2e-2"""
    from aphantasia_amd.engine import Engine
    from oracle import clip_vit_ref
    tf, n = CHAINS[chain], cfg['input_resolution']
    torch.manual_seed(0)
    np.random.seed(0)
    params = R.fft_params_init([1, 3, h, w]).contiguous()
    target = torch.randn(1, cfg['output_dim'], generator=torch.Generator().manual_seed(2))
    eng = Engine(params.to(dev).contiguous(), h, w, model, S, [(target, -1.0)], sim='mix', macro=0.4, transform=tf, lib=lib, use_graph=use_graph, **engine_kw)
    run = R.ReferenceRun(h, w, lambda x: clip_vit_ref.encode_image(weights, x, cfg), [(target, 1.0)], size=n, params=params.clone())
    torch.manual_seed(123)
    np.random.seed(123)
    for i in range(steps):
        prms = []
        table = R.draw_crop_table(S, n, h, w, 'uniform', 0.4, per_cut_hook=lambda c: prms.append(tf.draw(n)))
        want = run.step(table, tf_ref.per_cut(prms, chain == 'elastic', window=n))
        got = float(eng.step(table, [dict(p) for p in prms]))
        print('%s step %d: loss %.6f, oracle %.6f' % (chain, i, got, want))
        assert abs(got - want) < 1e-3, (i, got, want)
    with torch.no_grad():
        img = run.image(1.1)[0]
    rms = (eng.synthesize(1.1).cpu() - img).pow(2).mean().sqrt().item()
    assert rms < 2e-2, rms
    return eng


def check_engine_dual(lib, dev, models, weights, cfg, chain, h, w, S, steps, use_graph):
    """--dualmod (clip_fft.py:132-136,243-252): two models, two engines on ONE parameter leaf and ONE Adam state, alternating, both through the
    chain; against ReferenceRun(models=...) with the tf_ref per-cut transform, per-step |d loss| < 1e-3"""
    from aphantasia_amd.engine import Engine
    from oracle import clip_vit_ref
    tf, n = CHAINS[chain], cfg['input_resolution']
    torch.manual_seed(0)
    np.random.seed(0)
    params = R.fft_params_init([1, 3, h, w]).contiguous()
    targets = [torch.randn(1, cfg['output_dim'], generator=torch.Generator().manual_seed(2 + k)) for k in range(2)]
    leaf = params.to(dev).contiguous()
    kw = dict(sim='mix', macro=0.4, transform=tf, lib=lib, use_graph=use_graph)
    eng = Engine(leaf, h, w, models[0], S, [(targets[0], -1.0)], **kw)
    engs = [eng, Engine(leaf, h, w, models[1], S, [(targets[1], -1.0)], state=eng.state(), **kw)]
    enc = [lambda x, k=k: clip_vit_ref.encode_image(weights[k], x, cfg) for k in range(2)]
    run = R.ReferenceRun(h, w, None, None, size=n, params=params.clone(), models=[(enc[k], [(targets[k], 1.0)]) for k in range(2)])
    torch.manual_seed(77)
    np.random.seed(77)
    for i in range(steps):
        k = i % 2
        prms = []
        table = R.draw_crop_table(S, n, h, w, 'uniform', 0.4, per_cut_hook=lambda c: prms.append(tf.draw(n)))
        want = run.step(table, tf_ref.per_cut(prms, chain == 'elastic', window=n), model=k)
        got = float(engs[k].step(table, [dict(p) for p in prms]))
        print('%s dual step %d (model %d): loss %.6f, oracle %.6f' % (chain, i, k, got, want))
        assert abs(got - want) < 1e-3, (i, got, want)
    return engs


def check_engine_ranks(lib, dev, model, cfg, chain, h, w, S, world):
    """the cuts split over `world` ranks: every rank's partial loss and partial parameter gradient (the step up to its all-reduce), summed,
    equal the single-rank step's up to f32 summation order (1e-5 of the largest gradient entry)"""
    from aphantasia_amd.engine import Engine
    tf = CHAINS[chain]
    torch.manual_seed(0)
    np.random.seed(0)
    params = R.fft_params_init([1, 3, h, w]).contiguous().to(dev)
    target = torch.randn(1, cfg['output_dim'], generator=torch.Generator().manual_seed(2))
    prms = []
    table = R.draw_crop_table(S, cfg['input_resolution'], h, w, 'uniform', 0.4, per_cut_hook=lambda c: prms.append(tf.draw(cfg['input_resolution'])))

    def partial(rank, nranks):
        eng = Engine(params.clone(), h, w, model, S, [(target, -1.0)], sim='mix', transform=tf, lib=lib, use_graph=False, rank=rank, world=nranks)
        eng.inputs.upload(eng._step_items(ops.adam_hyper(1, 0.05), table, [dict(p) for p in prms], None, None))
        eng._enqueue_grad(None)
        return eng.grad.detach().double().cpu().clone(), float(eng.loss)
    g1, l1 = partial(0, 1)
    parts = [partial(r, world) for r in range(world)]
    gs, ls = sum(p[0] for p in parts), sum(p[1] for p in parts)
    print('%s ranks %d: loss %.7f vs %.7f, max |d grad| / max |grad| %.2e' % (chain, world, ls, l1, ((gs - g1).abs().max() / g1.abs().max()).item()))
    assert abs(ls - l1) < 1e-5 and (gs - g1).abs().max().item() <= 1e-5 * g1.abs().max().item()


def mode_cases():
    """(case, chain, forward mode) and (case, chain, gradient mode): every mode and both chains at the two small cases, the real layout
    (n = 224, patch 32) at the modes the engine runs plus one planar"""
    fwd = [(c, ch, m) for c in ('hand', 'drawn') for ch in CHAINS for m in FWD_MODES]
    fwd += [('vit_b32', ch, m) for ch in CHAINS for m in ('nchw_norm', 'patch_f16', 'patch_f32')]
    bwd = [(c, ch, m) for c in ('hand', 'drawn') for ch in CHAINS for m in BWD_MODES]
    bwd += [('vit_b32', ch, m) for ch in CHAINS for m in ('nchw_norm', 'patch_f16', 'grad_patch_f16')]
    return fwd, bwd


# ---------------------------------------------------------------------------- mutation table (not a test: `python tests/tf_checks.py`)
MUTANTS = [
    ('the angle\'s sign', [('fx = fmaf(cs, ux, fmaf(-sn, uy, c));', 'fx = fmaf(cs, ux, fmaf(sn, uy, c));'), ('fy = fmaf(sn, ux, fmaf(cs, uy, c));', 'fy = fmaf(-sn, ux, fmaf(cs, uy, c));')]),
    ('dx / dy swapped', [('const int y = i - (int)a[1], x = j - (int)a[0];', 'const int y = i - (int)a[0], x = j - (int)a[1];')]),
    ('ring value 0.5 -> 0', [('constexpr float kTfRing = 0.5f;', 'constexpr float kTfRing = 0.f;')]),
    ('erase applied after the rotation', [('xx >= 0 && xx < P && !(ERASE && in_rect(a, yy, xx));', 'xx >= 0 && xx < P;'),
                                          ('    canvas_tap<ERASE>(cut, a, y, x, n, 1.f, v);\n  }\n', '    canvas_tap<ERASE>(cut, a, y, x, n, 1.f, v);\n  }\n  if (ERASE && in_rect(a, y, x)) v[0] = v[1] = v[2] = 0.f;\n')]),
    ('the elastic -0.5 dropped', [('(float)P / (float)(P - 1), -0.5f)', '(float)P / (float)(P - 1), 0.f)')]),
    ('P / (P - 1) -> 1', [('(float)P / (float)(P - 1), -0.5f)', '1.f, -0.5f)')]),
    ('the patch window offset by 4', [('const int y = i - (int)a[1], x = j - (int)a[0];',
                                       'const int y = i + (is_window<OUT>::v ? 4 : 0) - (int)a[1], x = j + (is_window<OUT>::v ? 4 : 0) - (int)a[0];')]),
]


def mutation_table():
    """Each mutant of csrc/sampler_kornia.h (a textual patch, built for the interpreter beside the real objects) must FAIL a forward parity
    check that the real kernels pass.  Prints one line per mutant: how many of the forward checks of the two small cases it fails."""
    import os
    import shutil
    import subprocess
    import sys
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, 'emu'))
    import build_emu
    build_emu.build()
    csrc, bdir = build_emu.CSRC, os.path.join(build_emu.HERE, 'build')
    checks = [(c, ch, m) for c in ('hand', 'drawn') for ch in CHAINS for m in FWD_MODES]

    def failures(lib):
        bad = []
        for chk in checks:
            try:
                check_forward(lib, 'cpu', *chk)
            except AssertionError:
                bad.append(case_id(chk))
        return bad
    assert not failures(_ffi.Library(build_emu.OUT)), 'the unmutated kernels fail'
    rows = []
    for name, patches in MUTANTS:
        with tempfile.TemporaryDirectory() as tmp:
            src = open(os.path.join(csrc, 'sampler_kornia.h')).read()
            for old, new in patches:
                assert old in src, (name, old)
                src = src.replace(old, new)
            open(os.path.join(tmp, 'sampler_kornia.h'), 'w').write(src)
            shutil.copy(os.path.join(csrc, 'sampler.hip'), tmp)
            obj, so = os.path.join(tmp, 'sampler.o'), os.path.join(tmp, 'libmutant.so')
            subprocess.check_call([build_emu.CLANG, '-x', 'c++', '-std=c++17', '-O2', '-fPIC', '-DAPH_EMU', '-Wno-unused-value', '-I', build_emu.HERE, '-I', tmp,
                                   '-I', csrc, '-I', os.path.join(build_emu.ROOT, 'include'), '-c', os.path.join(tmp, 'sampler.hip'), '-o', obj])
            others = [os.path.join(bdir, s + '.emu.o') for s in build_emu.SOURCES if s != 'sampler.hip']
            subprocess.check_call([build_emu.CLANG, '-shared', '-fPIC', '-o', so, obj] + others)
            bad = failures(_ffi.Library(so))
        rows.append((name, len(bad), len(checks), bad[:3]))
    print('\nmutant -> failed forward checks (of %d: two small cases x two chains x five layouts)' % len(checks))
    for name, nbad, ntot, some in rows:
        print('  %-36s %2d / %d   e.g. %s' % (name, nbad, ntot, ', '.join(some)))
    assert all(r[1] > 0 for r in rows), 'a mutant passes every check'


if __name__ == '__main__':
    mutation_table()
