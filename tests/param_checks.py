"""fp64 checks of the two image parameterisers -- the inverse DWT (csrc/dwt.hip) and the FFT synthesis (csrc/synth.hip) with their adjoints --
shared by the interpreter tests (test_emu_kernels.py) and the GPU tests (test_gpu_kernels.py).  `lib` = a loaded C-ABI library (the
interpreter build) or None (the product), `dev` = where its tensors live.

Every output sits inside a buffer with GUARD sentinel floats on either side and is prefilled with NaN: after the calls the sentinels are
bit-identical and no NaN is left.  Every call is made twice and must give the same bits.  Each case states which path it expects to take
(levels in the coarse tail; column tile and radices) and asserts it through aph_idwt_coarse_levels / aph_synth_plan_describe first.
The checks return their worst ratios; the callers print them (profiles/param_fp64_bounds.txt holds a run of each)."""
import ctypes
import math

import numpy as np
import torch

from aphantasia_amd import _ffi, ops
from oracle import dwt_ref
from oracle import reference_path as R
import vit_component_checks as V

U = 2.0 ** -24          # fp32 unit roundoff
GUARD = 256             # sentinel floats on either side of an output (1 KiB: the output keeps its 16-byte alignment)
MARGIN = 4.0            # kernel / fp32-oracle margin of the measured bounds: another summation order, FMA contraction, the noise of a maximum
#                         over few elements (measured kernel / oracle: 0.2 - 3.1 over every case on the interpreter and on one MI355X, the largest
#                         at the generic radices 29 / 31 and at 2 x 2, where a plane has four values: profiles/param_fp64_bounds.txt)


def guarded(shape, dev):
    """(whole buffer, NaN-prefilled view of `shape` between two sentinel bands)"""
    n = math.prod(shape)
    big = V.sentinel(1, n + 2 * GUARD, torch.float32, dev).reshape(-1)
    view = big[GUARD:GUARD + n].view(shape)
    view.fill_(float('nan'))
    return big, view


def assert_guards(big, what):
    b = V.bits(big)
    assert bool((b[:GUARD] == V.SENT32).all()) and bool((b[-GUARD:] == V.SENT32).all()), '%s: a store outside the output' % what
    assert not bool(torch.isnan(big[GUARD:-GUARD]).any()), '%s: %d elements never written (or NaN)' % (what, int(torch.isnan(big[GUARD:-GUARD]).sum()))


def rel_max(got, ref):
    """max |got - ref| / max |ref|  (fp64; NaN / inf in got -> inf)"""
    err = (got.double().cpu() - ref).abs().nan_to_num(float('inf')).max().item()
    return err / max(ref.abs().max().item(), 1e-300)


# ------------------------------------------------------------------------------------------------------------------------- inverse DWT
def check_idwt_fp64(lib, dev, wave, h, w, sharp=0.3, seed=0, tail=None):
    """DWTSynth.forward / backward (aph_idwt_fwd / aph_idwt_bwd: every level, the coarse tail in one launch) on `raw` itself against
    oracle/dwt_ref.py in float64 (autograd against a seeded gw).  `tail`: the number of levels the case expects in the coarse tail.

    (a) element-wise, derived:  |got - ref| <= gamma_n A + |ref - f32(ref)| + eta  for every element of raw and of every gradient tensor,
        where A is the same chain on |coefficients| with |rec_lo|, |rec_hi| (forward: A = |G_1| ... |G_J| |Y|; adjoint: its autograd
        gradient against |gw|), gamma_n = n U / (1 - n U), U = 2^-24, and n = J (2 L + 3): an element passes
        through at most J levels; per level two separable passes, each a sum of L products (one rounding per product and at most L - 1
        additions: L per pass, 2 L); the two taps of each term are rec_lo / rec_hi rounded to f32 and act once per pass (2, together
        with the f32 gain they enter as factors (1 + d), counted like roundings); the multiply by the level's gain hscale (1).
        A follows each element's own magnitude, so the finest bands and the rows beyond an edge are held as tightly as the coarse ones.
        eta = n 2^-126 max(1, max_j hscale_j) max(1, sum |taps|)^(2 J), about 1e-33, is the underflow term: (1 + d) holds in fp32's normal
        range; a result below 2^-126 loses up to the subnormal spacing (or itself, where a mode flushes), times the gains that follow.
        It matters for the long filters only: the corner of dmey's Yl reaches the image through twelve taps of ~1e-12 each (1e-146).
    (b) per tensor, measured:  max |got - ref| / max |ref| <= MARGIN x the figure of dwt_ref in float32 on the same inputs (its worst
        tensor of the case), for raw, Yl and every Yh_j separately.
    (c) forward twice and backward twice: the same bits.   (d) sentinels and NaN prefill (grad_flat, bufs[0]).
    (e) the per-level calls agree with the all-levels calls: bit-equal under the interpreter, 1e-6 of the maximum on the GPU (two
        instantiations may contract their multiply-adds differently).
    And one direct aph_idwt_level_bwd with ll_h = h + 1, ll_w = w + 1 on a NaN-prefilled d_ll_grad: the extra row and column are 0."""
    from aphantasia_amd.dwt import DWTSynth
    L_ = lib if lib is not None else _ffi.lib()
    torch.manual_seed(seed)
    Ys = dwt_ref.init_params([1, 3, h, w], wave)
    syn = DWTSynth(h, w, wave, sharp, dev, lib=lib)
    assert [tuple(y.shape) for y in Ys] == list(syn.shapes)
    J, Lf = syn.J, syn.L
    lv = syn._level_arrays()
    got_tail = L_.call('aph_idwt_coarse_levels', lv['hs'], lv['ws'], J, Lf)
    assert tail is None or got_tail == tail, 'expected %s levels in the coarse tail, the library takes %d' % (tail, got_tail)

    def run(dtype, absolute=False, gw_=None):
        ys = [(y.abs() if absolute else y).detach().to(dtype).clone().requires_grad_(True) for y in Ys]
        raw = dwt_ref.dwt_image_raw(ys, wave, sharp, absolute)
        g = gw_ if gw_ is not None else torch.randn(raw.shape, generator=torch.Generator().manual_seed(seed + 3))
        (raw * (g.abs() if absolute else g).to(dtype)).sum().backward()
        return raw.detach().double(), [y.grad.double() for y in ys], g
    raw64, g64, gw = run(torch.float64)
    raw32, g32, _ = run(torch.float32, gw_=gw)
    A_raw, A_g, _ = run(torch.float64, True, gw)
    assert tuple(raw64.shape[2:]) == (syn.H, syn.W)
    n = J * (2 * Lf + 3)
    gam = n * U / (1 - n * U)
    eta = n * 2.0 ** -126 * max(1.0, max(syn.scale)) * max(1.0, max(float(f.abs().sum()) for f in dwt_ref.filters(wave))) ** (2 * J)
    bound_of = lambda A, ref: gam * A + (ref - ref.float().double()).abs() + eta

    flat = torch.cat([y.reshape(-1) for y in Ys]).to(dev).contiguous()
    d_raw = gw[0].to(dev).contiguous()
    syn.bufs[0].fill_(float('nan'))
    raw = syn.forward(flat).clone()
    assert not bool(torch.isnan(raw).any())
    big, grad = guarded((syn.numel,), dev)
    syn.backward(d_raw, grad)
    assert_guards(big, 'idwt backward')
    # (c)
    assert torch.equal(syn.forward(flat), raw), 'forward: other bits on the second launch'
    big2, grad2 = guarded((syn.numel,), dev)
    syn.backward(d_raw, grad2)
    assert_guards(big2, 'idwt backward (second)')
    assert torch.equal(grad2, grad), 'backward: other bits on the second launch'
    # (a)
    V.assert_within(raw.cpu(), raw64[0], bound_of(A_raw[0], raw64[0]), 'raw')
    out = {'a_raw': ((raw.cpu().double() - raw64[0]).abs() / bound_of(A_raw[0], raw64[0])).max().item()}
    gv = [g.cpu() for g in syn.views(grad)]
    names = ['Yl'] + ['Yh%d' % j for j in range(J)]
    worst_a = 0.0
    for name, got, ref, A in zip(names, gv, g64, A_g):
        V.assert_within(got, ref, bound_of(A, ref), 'grad ' + name)
        worst_a = max(worst_a, ((got.double() - ref).abs() / bound_of(A, ref)).max().item())
    out['a_grad'] = worst_a
    # (b)
    orc = {'raw': rel_max(raw32, raw64)}
    ker = {'raw': rel_max(raw, raw64[0])}
    for name, got, r32, ref in zip(names, gv, g32, g64):
        orc[name], ker[name] = rel_max(r32, ref), rel_max(got, ref)
    worst = max(orc.values())
    for name in ker:
        assert ker[name] <= MARGIN * worst, '%s: max err / max |ref| %.3g, fp32 oracle %.3g (its worst tensor %.3g)' % (name, ker[name], orc[name], worst)
    out['b_raw'] = ker['raw'] / worst
    out['b_Yl'] = ker['Yl'] / worst
    out['b_Yh'] = max(ker[k] for k in names[1:]) / worst
    out['oracle'] = worst
    # (e)
    raw2 = syn.forward_per_level(flat).clone()
    big3, grad3 = guarded((syn.numel,), dev)
    syn.backward_per_level(d_raw, grad3)
    assert_guards(big3, 'idwt backward per level')
    if dev == 'cpu':
        assert torch.equal(raw2, raw) and torch.equal(grad3, grad)
    else:
        assert (raw2 - raw).abs().max().item() <= 1e-6 * raw.abs().max().item()
        assert (grad3 - grad).abs().max().item() <= 1e-6 * grad.abs().max().item()
    # the low-band row / column that DWTInverse drops: zero gradient, the rest as without them
    hh, ww = syn.sizes[0]
    C = syn.C
    gh = torch.empty(C, 3, hh, ww, device=dev)
    bigl, gll = guarded((C, hh + 1, ww + 1), dev)
    st = ops._stream(flat)
    L_.call('aph_idwt_level_bwd', ops.ptr(d_raw), hh, ww, C, ops.ptr(syn.g0), ops.ptr(syn.g1), Lf, float(syn.scale[0]), ops.ptr(gll), hh + 1, ww + 1,
            ops.ptr(gh), st)
    assert_guards(bigl, 'aph_idwt_level_bwd with a dropped row and column')
    assert float(gll[:, hh, :].abs().max()) == 0.0 and float(gll[:, :, ww].abs().max()) == 0.0
    bigm, glm = guarded((C, hh, ww), dev)
    gh2 = torch.empty_like(gh)
    L_.call('aph_idwt_level_bwd', ops.ptr(d_raw), hh, ww, C, ops.ptr(syn.g0), ops.ptr(syn.g1), Lf, float(syn.scale[0]), ops.ptr(glm), hh, ww,
            ops.ptr(gh2), st)
    assert_guards(bigm, 'aph_idwt_level_bwd')
    assert torch.equal(gll[:, :hh, :ww], glm) and torch.equal(gh, gh2)
    return out


# --------------------------------------------------------------------------------------------------------------------------------- FFT
def describe_plan(lib, plan):
    """(TC, radices of H, radices of W) through aph_synth_plan_describe"""
    L_ = lib if lib is not None else _ffi.lib()
    o = (ctypes.c_int * 31)()
    L_.call('aph_synth_plan_describe', plan.handle, o)
    return o[0], [o[2 + i] for i in range(o[1])], [o[17 + i] for i in range(o[16])]


def _planes(got, ref):
    """per plane max |got - ref| / max |ref|"""
    return [rel_max(got[c], ref[c]) for c in range(ref.shape[0])]


def _hold(ratios, what, kernel, oracle, floor=U):
    """the measured rule: per plane, kernel <= MARGIN x max(fp32 oracle, floor); records the worst kernel / max(oracle, floor)"""
    worst = 0.0
    for c, (k, o) in enumerate(zip(kernel, oracle)):
        lim = max(o, floor)
        assert k <= MARGIN * lim, '%s plane %d: max err / max |ref| %.3g, fp32 oracle %.3g' % (what, c, k, o)
        worst = max(worst, k / lim)
    ratios[what] = worst


def check_fft_fp64(lib, dev, h, w, seed=0, tc=None, rad_h=None, rad_w=None):
    """aph_irfft2 / aph_rfft2 / aph_synth_fft_fwd / aph_synth_fft_bwd / aph_synth_stats / aph_synth_set_stats against torch.fft and
    reference_path.synth_fft in float64.  tc / rad_h / rad_w: the column tile and the radices (in pass order) the case expects.

    Measured rule (no derived element bound: an FFT's error is spread evenly, every output sums every input): per plane,
    max |got - ref| / max |ref| <= MARGIN x max(the same torch calls in float32, U).  MARGIN = 4 covers another factorisation and summation
    order, FMA contraction, and the direct-DFT passes of the generic radices, whose (R - 1)-term sums torch's specialised butterflies do
    not have.  The gradient is held twice: as it is, and divided by scale[ky, kx] (which spans 425 : 1 at 180 x 320), so that its
    high-frequency elements count as much as the low ones.  rgb: absolute error <= MARGIN x the fp32 oracle's.  {mean, std}: within
    f32 rounding of the fp64 statistics of the kernel's own raw, and of the reference's widened by the oracle's figure for raw."""
    L_ = lib if lib is not None else _ffi.lib()
    plan = ops.SynthPlan(3, h, w, lib=lib)
    got_tc, got_rh, got_rw = describe_plan(lib, plan)
    assert tc is None or got_tc == tc, 'expected TC %s, the plan has %d' % (tc, got_tc)
    assert rad_h is None or got_rh == list(rad_h), 'expected radices of H %s, the plan has %s' % (rad_h, got_rh)
    assert rad_w is None or got_rw == list(rad_w), 'expected radices of W %s, the plan has %s' % (rad_w, got_rw)
    assert math.prod(got_rh) == h and math.prod(got_rw) == w
    g = torch.Generator().manual_seed(seed + 6)
    wc = w // 2 + 1
    out = {}
    st = ops._stream(torch.empty(1, device=dev))

    def twice(shape, call, what):
        """runs call(view) on two guarded buffers; same bits, guards intact; returns the first result"""
        big, v = guarded(shape, dev)
        call(v)
        assert_guards(big, what)
        big2, v2 = guarded(shape, dev)
        call(v2)
        assert_guards(big2, what + ' (second)')
        assert torch.equal(v, v2), '%s: other bits on the second launch' % what
        return v

    # ---- the transform pair
    spec = torch.randn(3, h, wc, 2, generator=g)
    want = torch.fft.irfftn(torch.view_as_complex(spec.double()), s=(h, w), norm='ortho')
    o32 = torch.fft.irfftn(torch.view_as_complex(spec), s=(h, w), norm='ortho')
    spec_d = spec.to(dev).contiguous()
    got = twice((3, h, w), lambda v: ops.irfft2(plan, spec_d, out=v, lib=lib), 'aph_irfft2')
    _hold(out, 'irfft2', _planes(got, want), _planes(o32, want))
    img = torch.randn(3, h, w, generator=g)
    want = torch.view_as_real(torch.fft.rfftn(img.double(), s=(h, w), dim=[1, 2], norm='ortho'))
    o32 = torch.view_as_real(torch.fft.rfftn(img, s=(h, w), dim=[1, 2], norm='ortho'))
    img_d = img.to(dev).contiguous()
    got = twice((3, h, wc, 2), lambda v: ops.rfft2(plan, img_d, out=v, lib=lib), 'aph_rfft2')
    _hold(out, 'rfft2', _planes(got, want), _planes(o32, want))

    # ---- synthesis: shift, contrast 1.1, colour matrix; then without the colour matrix (decorrelate = 0; colcorr_t9 = NULL)
    params = 0.01 * torch.randn(1, 3, h, wc, 2, generator=g)
    # (fft_scale is symmetric in ky <-> H - ky; a seeded factor per element makes a wrongly indexed scale visible and keeps its range)
    scale = R.fft_scale(h, w, 1.5) * (1.0 + 0.25 * torch.rand(h, wc, generator=g))
    shift = 0.02 * torch.rand(1, 1, h, wc, 1, generator=g)
    cc_t = R.colcorr_t(1.8)
    contrast = float(np.float32(1.1))            # (the value the C ABI receives)
    gw = torch.randn(1, 3, h, w, generator=g)
    gscale = 0.5

    def reference(dtype, decorrelate, sh=shift, pr=params):
        p = pr.detach().to(dtype).clone().requires_grad_(True)
        raw = R.fft_image_raw(p, scale.to(dtype), h, w, None if sh is None else sh.to(dtype))
        rgb = R.to_rgb(R.std_normalise(raw, contrast), cc_t.to(dtype), decorrelate)
        (rgb * gw.to(dtype) * gscale).sum().backward()
        return raw.detach()[0].double(), rgb.detach()[0].double(), p.grad[0].double()
    params_d, scale_d = params[0].to(dev).contiguous(), scale.to(dev).contiguous()
    shift_d = shift.reshape(h, wc).to(dev).contiguous()
    gw_d = gw[0].to(dev).contiguous()
    cc9 = _ffi.floats(cc_t.flatten().tolist())
    sdiv = scale.double()[None, :, :, None]

    def fwd(pd, cc, decor, raw_v, rgb_v, sh=shift_d):
        L_.call('aph_synth_fft_fwd', plan.handle, ops.ptr(pd), ops.ptr(scale_d), ops.ptr(sh), contrast, cc, decor, ops.ptr(raw_v), ops.ptr(rgb_v), st)

    def bwd(raw_v, rgb_v, cc, decor, grad_v):
        L_.call('aph_synth_fft_bwd', plan.handle, ops.ptr(gw_d), gscale, ops.ptr(rgb_v), ops.ptr(raw_v), ops.ptr(scale_d), contrast, cc, decor,
                ops.ptr(grad_v), st)

    refs = {}
    for tag, cc, decor in (('', cc9, 1), (' plain', cc9, 0), (' nocc', None, 1)):
        coloured = tag == ''
        if coloured not in refs:
            refs[coloured] = reference(torch.float64, coloured) + reference(torch.float32, coloured)
        raw64, rgb64, grad64, raw32, rgb32, grad32 = refs[coloured]
        bigs = [guarded((3, h, w), dev) for _ in range(4)]
        fwd(params_d, cc, decor, bigs[0][1], bigs[1][1])
        stats = torch.full((2,), float('nan'), device=dev)
        L_.call('aph_synth_stats', plan.handle, ops.ptr(stats), st)
        fwd(params_d, cc, decor, bigs[2][1], bigs[3][1])
        for b, _ in bigs:
            assert_guards(b, 'aph_synth_fft_fwd' + tag)
        raw, rgb = bigs[0][1], bigs[1][1]
        assert torch.equal(raw, bigs[2][1]) and torch.equal(rgb, bigs[3][1]), 'aph_synth_fft_fwd%s: other bits on the second launch' % tag
        o_raw = _planes(raw32, raw64)
        _hold(out, 'raw' + tag, _planes(raw, raw64), o_raw)
        e_rgb, o_rgb = (rgb.double().cpu() - rgb64).abs().max().item(), (rgb32 - rgb64).abs().max().item()
        assert e_rgb <= MARGIN * o_rgb, 'rgb%s: max abs err %.3g, fp32 oracle %.3g' % (tag, e_rgb, o_rgb)
        out['rgb' + tag] = e_rgb / o_rgb
        if coloured:
            s = stats.double().cpu()
            own = raw.double().cpu()
            assert abs(s[0] - own.mean()).item() <= U * abs(own.mean().item()) + 1e-12 * own.std().item(), (s[0].item(), own.mean().item())
            assert abs(s[1] - own.std()).item() <= U * own.std().item() * (1 + 1e-5), (s[1].item(), own.std().item())
            widen = max(o_raw) * raw64.abs().max().item()
            assert abs(s[0] - raw64.mean()).item() <= U * abs(raw64.mean().item()) + widen
            assert abs(s[1] - raw64.std()).item() <= U * raw64.std().item() + widen * (raw64.numel() / (raw64.numel() - 1.0)) ** 0.5
        grad = twice((3, h, wc, 2), lambda v: bwd(raw, rgb, cc, decor, v), 'aph_synth_fft_bwd' + tag)
        _hold(out, 'grad' + tag, _planes(grad, grad64), _planes(grad32, grad64))
        _hold(out, 'grad/scale' + tag, _planes(grad.double().cpu() / sdiv, grad64 / sdiv), _planes(grad32 / sdiv, grad64 / sdiv))
        if not coloured:
            continue
        # ---- the statistics of forward(A) survive another forward: saved, restored, the same gradient bit for bit
        s_A = stats.clone()
        pB = (2.0 * params_d).contiguous()
        rawB, rgbB = torch.empty_like(raw), torch.empty_like(rgb)
        fwd(pB, cc, decor, rawB, rgbB, sh=None)
        stale = torch.empty_like(grad)
        bwd(raw, rgb, cc, decor, stale)
        assert not torch.equal(stale, grad), "forward(B) left forward(A)'s statistics in the plan: the round trip below would show nothing"
        L_.call('aph_synth_set_stats', plan.handle, ops.ptr(s_A), st)
        back = torch.empty_like(grad)
        bwd(raw, rgb, cc, decor, back)
        assert torch.equal(back, grad), 'aph_synth_set_stats(aph_synth_stats) did not restore the backward of forward(A)'
        s_B = torch.empty_like(s_A)
        L_.call('aph_synth_stats', plan.handle, ops.ptr(s_B), st)
        assert torch.equal(s_B, s_A)
    return out


# ------------------------------------------------------------------------------------------------------------------------------- cases
# (wave, h, w, levels expected in the coarse tail).  The tail kernels exist for L = 2, 4, 6, 8; its finest level is bounded by an output of
# 80 x 128 (haar) or, for the longer filters, by a coefficient band of 40 x 64.
def _idwt_cases():
    cases = []
    for wave, L in (('haar', 2), ('db2', 4), ('db3', 6), ('db4', 8), ('coif2', 12),           # every template (coif2: H2T 6 / LT 12, no tail)
                    ('sym5', 10), ('db7', 14), ('db10', 20)):                                    # run-time filter length
        for (h, w) in ((45, 70), (130, 84), (200, 300)):         # odd: the dropped row / column; portrait; several tiles per level, then the tail
            cases.append((wave, h, w, 5 if L <= 8 else 0))
    for wave in ('db20', 'coif10', 'dmey'):                       # L = 40, 60, 62: 116 - 120 KB of LDS; their bands never drop below L - 1
        cases += [(wave, 70, 90, 0), (wave, 33, 47, 0)]
    # tail boundary per instantiated length: the largest frame whose level 1 the tail still takes (6 of 7 levels), then one coefficient
    # over in H only and in W only (5 levels: level 1 goes to the per-level kernel)
    for wave, h, w in (('haar', 160, 256), ('db2', 154, 250), ('db3', 148, 244), ('db4', 142, 238)):
        cases += [(wave, h, w, 6), (wave, h + 2, w, 5), (wave, h, w + 2, 5)]
    return cases


IDWT_CASES = _idwt_cases()
IDWT_CASES_PRODUCT = [('db4', 540, 960, 5), ('sym5', 960, 540, 0)]          # GPU only (the fp64 oracle on the CPU is the larger part)

# (h, w, TC, radices of H, radices of W, runs under the interpreter too).  On the interpreter a case costs about 25 s whatever its size (the
# 1024-workgroup element-wise launches of every synthesis call), so only the small frames with a path of their own run there.
FFT_CASES = [
    (2, 2, 8, [2], [2], True), (2, 3, 8, [2], [3], False), (3, 2, 8, [3], [2], True),                          # minimum sizes
    (22, 51, 8, [2, 11], [3, 17], False), (76, 115, 8, [4, 19], [5, 23], False), (58, 93, 8, [2, 29], [3, 31], True),   # generic radices 11 - 31
    (49, 121, 8, [7, 7], [11, 11], True),                                                                     # squares
    (127, 74, 8, [127], [2, 37], False), (74, 127, 8, [2, 37], [127], True), (6, 4099, 8, [2, 3], [4099], False),      # one direct-sum pass, R = N
    (1369, 6, 5, [37, 37], [2, 3], False),                                                                    # two direct-sum passes
    (1280, 24, 6, [4, 4, 4, 4, 5], [4, 2, 3], False),                 # TC 6, 39 columns: a ragged last tile
    (2160, 20, 3, [4, 4, 3, 3, 3, 5], [4, 5], False), (4100, 6, 1, [4, 5, 5, 41], [2, 3], False),
    (8192, 4, 1, [4, 4, 4, 4, 4, 4, 2], [4], False),                  # 128 KB of column LDS
    (4, 8192, 8, [4], [4, 4, 4, 4, 4, 4, 2], False),                  # 128 KB of row LDS
    (1280, 720, 6, [4, 4, 4, 4, 5], [4, 4, 3, 3, 5], False), (2160, 3840, 3, [4, 4, 3, 3, 3, 5], [4, 4, 4, 4, 3, 5], False),      # product shapes
]


def show(tag, ratios):
    print('%s: %s' % (tag, '  '.join('%s %.3g' % kv for kv in ratios.items())))
