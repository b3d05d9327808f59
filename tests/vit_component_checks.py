"""Element-wise fp64 checks of the f16 ViT path's GEMM epilogues and LayerNorm variants (the launches `vit.hip` makes), shared by the
interpreter tests (test_emu_kernels.py) and the GPU tests (test_gpu_kernels.py).  `lib` = a loaded C-ABI library (the interpreter build)
or None (the product), `dev` = where its tensors live.

Every check fills its outputs with a NaN-payload sentinel and requires, besides the element bounds, that every element outside the
written window keeps the sentinel bit for bit, that the inputs are unchanged and that a second identical call gives the same bits."""
import ctypes

import torch

from aphantasia_amd import ops

EPI_F32, EPI_F16, EPI_F16_SCALE, EPI_RESIDUAL, EPI_GELU, EPI_GELU_BWD, EPI_PATCH_EMBED = range(7)     # APH_EPI_* (aphantasia_hip_test.h)
F16_OUT = (EPI_F16, EPI_F16_SCALE, EPI_GELU, EPI_GELU_BWD)
U = 2.0 ** -24                   # fp32 unit roundoff
H = 2.0 ** -11                   # f16 unit roundoff (round to nearest: |fl16(y) - y| <= 2^-11 |y| in the normal range)
H_SUB = 2.0 ** -25               # half the f16 subnormal spacing
F16_INF_AT = 65520.0             # fp32 values of at least this magnitude round to +-inf in f16
SENT32 = 0x7FC0DEAD              # NaN payloads no kernel produces
SENT16 = 0x7E5A
GUARD_ROWS = 16


def sentinel(rows, cols, dtype, dev):
    if dtype == torch.float32:
        return torch.full((rows, cols), SENT32, dtype=torch.int32, device=dev).view(torch.float32)
    return torch.full((rows, cols), SENT16, dtype=torch.int16, device=dev).view(torch.float16)


def bits(t):
    t = t.detach().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def assert_untouched(buf, written, what):
    """every element of `buf` outside the boolean mask `written` still holds the sentinel"""
    b = bits(buf)
    want = SENT32 if buf.dtype == torch.float32 else SENT16
    bad = (b != want) & ~written
    assert not bad.any(), '%s: %d stray stores, first at %s' % (what, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound element-wise (NaN / inf in got fail)"""
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        ratio = (err / bound).nan_to_num(float('inf')).max().item()
        raise AssertionError('%s: %d elements out of bound (worst err / bound %.3g); first at %s: got %r, want %r, bound %.3g' %
                             (what, int((~ok).sum()), ratio, i, got[i].item(), ref[i].item(), bound[i].item()))


def assert_f16(got, ref, e, what):
    """an f16 store of a value known to within e of ref: round to nearest (|out - ref| <= e + 2^-11 |ref| + 2^-25), and +-inf with the sign of
    ref where |ref| - e >= 65520; values within e of the overflow threshold may go either way.  Returns the number of infinities checked."""
    g = got.double()
    e = e.expand_as(ref)
    mag = ref.abs()
    over = mag - e >= F16_INF_AT
    amb = ~over & (mag + e >= F16_INF_AT)
    if over.any():
        want = torch.where(ref > 0, torch.tensor(float('inf'), dtype=torch.float64), torch.tensor(float('-inf'), dtype=torch.float64))
        assert torch.equal(g[over], want[over]), '%s: %d overflowing elements are not +-inf' % (what, int((g[over] != want[over]).sum()))
    fin = ~over & ~amb
    assert_within(got[fin], ref[fin], (e + H * mag + H_SUB)[fin], what)
    return int(over.sum())


# ------------------------------------------------------------------------------------------------------------------------------ GEMM
def gemm_epi(lib, A, lda, Bt, ldb, M, N, K, kind, out, ldo, aux=None, bias=None, res=None, scale=1.0, P=0, T=0, tile_cfg=0, ws=None,
             small_batch=1):
    ops._L(lib, A).call('aph_gemm_f16_epi_test', ops.ptr(A), lda, ops.ptr(Bt), ldb, M, N, K, ops.ptr(out), ldo, ops.ptr(aux), ops.ptr(bias),
                        ops.ptr(res), ctypes.c_float(scale), kind, P, T, tile_cfg, ops.ptr(ws), 0 if ws is None else ws.numel(), small_batch,
                        ops._stream(A))


def _operands(g, M, N, K, lda, ldb, over_rows, scale):
    """A [M, lda], Bt [N, ldb] f16 with NaN in the pitch padding (never read); |acc| ~ 1, except on over_rows, where |acc| ~ 65520 / |scale|"""
    A = torch.randn(M, lda, generator=g) * (2.0 / K ** 0.5)
    if over_rows:
        sig = min(3.0 * F16_INF_AT / (K ** 0.5 * abs(scale)), 14000.0)        # (4 sigma stays inside the f16 range)
        A[over_rows] = torch.randn(len(over_rows), lda, generator=g).clamp(-4, 4) * sig
    Bt = torch.randn(N, ldb, generator=g) * 0.5
    A[:, K:] = float('nan')
    Bt[:, K:] = float('nan')
    return A.half(), Bt.half()


def patch_geom(M):
    """(P, T) of a patch-embedding launch over M patch rows: S = the smallest factor of M above 1 images of P patches, T = P + 1 tokens"""
    S = next(d for d in range(2, M + 1) if M % d == 0) if M > 1 else 1
    return M // S, M // S + 1


def quick_gelu_ref(acc, bias, e_acc):
    """fp64 QuickGELU of u = acc + bias and the element bounds of the kernel's g and dg/du (before their f16 rounding).
    u is formed in fp32 from an accumulator that is e_acc off: eu = e_acc + 2^-24 (|acc| + |bias|).
    s = v_rcp_f32(1 + __expf(-1.702f u)): t = -1.702f u carries 2 roundings of |t| (constant, product) and __expf one more in its exp2
    argument (x log2 e), each a relative error 2^-24 |t| of E = exp(t); v_exp_f32 and v_rcp_f32 are 1 ulp (2^-23), 1 + E one rounding:
        eps_s = (1 - s) (3 * 2^-24 |t| + 2^-23) + 2^-24 + 2^-23            (relative error of s)
    g = u s:  |dg/du| eu (input error) + |g| (eps_s + 2^-24)
    dg = s + 1.702 (g - g s), the exact derivative s (1 + 1.702 u (1 - s)):  |d(dg)/du| <= 1.11 everywhere (max of 1.702 s(1-s) (2 + 1.702 u (1 - 2s))),
    so 1.2 eu from the input; g and g s carry 2 eps_s + 2^-22 relative, their difference 2^-24 of |g| more, the product with 1.702f 2^-23 of
    the result, + s its eps_s and 2^-24 of |dg|:  1.2 eu + 1.702 |g| (3 eps_s + 2^-21) + s eps_s + 2^-23 |dg|"""
    u = acc + bias
    eu = e_acc + U * (acc.abs() + bias.abs())
    s = torch.sigmoid(1.702 * u)
    gv = u * s
    dg = s * (1 + 1.702 * u * (1 - s))
    eps_s = (1 - s) * (3 * U * (1.702 * u).abs() + 2 * U) + 3 * U
    e_g = dg.abs() * eu + gv.abs() * (eps_s + U)
    e_dg = 1.2 * eu + 1.702 * gv.abs() * (3 * eps_s + 8 * U) + s * eps_s + 2 * U * dg.abs()
    return gv, dg, e_g, e_dg


def check_gemm_epilogue(lib, dev, kind, tile_cfg, M, N, K, lda=None, ldb=None, ldo=None, bias=True, scale=1.0, res_mag=4.0, P=0, T=0,
                        ws_floats=0, small_batch=1, overflow=True, seed=0, ws_residual=False, mfma_k=32):
    """One f16 GEMM with epilogue `kind` on tile configuration `tile_cfg` against fp64, element by element, plus the guard, input and
    repeatability checks.  e_acc = 1e-6 sum_k |a_k b_k| (the exact path's figure; the analytic worst case of K/32 accumulator roundings is
    (K/32) 2^-24 sum|ab|, which random operands do not approach).  ws_residual: the residual bound of the wave-specialised kernel
    (see below); mfma_k: products per accumulator rounding (32 for v_mfma_f32_16x16x32_f16; 1 under the interpreter, whose MFMA adds the
    products one by one).  Returns {'ratio': worst err / tight residual bound, 'inf': overflowing elements checked}."""
    g = torch.Generator().manual_seed(seed)
    lda, ldb = lda or K, ldb or K
    if ldo is None:
        ldo = N if kind == EPI_PATCH_EMBED else N + 8
    if kind == EPI_PATCH_EMBED and not P:
        P, T = patch_geom(M)
    over_rows = sorted({M - 1, M // 2}) if (overflow and kind in F16_OUT) else []
    A, Bt = _operands(g, M, N, K, lda, ldb, over_rows, scale)
    b = (torch.randn(N, generator=g) * 0.5) if (bias or kind in (EPI_RESIDUAL, EPI_GELU)) else None
    rows = M + GUARD_ROWS
    res = aux = pos = None
    if kind == EPI_RESIDUAL:
        res = torch.randn(rows, ldo, generator=g) * res_mag
    if kind == EPI_GELU_BWD:
        aux = (torch.rand(rows, ldo, generator=g) * 1.2 - 0.1).half()            # dg/du of the forward: (-0.1, 1.1)
    if kind == EPI_PATCH_EMBED:
        assert M % P == 0 and T > P
        pos = torch.randn(T, N, generator=g)
        out_shape, out_dt = ((M // P) * T + GUARD_ROWS, N), torch.float32
    else:
        out_shape, out_dt = (rows, ldo), (torch.float16 if kind in F16_OUT else torch.float32)
    ins = {'A': A, 'Bt': Bt, 'bias': b, 'res': res, 'dg': aux, 'pos': pos}
    ins_d = {k: (None if v is None else v.clone().to(dev)) for k, v in ins.items()}      # (a copy: .to() of a CPU tensor aliases it)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=dev) if ws_floats else None

    def run():
        out = sentinel(*out_shape, out_dt, dev)
        dgo = sentinel(rows, ldo, torch.float16, dev) if kind == EPI_GELU else None
        gemm_epi(lib, ins_d['A'], lda, ins_d['Bt'], ldb, M, N, K, kind, out, ldo, aux=dgo if kind == EPI_GELU else ins_d['dg'],
                 bias=ins_d['pos'] if kind == EPI_PATCH_EMBED else ins_d['bias'], res=ins_d['res'], scale=scale, P=P, T=T, tile_cfg=tile_cfg,
                 ws=ws, small_batch=small_batch)
        return out.cpu(), (None if dgo is None else dgo.cpu())
    out, dgo = run()
    out2, dgo2 = run()
    what = 'epi %d tile_cfg %d M=%d N=%d K=%d lda=%d ldb=%d ldo=%d' % (kind, tile_cfg, M, N, K, lda, ldb, ldo)
    assert torch.equal(bits(out), bits(out2)) and (dgo is None or torch.equal(bits(dgo), bits(dgo2))), what + ': two identical calls differ'
    for k, v in ins.items():
        if v is not None:
            assert torch.equal(bits(ins_d[k]), bits(v)), '%s: input %s changed' % (what, k)

    Am, Bm = A[:, :K].double(), Bt[:, :K].double()
    acc = Am @ Bm.t()
    e_acc = 1e-6 * (Am.abs() @ Bm.abs().t())
    win = torch.zeros(out_shape, dtype=torch.bool)
    stats = {'inf': 0, 'ratio': 0.0}
    if kind == EPI_PATCH_EMBED:
        m = torch.arange(M)
        orow = (m // P) * T + 1 + m % P
        pe = pos.double()[1 + m % P]
        win[orow, :] = True
        assert_within(out[orow], acc + pe, e_acc + 2 * U * (acc.abs() + pe.abs()), what)
        assert_untouched(out, win, what + ' (x0 outside the patch rows: class rows, guard rows)')
        return stats
    win[:M, :N] = True
    got = out[:M, :N]
    bd = torch.zeros(N, dtype=torch.float64) if b is None else b.double()
    if kind == EPI_F32:
        ref = acc * scale
        assert_within(got, ref, e_acc * abs(scale) + U * ref.abs(), what)
    elif kind == EPI_F16:
        ref = acc + bd
        stats['inf'] = assert_f16(got, ref, e_acc + U * (acc.abs() + bd.abs()), what)
    elif kind == EPI_F16_SCALE:
        ref = acc * scale
        stats['inf'] = assert_f16(got, ref, e_acc * abs(scale) + U * ref.abs(), what)
    elif kind == EPI_RESIDUAL:
        r = res[:M, :N].double()
        ref = r + acc + bd
        tight = e_acc + 2 * U * (r.abs() + acc.abs() + bd.abs())
        stats['ratio'] = ((got.double() - ref).abs() / tight).max().item()
        if ws_residual:
            # The wave-specialised kernel starts its accumulators at res + bias (vit_gemm_ws.h, ws_init), so each of its K/32 MFMA
            # accumulations rounds at the scale of |res + bias| (2^-24 each), plus the initial sum and the last partial: a bound of
            # (K/32 + 2) 2^-24 (|res| + |bias|) + e_acc, where the ring kernels round res + acc + bias twice at the end.
            bound = (K / mfma_k + 2) * U * (r.abs() + bd.abs()) + e_acc
        else:
            bound = tight
        assert_within(got, ref, bound, what)
    elif kind == EPI_GELU:
        gv, dg, e_g, e_dg = quick_gelu_ref(acc, bd, e_acc)
        stats['inf'] = assert_f16(got, gv, e_g, what + ' (g)')
        assert_f16(dgo[:M, :N], dg, e_dg, what + ' (dg/du)')
        win_dg = torch.zeros(rows, ldo, dtype=torch.bool)
        win_dg[:M, :N] = True
        assert_untouched(dgo, win_dg, what + ' (dg/du)')
    elif kind == EPI_GELU_BWD:
        d = aux[:M, :N].double()
        ref = acc * d
        stats['inf'] = assert_f16(got, ref, e_acc * d.abs() + U * ref.abs(), what)
    assert_untouched(out, win, what)
    if over_rows:
        assert stats['inf'] > 0, what + ': the overflow rows produced no infinity to check'
    return stats


# ------------------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_call(lib, mode, D, M, T, xs=1, res_T=0, flags=0, x=None, g=None, b=None, dy=None, res=None, out=None, out2=None, cls=None, pos=None,
            x_fill=None, x2=None, g2=None, b2=None):
    P = ops.ptr
    ops._L(lib, x).call('aph_ln_test', mode, D, M, T, xs, res_T, flags, P(x), P(g), P(b), P(dy), P(res), P(out), P(out2), P(cls), P(pos),
                        P(x_fill), P(x2), P(g2), P(b2), ops._stream(x))


def ln_fwd_ref(x, g, b):
    """fp64 LayerNorm of the rows of x and the bound of an fp32 kernel's result: mean and variance are sums of D terms (4 NV per lane, then
    a 6-level wave butterfly: <= 4 NV + 8 roundings of their magnitude); the centred value carries the mean's error, xhat the relative error of
    rstd (<= (2 NV + 8) 2^-24 with v_rsq_f32's ulp), the affine map 4 roundings:  48 2^-24 (|g| (rstd mean|x| + |xhat|) + |b|) (NV <= 4)."""
    x = x.double()
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / ((x - mu).pow(2).mean(1, keepdim=True) + 1e-5).sqrt()
    xh = (x - mu) * rstd
    y = xh * g.double() + b.double()
    e = 48 * U * (g.double().abs() * (rstd * x.abs().mean(1, keepdim=True) + xh.abs()) + b.double().abs())
    return y, e


def ln_bwd_ref(dy, x, g):
    """fp64 LayerNorm input gradient rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) and the bound of an fp32 kernel's result: every term carries
    the relative error of the statistics and of xhat (which grows with the cancellation rstd mean|x|) and the roundings of its D-term sums.
    gain: the map's bound on an error in dy (|d dx| <= gain max|d dy|), for a LayerNorm backward fused behind another one."""
    x, gd = x.double(), dy.double() * g.double()
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / ((x - mu).pow(2).mean(1, keepdim=True) + 1e-5).sqrt()
    xh = (x - mu) * rstd
    dx = rstd * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
    s1 = gd.abs().mean(1, keepdim=True)
    s2 = (gd * xh).abs().mean(1, keepdim=True)
    rho = 1 + rstd * x.abs().mean(1, keepdim=True)
    xm = xh.abs().max(1, keepdim=True).values
    e = 128 * U * rho * rstd * (gd.abs() + s1 + (1 + xh.abs()) * (s2 + s1 * xm)) + 2 * U * dx.abs()
    gain = rstd * g.double().abs().max() * (2 + xm * xm)
    return dx, e, gain


def _ln_inputs(gen, rows, D, offset=3.0):
    """rows of x with a per-row offset (the cancellation in x - mean), gains around 1 and biases around 0"""
    x = torch.randn(rows, D, generator=gen) + offset * torch.randn(rows, 1, generator=gen)
    gam = 1.0 + 0.3 * torch.randn(D, generator=gen)
    bet = 0.2 * torch.randn(D, generator=gen)
    return x, gam, bet


def _window(rows, cols, which):
    w = torch.zeros(rows, cols, dtype=torch.bool)
    w[which] = True
    return w


def _check_hilo(o16, y, e, D, what):
    hi, lo = o16[:, :D], o16[:, D:]
    assert_f16(hi, y, e, what + ' (hi)')
    # lo = f16(o - hi) with o - hi exact in fp32: hi + lo is the kernel's fp32 value to 2^-22 |o| (+ half an f16 subnormal step)
    assert_within(hi.double() + lo.double(), y, e * (1 + 2.0 ** -22) + 2.0 ** -22 * y.abs() + H_SUB, what + ' (hi + lo)')


def _twice(run, what):
    """run() twice: the same bits (every returned tensor)"""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert (x is None) == (y is None) and (x is None or torch.equal(bits(x), bits(y))), what + ': two identical calls differ'
    return a


def _unchanged(dd, ins, what):
    for k, v in ins.items():
        assert v is None or torch.equal(bits(dd[k]), bits(v)), '%s: input %s changed' % (what, k)


LN_CASES = ['pre', 'pre_ln1', 'pre_ln1_hilo', 'ln_f16', 'ln_f16_hilo', 'ln_f16_cls', 'bwd_ln2', 'bwd_ln2_cls', 'bwd_ln2_f16', 'bwd_ln1_fused',
            'bwd_ln1', 'bwd_ln1_res_T', 'bwd_pre']


def check_layernorm(lib, dev, case, D, S=3, T=5, seed=0):
    """One of the f16 path's LayerNorm launches (vit.hip; the launchers themselves are in vit_ops.h) against fp64:
      pre            ln_pre with class fill (x_fill = x0, as the ViT launches it), alone                           (vit_forward_impl, fusion off)
      pre_ln1[_hilo] the same fused with the first block's ln_1, f16 output ([hi | lo] rows)                        (vit_forward_impl)
      ln_f16[_hilo]  ln_1 / ln_2 with f16 output on all rows (xs = 1; hilo: ln_1 of the split-precision forward)     (vit_forward_impl)
      ln_f16_cls     ln_2 of the last block on its class rows only (xs = T)                                         (vit_forward_impl)
      bwd_ln2        ln_2 backward, fp32 residual stream: res aliases out32 (res2 = dx), + the f16 copy             (vit_backward_impl)
      bwd_ln2_cls    the same on the class rows of the last block (xs = T)                                          (vit_backward_impl)
      bwd_ln2_f16    ln_2 backward with res_f16: res aliases out16, no fp32 stream, xs = T                          (vit_backward_impl)
      bwd_ln1_fused  ln_1 backward with res_T = T fused with ln_pre's backward (PATCH_ROWS output)                  (vit_backward_impl)
      bwd_ln1[_res_T] ln_1 backward unfused (res aliases out32), res_T = 0 / T                                      (vit_backward_impl)
      bwd_pre        ln_pre backward alone, f32 dy, PATCH_ROWS output                                               (vit_backward_impl)
    M = S T rows (15 by default: not a multiple of the 4 rows of a workgroup); 16 guard rows behind every output.  Rows a launch must not
    read (class rows of x0 before ln_pre, rows between the class rows of an xs = T launch, residual rows outside res_T) hold NaN."""
    gen = torch.Generator().manual_seed(seed)
    M, G = S * T, GUARD_ROWS
    hilo = case.endswith('_hilo')
    W = 2 * D if hilo else D
    dv = lambda t: None if t is None else t.clone().to(dev)      # noqa: E731  (a copy: .to() of a CPU tensor aliases it)
    what = 'LayerNorm %s D=%d S=%d T=%d' % (case, D, S, T)
    cls_rows = torch.arange(M) % T == 0
    patch_rows = torch.arange(M)[~cls_rows]          # in the order of the PATCH_ROWS layout
    MP = S * (T - 1)

    if case.startswith('pre'):
        x, gam, bet = _ln_inputs(gen, M + G, D)
        x[:M][cls_rows] = float('nan')          # class rows of x0 before ln_pre: never read (the patch-embedding GEMM does not write them)
        cls, pos = torch.randn(D, generator=gen), torch.randn(T, D, generator=gen)
        fused = case != 'pre'
        g2, b2 = (1.0 + 0.3 * torch.randn(D, generator=gen), 0.2 * torch.randn(D, generator=gen)) if fused else (None, None)
        ins = dict(g=gam, b=bet, cls=cls, pos=pos, g2=g2, b2=b2)

        def run():
            xd = x.clone().to(dev)
            out = sentinel(M + G, D, torch.float32, dev)
            out2 = sentinel(M + G, W, torch.float16, dev) if fused else None
            dd = {k: dv(v) for k, v in ins.items()}
            ln_call(lib, 0, D, M, T, flags=int(hilo), x=xd, g=dd['g'], b=dd['b'], out=out, out2=out2, cls=dd['cls'], pos=dd['pos'], x_fill=xd,
                    g2=dd['g2'], b2=dd['b2'])
            _unchanged(dd, ins, what)
            return xd.cpu(), out.cpu(), (None if out2 is None else out2.cpu())
        xf, out, out2 = _twice(run, what)
        fill = (cls + pos[0]).expand(int(cls_rows.sum()), D)
        assert torch.equal(bits(xf[:M][cls_rows]), bits(fill)), what + ': class rows of x_fill != cls + pos[0]'
        keep = torch.ones(M + G, dtype=torch.bool)
        keep[:M][cls_rows] = False
        assert torch.equal(bits(xf[keep]), bits(x[keep])), what + ': x_fill written outside the class rows'
        xin = x[:M].clone()
        xin[cls_rows] = fill
        y, e = ln_fwd_ref(xin, gam, bet)
        assert_within(out[:M], y, e, what + ' (fp32 out)')
        assert_untouched(out, _window(M + G, D, slice(0, M)), what + ' (fp32 out)')
        if fused:
            # the second LayerNorm reads the first one's fp32 rows from registers: the kernel's own out is its exact input
            y2, e2 = ln_fwd_ref(out[:M], g2, b2)
            if hilo:
                _check_hilo(out2[:M], y2, e2, D, what + ' (fused ln_1)')
            else:
                assert_f16(out2[:M], y2, e2, what + ' (fused ln_1)')
            assert_untouched(out2, _window(M + G, W, slice(0, M)), what + ' (fused ln_1)')
        return

    if case.startswith('ln_f16'):
        xs = T if case == 'ln_f16_cls' else 1
        Mr = S if xs > 1 else M
        x, gam, bet = _ln_inputs(gen, M + G, D)
        if xs > 1:
            x[torch.arange(M + G) % T != 0] = float('nan')        # the rows the class-row launch must not read
        ins = dict(x=x, g=gam, b=bet)

        def run():
            dd = {k: dv(v) for k, v in ins.items()}
            out = sentinel(Mr + G, W, torch.float16, dev)
            ln_call(lib, 1, D, Mr, T, xs=xs, flags=int(hilo), x=dd['x'], g=dd['g'], b=dd['b'], out=out)
            _unchanged(dd, ins, what)
            return (out.cpu(),)
        out, = _twice(run, what)
        y, e = ln_fwd_ref(x[torch.arange(Mr) * xs], gam, bet)
        if hilo:
            _check_hilo(out[:Mr], y, e, D, what)
        else:
            assert_f16(out[:Mr], y, e, what)
        assert_untouched(out, _window(Mr + G, W, slice(0, Mr)), what)
        return

    x, gam, _ = _ln_inputs(gen, M + G, D)
    if case == 'bwd_pre':
        dy = torch.randn(M, D, generator=gen) * 0.5
        ins = dict(dy=dy, x=x, g=gam)

        def run():
            dd = {k: dv(v) for k, v in ins.items()}
            o16 = sentinel(MP + G, D, torch.float16, dev)
            ln_call(lib, 3, D, M, T, x=dd['x'], g=dd['g'], dy=dd['dy'], out2=o16)
            _unchanged(dd, ins, what)
            return (o16.cpu(),)
        o16, = _twice(run, what)
        dx, e, _ = ln_bwd_ref(dy[patch_rows], x[patch_rows], gam)
        assert_f16(o16[:MP], dx, e, what)
        assert_untouched(o16, _window(MP + G, D, slice(0, MP)), what)
        return

    # mode 2: the f16-dy backward
    assert case in ('bwd_ln2', 'bwd_ln2_cls', 'bwd_ln2_f16', 'bwd_ln1', 'bwd_ln1_res_T', 'bwd_ln1_fused'), case
    xs = T if case in ('bwd_ln2_cls', 'bwd_ln2_f16') else 1
    Mr = S if xs > 1 else M
    res_T = T if case in ('bwd_ln1_res_T', 'bwd_ln1_fused') else 0
    res_f16 = case == 'bwd_ln2_f16'
    fused = case == 'bwd_ln1_fused'
    dy = (torch.randn(Mr, D, generator=gen) * 0.5).half()
    rows = torch.arange(Mr) * xs                               # the rows of x / res / outputs the launch owns
    other = torch.ones(M + G, dtype=torch.bool)
    other[rows] = False
    if xs > 1:
        x[other] = float('nan')
    res = torch.randn(M + G, D, generator=gen) * 2.0
    has_res = torch.ones(M + G, dtype=torch.bool) if res_T == 0 else (torch.arange(M + G) % res_T == 0)
    res[~has_res] = float('nan')                               # rows without a residual: reading one poisons the row
    if xs > 1:
        res[other] = float('nan')
    if res_f16:
        res = res.half()
    xb, gb = (_ln_inputs(gen, M + G, D)[:2]) if fused else (None, None)
    ins = dict(dy=dy, x=x, g=gam, xb=xb, gb=gb)

    def run():
        dd = {k: dv(v) for k, v in ins.items()}
        if fused:
            rd = dv(res)
            o32, o16 = None, sentinel(MP + G, D, torch.float16, dev)
        elif res_f16:                                          # res aliases out16 (the f16-only gradient stream)
            o32 = None
            o16 = rd = dv(res)
        else:                                                  # res aliases out32 (res2 = dx)
            o32 = rd = dv(res)
            o16 = sentinel(M + G, D, torch.float16, dev)
        ln_call(lib, 2, D, Mr, T, xs=xs, res_T=res_T, flags=2 if res_f16 else 0, x=dd['x'], g=dd['g'], dy=dd['dy'], res=rd, out=o32, out2=o16,
                x2=dd['xb'], g2=dd['gb'])
        _unchanged(dd, ins, what)
        if fused:
            assert torch.equal(bits(rd), bits(res)), what + ': input res changed'
        return (None if o32 is None else o32.cpu()), o16.cpu()
    o32, o16 = _twice(run, what)
    dx, e, _ = ln_bwd_ref(dy, x[rows], gam)
    r = torch.where(has_res[rows][:, None], res[rows].double(), torch.zeros(1, dtype=torch.float64))
    want = dx + r
    e = e + 2 * U * r.abs()
    if fused:
        # the first gradient (fp32, in registers) is the dy of ln_pre's backward on the patch rows
        dxb, eb, gain = ln_bwd_ref(want[patch_rows], xb[patch_rows], gb)
        eb = eb + gain * (e[patch_rows] + U * want[patch_rows].abs()).max(1, keepdim=True).values
        assert_f16(o16[:MP], dxb, eb, what + ' (ln_pre gradient, patch rows)')
        assert_untouched(o16, _window(MP + G, D, slice(0, MP)), what)
        return
    assert_f16(o16[rows], want, e, what + ' (f16)')
    if res_f16:
        # rows outside the launch keep their values: res is the output buffer itself
        assert torch.equal(bits(o16[other]), bits(res[other])), what + ': rows outside the launch changed'
        return
    assert_within(o32[rows], want, e, what + ' (fp32 stream)')
    assert torch.equal(bits(o32[other]), bits(res[other])), what + ': fp32 stream changed outside the launch rows'
    assert_untouched(o16, _window(M + G, D, rows), what + ' (f16)')


# ------------------------------------------------------------------------------------------------------------------------- attention
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
KSL = 0.125 * LOG2E              # kSL of vit_attn.h
ATTN_KINDS = ('normal', 'flat', 'peaked', 'negative', 'loss_scaled', 'scaled_dO')
ATTN_CHUNK = 6000000             # elements of one [items, T, T] fp64 temporary of the reference


def attn_inputs(kind, S, T, heads, seed=0):
    """qkv [S T, 3 D], datt [S T, D] f16 of one input family (D = 64 heads):
      normal       randn * 1.5, datt = randn (check_attention's)
      flat         q, k * 0.05: P about 1 / T, many probabilities with equal exponents
      peaked       q, k = randn * 6 (the normal family's times 4): near one-hot rows, max_j P > 0.99 on 0.7 - 0.8 of them
      negative     q = u + 0.1 n, k = -u + 0.1 n with one u = 1.25 randn(64) per head: every score negative, lse < 0 -- a padded key (score 0)
                   would be the row maximum if the forward's mask were wrong, and at_p's clamp at 0 is what keeps the backward's p finite there
                   (1.25: with twelve heads the smallest |u|^2 still leaves lse < 0 at T = 256, where log T = 5.5)
      loss_scaled  the negative q / k, v_j = c + 0.05 n with c = +-16 per feature, dO_i = 40 c: |D_i| / 8 = 40 * 64 * 256 / 8 = 8.2e4 is past the
                   f16 range while every valid dS and the gradient (~1e3) are far inside it
      scaled_dO    normal with datt * 3000 (gradients ~1e4, still inside f16)"""
    assert kind in ATTN_KINDS, kind
    g = torch.Generator().manual_seed(seed)
    D, M = heads * 64, S * T
    qkv = torch.randn(M, 3 * D, generator=g) * 1.5
    datt = torch.randn(M, D, generator=g)
    if kind == 'flat':
        qkv[:, :2 * D] *= 0.05
    elif kind == 'peaked':
        qkv[:, :2 * D] *= 4.0
    elif kind == 'scaled_dO':
        datt *= 3000.0
    elif kind in ('negative', 'loss_scaled'):
        u = 1.25 * torch.randn(1, D, generator=g)
        qkv[:, :D] = u + 0.1 * torch.randn(M, D, generator=g)
        qkv[:, D:2 * D] = -u + 0.1 * torch.randn(M, D, generator=g)
        if kind == 'loss_scaled':
            c = 16.0 * (torch.randint(0, 2, (1, D), generator=g) * 2 - 1).float()
            qkv[:, 2 * D:] = c + 0.05 * torch.randn(M, D, generator=g)
            datt = (40.0 * c).expand(M, D).contiguous()
    return qkv.half(), datt.half()


def attn_items(x, S, T, heads, parts=1):
    """[S T, parts * heads * 64] rows -> `parts` fp64 tensors [S heads, T, 64], one (cut, head) item per leading index"""
    x = x.double().reshape(S, T, parts, heads, 64)
    return [x[:, :, i].permute(0, 2, 1, 3).reshape(S * heads, T, 64) for i in range(parts)]


def attn_rows(x, S, T, heads):
    """[S heads, T, 64] -> [S T, heads * 64]"""
    return x.reshape(S, heads, T, 64).permute(0, 2, 1, 3).reshape(S * T, heads * 64)


def attn_fwd_ref(q, k, v):
    """fp64 attention of a chunk of items [n, T, 64] on the RAW scores s = q . k (the kernels scale by 1/8 inside the exponent):
    e_s = 1e-6 |q| . |k| (the project's accumulator figure, check_gemm_epilogue), mx = max_j s, l = sum_j exp((s - mx) / 8), P, O = P v, lse"""
    s = q @ k.mT
    e_s = 1e-6 * (q.abs() @ k.abs().mT)
    mx = s.amax(-1, keepdim=True)
    pu = torch.exp((s - mx) / 8)
    l = pu.sum(-1, keepdim=True)
    P = pu / l
    return dict(s=s, e_s=e_s, mx=mx, e_mx=e_s.amax(-1, keepdim=True), l=l, P=P, O=P @ v, lse=mx / 8 + torch.log(l))


def attn_bwd_ref(s, L, q, k, v, dO, clamp):
    """fp64 attention backward from the saved log-sum-exp L [n, T, 1], as the kernels form it: Pb = exp(s / 8 - L) (clamp: min(., 1), at_p),
    dp = dO . v, D_i = sum_j Pb dp, dS = Pb / 8 (dp - D), dQ = dS k, dK = dS^T q, dV = Pb^T dO"""
    Pb = torch.exp(s / 8 - L)
    if clamp:
        Pb = Pb.clamp(max=1.0)
    dp = dO @ v.mT
    Dv = (Pb * dp).sum(-1, keepdim=True)
    dS = Pb / 8 * (dp - Dv)
    return dict(Pb=Pb, dp=dp, e_dp=1e-6 * (dO.abs() @ v.abs().mT), D=Dv, dS=dS, dQ=dS @ k, dK=dS.mT @ q, dV=Pb.mT @ dO)


class AttnStats:
    """what the families' preconditions need from the fp64 reference, gathered chunk by chunk"""

    def __init__(self):
        self.rows = self.peaked_rows = 0
        self.pmax_T = self.lse_max = self.s_max = self.D8_max = self.dS_max = self.out_max = float('-inf')

    def forward(self, r, T):
        pm = r['P'].amax(-1)
        self.rows += pm.numel()
        self.peaked_rows += int((pm > 0.99).sum())
        self.pmax_T = max(self.pmax_T, pm.max().item() * T)
        self.lse_max = max(self.lse_max, r['lse'].max().item())
        self.s_max = max(self.s_max, r['s'].max().item())
        self.out_max = max(self.out_max, r['O'].abs().max().item())

    def backward(self, b):
        self.D8_max = max(self.D8_max, b['D'].abs().max().item() / 8)
        self.dS_max = max(self.dS_max, b['dS'].abs().max().item())
        self.out_max = max(self.out_max, *(b[n].abs().max().item() for n in ('dQ', 'dK', 'dV')))

    def check_forward(self, kind, what):
        if kind == 'flat':
            assert self.pmax_T < 1.5, '%s: not flat (max P T = %.3g)' % (what, self.pmax_T)
        if kind == 'peaked':
            assert 2 * self.peaked_rows >= self.rows, '%s: only %d of %d rows have max P > 0.99' % (what, self.peaked_rows, self.rows)
        if kind in ('negative', 'loss_scaled'):
            assert self.lse_max < 0 and self.s_max < 0, '%s: max lse %.3g, max score %.3g are not negative' % (what, self.lse_max, self.s_max)

    def check_backward(self, kind, what):
        if kind == 'loss_scaled':
            assert self.D8_max > F16_INF_AT, '%s: max |D_i| / 8 = %.4g is inside the f16 range' % (what, self.D8_max)
            assert self.dS_max < 65504 and self.out_max < 65504, '%s: max |dS| %.4g, max |output| %.4g' % (what, self.dS_max, self.out_max)
        if kind == 'scaled_dO':
            assert 1e3 < self.out_max < 65504, '%s: max |gradient| %.4g' % (what, self.out_max)


def attn_call(lib, qkv, att, lse, datt, dqkv, S, T, heads, mode):
    ops._L(lib, qkv).call('aph_attn_test', ops.ptr(qkv), ops.ptr(att), ops.ptr(lse), ops.ptr(datt), None, ops.ptr(dqkv), S, T, heads, mode,
                          ops._stream(qkv))


def ratio_within(got, ref, bound):
    """worst |got - ref| / bound (inf where got is not finite)"""
    if not got.numel():
        return 0.0
    return ((got.double() - ref).abs() / bound).nan_to_num(float('inf')).max().item()


def ratio_f16(got, ref, e):
    """worst err / (e + 2^-11 |ref| + 2^-25) over the elements assert_f16 bounds (those that cannot round to infinity)"""
    e = e.expand_as(ref)
    fin = ref.abs() + e < F16_INF_AT
    return ratio_within(got[fin], ref[fin], (e + H * ref.abs() + H_SUB)[fin])


class Findings:
    """runs every assertion of a check, keeps the worst err / bound per output, and fails at the end with all of them in the message"""

    def __init__(self, what):
        self.what, self.ratio, self.failed = what, {}, []

    def run(self, f, *a):
        try:
            f(*a)
        except AssertionError as e:
            self.failed.append(str(e))

    def f16(self, name, got, ref, e):
        self.ratio[name] = max(self.ratio.get(name, 0.0), ratio_f16(got, ref, e))
        self.run(assert_f16, got, ref, e, '%s (%s)' % (self.what, name))

    def within(self, name, got, ref, bound):
        self.ratio[name] = max(self.ratio.get(name, 0.0), ratio_within(got, ref, bound))
        self.run(assert_within, got, ref, bound, '%s (%s)' % (self.what, name))

    def check(self, ok, msg):
        if not ok:
            self.failed.append(msg)

    def finish(self):
        assert not self.failed, '%s: worst err / bound %s\n%s' % (self.what, ' '.join('%s %.3g' % kv for kv in self.ratio.items()), '\n'.join(self.failed))
        return self.ratio


def attn_fwd_bound_f16(r, v, T):
    """(e_att, e_lse) of at_fwd_tiles / attn_fwd_mfma_g_kernel; docstring of check_attention_fp64"""
    e_x = KSL * (r['e_s'] + r['e_mx']) + 3 * U * KSL * (r['s'].abs() + r['mx'].abs())
    eps_p = LN2 * e_x + 2 * U
    eps_l = (r['P'] * eps_p).sum(-1, keepdim=True) + T * U
    av = v.abs()
    e_att = (r['P'] * (eps_p + H)) @ av + (H_SUB / r['l']) * av.sum(-2, keepdim=True) + (eps_l + (3 + T) * U) * (r['P'] @ av)
    e_lse = r['e_mx'] / 8 + eps_l + 4 * U * (r['mx'].abs() / 8 + torch.log(r['l'])) + 2 * U
    return e_att, e_lse


def attn_bwd_bound_f16(r, b, L, q, k, dO, T, O16=None, eps_extra=None, eD_extra=None):
    """(e_dQ, e_dK, e_dV) of attn_bwd_mfma_kernel (T <= 64) / attn_bwd_one_g_kernel (O16 = the f16 att rows it reads); eps_extra, eD_extra:
    what a kernel-made lse / att adds (the chained run); docstring of check_attention_fp64"""
    e_xb = KSL * r['e_s'] + 4 * U * (r['s'].abs() * KSL + L.abs() * LOG2E)
    eps_pb = LN2 * e_xb + 2 * U
    if eps_extra is not None:
        eps_pb = eps_pb + eps_extra
    Pb, dp, dS = b['Pb'], b['dp'], b['dS']
    if O16 is None:
        e_D = (Pb * (eps_pb * dp.abs() + b['e_dp'])).sum(-1, keepdim=True) + T * U * (Pb * dp.abs()).sum(-1, keepdim=True)
    else:
        e_D = ((O16 * dO).sum(-1, keepdim=True) - b['D']).abs() + 64 * U * (O16 * dO).abs().sum(-1, keepdim=True)
    if eD_extra is not None:
        e_D = e_D + eD_extra
    e_dS = dS.abs() * (eps_pb + 3 * U) + Pb / 8 * (b['e_dp'] + e_D) + H * dS.abs() + H_SUB
    e_dQ = e_dS @ k.abs() + 1e-6 * (dS.abs() @ k.abs())
    e_dK = e_dS.mT @ q.abs() + 1e-6 * (dS.abs().mT @ q.abs())
    e_dV = (Pb * (eps_pb + H) + H_SUB).mT @ dO.abs() + 1e-6 * (Pb.mT @ dO.abs())
    return e_dQ, e_dK, e_dV


def check_attention_fp64(lib, dev, S, T, heads, kind='normal', seed=0):
    """The f16 attention kernels of vit_attn.h through aph_attn_test against fp64 on the f16-rounded inputs, element by element, per (cut, head):
    the forward, the backward ALONE (fed att = f16(O_ref) and lse = f32(lse_ref), so that no forward error can cancel one of its own) and one
    chained run (kernel forward -> kernel backward).  Outputs start as sentinels with GUARD_ROWS rows / floats behind them that must keep
    them; inputs stay bit for bit; a second identical call gives the same bits.  At T <= 64 the backward's att input is all NaN: the
    one-tile kernel must not read it.  Returns the worst err / bound per output ('dq+' ...: the chained run).

    Notation: s = q . k raw, mx = max_j s, l = sum_j exp((s - mx) / 8), P = softmax(s / 8), U = 2^-24, H = 2^-11, H_SUB = 2^-25,
    kSL = 0.125 log2 e, e_s = 1e-6 |q| . |k| (an fp32 MFMA accumulator, the figure of check_gemm_epilogue).

    Forward (at_fwd_tiles, attn_fwd_mfma_g_kernel: the same arithmetic per score).
      e_x   = kSL (e_s + max_j e_s) + 3 U kSL (|s| + |mx|)    the exponent fma(s, kSL, -mxs), mxs = mx * kSL: s and the maximum (a computed
              score) carry their accumulator error; kSL is a rounded constant in both products, mxs is rounded once, the fma once
      eps_p = ln2 e_x + 2 U                                   relative error of p = 2^x; v_exp_f32 is 1 ulp (libm's exp2f in the interpreter is less)
      eps_l = sum_j P eps_p + T U                             l is summed from the fp32 p: at most T - 1 inexact additions (lane-local, two shuffles)
      e_att = (P (eps_p + H)) @ |v|                           each p, then its conversion to f16 in pack8 (unnormalised: p <= 1, relative H) ...
            + (H_SUB / l) sum_j |v_j|                         ... or absolute H_SUB where p is subnormal in f16, scaled by 1 / l like every term
            + (eps_l + (3 + T) U) (P @ |v|)                   l itself; 1.0f / l, its shuffle-free product with o (2 U, one to spare) and the T
                                                              accumulator additions of the two (2 NB) MFMAs at their worst case
      e_lse = max_j e_s / 8 + eps_l + 4 U (|mx| / 8 + log l) + 2 U     mx * 0.125f is exact; __logf(l) = v_log_f32(l) * ln2: 1 ulp, a rounded
              constant and a product (3 U log l, and an absolute 2 U where log l is near 0), the sum one rounding of |lse| <= |mx| / 8 + log l
    Backward, alone.  L = the lse it is fed, Pb = min(exp(s / 8 - L), 1) (at_p), dp = dO . v, e_dp = 1e-6 |dO| . |v|.
      e_xb  = kSL e_s + 4 U (|s| kSL + |L| log2 e)            fma(s, kSL, -L2), L2 = L * kLog2e: two rounded constants, the product L2, the fma
      eps_pb = ln2 e_xb + 2 U
      T <= 64 (attn_bwd_mfma_kernel: D_i = sum_j p dp in fp32, 16 per lane + two shuffles):
        e_D = sum_j Pb (eps_pb |dp| + e_dp) + T U sum_j Pb |dp|
      T > 64 (attn_bwd_one_g_kernel: D_i = dO_i . att_i from the f16 att rows, 16 products per thread + two shuffles):
        e_D = |sum_d f16(O) dO - sum_j Pb dp| + 64 U sum_d |f16(O) dO|        the first term is the kernel's method, not its rounding: att has
              been rounded to f16 before the kernel sees it.  Under loss_scaled (|O| ~ 16, |dO| = 640) it is as large as dp - D itself:
              the bound on dq / dk is then wide, and that width is the blocked kernel's real precision in that regime
      dS = Pb / 8 (dp - D) (at_ds):  e_dS = |dS| (eps_pb + 3 U) + Pb / 8 (e_dp + e_D) + H |dS| + H_SUB      p, three fp32 roundings, the
              two inputs of the difference, the f16 fragment (pack8; the dS^T image of the blocked kernel holds the same f16 values).
              at_ds clamps at +-65504: no valid dS of these inputs is that large (asserted for loss_scaled), so the clamp acts on padded
              keys / queries only, whose operand rows are zero
      e_dQ  = e_dS @ |k| + 1e-6 (|dS| @ |k|)      e_dK likewise over the queries with |q|
      e_dV  = (Pb (eps_pb + H) + H_SUB)^T @ |dO| + 1e-6 (Pb^T @ |dO|)                                     p as an f16 fragment, as in the forward
    Chained: the same with what the forward may hand over: eps_pb += e_lse (an error of L is a relative error of p), and at T > 64
      e_D += |dO| . (e_att + H |O| + H_SUB) (the kernel's att rows against O).

    T = 1 is exempt from any lower limit on the ratios (P = 1, dq = dk = 0)."""
    D, M, NL, G = heads * 64, S * T, S * heads * T, GUARD_ROWS
    what = 'attention %s S=%d T=%d heads=%d' % (kind, S, T, heads)
    qkv, datt = attn_inputs(kind, S, T, heads, seed)
    q, k, v = attn_items(qkv, S, T, heads, 3)
    dO, = attn_items(datt, S, T, heads)
    n_items = S * heads
    step = max(1, ATTN_CHUNK // (T * T))
    chunks = [slice(a, min(a + step, n_items)) for a in range(0, n_items, step)]

    # ---- the forward reference (O and lse are the inputs of the backward alone)
    st = AttnStats()
    O, e_att = torch.empty_like(q), torch.empty_like(q)
    lse, e_lse = torch.empty(n_items, T, 1, dtype=torch.float64), torch.empty(n_items, T, 1, dtype=torch.float64)
    for c in chunks:
        r = attn_fwd_ref(q[c], k[c], v[c])
        st.forward(r, T)
        O[c], lse[c] = r['O'], r['lse']
        e_att[c], e_lse[c] = attn_fwd_bound_f16(r, v[c], T)
    st.check_forward(kind, what)
    O_rows = attn_rows(O, S, T, heads)

    # ---- the kernels
    ins = dict(qkv=qkv, datt=datt)
    dd = {n: t.clone().to(dev) for n, t in ins.items()}      # (a copy: .to() of a CPU tensor aliases it)
    held = {}

    def fwd():
        att, ls = sentinel(M + G, D, torch.float16, dev), sentinel(1, NL + G, torch.float32, dev)
        attn_call(lib, dd['qkv'], att, ls, None, None, S, T, heads, 0)
        held['att'], held['lse'] = att, ls
        return att.cpu(), ls.cpu()

    att_in = sentinel(M + G, D, torch.float16, 'cpu')
    if T > 64:
        att_in[:M] = O_rows.half()
    lse_in = sentinel(1, NL + G, torch.float32, 'cpu')
    lse_in[0, :NL] = lse.reshape(-1).float()

    def bwd(a, ls):
        a0, l0 = bits(a).clone(), bits(ls).clone()
        dq = sentinel(M + G, 3 * D, torch.float16, dev)
        attn_call(lib, dd['qkv'], a, ls, dd['datt'], dq, S, T, heads, 1)
        assert torch.equal(bits(a), a0) and torch.equal(bits(ls), l0), what + ': the backward changed att / lse'
        return (dq.cpu(),)
    att, ls = _twice(fwd, what + ' forward')
    g_alone, = _twice(lambda: bwd(att_in.clone().to(dev), lse_in.clone().to(dev)), what + ' backward')
    g_chain, = bwd(held['att'], held['lse'])
    _unchanged(dd, ins, what)

    # ---- forward
    fd = Findings(what)
    fd.f16('att', att[:M], O_rows, attn_rows(e_att, S, T, heads))
    fd.within('lse', ls[0, :NL], lse.reshape(-1), e_lse.reshape(-1))
    fd.run(assert_untouched, att, _window(M + G, D, slice(0, M)), what + ' (att)')
    fd.run(assert_untouched, ls, _window(1, NL + G, (0, slice(0, NL))), what + ' (lse)')
    # ---- backward, chunk by chunk
    L_in = lse_in[0, :NL].double().reshape(n_items, T, 1)
    O16 = attn_items(att_in[:M], S, T, heads)[0] if T > 64 else None
    got = {'': attn_items(g_alone[:M], S, T, heads, 3), '+': attn_items(g_chain[:M], S, T, heads, 3)}
    for c in chunks:
        r = attn_fwd_ref(q[c], k[c], v[c])
        for tag in ('', '+'):
            L = L_in[c] if tag == '' else r['lse']
            b = attn_bwd_ref(r['s'], L, q[c], k[c], v[c], dO[c], clamp=True)
            if tag == '':
                st.backward(b)
                e = attn_bwd_bound_f16(r, b, L, q[c], k[c], dO[c], T, None if O16 is None else O16[c])
            else:
                eD = (dO[c].abs() * (e_att[c] + H * O[c].abs() + H_SUB)).sum(-1, keepdim=True) if T > 64 else None
                e = attn_bwd_bound_f16(r, b, L, q[c], k[c], dO[c], T, None if O16 is None else O16[c], eps_extra=e_lse[c], eD_extra=eD)
            for i, n in enumerate(('dQ', 'dK', 'dV')):
                fd.f16(n.lower() + tag, got[tag][i][c], b[n], e[i])
    st.check_backward(kind, what)
    for tag, gq in (('', g_alone), ('+', g_chain)):
        fd.run(assert_untouched, gq, _window(M + G, 3 * D, slice(0, M)), what + ' (dqkv%s)' % tag)
        if kind == 'loss_scaled':
            nf = int((~torch.isfinite(gq[:M].float())).sum())
            fd.check(nf == 0, '%s: %d NaN / inf in dqkv%s' % (what, nf, tag))
    return fd.finish()
