"""Checks of the exact (fp32) ViT path, shared by the interpreter tests (test_emu_exact.py) and the GPU tests (test_gpu_exact.py).
`lib` = a loaded C-ABI library (the interpreter build or the product), `dev` = where its tensors live."""
import ctypes

import numpy as np
import torch

from aphantasia_amd import _ffi, ops
from aphantasia_amd.weights import synthetic_visual_weights
from oracle import clip_vit_ref
import vit_component_checks as V

TINY = dict(input_resolution=32, patch_size=16, width=256, layers=2, heads=4, output_dim=128)


def gemm_f32(lib, dev, A, Bt, M, N, K, lda=None, ldb=None, a_rowP=0, bias=None, aux=None, epi=0, ldc=None, ws_floats=0):
    """aph_gemm_f32_test on device copies; returns (C, aux)"""
    lda, ldb, ldc = lda or K, ldb or K, ldc or N
    A, Bt = A.to(dev).contiguous(), Bt.to(dev).contiguous()
    C = torch.full((M, ldc), float('nan'), dtype=torch.float32, device=dev) if epi != 4 else aux.clone().to(dev)
    aux_d = None if aux is None else aux.clone().to(dev).contiguous()
    if epi == 2:
        aux_d = torch.full((M, ldc), float('nan'), dtype=torch.float32, device=dev)
    if epi == 4:
        aux_d = C
    b = None if bias is None else bias.to(dev).contiguous()
    ws = torch.empty(max(ws_floats, 1), dtype=torch.float32, device=dev) if ws_floats else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if A.is_cuda else ctypes.c_void_p(0)
    lib.call('aph_gemm_f32_test', ops.ptr(A), lda, a_rowP, ops.ptr(Bt), ldb, M, N, K, ops.ptr(C), ldc, ops.ptr(b), ops.ptr(aux_d), epi,
             ops.ptr(ws), ws_floats, st)
    return C.cpu(), (None if aux_d is None else aux_d.cpu())


def check_gemm_f32(lib, dev, M, N, K, lda=None, a_rowP=0, epi=0, ws_floats=0, seed=0):
    """every element within 1e-6 * sum_k |a b| of the fp64 product (and the epilogue's fp64 value)"""
    g = torch.Generator().manual_seed(seed)
    lda = lda or K
    rows = M + (M - 1) // a_rowP + 1 if a_rowP else M
    A = torch.randn(rows, lda, generator=g) * 3.0
    Bt = torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    aux = torch.randn(M, N, generator=g) if epi in (3, 4) else None
    C, aux_out = gemm_f32(lib, dev, A, Bt, M, N, K, lda=lda, a_rowP=a_rowP, bias=bias, aux=aux, epi=epi, ws_floats=ws_floats)
    idx = torch.arange(M)
    if a_rowP:
        idx = idx + idx // a_rowP + 1
    Am = A[idx, :K].double()
    acc = Am @ Bt.double().t()
    mag = Am.abs() @ Bt.double().abs().t()
    tol = 1e-6 * mag + 1e-30
    if epi == 0:
        err = (C.double() - acc).abs()
        assert (err <= tol).all(), (M, N, K, (err / tol).max().item())
    elif epi == 1:
        assert ((C.double() - (acc + bias.double())).abs() <= tol + 1e-6 * bias.double().abs()).all()
    elif epi == 2:
        u = acc + bias.double()
        s = torch.sigmoid(1.702 * u)
        gv, dg = u * s, s * (1 + 1.702 * u * (1 - s))
        # the GELU of an input that is accurate to tol: accurate to |dg| tol + a few ulp of the result
        assert ((C.double() - gv).abs() <= dg.abs() * (tol + 1e-6 * bias.double().abs()) + 4e-7 * gv.abs() + 1e-30).all()
        # dg/du: |d dg / du| < 4 times the input error, plus the roundings of s + 1.702 (g - g s)
        assert ((aux_out.double() - dg).abs() <= 4 * (tol + 1e-6 * bias.double().abs()) + 4e-7 * (s + 3.404 * gv.abs()) + 1e-7).all()
    elif epi == 3:
        assert ((C.double() - acc * aux.double()).abs() <= tol * aux.double().abs() + 1e-7 * (acc * aux.double()).abs()).all()
    else:
        want = aux.double() + acc + bias.double()
        assert ((C.double() - want).abs() <= tol + 1e-6 * (aux.double().abs() + bias.double().abs())).all()


def oracle64(cfg, S, seed_w=3, seed_x=1, scale_w=None):
    """fp64 oracle: weights, input, encodings and the input gradient of sum(enc * genc)"""
    w = synthetic_visual_weights(cfg, seed_w)
    if scale_w is not None:
        w = scale_w(w)
    R = cfg['input_resolution']
    x = torch.randn(S, 3, R, R, generator=torch.Generator().manual_seed(seed_x))
    xd = x.double().requires_grad_(True)
    wd = {k: v.double() for k, v in w.items()}
    enc = clip_vit_ref.encode_image(wd, xd, cfg)
    genc = torch.randn(S, cfg['output_dim'], generator=torch.Generator().manual_seed(2)).double() * 0.01
    (enc * genc).sum().backward()
    return w, x, enc.detach(), genc, xd.grad.detach()


def check_vit_exact(lib, dev, cfg=TINY, S=3, fwd_tol=1e-5, bwd_tol=1e-4, scale_w=None):
    """forward <= fwd_tol * max|enc|, input gradient <= bwd_tol * max|g| against the fp64 oracle; returns the two relative errors"""
    w, x, want, genc, gx_want = oracle64(cfg, S, scale_w=scale_w)
    p = cfg['patch_size']
    vit = ops.VitHandle(cfg, w, max_batch=S + 1, lib=lib)
    vit.enable_f32()
    patches = ops.patchify(x.to(dev).contiguous(), p, lib=lib, f32=True)
    assert patches.dtype == torch.float32
    enc = vit.forward(patches, S, f32=True)
    ferr = (enc.cpu().double() - want).abs().max().item() / want.abs().max().item()
    LS = 4096.0
    gp = vit.backward((genc.float() * LS).to(dev).contiguous(), S, out_scale=1.0 / LS, f32=True)
    gx = ops.unpatchify(gp, S, cfg['input_resolution'], p, lib=lib)
    berr = (gx.cpu().double() - gx_want).abs().max().item() / gx_want.abs().max().item()
    assert ferr <= fwd_tol and berr <= bwd_tol, (ferr, berr)
    return ferr, berr


def check_enable_f32_refusals(lib, dev):
    """forward_f32 before enable, backward_f32 after a non-f32 forward and backward after an f32 forward are refused with messages that name
    the call to make; enable is idempotent, counted by aph_vit_workspace_bytes, and a later weight reload refreshes the fp32 copies"""
    cfg = TINY
    w = synthetic_visual_weights(cfg, 3)
    S, p, R = 2, cfg['patch_size'], cfg['input_resolution']
    vit = ops.VitHandle(cfg, w, max_batch=S, lib=lib)
    base = vit.workspace_bytes()
    x = torch.randn(S, 3, R, R, generator=torch.Generator().manual_seed(1)).to(dev)
    p32 = ops.patchify(x, p, lib=lib, f32=True)
    out = torch.empty(S, cfg['output_dim'], device=dev)
    grad = torch.empty(p32.shape, device=dev)
    genc = torch.randn(S, cfg['output_dim'], generator=torch.Generator().manual_seed(2)).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if x.is_cuda else None
    rc = lib.cdll.aph_vit_forward_f32(vit.handle, ops.ptr(p32), S, ops.ptr(out), st)
    assert rc < 0 and 'aph_vit_enable_f32' in lib.last_error()
    vit.enable_f32()
    vit.enable_f32()
    assert vit.workspace_bytes() > base
    b1 = vit.workspace_bytes()
    vit.enable_f32()
    assert vit.workspace_bytes() == b1
    # backward_f32 after the f16 forward
    vit.forward(ops.patchify(x, p, lib=lib), S)
    rc = lib.cdll.aph_vit_backward_f32(vit.handle, ops.ptr(genc), S, ops.ptr(grad), ctypes.c_float(1.0), st)
    assert rc < 0 and 'aph_vit_forward_f32' in lib.last_error()
    # the f16 backward after the f32 forward
    enc = vit.forward(p32, S, f32=True).clone()
    rc = lib.cdll.aph_vit_backward(vit.handle, ops.ptr(genc), S, ops.ptr(grad), ctypes.c_float(1.0), st)
    assert rc < 0 and 'aph_vit_backward_f32' in lib.last_error()
    g1 = vit.backward(genc, S, f32=True).clone()
    # weight reload after enabling: the fp32 copies follow (fc2 scaled by 0.5 on every layer changes the exact forward like the oracle's)
    w2 = dict(w)
    for li in range(cfg['layers']):
        k = 'transformer.resblocks.%d.mlp.c_proj.weight' % li
        w2[k] = w[k] * 0.5
        a = np.ascontiguousarray(w2[k].numpy())
        lib.call('aph_vit_set_weight', vit.handle, k.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size)
    enc2 = vit.forward(p32, S, f32=True).clone()
    want2 = clip_vit_ref.encode_image({k: v.double() for k, v in w2.items()}, x.cpu().double(), cfg)
    assert not torch.equal(enc2, enc)
    assert (enc2.cpu().double() - want2).abs().max().item() <= 1e-5 * want2.abs().max().item()
    return g1


def to_patch_major(x, p):
    S, C, R, _ = x.shape
    g = R // p
    return x.reshape(S, C, g, p, g, p).permute(0, 2, 4, 3, 5, 1).reshape(S * g * g, p * p * C)


def check_sampler_f32(lib, dev, H=48, W=80, S=5, size=32, patch=16, augment=False, seed=0):
    """APH_OUT_PATCH_F32 == the patch-major rearrangement of APH_OUT_NCHW_NORM, bit for bit; the adjoint takes the mode and gives
    the APH_OUT_NCHW_NORM adjoint of the rearranged gradient"""
    from aphantasia_amd.transforms import pack_aug
    from oracle import augment_ref, reference_path as R
    torch.manual_seed(seed)
    np.random.seed(seed)
    rgb = torch.rand(3, H, W, generator=torch.Generator().manual_seed(seed)).to(dev).contiguous()
    geom = ops.make_geom(H, W, S, size, patch, 'uniform')
    table = R.draw_crop_table(S, size, H, W, 'uniform', 0.4)
    table_d = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    aug_d = None
    if augment:          # perspective on every other cut, erasing on some, rotations (the -tf fast chain)
        angles = [-30.0, 0.0, 17.0, 29.0, -5.0, 0.0]
        prms = []
        for s in range(S):
            sp, ep = augment_ref.perspective_get_params(size, size, 0.33)
            prms.append(dict(persp=augment_ref.perspective_coeffs(sp, ep) if s % 2 == 0 else None,
                             erase=(2, 3, size // 3, size // 2) if s % 6 in (1, 2) else None, angle=angles[s % 6]))
        aug_d = pack_aug(prms).to(dev)
    nchw = ops.sample_fwd(geom, rgb, table_d, aug_d, out_mode=_ffi.APH_OUT_NCHW_NORM, lib=lib)
    pm = ops.sample_fwd(geom, rgb, table_d, aug_d, out_mode=_ffi.APH_OUT_PATCH_F32, lib=lib)
    assert pm.dtype == torch.float32 and torch.equal(pm.cpu(), to_patch_major(nchw.cpu(), patch))
    g = torch.randn(S, 3, size, size, generator=torch.Generator().manual_seed(seed + 1))
    g_pm = to_patch_major(g, patch).contiguous().to(dev)
    a = ops.sample_bwd(geom, g.to(dev).contiguous(), table_d, aug_d, out_mode=_ffi.APH_OUT_NCHW_NORM, lib=lib)
    b = ops.sample_bwd(geom, g_pm, table_d, aug_d, out_mode=_ffi.APH_OUT_PATCH_F32, lib=lib)
    assert (a.cpu() - b.cpu()).abs().max().item() <= 1e-5 * a.abs().max().item()


# ------------------------------------------------------------------------------------------------------------ fp32 attention (vit_attn_f32.h)
def attn_f32_call(lib, qkv, att, lse, datt, delta, dqkv, S, T, heads, mode):
    ops._L(lib, qkv).call('aph_attn_f32_test', ops.ptr(qkv), ops.ptr(att), ops.ptr(lse), ops.ptr(datt), ops.ptr(delta), ops.ptr(dqkv), S, T, heads,
                          mode, ops._stream(qkv))


def attn_fwd_bound_f32(r, v):
    """(e_att, e_lse) of attn_fwd_f32_kernel; docstring of check_attention_f32"""
    U = V.U
    eps_p = (r['e_s'] + r['e_mx']) / 8 + U * (r['s'] - r['mx']).abs() / 8 + 2 * U
    eps_l = (r['P'] * eps_p).sum(-1, keepdim=True) + 10 * U
    e_att = (r['P'] * (eps_p + eps_l + 2 * U)) @ v.abs() + 1e-6 * (r['P'] @ v.abs())
    ll = torch.log(r['l'])
    e_lse = r['e_mx'] / 8 + eps_l + 2 * U * ll + U * (r['mx'].abs() / 8 + ll)
    return e_att, e_lse


def attn_bwd_bound_f32(r, b, L, q, k, dO, eps_extra=None):
    """(e_D, e_dQ, e_dK, e_dV) of attn_bwd_dq_f32_kernel / attn_bwd_dkv_f32_kernel; docstring of check_attention_f32"""
    U = V.U
    eps_pb = r['e_s'] / 8 + U * (r['s'].abs() / 8 + L.abs()) + 2 * U
    if eps_extra is not None:
        eps_pb = eps_pb + eps_extra
    Pb, dp = b['Pb'], b['dp']
    e_D = (Pb * (eps_pb * dp.abs() + b['e_dp'])).sum(-1, keepdim=True) + 10 * U * (Pb * dp.abs()).sum(-1, keepdim=True)
    dS8 = b['dS'].abs() * 8                                  # the kernels keep Pb (dp - D) and scale the contraction by 1 / 8
    e_dS8 = dS8 * (eps_pb + 2 * U) + Pb * (b['e_dp'] + e_D)
    e_dQ = (e_dS8 @ k.abs() + 1e-6 * (dS8 @ k.abs())) / 8
    e_dK = (e_dS8.mT @ q.abs() + 1e-6 * (dS8.mT @ q.abs())) / 8
    e_dV = (Pb * eps_pb).mT @ dO.abs() + 1e-6 * (Pb.mT @ dO.abs())
    return e_D, e_dQ, e_dK, e_dV


def check_attention_f32(lib, dev, S, T, heads, kind='normal', seed=0):
    """The exact path's fp32 attention (vit_attn_f32.h) through aph_attn_f32_test against fp64 on the same inputs (the families of
    vit_component_checks.attn_inputs, kept at their f16-representable values), element by element and per (cut, head): forward, the backward
    alone (fed lse = f32(lse_ref)) and one chained run; delta too.  Sentinels behind every output, inputs unchanged, two identical calls give
    the same bits.  Returns the worst err / bound per output ('dq+' ...: the chained run).

    Every contraction is an fp32 fma chain, bounded by the figure check_gemm_f32 uses: e_s = 1e-6 |q| . |k| (scores), e_dp = 1e-6 |dO| . |v|,
    1e-6 (P @ |v|) and the like for the output sums.  expf and logf: 1 ulp = 2 U (HIP's documented maximum).  U = 2^-24.
    Forward (attn_fwd_f32_kernel):  p = expf((s - mx) * 0.125f): the difference of two computed scores, one rounding (the product is exact)
      eps_p = (e_s + max_j e_s) / 8 + U |s - mx| / 8 + 2 U
      eps_l = sum_j P eps_p + 10 U              l: at most 4 terms per lane and the 6 levels of wave_sum
      e_att = (P (eps_p + eps_l + 2 U)) @ |v| + 1e-6 (P @ |v|)          P[j] = p * (1.0f / l): two roundings
      e_lse = max_j e_s / 8 + eps_l + 2 U log l + U (|mx| / 8 + log l)   mx * 0.125f exact, logf, the sum
    Backward (attn_bwd_dq_f32_kernel, attn_bwd_dkv_f32_kernel): Pb = expf(s * 0.125f - L) (no clamp), one rounding of the difference
      eps_pb = e_s / 8 + U (|s| / 8 + |L|) + 2 U
      e_D   = sum_j Pb (eps_pb |dp| + e_dp) + 10 U sum_j Pb |dp|         delta_i = sum_j Pb dp, summed like l; the dK / dV kernel reads it back
      dS' = Pb (dp - D):  e_dS' = |dS'| (eps_pb + 2 U) + Pb (e_dp + e_D)
      e_dQ = (e_dS' @ |k| + 1e-6 |dS'| @ |k|) / 8, e_dK likewise with |q|;  e_dV = (Pb eps_pb)^T @ |dO| + 1e-6 Pb^T @ |dO|
    Chained: eps_pb += e_lse.  loss_scaled here means: |D_i| ~ 6.6e5 next to dp - D ~ 3e2, results finite and within the same bounds."""
    D, M, NL, G = heads * 64, S * T, S * heads * T, V.GUARD_ROWS
    what = 'fp32 attention %s S=%d T=%d heads=%d' % (kind, S, T, heads)
    qkv, datt = (t.float() for t in V.attn_inputs(kind, S, T, heads, seed))
    q, k, v = V.attn_items(qkv, S, T, heads, 3)
    dO, = V.attn_items(datt, S, T, heads)
    n_items = S * heads
    step = max(1, V.ATTN_CHUNK // (T * T))
    chunks = [slice(a, min(a + step, n_items)) for a in range(0, n_items, step)]
    f32 = torch.float32

    st = V.AttnStats()
    O, e_att = torch.empty_like(q), torch.empty_like(q)
    lse, e_lse = torch.empty(n_items, T, 1, dtype=torch.float64), torch.empty(n_items, T, 1, dtype=torch.float64)
    for c in chunks:
        r = V.attn_fwd_ref(q[c], k[c], v[c])
        st.forward(r, T)
        O[c], lse[c] = r['O'], r['lse']
        e_att[c], e_lse[c] = attn_fwd_bound_f32(r, v[c])
    st.check_forward(kind, what)

    ins = dict(qkv=qkv, datt=datt)
    dd = {n: t.clone().to(dev) for n, t in ins.items()}
    held = {}

    def fwd():
        att, ls = V.sentinel(M + G, D, f32, dev), V.sentinel(1, NL + G, f32, dev)
        attn_f32_call(lib, dd['qkv'], att, ls, None, None, None, S, T, heads, 0)
        held['att'], held['lse'] = att, ls
        return att.cpu(), ls.cpu()
    lse_in = V.sentinel(1, NL + G, f32, 'cpu')
    lse_in[0, :NL] = lse.reshape(-1).float()
    att_nan = V.sentinel(M + G, D, f32, dev)                 # the backward takes no att: all NaN, and untouched afterwards

    def bwd(ls):
        l0 = V.bits(ls).clone()
        dq, dl = V.sentinel(M + G, 3 * D, f32, dev), V.sentinel(1, NL + G, f32, dev)
        attn_f32_call(lib, dd['qkv'], att_nan, ls, dd['datt'], dl, dq, S, T, heads, 1)
        assert torch.equal(V.bits(ls), l0), what + ': the backward changed lse'
        return dq.cpu(), dl.cpu()
    att, ls = V._twice(fwd, what + ' forward')
    g_alone, d_alone = V._twice(lambda: bwd(lse_in.clone().to(dev)), what + ' backward')
    g_chain, d_chain = bwd(held['lse'])
    V._unchanged(dd, ins, what)

    fd = V.Findings(what)
    fd.within('att', att[:M], V.attn_rows(O, S, T, heads), V.attn_rows(e_att, S, T, heads))
    fd.within('lse', ls[0, :NL], lse.reshape(-1), e_lse.reshape(-1))
    fd.run(V.assert_untouched, att, V._window(M + G, D, slice(0, M)), what + ' (att)')
    fd.run(V.assert_untouched, ls, V._window(1, NL + G, (0, slice(0, NL))), what + ' (lse)')
    fd.run(V.assert_untouched, att_nan.cpu(), torch.zeros(M + G, D, dtype=torch.bool), what + ' (att of the backward)')
    L_in = lse_in[0, :NL].double().reshape(n_items, T, 1)
    got = {'': V.attn_items(g_alone[:M], S, T, heads, 3), '+': V.attn_items(g_chain[:M], S, T, heads, 3)}
    dl = {'': d_alone[0, :NL].reshape(n_items, T, 1), '+': d_chain[0, :NL].reshape(n_items, T, 1)}
    for c in chunks:
        r = V.attn_fwd_ref(q[c], k[c], v[c])
        for tag in ('', '+'):
            L = L_in[c] if tag == '' else r['lse']
            b = V.attn_bwd_ref(r['s'], L, q[c], k[c], v[c], dO[c], clamp=False)
            if tag == '':
                st.backward(b)
            e = attn_bwd_bound_f32(r, b, L, q[c], k[c], dO[c], eps_extra=None if tag == '' else e_lse[c])
            fd.within('delta' + tag, dl[tag][c], b['D'], e[0])
            for i, n in enumerate(('dQ', 'dK', 'dV')):
                fd.within(n.lower() + tag, got[tag][i][c], b[n], e[1 + i])
    st.check_backward(kind, what)
    for tag, gq, gd in (('', g_alone, d_alone), ('+', g_chain, d_chain)):
        fd.run(V.assert_untouched, gq, V._window(M + G, 3 * D, slice(0, M)), what + ' (dqkv%s)' % tag)
        fd.run(V.assert_untouched, gd, V._window(1, NL + G, (0, slice(0, NL))), what + ' (delta%s)' % tag)
    return fd.finish()
