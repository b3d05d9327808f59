"""Checks of the depth estimator (csrc/depth.hip, depth_kernels.h, the X instantiation of lpips_conv.h, depth_epi.h's erf-GELU epilogue)
shared by the interpreter tests (test_emu_depthnet.py) and the GPU tests (test_gpu_depthnet.py).  `lib` = a loaded C-ABI library (the
interpreter build) or None (the product), `dev` = where its tensors live.

Element-wise checks go through the test entries of include/aphantasia_hip_test.h against fp64 computed from the SAME f16 operands the kernel
read.  U = 2^-24, H = 2^-11, H_SUB = 2^-25 (vit_component_checks).  The bounds are derived:
  attention      vit_component_checks.attn_fwd_bound_f16 with what the online softmax adds (attn_long_bound below)
  convolutions   lpips_checks.conv_bound: 2^-11 |ref| + 2 K 2^-24 sum|a w| + 2^-25 with K = 9 Cin + 3 (bias and the two residual terms are
                 fp32 additions inside the magnitude sum); the neck GEMM and the transpose convolution likewise with K = Cin + 1
  resize         2^-11 |ref| + 8 U sum_taps |w x| + 2^-25: each weight is one fp32 division and one subtraction from 1, the blend three
                 products and three additions deep
  erf-GELU GEMM  |gelu'| <= 1.13 times the accumulator figure 1e-6 |a| . |b| (check_gemm_epilogue's) + 2 U |u|, + 8 U (|u| + 1) for erff
                 and the three products around it, + one f16 rounding
The end-to-end gate is measured as lpips_checks does it: E16 = the error of the fp64 restatement run with the kernels' rounding points
(depthnet_ref.forward(rounding=True)) against the pure fp64 restatement; the kernel must be within 2 x E16 on max-abs and on relative L2, of
the un-normalised map and of the normalised one."""
import math
from ctypes import c_int, c_void_p, byref

import torch
import torch.nn.functional as F

from aphantasia_amd import _ffi, ops
from aphantasia_amd import depthnet as DN
import depthnet_ref as R
import lpips_checks as K
import vit_component_checks as V

U, H, H_SUB = V.U, V.H, V.H_SUB
L_, sync, banded, assert_bands, nhwc16, up = K.L_, K.sync, K.banded, K.assert_bands, K.nhwc16, K.up

# hidden 128 / 2 heads / 4 layers, neck 16-32-64-64, fusion 32, head 16: the configuration of the restatement test and of the interpreter
NARROW = dict(backbone_config=dict(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, out_indices=[1, 2, 3, 4]),
              neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32, head_hidden_size=16)
# Base's widths on two layers, each tapped twice (taps 1, 1, 2, 2): the GPU end-to-end network.  transformers' backbone cannot tap a layer
# twice; the restatement and the library can, and this network is only ever compared with the restatement.
BASE2 = dict(backbone_config=dict(hidden_size=768, num_hidden_layers=2, num_attention_heads=12, out_indices=[1, 1, 2, 2]),
             neck_hidden_sizes=[96, 192, 384, 768], fusion_hidden_size=128, head_hidden_size=32)


# ------------------------------------------------------------------------------------------------------------------------------ attention
ATTN_KINDS = ('normal', 'flat', 'peaked', 'negative')


def attn_tile_edges():
    """T = 1, one below / at / one above every query-tile and key-tile edge (both 64) up to three tiles, and 118"""
    return [1] + [e + d for e in (64, 128, 192) for d in (-1, 0, 1)] + [118]


def attn_long_bound(r, v, T):
    """attn_fwd_bound_f16 for attn_long_fwd_kernel.  n = ceil(T / 64) key tiles; A = max_j |s| bounds every running maximum.
      e_x    = kSL (e_s + max e_s) + 3 U kSL (|s| + A)          the exponent against the running maximum of its tile
      eps_sc = ln2 (2 kSL max e_s + 6 U kSL A) + 2 U             one rescale factor 2^((m_old - m_new) kSL): two computed maxima, the difference,
                                                                 the product, v_exp_f32
      eps_p  = ln2 e_x + 2 U + n (eps_sc + U)                    p, then at most n rescales of what it was added into (factor and product)
      eps_l  = sum_j P eps_p + (T + 2 n) U                       the fp32 row sum: T additions, l * sc + ls per tile
      e_att  = (P (eps_p + H)) @ |v| + (H_SUB / l) sum_j |v_j| + (eps_l + (3 + T) U) (P @ |v|)      as attn_fwd_bound_f16 (a rescale never
                                                                 exceeds 1, so the subnormal term keeps its form)"""
    n = (T + 63) // 64
    A = r['s'].abs().amax(-1, keepdim=True)
    e_x = V.KSL * (r['e_s'] + r['e_mx']) + 3 * U * V.KSL * (r['s'].abs() + A)
    eps_sc = V.LN2 * (2 * V.KSL * r['e_mx'] + 6 * U * V.KSL * A) + 2 * U
    eps_p = V.LN2 * e_x + 2 * U + n * (eps_sc + U)
    eps_l = (r['P'] * eps_p).sum(-1, keepdim=True) + (T + 2 * n) * U
    av = v.abs()
    return (r['P'] * (eps_p + H)) @ av + (H_SUB / r['l']) * av.sum(-2, keepdim=True) + (eps_l + (3 + T) * U) * (r['P'] @ av)


def check_attention(lib, dev, B, T, heads, kind, seed=0):
    """aph_depth_attn_test against fp64 from the same f16 operands, per (image, head), element by element -> worst err / bound"""
    D, M = heads * 64, B * T
    qkv, _ = V.attn_inputs(kind, B, T, heads, seed)
    d_qkv = qkv.to(dev)
    big, att = banded(M * D, torch.float16, dev)
    sync(dev)
    L_(lib).call('aph_depth_attn_test', ops.ptr(d_qkv), ops.ptr(att), B, T, heads, ops._stream(d_qkv))
    sync(dev)
    assert_bands(big, 'attention T=%d' % T)
    assert torch.equal(d_qkv.cpu(), qkv), 'attention: the input changed'
    got = att.cpu().view(M, D)
    assert not bool(torch.isnan(got).any()), 'attention T=%d: %d elements never written (or NaN)' % (T, int(torch.isnan(got).sum()))
    q, k, v = V.attn_items(qkv, B, T, heads, 3)
    g_items, = V.attn_items(got, B, T, heads)
    worst = 0.0
    for it in range(B * heads):      # one (image, head) at a time: [T, T] fp64 temporaries
        r = V.attn_fwd_ref(q[it:it + 1], k[it:it + 1], v[it:it + 1])
        worst = max(worst, V.ratio_f16(g_items[it:it + 1], r['O'], attn_long_bound(r, v[it:it + 1], T)))
    print('attention %-8s B=%d T=%d heads=%d (%s): max err / bound %.3f' % (kind, B, T, heads, dev, worst))
    assert worst <= 1.0, (kind, T, worst)
    return worst


# --------------------------------------------------------------------------------------------------------------------------- convolutions
CONV_VARIANTS = ('nobias', 'bias', 'bias_relu', 'residual', 'residual2', 'relu_in', 'relu_in_out', 'stride2', 'batch2')


def check_conv(lib, dev, cin, cout, h, w, variant, seed=0):
    """one launch of the X instantiation of the 3 x 3 kernel (aph_depth_conv_test) against fp64 -> err / bound"""
    gen = torch.Generator().manual_seed(seed * 1000 + CONV_VARIANTS.index(variant))
    B = 2 if variant == 'batch2' else 1
    n = up(cout, 16)
    xs = [K.conv_operands('normal', cin, cout, h, w, gen) for _ in range(B)]
    wt, b = xs[0][1], xs[0][2]
    x = torch.stack([t[0] for t in xs])                                           # [B, cin, h, w]
    wpad = torch.zeros(n, cin, 3, 3, dtype=torch.float64)
    wpad[:cout] = wt
    bpad = torch.zeros(n, dtype=torch.float64)
    bpad[:cout] = b
    bias = variant != 'nobias'
    relu = variant in ('bias_relu', 'relu_in_out')
    relu_in = variant in ('relu_in', 'relu_in_out', 'batch2')
    nres = 2 if variant in ('residual2', 'batch2') else 1 if variant == 'residual' else 0
    stride = 2 if variant == 'stride2' else 1
    res = [(torch.randn(B, n, h, w, generator=gen) * 2).half().double() for _ in range(nres)]
    d_x = torch.stack([nhwc16(x[i], up(cin, 8), 'cpu') for i in range(B)]).to(dev)
    d_w = K.pack(lib, dev, wpad, False)
    d_b = bpad.float().to(dev) if bias else None
    d_res = [torch.stack([nhwc16(t[i], n, 'cpu') for i in range(B)]).to(dev) for t in res] + [None, None]
    ho, wo = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    big, out = banded(B * ho * wo * n, torch.float16, dev)
    tbig, tmp = banded(B * h * w * n, torch.float16, dev)
    sync(dev)
    L_(lib).call('aph_depth_conv_test', ops.ptr(d_x), h, w, up(cin, 8), ops.ptr(d_w), n, ops.ptr(d_b), int(relu), int(relu_in), ops.ptr(d_res[0]),
                 ops.ptr(d_res[1]), B, stride, ops.ptr(tmp) if stride == 2 else None, ops.ptr(out), ops._stream(d_x))
    sync(dev)
    assert_bands(big, 'conv %s' % variant)
    assert_bands(tbig, 'conv %s (stride-1 scratch)' % variant)
    got = out.cpu().view(B, ho, wo, n).permute(0, 3, 1, 2).double()
    assert not bool(torch.isnan(got).any()), 'conv %s: %d elements never written (or NaN)' % (variant, int(torch.isnan(got).sum()))
    xin = torch.relu(x) if relu_in else x
    ref = F.conv2d(xin, wpad, bpad if bias else None, padding=1, stride=stride)
    mag = F.conv2d(xin.abs(), wpad.abs(), bpad.abs() if bias else None, padding=1, stride=stride)
    if relu:
        ref = torch.relu(ref)
    for t in res:
        ref = ref + t
        mag = mag + t.abs()
    ratio = ((got - ref).abs() / K.conv_bound(ref, mag, 9 * cin + 3)).max().item()
    print('conv %-11s %d->%d %dx%d (%s): max err / bound %.3f' % (variant, cin, cout, h, w, dev, ratio))
    assert ratio <= 1.0, (variant, ratio)
    return ratio


def check_lpips_instantiation_unmoved(lib, dev, cin, cout, h, w):
    """the LPIPS entry (X = false) and the new entry with nothing new switched on (X = true) give the same bits"""
    gen = torch.Generator().manual_seed(5)
    x, wt, b = K.conv_operands('normal', cin, cout, h, w, gen)
    d_x, d_w, d_b = nhwc16(x, up(cin, 8), dev), K.pack(lib, dev, wt, False), b.float().to(dev)
    outs = []
    for new in (False, True):
        big, out = banded(h * w * cout, torch.float16, dev)
        if new:
            L_(lib).call('aph_depth_conv_test', ops.ptr(d_x), h, w, up(cin, 8), ops.ptr(d_w), cout, ops.ptr(d_b), 1, 0, None, None, 1, 1, None, ops.ptr(out), ops._stream(d_x))
        else:
            L_(lib).call('aph_lpips_conv_test', ops.ptr(d_x), h, w, up(cin, 8), ops.ptr(d_w), cout, ops.ptr(d_b), 1, None, ops.ptr(out), None, 0, 0, ops._stream(d_x))
        sync(dev)
        assert_bands(big, 'conv')
        outs.append(out.cpu())
    assert torch.equal(V.bits(outs[0]), V.bits(outs[1]))


def check_gemm1x1(lib, dev, M, K_, N, bias=True, seed=0):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K_, generator=gen).half()
    bt = (torch.randn(N, K_, generator=gen) / math.sqrt(K_)).half()
    b = (torch.rand(N, generator=gen) - 0.5).float()
    d_a, d_bt, d_b = a.to(dev), bt.to(dev), b.to(dev) if bias else None
    big, out = banded(M * N, torch.float16, dev)
    sync(dev)
    L_(lib).call('aph_depth_gemm_test', ops.ptr(d_a), K_, ops.ptr(d_bt), M, N, K_, ops.ptr(d_b), ops.ptr(out), ops._stream(d_a))
    sync(dev)
    assert_bands(big, '1x1 gemm')
    got = out.cpu().view(M, N).double()
    ref = a.double() @ bt.double().T + (b.double() if bias else 0.0)
    mag = a.double().abs() @ bt.double().abs().T + (b.double().abs() if bias else 0.0)
    ratio = ((got - ref).abs() / K.conv_bound(ref, mag, K_ + 1)).nan_to_num(float('inf')).max().item()
    print('1x1 gemm M=%d K=%d N=%d (%s): max err / bound %.3f' % (M, K_, N, dev, ratio))
    assert ratio <= 1.0, ratio
    return ratio


def check_convt(lib, dev, k, cin, cout, gh, gw, B=2, seed=0):
    gen = torch.Generator().manual_seed(seed + k)
    x = torch.randn(B, cin, gh, gw, generator=gen).half().double()
    wt = (torch.randn(cin, cout, k, k, generator=gen) / math.sqrt(cin)).half().double()
    b = (torch.rand(cout, generator=gen) - 0.5).float().double()
    d_x = torch.stack([nhwc16(x[i], cin, 'cpu') for i in range(B)]).to(dev)
    d_b = b.float().to(dev)
    h_w = wt.float().contiguous()
    pbig, d_wp = banded(k * k * cout * cin, torch.float16, dev)
    big, out = banded(B * gh * k * gw * k * cout, torch.float16, dev)
    sync(dev)
    L_(lib).call('aph_depth_convt_test', ops.ptr(d_x), B, gh, gw, cin, c_void_p(h_w.data_ptr()), cout, k, ops.ptr(d_b), ops.ptr(d_wp), ops.ptr(out), ops._stream(d_x))
    sync(dev)
    assert_bands(big, 'transpose conv')
    assert_bands(pbig, 'transpose conv (packed weights)')
    got = out.cpu().view(B, gh * k, gw * k, cout).permute(0, 3, 1, 2).double()
    assert not bool(torch.isnan(got).any()), 'transpose conv: elements never written'
    ref = F.conv_transpose2d(x, wt, b, stride=k)
    mag = F.conv_transpose2d(x.abs(), wt.abs(), b.abs(), stride=k)
    ratio = ((got - ref).abs() / K.conv_bound(ref, mag, cin + 1)).max().item()
    print('transpose conv %dx%d s%d %d->%d on %dx%d (%s): max err / bound %.3f' % (k, k, k, cin, cout, gh, gw, dev, ratio))
    assert ratio <= 1.0, ratio
    return ratio


def resize_ref(x, Ho, Wo):
    """fp64 bilinear align_corners=True of x [B, C, h, w] by the formula: src = dst (in - 1) / (out - 1); -> (value, sum of |weight x|)"""
    _, _, h, w = x.shape

    def axis(n_in, n_out):
        src = torch.arange(n_out, dtype=torch.float64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        i0 = src.floor().long().clamp(max=n_in - 1)
        return i0, (i0 + 1).clamp(max=n_in - 1), src - i0

    y0, y1, fy = axis(h, Ho)
    x0, x1, fx = axis(w, Wo)
    fy, fx = fy.view(1, 1, -1, 1), fx.view(1, 1, 1, -1)

    def blend(t):
        top = t[:, :, y0][:, :, :, x0] * (1 - fx) + t[:, :, y0][:, :, :, x1] * fx
        bot = t[:, :, y1][:, :, :, x0] * (1 - fx) + t[:, :, y1][:, :, :, x1] * fx
        return top * (1 - fy) + bot * fy
    return blend(x), blend(x.abs())


def check_resize(lib, dev, h, w, Ho, Wo, C=16, B=2, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, h, w, generator=gen) * 3).half().double()
    d_x = torch.stack([nhwc16(x[i], C, 'cpu') for i in range(B)]).to(dev)
    big, out = banded(B * Ho * Wo * C, torch.float16, dev)
    sync(dev)
    L_(lib).call('aph_depth_resize_test', ops.ptr(d_x), B, h, w, C, ops.ptr(out), Ho, Wo, ops._stream(d_x))
    sync(dev)
    assert_bands(big, 'resize')
    got = out.cpu().view(B, Ho, Wo, C).permute(0, 3, 1, 2).double()
    assert not bool(torch.isnan(got).any()), 'resize: elements never written'
    ref, mag = resize_ref(x, Ho, Wo)
    if Ho > 1 and Wo > 1:       # the formula is torch's own
        assert torch.allclose(ref, F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=True), rtol=0, atol=1e-12)
    if (Ho, Wo) == (h, w):
        assert torch.equal(got, x), 'resize to the same size is not the identity'
    ratio = ((got - ref).abs() / (H * ref.abs() + 8 * U * mag + H_SUB)).max().item()
    print('resize %dx%d -> %dx%d C=%d (%s): max err / bound %.3f' % (h, w, Ho, Wo, C, dev, ratio))
    assert ratio <= 1.0, ratio
    return ratio


def check_gelu_gemm(lib, dev, M, N, K_, seed=0):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K_, generator=gen).half()
    bt = (torch.randn(N, K_, generator=gen) * (2.0 / math.sqrt(K_))).half()
    b = torch.randn(N, generator=gen).float()
    d_a, d_bt, d_b = a.to(dev), bt.to(dev), b.to(dev)
    big, out = banded(M * N, torch.float16, dev)
    sync(dev)
    L_(lib).call('aph_depth_gelu_gemm_test', ops.ptr(d_a), ops.ptr(d_bt), M, N, K_, ops.ptr(d_b), ops.ptr(out), ops._stream(d_a))
    sync(dev)
    assert_bands(big, 'gelu gemm')
    got = out.cpu().view(M, N).double()
    assert not bool(torch.isnan(got).any()), 'gelu gemm: elements never written'
    u = a.double() @ bt.double().T + b.double()
    ref = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
    e_u = 1e-6 * (a.double().abs() @ bt.double().abs().T + b.double().abs()) + 2 * U * u.abs()
    bound = 1.13 * e_u + 8 * U * (u.abs() + 1) + H * ref.abs() + H_SUB
    ratio = ((got - ref).abs() / bound).max().item()
    print('erf-GELU gemm M=%d N=%d K=%d (%s): max err / bound %.3f' % (M, N, K_, dev, ratio))
    assert ratio <= 1.0, ratio
    return ratio


# ------------------------------------------------------------------------------------------------------------------------------ end to end
def make_image(B, h, w, seed=0):
    """smooth structure plus noise, in (0, 1)"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing='ij')
    base = torch.stack([0.5 + 0.4 * torch.sin(6.0 * xx + 2.0 * c) * torch.cos(4.0 * yy - c) for c in range(3)])
    img = base[None] + 0.1 * torch.randn(B, 3, h, w, generator=g)
    return img.clamp(0.01, 0.99).float()


def errors(got, ref):
    """(max-abs, relative L2) of got against ref"""
    d = got.double() - ref
    return d.abs().max().item(), (d.norm() / ref.norm()).item()


_E2E_CACHE = {}


def e2e_reference(config_name, config, h, w, seed, B=1):
    """(weights, image, pure fp64 map, rounding-model map) of one case, computed once per session"""
    key = (config_name, h, w, seed, B)
    if key not in _E2E_CACHE:
        img = make_image(B, h, w, seed)
        sd, z = R.conditioned_weights(config, seed, img)
        pure = torch.relu(z)
        positive = (z > 0).double().mean().item()
        assert positive >= 0.99, 'only %.4f of the fp64 pixels are positive before the last ReLU' % positive
        _E2E_CACHE[key] = (sd, img, pure, R.forward(config, sd, img, rounding=True), positive)
    return _E2E_CACHE[key]


def check_e2e(lib, dev, config_name, config, h, w, seed=0, B=1):
    """aph_depth_forward against the pure fp64 restatement, gated by 2 x E16 -> dict of the measured figures"""
    sd, img, pure, model, positive = e2e_reference(config_name, config, h, w, seed, B)
    net = DN.DepthAnythingHIP.from_state_dict(config, sd, max_hw=(h, w), max_batch=B, lib=lib)
    d_img = img.to(dev)
    raw = net.forward(d_img, normalise=False)
    nrm = net.forward(d_img, normalise=True)
    sync(dev)
    raw, nrm = raw.cpu()[:, 0], nrm.cpu()[:, 0]
    assert not bool(torch.isnan(raw).any()) and not bool(torch.isnan(nrm).any())
    out = dict(positive=positive)
    ok = True
    for name, got, ref, mod in (('raw', raw, pure, model), ('normalised', nrm, R.normalise(pure), R.normalise(model))):
        e16 = errors(mod, ref)
        ek = errors(got, ref)
        out[name] = dict(E16_maxabs=e16[0], E16_rel_l2=e16[1], kernel_maxabs=ek[0], kernel_rel_l2=ek[1])
        print('end to end %s %dx%d B=%d seed %d (%s) %-10s: max-abs kernel %.4e  E16 %.4e (ratio %.3f);  rel-L2 kernel %.4e  E16 %.4e (ratio %.3f);  '
              'positive before the last ReLU %.4f' % (config_name, h, w, B, seed, dev, name, ek[0], e16[0], ek[0] / e16[0], ek[1], e16[1], ek[1] / e16[1], positive))
        ok = ok and ek[0] <= 2 * e16[0] and ek[1] <= 2 * e16[1]
    net.close()
    assert ok, out
    return out


def check_batch_and_flip(lib, dev, config, h, w, seed=1):
    """a batch-of-2 call equals two single calls bit for bit; depth_map on the hip backend equals the two-call formulation"""
    from aphantasia_amd import depthwarp as DW
    sd = DN.synthetic_weights(config, seed, last_bias=1.0)
    net = DN.DepthAnythingHIP.from_state_dict(config, sd, max_hw=(h, w), max_batch=2, lib=lib)
    img = make_image(2, h, w, seed).to(dev)
    for normalise in (False, True):
        both = net.forward(img, normalise=normalise)
        one = torch.cat([net.forward(img[i:i + 1], normalise=normalise) for i in range(2)])
        sync(dev)
        assert torch.equal(V.bits(both.cpu()), V.bits(one.cpu())), 'batch of 2 differs from two single calls (normalise=%s)' % normalise
    frame = make_image(1, 40, 56, seed + 1).to(dev)
    infer = DW.InferDepthAny.from_estimator(net, lib=lib)
    batched = DW.depth_map(frame, infer, res=h, lib=lib)
    two_calls = DW.depth_map(frame, lambda im: infer(im), res=h, lib=lib)       # a plain callable: the two-call formulation of depth.py:71-78
    sync(dev)
    assert torch.equal(V.bits(batched.cpu()), V.bits(two_calls.cpu())), 'depth_map: the batch-of-2 path differs from the two-call formulation'
    net.close()


def check_refusals(lib, dev):
    lb = L_(lib)
    c = DN.parse_config(NARROW)

    def create(hidden=128, layers=4, heads=2, swiglu=0, max_h=56, max_w=84, max_batch=2):
        out = c_void_p()
        rc = lb.cdll.aph_depth_create(hidden, layers, heads, swiglu, (c_int * 4)(*c['out_indices']), (c_int * 4)(*c['neck']), c['fusion'], c['head'], max_h, max_w,
                                      max_batch, byref(out))
        return rc, out

    rc, _ = create(swiglu=1)
    assert rc < 0 and 'SwiGLU' in lb.last_error(), lb.last_error()
    rc, _ = create(hidden=192, heads=3)
    assert rc < 0, 'hidden 192 accepted'
    rc, _ = create(max_h=57)
    assert rc < 0, 'max_h 57 accepted'
    rc, handle = create()
    assert rc == 0, lb.last_error()
    img = torch.zeros(3, 3, 70, 98, device=dev)
    out = torch.zeros(3, 1, 70, 98, device=dev)

    def fwd(B, h, w):
        rc = lb.cdll.aph_depth_forward(handle, ops.ptr(img), B, h, w, 1, ops.ptr(out), None)
        return rc, lb.last_error()

    rc, msg = fwd(1, 57, 84)
    assert rc < 0 and 'multiples of 14' in msg, msg
    rc, msg = fwd(1, 56, 85)
    assert rc < 0 and 'multiples of 14' in msg, msg
    rc, msg = fwd(1, 70, 84)
    assert rc < 0 and 'larger than' in msg, msg
    rc, msg = fwd(1, 56, 98)
    assert rc < 0 and 'larger than' in msg, msg
    rc, msg = fwd(3, 56, 84)
    assert rc < 0 and 'batch 3' in msg, msg
    # weights: nothing set -> the first name; all but one set -> that one; an unknown name and a wrong count are refused at once
    rc, msg = fwd(1, 56, 84)
    assert rc < 0 and 'backbone.embeddings.cls_token not set' in msg, msg
    sd = DN.synthetic_weights(NARROW, 0)
    missing = 'neck.convs.2.weight'
    for name, t in sd.items():
        if name in (missing, 'backbone.embeddings.position_embeddings'):
            continue
        assert lb.cdll.aph_depth_set_weight(handle, name.encode(), c_void_p(t.data_ptr()), t.numel()) == 0, lb.last_error()
    rc, msg = fwd(1, 56, 84)
    assert rc < 0 and missing + ' not set' in msg, msg
    t = sd[missing]
    assert lb.cdll.aph_depth_set_weight(handle, b'neck.convs.9.weight', c_void_p(t.data_ptr()), t.numel()) < 0 and 'unknown key' in lb.last_error()
    assert lb.cdll.aph_depth_set_weight(handle, missing.encode(), c_void_p(t.data_ptr()), t.numel() - 1) < 0 and 'expected' in lb.last_error()
    assert lb.cdll.aph_depth_set_weight(handle, missing.encode(), c_void_p(t.data_ptr()), t.numel()) == 0
    rc, msg = fwd(1, 56, 84)
    assert rc < 0 and 'position rows' in msg, msg        # every weight is there; the grid's position rows are not
    assert lb.cdll.aph_depth_destroy(handle) == 0
    # the Python layer
    import pytest
    from aphantasia_amd import depthwarp as DW
    with pytest.raises(ValueError, match='SwiGLU'):
        DN.DepthAnythingHIP.from_state_dict(dict(NARROW, backbone_config=dict(NARROW['backbone_config'], use_swiglu_ffn=True)), sd, lib=lib)
    broken = dict(sd)
    del broken['head.conv1.bias']
    with pytest.raises(KeyError, match='head.conv1.bias'):
        DN.DepthAnythingHIP.from_state_dict(NARROW, broken, lib=lib)
    net = DN.DepthAnythingHIP.from_state_dict(NARROW, sd, lib=lib)
    with pytest.raises(ValueError, match='multiples of 14'):
        net(torch.zeros(1, 3, 57, 84, device=dev))
    for backend in ('hip', 'torch'):
        with pytest.raises(RuntimeError, match='no local Depth-Anything-V2 checkpoint'):
            DW.InferDepthAny('B', dev, path=None, backend=backend)
    with pytest.raises(ValueError, match='backend'):
        DW.InferDepthAny('B', dev, path='.', backend='triton')
