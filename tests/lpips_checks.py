"""Checks of the LPIPS term (csrc/lpips.hip, lpips_conv.h, lpips_ops.h) shared by the interpreter tests (test_emu_lpips.py) and the GPU tests
(test_gpu_lpips.py).  `lib` = a loaded C-ABI library (the interpreter build) or None (the product), `dev` = where its tensors live.

Element-wise checks go through the test entries of include/aphantasia_hip_test.h against fp64 computed from the SAME f16 operands the kernel
read; where a decision depends on values (ReLU mask, pool argmax) both sides are given the same stored activations.  The bounds are derived:
  conv forward / dgrad   |out - ref| <= 2^-11 |ref| + 2 K 2^-24 sum|a w| + 2^-25       (one f16 rounding of the result, fp32 accumulation
                         over K = 9 Cin (9 Cout for dgrad) terms, f16 subnormal spacing); the fp32 bias add is inside the K term
  pool                   exact, forward and backward (tie: first maximum in row-major window order)
  head                   1e-5 relative: the value against |ref|, the gradient per pixel against that pixel's max |ref| over channels
                         (an all-zero column has a gradient of order 1 / eps = 1e10: a tensor-wide maximum would hide every other pixel)
  resize / adjoint       <= 32 2^-24 sum|tap x| per element; <R x, g> against <x, R^T g>
The end-to-end gate is measured, not invented: E16 = the error of the fp64 restatement run with the kernels' rounding model (lpips_ref.py)
against the pure fp64 restatement; the kernel must be within 2 x E16 on each measure (value, relative L2 and 1 - cosine of the gradient)."""
import math
from ctypes import c_int, c_void_p, byref

import torch
import torch.nn.functional as F

from aphantasia_amd import _ffi, ops
from aphantasia_amd import lpips as alpips
import lpips_ref as R
import vit_component_checks as V

BAND = 512
FULL = (64, 128, 256, 512, 512)
NARROW = (16, 16, 32, 32, 32)


def L_(lib):
    return lib if lib is not None else _ffi.lib()


def sync(dev):
    if str(dev).startswith('cuda'):
        torch.cuda.synchronize()


def banded(n, dtype, dev):
    """(whole buffer, NaN-prefilled view of n elements between two sentinel bands)"""
    big = V.sentinel(1, n + 2 * BAND, dtype, dev).reshape(-1)
    view = big[BAND:BAND + n]
    view.fill_(float('nan'))
    return big, view


def assert_bands(big, what):
    b = V.bits(big)
    want = V.SENT32 if big.dtype == torch.float32 else V.SENT16
    assert bool((b[:BAND] == want).all()) and bool((b[-BAND:] == want).all()), '%s: a store outside the buffer' % what


def nhwc16(t, cpad, dev):
    """t [C, H, W] (any float dtype) -> f16 [H, W, cpad] on dev, pad channels zero"""
    c, h, w = t.shape
    out = torch.zeros(h, w, cpad, dtype=torch.float16)
    out[:, :, :c] = t.permute(1, 2, 0).to(torch.float16)
    return out.contiguous().to(dev)


def up(v, m):
    return (v + m - 1) // m * m


def pack(lib, dev, w, dgrad):
    """w fp32 [cout, cin, 3, 3] -> the packed f16 operand, by the library's own routine"""
    cout, cin = w.shape[:2]
    n = 9 * (up(cin, 16) * cout if dgrad else cout * up(cin, 8))
    big, out = banded(n, torch.float16, dev)
    w = w.float().contiguous()
    sync(dev)
    L_(lib).call('aph_lpips_pack_test', c_void_p(w.data_ptr()), cout, cin, int(dgrad), ops.ptr(out), n)
    sync(dev)
    assert_bands(big, 'aph_lpips_pack_test')
    assert not bool(torch.isnan(out).any())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------- convolution
FWD_FAMILIES = ('normal', 'positive', 'onehot', 'f16max')
BWD_FAMILIES = ('normal', 'positive', 'onehot')
NFS = (4, 2, 1, 0)           # output channels per workgroup / 16 of aph_lpips_conv_test; 0 = the library's rule


def conv_operands(family, cin, cout, h, w, gen):
    """-> (activation [cin, h, w], weight [cout, cin, 3, 3], bias [cout]) as f16-representable doubles (bias fp32-representable)"""
    k = 9 * cin
    x = torch.randn(cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / k)
    b = (torch.rand(cout, generator=gen) - 0.5)
    if family == 'positive':
        x, wt, b = x.abs() + 0.01, wt.abs(), b.abs()
    elif family == 'onehot':
        x = torch.zeros(cin, h, w)
        x[int(torch.randint(cin, (1,), generator=gen)), h // 2, min(w - 1, w // 2 + 1)] = 1.0
        b = torch.zeros(cout)
    elif family == 'f16max':
        x = (30000.0 + 35000.0 * torch.rand(cin, h, w, generator=gen)) * torch.sign(torch.randn(cin, h, w, generator=gen))
        wt = wt * 2.0 ** -8            # outputs of a few hundred: far inside f16
    return x.half().double(), wt.half().double(), b.float().double()


def conv_bound(ref, mag, k):
    return 2.0 ** -11 * ref.abs() + 2.0 * k * 2.0 ** -24 * mag + 2.0 ** -25


def check_conv_fwd(lib, dev, cin, cout, h, w, seed=0):
    """one forward launch per input family against fp64 -> the worst ratio error / bound"""
    lb = L_(lib)
    worst = 0.0
    for fi, family in enumerate(FWD_FAMILIES):
        gen = torch.Generator().manual_seed(seed * 100 + fi)
        x, wt, b = conv_operands(family, cin, cout, h, w, gen)
        d_x = nhwc16(x, up(cin, 8), dev)
        d_w = pack(lib, dev, wt, False)
        d_b = b.float().to(dev)
        outs = []
        for nf in NFS:          # every workgroup shape, and the library's own choice: the same bits
            big, out = banded(h * w * cout, torch.float16, dev)
            lb.call('aph_lpips_conv_test', ops.ptr(d_x), h, w, up(cin, 8), ops.ptr(d_w), cout, ops.ptr(d_b), 1, None, ops.ptr(out), None, 0, nf, ops._stream(d_x))
            sync(dev)
            assert_bands(big, 'conv forward nf %d' % nf)
            outs.append(out.cpu())
            assert torch.equal(V.bits(outs[0]), V.bits(outs[-1])), 'conv forward: nf %d gives other bits than nf %d' % (nf, NFS[0])
        got = out.cpu().view(h, w, cout).permute(2, 0, 1).double()
        assert not bool(torch.isnan(got).any()), 'conv forward (%s): %d elements never written (or NaN)' % (family, int(torch.isnan(got).sum()))
        ref = torch.relu(F.conv2d(x[None], wt, b, padding=1)[0])
        mag = F.conv2d(x.abs()[None], wt.abs(), b.abs(), padding=1)[0]
        ratio = ((got - ref).abs() / conv_bound(ref, mag, 9 * cin)).max().item()
        print('conv fwd %d->%d %dx%d %-8s (%s): max err / bound %.3f' % (cin, cout, h, w, family, dev, ratio))
        assert ratio <= 1.0, (family, ratio)
        worst = max(worst, ratio)
    return worst


def check_conv_dgrad(lib, dev, cin, cout, h, w, seed=0):
    """the input gradient of the layer cin -> cout: the same kernel over the packed dgrad weights, masked by a stored activation; for cin = 3
    the planar fp32 output of the network's first layer as well"""
    lb = L_(lib)
    worst = 0.0
    n = up(cin, 16)
    for fi, family in enumerate(BWD_FAMILIES):
        gen = torch.Generator().manual_seed(seed * 100 + 50 + fi)
        g, wt_t, _ = conv_operands(family, cout, cin, h, w, gen)         # g [cout, h, w]; wt_t [cin, cout, 3, 3]
        wt = wt_t.permute(1, 0, 2, 3).contiguous()                       # the layer's weight [cout, cin, 3, 3]
        act = torch.relu(torch.randn(cin, h, w, generator=gen)).half().double()      # stored output of the layer below: about half zeros
        d_g = nhwc16(g, cout, dev)
        d_w = pack(lib, dev, wt, True)
        d_m = nhwc16(act, n, dev)
        outs = []
        for nf in NFS:
            big, out = banded(h * w * n, torch.float16, dev)
            big32, out32 = banded(3 * h * w, torch.float32, dev)
            lb.call('aph_lpips_conv_test', ops.ptr(d_g), h, w, cout, ops.ptr(d_w), n, None, 0, ops.ptr(d_m), ops.ptr(out), ops.ptr(out32) if cin == 3 else None,
                    3 if cin == 3 else 0, nf, ops._stream(d_g))
            sync(dev)
            assert_bands(big, 'conv dgrad nf %d' % nf)
            assert_bands(big32, 'conv dgrad fp32 nf %d' % nf)
            outs.append(out.cpu())
            assert torch.equal(V.bits(outs[0]), V.bits(outs[-1])), 'conv dgrad: nf %d gives other bits than nf %d' % (nf, NFS[0])
        got = out.cpu().view(h, w, n).permute(2, 0, 1).double()
        assert not bool(torch.isnan(got).any()), 'conv dgrad (%s): %d elements never written (or NaN)' % (family, int(torch.isnan(got).sum()))
        assert float(got[cin:].abs().max()) == 0.0 if n > cin else True, 'conv dgrad: pad channels are not zero'
        full = F.conv_transpose2d(g[None], wt, padding=1)[0]
        ref = full * (act > 0)
        mag = F.conv_transpose2d(g.abs()[None], wt.abs(), padding=1)[0]
        ratio = ((got[:cin] - ref).abs() / conv_bound(ref, mag, 9 * cout)).max().item()
        if cin == 3:
            got32 = out32.cpu().view(3, h, w).double()
            ratio = max(ratio, ((got32 - ref).abs() / conv_bound(ref, mag, 9 * cout)).max().item())
        print('conv dgrad %d<-%d %dx%d %-8s (%s): max err / bound %.3f' % (cin, cout, h, w, family, dev, ratio))
        assert ratio <= 1.0, (family, ratio)
        worst = max(worst, ratio)
    return worst


def conv_cases(widths, hh, hw):
    """every distinct (cin, cout, h, w) of the network on a half-size frame hh x hw"""
    out, cin, h, w = [], 3, hh, hw
    for s, n in enumerate(R.CONVS_OF_STAGE):
        if s:
            h, w = h // 2, w // 2
        for _ in range(n):
            if (cin, widths[s], h, w) not in out:
                out.append((cin, widths[s], h, w))
            cin = widths[s]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------ pool
def check_pool(lib, dev, h, w, c, seed=0):
    lb = L_(lib)
    gen = torch.Generator().manual_seed(seed + 7)
    x = torch.randint(0, 4, (c, h, w), generator=gen).double() * 0.5          # four levels: most windows have ties
    x[:, :2, :2] = 1.5                                                        # and one window that is all ties
    d_x = nhwc16(x, c, dev)
    hp, wp = h // 2, w // 2
    dp = torch.randn(c, hp, wp, generator=gen).half().double()
    d_dp = nhwc16(dp, c, dev)
    bigo, out = banded(hp * wp * c, torch.float16, dev)
    bigd, din = banded(h * w * c, torch.float16, dev)
    lb.call('aph_lpips_pool_test', ops.ptr(d_x), h, w, c, ops.ptr(out), ops.ptr(d_dp), ops.ptr(din), ops._stream(d_x))
    sync(dev)
    assert_bands(bigo, 'pool forward')
    assert_bands(bigd, 'pool backward')
    got = out.cpu().view(hp, wp, c).permute(2, 0, 1).double()
    assert torch.equal(got, F.max_pool2d(x[None], 2, 2)[0]), 'pool forward is not exact'
    win = torch.stack([x[:, 0:2 * hp:2, 0:2 * wp:2], x[:, 0:2 * hp:2, 1:2 * wp:2], x[:, 1:2 * hp:2, 0:2 * wp:2], x[:, 1:2 * hp:2, 1:2 * wp:2]])
    arg = win.argmax(0)                                                       # the first maximum in row-major window order
    want = torch.zeros(c, h, w, dtype=torch.float64)
    for k in range(4):
        want[:, (k // 2):2 * hp:2, (k % 2):2 * wp:2] = torch.where(arg == k, dp, torch.zeros_like(dp))
    gotd = din.cpu().view(h, w, c).permute(2, 0, 1).double()
    assert not bool(torch.isnan(gotd).any()), 'pool backward: elements never written'
    assert torch.equal(gotd, want), 'pool backward is not exact: %d elements differ' % int((gotd != want).sum())
    if h % 2:
        assert float(gotd[:, -1].abs().max()) == 0.0
    if w % 2:
        assert float(gotd[:, :, -1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------------ head
def check_head(lib, dev, p, c, seed=0):
    lb = L_(lib)
    gen = torch.Generator().manual_seed(seed + 11)
    f = torch.relu(torch.randn(p, c, generator=gen) + 0.3).half()
    fy = torch.relu(torch.randn(p, c, generator=gen) + 0.3).half()
    if p >= 4:             # an all-zero feature column on either side (not the same pixel)
        f[p // 3] = 0
        fy[p // 2] = 0
    lin = torch.rand(c, generator=gen)
    d_f, d_fy, d_lin = f.to(dev), fy.to(dev), lin.to(dev)
    bign, ny = banded(p * c, torch.float32, dev)
    bigg, hg = banded(p * c, torch.float32, dev)
    part = torch.zeros(512, dtype=torch.float64, device=dev)
    val = torch.full((1,), float('nan'), device=dev)
    lb.call('aph_lpips_head_test', ops.ptr(d_f), ops.ptr(d_fy), ops.ptr(d_lin), p, c, 1.0, ops.ptr(ny), ops.ptr(hg), ops.ptr(part), ops.ptr(val), ops._stream(d_f))
    sync(dev)
    assert_bands(bign, 'head normalised target')
    assert_bands(bigg, 'head gradient')
    leaf = f.double().t().reshape(c, p, 1).clone().requires_grad_(True)
    ny64 = R.unit_norm(fy.double().t().reshape(c, p, 1))
    per_pixel = (lin.double().view(-1, 1, 1) * (R.unit_norm(leaf) - ny64) ** 2).sum(0)
    per_pixel.sum().backward()
    ref_v = per_pixel.mean().item()
    ref_g = leaf.grad.reshape(c, p).t()
    got_v, got_g = float(val.item()), hg.cpu().view(p, c).double()
    assert math.isfinite(got_v) and bool(torch.isfinite(got_g).all()), 'head: a value or gradient is not finite'
    ev = abs(got_v - ref_v) / abs(ref_v)
    eg = ((got_g - ref_g).abs().max(1).values / ref_g.abs().max(1).values.clamp_min(1e-300)).max().item()
    en = ((ny.cpu().view(p, c).double() - ny64.reshape(c, p).t()).abs().max()).item()
    print('head P %d C %d (%s): value rel err %.3g, gradient rel err (per pixel) %.3g, normalised target abs err %.3g' % (p, c, dev, ev, eg, en))
    assert ev <= 1e-5 and eg <= 1e-5 and en <= 1e-6, (ev, eg, en)


# ---------------------------------------------------------------------------------------------------------------------------------------- resize
def cubic_matrix(n_in, n_out):
    """the [n_out, n_in] matrix of the align_corners bicubic resize (A = -0.75, clamped border taps) in fp64"""
    a = -0.75
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        num = o * (n_in - 1)
        i0, t = num // (n_out - 1), (num % (n_out - 1)) / (n_out - 1)

        def c1(x):
            return ((a + 2) * x - (a + 3)) * x * x + 1

        def c2(x):
            return ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
        for j, wgt in enumerate((c2(t + 1), c1(t), c1(1 - t), c2(2 - t))):
            m[o, min(max(i0 - 1 + j, 0), n_in - 1)] += wgt
    return m


def check_resize(lib, dev, h, w, seed=0):
    lb = L_(lib)
    gen = torch.Generator().manual_seed(seed + 13)
    ho, wo = h // 2, w // 2
    x = torch.rand(3, h, w, generator=gen)
    g = torch.randn(3, ho, wo, generator=gen)
    base = torch.randn(3, h, w, generator=gen)
    ry, rx = cubic_matrix(h, ho), cubic_matrix(w, wo)
    x64, g64 = x.double(), g.double()
    ref = ry @ x64 @ rx.t()
    assert float((ref - R.resize_half(x64)).abs().max()) < 1e-12, 'the test\'s own resize matrices disagree with torch'
    mag = ry.abs() @ x64.abs() @ rx.abs().t()
    d_x = x.to(dev).contiguous()
    bigo, out = banded(3 * ho * wo, torch.float32, dev)
    lb.call('aph_lpips_resize_test', ops.ptr(d_x), h, w, ops.ptr(out), 0, ops._stream(d_x))
    sync(dev)
    assert_bands(bigo, 'resize')
    got = out.cpu().view(3, ho, wo).double()
    r1 = ((got - ref).abs() / (32 * 2.0 ** -24 * mag + 1e-300)).max().item()
    # the adjoint accumulates on top of what the buffer holds
    d_g = g.to(dev).contiguous()
    biga, adj = banded(3 * h * w, torch.float32, dev)
    adj.copy_(base.reshape(-1))
    lb.call('aph_lpips_resize_test', ops.ptr(adj), h, w, ops.ptr(d_g), 1, ops._stream(d_g))
    sync(dev)
    assert_bands(biga, 'resize adjoint')
    gota = adj.cpu().view(3, h, w).double()
    refa = ry.t() @ g64 @ rx
    maga = ry.abs().t() @ g64.abs() @ rx.abs()
    r2 = (((gota - base.double()) - refa).abs() / (32 * 2.0 ** -24 * maga + 2.0 ** -23 * (base.double().abs() + refa.abs()) + 1e-300)).max().item()
    # exact transpose: <R x, g> == <x, R^T g>, each side within its element bounds of the same fp64 number
    lhs, rhs = (got * g64).sum().item(), (x64 * (gota - base.double())).sum().item()
    tol = 32 * 2.0 ** -24 * ((mag * g64.abs()).sum().item() + (maga * x64.abs()).sum().item()) + 2.0 ** -23 * ((base.double().abs() + refa.abs()) * x64).sum().item()
    print('resize %dx%d (%s): forward err / bound %.3f, adjoint err / bound %.3f, <Rx,g> - <x,RTg> = %.3g (tolerance %.3g)' % (h, w, dev, r1, r2, lhs - rhs, tol))
    assert r1 <= 1.0 and r2 <= 1.0 and abs(lhs - rhs) <= tol


# ------------------------------------------------------------------------------------------------------------------------------------ end to end
def measures(value, grad, v64, g64):
    """(relative value error, relative L2 error of the gradient, 1 - cosine)"""
    g, r = grad.double().reshape(-1), g64.double().reshape(-1)
    return (abs(float(value) - float(v64)) / abs(float(v64)), ((g - r).norm() / r.norm()).item(), 1.0 - (torch.dot(g, r) / (g.norm() * r.norm())).item())


_E2E = {}


def e2e_reference(widths, h, w, seed=0):
    """(weights, rgb, target, value64, grad64, E16 measures), computed once per shape and shared"""
    key = (tuple(widths), h, w, seed)
    if key not in _E2E:
        gen = torch.Generator().manual_seed(seed + 21)
        weights = alpips.synthetic_weights(widths, seed + 1)
        rgb, target = torch.rand(3, h, w, generator=gen), torch.rand(3, h, w, generator=gen)
        v64, g64 = R.value_and_grad(rgb, target, weights)
        v16, g16 = R.value_and_grad(rgb, target, weights, rounding=True)
        _E2E[key] = (weights, rgb, target, v64, g64, measures(v16, g16, v64, g64))
    return _E2E[key]


def check_e2e(lib, dev, widths, h, w, weight=1.0, seed=0):
    """aph_lpips_value_grad against the fp64 restatement, gated at 2 x E16 on each measure -> (E16, kernel) measures"""
    weights, rgb, target, v64, g64, e16 = e2e_reference(widths, h, w, seed)
    term = alpips.LPIPS(weights, h, w, device=dev, widths=widths, lib=lib)
    term.set_target(target.to(dev))
    d_rgb, d_w = rgb.to(dev).contiguous(), torch.full((1,), weight, device=dev)
    outs = []
    for _ in range(2):
        big, grad = banded(3 * h * w, torch.float32, dev)
        grad.zero_()
        loss = torch.zeros(1, device=dev)
        term.value_grad(d_rgb, d_w, loss, grad)
        sync(dev)
        assert_bands(big, 'aph_lpips_value_grad gradient')
        outs.append((loss.cpu().clone(), grad.cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'aph_lpips_value_grad: other bits on the second call'
    loss, grad = outs[0]
    assert bool(torch.isfinite(grad).all()) and math.isfinite(float(loss))
    # value only (no gradient buffer): the same value
    loss2 = torch.zeros(1, device=dev)
    term.value_grad(d_rgb, d_w, loss2, None)
    sync(dev)
    assert torch.equal(loss2.cpu(), loss)
    w32 = float(torch.tensor(weight, dtype=torch.float32))
    k = measures(float(loss) / w32, grad.double().view(3, h, w) / w32, v64, g64)
    print('lpips end to end %s %dx%d w=%g (%s): value %.6f (fp64 %.6f)' % ('x'.join(map(str, widths)), h, w, weight, dev, float(loss) / w32, float(v64)))
    print('   E16 (rounding model vs fp64): value %.3g  grad rel L2 %.3g  1-cos %.3g' % e16)
    print('   kernel vs fp64:               value %.3g  grad rel L2 %.3g  1-cos %.3g' % k)
    term.close()
    for name, a, b in zip(('value', 'gradient relative L2', 'gradient 1 - cosine'), k, e16):
        assert a <= 2.0 * b, '%s: kernel %.3g, 2 x E16 = %.3g' % (name, a, 2.0 * b)
    return e16, k


def check_dropin(lib, dev, widths, h, w, seed=0):
    """sim_loss(img, img_in, normalize=True) on half-size images: the value and the autograd gradient are aph_lpips_value_grad_half's, bit for
    bit, and that entry passes the 2 x E16 gate of its own rounding model (no resize on either side)"""
    weights = alpips.synthetic_weights(widths, seed + 1)
    gen = torch.Generator().manual_seed(seed + 31)
    hh, hw = h // 2, w // 2
    term = alpips.LPIPS(weights, h, w, device=dev, widths=widths, lib=lib)
    x, y = torch.rand(1, 3, hh, hw, generator=gen), torch.rand(1, 3, hh, hw, generator=gen)
    img, img_in = x.to(dev).requires_grad_(True), y.to(dev)
    loss = 0.5 * term(img, img_in, normalize=True)
    loss.backward()
    sync(dev)
    want_l, want_g = torch.zeros(1, device=dev), torch.zeros(3, hh, hw, device=dev)
    L_(lib).call('aph_lpips_value_grad_half', term.handle, ops.ptr(img.detach()), ops.ptr(term.one), ops.ptr(want_l), ops.ptr(want_g), ops._stream(want_g))
    sync(dev)
    assert torch.equal(loss.detach().cpu(), 0.5 * want_l[0].cpu()) and torch.equal(img.grad[0].cpu(), 0.5 * want_g.cpu())
    v64, g64 = R.value_and_grad(x[0], y[0], weights, resize=False)
    v16, g16 = R.value_and_grad(x[0], y[0], weights, rounding=True, resize=False)
    e16, k = measures(v16, g16, v64, g64), measures(float(want_l), want_g.cpu(), v64, g64)
    print('drop-in sim_loss %dx%d (%s): E16 %.3g %.3g %.3g   kernel %.3g %.3g %.3g' % ((hh, hw, dev) + e16 + k))
    for name, a, b in zip(('value', 'gradient relative L2', 'gradient 1 - cosine'), k, e16):
        assert a <= 2.0 * b, '%s: kernel %.3g, 2 x E16 = %.3g' % (name, a, 2.0 * b)
    with _raises(NotImplementedError):
        term(img, img_in, normalize=False)
    with _raises(ValueError):
        term(img[..., :-1], img_in[..., :-1])
    term.close()


class _raises:
    def __init__(self, exc):
        self.exc = exc

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None and issubclass(et, self.exc), 'expected %s' % self.exc.__name__
        return True


# -------------------------------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, dev):
    """create refusals and hook argument checks: the error code and the call's name, nothing launched (the output keeps its sentinel)"""
    lb = L_(lib)
    c = lb.cdll
    h = c_void_p()
    assert c.aph_lpips_create((c_int * 5)(64, 128, 250, 512, 512), 64, 64, byref(h)) == -3 and 'aph_lpips_create' in lb.last_error()
    assert c.aph_lpips_create((c_int * 5)(*FULL), 31, 64, byref(h)) == -3 and 'aph_lpips_create' in lb.last_error()
    assert c.aph_lpips_create((c_int * 5)(*FULL), 64, 30, byref(h)) == -3
    assert c.aph_lpips_create((c_int * 5)(*FULL), 64, 64, None) == -1
    assert not h.value
    assert c.aph_lpips_create((c_int * 5)(*NARROW), 33, 32, byref(h)) == 0 and h.value
    one = torch.zeros(8, dtype=torch.float32)
    assert c.aph_lpips_set_weight(h, b'features.1.weight', c_void_p(one.data_ptr()), 8) == -1 and 'unknown key' in lb.last_error()
    assert c.aph_lpips_set_weight(h, b'features.0.weight', c_void_p(one.data_ptr()), 8) == -1 and 'expected 432' in lb.last_error()
    assert c.aph_lpips_set_weight(h, b'lin4.weight', c_void_p(one.data_ptr()), 8) == -1 and 'expected 32' in lb.last_error()
    out = V.sentinel(1, 3 * 33 * 32, torch.float32, dev)
    img = torch.zeros(3, 33, 32, device=dev)
    w1 = torch.ones(1, device=dev)
    # weights not loaded, then no target: refused before anything is launched
    assert c.aph_lpips_set_target(h, ops.ptr(img), 33, 32, None) == -1 and 'not fully loaded' in lb.last_error()
    assert c.aph_lpips_value_grad(h, ops.ptr(img), ops.ptr(w1), None, ops.ptr(out), None) == -1 and 'aph_lpips_value_grad' in lb.last_error()
    for name, t in alpips.synthetic_weights(NARROW, 0).items():
        assert c.aph_lpips_set_weight(h, name.encode(), c_void_p(t.contiguous().data_ptr()), t.numel()) == 0, name
    assert c.aph_lpips_value_grad(h, ops.ptr(img), ops.ptr(w1), None, ops.ptr(out), None) == -1 and 'no target' in lb.last_error()
    assert c.aph_lpips_set_target(h, ops.ptr(img), 20, 20, None) == -1 and 'aph_lpips_set_target' in lb.last_error()
    sync(dev)
    V.assert_untouched(out, torch.zeros(out.shape, dtype=torch.bool), 'refused aph_lpips_value_grad')
    assert c.aph_lpips_destroy(h) == 0
    buf = V.sentinel(1, 4096, torch.float16, dev)
    p = ops.ptr(buf)
    assert c.aph_lpips_conv_test(p, 4, 4, 12, p, 16, None, 1, None, p, None, 0, 0, None) == -1 and 'aph_lpips_conv_test' in lb.last_error()
    assert c.aph_lpips_conv_test(p, 4, 4, 8, p, 24, None, 1, None, p, None, 0, 0, None) == -1
    assert c.aph_lpips_conv_test(p, 4, 4, 8, p, 16, None, 1, None, p, None, 0, 3, None) == -1
    assert c.aph_lpips_pool_test(p, 4, 4, 12, p, None, None, None) == -1 and 'aph_lpips_pool_test' in lb.last_error()
    assert c.aph_lpips_resize_test(p, 2, 8, p, 0, None) == -1 and 'aph_lpips_resize_test' in lb.last_error()
    sync(dev)
    V.assert_untouched(buf, torch.zeros(buf.shape, dtype=torch.bool), 'refused test entries')


# ---------------------------------------------------------------------------------------------------------------------------------------- engine
def ulp32(x):
    return float(torch.nextafter(torch.tensor(abs(x), dtype=torch.float32), torch.tensor(float('inf'))) - torch.tensor(abs(x), dtype=torch.float32))


def record_calls(lib, fn):
    """run fn() with every checked C-ABI call of `lib` recorded -> the list of entry names, in order"""
    names, orig = [], lib.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    lib.call = call
    try:
        fn()
    finally:
        del lib.call
    return names


def check_engine(lib, dev, model, widths, h, w, S, use_graph):
    """Engine(sync=term) against Engine(sync=None) from one state and one crop table.
    1. real learning rate, weight 0 on every step (two eager steps, then the captured step where use_graph): parameters and loss stay
       bit-identical to the term-off engine -- the term at weight 0 adds exact zeros, in eager launches and in replays;
    2. learning rate 0 (the state stands still), weights 1, 0.5, 0 on consecutive steps: loss - loss_off == fl(w * value) within one fp32 ulp
       of the loss, value = the stand-alone aph_lpips_value_grad on the step's image; the 0.5 step proves that a replay reads the weight of
       ITS step from the device; the 0 step gives loss_off's bits."""
    from aphantasia_amd.engine import Engine
    from oracle import reference_path as O
    lb = L_(lib)
    gen = torch.Generator().manual_seed(41)
    term = alpips.LPIPS(alpips.synthetic_weights(widths, 2), h, w, device=dev, widths=widths, lib=lib)
    term.set_target(torch.rand(3, h, w, generator=gen).to(dev))
    torch.manual_seed(0)
    p0 = O.fft_params_init([1, 3, h, w]).contiguous()
    target = torch.randn(1, model.visual.output_dim, generator=torch.Generator().manual_seed(2))
    size = model.visual.input_resolution
    torch.manual_seed(123)
    tb = O.draw_crop_table(S, size, h, w, 'uniform', 0.4)
    kw = dict(sim='mix', macro=0.4, lib=lib, use_graph=use_graph)
    on = Engine(p0.clone().to(dev).contiguous(), h, w, model, S, [(target, -1.0)], sync=term, **kw)
    off = Engine(p0.clone().to(dev).contiguous(), h, w, model, S, [(target, -1.0)], **kw)
    assert 'sync' in on.inputs.views and 'sync' not in off.inputs.views
    assert [l[:2] for l in off.inputs.layout] == [l[:2] for l in on.inputs.layout[:-1]], 'the sync part moved an existing step input'
    for i in range(4):
        l_on, l_off = float(on.step(tb, sync_weight=0.0)), float(off.step(tb))
        sync(dev)
        assert l_on == l_off and torch.equal(on.params, off.params), 'step %d at weight 0 differs from the term-off engine' % i
    if use_graph:
        assert on._graph is not None and off._graph is not None, 'the step was not captured'
    want_off = float(off.step(tb, lr=0.0))
    for wgt in (1.0, 0.5, 0.0):
        got = float(on.step(tb, lr=0.0, sync_weight=wgt))
        sync(dev)
        assert torch.equal(on.params, off.params), 'a step at learning rate 0 moved the parameters'
        val = torch.zeros(1, device=dev)
        term.value_grad(on.rgb, term.one, val, None)
        sync(dev)
        v = float(val)
        term_got, term_want = got - want_off, float(torch.tensor(wgt, dtype=torch.float32) * torch.tensor(v, dtype=torch.float32))
        print('engine (%s, graph %s) w=%g: loss %.7f, without the term %.7f, difference %.7g, w * value %.7g' % (dev, use_graph, wgt, got, want_off, term_got, term_want))
        assert v > 0 and abs(term_got - term_want) <= ulp32(got), (wgt, term_got, term_want, ulp32(got))
        if wgt == 0.0:
            assert got == want_off
    with _raises(ValueError):
        off.step(tb, sync_weight=1.0)
    with _raises(ValueError):
        Engine(p0.clone().to(dev).contiguous(), h + 2, w, model, S, [(target, -1.0)], sync=term, **kw)
    term.close()


# The C-ABI calls of one step of an engine built WITHOUT the term (40 x 56 frame, 5 cuts, --sharp on), recorded on the parent commit
# d115a0a ("ViT and text towers: one weight store, one arena path, named LN args") with lpips_checks.engine_call_sequence's recipe.
PARENT_STEP_CALLS = ['aph_synth_fft_fwd', 'aph_sample_fwd_tf', 'aph_vit_forward', 'aph_sim_loss', 'aph_vit_backward', 'aph_sample_bwd_tf', 'aph_rgb_sharp',
                     'aph_synth_fft_bwd', 'aph_adam_step_guarded']


def engine_call_sequence(lib, dev, model, h, w, S):
    """the C-ABI calls of one eager step of an engine built without the term"""
    from aphantasia_amd.engine import Engine
    from oracle import reference_path as O
    torch.manual_seed(0)
    p0 = O.fft_params_init([1, 3, h, w]).contiguous()
    target = torch.randn(1, model.visual.output_dim, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(123)
    tb = O.draw_crop_table(S, model.visual.input_resolution, h, w, 'uniform', 0.4)
    eng = Engine(p0.to(dev).contiguous(), h, w, model, S, [(target, -1.0)], sim='mix', macro=0.4, lib=lib, use_graph=False, sharp=0.3)
    eng.step(tb)
    return record_calls(L_(lib), lambda: eng.step(tb))
