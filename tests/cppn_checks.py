"""Checks of the CPPN generator (csrc/synth_cppn.h: aph_cppn_fwd / aph_cppn_bwd) shared by the interpreter tests (test_emu_cppn.py) and the GPU
tests (test_gpu_cppn.py).  `lib` = a loaded C-ABI library (the interpreter build) or None (the product), `dev` = where its tensors live.

`net_forward` is a torch restatement of the network (cppn.py:71-116) that takes a dtype.  tests/golden/cppn_ref.npz (tools/make_cppn_golden.py:
the reference's own classes) pins it in float64, image and gradient, to 1e-12; the checks below use it for the fp64 truth at every shape.

Tolerance: per case, the kernel's max |img - img64| and max |grad - grad64| / max |grad64| must each be <= MARGIN x the same figure of the
restatement evaluated in float32 on this CPU.  Both are f32 evaluations of one expression; they differ in summation order and in atanf (device
library against libm).  A factor of 4 covers that, and a wrong tap or layout does not fit in it.  Every element is compared."""
import math

import numpy as np
import torch

from aphantasia_amd import _ffi, ops
from aphantasia_amd.cppn import ACTS, CPPNSynth, layer_table
import vit_component_checks as V

MARGIN = 4.0
BAND = 1024             # canary floats on either side of the workspace and of every output (4 KB)

# (H, W, layers, nf, act, gscale, runs under the interpreter too)
CASES = [
    (3, 5, 1, 8, 'unbias', 1.0, True),            # fewer pixels than one tile, no hidden layer
    (23, 37, 3, 8, 'unbias', 1.0, True),          # ragged tile tail
    (23, 37, 2, 5, 'comp', 0.5, True),            # nf below and off the MFMA tile; gscale != 1
    (40, 56, 10, 24, 'unbias', 1.0, True),        # the default net
    (40, 56, 10, 24, 'comp', 1.0, True),
    (40, 56, 10, 24, 'relu', 1.0, True),
    (31, 33, 12, 32, 'unbias', 1.0, True),        # both limits
    (97, 131, 4, 20, 'unbias', 1.0, True),        # many workgroups (the second-stage reduction has real work), odd pixel count
    (128, 160, 10, 24, 'unbias', 1.0, False),     # GPU only
]


def case_id(c):
    return '%dx%d-l%d-nf%d-%s' % c[:5]


def activation(z, actfn):
    if actfn == 'relu':
        return (torch.relu(z) - 0.40) / 0.58
    t = torch.atan(z)
    return torch.cat([t / 0.67, (t * t - 0.45) / 0.396 if actfn == 'unbias' else (t * t) / 0.6], 0)


def net_forward(views, xs, ys, actfn, dtype):
    """views: [w0, b0, w1, b1, ...] (weights [out, in, 1, 1]); xs [W], ys [H] -> rgb [3, H, W] in `dtype`"""
    h, w = ys.numel(), xs.numel()
    x = torch.stack([xs.to(dtype)[None, :].expand(h, w), ys.to(dtype)[:, None].expand(h, w)])
    n = len(views) // 2
    for j in range(n):
        z = torch.einsum('oi,ihw->ohw', views[2 * j].to(dtype).reshape(views[2 * j].shape[0], -1), x) + views[2 * j + 1].to(dtype)[:, None, None]
        x = torch.sigmoid(z) if j == n - 1 else activation(z, actfn)
    return x


def net_image_and_grad(views, xs, ys, actfn, d_rgb, dtype):
    """-> (rgb, [gradient of sum(rgb * d_rgb) per view]) evaluated in `dtype`, returned as float64"""
    leaves = [v.detach().to(dtype).clone().requires_grad_(True) for v in views]
    img = net_forward(leaves, xs, ys, actfn, dtype)
    (img * d_rgb.to(dtype)).sum().backward()
    return img.detach().double(), [v.grad.double() for v in leaves]


def random_views(layers, nf, actfn, gen):
    """weights and biases with the reference's distributions, from a generator of the test's own"""
    views = []
    for i, o in layer_table(layers, nf, actfn):
        views += [torch.randn(o, i, 1, 1, generator=gen) * math.sqrt(1. / i), torch.rand(o, generator=gen) - 0.5]
    return views


def banded(n, dev):
    """(whole buffer, NaN-prefilled view of n floats between two canary bands)"""
    big = V.sentinel(1, n + 2 * BAND, torch.float32, dev).reshape(-1)
    view = big[BAND:BAND + n]
    view.fill_(float('nan'))
    return big, view


def assert_bands(big, what):
    b = V.bits(big)
    assert bool((b[:BAND] == V.SENT32).all()) and bool((b[-BAND:] == V.SENT32).all()), '%s: a store outside the buffer' % what


def flat_of(views):
    return torch.cat([v.reshape(-1) for v in views]).float().contiguous()


def gaps(img, grads, img64, g64):
    """(max |img - img64|, max |grad - grad64| / max |grad64|) with NaN / inf -> inf"""
    gi = (img.double() - img64).abs().nan_to_num(float('inf')).max().item()
    ref = torch.cat([g.reshape(-1) for g in g64])
    got = torch.cat([g.reshape(-1) for g in grads]).double()
    return gi, (got - ref).abs().nan_to_num(float('inf')).max().item() / ref.abs().max().item()


def check_fp64(lib, dev, h, w, layers, nf, actfn, gscale=1.0, seed=0):
    """forward and backward against fp64, the stash, determinism and the workspace bounds of one case -> its figures"""
    gen = torch.Generator().manual_seed(seed + 17)
    views = random_views(layers, nf, actfn, gen)
    syn = CPPNSynth(h, w, layers, nf, actfn, dev, lib=lib)
    assert [tuple(v.shape) for v in views] == list(syn.shapes)
    d_rgb = torch.randn(3, h, w, generator=gen) / (h * w)
    xs, ys = syn.xs.cpu(), syn.ys.cpu()
    img64, g64 = net_image_and_grad(views, xs, ys, actfn, d_rgb * gscale, torch.float64)
    img32, g32 = net_image_and_grad(views, xs, ys, actfn, d_rgb * gscale, torch.float32)
    gap_img, gap_grad = gaps(img32, g32, img64, g64)

    flat = flat_of(views).to(dev)
    d_rgb_d = d_rgb.to(dev).contiguous()
    ws_big, ws = banded(syn.ws.numel(), dev)
    rgb_big, rgb = banded(3 * h * w, dev)
    syn.forward(flat, out=rgb, ws=ws)
    assert_bands(rgb_big, 'aph_cppn_fwd rgb')
    assert not bool(torch.isnan(rgb).any()), 'aph_cppn_fwd: %d pixels never written (or NaN)' % int(torch.isnan(rgb).sum())
    # the stash changes nothing in the image
    rgb2_big, rgb2 = banded(3 * h * w, dev)
    syn.forward(flat, out=rgb2, stash=False)
    assert_bands(rgb2_big, 'aph_cppn_fwd rgb (no stash)')
    assert torch.equal(rgb, rgb2), 'aph_cppn_fwd: other bits without the stash'
    # backward twice: the same bits
    grads = []
    for k in range(2):
        g_big, g = banded(syn.numel, dev)
        syn.backward(flat, d_rgb_d, g, rgb=rgb, gscale=gscale, ws=ws)
        assert_bands(g_big, 'aph_cppn_bwd grad')
        assert not bool(torch.isnan(g).any()), 'aph_cppn_bwd: %d elements never written (or NaN)' % int(torch.isnan(g).sum())
        grads.append(g)
    assert torch.equal(grads[0], grads[1]), 'aph_cppn_bwd: other bits on the second launch'
    assert_bands(ws_big, 'workspace after forward + backward')
    k_img, k_grad = gaps(rgb.cpu().view(3, h, w), [v.cpu() for v in syn.views(grads[0])], img64, g64)
    out = dict(gap_img=gap_img, gap_grad=gap_grad, k_img=k_img, k_grad=k_grad)
    print('cppn %dx%d l%d nf%d %s (%s): image kernel %.3g / f32 %.3g   gradient kernel %.3g / f32 %.3g' %
          (h, w, layers, nf, actfn, dev, k_img, gap_img, k_grad, gap_grad))
    assert k_img <= MARGIN * gap_img, 'image: max err %.3g, torch f32 %.3g' % (k_img, gap_img)
    assert k_grad <= MARGIN * gap_grad, 'gradient: max err / max |grad| %.3g, torch f32 %.3g' % (k_grad, gap_grad)
    return out


def check_refusals(lib, dev):
    """out-of-range shapes and null pointers: -1 / -3 with the call's name, before any device work (the pointers are never dereferenced)"""
    L_ = lib if lib is not None else _ffi.lib()
    c = L_.cdll
    one = torch.zeros(64, device=dev)
    p, z = ops.ptr(one), None
    st = ops._stream(one)

    def fwd(layers=2, nf=8, act=0, params=p, rgb=p, H=2, W=2):
        return c.aph_cppn_fwd(params, layers, nf, act, p, p, H, W, z, rgb, st)

    def bwd(layers=2, nf=8, act=0, params=p, rgb=p, ws=p, H=2, W=2):
        return c.aph_cppn_bwd(params, layers, nf, act, p, p, H, W, p, 1.0, rgb, ws, p, st)
    for name, call in (('aph_cppn_fwd', fwd), ('aph_cppn_bwd', bwd)):
        for kw, code in ((dict(layers=0), -3), (dict(layers=13), -3), (dict(nf=0), -3), (dict(nf=33), -3), (dict(act=3), -3),
                         (dict(params=z), -1), (dict(rgb=z), -1), (dict(H=0), -1)):
            assert call(**kw) == code, (name, kw)
            assert name in L_.last_error(), (name, kw, L_.last_error())
    assert bwd(ws=z) == -1 and 'aph_cppn_bwd' in L_.last_error()
    assert c.aph_cppn_param_count(10, 24, 0) == 10803
    assert c.aph_cppn_param_count(13, 24, 0) == 0 and c.aph_cppn_ws_bytes(10, 33, 0, 8, 8) == 0


# ------------------------------------------------------------------------------------------------------------------------ fused engine
ENGINE_NET = (4, 12, 'unbias')          # a hidden stack, nf off the 8-channel k-step group


def reference_loop(views0, xs, ys, actfn, encode, target, tables, size, lr, dtype):
    """the reference's train(i) (cppn.py:268-297) composed from the restatement and the oracle's sampler, loss and optimiser, free-running
    over `tables` -> (loss per step, the first step's gradient per view as float64)"""
    from oracle import reference_path as R
    leaves = [v.detach().to(dtype).clone().requires_grad_(True) for v in views0]
    opt = R.make_optimizer(leaves, 'adam', lr)
    losses, first = [], None
    for tb in tables:
        img = net_forward(leaves, xs, ys, actfn, dtype)[None]
        enc = encode(R.slice_imgs(img, tb, size, 'uniform'))
        loss = -1.0 * R.sim_func(target.to(dtype), enc, None)
        opt.zero_grad()
        loss.backward()
        if first is None:
            first = [v.grad.double().clone() for v in leaves]
        opt.step()
        losses.append(float(loss.detach()))
    return losses, first


def check_engine(lib, dev, model, weights, cfg, h, w, S, steps, use_graph):
    """Engine(param_kind='cppn', optimizer='adam', lr 0.003, exact ViT) free-running for `steps` against the torch loop above in float32: loss
    within 1e-3 on every step; the first step's eng.grad against the same loop in float64 within MARGIN x the float32 loop's own gap.
    -> the engine (after the last step)"""
    from aphantasia_amd.cppn import cppn_image
    from aphantasia_amd.engine import Engine
    from oracle import reference_path as R
    from oracle import clip_vit_ref
    layers, nf, actfn = ENGINE_NET
    size = cfg['input_resolution']
    macro = 0.4 if min(h, w) >= size else 1.0        # a frame below the cut size: every cut from 0.9 .. 1 of the short side (utils.py:243), inside the frame
    torch.manual_seed(5)
    params, gen, _ = cppn_image([1, 3, h, w], layers, nf, actfn, device=dev, lib=lib)
    views0 = [p.detach().cpu().clone() for p in params]
    target = torch.randn(1, cfg['output_dim'], generator=torch.Generator().manual_seed(2))
    eng = Engine(gen.flat, h, w, model, S, [(target, -1.0)], sim='cossim', optimizer='adam', lr=0.003, macro=macro, lib=lib, exact=True,
                 use_graph=use_graph, param_kind='cppn', cppn=gen.synth)
    torch.manual_seed(123)
    tables = [R.draw_crop_table(S, size, h, w, 'uniform', macro) for _ in range(steps)]
    xs, ys = gen.synth.xs.cpu(), gen.synth.ys.cpu()
    w64 = {k: v.double() for k, v in weights.items()}
    want, g32 = reference_loop(views0, xs, ys, actfn, lambda x: clip_vit_ref.encode_image(weights, x, cfg), target, tables, size, 0.003, torch.float32)
    _, g64 = reference_loop(views0, xs, ys, actfn, lambda x: clip_vit_ref.encode_image(w64, x, cfg), target, tables[:1], size, 0.003, torch.float64)
    for i, tb in enumerate(tables):
        got = float(eng.step(tb))
        if i == 0:
            grad = [v.cpu() for v in gen.synth.views(eng.grad.detach().clone())]
        print('cppn engine step %d (%s): loss %.6f, torch f32 loop %.6f' % (i, dev, got, want[i]))
        assert abs(got - want[i]) < 1e-3, (i, got, want[i])
    ref = torch.cat([g.reshape(-1) for g in g64])
    gap = (torch.cat([g.reshape(-1) for g in g32]) - ref).abs().max().item() / ref.abs().max().item()
    k = (torch.cat([g.reshape(-1) for g in grad]).double() - ref).abs().nan_to_num(float('inf')).max().item() / ref.abs().max().item()
    print('cppn engine first gradient (%s): kernel %.3g / f32 %.3g of max |grad64|' % (dev, k, gap))
    assert k <= MARGIN * gap, 'first gradient: max err / max |grad| %.3g, torch f32 %.3g' % (k, gap)
    return eng, gen
