"""Checks of the ViT-L/14 ground: the T = 257 .. 320 attention kernels, the window patchify pair of 14-pixel patches (padded patch rows), the
tower with such rows and at width 1024, and whole engine steps on a 14-pixel model.  Shared by the interpreter tests (test_emu_vitl.py) and
the GPU tests (test_gpu_vitl.py): `lib` = a loaded C-ABI library (the interpreter build) or None (the product), `dev` = where tensors live."""
import numpy as np
import torch

from aphantasia_amd import _ffi, ops
from aphantasia_amd.weights import synthetic_visual_weights
from oracle import reference_path as R
from oracle import augment_ref, clip_vit_ref
import kernel_checks as K
import vit_component_checks as V

KEYS = ('input_resolution', 'patch_size', 'width', 'layers', 'heads', 'output_dim')


def cfg_of(*v):
    return dict(zip(KEYS, v))


TINY14 = cfg_of(28, 14, 256, 2, 4, 128)            # T = 5, padded patch rows (588 -> 640)
T257 = cfg_of(224, 14, 256, 1, 4, 128)             # T = 257: the five-block attention inside the tower
W1024 = cfg_of(56, 14, 1024, 2, 16, 768)           # width 1024, 16 heads, output_dim 768
ATTN_T = (257, 258, 272, 273, 288, 289, 305, 320)  # first row of the fifth block, 16-row tile edges, the 32-key block edge, the full case
WIN_CASES = ((14, 28, 28), (14, 28, 36), (14, 224, 232))      # (patch, R, R_src)


def _lib(lib):
    return lib if lib is not None else _ffi.lib()


# ------------------------------------------------------------------------------------------------------------------------- attention
def check_attention_refused(lib, dev, T=321, S=1, heads=2):
    """one token past the blocked kernels' limit: aph_attn_test refuses both modes and leaves every output element a sentinel"""
    L = _lib(lib)
    D, M = heads * 64, S * T
    qkv, datt = V.attn_inputs('normal', S, T, heads)
    qkv, datt = qkv.to(dev), datt.to(dev)
    att, lse, dq = V.sentinel(M, D, torch.float16, dev), V.sentinel(1, S * heads * T, torch.float32, dev), V.sentinel(M, 3 * D, torch.float16, dev)
    for mode in (0, 1):
        rc = L.cdll.aph_attn_test(ops.ptr(qkv), ops.ptr(att), ops.ptr(lse), ops.ptr(datt), None, ops.ptr(dq), S, T, heads, mode, ops._stream(qkv))
        assert rc < 0 and 'aph_attn_test' in L.last_error(), (mode, rc, L.last_error())
    if dev != 'cpu':
        torch.cuda.synchronize()
    for name, t in (('att', att), ('lse', lse), ('dqkv', dq)):
        V.assert_untouched(t, torch.zeros(t.shape, dtype=torch.bool), 'refused T=%d (%s)' % (T, name))


# ------------------------------------------------------------------------------------------------------------------------- patchify
def patch_index_ref(S, R_src, R, patch):
    """index restatement: for every element of the padded patch rows [S (R/patch)^2, Kp] the flat index into [S,3,R_src,R_src] it copies
    (k = (iy patch + ix) 3 + c), -1 in the pad columns"""
    g, kp, k3 = R // patch, ops.patch_row_elems(patch), 3 * patch * patch
    row = torch.arange(S * g * g).view(-1, 1)
    k = torch.arange(kp).view(1, -1)
    s, pr = row // (g * g), row % (g * g)
    py, px = pr // g, pr % g
    pix, c = k // 3, k % 3
    iy, ix = pix // patch, pix % patch
    idx = ((s * 3 + c) * R_src + (py * patch + iy)) * R_src + (px * patch + ix)
    return torch.where(k < k3, idx, torch.full_like(idx, -1))


def check_patchify_win(lib, dev, patch, R, R_src, S=2, seed=0):
    """aph_patchify_f16_win / aph_unpatchify_f32_win against the index restatement, bit for bit: the output starts as NaN sentinels (the pad
    columns must come out exactly zero), the guard rows behind it keep them; the adjoint writes exact zeros outside the window, every
    element of its output, and does not read the pad columns (they hold NaN)"""
    L = _lib(lib)
    what = 'patchify_win patch=%d R=%d R_src=%d' % (patch, R, R_src)
    gen = torch.Generator().manual_seed(seed)
    g, kp, k3, G = R // patch, ops.patch_row_elems(patch), 3 * patch * patch, V.GUARD_ROWS
    rows = S * g * g
    idx = patch_index_ref(S, R_src, R, patch)
    x = torch.randn(S, 3, R_src, R_src, generator=gen) * 3
    want = torch.where(idx >= 0, x.reshape(-1)[idx.clamp(min=0)], torch.zeros(())).half()
    out = V.sentinel(rows + G, kp, torch.float16, dev)
    xd = x.clone().to(dev)
    st = ops._stream(xd)
    for _ in range(2):                                  # the buffer is reused: the second call finds values, not sentinels, and gives the same
        L.call('aph_patchify_f16_win', ops.ptr(xd), S, R_src, R, patch, ops.ptr(out), st)
        got = out.cpu()
        assert torch.equal(V.bits(got[:rows]), V.bits(want)), what
        assert kp == k3 or (got[:rows, k3:] == 0).all() and not torch.signbit(got[:rows, k3:].float()).any(), what + ': pad columns'
    written = torch.zeros(rows + G, kp, dtype=torch.bool)
    written[:rows] = True
    V.assert_untouched(got, written, what)
    assert torch.equal(xd.cpu(), x), what + ': input changed'
    assert torch.equal(V.bits(ops.patchify(xd, patch, lib=lib, R=R).cpu()), V.bits(want)), what + ' (ops.patchify)'
    # the adjoint
    gp = torch.randn(rows, kp, generator=gen)
    gp[:, k3:] = float('nan')
    gscale = 0.37
    n = S * 3 * R_src * R_src
    want_g = torch.zeros(n)
    live = idx >= 0
    want_g[idx[live]] = gp[live] * torch.tensor(gscale, dtype=torch.float32)
    gout = V.sentinel(1, n + G, torch.float32, dev)
    gd = gp.clone().to(dev)
    L.call('aph_unpatchify_f32_win', ops.ptr(gd), S, R_src, R, patch, gscale, ops.ptr(gout), st)
    gg = gout.cpu()
    assert torch.equal(V.bits(gg[0, :n]), V.bits(want_g)), what + ' (adjoint)'
    outside = torch.ones(S, 3, R_src, R_src, dtype=torch.bool)
    outside[:, :, :R, :R] = False
    assert (V.bits(gg[0, :n]).view(S, 3, R_src, R_src)[outside] == 0).all(), what + ': not +0 outside the window'
    written = torch.zeros(1, n + G, dtype=torch.bool)
    written[0, :n] = True
    V.assert_untouched(gg, written, what + ' (adjoint)')
    assert torch.equal(V.bits(ops.unpatchify(gd, S, R, patch, gscale, lib=lib, R_src=R_src).cpu().reshape(-1)), V.bits(want_g)), what + ' (ops.unpatchify)'


def check_patchify_win_matches_pow2(lib, dev, patch, R=64, S=2):
    """patch 16 / 32 with R_src = R: the same bits as aph_patchify_f16 / aph_unpatchify_f32 (rows of 3 patch^2: no pad columns)"""
    L = _lib(lib)
    assert ops.patch_row_elems(patch) == 3 * patch * patch
    gen = torch.Generator().manual_seed(patch)
    x = (torch.randn(S, 3, R, R, generator=gen) * 3).to(dev)
    a = ops.patchify(x, patch, lib=lib)
    b = torch.empty_like(a)
    L.call('aph_patchify_f16_win', ops.ptr(x), S, R, R, patch, ops.ptr(b), ops._stream(x))
    assert torch.equal(V.bits(a), V.bits(b)), patch
    gp = torch.randn(a.shape, generator=gen).to(dev)
    ga = ops.unpatchify(gp, S, R, patch, 0.37, lib=lib)
    gb = torch.empty_like(ga)
    L.call('aph_unpatchify_f32_win', ops.ptr(gp), S, R, R, patch, 0.37, ops.ptr(gb), ops._stream(x))
    assert torch.equal(V.bits(ga), V.bits(gb)), patch


# ------------------------------------------------------------------------------------------------------------------------- the tower
def check_tower(lib, dev, cfg, S, check_fuse=False, pad=True):
    """kernel_checks.check_vit at its own tolerances, then (pad) the pad columns of the patch gradient after a backward: exactly zero"""
    ferr, berr = K.check_vit(lib, dev, cfg, S=S, check_fuse=check_fuse)
    print('%s S=%d: forward max-rel %.2e, input-gradient max-rel %.2e' % (tuple(cfg.values()), S, ferr, berr))
    if pad:
        check_pad_gradient(lib, dev, cfg, S)
    return ferr, berr


def check_pad_gradient(lib, dev, cfg, S, w=None):
    w = synthetic_visual_weights(cfg, 3) if w is None else w
    p, Rr = cfg['patch_size'], cfg['input_resolution']
    vit = ops.VitHandle(cfg, w, max_batch=S, lib=lib)
    assert vit.padded and vit.Kp == ops.patch_row_elems(p) > 3 * p * p
    x = torch.randn(S, 3, Rr, Rr, generator=torch.Generator().manual_seed(1)).to(dev)
    vit.forward(ops.patchify(x, p, lib=lib), S)
    gp = V.sentinel(S * vit.P, vit.Kp, torch.float32, dev)
    genc = (torch.randn(S, cfg['output_dim'], generator=torch.Generator().manual_seed(2)) * 0.01 * 1024).to(dev)
    vit.backward(genc, S, out=gp, out_scale=1.0 / 1024)
    gp = gp.cpu()
    assert torch.isfinite(gp).all() and gp[:, :3 * p * p].abs().max() > 0
    assert (V.bits(gp[:, 3 * p * p:]) == 0).all(), 'pad columns of the patch gradient are not exactly +0'


# ------------------------------------------------------------------------------------------------------------------------- whole steps
H, W, S_CUTS = 40, 56, 5


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)


def tiny14_model(lib, S=S_CUTS, cfg=TINY14):
    from aphantasia_amd.clip import CLIPModel
    w = synthetic_visual_weights(cfg, 3)
    return CLIPModel('tiny14', cfg, w, None, max_batch=S, lib=lib), w


def check_step(lib, dev, tf, steps, use_graph, cfg=TINY14):
    """`steps` free-running steps of an Engine on the 14-pixel tiny model against oracle.reference_path.ReferenceRun, with the comparison
    and tolerances tests/test_engine_emu.py / tests/test_gpu_step.py / tf_checks.check_engine apply to their TINY config: per-step
    |d loss| < 1e-3, final image RMS < 2e-2.  tf: 'none', 'fast' or 'custom' (the canvas-window path)."""
    from aphantasia_amd import transforms
    from aphantasia_amd.engine import Engine
    from aphantasia_amd.utils import draw_crop_params
    import tf_checks
    model, w = tiny14_model(lib, cfg=cfg)
    n = cfg['input_resolution']
    if tf == 'custom':
        eng = tf_checks.check_engine(lib, dev, model, w, cfg, 'custom', H, W, S_CUTS, steps, use_graph)
    else:
        trf = transforms.normalize() if tf == 'none' else transforms.transforms_fast
        seed_all(0)
        params = R.fft_params_init([1, 3, H, W]).contiguous()
        target = torch.randn(1, cfg['output_dim'], generator=torch.Generator().manual_seed(2))
        eng = Engine(params.to(dev).contiguous(), H, W, model, S_CUTS, [(target, -1.0)], sim='mix', macro=0.4, transform=trf, lib=lib,
                     use_graph=use_graph, rng='reference')
        run = R.ReferenceRun(H, W, lambda x: clip_vit_ref.encode_image(w, x, cfg), [(target, 1.0)], size=n, params=params.clone())
        seed_all(123)
        for i in range(steps):
            table, augs = draw_crop_params(S_CUTS, n, H, W, 'uniform', 0.4, trf if tf == 'fast' else None)
            per_cut = None if augs is None else (lambda c, cut, augs=augs: augment_ref.apply_fast(cut, augs[c], R.normalize))
            want = run.step(table, per_cut)
            got = float(eng.step(table, augs))
            print('-tf %s step %d: loss %.6f, oracle %.6f' % (tf, i, got, want))
            assert abs(got - want) < 1e-3, (tf, i, got, want)
        with torch.no_grad():
            img = run.image(1.1)[0]
        rms = (eng.synthesize(1.1).cpu() - img).pow(2).mean().sqrt().item()
        assert rms < 2e-2, rms
    assert eng.win and eng.patches.shape[1] == 640
    if use_graph:
        assert eng._graph is not None, 'the step was not captured'
    return eng


# ------------------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, dev):
    """the exact, split-precision and f16-gradient paths on a 14-pixel model: refused by the C ABI (APH_ERR_UNSUPPORTED, -3) and by the Engine,
    with messages that name the call; the default path of the same handle keeps working"""
    import pytest
    from aphantasia_amd.engine import Engine
    L = _lib(lib)
    model, w = tiny14_model(lib)
    vit = model.visual.handle
    for call in ('aph_vit_enable_f32', 'aph_vit_enable_hilo'):
        rc = getattr(L.cdll, call)(vit.handle)
        assert rc == -3 and call in L.last_error() and 'patch 14' in L.last_error(), (call, rc, L.last_error())
    with pytest.raises(RuntimeError, match='aph_vit_enable_f32'):
        vit.enable_f32()
    with pytest.raises(RuntimeError, match='aph_vit_enable_hilo'):
        vit.enable_hilo()
    params = R.fft_params_init([1, 3, H, W]).contiguous().to(dev)
    target = torch.randn(1, 128)
    for flag in ('exact', 'precise', 'grad_f16'):
        with pytest.raises(NotImplementedError, match=r'Engine\(%s=True\)' % flag):
            Engine(params, H, W, model, S_CUTS, [(target, -1.0)], lib=lib, **{flag: True})
    assert vit.workspace_bytes() > 0 and model.visual.handle is vit          # (no arena was added, no handle re-created)
    # a power-of-two patch whose rows would need padding (3 * 8^2 = 192) has no padded form -- the sampler's patch-major layouts write
    # 3 patch^2 elements a row -- and stays refused by aph_vit_create, as before; so does a power-of-two-patch tower of 257 tokens
    import ctypes
    for res, patch in ((64, 8), (32, 4), (256, 16)):
        h = ctypes.c_void_p()
        rc = L.cdll.aph_vit_create(res, patch, 256, 1, 4, 128, 1, ctypes.byref(h))
        assert rc == -3 and not h.value and 'aph_vit_create' in L.last_error(), (res, patch, rc, L.last_error())
    assert eng_routes_by_patch()
    for patch, want in ((32, 3072), (16, 768), (14, 640)):
        assert int(L.cdll.aph_patch_row_elems(patch)) == want == ops.patch_row_elems(patch)
    assert int(L.cdll.aph_patch_row_elems(0)) == 0 == ops.patch_row_elems(0)


def eng_routes_by_patch():
    """one predicate decides the route in every layer: a patch side that is no power of two takes the window pair and padded rows"""
    return all(ops._pow2(p) == (p & (p - 1) == 0) for p in range(1, 65)) and not ops._pow2(14) and ops._pow2(16)


# ------------------------------------------------------------------------------------------------------------------------- two ranks
def _rank_worker(rank, world, port, q, cuts):
    import os
    import sys
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    lib = _ffi.Library(build_emu.build())
    eng = _rank_engine(lib, rank, world, cuts)
    seed_all(123)
    losses = []
    for _ in range(2):
        eng.step()
        losses.append(eng.global_loss())
    q.put((rank, eng.params.clone().numpy(), losses))
    dist.barrier()
    dist.destroy_process_group()


def _rank_engine(lib, rank, world, cuts):
    from aphantasia_amd.engine import Engine
    model, _ = tiny14_model(lib, S=cuts)
    seed_all(0)
    params = R.fft_params_init([1, 3, H, W]).contiguous()
    target = torch.randn(1, 128, generator=torch.Generator().manual_seed(2))
    return Engine(params, H, W, model, cuts, [(target, -1.0)], sim='mix', macro=0.4, rank=rank, world=world, lib=lib)


def check_ranks_gloo(lib, world=2, cuts=5):
    """the 14-pixel tiny model's cuts split over two CPU ranks (3 + 2), one gloo all-reduce per step: the comparison and tolerances of
    tests/test_engine_emu.py::test_engine_ranks_gloo -- ranks bit-identical, the single-rank run up to summation order"""
    import torch.multiprocessing as mp
    from aphantasia_amd.comm import free_port
    eng = _rank_engine(lib, 0, 1, cuts)
    seed_all(123)
    want = []
    for _ in range(2):
        eng.step()
        want.append(eng.global_loss())
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q, cuts)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
    for r in range(1, world):
        assert np.array_equal(res[0][1], res[r][1]) and res[0][2] == res[r][2]
    d = np.abs(res[0][1] - eng.params.numpy())
    assert d.max() < 5e-3 and d.mean() < 5e-5, (d.max(), d.mean())
    assert np.allclose(res[0][2], want, atol=1e-4)
