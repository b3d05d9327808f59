"""GPU (MI355X): the exact (fp32) ViT path -- Engine(exact=True), clip.load(exact=True) -- against the fp32 CPU oracle: one C2 step,
stress-weight single steps at ViT-B/32 and B/16, the stress loss-curve ensemble with a HARD per-member 1e-3 gate, the 200-step C2 curve,
bitwise repeatability (two runs; graph replay against eager launches) and the drop-in autograd surface."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

from aphantasia_amd import clip as aclip, transforms
from aphantasia_amd.engine import Engine
from aphantasia_amd.weights import stress_visual_weights, visual_config
from oracle import reference_path as R
from oracle import clip_vit_ref
import exact_checks as X

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)


def model_of(name, max_batch, weights=None):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if weights is None:
            return aclip.load(name, seed=1, max_batch=max_batch, exact=True)[0]
        return aclip.CLIPModel(name, visual_config(name), weights, None, max_batch, exact=True)


def tool(name):
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'tools', name + '.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def rel_max(got, ref):
    got, ref = got.reshape(-1).double().cpu(), ref.reshape(-1).double()
    return (got - ref).abs().max().item() / ref.abs().max().item()


def test_c2_one_step_exact_vs_oracle():
    """1280x720, ViT-B/32, 200 cuts, the reference's draw order: |d loss| <= 5e-7, spectrum gradient <= 1e-5 max|g| (f16 mode: 3e-6, 1.1e-3)"""
    h, w, S = 720, 1280, 200
    m = model_of('ViT-B/32', S)
    seed_all(0)
    p0 = R.fft_params_init([1, 3, h, w])
    tgt = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))
    eng = Engine(p0.to(DEV).contiguous(), h, w, m, S, [(tgt, -1.0)], sim='mix', transform=transforms.normalize(), rng='reference',
                 use_graph=False, exact=True)
    run = R.ReferenceRun(h, w, lambda x: clip_vit_ref.encode_image(m.visual.weights, x, m.visual.cfg), [(tgt, 1.0)], params=p0)
    seed_all(11)
    table = R.draw_crop_table(S, 224, h, w, 'uniform', 0.4)
    got = float(eng.step(table))
    want = run.step(table)
    rel = rel_max(eng.grad, run.params.grad)
    print('C2 one exact step: |d loss| %.2e, spectrum gradient max rel %.2e' % (abs(got - want), rel))
    assert abs(got - want) <= 5e-7 and rel <= 1e-5, (got, want, rel)


@pytest.mark.parametrize('name,S', [('ViT-B/32', 4), ('ViT-B/16', 2)])
def test_stress_weights_single_step_input_gradient(name, S):
    """weights with realistic dynamic range (the ensemble's): input gradient <= 2e-5 max|g| against the fp64 oracle (B/16: T = 197)"""
    cfg = visual_config(name)
    ferr, berr = X.check_vit_exact(None, DEV, cfg, S=S, fwd_tol=1e-5, bwd_tol=2e-5,
                                   scale_w=lambda w: stress_visual_weights(cfg, 1))
    print('%s stress weights: forward %.2e, input gradient %.2e (of max)' % (name, ferr, berr))


def test_stress_ensemble_exact_mode():
    """every member of tests/golden/ensemble, 60 free-running steps in exact mode: HARD gate 1e-3 on every member at every step; the median
    member's worst step < 3e-4 (about 4x the oracle's own thread-count spread of 7.7e-5)"""
    ens = tool('loss_ensemble')
    mem = ens.members()
    assert len(mem) >= 24, len(mem)
    cfg = visual_config('ViT-B/32')
    by = {}
    for ws, cs, S, f in mem:
        by.setdefault((ws, S), []).append((cs, f))
    rows = []
    for (ws, S), lst in sorted(by.items()):
        model = model_of('ViT-B/32', S, stress_visual_weights(cfg, ws))
        for cs, f in lst:
            want = np.load(f)['loss']
            got, skipped = ens.run_member(model, S, cs, want, False, exact=True)
            assert np.isfinite(got).all() and skipped == 0, (ws, cs, S, skipped)
            rows.append((float(np.abs(got - want).max()), (ws, cs, S)))
        del model
        torch.cuda.empty_cache()
    mx = np.array([r[0] for r in rows])
    print('stress ensemble, exact: %d members, max |d loss| median %.2e  p90 %.2e  worst %.2e %s ; members past 1e-3: %d'
          % (len(mx), np.median(mx), np.quantile(mx, 0.9), mx.max(), max(rows)[1], int((mx > 1e-3).sum())))
    print('per member: ' + ' '.join('%.1e' % v for v in sorted(mx)))
    assert mx.max() < 1e-3, max(rows)
    assert np.median(mx) < 3e-4, np.median(mx)


def test_c2_s200_200_curve_exact():
    """BASELINE configs[1] verbatim (200 cuts, 200 free-running steps) in exact mode: worst step <= 5e-5 (f16 mode: 1.1e-4 .. 5.1e-4)"""
    worst, first, rms, _ = tool('loss_curve').run_fixture('c2_s200_200', exact=True)
    print('C2 200 cuts x 200 steps, exact: max |d loss| %.2e, final block-mean RMS %.4f' % (worst, rms))
    assert worst <= 5e-5, worst


def test_exact_steps_bitwise_repeatable_and_graph_equals_eager():
    h, w, S = 360, 640, 32
    m = model_of('ViT-B/32', S)
    tgt = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))

    def run(use_graph, n):
        seed_all(0)
        p0 = R.fft_params_init([1, 3, h, w])
        eng = Engine(p0.to(DEV).contiguous(), h, w, m, S, [(tgt, -1.0)], sim='mix', transform=transforms.normalize(), rng='reference',
                     use_graph=use_graph, exact=True)
        seed_all(5)
        losses = [float(eng.step(R.draw_crop_table(S, 224, h, w, 'uniform', 0.4))) for _ in range(n)]
        return losses, eng.params.detach().cpu().clone()
    l1, p1 = run(True, 10)
    l2, p2 = run(True, 10)
    assert l1 == l2 and torch.equal(p1, p2)
    l3, p3 = run(False, 10)
    assert l1 == l3 and torch.equal(p1, p3)


def test_clip_load_exact_encode_image_autograd():
    """the drop-in surface: clip.load(exact=True).encode_image under autograd against the fp64 oracle, at the single-step gates"""
    S = 6
    m = model_of('ViT-B/32', S)
    assert m.visual.exact
    x = torch.randn(S, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    genc = torch.randn(S, 512, generator=torch.Generator().manual_seed(2)) * 0.01
    xg = x.to(DEV).requires_grad_(True)
    enc = m.encode_image(xg)
    (enc * genc.to(DEV)).sum().backward()
    xd = x.double().requires_grad_(True)
    want = clip_vit_ref.encode_image({k: v.double() for k, v in m.visual.weights.items()}, xd, m.visual.cfg)
    (want * genc.double()).sum().backward()
    ferr, berr = rel_max(enc.detach(), want.detach()), rel_max(xg.grad, xd.grad)
    print('encode_image exact: forward %.2e, input gradient %.2e' % (ferr, berr))
    assert ferr <= 1e-5 and berr <= 1e-5, (ferr, berr)


def test_gemm_f32_full_shapes_vs_fp64():
    """the f32-input MFMA GEMM at the ViT's shapes on the device: every element within 1e-6 sum|a b| of fp64"""
    L = __import__('aphantasia_amd._ffi', fromlist=['lib']).lib()
    for M, N, K, lda, ws in [(9500, 2304, 768, None, 0), (1000, 768, 3072, None, 0), (190, 768, 3072, 50 * 3072, 1 << 22),
                             (190, 3072, 768, None, 1 << 22)]:
        X.check_gemm_f32(L, DEV, M, N, K, lda=lda, ws_floats=ws)
    for epi in (1, 2, 3, 4):
        X.check_gemm_f32(L, DEV, 300, 768, 768, epi=epi, seed=epi)
    X.check_sampler_f32(L, DEV, augment=False)
    X.check_sampler_f32(L, DEV, augment=True)
    X.check_enable_f32_refusals(L, DEV)


def _show(tag, ratios):
    print('%s: worst err / bound  %s' % (tag, '  '.join('%s %.3f' % kv for kv in ratios.items())))


@pytest.mark.parametrize('T', [1, 31, 32, 33, 50, 64, 65, 197, 255, 256])
def test_attention_f32_vs_fp64(T):
    """the fp32 attention kernels alone at 12 heads: the 32-row blocks' edges and T = 256, the 156 KiB dynamic-LDS launch no ViT reaches"""
    L = __import__('aphantasia_amd._ffi', fromlist=['lib']).lib()
    _show('fp32 T=%d normal' % T, X.check_attention_f32(L, DEV, S=3, T=T, heads=12, seed=T))


@pytest.mark.parametrize('S,T', [(24, 50), (6, 197), (3, 256)])
@pytest.mark.parametrize('kind', [k for k in X.V.ATTN_KINDS if k != 'normal'])
def test_attention_f32_families_vs_fp64(kind, S, T):
    L = __import__('aphantasia_amd._ffi', fromlist=['lib']).lib()
    _show('fp32 S=%d T=%d %s' % (S, T, kind), X.check_attention_f32(L, DEV, S=S, T=T, heads=12, kind=kind, seed=5))
