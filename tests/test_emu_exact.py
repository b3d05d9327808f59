"""CPU: the exact (fp32) ViT path under the host SIMT interpreter (tests/emu) -- the f32-input MFMA GEMM against fp64, the forward and
input gradient against the oracle run in float64 (gates ~300x tighter than the f16 path's check_vit: any f16 rounding left in the path fails
them), the APH_OUT_PATCH_F32 sampler mode, aph_vit_enable_f32's refusals, and an exact Engine step against the reference step."""
import os
import sys

import pytest
import torch

from aphantasia_amd import _ffi
import exact_checks as X

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.mark.parametrize('M,N,K,lda,a_rowP,ws', [
    (37, 128, 32, None, 0, 0),          # ragged M, a single k-tile
    (130, 256, 96, None, 0, 0),         # two row tiles (ragged), multi-tile k walk
    (5, 128, 256, 50 * 256, 0, 0),      # class-row pitch T * D
    (5, 128, 256, 50 * 256, 0, 1 << 16),  # the same split over k (small M): partials summed in split order
    (12, 128, 64, None, 4, 0),          # patch rows of a token-major buffer (row m + m / P + 1)
])
def test_gemm_f32_vs_fp64(emu, M, N, K, lda, a_rowP, ws):
    X.check_gemm_f32(emu, 'cpu', M, N, K, lda=lda, a_rowP=a_rowP, ws_floats=ws)


@pytest.mark.parametrize('epi', [1, 2, 3, 4])
def test_gemm_f32_epilogues(emu, epi):
    X.check_gemm_f32(emu, 'cpu', 40, 128, 64, epi=epi, seed=epi)


def test_gemm_f32_split_bitwise_repeatable(emu):
    A = torch.randn(7, 512)
    Bt = torch.randn(256, 512)
    c1, _ = X.gemm_f32(emu, 'cpu', A, Bt, 7, 256, 512, ws_floats=1 << 16)
    c2, _ = X.gemm_f32(emu, 'cpu', A, Bt, 7, 256, 512, ws_floats=1 << 16)
    assert torch.equal(c1, c2)


@pytest.mark.parametrize('res,S', [(32, 3), (64, 2), (112, 1), (224, 1)])     # T = 5 (K.TINY), 17, 50, 197
def test_vit_exact_vs_fp64_oracle(emu, res, S):
    cfg = dict(X.TINY, input_resolution=res)
    ferr, berr = X.check_vit_exact(emu, 'cpu', cfg, S=S)
    print('T = %d: forward %.2e, input gradient %.2e' % ((res // 16) ** 2 + 1, ferr, berr))


@pytest.mark.parametrize('augment', [False, True])
def test_sampler_patch_f32(emu, augment):
    X.check_sampler_f32(emu, 'cpu', augment=augment)


def test_vit_exact_needs_enable_f32(emu):
    X.check_enable_f32_refusals(emu, 'cpu')


def test_engine_exact_step_vs_reference_run(emu):
    """an Engine(exact=True) step on a tiny image against the oracle's ReferenceRun step (fp32 CPU): loss to 1e-6, spectrum gradient to
    1e-4 max|g|; exact is refused together with precise / grad_f16"""
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.engine import Engine
    from aphantasia_amd.weights import synthetic_visual_weights
    from oracle import reference_path as R
    from oracle import clip_vit_ref
    H, W, S = 40, 56, 5
    w = synthetic_visual_weights(X.TINY, 3)
    model = CLIPModel('tiny', X.TINY, w, None, max_batch=S, lib=emu, exact=True)
    torch.manual_seed(0)
    params = R.fft_params_init([1, 3, H, W]).contiguous()
    target = torch.randn(1, 128, generator=torch.Generator().manual_seed(2))
    for bad in (dict(precise=True), dict(grad_f16=True)):
        with pytest.raises(ValueError, match='exclusive'):
            Engine(params.clone(), H, W, model, S, [(target, -1.0)], sim='mix', lib=emu, exact=True, **bad)
    eng = Engine(params.clone(), H, W, model, S, [(target, -1.0)], sim='mix', macro=0.4, lib=emu, exact=True)
    assert eng.patches.dtype == torch.float32 and eng._patch_mode == _ffi.APH_OUT_PATCH_F32
    run = R.ReferenceRun(H, W, lambda x: clip_vit_ref.encode_image(w, x, X.TINY), [(target, 1.0)], size=32, params=params.clone())
    torch.manual_seed(7)
    table = R.draw_crop_table(S, 32, H, W, 'uniform', 0.4)
    want = run.step(table)
    got = float(eng.step(table))
    g_ref = run.params.grad.reshape(-1).double()
    gerr = (eng.grad.reshape(-1).double() - g_ref).abs().max().item() / g_ref.abs().max().item()
    assert abs(got - want) <= 1e-6 and gerr <= 1e-4, (got, want, gerr)


def test_clis_refuse_exact_with_precise():
    """clip_fft.py refuses --exact --precise; illustrip.py (which has no split-precision mode) takes --exact and refuses the pair too"""
    import clip_fft
    import illustrip
    assert clip_fft.get_args(['-t', 'x', '--exact']).exact and not clip_fft.get_args(['-t', 'x']).exact
    assert illustrip.get_args(['-t', 'x', '--exact']).exact and not illustrip.get_args(['-t', 'x']).exact
    for mod in (clip_fft, illustrip):
        with pytest.raises(SystemExit):
            mod.get_args(['-t', 'x', '--exact', '--precise'])


# ---- the fp32 attention kernels alone against fp64 (exact_checks.check_attention_f32): the kAtfRows = 32 row blocks (one row, a full block,
# one row into the next), lanes' 64-key strides, and T = 256 -- the 156 KiB dynamic-LDS launch no ViT reaches (T = n^2 + 1 <= 226)
def _show(tag, ratios):
    print('%s: worst err / bound  %s' % (tag, '  '.join('%s %.3f' % kv for kv in ratios.items())))


@pytest.mark.parametrize('T', [1, 31, 32, 33, 50, 64, 65, 197, 255, 256])
def test_attention_f32_vs_fp64(emu, T):
    _show('fp32 T=%d normal' % T, X.check_attention_f32(emu, 'cpu', S=2 if T <= 64 else 1, T=T, heads=2, seed=T))


@pytest.mark.parametrize('T', [50, 197])
@pytest.mark.parametrize('kind', [k for k in X.V.ATTN_KINDS if k != 'normal'])
def test_attention_f32_families_vs_fp64(emu, kind, T):
    _show('fp32 T=%d %s' % (T, kind), X.check_attention_f32(emu, 'cpu', S=1, T=T, heads=2, kind=kind, seed=3))
