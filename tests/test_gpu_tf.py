"""GPU (MI355X): the `-tf custom` / `-tf elastic` kernels of the product library -- the shared fp64 checks of tf_checks.py at every case and
mode, the fused engine with the tiny ViT through eager steps and graph replays, and one 1280x720 / ViT-B/32 step per chain against the oracle."""
import warnings

import numpy as np
import pytest
import torch

from aphantasia_amd import clip as aclip
from oracle import reference_path as R
from oracle import clip_vit_ref
import tf_checks as K
import tf_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TINY = dict(input_resolution=32, patch_size=16, width=256, layers=2, heads=4, output_dim=128)
FWD, BWD = K.mode_cases()


@pytest.mark.parametrize('case', FWD, ids=K.case_id)
def test_tf_forward_fp64(case):
    K.check_forward(None, DEV, *case)


@pytest.mark.parametrize('case', BWD, ids=K.case_id)
def test_tf_adjoint_fp64(case):
    K.check_adjoint(None, DEV, *case, gscale=0.5 if case[2] == 'nchw_norm' else 1.0)


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_tf_properties(chain):
    for name in ('hand', 'drawn'):
        K.check_dot_product(None, DEV, name, chain)
        K.check_window_gradient(None, DEV, name, chain)
    K.check_erase_preimage(None, DEV, chain)
    K.check_bitwise_repeat(None, DEV, 'hand', chain)
    K.check_bitwise_repeat(None, DEV, 'vit_b32', chain)


def test_tf_refusals_and_fast_forwarding():
    K.check_refusals(None, DEV)
    K.check_fast_forwarding(None, DEV)


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_engine_tf_free_running_across_graph_capture(chain):
    """tiny ViT, 40x56, 5 cuts, six steps: two eager, the capture, graph replays"""
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.weights import synthetic_visual_weights
    w = synthetic_visual_weights(TINY, 3)
    model = CLIPModel('tiny', TINY, w, None, max_batch=5)
    eng = K.check_engine(None, DEV, model, w, TINY, chain, 40, 56, 5, 6, use_graph=True)
    assert eng._graph is not None, 'the step was not captured'


def _tiny(seed=3, **kw):
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.weights import synthetic_visual_weights
    w = synthetic_visual_weights(TINY, seed)
    return CLIPModel('tiny', TINY, w, None, max_batch=5, **kw), w


@pytest.mark.parametrize('chain', list(K.CHAINS))
@pytest.mark.parametrize('mode', ['precise', 'exact', 'grad_f16'])
def test_engine_tf_modes_vs_oracle(mode, chain):
    """the other patch layouts of the engine (hi | lo rows, fp32 rows, the f16 gradient) through both chains, across the graph capture"""
    model, w = _tiny(exact=mode == 'exact')
    K.check_engine(None, DEV, model, w, TINY, chain, 40, 56, 5, 4, use_graph=True, **{mode: True})


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_engine_tf_dual_model_vs_oracle(chain):
    (m0, w0), (m1, w1) = _tiny(3), _tiny(5)
    K.check_engine_dual(None, DEV, [m0, m1], [w0, w1], TINY, chain, 40, 56, 4, 8, use_graph=True)


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_engine_tf_rank_shards_sum_to_the_single_rank_step(chain):
    model, _ = _tiny()
    K.check_engine_ranks(None, DEV, model, TINY, chain, 40, 56, 5, 3)


@pytest.fixture(scope='module')
def b32():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return aclip.load('ViT-B/32', seed=1, max_batch=24)[0]


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_c2_tf_step_vs_oracle(b32, chain):
    """1280x720, ViT-B/32, 24 cuts, the reference's draw order: one step against the oracle with the tf_ref per-cut transform; the gates of
    the 24-cut C2 single step of `-tf fast`, tests/test_gpu_parity_configs.py::test_c2_fast_transform_step_vs_oracle (|d loss| < 1e-3, gradient
    cosine > 0.999, max relative error < 5e-2)"""
    from aphantasia_amd.engine import Engine
    from aphantasia_amd.utils import draw_crop_params
    h, w, S = 720, 1280, 24
    tf = K.CHAINS[chain]
    torch.manual_seed(0)
    np.random.seed(0)
    p0 = R.fft_params_init([1, 3, h, w])
    tgt = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))
    eng = Engine(p0.to(DEV).contiguous(), h, w, b32, S, [(tgt, -1.0)], sim='mix', transform=tf, rng='reference', use_graph=False)
    cfg, wts = b32.visual.cfg, b32.visual.weights
    run = R.ReferenceRun(h, w, lambda x: clip_vit_ref.encode_image(wts, x, cfg), [(tgt, 1.0)], params=p0)
    torch.manual_seed(4)
    np.random.seed(4)
    table, augs = draw_crop_params(S, 224, h, w, 'uniform', 0.4, tf)
    assert sum(a['angle'] != 0 for a in augs) >= 8 and sum(a['angle'] == 0 for a in augs) >= 2
    assert sum(a['erase'] is not None for a in augs) >= (2 if chain == 'elastic' else 0)
    got = float(eng.step(table, [dict(a) for a in augs]))
    want = run.step(table, tf_ref.per_cut(augs, chain == 'elastic', window=224))
    got_g, ref_g = eng.grad.reshape(-1).double().cpu(), run.params.grad.reshape(-1).double()
    cos = torch.nn.functional.cosine_similarity(got_g, ref_g, dim=0).item()
    rel = (got_g - ref_g).abs().max().item() / ref_g.abs().max().item()
    print('C2 -tf %s one step: loss %.6f vs %.6f, grad cos %.6f, max rel %.2e' % (chain, got, want, cos, rel))
    assert abs(got - want) < 1e-3, (got, want)
    assert cos > 0.999 and rel < 5e-2, (cos, rel)
