"""CPU: the `-tf custom` / `-tf elastic` kernels (csrc/sampler_kornia.h) under the tests/emu interpreter -- the shared fp64 checks of tf_checks.py
and the fused engine against the oracle; the product library runs the identical checks in tests/test_gpu_tf.py."""
import os
import sys

import pytest

from aphantasia_amd import _ffi
import tf_checks as K

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
TINY = dict(input_resolution=32, patch_size=16, width=256, layers=2, heads=4, output_dim=128)
FWD, BWD = K.mode_cases()


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.mark.parametrize('case', FWD, ids=K.case_id)
def test_tf_forward_fp64(emu, case):
    K.check_forward(emu, 'cpu', *case)


@pytest.mark.parametrize('case', BWD, ids=K.case_id)
def test_tf_adjoint_fp64(emu, case):
    K.check_adjoint(emu, 'cpu', *case, gscale=0.5 if case[2] == 'nchw_norm' else 1.0)


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_tf_properties(emu, chain):
    for name in ('hand', 'drawn'):
        K.check_dot_product(emu, 'cpu', name, chain)
        K.check_window_gradient(emu, 'cpu', name, chain)
    K.check_erase_preimage(emu, 'cpu', chain)
    K.check_bitwise_repeat(emu, 'cpu', 'hand', chain)


def test_tf_refusals_and_fast_forwarding(emu):
    K.check_refusals(emu, 'cpu')
    K.check_fast_forwarding(emu, 'cpu')


def _model(emu, S, **kw):
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.weights import synthetic_visual_weights
    w = synthetic_visual_weights(TINY, 3)
    return CLIPModel('tiny', TINY, w, None, max_batch=S, lib=emu, **kw), w


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_engine_tf_free_running_vs_oracle(emu, chain):
    model, w = _model(emu, 5)
    K.check_engine(emu, 'cpu', model, w, TINY, chain, 40, 56, 5, 6, use_graph=False)


@pytest.mark.parametrize('chain', list(K.CHAINS))
@pytest.mark.parametrize('mode', ['precise', 'exact', 'grad_f16'])
def test_engine_tf_modes_vs_oracle(emu, mode, chain):
    """the other patch layouts of the engine (hi | lo rows, fp32 rows, the f16 gradient) through both chains"""
    model, w = _model(emu, 5, exact=mode == 'exact')
    K.check_engine(emu, 'cpu', model, w, TINY, chain, 40, 56, 5, 2, use_graph=False, **{mode: True})


def test_engine_tf_dual_model_vs_oracle(emu):
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.weights import synthetic_visual_weights
    ws = [synthetic_visual_weights(TINY, 3), synthetic_visual_weights(TINY, 5)]
    models = [CLIPModel('tiny', TINY, w, None, max_batch=4, lib=emu) for w in ws]
    K.check_engine_dual(emu, 'cpu', models, ws, TINY, 'custom', 40, 56, 4, 4, use_graph=False)


@pytest.mark.parametrize('chain', list(K.CHAINS))
def test_engine_tf_rank_shards_sum_to_the_single_rank_step(emu, chain):
    model, _ = _model(emu, 5)
    K.check_engine_ranks(emu, 'cpu', model, TINY, chain, 40, 56, 5, 2)
