"""GPU (MI355X): the CPPN kernels of the product library -- the shared fp64 checks of cppn_checks.py at every case, and the fused engine
with the real ViT-B/32 (synthetic weights) through eager steps and graph replays."""
import warnings

import pytest
import torch

from aphantasia_amd import clip as aclip
import cppn_checks as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_cppn_fwd_bwd_fp64(case):
    K.check_fp64(None, DEV, *case[:6])


def test_cppn_refusals():
    K.check_refusals(None, DEV)


def test_engine_cppn_vit_b32_eager_and_graph():
    """64x96, 4 cuts, 6 steps: two eager steps and four graph replays against the torch loop; then Engine.synthesize == a fresh aph_cppn_fwd"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = aclip.load('ViT-B/32', seed=1, max_batch=4, exact=True)[0]
    weights = {k: v.detach().float().cpu() for k, v in m.visual.weights.items()}
    eng, gen = K.check_engine(None, DEV, m, weights, m.visual.cfg, 64, 96, 4, 6, use_graph=True)
    assert eng._graph is not None, 'the step was not captured'
    fresh = torch.empty_like(eng.rgb)
    gen.synth.forward(eng.params, out=fresh, stash=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.synthesize(), fresh)
