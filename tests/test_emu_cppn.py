"""CPU: the CPPN kernels (csrc/synth_cppn.h) under the tests/emu interpreter -- the shared fp64 checks of cppn_checks.py, the drop-in autograd
surface and the fused engine; the product library runs the identical checks in tests/test_gpu_cppn.py."""
import os
import sys

import pytest
import torch

from aphantasia_amd import _ffi
import cppn_checks as K

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
TINY = dict(input_resolution=32, patch_size=16, width=256, layers=2, heads=4, output_dim=128)


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.mark.parametrize('case', [c for c in K.CASES if c[6]], ids=K.case_id)
def test_cppn_fwd_bwd_fp64(emu, case):
    K.check_fp64(emu, 'cpu', *case[:6])


def test_cppn_refusals(emu):
    K.check_refusals(emu, 'cpu')


def test_dropin_autograd_equals_the_c_abi(emu):
    """one loss.backward() through image_f leaves aph_cppn_bwd's gradient on every leaf, and torch.optim.Adam steps them in the flat buffer"""
    from aphantasia_amd.cppn import cppn_image
    torch.manual_seed(3)
    params, image_f, _ = cppn_image([1, 3, 9, 13], 3, 8, 'unbias', device='cpu', lib=emu)
    syn = image_f.synth
    gw = torch.randn(1, 3, 9, 13, generator=torch.Generator().manual_seed(4))
    opt = torch.optim.Adam(params, 0.003)
    img = image_f()
    assert tuple(img.shape) == (1, 3, 9, 13)
    (img * gw).sum().backward()
    want = torch.empty(syn.numel)
    rgb = syn.forward(image_f.flat.detach())
    assert torch.equal(rgb, img.detach()[0])
    syn.backward(image_f.flat.detach(), gw[0].contiguous(), want)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in params]), want)
    before = image_f.flat.detach().clone()
    opt.step()
    assert not torch.equal(image_f.flat.detach(), before) and torch.equal(torch.cat([p.detach().reshape(-1) for p in params]), image_f.flat.detach())


def test_engine_cppn_free_running_vs_torch_loop(emu):
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.weights import synthetic_visual_weights
    w = synthetic_visual_weights(TINY, 3)
    model = CLIPModel('tiny', TINY, w, None, max_batch=5, lib=emu, exact=True)
    eng, gen = K.check_engine(emu, 'cpu', model, w, TINY, 40, 56, 5, 4, use_graph=False)
    fresh = torch.empty_like(eng.rgb)
    gen.synth.forward(eng.params, out=fresh, stash=False)
    assert torch.equal(eng.synthesize(), fresh)
    with pytest.raises(NotImplementedError):
        eng.synthesize(shift=torch.zeros(1))
