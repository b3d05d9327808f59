"""CPU: the LPIPS term's kernels (csrc/lpips.hip, lpips_conv.h, lpips_ops.h) under the tests/emu interpreter on a narrow network -- the shared
checks of lpips_checks.py; the product library runs the identical checks at the VGG-16 widths in tests/test_gpu_lpips.py."""
import os
import sys

import pytest

from aphantasia_amd import _ffi
import lpips_checks as K

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
FRAME = (38, 54)        # half size 19 x 27: two tiles each way, ragged; stages 19x27, 9x13, 4x6, 2x3, 1x1 (two pools drop a row AND a column)


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.mark.parametrize('case', K.conv_cases(K.NARROW, FRAME[0] // 2, FRAME[1] // 2), ids=lambda c: '%d-%d-%dx%d' % c)
def test_conv_forward_fp64(emu, case):
    K.check_conv_fwd(emu, 'cpu', *case)


@pytest.mark.parametrize('case', K.conv_cases(K.NARROW, FRAME[0] // 2, FRAME[1] // 2), ids=lambda c: '%d-%d-%dx%d' % c)
def test_conv_dgrad_fp64(emu, case):
    K.check_conv_dgrad(emu, 'cpu', *case)


def test_conv_two_channel_blocks_and_chunks(emu):
    """more than 64 output channels (two workgroups along N, the second partial) and more than one 32-channel chunk"""
    K.check_conv_fwd(emu, 'cpu', 48, 80, 5, 7)
    K.check_conv_dgrad(emu, 'cpu', 80, 48, 5, 7)


@pytest.mark.parametrize('shape', [(19, 27, 16), (8, 6, 32), (2, 3, 8)], ids=lambda s: '%dx%dx%d' % s)
def test_pool_exact(emu, shape):
    K.check_pool(emu, 'cpu', *shape)


@pytest.mark.parametrize('pc', [(19 * 27, 16), (70, 32), (1, 64), (33, 512)], ids=lambda s: 'P%d-C%d' % s)
def test_head_fp64(emu, pc):
    K.check_head(emu, 'cpu', *pc)


@pytest.mark.parametrize('hw', [(38, 54), (33, 32), (75, 107)], ids=lambda s: '%dx%d' % s)
def test_resize_and_adjoint(emu, hw):
    K.check_resize(emu, 'cpu', *hw)


@pytest.mark.parametrize('weight', [1.0, 1e-3])
def test_value_grad_end_to_end(emu, weight):
    K.check_e2e(emu, 'cpu', K.NARROW, *FRAME, weight=weight)


def test_value_grad_smallest_frame(emu):
    K.check_e2e(emu, 'cpu', K.NARROW, 33, 32)


def test_dropin_sim_loss(emu):
    K.check_dropin(emu, 'cpu', K.NARROW, 33, 32)


def test_refusals(emu):
    K.check_refusals(emu, 'cpu')


TINY = dict(input_resolution=32, patch_size=16, width=256, layers=2, heads=4, output_dim=128)

@pytest.fixture(scope='module')
def tiny_model(emu):
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.weights import synthetic_visual_weights
    return CLIPModel('tiny', TINY, synthetic_visual_weights(TINY, 3), None, max_batch=5, lib=emu)


def test_engine_sync_term(emu, tiny_model):
    K.check_engine(emu, 'cpu', tiny_model, K.NARROW, 40, 56, 5, use_graph=False)


def test_engine_without_the_term_issues_the_parent_commits_calls(emu, tiny_model):
    assert K.engine_call_sequence(emu, 'cpu', tiny_model, 40, 56, 5) == K.PARENT_STEP_CALLS
