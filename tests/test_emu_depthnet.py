"""CPU: the depth estimator's kernels (csrc/depth.hip, depth_kernels.h, the batched / residual instantiation of lpips_conv.h) under the
tests/emu interpreter on a narrow network -- the shared checks of depthnet_checks.py; the product library runs the same checks, the long
sequences and a Base-width network in tests/test_gpu_depthnet.py."""
import os
import sys

import pytest

from aphantasia_amd import _ffi
import depthnet_checks as K

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.mark.parametrize('T', K.attn_tile_edges())
def test_attention_tile_edges_fp64(emu, T):
    K.check_attention(emu, 'cpu', 2, T, 2, 'normal')


@pytest.mark.parametrize('kind', K.ATTN_KINDS[1:])
def test_attention_families_fp64(emu, kind):
    K.check_attention(emu, 'cpu', 2, 118, 2, kind)


@pytest.mark.parametrize('variant', K.CONV_VARIANTS)
def test_conv_variants_fp64(emu, variant):
    K.check_conv(emu, 'cpu', 48, 80, 5, 7, variant)


@pytest.mark.parametrize('case', [(8, 8, 5, 7), (3, 16, 19, 27), (64, 64, 19, 27), (8, 48, 37, 65)], ids=lambda c: '%d-%d-%dx%d' % c)
def test_conv_shapes_fp64(emu, case):
    K.check_conv(emu, 'cpu', *case, variant='batch2')
    K.check_conv(emu, 'cpu', *case, variant='stride2')


def test_lpips_instantiation_keeps_its_bits(emu):
    K.check_lpips_instantiation_unmoved(emu, 'cpu', 48, 80, 19, 27)


@pytest.mark.parametrize('k', [4, 2])
def test_transpose_conv_fp64(emu, k):
    K.check_convt(emu, 'cpu', k, 48, 48, 5, 7)
    K.check_convt(emu, 'cpu', k, 8, 16, 5, 7, B=1)


@pytest.mark.parametrize('mkn', [(35, 128, 16), (70, 32, 32), (130, 72, 80)], ids=lambda s: 'M%d-K%d-N%d' % s)
def test_neck_gemm_fp64(emu, mkn):
    K.check_gemm1x1(emu, 'cpu', *mkn)
    K.check_gemm1x1(emu, 'cpu', *mkn, bias=False)


@pytest.mark.parametrize('case', [(5, 7, 9, 13), (9, 13, 18, 26), (5, 7, 10, 14), (5, 7, 5, 7), (1, 7, 1, 13), (1, 7, 3, 14), (19, 33, 37, 65)],
                         ids=lambda c: '%dx%d-%dx%d' % c)
def test_resize_fp64(emu, case):
    K.check_resize(emu, 'cpu', *case)


@pytest.mark.parametrize('mnk', [(35, 128, 64), (200, 256, 128)], ids=lambda s: 'M%d-N%d-K%d' % s)
def test_gelu_epilogue_fp64(emu, mnk):
    K.check_gelu_gemm(emu, 'cpu', *mnk)


def test_end_to_end_narrow(emu):
    K.check_e2e(emu, 'cpu', 'narrow', K.NARROW, 56, 84, seed=0)


def test_batch_and_flip(emu):
    K.check_batch_and_flip(emu, 'cpu', K.NARROW, 28, 42)


def test_refusals(emu):
    K.check_refusals(emu, 'cpu')
