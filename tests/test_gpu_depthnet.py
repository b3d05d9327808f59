"""GPU: the depth estimator on the product library -- the shared checks of depthnet_checks.py at the sizes the interpreter cannot reach (the
long sequences of 518 x 518 and 518 x 910 images, a Base-width network), the batch / flip identities, the refusals and the CLI flag."""
import os

import numpy as np
import pytest
import torch

import depthnet_checks as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('T', K.attn_tile_edges())
def test_attention_tile_edges_fp64(T):
    K.check_attention(None, DEV, 2, T, 2, 'normal')


@pytest.mark.parametrize('kind', K.ATTN_KINDS[1:])
def test_attention_families_fp64(kind):
    K.check_attention(None, DEV, 2, 118, 2, kind)


@pytest.mark.parametrize('T', [1370, 2406])
def test_attention_long_sequences_fp64(T):
    """T of a 518 x 518 and of a 518 x 910 image: 22 and 38 key tiles, the last one ragged"""
    K.check_attention(None, DEV, 2, T, 2, 'normal')


@pytest.mark.parametrize('variant', K.CONV_VARIANTS)
def test_conv_variants_fp64(variant):
    K.check_conv(None, DEV, 48, 80, 19, 27, variant)


@pytest.mark.parametrize('case', [(8, 8, 5, 7), (3, 16, 19, 27), (64, 64, 19, 27), (80, 48, 5, 7), (8, 48, 37, 65), (64, 80, 37, 65)], ids=lambda c: '%d-%d-%dx%d' % c)
def test_conv_shapes_fp64(case):
    K.check_conv(None, DEV, *case, variant='batch2')
    K.check_conv(None, DEV, *case, variant='stride2')


def test_lpips_instantiation_keeps_its_bits():
    K.check_lpips_instantiation_unmoved(None, DEV, 48, 80, 19, 27)
    K.check_lpips_instantiation_unmoved(None, DEV, 64, 64, 37, 65)


@pytest.mark.parametrize('k', [4, 2])
def test_transpose_conv_fp64(k):
    K.check_convt(None, DEV, k, 48, 48, 5, 7)
    K.check_convt(None, DEV, k, 80, 80, 5, 7)
    K.check_convt(None, DEV, k, 8, 16, 5, 7, B=1)


@pytest.mark.parametrize('mkn', [(35, 128, 16), (70, 32, 32), (130, 72, 80), (2 * 37 * 65, 768, 96)], ids=lambda s: 'M%d-K%d-N%d' % s)
def test_neck_gemm_fp64(mkn):
    K.check_gemm1x1(None, DEV, *mkn)
    K.check_gemm1x1(None, DEV, *mkn, bias=False)


@pytest.mark.parametrize('case', [(5, 7, 9, 13), (9, 13, 18, 26), (5, 7, 10, 14), (5, 7, 5, 7), (1, 7, 1, 13), (1, 7, 3, 14), (19, 33, 37, 65), (37, 65, 74, 130)],
                         ids=lambda c: '%dx%d-%dx%d' % c)
def test_resize_fp64(case):
    K.check_resize(None, DEV, *case)
    K.check_resize(None, DEV, *case, C=48, B=1)


@pytest.mark.parametrize('mnk', [(35, 128, 64), (200, 256, 128), (236, 3072, 768), (2740, 1536, 384)], ids=lambda s: 'M%d-N%d-K%d' % s)
def test_gelu_epilogue_fp64(mnk):
    """(236, 3072, 768) is the Base fc1 of the end-to-end test, (2740, 1536, 384) the Small fc1 of two 518 x 518 images: the ring kernels,
    whose epilogue is apply8"""
    K.check_gelu_gemm(None, DEV, *mnk)


def test_gelu_epilogue_wave_specialised_route_fp64():
    """M = 2 x 2406 rows (a batch of two 518 x 910 images), Base fc1: 19 x 24 = 456 tiles of 256 x 128 -> the wave-specialised kernel's ws_tile"""
    K.check_gelu_gemm(None, DEV, 4812, 3072, 768)


def test_end_to_end_narrow():
    K.check_e2e(None, DEV, 'narrow', K.NARROW, 56, 84, seed=0)


def test_end_to_end_base_width():
    K.check_e2e(None, DEV, 'base2', K.BASE2, 126, 182, seed=0)


def test_batch_and_flip():
    K.check_batch_and_flip(None, DEV, K.NARROW, 126, 182)


def test_refusals():
    K.check_refusals(None, DEV)


def test_cli_depth_backends(tmp_path):
    """illustrip.py -d with a tiny saved checkpoint: both backends finish, and their first-frame depth maps (the same first frame: same seed)
    agree.  The maps are 8-bit JPEGs of the min-max normalised depth, so the tolerance is in grey levels: 255 times the end-to-end gate on the
    normalised map (2 x E16 max-abs, measured on this network by check_e2e's reference) plus one level of quantisation, on the mean absolute
    difference (a JPEG block can move single pixels further than the map itself moved)."""
    pytest.importorskip('transformers')
    from PIL import Image
    from transformers import DepthAnythingConfig, DepthAnythingForDepthEstimation, Dinov2Config
    import illustrip
    from aphantasia_amd import depthnet as DN
    bc = Dinov2Config(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, image_size=518, patch_size=14, out_indices=[1, 2, 3, 4],
                      apply_layernorm=True, reshape_hidden_states=False)
    cfg = DepthAnythingConfig(backbone_config=bc, reassemble_hidden_size=128, neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32, head_hidden_size=16,
                              reassemble_factors=[4, 2, 1, 0.5])
    model = DepthAnythingForDepthEstimation(cfg)
    model.load_state_dict(DN.synthetic_weights(cfg.to_dict(), seed=2, last_bias=2.0), strict=False)
    ckpt = str(tmp_path / 'ckpt')
    model.save_pretrained(ckpt)
    del model
    maps = {}
    for backend in ('hip', 'torch'):
        out, dm = str(tmp_path / ('o_' + backend)), str(tmp_path / ('dm_' + backend))
        illustrip.main(['-t', 'a cat', '-nv', '--seed', '0', '--steps', '2', '--samples', '12', '--size', '96-64', '--out_dir', out, '-d', '0.3',
                        '--depth_weights', ckpt, '--depth_backend', backend, '--depth_dir', dm])
        files = sorted(os.listdir(dm))
        assert len(files) == 2, files
        maps[backend] = np.asarray(Image.open(os.path.join(dm, files[0])).convert('L'), dtype=np.float64)
    e16 = K.e2e_reference('narrow', K.NARROW, 56, 84, 0)
    gate = 2 * K.errors(K.R.normalise(e16[3]), K.R.normalise(e16[2]))[0]
    diff = np.abs(maps['hip'] - maps['torch']).mean()
    print('CLI: mean |hip - torch| of the first depth map = %.3f grey levels (tolerance %.3f)' % (diff, 255 * gate + 1))
    assert maps['hip'].std() > 1.0, 'the depth map is flat: nothing was compared'
    assert diff <= 255 * gate + 1
