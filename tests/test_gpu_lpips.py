"""GPU (MI355X): the LPIPS term of the product library at the VGG-16 widths -- the shared checks of lpips_checks.py.  The 75 x 107 frame has the
half size 37 x 53 and the stages 37x53, 18x26, 9x13, 4x6, 2x3: every stage off any tile multiple, two pools drop an odd row AND an odd column,
the last stage is smaller than one MFMA tile.  33 x 32 (half 16 x 16, last stage 1 x 1) is the smallest legal frame."""
import pytest

import lpips_checks as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FRAME = (75, 107)
CASES = K.conv_cases(K.FULL, FRAME[0] // 2, FRAME[1] // 2)


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%d-%d-%dx%d' % c)
def test_conv_forward_fp64(case):
    K.check_conv_fwd(None, DEV, *case)


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%d-%d-%dx%d' % c)
def test_conv_dgrad_fp64(case):
    K.check_conv_dgrad(None, DEV, *case)


@pytest.mark.parametrize('shape', [(37, 53, 64), (18, 26, 128), (9, 13, 256), (4, 6, 512), (2, 3, 8)], ids=lambda s: '%dx%dx%d' % s)
def test_pool_exact(shape):
    K.check_pool(None, DEV, *shape)


@pytest.mark.parametrize('pc', [(37 * 53, 64), (18 * 26, 128), (9 * 13, 256), (4 * 6, 512), (1, 512), (32 * 600, 64)], ids=lambda s: 'P%d-C%d' % s)
def test_head_fp64(pc):
    K.check_head(None, DEV, *pc)


@pytest.mark.parametrize('hw', [(75, 107), (33, 32), (64, 96)], ids=lambda s: '%dx%d' % s)
def test_resize_and_adjoint(hw):
    K.check_resize(None, DEV, *hw)


@pytest.mark.parametrize('weight', [1.0, 1e-3])
def test_value_grad_end_to_end(weight):
    K.check_e2e(None, DEV, K.FULL, *FRAME, weight=weight)


def test_value_grad_smallest_frame():
    K.check_e2e(None, DEV, K.FULL, 33, 32)


def test_dropin_sim_loss():
    K.check_dropin(None, DEV, K.FULL, 33, 32)


def test_refusals():
    K.check_refusals(None, DEV)


@pytest.fixture(scope='module')
def b32():
    import warnings
    from aphantasia_amd import clip as aclip
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return aclip.load('ViT-B/32', seed=1, max_batch=4)[0]


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
def test_engine_sync_term(b32, use_graph):
    K.check_engine(None, DEV, b32, K.FULL, 64, 96, 4, use_graph=use_graph)


def test_engine_without_the_term_issues_the_parent_commits_calls(b32):
    assert K.engine_call_sequence(None, DEV, b32, 64, 96, 4) == K.PARENT_STEP_CALLS


def test_clip_fft_sync_runs(tmp_path, capsys):
    """clip_fft.py -t .. -i IMG --sync 1 on synthetic weights and on local weight files; --sync without a readable -i prints the no-op line"""
    import os
    import warnings
    import numpy as np
    import torch
    from PIL import Image
    import clip_fft
    from aphantasia_amd import lpips as alpips
    img = os.path.join(tmp_path, 'in.png')
    Image.fromarray((np.random.default_rng(0).random((48, 80, 3)) * 255).astype(np.uint8)).save(img)
    base = ['-t', 'cat', '-nv', '--seed', '0', '--steps', '2', '--samples', '8', '--size', '96-64', '--no_save']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        clip_fft.main(base + ['-i', img, '--sync', '1', '--out_dir', os.path.join(tmp_path, 'o1')])
        assert 'the term is off' not in capsys.readouterr().out
        w = alpips.synthetic_weights(alpips.WIDTHS, 5)
        vgg, lp = os.path.join(tmp_path, 'vgg16.pth'), os.path.join(tmp_path, 'vgg.pth')
        torch.save({k: v for k, v in w.items() if k.startswith('features.')}, vgg)
        torch.save({'lin%d.model.1.weight' % s: w['lin%d.weight' % s].view(1, -1, 1, 1) for s in range(5)}, lp)
        clip_fft.main(base + ['-i', img, '--sync', '1', '--vgg-weights', vgg, '--lpips-weights', lp, '--out_dir', os.path.join(tmp_path, 'o2')])
        clip_fft.main(base + ['-i', os.path.join(tmp_path, 'missing.png'), '--sync', '1', '--out_dir', os.path.join(tmp_path, 'o3')])
    assert 'the term is off' in capsys.readouterr().out
