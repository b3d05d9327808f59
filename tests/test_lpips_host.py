"""CPU, no kernels: the LPIPS weight loader (aphantasia_amd/lpips.py) and the --sync command line of clip_fft.py."""
import os
import warnings

import pytest
import torch

from aphantasia_amd import lpips as alpips

NARROW = (16, 16, 32, 32, 32)


def _files(tmp_path, widths, lin_format):
    w = alpips.synthetic_weights(widths, 3)
    vgg, lp = os.path.join(tmp_path, 'vgg16.pth'), os.path.join(tmp_path, 'vgg.pth')
    sd = {k: v for k, v in w.items() if k.startswith('features.')}
    sd['classifier.0.weight'] = torch.zeros(4, 4)                  # the rest of a torchvision vgg16 state dict is ignored
    torch.save(sd, vgg)
    torch.save({lin_format % s: w['lin%d.weight' % s].view(1, -1, 1, 1) for s in range(5)}, lp)
    return w, vgg, lp


def test_layer_table_is_vgg16():
    t = alpips.layer_table()
    assert [i for i, _, _, _ in t] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [(a, b) for _, a, b, _ in t] == [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                                            (512, 512), (512, 512), (512, 512)]
    assert len(alpips.weight_shapes()) == 31 and alpips.weight_shapes()['lin2.weight'] == (256,)


@pytest.mark.parametrize('lin_format', ['lin%d.model.1.weight', 'lin%d.weight'])
def test_loader_maps_both_file_formats(tmp_path, lin_format):
    w, vgg, lp = _files(tmp_path, NARROW, lin_format)
    got = alpips.load_weights(vgg, lp, NARROW)
    assert set(got) == set(w)
    for k in w:
        assert got[k].dtype == torch.float32 and torch.equal(got[k], w[k]), k


def test_loader_refuses_wrong_shape_missing_key_and_half_a_pair(tmp_path):
    w, vgg, lp = _files(tmp_path, NARROW, 'lin%d.model.1.weight')
    with pytest.raises(ValueError, match='features.0.weight'):
        alpips.load_weights(vgg, lp)                                   # a narrow file against the VGG-16 widths
    sd = torch.load(vgg, weights_only=True)
    del sd['features.28.bias']
    torch.save(sd, vgg)
    with pytest.raises(KeyError, match='features.28.bias'):
        alpips.load_weights(vgg, lp, NARROW)
    bad = torch.load(lp, weights_only=True)
    bad['lin1.model.1.weight'] = torch.zeros(1, 8, 1, 1)
    torch.save(bad, lp)
    sd['features.28.bias'] = torch.zeros(32)
    torch.save(sd, vgg)
    with pytest.raises(ValueError, match='lin1'):
        alpips.load_weights(vgg, lp, NARROW)
    with pytest.raises(ValueError, match='BOTH'):
        alpips.load_weights(vgg, None, NARROW)


def test_synthetic_fallback_warns_and_is_seeded():
    with pytest.warns(UserWarning, match='SYNTHETIC'):
        a = alpips.load_weights(widths=NARROW, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        b = alpips.load_weights(widths=NARROW, seed=4)
    assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(alpips.weight_shapes(NARROW))
    assert all(float(a['lin%d.weight' % s].min()) >= 0 for s in range(5))


def test_product_term_refuses_cpu():
    with pytest.raises(RuntimeError, match='no CPU'):
        alpips.LPIPS(alpips.synthetic_weights(NARROW, 0), 64, 64, device='cpu', widths=NARROW)


def test_cli_sync_arguments():
    import clip_fft
    a = clip_fft.get_args(['-t', 'x', '-i', 'img.jpg', '--sync', '1', '--steps', '2', '--samples', '8', '--no_save'])
    assert a.sync == 1 and a.align == 'overscan' and a.vgg_weights is None and a.lpips_weights is None          # clip_fft.py:102
    b = clip_fft.get_args(['-t', 'x', '-i', 'img.jpg', '--sync', '1', '--samples', '200', '--vgg-weights', 'v.pth', '--lpips-weights', 'l.pth'])
    c = clip_fft.get_args(['-t', 'x', '-i', 'img.jpg', '--samples', '200'])
    assert clip_fft.derate_samples(b) == int(clip_fft.derate_samples(c) * 0.5)                                  # clip_fft.py:158
    assert (b.vgg_weights, b.lpips_weights) == ('v.pth', 'l.pth') and c.align == 'uniform'
    assert [clip_fft.prog_sync(i, 4) for i in range(4)] == [1, .75, .5, .25]                                    # clip_fft.py:269


def test_engine_step_input_layouts_are_unchanged_without_the_term():
    from aphantasia_amd.engine import step_input_parts
    for geometric in (False, True):
        for second in (False, True):
            base = step_input_parts(7, geometric, second)
            assert step_input_parts(7, geometric, second, False) == base
            with_sync = step_input_parts(7, geometric, second, True)
            assert with_sync[:-1] == base and with_sync[-1] == ('sync', (1,), torch.float32)
