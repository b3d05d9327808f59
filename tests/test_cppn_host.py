"""CPU: host side of the CPPN generator (aphantasia_amd/cppn.py, cppn.py) against tests/golden/cppn_ref.npz, which tools/make_cppn_golden.py
wrote from the reference's own classes: the restatement the kernel checks rest on, the seeded initialisation, the coordinate tables, the
`.npy` snapshot format, the parameter count and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

from aphantasia_amd import _ffi
from aphantasia_amd import cppn as C
import cppn_checks as K

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
ACTS = ['unbias', 'comp', 'relu']
NCASES = 4


@pytest.fixture(scope='module')
def ref(golden):
    return golden('cppn_ref.npz')


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


def case(ref, k):
    h, w, layers, nf, act = (int(v) for v in ref['c%d_cfg' % k])
    return h, w, layers, nf, ACTS[act], {n: ref['c%d_%s' % (k, n)] for n in ('seed', 'params', 'tail', 'mgrid', 'img64', 'drgb', 'grad64')}


def split(flat, layers, nf, actfn):
    views, o = [], 0
    for i, n in C.layer_table(layers, nf, actfn):
        views += [flat[o:o + i * n].view(n, i, 1, 1), flat[o + i * n:o + i * n + n]]
        o += i * n + n
    assert o == flat.numel()
    return views


@pytest.mark.parametrize('k', range(NCASES))
def test_restatement_matches_the_reference_in_fp64(ref, k):
    """cppn_checks.net_forward, image and gradient, to 1e-12 of the reference's CPPN evaluated in float64"""
    h, w, layers, nf, actfn, g = case(ref, k)
    mg = torch.from_numpy(g['mgrid'])
    xs, ys = mg[0, 0, 0, :], mg[0, 1, :, 0]
    views = split(torch.from_numpy(g['params']), layers, nf, actfn)
    img, grads = K.net_image_and_grad(views, xs, ys, actfn, torch.from_numpy(g['drgb']), torch.float64)
    assert (img - torch.from_numpy(g['img64'])).abs().max().item() <= 1e-12
    got, want = torch.cat([x.reshape(-1) for x in grads]), torch.from_numpy(g['grad64'])
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('k', range(NCASES))
def test_seeded_init_and_grid_are_the_references(ref, emu, k):
    """torch.manual_seed(seed); cppn_image(...) leaves the reference's weights bit for bit and has consumed the same draws; xs / ys are its mgrid"""
    h, w, layers, nf, actfn, g = case(ref, k)
    torch.manual_seed(int(g['seed']))
    params, gen, size = C.cppn_image([1, 3, h, w], layers, nf, actfn, device='cpu', lib=emu)
    tail = torch.rand(3)
    assert size is None and gen.synth.numel == g['params'].size == C.param_count(layers, nf, actfn)
    assert np.array_equal(gen.flat.numpy().view(np.int32), g['params'].view(np.int32))
    assert np.array_equal(tail.numpy(), g['tail'])
    assert [tuple(p.shape) for p in params] == list(gen.synth.shapes) and all(p.requires_grad and p.is_leaf for p in params)
    assert np.array_equal(np.broadcast_to(gen.synth.xs.numpy()[None, :], (h, w)).view(np.int32), g['mgrid'][0, 0].view(np.int32))
    assert np.array_equal(np.broadcast_to(gen.synth.ys.numpy()[:, None], (h, w)).view(np.int32), g['mgrid'][0, 1].view(np.int32))


def test_state_dict_keys(ref, emu):
    h, w, layers, nf, actfn, g = case(ref, NCASES - 1)
    _, gen, _ = C.cppn_image([1, 3, h, w], layers, nf, actfn, device='cpu', lib=emu)
    assert list(gen.state_dict().keys()) == [str(s) for s in ref['keys']]


def test_param_count():
    assert C.param_count(10, 24, 'unbias') == 10803 and C.param_count(10, 24, 'relu') == 72 + 9 * 600 + 75
    assert C.param_count(1, 8, 'comp') == 24 + 51


def test_snapshot_round_trip_and_reference_arrays(ref, emu, tmp_path):
    """export_data -> load_cppn returns the parameters; the reference's own export_data arrays load to the golden parameters; --resume path"""
    h, w, layers, nf, actfn, g = case(ref, 0)
    arrays = [ref['export_%d' % i] for i in range(int(ref['export_n']))]
    flat, l2, nf2, act2 = C.arrays_to_flat(arrays)
    assert (l2, nf2, act2) == (layers, nf, actfn)
    assert np.array_equal(flat.numpy().view(np.int32), g['params'].view(np.int32))
    _, gen, _ = C.cppn_image([1, 3, h, w], resume=arrays, device='cpu', lib=emu)
    assert (gen.synth.layers, gen.synth.nf, gen.synth.actfn) == (layers, nf, actfn) and torch.equal(gen.flat, flat)
    C.export_data(gen.state_dict(), str(tmp_path / 'snap'))
    back = np.load(str(tmp_path / 'snap.npy'), allow_pickle=True)
    assert len(back) == len(arrays) and all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(back, arrays))
    _, gen2, _ = C.cppn_image([1, 3, h, w], 2, 4, 'unbias', resume=str(tmp_path / 'snap.npy'), device='cpu', lib=emu)
    assert torch.equal(gen2.flat, flat)
    # relu is recognised by the second conv's input width (cppn.py:122)
    torch.manual_seed(1)
    _, gr, _ = C.cppn_image([1, 3, 4, 4], 3, 6, 'relu', device='cpu', lib=emu)
    C.export_data(gr.state_dict(), str(tmp_path / 'relu'))
    fr, l3, nf3, act3 = C.load_cppn(str(tmp_path / 'relu.npy'))
    assert (l3, nf3, act3) == (3, 6, 'relu') and torch.equal(fr, gr.flat)


def test_cli_defaults_derating_and_refusals(capsys):
    import cppn
    a = cppn.get_args(['-t', 'x'])
    assert a.size == [512, 512] and a.samples == 50 and a.lrate == 0.003 and (a.layers, a.nf, a.actfn) == (10, 24, 'unbias')
    assert (a.align, a.fstep, a.model, a.steps, a.macro, a.aest, a.transform, a.dualmod) == ('overscan', 1, 'ViT-B/32', 200, 0.4, 0., False, None)
    assert cppn.derate_samples(a) == 50
    assert cppn.get_args(['-t', 'x', '--size', '640-360']).size == [360, 640]
    assert cppn.derate_samples(cppn.get_args(['-t', 'x', '-m', 'ViT-B/16'])) == 12            # cppn.py:197-199
    a = cppn.get_args(['-t', 'x', '-dm', '2', '-m', 'ViT-B/16'])
    assert a.model == 'ViT-B/32' and cppn.derate_samples(a) == 34                             # cppn.py:66-67, 203
    assert cppn.derate_samples(cppn.get_args(['-t', 'x', '-tf'])) == 47                       # cppn.py:221
    for argv, word in ((['-sh', '0.5'], 'Sobel'), (['-ex'], 'shader export'), (['-tr'], 'translat'), (['-m', 'RN50'], 'RN50'),
                       (['-m', 'RN50x64'], 'RN50x64'), (['-m', 'ViT-L/14'], 'ViT-L/14')):
        with pytest.raises(SystemExit) as e:
            cppn.get_args(['-t', 'x'] + argv)
        assert word in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit):
        cppn.get_args(['-h'])
    assert 'transforms_fast' in capsys.readouterr().out           # what -tf means here is said in the help text
