"""CPU: host logic of `-tf custom` / `-tf elastic` -- the draws consume torch's and numpy's global streams exactly as the reference's
closures do (transforms.py:17-33,53-71,147-163), the packed augment rows, the bulk draws' distributions, the CLIs, encode_image's window
and the C ABI's refusals (through the interpreter build: no GPU here)."""
import os
import sys

import numpy as np
import pytest
import torch

from aphantasia_amd import _ffi, transforms
from aphantasia_amd.utils import draw_crop_params
from oracle import augment_ref, shim
from oracle import reference_path as R

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
ANGLES = list(range(-30, 30)) + 20 * [0]                      # transforms.py:150,160


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)


def literal_draw(elastic, P, log):
    """The random draws of ONE call of upstream's composed closure on a [1,3,P-8,P-8] cut, transcribed line by line, in order:
    transforms.py:149 T.RandomErasing(0.2) on the padded [1,3,P,P] canvas (torchvision forward: `torch.rand(1) < p`, then get_params),
    :57 `np.random.choice(angles)`, :19-21 random_elastic's `np.random.rand(2)`, `np.random.randint(8,64)`, `np.random.rand()` (which
    only shape a displacement of zeros), :30-31 jitter's `dx = np.random.choice(d)`, `dy = np.random.choice(d)`."""
    prm = dict(erase=None)
    if elastic:
        if torch.rand(1) < 0.2:
            prm['erase'] = augment_ref.erase_get_params(P, P)
    prm['angle'] = float(np.random.choice(ANGLES))
    if elastic:
        a = np.random.rand(2)
        k = np.random.randint(8, 64) * 2 + 1
        s = k / (np.random.rand() + 2.)
        log.append((tuple(a), k, s))
    dx = np.random.choice(8)
    dy = np.random.choice(8)
    prm['shift'] = (int(dx), int(dy))
    return prm


def rng_states():
    return torch.get_rng_state(), np.random.get_state()


def same_states(a, b):
    return torch.equal(a[0], b[0]) and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


@pytest.mark.parametrize('chain', ['custom', 'elastic'])
def test_draws_consume_the_reference_streams(chain):
    """draw() == the literal transcription, interleaved with the crop draws where upstream calls transform(cut) (utils.py:251); afterwards
    both global generators are in the same state"""
    tf = getattr(transforms, 'transforms_' + chain)
    elastic = chain == 'elastic'
    assert tf.geometric and tf.kind == (_ffi.APH_TF_ELASTIC if elastic else _ffi.APH_TF_CUSTOM) and tf.out_side(224) == 232
    nerase = 0
    for seed in range(8):
        for (h, w, size) in [(720, 1280, 224), (48, 80, 16)]:
            seed_all(seed)
            want, wasted = [], []
            table_w = R.draw_crop_table(24, size, h, w, 'uniform', 0.4, per_cut_hook=lambda c: want.append(literal_draw(elastic, size + 8, wasted)))
            end_w = rng_states()
            seed_all(seed)
            table_g, got = draw_crop_params(24, size, h, w, 'uniform', 0.4, tf)
            end_g = rng_states()
            assert np.array_equal(table_w, table_g)
            assert [(p['angle'], p['erase'], tuple(p['shift'])) for p in got] == [(p['angle'], p['erase'], p['shift']) for p in want]
            assert same_states(end_w, end_g)
            assert len(wasted) == (24 if elastic else 0)
            nerase += sum(p['erase'] is not None for p in got)
            for p in got:
                if p['erase'] is not None:              # drawn on the padded canvas: may reach past the cut's own side
                    i, j, eh, ew = p['erase']
                    assert 0 <= i and i + eh <= size + 8 and 0 <= j and j + ew <= size + 8
    assert (nerase > 20) == elastic and (nerase == 0) != elastic


@pytest.mark.skipif(not shim.available(), reason='the reference tree is not present')
@pytest.mark.parametrize('chain', ['custom', 'elastic'])
def test_draws_against_the_reference_closures_under_recording_stubs(chain, monkeypatch):
    """the reference's transforms.py imported in place (oracle/shim.py) with its kornia stub modules given functions that only RECORD their
    arguments and return the image: `transforms_custom` itself; for elastic its own pad / random_rotate / random_elastic / jitter factories
    around the one stage that is torchvision's (T.RandomErasing, a stub object in the imported module: its draws are the oracle's
    erase_get_params transcription)"""
    ref = shim.load_reference().transforms
    rec = []
    K = ref.K
    geometry = sys.modules['kornia.geometry']
    for obj, name, val in ((K, 'get_rotation_matrix2d', lambda center, angle, scale: rec.append(('angle', float(angle[0]))) or torch.zeros(1, 2, 3)),
                           (K, 'warp_affine', lambda img, M, dsize: img),
                           (K, 'translate', lambda img, t: rec.append(('shift', tuple(int(v) for v in t[0]))) or img),
                           (K, 'elastic_transform2d', lambda x, noise, k, s, a: rec.append(('noise', float(noise.abs().sum()), tuple(x.shape))) or x),
                           (geometry, 'transform', K), (ref.kornia, 'geometry', geometry)):
        monkeypatch.setattr(obj, name, val, raising=False)          # undone after the test: the shim's modules are shared by the process
    elastic = chain == 'elastic'
    tf = getattr(transforms, 'transforms_' + chain)

    def erasing(x):
        if torch.rand(1) < 0.2:
            rec.append(('erase', augment_ref.erase_get_params(x.shape[-2], x.shape[-1])))
        return x
    upstream = ref.transforms_custom if not elastic else ref.compose(
        [ref.pad(4, mode='constant', constant_value=0.5), erasing, ref.random_rotate(ANGLES), ref.random_elastic(), ref.jitter(8)])
    size = 32
    cut = torch.rand(1, 3, size, size)
    seed_all(3)
    for _ in range(40):
        upstream(cut)
    end_w = rng_states()
    seed_all(3)
    got = [tf.draw(size) for _ in range(40)]
    assert same_states(end_w, rng_states())
    assert [r[1] for r in rec if r[0] == 'angle'] == [p['angle'] for p in got]
    assert [r[1] for r in rec if r[0] == 'shift'] == [tuple(p['shift']) for p in got]
    assert [r[1] for r in rec if r[0] == 'erase'] == [p['erase'] for p in got if p['erase'] is not None]
    noise = [r for r in rec if r[0] == 'noise']
    assert len(noise) == (40 if elastic else 0) and all(r[1] == 0.0 and r[2] == (1, 3, size + 8, size + 8) for r in noise)


def test_pack_aug_rows():
    prms = [dict(persp=None, erase=None, angle=0.0, shift=(0, 0)), dict(persp=None, erase=(3, 0, 1, 39), angle=-30.0, shift=(7, 2)),
            dict(persp=None, erase=None, angle=17.0, shift=(2, 7))]
    t = transforms.pack_aug(prms)
    assert tuple(t.shape) == (3, _ffi.APH_AUG_STRIDE) and t.dtype == torch.float32
    assert t[:, 0].tolist() == [0, 7, 2] and t[:, 1].tolist() == [0, 2, 7]            # [0] dx, [1] dy
    assert (t[:, 2:9] == 0).all()                                                      # [8] = 0: no perspective stage
    assert t[1, 9:13].tolist() == [3, 0, 1, 39] and (t[0, 9:13] == 0).all()            # [9..12] the rectangle on the padded canvas
    assert t[:, 15].tolist() == [0, 1, 1]                                              # the zero-angle cut copies
    c, s = np.cos(np.radians(-30.0)), np.sin(np.radians(-30.0))
    assert abs(t[1, 13].item() - c) < 1e-7 and abs(t[1, 14].item() - s) < 1e-7 and t[0, 13].item() == 1.0 and t[0, 14].item() == 0.0
    for bad in ((8, 0), (0, -1)):
        with pytest.raises(ValueError, match='jitter'):
            transforms.pack_aug([dict(angle=0.0, shift=bad)])
    fast = transforms.pack_aug([dict(persp=None, erase=(1, 2, 3, 4), angle=5.0)])      # the rows of -tf fast are what they were
    assert fast[0, 0].item() == 0 and fast[0, 9:13].tolist() == [1, 2, 3, 4] and fast[0, 15].item() == 1


@pytest.mark.parametrize('chain', ['custom', 'elastic'])
def test_bulk_draws_ranges_and_frequencies(chain):
    fn = transforms.draw_elastic_bulk if chain == 'elastic' else transforms.draw_custom_bulk
    S, size = 40000, 224
    t = fn(S, size, np.random.default_rng(5))
    assert t.shape == (S, 16) and t.dtype == np.float32
    assert np.array_equal(getattr(transforms, 'transforms_' + chain).draw_bulk(64, size, np.random.default_rng(9)), fn(64, size, np.random.default_rng(9)))
    for col in (0, 1):                                  # dx, dy uniform on 0 .. 7: each value 1/8 +- 5 sigma
        v = t[:, col]
        assert np.array_equal(v, np.floor(v)) and v.min() == 0 and v.max() == 7
        freq = np.bincount(v.astype(np.int64), minlength=8) / S
        assert np.abs(freq - 0.125).max() < 5 * np.sqrt(0.125 * 0.875 / S)
    assert not t[:, 2:9].any()
    zero = (t[:, 15] == 0)
    assert abs(zero.mean() - 21 / 80) < 5 * np.sqrt((21 / 80) * (59 / 80) / S)          # 20 explicit zeros + the 0 of range(-30, 30)
    ang = np.degrees(np.arctan2(t[:, 14].astype(np.float64), t[:, 13].astype(np.float64)))
    assert ang.min() > -30.01 and ang.max() < 29.01 and np.abs(ang - np.rint(ang)).max() < 1e-4 and len(np.unique(np.rint(ang))) == 60
    erased = t[:, 11] > 0
    if chain == 'custom':
        assert not erased.any() and not t[:, 9:13].any()
    else:
        P = size + 8
        assert abs(erased.mean() - 0.2) < 5 * np.sqrt(0.2 * 0.8 / S)
        e = t[erased]
        assert (e[:, 9] >= 0).all() and (e[:, 9] + e[:, 11] <= P).all() and (e[:, 10] + e[:, 12] <= P).all() and (e[:, 11] < P).all() and (e[:, 12] < P).all()
        area = e[:, 11] * e[:, 12] / (P * P)
        assert 0.015 < area.min() and area.max() < 0.34 and (e[:, 9] + e[:, 11]).max() > size      # on the padded canvas, not the cut


def test_alias_package_and_cli_selection():
    import aphantasia.transforms as alias
    assert alias.transforms_custom is transforms.transforms_custom and alias.transforms_elastic is transforms.transforms_elastic
    import clip_fft
    import illustrip
    for name, want in (('custom', transforms.transforms_custom), ('elastic', transforms.transforms_elastic), ('fast', transforms.transforms_fast)):
        a = clip_fft.get_args(['-t', 'x', '-tf', name])
        assert clip_fft.pick_transform(a.transform) is want
        assert clip_fft.derate_samples(a) == int(200 * 0.95)                            # clip_fft.py:124-125: the derating was already there
        b = illustrip.get_args(['-t', 'x', '-tf', name])
        illustrip.check_supported(b)                                                    # no SystemExit
        assert clip_fft.pick_transform(b.transform) is want
    assert isinstance(clip_fft.pick_transform('none'), transforms.Transform) and not clip_fft.pick_transform('none').geometric
    with pytest.raises(SystemExit, match='--aest'):
        illustrip.check_supported(illustrip.get_args(['-t', 'x', '--aest', '1']))
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'clip_fft.py')).read()
    assert 'is not provided' not in src


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


def test_encode_image_takes_the_window_of_the_padded_canvas(emu):
    """[S,3,R+8,R+8] (what the custom / elastic chains return, as upstream) encodes as its top-left R x R window -- what conv1 with
    stride = kernel = patch reads of it -- with zero gradient outside; any other side still raises (225 and 240 among them)"""
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.weights import synthetic_visual_weights, visual_config
    cfg = dict(input_resolution=32, patch_size=16, width=256, layers=2, heads=4, output_dim=128)
    model = CLIPModel('tiny', cfg, synthetic_visual_weights(cfg, 3), None, max_batch=2, lib=emu)
    x = torch.randn(2, 3, 40, 40, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    enc = model.encode_image(x)
    want = model.encode_image(x.detach()[:, :, :32, :32].contiguous())
    assert torch.equal(enc.detach(), want)
    enc.square().sum().backward()
    assert x.grad[:, :, :32, :32].abs().max().item() > 0 and x.grad[:, :, 32:, :].abs().max().item() == 0 and x.grad[:, :, :, 32:].abs().max().item() == 0
    for side in (33, 39, 41, 48, 31):
        with pytest.raises(ValueError, match='encode_image expects'):
            model.encode_image(torch.zeros(1, 3, side, side))
    with pytest.raises(ValueError):
        model.encode_image(torch.zeros(1, 3, 40, 32))
    # the real towers: 232 is taken, 225 and 240 are not (no weights needed to say so)
    from aphantasia_amd.clip import VisualTransformer
    for name in ('ViT-B/32', 'ViT-B/16'):
        v = VisualTransformer.__new__(VisualTransformer)
        c = visual_config(name)
        v.input_resolution, v.patch_size = c['input_resolution'], c['patch_size']
        for side in (225, 240):
            with pytest.raises(ValueError, match='encode_image expects'):
                v(torch.zeros(1, 3, side, side))


def test_slice_imgs_returns_the_padded_canvas_with_autograd(emu, monkeypatch):
    """utils.slice_imgs(transform=transforms_custom | _elastic) -> [S,3,size+8,size+8] as upstream, differentiable (through the interpreter
    build: the product path insists on GPU tensors)"""
    from aphantasia_amd import ops, utils
    monkeypatch.setattr(ops, '_L', lambda lib, *t: emu)
    monkeypatch.setattr(_ffi, 'lib', lambda: emu)
    img = torch.rand(1, 3, 40, 56, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    for tf in (transforms.transforms_custom, transforms.transforms_elastic):
        seed_all(7)
        out = utils.slice_imgs([img], 3, 32, tf, 'uniform', 0.4, patch=16)[0]
        assert tuple(out.shape) == (3, 3, 40, 40)
        img.grad = None
        out.sum().backward()
        assert img.grad is not None and img.grad.abs().max().item() > 0


def test_c_abi_refusals(emu):
    import tf_checks
    tf_checks.check_refusals(emu, 'cpu')


@pytest.mark.parametrize('chain', ['custom', 'elastic'])
def test_engine_selects_the_chain_for_workspace_and_shards(emu, chain):
    """Engine(transform=...) sizes its sampler workspace by the chain kind and the shard's cut count, and a rank uploads its own rows of the
    augment table (rank 1 of 2 over 5 cuts: rows 3..4), from per-cut dicts and from a bulk-drawn table alike"""
    import ctypes
    from aphantasia_amd import ops
    from aphantasia_amd.clip import CLIPModel
    from aphantasia_amd.engine import Engine
    from aphantasia_amd.weights import synthetic_visual_weights
    cfg = dict(input_resolution=32, patch_size=16, width=256, layers=2, heads=4, output_dim=128)
    model = CLIPModel('tiny', cfg, synthetic_visual_weights(cfg, 3), None, max_batch=5, lib=emu)
    tf = getattr(transforms, 'transforms_' + chain)
    seed_all(0)
    params = R.fft_params_init([1, 3, 40, 56]).contiguous()
    eng = Engine(params, 40, 56, model, 5, [(torch.randn(1, 128), -1.0)], transform=tf, lib=emu, rank=1, world=2, rng='reference')
    assert eng.tf == tf.kind and (eng.lo, eng.hi) == (3, 5) and eng.geom.S == 2
    assert eng.tmp.numel() * 4 >= emu.cdll.aph_sample_ws_bytes_tf(ctypes.byref(eng.geom), tf.kind) > emu.cdll.aph_sample_ws_bytes(ctypes.byref(eng.geom), 0)
    table, augs = eng.draw()
    want = transforms.pack_aug([dict(a) for a in augs])
    eng.inputs.upload(eng._step_items(ops.adam_hyper(1, 0.05), table, augs, None, None))
    assert torch.equal(eng.aug, want[3:5]) and torch.equal(eng.table, torch.from_numpy(table[3:5]))
    bulk = tf.draw_bulk(5, 32, np.random.default_rng(1))
    eng.inputs.upload(eng._step_items(ops.adam_hyper(1, 0.05), table, bulk, None, None))
    assert torch.equal(eng.aug, torch.from_numpy(bulk[3:5]))
