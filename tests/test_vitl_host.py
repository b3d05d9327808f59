"""CPU, no kernels: the host logic of the ViT-L/14 tower -- its config, the CLIs' choices and derating, the checkpoint loader on
ViT-L/14 shapes, the padded patch-row length."""
import pytest
import torch

from aphantasia_amd import ops


def test_visual_config_vit_l14():
    from aphantasia_amd.weights import VIT_CONFIGS, visual_config
    cfg = visual_config('ViT-L/14')
    assert tuple(cfg.values()) == (224, 14, 1024, 24, 16, 768) == tuple(VIT_CONFIGS['ViT-L/14'].values())
    assert (cfg['input_resolution'] // cfg['patch_size']) ** 2 + 1 == 257 and cfg['heads'] * 64 == cfg['width']
    cfg['layers'] = 1
    assert visual_config('ViT-L/14')['layers'] == 24          # a copy


def test_patch_row_elems():
    assert [ops.patch_row_elems(p) for p in (32, 16, 14)] == [3072, 768, 640]
    assert all(ops.patch_row_elems(p) % 128 == 0 and 0 <= ops.patch_row_elems(p) - 3 * p * p < 128 for p in range(1, 65))
    assert ops.patch_row_elems(0) == 0


def test_clip_fft_choice_and_derating():
    import clip_fft
    a = clip_fft.get_args(['-t', 'x', '-m', 'ViT-L/14'])
    assert a.model == 'ViT-L/14' and 'ViT-L/14' in clip_fft.clip_models
    assert clip_fft.derate_samples(a) == 7                                            # int(200 * 0.04) = 8 -> int(8 * 0.95)  (illustra.py:97)
    assert clip_fft.derate_samples(clip_fft.get_args(['-t', 'x', '-m', 'ViT-L/14', '-tf', 'none'])) == 8
    a = clip_fft.get_args(['-t', 'x', '-m', 'ViT-L/14', '-dm', '2'])                  # -dm is unchanged: it selects ViT-B/32
    assert a.model == 'ViT-B/32' and clip_fft.derate_samples(a) == 43


def test_illustrip_choice_and_derating():
    import illustrip
    a = illustrip.get_args(['-t', 'x', '-m', 'ViT-L/14'])
    assert a.model == 'ViT-L/14' and illustrip.derate_samples(a) == int(int(a.samples * 0.04) * 0.95)


def test_cppn_keeps_its_refusal_and_says_why():
    import cppn
    assert 'ViT-L/14' in cppn.__doc__ and 'follow-up' in cppn.__doc__


def test_checkpoint_loader_roundtrip_vit_l14_shapes(tmp_path):
    """a synthetic state dict in OpenAI key layout with ViT-L/14 shapes at 2 layers: the loader derives the config from the tensors"""
    from aphantasia_amd.weights import load_openai_checkpoint, stress_visual_weights, synthetic_visual_weights, visual_config
    cfg = visual_config('ViT-L/14')
    cfg['layers'] = 2
    w = synthetic_visual_weights(cfg, 5)
    assert w['conv1.weight'].shape == (1024, 3, 14, 14) and w['positional_embedding'].shape == (257, 1024) and w['proj'].shape == (1024, 768)
    ws = stress_visual_weights(cfg, 5)
    assert set(ws) == set(w) and all(ws[k].shape == w[k].shape for k in w)
    sd = {'visual.' + k: v.half() for k, v in w.items()}
    sd['logit_scale'] = torch.tensor(4.6)
    path = str(tmp_path / 'vit_l14_2layers.pt')
    torch.save(sd, path)
    vis, got, full = load_openai_checkpoint(path)
    assert got == cfg
    assert set(vis) == set(w) and all(torch.equal(vis[k], w[k]) for k in w)          # (f16-representable values: the round trip is exact)
    assert 'logit_scale' in full


def test_clip_load_default_batch():
    from aphantasia_amd import clip as aclip
    assert aclip.DEFAULT_MAX_BATCH == {'ViT-L/14': 32}
    import inspect
    assert inspect.signature(aclip.load).parameters['max_batch'].default is None
