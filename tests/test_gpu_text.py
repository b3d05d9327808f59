"""GPU (MI355X): the CLIP text tower -- the causal fp32 attention element-wise against fp64 with its bit properties, aph_text_forward against
the fp64 restatement (tests/text_ref.py) at the tiny configuration and at the full-size ViT-B/32 and ViT-L/14 text towers on synthetic
weights, the C ABI's refusals, and encode_text / text_embedding on the device.  The checks are text_checks.py's, shared with test_emu_text.py."""
import gzip

import pytest
import torch

from aphantasia_amd import _ffi
import text_checks as C
import text_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _show(tag, ratios):
    print('%s: worst err / bound  %s' % (tag, '  '.join('%s %.3f' % kv for kv in ratios.items())))


@pytest.mark.parametrize('T', [1, 31, 32, 33, 64, 65, 77, 256])
def test_attention_causal_vs_fp64(T):
    _show('causal fp32 T=%d normal' % T, C.check_attention_causal(None, DEV, S=2 if T <= 65 else 1, T=T, heads=2, seed=T))


@pytest.mark.parametrize('kind', [k for k in C.V.ATTN_KINDS if k != 'normal'])
def test_attention_causal_families_vs_fp64(kind):
    _show('causal fp32 T=77 %s' % kind, C.check_attention_causal(None, DEV, S=1, T=77, heads=2, kind=kind, seed=3))


@pytest.mark.parametrize('ctx', [77, 9])
def test_text_tower_vs_fp64(ctx):
    C.check_tower(None, DEV, dict(C.TINY, context_length=ctx), tag='MI355X tiny')


def test_text_tower_b32_vs_fp64():
    """the ViT-B/32 (and B/16) text tower at full size, synthetic weights: ctx 77, width 512, 8 heads, 12 layers, vocabulary 49408, S = 3"""
    C.check_tower(None, DEV, C.B32, eots=[1, 38, 76], tag='MI355X B/32 text')


def test_text_tower_l14_vs_fp64():
    """the ViT-L/14 text tower: width 768, 12 heads, 12 layers, S = 1"""
    C.check_tower(None, DEV, C.L14, eots=[20], tag='MI355X L/14 text')


def test_text_refusals():
    C.check_refusals(_ffi.lib(), DEV)


def test_encode_text_on_device(tmp_path):
    """CLIPModel.encode_text / text_embedding on the product library: device tensors out, the interpreter test's gate"""
    from aphantasia_amd import clip as aclip
    from aphantasia_amd.weights import synthetic_text_weights, synthetic_visual_weights, text_weights
    merges = ['t h', 'th e</w>', 'c a', 'ca t</w>', 'a n', 'i n', 'in g</w>']
    vocab = tmp_path / aclip.BPE_VOCAB_NAME
    with gzip.open(vocab, 'wb') as f:
        f.write(('#version: 0.2\n' + '\n'.join(merges) + '\n').encode())
    vis_cfg = dict(input_resolution=32, patch_size=16, width=256, layers=1, heads=4, output_dim=128)
    cfg = dict(C.TINY, vocab_size=521)
    vis = synthetic_visual_weights(vis_cfg, 3)
    full = {'visual.' + k: v for k, v in vis.items()}
    full.update(synthetic_text_weights(cfg, 4))
    model = aclip.CLIPModel('tiny', vis_cfg, vis, full, max_batch=1, weights_path=str(tmp_path / 'ViT-tiny.pt'))
    prompts = ['the cat in the can', 'thing', '']
    tokens = aclip.tokenize(prompts, bpe_vocab=str(vocab), vocab_size=521)
    enc = model.encode_text(tokens)
    assert enc.is_cuda and enc.dtype == torch.float32 and enc.shape == (3, 128)
    w = text_weights(full)
    want = text_ref.encode_text({k: v.double() for k, v in w.items()}, tokens, cfg)
    e32 = (text_ref.encode_text(w, tokens, cfg).double() - want).abs().max().item()
    err = (enc.cpu().double() - want).abs().max().item()
    print('encode_text on the device: max |kernel - fp64| %.3e, fp32 restatement %.3e' % (err, e32))
    assert err <= C.GATE * e32, (err, e32)
    emb = aclip.text_embedding(model, prompts[0])          # the vocabulary beside the checkpoint path
    assert emb.is_cuda and torch.equal(emb[0], enc[0])
    model.release_text()
    assert model._text is None
