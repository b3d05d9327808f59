"""CPU: the CLIP text tower -- the reference restatement against transformers in fp64, the BPE tokenizer (hand-derived ids, agreement with
transformers.CLIPTokenizer, padding / overflow, file formats), and under the host SIMT interpreter (tests/emu) the causal fp32 attention, the
whole tower against fp64, the C ABI's refusals and the public surface (encode_text, tokenize, text_embedding, the CLIs' --bpe-vocab)."""
import gzip
import json
import os
import sys

import pytest
import torch

from aphantasia_amd import _ffi
from aphantasia_amd.tokenizer import Tokenizer, byte_symbols
import text_checks as C
import text_ref

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))

MERGES = ['t h', 'th e</w>', 'c a', 'ca t</w>', 'a n', 'i n', 'in g</w>']          # vocabulary size 512 + 7 + 2 = 521
VOCAB = 521
STRINGS = ["The cat, sitting in the can! it's 42 été", "a  photo\tof THE cat's hat...", 'than then the thething in-ing 1234 5.6',
           "don't we'll I'm they've you'd 'tis", 'ünïcödé straße — “quotes” ¿qué?', '  leading and trailing  ', 'x', '',
           'a_b c#d $100 50% (the) [cat] {in}', '日本語 the 猫', 'the the the ' * 30]


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.fixture(scope='module')
def vocab_file(tmp_path_factory):
    p = tmp_path_factory.mktemp('bpe') / 'bpe_simple_vocab_16e6.txt.gz'
    with gzip.open(p, 'wb') as f:
        f.write(('"bpe_simple_vocab_16e6.txt#version: 0.2\n' + '\n'.join(MERGES) + '\n').encode())
    return str(p)


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
def test_text_ref_vs_transformers():
    """text_ref.encode_text == transformers.CLIPTextModelWithProjection in fp64 (quick_gelu, in_proj split into q / k / v, eos = vocab - 1):
    2 layers, width 128, 2 heads, ctx 77, vocab 300, EOT at positions 1, 3 and 76; max-rel <= 1e-10"""
    tr = pytest.importorskip('transformers')
    from aphantasia_amd.weights import synthetic_text_weights
    cfg = dict(context_length=77, vocab_size=300, width=128, layers=2, heads=2, output_dim=64)
    w = {k: v.double() for k, v in synthetic_text_weights(cfg, 2).items()}
    g = torch.Generator().manual_seed(1)
    for k in w:                      # non-trivial biases and LayerNorm vectors, so that none of them can be dropped unnoticed
        if k.endswith('bias') or '.ln_' in k or k.startswith('ln_final'):
            w[k] = w[k] + 0.1 * torch.randn(w[k].shape, generator=g).double()
    hf_cfg = tr.CLIPTextConfig(vocab_size=300, hidden_size=128, intermediate_size=512, projection_dim=64, num_hidden_layers=2, num_attention_heads=2,
                               max_position_embeddings=77, hidden_act='quick_gelu', layer_norm_eps=1e-5, eos_token_id=299, bos_token_id=298,
                               pad_token_id=0, attn_implementation='sdpa')          # (its 'eager' attention rounds the softmax to float32: not an fp64 evaluation)
    model = tr.CLIPTextModelWithProjection(hf_cfg).double().eval()
    missing = model.load_state_dict(text_ref.to_transformers_state(w, cfg), strict=False)
    assert not missing.unexpected_keys and all('position_ids' in k for k in missing.missing_keys), missing
    tok = C.prompt_tokens(cfg, [1, 3, 76])
    with torch.no_grad():
        want = model(input_ids=tok.long()).text_embeds
    got = text_ref.encode_text(w, tok, cfg)
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print('text_ref vs transformers %s, fp64: max-rel %.2e' % (tr.__version__, rel))
    assert got.dtype == torch.float64 and rel <= 1e-10, rel


# ---------------------------------------------------------------------------------------------------------------- 2. the tokenizer
def test_tokenizer_hand_derived_ids(vocab_file):
    """512 't h', 513 'th e</w>', 514 'c a', 515 'ca t</w>'; 519 / 520 the markers"""
    t = Tokenizer(vocab_file, VOCAB)
    assert (t.sot, t.eot) == (519, 520)
    assert t.tokenize('the cat')[0, :5].tolist() == [519, 513, 515, 520, 0]
    assert t.tokenize('')[0, :3].tolist() == [519, 520, 0]
    sym = list(byte_symbols().values())
    assert len(set(sym)) == 256 and sym[0] == '!' and t.encode('!') == [256] and t.encode('a!') == [256 + sym.index('a'), 256]          # two pieces, each its own last symbol: 'a</w>', '!</w>'


def test_tokenizer_vs_transformers(vocab_file, tmp_path):
    tr = pytest.importorskip('transformers')
    sym = list(byte_symbols().values())
    vocab = sym + [s + '</w>' for s in sym] + [m.replace(' ', '') for m in MERGES] + ['<|startoftext|>', '<|endoftext|>']
    (tmp_path / 'vocab.json').write_text(json.dumps({s: i for i, s in enumerate(vocab)}), encoding='utf-8')
    (tmp_path / 'merges.txt').write_text('#version: 0.2\n' + '\n'.join(MERGES) + '\n', encoding='utf-8')
    hf = tr.CLIPTokenizer(str(tmp_path / 'vocab.json'), str(tmp_path / 'merges.txt'))
    ours = Tokenizer(vocab_file, VOCAB)
    for s in STRINGS:
        assert [ours.sot] + ours.encode(s) + [ours.eot] == hf(s)['input_ids'], s
    assert len(ours.encode(STRINGS[-1])) + 2 == 92


def test_tokenizer_padding_overflow_eot(vocab_file):
    t = Tokenizer(vocab_file, VOCAB)
    rows = t.tokenize(STRINGS[:3])
    assert rows.dtype == torch.int32 and rows.shape == (3, 77)
    for r, s in zip(rows, STRINGS[:3]):
        n = len(t.encode(s)) + 2
        assert r[0] == 519 and r[n - 1] == 520 and not r[n:].any() and int(r.argmax()) == n - 1
    long = STRINGS[-1]
    with pytest.raises(RuntimeError, match='the the the .* is too long for context length 77'):
        t.tokenize([long])
    cut = t.tokenize([long], truncate=True)[0]
    assert cut[76] == 520 and int(cut.argmax()) == 76 and cut[:76].tolist() == ([519] + t.encode(long))[:76]
    assert t.tokenize('the', context_length=9).shape == (1, 9)


def test_tokenizer_file_formats(vocab_file, tmp_path):
    """.gz and plain text read alike; the merge count follows vocab_size: a longer file is cut, a shorter one refused"""
    plain = tmp_path / 'merges.txt'
    plain.write_text('#version: 0.2\n' + '\n'.join(MERGES) + '\n', encoding='utf-8')
    a, b = Tokenizer(vocab_file, VOCAB), Tokenizer(str(plain), VOCAB)
    assert a.encoder == b.encoder and a.rank == b.rank
    short = Tokenizer(str(plain), 512 + 4 + 2)          # the first four merges only: 'an', 'in', 'ing</w>' are gone
    assert len(short.rank) == 4 and (short.sot, short.eot) == (516, 517)
    assert short.encode('the cat') == a.encode('the cat') and len(short.encode('ring')) == 4 and len(a.encode('ring')) == 2
    with pytest.raises(ValueError, match='merges'):
        Tokenizer(str(plain), 49408)


# -------------------------------------------------------------------------------------------------- 3. the causal attention alone
def _show(tag, ratios):
    print('%s: worst err / bound  %s' % (tag, '  '.join('%s %.3f' % kv for kv in ratios.items())))


@pytest.mark.parametrize('T', [1, 31, 32, 33, 64, 65, 77, 256])
def test_attention_causal_vs_fp64(emu, T):
    _show('causal fp32 T=%d normal' % T, C.check_attention_causal(emu, 'cpu', S=2 if T <= 65 else 1, T=T, heads=2, seed=T))


@pytest.mark.parametrize('kind', [k for k in C.V.ATTN_KINDS if k != 'normal'])
def test_attention_causal_families_vs_fp64(emu, kind):
    _show('causal fp32 T=77 %s' % kind, C.check_attention_causal(emu, 'cpu', S=1, T=77, heads=2, kind=kind, seed=3))


# ------------------------------------------------------------------------------------------------------------- 4. the whole tower
@pytest.mark.parametrize('ctx', [77, 9])
def test_text_tower_vs_fp64(emu, ctx):
    # (the interpreter runs a ctx = 77 forward in seconds: there one prompt is tried alone, the mid-sequence one; at ctx = 9 all four)
    C.check_tower(emu, 'cpu', dict(C.TINY, context_length=ctx), tag='interpreter tiny', alone=[3] if ctx == 77 else None)


# ------------------------------------------------------------------------------------------------------------------- 5. refusals
def test_text_refusals(emu):
    C.check_refusals(emu, 'cpu')


# ---------------------------------------------------------------------------------------------------------- 6. the public surface
TINY_VIS = dict(input_resolution=32, patch_size=16, width=256, layers=1, heads=4, output_dim=128)


def _full_state(text_cfg, seed=4):
    from aphantasia_amd.weights import synthetic_text_weights, synthetic_visual_weights
    vis = synthetic_visual_weights(TINY_VIS, 3)
    full = {'visual.' + k: v for k, v in vis.items()}
    full.update(synthetic_text_weights(text_cfg, seed))
    return vis, full


def test_public_surface(emu, vocab_file, tmp_path):
    from aphantasia_amd import clip as aclip
    from aphantasia_amd.weights import text_config, text_weights
    cfg = dict(C.TINY, context_length=9, vocab_size=VOCAB, layers=1)
    vis, full = _full_state(cfg)
    assert text_config(full) == cfg and set(text_weights(full)) == {k for k in full if not k.startswith('visual.')}
    model = aclip.CLIPModel('tiny', TINY_VIS, vis, full, max_batch=1, lib=emu)
    w = text_weights(full)

    def gate(enc, tokens):
        want = text_ref.encode_text({k: v.double() for k, v in w.items()}, tokens, cfg)
        e32 = (text_ref.encode_text(w, tokens, cfg).double() - want).abs().max().item()
        err = (enc.double() - want).abs().max().item()
        assert enc.dtype == torch.float32 and err <= C.GATE * e32, (err, e32)
    tokens = aclip.tokenize('the cat in the can', 9, bpe_vocab=vocab_file, vocab_size=VOCAB)
    assert tokens.dtype == torch.int32 and tokens.shape == (1, 9) and tokens[0, 0] == 519
    emb = aclip.text_embedding(model, 'the cat in the can', device='cpu', bpe_vocab=vocab_file)
    assert emb.shape == (1, 128)
    gate(emb, tokens)
    batch = aclip.tokenize(['the cat in the can', 'thing', '', 'a can'], 9, bpe_vocab=vocab_file, vocab_size=VOCAB)
    enc = model.encode_text(batch)
    gate(enc, batch)
    assert torch.equal(enc[0], emb[0])
    for i in (1, 2):
        assert torch.equal(model.encode_text(batch[i:i + 1].long())[0], enc[i])          # row by row; int64 tokens are taken too
    for bad in (batch.clone().fill_(VOCAB), -batch - 1, batch[:, :8], batch.float()):
        with pytest.raises(ValueError):
            model.encode_text(bad)
    assert model._text is not None and model._text.workspace_bytes() > 0
    model.release_text()
    assert model._text is None
    assert torch.equal(model.encode_text(batch[:1]), enc[:1])                              # rebuilt on demand
    # the vocabulary beside the checkpoint is found without the argument
    model.weights_path = os.path.join(os.path.dirname(vocab_file), 'ViT-tiny.pt')
    assert torch.equal(aclip.text_embedding(model, 'the cat in the can', device='cpu'), emb)


def test_cli_bpe_vocab_argument():
    import clip_fft
    import cppn
    import illustrip
    for mod in (clip_fft, illustrip, cppn):
        assert mod.get_args(['-t', 'x', '--bpe-vocab', '/some/vocab.gz']).bpe_vocab == '/some/vocab.gz'
        assert mod.get_args(['-t', 'x']).bpe_vocab is None


def test_checkpoint_model_without_vocabulary(emu, tmp_path):
    """no vocabulary reachable: the error names the file and where to pass it; the `clip` package is not imported on the way"""
    from aphantasia_amd import clip as aclip
    vis, full = _full_state(dict(C.TINY, context_length=9, vocab_size=VOCAB))
    model = aclip.CLIPModel('tiny', TINY_VIS, vis, full, max_batch=1, lib=emu, weights_path=str(tmp_path / 'ViT-tiny.pt'))
    with pytest.raises(RuntimeError, match=r'bpe_simple_vocab_16e6\.txt\.gz.*--bpe-vocab'):
        aclip.text_embedding(model, 'the cat', device='cpu')
    model.weights_path = None
    with pytest.raises(RuntimeError, match=r'bpe_simple_vocab_16e6\.txt\.gz'):
        aclip.text_embedding(model, 'the cat', device='cpu')
    with pytest.raises(RuntimeError, match='not found'):
        aclip.text_embedding(model, 'the cat', device='cpu', bpe_vocab=str(tmp_path / 'nothing.gz'))
    assert 'clip' not in sys.modules


def test_synthetic_model_keeps_its_hashed_target(emu):
    """a model without a checkpoint: the prompt's sha256 seeds a randn, exactly as before the text tower existed"""
    from aphantasia_amd import clip as aclip
    from aphantasia_amd.weights import synthetic_visual_weights
    model = aclip.CLIPModel('tiny', TINY_VIS, synthetic_visual_weights(TINY_VIS, 3), None, max_batch=1, lib=emu)
    emb = aclip.text_embedding(model, 'a red square', device='cpu')
    seed = int.from_bytes(__import__('hashlib').sha256(b'a red square').digest()[:4], 'little')
    assert seed == 2991955045
    assert torch.equal(emb, torch.randn(1, 128, generator=torch.Generator().manual_seed(seed)))
    assert emb[0, :3].tolist() == [-0.5782790780067444, -1.5133460760116577, -0.7347866892814636]          # as on the parent commit
    with pytest.raises(RuntimeError, match='checkpoint'):
        model.encode_text(torch.zeros(1, 77, dtype=torch.int32))
    model.release_text()

