"""CLIP for the optimisation loop: the pieces of `clip.load(...)`, `model.encode_image`, `model.encode_text` and `clip.tokenize`
that clip_fft.py:119,254 uses, running on the HIP ViT (csrc/vit.hip) and the HIP text tower (csrc/text.hip).

    model, _ = load('ViT-B/32', weights='/path/ViT-B-32.pt')     # OpenAI checkpoint if you have one
    model, _ = load('ViT-B/32')                                  # seeded synthetic weights (benchmarks/tests)
    enc = model.encode_image(cuts)                               # [S,3,224,224] normalised -> [S,512], autograd-aware
    txt = model.encode_text(tokenize(['a cat'], bpe_vocab='/path/bpe_simple_vocab_16e6.txt.gz'))      # int [n,77] -> f32 [n,512]
    txt = text_embedding(model, 'a cat', bpe_vocab=...)          # what the CLIs call: one prompt -> [1,512]

The text tower runs once per prompt, off the hot path, in fp32 (the kernels of the exact ViT path with a causal attention): no f16 mode.
It and the tokenizer (tokenizer.py) are this project's own; the `clip` package is never imported.  The BPE vocabulary is the user's file,
like the checkpoint.  A model without a checkpoint (synthetic weights) has no text tower: its prompts are mapped to seeded synthetic
target embeddings.
"""
import hashlib
import os
import warnings

import torch

from . import ops
from .tokenizer import Tokenizer
from .weights import load_openai_checkpoint, synthetic_visual_weights, text_config, text_weights, visual_config

BPE_VOCAB_NAME = 'bpe_simple_vocab_16e6.txt.gz'
TEXT_MAX_BATCH = 16       # prompts per aph_text_forward launch (encode_text walks a longer list in chunks of it)

LOSS_SCALE = 4096.0     # static scale of the fp16 backward chain (precision table)


class _Encode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, visual):
        S = x.shape[0]
        patches = ops.patchify(x.contiguous().float(), visual.patch_size, lib=visual.lib, f32=visual.exact)
        enc = visual._forward_patches(patches, S)
        ctx.visual, ctx.S = visual, S
        ctx.gen = visual._generation
        ctx.save_for_backward(patches)
        ctx.shape = x.shape
        return enc

    @staticmethod
    def backward(ctx, g):
        patches, = ctx.saved_tensors
        v = ctx.visual
        if v._generation != ctx.gen:          # another forward ran since: rebuild this node's activations
            v._forward_patches(patches, ctx.S)
            ctx.gen = v._generation
        # (exact mode keeps the power-of-two loss scale: multiplying by it and by its inverse is exact in fp32)
        gp = v.handle.backward((g.float() * LOSS_SCALE).contiguous(), ctx.S, out_scale=1.0 / LOSS_SCALE, f32=v.exact)
        return ops.unpatchify(gp, ctx.S, ctx.shape[2], v.patch_size, lib=v.lib), None


class VisualTransformer:
    """Stands in for clip.model.VisionTransformer: `.input_resolution`, `.patch_size`, callable."""

    def __init__(self, cfg, weights, max_batch=256, lib=None, exact=False):
        """exact: every forward / backward on the fp32 path (aph_vit_forward_f32 / aph_vit_backward_f32)"""
        self.lib = lib
        self.exact = bool(exact)
        self.cfg = dict(cfg)
        self.input_resolution = cfg['input_resolution']
        self.patch_size = cfg['patch_size']
        self.output_dim = cfg['output_dim']
        self.weights = weights
        self.handle = ops.VitHandle(cfg, weights, max_batch, lib=lib)
        if self.exact:
            self.handle.enable_f32()
        self._generation = 0

    def ensure_batch(self, S):
        if S > self.handle.max_batch:
            self.handle = ops.VitHandle(self.cfg, self.weights, S, lib=self.lib)
            if self.exact:
                self.handle.enable_f32()

    def _forward_patches(self, patches, S, out=None, hilo=False, f32=None):
        self.ensure_batch(S)
        self._generation += 1
        f32 = self.exact if f32 is None else f32
        if f32:
            self.handle.enable_f32()          # (a no-op once enabled: an Engine(exact=True) enables it before any capture)
        return self.handle.forward(patches, S, out, hilo=hilo, f32=f32)

    def __call__(self, x):
        R, p = self.input_resolution, self.patch_size
        if x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == x.shape[3] == R + 8 and (R + 8 - p) // p + 1 == R // p:
            # the padded canvas of transforms_custom / transforms_elastic (transforms.py:147-163): upstream's conv1, stride = kernel = patch,
            # makes R / p patches a side of it and never reads its last 8 rows and columns -- take the window it reads
            x = x[:, :, :R, :R]
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != R or x.shape[3] != R:
            raise ValueError('encode_image expects [S,3,%d,%d], got %s' % (R, R, tuple(x.shape)))
        return _Encode.apply(x, self)


class CLIPModel:
    def __init__(self, name, cfg, weights, full_state=None, max_batch=256, lib=None, exact=False, weights_path=None):
        self.name = name
        self.lib = lib
        self.visual = VisualTransformer(cfg, weights, max_batch, lib=lib, exact=exact)
        self._full_state = full_state
        self.synthetic = full_state is None
        self.weights_path = weights_path
        self._text = None              # ops.TextHandle, built from _full_state on the first encode_text
        self.text_cfg = None

    def encode_image(self, image):
        return self.visual(image)

    def _text_handle(self):
        if self._text is None:
            if self._full_state is None:
                raise RuntimeError('encode_text needs a checkpoint with a text tower (load(name, weights=...)); this model has synthetic '
                                   'visual weights only -- text_embedding(model, prompt) gives it a seeded synthetic target')
            self.text_cfg = text_config(self._full_state)
            self._text = ops.TextHandle(self.text_cfg, text_weights(self._full_state), TEXT_MAX_BATCH, lib=self.lib)
        return self._text

    def encode_text(self, tokens):
        """int tokens [n, context_length] (tokenize's rows) -> f32 [n, output_dim] on the visual tower's device; no gradient"""
        handle = self._text_handle()
        cfg = self.text_cfg
        tokens = torch.as_tensor(tokens)
        if tokens.dim() != 2 or tokens.shape[1] != cfg['context_length'] or tokens.dtype.is_floating_point or tokens.dtype == torch.bool:
            raise ValueError('encode_text expects integer tokens [n, %d], got %s %s' % (cfg['context_length'], tokens.dtype, tuple(tokens.shape)))
        host = tokens.detach().cpu().to(torch.int64)
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= cfg['vocab_size']):
            raise ValueError('encode_text: token ids must lie in [0, %d); got %d .. %d' % (cfg['vocab_size'], int(host.min()), int(host.max())))
        dev = 'cpu' if self.lib is not None else 'cuda'          # (lib: the host interpreter build of the tests)
        ids = host.to(torch.int32).contiguous().to(dev)
        out = torch.empty(ids.shape[0], cfg['output_dim'], dtype=torch.float32, device=dev)
        for s in range(0, ids.shape[0], TEXT_MAX_BATCH):
            handle.forward(ids[s:s + TEXT_MAX_BATCH], out=out[s:s + TEXT_MAX_BATCH])
        return out

    def release_text(self):
        """frees the text tower's device arena (about 0.25 GB for the ViT-B models, 0.5 GB for ViT-L/14); a later encode_text rebuilds it"""
        if self._text is not None:
            self._text.close()
            self._text = None

    def float(self):
        return self

    def eval(self):
        return self

    def cuda(self):
        return self


DEFAULT_MAX_BATCH = {'ViT-L/14': 32}     # cuts the activation arena is first sized for (others: 256); ensure_batch grows it


def _report_arena(model):
    """ViT-L/14 keeps 0.152 GB of activations per cut (profiles/vitl14.txt): say once what the handle reserved"""
    if model.name in DEFAULT_MAX_BATCH:
        h = model.visual.handle
        print(' %s: %.2f GB of device memory for weights and the activations of %d cuts' % (model.name, h.workspace_bytes() / 2 ** 30, h.max_batch),
              flush=True)
    return model


def load(name='ViT-B/32', device='cuda', jit=False, weights=None, seed=1, max_batch=None, exact=False):
    """-> (model, None).  weights: path to an OpenAI CLIP checkpoint; None = seeded synthetic weights.
    exact: the fp32 ViT path (f32-input MFMA GEMMs, fp32 attention and activations) -- what the reference computes on the CPU.
    max_batch: None = 256 cuts, 32 for ViT-L/14 (0.152 GB of activations per cut; Engine / encode_image grow the arena on demand)."""
    if max_batch is None:
        max_batch = DEFAULT_MAX_BATCH.get(name, 256)
    if weights is not None:
        vis, cfg, full = load_openai_checkpoint(weights)
        want = visual_config(name)
        if (cfg['patch_size'], cfg['width'], cfg['layers']) != (want['patch_size'], want['width'], want['layers']):
            raise ValueError('%s does not hold a %s visual tower' % (weights, name))
        return _report_arena(CLIPModel(name, cfg, vis, full, max_batch, exact=exact, weights_path=weights)), None
    cfg = visual_config(name)
    warnings.warn('aphantasia_amd.clip.load(%r): no checkpoint given -> seeded SYNTHETIC weights (seed %d); '
                  'images will not be meaningful, use --clip-weights for real runs' % (name, seed))
    return _report_arena(CLIPModel(name, cfg, synthetic_visual_weights(cfg, seed), None, max_batch, exact=exact)), None


_tokenizers = {}


def _tokenizer(bpe_vocab, vocab_size):
    key = (os.path.abspath(bpe_vocab), int(vocab_size))
    if key not in _tokenizers:
        _tokenizers[key] = Tokenizer(bpe_vocab, vocab_size)
    return _tokenizers[key]


def tokenize(texts, context_length=77, truncate=False, bpe_vocab=None, vocab_size=49408):
    """clip.tokenize: str or list of str -> int32 [n, context_length] (SOT, ids, EOT, zero padding).  bpe_vocab: the vocabulary file
    (upstream's bpe_simple_vocab_16e6.txt.gz, its text, or a HuggingFace merges.txt); vocab_size: rows of the checkpoint's token embedding."""
    if bpe_vocab is None:
        raise RuntimeError('tokenize needs the BPE vocabulary: pass bpe_vocab=/path/%s (the CLIs: --bpe-vocab)' % BPE_VOCAB_NAME)
    return _tokenizer(bpe_vocab, vocab_size).tokenize(texts, context_length, truncate)


def _find_vocab(model, bpe_vocab):
    if bpe_vocab is not None:
        if not os.path.isfile(bpe_vocab):
            raise RuntimeError('BPE vocabulary %s not found (%s of openai/CLIP, or a merges.txt)' % (bpe_vocab, BPE_VOCAB_NAME))
        return bpe_vocab
    beside = os.path.join(os.path.dirname(os.path.abspath(model.weights_path)), BPE_VOCAB_NAME) if model.weights_path else None
    if beside is not None and os.path.isfile(beside):
        return beside
    raise RuntimeError('text prompts need the BPE vocabulary %s of openai/CLIP (clip/%s in its repository): put it beside the checkpoint%s '
                       'or pass its path with --bpe-vocab (text_embedding(..., bpe_vocab=PATH))'
                       % (BPE_VOCAB_NAME, BPE_VOCAB_NAME, ' (%s)' % os.path.dirname(os.path.abspath(model.weights_path)) if model.weights_path else ''))


def text_embedding(model, text, device='cuda', bpe_vocab=None):
    """Target embedding for a prompt ([1, output_dim], detached).  A model with a checkpoint: this project's tokenizer and text tower
    (bpe_vocab, else bpe_simple_vocab_16e6.txt.gz beside the checkpoint).  A synthetic model: a deterministic vector derived from the
    prompt (so runs are reproducible)."""
    if not model.synthetic:
        # a real checkpoint: the target must come from its text tower -- a random stand-in would silently optimise towards
        # nothing while the output still looks like a valid run
        path = _find_vocab(model, bpe_vocab)
        cfg = text_config(model._full_state)
        tokens = tokenize(text, cfg['context_length'], bpe_vocab=path, vocab_size=cfg['vocab_size'])
        return model.encode_text(tokens).detach().clone().float()
    h = int.from_bytes(hashlib.sha256(text.encode()).digest()[:4], 'little')
    g = torch.Generator().manual_seed(h)
    return torch.randn(1, model.visual.output_dim, generator=g).to(device)


def release_text(*models):
    """the CLIs call this once their targets are built: frees every model's text arena"""
    for m in models:
        if m is not None:
            m.release_text()
