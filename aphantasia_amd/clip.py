"""CLIP image tower for the optimisation loop: the piece of `clip.load(...)` / `model.encode_image`
that clip_fft.py:119,254 uses, running on the HIP ViT (csrc/vit.hip).

    model, _ = load('ViT-B/32', weights='/path/ViT-B-32.pt')     # OpenAI checkpoint if you have one
    model, _ = load('ViT-B/32')                                  # seeded synthetic weights (benchmarks/tests)
    enc = model.encode_image(cuts)                               # [S,3,224,224] normalised -> [S,512], autograd-aware

The text tower / tokenizer (encode_text, clip.tokenize) run once per prompt, off the hot path; they
are taken from the `clip` package when it is importable together with a real checkpoint, otherwise
text prompts are mapped to seeded synthetic target embeddings (loud warning).
"""
import hashlib
import warnings

import torch

from . import ops
from .weights import load_openai_checkpoint, synthetic_visual_weights, visual_config

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
    def __init__(self, name, cfg, weights, full_state=None, max_batch=256, lib=None, exact=False):
        self.name = name
        self.visual = VisualTransformer(cfg, weights, max_batch, lib=lib, exact=exact)
        self._full_state = full_state
        self.synthetic = full_state is None

    def encode_image(self, image):
        return self.visual(image)

    def encode_text(self, text):
        raise NotImplementedError(
            'encode_text needs the OpenAI text tower + BPE vocabulary (the `clip` package and a real checkpoint); '
            'use aphantasia_amd.clip.text_embedding(model, prompt), which falls back to a seeded synthetic embedding')

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
        return _report_arena(CLIPModel(name, cfg, vis, full, max_batch, exact=exact)), None
    cfg = visual_config(name)
    warnings.warn('aphantasia_amd.clip.load(%r): no checkpoint given -> seeded SYNTHETIC weights (seed %d); '
                  'images will not be meaningful, use --clip-weights for real runs' % (name, seed))
    return _report_arena(CLIPModel(name, cfg, synthetic_visual_weights(cfg, seed), None, max_batch, exact=exact)), None


def text_embedding(model, text, device='cuda'):
    """Target embedding for a prompt ([1, output_dim], detached).  Real text tower when available,
    else a deterministic synthetic vector derived from the prompt (so runs are reproducible)."""
    if not model.synthetic:
        # a real checkpoint: the target must come from its text tower -- a random stand-in would silently optimise towards
        # nothing while the output still looks like a valid run
        try:
            import clip as openai_clip          # the reference's dependency (openai/CLIP); tokenizer + text tower
        except ImportError as e:
            raise RuntimeError('text prompts with a real CLIP checkpoint need the `clip` package (openai/CLIP: BPE vocabulary + text '
                               'tower); it is not importable here.  Pass image prompts (-i) or install it.') from e
        if getattr(model, '_text_model', None) is None:
            import copy
            model._text_model = openai_clip.model.build_model(copy.copy(model._full_state)).float().to(device).eval()
        with torch.no_grad():
            return model._text_model.encode_text(openai_clip.tokenize(text).to(device)).detach().clone().float()
    h = int.from_bytes(hashlib.sha256(text.encode()).digest()[:4], 'little')
    g = torch.Generator().manual_seed(h)
    return torch.randn(1, model.visual.output_dim, generator=g).to(device)
