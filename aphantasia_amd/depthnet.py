"""The Depth-Anything-V2 relative-depth estimator of `illustrip.py -d` on the HIP kernels of csrc/depth.hip (C ABI: aph_depth_*).

    net = DepthAnythingHIP.from_pretrained_dir(path)           # a local Hugging Face checkpoint directory, read on the CPU
    net = DepthAnythingHIP.from_state_dict(config, state_dict) # the same from a config dict and a state dict: no `transformers` needed
    depth = net(image)                                         # [B,3,h,w] in (0,1), h and w multiples of 14 -> [B,1,h,w], min-max normalised

`config` is what DepthAnythingConfig.to_dict() gives (backbone_config: hidden_size, num_hidden_layers, num_attention_heads, out_indices,
use_swiglu_ffn; neck_hidden_sizes, fusion_hidden_size, head_hidden_size); the state dict carries transformers' parameter names.  The position
embedding is interpolated from the checkpoint's grid to the image's here, once per size, exactly as transformers does (bicubic,
align_corners=False, in fp32): set-up, not hot path.  The device arena is sized for the largest image and batch seen so far and made again
when a larger one arrives; a frame loop of one size allocates once.  There is no torch fallback."""
from ctypes import c_int, c_void_p, byref

import torch
import torch.nn.functional as F

from . import _ffi
from .ops import _stream, ptr

PATCH = 14
SMALL = dict(backbone_config=dict(hidden_size=384, num_hidden_layers=12, num_attention_heads=6, out_indices=[3, 6, 9, 12]),
             neck_hidden_sizes=[48, 96, 192, 384], fusion_hidden_size=64, head_hidden_size=32)
BASE = dict(backbone_config=dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, out_indices=[3, 6, 9, 12]),
            neck_hidden_sizes=[96, 192, 384, 768], fusion_hidden_size=128, head_hidden_size=32)
LARGE = dict(backbone_config=dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, out_indices=[5, 12, 18, 24]),
             neck_hidden_sizes=[256, 512, 1024, 1024], fusion_hidden_size=256, head_hidden_size=32)


def parse_config(config):
    """-> dict(hidden, layers, heads, swiglu, out_indices, neck, fusion, head, grid) after refusing what the kernels do not implement"""
    bc = config['backbone_config']
    if hasattr(bc, 'to_dict'):
        bc = bc.to_dict()
    out_indices = bc.get('out_indices')
    if out_indices is None and bc.get('out_features'):
        out_indices = [int(s.replace('stage', '')) for s in bc['out_features']]
    c = dict(hidden=int(bc['hidden_size']), layers=int(bc['num_hidden_layers']), heads=int(bc['num_attention_heads']),
             swiglu=int(bool(bc.get('use_swiglu_ffn', False))), out_indices=[int(i) for i in (out_indices or [])],
             neck=[int(n) for n in config['neck_hidden_sizes']], fusion=int(config['fusion_hidden_size']), head=int(config['head_hidden_size']),
             grid=int(bc.get('image_size', 518)) // PATCH)
    if len(c['out_indices']) != 4 or len(c['neck']) != 4:
        raise ValueError('DepthAnythingHIP: four tapped layers and four neck widths expected, got %s / %s' % (c['out_indices'], c['neck']))
    checks = (('patch_size', bc.get('patch_size', PATCH), PATCH), ('mlp_ratio', bc.get('mlp_ratio', 4), 4),
              ('reassemble_factors', [float(f) for f in config.get('reassemble_factors', [4, 2, 1, 0.5])], [4.0, 2.0, 1.0, 0.5]),
              ('depth_estimation_type', config.get('depth_estimation_type', 'relative'), 'relative'),
              ('hidden_act', bc.get('hidden_act', 'gelu'), 'gelu'), ('layer_norm_eps', float(bc.get('layer_norm_eps', 1e-6)), 1e-6),
              ('apply_layernorm', bool(bc.get('apply_layernorm', True)), True), ('reshape_hidden_states', bool(bc.get('reshape_hidden_states', False)), False),
              ('num_register_tokens', int(bc.get('num_register_tokens', 0)), 0), ('head_in_index', int(config.get('head_in_index', -1)), -1))
    for name, got, want in checks:
        if got != want:
            raise ValueError('DepthAnythingHIP: %s = %r is not supported (the kernels implement %r)' % (name, got, want))
    return c


def weight_shapes(config):
    """-> {name: shape} of the state dict of this configuration (position_embeddings included, mask_token not)"""
    c = parse_config(config)
    D, Fh, Hh = c['hidden'], c['fusion'], c['head']
    s = {'backbone.embeddings.cls_token': (1, 1, D), 'backbone.embeddings.position_embeddings': (1, 1 + c['grid'] ** 2, D),
         'backbone.embeddings.patch_embeddings.projection.weight': (D, 3, PATCH, PATCH), 'backbone.embeddings.patch_embeddings.projection.bias': (D,)}
    for i in range(c['layers']):
        p = 'backbone.encoder.layer.%d.' % i
        for n in ('norm1', 'norm2'):
            s[p + n + '.weight'] = (D,)
            s[p + n + '.bias'] = (D,)
        for n in ('attention.attention.query', 'attention.attention.key', 'attention.attention.value', 'attention.output.dense'):
            s[p + n + '.weight'] = (D, D)
            s[p + n + '.bias'] = (D,)
        s[p + 'layer_scale1.lambda1'] = (D,)
        s[p + 'layer_scale2.lambda1'] = (D,)
        s[p + 'mlp.fc1.weight'] = (4 * D, D)
        s[p + 'mlp.fc1.bias'] = (4 * D,)
        s[p + 'mlp.fc2.weight'] = (D, 4 * D)
        s[p + 'mlp.fc2.bias'] = (D,)
    s['backbone.layernorm.weight'] = (D,)
    s['backbone.layernorm.bias'] = (D,)
    for i, C in enumerate(c['neck']):
        p = 'neck.reassemble_stage.layers.%d.' % i
        s[p + 'projection.weight'] = (C, D, 1, 1)
        s[p + 'projection.bias'] = (C,)
        if i != 2:
            k = (4, 2, 0, 3)[i]
            s[p + 'resize.weight'] = (C, C, k, k)
            s[p + 'resize.bias'] = (C,)
        s['neck.convs.%d.weight' % i] = (Fh, C, 3, 3)
        q = 'neck.fusion_stage.layers.%d.' % i
        s[q + 'projection.weight'] = (Fh, Fh, 1, 1)
        s[q + 'projection.bias'] = (Fh,)
        for u in (1, 2):
            for k in (1, 2):
                s[q + 'residual_layer%d.convolution%d.weight' % (u, k)] = (Fh, Fh, 3, 3)
                s[q + 'residual_layer%d.convolution%d.bias' % (u, k)] = (Fh,)
    s['head.conv1.weight'] = (Fh // 2, Fh, 3, 3)
    s['head.conv1.bias'] = (Fh // 2,)
    s['head.conv2.weight'] = (Hh, Fh // 2, 3, 3)
    s['head.conv2.bias'] = (Hh,)
    s['head.conv3.weight'] = (1, Hh, 1, 1)
    s['head.conv3.bias'] = (1,)
    return s


def synthetic_weights(config, seed=0, last_bias=0.0):
    """seeded weights with activations of order one at every layer: matrices and convolutions normal with variance 1 / fan-in (2 / fan-in in
    front of a ReLU), small biases, LayerNorm gains near 1, LayerScale near 0.5, position rows of order 0.1.  `last_bias`: the bias of the last
    1 x 1 convolution -- tests set it to 3 std - mean of the pre-activation on their input, so that the final ReLU cuts (almost) nothing and
    cannot hide an error."""
    g = torch.Generator().manual_seed(seed)
    w = {}
    for name, shape in weight_shapes(config).items():
        n = 1
        for d in shape:
            n *= d
        if name.endswith('lambda1'):
            t = 0.4 + 0.2 * torch.rand(shape, generator=g)
        elif 'norm' in name and name.endswith('weight'):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith('bias'):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith('cls_token'):
            t = torch.randn(shape, generator=g)
        elif name.endswith('position_embeddings'):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith('resize.weight') and shape[2] in (2, 4):      # transpose convolution: every output pixel sums over cin alone
            t = torch.randn(shape, generator=g) / shape[0] ** 0.5
        else:
            fan_in = n // shape[0]
            relu_in = name.startswith('neck.fusion') and 'convolution' in name or name == 'head.conv3.weight'
            t = torch.randn(shape, generator=g) * ((2.0 if relu_in else 1.0) / fan_in) ** 0.5
        w[name] = t.float()
    w['head.conv3.bias'] = torch.full((1,), float(last_bias))
    return w


def position_rows(pos_embed, gh, gw):
    """transformers' Dinov2Embeddings.interpolate_pos_encoding: [1, 1 + G G, D] -> [1 + gh gw, D] (the class row, then the G x G grid resized
    with bicubic, align_corners=False, in fp32; untouched when the grid already is gh x gw = G x G)"""
    pos = pos_embed.detach().cpu().reshape(-1, pos_embed.shape[-1])
    n = pos.shape[0] - 1
    G = int(round(n ** 0.5))
    if G * G != n:
        raise ValueError('position_embeddings: %d patch rows are not a square grid' % n)
    if gh == G and gw == G:
        return pos.clone()
    grid = pos[1:].reshape(1, G, G, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid.to(torch.float32), size=(gh, gw), mode='bicubic', align_corners=False).to(pos.dtype)
    return torch.cat([pos[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, -1)], 0)


class DepthAnythingHIP:
    """One estimator: the host copy of the weights and a device handle (aph_depth) for the largest (h, w, batch) seen so far."""

    def __init__(self, config, state_dict, max_hw=None, max_batch=2, lib=None):
        self.cfg = parse_config(config)
        if self.cfg['swiglu']:
            raise ValueError('DepthAnythingHIP: the SwiGLU feed-forward (the giant encoder) is not supported')
        shapes = weight_shapes(config)
        self.weights = {}
        for name, shape in shapes.items():
            if name not in state_dict:
                raise KeyError('DepthAnythingHIP: weight %s is missing from the state dict' % name)
            t = state_dict[name].detach().float().cpu().contiguous()
            if tuple(t.shape) != tuple(shape):
                raise ValueError('DepthAnythingHIP: %s has shape %s, expected %s' % (name, tuple(t.shape), tuple(shape)))
            self.weights[name] = t
        self.lib = lib if lib is not None else _ffi.lib()
        self.handle = None
        self.max_h = self.max_w = 0
        self.max_batch = int(max_batch)
        self.grid = None
        if max_hw is not None:
            self._create(int(max_hw[0]), int(max_hw[1]), self.max_batch)

    @classmethod
    def from_state_dict(cls, config, state_dict, **kw):
        return cls(config, state_dict, **kw)

    @classmethod
    def from_pretrained_dir(cls, path, **kw):
        """a local Hugging Face checkpoint directory (config.json + model.safetensors / pytorch_model.bin), read on the CPU"""
        import json
        import os
        with open(os.path.join(path, 'config.json')) as f:
            config = json.load(f)
        st = os.path.join(path, 'model.safetensors')
        if os.path.isfile(st):
            from safetensors.torch import load_file
            sd = load_file(st, device='cpu')
        elif os.path.isfile(os.path.join(path, 'pytorch_model.bin')):
            sd = torch.load(os.path.join(path, 'pytorch_model.bin'), map_location='cpu', weights_only=True)
        else:
            from transformers import AutoModelForDepthEstimation
            model = AutoModelForDepthEstimation.from_pretrained(path)
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            del model
        return cls(config, sd, **kw)

    def _create(self, h, w, batch):
        self.close()
        c = self.cfg
        out = c_void_p()
        self.lib.call('aph_depth_create', c['hidden'], c['layers'], c['heads'], c['swiglu'], (c_int * 4)(*c['out_indices']), (c_int * 4)(*c['neck']),
                      c['fusion'], c['head'], h, w, batch, byref(out))
        self.handle = out
        self.max_h, self.max_w, self.max_batch, self.grid = h, w, batch, None
        for name, t in self.weights.items():
            if name.endswith('position_embeddings'):
                continue
            self.lib.call('aph_depth_set_weight', self.handle, name.encode(), c_void_p(t.data_ptr()), t.numel())

    def workspace_bytes(self):
        return int(self.lib.cdll.aph_depth_workspace_bytes(self.handle)) if self.handle else 0

    def forward(self, image, normalise=True):
        """image [B,3,h,w] fp32 in (0,1) -> depth [B,1,h,w] fp32 on the same device"""
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError('DepthAnythingHIP: image must be [B,3,h,w], got %s' % (tuple(image.shape),))
        x = image.detach().float().contiguous()
        B, _, h, w = x.shape
        if h < PATCH or w < PATCH or h % PATCH or w % PATCH:
            raise ValueError('DepthAnythingHIP: image %d x %d: both sides must be multiples of %d' % (h, w, PATCH))
        if self.handle is None or h > self.max_h or w > self.max_w or B > self.max_batch:
            self._create(max(h, self.max_h), max(w, self.max_w), max(B, self.max_batch))
        if (h // PATCH, w // PATCH) != self.grid:
            rows = position_rows(self.weights['backbone.embeddings.position_embeddings'], h // PATCH, w // PATCH).float().contiguous()
            self.lib.call('aph_depth_set_pos_embed', self.handle, h // PATCH, w // PATCH, c_void_p(rows.data_ptr()), rows.numel())
            self.grid = (h // PATCH, w // PATCH)
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=x.device)
        self.lib.call('aph_depth_forward', self.handle, ptr(x), B, h, w, int(bool(normalise)), ptr(out), _stream(x))
        return out

    __call__ = forward

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.call('aph_depth_destroy', self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
