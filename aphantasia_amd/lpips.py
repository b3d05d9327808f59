"""The LPIPS (VGG-16) image term of `clip_fft.py --sync` on the HIP kernels of csrc/lpips.hip.

    sim_loss = load(H, W, vgg_path, lpips_path)  # one handle per frame size
    loss += w * sim_loss(F.interpolate(img, [H // 2, W // 2], ...), img_in, normalize=True)     # the reference's line, unchanged

`sim_loss(img, img_in)` takes the two HALF-size images [1,3,H//2,W//2] in [0,1] like the reference's call (clip_fft.py:221-222,268-270) and
returns a scalar with an autograd edge to `img`: a torch.autograd.Function over aph_lpips_value_grad_half.  The fused engine is handed the
term with its target set (`Engine(sync=sim_loss.set_target(img_in))`) and runs value and gradient on the FULL frame inside the step
(aph_lpips_value_grad), resize included.

Weights: a torchvision vgg16 state dict (features.N.weight / .bias) and the lpips package's vgg.pth (linL.model.1.weight), both LOCAL
files; with neither, seeded synthetic weights and a loud warning, as aphantasia_amd.clip.load does.  There is no torch fallback."""
import warnings
from ctypes import c_int, c_void_p, byref

import torch

from . import _ffi
from .ops import _stream, ptr

WIDTHS = (64, 128, 256, 512, 512)
CONVS_OF_STAGE = (2, 2, 3, 3, 3)
FEATURE_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)          # torchvision vgg16.features numbering of the 13 convolutions


def layer_table(widths=WIDTHS):
    """-> [(features index, cin, cout, stage)] of the 13 convolutions"""
    out, k, cin = [], 0, 3
    for s, n in enumerate(CONVS_OF_STAGE):
        for _ in range(n):
            out.append((FEATURE_IDX[k], cin, widths[s], s))
            cin = widths[s]
            k += 1
    return out


def weight_shapes(widths=WIDTHS):
    """-> {name: shape} of every tensor aph_lpips_set_weight takes"""
    shapes = {}
    for idx, cin, cout, _ in layer_table(widths):
        shapes['features.%d.weight' % idx] = (cout, cin, 3, 3)
        shapes['features.%d.bias' % idx] = (cout,)
    for s in range(5):
        shapes['lin%d.weight' % s] = (widths[s],)
    return shapes


def synthetic_weights(widths=WIDTHS, seed=0):
    """He-normal convolutions, small biases, lin weights uniform in [0, 1 / sqrt(C)) (non-negative like the trained ones)"""
    g = torch.Generator().manual_seed(seed)
    w = {}
    for idx, cin, cout, _ in layer_table(widths):
        w['features.%d.weight' % idx] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        w['features.%d.bias' % idx] = (torch.rand(cout, generator=g) - 0.5) * 0.2
    for s in range(5):
        w['lin%d.weight' % s] = torch.rand(widths[s], generator=g) / widths[s] ** 0.5
    return w


def map_state_dicts(vgg_sd=None, lpips_sd=None, widths=WIDTHS):
    """torchvision vgg16 state dict + lpips vgg.pth state dict -> {name: fp32 tensor} in this module's names.  A missing key, an
    unexpected shape or a half-given pair is refused."""
    if vgg_sd is None or lpips_sd is None:
        raise ValueError('LPIPS weights need BOTH files: the torchvision vgg16 state dict (--vgg-weights) and the lpips vgg.pth (--lpips-weights)')
    shapes = weight_shapes(widths)
    out = {}
    for name, shape in shapes.items():
        if name.startswith('features.'):
            src, key = vgg_sd, name
        else:
            src, key = lpips_sd, '%s.model.1.weight' % name[:4]
            if key not in src and name in src:
                key = name
        if key not in src:
            raise KeyError('LPIPS weights: key %s not found' % key)
        t = src[key].detach().float().cpu()
        if not name.startswith('features.'):
            if t.numel() != shape[0] or tuple(t.shape) not in ((1, shape[0], 1, 1), shape):
                raise ValueError('LPIPS weights: %s has shape %s, expected (1, %d, 1, 1)' % (key, tuple(t.shape), shape[0]))
            t = t.reshape(-1)
        elif tuple(t.shape) != shape:
            raise ValueError('LPIPS weights: %s has shape %s, expected %s' % (key, tuple(t.shape), shape))
        out[name] = t.contiguous()
    return out


def load_weights(vgg_path=None, lpips_path=None, widths=WIDTHS, seed=0):
    """local files -> weights; nothing given -> seeded SYNTHETIC weights with a warning"""
    if vgg_path is None and lpips_path is None:
        warnings.warn('aphantasia_amd.lpips.load_weights: no weight files given -> seeded SYNTHETIC weights (seed %d); the --sync term will '
                      'not be a perceptual distance, use --vgg-weights and --lpips-weights for real runs' % seed)
        return synthetic_weights(widths, seed)
    if vgg_path is None or lpips_path is None:
        return map_state_dicts(None, None, widths)
    return map_state_dicts(torch.load(vgg_path, map_location='cpu', weights_only=True),
                           torch.load(lpips_path, map_location='cpu', weights_only=True), widths)


class _ValueGrad(torch.autograd.Function):
    """value of the half-size image `img` against the term's bound target; the gradient comes from the same call"""

    @staticmethod
    def forward(ctx, img, term):
        x = img.detach().reshape(3, term.hh, term.hw).float().contiguous()
        grad = torch.zeros_like(x)
        loss = torch.zeros(1, device=x.device)
        term.lib.call('aph_lpips_value_grad_half', term.handle, ptr(x), ptr(term.one), ptr(loss), ptr(grad), _stream(x))
        ctx.save_for_backward(grad)
        ctx.shape = img.shape
        return loss[0].to(img.dtype)

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g).reshape(ctx.shape).to(g.dtype), None


class LPIPS:
    """One aph_lpips handle for an (H, W) frame: the term runs on its half size [H // 2, W // 2]."""

    def __init__(self, weights, H, W, device='cuda', widths=WIDTHS, lib=None):
        self.device = torch.device(device)
        if lib is None and self.device.type != 'cuda':
            raise RuntimeError('aphantasia_amd: the HIP path needs CUDA (ROCm) tensors; got device %s. There is no CPU implementation.' % self.device)
        self.lib = lib if lib is not None else _ffi.lib()
        self.H, self.W, self.widths = int(H), int(W), tuple(int(c) for c in widths)
        self.hh, self.hw = self.H // 2, self.W // 2
        self.handle = None
        for name in weight_shapes(self.widths):
            if name not in weights:
                raise KeyError('LPIPS: weight %s missing' % name)
        h = c_void_p()
        self.lib.call('aph_lpips_create', (c_int * 5)(*self.widths), self.H, self.W, byref(h))
        self.handle = h
        for name, t in weights.items():
            t = t.detach().float().cpu().contiguous()
            self.lib.call('aph_lpips_set_weight', self.handle, name.encode(), c_void_p(t.data_ptr()), t.numel())
        self.one = torch.ones(1, device=self.device)
        self._target_key = None
        self.has_target = False

    def workspace_bytes(self):
        return int(self.lib.cdll.aph_lpips_workspace_bytes(self.handle))

    def set_target(self, img):
        """img [.., 3, h, w] in [0, 1]: the full frame (resized on the device) or already half size.  -> self"""
        t = img.detach().reshape(3, img.shape[-2], img.shape[-1]).float().contiguous().to(self.device)
        self.lib.call('aph_lpips_set_target', self.handle, ptr(t), int(t.shape[1]), int(t.shape[2]), _stream(t))
        self._target_key = None
        self.has_target = True
        return self

    def value_grad(self, rgb, d_weight, d_loss, d_grad, stream=None):
        """the C call on the full frame: rgb [3,H,W]; d_weight one device float; *d_loss += w value, d_grad += w gradient (either may be None)"""
        self.lib.call('aph_lpips_value_grad', self.handle, ptr(rgb), ptr(d_weight), ptr(d_loss), ptr(d_grad), stream if stream is not None else _stream(rgb))

    def __call__(self, img, img_in, normalize=True):
        """the reference's call: sim_loss(img, img_in, normalize=True) on HALF-size images [1,3,H//2,W//2] -> scalar with a gradient edge to img"""
        if not normalize:
            raise NotImplementedError('LPIPS: only normalize=True (images in [0, 1]) is built, as the reference calls it')
        for t in (img, img_in):
            if tuple(t.shape[-2:]) != (self.hh, self.hw) or t.numel() != 3 * self.hh * self.hw:
                raise ValueError('LPIPS: expected [1, 3, %d, %d] images (half of the %d x %d frame), got %s' % (self.hh, self.hw, self.H, self.W, tuple(t.shape)))
        key = (img_in.data_ptr(), img_in._version)
        if self._target_key != key:
            self.set_target(img_in)
            self._target_key = key
        return _ValueGrad.apply(img, self)

    def close(self):
        if self.handle is not None:
            self.lib.call('aph_lpips_destroy', self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load(H, W, vgg_path=None, lpips_path=None, device='cuda', seed=0, lib=None):
    """-> LPIPS for an (H, W) frame at the VGG-16 widths, from local weight files or (neither given) synthetic weights"""
    return LPIPS(load_weights(vgg_path, lpips_path, WIDTHS, seed), H, W, device=device, lib=lib)
