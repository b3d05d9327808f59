"""CPPN image generator: host side of the reference's `cppn.py` network (cppn.py:71-116) -- a coordinate network of 1x1 convolutions whose
weights are the optimised parameters, image = sigmoid(net(x, y)).

Every weight and bias lives in ONE flat fp32 buffer (per conv in network order: weight [out, in, 1, 1], then bias [out]); the per-tensor views
under the reference's `state_dict` keys (`net.<i>.conv.weight` / `.bias`) share that storage, so the fused engine runs Adam and the multi-GPU
all-reduce on the flat buffer while torch.optim and the `.npy` snapshots keep working.  Forward and backward are one C-ABI call each
(csrc/synth_cppn.h: every layer fused per pixel tile on the f32-input MFMA, deterministic gradient sums).
"""
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _ffi, ops

ACTS = {'unbias': 0, 'comp': 1, 'relu': 2}
MAX_LAYERS, MAX_NF = 12, 32


def layer_table(layers, nf, actfn):
    """[(nf_in, nf_out)] of the layers + 1 convolutions (cppn.py:103-110)"""
    nhi = nf if actfn == 'relu' else 2 * nf
    return [(2, nf)] + [(nhi, nf)] * (layers - 1) + [(nhi, 3)]


def param_count(layers, nf, actfn):
    return sum(i * o + o for i, o in layer_table(layers, nf, actfn))


def mgrid_tables(h, w):
    """The two coordinate tables of get_mgrid (cppn.py:135-139: float64 linspace, cast to f32): channel 0 = x along W, channel 1 = y along H."""
    return torch.from_numpy(np.linspace(-1, 1, num=w).astype(np.float32)), torch.from_numpy(np.linspace(-1, 1, num=h).astype(np.float32))


class CPPNSynth:
    """The layer table, the coordinate tables, the workspace, and forward / backward on a flat parameter buffer."""

    def __init__(self, h, w, layers, nf, actfn, device, lib=None):
        if actfn not in ACTS:
            raise ValueError('unknown activation %r (available: %s)' % (actfn, ', '.join(ACTS)))
        if not (1 <= layers <= MAX_LAYERS and 1 <= nf <= MAX_NF):
            raise ValueError('CPPN: layers = %d, nf = %d; supported 1 .. %d layers of 1 .. %d features' % (layers, nf, MAX_LAYERS, MAX_NF))
        self.lib = lib if lib is not None else _ffi.lib()
        self.H, self.W, self.layers, self.nf, self.actfn, self.act = h, w, layers, nf, actfn, ACTS[actfn]
        self.table = layer_table(layers, nf, actfn)
        self.shapes, self.offsets, n = [], [], 0
        for i, o in self.table:
            for s in ((o, i, 1, 1), (o,)):
                self.shapes.append(s)
                self.offsets.append(n)
                n += math.prod(s)
        self.numel = n
        assert n == int(self.lib.cdll.aph_cppn_param_count(layers, nf, self.act))
        self.keys = [k for j in range(len(self.table)) for k in ('net.%d.conv.weight' % j, 'net.%d.conv.bias' % j)]
        xs, ys = mgrid_tables(h, w)
        self.xs, self.ys = xs.to(device), ys.to(device)
        nbytes = int(self.lib.cdll.aph_cppn_ws_bytes(layers, nf, self.act, h, w))
        self.ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        self.rgb = torch.empty(3, h, w, dtype=torch.float32, device=device)

    def views(self, flat):
        return [flat[o:o + math.prod(s)].view(s) for o, s in zip(self.offsets, self.shapes)]

    def state_dict(self, flat):
        return OrderedDict(zip(self.keys, self.views(flat)))

    def _args(self, flat):
        return (ops.ptr(flat), self.layers, self.nf, self.act, ops.ptr(self.xs), ops.ptr(self.ys), self.H, self.W)

    def forward(self, flat, out=None, stash=True, ws=None):
        """flat parameters -> rgb [3, H, W] (default: the tensor owned by this object).  stash=False: a forward that no backward follows."""
        out = self.rgb if out is None else out
        ws = self.ws if ws is None else ws
        self.lib.call('aph_cppn_fwd', *self._args(flat), ops.ptr(ws) if stash else None, ops.ptr(out), ops._stream(flat))
        return out

    def backward(self, flat, d_rgb, grad_flat, rgb=None, gscale=1.0, ws=None):
        """d_rgb [3, H, W] -> the gradient of every weight and bias, written into grad_flat (the parameters' layout); adjoint of the last
        stashing forward on `ws`, whose output was `rgb`"""
        rgb = self.rgb if rgb is None else rgb
        ws = self.ws if ws is None else ws
        if not d_rgb.is_contiguous() or d_rgb.numel() != 3 * self.H * self.W:
            raise ValueError('d_rgb must be a contiguous [3,%d,%d] tensor' % (self.H, self.W))
        self.lib.call('aph_cppn_bwd', *self._args(flat), ops.ptr(d_rgb), float(gscale), ops.ptr(rgb), ops.ptr(ws), ops.ptr(grad_flat),
                      ops._stream(flat))
        return grad_flat


def init_flat(layers, nf, actfn):
    """The reference's initial weights, consuming torch's global generator exactly as constructing its CPPN on the CPU does (cppn.py:75,
    84-86, per conv: nn.Conv2d's own initialisation, then weight.normal_(0, sqrt(1 / nf_in)), bias.uniform_(-.5, .5)) -> flat host tensor"""
    parts = []
    for i, o in layer_table(layers, nf, actfn):
        conv = torch.nn.Conv2d(i, o, 1, 1)
        with torch.no_grad():
            conv.weight.normal_(0., math.sqrt(1. / i))
            conv.bias.uniform_(-.5, .5)
        parts += [conv.weight.detach().reshape(-1), conv.bias.detach().reshape(-1)]
    return torch.cat(parts)


# ---- snapshots: the reference's .npy list format (cppn.py:150-162 export_data, :118-133 load_cppn) ---------------------------------
def export_data(cppn_dict, out_name):
    """state_dict -> out_name.npy: an object array [w0, b0, w1, b1, ...] with every weight permuted (3, 2, 1, 0)"""
    keys = list(cppn_dict.keys())
    arrays = []
    for lnum in range(0, len(keys), 2):
        arrays += [cppn_dict[keys[lnum]].detach().permute((3, 2, 1, 0)).cpu().numpy(), cppn_dict[keys[lnum + 1]].detach().cpu().numpy()]
    out = np.empty(len(arrays), dtype=object)
    for i, a in enumerate(arrays):
        out[i] = a
    np.save(out_name + '.npy', out)


def arrays_to_flat(arrays, actfn=None):
    """the arrays of a snapshot -> (flat host tensor, layers, nf, actfn).  The activation is inferred as at cppn.py:122: 'relu' when the
    second conv takes nf inputs, else the two-part one (`actfn` if it names one, else 'unbias')."""
    arrays = list(arrays)
    nf = int(arrays[0].shape[-1])
    layers = len(arrays) // 2 - 1
    if len(arrays) < 4 or len(arrays) % 2:
        raise ValueError('CPPN snapshot: %d arrays; expected weight / bias pairs of at least two convolutions' % len(arrays))
    act = 'relu' if arrays[0].shape[-1] == arrays[2].shape[-2] else (actfn if actfn in ('unbias', 'comp') else 'unbias')
    parts = []
    for (i, o), w, b in zip(layer_table(layers, nf, act), arrays[0::2], arrays[1::2]):
        w = torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(w, dtype=np.float32), (3, 2, 1, 0))))
        if tuple(w.shape) != (o, i, 1, 1) or tuple(np.shape(b)) != (o,):
            raise ValueError('CPPN snapshot: a conv of shape %s, expected %s' % (tuple(w.shape), (o, i, 1, 1)))
        parts += [w.reshape(-1), torch.from_numpy(np.asarray(b, dtype=np.float32)).reshape(-1)]
    return torch.cat(parts), layers, nf, act


def load_cppn(file, actfn=None):
    return arrays_to_flat(np.load(file, allow_pickle=True), actfn)


# ---- the drop-in autograd path ------------------------------------------------------------------------------------------------
class _CPPNFunction(torch.autograd.Function):
    """image_f(): the views are the leaves; each call owns its workspace and output until its backward has run"""

    @staticmethod
    def forward(ctx, gen, *views):
        flat = gen.flat_for(views)
        syn = gen.synth
        ws, rgb = torch.empty_like(syn.ws), torch.empty_like(syn.rgb)
        syn.forward(flat, out=rgb, ws=ws)
        ctx.gen, ctx.flat, ctx.ws, ctx.rgb = gen, flat, ws, rgb
        return rgb.unsqueeze(0)

    @staticmethod
    def backward(ctx, g):
        syn = ctx.gen.synth
        grad = torch.empty_like(ctx.flat)
        syn.backward(ctx.flat, g.reshape(3, syn.H, syn.W).float().contiguous(), grad, rgb=ctx.rgb, ws=ctx.ws)
        return (None,) + tuple(syn.views(grad))


class CPPNImage:
    """cppn.py's `snet(mgrid)` as a closure: `params` are leaf views into one flat buffer."""

    def __init__(self, h, w, layers, nf, actfn, device, lib=None):
        self.synth = CPPNSynth(h, w, layers, nf, actfn, device, lib=lib)
        self.flat = torch.empty(self.synth.numel, dtype=torch.float32, device=device)
        self.params = None

    def flat_for(self, views):
        mine = self.synth.views(self.flat)
        if all(v.data_ptr() == m.data_ptr() for v, m in zip(views, mine)):
            return self.flat
        return torch.cat([v.detach().reshape(-1).float() for v in views]).contiguous()

    def state_dict(self):
        return self.synth.state_dict(self.flat.detach())

    def __call__(self, *args, **kwargs):
        """-> rgb [1, 3, H, W] in (0, 1): the sigmoid output is the image, there is no to_valid_rgb stage"""
        return _CPPNFunction.apply(self, *self.params)


def cppn_image(shape, layers=10, nf=24, actfn='unbias', resume=None, device=None, lib=None):
    """-> (params, image_f, size): the list of weight / bias leaves in the reference's state_dict order, the generator, and None (a
    snapshot holds no size).  Random init draws from torch's global generator as the reference's CPPN(...) does; `resume`: a reference
    `.npy` snapshot (it then sets layers, nf and the activation, cppn.py:118-133) or the list of its arrays."""
    h, w = shape[2:]
    if resume is not None:
        if isinstance(resume, str):
            if not os.path.isfile(resume):
                print(' Snapshot not found:', resume)
                exit()
            init, layers, nf, actfn = load_cppn(resume, actfn)
        else:
            init, layers, nf, actfn = arrays_to_flat(resume, actfn)
    else:
        init = init_flat(layers, nf, actfn)
    if device is None:
        from .image import _device
        device = _device()
    gen = CPPNImage(h, w, layers, nf, actfn, device, lib=lib)
    gen.flat.copy_(init)
    gen.params = [v.requires_grad_(True) for v in gen.synth.views(gen.flat)]
    return gen.params, gen, None
