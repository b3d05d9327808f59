"""fp64 restatement of the --sync term: lpips.LPIPS(net='vgg') v0.1 with normalize=True on the half-size bicubic resize of two images
(reference clip_fft.py:219-222, 268-270), in plain torch on the CPU.

The lpips package is not installed where this project is developed: the definition below is restated from memory of that package and was
NEVER run against it.  It is the specification the kernels of csrc/lpips.hip are tested against.

  x = bicubic_resize(rgb, [H // 2, W // 2], align_corners=True)            (A = -0.75, no antialias)
  t = 2 x - 1;  t_c = (t_c - shift_c) / scale_c
  VGG-16 features: 13 x (conv 3x3 pad 1 + bias + ReLU), widths 64,64 | 128,128 | 256,256,256 | 512,512,512 | 512,512,512, a 2x2 stride-2 floor
  max-pool before stages 2 .. 5; taps f_1 .. f_5 = the ReLU outputs that end each stage
  n_l = f_l / (sqrt(sum_c f_l^2) + 1e-10);  d_l = mean_hw sum_c lin_l[c] (n_l(x) - n_l(y))^2;  value = sum_l d_l

`rounding` switches on the kernels' rounding model: weights, the network input and every stored activation rounded to f16 where the kernels
store them, and the backward stream rounded to f16 (times the handle's power-of-two scale, saturating) where the kernels store it: after every
ReLU mask, and at the pooled gradient.  The head, the resize and all sums stay fp64."""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
CONVS_OF_STAGE = (2, 2, 3, 3, 3)
FEATURE_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
EPS = 1e-10
F16_MAX = 65504.0


def resize_half(img):
    """img [3, H, W] -> [3, H // 2, W // 2]"""
    return F.interpolate(img[None], size=[img.shape[-2] // 2, img.shape[-1] // 2], mode='bicubic', align_corners=True)[0]


def scale_input(x):
    sh = torch.tensor(SHIFT, dtype=x.dtype).view(3, 1, 1)
    sc = torch.tensor(SCALE, dtype=x.dtype).view(3, 1, 1)
    return ((2 * x - 1) - sh) / sc


def f16(x):
    return x.to(torch.float16).to(x.dtype)


class _Stored(torch.autograd.Function):
    """a buffer the kernels store as f16: the value is rounded on the way up (fwd), the gradient (times gscale, saturating) on the way down"""

    @staticmethod
    def forward(ctx, x, fwd, gscale):
        ctx.gscale = gscale
        return f16(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.gscale is None:
            return g, None, None
        return f16((g * ctx.gscale).clamp(-F16_MAX, F16_MAX)) / ctx.gscale, None, None


def gscale_of(hh, hw):
    """the power of two csrc/lpips.hip scales its f16 backward stream by: 16 x the half-size pixel count rounded up to a power of two"""
    e = 0
    while (1 << e) < hh * hw:
        e += 1
    return float(2 ** (e + 4))


def features(t, weights, rounding=False, gscale=None):
    """t [3, h, w] scaled input -> the five taps [C_l, h_l, w_l]"""
    x = t[None]
    if rounding:
        x = _Stored.apply(x, True, None)
    taps, k = [], 0
    for s, n in enumerate(CONVS_OF_STAGE):
        if s:
            x = F.max_pool2d(x, 2, 2)
            if rounding:
                x = _Stored.apply(x, False, gscale)
        for _ in range(n):
            w = weights['features.%d.weight' % FEATURE_IDX[k]].to(t.dtype)
            b = weights['features.%d.bias' % FEATURE_IDX[k]].to(t.dtype)
            z = F.conv2d(x, f16(w) if rounding else w, b, padding=1)
            if rounding:
                z = _Stored.apply(z, True, gscale)
            x = torch.relu(z)
            k += 1
        taps.append(x[0])
    return taps


def unit_norm(f):
    """f [C, h, w] -> f / (sqrt(sum_c f^2) + eps); an all-zero column has norm 0 and derivative 1 / eps of its first-order term only"""
    ss = (f * f).sum(0, keepdim=True)
    pos = ss > 0
    s = torch.where(pos, torch.sqrt(torch.where(pos, ss, torch.ones_like(ss))), torch.zeros_like(ss))
    return f / (s + EPS)


def head(taps_x, normed_y, weights):
    total = 0
    for l, (fx, ny) in enumerate(zip(taps_x, normed_y)):
        lin = weights['lin%d.weight' % l].to(fx.dtype).view(-1, 1, 1)
        total = total + (lin * (unit_norm(fx) - ny) ** 2).sum(0).mean()
    return total


def value_and_grad(rgb, target, weights, rounding=False, dtype=torch.float64, resize=True):
    """rgb, target [3, H, W] in [0, 1] -> (value, dvalue/drgb [3, H, W]) in `dtype`; resize=False: the images already have the network's size"""
    w = {k: v.to(dtype) for k, v in weights.items()}
    rs = resize_half if resize else (lambda t: t)
    hh, hw = (rgb.shape[-2] // 2, rgb.shape[-1] // 2) if resize else rgb.shape[-2:]
    gs = gscale_of(hh, hw) if rounding else None
    with torch.no_grad():
        ny = [unit_norm(f) for f in features(scale_input(rs(target.to(dtype))), w, rounding, None)]
    leaf = rgb.detach().to(dtype).clone().requires_grad_(True)
    val = head(features(scale_input(rs(leaf)), w, rounding, gs), ny, w)
    val.backward()
    return val.detach(), leaf.grad.detach()
