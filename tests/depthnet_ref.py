"""fp64 restatement of transformers' DepthAnythingForDepthEstimation (models/dinov2/modeling_dinov2.py, models/depth_anything/
modeling_depth_anything.py) from a config and a state dict with transformers' parameter names -- what csrc/depth.hip is tested against.

    forward(config, sd, img)                 pure fp64: equals the transformers model in .double() to round-off (test_depthnet_ref.py)
    forward(config, sd, img, rounding=True)  the same arithmetic with the kernels' rounding points: f16 weights, f16 GEMM / attention /
                                             convolution operands and outputs, an unrounded residual stream, P rounded to f16 before P V

Both return the un-normalised map [B, h, w] and, with pre=True, the input of the last ReLU.  The position rows come from
aphantasia_amd.depthnet.position_rows (transformers interpolates them in fp32 whatever the model's dtype, and so does that)."""
import math

import torch
import torch.nn.functional as F

from aphantasia_amd import depthnet as DN

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _r16(rounding):
    return (lambda t: t.half().double()) if rounding else (lambda t: t)


def encoder_layer(x, sd, p, heads, q16, lam_fold):
    """one DINOv2 block on x [B, T, D] (fp64)"""
    D = x.shape[-1]
    W = lambda n: sd[p + n].double()
    h = q16(F.layer_norm(x, (D,), W('norm1.weight'), W('norm1.bias'), 1e-6))
    qkv = [q16(h @ q16(W('attention.attention.%s.weight' % n)).T + W('attention.attention.%s.bias' % n)) for n in ('query', 'key', 'value')]
    B, T, _ = x.shape
    q, k, v = (t.reshape(B, T, heads, 64).transpose(1, 2) for t in qkv)
    s = q @ k.transpose(-1, -2) / 8.0
    e = torch.exp(s - s.amax(-1, keepdim=True))
    att = q16((q16(e) @ v) / e.sum(-1, keepdim=True)).transpose(1, 2).reshape(B, T, D)
    wo, bo = lam_fold(W('attention.output.dense.weight'), W('attention.output.dense.bias'), W('layer_scale1.lambda1'))
    x = x + att @ q16(wo).T + bo
    h = q16(F.layer_norm(x, (D,), W('norm2.weight'), W('norm2.bias'), 1e-6))
    g = q16(F.gelu(h @ q16(W('mlp.fc1.weight')).T + W('mlp.fc1.bias')))
    w2, b2 = lam_fold(W('mlp.fc2.weight'), W('mlp.fc2.bias'), W('layer_scale2.lambda1'))
    return x + g @ q16(w2).T + b2


def forward(config, sd, img, rounding=False, pre=False):
    c = DN.parse_config(config)
    q16 = _r16(rounding)
    if rounding:      # LayerScale folded into the weights in fp32, as the library's upload does, then rounded with them
        lam_fold = lambda w, b, lam: ((w.float() * lam.float()[:, None]).double(), (b.float() * lam.float()).double())
    else:
        lam_fold = lambda w, b, lam: (w * lam[:, None], b * lam)
    W = lambda n: sd[n].double()
    img = img.double()
    B, _, h, w = img.shape
    gh, gw = h // 14, w // 14
    D = c['hidden']
    x = (img - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    x = F.conv2d(q16(x), q16(W('backbone.embeddings.patch_embeddings.projection.weight')), W('backbone.embeddings.patch_embeddings.projection.bias'), stride=14)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([W('backbone.embeddings.cls_token').expand(B, -1, -1), x], 1)
    x = x + DN.position_rows(sd['backbone.embeddings.position_embeddings'].double(), gh, gw)[None]
    taps = []
    for i in range(c['layers']):
        x = encoder_layer(x, sd, 'backbone.encoder.layer.%d.' % i, c['heads'], q16, lam_fold)
        for _ in range(c['out_indices'].count(i + 1)):      # (a layer tapped twice: not transformers', the GPU test's two-layer network)
            t = q16(F.layer_norm(x, (D,), W('backbone.layernorm.weight'), W('backbone.layernorm.bias'), 1e-6))
            taps.append(t[:, 1:].reshape(B, gh, gw, D).permute(0, 3, 1, 2))
    feats = []
    for i, t in enumerate(taps):
        p = 'neck.reassemble_stage.layers.%d.' % i
        t = q16(F.conv2d(t, q16(W(p + 'projection.weight')), W(p + 'projection.bias')))
        if i < 2:
            t = q16(F.conv_transpose2d(t, q16(W(p + 'resize.weight')), W(p + 'resize.bias'), stride=(4, 2)[i]))
        elif i == 3:
            t = q16(F.conv2d(t, q16(W(p + 'resize.weight')), W(p + 'resize.bias'), stride=2, padding=1))
        feats.append(q16(F.conv2d(t, q16(W('neck.convs.%d.weight' % i)), None, padding=1)))

    def unit(t, p, extra=None):
        y = q16(torch.relu(F.conv2d(torch.relu(t), q16(W(p + 'convolution1.weight')), W(p + 'convolution1.bias'), padding=1)))
        y = F.conv2d(y, q16(W(p + 'convolution2.weight')), W(p + 'convolution2.bias'), padding=1) + t
        return q16(y + extra if extra is not None else y)

    fused = None
    for idx in range(4):
        i = 3 - idx
        p = 'neck.fusion_stage.layers.%d.' % idx
        hid = feats[i] if fused is None else unit(feats[i], p + 'residual_layer1.', fused)
        hid = unit(hid, p + 'residual_layer2.')
        size = feats[i - 1].shape[2:] if idx < 3 else (2 * hid.shape[2], 2 * hid.shape[3])
        hid = q16(F.interpolate(hid, size=tuple(size), mode='bilinear', align_corners=True))
        fused = q16(F.conv2d(hid, q16(W(p + 'projection.weight')), W(p + 'projection.bias')))
    y = q16(F.conv2d(fused, q16(W('head.conv1.weight')), W('head.conv1.bias'), padding=1))
    y = q16(F.interpolate(y, size=(h, w), mode='bilinear', align_corners=True))
    y = q16(torch.relu(F.conv2d(y, q16(W('head.conv2.weight')), W('head.conv2.bias'), padding=1)))
    z = F.conv2d(y, W('head.conv3.weight'), W('head.conv3.bias'))[:, 0]
    return (torch.relu(z), z) if pre else torch.relu(z)


def normalise(d):
    lo = d.flatten(1).amin(1).view(-1, 1, 1)
    hi = d.flatten(1).amax(1).view(-1, 1, 1)
    return (d - lo) / (hi - lo)


def conditioned_weights(config, seed, img):
    """synthetic weights whose last bias is 3 std - mean of the fp64 pre-activation on `img`: the final ReLU then passes >= 99 % of the pixels
    (checked by the callers) and cannot hide an error.  -> (weights, the fp64 pre-activation under them: the bias is the last thing added)"""
    sd = DN.synthetic_weights(config, seed)
    _, z = forward(config, sd, img, pre=True)
    sd = DN.synthetic_weights(config, seed, last_bias=float(3.0 * z.std() - z.mean()))
    return sd, z + sd['head.conv3.bias'].double()
