"""The --sync term's cost on the GPU.  Prints ONE JSON line and writes it to --out (default profiles/sync_bench.json).

1. aph_lpips_value_grad alone (VGG-16 widths, seeded synthetic weights) on a 1280x720 frame (the network runs at 640x360) and on 512x512,
   against the same term as stock torch ops under autograd on the same GPU in the same process: (a) in fp32 -- what the reference runs
   (`.float()`), the fallback a user had until now -- and (b) in f16.  HIP events around each value + gradient, warm-up, the three
   alternating, the median of --reps repetitions.  Beside them the floors: the convolutions' FLOPs (forward + input gradient, no weight
   gradient) at the f16 MFMA peak, and the bytes the f16 NHWC layout moves at 5 TB/s.
2. The whole Engine step at clip_fft.py's geometry with `-i IMG --sync 1` (1280x720, ViT-B/32 on seeded synthetic weights, 95 cuts, align
   overscan, graph replay) against the same 95-cut step without the term: blocks of --block steps between events, alternating, medians.

    python tools/sync_bench.py [--reps 20] [--block 10] [--out PATH] [--no-engine]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from aphantasia_amd import clip as aclip, transforms  # noqa: E402
from aphantasia_amd import lpips as alpips  # noqa: E402
from aphantasia_amd.engine import Engine  # noqa: E402

PEAK_F16_TF = 2516.6         # v_mfma_f32_16x16x32_f16: 1024 FLOP / clock / SIMD x 1024 SIMDs x 2.4 GHz
HBM_TBS = 5.0
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)


def floors(h, w):
    """convolution FLOPs (forward + dgrad) and the bytes of the f16 activations written and read, for a frame h x w"""
    hh, hw, flop, bytes_ = h // 2, w // 2, 0.0, 0.0
    for _, cin, cout, s in alpips.layer_table():
        p = (hh >> s) * (hw >> s)
        flop += 2 * 2.0 * 9 * cin * cout * p
        bytes_ += 2.0 * p * (cin + cout) * 2 * 2          # forward: read in, write out; dgrad: read gradient, write gradient
        bytes_ += 2.0 * p * cout                          # the ReLU mask read
    return dict(conv_gflop=round(flop / 1e9, 1), mfma_floor_ms=round(flop / (PEAK_F16_TF * 1e12) * 1e3, 4), traffic_mb=round(bytes_ / 1e6, 1),
                traffic_floor_ms=round(bytes_ / (HBM_TBS * 1e12) * 1e3, 4))


class TorchLPIPS:
    """the term as stock torch ops (conv2d, max_pool2d, autograd) in `dtype`; the target's normalised taps are constants"""

    def __init__(self, weights, target, dtype):
        self.dtype = dtype
        self.w = {k: v.cuda().to(dtype) for k, v in weights.items()}
        self.sh = torch.tensor(SHIFT, device='cuda', dtype=dtype).view(1, 3, 1, 1)
        self.sc = torch.tensor(SCALE, device='cuda', dtype=dtype).view(1, 3, 1, 1)
        with torch.no_grad():
            self.ny = [self.norm(f) for f in self.features(self.resize(target))]

    def resize(self, img):
        return F.interpolate(img[None], [img.shape[-2] // 2, img.shape[-1] // 2], mode='bicubic', align_corners=True).to(self.dtype)

    def features(self, x):
        x = ((2 * x - 1) - self.sh) / self.sc
        taps, k = [], 0
        for s, n in enumerate(alpips.CONVS_OF_STAGE):
            if s:
                x = F.max_pool2d(x, 2, 2)
            for _ in range(n):
                i = alpips.FEATURE_IDX[k]
                x = torch.relu(F.conv2d(x, self.w['features.%d.weight' % i], self.w['features.%d.bias' % i], padding=1))
                k += 1
            taps.append(x)
        return taps

    @staticmethod
    def norm(f):
        return f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)

    def value_grad(self, rgb):
        leaf = rgb.detach().requires_grad_(True)
        total = 0
        for l, (f, ny) in enumerate(zip(self.features(self.resize(leaf)), self.ny)):
            total = total + (self.w['lin%d.weight' % l].view(1, -1, 1, 1) * (self.norm(f) - ny) ** 2).sum(1).mean()
        total.float().backward()
        return total.detach(), leaf.grad


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup=3):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for r in range(reps):
        order = list(fns) if r % 2 == 0 else list(fns)[::-1]
        for k in order:
            ms[k].append(timed(fns[k]))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}, {k: round(min(v), 4) for k, v in ms.items()}


def bench_term(h, w, reps):
    gen = torch.Generator().manual_seed(0)
    weights = alpips.synthetic_weights(alpips.WIDTHS, 1)
    rgb, target = torch.rand(3, h, w, generator=gen).cuda(), torch.rand(3, h, w, generator=gen).cuda()
    term = alpips.LPIPS(weights, h, w).set_target(target)
    loss, grad, one = torch.zeros(1, device='cuda'), torch.zeros(3, h, w, device='cuda'), torch.ones(1, device='cuda')
    t32, t16 = TorchLPIPS(weights, target, torch.float32), TorchLPIPS(weights, target, torch.float16)

    def fused():
        term.value_grad(rgb, one, loss, grad)
    med, best = alternate(dict(fused=fused, torch_fp32=lambda: t32.value_grad(rgb), torch_f16=lambda: t16.value_grad(rgb)), reps)
    loss.zero_(); grad.zero_()
    fused()
    v32, g32 = t32.value_grad(rgb)
    torch.cuda.synchronize()
    out = dict(h=h, w=w, median_ms=med, min_ms=best, vs_torch_fp32=round(med['torch_fp32'] / med['fused'], 2), vs_torch_f16=round(med['torch_f16'] / med['fused'], 2),
               value=float(loss), value_torch_fp32=float(v32), grad_rel_l2_vs_torch_fp32=float('%.3g' % ((grad - g32).norm() / g32.norm()).item()),
               arena_mb=round(term.workspace_bytes() / 2 ** 20, 1))
    out.update(floors(h, w))
    out['conv_tflops'] = round(out['conv_gflop'] / med['fused'], 1)
    term.close()
    return out


def bench_engine(reps, block):
    h, w, S = 720, 1280, 95
    torch.manual_seed(0)
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, _ = aclip.load('ViT-B/32', seed=1, max_batch=S)
    target = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))
    term = alpips.LPIPS(alpips.synthetic_weights(alpips.WIDTHS, 1), h, w).set_target(torch.rand(3, h, w).cuda())
    common = dict(sim='mix', align='overscan', macro=0.4, transform=transforms.normalize())
    p0 = (0.01 * torch.randn(1, 3, h, w // 2 + 1, 2)).cuda().contiguous()
    engines = dict(sync=Engine(p0.clone(), h, w, model, S, [(target, -1.0)], sync=term, **common), plain=Engine(p0.clone(), h, w, model, S, [(target, -1.0)], **common))

    def steps(name):
        e = engines[name]

        def run():
            for _ in range(block):
                e.step(sync_weight=0.5) if name == 'sync' else e.step()
        return run
    med, best = alternate({k: steps(k) for k in engines}, reps, warmup=2)
    per = {k: round(v / block, 4) for k, v in med.items()}
    return dict(config=dict(h=h, w=w, model='ViT-B/32', samples=S, align='overscan', graph=True, block=block), ms_per_step=per,
                min_ms_per_step={k: round(v / block, 4) for k, v in best.items()}, sync_cost_ms=round(per['sync'] - per['plain'], 4),
                graph_captured={k: e._graph is not None for k, e in engines.items()}, skipped_steps={k: int(e.guard[0]) for k, e in engines.items()})


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--block', type=int, default=10)
    p.add_argument('--no-engine', action='store_true')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sync_bench.json'))
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('sync_bench.py measures on the GPU; none is available')
    out = dict(metric='sync_lpips', reps=a.reps, device=torch.cuda.get_device_name(0), term=[bench_term(720, 1280, a.reps), bench_term(512, 512, a.reps)])
    if not a.no_engine:
        out['engine_step'] = bench_engine(a.reps, a.block)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
