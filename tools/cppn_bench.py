"""The CPPN generator's cost on the GPU, two ways.  Prints ONE JSON line and writes it to --out (default profiles/cppn_bench.json).

1. aph_cppn_fwd + aph_cppn_bwd alone (3 launches) for the default net (10 layers, nf 24, unbias) at 512x512 and 1280x720, against the same
   network as plain torch ops under autograd on the same GPU in the same process (what a user would otherwise run; independent of the code
   under test).  HIP events around each forward + backward, warm-up, the two alternating, the median of --reps repetitions.  Beside them the
   two floors: the f32 MFMAs the kernels issue at the 157.3 TF peak, and writing + reading the stash at 5 TB/s.
2. The whole Engine step at cppn.py's defaults (512x512, ViT-B/32 on seeded synthetic weights, 47 cuts, -tf fast, Adam, graph replay) against the
   same engine with param_kind='pixel', the step with no generator network: blocks of --block steps between events, alternating, medians.

    python tools/cppn_bench.py [--reps 30] [--block 10] [--out PATH]
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

from aphantasia_amd import clip as aclip, transforms  # noqa: E402
from aphantasia_amd.cppn import cppn_image, layer_table  # noqa: E402
from aphantasia_amd.engine import Engine  # noqa: E402

PEAK_F32_TF = 157.3          # v_mfma_f32_32x32x2_f32: 64 FLOP / clock / SIMD x 1024 SIMDs x 2.4 GHz
HBM_TBS = 5.0                # achievable HBM rate the stash floor is quoted at
LAYERS, NF, ACT = 10, 24, 'unbias'


def mfma_per_subtile(layers, nf, actfn):
    """32x32x2 MFMAs per 32-pixel sub-tile as csrc/synth_cppn.h issues them -> (forward, backward)"""
    nq, ks = (1 if actfn == 'relu' else 2), 4 * ((nf + 7) // 8)
    fwd = 1 + layers * nq * ks
    bwd = 16 + sum(16 * nq + nq * (4 if l == layers else ks) for l in range(1, layers + 1))
    return fwd, bwd


def floors_ms(h, w):
    fwd, bwd = mfma_per_subtile(LAYERS, NF, ACT)
    tiles = (h * w + 31) // 32
    flop = (fwd + bwd) * tiles * 2.0 * 32 * 32 * 2
    useful = 3 * 2.0 * sum(i * o for i, o in layer_table(LAYERS, NF, ACT)) * h * w
    stash = 2.0 * LAYERS * NF * 4 * h * w
    return dict(mfma_issued_gflop=round(flop / 1e9, 2), network_gflop=round(useful / 1e9, 2), mfma_floor_ms=round(flop / (PEAK_F32_TF * 1e12) * 1e3, 4),
                stash_mb=round(stash / 2 / 1e6, 1), stash_floor_ms=round(stash / (HBM_TBS * 1e12) * 1e3, 4))


def torch_net(views, xs, ys):
    """the network as torch ops on [C, H W] (cppn.py:71-116)"""
    h, w = ys.numel(), xs.numel()
    x = torch.stack([xs[None, :].expand(h, w), ys[:, None].expand(h, w)]).reshape(2, h * w)
    n = len(views) // 2
    for j in range(n):
        z = views[2 * j].reshape(views[2 * j].shape[0], -1) @ x + views[2 * j + 1][:, None]
        if j == n - 1:
            return torch.sigmoid(z).reshape(3, h, w)
        t = torch.atan(z)
        x = torch.cat([t / 0.67, (t * t - 0.45) / 0.396], 0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup=5):
    """{name: median ms} of `reps` timings of each callable, taken in alternating order after `warmup` untimed rounds"""
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


def bench_pair(h, w, reps):
    torch.manual_seed(0)
    params, gen, _ = cppn_image([1, 3, h, w], LAYERS, NF, ACT)
    syn, flat = gen.synth, gen.flat
    d_rgb = (torch.randn(3, h, w) / (h * w)).cuda().contiguous()
    grad = torch.empty_like(flat)
    leaves = [p.detach().clone().requires_grad_(True) for p in params]

    def fused():
        syn.forward(flat)
        syn.backward(flat, d_rgb, grad)

    def autograd():
        for p in leaves:
            p.grad = None
        (torch_net(leaves, syn.xs, syn.ys) * d_rgb).sum().backward()
    med, best = alternate(dict(fused=fused, torch_autograd=autograd), reps)
    fwd_only, _ = alternate(dict(fused_fwd=lambda: syn.forward(flat), fused_fwd_nostash=lambda: syn.forward(flat, stash=False)), reps)
    ref = torch.cat([p.grad.reshape(-1) for p in leaves])
    same = ((grad - ref).abs().max() / ref.abs().max()).item()
    out = dict(h=h, w=w, median_ms=med, min_ms=best, forward_ms=fwd_only, speedup=round(med['torch_autograd'] / med['fused'], 2),
               grad_max_rel_diff=float('%.3g' % same))
    out.update(floors_ms(h, w))
    return out


def bench_engine(reps, block):
    h = w = 512
    S = 47
    torch.manual_seed(0)
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, _ = aclip.load('ViT-B/32', seed=1, max_batch=S)
    target = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))
    common = dict(sim='cossim', lr=0.003, optimizer='adam', align='overscan', macro=0.4, transform=transforms.transforms_fast)
    _, gen, _ = cppn_image([1, 3, h, w], LAYERS, NF, ACT)
    engines = dict(cppn=Engine(gen.flat, h, w, model, S, [(target, -1.0)], param_kind='cppn', cppn=gen.synth, **common),
                   pixel=Engine((0.01 * torch.randn(1, 3, h, w)).cuda().contiguous(), h, w, model, S, [(target, -1.0)], param_kind='pixel', **common))

    def steps(e):
        def run():
            for _ in range(block):
                e.step()
        return run
    med, best = alternate({k: steps(e) for k, e in engines.items()}, reps, warmup=2)
    per = {k: round(v / block, 4) for k, v in med.items()}
    return dict(config=dict(h=h, w=w, model='ViT-B/32', samples=S, transform='fast', optimizer='adam', graph=True, block=block),
                ms_per_step=per, min_ms_per_step={k: round(v / block, 4) for k, v in best.items()},
                cppn_cost_ms=round(per['cppn'] - per['pixel'], 4), steps_per_s={k: round(1e3 / v, 2) for k, v in per.items()},
                graph_captured={k: e._graph is not None for k, e in engines.items()}, skipped_steps={k: int(e.guard[0]) for k, e in engines.items()})


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=30)
    p.add_argument('--block', type=int, default=10)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cppn_bench.json'))
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('cppn_bench.py measures on the GPU; none is available')
    out = dict(metric='cppn_generator', net=dict(layers=LAYERS, nf=NF, act=ACT), reps=a.reps, device=torch.cuda.get_device_name(0),
               fwd_bwd=[bench_pair(512, 512, a.reps), bench_pair(720, 1280, a.reps)], engine_step=bench_engine(a.reps, a.block))
    line = json.dumps(out)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
