"""The three geometric augment chains (-tf fast | custom | elastic) side by side at C2 (1280x720, ViT-B/32 on seeded synthetic weights, 190 cuts),
on one GPU in one process.  Prints a text report and writes it to --out (default profiles/tf_chains.txt).

1. The whole Engine step (bulk draws, graph replay): blocks of --block steps between HIP events, the three engines alternating, per-block
   steps/s; median, quartiles, min and max per chain.  `custom` does strictly less than `fast` (no perspective pass, no scratch round trip
   after the crop): its median must not fall below fast's by more than the spread (max - min) of fast's own blocks in this run -- the
   report says whether it did, and gives the interquartile range beside it.
2. The sampler calls alone at the same geometry: aph_sample_fwd[_tf] (crop + resize, then the chain) and aph_sample_bwd[_tf] (the chain's
   adjoint, then the crop adjoint) between events, alternating with the plain crop (`-tf none`), medians; chain cost = call - plain crop.

    python tools/tf_bench.py [--reps 30] [--block 10] [--out PATH]
"""
import argparse
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aphantasia_amd import _ffi, clip as aclip, ops, transforms  # noqa: E402
from aphantasia_amd.engine import Engine  # noqa: E402
from aphantasia_amd.utils import draw_crop_params_bulk  # noqa: E402

H, W, S, SIZE, PATCH = 720, 1280, 190, 224, 32
CHAINS = dict(fast=transforms.transforms_fast, custom=transforms.transforms_custom, elastic=transforms.transforms_elastic)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup):
    """{name: [ms]} of `reps` timings of each callable, taken in alternating order after `warmup` untimed rounds"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for r in range(reps):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            ms[k].append(timed(fns[k]))
    return ms


def quart(v):
    q = statistics.quantiles(v, n=4)
    return min(v), q[0], statistics.median(v), q[2], max(v)


def bench_steps(reps, block, lines):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, _ = aclip.load('ViT-B/32', seed=1, max_batch=S)
    target = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))
    engines = {}
    for name, tf in CHAINS.items():
        torch.manual_seed(0)
        np.random.seed(0)
        p0 = (0.01 * torch.randn(1, 3, H, W // 2 + 1, 2)).cuda().contiguous()
        engines[name] = Engine(p0, H, W, model, S, [(target, -1.0)], sim='mix', transform=tf)

    def steps(e):
        def run():
            for _ in range(block):
                e.step()
        return run
    ms = alternate({k: steps(e) for k, e in engines.items()}, reps, warmup=2)
    rate = {k: [1e3 * block / t for t in v] for k, v in ms.items()}
    lines.append('whole step, %dx%d, ViT-B/32, %d cuts, bulk draws, graph replay (%s); %d blocks of %d steps per chain, alternating' %
                 (W, H, S, ', '.join('%s: %s' % (k, 'captured' if e._graph is not None else 'EAGER') for k, e in engines.items()), reps, block))
    lines.append('  chain     steps/s: min     q1    median     q3     max     ms/step (median)   skipped steps')
    for k, v in rate.items():
        lo, q1, med, q3, hi = quart(v)
        lines.append('  %-8s %14.2f %7.2f %8.2f %7.2f %7.2f %14.3f %14d' % (k, lo, q1, med, q3, hi, 1e3 / med, int(engines[k].guard[0])))
    flo, fq1, fmed, fq3, fhi = quart(rate['fast'])
    for k in ('custom', 'elastic'):
        med = statistics.median(rate[k])
        lines.append('  %s - fast: %+.2f steps/s (%+.2f %%); spread of fast\'s blocks: max - min %.2f, interquartile %.2f -> %s' %
                     (k, med - fmed, 100 * (med - fmed) / fmed, fhi - flo, fq3 - fq1,
                      'not below fast by more than its spread' if med >= fmed - (fhi - flo) else 'BELOW fast by more than its spread'))
    del engines
    return rate


def bench_sampler(reps, lines):
    dev = 'cuda'
    geom = ops.make_geom(H, W, S, SIZE, PATCH, 'uniform')
    rng = np.random.default_rng(1)
    rgb = torch.rand(3, H, W, device=dev)
    grgb = torch.empty_like(rgb)
    patches = torch.empty(S * (SIZE // PATCH) ** 2, 3 * PATCH * PATCH, dtype=torch.float16, device=dev)
    gpatch = torch.randn(patches.shape, device=dev)
    fwd, bwd = {}, {}
    keep = []
    for name in ('none',) + tuple(CHAINS):
        tf = CHAINS.get(name)
        table, aug = draw_crop_params_bulk(S, SIZE, H, W, 'uniform', 0.4, tf, rng)
        table = torch.from_numpy(table).to(dev)
        aug = torch.from_numpy(aug).to(dev) if aug is not None else None
        kind = tf.kind if tf is not None else _ffi.APH_TF_FAST
        ws = ops.sample_ws(geom, aug is not None, dev, None, kind)
        keep.append((table, aug, ws))
        fwd[name] = (lambda t=table, a=aug, w=ws, k=kind: ops.sample_fwd(geom, rgb, t, a, w, patches, _ffi.APH_OUT_PATCH_F16, tf=k))
        bwd[name] = (lambda t=table, a=aug, w=ws, k=kind: ops.sample_bwd(geom, gpatch, t, a, w, grgb, _ffi.APH_OUT_PATCH_F16, tf=k))
    lines.append('')
    lines.append('sampler calls alone, same geometry, f16 patch rows out / f32 patch-major gradient in; median of %d, alternating; us' % reps)
    lines.append('  chain      forward call   chain part   backward call   chain part')
    mf = {k: statistics.median(v) * 1e3 for k, v in alternate(fwd, reps, warmup=5).items()}
    mb = {k: statistics.median(v) * 1e3 for k, v in alternate(bwd, reps, warmup=5).items()}
    for k in fwd:
        lines.append('  %-8s %14.1f %12.1f %15.1f %12.1f' % (k, mf[k], mf[k] - mf['none'], mb[k], mb[k] - mb['none']))
    return mf, mb


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=30)
    p.add_argument('--block', type=int, default=10)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tf_chains.txt'))
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('tf_bench.py measures on the GPU; none is available')
    lines = ['tools/tf_bench.py --reps %d --block %d on %s' % (a.reps, a.block, torch.cuda.get_device_name(0))]
    bench_steps(a.reps, a.block, lines)
    bench_sampler(a.reps, lines)
    text = '\n'.join(lines) + '\n'
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
