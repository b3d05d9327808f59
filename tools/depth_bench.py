"""The depth estimator's cost on the GPU.  Prints ONE JSON line and writes it to --out (default profiles/depth_bench.json).

Per configuration (Small, Base; seeded synthetic weights) and size (518 x 910: what a 1280 x 720 frame gives; 518 x 518), a batch of two (the
image and its mirror, as depth_map sends them), three legs alternating on the same GPU in the same process:
  hip         DepthAnythingHIP (csrc/depth.hip), normalisation and min-max included
  torch_fp32  transformers' DepthAnythingForDepthEstimation in fp32 eager mode + InferDepthAny's normalisation and min-max: what
              `--depth_backend torch` runs
  torch_f16   the same model under torch.autocast(float16)
HIP events around each call, warm-up, the median and the minimum of --reps repetitions.  Beside them the floors: GEMM, attention and
convolution FLOPs at the f16 MFMA peak, and the f16 activation bytes (every kernel's output written once and read once) at 5 TB/s.

    python tools/depth_bench.py [--reps 10] [--configs small base] [--sizes 518x910 518x518] [--no-torch] [--hip-only-once] [--out PATH]

--hip-only-once: one warm-up call and ONE timed call of the HIP leg alone, for a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from aphantasia_amd import depthnet as DN  # noqa: E402

PEAK_F16_TF = 2516.6         # v_mfma_f32_16x16x32_f16: 1024 FLOP / clock / SIMD x 1024 SIMDs x 2.4 GHz
HBM_TBS = 5.0
CONFIGS = dict(small=DN.SMALL, base=DN.BASE, large=DN.LARGE)


def floors(config, h, w, B):
    """FLOPs by kind and the f16 activation bytes of one forward of B images"""
    c = DN.parse_config(config)
    D, L, F_, Hh = c['hidden'], c['layers'], c['fusion'], c['head']
    gh, gw = h // 14, w // 14
    P, T = gh * gw, gh * gw + 1
    gemm = 2.0 * B * P * 588 * D + L * 2.0 * B * T * D * (3 * D + D + 4 * D + 4 * D)
    attn = L * 4.0 * B * T * T * D
    act = L * 2.0 * B * T * D * (1 + 3 + 1 + 4) * 2 + L * 4.0 * B * T * D * 2 * 2          # f16 GEMM operands / outputs, the fp32 stream twice
    sizes = [(4 * gh, 4 * gw), (2 * gh, 2 * gw), (gh, gw), ((gh + 1) // 2, (gw + 1) // 2)]
    conv = 0.0
    for i, C in enumerate(c['neck']):
        hh, ww = sizes[i]
        gemm += 2.0 * B * P * D * C + (2.0 * B * P * C * C * (16, 4)[i] if i < 2 else 0.0)
        conv += (2.0 * 9 * B * P * C * C if i == 3 else 0.0) + 2.0 * 9 * B * hh * ww * C * F_
        act += 2.0 * B * hh * ww * (C + F_) * 2
    for idx in range(4):
        hh, ww = sizes[3 - idx]
        nh, nw = sizes[2 - idx] if idx < 3 else (2 * hh, 2 * ww)
        conv += (4 if idx else 2) * 2.0 * 9 * B * hh * ww * F_ * F_
        gemm += 2.0 * B * nh * nw * F_ * F_
        act += 2.0 * B * ((4 if idx else 2) * hh * ww + 2 * nh * nw) * F_ * 2
    conv += 2.0 * 9 * B * 64 * P * F_ * (F_ // 2) + 2.0 * 9 * B * h * w * (F_ // 2) * Hh
    act += 2.0 * B * (64 * P * (F_ // 2) + h * w * (F_ // 2) + h * w * Hh) * 2
    total = gemm + attn + conv
    return dict(gemm_gflop=round(gemm / 1e9, 1), attn_gflop=round(attn / 1e9, 1), conv_gflop=round(conv / 1e9, 1),
                mfma_floor_ms=round(total / (PEAK_F16_TF * 1e12) * 1e3, 3), activation_mb=round(act / 1e6, 1),
                traffic_floor_ms=round(act / (HBM_TBS * 1e12) * 1e3, 3))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup=2):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for r in range(reps):
        order = list(fns) if r % 2 == 0 else list(fns)[::-1]
        for k in order:
            ms[k].append(timed(fns[k]))
    return ({k: round(statistics.median(v), 3) for k, v in ms.items()}, {k: round(min(v), 3) for k, v in ms.items()},
            {k: round(max(v), 3) for k, v in ms.items()})


def torch_model(config, sd):
    from transformers import DepthAnythingConfig, DepthAnythingForDepthEstimation, Dinov2Config
    c = DN.parse_config(config)
    bc = Dinov2Config(hidden_size=c['hidden'], num_hidden_layers=c['layers'], num_attention_heads=c['heads'], image_size=518, patch_size=14,
                      out_indices=c['out_indices'], apply_layernorm=True, reshape_hidden_states=False)
    cfg = DepthAnythingConfig(backbone_config=bc, reassemble_hidden_size=c['hidden'], neck_hidden_sizes=c['neck'], fusion_hidden_size=c['fusion'],
                              head_hidden_size=c['head'], reassemble_factors=[4, 2, 1, 0.5])
    model = DepthAnythingForDepthEstimation(cfg)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def bench(name, h, w, reps, with_torch, once):
    config, B = CONFIGS[name], 2
    sd = DN.synthetic_weights(config, seed=1, last_bias=2.0)
    img = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(0)).cuda()
    net = DN.DepthAnythingHIP.from_state_dict(config, sd, max_hw=(h, w), max_batch=B)
    legs = dict(hip=lambda: net(img))
    out = dict(config=name, h=h, w=w, batch=B, arena_mb=round(net.workspace_bytes() / 2 ** 20, 1))
    out.update(floors(config, h, w, B))
    if once:
        net(img)
        torch.cuda.synchronize()
        out['hip_once_ms'] = round(timed(legs['hip']), 3)
        net.close()
        return out
    if with_torch:
        model = torch_model(config, sd)
        mean = torch.tensor([0.485, 0.456, 0.406], device='cuda').view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225], device='cuda').view(1, 3, 1, 1)

        def torch_leg(autocast):
            @torch.no_grad()
            def run():
                with torch.autocast('cuda', dtype=torch.float16, enabled=autocast):
                    d = model(pixel_values=(img - mean) / std).predicted_depth.float()
                lo, hi = d.flatten(1).amin(1).view(-1, 1, 1), d.flatten(1).amax(1).view(-1, 1, 1)
                return (d - lo) / (hi - lo)
            return run
        legs['torch_fp32'], legs['torch_f16'] = torch_leg(False), torch_leg(True)
    med, best, worst = alternate(legs, reps)
    out.update(median_ms=med, min_ms=best, max_ms=worst)
    if with_torch:
        a, b = net(img)[:, 0], legs['torch_fp32']()
        torch.cuda.synchronize()
        out['rel_l2_vs_torch_fp32'] = float('%.3g' % ((a - b).norm() / b.norm()).item())
        out['vs_torch_fp32'] = round(med['torch_fp32'] / med['hip'], 2)
        out['vs_torch_f16'] = round(med['torch_f16'] / med['hip'], 2)
    out['mfma_tflops'] = round((out['gemm_gflop'] + out['attn_gflop'] + out['conv_gflop']) / med['hip'], 1)
    net.close()
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--configs', nargs='+', default=['small', 'base'], choices=sorted(CONFIGS))
    p.add_argument('--sizes', nargs='+', default=['518x910', '518x518'])
    p.add_argument('--no-torch', action='store_true')
    p.add_argument('--hip-only-once', action='store_true')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'depth_bench.json'))
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('depth_bench.py measures on the GPU; none is available')
    runs = []
    for name in a.configs:
        for s in a.sizes:
            h, w = (int(v) for v in s.split('x'))
            runs.append(bench(name, h, w, a.reps, not a.no_torch, a.hip_only_once))
    out = dict(metric='depth_estimator', reps=a.reps, device=torch.cuda.get_device_name(0), runs=runs)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
