"""Exact (fp32) ViT mode at bench.py's `value` configuration: 1280x720 FFT image, ViT-B/32 (seeded synthetic weights), 190 cuts,
-tf fast, graph replay -- Engine(exact=True).  Prints ONE JSON line: steps/s, ms/step, and the GEMM family's achieved TF/s from
aph_vit_profile (eager steps, a HIP event pair around every GEMM launch) against the 157.3 TF f32-input MFMA peak.

    python tools/exact_bench.py [--steps 50] [--warmup 10] [--samples 190]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aphantasia_amd import clip as aclip, transforms  # noqa: E402
from aphantasia_amd.engine import Engine  # noqa: E402

PEAK_F32_TF = 157.3          # v_mfma_f32_32x32x2_f32: 64 FLOP / clock / SIMD x 1024 SIMDs x 2.4 GHz


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=50)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--samples', type=int, default=190)
    p.add_argument('--profile-steps', type=int, default=5)
    a = p.parse_args(argv)
    h, w, S = 720, 1280, a.samples
    torch.manual_seed(0)
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, _ = aclip.load('ViT-B/32', seed=1, max_batch=S, exact=True)
    leaf = (0.01 * torch.randn(1, 3, h, w // 2 + 1, 2)).cuda().contiguous()
    target = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))
    eng = Engine(leaf, h, w, model, S, [(target, -1.0)], sim='mix', transform=transforms.transforms_fast, exact=True)
    for _ in range(a.warmup):
        loss = eng.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = eng.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    loss = float(loss)
    lib, v = eng.lib, eng.visual.handle
    eng.use_graph = False
    lib.call('aph_vit_profile', v.handle, 1)
    for _ in range(a.profile_steps):
        eng.step()
    torch.cuda.synchronize()
    ms, n, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
    lib.call('aph_vit_profile_read', v.handle, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
    lib.call('aph_vit_profile', v.handle, 0)
    tf = fl.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0
    out = dict(metric='exact_mode_c2', config=dict(h=h, w=w, model='ViT-B/32', samples=S, transform='fast', graph=True),
               steps=a.steps, warmup=a.warmup, steps_per_s=round(1.0 / dt, 3), ms_per_step=round(dt * 1e3, 3), loss=loss,
               skipped_steps=int(eng.guard[0]),
               gemm=dict(launches_per_step=n.value // max(a.profile_steps, 1), ms_per_step=round(ms.value / a.profile_steps, 3),
                         tflop_per_step=round(fl.value / a.profile_steps / 1e12, 4), achieved_tf=round(tf, 2), peak_tf=PEAK_F32_TF,
                         frac_of_peak=round(tf / PEAK_F32_TF, 4)))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
