"""ViT-L/14 (T = 257 attention, 14-pixel patches, width 1024) measured: writes profiles/vitl14.txt (or --out).

  steps      steps/s of the fused engine at 1280x720, -tf fast, graph replay, at the CLI's own cut count (7) and at 47 and 190 cuts
  attention  per-launch time of the T = 257 forward / backward (five 64-token blocks) next to the four-block kernels at T = 256, alternating
             runs, the same S x heads.  (The four-block instantiations are the parent commit's, instruction for instruction.)
             Structural expectation: 5/4 on key blocks x 17/16 on query tiles = 1.33.
  gemm       per-shape time of the width-1024 GEMMs at M = 47 cuts x 257 tokens (the method of tools/gemm_shapes_bench.py, automatic routing)
  errors     one full-depth (24 layers) step at S = 1: embedding max-rel and input-gradient max-rel against the fp32 CPU restatement
             (oracle/clip_vit_ref.encode_image) -- the figure tests/test_gpu_vitl.py gates at twice its value

    python tools/vitl_bench.py [--out profiles/vitl14.txt] [--only steps,attention,gemm,errors] [--steps 10]
"""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aphantasia_amd import _ffi, clip as aclip, ops, transforms  # noqa: E402
from aphantasia_amd.engine import Engine  # noqa: E402
from aphantasia_amd.weights import synthetic_visual_weights, visual_config  # noqa: E402

NAME = 'ViT-L/14'


def timed(f, reps, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch


def bench_steps(say, steps, cuts=(7, 47, 190)):
    h, w = 720, 1280
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, _ = aclip.load(NAME, seed=1, max_batch=max(cuts))
    say('arena: %.2f GB for weights and %d cuts (aph_vit_workspace_bytes)' % (model.visual.handle.workspace_bytes() / 2 ** 30, max(cuts)))
    for S in cuts:
        torch.manual_seed(0)
        np.random.seed(0)
        leaf = (0.01 * torch.randn(1, 3, h, w // 2 + 1, 2)).cuda().contiguous()
        target = torch.randn(1, 768, generator=torch.Generator().manual_seed(2))
        eng = Engine(leaf, h, w, model, S, [(target, -1.0)], sim='mix', transform=transforms.transforms_fast)
        for _ in range(4):
            loss = eng.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = eng.step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        say('steps  1280x720 -tf fast %3d cuts: %8.3f steps/s  %8.2f ms/step  (graph %s, loss %.4f, skipped %d)'
            % (S, 1.0 / dt, dt * 1e3, eng._graph is not None, float(loss), int(eng.guard[0])))
        del eng
    del model
    torch.cuda.empty_cache()


def bench_attention(say, heads=16):
    L = _ffi.lib()
    for S in (7, 47):
        bufs = {}
        for T in (256, 257):
            D, M = heads * 64, S * T
            g = torch.Generator().manual_seed(T)
            qkv = (torch.randn(M, 3 * D, generator=g) * 1.5).half().cuda()
            datt = torch.randn(M, D, generator=g).half().cuda()
            bufs[T] = (qkv, datt, torch.empty(M, D, dtype=torch.float16, device='cuda'), torch.empty(S * heads * T, device='cuda'),
                       torch.empty(M, 3 * D, dtype=torch.float16, device='cuda'))

        def call(T, mode):
            qkv, datt, att, lse, dq = bufs[T]
            L.call('aph_attn_test', ops.ptr(qkv), ops.ptr(att), ops.ptr(lse), ops.ptr(datt), None, ops.ptr(dq), S, T, heads, mode, ops._stream(qkv))
        res = {(T, m): [] for T in (256, 257) for m in (0, 1)}
        for _ in range(3):                      # alternating runs
            for T in (256, 257):
                for m in (0, 1):
                    res[(T, m)].append(timed(lambda: call(T, m), 30))
        med = {k: sorted(v)[1] for k, v in res.items()}
        for m, nm in ((0, 'forward '), (1, 'backward')):
            say('attention %s S x heads = %4d: T=256 (4 blocks) %8.1f us   T=257 (5 blocks) %8.1f us   ratio %.2f   (runs: %s | %s)'
                % (nm, S * heads, med[(256, m)], med[(257, m)], med[(257, m)] / med[(256, m)],
                   ' '.join('%.1f' % v for v in res[(256, m)]), ' '.join('%.1f' % v for v in res[(257, m)])))


def bench_gemm(say, cuts=47, D=1024):
    L = _ffi.lib()
    M, Mp = cuts * 257, cuts * 256
    shapes = [('patch-embed', Mp, D, 640), ('qkv', M, 3 * D, D), ('outproj/dout', M, D, D), ('fc1/dfc2', M, 4 * D, D), ('fc2/dfc1', M, D, 4 * D),
              ('dqkv', M, D, 3 * D), ('patch dgrad', Mp, 640, D)]
    for name, M_, N, K in shapes:
        A = torch.randn(M_, K, device='cuda').half()
        B = torch.randn(N, K, device='cuda').half()
        C = torch.empty(M_, N, device='cuda')
        us = timed(lambda: L.call('aph_gemm_f16_ld', ops.ptr(A), K, ops.ptr(B), K, M_, N, K, ops.ptr(C), 0, ops._stream(A)), 20)
        say('gemm   %-13s %6d x %5d x %5d : %8.1f us  %6.0f TF/s' % (name, M_, N, K, us, 2.0 * M_ * N * K / us / 1e6))


def full_depth_errors(seed=3, S=1):
    """-> (embedding max-rel, input-gradient max-rel) of one 24-layer forward + backward against the fp32 CPU restatement"""
    from oracle import clip_vit_ref
    cfg = visual_config(NAME)
    w = synthetic_visual_weights(cfg, seed)
    R, p = cfg['input_resolution'], cfg['patch_size']
    x = torch.randn(S, 3, R, R, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    want = clip_vit_ref.encode_image(w, x, cfg)
    genc = torch.randn(S, cfg['output_dim'], generator=torch.Generator().manual_seed(2)) * 0.01
    (want * genc).sum().backward()
    vit = ops.VitHandle(cfg, w, max_batch=S)
    enc = vit.forward(ops.patchify(x.detach().cuda().contiguous(), p), S)
    LS = 1024.0
    gp = vit.backward((genc * LS).cuda().contiguous(), S, out_scale=1.0 / LS)
    gx = ops.unpatchify(gp, S, R, p)
    ferr = (enc.cpu() - want.detach()).abs().max().item() / want.abs().max().item()
    berr = (gx.cpu() - x.grad).abs().max().item() / x.grad.abs().max().item()
    return ferr, berr


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vitl14.txt'))
    ap.add_argument('--only', default='errors,attention,gemm,steps')
    ap.add_argument('--steps', type=int, default=10)
    a = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, 'w') as f:              # rewritten after every line: a partial run leaves what it measured
            f.write('\n'.join(lines) + '\n')
    say('tools/vitl_bench.py on %s (%s)' % (torch.cuda.get_device_name(0), ' '.join(sys.argv[1:]) or 'defaults'))
    only = a.only.split(',')
    if 'errors' in only:
        ferr, berr = full_depth_errors()
        say('errors full depth (24 layers, S = 1, synthetic weights seed 3) vs fp32 CPU: embedding max-rel %.3e  input-gradient max-rel %.3e' % (ferr, berr))
    if 'attention' in only:
        bench_attention(say)
    if 'gemm' in only:
        bench_gemm(say)
    if 'steps' in only:
        bench_steps(say, a.steps)


if __name__ == '__main__':
    main()
