"""Per-level time of the inverse DWT and its adjoint (default: C4's size, 3840x2160 db3, 11 levels), HIP events around each C-ABI call.
    python tools/exp/dwt_levels.py [h w [wavelet]]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aphantasia_amd import ops
from aphantasia_amd.dwt import DWTSynth
h, w = (int(v) for v in (sys.argv[1:3] if len(sys.argv) > 2 else (2160, 3840)))
syn = DWTSynth(h, w, sys.argv[3] if len(sys.argv) > 3 else 'db3', 0.3, 'cuda')
flat = torch.randn(syn.numel, device='cuda') * 0.01
grad = torch.empty_like(flat)
graw = torch.randn(3, syn.H, syn.W, device='cuda')
def timeit(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
print('all levels: forward %.1f us, adjoint %.1f us' % (timeit(lambda: syn.forward(flat)), timeit(lambda: syn.backward(graw, grad))))
ys = syn.views(flat); gs = syn.views(grad)
st = ops._stream(flat)
def level_us(call, tensors, lev):
    """(j, band size, output size, us, TB/s, MB) of one per-level call"""
    (hh, ww), (ho, wo) = lev[1], syn.out_sizes[lev[0]]
    by = 4.0 * 3 * (4 * hh * ww + ho * wo)
    us = timeit(lambda: call(tensors, *lev, st))
    return lev[0], hh, ww, ho, wo, us, by / us / 1e6, by / 1e6
for lev in reversed(list(syn.levels(ys[0], syn.bufs))):
    print('fwd level %2d: in %4dx%4d -> out %4dx%4d  %7.1f us  %6.2f TB/s (%.1f MB)' % level_us(syn.level_fwd, ys, lev))
for lev in syn.levels(gs[0], [graw] + syn.gbufs[1:]):
    j, _, _, _, _, us, tbs, mb = level_us(syn.level_bwd, gs, lev)
    print('adj level %2d: %7.1f us  %6.2f TB/s (%.1f MB)' % (j, us, tbs, mb))
