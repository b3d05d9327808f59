"""The CLIP text tower's run time and arena size on one GPU: one prompt and a full batch through aph_text_forward at the ViT-B/32 and ViT-L/14
text configurations, synthetic weights; median of 30 event-timed launches after 5 warm-ups (profiles/text_tower.txt).  Not on the hot path: the
tower runs once per prompt."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aphantasia_amd import ops                                    # noqa: E402
from aphantasia_amd.weights import synthetic_text_weights         # noqa: E402

CONFIGS = {'B/32': dict(context_length=77, vocab_size=49408, width=512, layers=12, heads=8, output_dim=512),
           'L/14': dict(context_length=77, vocab_size=49408, width=768, layers=12, heads=12, output_dim=768)}
MAX_BATCH = 16

if __name__ == '__main__':
    for name, cfg in CONFIGS.items():
        th = ops.TextHandle(cfg, synthetic_text_weights(cfg, 4), max_batch=MAX_BATCH)
        for S in (1, MAX_BATCH):
            tok = torch.zeros(S, 77, dtype=torch.int32)
            tok[:, 0], tok[:, 1:20], tok[:, 20] = cfg['vocab_size'] - 2, 1000, cfg['vocab_size'] - 1
            tok = tok.cuda()
            out = torch.empty(S, cfg['output_dim'], device='cuda')
            for _ in range(5):
                th.forward(tok, out)
            torch.cuda.synchronize()
            ts = []
            for _ in range(30):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                th.forward(tok, out)
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            print('%s text tower, S = %d (arena for %d prompts: %.3f GB): median %.3f ms, min %.3f, max %.3f over 30 launches'
                  % (name, S, MAX_BATCH, th.workspace_bytes() / 2 ** 30, statistics.median(ts), min(ts), max(ts)), flush=True)
        th.close()
