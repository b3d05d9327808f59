"""What clip_fft.py, illustrip.py and cppn.py share on the host: seeding, the multi-rank bootstrap, model / aesthetic-head loading, the
prompt grammar, the reference-image target, the progress lines, the frame writer and the end of a run.  One copy of each; the scripts keep
their flags, their sample-count derating and a main() that reads top to bottom."""
import os
import queue
import shutil
import sys
import threading
import time
import warnings

import numpy as np
import torch


def pick_transform(name):
    """-tf none | fast | custom | elastic (clip_fft.py:121-128 upstream) -> the Engine's `transform` argument"""
    from aphantasia_amd import transforms
    return {'fast': transforms.transforms_fast, 'custom': transforms.transforms_custom, 'elastic': transforms.transforms_elastic}.get(name) or transforms.normalize()


def check_samples(n):
    """upstream, `--samples 1` with the default `-tf fast` derates to int(1 * 0.95) = 0 cuts and dies in torch.cat([])
    (clip_fft.py:169, utils.py:253); say so instead"""
    if n < 1:
        raise SystemExit(' --samples derates to %d cuts for this model / transform (clip_fft.py:125-169): nothing to optimise; '
                         'raise --samples or use -tf none' % n)


def seed_all(seed):
    if seed is not None:
        torch.manual_seed(seed)
        np.random.seed(seed)


def is_dual_step(i, dm):
    """-dm N: the steps list(range(steps))[N::N] of upstream (clip_fft.py:134,243) run the second model"""
    return dm is not None and i >= dm and i % dm == 0


def _rank_entry(local_rank, main, argv, world, port, run_id):
    os.environ.update(RANK=str(local_rank), LOCAL_RANK=str(local_rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port), APH_RUN_ID=run_id, HSA_ENABLE_IPC_MODE_LEGACY='0')
    main(argv)


def bootstrap_ranks(a, argv, main, prefix, **quiet):
    """Multi-GPU (the reference is single-GPU): the cuts are split over the ranks of one node, one process per GPU,
    ONE RCCL all-reduce of the parameter gradient per step (aph_allreduce_f32).  Either launched by torchrun (RANK / WORLD_SIZE /
    LOCAL_RANK in the environment) or spawned from here with --ranks N: then `main(argv)` has run in every rank and None is returned.
    Otherwise -> (rank, world, comm); on a non-zero rank the fields of `quiet` are set on `a` (rank 0 reports and writes the files)."""
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    if a.ranks > 1 and 'RANK' not in os.environ:
        from aphantasia_amd import comm as acomm
        argv = list(sys.argv[1:] if argv is None else argv)
        if a.seed is None:
            argv += ['--seed', str(int.from_bytes(os.urandom(3), 'little'))]          # every rank must draw the same crop tables
        port = 20000 + int.from_bytes(os.urandom(2), 'little') % 20000
        acomm.spawn_ranks(_rank_entry, (main, argv, a.ranks, port, '%s%d' % (prefix, os.getpid())), a.ranks)
        return None
    comm = None
    if world > 1:
        if a.seed is None:
            raise SystemExit(' multi-rank runs need --seed (every rank draws the same crop / augment tables and takes its share of the cuts)')
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', rank)))
        from aphantasia_amd import comm as acomm
        comm = acomm.create(rank, world)
        if rank != 0:
            vars(a).update(quiet)
    return rank, world, comm


def load_models(name, weights, second=None, weights2=None):
    """-> (model, second model or None); without a checkpoint the weights are synthetic: one line here instead of a warning per model"""
    from aphantasia_amd import clip as aclip
    with warnings.catch_warnings():
        if weights is None:
            print(' !! no --clip-weights given: using seeded SYNTHETIC CLIP weights (timing / plumbing only)')
            warnings.simplefilter('ignore')
        model = aclip.load(name, weights=weights)[0]
        return model, (aclip.load(second, weights=weights2)[0] if second is not None else None)


def split_prompt(txt):
    """'a|b:0.5' -> [('a', 1.0), ('b', 0.5)] (clip_fft.py:145-149, illustrip.py:186-190 upstream; a part with two colons raises there too)"""
    parts = []
    for sub in txt.split('|'):
        wt = 1.
        if ':' in sub:
            sub, wt = sub.split(':')
        parts.append((sub, float(wt)))
    return parts


def load_aest(path, strength):
    """--aest: utils.py:402-413 aesthetic_model() -> (weight, bias, strength) for the Engine, or None"""
    if strength == 0:
        return None
    if path is None or not os.path.isfile(path):
        raise SystemExit(' --aest needs the LAION linear head: pass its state dict with --aest-weights (upstream downloads '
                         'sa_0_4_<model>_linear.pth from github.com/LAION-AI/aesthetic-predictor; there is no network here)')
    sd = torch.load(path, map_location='cpu')
    return (sd['weight'].float(), float(sd['bias'].reshape(-1)[0]), strength)


def check_aest(head, model, flag):
    """utils.py:403: nf = 768 for ViT-L/14, 512 for ViT-B/*"""
    if head is not None and head[0].numel() != model.visual.output_dim:
        raise SystemExit(' %s: a head of %d inputs, but %s encodes into %d (sa_0_4_vit_l_14_linear.pth is the 768-wide one)'
                         % (flag, head[0].numel(), model.name, model.visual.output_dim))


def image_target_rows(path, models, samples, modsize, align):
    """-i IMG -> (the image [1,3,H,W] on the device, its per-cut embedding under each model: clip_fft.py:216,267).  ONE slice_imgs (it
    draws from the global generators) serves every model."""
    from aphantasia_amd import transforms
    from aphantasia_amd.utils import slice_imgs, img_read
    img_in = torch.from_numpy(img_read(path) / 255.).unsqueeze(0).permute(0, 3, 1, 2).cuda().float()[:, :3]
    with torch.no_grad():
        in_sliced = slice_imgs([img_in], samples, modsize, transforms.normalize(), align, patch=models[0].visual.patch_size)[0]
        return img_in, [m.encode_image(in_sliced).detach().clone() for m in models]


class Progress:
    """The loop's clock and its report: a line every tenth step and at the last one, the `done:` line at the end"""

    def __init__(self, n, unit, verbose, world=1):
        self.n, self.unit, self.verbose, self.world = n, unit, verbose, world
        self.t0 = time.time()

    def due(self, i):
        return i % 10 == 9 or i == self.n - 1

    def tick(self, i, eng):
        if (self.verbose or self.world > 1) and self.due(i):
            gl = eng.global_loss()             # (a collective when world > 1: every rank takes part, the verbose one prints)
            if self.verbose:
                print(' %s %d/%d  loss %.4f  %.1f %ss/s' % (self.unit, i + 1, self.n, gl, (i + 1) / (time.time() - self.t0), self.unit), flush=True)

    def done(self):
        dt = time.time() - self.t0
        print(' done: %d %ss in %.1fs (%.1f %ss/s)%s' % (self.n, self.unit, dt, self.n / dt, self.unit, ' on %d ranks' % self.world if self.world > 1 else ''))


def finish_frames(writer, tempdir, pattern, video_path, last_copy=None):
    """every frame on disk, the video if ffmpeg is there, the last frame copied to `last_copy`"""
    from aphantasia_amd.utils import img_list
    writer.close()
    if shutil.which('ffmpeg'):
        os.system('ffmpeg -v warning -y -i %s/\\%s.jpg "%s.mp4"' % (tempdir, pattern, video_path))
    frames = img_list(tempdir) if last_copy is not None else []
    if frames:
        shutil.copy(frames[-1], last_copy)


class FrameWriter:
    """Background JPEG writers: the reference converts and encodes every frame synchronously inside the hot loop
    (clip_fft.py:297-306, utils.py:94-100).  Here the loop only enqueues a device-side uint8 conversion and an async
    copy into a pinned ring; a small thread pool waits for the copy event and encodes (PIL releases the GIL)."""
    THREADS = 4        # (8 threads measured the same with-save rate: 153.6-154.0 vs 153.2 steps/s -- the encoders are not the limit)
    RING = 16          # slots of (device uint8 buffer, pinned host buffer); a slot is reused only after its writer released it (below)

    def __init__(self, h, w, switch_interval=None):
        # switch_interval: optionally lower the interpreter's GIL switch interval (default 5 ms) for the encoder threads' sake.  Measured in
        # round 6 (tools/exp/save_ab.py, profiles/r06_save_ab.txt): 158.7 / 158.6 / 158.7 steps/s at 5 / 0.5 / 0.1 ms against 163.8 without
        # saving -- the 3 % the per-step frame costs is device work (the contrast-1.1 synthesis, the uint8 conversion, the copy) and the
        # loop's own enqueue calls, not GIL hand-over; left at the interpreter's setting.
        if switch_interval is not None and sys.getswitchinterval() > switch_interval:
            sys.setswitchinterval(switch_interval)
        self.q = queue.Queue(maxsize=8)
        self.h, self.w = h, w
        self.bufs = [torch.empty(h, w, 3, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
        # device-side uint8 ring + a copy stream of its own: the conversion is ONE launch on the step's stream (aph_rgb_to_u8), the
        # 2.7 MB device->host copy waits for it on the side stream, so the next step's launches do not queue behind the PCIe transfer
        self.dev = None
        self.copy_stream = None
        self.n = 0
        # slot discipline: `free[k]` is released by the worker AFTER imsave (a straggling encoder keeps its pinned buffer), and the copy
        # event of the slot's previous use is waited for on the step's stream before aph_rgb_to_u8 rewrites the device buffer
        self.free = [threading.Semaphore(1) for _ in range(self.RING)]
        self.copy_ev = [None] * self.RING
        self.ts = [threading.Thread(target=self._run, daemon=True) for _ in range(self.THREADS)]
        for t in self.ts: t.start()

    def _run(self):
        from PIL import Image
        while True:
            item = self.q.get()
            if item is None:
                self.q.task_done()
                return
            buf, ev, fname, k = item
            try:
                ev.synchronize()
                Image.fromarray(buf.numpy()).save(fname, quality=95)
            finally:
                self.free[k].release()
                self.q.task_done()

    def put(self, img, fname, gamma=1.0):
        """img: device float32 [3,H,W] in [0,1]; same arithmetic as utils.checkout: clip(img ** gamma * 255, 0, 255).astype(uint8)"""
        from aphantasia_amd import _ffi, ops
        if self.dev is None:
            self.dev = [torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=img.device) for _ in range(self.RING)]
            self.copy_stream = torch.cuda.Stream(device=img.device)
        k = self.n % self.RING
        self.n += 1
        buf, dbuf = self.bufs[k], self.dev[k]
        img = img.contiguous()
        self.free[k].acquire()                                        # the encoder that used this slot RING frames ago has written its file
        if self.copy_ev[k] is not None:
            torch.cuda.current_stream(img.device).wait_event(self.copy_ev[k])      # ... and its device->host copy has read dbuf
        _ffi.lib().call('aph_rgb_to_u8', ops.ptr(img), self.h, self.w, float(gamma), ops.ptr(dbuf), ops._stream(img))
        done = torch.cuda.Event(); done.record()                      # on the step's stream: the conversion has read `img`
        self.copy_stream.wait_event(done)
        with torch.cuda.stream(self.copy_stream):
            buf.copy_(dbuf, non_blocking=True)
            ev = torch.cuda.Event(); ev.record()
        self.copy_ev[k] = ev
        self.q.put((buf, ev, fname, k))

    def drain(self):
        """block until every frame handed to put() is on disk"""
        self.q.join()

    def close(self):
        for _ in self.ts: self.q.put(None)
        for t in self.ts: t.join()
