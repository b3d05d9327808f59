#!/usr/bin/env python
"""Text/image -> image optimisation on MI355X: drop-in for the reference's clip_fft.py.

Same command line (every flag of the reference's get_args, clip_fft.py:37-77, with the same defaults,
post-parse overrides and sample-count derating arithmetic), same output naming and `.pt` snapshot
format.  Additive flags: --clip-weights PATH (OpenAI CLIP checkpoint; without it seeded synthetic
weights are used and the pictures are meaningless), --seed N (seeds torch + numpy; the reference is
unseeded), --no_save (skip the per-step JPEG, for timing).

The whole loss -- text / style / subtract prompts, a reference image, any --sim, --sharp, --enforce, --expand, --noise and
--aest (with --aest-weights: the LAION linear head cannot be downloaded here) -- runs through the fused HIP engine
(aphantasia_amd/engine.py), and so does --sync: the LPIPS (VGG-16) term against the -i image runs on HIP kernels of its own
(aphantasia_amd/lpips.py) inside the step; --vgg-weights / --lpips-weights name its two LOCAL weight files (torchvision's vgg16 state dict
and the lpips package's vgg.pth), without them seeded synthetic weights are used with a warning.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from aphantasia_amd import run                                                      # noqa: E402
from aphantasia_amd.run import FrameWriter, check_samples, pick_transform           # noqa: E402,F401  (bench.py, tools/exp and the tests take them from here)

clip_models = ['ViT-B/16', 'ViT-B/32', 'ViT-L/14', 'RN101', 'RN50x16', 'RN50x4', 'RN50']


def get_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('-t',  '--in_txt',  default=None, help='input text')
    parser.add_argument('-t2', '--in_txt2', default=None, help='input text - style')
    parser.add_argument('-t0', '--in_txt0', default=None, help='input text to subtract')
    parser.add_argument('-i',  '--in_img',  default=None, help='input image')
    parser.add_argument('-wi', '--weight_img', default=0.5, type=float, help='weight for images')
    parser.add_argument(       '--out_dir', default='_out')
    parser.add_argument('-s',  '--size',    default='1280-720', help='Output resolution')
    parser.add_argument('-r',  '--resume',  default=None, help='Path to saved FFT snapshots, to resume from')
    parser.add_argument('-ops', '--opt_step', default=1, type=int, help='How many optimizing steps per save step')
    parser.add_argument('-tr', '--translate', action='store_true', help='Translate text with Google Translate')
    parser.add_argument(       '--save_pt', action='store_true', help='Save FFT snapshots for further use')
    parser.add_argument('-v',  '--verbose',    dest='verbose', action='store_true')
    parser.add_argument('-nv', '--no-verbose', dest='verbose', action='store_false')
    parser.set_defaults(verbose=True)
    # training
    parser.add_argument('-m',  '--model',   default='ViT-B/32', choices=clip_models, help='Select CLIP model to use')
    parser.add_argument(       '--steps',   default=200, type=int, help='Total iterations')
    parser.add_argument(       '--samples', default=200, type=int, help='Samples to evaluate')
    parser.add_argument('-lr', '--lrate',   default=0.05, type=float, help='Learning rate')
    parser.add_argument('-p',  '--prog',    action='store_true', help='Enable progressive lrate growth (up to double a.lrate)')
    parser.add_argument('-dm', '--dualmod', default=None, type=int, help='Every this step use another CLIP ViT model')
    # wavelet
    parser.add_argument(       '--dwt',     action='store_true', help='Use DWT instead of FFT')
    parser.add_argument('-w',  '--wave',    default='coif2', help='wavelets: db[1..], coif[1..], haar, dmey')
    # tweaks
    parser.add_argument('-a',  '--align',   default='uniform', choices=['central', 'uniform', 'overscan', 'overmax'], help='Sampling distribution')
    parser.add_argument('-tf', '--transform', default='fast', choices=['none', 'fast', 'custom', 'elastic'], help='augmenting transforms')
    parser.add_argument('-opt', '--optimizer', default='adam_custom', choices=['adam', 'adamw', 'adam_custom', 'adamw_custom'], help='Optimizer')
    parser.add_argument(       '--contrast', default=1.1, type=float)
    parser.add_argument(       '--colors',  default=1.8, type=float)
    parser.add_argument(       '--decay',   default=1.5, type=float)
    parser.add_argument('-sh', '--sharp',   default=0., type=float)
    parser.add_argument('-mm', '--macro',   default=0.4, type=float, help='Endorse macro forms 0..1 ')
    parser.add_argument(       '--aest',    default=0., type=float, help='Enhance aesthetics')
    parser.add_argument('-e',  '--enforce', default=0, type=float, help='Enforce details (by boosting similarity between two parallel samples)')
    parser.add_argument('-x',  '--expand',  default=0, type=float, help='Boosts diversity (by enforcing difference between prev/next samples)')
    parser.add_argument('-n',  '--noise',   default=0, type=float, help='Add noise to suppress accumulation')
    parser.add_argument('-c',  '--sync',    default=0, type=float, help='Sync output to input image')
    parser.add_argument(       '--invert',  action='store_true', help='Invert criteria')
    parser.add_argument(       '--sim',     default='mix', help='Similarity function (dot/angular/spherical/mixed; None = cossim)')
    # additive (not in the reference)
    parser.add_argument(       '--clip-weights', dest='clip_weights', default=None, help='OpenAI CLIP checkpoint (ViT-B-32.pt); second model: --clip-weights2')
    parser.add_argument(       '--clip-weights2', dest='clip_weights2', default=None, help='checkpoint of the --dualmod model (ViT-B-16.pt)')
    parser.add_argument(       '--bpe-vocab', dest='bpe_vocab', default=None, help='BPE vocabulary of the text prompts (bpe_simple_vocab_16e6.txt.gz; default: beside the checkpoint)')
    parser.add_argument(       '--seed',    default=None, type=int, help='seed torch/numpy RNG (reference: unseeded)')
    parser.add_argument(       '--no_save', action='store_true', help='do not write the per-step JPEG frames')
    parser.add_argument(       '--precise', action='store_true', help='opt-in split-precision ViT forward (patch-embedding and QKV GEMMs on hi + lo f16 activation pairs): ~5 %% slower, lower single-step gradient error; '
                               'on the stress-weight loss-curve ensemble not significantly closer to the fp32 CPU reference than the default')
    parser.add_argument(       '--exact', action='store_true', help='opt-in fp32 ViT (f32-input MFMA GEMMs, fp32 attention / activations / gradient stream): '
                               'the reference\'s fp32 CPU numerics up to summation order; measured 26.3 steps/s at C2 (1280x720, 190 cuts, -tf fast) against ~160-174 for the default, i.e. ~6x the step time.  Exclusive with --precise')
    parser.add_argument(       '--fast-f16', action='store_true', help='(the default since round 6; accepted for old command lines) f16 operands on every ViT GEMM, as the reference runs CLIP on a GPU')
    parser.add_argument(       '--aest-weights', dest='aest_weights', default=None, help="state dict of the LAION aesthetic head (sa_0_4_vit_b_32_linear.pth: "
                               "{'weight': [1,512], 'bias': [1]}); upstream downloads it (utils.py:402-413), there is no network here")
    parser.add_argument(       '--aest-weights2', dest='aest_weights2', default=None, help='the head of the --dualmod model (sa_0_4_vit_b_16_linear.pth)')
    parser.add_argument(       '--vgg-weights', dest='vgg_weights', default=None, help='--sync: torchvision vgg16 state dict (features.N.weight / .bias), a local file; '
                               'upstream lets the lpips package download it, there is no network here')
    parser.add_argument(       '--lpips-weights', dest='lpips_weights', default=None, help="--sync: the lpips package's weights/v0.1/vgg.pth (linL.model.1.weight), a local file")
    parser.add_argument(       '--rng',     default=None, choices=['bulk', 'reference'], help="host random draws: 'reference' = the reference's exact draw "
                               "order on torch's / numpy's global generators (a seeded run reproduces the reference's crop and augment tables); "
                               "'bulk' = vectorised draws from a numpy Generator (same distributions, a different stream, ~10x less host time). "
                               "Default: reference when --seed is given, else bulk")
    parser.add_argument(       '--ranks',   default=1, type=int, help='GPUs of this node to shard the cuts over (launch with torchrun, or let this flag spawn the ranks)')
    parser.add_argument(       '--graph-allreduce', action='store_true', help='with --ranks N: capture the whole step INCLUDING its RCCL all-reduce into one hipGraph '
                               '(opt-in: multi-rank steps launch eagerly by default; same as APH_MULTIRANK_GRAPH=1)')
    parser.add_argument(       '--no-graph', action='store_true', help='eager launches instead of hipGraph replay (debugging)')
    a = parser.parse_args(argv)
    if a.exact and a.precise:
        parser.error('--exact and --precise are mutually exclusive (the exact path is fp32 end to end)')

    if a.size is not None: a.size = [int(s) for s in a.size.split('-')][::-1]        # clip_fft.py:80
    if len(a.size) == 1: a.size = a.size * 2
    if (a.in_img is not None and a.sync != 0) or a.resume is not None: a.align = 'overscan'
    if a.translate is True:
        print('\n Install googletrans module to enable translation!'); exit()
    if a.dualmod is not None:                                                         # clip_fft.py:86-88
        a.model = 'ViT-B/32'
        a.sim = 'cossim'
    if a.rng is None:
        a.rng = 'reference' if a.seed is not None else 'bulk'
    return a


def derate_samples(a):
    """The reference's sample-count arithmetic, in its order (clip_fft.py:125-127,134,157-169,187,199)."""
    xmem = {'ViT-B/16': 0.25, 'ViT-L/14': 0.04, 'RN50': 0.5, 'RN50x4': 0.16, 'RN50x16': 0.06, 'RN101': 0.33}      # (ViT-L/14: illustra.py:97, the same generator)
    s = a.samples
    if a.model in xmem:
        s = int(s * xmem[a.model])
    if a.dualmod is not None:
        s = int(s * 0.23)
    if a.enforce != 0:
        s = int(s * 0.5)
    if a.sync > 0:
        s = int(s * 0.5)
    if a.transform in ('elastic', 'custom', 'fast'):
        s = int(s * 0.95)
    if a.in_txt2 is not None:
        s = int(s * 0.75)
    if a.in_txt0 is not None:
        s = int(s * 0.75)
    return s


def prog_sync(i, n):
    """the --sync term's decay over the run (clip_fft.py:269): (N - i) / N with N = steps // opt_step"""
    return (n - i) / n


def main(argv=None):
    a = get_args(argv)
    ranks = run.bootstrap_ranks(a, argv, main, 'r', verbose=False, no_save=True, save_pt=False)      # (--ranks N: the ranks were spawned and have run)
    if ranks is None:
        return
    rank, world, comm = ranks
    run.seed_all(a.seed)
    if not a.model.startswith('ViT'):
        raise SystemExit(' the MI355X path covers the ViT CLIP models (ViT-B/32, ViT-B/16, ViT-L/14); got %s' % a.model)
    from aphantasia_amd import clip as aclip
    from aphantasia_amd.image import to_valid_rgb, fft_image, dwt_image
    from aphantasia_amd.utils import basename, txt_clean
    from aphantasia_amd.engine import Engine

    shape = [1, 3, *a.size]
    if a.dwt is True:
        params, image_f, sz = dwt_image(shape, a.wave, 0.3, a.colors, a.resume)
    else:
        params, image_f, sz = fft_image(shape, 0.07, a.decay, a.resume)
    if sz is not None: a.size = sz
    rgb_f = to_valid_rgb(image_f, colors=a.colors)

    if a.prog is True:
        lr1 = a.lrate * 2
        lr0 = lr1 * 0.01
    else:
        lr0 = a.lrate
    sign = 1. if a.invert is True else -1.

    model_clip, model_clip2 = run.load_models(a.model, a.clip_weights, 'ViT-B/16' if a.dualmod is not None else None, a.clip_weights2)
    a.modsize = model_clip.visual.input_resolution
    if a.verbose is True: print(' using model', a.model)
    a.samples = derate_samples(a)
    check_samples(a.samples)
    if a.dualmod is not None:
        print(' dual model every %d step' % a.dualmod)

    def enc_text(txt, model=model_clip):                                              # clip_fft.py:143-154
        return [(aclip.text_embedding(model, subtxt, bpe_vocab=a.bpe_vocab), wt) for subtxt, wt in run.split_prompt(txt)]

    trform_f = pick_transform(a.transform)
    out_name = []
    targets, targets2 = [], []          # (embedding, coef) for model 1 / model 2
    img_in = None
    if a.in_txt is not None:
        if a.verbose is True: print(' topic text: ', a.in_txt)
        targets += [(e, sign * w) for e, w in enc_text(a.in_txt)]
        out_name.append(txt_clean(a.in_txt).lower()[:40])
        if a.dualmod is not None: targets2 += [(e, sign * w) for e, w in enc_text(a.in_txt, model_clip2)]
    if a.in_txt2 is not None:
        if a.verbose is True: print(' style text:', a.in_txt2)
        targets += [(e, sign * w) for e, w in enc_text(a.in_txt2)]
        out_name.append(txt_clean(a.in_txt2).lower()[:40])
        if a.dualmod is not None: targets2 += [(e, sign * w) for e, w in enc_text(a.in_txt2, model_clip2)]
    if a.in_txt0 is not None:
        if a.verbose is True: print(' subtract text:', a.in_txt0)
        targets += [(e, -sign * w) for e, w in enc_text(a.in_txt0)]
        out_name.append('off-' + txt_clean(a.in_txt0).lower()[:40])
        if a.dualmod is not None: targets2 += [(e, -sign * w) for e, w in enc_text(a.in_txt0, model_clip2)]
    if a.in_img is not None and os.path.isfile(a.in_img):
        if a.verbose is True: print(' ref image:', basename(a.in_img))
        img_in, rows = run.image_target_rows(a.in_img, [m for m in (model_clip, model_clip2) if m is not None], a.samples, a.modsize, a.align)
        for t, r in zip((targets, targets2), rows): t.append((r, sign * a.weight_img))                  # per-cut pairs, clip_fft.py:216,267
        out_name.append(basename(a.in_img).replace(' ', '_'))
    assert targets, ' Loss not defined, check the inputs'                              # clip_fft.py:286
    aclip.release_text(model_clip, model_clip2)     # the targets are built: the text arenas can go

    if a.verbose is True: print(' samples:', a.samples)
    out_name = '-'.join(out_name)
    out_name += '-%s' % a.model.replace('/', '').replace('-', '') if a.dualmod is None else '-dm%d' % a.dualmod
    tempdir = os.path.join(a.out_dir, out_name)
    os.makedirs(tempdir, exist_ok=True)

    aest1 = run.load_aest(a.aest_weights, a.aest)
    aest2 = run.load_aest(a.aest_weights2, a.aest) if a.dualmod is not None else None
    run.check_aest(aest1, model_clip, '--aest-weights')
    if a.dualmod is not None: run.check_aest(aest2, model_clip2, '--aest-weights2')
    h, w = a.size
    if a.dwt is True:
        pk = dict(param_kind='dwt', dwt=image_f.synth)
        leaf = image_f.flat
        h, w = image_f.synth.H, image_f.synth.W
    else:
        pk = dict(param_kind='fft')
        leaf = params[0]
    # --sync (clip_fft.py:219-222, 268-270): LPIPS between the half-size image and the half-size -i image, inside the fused step
    sync = None
    if a.sync > 0:
        if img_in is None:
            print(' --sync: no readable -i image, the term is off (as upstream, clip_fft.py:268)')
        else:
            from aphantasia_amd import lpips as alpips
            sync = alpips.load(h, w, a.vgg_weights, a.lpips_weights, device='cuda')
            sync.set_target(F.interpolate(img_in, [h // 2, w // 2], mode='bicubic', align_corners=True).float())
            if a.verbose is True: print(' sync: LPIPS (VGG-16) on %d x %d, arena %.0f MB' % (h // 2, w // 2, sync.workspace_bytes() / 2 ** 20))
    pk['sync'] = sync
    n_sync = max(a.steps // a.opt_step, 1)
    eng = Engine(leaf, h, w, model_clip, a.samples, targets, sim=a.sim, colors=a.colors, decay=a.decay, lr=lr0,
                 optimizer=a.optimizer, align=a.align, macro=a.macro, transform=trform_f, sharp=a.sharp, expand=a.expand, enforce=a.enforce, rng=a.rng,
                 rank=rank, world=world, comm=comm, aest=aest1, precise=a.precise, exact=a.exact, graph_allreduce=a.graph_allreduce or None, use_graph=not a.no_graph, **pk)
    h, w = eng.h, eng.w
    eng2 = None
    if a.dualmod is not None:
        eng2 = Engine(leaf, h, w, model_clip2, a.samples, targets2, sim=a.sim, colors=a.colors, decay=a.decay, lr=lr0,
                      optimizer=a.optimizer, align=a.align, macro=a.macro, transform=trform_f, state=eng.state(), sharp=a.sharp, expand=a.expand, enforce=a.enforce, rng=a.rng,
                      rank=rank, world=world, comm=comm, aest=aest2, precise=a.precise, exact=a.exact, graph_allreduce=a.graph_allreduce or None, use_graph=not a.no_graph, **pk)

    writer = None if a.no_save else FrameWriter(h, w)
    # empirical tone mapping of the saved frames (clip_fft.py:300-303): **1.3 with --sync, **(1 + sharp/2) with --sharp
    gamma = 1.3 if (a.sync > 0 and a.in_img is not None) else (1 + a.sharp / 2. if a.sharp != 0 else 1.0)
    prog = run.Progress(a.steps, 'step', a.verbose, world)
    for i in range(a.steps):
        e = eng2 if run.is_dual_step(i, a.dualmod) else eng
        lr_cur = lr0 + (i / a.steps) * (lr1 - lr0) if a.prog is True else lr0      # clip_fft.py:288-291
        shift = None
        if a.noise > 0 and a.dwt is not True:
            shift = (a.noise * torch.rand(1, 1, h, w // 2 + 1, 1)).reshape(h, w // 2 + 1).cuda().contiguous()
        e.step(lr=lr_cur, shift=shift, sync_weight=prog_sync(i, n_sync) * a.sync if sync is not None else None)
        if a.expand > 0:                                                                # clip_fft.py:276-280: prev_enc = out_enc.detach()
            for other in (eng, eng2):
                if other is not None: other.set_prev_enc(e.enc)
        if i % a.opt_step == 0 and writer is not None:
            img = e.synthesize(a.contrast)                                              # clip_fft.py:298-299
            writer.put(img.reshape(3, h, w), os.path.join(tempdir, '%04d.jpg' % (i // a.opt_step)), gamma)
        prog.tick(i, e)
    torch.cuda.synchronize()
    if writer is not None:
        run.finish_frames(writer, tempdir, '%04d', os.path.join(a.out_dir, out_name), os.path.join(a.out_dir, '%s-%d.jpg' % (out_name, a.steps)))
    if a.save_pt is True:
        torch.save([p.detach().cpu() for p in params], '%s.pt' % os.path.join(a.out_dir, out_name))   # clip_fft.py:315 (list of tensors)
    if rank == 0:
        prog.done()


if __name__ == '__main__':
    main()
