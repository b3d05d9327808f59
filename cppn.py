#!/usr/bin/env python
"""Text/image -> CPPN image optimisation on MI355X: drop-in for the reference's cppn.py.

The image is a coordinate network of 1x1 convolutions (cppn.py:71-116) whose weights are optimised against CLIP.  Same flags and defaults as
the reference's get_args (cppn.py:33-68), the same sample-count derating, loss (plain cosine similarity: -1 text, +0.5 `-t0`, -1 reference
image; `--aest`), optimiser (Adam, lr 0.003), per-`fstep` JPEG and `.npy` snapshot (the reference's list format: `--resume` reads its
snapshots).  Generator, sampler, ViT, loss and Adam run as one fused step (aphantasia_amd/engine.py, param_kind='cppn').

Additive flags, with the meaning they have in clip_fft.py: --clip-weights[2], --aest-weights[2], --seed, --rng, --no_save, --no-graph, --exact.
Refused with a message: -sh (the Sobel derivative is not built), -ex (shader export is not part of this path), the RN* and ViT-L/14 models, -tr.
(The ViT-L/14 tower itself exists now -- aphantasia_amd.clip.load('ViT-L/14'), clip_fft.py -m ViT-L/14; admitting the flag here, with
cppn.py:197's 0.11 derating, is the follow-up.)
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from aphantasia_amd import run          # noqa: E402

clip_models = ['ViT-B/16', 'ViT-B/32', 'ViT-L/14', 'RN50', 'RN50x4', 'RN50x16', 'RN50x64', 'RN101']


def get_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('-i',  '--in_img',  default=None, help='input image')
    parser.add_argument('-t',  '--in_txt',  default=None, help='input text')
    parser.add_argument('-t0', '--in_txt0', default=None, help='input text to subtract')
    parser.add_argument(       '--out_dir', default='_out')
    parser.add_argument('-r',  '--resume',  default=None, help='Input CPPN model (NPY file) to resume from')
    parser.add_argument('-s',  '--size',    default='512-512', help='Output resolution')
    parser.add_argument(       '--fstep',   default=1, type=int, help='Saving step')
    parser.add_argument('-tr', '--translate', action='store_true')
    parser.add_argument('-v',  '--verbose', action='store_true')
    parser.add_argument('-ex', '--export',  action='store_true', help='(refused: shader export is not part of this path)')
    # networks
    parser.add_argument('-l',  '--layers',  default=10, type=int, help='CPPN layers')
    parser.add_argument('-nf', '--nf',      default=24, type=int, help='num features')
    parser.add_argument('-act', '--actfn',  default='unbias', choices=['unbias', 'comp', 'relu'], help='activation function')
    parser.add_argument('-dec', '--decim',  default=3, type=int, help='Decimal precision for export')
    # training
    parser.add_argument('-m',  '--model',   default='ViT-B/32', choices=clip_models, help='Select CLIP model to use')
    parser.add_argument('-dm', '--dualmod', default=None, type=int, help='Every this step use another CLIP ViT model')
    parser.add_argument(       '--steps',   default=200, type=int, help='Total iterations')
    parser.add_argument(       '--samples', default=50, type=int, help='Samples to evaluate')
    parser.add_argument('-lr', '--lrate',   default=0.003, type=float, help='Learning rate')
    parser.add_argument('-a',  '--align',   default='overscan', choices=['central', 'uniform', 'overscan'], help='Sampling distribution')
    parser.add_argument('-sh', '--sharp',   default=0, type=float, help='(refused: the Sobel derivative is not built)')
    parser.add_argument('-tf', '--transform', action='store_true', help='use augmenting transforms: here `transforms_fast` (the reference names '
                                                                        '`transforms.trfm_fast`, which does not exist)')
    parser.add_argument('-mc', '--macro',   default=0.4, type=float, help='Endorse macro forms 0..1; -1 = normal big')
    parser.add_argument(       '--aest',    default=0., type=float)
    # additive (not in the reference; as in clip_fft.py)
    parser.add_argument(       '--clip-weights', dest='clip_weights', default=None, help='OpenAI CLIP checkpoint (ViT-B-32.pt); second model: --clip-weights2')
    parser.add_argument(       '--clip-weights2', dest='clip_weights2', default=None, help='checkpoint of the --dualmod model (ViT-B-16.pt)')
    parser.add_argument(       '--bpe-vocab', dest='bpe_vocab', default=None, help='BPE vocabulary of the text prompts (bpe_simple_vocab_16e6.txt.gz; default: beside the checkpoint)')
    parser.add_argument(       '--aest-weights', dest='aest_weights', default=None, help='state dict of the LAION aesthetic head of the model')
    parser.add_argument(       '--aest-weights2', dest='aest_weights2', default=None, help='the head of the --dualmod model')
    parser.add_argument(       '--seed',    default=None, type=int, help='seed torch/numpy RNG (reference: unseeded); the network then starts from the reference\'s weights')
    parser.add_argument(       '--rng',     default=None, choices=['bulk', 'reference'], help='host random draws (clip_fft.py --rng); default: reference when --seed is given, else bulk')
    parser.add_argument(       '--no_save', action='store_true', help='do not write the per-step JPEG frames and snapshots')
    parser.add_argument(       '--no-graph', action='store_true', help='eager launches instead of hipGraph replay (debugging)')
    parser.add_argument(       '--exact',   action='store_true', help='opt-in fp32 ViT (clip_fft.py --exact)')
    a = parser.parse_args(argv)
    if a.size is not None: a.size = [int(s) for s in a.size.split('-')][::-1]        # cppn.py:62-63
    if len(a.size) == 1: a.size = a.size * 2
    if a.dualmod is not None:                                                         # cppn.py:66-67
        a.model = 'ViT-B/32'
    if a.rng is None:
        a.rng = 'reference' if a.seed is not None else 'bulk'
    check_supported(a)
    return a


def check_supported(a):
    """what the reference's command line has and this path does not: refused with a message, never silently ignored"""
    if a.translate:
        raise SystemExit(' -tr: translation needs the googletrans module and a network; translate the prompt beforehand')
    if a.export:
        raise SystemExit(' -ex: shader export (shader_expo.py) is not part of the MI355X path; the .npy snapshots are the reference\'s, export them there')
    if a.sharp != 0:
        raise SystemExit(' -sh: the Sobel derivative of cppn.py:291-292 is not built (aph_rgb_sharp is the `naiv` form of clip_fft.py)')
    if not a.model.startswith('ViT-B'):
        raise SystemExit(' the MI355X path covers the ViT CLIP models ViT-B/32 and ViT-B/16; got %s' % a.model)


def derate_samples(a):
    """The reference's sample-count arithmetic, in its order (cppn.py:197-203, 221)."""
    xmem = {'ViT-B/16': 0.25, 'ViT-L/14': 0.11, 'RN50': 0.5, 'RN50x4': 0.16, 'RN50x16': 0.06, 'RN50x64': 0.04, 'RN101': 0.33}
    s = a.samples
    if a.model in xmem:
        s = int(s * xmem[a.model])
    if a.dualmod is not None:
        s = int(s * 0.69)            # second is vit-16
    if a.transform is True:
        s = int(s * 0.95)
    return s


def main(argv=None):
    a = get_args(argv)
    run.seed_all(a.seed)
    from aphantasia_amd import clip as aclip, transforms
    from aphantasia_amd.cppn import cppn_image, export_data
    from aphantasia_amd.utils import basename, txt_clean
    from aphantasia_amd.engine import Engine

    resume = a.resume if a.resume is not None and os.path.isfile(a.resume) else None          # cppn.py:179
    params, image_f, _ = cppn_image([1, 3, *a.size], a.layers, a.nf, a.actfn, resume)
    syn = image_f.synth
    a.layers, a.nf, a.actfn = syn.layers, syn.nf, syn.actfn
    print(' .. %d vars, %d layers, %d nf, act %s' % (len(params), a.layers, a.nf, a.actfn))

    model_clip, model_clip2 = run.load_models(a.model, a.clip_weights, 'ViT-B/16' if a.dualmod is not None else None, a.clip_weights2)
    a.modsize = model_clip.visual.input_resolution
    a.samples = derate_samples(a)
    run.check_samples(a.samples)
    if a.dualmod is not None:
        print(' dual model every %d step' % a.dualmod)
    aest1 = run.load_aest(a.aest_weights, a.aest)
    aest2 = run.load_aest(a.aest_weights2, a.aest) if a.dualmod is not None else None

    trform_f = transforms.transforms_fast if a.transform is True else transforms.normalize()
    models = [model_clip] + ([model_clip2] if model_clip2 is not None else [])
    targets = [[] for _ in models]            # (embedding, coef) per model: cppn.py:283-290
    out_name = []
    if a.in_txt is not None:
        print(' ref text: ', basename(a.in_txt))
        for t, m in zip(targets, models): t.append((aclip.text_embedding(m, a.in_txt, bpe_vocab=a.bpe_vocab), -1.0))
        out_name.append(txt_clean(a.in_txt))
    if a.in_txt0 is not None:
        print(' no text: ', basename(a.in_txt0))
        for t, m in zip(targets, models): t.append((aclip.text_embedding(m, a.in_txt0, bpe_vocab=a.bpe_vocab), 0.5))
    if a.in_img is not None and os.path.isfile(a.in_img):
        print(' ref image:', basename(a.in_img))
        rows = run.image_target_rows(a.in_img, models, a.samples, a.modsize, a.align)[1]
        for t, r in zip(targets, rows): t.append((r, -1.0))                                                     # per-cut pairs
        out_name.append(basename(a.in_img).replace(' ', '_'))
    if not targets[0]:
        raise SystemExit(' Loss not defined, check the inputs (-t, -t0, -i)')
    aclip.release_text(*models)                                                      # the targets are built: the text arenas can go

    sfx = '-l%d-n%d' % (a.layers, a.nf)                                              # cppn.py:259-265
    if a.dualmod is not None: sfx += '-dm%d' % a.dualmod
    if a.aest != 0:           sfx += '-ae%.2g' % a.aest
    out_name = os.path.join(a.out_dir, 'cppn', '-'.join(out_name) + sfx)
    tempdir = out_name
    os.makedirs(tempdir, exist_ok=True)
    print(a.samples)

    h, w = a.size
    common = dict(sim='cossim', lr=a.lrate, optimizer='adam', align=a.align, macro=a.macro, transform=trform_f, rng=a.rng, exact=a.exact,
                  use_graph=not a.no_graph, param_kind='cppn', cppn=syn)
    eng = Engine(image_f.flat, h, w, model_clip, a.samples, targets[0], aest=aest1, **common)
    eng2 = None
    if model_clip2 is not None:
        eng2 = Engine(image_f.flat, h, w, model_clip2, a.samples, targets[1], aest=aest2, state=eng.state(), **common)

    writer = None if a.no_save else run.FrameWriter(h, w)
    prog = run.Progress(a.steps, 'step', a.verbose)
    for i in range(a.steps):
        e = eng2 if run.is_dual_step(i, a.dualmod) else eng
        e.step()
        if i % a.fstep == 0 and writer is not None:                                   # cppn.py:299-304
            fname = os.path.join(tempdir, '%04d' % (i // a.fstep))
            writer.put(e.synthesize().reshape(3, h, w), fname + '.jpg')
            export_data(image_f.state_dict(), fname)
        prog.tick(i, e)
    torch.cuda.synchronize()
    if writer is not None:
        export_data(image_f.state_dict(), out_name)                                    # cppn.py:312 (the .npy; no shaders)
        run.finish_frames(writer, tempdir, '%04d', out_name, out_name + '-%d.jpg' % a.steps)
    prog.done()


if __name__ == '__main__':
    main()
