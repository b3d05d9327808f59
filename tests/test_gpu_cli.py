"""clip_fft.py, illustrip.py and cppn.py end to end on seeded synthetic CLIP weights: 128x96, 12 samples, 3 steps each.  Output names, a
finite loss in the last progress line, and a second seeded run that writes the same bytes (profiles/cli_run_module_parity.txt: the scripts
are bitwise repeatable on one MI355X)."""
import hashlib
import math
import os
import re

import pytest

pytestmark = pytest.mark.gpu
BASE = ['--seed', '1', '--size', '128-96', '--samples', '12', '--steps', '3']


def run_twice(script, argv, tmp_path, capsys):
    """-> (files of run 1 relative to its --out_dir, stdout of run 1); asserts run 2 wrote the same names with the same snapshot / frame bytes"""
    mod = __import__(script)
    trees = []
    for k in (1, 2):
        out = str(tmp_path / ('o%d' % k))
        mod.main(BASE + argv + ['--out_dir', out])
        text = capsys.readouterr().out
        files = {os.path.relpath(os.path.join(d, f), out): hashlib.sha256(open(os.path.join(d, f), 'rb').read()).hexdigest()
                 for d, _, fs in os.walk(out) for f in fs if not f.endswith('.mp4')}          # (the video, where ffmpeg is installed)
        trees.append((files, text))
    (files, text), (files2, _) = trees
    assert sorted(files) == sorted(files2)
    assert [n for n in files if files[n] != files2[n]] == []
    return sorted(files), text


def last_loss(text, unit):
    lines = [l for l in text.splitlines() if l.startswith(' %s 3/3  loss ' % unit)]
    assert len(lines) == 1 and text.splitlines()[-1].startswith(' done: 3 %ss in ' % unit)
    loss = float(re.match(r' %s 3/3  loss (\S+)  \S+ %ss/s$' % (unit, unit), lines[0]).group(1))
    assert math.isfinite(loss)


def test_clip_fft_dualmod(tmp_path, capsys):
    files, text = run_twice('clip_fft', ['-t', 'cat', '-dm', '2', '--save_pt'], tmp_path, capsys)
    assert files == sorted(['cat-dm2-3.jpg', 'cat-dm2.pt'] + ['cat-dm2/%04d.jpg' % i for i in range(3)])
    assert ' dual model every 2 step\n' in text
    last_loss(text, 'step')


def test_illustrip_fft(tmp_path, capsys):
    files, text = run_twice('illustrip', ['-t', 'cat', '--gen', 'FFT'], tmp_path, capsys)
    assert files == ['cat-FFT/%06d.jpg' % i for i in range(3)]
    last_loss(text, 'frame')


def test_cppn(tmp_path, capsys):
    files, text = run_twice('cppn', ['-t', 'cat', '-v'], tmp_path, capsys)
    assert files == sorted(['cppn/cat-l10-n24-3.jpg', 'cppn/cat-l10-n24.npy'] + ['cppn/cat-l10-n24/%04d.%s' % (i, e) for i in range(3) for e in ('jpg', 'npy')])
    last_loss(text, 'step')
