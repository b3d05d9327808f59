"""TEST INFRASTRUCTURE.  Generates tests/golden/pywt_dwt.npz: PyWavelets' own waverec2 / wavedec2 (mode 'symmetric')
on the seeded inputs of tests/test_oracle_dwt.py, so that those tests pin the DWT restatement without PyWavelets.
PyWavelets runs out of process (oracle/pywt_dump.py) under an interpreter that has it (1.1.1: the version the reference's notebook pins):
    python -m oracle.make_pywt_goldens PYTHON_WITH_PYWT
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import dwt_ref  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'pywt_dwt.npz')
IDWT_CASES = [('db3', 45, 70), ('coif2', 64, 96), ('haar', 33, 40), ('db2', 50, 37)]
FWD_CASES = [('db3', 45, 70), ('coif2', 64, 96), ('haar', 33, 40)]


def idwt_coeffs(wave, h, w):
    """[yl, yh_finest, ...] float64, as dwt_ref.init_params draws them from torch seed 0"""
    torch.manual_seed(0)
    return [y.double() for y in dwt_ref.init_params([1, 3, h, w], wave)]


def fwd_image(h, w):
    g = torch.Generator().manual_seed(3)
    return torch.rand(1, 1, h, w, generator=g, dtype=torch.float64)


def idwt_key(wave, h, w):
    return 'waverec2_%s_%dx%d' % (wave, h, w)


def fwd_key(wave, h, w):
    return 'wavedec2_%s_%dx%d_' % (wave, h, w)


def main(py):
    from aphantasia_amd.dwt import max_level
    dump = os.path.join(ROOT, 'oracle', 'pywt_dump.py')
    res = {}
    with tempfile.TemporaryDirectory() as td:
        inp = os.path.join(td, 'in.npz')
        for wave, h, w in IDWT_CASES:
            Ys = idwt_coeffs(wave, h, w)
            d = dict(J=len(Ys) - 1, wave=wave, yl=Ys[0][0].numpy())
            for j in range(len(Ys) - 1):
                d['yh%d' % j] = Ys[j + 1][0].permute(1, 0, 2, 3).numpy()      # [3 bands, C, h, w]
            np.savez(inp, **d)
            out = os.path.join(td, 'out.npy')
            subprocess.check_call([py, dump, 'waverec2', inp, out], stderr=subprocess.DEVNULL)
            res[idwt_key(wave, h, w)] = np.load(out)
        for wave, h, w in FWD_CASES:
            np.savez(inp, x=fwd_image(h, w)[0, 0].numpy(), wave=wave, J=max_level(h, w))
            out = os.path.join(td, 'out.npz')
            subprocess.check_call([py, dump, 'wavedec2', inp, out], stderr=subprocess.DEVNULL)
            for k, v in np.load(out).items():
                res[fwd_key(wave, h, w) + k] = v
    version = subprocess.check_output([py, '-c', 'import pywt; print(pywt.__version__)'], stderr=subprocess.DEVNULL).decode().strip()
    np.savez_compressed(OUT, pywt_version=np.array(version), **res)
    print('%s: %d arrays, PyWavelets %s, %d bytes' % (OUT, len(res), version, os.path.getsize(OUT)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
