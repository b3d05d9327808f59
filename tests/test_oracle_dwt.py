"""CPU: the DWT oracle restatement (oracle/dwt_ref.py) pinned against PyWavelets 1.1.1: its waverec2 / wavedec2 outputs on
these seeded inputs are stored in tests/golden/pywt_dwt.npz (oracle/make_pywt_goldens.py)."""
import numpy as np
import pytest

from oracle import dwt_ref
from oracle import make_pywt_goldens as P


@pytest.mark.parametrize('wave,h,w', P.IDWT_CASES)
def test_idwt_vs_pywt(golden, wave, h, w):
    Ys = P.idwt_coeffs(wave, h, w)
    img = dwt_ref.idwt(Ys[0], Ys[1:], wave)
    assert img.shape[-2] in (h, h + 1) and img.shape[-1] in (w, w + 1)
    want = golden('pywt_dwt.npz')[P.idwt_key(wave, h, w)]
    assert np.abs(img[0].numpy() - want).max() < 1e-10 * max(1.0, np.abs(want).max())


def test_shapes_match_survey_probe():
    # SURVEY.md section 2.3 (probed with pywt 1.1.1): 2160x3840 db3 -> 11 levels with these sizes
    J, sizes = dwt_ref.coeff_shapes(2160, 3840, 'db3')
    assert J == 11
    assert [s[0] for s in sizes] == [1082, 543, 274, 139, 72, 38, 21, 13, 9, 7, 6]
    assert [s[1] for s in sizes] == [1922, 963, 484, 244, 124, 64, 34, 19, 12, 8, 6]
    assert dwt_ref.max_level(720, 1280) == 9 and dwt_ref.max_level(224, 224) == 7
    assert (720 + 12 - 1) // 2 == 365


@pytest.mark.parametrize('wave,h,w', P.FWD_CASES)
def test_forward_dwt_host_vs_pywt_and_round_trip(golden, wave, h, w):
    """aphantasia_amd.dwt.dwt_forward_host (img2dwt, image.py:82-94) == pywt.wavedec2(mode='symmetric');
    and the oracle's inverse transform reconstructs the image from it (perfect reconstruction, band order included)"""
    from aphantasia_amd.dwt import dwt_forward_host, max_level
    x = P.fwd_image(h, w)
    J = max_level(h, w)
    yl, yh = dwt_forward_host(x, wave)
    assert len(yh) == J
    g = golden('pywt_dwt.npz')
    want = {k[len(P.fwd_key(wave, h, w)):]: v for k, v in g.items() if k.startswith(P.fwd_key(wave, h, w))}
    assert len(want) == J + 1
    assert np.abs(yl[0, 0].numpy() - want['yl']).max() < 1e-5
    for j in range(J):
        assert np.abs(yh[j][0, 0].numpy() - want['yh%d' % j]).max() < 1e-5, j
    rec = dwt_ref.idwt(yl.double(), [y.double() for y in yh], wave)
    assert (rec[..., :h, :w] - x).abs().max().item() < 1e-5
