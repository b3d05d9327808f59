"""CPU: the coordinate-exact float64 restatement of the crop sampler and the `-tf fast` chain (sampler_ref.py) pinned against the
reference-generated golden, the float32 oracle and, where present, the torchvision fixture -- no kernel involved -- and then the kernels of
csrc/sampler_crop.h, sampler_crop_adjoint.h and sampler_warp.h under the tests/emu interpreter held to it (sampler_checks.py); the product
library runs the identical checks in tests/test_gpu_sampler.py.  Every case runs here too: the largest (`lds-224`, `lds-256`, `fast-224`)
take 10 to 25 s per adjoint check under the interpreter, under the 30 s that would make them GPU-only."""
import os
import sys

import pytest

from aphantasia_amd import _ffi
import kernel_checks
import sampler_checks as K

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
FWD, BWD = K.mode_cases()


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


# ---------------------------------------------------------------------------- the restatement's own pins
@pytest.mark.parametrize('align', ['uniform', 'central', 'overscan', 'overmax'])
def test_reference_vs_golden(golden, align):
    K.check_reference_vs_golden(golden('slice_48x80.npz'), align)


@pytest.mark.parametrize('name', list(K.CROP_CASES) + list(K.FAST_CASES))
def test_reference_vs_fp32_oracle(name):
    K.check_reference_vs_oracle(name)


def test_reference_vs_torchvision_fixture():
    K.check_reference_vs_tv_fixture(kernel_checks.tv_fixture_or_skip())


def test_reference_adjoint_is_the_transpose():
    """<A x, g> == <x, A^T g> in float64, crop with wrap padding and all three warp stages"""
    import numpy as np
    case = K.Case.get('fast_b-overscan')
    smp, x, g = case.sampler(), case.img.double().numpy(), case.g.double().numpy()
    lhs, rhs = (smp.forward(x) * g).sum(), (x * smp.adjoint(g)).sum()
    assert abs(lhs - rhs) <= 64 * 2.0 ** -53 * (smp.forward(np.abs(x), mode='abs') * np.abs(g)).sum(), (lhs, rhs)


# ---------------------------------------------------------------------------- the kernels under the interpreter
@pytest.mark.parametrize('case', FWD, ids=K.case_id)
def test_sampler_forward_fp64(emu, case):
    K.check_forward(emu, 'cpu', *case)


@pytest.mark.parametrize('case', BWD, ids=K.case_id)
def test_sampler_adjoint_fp64(emu, case):
    K.check_adjoint(emu, 'cpu', *case)
