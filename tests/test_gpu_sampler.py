"""GPU (MI355X): the crop sampler and the `-tf fast` chain of the product library held element-wise to the coordinate-exact float64
restatement (sampler_ref.py), at every case, layout and crop-adjoint kernel path of sampler_checks.py -- the checks test_emu_sampler.py runs
under the interpreter."""
import pytest

import sampler_checks as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FWD, BWD = K.mode_cases()


@pytest.mark.parametrize('case', FWD, ids=K.case_id)
def test_sampler_forward_fp64(case):
    K.check_forward(None, DEV, *case)


@pytest.mark.parametrize('case', BWD, ids=K.case_id)
def test_sampler_adjoint_fp64(case):
    K.check_adjoint(None, DEV, *case)
