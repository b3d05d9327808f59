"""CPU: the ViT-L/14 ground under the tests/emu interpreter (bodies in vitl_checks.py) -- the five-block attention kernels against fp64, the
window patchify pair bit for bit, the tower on padded 14-pixel patch rows and at width 1024, whole engine steps against the oracle, the
refusals.  tests/test_gpu_vitl.py runs the same checks, and more shapes, on the product library."""
import os
import sys

import pytest

from aphantasia_amd import _ffi
import vit_component_checks as V
import vitl_checks as C

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.mark.parametrize('T', [257, 320])
def test_attention_five_blocks_vs_fp64(emu, T):
    r = V.check_attention_fp64(emu, 'cpu', S=2, T=T, heads=2, kind='normal')
    print('T=%d normal: worst err / bound %s' % (T, ' '.join('%s %.3g' % kv for kv in r.items())))


def test_attention_past_320_tokens_is_refused(emu):
    C.check_attention_refused(emu, 'cpu')


@pytest.mark.parametrize('patch,R,R_src', C.WIN_CASES)
def test_patchify_win_bits(emu, patch, R, R_src):
    C.check_patchify_win(emu, 'cpu', patch, R, R_src)


@pytest.mark.parametrize('patch', [16, 32])
def test_patchify_win_equals_the_power_of_two_entries(emu, patch):
    C.check_patchify_win_matches_pow2(emu, 'cpu', patch)


def test_tower_padded_patch_rows(emu):
    C.check_tower(emu, 'cpu', C.TINY14, S=3, check_fuse=True)


def test_tower_257_tokens(emu):
    C.check_tower(emu, 'cpu', C.T257, S=1)


def test_tower_width_1024(emu):
    # (one cut -- 17 rows through the width-1024 GEMMs -- and no second pass for the pad columns: the interpreter is slow; the GPU test runs both)
    C.check_tower(emu, 'cpu', C.W1024, S=1, pad=False)


@pytest.mark.parametrize('tf', ['none', 'fast', 'custom'])
def test_engine_steps_vs_oracle(emu, tf):
    C.check_step(emu, 'cpu', tf, steps=2, use_graph=False)


def test_refusals(emu):
    C.check_refusals(emu, 'cpu')


def test_engine_two_ranks_gloo(emu):
    C.check_ranks_gloo(emu)
