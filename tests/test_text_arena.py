"""The text tower's arena keeps its size to the byte (the ViT's pin is tests/test_emu_vit_weights.py::test_arena_sizes_unchanged): every buffer
of the arena keeps its offset only if the total does.  aph_text_workspace_bytes right after aph_text_create -- no weights uploaded, nothing
launched -- under the host SIMT interpreter (tests/emu) and on the MI355X."""
import ctypes
import os
import sys

import pytest

from aphantasia_amd import _ffi
import text_checks as C

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))

# read from the library as it was when the text tower carved its arena with a table and a rounding of its own (before csrc/tower_store.h):
# (configuration, max_batch, bytes)
ARENA_BYTES = [
    (C.TINY, 1, 7705856),
    (C.TINY, 3, 9443072),
    (dict(C.TINY, context_length=9, layers=1), 2, 3811840),
    (C.B32, 16, 281506304),
    (C.L14, 16, 536292096),
]


def check_arena_bytes(lib, cfg, max_batch, want):
    h = ctypes.c_void_p()
    assert lib.cdll.aph_text_create(cfg['context_length'], cfg['vocab_size'], cfg['width'], cfg['layers'], cfg['heads'], cfg['output_dim'], max_batch,
                                    ctypes.byref(h)) == 0, lib.last_error()
    try:
        assert int(lib.cdll.aph_text_workspace_bytes(h)) == want
    finally:
        lib.cdll.aph_text_destroy(h)


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


@pytest.mark.parametrize('cfg,max_batch,want', ARENA_BYTES)
def test_text_arena_sizes_unchanged(emu, cfg, max_batch, want):
    check_arena_bytes(emu, cfg, max_batch, want)


@pytest.mark.gpu
@pytest.mark.parametrize('cfg,max_batch,want', ARENA_BYTES)
def test_text_arena_sizes_unchanged_gpu(cfg, max_batch, want):
    check_arena_bytes(_ffi.lib(), cfg, max_batch, want)
