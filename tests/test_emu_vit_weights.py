"""CPU: the ViT handle's weight table under the host SIMT interpreter (tests/emu) -- "loaded" means every checkpoint tensor has been uploaded,
not a number of uploads, and the arenas keep the sizes they had before the table replaced the hand-written carve lists."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from aphantasia_amd import _ffi, ops
from aphantasia_amd.weights import synthetic_visual_weights
import kernel_checks as K

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))


@pytest.fixture(scope='module')
def emu():
    import build_emu
    return _ffi.Library(build_emu.build())


def _set(lib, vit, key, tensor):
    a = np.ascontiguousarray(tensor.numpy())
    return lib.cdll.aph_vit_set_weight(vit.handle, key.encode(), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.size))


def test_loaded_means_every_tensor_not_a_number_of_uploads(emu):
    """one tensor uploaded 8 + 12 L times leaves the handle unloaded: the forward and both enable calls refuse it; every tensor once, and one
    of them twice, is accepted"""
    cfg = K.TINY
    w = synthetic_visual_weights(cfg, 3)
    total = 8 + 12 * cfg['layers']
    assert len(w) == total
    S, R, p = 2, cfg['input_resolution'], cfg['patch_size']
    patches = ops.patchify(torch.randn(S, 3, R, R, generator=torch.Generator().manual_seed(1)), p, lib=emu)
    out = torch.empty(S, cfg['output_dim'])
    vit = ops.VitHandle(cfg, {}, max_batch=S, lib=emu)
    for _ in range(total):
        assert _set(emu, vit, 'ln_pre.weight', w['ln_pre.weight']) == 0
    assert emu.cdll.aph_vit_forward(vit.handle, ops.ptr(patches), S, ops.ptr(out), None) < 0
    assert 'weights not fully loaded' in emu.last_error() and 'aph_vit_forward' in emu.last_error()
    assert emu.cdll.aph_vit_enable_hilo(vit.handle) < 0
    assert 'weights not fully loaded' in emu.last_error() and 'aph_vit_enable_hilo' in emu.last_error()
    assert emu.cdll.aph_vit_enable_f32(vit.handle) < 0
    assert 'weights not fully loaded' in emu.last_error() and 'aph_vit_enable_f32' in emu.last_error()
    # all but one tensor: still refused; a wrong key and a wrong size do not count either
    last = 'transformer.resblocks.%d.mlp.c_proj.bias' % (cfg['layers'] - 1)
    for k, t in w.items():
        if k != last:
            assert _set(emu, vit, k, t) == 0
    assert _set(emu, vit, 'transformer.resblocks.%d.mlp.c_proj.bias' % cfg['layers'], w[last]) < 0 and 'unknown key' in emu.last_error()
    assert _set(emu, vit, last, w['proj']) < 0 and 'elements, expected' in emu.last_error()
    assert emu.cdll.aph_vit_forward(vit.handle, ops.ptr(patches), S, ops.ptr(out), None) < 0
    assert 'weights not fully loaded' in emu.last_error()
    assert _set(emu, vit, last, w[last]) == 0
    assert _set(emu, vit, 'proj', w['proj']) == 0           # a second upload of a tensor
    enc = vit.forward(patches, S).clone()
    want = ops.VitHandle(cfg, w, max_batch=S, lib=emu).forward(patches, S)
    assert torch.equal(enc, want)
    vit.enable_hilo()
    vit.enable_f32()


# aph_vit_workspace_bytes of the library before the weight table (its carve lists written out by hand), from a build of it under the interpreter:
# (bare handle, after aph_vit_enable_hilo, after aph_vit_enable_f32 on top)
TINY_CFG = dict(K.TINY)
B32 = dict(input_resolution=224, patch_size=32, width=768, layers=2, heads=12, output_dim=512)      # 50 tokens
B16 = dict(input_resolution=224, patch_size=16, width=768, layers=3, heads=12, output_dim=512)      # 197 tokens
ARENA_BYTES = [
    (TINY_CFG, 2, (11812352, 14171648, 28638976)),
    (TINY_CFG, 5, (12173824, 14533120, 29467648)),
    (B32, 2, (80878080, 104471040, 244165888)),
    (B16, 3, (149018368, 172611328, 403804672)),
]


def arena_bytes(lib, cfg, max_batch):
    vit = ops.VitHandle(cfg, synthetic_visual_weights(cfg, 3), max_batch=max_batch, lib=lib)
    b0 = vit.workspace_bytes()
    vit.enable_hilo()
    b1 = vit.workspace_bytes()
    vit.enable_f32()
    return b0, b1, vit.workspace_bytes()


@pytest.mark.parametrize('cfg,max_batch,want', ARENA_BYTES)
def test_arena_sizes_unchanged(emu, cfg, max_batch, want):
    """every buffer keeps its offset from its arena's base only if the totals do: the three arenas, summed as aph_vit_workspace_bytes does"""
    assert arena_bytes(emu, cfg, max_batch) == want
