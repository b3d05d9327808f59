"""Checks of the CLIP text tower (csrc/text.hip, the causal instantiation of vit_attn_f32.h), shared by the interpreter tests
(test_emu_text.py) and the GPU tests (test_gpu_text.py).  `lib` = a loaded C-ABI library (the interpreter build or the product),
`dev` = where its tensors live.  The checks return their figures; the callers print them (profiles/text_fp64_bounds.txt holds a run)."""
import ctypes
from fractions import Fraction

import numpy as np
import torch

from aphantasia_amd import ops
from aphantasia_amd.weights import synthetic_text_weights
import exact_checks as X
import text_ref
import vit_component_checks as V

TINY = dict(context_length=77, vocab_size=300, width=256, layers=2, heads=4, output_dim=128)
B32 = dict(context_length=77, vocab_size=49408, width=512, layers=12, heads=8, output_dim=512)
L14 = dict(context_length=77, vocab_size=49408, width=768, layers=12, heads=12, output_dim=768)
GATE = 4.0      # kernel error <= GATE x the error of the fp32 torch evaluation of the same restatement (the CPPN and -tf checks' rule)


# ------------------------------------------------------------------------------------------------------------ causal fp32 attention
def attn_causal_ref(q, k, v):
    """V.attn_fwd_ref with query row i seeing the keys j <= i only.  The quantities attn_fwd_bound_f32 reads are the masked ones: P = 0 on the
    hidden keys, whose score is reported as the row maximum (s - mx = 0) with no score error, so that they add nothing to any bound."""
    T = q.shape[1]
    vis = torch.ones(T, T, dtype=torch.bool).tril()
    s = q @ k.mT
    e_s = torch.where(vis, 1e-6 * (q.abs() @ k.abs().mT), torch.zeros((), dtype=s.dtype))
    mx = s.masked_fill(~vis, float('-inf')).amax(-1, keepdim=True)
    s = torch.where(vis, s, mx.expand_as(s))
    pu = torch.where(vis, torch.exp((s - mx) / 8), torch.zeros((), dtype=s.dtype))
    l = pu.sum(-1, keepdim=True)
    P = pu / l
    return dict(s=s, e_s=e_s, mx=mx, e_mx=e_s.amax(-1, keepdim=True), l=l, P=P, O=P @ v, lse=mx / 8 + torch.log(l))


def fma32(a, b, c):
    """fmaf(a, b, c) of three fp32 values, exactly: the rational a b + c rounded once to fp32 (nearest, ties to even)"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    f = np.float32(float(x))                      # within one fp32 step of the answer; choose among it and its neighbours
    cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    def key(y):
        even = (int(np.float32(y).view(np.int32)) & 1) == 0
        return (abs(Fraction(float(y)) - x), 0 if even else 1)
    return min(cands, key=key)


def causal_call(lib, qkv, S, T, heads):
    """aph_attn_causal_f32_test into sentinel-filled outputs with guard rows -> (att [M + G, D], lse [1, NL + G]) on the CPU"""
    D, M, NL, G = heads * 64, S * T, S * heads * T, V.GUARD_ROWS
    att, ls = V.sentinel(M + G, D, torch.float32, qkv.device), V.sentinel(1, NL + G, torch.float32, qkv.device)
    ops.attn_causal_f32(qkv, att, ls, S, T, heads, lib=lib)
    return att.cpu(), ls.cpu()


def check_attention_causal(lib, dev, S, T, heads, kind='normal', seed=0):
    """The causal fp32 attention forward through aph_attn_causal_f32_test:
      (a) every element of att and lse against the fp64 causal softmax, within exact_checks.attn_fwd_bound_f32 of the masked quantities;
          sentinels behind the outputs, inputs unchanged, two calls give the same bits
      (b) row 0 exactly: att = v_0 bit for bit (the single probability is 1), lse = (q_0 . k_0 as the kernel's fma chain) / 8
      (c) causality as a bit property: K and V of every key j > i* replaced by other values, +-1e30 and NaN among them, leave rows <= i* of att
          and lse unchanged in every bit (a kernel that computes the hidden scores and discards them fails on the NaN)
      (d) the last row sees every key: bit-identical to the non-causal kernel's last row
    Returns the worst err / bound of att and lse."""
    D, M, NL = heads * 64, S * T, S * heads * T
    what = 'causal fp32 attention %s S=%d T=%d heads=%d' % (kind, S, T, heads)
    qkv = V.attn_inputs(kind, S, T, heads, seed)[0].float()
    q, k, v = V.attn_items(qkv, S, T, heads, 3)
    r = attn_causal_ref(q, k, v)
    e_att, e_lse = X.attn_fwd_bound_f32(r, v)
    d_qkv = qkv.clone().to(dev)
    att, ls = V._twice(lambda: causal_call(lib, d_qkv, S, T, heads), what)
    V._unchanged(dict(qkv=d_qkv), dict(qkv=qkv), what)
    fd = V.Findings(what)
    fd.within('att', att[:M], V.attn_rows(r['O'], S, T, heads), V.attn_rows(e_att, S, T, heads))           # (a)
    fd.within('lse', ls[0, :NL], r['lse'].reshape(-1), e_lse.reshape(-1))
    fd.run(V.assert_untouched, att, V._window(M + V.GUARD_ROWS, D, slice(0, M)), what + ' (att)')
    fd.run(V.assert_untouched, ls, V._window(1, NL + V.GUARD_ROWS, (0, slice(0, NL))), what + ' (lse)')

    q3 = qkv.reshape(S, T, 3, heads, 64)                                                                   # (b)
    for s in range(S):
        for h in range(heads):
            fd.check(torch.equal(V.bits(att[s * T, h * 64:(h + 1) * 64]), V.bits(q3[s, 0, 2, h])), '%s: att row 0 of (%d, %d) is not v_0' % (what, s, h))
            a = np.float32(0)
            for d in range(64):
                a = fma32(q3[s, 0, 0, h, d].item(), q3[s, 0, 1, h, d].item(), a)
            got = ls[0, (s * heads + h) * T].item()
            fd.check(np.float32(got) == np.float32(a) * np.float32(0.125), '%s: lse row 0 of (%d, %d) = %r, fma chain / 8 = %r' %
                     (what, s, h, got, float(a) / 8))

    lse_rows = ls[0, :NL].reshape(S, heads, T)                                                             # (c)
    g = torch.Generator().manual_seed(seed + 77)
    for istar in sorted({i for i in (0, 31, 32, T - 2) if 0 <= i < T - 1}):
        other = qkv.clone().reshape(S, T, 3 * D)
        tail = torch.randn(S, T - 1 - istar, 2 * D, generator=g) * 3.0
        flat = tail.reshape(-1)
        n = flat.numel()
        flat[torch.arange(0, n, 7)] = float('nan')
        flat[torch.arange(1, n, 11)] = 1e30
        flat[torch.arange(2, n, 13)] = -1e30
        other[:, istar + 1:, D:] = tail
        att2, ls2 = causal_call(lib, other.reshape(M, 3 * D).contiguous().to(dev), S, T, heads)
        a1, a2 = V.bits(att[:M]).reshape(S, T, D)[:, :istar + 1], V.bits(att2[:M]).reshape(S, T, D)[:, :istar + 1]
        l1, l2 = V.bits(lse_rows)[:, :, :istar + 1], V.bits(ls2[0, :NL].reshape(S, heads, T))[:, :, :istar + 1]
        fd.check(torch.equal(a1, a2), '%s: K / V of the keys > %d reach att rows <= %d (%d elements differ)' % (what, istar, istar, int((a1 != a2).sum())))
        fd.check(torch.equal(l1, l2), '%s: K of the keys > %d reaches lse rows <= %d' % (what, istar, istar))

    fatt, fls = V.sentinel(M, D, torch.float32, dev), V.sentinel(1, NL, torch.float32, dev)               # (d)
    X.attn_f32_call(lib, d_qkv, fatt, fls, None, None, None, S, T, heads, 0)
    last = torch.arange(S) * T + T - 1
    fd.check(torch.equal(V.bits(att[:M])[last], V.bits(fatt)[last]), what + ': the last row differs from the non-causal kernel\'s (att)')
    fd.check(torch.equal(V.bits(lse_rows)[:, :, T - 1], V.bits(fls).reshape(S, heads, T)[:, :, T - 1]),
             what + ': the last row differs from the non-causal kernel\'s (lse)')
    return fd.finish()


# ------------------------------------------------------------------------------------------------------------------------ whole tower
def prompt_tokens(cfg, eots, seed=5):
    """int32 [len(eots), ctx]: SOT (vocab - 2), random ids in [1, vocab - 2), EOT (vocab - 1) at position eots[i], zero padding"""
    g = torch.Generator().manual_seed(seed)
    vocab, ctx = cfg['vocab_size'], cfg['context_length']
    tok = torch.zeros(len(eots), ctx, dtype=torch.int32)
    for i, e in enumerate(eots):
        assert 1 <= e < ctx
        tok[i, 0] = vocab - 2
        tok[i, 1:e] = torch.randint(1, vocab - 2, (e - 1,), generator=g).int()
        tok[i, e] = vocab - 1
    return tok


def default_eots(ctx):
    """EOT at positions 1, 2, ctx - 1 and mid-sequence"""
    return [1, 2, ctx - 1, ctx // 2]


_refs = {}


def tower_ref(cfg, seed_w, eots):
    """(weights, tokens, fp64 embedding, max |fp32 torch evaluation - fp64|), computed once per configuration and shared"""
    key = (tuple(sorted(cfg.items())), seed_w, tuple(eots))
    if key not in _refs:
        w = synthetic_text_weights(cfg, seed_w)
        tok = prompt_tokens(cfg, eots)
        want = text_ref.encode_text({k: v.double() for k, v in w.items()}, tok, cfg)
        e32 = (text_ref.encode_text(w, tok, cfg).double() - want).abs().max().item()
        _refs[key] = (w, tok, want, e32)
    return _refs[key]


def check_tower(lib, dev, cfg=TINY, eots=None, seed_w=4, tag='tower', invariants=True, alone=None):
    """aph_text_forward against text_ref in fp64: max |kernel - fp64| over the embedding <= GATE x max |fp32 torch - fp64|.
    invariants: ids after the EOT, ids >= vocab (clamped by the kernel) among them, leave enc bit-identical; a prompt alone (S = 1) gives
    the bits it has in the batch (alone: the prompts to try, default all).  Returns (kernel error, fp32 restatement's error)."""
    eots = default_eots(cfg['context_length']) if eots is None else eots
    w, tok, want, e32 = tower_ref(cfg, seed_w, eots)
    S = len(eots)
    th = ops.TextHandle(cfg, w, max_batch=S, lib=lib)
    assert th.workspace_bytes() > 4 * sum(v.numel() for v in w.values())
    enc = th.forward(tok.to(dev)).cpu()
    err = (enc.double() - want).abs().max().item()
    print('%s ctx=%d width=%d layers=%d S=%d: max |kernel - fp64| %.3e, fp32 restatement %.3e, ratio %.2f (max |enc| %.3g)'
          % (tag, cfg['context_length'], cfg['width'], cfg['layers'], S, err, e32, err / e32, want.abs().max().item()))
    assert torch.isfinite(enc).all() and err <= GATE * e32, (err, e32)
    if invariants:
        junk = tok.clone()
        g = torch.Generator().manual_seed(9)
        for i, e in enumerate(eots):
            n = cfg['context_length'] - 1 - e
            if n:
                fill = torch.randint(0, cfg['vocab_size'] - 1, (n,), generator=g).int()          # below the EOT id: the argmax stays
                fill[::3] = cfg['vocab_size'] + 5 + i                                            # past the table: clamped to vocab - 1 = the EOT id
                junk[i, e + 1:] = fill
        assert not torch.equal(junk, tok)
        enc_j = th.forward(junk.to(dev)).cpu()
        assert torch.equal(V.bits(enc_j), V.bits(enc)), 'ids after the EOT change the embedding'
        for i in (range(S) if alone is None else alone):
            one = th.forward(tok[i:i + 1].contiguous().to(dev)).cpu()
            assert torch.equal(V.bits(one[0]), V.bits(enc[i])), 'prompt %d alone differs from its row in the batch' % i
    th.close()
    return err, e32


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, dev):
    """every refusal of aph_text_*: its error code with a message, nothing launched (the output keeps its sentinel)"""
    from aphantasia_amd._ffi import ptr
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    h = ctypes.c_void_p()

    def create(ctx=9, vocab=300, width=256, layers=1, heads=4, out=128, mb=2):
        return lib.cdll.aph_text_create(ctx, vocab, width, layers, heads, out, mb, ctypes.byref(h))
    for kw, code, word in ((dict(heads=3), ERR_UNSUPPORTED, 'head'), (dict(width=320, heads=5), ERR_UNSUPPORTED, '256'),
                           (dict(width=128, heads=2), ERR_UNSUPPORTED, '256'), (dict(ctx=257), ERR_UNSUPPORTED, 'context'),
                           (dict(ctx=0), ERR_UNSUPPORTED, 'context'), (dict(mb=0), ERR_ARG, 'max_batch')):
        rc = create(**kw)
        assert rc == code and word in lib.last_error() and 'aph_text_create' in lib.last_error(), (kw, rc, lib.last_error())
    cfg = dict(TINY, context_length=9, layers=1)
    w = synthetic_text_weights(cfg, 1)
    assert create() == 0
    try:
        tok = prompt_tokens(cfg, [3, 5, 8]).to(dev)
        out = V.sentinel(3, cfg['output_dim'], torch.float32, dev)
        st = ops._stream(tok)

        def fwd(S):
            return lib.cdll.aph_text_forward(h, ptr(tok), S, ptr(out), st)

        def put(k, a):
            a = np.ascontiguousarray(a.numpy())
            return lib.cdll.aph_text_set_weight(h, k.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size)
        assert fwd(2) == ERR_ARG and 'not fully loaded (0 of' in lib.last_error()
        assert put('visual.proj', w['text_projection']) == ERR_ARG and 'unknown key' in lib.last_error()
        assert put('text_projection', w['text_projection'][:-1]) == ERR_ARG and 'expected' in lib.last_error()
        last = list(w)[-1]
        for k, v in w.items():
            if k != last:
                assert put(k, v) == 0
        assert fwd(2) == ERR_ARG and 'not fully loaded' in lib.last_error()
        assert put(last, w[last]) == 0
        assert fwd(3) == ERR_ARG and 'batch 3 outside 1..2' in lib.last_error()
        assert fwd(0) == ERR_ARG
        assert lib.cdll.aph_text_forward(h, None, 1, ptr(out), st) == ERR_ARG and 'null' in lib.last_error()
        V.assert_untouched(out.cpu(), torch.zeros(3, cfg['output_dim'], dtype=torch.bool), 'refused aph_text_forward calls')
        assert fwd(2) == 0
        assert torch.isfinite(out.cpu()[:2]).all()
        assert int(lib.cdll.aph_text_workspace_bytes(h)) > 0 and int(lib.cdll.aph_text_workspace_bytes(None)) == 0
    finally:
        lib.cdll.aph_text_destroy(h)
    # the causal hook refuses what aph_attn_f32_test refuses
    qkv = torch.zeros(4, 3 * 64, device=dev)
    att, ls = V.sentinel(4, 64, torch.float32, dev), V.sentinel(1, 4, torch.float32, dev)
    for S, T, heads in ((0, 4, 1), (1, 0, 1), (1, 257, 1), (1, 4, 0)):
        rc = lib.cdll.aph_attn_causal_f32_test(ptr(qkv), ptr(att), ptr(ls), S, T, heads, ops._stream(qkv))
        assert rc == ERR_ARG and 'aph_attn_causal_f32_test' in lib.last_error()
    assert lib.cdll.aph_attn_causal_f32_test(None, ptr(att), ptr(ls), 1, 4, 1, ops._stream(qkv)) == ERR_ARG
    V.assert_untouched(att.cpu(), torch.zeros(4, 64, dtype=torch.bool), 'refused aph_attn_causal_f32_test calls')
