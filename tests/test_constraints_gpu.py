"""Constrained decoding on the MI355X, kernel by kernel through the debug hooks (include/gitcap.h), exact comparisons only:

  a. ban_mask_kernel against the restatement of tests/constraints_reference.py, word for word, on one reused buffer;
  b. the BAN forms of the vocabulary head: logits, arg-max partials and (LSE) sum partials against the plain head's own fp32
     logits with -inf written at the banned columns -- the selection / log-probability restatements for the winner, and for the
     sum partial the unconstrained LSE head itself, launched on the row alone with the ban expressed as a -inf bias (the head is
     batch invariant: the same MFMA chain, so the same bits);
  c. the BAN forms of the beam ranking and the sampling kernel against their unconstrained hooks on pre-masked logits."""
import ctypes

import numpy as np
import pytest
import torch

import constraints_reference as C
import logprob_reference as L
import selection_reference as R
from gpu_support import (IDX_FILL, NAN, assert_tail, lib, poisoned, ptr, run_vocab_head, softmax_head_inputs, stream,  # noqa: F401
                         to_dev)

pytestmark = pytest.mark.gpu
NINF = float("-inf")
GUARD = 0xA5A5


# ---- a. the mask builder ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [97, 30522])
def test_ban_mask_equals_the_restatement_on_a_reused_buffer(lib, V):
    ld, rows, pad = C.mask_ld(V), 3, 8
    buf = to_dev(np.full(pad + rows * ld + pad, GUARD, np.uint16).view(np.int16), torch.int16)            # 0xA5A5 everywhere
    view = buf[pad:pad + rows * ld]
    for name, p, cur_len, n, m, sep, sup in C.builder_cases(V):
        ids = to_dev(p, torch.int64)
        sp = to_dev(np.array(sup, np.int32), torch.int32) if sup else None
        rc = lib.gitcap_dbg_ban_mask(ptr(ids), ids.shape[1], rows, cur_len, n, m, sep, ptr(sp), len(sup), V, ptr(view), ld, stream())
        torch.cuda.synchronize()
        assert rc == 0, name
        got = view.cpu().numpy().view(np.uint16).reshape(rows, ld)
        want = C.ban_mask(p, cur_len, n, m, sep, sup, V, ld)
        assert np.array_equal(got, want), name
        guard = buf.cpu().numpy().view(np.uint16)
        assert (guard[:pad] == GUARD).all() and (guard[pad + rows * ld:] == GUARD).all(), name
    if V == 30522:
        assert ld == 1908 and V % 16 == 10
    assert lib.gitcap_dbg_ban_mask(ptr(ids), ids.shape[1], rows, 4, 2, 0, 2, None, 1, V, ptr(view), ld, stream()) == -1     # list without pointer
    assert lib.gitcap_dbg_ban_mask(ptr(ids), ids.shape[1], rows, 4, 2, 0, 2, None, 0, V, ptr(view), ld - 1, stream()) == -1  # odd / short ld
    assert lib.gitcap_dbg_ban_mask(ptr(ids), ids.shape[1], rows, 13, 2, 0, 2, None, 0, V, ptr(view), ld, stream()) == -1     # cur_len > ld_ids
    assert lib.gitcap_dbg_ban_mask(ptr(ids), ids.shape[1], rows, 4, -1, 0, 2, None, 0, V, ptr(view), ld, stream()) == -1


# ---- b. the head ----------------------------------------------------------------------------------------------------------------

def _run_banned(lib, X, W, wscale, bias, M, N, K, mask, lse, share):
    nt = (N + 15) // 16
    logits, val = poisoned(M * N + 16, NAN), poisoned(M * nt + 16, NAN)
    idx, ssum = poisoned(M * nt + 16, IDX_FILL, torch.int32), poisoned(M * nt + 16, NAN)
    old = lib.gitcap_dbg_config(10, share)
    try:
        rc = lib.gitcap_dbg_vocab_head_banned(ptr(X), K, ptr(W), ptr(wscale), ptr(bias), M, N, K, ptr(logits), ptr(val), ptr(idx),
                                              ptr(ssum) if lse else None, ptr(mask), mask.shape[1], stream())
        torch.cuda.synchronize()
    finally:
        lib.gitcap_dbg_config(10, old)
    assert rc == 0
    assert_tail(logits, M * N, NAN); assert_tail(val, M * nt, NAN); assert_tail(idx, M * nt, IDX_FILL)
    assert_tail(ssum, M * nt if lse else 0, NAN)
    return logits[:M * N].view(M, N), val[:M * nt].view(M, nt), idx[:M * nt].view(M, nt), ssum[:M * nt].view(M, nt) if lse else None


def _head_masks(lg, N):
    """per row: ban a tile's maximum / nothing / a whole tile + the row maximum + the edge columns, by row % 3"""
    M, nt = lg.shape[0], (N + 15) // 16
    mask = np.zeros((M, C.mask_ld(N)), np.uint16)

    def ban(m, c):
        mask[m, c >> 4] |= np.uint16(1 << (c & 15))
    for m in range(M):
        if m % 3 == 1:
            continue                                        # ban nothing
        for t in range(0, nt, 2):                          # the maximum of every other tile: the runner-up must win
            seg = lg[m, t * 16:min(N, t * 16 + 16)]
            ban(m, t * 16 + int(np.argmax(seg)))
        if m % 3 == 2:
            for c in range(16, min(32, N)):                # a whole tile
                ban(m, c)
            for c in (0, 15, N - 1, int(np.argmax(lg[m]))):
                ban(m, c)
    return mask


def _head_case(lib, M, N, K, fp8, share=1):
    X, W, wscale, bias = softmax_head_inputs(M, N, K, fp8, seed=9100 + 10 * M + N + K)
    # two equal maxima in tile 0 of row 0 (columns 3 and 9 get the same weights and bias), the first of them banned below
    Wb = W.view(torch.uint8) if fp8 else W.view(torch.int16)
    Wb[9] = Wb[3]
    bias[9] = bias[3]
    if wscale is not None:
        wscale[9] = wscale[3]
    plain = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, share=share, hook="lse")
    lg = plain.logits.cpu().numpy()
    assert lg[0, 3] == lg[0, 9]
    boost = float(lg[0].max() - lg[0, 3]) + 4.0
    bias[3] += boost
    bias[9] += boost
    plain = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, share=share, hook="lse")
    lg = plain.logits.cpu().numpy()
    assert lg[0, 3] == lg[0, 9] == lg[0].max()
    mask = _head_masks(lg, N)
    mask[0, 0] |= np.uint16(1 << 3)                       # the first of the two equal maxima
    mask[0, 0] &= np.uint16(~(1 << 9) & 0xFFFF)
    dmask = to_dev(mask.view(np.int16), torch.int16)
    want = C.mask_logits(lg, mask)
    rv, ri, _ = L.tile_partials(want)
    sv, si = R.tile_partials(want)
    for lse in (False, True):
        logits, val, idx, ssum = _run_banned(lib, X, W, wscale, bias, M, N, K, dmask, lse, share)
        got = logits.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                     # -inf at the banned columns, the rest untouched
        assert np.array_equal(val.cpu().numpy().astype(np.float64), rv) and np.array_equal(idx.cpu().numpy().astype(np.int64), ri)
        assert np.array_equal(val.cpu().numpy().astype(np.float64), sv) and np.array_equal(idx.cpu().numpy().astype(np.int64), si)
        assert int(idx[0, 0]) == 9                                                            # the second of the equal maxima wins
        if M > 2 and N >= 32:
            assert float(val[2, 1]) == NINF and int(idx[2, 1]) == L.SENTINEL                  # the wholly banned tile
        for m in range(M):                                                                    # nothing banned: the plain head's bits
            if m % 3 == 1:
                assert torch.equal(val[m], plain.val[m]) and torch.equal(idx[m], plain.idx[m]) and torch.equal(logits[m], plain.logits[m])
                if lse:
                    assert torch.equal(ssum[m], plain.sum[m])
        if lse:
            if M > 2 and N >= 32:
                assert float(ssum[2, 1]) == 0.0
            tok_want, _ = L.token_logprobs(want)
            assert [R.argmax_partials(val[m].cpu().numpy(), idx[m].cpu().numpy()) for m in range(M)] == tok_want.tolist()
            # the sum partial, bit for bit: the unconstrained LSE head on the row alone with the ban as a -inf bias
            for m in sorted({0, 2 % M, M - 1, min(16, M - 1)}):
                b2 = bias.clone()
                b2[torch.as_tensor(np.nonzero(np.isinf(want[m]))[0], device="cuda")] = NINF
                one = run_vocab_head(lib, X[m:m + 1].contiguous(), K, W, wscale, b2, 1, N, K, share=share, hook="lse")
                assert torch.equal(one.sum[0], ssum[m]) and torch.equal(one.val[0], val[m]) and torch.equal(one.idx[0], idx[m]), m
    # a mask that bans nothing equals the plain hooks, bit for bit
    zero = torch.zeros_like(dmask)
    logits, val, idx, ssum = _run_banned(lib, X, W, wscale, bias, M, N, K, zero, True, share)
    assert torch.equal(logits, plain.logits) and torch.equal(val, plain.val) and torch.equal(idx, plain.idx) and torch.equal(ssum, plain.sum)


@pytest.mark.parametrize("M", [1, 16, 17, 64])
@pytest.mark.parametrize("fp8", [False, True])
def test_head_banned_tiny_vocabulary(lib, M, fp8):
    """V = 97: seven tiles, the last workgroup holds three, the last tile one valid column.  K = 128: the e4m3 head's small width."""
    _head_case(lib, M, 97, 128, fp8)


@pytest.mark.parametrize("M,fp8", [(17, False), (20, True)])
def test_head_banned_model_vocabulary(lib, M, fp8):
    """V = 30522 at D = 768: 1908 tiles, a ragged last tile of 10 columns."""
    _head_case(lib, M, 30522, 768, fp8)


@pytest.mark.parametrize("fp8", [False, True])
def test_head_banned_single_wave_form(lib, fp8):
    """gitcap_dbg_config(10, 0): one single-wave workgroup per tile (skinny_full_ban_kernel)"""
    _head_case(lib, 17, 97, 128, fp8, share=0)


def test_head_banned_rejects_bad_arguments(lib):
    X, W, wscale, bias = softmax_head_inputs(2, 97, 128, False, seed=3)
    mask = torch.zeros((2, C.mask_ld(97)), dtype=torch.int16, device="cuda")
    val, idx = poisoned(2 * 7, NAN), poisoned(2 * 7, IDX_FILL, torch.int32)
    head = (ptr(X), 128, ptr(W), None, ptr(bias), 2, 97, 128, None, ptr(val), ptr(idx), None)
    assert lib.gitcap_dbg_vocab_head_banned(*head, None, 8, stream()) == -1
    assert lib.gitcap_dbg_vocab_head_banned(*head, ptr(mask), 7, stream()) == -1            # odd
    assert lib.gitcap_dbg_vocab_head_banned(*head, ptr(mask), 6, stream()) == -1            # short
    assert lib.gitcap_dbg_vocab_head_banned(*head, ptr(mask), 8, stream()) == 0
    torch.cuda.synchronize()


# ---- c. beam ranking and sampling -------------------------------------------------------------------------------------------------

def _beam_inputs(B, beams, V, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = B * beams
    logits = torch.randn(rows, V, device="cuda", generator=g) * 3
    scores = torch.randn(rows, device="cuda", generator=g)
    prefix = torch.randint(0, V, (rows, 6), device="cuda", generator=g)
    lg = logits.cpu().numpy()
    mask = np.zeros((rows, C.mask_ld(V)), np.uint16)
    for r in range(rows):
        cols = [int(np.argmax(lg[r])), 0, V - 1] + ([2047, 2048] if V > 2048 else []) + [int(prefix[r, 1])]
        if r % 2:
            cols += list(range(32, 48))
        for c in cols:
            mask[r, c >> 4] |= np.uint16(1 << (c & 15))
    if V > 2048:                                         # the chunk edge holds the row's runner-ups: they must not come back
        logits[:, 2047] = logits.max() + 1
        logits[:, 2048] = logits.max() + 1
        lg = logits.cpu().numpy()
    return logits, scores, prefix, mask, to_dev(C.mask_logits(lg, mask), torch.float32)


@pytest.mark.parametrize("B,beams,V,K,rp", [(2, 3, 97, 6, 1.0), (2, 3, 97, 6, 1.3), (1, 4, 4122, 8, 1.0), (2, 4, 4122, 16, 0.7)])
def test_beam_topk_constrained_equals_the_hook_on_masked_logits(lib, B, beams, V, K, rp):
    logits, scores, prefix, mask, masked = _beam_inputs(B, beams, V, 50 + V + K)
    dmask = to_dev(mask.view(np.int16), torch.int16)

    def run(fn, lg, *tail):
        s, i = poisoned(B * K + 8, NAN), poisoned(B * K + 8, -9, torch.int32)
        rc = fn(ptr(lg), V, ptr(scores), ptr(prefix), prefix.shape[1], 5, ctypes.c_float(rp), B, beams, V, K, ptr(s), ptr(i), *tail, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert_tail(s, B * K, NAN); assert_tail(i, B * K, -9)
        return s[:B * K], i[:B * K]
    ws, wi = run(lib.gitcap_beam_topk_penalized, masked)
    gs, gi = run(lib.gitcap_beam_topk_constrained, logits, ptr(dmask), dmask.shape[1])
    assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gi, wi)
    fs, fi = run(lib.gitcap_beam_topk_penalized, logits)
    assert not torch.equal(fi, gi)                                      # the banned top candidates were candidates
    words = (gi % V).cpu().numpy().reshape(B, K)
    rows = (np.arange(B)[:, None] * beams + (gi.cpu().numpy().reshape(B, K) // V))
    for b in range(B):
        for w, r in zip(words[b], rows[b]):
            assert not (int(mask[r, w >> 4]) >> (w & 15)) & 1
    assert lib.gitcap_beam_topk_constrained(ptr(logits), V, ptr(scores), ptr(prefix), 6, 5, ctypes.c_float(rp), B, beams, V, K, ptr(gs), ptr(gi),
                                            None, dmask.shape[1], stream()) == -1


@pytest.mark.parametrize("V,rp,T,top_k,top_p", [(97, 1.0, 1.0, 0, 1.0), (97, 1.3, 0.7, 5, 1.0), (4122, 1.0, 1.3, 0, 0.9), (4122, 1.2, 1.0, 50, 0.95)])
def test_sample_rows_constrained_equals_the_hook_on_masked_logits(lib, V, rp, T, top_k, top_p):
    B, beams, pn, seed = 2, 3, 2, 1234567
    logits, scores, prefix, mask, masked = _beam_inputs(B, beams, V, 80 + V + top_k)
    dmask = to_dev(mask.view(np.int16), torch.int16)
    rows, K = B * beams, beams * pn

    def run(fn, lg, *tail):
        s, i = poisoned(B * K + 8, NAN), poisoned(B * K + 8, -9, torch.int32)
        kept, logz = poisoned(rows + 8, -9, torch.int32), poisoned(rows + 8, NAN)
        rc = fn(ptr(lg), V, ptr(scores), ptr(prefix), prefix.shape[1], 5, ctypes.c_float(rp), B, beams, V, pn, ctypes.c_float(T), top_k,
                ctypes.c_float(top_p), ctypes.c_uint64(seed), ptr(s), ptr(i), ptr(kept), ptr(logz), *tail, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert_tail(s, B * K, NAN); assert_tail(i, B * K, -9); assert_tail(kept, rows, -9); assert_tail(logz, rows, NAN)
        return s[:B * K], i[:B * K], kept[:rows], logz[:rows]
    want = run(lib.gitcap_sample_rows, masked)
    got = run(lib.gitcap_sample_rows_constrained, logits, ptr(dmask), dmask.shape[1])
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    free = run(lib.gitcap_sample_rows, logits)
    assert not torch.equal(free[3], got[3])                             # the banned columns carried mass
