"""The student's constrained decoding on the MI355X, kernel by kernel through the debug hooks (include/gitcap.h), exact comparisons:

  a. gitcap_dbg_ban_mask_rec -- the mask builder whose rules come from a device record when the kernel runs -- against the
     restatement of tests/constraints_reference.py byte for byte, against gitcap_dbg_ban_mask on the same inputs, on ONE poisoned
     buffer reused case after case; the record rewritten between two launches with the same arguments; a full and an over-full list;
  b. the BAN forms of the vocabulary head at the student's widths (K = 64 with V = 97, K = 576 with V = 30522): logits = the plain
     head's with -inf at the banned columns, the arg-max partials exactly those of the selection / log-probability restatements on
     that masked row, the sum partial and the merged log-probability within the 2e-5 that tests/test_logprob_gpu.py derives."""
import numpy as np
import pytest
import torch

import constraints_reference as C
import logprob_reference as L
import selection_reference as R
import student_constraints_support as S
from gpu_support import (IDX_FILL, NAN, assert_tail, lib, poisoned, ptr, run_vocab_head, softmax_head_inputs, stream,  # noqa: F401
                         to_dev)

pytestmark = pytest.mark.gpu
NINF = float("-inf")
GUARD = int(np.array([0xA5A5], np.uint16).view(np.int16)[0])
TOL = 2e-5                          # tests/test_logprob_gpu.py derives it
ROWS, PAD = 3, 16


# ---- a. the mask builder ------------------------------------------------------------------------------------------------------

class _Masks:
    """One poisoned mask buffer for the record form and one for the argument form; the record inside a longer buffer whose words
    behind it name column 5 (a reader that runs past the record bans it)."""

    def __init__(self, lib, V):
        self.lib, self.V, self.ld = lib, V, C.mask_ld(V)
        self.buf = poisoned(ROWS * self.ld + PAD, GUARD, torch.int16)
        self.buf_args = poisoned(ROWS * self.ld + PAD, GUARD, torch.int16)
        self.rec = poisoned(S.REC_WORDS + PAD, 5, torch.int32)

    def _read(self, buf, what):
        assert_tail(buf, ROWS * self.ld, GUARD)
        return buf[:ROWS * self.ld].cpu().numpy().view(np.uint16).reshape(ROWS, self.ld), what

    def write_record(self, rec):
        self.rec[:S.REC_WORDS].copy_(torch.as_tensor(rec))

    def run_rec(self, ids, cur_len, sep):
        rc = self.lib.gitcap_dbg_ban_mask_rec(ptr(ids), ids.shape[1], ROWS, cur_len, sep, ptr(self.rec), self.V, ptr(self.buf), self.ld, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert bool((self.rec[S.REC_WORDS:] == 5).all())
        return self._read(self.buf, "record form")[0]

    def run_args(self, ids, cur_len, n, m, sep, sup):
        sp = to_dev(np.array(sup, np.int32), torch.int32) if sup else None
        rc = self.lib.gitcap_dbg_ban_mask(ptr(ids), ids.shape[1], ROWS, cur_len, n, m, sep, ptr(sp), len(sup), self.V, ptr(self.buf_args), self.ld,
                                          stream())
        torch.cuda.synchronize()
        assert rc == 0
        return self._read(self.buf_args, "argument form")[0]


@pytest.mark.parametrize("V", [97, 30522, 131072])
def test_record_form_equals_the_restatement_and_the_argument_form(lib, V):
    k = _Masks(lib, V)
    for name, p, cur_len, n, m, sep, sup in C.builder_cases(V):            # IN ORDER on ONE buffer
        ids = to_dev(p, torch.int64)
        k.write_record(S.pack_record(n, m, sup, fill=5))
        got = k.run_rec(ids, cur_len, sep)
        want = C.ban_mask(p, cur_len, n, m, sep, sup, V, k.ld)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), name
        assert np.array_equal(got, k.run_args(ids, cur_len, n, m, sep, sup)), name
    if V == 30522:
        assert k.ld == 1908 and V % 16 == 10
    if V == 131072:
        assert k.ld == 8192                                                  # the whole LDS bitmap, every word stored
    view = k.buf[:ROWS * k.ld]
    assert lib.gitcap_dbg_ban_mask_rec(ptr(ids), ids.shape[1], ROWS, 4, 2, None, V, ptr(view), k.ld, stream()) == -1           # no record
    assert lib.gitcap_dbg_ban_mask_rec(ptr(ids), ids.shape[1], ROWS, 4, 2, ptr(k.rec), V, ptr(view), k.ld - 1, stream()) == -1  # odd / short ld
    assert lib.gitcap_dbg_ban_mask_rec(ptr(ids), ids.shape[1], ROWS, 13, 2, ptr(k.rec), V, ptr(view), k.ld, stream()) == -1     # cur_len > ld_ids
    assert lib.gitcap_dbg_ban_mask_rec(ptr(ids), ids.shape[1], ROWS, 4, 2, ptr(k.rec), 131073, ptr(view), k.ld, stream()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("V", [97, 30522])
def test_rules_are_read_when_the_kernel_runs(lib, V):
    """The same launch arguments twice, the record rewritten in between: two different masks, each the restatement's."""
    k = _Masks(lib, V)
    cases = C.builder_cases(V)
    _, p, cur_len, _, _, sep, _ = cases[0]
    ids = to_dev(p, torch.int64)
    seen = []
    for n, m, sup in ((3, 12, [0, 15, 16, V - 1]), (1, 0, []), (0, 0, [7]), (2, cur_len, [V - 2, V - 2]), (0, 0, [])):
        k.write_record(S.pack_record(n, m, sup, fill=5))
        got = k.run_rec(ids, cur_len, sep)
        assert np.array_equal(got, C.ban_mask(p, cur_len, n, m, sep, sup, V, k.ld)), (n, m, sup)
        seen.append(got.copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]) and not seen[4].any()


@pytest.mark.parametrize("V", [97, 30522])
def test_full_list_and_a_count_beyond_the_record(lib, V):
    k = _Masks(lib, V)
    _, p, cur_len, _, _, sep, _ = C.builder_cases(V)[1]
    ids = to_dev(p, torch.int64)
    # 256 ids: duplicates, ids outside the vocabulary, the last entry a column no other entry names
    sup = [6 + (11 * i) % (V - 12) if i % 5 else (V + i if i % 2 else -1 - i) for i in range(255)] + [V - 3]      # in-vocabulary ids in 6 .. V - 7
    sup[21] = sup[11]
    assert len(sup) == 256 and len(set(sup)) < 256 and V - 3 not in sup[:255] and 5 not in sup
    want = C.ban_mask(p, cur_len, 0, 0, sep, sup, V, k.ld)
    assert (int(want[0, (V - 3) >> 4]) >> ((V - 3) & 15)) & 1 and not (int(want[0, 0]) >> 5) & 1
    k.write_record(S.pack_record(0, 0, sup))
    full = k.run_rec(ids, cur_len, sep)
    assert np.array_equal(full, want)
    assert np.array_equal(full, k.run_args(ids, cur_len, 0, 0, sep, sup))
    for count in (300, 257, 1 << 30):                                        # behaves as 256: column 5 behind the record stays clear
        k.write_record(S.pack_record(0, 0, sup, n_suppress=count))
        assert np.array_equal(k.run_rec(ids, cur_len, sep), want), count
    k.write_record(S.pack_record(0, 0, sup, n_suppress=-7))                  # and a negative count as 0
    assert not k.run_rec(ids, cur_len, sep).any()
    # garbage rule words ban nothing and read nothing
    k.write_record(S.pack_record(-3, -9, []))
    assert not k.run_rec(ids, cur_len, sep).any()
    k.write_record(S.pack_record(1 << 30, 0, []))
    assert not k.run_rec(ids, cur_len, sep).any()


# ---- b. the BAN head at the student's widths ---------------------------------------------------------------------------------------

def _run_banned(lib, X, W, bias, M, N, K, mask, lse, share):
    nt = (N + 15) // 16
    logits, val = poisoned(M * N + 16, NAN), poisoned(M * nt + 16, NAN)
    idx, ssum = poisoned(M * nt + 16, IDX_FILL, torch.int32), poisoned(M * nt + 16, NAN)
    old = lib.gitcap_dbg_config(10, share)
    try:
        rc = lib.gitcap_dbg_vocab_head_banned(ptr(X), K, ptr(W), None, ptr(bias), M, N, K, ptr(logits), ptr(val), ptr(idx),
                                              ptr(ssum) if lse else None, ptr(mask), mask.shape[1], stream())
        torch.cuda.synchronize()
    finally:
        lib.gitcap_dbg_config(10, old)
    assert rc == 0
    assert_tail(logits, M * N, NAN); assert_tail(val, M * nt, NAN); assert_tail(idx, M * nt, IDX_FILL)
    assert_tail(ssum, M * nt if lse else 0, NAN)
    return logits[:M * N].view(M, N), val[:M * nt].view(M, nt), idx[:M * nt].view(M, nt), ssum[:M * nt].view(M, nt) if lse else None


def _masks(lg, N):
    """Every row but those with m % 3 == 1 of a launch of more than two rows: the maximum of every other tile (the runner-up must
    win), the whole of tile 1, the row maximum and the edge columns."""
    M, nt = lg.shape[0], (N + 15) // 16
    mask = np.zeros((M, C.mask_ld(N)), np.uint16)
    for m in range(M):
        if M > 2 and m % 3 == 1:
            continue
        cols = [t * 16 + int(np.argmax(lg[m, t * 16:min(N, t * 16 + 16)])) for t in range(m % 2, nt, 2)]
        cols += list(range(16, 32)) + [0, 15, N - 1, int(np.argmax(lg[m]))]
        for c in cols:
            mask[m, c >> 4] |= np.uint16(1 << (c & 15))
    return mask


def _head_case(lib, M, N, K, share=1):
    X, W, _, bias = softmax_head_inputs(M, N, K, False, seed=9300 + 10 * M + N + K)
    plain = run_vocab_head(lib, X, K, W, None, bias, M, N, K, share=share, hook="lse")
    lg = plain.logits.cpu().numpy()
    mask = _masks(lg, N)
    dmask = to_dev(mask.view(np.int16), torch.int16)
    want = C.mask_logits(lg, mask)
    assert all(np.isinf(want[m, int(np.argmax(lg[m]))]) and np.isinf(want[m, 16:32]).all() for m in range(M) if not (M > 2 and m % 3 == 1))
    rv, ri, rs = L.tile_partials(want)
    sv, si = R.tile_partials(want)
    want_tok, want_lp = L.token_logprobs(want)
    for lse in (False, True):
        logits, val, idx, ssum = _run_banned(lib, X, W, bias, M, N, K, dmask, lse, share)
        assert np.array_equal(logits.cpu().numpy().view(np.uint32), want.view(np.uint32))     # -inf at the banned columns, the rest untouched
        dv, di = val.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
        assert np.array_equal(dv, rv) and np.array_equal(di, ri) and np.array_equal(dv, sv) and np.array_equal(di, si)
        assert [R.argmax_partials(dv[m], di[m]) for m in range(M)] == want_tok.tolist()
        for m in range(M):
            if M > 2 and m % 3 == 1:                                                          # nothing banned: the plain head's bits
                assert torch.equal(val[m], plain.val[m]) and torch.equal(idx[m], plain.idx[m]) and torch.equal(logits[m], plain.logits[m])
                assert not lse or torch.equal(ssum[m], plain.sum[m])
            else:
                assert dv[m, 1] == NINF and di[m, 1] == L.SENTINEL and want_tok[m] != int(np.argmax(lg[m]))
        if lse:
            ds = ssum.cpu().numpy().astype(np.float64)
            empty = rv == NINF
            assert (ds[empty] == 0.0).all() and not np.isnan(ds).any()
            rel = float((np.abs(ds[~empty] - rs[~empty]) / rs[~empty]).max())
            lp = np.array([L.merge(dv[m], di[m], ds[m])[1] for m in range(M)])
            err = float(np.abs(lp - want_lp).max())
            print(f"BAN head M={M} N={N} K={K} share={share}: max relative error of a tile sum {rel:.3e}, max |lp - fp64| {err:.3e}")
            assert rel <= TOL and err <= TOL


@pytest.mark.parametrize("M", [1, 2, 17])
def test_head_banned_tiny_student(lib, M):
    """K = 64, V = 97: seven tiles, the last one a single valid column"""
    _head_case(lib, M, 97, 64)


@pytest.mark.parametrize("M", [1, 2, 17])
def test_head_banned_student_decoder(lib, M):
    """K = 576, V = 30522: 1908 tiles, a ragged last tile of 10 columns"""
    _head_case(lib, M, 30522, 576)


def test_head_banned_single_wave_form_at_the_student_width(lib):
    _head_case(lib, 17, 97, 64, share=0)
