"""Caption scoring on the MI355X, kernel by kernel through the gitcap_dbg_vocab_head_score / gitcap_dbg_score_final hooks:

  a. the head with target capture (skinny.hip: logits_epilogue<true, true>): tgt_logit bit for bit the logit gitcap_dbg_vocab_head
     writes for that element, the three partials bit for bit those of gitcap_dbg_vocab_head_lse, rows whose target is out of range
     untouched, both head forms, both weight storages, bitwise invariance to the rows in the launch and to the head form;
  b. score_final on hand-made partials against the fp64 restatement of tests/score_reference.py.

Tolerance of a token log-probability, derived and not measured: lp = fl(fl(y_t - M) + lp_winner).  lp_winner carries the 2e-5 nats
tests/test_logprob_gpu.py derives for the merged sums.  The two new operations are one rounded fp32 subtraction and one rounded
fp32 add; y_t - M <= 0 and lp_winner <= 0 (up to its own error), so both magnitudes are at most |lp| and each rounding is at most
2^-24 |lp|: 2e-5 + 2^-23 |lp_ref|, absolute (score_reference.bound_lp) -- the estimate of the feature's description, confirmed.
row_sum adds T - 1 such terms with one accumulator: the terms' bounds plus (T - 1) * 2^-24 * sum |lp| (score_reference.bound_sum).
row_cnt, top1_ids and the -inf pattern are exact; top1_lp is bit for bit gitcap_dbg_argmax_final_lp's."""
import numpy as np
import pytest
import torch

import logprob_reference as L
import score_reference as S
from gpu_support import TGT_FILL, lib, ptr, run_vocab_head, softmax_head_inputs, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

NINF = float("-inf")
SENT = TGT_FILL                 # pre-fill of tgt_logit
IGN = 7                         # the ignore_id the head must NOT know about (score_final's business)


def _targets(M, N, logits):
    """One target per row, cycling through: column 0, N - 1, the tile edge 15 | 16, inside the last (tail) tile, the row's arg-max,
    a -inf column (bias), and -1, N, N + 3, IGN."""
    am = logits.argmax(dim=1).cpu().numpy()
    ninf_col = int(torch.isinf(logits[0]).nonzero()[0]) if bool(torch.isinf(logits[0]).any()) else 1
    tail = (N - 1) // 16 * 16 + min(2, (N - 1) % 16)
    pool = [0, N - 1, min(15, N - 1), min(16, N - 1), tail, None, ninf_col, -1, N, N + 3, IGN]
    return np.array([int(am[m]) if pool[m % len(pool)] is None else pool[m % len(pool)] for m in range(M)], dtype=np.int64)


def _head_score_case(lib, M, N, K, fp8):
    X, W, wscale, bias = softmax_head_inputs(M, N, K, fp8, seed=9000 + 100 * M + N + K)
    bias[3 if N > 3 else 1] = NINF
    lg, val0, idx0, sum0 = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, hook="lse")[:4]              # the logits and partials of the existing hooks
    targets = _targets(M, N, lg)
    inr = (targets >= 0) & (targets < N)
    want = torch.full((M,), SENT, device="cuda")
    rows = torch.as_tensor(np.nonzero(inr)[0], device="cuda")
    want[rows] = lg[rows, torch.as_tensor(targets[inr], device="cuda")]
    res = {}
    for share in (1, 0):
        _, val, idx, ssum, tl = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, share=share, hook="score", targets=targets, want_logits=False)
        assert torch.equal(val, val0) and torch.equal(idx, idx0) and torch.equal(ssum, sum0), share
        assert torch.equal(tl.view(torch.int32), want.view(torch.int32)), (share, tl, want)      # bit for bit; untouched where out of range
        res[share] = tl
    assert bool(torch.isinf(want).any()) or M < 7                                    # the -inf column is among the targets
    # with a logits buffer the launch writes the same logits as the hook without targets
    lg2, _, _, _, tl2 = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, hook="score", targets=targets)
    assert torch.equal(lg2, lg) and torch.equal(tl2.view(torch.int32), want.view(torch.int32))
    # the rows beside a row do not matter: every row launched alone, in both forms
    for m in sorted({0, M - 1, min(M - 1, 15), min(M - 1, 16)}):
        for share in (1, 0):
            _, v1, i1, s1, t1 = run_vocab_head(lib, X[m:m + 1].contiguous(), K, W, wscale, bias, 1, N, K, share=share, hook="score", targets=targets[m:m + 1],
                                               want_logits=False)
            assert torch.equal(v1, val0[m:m + 1]) and torch.equal(s1, sum0[m:m + 1]) and torch.equal(t1.view(torch.int32), want[m:m + 1].view(torch.int32))


@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("N,K,fp8", [(16, 64, False), (77, 64, False), (16, 128, False), (77, 128, False), (77, 128, True), (16, 128, True)])
def test_head_target_capture(lib, M, N, K, fp8):
    """M: one, two and three m-tiles, each with a tail.  N = 16: one tile (never the shared form); 77: five tiles -- two workgroups,
    the second with one active wave and a 13-column tail tile.  e4m3 weights at K = 128."""
    _head_score_case(lib, M, N, K, fp8)


def test_head_score_hook_rejects_bad_arguments(lib):
    x = torch.zeros(16, 64, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(64, device="cuda")
    i = torch.zeros(64, device="cuda", dtype=torch.int32)
    t = torch.zeros(4, device="cuda", dtype=torch.int64)
    assert lib.gitcap_dbg_vocab_head_score(ptr(x), 64, ptr(x), None, None, 1, 16, 64, None, ptr(f), ptr(i), ptr(f), None, ptr(f), None) == -1
    assert lib.gitcap_dbg_vocab_head_score(ptr(x), 64, ptr(x), None, None, 1, 16, 64, None, ptr(f), ptr(i), ptr(f), ptr(t), None, None) == -1
    assert lib.gitcap_dbg_vocab_head_score(ptr(x), 64, ptr(x), None, None, 1, 16, 64, None, ptr(f), ptr(i), None, ptr(t), ptr(f), None) == -1
    assert lib.gitcap_dbg_score_final(ptr(f), ptr(i), ptr(f), 1, ptr(f), ptr(t), 2, 1, 2, None, -1, 16, None, 1, None, None, None, None, None) == -1
    assert lib.gitcap_dbg_score_final(ptr(f), ptr(i), ptr(f), 1, ptr(f), ptr(t), 2, 1, 1, None, -1, 16, ptr(f), 1, None, None, None, None, None) == -1   # T < 2
    assert lib.gitcap_dbg_score_final(ptr(f), ptr(i), ptr(f), 1, ptr(f), ptr(t), 1, 1, 2, None, -1, 16, ptr(f), 1, None, None, None, None, None) == -1   # ld_ids < T


# ---- b. score_final on hand-made partials -----------------------------------------------------------------------------------

def _final_inputs(nt, T, use_lengths):
    """Hand-made partials, target logits, ids and lengths of one case, the fp64 result, and the checks that the INPUTS cover what
    the case is for (host only: nothing here looks at a device value)."""
    rng = np.random.default_rng(17 * nt + T + use_lengths)
    V = 16 * nt - 3 if nt > 1 else 13
    base = np.arange(nt, dtype=np.int64) * 16 + 5

    def fresh(spread=1.0):
        v = (rng.permutation(nt).astype(np.float32) / nt - 2.0) * np.float32(spread)
        return v, base.copy(), (1.0 + 15.0 * rng.random(nt)).astype(np.float32)

    def make(kind):
        v, i, s = fresh(8.0 if kind == 1 else 1.0)
        if kind == 2:
            v[:] = 1.0                                                            # all tiles tie: the first index
        elif kind == 3 and nt > 1:
            dead = np.arange(1, nt, 3)
            dead = dead[dead != int(np.argmax(v))]
            v[dead], i[dead], s[dead] = NINF, L.SENTINEL, 0.0                     # -inf tiles
        elif kind == 4:
            v[:], i[:], s[:] = NINF, L.SENTINEL, 0.0                              # an all -inf row
        return v, i, s
    R = 4
    val = np.zeros((R * T, nt), np.float32); idx = np.zeros((R * T, nt), np.int64); ssum = np.zeros((R * T, nt), np.float32)
    tgt = np.full(R * T, np.nan, np.float32)                                      # never-written target logits stay poison
    y = np.zeros((R, T), np.int64); y[:, 0] = 101
    for r in range(R):
        for j in range(T):
            m = r * T + j
            kind = (r + j) % 5
            val[m], idx[m], ssum[m] = make(kind)
            if j + 1 < T:
                c = [3, V - 1, IGN, -1, V, V + 3][(2 * r + j) % 6] if (r + j) % 3 == 0 else int(rng.integers(0, V))
                y[r, j + 1] = c
                if 0 <= c < V:            # what the head captured: at most the row's maximum; -inf on an all -inf row and now and then
                    M = val[m].max()
                    tgt[m] = NINF if (kind == 4 or (r + j) % 7 == 3) else (M if (r + j) % 4 == 1 else M - np.float32(20.0 * rng.random()))
    lengths = np.array([1, 2, T, max(1, T - 1)], dtype=np.int64) if use_lengths else None
    want = S.score_partials(val, idx, ssum, tgt, y, lengths, IGN, V)
    ok = S.counted(y, lengths, IGN, V)
    if T > 2:               # (T = 2 is the shortest caption: four positions, too few to hold every kind)
        assert np.isneginf(want["token_lp"]).any() and (~ok).any() and ok.any()
    if use_lengths:         # lengths 1: nothing counted; 2: the first position at most
        assert want["count"][0] == 0 and want["sum"][0] == 0.0 and want["count"][1] <= 1
    return V, val, idx, ssum, tgt, y, lengths, want, ok


def _final_case(lib, nt, T, use_lengths):
    V, val, idx, ssum, tgt, y, lengths, want, ok = _final_inputs(nt, T, use_lengths)
    R = y.shape[0]
    ld_ids, ld_lp = T + 2, T + 1
    yp = np.full((R, ld_ids), 3, np.int64); yp[:, :T] = y
    d_val, d_idx, d_sum, d_tgt, d_y = to_dev(val, torch.float32), to_dev(idx, torch.int32), to_dev(ssum, torch.float32), to_dev(tgt, torch.float32), to_dev(yp, torch.int64)
    d_len = to_dev(lengths, torch.int32) if use_lengths else None
    lp = torch.full((R, ld_lp), float("nan"), device="cuda")
    rsum = torch.full((R + 1,), float("nan"), device="cuda")
    rcnt = torch.full((R + 1,), -9, device="cuda", dtype=torch.int32)
    t1 = torch.full((R * (T - 1) + 1,), -9, device="cuda", dtype=torch.int64)
    t1lp = torch.full((R * (T - 1) + 1,), float("nan"), device="cuda")
    rc = lib.gitcap_dbg_score_final(ptr(d_val), ptr(d_idx), ptr(d_sum), nt, ptr(d_tgt), ptr(d_y), ld_ids, R, T, ptr(d_len), IGN, V,
                                    ptr(lp), ld_lp, ptr(rsum), ptr(rcnt), ptr(t1), ptr(t1lp), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(lp[:, T - 1:]).all()) and bool(torch.isnan(rsum[R:]).all()) and int(rcnt[R]) == -9 and int(t1[-1]) == -9
    # top-1: bit for bit the greedy loop's arg-max launch on the same partials
    out = torch.full((R * T,), -9, device="cuda", dtype=torch.int64)
    alp = torch.full((R * T,), float("nan"), device="cuda")
    assert lib.gitcap_dbg_argmax_final_lp(ptr(d_val), ptr(d_idx), nt, R * T, 1, 0, ptr(out), 1, None, 0, -1, None, ptr(d_sum), ptr(alp), 1, stream()) == 0
    torch.cuda.synchronize()
    keep = torch.as_tensor([r * T + j for r in range(R) for j in range(T - 1)], device="cuda")
    assert torch.equal(t1[:-1], out[keep]) and torch.equal(t1lp[:-1].view(torch.int32), alp[keep].view(torch.int32))
    assert t1[:-1].cpu().numpy().reshape(R, T - 1).tolist() == want["top1_ids"].tolist()
    g = lp[:, :T - 1].cpu().numpy().astype(np.float64)
    w = want["token_lp"]
    assert not np.isnan(g).any() and np.array_equal(np.isneginf(g), np.isneginf(w))
    fin = np.isfinite(w)
    err = np.abs(g[fin] - w[fin])
    if fin.any():
        print(f"score_final nt={nt} T={T} lengths={use_lengths}: lp {w[fin].min():.3f} .. {w[fin].max():.3f}, max |device - fp64| {err.max():.3e}")
    assert (err <= S.bound_lp(w[fin])).all()
    assert (g[~ok] == 0.0).all()                                                   # ignored positions: exactly 0
    assert rcnt[:R].cpu().numpy().tolist() == want["count"].tolist() == ok.sum(1).tolist()
    gs = rsum[:R].cpu().numpy().astype(np.float64)
    for r in range(R):
        if np.isfinite(want["sum"][r]):
            print(f"     row {r}: sum {want['sum'][r]:.4f} count {want['count'][r]} |device - fp64| {abs(gs[r] - want['sum'][r]):.3e}")
            assert abs(gs[r] - want["sum"][r]) <= S.bound_sum(w[r][ok[r]])
        else:
            assert gs[r] == want["sum"][r]
    if use_lengths:
        assert gs[0] == 0.0                                                        # lengths 1: nothing counted
    # nullable outputs: token_lp alone gives the same values
    lp2 = torch.full((R, ld_lp), float("nan"), device="cuda")
    assert lib.gitcap_dbg_score_final(ptr(d_val), ptr(d_idx), ptr(d_sum), nt, ptr(d_tgt), ptr(d_y), ld_ids, R, T, ptr(d_len), IGN, V,
                                      ptr(lp2), ld_lp, None, None, None, None, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(lp2[:, :T - 1].view(torch.int32), lp[:, :T - 1].view(torch.int32))


@pytest.mark.parametrize("use_lengths", [False, True])
@pytest.mark.parametrize("nt,T", [(1, 2), (5, 7), (258, 5), (1908, 4)])
def test_score_final_hand_made_partials(lib, nt, T, use_lengths):
    """One tile and the shortest caption; a few tiles; a remainder of two past one tile per thread; the 30522-word vocabulary.
    Ties, -inf tiles, all -inf rows, -inf target logits, targets at -1, V, V + 3 and ignore_id, lengths 1, 2, T - 1 and T,
    row pitches that are not the identity, poison around every output."""
    _final_case(lib, nt, T, use_lengths)


def test_score_final_is_independent_of_the_rows_beside_it(lib):
    nt, T, V = 258, 4, 4100
    rng = np.random.default_rng(3)
    R = 3
    val = (rng.random((R * T, nt)).astype(np.float32) - 2.0); idx = np.tile(np.arange(nt) * 16 + 1, (R * T, 1))
    ssum = (1.0 + 15.0 * rng.random((R * T, nt))).astype(np.float32)
    tgt = (val.max(1) - rng.random(R * T).astype(np.float32) * 9.0).astype(np.float32)
    y = rng.integers(0, V, (R, T)).astype(np.int64)

    def run(r0, r1):
        n = r1 - r0
        a = [to_dev(x[r0 * T:r1 * T], t) for x, t in ((val, torch.float32), (idx, torch.int32), (ssum, torch.float32), (tgt, torch.float32))]
        lp = torch.zeros((n, T - 1), device="cuda"); rs = torch.zeros((n,), device="cuda")
        assert lib.gitcap_dbg_score_final(ptr(a[0]), ptr(a[1]), ptr(a[2]), nt, ptr(a[3]), ptr(to_dev(y[r0:r1], torch.int64)), T, n, T, None, -1, V,
                                          ptr(lp), T - 1, ptr(rs), None, None, None, stream()) == 0
        torch.cuda.synchronize()
        return lp.view(torch.int32), rs.view(torch.int32)
    lp, rs = run(0, R)
    for r in range(R):
        l1, s1 = run(r, r + 1)
        assert torch.equal(l1[0], lp[r]) and torch.equal(s1[0], rs[r])
