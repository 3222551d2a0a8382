"""Plain numpy restatement, in fp64, of how given captions are scored without a logits tensor (include/gitcap.h: gitcap_score;
csrc/skinny.hip: logits_epilogue<true, true>, csrc/select.hip: score_final_kernel / score_rows_kernel), built on
tests/logprob_reference.py:

  the scoring head leaves the three per-tile partials of every (row, position) and the one logit of the position's given next
  token y[r][j + 1]; the merge forms the winner and its log-probability as the greedy loop does (logprob_reference.merge) and
      lp[r][j] = (y_t - M) - log(total) = (y_t - M) + lp_winner,   -inf for a -inf target logit;
  a position is ignored (lp 0, not counted) when its target lies outside [0, V), equals ignore_id, or j + 1 >= lengths[r];
  row_sum adds the counted positions in ascending position order.

``wrong`` names one deliberately wrong variant (tests/test_score.py shows that the test inputs tell each from the right one):
  "target_shift"  the target taken from y[r][j] instead of y[r][j + 1]
  "drop_tail"     the ragged last tile left out of the partials
  "length_off"    the lengths rule off by one (j + 1 > lengths[r])
  "ignore_counted" ignore_id counted like any token
  "sum_all"       row_sum / row_cnt over every position whose target is a word, whatever lengths and ignore_id say
"""
import numpy as np

import logprob_reference as L


def counted(y, lengths, ignore_id, V, wrong=None):
    """y int64 [R][T] -> bool [R][T - 1]."""
    y = np.asarray(y, dtype=np.int64)
    R, T = y.shape
    tgt = y[:, 1:]
    ok = (tgt >= 0) & (tgt < V)
    if wrong != "ignore_counted":
        ok &= tgt != ignore_id
    if lengths is not None:
        j1 = np.arange(1, T)[None, :]
        ln = np.asarray(lengths, dtype=np.int64)[:, None]
        ok &= (j1 <= ln) if wrong == "length_off" else (j1 < ln)
    return ok


def score_partials(val, idx, ssum, tgt_logit, y, lengths=None, ignore_id=-1, V=None, wrong=None):
    """Partials [R * T][ntiles] and target logits [R * T] by head row m = r * T + j -> dict of token_lp fp64 [R][T - 1], sum [R],
    count [R], top1_ids [R][T - 1], top1_lp [R][T - 1]."""
    y = np.asarray(y, dtype=np.int64)
    R, T = y.shape
    ok = counted(y, lengths, ignore_id, V, wrong)
    lp = np.zeros((R, T - 1))
    raw = np.zeros((R, T - 1))
    t1 = np.zeros((R, T - 1), dtype=np.int64)
    t1lp = np.zeros((R, T - 1))
    for r in range(R):
        for j in range(T - 1):
            m = r * T + j
            t1[r, j], t1lp[r, j] = L.merge(val[m], idx[m], ssum[m])
            word = 0 <= y[r, j + 1] < V
            if ok[r, j] or (wrong == "sum_all" and word):
                yt = float(tgt_logit[m])
                M = float(np.max(np.asarray(val[m], dtype=np.float64)))
                raw[r, j] = -np.inf if yt == -np.inf else (yt - M) + t1lp[r, j]
            if ok[r, j]:
                lp[r, j] = raw[r, j]
    tot = np.zeros(R)
    cnt = np.zeros(R, dtype=np.int64)
    for r in range(R):
        for j in range(T - 1):                              # ascending positions, one accumulator
            take = (0 <= y[r, j + 1] < V) if wrong == "sum_all" else ok[r, j]
            if take:
                tot[r] += raw[r, j]
                cnt[r] += 1
    return dict(token_lp=lp, sum=tot, count=cnt, top1_ids=t1, top1_lp=t1lp)


def score_logits(logits, y, lengths=None, ignore_id=-1, wrong=None):
    """logits [R][T][V] (any float; finite or -inf), y int64 [R][T] -> score_partials' dict, through the partials."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    R, T, V = x.shape
    flat = x.reshape(R * T, V)
    val, idx, ssum = L.tile_partials(flat[:, :V // L.TILE * L.TILE] if wrong == "drop_tail" and V % L.TILE and V > L.TILE else flat)
    tgt = np.full(R * T, np.nan)                             # what the head never wrote stays poison
    for r in range(R):
        for j in range(T - 1):
            c = y[r, j] if wrong == "target_shift" else y[r, j + 1]
            if 0 <= c < V:
                tgt[r * T + j] = flat[r * T + j, c]
    return score_partials(val, idx, ssum, tgt, y, lengths, ignore_id, V, wrong)


def bound_lp(lp_ref):
    """|device - fp64| allowed for a token log-probability: 2e-5 nats for the merged sums (tests/test_logprob_gpu.py) plus the two
    rounded fp32 operations of the target term, y_t - M and the add, each 2^-24 relative on a magnitude of at most |lp|."""
    a = np.abs(np.asarray(lp_ref, dtype=np.float64))
    return 2e-5 + 2.0 ** -23 * np.where(np.isfinite(a), a, 0.0)


def bound_sum(lp_ref_row):
    """The same per term, plus the T - 1 rounded fp32 adds of the row: (T - 1) * 2^-24 * sum |lp|."""
    a = np.abs(np.asarray(lp_ref_row, dtype=np.float64))
    a = np.where(np.isfinite(a), a, 0.0)
    return float(bound_lp(a).sum() + a.size * 2.0 ** -24 * a.sum())
