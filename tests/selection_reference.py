"""Restatement of the token-selection kernels in numpy fp64 / plain Python, written from their contracts (csrc/kernels.h,
the comments above the kernels in csrc/rowops.hip and csrc/skinny.hip), for tests/test_selection.py and
tests/test_selection_gpu.py.

The rule everywhere: the largest value wins, the smallest index among equals.  Inputs must be free of NaN."""
import numpy as np

SENTINEL = 0x7FFFFFFF          # index of a slot that holds no candidate (its value is -inf)
TILE = 16                      # columns per arg-max partial of the vocabulary head


def argmax_first(row):
    """First occurrence of the maximum of a 1-d row; an empty row, or one without a value above -inf, gives 0."""
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    assert not np.isnan(row).any()
    best, bi = -np.inf, 0
    for i, v in enumerate(row.tolist()):
        if v > best:
            best, bi = v, i
    return bi


def tile_partials(logits):
    """logits [M][N] -> (val fp64 [M][ntiles], idx int64 [M][ntiles]): per 16-column tile the largest logit and the first
    column (of the whole row) that holds it; a tile without a value above -inf has idx SENTINEL."""
    x = np.asarray(logits, dtype=np.float64)
    assert x.ndim == 2 and not np.isnan(x).any()
    M, N = x.shape
    nt = (N + TILE - 1) // TILE
    pad = np.full((M, nt * TILE), -np.inf)
    pad[:, :N] = x
    t = pad.reshape(M, nt, TILE)
    val = t.max(axis=2)
    idx = t.argmax(axis=2).astype(np.int64) + np.arange(nt, dtype=np.int64)[None, :] * TILE      # np.argmax: first occurrence
    idx[val == -np.inf] = SENTINEL
    return val, idx


def argmax_partials(val, idx):
    """The token of one row from its partials: among the partials with the largest value the smallest idx; SENTINEL (nothing
    above -inf anywhere) or an empty row -> 0."""
    val = np.asarray(val, dtype=np.float64).reshape(-1)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    assert val.shape == idx.shape and not np.isnan(val).any()
    if val.size == 0:
        return 0
    tok = int(idx[val == val.max()].min())
    return 0 if tok == SENTINEL else tok


def draft_accept(tok, ids, sep_id):
    """tok [B][n]: the model's token after draft positions 0..j of caption r; ids [B][ld]: column 0 = CLS, columns 1..n = the
    staged draft (-1 = no word).  Returns a dict:
      a_r      [B] leading positions of row r whose token equals the draft's next token ids[r][j + 1]
      a        min over the rows (the loop advances all rows in lockstep)
      covered  a + 1 steps when a < n (the token at position a is the model's own), else n
      ids      a copy with columns 1..covered replaced by the model's tokens; everything else as it was
      sep_cnt  [covered] rows whose token at step t is sep_id
      host     (a, 1 if all rows emitted sep_id in one of the covered steps else 0)"""
    tok = np.asarray(tok, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    B, n = tok.shape
    assert ids.shape[0] == B and ids.shape[1] >= n + 1 and 1 <= n
    a_r = []
    for r in range(B):
        j = 0
        while j < n and tok[r, j] == ids[r, j + 1]:
            j += 1
        a_r.append(j)
    a = min(a_r)
    covered = a + 1 if a < n else n
    out = ids.copy()
    out[:, 1:covered + 1] = tok[:, :covered]
    sep_cnt = [int((tok[:, t] == sep_id).sum()) for t in range(covered)]
    return {"a_r": a_r, "a": a, "covered": covered, "ids": out, "sep_cnt": sep_cnt,
            "host": (a, 1 if any(c == B for c in sep_cnt) else 0)}


def beam_candidates(logits, beam_scores, beams, K):
    """logits [B*beams][V], beam_scores [B*beams] -> (scores fp64 [B][K], idx int64 [B][K], gap [B]).
    Candidate (j, v) of clip b scores log_softmax(logits[b*beams + j])[v] + beam_scores[b*beams + j] in fp64 (the softmax over
    the finite logits of the row); non-finite logits are no candidates.  The K best under a stable sort on (descending score,
    ascending flat index j*V + v); slots past the last candidate hold (-inf, SENTINEL).
    gap[b]: the smallest difference between DISTINCT consecutive scores among the first K + 1 candidates (inf when there are
    none) -- how far the inputs keep the order away from fp32 rounding; exact ties are the designed ones and do not count."""
    x = np.asarray(logits, dtype=np.float64)
    bs = np.asarray(beam_scores, dtype=np.float64).reshape(-1)
    assert x.ndim == 2 and x.shape[0] % beams == 0 and bs.shape[0] == x.shape[0] and not np.isnan(x).any()
    R, V = x.shape
    B = R // beams
    fin = np.isfinite(x)
    sc = np.full(x.shape, -np.inf)
    for r in range(R):
        f = x[r][fin[r]]
        if f.size:
            m = f.max()
            sc[r][fin[r]] = f - (m + np.log(np.exp(f - m).sum())) + bs[r]
    scores = np.full((B, K), -np.inf)
    idx = np.full((B, K), SENTINEL, dtype=np.int64)
    gap = np.full(B, np.inf)
    for b in range(B):
        flat = sc[b * beams:(b + 1) * beams].reshape(-1)
        valid = fin[b * beams:(b + 1) * beams].reshape(-1)
        order = np.argsort(-flat, kind="stable")                  # stable: equal scores keep ascending flat index
        order = order[valid[order]][:K + 1]
        k = min(K, order.size)
        scores[b, :k] = flat[order[:k]]
        idx[b, :k] = order[:k]
        d = -np.diff(flat[order])
        d = d[d > 0]
        if d.size:
            gap[b] = d.min()
    return scores, idx, gap
