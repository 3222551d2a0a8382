"""Restatement of the token-selection kernels in numpy fp64 / plain Python, written from their contracts (csrc/kernels.h,
the comments above the kernels in csrc/select.hip, csrc/search.hip and csrc/skinny.hip), for tests/test_selection.py and
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


# ---- inputs of the draft_accept tests (tests/test_selection_gpu.py, tests/test_logprob_gpu.py) ----

DRAFT_NT, DRAFT_SEP, DRAFT_POISON = 5, 9, -777


def draft_scenario(B, n, a_rows, sep_at, rng):
    """Model tokens tok [B][n] with SEP at the (row, step) pairs of sep_at, and ids [B][ld] whose draft agrees with row r at
    exactly its first a_rows[r] positions (the first disagreement of row 0 is a staged -1); ld = n + 4."""
    vocab, ld = 16 * DRAFT_NT, n + 4
    tok = rng.integers(10, vocab, (B, n))
    for r, t in sep_at:
        tok[r, t] = DRAFT_SEP
    ids = np.full((B, ld), DRAFT_POISON, np.int64)
    ids[:, 0] = 1
    for r in range(B):
        for j in range(n):
            if j < a_rows[r] or (j > a_rows[r] and rng.random() < 0.5):
                ids[r, j + 1] = tok[r, j]
            elif j == a_rows[r] and r == 0:
                ids[r, j + 1] = -1
            else:
                ids[r, j + 1] = 10 + (tok[r, j] - 10 + 1 + rng.integers(0, vocab - 12)) % (vocab - 10)
                assert ids[r, j + 1] != tok[r, j]
    # partials that reduce to tok: the winner's tile holds 2.0 and the token; every second row has an equal value with a
    # larger index in another tile (the tie rule picks the token)
    val = rng.random((B * n, DRAFT_NT)).astype(np.float32)
    idx = np.arange(DRAFT_NT, dtype=np.int64)[None, :] * 16 + rng.integers(0, 16, (B * n, DRAFT_NT))
    for m in range(B * n):
        t = int(tok[m // n, m % n])
        val[m, t // 16], idx[m, t // 16] = 2.0, t
        if m % 2:
            o = (t // 16 + 1 + m % (DRAFT_NT - 1)) % DRAFT_NT
            val[m, o], idx[m, o] = 2.0, t + 1 + m % 3
    return tok, ids, val, idx


def draft_scenarios(B, n):
    mid = n // 2
    out = [([n] * B, [(r, n - 1) for r in range(B)]),                           # a = n; all rows SEP in the last step: fired
           ([0] + [n] * (B - 1), [(r, 0) for r in range(B)])]                   # a = 0; SEP at once in the model's own tokens
    if n >= 2:
        stair = [min(n, mid + r % 3) for r in range(B)]                         # rows disagree at different positions
        sep = [(r, mid + 1) for r in range(B)] if mid + 1 < n else []           # all rows, but beyond `covered`: not fired
        sep += [(r, r % (mid + 1)) for r in range(B)] if B > 1 else []          # inside `covered`, in different steps
        out.append((stair, sep))
        out.append(([n] * (B - 1) + [mid], []))                                 # the minimum sits in the last row
    return out


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
