"""Plain numpy restatement, in fp64, of how the greedy loops get the log-probability of the token they emit without a logits
tensor (csrc/skinny.hip: logits_epilogue, csrc/lp_partials.h: lp_partials):

  the vocabulary head leaves three partials per 16-column tile of a row: the largest logit, the first column that holds it, and
  the sum of exp(logit - that maximum) over the tile's columns (0 for a tile with no logit above -inf);
  the arg-max launch picks the winner (largest value, smallest index among equals) and merges the sums:
      lp = -log(sum_t sum[t] * exp(max[t] - M)),  M = the winner's logit = log_softmax(logits)[winner].
"""
import numpy as np

SENTINEL = 0x7FFFFFFF          # index of a tile that holds no logit above -inf
TILE = 16


def tile_partials(logits):
    """logits [M][N] -> (val fp64, idx int64, sum fp64), each [M][ntiles]; the last tile may be ragged."""
    x = np.asarray(logits, dtype=np.float64)
    assert x.ndim == 2 and not np.isnan(x).any()
    M, N = x.shape
    nt = (N + TILE - 1) // TILE
    val = np.full((M, nt), -np.inf)
    idx = np.full((M, nt), SENTINEL, dtype=np.int64)
    ssum = np.zeros((M, nt))
    for m in range(M):
        for t in range(nt):
            seg = x[m, t * TILE:min(N, (t + 1) * TILE)]
            best = seg.max()
            if best == -np.inf:
                continue                                    # nothing above -inf: (-inf, SENTINEL, 0), never -inf - -inf
            val[m, t] = best
            idx[m, t] = t * TILE + int(np.argmax(seg))      # first occurrence
            ssum[m, t] = np.exp(seg - best).sum()
    return val, idx, ssum


def merge(val, idx, ssum):
    """One row's partials -> (token, lp): the token under the tie rule (0 for a row with nothing above -inf, whose lp is -inf)."""
    val = np.asarray(val, dtype=np.float64).reshape(-1)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    ssum = np.asarray(ssum, dtype=np.float64).reshape(-1)
    M = val.max() if val.size else -np.inf
    if M == -np.inf:
        return 0, -np.inf
    tok = int(idx[val == M].min())
    live = val > -np.inf                                    # -inf tiles are skipped
    total = float((ssum[live] * np.exp(val[live] - M)).sum())
    return (0 if tok == SENTINEL else tok), -np.log(total)


def token_logprobs(logits):
    """logits [M][N] -> (tokens int64 [M], lp fp64 [M]) through the partials."""
    val, idx, ssum = tile_partials(logits)
    out = [merge(val[m], idx[m], ssum[m]) for m in range(val.shape[0])]
    return np.array([t for t, _ in out], dtype=np.int64), np.array([l for _, l in out], dtype=np.float64)
