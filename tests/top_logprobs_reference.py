"""Plain restatement of the top-k alternatives of a vocabulary-head row (include/gitcap.h: gitcap_attach_top_logprobs), the
inputs the kernel tests run on, and four WRONG kernels restated the same way, so that tests/test_top_logprobs.py can show
that those inputs tell each of them from the right answer.

The rule: columns with a logit above -inf are ranked by (logit descending, column ascending); rank j reports the column and
fp32(fp32(logit - M) + lp_winner), M = the row's largest logit, lp_winner = the winner's log-probability (-log z as the
selection kernels merge it).  Ranks the row cannot fill hold id -1 and lp -inf.

The inputs are built from small integers -- activations in {-1, 0, 1}, weights k / 64 with |k| <= 8 (bf16 and e4m3 hold them
exactly), biases and planted offsets in multiples of 1 / 16 -- so every product and every partial sum of a logit is exact in
fp32 in any order: the logits computed here ARE the device's logits, duplicated weight rows give equal logits, and ties are
plentiful without being planted (a 30522-column row of multiples of 1 / 64)."""
import numpy as np

NINF = np.float32(-np.inf)


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def ranked(logits):
    """columns with a logit above -inf, best first: (logit descending, column ascending)"""
    lg = np.asarray(logits, np.float32)
    cols = np.flatnonzero(lg > NINF)
    return cols[np.lexsort((cols, -lg[cols].astype(np.float64)))]


def top_k(logits, M, lp_winner, k):
    """-> (ids int64 [k], lp fp32 [k]) of one row of fp32 logits (a banned column is -inf)"""
    lg = np.asarray(logits, np.float32)
    order = ranked(lg)[:k]
    ids = np.full(k, -1, np.int64)
    lp = np.full(k, NINF, np.float32)
    ids[:len(order)] = order
    lp[:len(order)] = (lg[order] - np.float32(M)).astype(np.float32) + np.float32(lp_winner)
    return ids, lp


# ---- the kernel's plan, and four wrong ones -----------------------------------------------------------------------------------

def tile_plan_top_k(raw, V, ban, M, lp_winner, k, wrong=None):
    """The kernel's plan on one row: raw = the logits of all ceil(V / 16) * 16 weight rows, padding included, before the ban
    (bool [V], nullable).  The head's partial of a tile is its best allowed column < V; the k best tiles by (val descending, idx
    ascending) are recomputed and their candidates ranked.  wrong:
      "tile_ties"   tiles are picked by value alone (equal values: the LATER tile first, as a selection without the index would);
      "one_per_tile" only each picked tile's representative is a candidate;
      "padding"     the recomputed columns >= V are candidates;
      "no_ban"      the recomputed logits ignore the ban word."""
    raw = np.asarray(raw, np.float32)
    nt = len(raw) // 16
    head = raw.copy()
    head[V:] = NINF
    if ban is not None:
        head[:V][np.asarray(ban, bool)] = NINF
    reps = []                                           # (val, idx) of the non-empty tiles
    for t in range(nt):
        seg = head[16 * t:16 * t + 16]
        if (seg > NINF).any():
            c = int(np.argmax(seg))                     # first maximum: the smallest column among equals
            reps.append((float(seg[c]), 16 * t + c))
    reps.sort(key=(lambda r: (-r[0], -r[1])) if wrong == "tile_ties" else (lambda r: (-r[0], r[1])))
    cand = np.full(len(raw), NINF, np.float32)
    for val, idx in reps[:k]:
        t = idx // 16
        if wrong == "one_per_tile":
            cand[idx] = head[idx]
            continue
        seg = (raw if wrong == "no_ban" else head)[16 * t:16 * t + 16].copy()
        if wrong == "padding":
            seg = np.where(np.arange(16 * t, 16 * t + 16) >= V, raw[16 * t:16 * t + 16], seg)
        elif wrong == "no_ban":
            seg[np.arange(16 * t, 16 * t + 16) >= V] = NINF
        cand[16 * t:16 * t + 16] = seg
    return top_k(cand, M, lp_winner, k)


def winner_stats(logits):
    """(M, lp_winner) of a row in fp64, rounded to fp32 -- for the CPU tests; the GPU tests take the device's own"""
    lg = np.asarray(logits, np.float64)
    if not (lg > -np.inf).any():
        return NINF, NINF
    m = lg.max()
    return np.float32(m), np.float32(-np.log(np.exp(lg[lg > -np.inf] - m).sum()))


# ---- inputs -------------------------------------------------------------------------------------------------------------------

SCENARIOS = ("natural", "cluster", "spread", "ban_winner", "ban_keep3")


def _tiles(nt):
    step = max(1, (nt - 2) // 8)
    return [(1 + j * step) % nt for j in range(8)]


def head_case(M, V, D, scenario, seed=0):
    """-> dict(X fp32 [M, D], W fp32 [Vp, D], bias fp32 [V], ban bool [M, V] or None, logits fp32 [M, Vp]: the raw logits of every
    weight row, padding included and unbanned).  Scenarios:
      natural     nothing planted;
      cluster     five of every row's eight best in ONE tile, two of them from duplicated weight rows (equal logits inside a tile),
                  the other three in other tiles, two of those a duplicated pair (equal logits across tiles);
      spread      the eight best each in a tile of its own, ranks 1 and 2 a duplicated pair across tiles;
      ban_winner  cluster + a mask that bans every row's winner and one column in sixteen;
      ban_keep3   cluster + a mask that leaves three columns per row.
    With V no multiple of 16 the padded weight rows hold the largest values of the matrix, aligned with row 0."""
    assert scenario in SCENARIOS
    rng = np.random.default_rng(1000003 * seed + 7919 * M + 31 * V + D)
    Vp, nt = (V + 15) // 16 * 16, (V + 15) // 16
    X = rng.integers(-1, 2, size=(M, D)).astype(np.float32)
    W = (rng.integers(-8, 9, size=(Vp, D)) / 64.0).astype(np.float32)
    bias = (rng.integers(-16, 17, size=V) / 16.0).astype(np.float32)
    W[V:] = np.where(X[0] >= 0, 1.0, -1.0).astype(np.float32) * np.float32(8.0 / 64.0)
    tl = _tiles(nt)
    if scenario == "spread":
        cols = [16 * tl[j] + (3 * j) % 16 for j in range(7)] + [16 * (nt - 1) + 1]      # (the last one beside the padded rows)
        boost = [64.0, 50.0, 50.0, 40.0, 34.0, 28.0, 23.0, 18.0]     # (wider apart than the +-5 the random part reaches at D = 768)
        dups = [(1, 2)]
    elif scenario != "natural":
        cols = [16 * tl[0] + c for c in (1, 4, 6, 9, 15)] + [16 * (nt - 1) + 3, 16 * tl[2] + 5, 16 * tl[3] + 3]   # (one in the last tile)
        boost = [24.0, 23.0, 23.0, 22.0, 21.0, 23.5, 22.5, 22.5]
        dups = [(1, 2), (6, 7)]
    else:
        cols, boost, dups = [], [], []
    for a, b in dups:
        if cols[a] < V and cols[b] < V:
            W[cols[b]] = W[cols[a]]
    for c, bst in zip(cols, boost):
        if c < V:
            bias[c] = bst
    logits = (X.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    logits[:, :V] += bias[None, :]
    ban = None
    if scenario == "ban_winner":
        ban = np.zeros((M, V), bool)
        ban[:, rng.integers(0, 16)::16] = True
        ban[np.arange(M), np.argmax(logits[:, :V], axis=1)] = True
    elif scenario == "ban_keep3":
        ban = np.ones((M, V), bool)
        for m in range(M):
            ban[m, [cols[0], (16 * m + 2) % V, V - 1]] = False       # (an odd, an even and the last column: three different ones)
    return dict(X=X, W=W, bias=bias, ban=ban, logits=logits)


def pack_ban(ban, ld):
    """bool [M, V] -> uint16 [M, ld]: bit c & 15 of word c >> 4 = column c banned"""
    M, V = ban.shape
    out = np.zeros((M, ld), np.uint16)
    r, c = np.nonzero(ban)
    np.bitwise_or.at(out, (r, c >> 4), (1 << (c & 15)).astype(np.uint16))
    return out


def masked(case, m):
    """row m's logits as the head forms them: columns < V, banned ones -inf"""
    V = len(case["bias"])
    lg = case["logits"][m, :V].copy()
    if case["ban"] is not None:
        lg[case["ban"][m]] = NINF
    return lg
