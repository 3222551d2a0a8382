"""Plain numpy / Python restatement of the per-row draft verification of the teacher's greedy loop, written from the contracts in
csrc/kernels.h (launch_draft_accept_rows, ArgmaxArgs::keep_len) and csrc/host_logic.h (draft_tail_plan), for
tests/test_draft_rows.py and tests/test_draft_rows_gpu.py.  Tokens come from selection_reference's arg-max (largest value, smallest
index among equals), log-probabilities from logprob_reference's merge."""
import functools

import numpy as np

import logprob_reference as lpref
import selection_reference as sel


def tokens_of_partials(val, idx):
    """partials [M][ntiles] -> the token of every row under the loop's tie rule"""
    return np.array([sel.argmax_partials(val[m], idx[m]) for m in range(val.shape[0])], dtype=np.int64)


def logprobs_of_partials(val, idx, ssum):
    return np.array([lpref.merge(val[m], idx[m], ssum[m])[1] for m in range(val.shape[0])], dtype=np.float64)


def accept_rows(tok, ids, sep_id, sep_cnt, lp=None, lp_out=None, variant=None):
    """tok [B][n]: the model's token after draft positions 0..j of caption r; ids [B][ld]: column 0 = CLS, columns 1..n the staged
    draft (-1 = no word); sep_cnt: the counters before the launch (it adds); lp [B][n] (optional) with lp_out [B][ld_lp] before the
    launch.  -> dict(a_r, covered, ids, len, sep_cnt, lp_out, host = (min covered, max covered, sum a_r, fired)).
    variant: one of the wrong forms tests/test_draft_rows.py must catch -- "lockstep" (every row's length is the minimum),
    "covered_a" (covered = a instead of a + 1), "fired_max" (fired looked for below max covered)."""
    tok = np.asarray(tok, dtype=np.int64)
    out = np.array(ids, dtype=np.int64, copy=True)
    B, n = tok.shape
    assert out.shape[0] == B and out.shape[1] >= n + 1 and n >= 1
    cnt = np.array(sep_cnt, dtype=np.int64, copy=True)
    lpo = None if lp_out is None else np.array(lp_out, copy=True)
    a_r = []
    for r in range(B):
        j = 0
        while j < n and tok[r, j] == out[r, j + 1]:
            j += 1
        a_r.append(j)
    if variant == "covered_a":
        covered = [min(a, n) for a in a_r]
    else:
        covered = [min(a + 1, n) for a in a_r]
    if variant == "lockstep":
        covered = [min(covered)] * B
    for r in range(B):
        for j in range(covered[r]):
            out[r, j + 1] = tok[r, j]
            if tok[r, j] == sep_id:
                cnt[j] += 1
            if lpo is not None:
                lpo[r, j] = lp[r][j]
    lo, hi = min(covered), max(covered)
    fired = any(cnt[j] == B for j in range(hi if variant == "fired_max" else lo))
    return {"a_r": a_r, "covered": covered, "ids": out, "len": [1 + c for c in covered], "sep_cnt": cnt, "lp_out": lpo,
            "host": (lo, hi, int(sum(a_r)), 1 if fired else 0)}


def argmax_keep(tok, lp, out, lp_out, sep_cnt, step, sep_id, length, variant=None):
    """The KEEP arg-max of the step that writes position p = step + 1: tok [rows] / lp [rows] the model's token and log-probability,
    out [rows] / lp_out [rows] the words at position p before the launch, length [rows] the rows' verified lengths.  A row with
    p < length[r] keeps out and lp_out, adds nothing to sep_cnt and embeds the stored id.  -> (out, lp_out, sep_cnt, embedded ids).
    variant: "sep_twice" (a kept row's SEP counted again), "lp_zero" (0.0 written on a kept row)."""
    out = np.array(out, dtype=np.int64, copy=True)
    lpo = None if lp_out is None else np.array(lp_out, copy=True)
    cnt = np.array(sep_cnt, dtype=np.int64, copy=True)
    p = step + 1
    for r in range(out.shape[0]):
        if p < length[r]:
            if variant == "sep_twice" and out[r] == sep_id:
                cnt[step] += 1
            if variant == "lp_zero" and lpo is not None:
                lpo[r] = 0.0
            continue
        out[r] = tok[r]
        if tok[r] == sep_id:
            cnt[step] += 1
        if lpo is not None:
            lpo[r] = lp[r]
    return out, lpo, cnt, out.copy()


def tail_plan(min_covered, max_covered, fired, max_len, stop_all_sep):
    """csrc/host_logic.h: draft_tail_plan -> (run, t_first, keep_below)"""
    run = min_covered < max_len and not (stop_all_sep and fired)
    return run, min_covered, 1 + max_covered


def finish_steps(sep_cnt, rows, max_len, stop_all_sep):
    if stop_all_sep:
        for t in range(max_len):
            if sep_cnt[t] == rows:
                return t + 1
    return max_len


def plain_loop(next_token, B, max_len, cls, sep_id):
    """The plain greedy loop over a toy model next_token(r, prefix tuple) -> (token, lp): ids [B][max_len + 1], lp, sep_cnt"""
    ids = np.full((B, max_len + 1), -7, dtype=np.int64)
    ids[:, 0] = cls
    lp = np.zeros((B, max_len))
    cnt = np.zeros(max_len + 1, dtype=np.int64)
    for t in range(max_len):
        for r in range(B):
            ids[r, t + 1], lp[r, t] = next_token(r, tuple(ids[r, :t + 1]))
            cnt[t] += ids[r, t + 1] == sep_id
    return ids, lp, cnt


def draft_loop(next_token, draft, B, max_len, cls, sep_id, vocab, stop_all_sep, variant=None):
    """stage + verify + accept + KEEP tail over the same toy model -> (ids, lp, sep_cnt, steps, accept dict, tail steps run).
    Columns the call does not write keep -7 (ids) / NaN (lp)."""
    draft = np.asarray(draft, dtype=np.int64)
    n = draft.shape[1] - 1
    ids = np.full((B, max_len + 1), -7, dtype=np.int64)
    ids[:, 0] = cls
    ids[:, 1:n + 1] = np.where((draft[:, 1:] >= 0) & (draft[:, 1:] < vocab), draft[:, 1:], -1)
    lp = np.full((B, max_len), np.nan)
    tok = np.zeros((B, n), dtype=np.int64)
    tlp = np.zeros((B, n))
    for r in range(B):
        for j in range(n):
            tok[r, j], tlp[r, j] = next_token(r, tuple(ids[r, :j + 1]))
    acc = accept_rows(tok, ids, sep_id, np.zeros(max_len + 1, dtype=np.int64), tlp, lp,
                      variant if variant in ("lockstep", "covered_a", "fired_max") else None)
    ids, lp, cnt = acc["ids"], acc["lp_out"], acc["sep_cnt"]
    run, t_first, keep_below = tail_plan(acc["host"][0], acc["host"][1], acc["host"][3] != 0, max_len, stop_all_sep)
    ran = 0
    for t in range(t_first, max_len if run else t_first):
        res = [next_token(r, tuple(ids[r, :t + 1])) for r in range(B)]
        length = acc["len"] if t + 1 < keep_below else [0] * B
        ids[:, t + 1], lp[:, t], cnt, _ = argmax_keep([x[0] for x in res], [x[1] for x in res], ids[:, t + 1], lp[:, t], cnt, t,
                                                      sep_id, length, variant if variant in ("sep_twice", "lp_zero") else None)
        ran += 1
    return ids, lp, cnt, finish_steps(cnt, B, max_len, stop_all_sep), acc, ran


# ---- the inputs of tests/test_draft_rows_gpu.py (tests/test_draft_rows.py shows that they tell the wrong variants apart) ---------
SEP, CLS = 3, 1
ACCEPT_SHAPES = [(B, n, V) for B in (1, 3, 16) for n in (1, 2, 20, 63) for V in (100, 30522)]
PATTERNS = ("zero", "full", "mixed")


def fast_partials(logits):
    """logprob_reference.tile_partials, vectorised (the same three arrays; tests/test_draft_rows.py compares them)"""
    M, N = logits.shape
    nt = (N + 15) // 16
    pad = np.full((M, nt * 16), -np.inf)
    pad[:, :N] = logits
    t = pad.reshape(M, nt, 16)
    val = t.max(axis=2)
    idx = t.argmax(axis=2).astype(np.int64) + np.arange(nt, dtype=np.int64)[None, :] * 16
    live = val > -np.inf
    idx[~live] = lpref.SENTINEL
    with np.errstate(invalid="ignore"):
        ssum = np.where(live, np.exp(t - np.where(live, val, 0.0)[:, :, None]).sum(axis=2), 0.0)
    return val, idx, ssum


@functools.lru_cache(maxsize=4)
def accept_case(B, n, V, pattern, sep, seed):
    """-> dict(val, idx, sum fp32 [B * n][ntiles], ids int64 [B][n + 3] staged (-1 = no word), sep_cnt0 int32 [n + 2], a_r).
    pattern: every row rejects at once / accepts all / rows differ.  sep: "none"; "same" = every row emits SEP at step 0 (covered by
    all); "diff" = SEP at different covered steps, SEP behind a row's covered part, and a step j >= min covered whose counter
    reaches B only through what sep_cnt0 held.  Row 0 has a tie between two tiles, every row an all -inf tile."""
    rng = np.random.default_rng(seed)
    a_r = {"zero": [0] * B, "full": [n] * B, "mixed": [(5 * r + 1) % (n + 1) for r in range(B)]}[pattern]
    cov = [min(a + 1, n) for a in a_r]
    tok = rng.integers(4, V, size=(B, n))
    if sep == "same":
        tok[:, 0] = SEP
    sep_cnt0 = np.zeros(n + 2, dtype=np.int32)
    if sep == "diff":
        for r in range(B):
            tok[r, r % cov[r]] = SEP                      # a covered step of its own
            if cov[r] < n:
                tok[r, n - 1] = SEP                       # behind the covered part: not counted
        j = min(cov)
        if max(cov) > j:
            for r in range(B):
                if cov[r] > j:
                    tok[r, j] = SEP
            sep_cnt0[j] = sum(c <= j for c in cov)
    logits = rng.standard_normal((B * n, V)).astype(np.float32).astype(np.float64)
    logits[:, 16:32] = -np.inf
    tok = np.where((tok >= 16) & (tok < 32), tok + 16, tok)
    for m in range(B * n):
        logits[m, tok[m // n, m % n]] = 9.0
    if V > 64 and tok[0, 0] + 48 < V:
        logits[0, tok[0, 0] + 48] = 9.0                   # the same maximum three tiles on: the smaller index wins
    val, idx, ssum = fast_partials(logits)
    ids = np.full((B, n + 3), -9, dtype=np.int64)
    ids[:, 0] = CLS
    for r in range(B):
        ids[r, 1:n + 1] = rng.integers(4, V, size=n)
        ids[r, 1:a_r[r] + 1] = tok[r, :a_r[r]]
        if a_r[r] < n:
            ids[r, a_r[r] + 1] = (-1, (tok[r, a_r[r]] + 1) % V, -1)[r % 3]       # -1: what a draft id of -1 or >= V is staged as
            ids[r, a_r[r] + 2:n + 1] = tok[r, a_r[r] + 1:]                       # matches behind the first mismatch do not count
    return dict(val=val.astype(np.float32), idx=idx.astype(np.int32), sum=ssum.astype(np.float32), ids=ids, sep_cnt0=sep_cnt0,
                a_r=a_r, tok=tok)


def keep_case(rows, V, max_len, seed):
    """Kept and free rows mixed at step = pos - 1 for pos at len - 1, len and max_len - 1 of row 0 -> list of dicts"""
    rng = np.random.default_rng(seed)
    length = [2 + (3 * r) % (max_len - 2) for r in range(rows)]
    length[0], length[1] = 4, max_len                     # row 1 is kept at every position
    length[3::4] = [1] * len(length[3::4])                # rows with nothing verified behind CLS: never kept
    cases = []
    for pos in sorted({max(1, length[0] - 1), length[0], max_len - 1}):
        tok = rng.integers(4, V, size=rows)
        tok[::2] = SEP
        logits = rng.standard_normal((rows, V)).astype(np.float32).astype(np.float64)
        logits[np.arange(rows), tok] = 9.0
        val, idx, ssum = fast_partials(logits)
        out0 = rng.integers(4, V, size=rows)
        out0[::3] = SEP                                   # a kept SEP: counted by the accept launch, not again
        cases.append(dict(val=val.astype(np.float32), idx=idx.astype(np.int32), sum=ssum.astype(np.float32), tok=tok, out0=out0,
                          len=np.array(length, dtype=np.int32), step=pos - 1))
    return cases
