"""Restatement of prompted decoding (include/gitcap.h: gitcap_attach_prompt) in numpy / plain Python, written from the contracts of
the forced forms of argmax_final_kernel and of the beam-step kernels (csrc/kernels.h, csrc/select.hip, csrc/search.hip), for tests/test_prompt.py
and tests/test_prompt_gpu.py.  The free case of a selection is tests/selection_reference.py's.

`fault=` builds the subtly wrong kernels tests/test_prompt.py must see caught by the inputs the GPU tests use:
  "le"            forcing at p <= len instead of p < len
  "count_sep"     a forced SEP counted by the stop rule
  "add_hyp"       a forced step that still stores finished hypotheses
  "touch_scores"  a forced step that still writes beam_scores"""
import numpy as np

import selection_reference as R

SEP, CLS = 5, 1
POISON = -777


def clamp_len(n, max_len):
    return min(max(int(n), 1), max_len)


def forced_select(val, idx, prompt, lengths, max_len, step, sep_id, fault=None):
    """One forced arg-max launch over partials val / idx [rows][ntiles]: position p = step + 1.
    -> (tokens [rows], forced [rows] bool, rows counted as SEP).  A forced row's log-probability is 0.0."""
    p = step + 1
    toks, forced, n_sep = [], [], 0
    for r in range(len(val)):
        n = clamp_len(lengths[r], max_len)
        f = p <= n if fault == "le" else p < n
        f = f and p < prompt.shape[1]
        t = int(prompt[r, p]) if f else R.argmax_partials(val[r], idx[r])
        if t == sep_id and (not f or fault == "count_sep"):
            n_sep += 1
        toks.append(t)
        forced.append(f)
    return toks, forced, n_sep


def greedy_direct(logits_of, B, steps, prompt, lengths, sep_id):
    """The direct loop: at each step the arg-max over full logits, overwritten at prompt positions.  logits_of(ids [B][t + 1], t)
    -> [B][V].  -> (ids [B][steps + 1], sep_cnt [steps])"""
    ids = np.zeros((B, steps + 1), np.int64)
    ids[:, 0] = prompt[:, 0]
    sep_cnt = []
    for t in range(steps):
        x = logits_of(ids[:, :t + 1], t)
        tok = np.array([R.argmax_first(x[b]) for b in range(B)])
        cnt = 0
        for b in range(B):
            if t + 1 < lengths[b]:
                ids[b, t + 1] = prompt[b, t + 1]
            else:
                ids[b, t + 1] = tok[b]
                cnt += int(tok[b] == sep_id)
        sep_cnt.append(cnt)
    return ids, sep_cnt


def greedy_restated(logits_of, B, steps, prompt, lengths, max_len, sep_id, fault=None):
    """The same loop through the head's per-tile partials and forced_select."""
    ids = np.zeros((B, steps + 1), np.int64)
    ids[:, 0] = prompt[:, 0]
    sep_cnt = []
    for t in range(steps):
        val, idx = R.tile_partials(logits_of(ids[:, :t + 1], t))
        toks, _, n_sep = forced_select(val, idx, prompt, lengths, max_len, t, sep_id, fault)
        ids[:, t + 1] = toks
        sep_cnt.append(n_sep)
    return ids, sep_cnt


# ---- the beam step ----------------------------------------------------------------------------------------------------------------

def beam_init(B, beams, n, L, cls=CLS):
    R_ = B * beams
    st = dict(ids0=np.full((R_, L), POISON, np.int64), ids1=np.full((R_, L), POISON, np.int64), words=np.full(R_, cls, np.int64),
              hyp_ids=np.full((B, n, L), POISON, np.int64), beam_scores=np.zeros(R_, np.float32), hyp_score=np.zeros((B, n), np.float32),
              src_rows=np.arange(R_, dtype=np.int32), done=np.zeros(B, np.int32), hyp_len=np.zeros((B, n), np.int32))
    st["ids0"][:, 0] = cls
    st["beam_scores"][:] = np.where(np.arange(R_) % beams == 0, 0.0, -1e9)
    return st


def _f32(x):
    return np.float32(x)


def _norm(score, length, lp):
    return _f32(_f32(score) / _f32(np.power(_f32(length), _f32(lp))))


def _free_clip(st, b, n, cs, ci, beams, K, V, cur_len, L, eos, lp, cur, sampled, write_scores=True, write_ids=True):
    old = st["ids1" if cur else "ids0"]
    hl, hs, hyp = st["hyp_len"][b], st["hyp_score"][b], st["hyp_ids"][b]
    cnt = 0
    while cnt < n and hl[cnt] > 0:
        cnt += 1
    done = st["done"][b] != 0
    if not done and cnt == n:
        best = max(cs) if sampled else cs[0]
        done = min(hs[:n]) >= _norm(best, L - 1, lp)
    src, word, kept = [0] * beams, [eos] * beams, 0
    if not done:
        for c in range(K):
            if kept >= beams:
                break
            if sampled and ci[c] == R.SENTINEL:
                continue
            beam_id, w = divmod(int(ci[c]), V)
            if w == eos or cur_len + 1 == L:
                score = _norm(cs[c], cur_len, lp)
                row = old[b * beams + beam_id, :cur_len].copy()
                if cnt < n:
                    e = cnt
                    cnt += 1
                else:
                    e = int(np.argmin(hs[:n]))                    # the earliest stored of equal minima
                    if not score > hs[e]:
                        continue
                    for i in range(e, n - 1):
                        hs[i], hl[i] = hs[i + 1], hl[i + 1]
                        hyp[i, :hl[i]] = hyp[i + 1, :hl[i]]
                    e = n - 1
                hs[e], hl[e] = score, cur_len
                hyp[e, :cur_len] = row
            else:
                src[kept], word[kept] = b * beams + beam_id, w
                if write_scores:
                    st["beam_scores"][b * beams + kept] = cs[c]
                kept += 1
    if kept < beams:
        for j in range(kept if sampled else 0, beams):
            src[j], word[j] = 0, eos
            if write_scores:
                st["beam_scores"][b * beams + j] = 0.0
    st["done"][b] = 1 if done else 0
    if write_ids:
        new = st["ids0" if cur else "ids1"]
        for j in range(beams):
            r = b * beams + j
            new[r, :cur_len] = old[src[j], :cur_len]
            new[r, cur_len] = word[j]
            st["words"][r], st["src_rows"][r] = word[j], src[j]


def beam_step(st, n, cand_scores, cand_idx, B, beams, K, V, cur_len, L, eos, lp, cur, sampled=False, prompt=None, lengths=None,
              prompt_max_len=0, fault=None):
    """One bookkeeping step over the state dict `st` (in place).  prompt given: a clip with cur_len < lengths[b] (clamped to
    [1, prompt_max_len]) is forced -- every beam keeps its prefix and appends prompt[b][cur_len], src_rows is the identity, nothing
    else of the clip is touched and its candidates are not read."""
    old, new = st["ids1" if cur else "ids0"], st["ids0" if cur else "ids1"]
    for b in range(B):
        forced = False
        if prompt is not None:
            nlen = clamp_len(lengths[b], prompt_max_len)
            forced = (cur_len <= nlen if fault == "le" else cur_len < nlen) and cur_len < prompt.shape[1]
        if not forced:
            _free_clip(st, b, n, cand_scores[b], cand_idx[b], beams, K, V, cur_len, L, eos, lp, cur, sampled)
            continue
        if fault in ("add_hyp", "touch_scores"):                  # the wrong kernels: part of the free bookkeeping still runs
            keep = {k: st[k].copy() for k in ("beam_scores", "done", "hyp_len", "hyp_score", "hyp_ids")}
            _free_clip(st, b, n, cand_scores[b], cand_idx[b], beams, K, V, cur_len, L, eos, lp, cur, sampled, write_ids=False)
            for k in (("beam_scores",) if fault == "add_hyp" else ("hyp_len", "hyp_score", "hyp_ids")) + ("done",):
                st[k][...] = keep[k]
        for j in range(beams):
            r = b * beams + j
            new[r, :cur_len] = old[r, :cur_len]
            new[r, cur_len] = prompt[b, cur_len]
            st["words"][r], st["src_rows"][r] = prompt[b, cur_len], r


def beam_finish(st, n, B, L, eos):
    """-> (decoded [B][n][L], logprobs [B][n]) by descending score, equal scores in storage order"""
    dec = np.full((B, n, L), eos, np.int64)
    lps = np.full((B, n), -1e5, np.float32)
    for b in range(B):
        stored = [i for i in range(n) if st["hyp_len"][b, i] > 0]
        for rank, i in enumerate(sorted(stored, key=lambda i: (-st["hyp_score"][b, i], i))):
            m = st["hyp_len"][b, i]
            dec[b, rank, :m] = st["hyp_ids"][b, i, :m]
            lps[b, rank] = st["hyp_score"][b, i]
    return dec, lps


# ---- the inputs of tests/test_prompt_gpu.py (built here so that tests/test_prompt.py can show what they catch) ----------------------

SEL_STEP = 2                    # the launch writes position 3
SEL_MAX_LEN = 6


def selection_inputs(nt, seed=0):
    """4 rows of partials [4][nt] and their prompts, lengths {1, 2, step + 1, step + 2}, for the launches of steps SEL_STEP - 1 and
    SEL_STEP (positions p = SEL_STEP and SEL_STEP + 1).  At SEL_STEP: rows 0 and 1 are free, row 2 is just free (p == its length:
    `<=` would force it) and row 3 is at its last forced position, where its prompt holds SEP (not counted).  At SEL_STEP - 1: row
    2 is at its last forced position and row 3 is forced onto the very token its partials elect.  Row 1's arg-max is SEP
    (counted), row 2 is all -inf (free: token 0), row 0's arg-max sits in the last tile."""
    rng = np.random.default_rng(seed + nt)
    val = (rng.permutation(4 * nt).reshape(4, nt).astype(np.float32) / (4 * nt) - 2.0)
    idx = np.arange(nt, dtype=np.int64)[None, :] * 16 + rng.integers(0, 16, (4, nt))
    val[0, nt - 1] = 3.0
    val[1, 0], idx[1, 0] = 3.0, SEP
    val[2], idx[2] = -np.inf, R.SENTINEL
    val[3, nt // 2] = 3.0
    vocab = 16 * nt
    prompt = rng.integers(6, max(7, vocab), (4, SEL_MAX_LEN + 2)).astype(np.int64) % vocab
    prompt[:, 0] = CLS
    p = SEL_STEP + 1
    prompt[3, p] = SEP                                            # a forced SEP
    prompt[2, p] = 7 % vocab                                      # what `<=` would force on the masked row (its arg-max is 0)
    prompt[3, p - 1] = idx[3, nt // 2]                            # a forced token that equals the row's arg-max
    lengths = np.array([1, 2, SEL_STEP + 1, SEL_STEP + 2], np.int32)
    return val, idx, prompt, lengths


def beam_inputs(beams, n, sampled, seed=0):
    """B = 3 clips at cur_len = 2 of L = 8: clip 0 forced (lengths 4), clip 1 free (lengths 2: its prompt just ended; `<=` would
    force it), clip 2 done.  The forced clip's best candidate is EOS (a wrong kernel stores a hypothesis) and its candidate scores
    differ from its beam scores (a wrong kernel rewrites them).  -> (state dict, cand_scores [3][K], cand_idx [3][K], prompt,
    lengths, constants dict)"""
    B, L, V, eos, cur_len, K = 3, 8, 40, SEP, 2, min(16, 2 * beams)
    rng = np.random.default_rng(seed + 10 * beams + n + (100 if sampled else 0))
    st = beam_init(B, beams, n, L)
    st["ids0"][:, 1] = rng.integers(6, V, B * beams)
    st["beam_scores"][:] = -rng.random(B * beams).astype(np.float32) - 0.5
    st["words"][:] = st["ids0"][:, 1]
    st["done"][2] = 1
    st["hyp_len"][2, 0], st["hyp_score"][2, 0] = 2, -0.25
    st["hyp_ids"][2, 0, :2] = [CLS, 9]
    if n > 1:                                                     # clip 1 holds one hypothesis already
        st["hyp_len"][1, 0], st["hyp_score"][1, 0] = 2, -3.5
        st["hyp_ids"][1, 0, :2] = [CLS, 11]
    cs = np.sort(-rng.random((B, K)).astype(np.float32) * 4.0 - 0.1, axis=1)[:, ::-1].copy()
    ci = np.zeros((B, K), np.int64)
    for b in range(B):
        words = rng.permutation(np.arange(6, V))[:K]
        ci[b] = rng.integers(0, beams, K) * V + words
    if sampled:                                                   # draws come in no order; one row ran out of columns
        perm = rng.permutation(K)
        cs, ci = cs[:, perm].copy(), ci[:, perm].copy()
        cs[1, 0], ci[1, 0] = -np.inf, R.SENTINEL
    ci[0, 0] = (ci[0, 0] // V) * V + eos                          # the forced clip's first candidate finishes a hypothesis
    ci[1, 1] = (ci[1, 1] // V) * V + eos                          # the free clip stores one
    prompt = rng.integers(6, V, (B, 6)).astype(np.int64)
    prompt[:, 0] = CLS
    lengths = np.array([4, 2, 1], np.int32)
    return st, cs, ci, prompt, lengths, dict(B=B, beams=beams, K=K, V=V, cur_len=cur_len, L=L, eos=eos, lp=0.6, cur=0, pmax=4)
