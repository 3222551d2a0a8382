"""Plain restatements for the search options of the device-resident search (include/gitcap.h: gitcap_search_options), the inputs
the GPU tests run, and the instrumented oracle run of the toy search.  No GPU, no library: tests/test_search_options.py holds this
file to oracle/search_oracle.py; tests/test_search_options_gpu.py holds the kernels to this file.

  penalize           the repetition penalty of model.py:522-531 in numpy fp32 -- the exact fp32 values the device must rank;
                     its output feeds selection_reference.beam_candidates (log-softmax + beam score + top K in fp64).
  fault=...          the same with one planted mistake; the CPU test shows that each one changes the expected output of the cases
                     below, i.e. that the GPU test would see it.
  topk_cases         the penalised top-k inputs.
  toy_search         oracle.search_oracle.beam_search on the table-driven toy model, with its BeamHypotheses instrumented.
"""
import numpy as np
import torch

import selection_reference as R
from oracle import search_oracle

NINF = float("-inf")


def penalize(logits_f32, prefix_ids, rp, fault=None):
    """logits_f32 [rows][V] fp32, prefix_ids [rows][cur_len] int64 -> fp32 [rows][V]: every column that occurs in the row's prefix
    becomes x < 0 ? x * rp : x / rp in fp32 (once however often it occurs; an id outside [0, V) is no column)."""
    x = np.array(logits_f32, dtype=np.float32, copy=True)
    ids = np.asarray(prefix_ids, dtype=np.int64)
    assert x.ndim == 2 and ids.ndim == 2 and ids.shape[0] == x.shape[0]
    rp32 = np.float32(rp)
    V = x.shape[1]
    for r in range(x.shape[0]):
        row = ids[r].tolist()
        if fault == "cls_skipped":
            row = row[1:]
        for v in (row if fault == "repeat_twice" else sorted(set(row))):
            if not 0 <= v < V:
                continue
            neg = x[r, v] < 0
            if fault == "sign_swapped":
                neg = not neg
            x[r, v] = x[r, v] * rp32 if neg else x[r, v] / rp32
    return x


def expected_candidates(x, bs, prefix, rp, beams, K, fault=None):
    """-> (scores fp64 [B][K], idx [B][K], gap [B]) of selection_reference.beam_candidates on the penalised logits.
    fault 'after_softmax': the penalty applied to the log-probabilities instead (the row's log-sum-exp is the raw one)."""
    bs32 = np.asarray(bs, np.float32)
    if fault == "after_softmax":
        x64 = np.asarray(x, np.float64)
        m = x64.max(axis=1, keepdims=True)
        lsm = (x64 - (m + np.log(np.exp(x64 - m).sum(axis=1, keepdims=True)))).astype(np.float32)
        pen = penalize(lsm, prefix, rp)                       # not a distribution any more: rank it as it is
        sc = pen.astype(np.float64) + bs32.astype(np.float64)[:, None]
        B = x.shape[0] // beams
        scores, idx = np.empty((B, K)), np.empty((B, K), np.int64)
        for b in range(B):
            flat = sc[b * beams:(b + 1) * beams].reshape(-1)
            order = np.argsort(-flat, kind="stable")[:K]
            scores[b], idx[b] = flat[order], order
        return scores, idx, None
    return R.beam_candidates(penalize(x, prefix, rp, fault), bs32, beams, K)


# ---- penalised top-k inputs ----------------------------------------------------------------------------------------------------

TOPK_V, TOPK_BEAMS, TOPK_K, TOPK_B = 4100, 3, 6, 2


def _spiked(rng, rows, V, places, low=-1.0, top=6.0, step=0.31):
    """Background logits in [low, low + 1), and (row, column) spikes top, top - step, ... in the order given."""
    x = (rng.random((rows, V), dtype=np.float32) + np.float32(low)).astype(np.float32)
    assert len(set(places)) == len(places)
    for k, (r, v) in enumerate(places):
        x[r, v] = np.float32(top - step * k)
    return x


def topk_cases():
    """name -> dict(x [B*beams][V] fp32, bs, prefix int64 [B*beams][ld_ids], cur_len, rp, beams, K).  Columns of prefix behind cur_len
    name spiked columns: a kernel that read them would rank differently."""
    rng = np.random.default_rng(522)
    V, beams, K, B = TOPK_V, TOPK_BEAMS, TOPK_K, TOPK_B
    rows = B * beams
    cases = {}

    def case(name, x, prefix, cur_len, rp, beams_=beams, K_=K):
        cases[name] = dict(x=x, bs=(rng.random(x.shape[0]) - 1.0).astype(np.float32), prefix=np.asarray(prefix, np.int64), cur_len=cur_len,
                           rp=rp, beams=beams_, K=K_)

    # 1. prefix tokens at the chunk edges: columns 0, 2047, 2048, V - 1, all of them spikes, among unpenalised spikes
    edge = [0, 2047, 2048, V - 1]
    other = [5, 2046, 2049, V - 2, 1000, 3000, 4095, 4096]
    for rp in (1.5, 0.5):                                                                   # 7. both directions
        x = _spiked(rng, rows, V, [(r, c) for c in other for r in range(rows)], top=5.4, step=0.013)
        for r in range(rows):                                                               # every edge column is a spike in every row
            for i, c in enumerate(edge):
                x[r, c] = np.float32(6.0 - 0.17 * i - 0.029 * r)
        case("edges_rp%s" % rp, x, np.tile(np.array(edge + [5]), (rows, 1)), 4, rp)        # column 5 lies behind cur_len
    # 2. the row maximum is penalised: another column wins and the log-sum-exp moves
    x = _spiked(rng, rows, V, [(r, 100 + 7 * r + 300 * k) for r in range(rows) for k in range(3)], step=0.23)
    for r in range(rows):
        x[r, 2500 + r] = np.float32(9.0 + 0.1 * r)
    case("max_penalised", x, [[0, 2500 + r, 3] for r in range(rows)], 3, 1.5)
    # 3. a positive, a negative, an exact-zero and a -inf logit, all penalised; the background is far below, so negative logits rank
    x = (rng.random((rows, V), dtype=np.float32) - np.float32(9.0)).astype(np.float32)
    for r in range(rows):
        vals = [2.0, 0.0, -0.5, -1.1, -1.6, -2.3, -2.9, 1.3, NINF]
        cols = [10, 2047, 2048, 4099, 300, 301, 302, 303, 2050]
        for v, c in zip(vals, cols):
            x[r, c] = np.float32(v - 0.013 * r) if np.isfinite(v) and v != 0.0 else np.float32(v)
    case("signs", x, [[10, 2047, 2048, 4099, 2050, 301]] * rows, 6, 1.5)
    case("signs_rp0.5", x.copy(), [[10, 2047, 2048, 4099, 2050, 301]] * rows, 6, 0.5)
    # 4. a token three times in the prefix: penalised once
    x = _spiked(rng, rows, V, [(r, c) for r in range(rows) for c in (77 + r, 400, 2100 + r, 3333)], step=0.19)
    case("repeat3", x, [[0, 77 + r, 77 + r, 77 + r, 3333] for r in range(rows)], 5, 1.5)
    # 5. a different prefix for every row (every row holds the same spikes)
    x = _spiked(rng, rows, V, [(r, c) for c in (11, 2047, 2048, 2222, 4099, 600, 601) for r in range(rows)], step=0.011)
    pre = [[0, 11, 2047], [0, 2048, 2222], [0, 4099, 600], [0, 601, 11], [0, 2222, 4099], [0, 2047, 601]]
    case("per_row", x, pre, 3, 1.5)
    # 6. cur_len 1 (CLS only; column 0 is the clip's best logit) and cur_len 63 (more ids than a wave)
    x = _spiked(rng, rows, V, [(r, c) for r in range(rows) for c in (0, 9 + r, 2048 + r, 4000)], step=0.27)
    case("cls_only", x, [[0, 9 + r, 4000] for r in range(rows)], 1, 1.5)                    # 9 + r, 4000: behind cur_len
    pre = rng.integers(1, V, size=(rows, 64))
    pre[:, 0] = 0
    x = _spiked(rng, rows, V, [(r, int(pre[r, t])) for r in range(rows) for t in (62, 31, 1)] +
                [(r, 700 + r) for r in range(rows)] + [(r, 701 + rows + r) for r in range(rows)], step=0.07)
    for r in range(rows):
        pre[r, 63] = 700 + r                                                                # behind cur_len: a spike that stays
    case("cur_len63", x, pre, 63, 1.5)
    # 8. ids that are no column: -1, V, 3 * 2048 + 4 (column 4 of a chunk past the last), 2^33 + 5 (column 5 after a 32-bit truncation)
    x = _spiked(rng, rows, V, [(r, c) for r in range(rows) for c in (4, 5, 4099, 2051, 52)], step=0.037)
    case("ignored_ids", x, [[0, -1, V, 3 * 2048 + 4, 2 ** 33 + 5, 52]] * rows, 6, 1.5)
    # 9. the vocabulary of the model: 15 chunks, the last one 1850 columns wide
    Vb, beams_b, Kb = 30522, 4, 8
    rows_b = 2 * beams_b
    cols = [0, 2047, 2048, 30521, 28672, 28671, 15000, 101, 102, 20000, 9999]
    x = _spiked(rng, rows_b, Vb, [(b * beams_b + k % beams_b, c) for b in range(2) for k, c in enumerate(cols)], step=0.21)
    case("vocab30522", x, [[101, 30521, 2048, 28672, 102, 15000 + r] for r in range(rows_b)], 6, 1.5, beams_b, Kb)
    # 10. K = 12: the 16-deep lists.  Three chunks, the last one 4 columns wide; penalised spikes at 2047, 2048 and V - 1; id 2053 is
    # column 5 of chunk 1 while the spike at column 5 lies in chunk 0 (a chunk-relative reading would penalise it); columns
    # 7 + r, 263 + r, 519 + r belong to one thread of the chunk kernel, so its list holds three of the winners
    beams_k, Kk = 4, 12
    rows_k = 2 * beams_k
    x = _spiked(rng, rows_k, V, [(r, c) for c in (2047, 2048, V - 1, 5) for r in range(rows_k)] +
                [(r, c + r) for c in (7, 263, 519, 3000) for r in range(rows_k)], step=0.043)
    case("k12", x, [[2047, 2048, V - 1, 2053, 5]] * rows_k, 4, 1.5, beams_k, Kk)                # column 5 lies behind cur_len
    return cases


FAULT_CASES = {"after_softmax": "max_penalised", "repeat_twice": "repeat3", "cls_skipped": "cls_only", "sign_swapped": "signs"}


# ---- the toy search --------------------------------------------------------------------------------------------------------------

TOY_V, TOY_EOS, TOY_CLS, TOY_B, TOY_MAXLEN = 23, 22, 0, 3, 7
TOY_SEED = 9


def toy_table(seed=TOY_SEED):
    """Logits by (clip, position % 8, last token), the scheme of tests/test_selection_gpu.py: _beam_table.  Clip 0: EOS is the best
    candidate of step 1 and a strong one later, so that clip finishes hypotheses early and often (evictions, rejections, and with
    n = 1 it is done at step 2); clip 2: EOS towers over every row of step 3; clip 1: plain."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(TOY_B, 8, TOY_V, TOY_V, generator=g) * 2.0
    table[0, 0, TOY_CLS, TOY_EOS] = 12.0
    table[0, 1:, :, TOY_EOS] += 3.0
    table[2, 2, :, TOY_EOS] = 9.0
    return table


def toy_search(table, beams, lp, n, rp):
    """-> (decoded [B][n][L], logprobs [B][n], prefixes the step function saw, log).  log: per clip 'short' = steps at which the clip
    held some but fewer than n hypotheses, 'evicted' / 'rejected' = adds to a full container that replaced / did not replace,
    'done_at' = the step (cur_len) whose is_done first said yes."""
    seen = []
    log = {"short": [0] * TOY_B, "evicted": [0] * TOY_B, "rejected": [0] * TOY_B, "done_at": [None] * TOY_B}
    made = []
    cur = {"len": 0}

    class Hyp(search_oracle.BeamHypotheses):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.clip = len(made)
            made.append(self)

        def add(self, hyp, s):
            full = len(self.hyp) == self.n_hyp
            before = [id(h) for _, h in self.hyp]
            super().add(hyp, s)
            if full:
                log["rejected" if [id(h) for _, h in self.hyp] == before else "evicted"][self.clip] += 1

        def is_done(self, best):
            r = super().is_done(best)
            if 0 < len(self.hyp) < self.n_hyp:
                log["short"][self.clip] += 1
            if r and log["done_at"][self.clip] is None:
                log["done_at"][self.clip] = cur["len"]
            return r

    clip = torch.arange(TOY_B * beams) // beams

    def step(ids):
        seen.append(ids.clone())
        cur["len"] = ids.shape[1]
        return table[clip, (ids.shape[1] - 1) % 8, ids[:, -1] % TOY_V].clone()

    orig = search_oracle.BeamHypotheses
    search_oracle.BeamHypotheses = Hyp
    try:
        dec, lps, _ = search_oracle.beam_search(torch.full((TOY_B, 1), TOY_CLS), step, eos_index=TOY_EOS, max_steps=TOY_MAXLEN,
                                                beam_size=beams, per_node_beam_size=2, length_penalty=lp, num_keep_best=n,
                                                repetition_penalty=rp)
    finally:
        search_oracle.BeamHypotheses = orig
    return dec.view(TOY_B, n, TOY_MAXLEN), lps, seen, log


def toy_configs():
    return [(n, beams, lp, rp) for beams in (1, 3, 4) for n in sorted({1, 2, 3, 2 * beams}) for lp in (0.0, 0.6) for rp in (1.0, 1.7)]


def replay_search(step_logits, B, beams, K, L, eos, cls, lp, n, rp):
    """The search of oracle.search_oracle.beam_search replayed from recorded per-step logits [L - 1][B * beams][V] (what a device
    search saved), ranking with expected_candidates: -> (decoded [B][n][L], logprobs [B][n], the smallest gap between distinct
    consecutive candidate scores among the first K + 1 of any step of a clip that was still searching)."""
    x = np.asarray(step_logits, np.float32)
    V = x.shape[2]
    ids = np.full((B * beams, 1), cls, np.int64)
    scores = np.tile(np.array([0.0] + [-1e9] * (beams - 1), np.float32), B)
    hyps = [search_oracle.BeamHypotheses(n, L, lp, early_stopping=False) for _ in range(B)]
    done, min_gap = [False] * B, float("inf")
    for cur_len in range(1, L):
        ws, wi, gap = expected_candidates(x[cur_len - 1], scores, ids, rp, beams, K)
        new_scores, new_words, new_src = [], [], []
        for b in range(B):
            done[b] = done[b] or hyps[b].is_done(float(ws[b].max()))
            kept = []
            if not done[b]:
                min_gap = min(min_gap, float(gap[b]))
                for idx, s in zip(wi[b].tolist(), ws[b].tolist()):
                    beam_id, word = divmod(idx, V)
                    if word == eos or cur_len + 1 == L:
                        hyps[b].add(torch.from_numpy(ids[b * beams + beam_id, :cur_len].copy()), float(np.float32(s)))
                    else:
                        kept.append((np.float32(s), word, b * beams + beam_id))
                    if len(kept) == beams:
                        break
            if len(kept) < beams:
                kept = [(np.float32(0.0), eos, 0)] * beams
            for s, w, r in kept:
                new_scores.append(s); new_words.append(w); new_src.append(r)
        ids = np.concatenate([ids[np.array(new_src)], np.array(new_words, np.int64)[:, None]], axis=1)
        scores = np.array(new_scores, np.float32)
    decoded = np.full((B, n, L), eos, np.int64)
    logprobs = np.full((B, n), -1e5, np.float64)
    for b, h in enumerate(hyps):
        order = sorted(range(len(h.hyp)), key=lambda i: -h.hyp[i][0])          # stable: equal scores in storage order
        for k, i in enumerate(order[:n]):
            decoded[b, k, :len(h.hyp[i][1])] = h.hyp[i][1].numpy()
            logprobs[b, k] = h.hyp[i][0]
    return decoded, logprobs, min_gap
