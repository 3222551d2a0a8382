"""What the student's prompted-decoding tests share (tests/test_student_prompt.py on the CPU, the two *_gpu.py files on the device):
numpy restatements of student_prompt_stage_kernel and of student_beam_step_kernel (plain and forced), the inputs the per-kernel GPU
tests upload, the prompts of the end-to-end cases, and the yardsticks -- a greedy loop and the device-shaped beam loop over any
``forward_decoder(ids, memory) -> logits`` that take the prompt's token inside a row's prompt.

``wrong=`` turns a restatement into one of three mistakes a kernel could make, so that the tests can show their cases tell them
apart: "pos" (the forced selection looks at the position it reads instead of the one it writes), "noclamp" (lengths used as given)
and "permute" (a forced beam step that follows the candidates' source rows instead of keeping every row's own prefix)."""
import numpy as np
import torch

B, L, K = 3, 10, 3                  # clips, greedy steps / beam max_len, beams of the end-to-end cases
MEM_SEED = 7                        # a memory on which the tiny model answers every prompt of the cases with other tokens
PAD = 0


def prompt_len(lengths, r, max_len, wrong=None):
    n = int(lengths[r])
    return n if wrong == "noclamp" else min(max(n, 1), max_len)


# ---- the stage kernel -------------------------------------------------------------------------------------------------------------

def stage(prm_ids, prm_len, rows, k, max_len, cls, ids, lp=None, pmin=1, wrong=None):
    """ids [rows][ld] (and lp [rows][ld_lp]) as the launch leaves them; the inputs are not modified.  Row r takes prompt row r // k."""
    ids = np.array(ids, dtype=np.int64)
    lp = None if lp is None else np.array(lp, dtype=np.float32)
    ld = ids.shape[1]
    for r in range(rows):
        n = prompt_len(prm_len, r // k, max_len, wrong)
        for i in range(ld):
            ids[r, i] = prm_ids[r // k, i] if 1 <= i < n else cls
        if lp is not None:
            lp[r, :max(pmin - 1, 0)] = 0.0
    return ids, lp


def stage_inputs():
    """The per-kernel case: ld = 12, lengths 1, 4, 11 and one each of 0 and 99 (the clamp), max_len 11 -> prompt table [5][12] whose
    column 11 no launch may read, lengths, max_len, cls.  (Five rows: one per length the case names.)"""
    g = np.random.default_rng(5)
    prm = g.integers(1, 90, size=(5, 12)).astype(np.int64)
    prm[:, 11] = 7777                   # behind max_len: a read here is a read the clamp must prevent
    return prm, np.array([1, 4, 11, 0, 99], dtype=np.int32), 11, 101


# ---- the beam bookkeeping step ------------------------------------------------------------------------------------------------------

def beam_step(cand_scores, cand_idx, ids_cur, ids_next, scores, src_rows, B_, k, V, t, prompt=None, wrong=None):
    """-> (ids_next, scores, src_rows) as the launch leaves them.  prompt = (ids [B][ld], lengths [B], max_len) or None; the forced
    form runs where t + 1 < max_len, and in it a clip with t + 1 < its length is not ranked."""
    ids_next, scores, src_rows = np.array(ids_next, dtype=np.int64), np.array(scores, dtype=np.float32), np.array(src_rows, dtype=np.int32)
    for b in range(B_):
        forced = prompt is not None and t + 1 < prompt[2] and t + 1 < prompt_len(prompt[1], b, prompt[2])
        for j in range(k):
            idx = int(cand_idx[b * k + j])
            beam, tok = idx // V, idx % V
            dst = b * k + j
            if forced:
                src = b * k + beam if wrong == "permute" else dst
                ids_next[dst, :t + 1] = ids_cur[src, :t + 1]
                ids_next[dst, t + 1] = prompt[0][b, t + 1]
                src_rows[dst] = src
            else:
                src = b * k + beam
                ids_next[dst, :t + 1] = ids_cur[src, :t + 1]
                ids_next[dst, t + 1] = tok
                scores[dst] = cand_scores[b * k + j]
                src_rows[dst] = src
    return ids_next, scores, src_rows


def beam_step_inputs():
    """The per-kernel case: B = 2, k = 3, V = 40, t = 2, ld = 8; clip 0 inside its prompt (length 5), clip 1 free (length 2)."""
    g = np.random.default_rng(9)
    Bn, k, V, ld = 2, 3, 40, 8
    d = dict(B=Bn, k=k, V=V, t=2, ld=ld)
    d["cand_scores"] = (-g.random(Bn * k)).astype(np.float32)
    d["cand_idx"] = np.array([2 * V + 5, 0 * V + 7, 2 * V + 39, 1 * V + 0, 1 * V + 3, 0 * V + 11], dtype=np.int32)     # beams 2 0 2 | 1 1 0
    d["ids_cur"] = g.integers(1, V, size=(Bn * k, ld)).astype(np.int64)
    d["prompt_ids"] = g.integers(1, V, size=(Bn, ld)).astype(np.int64)
    d["lengths"] = np.array([5, 2], dtype=np.int32)
    d["prompt_max_len"] = 5
    return d


# ---- the prompts of the end-to-end cases ------------------------------------------------------------------------------------------------

def case_prompts(free, V, cls):
    """free: the unprompted greedy captions [B][1 + L] -> {case: list of B rows (lists, CLS first)}.  Token j of a prompt is
    free[b][j] + 1 + j folded into the vocabulary: never the token the model emits there.  "ragged" has one PAD inside the longest
    prompt (the self-attention's key mask) and one row without a prompt."""
    free = np.asarray(free)

    def row(b, n):
        return [cls] + [int((free[b, j] + 1 + j) % V) for j in range(1, n)]
    shared = [row(b, 4) for b in range(B)]
    ragged = [row(0, 1), row(1, 3), row(2, 6)]
    ragged[2][3] = PAD
    return dict(shared4=shared, ragged=ragged)


def table(prompts, cls):
    """list of rows -> (ids int64 [B][max length] padded with CLS, lengths int32 [B])"""
    n = max(len(r) for r in prompts)
    ids = np.full((len(prompts), n), cls, dtype=np.int64)
    for b, r in enumerate(prompts):
        ids[b, :len(r)] = r
    return ids, np.array([len(r) for r in prompts], dtype=np.int32)


# ---- yardsticks ------------------------------------------------------------------------------------------------------------------

def greedy_yardstick(forward, memory, max_len, prompts, cls, wrong=None):
    """-> (ids int64 [B][1 + max_len], forced bool [B][max_len], the last-position logits of every step [max_len][B][V]): the loop
    on the growing prefix, the rows staged as the stage kernel stages them; position t + 1 takes the prompt's token while
    t + 1 < the row's length, else the first arg-max."""
    prm, lens = table(prompts, cls)
    Bn = len(prompts)
    ids, _ = stage(prm, lens, Bn, 1, max_len, cls, np.zeros((Bn, max_len + 1), dtype=np.int64))
    forced = np.zeros((Bn, max_len), dtype=bool)
    rows = []
    for t in range(max_len):
        lg = forward(torch.as_tensor(ids[:, :t + 1]), memory)[:, -1].float().cpu().numpy()
        rows.append(lg)
        pos = t if wrong == "pos" else t + 1
        for b in range(Bn):
            n = min(max(int(lens[b]), 1), max_len)
            forced[b, t] = pos < n
            ids[b, t + 1] = prm[b, pos] if forced[b, t] else int(lg[b].argmax())
    return ids, forced, np.stack(rows, 0)


def beam_yardstick(forward, memory, max_len, k, prompts, cls, wrong=None):
    """The device's search on B * k lockstep rows -> the best beam [B][max_len].  Scores start at [0, -1e9, ..]; at step t a clip
    with t + 1 < its length appends the prompt's token to every row (scores untouched), any other clip keeps the k best of its
    k * V candidates score + log_softmax, best first, ties to the smaller flat index.  memory: [B][F][D]."""
    prm, lens = table(prompts, cls)
    Bn = len(prompts)
    pm = max_len - 1
    ids0, _ = stage(prm, lens, Bn * k, k, pm, cls, np.zeros((Bn * k, max_len), dtype=np.int64))
    cur = ids0
    scores = np.tile(np.array([0.0] + [-1e9] * (k - 1), dtype=np.float32), Bn)
    src = np.zeros(Bn * k, dtype=np.int32)
    mem = memory.repeat_interleave(k, dim=0)
    for t in range(max_len - 1):
        logp = torch.log_softmax(forward(torch.as_tensor(cur[:, :t + 1]), mem)[:, -1].float().cpu(), dim=-1).numpy()
        V = logp.shape[1]
        cs, ci = np.zeros(Bn * k, dtype=np.float32), np.zeros(Bn * k, dtype=np.int32)
        for b in range(Bn):
            flat = (scores[b * k:(b + 1) * k, None] + logp[b * k:(b + 1) * k]).reshape(-1)
            order = np.lexsort((np.arange(flat.size), -flat))[:k]
            cs[b * k:(b + 1) * k], ci[b * k:(b + 1) * k] = flat[order], order
        cur, scores, src = beam_step(cs, ci, cur, cur.copy(), scores, src, Bn, k, V, t, (prm_pad(prm, max_len), lens, pm), wrong)
    return cur[::k].copy()


def prm_pad(prm, ld):
    """the prompt table widened to ld columns (the forced step indexes column t + 1 < max_len - 1)"""
    out = np.zeros((prm.shape[0], max(ld, prm.shape[1])), dtype=np.int64)
    out[:, :prm.shape[1]] = prm
    return out
