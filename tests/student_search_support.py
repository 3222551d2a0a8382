"""The certified cases of the student's search that ends hypotheses at SEP (tests/test_student_search.py certifies them on the CPU,
tests/test_student_search_e2e_gpu.py runs them on the device): the tiny student with a scaled head and a raised SEP bias, 3 clips, k = 3, max_len = 8.
Seeds and the bias were searched for on the CPU oracle (oracle/student_oracle.py, bf16 operands) so that the host search alone
shows every path of the bookkeeping and no decision hangs on a score gap below 1e-3."""
from __future__ import annotations

import numpy as np
import torch

K, MAX_LEN, CLIPS = 3, 8, 3
SEED_W, SEED_MEM, SEP_BIAS, HEAD_GAIN = 5, 3, 2.0, 3.0

# search options: A the defaults; D a negative length penalty (shorter is better, and is_done's bound is no upper bound any more, so
# what is kept depends on how long the search goes on) and B = D with two hypotheses kept; C every option at once
OPTS = dict(A=dict(), D=dict(length_penalty=-0.3), B=dict(num_keep_best=2, length_penalty=-0.3),
            C=dict(num_keep_best=3, length_penalty=0.6, per_node_beam_size=2, repetition_penalty=1.3))
# inputs: the clips' frame counts (None: all mem_tokens), prompts (token lists without CLS) and constraints
INPUTS = dict(plain=dict(), min_length=dict(min_length=4), prompts=dict(prompt=[[], [5], [7, 9]]), ragged=dict(frame_counts=[6, 2, 5]))
CASES = [("plain", "A"), ("plain", "D"), ("plain", "B"), ("plain", "C"), ("min_length", "A"), ("prompts", "B"), ("ragged", "C")]
GAP_MIN = 1e-3


def tiny_weights(seed_w=None, sep_bias=None, head_gain=None):
    """The tiny student's synthetic weights with the head's rows scaled by HEAD_GAIN -- next-token distributions with a few likely
    tokens, as a trained model's, instead of near-uniform ones -- and the SEP bias raised."""
    from gitcap.student_config import student_synthetic_weights, student_tiny
    cfg = student_tiny()
    w = dict(student_synthetic_weights(cfg, SEED_W if seed_w is None else seed_w))
    w["linear.weight"] = (w["linear.weight"] * np.float32(HEAD_GAIN if head_gain is None else head_gain)).astype(np.float32)
    bias = np.array(w["linear.bias"], copy=True)
    bias[cfg.sep_token_id] += SEP_BIAS if sep_bias is None else sep_bias
    w["linear.bias"] = bias
    return cfg, w


def clip_memories(cfg, inp, seed_mem=None):
    """One memory tensor [F_b, D] per clip."""
    from oracle.student_oracle import make_memory
    mem = make_memory(CLIPS, cfg.mem_tokens, cfg.d_model, SEED_MEM if seed_mem is None else seed_mem)
    counts = inp.get("frame_counts") or [cfg.mem_tokens] * CLIPS
    return [mem[b, :n].contiguous() for b, n in enumerate(counts)]


def prompt_rows(cfg, inp):
    return [torch.tensor([cfg.cls_token_id] + p, dtype=torch.int64) for p in inp["prompt"]] if "prompt" in inp else None


def oracle_search(cfg, w, inp, opts, seed_mem=None):
    """gitcap.search.eos_beam_search over the CPU oracle's logits -> (result dict, stats)"""
    from gitcap.search import banned_tokens, eos_beam_search
    from oracle.student_oracle import StudentOracle
    oracle = StudentOracle(cfg, w, emulate_bf16=True)
    mems = clip_memories(cfg, inp, seed_mem)
    V, sep, m = cfg.vocab_length, cfg.sep_token_id, inp.get("min_length", 0)

    def step(ids):
        return torch.cat([oracle.forward_decoder(ids[b * K:(b + 1) * K], mems[b][None].expand(K, -1, -1))[:, -1] for b in range(CLIPS)], 0)

    def rule(logits, ids):
        logits = logits.clone()
        for r, pre in enumerate(ids.tolist()):
            logits[r, banned_tokens(pre, 0, m, sep, [], V)] = float("-inf")
        return logits

    rows = prompt_rows(cfg, inp)
    start = [[cfg.cls_token_id]] * CLIPS if rows is None else [r.tolist() for r in rows]
    stats = {}
    res = eos_beam_search(step, start, k=K, max_len=MAX_LEN, sep_id=sep, rule=rule if m else None, stats=stats, **opts)
    return res, stats
