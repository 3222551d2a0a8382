"""Constrained decoding without a GPU: the restatement of tests/constraints_reference.py against HF's logits processors, the host
search operator's options against a loop built on the restatement, the header, and that the inputs of the GPU test of the mask
builder tell the plausible wrong builders apart."""
import os
import re

import numpy as np
import pytest
import torch

import constraints_reference as C
from gitcap import _lib
from gitcap.search import GeneratorWithBeamSearch, banned_tokens, check_constraints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 97


def _planted(rng, rows, L, V):
    """random prefixes with planted repeats: a short motif copied to several places, one of them the tail"""
    ids = rng.integers(0, V, size=(rows, L))
    for r in range(rows):
        m = rng.integers(0, V, size=3)
        for at in (1, 5, L - 3):
            ids[r, at:at + 3] = m
    return ids


def test_restatement_equals_hf_processors():
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(5)
    L = 12
    ids = _planted(rng, 6, L, V)
    ids[0, :] = [7, 8, 9, 7, 8, 9, 3, 7, 8, 9, 7, 8]                    # the 2-gram (7, 8) recurs: three continuations seen, 9 thrice
    sep, sup = 2, [0, 15, 16, V - 1, 15]
    for n in (1, 2, 3, 4):
        proc = lp.NoRepeatNGramLogitsProcessor(n)
        for cur_len in sorted({max(1, n - 2), max(1, n - 1), n, n + 1, 8, L}):
            scores = proc(torch.as_tensor(ids[:, :cur_len]), torch.zeros(ids.shape[0], V))
            for r in range(ids.shape[0]):
                hf = set(torch.nonzero(torch.isinf(scores[r])).reshape(-1).tolist())
                assert C.banned_columns(ids[r], cur_len, n, 0, sep, [], V) == hf, (n, cur_len, r)
    assert C.banned_columns(ids[0], 12, 3, 0, sep, [], V) == {9}        # (7, 8) -> 9 at three places, banned once
    for m in (5, 6):
        for cur_len in (m - 1, m):
            scores = lp.MinLengthLogitsProcessor(m, sep)(torch.as_tensor(ids[:, :cur_len]), torch.zeros(ids.shape[0], V))
            hf = set(torch.nonzero(torch.isinf(scores[0])).reshape(-1).tolist())
            assert C.banned_columns(ids[0], cur_len, 0, m, sep, [], V) == hf == ({sep} if cur_len < m else set())
    scores = lp.SuppressTokensLogitsProcessor(sup)(torch.as_tensor(ids[:, :4]), torch.zeros(ids.shape[0], V))
    assert C.banned_columns(ids[0], 4, 0, 0, sep, sup, V) == set(torch.nonzero(torch.isinf(scores[0])).reshape(-1).tolist())
    # the union, through the mask and back
    mask = C.ban_mask(ids, 9, 2, 12, sep, sup, V)
    got = C.mask_logits(np.zeros((ids.shape[0], V), np.float32), mask)
    for r in range(ids.shape[0]):
        assert set(np.nonzero(np.isinf(got[r]))[0].tolist()) == C.banned_columns(ids[r], 9, 2, 12, sep, sup, V)


def test_host_side_rule_is_the_restatement():
    rng = np.random.default_rng(9)
    ids = _planted(rng, 8, 12, V)
    ids[3, 2] = -1
    ids[4, 4] = V
    for n in (0, 1, 2, 3, 4):
        for cur_len in (1, 2, 3, 4, 9, 12):
            for m in (0, cur_len, cur_len + 1):
                for sup in ([], [0, V - 1, V, -1, 5, 5]):
                    for r in range(ids.shape[0]):
                        want = sorted(C.banned_columns(ids[r], cur_len, n, m, 2, sup, V))
                        assert banned_tokens(ids[r, :cur_len].tolist(), n, m, 2, sup, V) == want
    with pytest.raises(ValueError):
        check_constraints(-1, 0, None)
    with pytest.raises(ValueError):
        check_constraints(0, -2, None)
    with pytest.raises(ValueError):
        check_constraints(0, 0, list(range(257)))
    with pytest.raises(ValueError):
        check_constraints(0, 0, torch.tensor([1.0]))
    assert check_constraints(2, 3, torch.tensor([4, 4], dtype=torch.int32)) == (2, 3, [4, 4])


class _CpuSearch(GeneratorWithBeamSearch):
    """the operator with its one kernel call replaced by torch on the host"""

    def _topk(self, logits, beam_scores, B):
        beams, Vv = self.beam_size, logits.shape[-1]
        sc = torch.log_softmax(logits.double(), -1).float() + beam_scores[:, None]
        s, i = torch.topk(sc.view(B, beams * Vv), self.per_node_beam_size * beams, dim=1)
        return s, i.to(torch.int32)


@pytest.mark.parametrize("kw", [dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2, min_length=6), dict(suppress_tokens=[3, 4, 5, 200]),
                                dict(no_repeat_ngram_size=3, min_length=4, suppress_tokens=[7], repetition_penalty=1.3)])
def test_host_operator_equals_a_loop_on_the_restatement(kw):
    g = torch.Generator().manual_seed(11)
    Vv, sep, cls, B, beams, steps = 40, 2, 1, 2, 3, 9
    table = torch.randn(Vv, Vv, generator=g) * 2
    table[:, sep] += 1.5                                                  # SEP early: min_length bites
    table[torch.arange(Vv), torch.arange(Vv)] += 3.0                    # repeats are attractive: the n-gram rule bites

    def step(ids):
        return table[ids[:, -1]] + 0.1 * ids.shape[1]

    rp = kw.get("repetition_penalty", 1.0)
    n, m, sup = kw.get("no_repeat_ngram_size", 0), kw.get("min_length", 0), kw.get("suppress_tokens", [])

    def masked_step(ids):
        lg = step(ids).numpy()
        mask = C.ban_mask(ids.numpy(), ids.shape[1], n, m, sep, sup, Vv)
        return torch.as_tensor(C.mask_logits(lg, mask))

    start = torch.full((B, 1), cls, dtype=torch.long)
    got = _CpuSearch(sep, steps, beams, 2, 0.6, **kw).search(start, step, num_keep_best=2)
    want = _CpuSearch(sep, steps, beams, 2, 0.6, repetition_penalty=rp).search(start, masked_step, num_keep_best=2)
    free = _CpuSearch(sep, steps, beams, 2, 0.6, repetition_penalty=rp).search(start, step, num_keep_best=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], free[0])                             # the options bite
    for seq in got[0].reshape(-1, steps).tolist():
        body = seq[:seq.index(sep, 1) + 1] if sep in seq[1:] else seq
        assert not (n and C.repeats_ngram(body, n)) and not set(body) & set(sup)
        assert len(body) > m or sep not in seq[1:] or m == 0, (seq, m)


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "gitcap.h")).read()
    src = open(os.path.join(ROOT, "real-time-video-captioning_amd", "csrc", "gitcap.hip")).read()
    assert re.search(r"#define\s+GITCAP_ABI_VERSION\s+1\b", src)           # additions only
    for name in ("gitcap_attach_constraints", "gitcap_dbg_ban_mask", "gitcap_dbg_vocab_head_banned", "gitcap_beam_topk_constrained",
                 "gitcap_sample_rows_constrained"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SYMBOLS
    assert re.search(r"typedef struct gitcap_constraints \{[^}]*no_repeat_ngram_size;[^}]*min_length;[^}]*suppress;[^}]*n_suppress;[^}]*\}", text)
    assert [f for f, _ in _lib.CConstraints._fields_] == ["no_repeat_ngram_size", "min_length", "suppress", "n_suppress"]


def _wrong_builders():
    def no_clear(state, *a):
        state |= C.ban_mask(*a)
        return state.copy()

    def window_off_by_one(state, p, cur_len, n, m, sep, sup, Vv):
        return C.ban_mask(p, cur_len - 1 if n > 1 else cur_len, n, 0, sep, [], Vv) | C.ban_mask(p, cur_len, 0, m, sep, sup, Vv)

    def column_before(state, p, cur_len, n, m, sep, sup, Vv):
        out = C.ban_mask(p, cur_len, 0, m, sep, sup, Vv)
        for r, row in enumerate(p):
            for i in range(0, cur_len - n + 1):
                if n >= 1 and all(int(row[i + j]) == int(row[cur_len - n + 1 + j]) for j in range(n - 1)):
                    c = int(row[i + n - 2]) if n > 1 else -1
                    if 0 <= c < Vv:
                        out[r, c >> 4] |= np.uint16(1 << (c & 15))
        return out

    return dict(no_clear=no_clear, window_off_by_one=window_off_by_one, column_before=column_before)


@pytest.mark.parametrize("Vv", [97, 30522])
def test_gpu_inputs_tell_the_wrong_builders_apart(Vv):
    cases = C.builder_cases(Vv)
    for name, wrong in _wrong_builders().items():
        state = np.zeros((3, C.mask_ld(Vv)), np.uint16)
        differs = False
        for _, p, cur_len, n, m, sep, sup in cases:
            got = wrong(state, p, cur_len, n, m, sep, sup, Vv)
            differs |= not np.array_equal(got, C.ban_mask(p, cur_len, n, m, sep, sup, Vv))
        assert differs, name
    # and what the cases must cover
    first = C.ban_mask(*cases[0][1:], Vv)
    for c in (0, 15, 16, Vv - 1):
        assert (int(first[0, c >> 4]) >> (c & 15)) & 1, c
    if Vv == 30522:
        assert Vv % 16 == 10 and int(first[0, (Vv - 1) >> 4]) >> 10 == 0
    assert not C.ban_mask(*cases[4][1:], Vv).any() and not C.ban_mask(*cases[5][1:], Vv).any()
