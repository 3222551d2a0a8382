"""Prompted decoding on the CPU: the restatement of tests/prompt_reference.py against direct loops and the search oracle, the C ABI's
new symbols, and proof that the inputs tests/test_prompt_gpu.py uses catch the subtly wrong kernels."""
import copy

import numpy as np
import pytest
import torch

import prompt_reference as P
import selection_reference as R
from oracle import search_oracle

V, STEPS = 16 * 9 - 1, 9                # a vocabulary that ends inside a tile


def _logits_of(seed):
    table = np.random.default_rng(seed).standard_normal((64, V)).astype(np.float32)
    table[:, 3] = -np.inf               # a masked column
    table[7] = -np.inf                  # a masked row: token 0
    table[11, P.SEP] = 9.0              # rows that emit SEP
    table[12, P.SEP] = 9.0

    def f(ids, t):
        return table[(ids[:, -1] * 7 + 3 * t) % 64]
    return f


def test_symbols_and_keywords():
    from gitcap import _lib
    from gitcap.model import GitCaptioner
    import inspect
    for name in ("gitcap_attach_prompt", "gitcap_dbg_argmax_final_forced", "gitcap_dbg_beam_step_forced"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    for fn in ("greedy_decode", "greedy_decode_async", "infer", "infer_async", "caption_stream"):
        assert {"prompt", "prompt_lengths"} <= set(inspect.signature(getattr(GitCaptioner, fn)).parameters), fn


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_forced_selection_restatement_vs_direct_loop(seed):
    rng = np.random.default_rng(seed)
    B = 5
    lengths = np.array([1, 2, 4, STEPS, 3], np.int32)
    prompt = rng.integers(0, V, (B, STEPS + 1)).astype(np.int64)
    prompt[:, 0] = P.CLS
    prompt[2, 2] = P.SEP                 # a forced SEP
    f = _logits_of(seed)
    ids_d, sep_d = P.greedy_direct(f, B, STEPS, prompt, lengths, P.SEP)
    ids_r, sep_r = P.greedy_restated(f, B, STEPS, prompt, lengths, STEPS, P.SEP)
    assert np.array_equal(ids_d, ids_r) and sep_d == sep_r
    for b in range(B):
        assert np.array_equal(ids_d[b, :lengths[b]], prompt[b, :lengths[b]])
    plain, _ = P.greedy_direct(f, B, STEPS, prompt, np.ones(B, np.int32), P.SEP)
    assert np.array_equal(plain[0], ids_d[0]) and not np.array_equal(plain[3], ids_d[3])
    # a length beyond max_len is clamped: nothing behind max_len is forced
    ids_c, _ = P.greedy_restated(f, B, STEPS, prompt, np.full(B, 99, np.int32), 3, P.SEP)
    assert np.array_equal(ids_c[:, :3], prompt[:, :3])
    ids_3, _ = P.greedy_restated(f, B, STEPS, prompt, np.full(B, 3, np.int32), 3, P.SEP)
    assert np.array_equal(ids_c, ids_3)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("plen", [1, 2, 4])
def test_forced_beam_steps_vs_search_oracle_started_from_the_prompt(plen, n):
    """A batch-of-one prompt: forced steps 1 .. plen - 1, then free steps on the oracle's candidates == the oracle's search
    started from that prompt (model.py:436-437)."""
    beams, pnb, L, lp, eos, Vt = 3, 2, 9, 0.6, P.SEP, 50
    K = beams * pnb
    table = torch.from_numpy(np.random.default_rng(plen).standard_normal((97, Vt)).astype(np.float32) * 2.0)

    def step(ids):
        return table[(ids[:, -1] * 5 + ids.shape[1] * 11 + ids[:, 0]) % 97]

    prompt = np.array([[P.CLS, 17, 23, 8, 31]], np.int64)
    start = torch.from_numpy(prompt[:, :plen])
    dec, lps, _ = search_oracle.beam_search(start, step, eos_index=eos, max_steps=L, beam_size=beams, per_node_beam_size=pnb,
                                            length_penalty=lp, num_keep_best=n)
    st = P.beam_init(1, beams, n, L)
    lengths = np.array([plen], np.int32)
    cur = 0
    for cur_len in range(1, L):
        ids = st["ids1" if cur else "ids0"][:, :cur_len]
        cs = ci = np.zeros((1, K))
        if cur_len >= plen:
            logits = step(torch.from_numpy(ids.copy())).numpy()
            cs, ci, _ = R.beam_candidates(logits, st["beam_scores"], beams, K)
        P.beam_step(st, n, cs.astype(np.float32), ci, 1, beams, K, Vt, cur_len, L, eos, lp, cur, prompt=prompt, lengths=lengths,
                    prompt_max_len=max(plen, 1))
        cur ^= 1
    got, got_lp = P.beam_finish(st, n, 1, L, eos)
    want = dec.numpy().reshape(1, n, L)
    assert np.array_equal(got, want), (got, want)
    assert np.allclose(got_lp, lps.numpy().reshape(1, n), atol=1e-5)
    assert np.array_equal(got[0, 0, :plen], prompt[0, :plen])


# ---- the GPU inputs catch the wrong kernels ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [9, 257])
def test_selection_inputs_catch_the_wrong_kernels(nt):
    val, idx, prompt, lengths = P.selection_inputs(nt)
    seen = {"le": False, "count_sep": False}
    for step in (P.SEL_STEP - 1, P.SEL_STEP):
        toks, forced, n_sep = P.forced_select(val, idx, prompt, lengths, P.SEL_MAX_LEN, step, P.SEP)
        for fault in seen:
            t2, f2, s2 = P.forced_select(val, idx, prompt, lengths, P.SEL_MAX_LEN, step, P.SEP, fault)
            seen[fault] |= (t2, s2) != (toks, n_sep)
    assert all(seen.values()), seen
    # what the docstring promises about the rows
    toks, forced, n_sep = P.forced_select(val, idx, prompt, lengths, P.SEL_MAX_LEN, P.SEL_STEP, P.SEP)
    assert forced == [False, False, False, True] and toks[3] == P.SEP and toks[1] == P.SEP and toks[2] == 0 and n_sep == 1
    assert toks[0] == idx[0, nt - 1]
    toks, forced, _ = P.forced_select(val, idx, prompt, lengths, P.SEL_MAX_LEN, P.SEL_STEP - 1, P.SEP)
    assert forced == [False, False, True, True] and toks[3] == R.argmax_partials(val[3], idx[3])


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("beams", [2, 4])
def test_beam_inputs_catch_the_wrong_kernels(beams, n, sampled):
    st0, cs, ci, prompt, lengths, c = P.beam_inputs(beams, n, sampled)

    def run(fault=None):
        st = copy.deepcopy(st0)
        P.beam_step(st, n, cs, ci, c["B"], c["beams"], c["K"], c["V"], c["cur_len"], c["L"], c["eos"], c["lp"], c["cur"], sampled,
                    prompt, lengths, c["pmax"], fault)
        return st
    right = run()
    same = lambda a, b: all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    for fault in ("le", "add_hyp", "touch_scores"):
        assert not same(right, run(fault)), fault
    # the forced clip: appended its prompt token, identity rows, scores / hypotheses / done untouched
    nb = c["beams"]
    assert (right["words"][:nb] == prompt[0, c["cur_len"]]).all() and (right["src_rows"][:nb] == np.arange(nb)).all()
    assert np.array_equal(right["beam_scores"][:nb], st0["beam_scores"][:nb]) and np.array_equal(right["hyp_len"][0], st0["hyp_len"][0])
    assert right["hyp_len"][1].max() == c["cur_len"]              # the free clip stored its EOS candidate
    assert right["done"].tolist() == [0, 0, 1] and (right["words"][2 * nb:] == c["eos"]).all()
