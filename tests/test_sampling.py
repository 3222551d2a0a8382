"""Sampling on the device, the part that needs no GPU: the restatements of tests/sampling_reference.py against published vectors,
the oracle and statistics; the library's exports.  The GPU tests hold the kernels to these restatements."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sampling_reference as S
from oracle import search_oracle


def test_library_exports_the_sampling_entry_points():
    from gitcap import _lib
    lib = _lib.load()
    for name in ("gitcap_attach_sampling", "gitcap_sample_rows", "gitcap_dbg_beam_step_sampled"):
        assert hasattr(lib, name), name
    assert [f for f, _ in _lib.CSamplingOptions._fields_] == ["temperature", "top_k", "top_p", "seed"]
    assert ctypes.sizeof(_lib.CSamplingOptions) == 24
    assert lib.gitcap_attach_sampling(None, None) == -1          # a null handle is refused before anything is touched


def test_philox_known_answers():
    """The known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds)."""
    def run(c, k):
        return ["%08x" % x for x in S.philox4x32_10(np.array([c], dtype=np.uint32), k)[0]]
    assert run([0, 0, 0, 0], (0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert run([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert run([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0)) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_uniforms_lie_strictly_inside_the_unit_interval_and_follow_the_counter():
    u = S.uniforms(3, 2, 5, 37)
    assert u.min() > 0 and u.max() < 1 and len(u) == 37
    x = S.philox4x32_10(np.array([[9, 2, 5, 0]], dtype=np.uint32), (3, 0))[0]
    assert u[36] == ((int(x[0]) >> 8) + 0.5) * 2.0 ** -24        # column 36 = lane 0 of counter 9
    assert not np.array_equal(u, S.uniforms(3, 3, 5, 37)) and not np.array_equal(u, S.uniforms(3, 2, 6, 37))
    assert not np.array_equal(u, S.uniforms(3 + 2 ** 32, 2, 5, 37))             # the high word of the seed is the second key word


@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (0, 0.5), (0, 1e-6), (3, 1.0), (1, 1.0), (40, 1.0), (5, 0.7), (0, 0.999)])
def test_filter_by_value_is_the_oracles_filter_on_rows_without_ties(top_k, top_p):
    rng = np.random.default_rng(11)
    for scale in (4.0, 0.25):
        z = rng.standard_normal((6, 33)) * scale
        z[1, ::4] = -np.inf
        ref = search_oracle.top_k_top_p_filtering(torch.from_numpy(z), top_k=top_k, top_p=top_p, min_tokens_to_keep=2).numpy()
        for r in range(6):
            assert np.array_equal(S.filter_by_value(z[r], top_k, top_p), ref[r]), (scale, r)


def test_five_logit_known_answers():
    """The 5-logit rows of tests/test_search.py: top_k = 1 keeps 2 (min_tokens_to_keep), top_p keeps ranks 0..2 at least."""
    z = np.log(np.array([0.5, 0.25, 0.15, 0.07, 0.03]))
    assert (S.filter_by_value(z, 1, 1.0) > -np.inf).tolist() == [True, True, False, False, False]
    assert (S.filter_by_value(z, 0, 0.1) > -np.inf).tolist() == [True, True, True, False, False]
    assert (S.filter_by_value(z, 0, 0.92) > -np.inf).tolist() == [True, True, True, True, False]
    d = S.draw_rows(z[None].astype(np.float32), [0.0], None, 1.0, 1.0, 1, 1.0, 5, 1, 2)
    assert sorted(d["words"][0]) == [0, 1] and d["kept"][0] == 2
    assert abs(d["logz"][0] - math.log(0.75)) < 1e-6


def test_first_draw_frequencies_follow_the_softmax():
    """40 000 rows at V = 16, one seed: chi-square of the first draw's counts against the softmax, at p = 1e-6 (df = 15: 52.0)."""
    V, rows = 16, 40000
    z = np.random.default_rng(3).standard_normal(V)
    p = np.exp(z) / np.exp(z).sum()
    counts = np.zeros(V)
    for r in range(rows):
        key = z - np.log(-np.log(S.uniforms(123456789, r, 1, V)))
        counts[int(np.argmax(key))] += 1
    chi2 = float(((counts - rows * p) ** 2 / (rows * p)).sum())
    print("chi2 = %.2f" % chi2)
    assert chi2 < 52.0


def test_pair_frequencies_are_those_of_sampling_without_replacement():
    """V = 4, pn = 2: ordered pairs against p_i * p_j / (1 - p_i); chi-square at p = 1e-6 (df = 11: 43.2)."""
    z = np.array([0.3, -0.5, 1.1, 0.0])
    p = np.exp(z) / np.exp(z).sum()
    rows, counts = 30000, np.zeros((4, 4))
    for r in range(rows):
        a, b = S._top(z - np.log(-np.log(S.uniforms(42, r, 3, 4))), 2)
        counts[a, b] += 1
    exp = np.array([[0 if i == j else rows * p[i] * p[j] / (1 - p[i]) for j in range(4)] for i in range(4)])
    off = ~np.eye(4, dtype=bool)
    chi2 = float(((counts[off] - exp[off]) ** 2 / exp[off]).sum())
    print("chi2 = %.2f" % chi2)
    assert counts.trace() == 0 and chi2 < 43.2


def _toy_step(table, beams):
    def step(ids):
        return torch.from_numpy(S.toy_logits(table, ids[:, -1].numpy(), beams, ids.shape[1]))
    return step


def _forced(beams):
    """Draws no sampler without replacement would make -- EOS twice in a row -- so that a clip is left with no live beam (clip 0) and
    with one (clip 2) at step 1: {(cur_len, row): words}."""
    E = S.TOY_EOS
    f = {(1, r): [E, E] for r in range(beams)}
    f.update({(1, 2 * beams + r): [E, E] for r in range(beams - 1)})
    f[(1, 3 * beams - 1)] = [E, 5]
    return f


def _forcing(base, forced):
    state = {"cur_len": 1}

    def multinomial(probs, num_samples, replacement=False, *, generator=None):
        out = base(probs, num_samples)
        for (cl, r), w in forced.items():
            if cl == state["cur_len"]:
                out[r] = torch.tensor(w)
        state["cur_len"] += 1
        return out
    return multinomial


@pytest.mark.parametrize("n,beams,top_k,top_p,T,rp,force", [(1, 2, 0, 1.0, 1.0, 1.0, False), (3, 4, 5, 1.0, 0.7, 1.3, False),
                                                             (2, 3, 0, 0.9, 2.0, 1.0, False), (1, 4, 0, 1.0, 1.0, 1.0, True),
                                                             (3, 2, 0, 1.0, 1.0, 1.3, True)])
def test_patched_oracle_host_operator_and_restated_loop_agree(monkeypatch, n, beams, top_k, top_p, T, rp, force):
    """torch.multinomial replaced by the contract's draws: oracle.search_oracle.beam_search(do_sample=True) = the host operator =
    draw_rows + Book (the unsorted bookkeeping on the device's state).  force: with EOS drawn by every row of clip 0 (kept == 0: all
    beams padded) and by all but one draw of clip 2 (0 < kept < beams: only the missing beams padded) at step 1."""
    from gitcap.search import GeneratorWithBeamSearch
    table, seed, lp, pn = S.toy_table(), 2024, 0.6, 2
    forced = _forced(beams) if force else {}
    start = torch.full((S.TOY_B, 1), S.TOY_CLS)
    monkeypatch.setattr(torch, "multinomial", _forcing(S.multinomial_from_philox(seed), forced))
    dec, lps, _ = search_oracle.beam_search(start, _toy_step(table, beams), eos_index=S.TOY_EOS, max_steps=S.TOY_L, beam_size=beams,
                                            per_node_beam_size=pn, length_penalty=lp, num_keep_best=n, repetition_penalty=rp,
                                            temperature=T, do_sample=True, top_k=top_k, top_p=top_p)
    monkeypatch.setattr(torch, "multinomial", _forcing(S.multinomial_from_philox(seed), forced))
    host = GeneratorWithBeamSearch(S.TOY_EOS, S.TOY_L, beams, pn, lp, repetition_penalty=rp, temperature=T)
    hdec, hlps, _ = host.search(start, _toy_step(table, beams), num_keep_best=n, do_sample=True, top_k=top_k, top_p=top_p)
    assert torch.equal(hdec, dec) and torch.allclose(hlps, lps, atol=1e-5)
    book = S.Book(S.TOY_B, beams, n, S.TOY_L, S.TOY_CLS, S.TOY_EOS, lp)
    partial = empty = 0
    for cur_len in range(1, S.TOY_L):
        ci, cs = S.toy_candidates(table, book, beams, pn, rp, T, top_k, top_p, seed, cur_len, forced)
        was_done = list(book.done)
        book.step(cs, ci, S.TOY_V, cur_len)
        for b in range(S.TOY_B):
            live = sum(w != S.TOY_EOS for w in book.words[b * beams:(b + 1) * beams])
            if not was_done[b] and not book.done[b] and cur_len + 1 < S.TOY_L:
                partial += 0 < live < beams
                empty += live == 0
    bdec, blps = book.finish()
    if n == 1:
        bdec = bdec[:, 0]
    assert np.array_equal(bdec, dec.numpy()), (bdec, dec)
    assert np.allclose(blps, lps.numpy(), atol=1e-4)
    print("clips padded partially / wholly:", partial, empty)
    assert (partial >= 1 and empty >= 1) == force


def test_gpu_inputs_stay_inside_the_undecidable_cap():
    """On the very inputs of tests/test_sampling_gpu.py at most 1 % of a case's rows may be undecidable (with <= 8 rows: none)."""
    worst = 0
    for c in S.row_cases():
        d = S.case_reference(c)
        rows = len(d["kept"])
        bad = sum(not all(S.decidable(d, r)) for r in range(rows))
        worst = max(worst, bad)
        assert bad * 100 <= rows, (c["id"], bad, rows)
    print("most undecidable rows in a case:", worst)
