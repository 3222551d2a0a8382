"""The student's search that ends hypotheses at SEP, on the CPU: gitcap.search.eos_beam_search -- the logic of
StudentCaptioner.beam_search_host(eos=True), device free -- against the search operator of oracle/search_oracle.py on random logits,
and the certification of the cases tests/test_student_search_e2e_gpu.py runs on the device (tests/student_search_support.py)."""
import functools

import pytest
import torch

import student_search_support as S
from gitcap.search import eos_beam_search
from oracle.search_oracle import beam_search as oracle_search

V, SEP, CLS = 23, 2, 1


def table_step(seed, quantum):
    """logits as a fixed function of a row's prefix.  quantum > 0: every logit below the row's 7 largest is rounded down to a multiple
    of it, so that the rows are full of equal logits.  A clip takes k * pn = 6 candidates, at most 6 of one row, so the ties are in
    every ranking's input but below its cut: torch.topk, which the oracle ranks with, leaves the order of equal values open."""
    def row(prefix):
        g = torch.Generator().manual_seed(hash((seed,) + tuple(prefix)) % (2 ** 31))
        x = torch.randn(V, generator=g) * 2.0
        x[SEP] += 1.5
        if quantum:
            low = x < x.sort(descending=True).values[6]
            x[low] = torch.floor(x[low] / quantum) * quantum
        return x
    return lambda ids: torch.stack([row(r) for r in ids.tolist()], 0)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("length_penalty", [1.0, 0.6])
@pytest.mark.parametrize("rp", [1.0, 1.3])
@pytest.mark.parametrize("quantum", [0.0, 0.5])
def test_host_search_equals_the_oracle_operator(n, length_penalty, rp, quantum):
    B, k, pn, L = 3, 3, 2, 9
    step = table_step(7 * n + int(10 * length_penalty) + int(10 * rp), quantum)
    got = eos_beam_search(step, [[CLS]] * B, k=k, max_len=L, sep_id=SEP, length_penalty=length_penalty, num_keep_best=n,
                          per_node_beam_size=pn, repetition_penalty=rp)
    dec, lp, _ = oracle_search(torch.full((B, 1), CLS, dtype=torch.long), step, eos_index=SEP, max_steps=L, beam_size=k, per_node_beam_size=pn,
                               length_penalty=length_penalty, num_keep_best=n, repetition_penalty=rp)
    assert torch.equal(got["predictions"], dec.view(B, n, L))
    assert torch.equal(got["scores"], lp)
    stored = got["scores"] > -1e4
    assert bool(stored.any()) and torch.equal(got["lengths"] > 0, stored)
    # a stored hypothesis is its tokens, then SEP to the end
    for b in range(B):
        for r in range(n):
            assert bool((got["predictions"][b, r, int(got["lengths"][b, r]):] == SEP).all())


@functools.lru_cache(maxsize=None)
def certified():
    cfg, w = S.tiny_weights()
    return {case: S.oracle_search(cfg, w, S.INPUTS[case[0]], S.OPTS[case[1]]) for case in S.CASES}


def test_certified_cases_show_every_path_of_the_bookkeeping():
    """Over the cases: a clip done before the last step; a clip none of whose hypotheses was finished by SEP (all stored at the last
    step, where every candidate finishes one: a clip always stores some); a stored hypothesis displaced by a better one."""
    stats = [st for _, st in certified().values()]
    assert any(d is not None and d < S.MAX_LEN - 1 for st in stats for d in st["done_step"])
    assert any(c == 0 for st in stats for c in st["sep_hyps"])
    assert any(c > 0 for st in stats for c in st["displaced"])


def test_two_kept_hypotheses_change_rank_0_on_some_clip():
    """Under the negative length penalty of option sets D / B: with one hypothesis kept a clip is done as soon as it holds one, with
    two the search goes on and finds a better one.  (For length penalties >= 0 is_done's bound is an upper bound of every later
    hypothesis's score, and rank 0 cannot depend on num_keep_best.)"""
    one, two = certified()[("plain", "D")][0], certified()[("plain", "B")][0]
    assert bool((one["predictions"][:, 0] != two["predictions"][:, 0]).any(dim=-1).any())


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "-".join(c))
def test_certified_cases_decide_nothing_on_a_close_score(case):
    _, st = certified()[case]
    print(case, "smallest deciding gap", st["min_gap"])
    assert st["min_gap"] >= S.GAP_MIN
