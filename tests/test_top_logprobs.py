"""The top-k alternatives' restatement (tests/top_logprobs_reference.py) against torch, the kernel's tile plan against the
restatement, and the inputs of tests/test_top_logprobs_gpu.py against four wrong kernels: each must differ from the right answer
on at least one of them."""
import numpy as np
import pytest
import torch

import top_logprobs_reference as T

TOL = 2e-5          # nats: the bound tests/logprob_reference.py derives for a merged log-sum-exp


@pytest.mark.parametrize("V,k", [(40, 1), (40, 8), (1000, 8), (30522, 32)])
def test_restatement_is_topk_of_log_softmax(V, k):
    g = torch.Generator().manual_seed(V + k)
    lg = (torch.randn(3, V, generator=g, dtype=torch.float64) * 3).float()          # tie-free
    ref = torch.log_softmax(lg.double(), 1)
    want_lp, want_ids = torch.topk(ref, k, dim=1)
    for m in range(3):
        M, lpw = T.winner_stats(lg[m].numpy())
        ids, lp = T.top_k(lg[m].numpy(), M, lpw, k)
        assert ids.tolist() == want_ids[m].tolist()
        assert np.abs(lp.astype(np.float64) - want_lp[m].numpy()).max() <= TOL
        assert lp[0] == lpw                                                         # rank 0: (M - M) + lp_winner


def test_restatement_ties_and_padding():
    lg = np.array([1.0, 3.0, -np.inf, 3.0, 2.0, 3.0], np.float32)
    ids, lp = T.top_k(lg, 3.0, -0.5, 8)
    assert ids.tolist() == [1, 3, 5, 4, 0, -1, -1, -1]
    assert lp[:5].tolist() == [-0.5, -0.5, -0.5, -1.5, -2.5] and np.isneginf(lp[5:]).all()
    ids, lp = T.top_k(np.full(4, -np.inf, np.float32), -np.inf, -np.inf, 2)
    assert ids.tolist() == [-1, -1] and np.isneginf(lp).all() and not np.isnan(lp).any()


CASES = [(1, 40, 64), (18, 40, 64), (18, 1000, 128), (2, 30522, 768)]


@pytest.mark.parametrize("M,V,D", CASES)
@pytest.mark.parametrize("scenario", T.SCENARIOS)
def test_tile_plan_is_the_restatement(M, V, D, scenario):
    """the k best columns lie in the k best tiles by representative: the kernel's plan gives the plain top-k, ties and bans included"""
    case = T.head_case(M, V, D, scenario)
    for m in (0, M - 1):
        lg = T.masked(case, m)
        Mx, lpw = T.winner_stats(lg)
        for k in (1, 2, 8, 32):
            want = T.top_k(lg, Mx, lpw, k)
            got = T.tile_plan_top_k(case["logits"][m], V, None if case["ban"] is None else case["ban"][m], Mx, lpw, k)
            assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]), (scenario, m, k)


def _differs(wrong, M, V, D, scenario, ks=(1, 2, 8, 32)):
    case = T.head_case(M, V, D, scenario)
    for m in range(M):
        lg = T.masked(case, m)
        Mx, lpw = T.winner_stats(lg)
        for k in ks:
            got = T.tile_plan_top_k(case["logits"][m], V, None if case["ban"] is None else case["ban"][m], Mx, lpw, k, wrong=wrong)
            if got[0].tolist() != T.top_k(lg, Mx, lpw, k)[0].tolist():
                return True
    return False


def test_inputs_separate_the_wrong_kernels():
    # tiles picked without the index tie-break: ranks 1 and 2 of "spread" are equal logits in different tiles, k = 2 keeps one
    assert _differs("tile_ties", 18, 1000, 128, "spread", ks=(2,))
    assert _differs("tile_ties", 2, 30522, 768, "spread", ks=(2,))
    # one candidate per tile: five of the eight best share a tile
    assert _differs("one_per_tile", 18, 1000, 128, "cluster", ks=(8,))
    assert _differs("one_per_tile", 1, 40, 64, "cluster", ks=(8,))
    # columns >= V admitted: the padded weight rows hold the largest values (V = 40: 8 padded rows, 30522: 6)
    assert _differs("padding", 1, 40, 64, "natural")
    assert _differs("padding", 2, 30522, 768, "cluster")
    # the ban word ignored: the winner is banned / three columns are left
    assert _differs("no_ban", 18, 1000, 128, "ban_winner", ks=(1,))
    assert _differs("no_ban", 1, 40, 64, "ban_keep3", ks=(8,))


def test_ban_keep3_pads_with_minus_one():
    case = T.head_case(18, 1000, 128, "ban_keep3")
    for m in range(18):
        lg = T.masked(case, m)
        ids, lp = T.top_k(lg, *T.winner_stats(lg), 8)
        assert (ids[:3] >= 0).all() and (ids[3:] == -1).all() and np.isneginf(lp[3:]).all() and np.isfinite(lp[:3]).all()


def test_pack_ban_bits():
    ban = np.zeros((2, 40), bool)
    ban[0, [0, 17, 39]] = True
    ban[1, 15] = True
    m = T.pack_ban(ban, 4)
    assert m.tolist() == [[1, 2, 1 << 7, 0], [1 << 15, 0, 0, 0]]
