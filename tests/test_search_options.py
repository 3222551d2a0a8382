"""tests/search_options_reference.py against oracle/search_oracle.py, on the CPU: the fp32 restatement of the repetition penalty
is the oracle's loop bit for bit, every planted fault changes what the GPU test expects, and the toy tables make the n-best
container do what the GPU test is about."""
import numpy as np
import pytest
import torch

import search_options_reference as S
import selection_reference as R
from oracle import search_oracle

CASES = S.topk_cases()


class _Capture:
    """Stands in for torch.nn.functional inside the oracle: records what reaches log_softmax -- the penalised scores."""

    def __init__(self):
        self.rows = []

    def log_softmax(self, x, dim):
        self.rows.append(x.detach().clone())
        return torch.nn.functional.log_softmax(x, dim=dim)

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)


@pytest.mark.parametrize("rp", [1.5, 0.5, 1.7, 1.3])
def test_penalize_is_the_oracles_loop_bit_for_bit(monkeypatch, rp):
    """The oracle's loop (search_oracle.py:101-107) runs inside beam_search: drive a search whose step function returns recorded
    logits and compare what the oracle hands to log_softmax with penalize() of the same logits and prefixes."""
    cap = _Capture()
    monkeypatch.setattr(search_oracle, "F", cap)
    g = torch.Generator().manual_seed(int(rp * 10))
    B, beams, V, L = 2, 3, 37, 6
    fed = []

    def step(ids):
        x = torch.randn(ids.shape[0], V, generator=g) * 3.0
        x[:, 5] = 0.0                       # an exact zero and a -inf that the prefixes reach
        x[:, 7] = float("-inf")
        x[0, ids[0, -1]] = 4.0
        fed.append((ids.clone(), x.clone()))
        return x

    start = torch.tensor([[5], [7]])
    search_oracle.beam_search(start, step, eos_index=V - 1, max_steps=L, beam_size=beams, per_node_beam_size=2, length_penalty=0.6,
                              num_keep_best=2, repetition_penalty=rp)
    assert len(fed) == len(cap.rows) >= 3
    hit = 0
    for (ids, x), got in zip(fed, cap.rows):
        want = S.penalize(x.numpy(), ids.numpy(), rp)
        assert got.dtype == torch.float32
        assert np.array_equal(want.view(np.uint32), got.numpy().view(np.uint32))
        hit += int((want != x.numpy()).sum())
    assert hit > 0


def test_penalize_rules_by_hand():
    x = np.array([[2.0, -2.0, 0.0, float("-inf"), 3.0, 1.0]], np.float32)
    got = S.penalize(x, [[0, 1, 2, 3, 0, 0, -1, 6, 2 ** 33 + 5]], 2.0)
    assert got.tolist() == [[1.0, -4.0, 0.0, float("-inf"), 3.0, 1.0]]
    assert S.penalize(x, [[4]], np.float32(0.5)).tolist() == [[2.0, -2.0, 0.0, float("-inf"), 6.0, 1.0]]
    assert x.tolist()[0][0] == 2.0          # the input is not written


@pytest.mark.parametrize("name", sorted(CASES))
def test_topk_cases_keep_their_candidates_apart(name):
    """The input condition of tests/test_selection_gpu.py: distinct candidate scores more than 1e-3 apart, and here also: the
    penalty changes the winners (a kernel that ignored it would fail), and prefix columns behind cur_len would change them again."""
    c = CASES[name]
    pre = c["prefix"][:, :c["cur_len"]]
    ws, wi, gap = S.expected_candidates(c["x"], c["bs"], pre, c["rp"], c["beams"], c["K"])
    assert float(gap.min()) > 1e-3, (name, gap)
    assert not (wi == R.SENTINEL).any()
    _, raw_i, _ = R.beam_candidates(c["x"], c["bs"], c["beams"], c["K"])
    assert not np.array_equal(wi, raw_i)
    if c["prefix"].shape[1] > c["cur_len"]:
        fs, fi, _ = S.expected_candidates(c["x"], c["bs"], c["prefix"], c["rp"], c["beams"], c["K"])
        assert not np.array_equal(wi, fi) or np.abs(ws - fs).max() > 1e-3


@pytest.mark.parametrize("fault", sorted(S.FAULT_CASES))
def test_planted_faults_change_the_expected_output(fault):
    c = CASES[S.FAULT_CASES[fault]]
    pre = c["prefix"][:, :c["cur_len"]]
    ws, wi, _ = S.expected_candidates(c["x"], c["bs"], pre, c["rp"], c["beams"], c["K"])
    fs, fi, _ = S.expected_candidates(c["x"], c["bs"], pre, c["rp"], c["beams"], c["K"], fault=fault)
    assert not np.array_equal(wi, fi), fault
    assert np.abs(ws - fs).max() > 1e-2, fault            # a hundred times the bar the GPU test holds the scores to


def test_ignored_ids_would_matter_if_used():
    c = CASES["ignored_ids"]
    V = c["x"].shape[1]
    pre = c["prefix"][:, :c["cur_len"]]
    assert {-1, V} <= set(pre[0].tolist())
    _, wi, _ = S.expected_candidates(c["x"], c["bs"], pre, c["rp"], c["beams"], c["K"])
    wrapped = np.where((pre < 0) | (pre >= V), pre % 2 ** 32 % 2048, pre)          # truncated / chunk-relative readings of the same ids
    _, fi, _ = S.expected_candidates(c["x"], c["bs"], wrapped, c["rp"], c["beams"], c["K"])
    assert not np.array_equal(wi, fi)


def test_toy_tables_exercise_the_nbest_container():
    """On the oracle alone: a clip holds fewer than n hypotheses for several steps, an eviction happens, a candidate is rejected at
    the strict >, and with n = 3 a clip is not done at the step where n = 1 is."""
    table = S.toy_table()
    _, _, _, one = S.toy_search(table, 4, 0.6, 1, 1.0)
    dec, lps, _, three = S.toy_search(table, 4, 0.6, 3, 1.0)
    assert max(three["short"]) >= 3
    assert sum(three["evicted"]) >= 1 and sum(three["rejected"]) >= 1
    assert one["done_at"][0] == 2 and three["done_at"][0] != 2
    assert any(a is not None and a != b for a, b in zip(one["done_at"], three["done_at"]))
    assert dec.shape == (S.TOY_B, 3, S.TOY_MAXLEN) and lps.shape == (S.TOY_B, 3)


@pytest.mark.parametrize("cfg", S.toy_configs(), ids=lambda c: "n%d_b%d_lp%s_rp%s" % c)
def test_toy_search_scores_are_apart(cfg):
    """torch.topk defines no order among equal scores: the stored scores of every clip are more than 1e-3 apart."""
    n, beams, lp, rp = cfg
    _, lps, _, _ = S.toy_search(S.toy_table(), beams, lp, n, rp)
    for b in range(S.TOY_B):
        v = sorted(x for x in lps[b].tolist() if x > -1e4)
        assert all(hi - lo > 1e-3 for lo, hi in zip(v, v[1:])), (cfg, b, v)
