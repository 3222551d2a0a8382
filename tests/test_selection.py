"""tests/selection_reference.py is the yardstick of tests/test_selection_gpu.py; here it is held against torch.argmax /
torch.topk on tie-free inputs and against hand-worked tie cases, so that it is not taken on trust."""
import numpy as np
import torch

import selection_reference as R

NINF = float("-inf")


def test_argmax_first_and_tile_partials_vs_torch_on_tie_free_rows():
    g = torch.Generator().manual_seed(0)
    for M, N in [(1, 1), (3, 16), (2, 17), (5, 997), (4, 48)]:
        x = torch.randn(M, N, generator=g, dtype=torch.float64)
        assert x.unique().numel() == x.numel()
        assert [R.argmax_first(r) for r in x.numpy()] == x.argmax(dim=1).tolist()
        val, idx = R.tile_partials(x.numpy())
        nt = (N + 15) // 16
        assert val.shape == idx.shape == (M, nt)
        for t in range(nt):
            blk = x[:, t * 16:(t + 1) * 16]
            assert np.array_equal(val[:, t], blk.max(dim=1).values.numpy())
            assert idx[:, t].tolist() == (blk.argmax(dim=1) + t * 16).tolist()
        assert [R.argmax_partials(v, i) for v, i in zip(val, idx)] == x.argmax(dim=1).tolist()


def test_argmax_hand_worked_ties_and_empty_rows():
    assert R.argmax_first([]) == 0
    assert R.argmax_first([NINF, NINF, NINF]) == 0
    assert R.argmax_first([1.0, 3.0, 3.0, 2.0]) == 1
    assert R.argmax_first([NINF, -5.0, NINF, -5.0]) == 1
    assert R.argmax_first([2.0] * 7) == 0
    # 20 columns = tiles {0..15}, {16..19}; ties inside a tile and across the two
    row = np.full((1, 20), -1.0)
    row[0, [3, 9, 18, 19]] = 4.0
    val, idx = R.tile_partials(row)
    assert val.tolist() == [[4.0, 4.0]] and idx.tolist() == [[3, 18]]
    assert R.argmax_partials(val[0], idx[0]) == 3
    # a tile without a value above -inf carries the sentinel; a row of such tiles gives token 0
    row = np.full((1, 33), NINF)
    val, idx = R.tile_partials(row)
    assert idx.tolist() == [[R.SENTINEL] * 3] and R.argmax_partials(val[0], idx[0]) == 0
    row[0, 32] = -7.0
    val, idx = R.tile_partials(row)
    assert idx.tolist() == [[R.SENTINEL, R.SENTINEL, 32]] and R.argmax_partials(val[0], idx[0]) == 32
    # the rule is on the stored index, not on the position of the partial
    assert R.argmax_partials([1.0, 5.0, 5.0, 5.0], [0, 40, 20, 30]) == 20
    assert R.argmax_partials([], []) == 0
    assert R.argmax_partials([NINF, NINF], [7, 5]) == 5             # equal values (-inf): still the smallest index


def test_draft_accept_hand_worked():
    sep = 9
    # B = 2, n = 4, ld = 6 (one spare column); row 0 agrees at 3 positions, row 1 at 1 -> a = 1, covered = 2
    ids = np.array([[1, 5, 6, 7, 8, 77], [1, 5, 2, 7, 8, 77]])
    tok = np.array([[5, 6, 7, 3], [5, 4, 7, 8]])
    r = R.draft_accept(tok, ids, sep)
    assert r["a_r"] == [3, 1] and r["a"] == 1 and r["covered"] == 2
    assert r["ids"].tolist() == [[1, 5, 6, 7, 8, 77], [1, 5, 4, 7, 8, 77]]
    assert r["sep_cnt"] == [0, 0] and r["host"] == (1, 0)
    # a = 0: the first token is the model's own; all rows emit SEP there -> fired
    r = R.draft_accept(np.array([[sep, 2], [sep, 3]]), np.array([[1, 4, 2], [1, sep, 4]]), sep)
    assert r["a_r"] == [0, 1] and r["a"] == 0 and r["covered"] == 1 and r["sep_cnt"] == [2] and r["host"] == (0, 1)
    assert r["ids"].tolist() == [[1, sep, 2], [1, sep, 4]]
    # a = n: every position accepted, covered = n; SEP in different steps does not fire
    r = R.draft_accept(np.array([[sep, 2], [3, sep]]), np.array([[1, sep, 2], [1, 3, sep]]), sep)
    assert r["a"] == 2 and r["covered"] == 2 and r["sep_cnt"] == [1, 1] and r["host"] == (2, 0)
    # a staged -1 equals no token; SEP of all rows beyond `covered` does not fire
    r = R.draft_accept(np.array([[4, sep, sep]]), np.array([[1, 4, -1, sep]]), sep)
    assert r["a"] == 1 and r["covered"] == 2 and r["sep_cnt"] == [0, 1] and r["host"] == (1, 1)
    r = R.draft_accept(np.array([[4, 5, sep]]), np.array([[1, -1, 5, sep]]), sep)
    assert r["a"] == 0 and r["covered"] == 1 and r["sep_cnt"] == [0] and r["host"] == (0, 0)
    assert r["ids"].tolist() == [[1, 4, 5, sep]]


def test_beam_candidates_vs_torch_topk_on_tie_free_inputs():
    g = torch.Generator().manual_seed(3)
    for B, beams, V, K in [(2, 3, 50, 6), (1, 1, 9, 2), (3, 4, 257, 8), (1, 16, 33, 16)]:
        logits = torch.randn(B * beams, V, generator=g, dtype=torch.float64) * 3
        bs = torch.randn(B * beams, generator=g, dtype=torch.float64)
        ref = (torch.log_softmax(logits, -1) + bs[:, None]).view(B, beams * V)
        rs, ri = ref.topk(K, dim=1)
        s, i, gap = R.beam_candidates(logits.numpy(), bs.numpy(), beams, K)
        assert np.array_equal(i, ri.numpy())
        assert np.allclose(s, rs.numpy(), rtol=0, atol=1e-12)
        top = ref.topk(K + 1, dim=1).values.numpy()
        assert np.allclose(gap, (-np.diff(top, axis=1)).min(axis=1), rtol=0, atol=1e-12)


def test_beam_candidates_hand_worked_ties_and_masks():
    ln = np.log
    # one beam, V = 4, equal logits: uniform distribution, ties by index
    s, i, gap = R.beam_candidates(np.zeros((1, 4)), [0.0], 1, 3)
    assert i.tolist() == [[0, 1, 2]] and np.allclose(s, -ln(4)) and gap[0] == np.inf
    # two beams with identical rows and scores: the lower beam's candidate comes first at every level
    row = ln(np.array([0.5, 0.125, 0.25, 0.125]))
    s, i, gap = R.beam_candidates(np.stack([row, row]), [-1.0, -1.0], 2, 4)
    assert i.tolist() == [[0, 4, 2, 6]]
    assert np.allclose(s[0], [ln(0.5) - 1, ln(0.5) - 1, ln(0.25) - 1, ln(0.25) - 1])
    assert np.isclose(gap[0], ln(2))                               # 0.5 -> 0.25 and 0.25 -> 0.125: both ln 2
    # the first step of a search: identical rows, scores [0, -1e9]: everything comes from beam 0
    s, i, _ = R.beam_candidates(np.stack([row, row]), [0.0, -1e9], 2, 4)
    assert i.tolist() == [[0, 2, 1, 3]]
    # -inf is no candidate and has no share of the softmax; fewer than K candidates leave sentinels
    x = np.array([[NINF, ln(3.0), NINF, ln(1.0)]])
    s, i, gap = R.beam_candidates(x, [0.5], 1, 3)
    assert i.tolist() == [[1, 3, R.SENTINEL]]
    assert np.allclose(s[0, :2], [ln(0.75) + 0.5, ln(0.25) + 0.5]) and s[0, 2] == NINF
    assert np.isclose(gap[0], ln(3.0))
    # a row of -inf only contributes nothing; two clips are independent
    x = np.array([[NINF, NINF], [0.0, ln(3.0)], [ln(3.0), 0.0], [NINF, NINF]])
    s, i, _ = R.beam_candidates(x, [0.0, 0.0, 0.0, 0.0], 2, 2)
    assert i.tolist() == [[3, 2], [0, 1]]
