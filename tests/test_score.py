"""The fp64 restatement of caption scoring (tests/score_reference.py) against torch.log_softmax + gather on the CPU, the proof
that the test inputs tell subtly wrong kernels from the right one, and the presence of the new C ABI symbols."""
import os
import re

import numpy as np
import pytest
import torch

import score_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")
V, T, IGN, SEP = 77, 7, 40, 5            # 77 columns: five tiles, a ragged last one of 13


def _inputs():
    """Three rows of logits [T][V] with -inf columns and ids that put targets on column 0, V - 1, the tile edge 15 | 16, inside the
    ragged tile, on the arg-max, on a -inf column, outside the vocabulary and on ignore_id; lengths 7 (all), 4 and 1 (nothing)."""
    rng = np.random.default_rng(11)
    lg = (3.0 * rng.standard_normal((3, T, V))).astype(np.float32).astype(np.float64)
    lg[:, :, 33] = NINF
    lg[1, 2, 64:] = NINF                                      # an empty ragged tile
    lg[:, :, 70] += 6.0                                       # weight in the ragged tile: dropping it must show
    y = np.array([[101, 0, V - 1, 15, 16, 70, 33],
                  [101, int(np.argmax(lg[1, 0])), IGN, 66, SEP, 76, 3],
                  [101, 9, -1, V, V + 3, IGN, 12]], dtype=np.int64)
    return lg, y, np.array([T, 4, 1], dtype=np.int64)


def _torch_reference(lg, y, lengths, ignore_id):
    R, T_, V_ = lg.shape
    lsm = torch.log_softmax(torch.as_tensor(lg), dim=2).numpy()
    ok = S.counted(y, lengths, ignore_id, V_)
    lp = np.zeros((R, T_ - 1))
    for r in range(R):
        for j in range(T_ - 1):
            if ok[r, j]:
                lp[r, j] = lsm[r, j, y[r, j + 1]]
    return lp, np.array([lp[r][ok[r]].sum() for r in range(R)]), ok.sum(1), lsm[:, :-1].argmax(2), lsm[:, :-1].max(2)


@pytest.mark.parametrize("use_lengths", [False, True])
def test_restatement_is_log_softmax_gather(use_lengths):
    lg, y, lengths = _inputs()
    ln = lengths if use_lengths else None
    got = S.score_logits(lg, y, ln, IGN)
    lp, tot, cnt, t1, t1lp = _torch_reference(lg, y, ln, IGN)
    fin = np.isfinite(lp)
    assert np.array_equal(np.isneginf(got["token_lp"]), np.isneginf(lp)) and not np.isnan(got["token_lp"]).any()
    assert np.abs(got["token_lp"][fin] - lp[fin]).max() <= 1e-11
    assert got["count"].tolist() == cnt.tolist()
    assert got["top1_ids"].tolist() == t1.tolist() and np.abs(got["top1_lp"] - t1lp).max() <= 1e-11
    for r in range(3):
        assert got["sum"][r] == tot[r] or abs(got["sum"][r] - tot[r]) <= 1e-10
    assert got["token_lp"][0, 5] == NINF and got["sum"][0] == NINF          # the -inf target column
    if use_lengths:
        assert cnt.tolist() == [6, 2, 0] and got["sum"][2] == 0.0
    else:
        assert cnt.tolist() == [6, 5, 2]


def test_all_minus_inf_row_gives_minus_inf_never_nan():
    lg = np.full((1, 3, V), NINF)
    got = S.score_logits(lg, np.array([[101, 4, 5]]), None, -1)
    assert got["token_lp"].tolist() == [[NINF, NINF]] and got["sum"][0] == NINF and got["top1_lp"].tolist() == [[NINF, NINF]]
    assert got["top1_ids"].tolist() == [[0, 0]] and got["count"].tolist() == [2]


@pytest.mark.parametrize("wrong", ["target_shift", "drop_tail", "length_off", "ignore_counted", "sum_all"])
def test_inputs_catch_wrong_kernels(wrong):
    """Each deliberately wrong variant misses the bound the GPU tests hold the device to, on these very inputs."""
    lg, y, lengths = _inputs()
    lp, tot, cnt, _, _ = _torch_reference(lg, y, lengths, IGN)
    bad = S.score_logits(lg, y, lengths, IGN, wrong=wrong)

    def miss(a, b, bound):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        both = np.isfinite(a) & np.isfinite(b)
        d = np.abs(np.where(both, a, 0.0) - np.where(both, b, 0.0))
        return bool((np.isfinite(a) != np.isfinite(b)).any() or np.isnan(a).any() or (d > np.broadcast_to(bound, a.shape))[both].any())
    misses = (miss(bad["token_lp"], lp, S.bound_lp(lp)) or bad["count"].tolist() != cnt.tolist() or
              miss(bad["sum"], tot, np.array([S.bound_sum(lp[r]) for r in range(3)])))
    assert misses, wrong
    good = S.score_logits(lg, y, lengths, IGN)
    assert not miss(good["token_lp"], lp, S.bound_lp(lp)) and good["count"].tolist() == cnt.tolist()


def test_bounds_are_the_documented_ones():
    assert S.bound_lp(0.0) == 2e-5 and abs(S.bound_lp(-8.0) - (2e-5 + 8 * 2.0 ** -23)) < 1e-18 and S.bound_lp(NINF) == 2e-5
    assert abs(S.bound_sum([-1.0, -3.0]) - (4e-5 + 4 * 2.0 ** -23 + 2 * 2.0 ** -24 * 4.0)) < 1e-15


NEW_SYMBOLS = ["gitcap_score", "gitcap_student_score", "gitcap_dbg_vocab_head_score", "gitcap_dbg_score_final",
               "gitcap_dbg_score_target_logits", "gitcap_student_dbg_score_target_logits"]


def test_new_symbols_are_declared():
    from gitcap import _lib
    header = open(os.path.join(ROOT, "include", "gitcap.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\bint " + name + r"\(", header), name
    src = open(os.path.join(ROOT, "real-time-video-captioning_amd", "csrc", "gitcap.hip")).read()
    assert re.search(r"#define GITCAP_ABI_VERSION\s+1\b", src)              # only additions


def test_caption_confidence_accepts_the_score_dict():
    from gitcap.confidence import caption_confidence
    d = dict(sum=torch.tensor([-2.0, 0.0, -1.0]), count=torch.tensor([4, 0, 1], dtype=torch.int32))
    got = caption_confidence(d)
    assert torch.allclose(got, torch.tensor([np.exp(-0.5), 1.0, np.exp(-1.0)], dtype=torch.float32))
    with pytest.raises(ValueError):
        caption_confidence(torch.zeros(1, 2, dtype=torch.int64))


def test_rerank_scores_and_lengths_helpers():
    from gitcap import scoring
    d = scoring.rerank_scores(dict(sum=torch.tensor([[-4.0, -1.0, -2.0, 0.0]]), count=torch.tensor([[4, 1, 1, 0]], dtype=torch.int32)), 0.6)
    want = torch.tensor([[-4.0 / 4 ** 0.6, -1.0, -2.0, NINF]])
    assert torch.allclose(d["scores"], want) and d["order"].tolist() == [[1, 0, 2, 3]]
    ids = torch.tensor([[[101, 7, SEP, 9, SEP], [101, 7, 8, 9, 10]]])
    assert scoring.row_lengths(ids, SEP, True, None).tolist() == [[3, 5]]
    assert scoring.row_lengths(ids, SEP, True, torch.tensor([2])).tolist() == [[2, 2]]
    assert scoring.row_lengths(ids, SEP, False, None) is None
