"""CPU: the per-row draft verification, restated (tests/draft_rows_reference.py), reproduces the plain greedy loop over a toy model,
and the inputs of tests/test_draft_rows_gpu.py tell the wrong variants of the kernels apart."""
import numpy as np
import pytest

import draft_rows_reference as ref

V, MAX_LEN = 50, 10


def toy(seed):
    """A deterministic next-token function of (row, prefix) that emits SEP now and then; every row the same rule"""
    def f(r, prefix):
        h = hash((seed,) + tuple(int(x) for x in prefix)) & 0xFFFFFF
        tok = ref.SEP if h % 4 == 0 else 4 + h % (V - 4)
        return tok, -(h % 1000) / 100.0
    return f


@pytest.mark.parametrize("stop_all_sep", [False, True])
@pytest.mark.parametrize("seed", range(8))
def test_draft_loop_equals_plain_loop(seed, stop_all_sep):
    rng = np.random.default_rng(seed)
    B = 1 + seed % 4
    f = toy(seed)
    ids, lp, cnt = ref.plain_loop(f, B, MAX_LEN, ref.CLS, ref.SEP)
    steps = ref.finish_steps(cnt, B, MAX_LEN, stop_all_sep)
    for n in (1, 4, MAX_LEN):
        draft = np.concatenate([ids[:, :1], rng.integers(-2, V + 3, size=(B, n))], axis=1)
        for r in range(B):                                  # rows keep different shares of the plain caption
            k = int(rng.integers(0, n + 1))
            draft[r, 1:k + 1] = ids[r, 1:k + 1]
        d_ids, d_lp, d_cnt, d_steps, acc, ran = ref.draft_loop(f, draft, B, MAX_LEN, ref.CLS, ref.SEP, V, stop_all_sep)
        assert d_steps == steps
        assert np.array_equal(d_ids[:, :steps + 1], ids[:, :steps + 1])
        assert np.array_equal(d_lp[:, :steps], lp[:, :steps])
        assert np.array_equal(d_cnt[:steps], cnt[:steps])
        if not stop_all_sep:
            assert np.array_equal(d_ids, ids) and np.array_equal(d_cnt, cnt)
        assert acc["host"][2] == sum(acc["a_r"]) and all(c == min(a + 1, n) for c, a in zip(acc["covered"], acc["a_r"]))


def _accept(case, variant=None):
    val, idx, ssum = (case[k].astype(np.float64) for k in ("val", "idx", "sum"))
    B, n = case["ids"].shape[0], case["ids"].shape[1] - 3
    tok = ref.tokens_of_partials(val, idx.astype(np.int64)).reshape(B, n)
    lp = ref.logprobs_of_partials(val, idx.astype(np.int64), ssum).reshape(B, n)
    lp0 = np.full((B, n + 2), np.nan)
    return ref.accept_rows(tok, case["ids"], ref.SEP, case["sep_cnt0"], lp, lp0, variant), tok


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in ("ids", "len", "sep_cnt", "lp_out", "host"))


def test_accept_cases_hold_what_they_promise():
    for B, n, V_ in ((3, 20, 100), (16, 63, 100), (16, 2, 100)):
        case = ref.accept_case(B, n, V_, "mixed", "diff", 5)
        good, tok = _accept(case)
        assert np.array_equal(tok, case["tok"]) and good["a_r"] == case["a_r"]
    x = np.random.default_rng(0).standard_normal((5, 100))
    x[:, 16:32] = -np.inf
    x[2, 40:] = -np.inf
    for k, (a, b) in enumerate(zip(ref.fast_partials(x), ref.lpref.tile_partials(x))):
        assert np.array_equal(a, b) if k < 2 else np.allclose(a, b, rtol=1e-14, atol=0)        # (the sums: another order of adds)
    assert ref.accept_case(3, 20, 30522, "mixed", "none", 1)["idx"].shape[1] == 1908
    assert (ref.accept_case(3, 20, 100, "mixed", "none", 1)["idx"][:, 1] == 0x7FFFFFFF).all()      # the all -inf tile


@pytest.mark.parametrize("variant", ["lockstep", "covered_a", "fired_max"])
def test_gpu_accept_inputs_catch_wrong_variant(variant):
    caught = 0
    for B, n, V_ in ref.ACCEPT_SHAPES:
        if V_ != 100:
            continue                                        # (the same rows at the larger vocabulary: the GPU test's tile count)
        for pattern in ref.PATTERNS:
            for sep in ("none", "same", "diff"):
                case = ref.accept_case(B, n, V_, pattern, sep, 7)
                caught += not _same(_accept(case)[0], _accept(case, variant)[0])
    assert caught > 0


@pytest.mark.parametrize("variant", ["sep_twice", "lp_zero"])
def test_gpu_keep_inputs_catch_wrong_variant(variant):
    caught = 0
    for case in ref.keep_case(16, 100, 10, 3):
        lp = ref.logprobs_of_partials(case["val"].astype(np.float64), case["idx"].astype(np.int64), case["sum"].astype(np.float64))
        args = (case["tok"], lp, case["out0"], np.full(16, -2.5), np.zeros(12, dtype=np.int64), case["step"], ref.SEP, case["len"])
        good, bad = ref.argmax_keep(*args), ref.argmax_keep(*args, variant)
        caught += not all(np.array_equal(g, b) for g, b in zip(good, bad))
    assert caught > 0


def test_tail_plan():
    assert ref.tail_plan(3, 7, False, 10, True) == (True, 3, 8)
    assert ref.tail_plan(10, 10, False, 10, False)[0] is False          # everything covered
    assert ref.tail_plan(3, 7, True, 10, True)[0] is False              # the stop rule fired inside the covered part
    assert ref.tail_plan(3, 7, True, 10, False)[0] is True              # ... which stop = never ignores
