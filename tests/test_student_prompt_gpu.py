"""The two kernels behind the student's prompted loops, through their debug hooks, exact against the numpy restatements of
tests/student_prompt_reference.py: student_prompt_stage_kernel (the clamp, both indexing modes, the zeroed log-probability columns,
nothing written around its rows) and student_beam_step_kernel, plain and forced.  (The forced arg-max of the greedy loop is the
teacher's: gitcap_dbg_argmax_final_forced, tests/test_prompt_gpu.py.)"""
import numpy as np
import pytest
import torch

import student_prompt_reference as P
from gpu_support import assert_tail, lib, poisoned, ptr, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

IDS_FILL, LP_FILL = -3, float("nan")


@pytest.mark.parametrize("k,pmin", [(1, 1), (1, 4), (3, 1)])
def test_stage_kernel(lib, k, pmin):
    """Lengths 1, 4, 11, 0 and 99 at ld = 12, max_len 11: rows as restated, the table's column behind max_len never copied, the lp
    columns 0 .. pmin - 2 zeroed and no other, the elements in front of and behind both outputs untouched."""
    prm, lens, max_len, cls = P.stage_inputs()
    rows, ld, ld_lp, pad = 5 * k, 12, 11, 16
    ids_buf = poisoned(pad + rows * ld + pad, IDS_FILL, torch.int64)
    lp_buf = poisoned(pad + rows * ld_lp + pad, LP_FILL)
    ids, lp = ids_buf[pad:pad + rows * ld], lp_buf[pad:pad + rows * ld_lp]
    rc = lib.gitcap_dbg_student_prompt_stage(ptr(to_dev(prm, torch.int64)), 12, ptr(to_dev(lens, torch.int32)), rows, k, max_len, cls, ptr(ids), ld,
                                             ptr(lp), ld_lp, pmin, stream())
    assert rc == 0
    torch.cuda.synchronize()
    want_ids, want_lp = P.stage(prm, lens, rows, k, max_len, cls, np.full((rows, ld), IDS_FILL, np.int64),
                                np.full((rows, ld_lp), np.nan, np.float32), pmin)
    got_ids, got_lp = ids.cpu().numpy().reshape(rows, ld), lp.cpu().numpy().reshape(rows, ld_lp)
    assert np.array_equal(got_ids, want_ids)
    assert not (got_ids == 7777).any()
    assert np.array_equal(np.isnan(got_lp), np.isnan(want_lp)) and (got_lp[:, :pmin - 1] == 0.0).all()
    assert bool((ids_buf[:pad] == IDS_FILL).all()) and bool((ids_buf[pad + rows * ld:] == IDS_FILL).all())
    assert bool(torch.isnan(lp_buf[:pad]).all()) and bool(torch.isnan(lp_buf[pad + rows * ld_lp:]).all())
    # without lp the ids are the same and nothing else is touched
    ids2 = poisoned(rows * ld + pad, IDS_FILL, torch.int64)
    assert lib.gitcap_dbg_student_prompt_stage(ptr(to_dev(prm, torch.int64)), 12, ptr(to_dev(lens, torch.int32)), rows, k, max_len, cls, ptr(ids2), ld,
                                               None, 0, pmin, stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ids2[:rows * ld].cpu().numpy().reshape(rows, ld), want_ids)
    assert_tail(ids2, rows * ld, IDS_FILL)


def test_stage_kernel_refuses_what_could_leave_a_row(lib):
    prm, lens, max_len, cls = P.stage_inputs()
    p, n = to_dev(prm, torch.int64), to_dev(lens, torch.int32)
    ids = poisoned(5 * 12, IDS_FILL, torch.int64)
    lp = poisoned(5 * 11, LP_FILL)
    ok = (ptr(p), 12, ptr(n), 5, 1, 11, cls, ptr(ids), 12, ptr(lp), 11, 4, stream())
    for i, v in [(1, 10), (8, 10), (5, 0), (5, 13), (3, 0), (4, 0), (11, 0), (11, 13), (0, None), (2, None), (7, None)]:
        bad = list(ok)
        bad[i] = v
        assert lib.gitcap_dbg_student_prompt_stage(*bad) != 0, (i, v)
    torch.cuda.synchronize()
    assert bool((ids == IDS_FILL).all()) and bool(torch.isnan(lp).all())


def _beam_step(lib, d, prompt):
    n, ld = d["B"] * d["k"], d["ld"]
    nxt = poisoned(n * ld + 8, IDS_FILL, torch.int64)
    scores = torch.arange(n, dtype=torch.float32, device="cuda")
    src = poisoned(n + 8, -3, torch.int32)
    cs, ci = to_dev(d["cand_scores"], torch.float32), to_dev(d["cand_idx"], torch.int32)
    cs0, ci0 = cs.clone(), ci.clone()
    pi, pl = (to_dev(d["prompt_ids"], torch.int64), to_dev(d["lengths"], torch.int32)) if prompt else (None, None)
    rc = lib.gitcap_dbg_student_beam_step(ptr(cs), ptr(ci), ptr(to_dev(d["ids_cur"], torch.int64)), ptr(nxt), ptr(scores), ptr(src),
                                          d["B"], d["k"], d["V"], d["t"], ld, ptr(pi), ld, ptr(pl), d["prompt_max_len"] if prompt else 0, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(cs, cs0) and torch.equal(ci, ci0)            # the candidates' rows are inputs
    assert_tail(nxt, n * ld, IDS_FILL)
    assert_tail(src, n, -3)
    return nxt[:n * ld].cpu().numpy().reshape(n, ld), scores.cpu().numpy(), src[:n].cpu().numpy()


@pytest.mark.parametrize("prompt", [False, True])
def test_beam_step_kernel(lib, prompt):
    """B = 2, k = 3, V = 40, t = 2.  Plain: bit for bit the restatement of the kernel as it was.  Forced: clip 0 (length 5) keeps
    every row's own prefix, appends its prompt's token, src_rows 0 1 2, scores untouched; clip 1 (length 2) is the plain step."""
    d = P.beam_step_inputs()
    n = d["B"] * d["k"]
    pr = (d["prompt_ids"], d["lengths"], d["prompt_max_len"]) if prompt else None
    want = P.beam_step(d["cand_scores"], d["cand_idx"], d["ids_cur"], np.full((n, d["ld"]), IDS_FILL, np.int64), np.arange(n, dtype=np.float32),
                       np.full(n, -3, np.int32), d["B"], d["k"], d["V"], d["t"], pr)
    got = _beam_step(lib, d, prompt)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (g, w)
    assert (got[0][:, d["t"] + 2:] == IDS_FILL).all()               # columns behind t + 1 are not written
    if prompt:
        assert got[2][:3].tolist() == [0, 1, 2] and got[1][:3].tolist() == [0.0, 1.0, 2.0]
        assert (got[0][:3, d["t"] + 1] == d["prompt_ids"][0, d["t"] + 1]).all()
        wrong = P.beam_step(d["cand_scores"], d["cand_idx"], d["ids_cur"], np.full((n, d["ld"]), IDS_FILL, np.int64), np.arange(n, dtype=np.float32),
                            np.full(n, -3, np.int32), d["B"], d["k"], d["V"], d["t"], pr, wrong="permute")
        assert not np.array_equal(got[0], wrong[0]) and not np.array_equal(got[2], wrong[2])


def test_beam_step_behind_the_longest_prompt_is_the_plain_launch(lib):
    d = P.beam_step_inputs()
    plain = _beam_step(lib, d, False)
    d2 = dict(d, prompt_max_len=3)                                  # t + 1 = 3 is not below it: no clip is forced, whatever the lengths say
    for g, w in zip(_beam_step(lib, d2, True), plain):
        assert np.array_equal(g, w)
