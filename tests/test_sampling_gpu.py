"""The kernels behind gitcap_attach_sampling on the MI355X, through their stateless hooks:

  a. gitcap_sample_rows against tests/sampling_reference.py: draw_rows (fp64; the filter is the oracle's): words exactly, scores, kept
     counts and log-sum-exps within the bounds derived there.  A row whose reference margin is under its bound is left out and
     counted: at most 1 % of a case's rows (tests/test_sampling.py shows the inputs stay inside that on the reference alone);
  b. the candidate layout, two runs bit for bit, a row's result independent of the rows beside it;
  c. gitcap_dbg_beam_step_sampled driven as whole toy searches, state by state against sampling_reference.Book.
"""
import ctypes

import numpy as np
import pytest
import torch

import sampling_reference as S
from gpu_support import beam_state, lib, ptr, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = S.row_cases()


def _run(lib, x, bs, prefix, cur_len, rp, B, beams, pn, T, top_k, top_p, seed, pad=0, stats=True):
    rows, V = x.shape
    ld, K = V + pad, beams * pn
    buf = np.full((rows, ld), 1e30, np.float32)                    # row padding the kernel must not read
    buf[:, :V] = x
    d_x, d_bs = to_dev(buf, torch.float32), to_dev(bs, torch.float32)
    d_pre = to_dev(prefix, torch.int64) if prefix is not None else None
    out_s = torch.full((B * K + 4,), float("nan"), device="cuda")
    out_i = torch.full((B * K + 4,), -5, device="cuda", dtype=torch.int32)
    kept = torch.full((rows + 2,), -5, device="cuda", dtype=torch.int32) if stats else None
    logz = torch.full((rows + 2,), float("nan"), device="cuda") if stats else None
    rc = lib.gitcap_sample_rows(ptr(d_x), ld, ptr(d_bs), ptr(d_pre), 0 if prefix is None else prefix.shape[1], cur_len, ctypes.c_float(rp),
                                B, beams, V, pn, ctypes.c_float(T), top_k, ctypes.c_float(top_p), ctypes.c_uint64(seed), ptr(out_s),
                                ptr(out_i), ptr(kept), ptr(logz), stream())
    torch.cuda.synchronize()
    return rc, out_s, out_i, kept, logz


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_sample_rows_vs_restatement(lib, c):
    B, beams, pn, V = c["B"], c["beams"], c["pn"], c["x"].shape[1]
    rows, K = B * beams, beams * pn
    d = S.case_reference(c)
    rc, out_s, out_i, kept, logz = _run(lib, c["x"], c["bs"], c["prefix"], c["cur_len"], c["rp"], B, beams, pn, c["T"], c["top_k"],
                                        c["top_p"], c["seed"], c["pad"])
    assert rc == 0
    assert bool(torch.isnan(out_s[B * K:]).all()) and bool((out_i[B * K:] == -5).all()) and bool((kept[rows:] == -5).all())
    got_s, got_i = out_s[:B * K].view(B, K).cpu().numpy().astype(np.float64), out_i[:B * K].view(B, K).cpu().numpy()
    kept, logz = kept.cpu().numpy(), logz.cpu().numpy().astype(np.float64)
    left_out, worst = 0, 0.0
    for r in range(rows):
        cut_ok, keys_ok = S.decidable(d, r)
        if not (cut_ok and keys_ok):
            left_out += 1
            continue
        assert kept[r] == d["kept"][r], (r, kept[r], d["kept"][r])
        assert abs(logz[r] - d["logz"][r]) <= d["logz_bound"][r], (r, logz[r], d["logz"][r], d["logz_bound"][r])
        b, j = divmod(r, beams)
        for k in range(pn):
            p = j * pn + k
            if k >= len(d["words"][r]):                            # fewer kept columns than draws: the sentinel
                assert got_i[b, p] == 0x7FFFFFFF and got_s[b, p] == -np.inf
                continue
            assert got_i[b, p] == (p % beams) * V + d["words"][r][k], (r, k, got_i[b, p], d["words"][r])
            err = abs(got_s[b, p] - d["scores"][r][k])
            worst = max(worst, err / d["score_bound"][r][k])
            assert err <= d["score_bound"][r][k], (r, k, got_s[b, p], d["scores"][r][k], d["score_bound"][r][k])
    print("%s: rows left out %d of %d; worst score error / bound %.3f" % (c["id"], left_out, rows, worst))
    assert left_out * 100 <= rows


def test_layout_repeatability_and_independence_of_the_batch(lib):
    B, beams, pn, V = 2, 4, 2, 2049
    x = S.gaussian_rows(9, B * beams, V, 1.0)
    bs = np.linspace(-3, 0, B * beams).astype(np.float32)
    args = dict(prefix=None, cur_len=3, rp=1.0, pn=pn, T=0.7, top_k=50, top_p=1.0, seed=77)
    rc, s1, i1, k1, z1 = _run(lib, x, bs, B=B, beams=beams, **args)
    rc2, s2, i2, k2, z2 = _run(lib, x, bs, B=B, beams=beams, **args)
    assert rc == 0 and rc2 == 0
    for a, b in ((s1, s2), (z1, z2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(i1, i2) and torch.equal(k1, k2)
    d = S.draw_rows(x, bs, None, 1.0, 0.7, 50, 1.0, 77, 3, pn)
    ci, _ = S.layout(d["words"], d["scores"], B, beams, pn, V)
    assert all(all(S.decidable(d, r)) for r in range(B * beams))
    assert np.array_equal(i1[:B * beams * pn].view(B, beams * pn).cpu().numpy(), ci)
    # candidate p of a clip: draw p % pn of beam p // pn, offset (p % beams) * V -- the offsets are tiled, not beam-major
    assert (ci[0] // V).tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    # the first clip alone, and its rows as one-beam clips: the same words and filtered rows (row index = Philox row)
    rc, s3, i3, k3, z3 = _run(lib, x[:beams], bs[:beams], B=1, beams=beams, **args)
    assert rc == 0 and torch.equal(i3[:beams * pn], i1[:beams * pn]) and torch.equal(z3[:beams].view(torch.int32), z1[:beams].view(torch.int32))
    assert torch.equal(s3[:beams * pn].view(torch.int32), s1[:beams * pn].view(torch.int32))
    rc, s4, i4, k4, z4 = _run(lib, x[:beams], bs[:beams], B=beams, beams=1, **args)
    assert rc == 0 and torch.equal(i4[:beams * pn] % V, i1[:beams * pn] % V) and torch.equal(k4[:beams], k1[:beams])
    # another seed draws other words
    rc, s5, i5, _, z5 = _run(lib, x, bs, B=B, beams=beams, **dict(args, seed=78))
    assert rc == 0 and not torch.equal(i5, i1) and torch.equal(z5.view(torch.int32), z1.view(torch.int32))


def test_sample_rows_refuses_bad_arguments(lib):
    B, beams, pn, V = 1, 2, 2, 40
    x = S.gaussian_rows(1, B * beams, V, 1.0)
    bs = np.zeros(B * beams, np.float32)
    pre = np.zeros((B * beams, 4), np.int64)
    ok = dict(prefix=pre, cur_len=2, rp=1.3, B=B, beams=beams, pn=pn, T=1.0, top_k=0, top_p=1.0, seed=1, stats=False)
    assert _run(lib, x, bs, **ok)[0] == 0
    for bad in (dict(T=0.0), dict(T=float("inf")), dict(T=float("nan")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
                dict(top_p=float("nan")), dict(rp=0.0), dict(rp=float("inf")), dict(beams=17, B=1), dict(pn=9), dict(pn=0),
                dict(prefix=None), dict(cur_len=0), dict(cur_len=5)):
        rc, out_s, out_i, _, _ = _run(lib, x, bs, **dict(ok, **bad))
        assert rc == -1, bad
        assert bool(torch.isnan(out_s).all()) and bool((out_i == -5).all()), bad       # nothing was launched
    assert _run(lib, x[:, :1], bs, **dict(ok, rp=1.0))[0] == -1                          # per_node > V
    assert _run(lib, np.zeros((2, 32769), np.float32), bs, **dict(ok, rp=1.0))[0] == -1  # a row wider than the kernel holds
    assert _run(lib, x, bs, **dict(ok, prefix=None, rp=1.0))[0] == 0                     # rp 1: the prefix is not read


# ---- c. the bookkeeping for unsorted candidates ---------------------------------------------------------------------------------

def _forced(beams, mode):
    """EOS drawn by one row, by all rows but one, and by every live row of a clip (tests/test_sampling.py: _forced)."""
    E = S.TOY_EOS
    if mode == "none":
        return {}
    f = {(1, r): [E, E] for r in range(beams)}                                  # clip 0: every row -> kept == 0
    f.update({(1, 2 * beams + r): [E, E] for r in range(beams - 1)})            # clip 2: all but one draw -> one live beam
    f[(1, 3 * beams - 1)] = [E, 5]
    f[(2, beams)] = [E, E]                                                      # clip 1, step 2: one row
    return f


@pytest.mark.parametrize("lp", [0.0, 0.6])
@pytest.mark.parametrize("n,beams,mode", [(1, 2, "none"), (1, 4, "forced"), (3, 2, "forced"), (3, 4, "forced"), (3, 4, "none")])
def test_sampled_bookkeeping_vs_restatement(lib, n, beams, mode, lp):
    """Whole toy searches to the last step.  The candidates come from the restated draw (fp32-rounded scores, unsorted, the maximum
    rarely in slot 0) and go to both sides: integers exactly, beam scores bit for bit, hypothesis scores within 4 ulp (one powf and
    one divide on the device; exactly for length_penalty 0)."""
    B, V, L, pn = S.TOY_B, S.TOY_V, S.TOY_L, 2
    K = beams * pn
    table, forced = S.toy_table(), _forced(beams, mode)
    book = S.Book(B, beams, n, L, S.TOY_CLS, S.TOY_EOS, lp)
    t, bb1, bbn = beam_state(B, beams, n, L)
    assert lib.gitcap_dbg_beam_init(ctypes.byref(bb1), B, beams, L, S.TOY_CLS, stream()) == 0
    t["hyp_len"].zero_()
    ids, cur, max_not_first = [t["ids0"], t["ids1"]], 0, 0
    for cur_len in range(1, L):
        ci, cs = S.toy_candidates(table, book, beams, pn, 1.0, 1.0, 0, 1.0, 31337, cur_len, forced)
        cs32 = cs.astype(np.float32)
        max_not_first += int((cs32.argmax(axis=1) != 0).sum())
        d_cs, d_ci = to_dev(cs32, torch.float32), to_dev(ci, torch.int32)
        assert lib.gitcap_dbg_beam_step_sampled(ctypes.byref(bbn), ptr(d_cs), ptr(d_ci), B, beams, K, V, cur_len, L, S.TOY_EOS,
                                                ctypes.c_float(lp), cur, stream()) == 0
        torch.cuda.synchronize()
        book.step(cs32, ci, V, cur_len)
        cur ^= 1
        assert t["words"].tolist() == book.words and t["src_rows"].tolist() == book.src_rows, cur_len
        assert t["done"].tolist() == [int(x) for x in book.done], cur_len
        assert ids[cur][:, :cur_len + 1].tolist() == book.ids, cur_len
        assert np.array_equal(t["beam_scores"].cpu().numpy().view(np.uint32), np.array(book.beam_scores, np.float32).view(np.uint32))
        for b in range(B):
            h = book.hyps[b]
            assert t["hyp_len"][b].tolist() == [len(x[1]) for x in h] + [0] * (n - len(h)), (cur_len, b)
            for i, (s, seq) in enumerate(h):
                assert t["hyp_ids"][b, i, :len(seq)].tolist() == seq
                got = float(t["hyp_score"][b, i])
                assert got == float(s) if lp == 0.0 else abs(got - float(s)) <= 4 * S.EPS * abs(float(s)), (cur_len, b, i, got, s)
    assert max_not_first >= 1
    dec = torch.full((B, n, L), -777, device="cuda", dtype=torch.int64)
    lps = torch.full((B, n), float("nan"), device="cuda")
    assert lib.gitcap_dbg_beam_finish_nbest(ctypes.byref(bbn), B, L, S.TOY_EOS, ptr(dec), ptr(lps), stream()) == 0
    torch.cuda.synchronize()
    rdec, rlps = book.finish()
    assert np.array_equal(dec.cpu().numpy(), rdec)
    assert np.allclose(lps.cpu().numpy(), rlps, rtol=4 * S.EPS, atol=0)


def test_sampled_step_refuses_bad_arguments(lib):
    from gitcap._lib import CDbgBeamBuffersNbest
    B, beams, L, K, V = 2, 2, 5, 4, 23
    t, _, bbn = beam_state(B, beams, 3, L)
    before = {k: v.clone() for k, v in t.items()}
    cs = torch.zeros(B, K, device="cuda")
    ci = torch.zeros(B, K, device="cuda", dtype=torch.int32)
    step = lambda bb, cur_len=1, cur=0, beams=beams, K=K: lib.gitcap_dbg_beam_step_sampled(
        ctypes.byref(bb), ptr(cs), ptr(ci), B, beams, K, V, cur_len, L, 22, ctypes.c_float(0.6), cur, stream())
    for bad_n in (0, 17):
        bad = CDbgBeamBuffersNbest(*[getattr(bbn, f) for f, _ in CDbgBeamBuffersNbest._fields_[:-1]], bad_n)
        assert step(bad) == -1
    assert step(bbn, cur_len=0) == -1 and step(bbn, cur_len=L) == -1 and step(bbn, cur=2) == -1
    assert step(bbn, beams=17) == -1 and step(bbn, K=17) == -1
    torch.cuda.synchronize()
    for k in t:
        a, b = t[k], before[k]
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
