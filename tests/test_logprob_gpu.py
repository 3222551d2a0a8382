"""The token log-probability arithmetic on the MI355X, kernel by kernel through the gitcap_dbg_*_lse / _lp hooks, against the fp64
restatement of tests/logprob_reference.py:

  a. the vocabulary head's third partial (skinny.hip: logits_epilogue), reference = the restatement applied to the DEVICE's own
     fp32 logits, so that only the new arithmetic is measured; amax_val / amax_idx bit for bit those of the hook without it;
  b. bitwise invariants of the third partial: the form of the head kernel, the number of rows in the launch;
  c. argmax_final's merge on hand-made partials; tokens and embedded rows bit for bit those of the hook without it;
  d. draft_accept's covered positions; everything else identical to the hook without it.

Tolerance |lp_device - lp_fp64| <= 2e-5 nats, absolute, derived and not measured: every term is exp(x), x <= 0; the fp32
subtraction and the log2(e) scaling perturb a term by about 2 * 2^-24 * |x| relative, and weighted by the softmax
sum_i p_i |x_i| <= ln V ~ 10.3, i.e. about 1.3e-6 on the sum; the ~24-deep fixed summation tree adds about 1.4e-6, the merge's
rescale about the same again, v_exp_f32 / v_log_f32 a few 1e-7: about 5e-6 in all, times 4.  A relative error d of a sum is an
absolute error d of its log, so the same number bounds the relative error of a single tile's sum (16 terms: far less is used)."""
import ctypes

import numpy as np
import pytest
import torch

import logprob_reference as L
import selection_reference as R
from selection_reference import DRAFT_NT, DRAFT_SEP, draft_scenario, draft_scenarios
from gpu_support import lib, ptr, run_vocab_head, softmax_head_inputs, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 2e-5
NINF = float("-inf")


# ---- a. / b. the head's third partial ---------------------------------------------------------------------------------------

def _argmax_final_lp(lib, val, idx, ssum, rows, nt):
    out = torch.full((rows,), -9, device="cuda", dtype=torch.int64)
    lp = torch.full((rows,), float("nan"), device="cuda")
    rc = lib.gitcap_dbg_argmax_final_lp(ptr(val), ptr(idx), nt, rows, 1, 0, ptr(out), 1, None, 0, -1, None, ptr(ssum), ptr(lp), 1, stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy(), lp.cpu().numpy().astype(np.float64)


def _head_case(lib, M, N, K, fp8=False, ninf=False):
    nt = (N + 15) // 16
    X, W, wscale, bias = softmax_head_inputs(M, N, K, fp8, seed=7000 + 100 * M + N + K, ninf=ninf)
    logits, val, idx, ssum = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, hook="lse")[:4]
    lg0, val0, idx0, _ = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K)[:4]
    assert torch.equal(logits, lg0) and torch.equal(val, val0) and torch.equal(idx, idx0)        # y, best, bi untouched
    lg = logits.cpu().numpy()
    assert not np.isnan(lg).any()
    rv, ri, rs = L.tile_partials(lg)
    assert np.array_equal(val.cpu().numpy().astype(np.float64), rv) and np.array_equal(idx.cpu().numpy().astype(np.int64), ri)
    ds = ssum.cpu().numpy().astype(np.float64)
    empty = rv == NINF
    assert (ds[empty] == 0.0).all() and not np.isnan(ds).any()                  # the 0-sum rule, never -inf - -inf
    rel = np.abs(ds[~empty] - rs[~empty]) / rs[~empty]
    print(f"head M={M} N={N} K={K} fp8={fp8} ninf={ninf}: max relative error of a tile sum {rel.max():.3e}, empty tiles {int(empty.sum())}")
    assert rel.max() <= TOL
    # through the merge on the device: the chosen token's log-probability against fp64 on the same logits
    tok, lp = _argmax_final_lp(lib, val.contiguous(), idx.contiguous(), ssum.contiguous(), M, nt)
    want_tok, want_lp = L.token_logprobs(lg)
    err = np.abs(lp - want_lp)
    print(f"     log-probabilities {want_lp.min():.4f} .. {want_lp.max():.4f}, max |device - fp64| {err.max():.3e}")
    assert tok.tolist() == want_tok.tolist() == [int(np.argmax(lg[m])) for m in range(M)]
    assert err.max() <= TOL
    ref = torch.log_softmax(torch.as_tensor(lg).double(), 1).numpy()[np.arange(M), want_tok]
    assert np.abs(want_lp - ref).max() <= 1e-11                                  # the restatement is the log-softmax
    if ninf:
        assert empty.any() and empty[:, 1].all()
    return ssum


@pytest.mark.parametrize("M,N,K", [(1, 10, 64), (2, 48, 576), (16, 64, 768), (17, 65, 64), (33, 65, 576), (33, 4122, 768),
                                   (1, 4122, 576), (2, 64, 64), (17, 48, 768)])
def test_head_sum_partials(lib, M, N, K):
    """N = 10: fewer than 16 columns; 48: never the shared form; 64: the smallest shared launch; 65: a last tile with one valid
    column; 4122: 258 tiles -- a last workgroup with two of four waves active, a final-reduce stride with a remainder, a ragged
    last tile of 10 columns.  K = 576: 4.5 pieces per thread.  M = 1 .. 33: one, two and three m-tiles."""
    _head_case(lib, M, N, K)


def test_head_sum_partials_e4m3_weights(lib):
    _head_case(lib, 17, 4122, 768, fp8=True)


@pytest.mark.parametrize("M,N,K", [(2, 65, 64), (33, 4122, 768)])
def test_head_sum_partials_masked_columns(lib, M, N, K):
    """A bias of -inf on a whole tile (its sum is 0 and it is skipped by the merge) and on scattered columns."""
    _head_case(lib, M, N, K, ninf=True)


@pytest.mark.parametrize("N,K", [(65, 576), (4122, 768)])
def test_head_sum_partials_bitwise_invariants(lib, N, K):
    """The third partial does not depend on the form of the head kernel (gitcap_dbg_config(10, .)) nor on the rows beside it."""
    M = 33
    X, W, wscale, bias = softmax_head_inputs(M, N, K, False, seed=N + K)
    a = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, share=1, hook="lse")[:4]
    b = run_vocab_head(lib, X, K, W, wscale, bias, M, N, K, share=0, hook="lse")[:4]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for m in (0, 15, 16, 32):
        for share in (1, 0):
            one = run_vocab_head(lib, X[m:m + 1].contiguous(), K, W, wscale, bias, 1, N, K, share=share, hook="lse")[:4]
            for u, v in zip(a, one):
                assert torch.equal(u[m:m + 1], v), (m, share)


def test_lse_hooks_reject_bad_arguments(lib):
    x = torch.zeros(16, 64, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(64, device="cuda")
    i = torch.zeros(64, device="cuda", dtype=torch.int32)
    o = torch.zeros(4, device="cuda", dtype=torch.int64)
    assert lib.gitcap_dbg_vocab_head_lse(ptr(x), 64, ptr(x), None, None, 1, 16, 64, ptr(f), ptr(f), ptr(i), None, None) == -1    # no sum buffer
    assert lib.gitcap_dbg_vocab_head_lse(ptr(x), 64, ptr(x), None, None, 1, 16, 64, ptr(f), None, None, ptr(f), None) == -1     # sum without the pair
    assert lib.gitcap_dbg_argmax_final_lp(ptr(f), ptr(i), 1, 1, 1, 0, ptr(o), 1, None, 0, -1, None, None, ptr(f), 1, None) == -1
    assert lib.gitcap_dbg_argmax_final_lp(ptr(f), ptr(i), 1, 1, 1, 0, ptr(o), 1, None, 0, -1, None, ptr(f), None, 1, None) == -1
    assert lib.gitcap_dbg_argmax_final_lp(ptr(f), ptr(i), 1, 1, 1, 0, ptr(o), 1, None, 0, -1, None, ptr(f), ptr(f), 0, None) == -1


# ---- c. the final merge -----------------------------------------------------------------------------------------------------

SEP = 5


def _merge_rows(nt, rng):
    """Hand-made rows of partials (val, idx, sum): idx[t] = 16 t + 5; sums as a 16-column tile leaves them, in [1, 16)."""
    base = np.arange(nt, dtype=np.int64) * 16 + 5

    def fresh(spread=1.0):
        v = (rng.permutation(nt).astype(np.float32) / nt - 2.0) * np.float32(spread)      # distinct values
        return v, base.copy(), (1.0 + 15.0 * rng.random(nt)).astype(np.float32)
    rows = [fresh(), fresh(8.0)]
    v, i, s = fresh(); v[nt - 1] = 0.5; rows.append((v, i, s))                  # the winner in the last tile
    v, i, s = fresh(); v[0] = 50.0; s[0] = 1.0; rows.append((v, i, s))          # peaked: p = 1 up to e^-51
    v, i, s = fresh()                                                           # -inf tiles, scattered and a run; the winner survives
    dead = np.unique(np.concatenate([np.arange(1, nt, 3), np.arange(nt // 2, min(nt, nt // 2 + 70))]))
    dead = dead[dead != int(np.argmax(v))] if nt > 1 else dead[:0]
    v[dead], i[dead], s[dead] = NINF, L.SENTINEL, 0.0
    rows.append((v, i, s))
    v, i, s = fresh(); v[:] = 1.0; rows.append((v, i, s))                       # all tiles tie: the first index
    rows.append((np.full(nt, NINF, np.float32), np.full(nt, L.SENTINEL, np.int64), np.zeros(nt, np.float32)))   # empty: token 0, lp -inf
    return rows


def _merge_case(lib, nt, D=0):
    rng = np.random.default_rng(31 * nt + D)
    rows = _merge_rows(nt, rng)
    n = len(rows)
    stride, off, ld_out, ld_lp, step = 2, 1, 3, 2, 2
    val = np.full((n * stride, nt), 9.0, np.float32)            # rows the launch must not read
    idx = np.full((n * stride, nt), 7, np.int64)
    ssum = np.full((n * stride, nt), 1e30, np.float32)
    for r, (v, i, s) in enumerate(rows):
        val[r * stride + off], idx[r * stride + off], ssum[r * stride + off] = v, i, s
    want = [L.merge(v, i, s) for v, i, s in rows]
    assert [t for t, _ in want] == [R.argmax_partials(v, i) for v, i, _ in rows]
    assert want[2][0] == 16 * (nt - 1) + 5 and want[-1] == (0, NINF)
    d_val, d_idx, d_sum = to_dev(val, torch.float32), to_dev(idx, torch.int32), to_dev(ssum, torch.float32)
    emb = None
    from gitcap._lib import CDbgNextEmbed

    def launch(with_lp):
        out = torch.full((n, ld_out), -7, device="cuda", dtype=torch.int64)
        lp = torch.full((n, ld_lp), float("nan"), device="cuda")
        sep_cnt = to_dev([100, 200, 300, 400], torch.int32)
        xf = xb = e = None
        if D:
            g = torch.Generator(device="cuda").manual_seed(D)
            vocab, position = 16 * nt, 3
            word = torch.randn(vocab, D, device="cuda", generator=g)
            pos = torch.randn(position + 2, D, device="cuda", generator=g)
            gamma, beta = torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)
            xf = torch.full((n + 1, D), float("nan"), device="cuda")
            xb = torch.full((n + 1, D), float("nan"), device="cuda", dtype=torch.bfloat16)
            e = CDbgNextEmbed(word.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, D, vocab, position,
                              xf.data_ptr(), xb.data_ptr())
        ep = ctypes.byref(e) if e else None
        if with_lp:
            rc = lib.gitcap_dbg_argmax_final_lp(ptr(d_val), ptr(d_idx), nt, n, stride, off, ptr(out), ld_out, ptr(sep_cnt), step, SEP, ep,
                                                ptr(d_sum), ptr(lp), ld_lp, stream())
        else:
            rc = lib.gitcap_dbg_argmax_final(ptr(d_val), ptr(d_idx), nt, n, stride, off, ptr(out), ld_out, ptr(sep_cnt), step, SEP, ep, stream())
        torch.cuda.synchronize()
        assert rc == 0
        return out, lp, sep_cnt, xf, xb
    out, lp, sep_cnt, xf, xb = launch(True)
    out0, lp0, sep0, xf0, xb0 = launch(False)
    assert torch.equal(out, out0) and torch.equal(sep_cnt, sep0) and bool(torch.isnan(lp0).all())
    if D:
        assert torch.equal(xf[:n], xf0[:n]) and torch.equal(xb[:n], xb0[:n]) and not bool(torch.isnan(xf[:n]).any())
        assert bool(torch.isnan(xf[n]).all())
    got = out.cpu().numpy()
    assert got[:, 0].tolist() == [t for t, _ in want] and bool((got[:, 1:] == -7).all())
    glp = lp.cpu().numpy().astype(np.float64)
    assert np.isnan(glp[:, 1:]).all()
    wlp = np.array([l for _, l in want])
    assert glp[-1, 0] == NINF
    err = np.abs(glp[:-1, 0] - wlp[:-1])
    print(f"merge nt={nt} D={D}: lp {wlp[:-1].min():.4f} .. {wlp[:-1].max():.4f}, max |device - fp64| {err.max():.3e}")
    assert err.max() <= TOL
    assert -TOL <= glp[3, 0] <= 0.0                              # the peaked row (the device may return exactly 0)


@pytest.mark.parametrize("nt", [1, 5, 256, 258, 1908])
def test_argmax_final_lp_hand_made_partials(lib, nt):
    """One tile; a few; exactly one per thread; a remainder of two; the 30522-word vocabulary.  -inf tiles, the empty row, the
    winner in the last tile, row_stride / row_off / ld_out / ld_lp that are not the identity, poison around every output."""
    _merge_case(lib, nt)


@pytest.mark.parametrize("nt,D", [(5, 64), (258, 576), (1908, 768)])
def test_argmax_final_lp_with_next_embed(lib, nt, D):
    _merge_case(lib, nt, D)


def test_argmax_final_lp_is_independent_of_the_rows_beside_it(lib):
    """The fixed summation order: row r of a 7-row launch == the same partials launched alone, bit for bit."""
    nt = 1908
    rows = _merge_rows(nt, np.random.default_rng(5))
    n = len(rows)
    val = to_dev(np.stack([v for v, _, _ in rows]), torch.float32)
    idx = to_dev(np.stack([i for _, i, _ in rows]), torch.int32)
    ssum = to_dev(np.stack([s for _, _, s in rows]), torch.float32)
    tok, lp = _argmax_final_lp(lib, val, idx, ssum, n, nt)
    for r in range(n):
        t1, l1 = _argmax_final_lp(lib, val[r:r + 1].contiguous(), idx[r:r + 1].contiguous(), ssum[r:r + 1].contiguous(), 1, nt)
        assert t1[0] == tok[r] and l1.view(np.int64)[0] == lp.view(np.int64)[r]


# ---- d. draft_accept --------------------------------------------------------------------------------------------------------

LP_POISON = -12345.0


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("B", [1, 3])
def test_draft_accept_lp_vs_restatement(lib, B, n):
    rng = np.random.default_rng(100 * B + n)
    tok_scratch = torch.full((B * n,), -3, device="cuda", dtype=torch.int32)
    ticket = torch.zeros(1, device="cuda", dtype=torch.int32)
    ld_lp = n + 3
    for a_rows, sep_at in draft_scenarios(B, n):          # every launch on the same ticket word
        tok, ids, val, idx = draft_scenario(B, n, a_rows, sep_at, rng)
        ssum = (1.0 + 15.0 * rng.random(val.shape)).astype(np.float32)
        want = R.draft_accept(tok, ids, DRAFT_SEP)
        ld = ids.shape[1]
        d_val, d_idx, d_sum = to_dev(val, torch.float32), to_dev(idx, torch.int32), to_dev(ssum, torch.float32)
        res = []
        for with_lp in (True, False):
            d_ids = to_dev(ids, torch.int64)
            sep_cnt = torch.full((n + 2,), 77, device="cuda", dtype=torch.int32)
            lp = torch.full((B, ld_lp), LP_POISON, device="cuda")
            host = (ctypes.c_int32 * 2)(-5, -5)
            if with_lp:
                rc = lib.gitcap_dbg_draft_accept_lp(ptr(d_val), ptr(d_idx), DRAFT_NT, B, n, ptr(d_ids), ld, ptr(tok_scratch), ptr(ticket),
                                                    ptr(sep_cnt), DRAFT_SEP, host, ptr(d_sum), ptr(lp), ld_lp, stream())
            else:
                rc = lib.gitcap_dbg_draft_accept(ptr(d_val), ptr(d_idx), DRAFT_NT, B, n, ptr(d_ids), ld, ptr(tok_scratch), ptr(ticket),
                                                 ptr(sep_cnt), DRAFT_SEP, host, stream())
            torch.cuda.synchronize()
            assert rc == 0 and int(ticket.item()) == 0
            res.append((d_ids.cpu(), sep_cnt.cpu(), (host[0], host[1]), lp.cpu().numpy().astype(np.float64)))
        (ids1, sep1, host1, lp1), (ids0, sep0, host0, lp0) = res
        assert torch.equal(ids1, ids0) and torch.equal(sep1, sep0) and host1 == host0 == tuple(want["host"])
        assert np.array_equal(ids1.numpy(), want["ids"])
        assert (lp0 == LP_POISON).all()
        covered = want["covered"]
        assert (lp1[:, covered:] == LP_POISON).all()                            # nothing behind the covered positions
        for r in range(B):
            for j in range(covered):
                m = r * n + j
                t, l = L.merge(val[m], idx[m], ssum[m])
                assert t == tok[r, j] and abs(lp1[r, j] - l) <= TOL, (r, j, lp1[r, j], l)
