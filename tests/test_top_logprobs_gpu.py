"""The top-k alternatives kernel on the MI355X through gitcap_dbg_head_topk (the three-partial head, or its BAN form, + the new
launch).  The yardstick is exact: the expected ranks are the restatement of tests/top_logprobs_reference.py applied to the
DEVICE's own logits (the head hook with `logits` set: the same MFMA chain, the same bits) and the device's own winner
log-probability (gitcap_dbg_argmax_final_lp on the same partials).  ids must be equal, log-probabilities must compare ==, rank 0
must be the arg-max launch's token and value.  Nothing here depends on a measured tolerance.

Shapes: D in {64, 128, 768} (+ one case each of the other head widths), V = 40 (3 tiles, the last with 8 columns: fewer tiles
than k), 1000, 30522 (1908 tiles, the last with 10 columns) and 33000 (2063 tiles: beyond the partials the kernel stages in
LDS), M = 1 and 18 (two m-tiles of the head, a ragged second), k in {1, 2, 8, 32}, bf16 and e4m3 weights, row-major and
fragment-major.  Inputs: top_logprobs_reference.head_case."""
import numpy as np
import pytest
import torch

import top_logprobs_reference as T
from gpu_support import NAN, assert_tail, e4m3_rows, lib, poisoned, ptr, stream  # noqa: F401

pytestmark = pytest.mark.gpu

KS = (1, 2, 8, 32)
ID_FILL = -777


def _upload(lib, case, fp8, packed):
    X = torch.as_tensor(case["X"]).cuda().bfloat16()
    Wf = torch.as_tensor(case["W"]).cuda()
    if fp8:
        W, wscale, back = e4m3_rows(Wf)
    else:
        W, wscale = Wf.bfloat16(), None
        back = W.float()
    assert torch.equal(back, Wf) and torch.equal(X.float().cpu(), torch.as_tensor(case["X"]))      # the stored operands are exact
    Wpk = None
    if packed:
        Wpk = torch.empty_like(W)
        assert lib.gitcap_dbg_pack_frags(ptr(W), ptr(Wpk), W.shape[0], W.shape[1], 1 if fp8 else 2, stream()) == 0
    bias = torch.as_tensor(case["bias"]).cuda()
    mask, ld = None, 0
    if case["ban"] is not None:
        ld = (W.shape[0] // 16 + 1) // 2 * 2
        mask = torch.as_tensor(T.pack_ban(case["ban"], ld).view(np.int16)).cuda()
    return X, W, Wpk, wscale, bias, mask, ld


def _device_rows(lib, X, W, wscale, bias, mask, ld, M, V, D):
    """the device's own logits [M, V], arg-max tokens and winner log-probabilities of the rows"""
    nt = (V + 15) // 16
    logits, val, ssum = poisoned(M * V, NAN), poisoned(M * nt, NAN), poisoned(M * nt, NAN)
    idx = poisoned(M * nt, -5, torch.int32)
    head = (ptr(X), D, ptr(W), ptr(wscale), ptr(bias), M, V, D, ptr(logits), ptr(val), ptr(idx), ptr(ssum))
    rc = lib.gitcap_dbg_vocab_head_banned(*head, ptr(mask), ld, stream()) if mask is not None else lib.gitcap_dbg_vocab_head_lse(*head, stream())
    assert rc == 0
    tok = torch.full((M,), -9, device="cuda", dtype=torch.int64)
    lp = poisoned(M, NAN)
    assert lib.gitcap_dbg_argmax_final_lp(ptr(val), ptr(idx), nt, M, 1, 0, ptr(tok), 1, None, 0, -1, None, ptr(ssum), ptr(lp), 1, stream()) == 0
    torch.cuda.synchronize()
    return logits.view(M, V).cpu().numpy(), tok.cpu().numpy(), lp.cpu().numpy()


def _topk(lib, X, W, Wpk, wscale, bias, mask, ld, M, V, D, k):
    ids, lp = poisoned(M * k + 16, ID_FILL, torch.int64), poisoned(M * k + 16, NAN)
    rc = lib.gitcap_dbg_head_topk(ptr(X), D, M, ptr(W), ptr(Wpk), ptr(wscale), ptr(bias), V, D, k, ptr(mask), ld, ptr(ids), ptr(lp), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert_tail(ids, M * k, ID_FILL)
    assert_tail(lp, M * k, NAN)
    return ids[:M * k].view(M, k).cpu().numpy(), lp[:M * k].view(M, k).cpu().numpy()


SHAPES = [(1, 40, 64, False, False), (18, 40, 64, False, True), (18, 40, 128, True, False),
          (18, 1000, 128, False, False), (18, 1000, 128, True, True), (1, 1000, 768, True, False), (18, 1000, 768, False, True),
          (18, 30522, 768, False, False), (18, 30522, 768, True, True), (1, 30522, 64, False, True), (18, 30522, 128, True, False),
          (18, 1000, 256, False, False), (18, 1000, 576, False, True), (18, 1000, 1024, False, False),
          (2, 33000, 64, False, False)]


@pytest.mark.parametrize("scenario", T.SCENARIOS)
@pytest.mark.parametrize("M,V,D,fp8,packed", SHAPES)
def test_head_topk_is_exact(lib, M, V, D, fp8, packed, scenario):
    case = T.head_case(M, V, D, scenario)
    X, W, Wpk, wscale, bias, mask, ld = _upload(lib, case, fp8, packed)
    dev_logits, tok, lpw = _device_rows(lib, X, W, wscale, bias, mask, ld, M, V, D)
    for m in range(M):                                   # the inputs are exact in fp32: the device's logits are the reference's
        assert np.array_equal(dev_logits[m], T.masked(case, m)), m
    for k in KS:
        ids, lp = _topk(lib, X, W, Wpk, wscale, bias, mask, ld, M, V, D, k)
        assert not np.isnan(lp).any()
        for m in range(M):
            want_ids, want_lp = T.top_k(dev_logits[m], dev_logits[m].max(), lpw[m], k)
            assert ids[m].tolist() == want_ids.tolist(), (k, m)
            assert np.array_equal(lp[m], want_lp), (k, m, lp[m], want_lp)          # ==, -inf padding included
        assert ids[:, 0].tolist() == tok.tolist() and np.array_equal(lp[:, 0], lpw)   # rank 0 = the arg-max launch
        if scenario == "ban_keep3":
            assert (ids[:, :3] >= 0).all() and (ids[:, 3:] == -1).all() and np.isneginf(lp[:, 3:]).all()
        if scenario == "ban_winner":
            assert not case["ban"][np.arange(M)[:, None], ids.clip(0)][ids >= 0].any()   # no banned column is reported
        assert (ids < V).all()                                                           # nor a padded weight row
    if M > 1:       # a row does not depend on the rows beside it: row M - 1 alone, bit for bit
        m = M - 1
        one = _topk(lib, X[m:m + 1].contiguous(), W, Wpk, wscale, bias, None if mask is None else mask[m:m + 1].contiguous(), ld, 1, V, D, 8)
        all_ = _topk(lib, X, W, Wpk, wscale, bias, mask, ld, M, V, D, 8)
        assert np.array_equal(one[0][0], all_[0][m]) and np.array_equal(one[1][0].view(np.int32), all_[1][m].view(np.int32))


def test_head_topk_all_columns_banned(lib):
    """no column above -inf: every rank is padding, no NaN"""
    case = T.head_case(2, 40, 64, "natural")
    case["ban"] = np.ones((2, 40), bool)
    X, W, Wpk, wscale, bias, mask, ld = _upload(lib, case, False, False)
    ids, lp = _topk(lib, X, W, Wpk, wscale, bias, mask, ld, 2, 40, 64, 8)
    assert (ids == -1).all() and np.isneginf(lp).all()


def test_head_topk_rejects_bad_arguments(lib):
    x = torch.zeros(16, 64, device="cuda", dtype=torch.bfloat16)
    o = torch.zeros(64, device="cuda", dtype=torch.int64)
    f = torch.zeros(64, device="cuda")
    ok = lambda k=2, D=64, X=x, ids=o: lib.gitcap_dbg_head_topk(ptr(X), D, 1, ptr(x), None, None, None, 16, D, k, None, 0, ptr(ids), ptr(f), stream())
    assert ok() == 0
    assert ok(k=0) == -1 and ok(k=33) == -1 and ok(D=96) == -1 and ok(X=None) == -1 and ok(ids=None) == -1
    torch.cuda.synchronize()
