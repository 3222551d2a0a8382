"""GPU: launch_draft_accept_rows and the KEEP form of launch_argmax_final through their hooks, against tests/draft_rows_reference.py,
exactly.  The log-probability bits are those of gitcap_dbg_argmax_final_lp on the same partial rows (lp_partials' bits; that launch
is checked against fp64 in tests/test_logprob_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import draft_rows_reference as ref
from gpu_support import NAN, assert_tail, lib, poisoned, ptr, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _loop_lp(lib, val, idx, ssum, rows, nt):
    """(tokens, log-probability bits) of `rows` partial rows as the token loop's arg-max launch forms them"""
    out = poisoned(rows, -777, I64)
    lp = poisoned(rows, NAN)
    assert lib.gitcap_dbg_argmax_final_lp(ptr(val), ptr(idx), nt, rows, 1, 0, ptr(out), 1, None, 0, ref.SEP, None, ptr(ssum), ptr(lp), 1,
                                          stream()) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), lp.cpu().numpy()


def _run_accept(lib, case, B, n, with_lp, bufs=None):
    nt = case["val"].shape[1]
    val, idx, ssum = to_dev(case["val"], F32), to_dev(case["idx"], I32), to_dev(case["sum"], F32)
    ld, ld_lp = n + 3, n + 2
    ids = torch.cat([to_dev(case["ids"], I64).reshape(-1), poisoned(16, -777, I64)])
    length = poisoned(B + 16, -777, I32)
    cnt = torch.cat([to_dev(case["sep_cnt0"], I32), poisoned(16, -777, I32)])
    lp_out = poisoned(B * ld_lp + 16, NAN)
    tok, row_res, ticket = bufs or (torch.zeros(B * n, dtype=I32, device="cuda"), torch.zeros(2 * B, dtype=I32, device="cuda"),
                                    torch.zeros(1 + B, dtype=I32, device="cuda"))
    host = (ctypes.c_int32 * (4 + B))()
    head = (ptr(val), ptr(idx), nt, B, n, ptr(ids), ld, ptr(length), ptr(tok), ptr(row_res), ptr(ticket), ptr(cnt), ref.SEP, host)
    if with_lp:
        rc = lib.gitcap_dbg_draft_accept_rows_lp(*head, ptr(ssum), ptr(lp_out), ld_lp, stream())
    else:
        rc = lib.gitcap_dbg_draft_accept_rows(*head, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert int(ticket.abs().sum()) == 0                                     # re-armed
    # the restatement, on the loop's own tokens and log-probability bits
    tok_ref, lp_bits = _loop_lp(lib, val, idx, ssum, B * n, nt)
    assert np.array_equal(tok_ref, ref.tokens_of_partials(case["val"].astype(np.float64), case["idx"].astype(np.int64)))
    lp0 = np.full((B, ld_lp), np.nan, dtype=np.float32)
    want = ref.accept_rows(tok_ref.reshape(B, n), case["ids"], ref.SEP, case["sep_cnt0"], lp_bits.reshape(B, n) if with_lp else None,
                           lp0 if with_lp else None)
    assert want["a_r"] == case["a_r"]
    assert np.array_equal(ids[:B * ld].view(B, ld).cpu().numpy(), want["ids"])
    assert np.array_equal(length[:B].cpu().numpy(), want["len"])
    assert np.array_equal(cnt[:n + 2].cpu().numpy(), want["sep_cnt"])
    assert tuple(host[:4]) == want["host"] and list(host[4:4 + B]) == want["a_r"]
    if with_lp:
        got = lp_out[:B * ld_lp].view(B, ld_lp).cpu().numpy()
        assert np.array_equal(got.view(np.int32), want["lp_out"].view(np.int32))       # NaN poison behind the covered part included
    else:
        assert_tail(lp_out, 0, NAN)
    assert_tail(ids, B * ld, -777)
    assert_tail(length, B, -777)
    assert_tail(cnt, n + 2, -777)
    assert_tail(lp_out, B * ld_lp, NAN)
    return tok, row_res, ticket


@pytest.mark.parametrize("with_lp", [False, True])
@pytest.mark.parametrize("B,n,V", ref.ACCEPT_SHAPES)
def test_accept_rows_exact(lib, B, n, V, with_lp):
    # every pattern at the small vocabulary; at 30 522 words (1908 tiles) the pattern whose rows differ, with SEP in different steps
    combos = [(p, s) for p in ref.PATTERNS for s in ("none", "same", "diff")] if V == 100 else [("mixed", "diff"), ("full", "same")]
    bufs = None
    for pattern, sep in combos:                                             # back to back on the same scratch: the tickets re-arm
        bufs = _run_accept(lib, ref.accept_case(B, n, V, pattern, sep, 7), B, n, with_lp, bufs)


def test_accept_rows_rejects_bad_arguments(lib):
    case = ref.accept_case(1, 2, 100, "zero", "none", 0)
    val, idx = to_dev(case["val"], F32), to_dev(case["idx"], I32)
    ids, z = to_dev(case["ids"], I64), torch.zeros(8, dtype=I32, device="cuda")
    host = (ctypes.c_int32 * 8)()
    for B, n, ld in ((1, 64, 70), (1, 0, 5), (0, 2, 5), (1, 2, 2)):
        assert lib.gitcap_dbg_draft_accept_rows(ptr(val), ptr(idx), 7, B, n, ptr(ids), ld, ptr(z), ptr(z), ptr(z), ptr(z), ptr(z),
                                                ref.SEP, host, stream()) != 0


@pytest.mark.parametrize("with_lp", [False, True])
@pytest.mark.parametrize("embed", [False, True])
@pytest.mark.parametrize("V", [100, 30522])
def test_argmax_keep_exact(lib, V, embed, with_lp):
    from gitcap._lib import CDbgNextEmbed
    rows, max_len, D = 16, 10, 128
    g = torch.Generator(device="cuda").manual_seed(1)
    word, pos = torch.randn(V, D, device="cuda", generator=g), torch.randn(max_len + 1, D, device="cuda", generator=g)
    gamma, beta = torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)
    for case in ref.keep_case(rows, V, max_len, 3):
        nt = case["val"].shape[1]
        val, idx, ssum = to_dev(case["val"], F32), to_dev(case["idx"], I32), to_dev(case["sum"], F32)
        step, ld = case["step"], max_len + 1
        tok_ref, lp_bits = _loop_lp(lib, val, idx, ssum, rows, nt)
        assert np.array_equal(tok_ref, case["tok"])
        ids0 = np.full((rows, ld), -5, dtype=np.int64)
        ids0[:, step + 1] = case["out0"]
        lp0 = np.full((rows, max_len), -2.5, dtype=np.float32)
        cnt0 = np.arange(max_len + 1, dtype=np.int32)

        def launch(keep):
            ids = torch.cat([to_dev(ids0, I64).reshape(-1), poisoned(16, -777, I64)])
            lp = torch.cat([to_dev(lp0, F32).reshape(-1), poisoned(16, NAN)])
            cnt = torch.cat([to_dev(cnt0, I32), poisoned(16, -777, I32)])
            xf, xb = poisoned(rows * D + 16, NAN), poisoned(rows * D + 16, NAN, torch.bfloat16)
            emb = CDbgNextEmbed(word.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, D, V, step + 1, xf.data_ptr(),
                                xb.data_ptr()) if embed else None
            head = (ptr(val), ptr(idx), nt, rows, 1, 0, ctypes.c_void_p(ids.data_ptr() + 8 * (step + 1)), ld, ptr(cnt), step, ref.SEP,
                    ctypes.byref(emb) if embed else None)
            lpp = ctypes.c_void_p(lp.data_ptr() + 4 * step)
            if keep:
                rc = lib.gitcap_dbg_argmax_final_keep(*head, ptr(ssum) if with_lp else None, lpp if with_lp else None, max_len,
                                                      ptr(to_dev(case["len"], I32)), stream())
            elif with_lp:
                rc = lib.gitcap_dbg_argmax_final_lp(*head, ptr(ssum), lpp, max_len, stream())
            else:
                rc = lib.gitcap_dbg_argmax_final(*head, stream())
            torch.cuda.synchronize()
            assert rc == 0
            return ids, lp, cnt, xf, xb

        ids, lp, cnt, xf, xb = launch(True)
        w_out, w_lp, w_cnt, w_emb = ref.argmax_keep(tok_ref, lp_bits, case["out0"], lp0[:, step], cnt0, step, ref.SEP, case["len"])
        kept = step + 1 < case["len"]
        assert kept.any() and not kept.all()                                # kept and free rows mixed
        want_ids = ids0.copy()
        want_ids[:, step + 1] = w_out
        assert np.array_equal(ids[:rows * ld].view(rows, ld).cpu().numpy(), want_ids)
        assert np.array_equal(cnt[:max_len + 1].cpu().numpy(), w_cnt)
        want_lp = lp0.copy()
        if with_lp:
            want_lp[:, step] = w_lp
        assert np.array_equal(lp[:rows * max_len].view(rows, max_len).cpu().numpy().view(np.int32), want_lp.view(np.int32))
        assert_tail(ids, rows * ld, -777)
        assert_tail(cnt, max_len + 1, -777)
        assert_tail(lp, rows * max_len, NAN)
        if embed:
            # the embedded rows are the plain launch's on the tokens the kept launch ends with: plant them as the winners' ids
            ids0_p = ids0.copy()
            ids_p, _, _, xf_p, xb_p = launch(False)
            free = ~kept
            assert torch.equal(xf[:rows * D].view(rows, D)[torch.from_numpy(free)].view(I32),
                               xf_p[:rows * D].view(rows, D)[torch.from_numpy(free)].view(I32))
            # a kept row: the embedding of the stored id = embedding + LayerNorm computed in fp64 within 1e-4
            x = (word[torch.from_numpy(w_emb).cuda()] + pos[step + 1]).double()
            y = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5) * gamma.double() + beta.double()
            assert float((xf[:rows * D].view(rows, D).double() - y).abs().max()) < 1e-4
            assert_tail(xf, rows * D, NAN)
            del ids0_p, ids_p, xb_p
        else:
            assert_tail(xf, 0, NAN)
