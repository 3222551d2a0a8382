"""The dual vocabulary head and the divergence merge through their debug hooks (include/gitcap.h: gitcap_dbg_vocab_head_dual,
gitcap_dbg_distill_final), against tests/distill_reference.py applied to the DEVICE's own fp32 logits (the single heads', which
the dual head must reproduce bit for bit), under the bound derived there."""
import ctypes

import numpy as np
import pytest
import torch

import distill_reference as D
import score_reference as S
from gitcap._lib import CDistillOut
from gpu_support import (IDX_FILL, NAN, TGT_FILL, assert_tail, close_to_fp64, lib, poisoned, ptr, run_vocab_head, same_bits, stream,  # noqa: F401
                         to_dev)

pytestmark = pytest.mark.gpu
PAD = 16
NAMES = ("t_max", "t_idx", "t_sum", "s_max", "s_idx", "s_sum", "cross")


def _dev(inp):
    return {k: (v.cuda() if v is not None else None) for k, v in inp.items()}


def run_dual(lib, d, M, N, Kt, Ks, tau, targets=None, rows=None):
    """one launch of the dual head over rows `rows` (default all) -> dict of the seven partials [M][nt] + t_logit / s_logit [M]"""
    Xt, Xs = (d["Xt"], d["Xs"]) if rows is None else (d["Xt"][rows].contiguous(), d["Xs"][rows].contiguous())
    nt = (N + 15) // 16
    buf = {k: poisoned(M * nt + PAD, IDX_FILL if k.endswith("idx") else NAN, torch.int32 if k.endswith("idx") else torch.float32) for k in NAMES}
    tl, sl = poisoned(M + PAD, TGT_FILL), poisoned(M + PAD, TGT_FILL)
    tg = to_dev(targets, torch.int64)
    rc = lib.gitcap_dbg_vocab_head_dual(ptr(Xt), Kt, ptr(d["Wt"]), ptr(d["wscale"]), ptr(d["bt"]), Kt, ptr(Xs), Ks, ptr(d["Ws"]), ptr(d["bs"]),
                                        Ks, M, N, ctypes.c_float(1.0 / tau), *[ptr(buf[k]) for k in NAMES], ptr(tg), ptr(tl), ptr(sl), stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k in NAMES:
        assert_tail(buf[k], M * nt, IDX_FILL if k.endswith("idx") else NAN)
    assert_tail(tl, M if targets is not None else 0, TGT_FILL)
    assert_tail(sl, M if targets is not None else 0, TGT_FILL)
    out = {k: buf[k][:M * nt].view(M, nt) for k in NAMES}
    out.update(t_logit=tl[:M], s_logit=sl[:M])
    return out


def run_final(lib, p, nt, ids, rows, T, lengths, ignore_id, V, want_lp=True):
    """gitcap_dbg_distill_final on poisoned outputs -> dict of host arrays"""
    n = rows * T
    kl, tlp, slp = poisoned(n + PAD, NAN), poisoned(rows * (T - 1) + PAD, NAN), poisoned(rows * (T - 1) + PAD, NAN)
    t1, s1 = poisoned(n + PAD, -777, torch.int64), poisoned(n + PAD, -777, torch.int64)
    ag = poisoned(n + PAD, 77, torch.uint8)
    rs, rc_ = poisoned(rows + PAD, NAN), poisoned(rows + PAD, -777, torch.int32)
    want_lp = want_lp and T > 1
    out = CDistillOut(kl.data_ptr(), T, t1.data_ptr(), s1.data_ptr(), ag.data_ptr(), tlp.data_ptr() if want_lp else None,
                      slp.data_ptr() if want_lp else None, T - 1, rs.data_ptr(), rc_.data_ptr())
    idd, ln = to_dev(ids, torch.int64), to_dev(lengths, torch.int32)
    rc = lib.gitcap_dbg_distill_final(*[ptr(p[k]) for k in NAMES], nt, ptr(p["t_logit"]), ptr(p["s_logit"]), ptr(idd), T, rows, T, ptr(ln),
                                      ignore_id, V, ctypes.byref(out), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert_tail(kl, n, NAN); assert_tail(t1, n, -777); assert_tail(s1, n, -777); assert_tail(ag, n, 77)
    assert_tail(tlp, rows * (T - 1) if want_lp else 0, NAN); assert_tail(slp, rows * (T - 1) if want_lp else 0, NAN)
    assert_tail(rs, rows, NAN); assert_tail(rc_, rows, -777)
    return dict(kl=kl[:n].view(rows, T), t_top1=t1[:n].view(rows, T), s_top1=s1[:n].view(rows, T), agree=ag[:n].view(rows, T),
                t_lp=tlp[:rows * (T - 1)].view(rows, T - 1), s_lp=slp[:rows * (T - 1)].view(rows, T - 1), kl_sum=rs[:rows], count=rc_[:rows])


def single_heads(lib, d, M, N, Kt, Ks):
    """each model alone through the existing LSE head (the e4m3 teacher as the bf16 matrix with the same values: exact)"""
    ht = run_vocab_head(lib, d["Xt"], Kt, d["Wt_bf16"], None, d["bt"], M, N, Kt, hook="lse")
    hs = run_vocab_head(lib, d["Xs"], Ks, d["Ws"], None, d["bs"], M, N, Ks, hook="lse")
    return ht, hs


def check_against_reference(lib, d, M, N, Kt, Ks, tau, ht, hs, what):
    ids, targets, lengths, ign = D.caption(M, N)
    p = run_dual(lib, d, M, N, Kt, Ks, tau, targets)
    nt = (N + 15) // 16
    got = run_final(lib, p, nt, ids, 1, M, lengths, ign, N)
    ref = D.distill_logits(ht.logits.cpu().numpy()[None], hs.logits.cpu().numpy()[None], ids, lengths, ign, tau)
    kl = got["kl"].cpu().numpy().astype(np.float64)
    inf = np.isinf(ref["kl"])
    assert np.array_equal(np.isinf(kl) & (kl > 0), inf), what
    assert not np.isnan(kl).any() and (kl >= -D.bound_kl(ref["G"])).all(), what
    fin = ~inf
    if fin.any():
        close_to_fp64(kl[fin], ref["kl"][fin], D.bound_kl(ref["G"])[fin], what + " kl", flips=False)
    assert np.array_equal(got["t_top1"].cpu().numpy(), ref["t_top1"]) and np.array_equal(got["s_top1"].cpu().numpy(), ref["s_top1"]), what
    assert np.array_equal(got["agree"].cpu().numpy().astype(bool), ref["agree"]), what
    assert int(got["count"][0]) == int(ref["count"][0]), what
    if np.isfinite(ref["kl_sum"][0]):
        bsum = float(D.bound_kl(ref["G"]).sum() + M * 2.0 ** -24 * np.abs(ref["kl"]).sum())
        close_to_fp64(got["kl_sum"].cpu().numpy(), ref["kl_sum"], bsum, what + " kl_sum", flips=False)
    else:
        assert float(got["kl_sum"][0]) == float("inf"), what
    if M > 1:
        for k in ("t_lp", "s_lp"):
            lp, r = got[k].cpu().numpy().astype(np.float64), ref[k]
            assert np.array_equal(np.isinf(lp), np.isinf(r)) and not np.isnan(lp).any(), what
            f = np.isfinite(r)
            assert (lp[~ref["counted"]] == 0).all(), what
            close_to_fp64(lp[f], r[f], S.bound_lp(r[f]), what + " " + k, flips=False)
    return p


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("Kt,Ks", D.KS)
@pytest.mark.parametrize("N", D.NS)
@pytest.mark.parametrize("M", D.MS)
def test_dual_head_and_merge(lib, M, N, Kt, Ks, fp8):
    d = _dev(D.dual_inputs(M, N, Kt, Ks, fp8))
    ht, hs = single_heads(lib, d, M, N, Kt, Ks)
    for tau in D.TEMPS:
        p = check_against_reference(lib, d, M, N, Kt, Ks, tau, ht, hs, f"M={M} N={N} K={Kt}+{Ks} fp8={fp8} tau={tau}")
        if tau == 1.0:          # the six single-model partials: bit for bit those of each model's own LSE head
            assert same_bits(p["t_max"], ht.val) and torch.equal(p["t_idx"], ht.idx) and same_bits(p["t_sum"], ht.sum)
            assert same_bits(p["s_max"], hs.val) and torch.equal(p["s_idx"], hs.idx) and same_bits(p["s_sum"], hs.sum)


@pytest.mark.parametrize("ninf", ["teacher", "student", "both"])
@pytest.mark.parametrize("Kt,Ks", [(128, 64), (768, 576)])
def test_minus_inf_columns(lib, Kt, Ks, ninf):
    """-inf bias columns (one whole tile among them): the teacher's contribute nothing, the student's alone make every row's kl +inf,
    the same columns in both leave a finite kl; NaN never appears."""
    M, N = 17, 197
    d = _dev(D.dual_inputs(M, N, Kt, Ks, False, ninf=ninf))
    ht, hs = single_heads(lib, d, M, N, Kt, Ks)
    for tau in D.TEMPS:
        p = check_against_reference(lib, d, M, N, Kt, Ks, tau, ht, hs, f"ninf={ninf} K={Kt}+{Ks} tau={tau}")
        assert not torch.isnan(p["cross"]).any()
        tile = slice(1, 2)                                   # columns 16 .. 31
        if ninf in ("teacher", "both"):
            assert bool((p["t_sum"][:, tile] == 0).all()) and bool((p["cross"][:, tile] == 0).all())
        ids, _, lengths, ign = D.caption(M, N)
        kl = run_final(lib, p, (N + 15) // 16, ids, 1, M, None, ign, N, want_lp=False)["kl"]
        assert bool(torch.isinf(kl).all()) if ninf == "student" else bool(torch.isfinite(kl).all())


@pytest.mark.parametrize("Kt,Ks", D.KS)
def test_row_alone_and_among_others(lib, Kt, Ks):
    """a row's partials and results are bitwise the same at M = 1 as inside M = 37"""
    M, N = 37, 197
    d = _dev(D.dual_inputs(M, N, Kt, Ks, False))
    ids, targets, _, ign = D.caption(M, N)
    nt = (N + 15) // 16
    for tau in D.TEMPS:
        full = run_dual(lib, d, M, N, Kt, Ks, tau, targets)
        allr = run_final(lib, full, nt, ids, M, 1, None, ign, N, want_lp=False)
        for r in (0, 15, 16, 36):
            one = run_dual(lib, d, 1, N, Kt, Ks, tau, targets[r:r + 1], rows=slice(r, r + 1))
            for k in NAMES + ("t_logit", "s_logit"):
                a, b = one[k].reshape(-1), full[k][r].reshape(-1)
                assert torch.equal(a, b) if a.dtype == torch.int32 else same_bits(a, b), (k, r, tau)
            alone = run_final(lib, one, nt, ids[:, r:r + 1], 1, 1, None, ign, N, want_lp=False)
            assert same_bits(alone["kl"].reshape(-1), allr["kl"][r].reshape(-1)), (r, tau)
            assert int(alone["t_top1"][0, 0]) == int(allr["t_top1"][r, 0]) and int(alone["s_top1"][0, 0]) == int(allr["s_top1"][r, 0])


def test_refusals(lib):
    """bad arguments: GITCAP_ERR_ARG, nothing written"""
    M, N, Kt, Ks = 3, 97, 128, 64
    d = _dev(D.dual_inputs(M, N, Kt, Ks, False))
    nt = (N + 15) // 16
    buf = {k: poisoned(M * nt, IDX_FILL if k.endswith("idx") else NAN, torch.int32 if k.endswith("idx") else torch.float32) for k in NAMES}
    def call(Kt_=Kt, Ks_=Ks, inv=1.0, M_=M):
        return lib.gitcap_dbg_vocab_head_dual(ptr(d["Xt"]), Kt, ptr(d["Wt"]), None, ptr(d["bt"]), Kt_, ptr(d["Xs"]), Ks, ptr(d["Ws"]), ptr(d["bs"]),
                                              Ks_, M_, N, ctypes.c_float(inv), *[ptr(buf[k]) for k in NAMES], None, None, None, stream())
    for kw in (dict(Kt_=96), dict(Ks_=128), dict(inv=0.0), dict(inv=-1.0), dict(inv=float("inf")), dict(inv=float("nan")), dict(M_=0)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    for k in NAMES:
        assert_tail(buf[k], 0, IDX_FILL if k.endswith("idx") else NAN)
