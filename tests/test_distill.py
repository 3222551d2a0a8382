"""tests/distill_reference.py held to torch, its -inf rules, the fast-exp measurement behind its bound, and proof that the
inputs of tests/test_distill_gpu.py tell deliberately wrong kernels from the right one.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")


def _logits(R, T, V, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, T, V)) * 3).astype(np.float32), (rng.standard_normal((R, T, V)) * 3).astype(np.float32)


@pytest.mark.parametrize("tau", [1.0, 2.0, 0.7])
@pytest.mark.parametrize("V", [97, 197, 16])
def test_restatement_is_kl_div_and_cross_entropy(V, tau):
    R, T = 3, 5
    t, s = _logits(R, T, V, V)
    y = np.random.default_rng(1).integers(0, V, (R, T))
    y[0, 2] = 0
    o = D.distill_logits(t, s, y, temperature=tau)
    ts, ss = D.scaled(t, s, tau)
    ref = F.kl_div(torch.log_softmax(torch.from_numpy(ss), -1), torch.softmax(torch.from_numpy(ts), -1), reduction="batchmean") * tau * tau
    assert abs(D.kl_loss(o["kl"], R, tau) - float(ref)) <= 1e-10 * max(1.0, abs(float(ref)))
    ce = F.cross_entropy(torch.from_numpy(ss)[:, :-1].reshape(-1, V), torch.from_numpy(y)[:, 1:].reshape(-1), ignore_index=0)
    assert abs(D.ce_loss(o["s_lp"], y) - float(ce)) <= 1e-10 * max(1.0, abs(float(ce)))
    assert np.array_equal(o["t_top1"], ts.argmax(-1)) and np.array_equal(o["s_top1"], ss.argmax(-1))


def test_lengths_rule():
    t, s = _logits(2, 4, 40, 3)
    y = np.ones((2, 4), np.int64)
    o = D.distill_logits(t, s, y, lengths=np.array([1, 3]))
    full = D.distill_logits(t, s, y)
    assert (o["kl"][0, 1:] == 0).all() and o["kl"][0, 0] == full["kl"][0, 0] and (o["kl"][1, 3] == 0)
    assert list(o["count"]) == [1, 3] and abs(o["kl_sum"][1] - full["kl"][1, :3].sum()) < 1e-12


def test_minus_inf_rules():
    t, s = _logits(1, 1, 48, 5)
    tt, ss = t.copy(), s.copy()
    tt[..., 3] = NINF                                            # teacher only: contributes nothing
    a = D.distill_logits(tt, ss, np.ones((1, 1), np.int64))["kl"][0, 0]
    ref = F.kl_div(torch.log_softmax(torch.from_numpy(ss).double(), -1), torch.softmax(torch.from_numpy(tt).double(), -1), reduction="sum")
    assert np.isfinite(a) and abs(a - float(ref)) < 1e-10
    ss[..., 7] = NINF                                            # student only: +inf
    assert D.distill_logits(t, ss, np.ones((1, 1), np.int64))["kl"][0, 0] == np.inf
    tt[..., 7] = NINF                                            # both: finite again
    assert np.isfinite(D.distill_logits(tt, ss, np.ones((1, 1), np.int64))["kl"][0, 0])
    tt[..., 16:32] = NINF                                        # a whole -inf tile: t_sum = cross = 0
    p = D.dual_partials(tt.reshape(1, -1).astype(np.float64), ss.reshape(1, -1).astype(np.float64))
    assert p["t_sum"][0, 1] == 0 and p["cross"][0, 1] == 0 and p["t_max"][0, 1] == NINF
    ss[..., 16:32] = NINF
    o = D.distill_logits(tt, ss, np.ones((1, 1), np.int64))
    assert np.isfinite(o["kl"]).all() and not np.isnan(o["G"]).any()
    allinf = np.full_like(t, NINF)
    assert D.distill_logits(allinf, s, np.ones((1, 1), np.int64))["kl"][0, 0] == 0.0


def _gpu_cases():
    for M in D.MS:
        for N in D.NS:
            for Kt, Ks in D.KS[:2] if N == 1000 else D.KS:       # (host matmuls: the largest pair once per N is enough here)
                yield M, N, Kt, Ks


def test_fast_exp_factor_is_the_recorded_one():
    """DELTA_MEASURED: the fp32 restatement of the kernels' loops against fp64 on the GPU tests' inputs; the bound takes it x 4"""
    worst = 0.0
    for M, N, Kt, Ks in _gpu_cases():
        for fp8 in (False, True):
            t, s = D.host_logits(D.dual_inputs(M, N, Kt, Ks, fp8))
            for tau in D.TEMPS:
                worst = max(worst, D.delta_of(*D.scaled(t, s, tau)))
    print(f"worst |A32 - A64| / G = {worst:.3e}")
    assert worst <= D.DELTA_MEASURED and D.K_REL == 4 * D.DELTA_MEASURED


@pytest.mark.parametrize("wrong", ["wrong_centre", "no_recentre", "swapped", "drop_tail", "temp_one"])
def test_wrong_kernels_miss_the_bound(wrong):
    seen = 0
    for M, N, Kt, Ks in _gpu_cases():
        if Kt != 128 or M == 1:
            continue
        t, s = D.host_logits(D.dual_inputs(M, N, Kt, Ks, False))
        ids, _, lengths, ign = D.caption(M, N)
        for tau in D.TEMPS:
            if wrong == "temp_one" and tau == 1.0:
                continue
            good = D.distill_logits(t[None], s[None], ids, lengths, ign, tau)
            bad = D.distill_logits(t[None], s[None], ids, lengths, ign, tau, wrong=wrong)
            ratio = float((np.abs(bad["kl"] - good["kl"]) / D.bound_kl(good["G"])).max())
            assert ratio > 10.0, (wrong, M, N, tau, ratio)
            seen += 1
    assert seen >= 6


def test_abi_version_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "gitcap.h")).read()
    src = open(os.path.join(ROOT, "real-time-video-captioning_amd", "csrc", "gitcap.hip")).read()
    assert re.search(r"#define\s+GITCAP_ABI_VERSION\s+1\b", src)
    from gitcap import _lib
    for name in ("gitcap_distill", "gitcap_dbg_vocab_head_dual", "gitcap_dbg_distill_final"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\(" % name, hdr)
    assert len(_lib.CDistillOut._fields_) == 10
    import gitcap
    assert callable(gitcap.distill_report)
