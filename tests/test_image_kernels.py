"""The fp64 restatements of tests/image_kernels_reference.py against the obvious torch.float64 formulation, and -- for every input
generator and shape of tests/test_image_kernels_gpu.py -- an fp32 emulation of the operation on the CPU (plain numpy, two summation
orders): it must stay within the derived bound with at most 2 % of its bf16 outputs off the correctly rounded reference.  That shows
the bounds and the cap are attainable by a correct implementation before the device runs.  No GPU, no library."""
import numpy as np
import pytest
import torch

import image_kernels_reference as R
from text_rows_reference import bf16_rne, e4m3_decode, e4m3_encode, flip_share, gelu, quick_gelu

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))                     # noqa: E731


def _within(got, ref, bound, what, flips_ref=None, mask=None):
    ratio = float((np.abs(got - ref) / bound).max())
    assert ratio <= 1.0, (what, ratio)
    if flips_ref is not None:
        m = np.ones(ref.shape, bool) if mask is None else mask
        share = flip_share(got[m], flips_ref[m])
        assert share <= 0.02, (what, share)


# ---- restatements ---------------------------------------------------------------------------------------------------------------

def test_gemm_restatement_equals_torch_float64():
    q = R.gemm_inputs(128, 64, 192, 1)
    y, e = R.gemm(q["A"], q["W"], q["bias"], q["resid"])
    want = T(q["A"]) @ T(q["W"]).t() + T(q["bias"]) + T(q["resid"])
    assert np.allclose(y, want.numpy(), rtol=1e-13, atol=1e-13)
    assert (e > 0).all() and np.array_equal(y[2], q["bias"] + q["resid"][2])          # the zero row
    for epi, act in ((1, lambda t: t * torch.sigmoid(1.702 * t)), (2, torch.nn.functional.gelu)):
        assert np.allclose(R.act(epi, y), act(T(y)).numpy(), rtol=1e-12, atol=1e-14)
    assert R.ACT[8] is quick_gelu and R.ACT[9] is gelu


def test_f8_truncation_restates_the_probe():
    """The probe's rows: beside 256 a product 2^-5 survives, 2^-6 vanishes, 1.75 2^-4 arrives as 1.5 2^-4; other groups are exact."""
    W = np.ones((1, 128))
    row = lambda pairs: np.array([[dict(pairs).get(k, 0.0) for k in range(128)]])                  # noqa: E731
    for pairs, want in (([(0, 256.0), (1, 2.0 ** -5)], 256 + 2.0 ** -5), ([(0, 256.0), (1, 2.0 ** -6)], 256.0),
                        ([(0, 256.0), (1, -2.0 ** -6)], 256.0), ([(0, 256.0), (1, 1.75 * 2.0 ** -4)], 256 + 1.5 * 2.0 ** -4),
                        ([(0, 256.0), (33, 2.0 ** -9)], 256 + 2.0 ** -9), ([(0, 256.0), (1, -256.0), (2, 2.0 ** -6)], 0.0),
                        ([(0, 256.0)] + [(k, 2.0 ** -9) for k in range(1, 128)], 256 + 120 * 2.0 ** -9)):
        A = row(pairs)
        assert R.gemm_f8_model(A, W, 0.0)[0, 0] == want
        assert abs(want - A.sum()) <= R.f8_truncation(A, W)[0, 0] <= 7 * 2.0 ** -5


def test_fp8_inputs_are_exact_codes():
    q = R.gemm_f8_inputs(256, 256, 128, 2)
    assert np.array_equal(e4m3_encode(q["A"] / R.F8_ASCALE), q["Ac"]) and np.array_equal(e4m3_decode(q["Wc"]) * q["wscale"][:, None], q["W"])
    assert np.array_equal(T(q["Ac"]).view(torch.float8_e4m3fn).double().numpy() * R.F8_ASCALE, q["A"])
    assert not ((q["Ac"] & 0x7f) == 0x7f).any() and not ((q["Wc"] & 0x7f) == 0x7f).any()        # no NaN code among the operands
    assert (np.log2(q["wscale"]) % 1 == 0).all()


@pytest.mark.parametrize("D", [64, 100, 768])
def test_layernorm_restatement_equals_torch_float64(D):
    q = R.ln_inputs(9, D, 3)
    ref, bound = R.ln_rows(q, 1e-5)
    want = torch.nn.functional.layer_norm(T(q["x"]), (D,), T(q["g"]), T(q["b"]), 1e-5).numpy()
    assert np.allclose(ref, want, rtol=1e-9, atol=1e-9)
    const = [r for r, k in enumerate(R.row_kinds(9)) if k == "const"]
    assert np.array_equal(ref[const], np.broadcast_to(q["b"], (len(const), D))) and (bound > 0).all()


def test_gemm_ln_restatement_equals_torch_float64():
    q = R.gemm_ln_inputs(256, 768, 64, True, 4)
    x, e, ln, bound = R.gemm_ln(q)
    tx = T(q["A"]) @ T(q["W"]).t() + T(q["bias"]) + T(q["resid"])
    assert np.allclose(x, tx.numpy(), rtol=1e-13, atol=1e-12)
    assert np.allclose(ln, torch.nn.functional.layer_norm(tx, (768,), T(q["g"]), T(q["b"]), 1e-5).numpy(), rtol=1e-7, atol=1e-7)
    hard, const = x[R.GEMM_LN_HARD_ROW], x[R.GEMM_LN_CONST_ROW]
    assert abs(hard.mean() - 1e3) < 0.01 and 5e-3 < hard.std() < 2e-2 and (const == 0.75).all()
    assert np.array_equal(ln[R.GEMM_LN_CONST_ROW], q["b"])


@pytest.mark.parametrize("kind", R.ATTN_KINDS)
def test_attn_restatement_equals_torch_float64(kind):
    G, S, H = 2, 97, 3
    qkv = R.attn_inputs(G, S, H, kind, 5)
    ctx, ctxp, bound = R.attn_full(qkv, G, S, H)
    q, k, v = (t.view(G, S, H, 64).transpose(1, 2) for t in T(qkv).split(64 * H, dim=1))
    want = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).transpose(1, 2).reshape(G * S, 64 * H).numpy()
    assert np.allclose(ctx, want, rtol=1e-11, atol=1e-12)
    assert (np.abs(ctxp - ctx) <= bound).all()
    if kind == "mean":          # equal scores: every p is 1, its rounding exact, the context the mean of V
        assert np.array_equal(ctxp, ctx)
        assert np.allclose(ctx.reshape(G, S, H, 64), np.broadcast_to(qkv.reshape(G, S, 3, H, 64)[:, :, 2].mean(axis=1, keepdims=True), (G, S, H, 64)))
    if kind == "late":          # the last key holds most of the mass, not all of it
        p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)[..., -1]
        assert 0.85 < float(p.min()) and float(p.max()) < 0.9999


def test_a_missed_key_is_outside_the_bound():
    """What the device test would report for the mistakes of the issue's mutation list, on the CPU: the reference of S keys against
    the context of a kernel that drops the last key (mask at key > S - 1 ...), or counts a padded copy of it (key >= S + 1)."""
    for S in (33, 97, 129, 289):
        for kind in ("late", "mean"):
            qkv = R.attn_inputs(1, S, 1, kind, S)
            ctx, ctxp, bound = R.attn_full(qkv, 1, S, 1)
            dropped = R.attn_full(np.delete(qkv, S - 1, axis=0), 1, S - 1, 1)[0]
            dup = R.attn_full(np.concatenate([qkv, qkv[-1:]]), 1, S + 1, 1)[0][:S]
            for wrong in (dropped, dup[:S - 1]):
                got = bf16_rne(wrong)
                assert (np.abs(got - ctx[:S - 1]) > bound[:S - 1]).any() or flip_share(got, ctxp[:S - 1]) > 0.02, (S, kind)


# ---- fp32 emulations: the bounds and the 2 % cap are attainable -----------------------------------------------------------------

@pytest.mark.parametrize("M,N", sorted({(M, N) for _, M, N in R.GEMM_SHAPES}))
@pytest.mark.parametrize("K", R.GEMM_KS)
def test_gemm_fp32_emulation_meets_the_bounds(M, N, K):
    q = R.gemm_inputs(M, N, K, M + N + K)
    for order in ("seq", "pair"):
        for resid in (None, q["resid"]):
            y, e = R.gemm(q["A"], q["W"], q["bias"], resid)
            got = R.gemm_fp32(q["A"], q["W"], q["bias"], resid, order)
            _within(got, y, e, ("fp32", M, N, K, order))
            if resid is None:
                _within(bf16_rne(got), y, R.rounded_bound(y, e), ("bf16", M, N, K, order), flips_ref=y)
                if K == R.GEMM_ACT_K:
                    for epi in (1, 2):
                        out = R.act(epi, got)
                        dev = bf16_rne(out.astype(np.float32).astype(np.float64))
                        bound, ok = R.act_bound_bf16(got, out)
                        assert ok.mean() > 0.6
                        _within(dev, out, bound, ("act", epi), flips_ref=out, mask=ok)


@pytest.mark.parametrize("K", R.F8_KS)
def test_gemm_f8_fp32_emulation_meets_the_bounds(K):
    q = R.gemm_f8_inputs(256, 256, K, K)
    y, e = R.gemm_f8(q["A"], q["W"], q["bias"])
    model = R.gemm_f8_model(q["A"], q["W"], q["bias"])                  # the matrix instruction's truncation, as probed
    assert (np.abs(model - y) <= R.f8_truncation(q["A"], q["W"]) + 1e-15 * np.abs(y)).all() and (model != y).mean() > 0.5
    for order in ("seq", "pair"):
        got = R.gemm_fp32(q["A"], q["W"], q["bias"], None, order)
        _within(got, y, e, ("f8 fp32", K, order))
        _within(bf16_rne(got), y, R.rounded_bound(y, e), ("f8 bf16", K, order), flips_ref=y)
        for epi in (8, 9):
            act = R.act(epi, got)
            inv = 16.0
            want = e4m3_decode(e4m3_encode(act * inv)) / inv
            dev = e4m3_decode(e4m3_encode(act.astype(np.float32).astype(np.float64) * inv)) / inv
            assert (np.abs(dev - want) <= R.e4m3_step(want, inv)).all() and np.mean(dev != want) <= 0.02
            inv = R.clamp_scale(act, 0.1)
            over = np.abs(act * inv) > 448.0
            assert 0.05 < over.mean() < 0.5
            codes = e4m3_encode(act * inv)
            assert ((codes[over] & 0x7f) == 0x7e).all() and not ((codes & 0x7f) == 0x7f).any()


@pytest.mark.parametrize("D", R.LN_CANON + R.LN_OTHER)
@pytest.mark.parametrize("eps", R.LN_EPS)
def test_layernorm_fp32_emulation_meets_the_bounds(D, eps):
    for rows in R.LN_ROWS:
        for first in ((0, 1, 2) if rows < 3 else (0,)):
            q = R.ln_inputs(rows, D, rows * 7 + first, first)
            ref, bound = R.ln_rows(q, eps)
            ok = R.decided(ref, bound)
            rn = np.array([k == "randn" for k in R.row_kinds(rows, first)])
            if rn.any():
                assert ok[rn].mean() > 0.95, (rows, D, eps)              # the flip share is counted on nearly every ordinary element
            for order in ("seq", "pair"):
                got = R.ln_fp32(q["x"], q["g"], q["b"], eps, order)
                _within(got, ref, bound, ("ln", rows, D, eps, order))
                if ok.any():
                    _within(bf16_rne(got), ref, R.rounded_bound(ref, bound), ("ln bf16", rows, D, eps, order), flips_ref=ref, mask=ok)


@pytest.mark.parametrize("M,N,K,post,with_resid", [c for c in R.GEMM_LN_CASES if c[0] == 256 or c[2] == 192])
def test_gemm_ln_fp32_emulation_meets_the_bounds(M, N, K, post, with_resid):
    q = R.gemm_ln_inputs(M, N, K, with_resid, M + N + K)
    x, e, ln, bound = R.gemm_ln(q)
    for order in ("seq", "pair"):
        x32 = R.gemm_fp32(q["A"], q["W"], q["bias"], q["resid"], order)
        _within(x32, x, e, ("x", order))
        got = R.ln_fp32(x32, q["g"], q["b"], R.GEMM_LN_EPS, order)
        _within(got, ln, bound, ("ln(x)", order))
        _within(bf16_rne(got), ln, R.rounded_bound(ln, bound), ("ln(x) bf16", order), flips_ref=ln)


@pytest.mark.parametrize("G,H,S", R.attn_cases())
def test_attn_fp32_emulation_meets_the_bounds(G, H, S):
    for kind in R.ATTN_KINDS:
        qkv = R.attn_inputs(G, S, H, kind, S + G)
        ctx, ctxp, bound = R.attn_full(qkv, G, S, H)
        assert R.attn_full.second_share < 0.01, (S, kind, R.attn_full.second_share)        # the second-order remainder
        for order in ("tiles", "whole"):
            got = R.attn_fp32(qkv, G, S, H, order)
            _within(got, ctx, bound, ("attn", G, H, S, kind, order), flips_ref=ctxp if order == "tiles" else None)
