"""The image-path kernels on the MI355X at the shapes that reach each of their branches, run alone through the existing debug hooks
(gitcap_dbg_gemm, _gemm_f8, _gemm_ln, _attn_full, _layernorm), against the fp64 restatements and derived bounds of
tests/image_kernels_reference.py.  Every output lies in a poisoned buffer whose surroundings must stay poison.
tests/test_image_kernels.py runs the same generators through fp32 emulations on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import image_kernels_reference as R
from gpu_support import NAN, assert_tail, close_to_fp64, f64, lib, poisoned, ptr, same_bits, stream, to_dev  # noqa: F401
from text_rows_reference import e4m3_decode, e4m3_encode, flip_share

pytestmark = pytest.mark.gpu

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
TAIL = 64


def _at(t, elems):
    """the address `elems` elements into tensor t"""
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def _flips(dev, ref, what):
    share = flip_share(dev, ref)
    print(f"{what}: share off the correctly rounded value {share:.4f}")
    assert share <= 0.02, what


# ---- tile GEMMs -----------------------------------------------------------------------------------------------------------------

def _gemm(lib, q, d, M, N, K, epi, tile):
    dt = F32 if epi in (3, 4) else BF
    out = poisoned(M * N + TAIL, NAN, dt)
    rc = lib.gitcap_dbg_gemm(ptr(d["A"]), ptr(d["W"]), ptr(d["bias"]), ptr(d["resid"]) if epi == 3 else None, ptr(out), M, N, K, epi, tile, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert_tail(out, M * N, NAN)
    return f64(out[:M * N]).reshape(M, N)


@pytest.mark.parametrize("K", R.GEMM_KS)
@pytest.mark.parametrize("tile,M,N", R.GEMM_SHAPES)
def test_gemm_edge_depths_vs_fp64(lib, tile, M, N, K):
    """K = 64 .. 320: one, two, three (odd; fewer than the 64-tile ring holds) and five K steps, one tile and two.
    GELU epilogues (K = 192): against act64 of the device's own epi-4 output, half a bf16 ulp + EPS_ACT |pre|.  Measured on an
    MI355X: largest excess over the half ulp 8.282e-09 |pre| (quick_gelu) and 7.713e-08 |pre| (erf_gelu); EPS_ACT = 2 x 7.713e-08
    (image_kernels_reference.py, docs/LAB_NOTEBOOK.md).  The share off the correctly rounded value is counted where that error
    is below a sixteenth of the output's ulp (not in erf_gelu's far negative tail, where the output vanishes and the error does not)."""
    q = R.gemm_inputs(M, N, K, M + N + K)
    d = dict(A=to_dev(q["A"], BF), W=to_dev(q["W"], BF), bias=to_dev(q["bias"], F32), resid=to_dev(q["resid"], F32))
    what = f"gemm tile={tile} M={M} N={N} K={K}"
    y, e = R.gemm(q["A"], q["W"], q["bias"])
    pre = _gemm(lib, q, d, M, N, K, 4, tile)
    close_to_fp64(pre, y, e, what + " epi 4", flips=False)
    yr, er = R.gemm(q["A"], q["W"], q["bias"], q["resid"])
    close_to_fp64(_gemm(lib, q, d, M, N, K, 3, tile), yr, er, what + " epi 3", flips=False)
    close_to_fp64(_gemm(lib, q, d, M, N, K, 0, tile), y, R.rounded_bound(y, e), what + " epi 0")
    if K == R.GEMM_ACT_K:
        for epi in (1, 2):
            out = R.act(epi, pre)
            got = _gemm(lib, q, d, M, N, K, epi, tile)
            bound, ok = R.act_bound_bf16(pre, out)
            close_to_fp64(got, out, bound, what + f" epi {epi}", flips=False)
            assert ok.mean() > 0.6
            _flips(got[ok], out[ok], what + f" epi {epi}")


# ---- fp8 tile GEMM --------------------------------------------------------------------------------------------------------------

def _gemm_f8(lib, d, M, N, K, epi, inv):
    dt = {4: F32, 0: BF}.get(epi, U8)
    out = poisoned(M * N + TAIL, NAN if dt != U8 else 0x55, dt)
    rc = lib.gitcap_dbg_gemm_f8(ptr(d["Ac"]), ptr(d["Wc"]), ptr(d["wscale"]), R.F8_ASCALE, ptr(d["bias"]), ptr(out), M, N, K, epi, inv, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert_tail(out, M * N, NAN if dt != U8 else 0x55)
    return out[:M * N].view(M, N)


@pytest.mark.parametrize("K", R.F8_KS)
def test_gemm_f8_edge_depths_and_clamp_vs_fp64(lib, K):
    """One, two and three 128-deep steps; epi 4 / 0 against the fp64 product of the dequantised operands; the e4m3 GELU epilogues
    against act64 of the device's epi-4 output (one e4m3 step + EPS_ACT |pre|, at most 2 % off the nearest code), once in range
    and once with out8_inv so large that a known share of the outputs lies beyond 448: those must be the codes 0x7e / 0xfe of
    their sign, and no NaN code (0x7f / 0xff) may appear anywhere.
    The bound carries the truncation of the e4m3 matrix instruction (image_kernels_reference.f8_truncation): without it K = 128,
    epi 4 stood at 1.140 of gamma(2 (K + 3)) (|A| |W|^T + |bias|) -- element (108, 31) off by exactly 2^-12 -- with errors of the
    same size at K = 256 and 384, while the bf16 tile kernels use 1.5 % of the same fp32 bound."""
    M = N = 256
    q = R.gemm_f8_inputs(M, N, K, K)
    d = dict(Ac=to_dev(q["Ac"], U8), Wc=to_dev(q["Wc"], U8), wscale=to_dev(q["wscale"], F32), bias=to_dev(q["bias"], F32))
    y, e = R.gemm_f8(q["A"], q["W"], q["bias"])
    pre = f64(_gemm_f8(lib, d, M, N, K, 4, 0.0))
    e32 = R.gemm(q["A"], q["W"], q["bias"])[1]
    print(f"gemm_f8 K={K} epi 4: max |device - fp64| / the fp32 accumulation term alone = {float((np.abs(pre - y) / e32).max()):.3f}, "
          f"max |device - truncation model| / that term = {float((np.abs(pre - R.gemm_f8_model(q['A'], q['W'], q['bias'])) / e32).max()):.3f}")
    close_to_fp64(pre, y, e, f"gemm_f8 K={K} epi 4", flips=False)
    close_to_fp64(f64(_gemm_f8(lib, d, M, N, K, 0, 0.0)), y, R.rounded_bound(y, e), f"gemm_f8 K={K} epi 0")
    for epi in (8, 9):
        out = R.act(epi, pre)
        for inv, clamped in ((16.0, False), (R.clamp_scale(out, 0.1), True)):
            codes = _gemm_f8(lib, d, M, N, K, epi, inv).cpu().numpy()
            assert not ((codes & 0x7f) == 0x7f).any(), "a NaN code in the output"
            got, want = e4m3_decode(codes) / inv, e4m3_decode(e4m3_encode(out * inv)) / inv
            ratio = float((np.abs(got - want) / (R.e4m3_step(want, inv) + R.EPS_ACT * np.abs(pre))).max())
            share = float(np.mean(got != want))
            over = np.abs(out * inv) > 448.0 * (1 + 2.0 ** -20)
            print(f"gemm_f8 K={K} epi {epi} out8_inv={inv}: max |device - nearest code| / step = {ratio:.3f}, share off it {share:.4f}, "
                  f"share beyond 448: {over.mean():.4f}")
            assert ratio <= 1.0 and share <= 0.02
            assert (0.05 < over.mean() < 0.5) if clamped else over.mean() < 0.01
            assert np.array_equal(codes[over], np.where(out[over] < 0, 0xfe, 0x7e).astype(np.uint8))


# ---- GEMM + LayerNorm -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K,post,with_resid", R.GEMM_LN_CASES)
def test_gemm_layernorm_edge_rows_vs_fp64(lib, M, N, K, post, with_resid):
    """The fused epilogue and GEMM (each tile) + row kernel, launched twice each: bitwise equal, and LN(A W^T + bias + resid) within
    ln_bound carrying the GEMM's error, on n(0, 1) rows, a row of mean 1e3 and deviation 1e-2 (the (mean, M2) segment merge) and an
    exactly constant row.  post = 0: out_f32 = x within the GEMM bound."""
    q = R.gemm_ln_inputs(M, N, K, with_resid, M + N + K)
    A, W, bias, resid = to_dev(q["A"], BF), to_dev(q["W"], BF), to_dev(q["bias"], F32), to_dev(q["resid"], F32)
    g, b = to_dev(q["g"], F32), to_dev(q["b"], F32)
    outs = []
    for fused, tile in ((1, 256), (0, 256), (0, 128), (0, 64)):
        of, ob = poisoned(M * N + TAIL, NAN), poisoned(M * N + TAIL, NAN, BF)
        for _ in range(2):
            rc = lib.gitcap_dbg_gemm_ln(ptr(A), ptr(W), ptr(bias), ptr(resid), ptr(g), ptr(b), ctypes.c_float(R.GEMM_LN_EPS), ptr(of), ptr(ob),
                                        M, N, K, post, fused, tile, stream())
            torch.cuda.synchronize()
            assert rc == 0
        assert_tail(of, M * N, NAN)
        assert_tail(ob, M * N, NAN)
        outs.append((of, ob))
    for of, ob in outs[1:]:
        assert same_bits(outs[0][0], of) and same_bits(outs[0][1], ob)
    x, e, ln, bound = R.gemm_ln(q)
    of, ob = (f64(t[:M * N]).reshape(M, N) for t in outs[0])
    what = f"gemm_ln M={M} N={N} K={K} post={post} resid={with_resid}"
    if post:
        close_to_fp64(of, ln, bound, what + " out_f32 = LN(x)", flips=False)
    else:
        close_to_fp64(of, x, e, what + " out_f32 = x", flips=False)
    close_to_fp64(ob, ln, R.rounded_bound(ln, bound), what + " bf16")
    if with_resid:
        assert np.array_equal(ob[R.GEMM_LN_CONST_ROW], f64(b.bfloat16()))          # a constant row is beta, exactly


# ---- row LayerNorm --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("D", R.LN_CANON + R.LN_OTHER)
def test_layernorm_edge_rows_and_widths_vs_fp64(lib, D, eps):
    """Every canonical width and three on the two-pass path (100, 260, 1020), 1 .. 9 rows (4 per workgroup), the three row kinds.
    The bf16 output is the rounding of the fp32 output bit for bit; its share off the correctly rounded reference is counted where
    the fp32 bound decides the rounding (image_kernels_reference.decided)."""
    for rows in R.LN_ROWS:
        for first in ((0, 1, 2) if rows < 3 else (0,)):
            q = R.ln_inputs(rows, D, rows * 7 + first, first)
            x, g, b = to_dev(q["x"], F32), to_dev(q["g"], F32), to_dev(q["b"], F32)
            of, ob = poisoned(rows * D + TAIL, NAN), poisoned(rows * D + TAIL, NAN, BF)
            rc = lib.gitcap_dbg_layernorm(ptr(x), ptr(g), ptr(b), ctypes.c_float(eps), rows, D, ptr(of), ptr(ob), stream())
            torch.cuda.synchronize()
            assert rc == 0
            assert_tail(of, rows * D, NAN)
            assert_tail(ob, rows * D, NAN)
            assert same_bits(ob[:rows * D], of[:rows * D].bfloat16())
            ref, bound = R.ln_rows(q, eps)
            what = f"layernorm rows={rows} D={D} eps={eps} first kind {R.ROW_KINDS[first]}"
            got, gotb = f64(of[:rows * D]).reshape(rows, D), f64(ob[:rows * D]).reshape(rows, D)
            close_to_fp64(got, ref, bound, what, flips=False)
            close_to_fp64(gotb, ref, R.rounded_bound(ref, bound), what + " bf16", flips=False)
            ok = R.decided(ref, bound)
            if ok.any():
                _flips(gotb[ok], ref[ok], what + " bf16")


@pytest.mark.parametrize("D", R.LN_REFUSED)
def test_layernorm_refuses_other_widths(lib, D):
    """launch_layernorm returns hipErrorInvalidValue before any launch: the hook's GITCAP_ERR_HIP (-3), and nothing is written."""
    x, g = poisoned(4 * 1032, NAN), poisoned(1032, NAN)
    of = poisoned(4 * 1032, NAN)
    assert lib.gitcap_dbg_layernorm(ptr(x), ptr(g), ptr(g), ctypes.c_float(1e-5), 4, D, ptr(of), None, stream()) == -3
    torch.cuda.synchronize()
    assert_tail(of, 0, NAN)


# ---- attn_full ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,H,S", R.attn_cases())
def test_attn_full_tile_edges_vs_fp64(lib, G, H, S):
    """Every form of the ragged last key tile (S % 64 in 1..32: the half form; 33..63: the masked full form, behind no, one and
    several full tiles), S a multiple of the 128 queries of a workgroup and one past it, S = 1; both maps of the workgroup id.
    The G S rows lie inside a NaN-poisoned qkv (the kernel must read no other row) and a NaN-poisoned ctx with guard rows.
    The flip share is counted against the reference with P rounded to bf16 where the kernel rounds it (attn_full's docstring)."""
    W, pad = 64 * H, 3
    for kind in R.ATTN_KINDS:
        qkv = R.attn_inputs(G, S, H, kind, S + G)
        big = poisoned((G * S + 2 * pad, 3 * W), NAN, BF)
        big[pad:pad + G * S] = to_dev(qkv, BF)
        ctx = poisoned((G * S + 2 * pad, W), NAN, BF)
        rc = lib.gitcap_dbg_attn_full(_at(big, pad * 3 * W), _at(ctx, pad * W), G, S, H, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert bool(torch.isnan(ctx[:pad].float()).all()) and bool(torch.isnan(ctx[pad + G * S:].float()).all()), "a row outside was written"
        assert bool(torch.isfinite(ctx[pad:pad + G * S].float()).all())
        ref, refp, bound = R.attn_full(qkv, G, S, H)
        got = f64(ctx[pad:pad + G * S])
        what = f"attn_full G={G} H={H} S={S} {kind}"
        close_to_fp64(got, ref, bound, what, flips=False)
        _flips(got, refp, what)
