"""Plain fp64 statements of the image-path kernels (tile GEMMs of gemm.hip / gemm256.hip and their epilogues, the residual +
LayerNorm epilogue, attn_full, the row LayerNorm), the per-element error bounds that go with them and the input generators of
tests/test_image_kernels_gpu.py (run on the CPU, with fp32 emulations of the same operations, by tests/test_image_kernels.py).

Nothing here imports the oracle or the library.  Operands are float64 arrays that hold bf16, fp32 or e4m3 x 2^k values exactly.
The number formats, gamma, layernorm, ln_bound and flip_share are those of text_rows_reference.py.

Bounds.  u = 2^-24 (fp32, round to nearest).  A bf16 value has 8 significant bits.

GEMM, fp32 outputs (epi 3, 4):  y = A W^T + bias (+ resid).  A product of two bf16 (or two e4m3) values is exact in fp32, so the
  error is that of K fp32 additions in an order the matrix core does not document, plus the adds of the epilogue (bias, resid).
  The rounding of the MFMA accumulator is not documented either: it is taken as 2^-23 per operation (truncation's worst case)
  instead of gamma's 2^-24, which is gamma(2 n) exactly:
      e_gemm = gamma(2 (K + 3)) (|A| |W|^T + |bias| + |resid|)                                                      (gemm)
GEMM, bf16 output (epi 0):  the device rounds y + d, |d| <= e_gemm, to bf16: |bf16(y + d) - y| <= e_gemm + half a bf16 ulp of
  y + d, and ulp(y + d) <= ulp(|y| + e_gemm):  e_gemm + bf16_ulp(|y| + e_gemm) / 2  (= half an ulp of y wherever e_gemm does not
  reach the next binade).                                                                                     (rounded_bound)
GELU epilogues (bf16 epi 1, 2; e4m3 epi 8, 9):  v_exp_f32 / v_rcp_f32 have no error statement in the sources, so the activation is
  checked from the DEVICE's fp32 pre-activation (an epi-4 launch on the same operands): |out - act64(pre)| <= half a bf16 ulp
  (one e4m3 step) + EPS_ACT |pre|, EPS_ACT measured once on an MI355X (below).                                   (act_bound)
fp8 GEMM:  operands are code x scale exactly (powers of two), the accumulator is scaled exactly: the bound above on the
  dequantised values -- plus what v_mfma_scale_f32_16x16x128_f8f6f4 loses before it accumulates, which is not an fp32 sum of exact
  products (gemm_f8, F8_KEEP_BITS).
Row LayerNorm / GEMM + LayerNorm:  ln_bound (text_rows_reference.py) with the counts of these kernels, see ln_rows / gemm_ln.
attn_full:  see attn_full below.
"""
from __future__ import annotations

import math

import numpy as np

from text_rows_reference import (U32, bf16_rne, bf16_ulp, e4m3_decode, e4m3_encode, flip_share, gamma, gelu, layernorm, ln_bound,
                                 quick_gelu)

__all__ = ["flip_share"]

f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)          # noqa: E731  (the fp32 values of a, as fp64)


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------

def gamma_mfma(n):
    """n accumulator operations at 2^-23 each (module docstring)."""
    return gamma(2 * n)


def rounded_bound(y, e):
    """|bf16(y + d) - y| for |d| <= e."""
    return e + 0.5 * bf16_ulp(np.abs(y) + e)


def gemm(A, W, bias, resid=None):
    """y = A W^T + bias (+ resid) and e_gemm (fp32 outputs; rounded_bound(y, e) for the bf16 output)."""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    K = A.shape[1]
    y = A @ W.T + bias + (0.0 if resid is None else resid)
    mag = np.abs(A) @ np.abs(W).T + np.abs(bias) + (0.0 if resid is None else np.abs(resid))
    return y, gamma_mfma(K + 3) * mag


ACT = {1: quick_gelu, 2: gelu, 8: quick_gelu, 9: gelu}


def act(epi, x):
    with np.errstate(over="ignore"):            # quick_gelu far below zero: x / (1 + inf) = -0
        return ACT[epi](np.asarray(x, np.float64))

# The activation term.  Measured on an MI355X over GEMM_SHAPES at K = GEMM_ACT_K, 258048 values per epilogue (docs/LAB_NOTEBOOK.md,
# "fp64 edge-shape tests of the image-path kernels"): the largest (|device - act64(pre)| - half a bf16 ulp of the reference) / |pre|
# was 8.282e-09 for quick_gelu and 7.713e-08 for erf_gelu (common.h: its erf is off by up to 1.5e-7, times |pre| / 2).  An excess
# shows only where the reference sits within the activation's error of a rounding boundary, so the observed maximum undershoots the
# true one: the constant is 2 x the larger measurement.
EPS_ACT_MEASURED = 7.713e-08
EPS_ACT = 2 * EPS_ACT_MEASURED


def act_bound_bf16(pre, out):
    """-> (bound on |device_bf16 - act64(pre)|, the elements whose rounding the activation decides).  The error EPS_ACT |pre| is
    absolute in the output: far below zero, where erf_gelu(x) -> -0 faster than |x| 1.5e-7, it exceeds the output's bf16 ulp and
    'the correctly rounded value' is not a property the kernel's erf can have; the flip share is counted on `decided` only."""
    e = EPS_ACT * np.abs(pre)
    return rounded_bound(out, e), decided(out, e)


def e4m3_step(want, out8_inv):
    """One e4m3 step at `want` (a decoded value / out8_inv), as tests/test_kernels_gpu.py takes it: an eighth of the value, at
    least the spacing of the smallest normals."""
    return np.maximum(np.abs(want) * 2.0 ** -3, 2.0 ** -6 / out8_inv)


def gemm_inputs(M, N, K, seed):
    """A [M][K] and W [N][K] as bf16 values, bias [N] and resid [M][N] as fp32 values.  A row m carries the offset 0.25 ((m % 7) - 3),
    W column n the ramp ((n % 11) - 5) / (10 sqrt K) (1 + (k % 5) / 4): a swapped or shifted fragment changes the product.  Row 1
    of A is 64 + n(0, 1) (a large common value whose products cancel in the sum), row 2 is zero."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)) + 0.25 * ((np.arange(M) % 7) - 3)[:, None]
    W = rng.standard_normal((N, K)) / math.sqrt(K)
    W += ((np.arange(N) % 11) - 5)[:, None] / (10 * math.sqrt(K)) * (1 + (np.arange(K) % 5) / 4)[None, :]
    A[1] = 64.0 + rng.standard_normal(K)
    A[2] = 0.0
    bias = f32(np.linspace(-1.5, 1.5, N) + 0.25 * rng.standard_normal(N))
    resid = f32(rng.standard_normal((M, N)) * 2 + 0.5)
    return dict(A=bf16_rne(A), W=bf16_rne(W), bias=bias, resid=resid)


GEMM_SHAPES = [(tile, mult * tile, tile) for tile in (64, 128, 256) for mult in (1, 2)]        # (tile, M, N)
GEMM_KS = (64, 128, 192, 320)       # K steps of 64: 1 (no pipeline), 2, 3 (odd, < the 64-tile ring's depth beyond its prologue), 5
GEMM_ACT_K = 192


def gemm_fp32(A, W, bias, resid, order):
    """The same operation in numpy fp32.  order 'seq': one k after the other; 'pair': 32-wide partial sums added in a binary tree."""
    A32, W32 = np.asarray(A, np.float32), np.asarray(W, np.float32)
    K = A32.shape[1]
    if order == "seq":
        acc = np.zeros((A32.shape[0], W32.shape[0]), np.float32)
        for k in range(K):
            acc = acc + A32[:, k, None] * W32[None, :, k]
    else:
        parts = [A32[:, k0:k0 + 32] @ W32[:, k0:k0 + 32].T for k0 in range(0, K, 32)]
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        acc = parts[0]
    y = acc + np.asarray(bias, np.float32)
    if resid is not None:
        y = y + np.asarray(resid, np.float32)
    return y.astype(np.float64)


# ---- fp8 GEMM -------------------------------------------------------------------------------------------------------------------

F8_KS = (128, 256, 384)             # K steps of 128: 1, 2, 3
F8_ASCALE = 1.0 / 16.0


def gemm_f8_inputs(M, N, K, seed):
    """e4m3 codes of A (scale 1/16) and of W (a power of two per row), the values they stand for, bias [N]."""
    rng = np.random.default_rng(seed)
    a = np.clip(rng.standard_normal((M, K)) * 1.5 + 0.25 * ((np.arange(M) % 7) - 3)[:, None], -27, 27)
    a[1] = 16.0 + rng.standard_normal(K)
    a[2] = 0.0
    w = rng.standard_normal((N, K)) / math.sqrt(K) + ((np.arange(N) % 11) - 5)[:, None] / (10 * math.sqrt(K))
    wscale = np.exp2(np.ceil(np.log2(np.abs(w).max(axis=1) / 448.0)))
    Ac, Wc = e4m3_encode(a / F8_ASCALE), e4m3_encode(w / wscale[:, None])
    bias = f32(np.linspace(-1, 1, N) + 0.1 * rng.standard_normal(N))
    return dict(Ac=Ac, Wc=Wc, wscale=wscale, A=e4m3_decode(Ac) * F8_ASCALE, W=e4m3_decode(Wc) * wscale[:, None], bias=bias)


# What one v_mfma_scale_f32_16x16x128_f8f6f4 does with its 128 e4m3 products, probed on an MI355X through gitcap_dbg_gemm_f8 at K = 128
# (one instruction per output; W = 1, rows of A with one large value and small ones, docs/LAB_NOTEBOOK.md has the table): the
# products of 8 consecutive k (8 bytes of a lane's operand) are aligned to the exponent E of the largest of them and cut off --
# towards zero, before any sum, also where the large ones cancel -- below 2^(E - 13): beside 256 = 2^8 a product 2^-5 survives and
# 2^-6 vanishes, 1.75 2^-4 arrives as 1.5 2^-4, in every position of the group, at either sign, with the products scaled by 2^-6 as
# well.  Products of other groups, the groups' sums and the accumulator are not affected (exact in every probe).
F8_GROUP, F8_KEEP_BITS = 8, 13


def f8_truncation(A, W):
    """sum over the groups of 8 k of what each product may lose: nothing if it is a multiple of 2^(E - 13), E the exponent of the
    group's largest |a_k w_k| (the instruction's E is at most that, so its grid is that or finer), otherwise less than that
    spacing and no more than the product itself.  All losses point towards zero, so their sum bounds their effect."""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    out = np.zeros((A.shape[0], W.shape[0]))
    for k0 in range(0, A.shape[1], F8_GROUP):
        P = np.abs(A[:, None, k0:k0 + F8_GROUP] * W[None, :, k0:k0 + F8_GROUP])
        mx = P.max(axis=-1, keepdims=True)
        _, ex = np.frexp(np.where(mx > 0, mx, 1.0))
        grid = np.ldexp(1.0, ex - 1 - F8_KEEP_BITS)
        q = P / grid
        out += np.where(q == np.rint(q), 0.0, np.minimum(P, grid)).sum(axis=-1)
    return out


def gemm_f8(A, W, bias):
    """The fp8 tile GEMM on the dequantised operands: y, and e_gemm + the instruction's truncation."""
    y, e = gemm(A, W, bias)
    return y, e + f8_truncation(A, W)


def gemm_f8_model(A, W, bias):
    """The probed arithmetic itself, in fp64: every product cut to its group's grid (E from the largest product), then summed."""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    acc = np.zeros((A.shape[0], W.shape[0]))
    for k0 in range(0, A.shape[1], F8_GROUP):
        P = A[:, None, k0:k0 + F8_GROUP] * W[None, :, k0:k0 + F8_GROUP]
        mx = np.abs(P).max(axis=-1, keepdims=True)
        _, ex = np.frexp(np.where(mx > 0, mx, 1.0))
        grid = np.ldexp(1.0, ex - 1 - F8_KEEP_BITS)
        acc += (np.trunc(P / grid) * grid).sum(axis=-1)
    return acc + bias


def clamp_scale(act, share):
    """A power-of-two out8_inv under which about `share` of |act| x out8_inv lies beyond 448."""
    q = np.quantile(np.abs(act), 1.0 - share)
    return float(np.exp2(np.ceil(np.log2(448.0 / q))))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------

LN_CANON = (64, 128, 256, 512, 768, 1024)
LN_OTHER = (100, 260, 1020)          # launch_layernorm takes D % 4 == 0, D <= 1024: below one 256-column slice, 4 past it, the largest
LN_REFUSED = (770, 1028)             # not a multiple of 4; above 1024
LN_ROWS = (1, 3, 4, 5, 9)            # 4 rows per workgroup
LN_EPS = (1e-5, 1e-12)
ROW_KINDS = ("randn", "hard", "const")


def ln_sum_depth(D):
    """The number of roundings on the way to the row mean (ln_bound's sum_depth).  Canonical widths (ln_canon.h): 2 adds of the
    lane's 4 values, 4 tree steps, x 1/64, then D / 64 - 1 merges of two roundings each (d = mean_s - mu, the fma).  Other widths
    (layernorm_kernel): 4 adds per 256-column slice in the lane, 6 butterfly steps, the division."""
    if D in LN_CANON:
        return 7 + 2 * (D // 64 - 1)
    return 4 * ((D + 255) // 256) + 7


def ln_rows_bound(slab_terms, tail_terms, g, b, eps, D, depth=None):
    """ln_bound with this kernel's counts.  The canonical form does not centre the row on its mean: M2 = ||r||^2 with r the D
    deviations from the SEGMENT means and the D / 64 - 1 between-segment steps sqrt(n_a 64 / n) (mean_s - mu) (Chan's update, an
    identity in exact arithmetic).  Each entry is off by at most dx (ln_bound's error of a centred value) times its weight, the
    weights squared sum to < 2 D, so sqrt(M2) is off by at most sqrt(2 D) max(dx): sqrt 2 x the relative error ln_bound gives rstd.
    The difference, (sqrt 2 - 1) max(dx) / sigma on |x - mu| / sigma |g|, is added."""
    sd = ln_sum_depth(D)
    bound = ln_bound(slab_terms, tail_terms, g, b, eps, depth=depth, sum_depth=sd)
    if D in LN_CANON:
        terms = list(slab_terms) + list(tail_terms)
        x = sum(np.asarray(t, np.float64) for t in terms)
        dep = 3 + (len(slab_terms) + 7) // 8 if depth is None else depth
        e_in = U32 * sum(np.abs(t) for t in tail_terms) + U32 * np.abs(x) + dep * U32 * sum([np.abs(t) for t in slab_terms], 0 * x)
        mu = x.mean(axis=-1, keepdims=True)
        sig = np.sqrt(((x - mu) ** 2).mean(axis=-1, keepdims=True) + eps)
        dx = e_in + sd * U32 * np.abs(x).mean(axis=-1, keepdims=True) + e_in.mean(axis=-1, keepdims=True) + U32 * np.abs(x - mu)
        bound = bound + (math.sqrt(2) - 1) * dx.max(axis=-1, keepdims=True) / sig * np.abs(x - mu) / sig * np.abs(g)
    return bound


def row_kinds(rows, first=0):
    return [ROW_KINDS[(r + first) % 3] for r in range(rows)]


def ln_inputs(rows, D, seed, first=0):
    """x [rows][D] fp32 values: row r is of kind (r + first) % 3 -- n(1, 3); 1e3 + 1e-2 n(0, 1) (a large mean over a small variance);
    the constant 0.75.  gamma / beta depend on the column."""
    rng = np.random.default_rng(seed)
    x = np.empty((rows, D))
    for r, kind in enumerate(row_kinds(rows, first)):
        x[r] = {"randn": rng.standard_normal(D) * 3 + 1, "hard": 1e3 + 1e-2 * rng.standard_normal(D), "const": np.full(D, 0.75)}[kind]
    n = np.arange(D)
    return dict(x=f32(x), g=f32(1.0 + 0.5 * np.sin(n)), b=f32(0.3 * np.cos(n * 0.7)))


def ln_rows(q, eps):
    """LayerNorm of exact fp32 rows and its bound (the row is ln_bound's one tail term)."""
    D = q["x"].shape[1]
    return layernorm(q["x"], q["g"], q["b"], eps), ln_rows_bound([], [q["x"]], q["g"], q["b"], eps, D)


def decided(ref, e):
    """Elements whose bf16 rounding the fp32 arithmetic decides: the bound in front of the rounding is below a sixteenth of a bf16
    ulp.  Elsewhere (the large-mean row, a constant row under eps = 1e-12) 'the correctly rounded value' is not a property an fp32
    LayerNorm can have, and only the bound is asserted."""
    return e <= bf16_ulp(ref) / 16


def ln_fp32(x, g, b, eps, order):
    """numpy fp32: 'seq' two-pass with sequential sums; 'pair' two-pass with numpy's pairwise sums."""
    x32, g32, b32 = (np.asarray(t, np.float32) for t in (x, g, b))
    D = x32.shape[1]
    if order == "seq":
        s = np.zeros(x32.shape[0], np.float32)
        for c in range(D):
            s = s + x32[:, c]
        mean = (s / np.float32(D))[:, None]
        d = x32 - mean
        v = np.zeros(x32.shape[0], np.float32)
        for c in range(D):
            v = v + d[:, c] * d[:, c]
        var = (v / np.float32(D))[:, None]
    else:
        mean = x32.mean(axis=1, keepdims=True, dtype=np.float32)
        d = x32 - mean
        var = (d * d).mean(axis=1, keepdims=True, dtype=np.float32)
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps))
    return (d * rstd * g32 + b32).astype(np.float64)


# ---- GEMM + LayerNorm -----------------------------------------------------------------------------------------------------------

GEMM_LN_CASES = [(M, N, K, post, with_resid) for M in (256, 512) for N in (768, 1024) for K in (64, 192)
                 for post, with_resid in ((0, True), (1, True), (1, False))]
GEMM_LN_HARD_ROW, GEMM_LN_CONST_ROW = 5, 9
GEMM_LN_EPS = 1e-5


def gemm_ln_inputs(M, N, K, with_resid, seed):
    """n(0, 1) rows; with a residual, row 5 of x is 1e3 + 1e-2 n(0, 1), built through resid (the GEMM part stays ordinary), and row 9
    is exactly constant: a zero row of A, a zero row of resid, and the bias is the constant 0.75 for the whole launch."""
    rng = np.random.default_rng(seed)
    A = bf16_rne(rng.standard_normal((M, K)) + 0.25 * ((np.arange(M) % 7) - 3)[:, None])
    W = bf16_rne(rng.standard_normal((N, K)) / math.sqrt(K))
    A[GEMM_LN_CONST_ROW] = 0.0
    bias = np.full(N, 0.75)
    resid = None
    if with_resid:
        resid = rng.standard_normal((M, N)) * 2 + 0.5
        resid[GEMM_LN_HARD_ROW] = 1e3 + 1e-2 * rng.standard_normal(N) - (A[GEMM_LN_HARD_ROW] @ W.T + bias)
        resid[GEMM_LN_CONST_ROW] = 0.0
        resid = f32(resid)
    n = np.arange(N)
    return dict(A=A, W=W, bias=bias, resid=resid, g=f32(1.0 + 0.5 * np.sin(n)), b=f32(0.3 * np.cos(n * 0.7)))


def gemm_ln(q):
    """x = A W^T + bias (+ resid), e_gemm, LN(x) and its bound.  The row that enters the LayerNorm carries the GEMM's error: the
    products are passed to ln_bound as two slab terms, the sum P of the positive and -N of the negative ones (P - N = A W^T and
    P + N = |A| |W|^T), with depth gamma_mfma(K + 3) / u, and bias / resid as its tail terms: its input error is then
    gamma_mfma(K + 3) |A| |W|^T + u (|bias| + |resid|) + u |x|, which covers the accumulator and both adds of the epilogue."""
    A, W, bias, resid = q["A"], q["W"], q["bias"], q["resid"]
    K, N = A.shape[1], W.shape[0]
    x, e_gemm = gemm(A, W, bias, resid)
    Ap, An, Wp, Wn = np.maximum(A, 0), np.maximum(-A, 0), np.maximum(W, 0), np.maximum(-W, 0)
    P, Nn = Ap @ Wp.T + An @ Wn.T, Ap @ Wn.T + An @ Wp.T
    tail = [np.broadcast_to(bias, x.shape)] + ([resid] if resid is not None else [])
    bound = ln_rows_bound([P, -Nn], tail, q["g"], q["b"], GEMM_LN_EPS, N, depth=gamma_mfma(K + 3) / U32)
    return x, e_gemm, layernorm(x, q["g"], q["b"], GEMM_LN_EPS), bound


# ---- attn_full ------------------------------------------------------------------------------------------------------------------

ATTN_S = (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 191, 255, 256, 289)
ATTN_GH = ((1, 1), (4, 2))           # H G % 8 == 0: the XCD remap of the workgroup id
ATTN_GH_OTHER = (1, 3)               # the plain map with more than one head
ATTN_S_OTHER = (33, 129, 191)
ATTN_KINDS = ("randn", "late", "mean")
EXP2_REL = 2.0 ** -22                # v_exp_f32: 1 ulp in the ISA manual, not restated in the sources; 2 ulp taken


def attn_inputs(G, S, H, kind, seed):
    """qkv [G S][3 W] bf16 values.  'randn': 1.5 n(0, 1).  'late': every query scores the LAST key of its group 8 above the
    others (about e^8 / (e^8 + S - 1) of the mass -- the others still count), that key's V is +-4 by column; for S % 64 in 33..63
    it lies in the second 32-key half of the ragged tile.  'mean': q = 0, every score equal, v_j[d] = j / S - d / 64: the context
    is the mean over the keys, near zero in the middle columns, so a dropped, duplicated or padded key moves it by far more than
    it is rounded."""
    rng = np.random.default_rng(seed)
    W = 64 * H
    x = rng.standard_normal((G, S, 3, H, 64)) * 1.5
    d = np.arange(64)
    if kind == "late":
        x[:, :, 0] = 0.5 + 0.1 * rng.standard_normal((G, S, H, 64))
        x[:, :, 1] = 0.1 * rng.standard_normal((G, S, H, 64))
        x[:, S - 1, 1] = 2.0
        x[:, S - 1, 2] = 4.0 * np.where((d[None, None, :] + np.arange(H)[None, :, None] + np.arange(G)[:, None, None]) % 3 == 0, -1.0, 1.0)
    elif kind == "mean":
        x[:, :, 0] = 0.0
        x[:, :, 2] = (np.arange(S)[None, :, None, None] / S - d / 64.0) * (1 + np.arange(H)[None, None, :, None])
    return bf16_rne(x.reshape(G * S, 3 * W))


def attn_full(qkv, G, S, H):
    """ctx = sum_j p_j v_j / sum_j p_j, p_j = exp(0.125 q . k_j - max) -> (ctx [G S][W], ctx_p, bound).

    What attention.hip does (attn_full_kernel): per 64-key tile, scores by MFMA (64 products), the tile's maximum joins the running
    maximum m_t, p'_j = exp2((s_j - m_t) c) in fp32; l_run sums the UNROUNDED fp32 p' (l = l alpha + psum), the P.V product takes
    p' ROUNDED to bf16 (v_cvt_pk_bf16_f32, nearest even) -- at the running maximum of the key's own tile; later tiles multiply O and l
    by alpha = exp2((m_old - m_new) c).  Only the numerator sees the bf16 rounding.  With A = sum p_j |v_j| / sum p_j, first order:
      P's rounding:   sum_j half_ulp_bf16(p'_j) exp(m_t - m) |v_j| / sum p.  (Between 2^-9 p_j at the top of a binade and 2^-8 p_j at
                      its bottom; taken per term at the value the kernel rounds.  Once: the denominator is not rounded.)
      scores:         |ds_j| <= gamma_mfma(64) sum_d |q_d| |k_jd|, a relative error 0.125 |ds_j| of p_j; the exponent's own arithmetic
                      (the constant c, m c, the fma: <= u 0.125 (2 |s - m| + |m|) <= 5 u 0.125 max|s|) and v_exp_f32 (EXP2_REL), once
                      for p' and once per later alpha: ntiles (5 u 0.125 max|s| + EXP2_REL).  A relative error eps_j of p_j in the
                      numerator and the denominator alike moves ctx by sum p_j eps_j (v_j - ctx) / sum p.
      accumulation:   O: S products and ntiles rescalings in the MFMA accumulator, gamma_mfma(S + ntiles) A; l: S + ntiles + 1
                      fp32 additions, gamma(S + ntiles + 1) |ctx|; 1 / l and the product: 3 u |ctx|.
      second order:   the product of any two of the relative errors above, (2^-8 + max eps_j + gamma_mfma(S + ntiles))^2 (A + |ctx|):
                      included (it is below 1 % of the bound on every input here, tests/test_image_kernels.py asserts it).
      output:         rounded_bound: half a bf16 ulp on top.
    ctx_p is the same sum with p' rounded to bf16 where the kernel rounds it (fp64 otherwise): the value 'correctly rounded' refers
    to for this kernel -- P enters P.V as bf16 by design -- and the one the flip share is counted against."""
    W = 64 * H
    x = np.asarray(qkv, np.float64).reshape(G, S, 3, H, 64)
    ctx, ctxp, bound, second = (np.empty((G, S, H, 64)) for _ in range(4))
    nt = (S + 63) // 64
    tile_of = np.arange(S) // 64
    for g in range(G):
        for h in range(H):
            q, k, v = x[g, :, 0, h], x[g, :, 1, h], x[g, :, 2, h]
            s = q @ k.T                                                                  # raw scores; the softmax takes s / 8
            smag = np.abs(q) @ np.abs(k).T
            run = np.maximum.accumulate(np.stack([s[:, tile_of == t].max(axis=1) for t in range(nt)], axis=1), axis=1)      # [S][nt]
            m = run[:, -1:]
            m_t = run[:, tile_of]                                                        # the running maximum at key j's tile
            p1 = np.exp(0.125 * (s - m_t))
            scale = np.exp(0.125 * (m_t - m))
            p = np.exp(0.125 * (s - m))
            den = p.sum(axis=1, keepdims=True)
            c = (p @ v) / den
            A = (p @ np.abs(v)) / den
            e_p = ((0.5 * bf16_ulp(p1 * (1 + 2.0 ** -20)) * scale) @ np.abs(v)) / den
            eps = 0.125 * gamma_mfma(64) * smag + nt * (5 * U32 * 0.125 * np.abs(s).max(axis=1, keepdims=True) + EXP2_REL)
            e_eps = ((p * eps) @ np.abs(v)) / den + np.abs(c) * (p * eps).sum(axis=1, keepdims=True) / den
            e_acc = gamma_mfma(S + nt) * (1 + 2.0 ** -8) * A + (gamma(S + nt + 1) + 3 * U32) * np.abs(c)
            rel = 2.0 ** -8 + eps.max(axis=1, keepdims=True) + gamma_mfma(S + nt)
            e2 = rel ** 2 * (A + np.abs(c))
            ctx[g, :, h], ctxp[g, :, h] = c, ((bf16_rne(p1) * scale) @ v) / den
            bound[g, :, h], second[g, :, h] = e_p + e_eps + e_acc + e2, e2
    flat = lambda a: a.reshape(G * S, W)                                                 # noqa: E731
    e = flat(bound)
    attn_full.second_share = float((flat(second) / rounded_bound(flat(ctx), e)).max())
    return flat(ctx), flat(ctxp), rounded_bound(flat(ctx), e)


def attn_fp32(qkv, G, S, H, order):
    """numpy fp32 with P rounded to bf16 in the P.V product.  'tiles': the online softmax over 64-key tiles (running maximum,
    rescaling, P rounded at the running maximum); 'whole': one pass under the row maximum."""
    W = 64 * H
    x = np.asarray(qkv, np.float32).reshape(G, S, 3, H, 64)
    out = np.empty((G, S, H, 64))
    one8 = np.float32(0.125)
    for g in range(G):
        for h in range(H):
            q, k, v = x[g, :, 0, h], x[g, :, 1, h], x[g, :, 2, h]
            s = q @ k.T
            if order == "whole":
                p = np.exp((s - s.max(axis=1, keepdims=True)) * one8)
                o = bf16_rne(p.astype(np.float64)).astype(np.float32) @ v
                l = p.sum(axis=1, keepdims=True, dtype=np.float32)
            else:
                m = np.full((S, 1), -np.inf, np.float32)
                l = np.zeros((S, 1), np.float32)
                o = np.zeros((S, 64), np.float32)
                for k0 in range(0, S, 64):
                    st = s[:, k0:k0 + 64]
                    m_new = np.maximum(m, st.max(axis=1, keepdims=True))
                    alpha = np.exp((m - m_new) * one8)
                    p = np.exp((st - m_new) * one8)
                    l = l * alpha + p.sum(axis=1, keepdims=True, dtype=np.float32)
                    o = o * alpha + bf16_rne(p.astype(np.float64)).astype(np.float32) @ v[k0:k0 + 64]
                    m = m_new
            out[g, :, h] = bf16_rne((o * (np.float32(1) / l)).astype(np.float64))
    return out.reshape(G * S, W)


def attn_cases():
    return [(G, H, S) for S in ATTN_S for G, H in ATTN_GH] + [(ATTN_GH_OTHER[0], ATTN_GH_OTHER[1], S) for S in ATTN_S_OTHER]
