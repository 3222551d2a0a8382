"""Plain fp64 statements of the TinyViT encoder's kernels (csrc/tinyvit.hip) and of the student decoder's attention (csrc/student.hip:
attn_small_kernel), the per-element error bounds that go with them, and the input generators of tests/test_encoder_kernels_gpu.py (run
on the CPU by tests/test_encoder_kernels.py).

Nothing here imports the library.  Operands are float64 arrays that hold bf16 values exactly (fp32 where the kernel reads fp32).
Number formats, gamma, GELU and the LayerNorm bound come from tests/text_rows_reference.py.

Bounds.  u = 2^-24 (fp32); rounding to bf16 moves a value by at most half a bf16 ulp.
  * tv_gemm: the fp32 accumulator, gamma(K) sum|a||w| (the worst case of any order); + bias, u |y|; erf-GELU, gelu_term; + residual,
    u |.|; a second gelu_term for the GELU behind the residual; half a bf16 ulp of the reference for the output.
  * tv_dwconv: nine bf16 x fp32 products, each rounded, eight adds and the bias: at most ten roundings of partial sums that never
    exceed sum|x||w| + |bias|, gamma(11) of it; gelu_term; half a bf16 ulp.
  * tv_ln: ln_bound on the exact row with the kernel's summation depth (a lane adds its 8 ceil(C / 512) values one after the other,
    then 6 butterfly steps); half a bf16 ulp.
  * tv_pool: HW - 1 adds in ascending order, gamma(HW) sum|x|, carried through the division (/ HW), and the division's own
    rounding, u |mean|.  The output is fp32.
  * tv_im2col, tv_to_nchw: exact.
  * tv_attn, attn_small: half a bf16 ulp of the fp64 context plus delta, the fp32 term of the score sums, the fast exp, the
    (running) normalisation and the division.  __expf's error is not specified, so delta is measured -- on the CPU, against the fp64
    reference, never against the device: the worst |fp32 - fp64| / |ctx| of a numpy fp32 restatement of each kernel's own loop over
    every input of the device test (DELTA_TV_ATTN_MEASURED, DELTA_ATTN_SMALL_MEASURED; tests/test_encoder_kernels.py recomputes
    them, profiles/r16_encoder_kernels.txt has the run); delta = 4 x that x |ctx| (the device's v_exp_f32 is not numpy's exp2),
    capped at a quarter of a bf16 ulp of the context so that it can never grow to hide a wrong key.  A relative measure needs a
    context that does not cancel: every V column keeps one sign over the keys (attn_v), so |ctx| >= min|v|.
"""
from __future__ import annotations

import math

import numpy as np

from text_rows_reference import U32, bf16_rne, bf16_ulp, flip_share, gamma, gelu, layernorm, ln_bound   # noqa: F401  (re-exported)

TV_GELU, TV_RES, TV_RES_GELU = 1, 2, 4            # csrc/tinyvit.hip
TV_ATTN_SCALE = 32.0 ** -0.5

F32 = np.float32


def f32(a):
    """fp64 array of the fp32 roundings of a"""
    return np.asarray(a, np.float32).astype(np.float64)


def gelu_term(y, e):
    """-> (gelu(y), bound on |gelu_fp32(y + e') - gelu(y)| for |e'| <= e): the erf polynomial's 1.5e-7 (csrc/common.h), four fp32
    roundings of the surrounding arithmetic, and the incoming error through |gelu'| <= 1.13 (text_rows_reference.py)."""
    out = gelu(y)
    return out, 1.13 * e + 0.5 * np.abs(y) * 1.5e-7 + 4 * U32 * np.abs(out) + 2 * U32 * np.abs(y)


def differs(wrong, ref, bound, factor=10.0):
    """True where a wrong variant misses the bound by `factor`, or is NaN / not NaN where the reference is not / is."""
    wrong, ref = np.asarray(wrong, np.float64), np.asarray(ref, np.float64)
    nw, nr = np.isnan(wrong), np.isnan(ref)
    with np.errstate(invalid="ignore"):
        return (nw != nr) | (~nw & ~nr & (np.abs(wrong - ref) > factor * bound))


# ---- fp32 helpers of the restatements ------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in fp64"""
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def erf_gelu32(x):
    """csrc/common.h: erf_gelu with fast_erf (Abramowitz-Stegun 7.1.26) in fp32; rcp and exp2 correctly rounded here."""
    x = np.asarray(x, F32)
    a = x * F32(0.70710678118654752)
    z = np.abs(a)
    t = (1.0 / _fma32(F32(0.3275911) * np.ones_like(z), z, F32(1.0)).astype(np.float64)).astype(F32)
    p = np.full_like(z, F32(1.061405429))
    for c in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        p = _fma32(p, t, F32(c))
    e = np.exp2(((F32(-1.4426950408889634) * z) * z).astype(np.float64)).astype(F32)
    r = np.copysign(_fma32(-(p * t), e, F32(1.0)), a)
    hx = F32(0.5) * x
    return _fma32(hx, r, hx)


def expf32(x):
    """__expf as exp2(x * log2 e) in fp32 (the argument's rounding is the error a fast exp adds)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp2((np.asarray(x, F32) * F32(1.4426950408889634)).astype(np.float64)).astype(F32)


# ---- tv_gemm ----------------------------------------------------------------------------------------------------------------------

def tv_gemm(A, W, bias, res, epi, variant=None):
    """out[m][n] = epi(A[m] . W[n] + bias[n]); epi 0, TV_GELU, TV_RES (+ res), TV_RES | TV_RES_GELU (+ res, then GELU) -> (out, bound).
    variant 'res_gelu_order' (TV_RES | TV_RES_GELU only): the GELU in front of the residual add instead of behind it."""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    K = A.shape[1]
    y = A @ W.T + bias
    e = gamma(K) * (np.abs(A) @ np.abs(W).T) + U32 * np.abs(y)
    if variant == "res_gelu_order":
        return gelu(y) + res, None
    if epi & TV_GELU:
        y, e = gelu_term(y, e)
    if epi & TV_RES:
        y = y + res
        e = e + U32 * np.abs(y)
    if epi & TV_RES_GELU:
        y, e = gelu_term(y, e)
    return y, e + 0.5 * bf16_ulp(y)


def tv_gemm_fp32(A, W, bias, res, epi):
    """The same in fp32: k in steps of 32, the epilogue in the kernel's order with its erf polynomial.  -> bf16 values"""
    A32, W32 = np.asarray(A, F32), np.asarray(W, F32)
    acc = np.zeros((A32.shape[0], W32.shape[0]), F32)
    for k0 in range(0, A32.shape[1], 32):
        acc = acc + A32[:, k0:k0 + 32] @ W32[:, k0:k0 + 32].T
    v = acc + np.asarray(bias, F32)
    if epi & TV_GELU:
        v = erf_gelu32(v)
    if epi & TV_RES:
        v = v + np.asarray(res, F32)
    if epi & TV_RES_GELU:
        v = erf_gelu32(v)
    return bf16_rne(v.astype(np.float64))


def tv_gemm_buffer(out, rows, ld, fill=np.nan):
    """`out` [M][N] in a [rows][ld] buffer of `fill`: what the device buffer must hold after a launch."""
    buf = np.full((rows, ld), fill)
    buf[:out.shape[0], :out.shape[1]] = out
    return buf


GEMM_CASES = [(1, 4, 32, 0), (31, 16, 32, TV_GELU), (33, 36, 64, TV_GELU), (70, 96, 448, 0), (64, 160, 640, TV_RES),
              (294, 576, 576, TV_RES), (50, 96, 384, TV_RES | TV_RES_GELU)]          # (M, N, K, epi)


def gemm_strides(N, K, wide):
    """(lda, ldo, ldr) of the two layouts every case runs in"""
    return (K + 8, N + 4, N + 12) if wide else (K, N, N)


def gemm_inputs(M, N, K, epi, seed):
    """A [M][K], W [N][K], res [M][N] bf16 values, bias fp32 [N] that depends on the column.  The pre-activation has a standard
    deviation near 1, so the GELU's far negative tail (where its value is smaller than the polynomial's error) stays rare."""
    rng = np.random.default_rng(seed)
    A = bf16_rne(rng.standard_normal((M, K)))
    W = bf16_rne(rng.standard_normal((N, K)) * (0.7 / math.sqrt(K)))
    bias = f32(np.linspace(-1.0, 1.0, N) + 0.2 * rng.standard_normal(N))
    res = bf16_rne(0.5 * rng.standard_normal((M, N)) + 0.25 * np.sin(np.arange(M))[:, None])
    return dict(A=A, W=W, bias=bias, res=res if epi & TV_RES else None)


# ---- tv_im2col / tv_to_nchw ---------------------------------------------------------------------------------------------------------

def tv_im2col(x, f32_nchw, Kp):
    """3x3 stride-2 pad-1 patches: out[(f, oy, ox)][ci * 9 + ky * 3 + kx] = x[f][ci][2 oy - 1 + ky][2 ox - 1 + kx] (0 outside the frame and
    for columns >= 9 Cin); x fp32 [n][Cin][H][W] (rounded to bf16) or bf16 [n][H][W][Cin].  -> [n * Ho * Wo][Kp], exact."""
    x = np.asarray(x, np.float64)
    if not f32_nchw:
        x = x.transpose(0, 3, 1, 2)
    n, Cin, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = np.zeros((n, Cin, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, Ho, Wo, Kp))
    for ky in range(3):
        for kx in range(3):
            out[..., ky * 3 + kx:9 * Cin:9] = xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2].transpose(0, 2, 3, 1)
    return bf16_rne(out.reshape(n * Ho * Wo, Kp))


IM2COL_CASES = [(1, 2, 2, 3, 32), (2, 4, 6, 3, 32), (1, 6, 4, 16, 160), (2, 8, 8, 48, 448)]          # (n, H, W, Cin, Kp)


def im2col_inputs(n, H, W, Cin, f32_nchw, seed):
    """A distinct value per (frame, pixel, channel): fp32 values that are not bf16 values (the kernel's rounding shows), or bf16."""
    rng = np.random.default_rng(seed)
    shape = (n, Cin, H, W) if f32_nchw else (n, H, W, Cin)
    x = rng.standard_normal(shape) + 0.01 * np.arange(int(np.prod(shape))).reshape(shape)
    return f32(x) if f32_nchw else bf16_rne(x)


def tv_to_nchw(x):
    """x [n][HW][C] -> [n][C][HW], exact"""
    return np.asarray(x, np.float64).transpose(0, 2, 1).copy()


# ---- tv_dwconv ------------------------------------------------------------------------------------------------------------------------

def tv_dwconv(x, w9, bias, stride, gelu_on, variant=None):
    """out[f][oy][ox][c] = sum_t x[f][s oy - 1 + ky][s ox - 1 + kx][c] w9[t = ky * 3 + kx][c] + bias[c] (-> GELU); x [n][H][W][C]
    -> (out [n][Ho][Wo][C], bound).  variant: 'taps_transposed' (tap (ky, kx) weighs with w9[kx * 3 + ky]), 'no_frame_boundary' (the
    frames stacked into one tall image: a tap above row 0 of frame f reads the last row of frame f - 1), 'stride_one_axis' (the
    stride applied to y only)."""
    x, w9 = np.asarray(x, np.float64), np.asarray(w9, np.float64)
    n, H, W, C = x.shape
    Ho, Wo = H // stride, W // stride
    if variant == "no_frame_boundary":
        xp = np.zeros((1, n * H + 2, W + 2, C))
        xp[0, 1:-1, 1:-1] = x.reshape(n * H, W, C)
    else:
        xp = np.zeros((n, H + 2, W + 2, C))
        xp[:, 1:-1, 1:-1] = x
    sx = 1 if variant == "stride_one_axis" else stride
    acc, mag = np.zeros((n, Ho, Wo, C)), np.zeros((n, Ho, Wo, C))
    for ky in range(3):
        for kx in range(3):
            w = w9[kx * 3 + ky] if variant == "taps_transposed" else w9[ky * 3 + kx]
            if variant == "no_frame_boundary":
                rows = (np.arange(n)[:, None] * H + stride * np.arange(Ho)[None, :] + ky).reshape(-1)
                tap = xp[0, rows][:, kx:kx + sx * Wo:sx].reshape(n, Ho, Wo, C)
            else:
                tap = xp[:, ky:ky + stride * Ho:stride, kx:kx + sx * Wo:sx]
            acc += tap * w
            mag += np.abs(tap * w)
    y = acc + bias
    e = gamma(11) * (mag + np.abs(bias))
    if gelu_on:
        y, e = gelu_term(y, e)
    return y, e + 0.5 * bf16_ulp(y)


def tv_dwconv_fp32(x, w9, bias, stride, gelu_on):
    x32 = np.asarray(x, F32)
    n, H, W, C = x32.shape
    Ho, Wo = H // stride, W // stride
    xp = np.zeros((n, H + 2, W + 2, C), F32)
    xp[:, 1:-1, 1:-1] = x32
    acc = np.zeros((n, Ho, Wo, C), F32)
    for t in range(9):
        ky, kx = divmod(t, 3)
        acc = acc + xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] * np.asarray(w9[t], F32)
    v = acc + np.asarray(bias, F32)
    return bf16_rne((erf_gelu32(v) if gelu_on else v).astype(np.float64))


DWCONV_CASES = [(1, 1, 1, 8, 1, False), (2, 3, 5, 8, 1, True), (1, 4, 6, 16, 2, True), (2, 7, 7, 40, 1, False),
                (1, 8, 8, 160, 2, True)]                                               # (n, H, W, C, stride, gelu)


def dwconv_inputs(n, H, W, C, seed):
    """x distinct per (frame, pixel, channel); taps that depend on the tap and the channel (no two taps of a channel alike, so a
    transposed or shifted tap shows); a bias that depends on the channel."""
    rng = np.random.default_rng(seed)
    x = bf16_rne(rng.standard_normal((n, H, W, C)) + 0.5 * np.sin(np.arange(n * H * W * C)).reshape(n, H, W, C))
    w9 = f32(0.3 * rng.standard_normal((9, C)) + 0.1 * (np.arange(9)[:, None] - 4) * (1 + (np.arange(C)[None, :] % 3)))
    bias = f32(np.linspace(-0.5, 0.5, C) + 0.1 * rng.standard_normal(C))
    return dict(x=x, w9=w9, bias=bias)


def dwconv_variants(n, H, W, C, stride, gelu_on):
    """The wrong variants a case can tell apart at all: a frame boundary needs two frames, the stride a stride, a transposed tap
    a pixel with a neighbour."""
    return ((["taps_transposed"] if H * W > 1 else []) + (["no_frame_boundary"] if n > 1 else []) +
            (["stride_one_axis"] if stride == 2 else []))


# ---- tv_ln ---------------------------------------------------------------------------------------------------------------------------

def tv_ln(x, g, b, eps, divisor=None):
    """LayerNorm of the rows of x [M][C] -> (out, bound).  divisor: a wrong kernel's count in place of C for the mean and the variance."""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    if divisor is not None:
        mu = x.sum(axis=1, keepdims=True) / divisor
        var = ((x - mu) ** 2).sum(axis=1, keepdims=True) / divisor
        return (x - mu) / np.sqrt(var + eps) * g + b, None
    y = layernorm(x, g, b, eps)
    depth = 8 * ((C + 511) // 512) + 6
    return y, ln_bound([], [x], g, b, eps, sum_depth=depth) + 0.5 * bf16_ulp(y)


def tv_ln_fp32(x, g, b, eps):
    """Two-pass fp32 statistics in the kernel's order: lane l adds columns 8 (l + 64 j) .. + 7, j ascending; a xor butterfly over the
    64 lanes."""
    x32 = np.asarray(x, F32)
    M, C = x32.shape

    def wave_sum(vals):                                   # vals [M][C] -> [M]
        lanes = np.zeros((M, 64), F32)
        for j in range((C + 511) // 512):
            for r in range(8):
                cols = 8 * (np.arange(64) + 64 * j) + r
                ok = cols < C
                lanes[:, ok] = lanes[:, ok] + vals[:, cols[ok]]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, np.arange(64) ^ o]
        return lanes[:, 0]
    mean = wave_sum(x32) / F32(C)
    d = x32 - mean[:, None]
    rstd = F32(1.0) / np.sqrt(wave_sum(d * d) / F32(C) + F32(eps))
    return bf16_rne((d * rstd[:, None] * np.asarray(g, F32) + np.asarray(b, F32)).astype(np.float64))


LN_CASES = [(1, 8), (5, 32), (4, 160), (3, 448), (9, 576), (2, 2048)]                    # (M, C)


def ln_inputs(M, C, seed):
    """Rows with a column-dependent offset, gamma / beta that depend on the column; the last row of a case with more than one row is
    the hard one: a mean of 257 and a spread of 1 from the bf16 values 256 and 258 (a one-pass variance in fp32 loses it)."""
    rng = np.random.default_rng(seed)
    x = bf16_rne(rng.standard_normal((M, C)) * (1.0 + np.arange(M)[:, None] % 3) + np.linspace(-1, 1, C))
    if M > 1:
        x[-1] = 256.0 + 2.0 * ((np.arange(C) * 7 // 3 + rng.integers(0, 2, C)) % 2)
    g = f32(1.0 + 0.5 * np.sin(np.arange(C)))
    b = f32(0.3 * np.cos(np.arange(C) * 0.7))
    return dict(x=x, g=g, b=b, eps=1e-5)


# ---- tv_pool -------------------------------------------------------------------------------------------------------------------------

def tv_pool(x, divisor=None):
    """mem[f][c] = mean over the HW pixels of x [n][HW][C] -> (mem, bound) (fp32 output)."""
    x = np.asarray(x, np.float64)
    HW = x.shape[1]
    if divisor is not None:
        return x.sum(axis=1) / divisor, None
    mean = x.mean(axis=1)
    return mean, gamma(HW) * np.abs(x).sum(axis=1) / HW + U32 * np.abs(mean)


def tv_pool_fp32(x):
    x32 = np.asarray(x, F32)
    s = np.zeros((x32.shape[0], x32.shape[2]), F32)
    for p in range(x32.shape[1]):
        s = s + x32[:, p]
    return (s / F32(x32.shape[1])).astype(np.float64)


POOL_CASES = [(1, 1, 32), (2, 49, 576), (3, 196, 64), (1, 4, 320)]                       # (n, HW, C)
NCHW_CASES = [(2, 49, 576), (1, 4, 320)]


def pool_inputs(n, HW, C, seed):
    rng = np.random.default_rng(seed)
    return bf16_rne(rng.standard_normal((n, HW, C)) + np.linspace(-2, 2, C) + 0.3 * np.arange(n)[:, None, None])


# ---- attention: shared ----------------------------------------------------------------------------------------------------------------

# Worst |fp32 restatement - fp64| / |ctx| over the inputs of the device test, measured on the CPU (profiles/r16_encoder_kernels.txt;
# tests/test_encoder_kernels.py recomputes both and holds them to these values).
DELTA_TV_ATTN_MEASURED = 1.2e-6
DELTA_ATTN_SMALL_MEASURED = 4.5e-7


def attn_delta(ctx64, measured):
    """4 x the measured relative fp32 term, capped at a quarter of a bf16 ulp of the context"""
    return np.minimum(4.0 * measured * np.abs(ctx64), 0.25 * bf16_ulp(ctx64))


def attn_bound(ctx64, measured):
    return 0.5 * bf16_ulp(ctx64) + attn_delta(ctx64, measured)


def attn_v(rng, keys_shape, hd):
    """V [...keys][hd]: magnitudes in [1, 2) (the callers may scale a key's row) that differ from key to key, one sign per column (alternating in pairs): a context is a
    convex mix of its keys' values, so it keeps that sign and |ctx| >= 1 -- no cancellation, and a dropped or foreign key moves it
    by a good part of its own size."""
    sign = np.where((np.arange(hd) // 2) % 2 == 0, 1.0, -1.0)
    return bf16_rne((1.0 + rng.uniform(0, 1, tuple(keys_shape) + (hd,)) * 0.996) * sign)


# ---- tv_attn --------------------------------------------------------------------------------------------------------------------------

def bias_idx(ws, swap=False):
    """[N][N] index into a head's compact table: |dy| ws + |dx| for tokens p = (py, px), q = (qy, qx) in row-major order -- which is
    the order in which (|dy|, |dx|) first appears over points x points (timm's rule; test_encoder_kernels.py checks it against
    tinyvit_reference.attention_bias_idxs).  swap: |dx| ws + |dy|, a wrong kernel."""
    p = np.arange(ws * ws)
    dy = np.abs(p[:, None] // ws - p[None, :] // ws)
    dx = np.abs(p[:, None] % ws - p[None, :] % ws)
    return dx * ws + dy if swap else dy * ws + dx


def window_rows(n, H, W, ws, shift=0):
    """[windows][N] row numbers of qkv / ctx: window (f, wy, wx) frame-major, token i = (i / ws, i % ws).  shift: the window's columns
    start `shift` pixels further right (wrapping inside the row), a wrong kernel."""
    f, wy, wx, iy, ix = np.meshgrid(np.arange(n), np.arange(H // ws), np.arange(W // ws), np.arange(ws), np.arange(ws), indexing="ij")
    rows = (f * H + wy * ws + iy) * W + (wx * ws + ix + shift) % W
    return rows.reshape(n * (H // ws) * (W // ws), ws * ws)


def _tv_attn_operands(qkv, n, H, W, heads, ws, key_shift=0):
    t = np.asarray(qkv).reshape(n * H * W, heads, 3, 32)
    rq, rk = window_rows(n, H, W, ws), window_rows(n, H, W, ws, key_shift)
    q = t[rq][:, :, :, 0].transpose(0, 2, 1, 3)                       # [windows][heads][N][32]
    k = t[rk][:, :, :, 1].transpose(0, 2, 1, 3)
    v = t[rk][:, :, :, 2].transpose(0, 2, 1, 3)
    return q, k, v, rq


def tv_attn(qkv, ab, n, H, W, heads, ws, variant=None):
    """ctx = softmax(q k^T 32^-1/2 + table[h]) v per (window, head); qkv [n H W][96 heads] (head h: q | k | v at columns 96 h + 0 / 32 /
    64), ab the compact table [heads][ws^2] -> ctx [n H W][32 heads], fp64, unrounded.  variant: 'swap_dydx' (bias_idx
    swap), 'next_head_table' (head h reads the table of head h + 1), 'window_shift' (the keys of a window taken one pixel to the
    right), 'last_key' (the window's last key dropped)."""
    N = ws * ws
    q, k, v, rq = _tv_attn_operands(qkv, n, H, W, heads, ws, 1 if variant == "window_shift" else 0)
    dense = np.asarray(ab, np.float64)[:, bias_idx(ws, variant == "swap_dydx")]            # [heads][N][N]
    if variant == "next_head_table":
        dense = np.roll(dense, -1, axis=0)
    s = np.einsum("whid,whjd->whij", q, k) * TV_ATTN_SCALE + dense[None]
    if variant == "last_key":
        s, v = s[..., :N - 1], v[:, :, :N - 1]
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    o = np.einsum("whij,whjd->whid", p / p.sum(axis=-1, keepdims=True), v)
    ctx = np.zeros((n * H * W, heads * 32))
    ctx[rq.reshape(-1)] = o.transpose(0, 2, 1, 3).reshape(-1, heads * 32)
    return ctx


def tv_attn_fp32(qkv, ab, n, H, W, heads, ws):
    """The kernel's loop in fp32: keys in ascending order, the score summed over d = 0 .. 31 in order, a running maximum that rescales
    what was summed so far, __expf, one division at the end.  -> fp64 array of the fp32 context (unrounded)"""
    N = ws * ws
    q, k, v, rq = _tv_attn_operands(qkv, n, H, W, heads, ws)
    q, k, v = q.astype(F32), k.astype(F32), v.astype(F32)
    dense = np.asarray(ab, F32)[:, bias_idx(ws)]
    shape = q.shape[:3]
    o = np.zeros(q.shape, F32)
    mx = np.full(shape, -np.inf, F32)
    l = np.zeros(shape, F32)
    for j in range(N):
        s = np.zeros(shape, F32)
        for d in range(32):
            s = s + q[..., d] * k[:, :, j, None, d]
        s = s * F32(0.17677669529663687) + dense[None, :, :, j]
        up = s > mx
        corr = np.where(up, expf32(mx - s), F32(1.0))
        l = l * corr
        o = o * corr[..., None]
        mx = np.where(up, s, mx)
        p = expf32(s - mx)
        l = l + p
        o = o + p[..., None] * v[:, :, j, None, :]
    o = o * (F32(1.0) / l)[..., None]
    ctx = np.zeros((n * H * W, heads * 32))
    ctx[rq.reshape(-1)] = o.astype(np.float64).transpose(0, 2, 1, 3).reshape(-1, heads * 32)
    return ctx


TV_ATTN_CASES = [(1, 1, 1, 1, 1, "n"), (1, 2, 2, 1, 2, "n"), (1, 3, 6, 2, 3, "n"), (2, 4, 8, 2, 4, "n"), (2, 7, 14, 5, 7, "n"),
                 (1, 13, 13, 1, 13, "n"), (1, 14, 28, 3, 14, "n"), (1, 7, 7, 2, 7, "ascending"), (1, 7, 14, 1, 7, "max_first")]
# (n, H, W, heads, ws, kind): N = 1, 4, 9 (blockDim 64, 9 threads at work), 16, 49, 169 (192), 196 (256); H != W; 1, 2, 3 and 5 heads


def tv_attn_inputs(n, H, W, heads, ws, kind, seed):
    """qkv bf16 values, the compact table fp32.  q, k ~ n(0, 1) (scores ~ n(0, 1)), v = attn_v; the table is spread over [-2, 2] with
    no two entries of a head alike and none shared between heads: a wrong entry moves a logit by O(1).  kind 'ascending' /
    'max_first': the score of a window's key j is 0.25 j / -0.25 j plus a table of +-0.05, so the running maximum rises at every key /
    is the first key's."""
    rng = np.random.default_rng(seed)
    N = ws * ws
    t = rng.standard_normal((n * H * W, heads, 3, 32))
    ab = rng.permutation(np.linspace(-2.0, 2.0, heads * N)).reshape(heads, N)
    if kind != "n":
        rows = window_rows(n, H, W, ws)
        j = np.zeros(n * H * W)
        j[rows.reshape(-1)] = np.tile(np.arange(N), rows.shape[0])
        t[:, :, :2] *= 0.05
        t[:, :, 0, 0] = 1.0
        t[:, :, 1, 0] = (j * (0.25 if kind == "ascending" else -0.25) / TV_ATTN_SCALE)[:, None]
        ab = ab * 0.025
    t[:, :, 2] = attn_v(rng, (n * H * W, heads), 32)
    if kind == "n":
        t[window_rows(n, H, W, ws)[:, -1], :, 2] *= 8.0                # a window's last key weighs 8 x: leaving it out shows at 169 keys too
    return dict(qkv=bf16_rne(t.reshape(n * H * W, heads * 96)), ab=f32(ab))


def tv_attn_variants(n, H, W, heads, ws, kind):
    """The wrong variants a case can tell apart at all.  One key: the softmax is 1 whatever the table holds.  The next head's table
    needs a second head.  'ascending' / 'max_first' are there for the running maximum: their table of +-0.05 is too flat to show a
    wrong entry; the weight sits on the last key of 'ascending' (dropping it shows) and on the first of 'max_first' (a shifted window
    loses it)."""
    if ws == 1:
        return []
    if kind != "n":
        return ["last_key"] if kind == "ascending" else ["window_shift"]
    return ["swap_dydx", "window_shift", "last_key"] + (["next_head_table"] if heads > 1 else [])


# ---- attn_small ----------------------------------------------------------------------------------------------------------------------

def attn_small(a, variant=None, fp32=False):
    """The student decoder's attention.  a = attn_small_inputs(...): query m = (r, j) reads q from ring row q_row_off + j of text row r,
    sees keys 0 .. nkeys - 1 (nkeys > 0) or 0 .. t0 + j (causal) of row r, but for those whose ids[r][key] == pad_id; scale hd^-1/2.
    -> ctx [rows * T][H][hd] in fp64, NaN where every key of a query is masked (softmax of nothing, as torch).
    variant: 'causal_short' (keys 0 .. t0 + j - 1), 'mask_next_row' (the PAD mask of row r + 1), 'q_row_off' (q_row_off ignored).
    fp32: the kernel's loop -- the score summed over d in order, the maximum, __expf, a butterfly sum of the 64 lanes' p, p / sum, then
    P . V over the keys in ascending order."""
    rows, T, t0, nkeys, H, hd = a["rows"], a["T"], a["t0"], a["nkeys"], a["H"], a["hd"]
    ft = F32 if fp32 else np.float64
    ctx = np.full((rows * T, H, hd), np.nan)
    for m in range(rows * T):
        r, j = divmod(m, T)
        nk = nkeys if nkeys > 0 else t0 + j + (0 if variant == "causal_short" else 1)
        qrow = j if variant == "q_row_off" else a["q_row_off"] + j
        masked = np.zeros(nk, bool)
        if a["ids"] is not None:
            masked = a["ids"][(r + 1) % rows if variant == "mask_next_row" else r, :nk] == a["pad_id"]
        if nk == 0 or masked.all():
            continue
        for h in range(H):
            q = a["q"][r, qrow, h].astype(ft)
            k, v = a["k"][r, :nk, h].astype(ft), a["v"][r, :nk, h].astype(ft)
            if fp32:
                acc = np.zeros(nk, F32)
                for d in range(hd):
                    acc = acc + q[d] * k[:, d]
                s = np.where(masked, -np.inf, acc * (F32(1.0) / np.sqrt(F32(hd)))).astype(F32)
                lanes = np.zeros(64, F32)
                lanes[:nk] = expf32(s - s.max())
                for o in (32, 16, 8, 4, 2, 1):
                    lanes = lanes + lanes[np.arange(64) ^ o]
                ps = lanes * 0
                ps[:nk] = expf32(s - s.max()) / lanes[0]
                out = np.zeros(hd, F32)
                for i in range(nk):
                    out = out + ps[i] * v[i]
                ctx[m, h] = out.astype(np.float64)
            else:
                s = np.where(masked, -np.inf, (k @ q) / math.sqrt(hd))
                p = np.exp(s - s.max())
                ctx[m, h] = (p / p.sum()) @ v
    return ctx


ATTN_SMALL_CASES = [(1, 1, 0, 0, 1, 8), (2, 3, 5, 0, 2, 32), (1, 1, 63, 0, 4, 64), (2, 2, 0, 0, 1, 128),      # causal
                    (3, 1, 0, 6, 4, 64), (1, 4, 0, 64, 2, 40)]                                               # cross
# (rows, T, t0, nkeys, H, hd): 1 key, 64 keys, hd 8 / 32 / 40 / 64 / 128 (two output columns per lane at 128)

PAD_ID = 7


def attn_small_inputs(rows, T, t0, nkeys, H, hd, with_ids, seed):
    """q in a ring of q_rows = T + 5 rows per text row at q_row_off = 3 (the other ring rows hold other finite values), k / v
    [rows][keys][H][hd] with `keys` = what the last query sees; ids [rows][keys + 2] (with_ids) mask, row by row in turn, the first
    key, a middle key and the last key -- at one key (case 0) that is every key of the row: NaN.  The value rows of the keys a wrong bound or mask
    is most likely to lose (the queries' own positions, the last cross key) are 8 x as large as the others."""
    rng = np.random.default_rng(seed)
    keys = nkeys if nkeys > 0 else t0 + T
    q_row_off, q_rows = 3, T + 5
    q = bf16_rne(rng.standard_normal((rows, q_rows, H, hd)))
    k = bf16_rne(rng.standard_normal((rows, keys, H, hd)))
    v = attn_v(rng, (rows, keys, H), hd)
    v[:, (nkeys - 1 if nkeys > 0 else t0):] *= 8.0            # the queries' own positions (causal) / the last key (cross) weigh 8 x
    ids = None
    if with_ids:
        ids = rng.integers(PAD_ID + 1, 1000, size=(rows, keys + 2)).astype(np.int64)
        for r in range(rows):
            ids[r, (0, keys // 2, keys - 1)[r % 3]] = PAD_ID
            ids[r, keys:] = PAD_ID                                     # behind the keys: never read
    return dict(rows=rows, T=T, t0=t0, nkeys=nkeys, H=H, hd=hd, keys=keys, q=q, k=k, v=v, ids=ids, pad_id=PAD_ID, q_row_off=q_row_off,
                q_rows=q_rows)


def attn_small_variants(rows, T, t0, nkeys, H, hd, with_ids):
    """The wrong variants a case can tell apart at all: a query with one key left has that key's value as its context whatever q is
    (or NaN when the key is PAD); another row's mask needs another row."""
    keys = nkeys if nkeys > 0 else t0 + T
    if keys == 1:
        return [] if with_ids else ["causal_short"]
    return ((["q_row_off"] if keys - (1 if with_ids else 0) > 1 else []) + (["causal_short"] if nkeys == 0 else []) +
            (["mask_next_row"] if with_ids and rows > 1 else []))
