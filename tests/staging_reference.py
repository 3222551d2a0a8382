"""Plain fp64 / numpy statements of the teacher's staging and layout kernels (csrc/preproc.hip, the plain row kernels of
csrc/rowops.hip and the text embedding of csrc/select.hip), and the inputs of tests/test_staging_gpu.py (kept honest on the CPU by tests/test_staging.py).

Nothing here imports the oracle or the library.  Number formats, LayerNorm and its bound come from text_rows_reference.

The frame transform (preprocess64).  ToTensor -> Resize(crop, bicubic) -> CenterCrop(crop) -> BGR->RGB -> Normalize, with the geometry
of oracle/preprocess_oracle.py.  The source coordinate of destination index d is taken as the transform defines it in fp32,
sy = fp32(H) / fp32(newH), r = fp32(fp32(sy * (d + 0.5)) - 0.5): two roundings, no fused multiply-add.  Everything behind it is fp64:
t = r - floor(r), the four cubic-convolution weights (A = -0.75), taps clamped to the image, x pass then y pass, channel swap,
(v - mean) / std with the fp32 constants.  `magnitude` is the same sum with |w| and |p|, plus mean, over std.

Bound on |kernel - preprocess64|, counted in roundings of u = 2^-24 (preprocess_roundings), S = sum |wy_i| |wx_j| p_ij:
  * terms that scale with S: p / 255 (1), the product with wx (1), the x pass' three adds behind the first (3), the product with wy
    (1), the y pass' three adds (3): 9 u S.
  * the normalisation: the subtraction, u |v - mean| <= u (S + mean); the multiplication by 1 / std and the fp32 rounding of that
    constant, 2 u |out|: together at most 3 u magnitude.
  * the weights.  A weight polynomial is evaluated in fp32 by Horner's rule on exact coefficients, as the transform defines it
    (ATen's cubic_convolution1 / 2 are the same expressions):
        cc1(x) = ((1.25 x - 2.25) x) x + 1            x in [0, 1]      (the two inner taps: x = t, 1 - t)
        cc2(x) = ((-0.75 x + 3.75) x - 6) x + 3       x in [1, 2]      (the two outer taps: x = t + 1, 2 - t)
    Counting half an ulp per intermediate (they reach 4.5 and 6 = |8 A| in cc2, times the powers of x still to come) gives up to
    24 u ABSOLUTE at x = 2, where the weight itself is 0: an error that does not scale with its weight cannot be bounded by a
    multiple of sum |w| |p|, and against the floor mean / std of magnitude it would cost a constant near 190.  So the weights'
    rounding is not bounded but evaluated: axis_taps repeats the six (five) fp32 operations of each polynomial on the fp32 t and
    arguments (numpy float32, no contraction -- the library is built without it) and Ex_j / Ey_i = |w_fp32 - w_fp64| / u + 1/2, the
    half unit for one more rounding of a value below 1.  They enter the pixel as sum_ij (|wy_i| Ex_j + Ey_i |wx_j|) p_ij.
  * 2^-20 relative on top for the second-order terms.
Together: roundings = (9 S + weight term) / std + 3 magnitude; the identity case (no resize) is 1 + 3 roundings.  The weight term
depends on the frame; preprocess_roundings / magnitude is at most 40.5 on the frames of PRE_CASES (12 .. 16 on average) and PRE_C = 48
is the constant of the GPU test's bound PRE_C 2^-24 magnitude: tests/test_staging.py asserts, from the frames alone, that it covers
every element of every one of them.

embed_text: ln_bound of text_rows_reference with no slab terms and the two tail terms word[id], pos[t0 + j] (one add).

Everything else moves or rounds data and is compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from text_rows_reference import U32, bf16_rne, e4m3_decode, layernorm, ln_bound  # noqa: F401  (re-exported for the tests)

MEAN = np.array([0.48145466, 0.4578275, 0.40821073], np.float32).astype(np.float64)
STD = np.array([0.26862954, 0.26130258, 0.27577711], np.float32).astype(np.float64)
A = -0.75
PRE_C = 48.0

# (H, W, crop): H < W, H > W, H == W != crop, identity, upsampling in both axes, crop offsets 0 and odd, crop^2 % 256 != 0
PRE_GEOMETRIES = [(9, 16, 8), (16, 9, 8), (11, 11, 8), (8, 8, 8), (5, 7, 8), (30, 41, 12), (37, 53, 28), (53, 37, 28), (29, 28, 28),
                  (28, 33, 28), (64, 48, 16), (17, 16, 16), (16, 21, 16), (100, 300, 32)]
# the GPU test's launches: (nf, H, W, crop); (3, 37, 53, 28): the last workgroup is partial and a workgroup spans two frames
PRE_CASES = [(nf, H, W, crop) for nf in (1, 3) for (H, W, crop) in PRE_GEOMETRIES]


def frames_u8(nf, H, W, seed):
    """uint8 BGR camera frames [nf][H][W][3]: noise, with the extreme values 0 and 255 on the border rows and columns"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(nf, H, W, 3), dtype=np.uint8)
    f[:, 0, ::2] = 255
    f[:, -1, 1::2] = 0
    f[:, ::2, 0] = 0
    f[:, 1::2, -1] = 255
    return f


def pre_case_frames(i):
    """the frames of PRE_CASES[i]"""
    nf, H, W, _ = PRE_CASES[i]
    return frames_u8(nf, H, W, 100 + i)


# ---- the frame transform ----------------------------------------------------------------------------------------------------------

def geometry(H, W, crop):
    """Resize(crop) + CenterCrop(crop) of an H x W frame -> (newH, newW, top, left); offsets round half to even"""
    if H <= W:
        nh, nw = crop, int(crop * W / H)
    else:
        nh, nw = int(crop * H / W), crop
    return nh, nw, int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))


def cc1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def cc2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def _cc1_f32(x):
    return ((np.float32(A + 2.0) * x - np.float32(A + 3.0)) * x * x + np.float32(1.0)).astype(np.float32)


def _cc2_f32(x):
    return (((np.float32(A) * x - np.float32(5.0 * A)) * x + np.float32(8.0 * A)) * x - np.float32(4.0 * A)).astype(np.float32)


def axis_taps(n_src, n_new, off, crop):
    """One axis: destination o < crop reads source taps idx [crop][4] (clamped) with weights w [crop][4]; err [crop][4] = the distance
    of the fp32 weight from w in units of 2^-24, plus half a unit (module docstring)."""
    s = np.float32(n_src) / np.float32(n_new)
    d = (np.arange(crop) + off).astype(np.float32) + np.float32(0.5)
    r32 = ((s * d).astype(np.float32) - np.float32(0.5)).astype(np.float32)
    r = r32.astype(np.float64)
    f = np.floor(r)
    t = r - f
    idx = np.clip(f[:, None].astype(np.int64) - 1 + np.arange(4)[None, :], 0, n_src - 1)
    w = np.stack([cc2(t + 1.0), cc1(t), cc1(1.0 - t), cc2(2.0 - t)], axis=1)
    t32 = (r32 - np.floor(r32)).astype(np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    w32 = np.stack([_cc2_f32(t32 + one), _cc1_f32(t32), _cc1_f32(one - t32), _cc2_f32(two - t32)], axis=1)
    assert w32.dtype == np.float32
    return idx, w, np.abs(w32.astype(np.float64) - w) / U32 + 0.5


def _two_pass(P, yi, wy, xi, wx):
    """sum_i wy[oy][i] sum_j wx[ox][j] P[yi[oy][i]][xi[ox][j]][c] -> [crop][crop][3]"""
    a = np.einsum("hojc,oj->hoc", P[:, xi], wx)                 # x pass, every source row
    return np.einsum("yioc,yi->yoc", a[yi], wy)


def _pre(img_u8, crop):
    img = np.asarray(img_u8)
    H, W, _ = img.shape
    nh, nw, top, left = geometry(H, W, crop)
    P = img.astype(np.float64) / 255.0
    if (nh, nw) == (H, W):
        v = P[top:top + crop, left:left + crop]
        return v, v, np.zeros_like(v), True
    yi, wy, ey = axis_taps(H, nh, top, crop)
    xi, wx, ex = axis_taps(W, nw, left, crop)
    v = _two_pass(P, yi, wy, xi, wx)
    S = _two_pass(P, yi, np.abs(wy), xi, np.abs(wx))
    werr = _two_pass(P, yi, np.abs(wy), xi, ex) + _two_pass(P, yi, ey, xi, np.abs(wx))
    return v, S, werr, False


def _chw_rgb(x):
    return np.ascontiguousarray(x[..., ::-1].transpose(2, 0, 1))


def preprocess64(img_u8, crop):
    """uint8 HWC BGR frame -> (value, magnitude), fp64 [3][crop][crop] RGB each (module docstring)"""
    v, S, _, _ = _pre(img_u8, crop)
    m, s = MEAN[:, None, None], STD[:, None, None]
    return (_chw_rgb(v) - m) / s, (_chw_rgb(S) + m) / s


def preprocess_roundings(img_u8, crop):
    """The bound on |kernel - preprocess64| in units of 2^-24, [3][crop][crop], counted as the module docstring says"""
    v, S, werr, identity = _pre(img_u8, crop)
    m, s = MEAN[:, None, None], STD[:, None, None]
    mag = (_chw_rgb(S) + m) / s
    n = _chw_rgb(S) / s if identity else (9.0 * _chw_rgb(S) + _chw_rgb(werr)) / s
    return (n + 3.0 * mag) * (1.0 + 2.0 ** -20)


# ---- row layouts ------------------------------------------------------------------------------------------------------------------

def patch_rows(frames, p, Kp, fill=0.0):
    """frames [nf][3][img][img] -> [nf * G * G][Kp], row (frame, gy, gx), column k = c p p + py p + px; columns >= 3 p p hold `fill`"""
    frames = np.asarray(frames)
    nf, _, img, _ = frames.shape
    G = img // p
    out = np.full((nf * G * G, Kp), fill, frames.dtype)
    for f in range(nf):
        for gy in range(G):
            for gx in range(G):
                out[(f * G + gy) * G + gx, :3 * p * p] = frames[f, :, gy * p:gy * p + p, gx * p:gx * p + p].reshape(-1)
    return out


def stem_rows(frames):
    """frames [nf][3][crop][crop] -> [nf * Ho * Ho][32], Ho = crop / 2: the 3x3 stride-2 pad-1 windows, column k = ci 9 + ky 3 + kx,
    zero at taps outside the frame and at k >= 27"""
    frames = np.asarray(frames)
    nf, _, crop, _ = frames.shape
    Ho = crop // 2
    out = np.zeros((nf * Ho * Ho, 32), frames.dtype)
    for f in range(nf):
        for oy in range(Ho):
            for ox in range(Ho):
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                        if 0 <= iy < crop and 0 <= ix < crop:
                            out[(f * Ho + oy) * Ho + ox, np.arange(3) * 9 + ky * 3 + kx] = frames[f, :, iy, ix]
    return out


def ring_slot(head, j, F):
    return (head + j) % F


def window_scatter(ring, src, head):
    """ring [B][F][rows][D] (changed in place and returned) <- src [B][n][rows][D]: frame j of clip b to slot (head + j) % F"""
    B, n = src.shape[:2]
    F = ring.shape[1]
    for b in range(B):
        for j in range(n):
            ring[b, ring_slot(head, j, F)] = src[b, j]
    return ring


def window_assemble(ring, temporal, head):
    """ring fp32 [B][F][N][D], temporal fp32 [F][D] or None -> the fp32 sums [B * F * N][D], window position f = slot (head + f) % F"""
    B, F, N, D = ring.shape
    out = np.empty((B, F, N, D), np.float32)
    for f in range(F):
        x = ring[:, ring_slot(head, f, F)].astype(np.float32)
        out[:, f] = x if temporal is None else x + temporal[f].astype(np.float32)[None, None, :]
    return out.reshape(B * F * N, D)


def ragged_tables(counts, N):
    """per-clip frame counts -> off [B], len [B] (in rows of N per frame), pos [sum counts] (the frame's index inside its clip)"""
    counts = np.asarray(counts, np.int64)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    pos = np.concatenate([np.arange(n) for n in counts])
    return (start * N).astype(np.int32), (counts * N).astype(np.int32), pos.astype(np.int32)


def ragged_temporal(ln, temporal, pos, N):
    """ln fp32 [frames * N][D] + temporal[pos[row / N]] -> the fp32 sums"""
    return (ln.astype(np.float32) + temporal.astype(np.float32)[np.repeat(np.asarray(pos), N)]).astype(np.float32)


def gather_hidden(img, txt, B, S_img, T):
    """img [entries][B * S_img][D], txt [entries][B * T][D] -> [B][entries][S_img + T][D]"""
    E, _, D = img.shape
    out = np.empty((B, E, S_img + T, D), img.dtype)
    for b in range(B):
        out[b, :, :S_img] = img[:, b * S_img:(b + 1) * S_img]
        out[b, :, S_img:] = txt[:, b * T:(b + 1) * T]
    return out


def gather_txt_rows(src, dst, src_rows, t_len):
    """dst [layers][rows][Tmax][width] (changed in place and returned): dst[l][r][t] = src[l][src_rows[r]][t] for t < t_len"""
    for r, sr in enumerate(src_rows):
        dst[:, r, :t_len] = src[:, sr, :t_len]
    return dst


# ---- number formats ---------------------------------------------------------------------------------------------------------------

def dequant(codes, scale):
    """e4m3 codes [rows][K] x one scale per row -> the bf16 values (the rounding is the identity for power-of-two scales in range);
    the two NaN codes (S.1111.111) give NaN"""
    codes = np.asarray(codes)
    v = bf16_rne(e4m3_decode(codes) * np.asarray(scale, np.float64)[:, None])
    return np.where((codes & 0x7f) == 0x7f, np.nan, v)


def bits_of_bf16(x):
    """bf16 values held in fp64 / fp32 (NaN allowed) -> their uint16 bit patterns, as the device stores them (NaN: 0x7fc0 | sign)"""
    return (np.asarray(x, np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_of_f32(x32):
    """fp32 array -> the bits of its bf16 rounding (nearest even; +-inf stay, NaN stays a NaN): what pack_bf2 / f2bf give"""
    x32 = np.asarray(x32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = bf16_rne(np.where(np.isfinite(x32), x32, 0.0).astype(np.float64))
    r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, r), r)            # rounded past the largest bf16
    return bits_of_bf16(np.where(np.isfinite(x32), r, x32.astype(np.float64)))


DEQUANT_EXPONENTS = (-20, -9, 0, 3, 8)
E4M3_NAN_CODES = (0x7f, 0xff)
