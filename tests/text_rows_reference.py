"""Plain fp64 statements of the decoder's text-row kernels (csrc/kernels.h and the kernel headers' comments), the per-element
error bounds that go with them, and the input generators of tests/test_text_rows_gpu.py (run on the CPU by tests/test_text_rows.py).

Nothing here imports the oracle or the library.  Operands are passed as float64 arrays that hold bf16 (or e4m3 x 2^k) values exactly.

Bounds.  u = 2^-24 (fp32), a bf16 value has 8 significant bits: rounding to bf16 moves a value by at most half a bf16 ulp.
  * fp32 GEMM accumulator over K products of bf16 operands (each product exact in fp32):  gamma(K) * sum_k |x_k| |w_k| with
    gamma(K) = K u / (1 - K u), the worst case of any summation order (the matrix core's order is not documented).
  * + bias: one more fp32 rounding, u |y|.
  * erf-GELU: the kernel's erf is Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 (common.h), so |d gelu| <= 0.5 |y| 1.5e-7 plus four
    fp32 roundings of the surrounding arithmetic (4 u |gelu| + 2 u |y|), plus the accumulator's error through |gelu'| <= 1.13.
  * bf16 output: half a bf16 ulp of the reference value on top.
  * LayerNorm in fp32 (rowln.h: two-pass, wave sums): see ln_bound.
"""
from __future__ import annotations

import math

import numpy as np

U32 = 2.0 ** -24


# ---- number formats ---------------------------------------------------------------------------------------------------------

def bf16_ulp(x):
    """Spacing of bf16 at |x| (2^-133 in the denormal range)."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(np.where(x > 0, x, 1.0))
    e = np.where(x > 0, e, -200)
    return np.ldexp(1.0, np.maximum(e - 8, -133))


def bf16_rne(x):
    """fp64 -> nearest bf16 value (ties to even), as fp64; one rounding, not through fp32."""
    x = np.asarray(x, np.float64)
    ulp = bf16_ulp(x)
    return np.rint(x / ulp) * ulp


def e4m3_encode(v):
    """OCP e4m3 code (uint8) of v, round to nearest even, |v| clamped at 448."""
    v = np.asarray(v, np.float64)
    a = np.minimum(np.abs(v), 448.0)
    _, e = np.frexp(np.where(a > 0, a, 1.0))
    e = np.maximum(e - 1, -6)                      # floor(log2 a), at least the smallest normal exponent
    q = np.rint(a / np.ldexp(1.0, e - 3))          # in units of the binade's spacing: 8..16 normal, 0..8 denormal
    code = np.where(a < 2.0 ** -6, q, (e + 7) * 8 + (q - 8)).astype(np.int64)      # q == 16 carries into the next exponent by itself
    code = np.where(a > 0, code, 0)
    return (code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def e4m3_decode(c):
    c = np.asarray(c).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, np.ldexp(1.0 + m / 8.0, e - 7))
    return np.where(c & 0x80, -mag, mag)


def quant_rows_e4m3(Wf):
    """Per-row power-of-two scale (smallest 2^e with amax <= 448 2^e) and codes of a weight matrix -> (codes uint8, scale, values)."""
    Wf = np.asarray(Wf, np.float64)
    amax = np.abs(Wf).max(axis=1)
    scale = np.exp2(np.ceil(np.log2(np.maximum(amax, 1e-30) / 448.0)))
    codes = e4m3_encode(Wf / scale[:, None])
    return codes, scale, e4m3_decode(codes) * scale[:, None]


# ---- layout kernels ------------------------------------------------------------------------------------------------------------

def pack_frags(src):
    """[rows16][K] -> flat [tile][k32][lane][8], lane = n % 16 + 16 * ((k % 32) / 8) (rowops.hip)."""
    src = np.asarray(src)
    R, K = src.shape
    assert R % 16 == 0 and K % 32 == 0
    t = src.reshape(R // 16, 16, K // 32, 4, 8)            # tile, n % 16, k32, (k % 32) / 8, k % 8
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1, 4)).reshape(-1)


def pack_frags_by_formula(src):
    """The same, element by element from the index formula (the hand check of pack_frags)."""
    src = np.asarray(src)
    R, K = src.shape
    out = np.empty(R * K, src.dtype)
    for n in range(R):
        for k in range(K):
            lane = n % 16 + 16 * ((k % 32) // 8)
            out[(((n // 16) * (K // 32) + k // 32) * 64 + lane) * 8 + k % 8] = src[n, k]
    return out


def kv_quant_v(kv, D, H, pitch):
    """V slice (columns 2D..3D) of kv [rows][3D] -> codes uint8 [H][pitch][64], scales [H][pitch], written mask [H][pitch].
    Per (row, head): scale = the smallest 2^e, e >= -126, with amax <= 448 2^e; an all-zero group has scale 1 (rowops.hip: the
    kernel starts from scale = 1 and only a positive amax changes it) and codes 0.  Rows >= rows are not written."""
    kv = np.asarray(kv, np.float64)
    rows = kv.shape[0]
    v = kv[:, 2 * D:3 * D].reshape(rows, H, 64)
    amax = np.abs(v).max(axis=2)
    e = np.ceil(np.log2(np.where(amax > 0, amax, 1.0) / 448.0))
    scale = np.where(amax > 0, np.exp2(np.maximum(e, -126.0)), 1.0)
    codes = np.zeros((H, pitch, 64), np.uint8)
    scales = np.zeros((H, pitch))
    written = np.zeros((H, pitch), bool)
    codes[:, :rows] = e4m3_encode(v / scale[:, :, None]).transpose(1, 0, 2)
    scales[:, :rows] = scale.T
    written[:, :rows] = True
    return codes, scales, written


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------

def gamma(K):
    return K * U32 / (1 - K * U32)


_erf = np.vectorize(math.erf)


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def quick_gelu(x):
    return x / (1.0 + np.exp(-1.702 * x))


def layernorm(x, g, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def ln_bound(slab_terms, tail_terms, g, b, eps, depth=None, sum_depth=None):
    """Bound on |LN_fp32 - LN_fp64| for rows x = sum(slab_terms) + sum(tail_terms) (exact fp32 inputs, broadcastable to [M][D]).
    e_in follows the documented summation order (rowln.h): slabs in trees of 8 (3 adds deep), the group sums in ascending order
    (ngroups adds), each rounding at most u x the sum of the magnitudes below it; the two tail terms (bias + residual, or word +
    position) are added to each other (u sum|tail|) and then to the slab sum (u |x|).  Mean: a lane sum + wave butterfly of D
    values, (log2 D + 3) u mean|x|, plus mean(e_in).  Each centred value is then off by dx = e_in + e_mean + u |x - mu|; rstd inherits
    max(dx) / sigma relative plus (log2 D + 6) u for its own sum, division and rsqrt.  y = (x - mu) rstd g + b: three more roundings.
    depth / sum_depth replace the two counts for another order (txt_block: the H partials one after the other, depth H; a row sum
    of 6 butterfly steps and 16 wave sums in order, sum_depth 22)."""
    terms = list(slab_terms) + list(tail_terms)
    x = sum(np.asarray(t, np.float64) for t in terms)
    D = x.shape[-1]
    depth = 3 + (len(slab_terms) + 7) // 8 if depth is None else depth
    sum_depth = math.log2(D) + 3 if sum_depth is None else sum_depth
    e_in = 0 * x + U32 * sum(np.abs(np.asarray(t, np.float64)) for t in tail_terms) + U32 * np.abs(x)
    if slab_terms:
        e_in = e_in + depth * U32 * sum(np.abs(np.asarray(t, np.float64)) for t in slab_terms)
    mu = x.mean(axis=-1, keepdims=True)
    e_mu = sum_depth * U32 * np.abs(x).mean(axis=-1, keepdims=True) + e_in.mean(axis=-1, keepdims=True)
    sig = np.sqrt(((x - mu) ** 2).mean(axis=-1, keepdims=True) + eps)
    dx = e_in + e_mu + U32 * np.abs(x - mu)
    rel = dx.max(axis=-1, keepdims=True) / sig + (sum_depth + 3) * U32
    y = layernorm(x, g, b, eps)
    return np.abs(g) * (dx / sig + np.abs(x - mu) / sig * (rel + 3 * U32)) + U32 * (np.abs(y) + np.abs(b))


def orow(m, T, row_stride, row_off):
    return (m // T) * row_stride + row_off + m % T


def skinny(X, W, wscale, bias, N, epi, gelu_fn=gelu):
    """y[m][n] = epi(X W^T * wscale + bias), n < N, and the bound on |device_bf16 - y| (module docstring).  epi 0 / 1 / 2."""
    X = np.asarray(X, np.float64)
    Wv = np.asarray(W, np.float64)[:N] * (1.0 if wscale is None else np.asarray(wscale, np.float64)[:N, None])
    K = X.shape[1]
    acc = X @ Wv.T
    y = acc + (0.0 if bias is None else np.asarray(bias, np.float64)[:N])
    e = gamma(K) * (np.abs(X) @ np.abs(Wv).T) + U32 * np.abs(y)
    if epi == 1:
        out = gelu_fn(y)
        e = 1.13 * e + 0.5 * np.abs(y) * 1.5e-7 + 4 * U32 * np.abs(out) + 2 * U32 * np.abs(y)
    elif epi == 2:
        out = np.maximum(y, 0.0)
    else:
        out = y
    return out, e + 0.5 * bf16_ulp(out)


def scatter_rows(y, T, row_stride, row_off, n_rows, fill=np.nan):
    """Rows of y placed at orow(m) of an [n_rows][N] array filled with `fill`."""
    out = np.full((n_rows, y.shape[1]), fill)
    for m in range(y.shape[0]):
        out[orow(m, T, row_stride, row_off)] = y[m]
    return out


def prologue_rows(kind, *, slabs=None, bias=None, resid=None, ids=None, T=1, t0=0, word=None, pos=None, g=None, b=None, eps=1e-5,
                  nslab=None):
    """The fp64 rows of the row prologue and their bound.  kind 1: LN(sum_s slab[s] + bias + resid); kind 2: LN(word[id] +
    pos[t0 + j]) with id clamped into the table (rowln.h: row_load_embed_tok -- never an index outside it)."""
    if kind == 1:
        ns = slabs.shape[0] if nslab is None else nslab
        st, tt = [slabs[s] for s in range(ns)], [bias[None, :], resid]
    else:
        ids = np.asarray(ids)
        rows = []
        for r in range(ids.shape[0]):
            for j in range(T):
                tok = min(max(int(ids[r, j]), 0), word.shape[0] - 1)
                rows.append((word[tok], pos[t0 + j]))
        st, tt = [], [np.stack([w for w, _ in rows]), np.stack([p for _, p in rows])]
    x = sum(np.asarray(t, np.float64) for t in st + tt)
    return layernorm(x, g, b, eps), ln_bound(st, tt, g, b, eps)


def splitk(X, W, wscale, N, ksplit):
    """slab[s][m][n] = X[m][s Ks:(s+1) Ks] . W[n][the same] * wscale[n] and the fp32 accumulator bound."""
    X = np.asarray(X, np.float64)
    Wv = np.asarray(W, np.float64)[:N] * (1.0 if wscale is None else np.asarray(wscale, np.float64)[:N, None])
    K = X.shape[1]
    Ks = K // ksplit
    out = np.stack([X[:, s * Ks:(s + 1) * Ks] @ Wv[:, s * Ks:(s + 1) * Ks].T for s in range(ksplit)])
    bnd = np.stack([gamma(Ks) * (np.abs(X[:, s * Ks:(s + 1) * Ks]) @ np.abs(Wv[:, s * Ks:(s + 1) * Ks]).T) for s in range(ksplit)])
    return out, bnd


def ln_reduce(slabs, bias, resid, g, b, eps, nslab=None):
    return prologue_rows(1, slabs=slabs, bias=bias, resid=resid, g=g, b=b, eps=eps, nslab=nslab)


def ffn_txt(X, W1, s1, b1, W2, s2, h=None, gelu_fn=gelu, nslab=None):
    """h = bf16(GELU(X W1^T + b1)) (rounded where the FC1 launch rounds), slab[s] = h[:, 64 s:64 s+64] . W2[:, the same]^T.
    -> (h64 unrounded, bound on |h_bf16 - h64|, slabs from `h` (default: bf16_rne(h64)), bound on the slabs given that h)."""
    F = np.asarray(W1).shape[0]
    D = np.asarray(W2).shape[0]
    h64, hb = skinny(X, W1, s1, b1, F, 1, gelu_fn)
    hq = bf16_rne(h64) if h is None else np.asarray(h, np.float64)
    slabs, sb = splitk(hq, W2, s2, D, F // 64)
    if nslab is not None:
        slabs, sb = slabs[:nslab], sb[:nslab]
    return h64, hb, slabs, sb


# ---- txt_block -------------------------------------------------------------------------------------------------------------------

# The fp32 softmax / v_exp_f32 term of the context.  It cannot be derived from the sources: it is the largest |ctx_device - ctx64|
# over TXT_CASES on an MI355X, recovered from `part` with identity slices for Wo (profiles/r11_text_row_kernels.txt has the run).
# delta = 4 x that value, capped per element at a quarter of a bf16 ulp of the context value it sits beside.
# The measurement is taken behind the context's bf16 rounding (that is all `part` shows), so it contains that rounding's half ulp and
# 4 x it exceeds the cap wherever |ctx| < 32: on these inputs delta is the cap.  Beside the rounding the run left 5.1e-5.
DELTA_MEASURED = 0.0156758


def txt_delta(ctx64):
    return np.minimum(4.0 * DELTA_MEASURED, 0.25 * bf16_ulp(ctx64))


def txt_block(q, variant=None, emulate=False):
    """The attention sub-layer of M = rows * T text rows (kernels.h: TxtBlockArgs; txtblock.hip).  q = txt_block_inputs(...).
    Query m = (r, j), position tq = t0 + j, reads q from kv_txt[r][tq][0:D]; it attends the image keys of clip r / beams (rows
    clip * S .. clip * S + S - 1 of kv_img; k at D..2D, v at 2D..3D, or v_img = code * scale where the image V is e4m3) and the
    text keys 0..tq of row r; scale 1/8; ctx is rounded to bf16; part[m][h] = ctx_h . Wo[:, 64 h:64 h + 64]^T (Wo holds the
    values, e4m3 x aoscale included); x1 = LN(sum_h part + aob + xin).
    -> dict(ctx [M][H][64] unrounded, part [M][H][D], bound on |part_device - part|, x1 [M][D]).
    Bound on a context element: the kernel's documented rounding points are P (bf16 in the PV product, while the normaliser sums
    the fp32 P: at most 2^-8 sum_k p_k |v_kd|) and the context itself (2^-8 |ctx| -- half a bf16 ulp -- on whichever side of a
    boundary the fp32 value lands), and txt_delta for the fp32 arithmetic in front of them.  With e the error in front of the last
    rounding, |bf16(c + e) - c| <= |e| + 2^-8 |c + e| <= 2^-8 |c| + (1 + 2^-8) |e|: the P and delta terms carry that factor.
    part: |Wo_h| times that, plus the fp32 accumulator of the 64 products, gamma(64) |Wo_h| |ctx|.
    variant: one subtly wrong kernel -- 'causal' (keys 0..tq-1), 'last_img' (the last image key dropped), 'clip' (clip r instead
    of r / beams), 'swap' (the part slots of heads 0 and 1 exchanged).
    emulate: the same operation in fp32 with the bf16 rounding of P (an fp32 implementation, not the device's order)."""
    D, H, S, T, t0, beams, rows = q["D"], q["H"], q["S_img"], q["T"], q["t0"], q["beams"], q["rows"]
    ft = np.float32 if emulate else np.float64
    kv_img, kv_txt = q["kv_img"], q["kv_txt"]
    v_img = q["v_img"] if q.get("v_img") is not None else kv_img[:, 2 * D:]
    Wo = np.asarray(q["Wo"], np.float64)
    M = rows * T
    ctx = np.zeros((M, H, 64))
    A = np.zeros((M, H, 64))
    for m in range(M):
        r, j = divmod(m, T)
        tq = t0 + j
        clip = r if variant == "clip" else r // beams
        ni = S - 1 if variant == "last_img" else S
        nt = tq if variant == "causal" else tq + 1
        for h in range(H):
            c = slice(h * 64, h * 64 + 64)
            qv = kv_txt[r, tq, :D][c].astype(ft)
            K = np.concatenate([kv_img[clip * S:clip * S + ni, D:2 * D][:, c], kv_txt[r, :nt, D:2 * D][:, c]]).astype(ft)
            V = np.concatenate([v_img[clip * S:clip * S + ni][:, c], kv_txt[r, :nt, 2 * D:][:, c]]).astype(ft)
            sc = (K @ qv) * ft(0.125)
            p = np.exp(sc - sc.max())
            pv = bf16_rne(p.astype(np.float64)).astype(ft) if emulate else p
            ctx[m, h] = (pv @ V) / p.sum(dtype=ft)
            A[m, h] = (p.astype(np.float64) @ np.abs(V.astype(np.float64))) / float(p.sum())
    cb = bf16_rne(ctx)
    Wh = Wo.reshape(D, H, 64).transpose(1, 0, 2)                                   # [H][D][64]
    part = np.einsum("mhd,hnd->mhn", cb, Wh)
    if emulate:
        part = np.einsum("mhd,hnd->mhn", cb.astype(np.float32), Wh.astype(np.float32)).astype(np.float64)
    cbound = 2.0 ** -8 * np.abs(ctx) + (1 + 2.0 ** -8) * (2.0 ** -8 * A + txt_delta(ctx))
    bound = np.einsum("mhd,hnd->mhn", cbound + gamma(64) * np.abs(ctx), np.abs(Wh))
    if variant == "swap":
        part = part[:, [1, 0] + list(range(2, H))]
    x1 = layernorm(part.sum(axis=1) + q["aob"] + q["xin"], q["g1"], q["b1"], q["eps"])
    return dict(ctx=ctx, part=part, bound=bound, x1=x1)


def txt_x1(part_dev, q):
    """x1 from the device's own partials: the exact LayerNorm of sum_h part + aob + xin and the bound of the fp32 reducer (the H
    partials are added one after the other, then (aob + xin))."""
    H = part_dev.shape[1]
    st = [part_dev[:, h] for h in range(H)]
    tt = [q["aob"][None, :], q["xin"]]
    x = sum(st) + q["aob"] + q["xin"]
    return layernorm(x, q["g1"], q["b1"], q["eps"]), ln_bound(st, tt, q["g1"], q["b1"], q["eps"], depth=H, sum_depth=22)


TXT_CASES = [
    # (D, rows, beams, T, t0, S_img, e4m3 output dense, e4m3 image V, kind).  S_img: 32-key groups are dealt to 16 virtual waves --
    # 1 / 31 / 32 / 33 (waves without a group, one group, one key into the next), 511 / 512 / 513 (one round, one key into the
    # second), 1182 (three rounds); t0 0 / 1 / 30 / 31 / 32 (the text keys cross a group edge); H 12 with M 1, 2, 3, 5 (6) and
    # beams 1 / 3 (the split of heads 8..11 into halves of whole clips)
    (128, 1, 1, 1, 0, 1, False, False, "n"), (128, 2, 1, 1, 1, 31, True, False, "n"), (128, 3, 3, 1, 30, 32, False, True, "n"),
    (128, 5, 1, 1, 31, 33, True, True, "n"), (128, 2, 1, 5, 0, 511, False, False, "n"), (128, 1, 1, 5, 29, 513, False, True, "n"),
    (768, 1, 1, 1, 0, 512, False, False, "n"), (768, 2, 1, 1, 32, 513, True, False, "n"), (768, 3, 3, 1, 1, 33, False, True, "n"),
    (768, 5, 1, 1, 31, 31, False, False, "n"), (768, 6, 3, 1, 30, 511, True, True, "n"), (768, 1, 1, 5, 0, 1, False, False, "n"),
    (768, 1, 1, 5, 29, 32, True, False, "n"), (768, 1, 1, 1, 2, 1182, False, True, "n"),
    (768, 3, 1, 1, 5, 33, False, False, "peak_img"), (768, 3, 1, 1, 5, 33, False, False, "peak_txt"),
    (128, 2, 1, 1, 1, 2, False, False, "equal")]


def txt_block_inputs(D, rows, beams, T, t0, S, fp8, v8, kind, seed, identity=False):
    """bf16 operands of one launch.  Scores are n(0, 1) but for two keys per query: the last image key of its clip and the text
    key at its own position score cI / cX higher (6: peaked but finite, each a few per cent to a third of the mass), and their V
    rows are large (4) and differ by key, so that a kernel that drops one of them, or reads another clip, moves the context far
    more than it is rounded.  kind 'peak_img' / 'peak_txt': that key scores 12 and holds almost all the mass, the other one 8
    with a V of 32; 'equal': q = 0, every score equal.  Every row has image keys of its own (`rows` clips, the launch uses
    rows / beams of them): clip r instead of r / beams reads other data, never outside.  Wo is 'diagonal' in every 64-block
    (column 64 h + d feeds outputs n = d mod 64, with a weight that depends on n and h) plus small noise, so that part shows the
    context undiluted; identity: exactly the identity slices (the delta measurement).  Unused cache rows and q slots are NaN."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    H, Tmax = D // 64, t0 + T + 2
    cI, cX, vI, vX = {"n": (6, 6, 4, 4), "equal": (6, 6, 4, 4), "peak_img": (12, 8, 1, 32), "peak_txt": (8, 12, 32, 1)}[kind]
    kv_img = rng.standard_normal((rows * S, 3 * D))
    kv_img[:, :D] = np.nan
    kv_txt = np.full((rows, Tmax, 3 * D), np.nan)
    kv_txt[:, :t0 + T, D:] = rng.standard_normal((rows, t0 + T, 2 * D))
    qq = bf16_rne(rng.standard_normal((rows, T, D))) * (0.0 if kind == "equal" else 1.0)
    kv_txt[:, t0:t0 + T, :D] = qq
    d = np.arange(64)
    for r in range(rows):
        members = [r] if r * beams >= rows else list(range(r * beams, min(rows, r * beams + beams)))   # the rows clip r serves
        for h in range(H):
            c = slice(h * 64, h * 64 + 64)
            Q = np.concatenate([qq[x, :, c] for x in members])
            if kind != "equal":
                kv_img[r * S + S - 1, D + h * 64:D + h * 64 + 64] = np.linalg.pinv(Q) @ np.full(Q.shape[0], 8.0 * cI)
            kv_img[r * S + S - 1, 2 * D + h * 64:2 * D + h * 64 + 64] = vI * np.where((d + h + r) % 3 == 0, -1.0, 1.0)
            for j in range(T):
                qv = qq[r, j, c]
                if kind != "equal":
                    kv_txt[r, t0 + j, D + h * 64:D + h * 64 + 64] += 8.0 * cX * qv / (qv @ qv)
                kv_txt[r, t0 + j, 2 * D + h * 64:2 * D + h * 64 + 64] = vX * np.where((d + 2 * h + r + j) % 4 < 2, -1.0, 1.0) * (1 + 0.25 * (j % 3))
    kv_img, kv_txt = bf16_rne(kv_img), bf16_rne(kv_txt)
    n = np.arange(D)
    Wf = np.zeros((D, D))
    for h in range(H):
        Wf[n, h * 64 + n % 64] = 1.0 if identity else (1.0 + 0.5 * np.sin(n + 3.0 * h)) * np.where((n // 64 + h) % 2, -1.0, 1.0)
    if not identity:
        Wf += 0.02 * rng.standard_normal((D, D)) * (Wf == 0)
    if fp8:
        codes, scale, Wv = quant_rows_e4m3(Wf)
        out = dict(Wo=Wv, Wcodes=codes, aoscale=scale)
    else:
        out = dict(Wo=bf16_rne(Wf), Wcodes=None, aoscale=None)
    pitch = rows * S + 3
    if v8:
        codes, scales, _ = kv_quant_v(kv_img, D, H, pitch)
        vals = e4m3_decode(codes[:, :rows * S]) * scales[:, :rows * S, None]               # [H][keys][64]
        out.update(v8=codes, vs=scales, v_img=vals.transpose(1, 0, 2).reshape(rows * S, D))
    else:
        out.update(v8=None, vs=None, v_img=None)
    out.update(D=D, H=H, rows=rows, beams=beams, T=T, t0=t0, Tmax=Tmax, S_img=S, pitch=pitch, kv_img=kv_img, kv_txt=kv_txt,
               aob=f32(np.linspace(-1, 1, D) + 0.1 * rng.standard_normal(D)), xin=f32(rng.standard_normal((rows * T, D))),
               g1=f32(1.0 + 0.5 * np.sin(n)), b1=f32(0.3 * np.cos(n * 0.7)), eps=1e-5)
    return out


def txt_variants(D, rows, beams, T, t0, S, fp8, v8, kind):
    """The wrong variants a case can tell apart at all: another clip needs beams > 1 and a second row."""
    return ["causal", "last_img", "swap"] + (["clip"] if beams > 1 and rows > 1 else [])


# ---- fp32 emulation of the same ops (boundary-flip share on the CPU) -------------------------------------------------------------

def skinny_fp32(X, W, wscale, bias, N, epi):
    """The same op with a sequential-k fp32 accumulator (numpy float32): an fp32 implementation, not the device's order."""
    X32 = np.asarray(X, np.float32)
    Wv = (np.asarray(W, np.float64)[:N] * (1.0 if wscale is None else np.asarray(wscale, np.float64)[:N, None])).astype(np.float32)
    acc = np.zeros((X32.shape[0], N), np.float32)
    for k0 in range(0, X32.shape[1], 32):
        acc = acc + X32[:, k0:k0 + 32] @ Wv[:, k0:k0 + 32].T
    y = acc + (np.float32(0) if bias is None else np.asarray(bias, np.float32)[:N])
    if epi == 1:
        y = gelu(y.astype(np.float64)).astype(np.float32)
    elif epi == 2:
        y = np.maximum(y, np.float32(0))
    return bf16_rne(y.astype(np.float64))


def flip_share(dev_bf16, ref64):
    """Share of elements that differ from the correctly rounded reference at all."""
    return float(np.mean(np.asarray(dev_bf16, np.float64) != bf16_rne(ref64)))


# ---- input generators (shared by the CPU and the device tests) ------------------------------------------------------------------------

def _bf(a):
    return bf16_rne(a)


def gemm_inputs(M, N, K, fp8, seed, guard=True):
    """X [M][K] bf16 values, W [Npad16][K] (bf16 values, or e4m3 codes + scale), bias [N] that depends on n.  Padded weight rows
    n >= N are 8 x a row of X: without the n < N guard they would store a huge value (and, unguarded, behind the row)."""
    rng = np.random.default_rng(seed)
    Np = (N + 15) // 16 * 16
    X = _bf(rng.standard_normal((M, K)))
    Wf = rng.standard_normal((Np, K)) * (1.0 / math.sqrt(K))
    if guard:
        for n in range(N, Np):
            Wf[n] = 8.0 * X[n % M]
    bias = np.linspace(-1.5, 1.5, N) + 0.25 * rng.standard_normal(N)
    bias = bias.astype(np.float32).astype(np.float64)
    if fp8:
        codes, scale, Wv = quant_rows_e4m3(Wf)
        return dict(X=X, W=Wv / scale[:, None], Wcodes=codes, wscale=scale, bias=bias)
    return dict(X=X, W=_bf(Wf), Wcodes=None, wscale=None, bias=bias)


SKINNY_CASES = (
    # (M, N, K, fp8, epi, T, row_stride, row_off): every instantiated depth, N 16 / 48 / 2304 and ragged N, M 1 .. 33, three epilogues,
    # and scatters into a [R][Tmax][3D] cache (T rows per text row at row_off of a row_stride-row block)
    [(1, 16, 64, False, 0, 1, 1, 0), (2, 48, 128, False, 1, 1, 1, 0), (16, 2304, 256, False, 2, 1, 1, 0),
     (17, 40, 576, False, 0, 1, 1, 0), (33, 2304, 768, False, 0, 3, 8, 2), (17, 21, 1024, False, 1, 1, 5, 3),
     (33, 48, 64, False, 2, 11, 16, 4), (2, 2304, 768, False, 1, 2, 6, 1), (1, 13, 768, False, 0, 1, 4, 3),
     (16, 16, 1024, False, 2, 4, 9, 5), (17, 128, 128, True, 0, 1, 1, 0), (33, 768, 768, True, 1, 3, 7, 1),
     (2, 120, 768, True, 2, 1, 3, 2), (1, 768, 128, True, 0, 1, 2, 1)])

SPLITK_CASES = (
    # (M, N, K, ksplit (0 = default), fp8): per-slab depths 1, 2, 6, 8, 12 x 32 (e4m3 1, 2, 12)
    [(1, 16, 32, 1, False), (15, 48, 64, 1, False), (16, 32, 768, 0, False), (17, 768, 1024, 4, False), (17, 128, 3072, 8, False),
     (1, 128, 128, 2, False), (16, 16, 576, 3, False), (15, 128, 3072, 48, False), (17, 48, 128, 4, True), (1, 128, 128, 2, True),
     (16, 768, 3072, 0, True), (15, 16, 768, 2, True)])
# The launcher's default number of slabs (ksplit 0) at the two widths the decoder has, the only place the tests restate it: the
# output dense (K = 768: four slabs of 6 x 32) and FC2 (K = 3072: eight slabs of 12 x 32).  Every other case passes ksplit itself.
DEFAULT_KSPLIT = {768: 4, 3072: 8}

LN_CASES = [(1, 128, 1), (5, 576, 8), (1, 768, 9), (5, 1024, 48), (5, 768, 64), (1, 1024, 64), (5, 128, 9), (1, 576, 48)]   # (M, D, nslab)

FFN_CASES = [(1, 128, 64, False), (2, 128, 128, True), (16, 768, 64, False), (17, 768, 128, False), (33, 128, 3072, False),
             (48, 768, 3072, False), (33, 768, 3072, True), (48, 128, 128, True), (2, 768, 128, True), (16, 128, 3072, True)]
# (M, D, F, fp8): one tile, the pair loop (32 < M) and its odd tail (M = 33 .. 48: three tiles)

PROLOGUE_CASES = [(1, 64, 1, 3), (2, 128, 1, 17), (1, 576, 1, 48), (2, 768, 1, 32), (1, 768, 1, 16), (2, 64, 2, 0), (1, 128, 2, 0),
                  (2, 576, 2, 0), (1, 768, 2, 0)]   # (M, K, kind, nslab)


def ln_inputs(M, D, nslab, seed, hard_row=True):
    """Slabs that partly cancel, a bias and gamma / beta that depend on the column; row 0 (hard_row) has a large mean and a small
    variance: its slabs are 100 x smaller and the residual is 300 + 0.05 n(0, 1)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    slabs = f32(rng.standard_normal((nslab, M, D)) * (1.0 + np.arange(nslab)[:, None, None] % 3))
    bias = f32(np.linspace(-1, 1, D) + 0.1 * rng.standard_normal(D))
    resid = f32(rng.standard_normal((M, D)))
    if hard_row:
        slabs[:, 0, :] *= 1e-2
        resid[0] = f32(300.0 + 0.05 * rng.standard_normal(D))
    g = f32(1.0 + 0.5 * np.sin(np.arange(D)))
    b = f32(0.3 * np.cos(np.arange(D) * 0.7))
    return dict(slabs=slabs, bias=bias, resid=resid, g=g, b=b, eps=1e-5)


def embed_inputs(M, D, seed, vocab=50, T=1, t0=3):
    """ids [rows][T] with an id at vocab - 1, and (rows > 1 or T > 1) one outside the vocabulary, which the kernel clamps."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    word = f32(rng.standard_normal((vocab, D)))
    pos = f32(0.5 * rng.standard_normal((t0 + T + 2, D)))
    ids = rng.integers(0, vocab, size=(M // T, T)).astype(np.int64)
    ids.flat[0] = vocab - 1
    if ids.size > 1:
        ids.flat[1] = vocab + 7
    g = f32(1.0 + 0.5 * np.sin(np.arange(D)))
    b = f32(0.3 * np.cos(np.arange(D) * 0.7))
    return dict(ids=ids, word=word, pos=pos, g=g, b=b, eps=1e-5, T=T, t0=t0, vocab=vocab)


def ffn_inputs(M, D, F, fp8, seed):
    rng = np.random.default_rng(seed)
    a = gemm_inputs(M, F, D, fp8, seed, guard=False)
    W2f = rng.standard_normal((D, F)) * (1.0 / 8.0) * (1.0 + (np.arange(F)[None, :] // 64) % 4)       # slices of different weight
    if fp8:
        c2, s2, v2 = quant_rows_e4m3(W2f)
        a.update(W2=v2 / s2[:, None], W2codes=c2, w2scale=s2)
    else:
        a.update(W2=_bf(W2f), W2codes=None, w2scale=None)
    return a


def kv_quant_inputs(rows, D, H, seed):
    """V groups with the edges of the scale rule: amax exactly 448 2^e, one bf16 step below and above it, a zero group, a group of
    small normals (amax 2^-120: its scale would need an exponent below fp32's) and one of bf16 denormals."""
    rng = np.random.default_rng(seed)
    kv = _bf(rng.standard_normal((rows, 3 * D)) * np.exp2(rng.integers(-6, 6, size=(rows, 1))))
    v = kv[:, 2 * D:].reshape(rows, H, 64)
    edges = [("on", 448.0 * 2.0 ** -5), ("below", 446.0 * 2.0 ** -5), ("above", 450.0 * 2.0 ** -5), ("binade", 224.0 * 2.0 ** 3),
             ("zero", 0.0), ("tiny", 2.0 ** -120), ("denormal", 3 * 2.0 ** -130)]
    for i, (_, amax) in enumerate(edges):
        r, h = i % rows, (i // rows) % H
        if amax == 0.0:
            v[r, h] = 0.0
            continue
        grp = _bf(rng.uniform(-1, 1, 64) * amax * 0.99)
        grp = np.where(np.abs(grp) > amax, amax, grp)
        grp[(7 * i) % 64] = -amax if i % 2 else amax
        v[r, h] = grp
    kv[:, 2 * D:] = v.reshape(rows, D)
    return kv
