"""fp64 restatement of the attention maps of csrc/attnmap.hip, the per-element bound, and the inputs of the device test.

Definitions.  Text row r belongs to clip c = r // rows_per_clip.  For layer l, head h and position j,
    p[l][h][r][j][.] = softmax( q . k / sqrt(64) )  over  (clip c's image keys ; the row's text keys 0 .. j)
with q and k the bf16 values of the caches: kv_txt [L][rows][Tmax][3 D] = q | k | v of the text rows, kv_img [L][img_rows][3 D].
The outputs are means over the heads and the selected layers (layer = -1: all):
    frame_mass [rows][T][Fmax]  mass on the N tokens of frame f, 0 for f >= the clip's frames
    text_mass  [rows][T]        mass on the text keys
    patch_map  [rows][T][Smax]  mean probability per image token, 0 beyond the clip's tokens
and positions j >= lengths[r] are zeros.

Bound (per element, absolute; u = 2^-24).  The kernel's rounding points:
  * the score: 64 products of bf16 pairs (exact in fp32) summed in fp32, |ds| <= gamma(64) A with A = sum_d |q_d k_d|; times
    c = log2(e) / 8 in fp32 (u |t|) and minus the row maximum (u |t - M|): the exponent's error e <= c (gamma(64) + 2u) A + u |t - M|,
    and |t - M| <= 2 c Amax.  The maximum itself cancels (numerator and sum use the same one).
  * exp2 turns e into a relative error ln2 e, of the numerator and (the worst key's) of the sum: 2 ln2 E, E = the row's largest e.
  * the sum over the keys: lane-local over ceil(tiles / 4) tiles, a 16-lane butterfly, four waves: gamma(ceil(tiles / 4) + 7); the
    division: u.
  * the mean: nl H additions in registers and one division: gamma(nl H + 1) on the mean.
  * the frame's mass: lane-local over ceil(N / 64) chunks, butterfly, waves: gamma(ceil(N / 64) + 7) on the mass.
  * the fast exp (v_exp_f32, error not specified): by the project's convention 4 x the error of an fp32 numpy restatement of the
    kernel's loop against fp64, measured on the CPU over the device test's inputs (DELTA_MEASURED; tests/test_attention_map.py
    recomputes it, profiles/r26_attention_map_bound.txt has the run), relative to the value, capped at a quarter of a bf16 ulp of
    the value as tests/encoder_kernels_reference.py caps it, so that it can never grow to hide a wrong key.
  * v_exp_f32 flushes results below 2^-126: an absolute 2^-120 covers every flushed term of a sum.
The row-sum bound (sum_f frame_mass + text_mass against 1) is the sum of the row's element bounds plus gamma(Fmax + 1) for the
test's own fp64 additions of fp32 values -- which are exact, so only the element bounds remain.
"""
import math

import numpy as np

from text_rows_reference import U32, bf16_rne, bf16_ulp, gamma

F32 = np.float32
C_LOG2 = 0.125 * 1.4426950408889634
# worst |fp32 restatement - fp64| / value over the device test's inputs (values >= 2^-100), measured on the CPU
DELTA_MEASURED = 7.0e-6

VARIANTS = ("no_scale", "future_key", "frame_off_by_one", "wrong_clip", "drop_head", "drop_layer", "wrong_count")


def clip_rows(case, c):
    """(first image row, image rows) of clip c"""
    if case.get("off") is not None:
        return int(case["off"][c]), int(case["len"][c])
    return c * case["S_img"], case["S_img"]


def _layers(case):
    return list(range(case["L"])) if case["layer"] < 0 else [case["layer"]]


def _qk(case, l, r, h, clip):
    """q [T][64], image keys [S][64] of `clip`, text keys [T][64] of (layer, row, head) as fp64"""
    D, T = case["D"], case["T"]
    row0, S = clip_rows(case, clip)
    txt = case["kv_txt"][l, r, :T].astype(np.float64)
    q, kt = txt[:, h * 64:h * 64 + 64], txt[:, D + h * 64:D + h * 64 + 64]
    ki = case["kv_img"][l, row0:row0 + S, D + h * 64:D + h * 64 + 64].astype(np.float64)
    return q, ki, kt


def maps_fp64(case, variant=None, want_bound=False):
    """-> frame_mass, text_mass, patch_map (fp64) [, their bounds].  variant: one of VARIANTS, a kernel that is wrong in that way."""
    L, H, rows, T, N, Smax = case["L"], case["H"], case["rows"], case["T"], case["N"], case["Smax"]
    Fmax = Smax // N if N else 0
    lengths = case.get("lengths")
    layers = _layers(case)
    if variant == "drop_layer":
        layers = layers[:-1] if len(layers) > 1 else layers
    heads = list(range(H - 1 if variant == "drop_head" else H))
    cnt = len(_layers(case)) * H if variant in ("drop_head", "drop_layer") else len(layers) * len(heads)
    if variant == "wrong_count":
        cnt = cnt + 1
    fm, tm, pm = np.zeros((rows, T, max(Fmax, 1))), np.zeros((rows, T)), np.zeros((rows, T, max(Smax, 1)))
    bp, bt = np.zeros_like(pm), np.zeros_like(tm)
    causal = np.arange(T)[None, :] <= np.arange(T)[:, None] + (1 if variant == "future_key" else 0)
    for r in range(rows):
        clip = r // case["rows_per_clip"]
        if variant == "wrong_clip":         # the clip a kernel that forgets rows_per_clip would take
            clip = min(r, rows // case["rows_per_clip"] - 1)
        len_r = T if lengths is None else int(np.clip(lengths[r], 0, T))
        S = clip_rows(case, clip)[1]
        for l in layers:
            for h in heads:
                q, ki, kt = _qk(case, l, r, h, clip)
                k = np.concatenate([ki, kt])
                s = q @ k.T
                A = np.abs(q) @ np.abs(k).T
                vis = np.concatenate([np.ones((T, S), bool), causal], axis=1)
                t = np.where(vis, s * (1.0 if variant == "no_scale" else 0.125), -np.inf)
                p = np.exp(t - t.max(axis=1, keepdims=True))
                p = p / p.sum(axis=1, keepdims=True)
                p[len_r:] = 0.0
                pm[r, :, :S] += p[:, :S]
                tm[r] += p[:, S:].sum(axis=1)
                if want_bound:
                    Amax = np.where(vis, A, 0.0).max(axis=1, keepdims=True)
                    E = C_LOG2 * (gamma(64) + 2 * U32) * Amax + U32 * 2 * C_LOG2 * Amax
                    tiles = (S + 15) // 16 + (T + 15) // 16
                    rel = 2 * math.log(2.0) * E + gamma((tiles + 3) // 4 + 7) + U32
                    bp[r, :, :S] += p[:, :S] * rel
                    bt[r] += (p[:, S:] * rel).sum(axis=1)
    pm /= cnt
    tm /= cnt
    shift = 1 if variant == "frame_off_by_one" else 0
    for r in range(rows):
        S = clip_rows(case, r // case["rows_per_clip"])[1]
        for f in range(S // N if N else 0):
            fm[r, :, f] = pm[r, :, f * N + shift:min((f + 1) * N + shift, S)].sum(axis=1)
    fm, pm = fm[:, :, :Fmax], pm[:, :, :Smax]
    if not want_bound:
        return fm, tm, pm
    nlh = len(layers) * len(heads)
    bp, bt = bp[:, :, :Smax] / cnt, bt / cnt

    def tail(v, b, extra):
        return b + v * (gamma(nlh + 1) + extra) + np.minimum(4.0 * DELTA_MEASURED * v, 0.25 * bf16_ulp(v)) + 2.0 ** -120
    bf = np.zeros_like(fm)
    for f in range(Fmax):
        bf[:, :, f] = bp[:, :, f * N:(f + 1) * N].sum(axis=2)
    g_frame = gamma((N + 63) // 64 + 7)
    g_text = gamma((min(T, 16) + 63) // 64 + 7)
    return fm, tm, pm, tail(fm, bf, g_frame), tail(tm, bt, g_text), tail(pm, bp, 0.0)


def _exp2_32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp2(np.asarray(x, F32).astype(np.float64)).astype(F32)


def maps_fp32(case):
    """The kernel's loop in fp32 numpy (exp2 correctly rounded here): the score summed over d in order, times c, the maximum, the
    sum of exp2 over the keys in order, exp2 / sum, the heads and layers added in order, one division, the frame's keys in order.
    -> frame_mass, text_mass, patch_map as fp64 arrays of fp32 values"""
    L, H, rows, T, N, Smax = case["L"], case["H"], case["rows"], case["T"], case["N"], case["Smax"]
    Fmax = Smax // N if N else 0
    lengths = case.get("lengths")
    layers = _layers(case)
    fm, tm, pm = np.zeros((rows, T, max(Fmax, 1)), F32), np.zeros((rows, T), F32), np.zeros((rows, T, max(Smax, 1)), F32)
    causal = np.arange(T)[None, :] <= np.arange(T)[:, None]
    for r in range(rows):
        len_r = T if lengths is None else int(np.clip(lengths[r], 0, T))
        S = clip_rows(case, r // case["rows_per_clip"])[1]
        acc = np.zeros((T, S + T), F32)
        for l in layers:
            for h in range(H):
                q, ki, kt = _qk(case, l, r, h, r // case["rows_per_clip"])
                q, k = q.astype(F32), np.concatenate([ki, kt]).astype(F32)
                s = np.zeros((T, S + T), F32)
                for d in range(64):
                    s = s + q[:, d, None] * k[None, :, d]
                vis = np.concatenate([np.ones((T, S), bool), causal], axis=1)
                t = np.where(vis, s * F32(C_LOG2), F32(-np.inf)).astype(F32)
                e = _exp2_32(t - t.max(axis=1, keepdims=True))
                ssum = np.zeros(T, F32)
                for i in range(S + T):
                    ssum = ssum + e[:, i]
                acc = acc + e / ssum[:, None]
        acc = acc / F32(len(layers) * H)
        acc[len_r:] = 0
        pm[r, :, :S] = acc[:, :S]
        for i in range(T):
            tm[r] = tm[r] + acc[:, S + i]
        for f in range(S // N if N else 0):
            for i in range(N):
                fm[r, :, f] = fm[r, :, f] + acc[:, f * N + i]
    return fm[:, :, :Fmax].astype(np.float64), tm.astype(np.float64), pm[:, :, :Smax].astype(np.float64)


# ---- the inputs of the device test -----------------------------------------------------------------------------------------------

def make_case(name, L=2, H=2, rows=2, rows_per_clip=1, T=17, Tmax=20, N=197, frames=(3,), layer=-1, lengths=None, seed=0, special=None):
    """A caller-built cache: bf16 values (as fp32 arrays) of unit scale, NaN in every cell the kernels must not read -- text
    positions >= T, and (ragged: frames = one count per clip) a gap of NaN rows between the clips' image rows.
    special: 'dominant' (one image key of row 0 scores far above the rest, and the keys of the last frame far below: exp
    underflows), 'future' (text key j + 1 scores hugely for every j)."""
    rng = np.random.default_rng(seed)
    D = 64 * H
    clips = rows // rows_per_clip
    ragged = len(frames) > 1
    counts = list(frames) if ragged else [frames[0]] * clips
    assert len(counts) == clips
    Smax = max(counts) * N
    kv_txt = bf16_rne(rng.standard_normal((L, rows, Tmax, 3 * D))).astype(F32)
    if ragged:
        off, at = [], 3                             # NaN rows in front of, between and behind the clips
        for n in counts:
            off.append(at)
            at += n * N + 2
        img_rows = at
        ln = [n * N for n in counts]
    else:
        off = ln = None
        img_rows = clips * Smax
    kv_img = bf16_rne(rng.standard_normal((L, img_rows, 3 * D))).astype(F32)
    if special == "dominant":
        q0 = kv_txt[:, 0, :, :64]                   # head 0 of row 0: key 7 is 6 x q of position 2, the last frame's keys -8 x q
        row0 = off[0] if ragged else 0
        kv_img[:, row0 + 7, D:D + 64] = bf16_rne(6.0 * q0[:, 2])
        kv_txt[:, 0, :, :D] = bf16_rne(4.0 * kv_txt[:, 0, :, :D])
        kv_img[:, row0 + (counts[0] - 1) * N:row0 + counts[0] * N, D:2 * D] = bf16_rne(-8.0 * np.tile(kv_txt[:, 0, 2:3, :D], (1, N, 1)))
    if special == "future":                         # key j + 1 = 50 x q_j: a kernel that lets it in puts all mass there
        for j in range(T - 1):
            kv_txt[:, :, j + 1, D:2 * D] = bf16_rne(50.0 * kv_txt[:, :, j, :D])
    kv_txt[:, :, T:] = np.nan
    kv_txt[:, :, :, 2 * D:] = np.nan                # v is never read
    kv_img[:, :, :D] = np.nan                       # nor the image rows' q, nor their v
    kv_img[:, :, 2 * D:] = np.nan
    if ragged:
        keep = np.zeros(img_rows, bool)
        for o, n in zip(off, ln):
            keep[o:o + n] = True
        kv_img[:, ~keep] = np.nan
    return dict(name=name, L=L, H=H, D=D, rows=rows, rows_per_clip=rows_per_clip, T=T, Tmax=Tmax, N=N, S_img=0 if ragged else Smax,
                Smax=Smax, img_rows=img_rows, off=None if off is None else np.asarray(off, np.int32),
                len=None if ln is None else np.asarray(ln, np.int32), layer=layer,
                lengths=None if lengths is None else np.asarray(lengths, np.int32), kv_txt=kv_txt, kv_img=kv_img)


def device_cases():
    """The shapes of tests/test_attention_map_gpu.py: the smallest at which the kernels take another path."""
    return [
        make_case("N197_F3_T17", seed=1),                                                       # 13 key tiles, 2 position tiles
        make_case("N5_F1_T1_H1_L1", L=1, H=1, rows=1, T=1, Tmax=3, N=5, frames=(1,), seed=2),
        make_case("H12_layer0_T16_rpc2", H=12, rows=4, rows_per_clip=2, T=16, Tmax=16, N=5, layer=0, seed=3),
        make_case("layer1_F1_N197", rows=1, T=3, Tmax=8, frames=(1,), layer=1, seed=4),
        make_case("ragged_1_and_3_rpc2", rows=4, rows_per_clip=2, T=5, Tmax=6, N=5, frames=(1, 3), seed=5),
        make_case("ragged_N197", rows=2, T=2, Tmax=4, frames=(3, 1), seed=6),
        make_case("lengths_0_1_T", rows=3, T=17, Tmax=18, N=5, lengths=(0, 1, 17), seed=7),
        make_case("dominant_underflow", rows=2, T=4, Tmax=5, N=5, seed=8, special="dominant"),
        make_case("future_key", rows=2, T=17, Tmax=17, N=5, frames=(1,), seed=9, special="future"),
    ]


# ---- the student's read-out (student.hip: cross_probs_kernel, cross_mean_kernel) ---------------------------------------------------

# worst |fp32 restatement - fp64| / value of cross_case's inputs, measured on the CPU (tests/test_attention_map.py recomputes it)
DELTA_CROSS_MEASURED = 1.0e-6


def cross_case(F, rows=2, T=3, H=8, hd=72, lengths=None, seed=0):
    """q bf16 values [rows * T][H * hd], memory keys [rows][F][2 H hd] (k | v as the student lays them out; v is NaN: never read)"""
    rng = np.random.default_rng(seed)
    q = bf16_rne(rng.standard_normal((rows * T, H * hd))).astype(F32)
    kv = bf16_rne(rng.standard_normal((rows, F, 2 * H * hd))).astype(F32)
    kv[:, :, H * hd:] = np.nan
    return dict(F=F, rows=rows, T=T, H=H, hd=hd, q=q, kv=kv, lengths=None if lengths is None else np.asarray(lengths, np.int32))


def cross_fp64(c, variant=None):
    """-> probs [M][H][F], frame_mass [rows][T][F], and their bounds.  The kernel's rounding points: hd products summed in fp32
    (gamma(hd) A), times hd^-1/2 (rsqrt and the product: 2u |s|), minus the maximum (u |s - max| <= 2u Amax / sqrt(hd)), __expf (the
    measured term, capped as above), the 64-lane butterfly (gamma(6)) and the division (u); the mean: gamma(H + 1).
    variant 'no_scale' / 'next_row' (the memory of row r + 1) / 'drop_head': wrong kernels."""
    F, rows, T, H, hd = c["F"], c["rows"], c["T"], c["H"], c["hd"]
    q = c["q"].astype(np.float64).reshape(rows, T, H, hd)
    k = c["kv"][:, :, :H * hd].astype(np.float64).reshape(rows, F, H, hd)
    if variant == "next_row":
        k = np.roll(k, -1, axis=0)
    s = np.einsum("rthd,rfhd->rthf", q, k)
    A = np.einsum("rthd,rfhd->rthf", np.abs(q), np.abs(k))
    sc = 1.0 if variant == "no_scale" else 1.0 / math.sqrt(hd)
    e = np.exp(s * sc - (s * sc).max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    E = (gamma(hd) + 4 * U32) * A.max(-1, keepdims=True) / math.sqrt(hd)
    bp = p * (2 * E + gamma(6) + U32) + np.minimum(4.0 * DELTA_CROSS_MEASURED * p, 0.25 * bf16_ulp(p)) + 2.0 ** -120
    heads = H - 1 if variant == "drop_head" else H
    fm = p[:, :, :heads].sum(2) / H
    bf = bp.sum(2) / H + fm * gamma(H + 1)
    if c["lengths"] is not None:
        for r in range(rows):
            fm[r, int(c["lengths"][r]):] = 0
    return p.reshape(rows * T, H, F), fm, bp.reshape(rows * T, H, F), bf


def cross_fp32(c):
    """cross_probs_kernel's loop in fp32 numpy (exp correctly rounded): products summed over d in order, times fp32 hd^-1/2, the
    maximum, exp, the butterfly sum of 64 lanes, the division; the heads added in order and divided"""
    F, rows, T, H, hd = c["F"], c["rows"], c["T"], c["H"], c["hd"]
    q = c["q"].reshape(rows, T, H, hd)
    k = c["kv"][:, :, :H * hd].reshape(rows, F, H, hd)
    s = np.zeros((rows, T, H, F), F32)
    for d in range(hd):
        s = s + np.einsum("rth,rfh->rthf", q[..., d], k[..., d]).astype(F32)
    s = s * (F32(1.0) / np.sqrt(F32(hd)))
    e = np.exp((s - s.max(-1, keepdims=True)).astype(np.float64)).astype(F32)
    lanes = np.zeros((rows, T, H, 64), F32)
    lanes[..., :F] = e
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., np.arange(64) ^ o]
    p = e / lanes[..., :1]
    fm = np.zeros((rows, T, F), F32)
    for h in range(H):
        fm = fm + p[:, :, h]
    fm = fm / F32(H)
    return p.reshape(rows * T, H, F).astype(np.float64), fm.astype(np.float64)


def cross_cases():
    return [cross_case(1, seed=11), cross_case(6, seed=12, lengths=(0, 2)), cross_case(64, rows=1, T=2, seed=13)]


def case_from_oracle(cfg, weights, frames, ids):
    """The q and k that oracle/git_oracle.py's _attn sees (wrapped, not edited; bf16 emulation) in a full pass of `frames`
    [B, F, ...] and `ids` [B, T], as a case of maps_fp64: the model's own magnitudes for a bound on the device's maps."""
    import torch
    from oracle.git_oracle import GitOracle
    orc = GitOracle(cfg, weights, emulate_bf16=True)
    _, mem = orc.forward_image_enc(frames)
    seen, inner = [], orc._attn
    orc._attn = lambda q, k, v, klimit: (seen.append((q.double(), k.double())), inner(q, k, v, klimit))[1]
    orc.decoder_full(mem, ids)
    L, H, D = cfg.dec_layers, cfg.dec_heads, cfg.dec_width
    B, T, S = ids.shape[0], ids.shape[1], mem.shape[1]
    kv_txt, kv_img = np.zeros((L, B, T, 3 * D), F32), np.zeros((L, B * S, 3 * D), F32)
    for l, (q, k) in enumerate(seen):
        kv_txt[l, :, :, :D] = q[:, :, S:].transpose(1, 2).reshape(B, T, D).numpy()
        kv_txt[l, :, :, D:2 * D] = k[:, :, S:].transpose(1, 2).reshape(B, T, D).numpy()
        kv_img[l, :, D:2 * D] = k[:, :, :S].transpose(1, 2).reshape(B * S, D).numpy()
    return dict(name="oracle", L=L, H=H, D=D, rows=B, rows_per_clip=1, T=T, Tmax=T, N=S // frames.shape[1], S_img=S, Smax=S,
                img_rows=B * S, off=None, len=None, layer=-1, lengths=None, kv_txt=kv_txt, kv_img=kv_img)
