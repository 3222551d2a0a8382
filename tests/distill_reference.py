"""Plain numpy restatement, in fp64, of the teacher-student divergence pass (include/gitcap.h: gitcap_distill; csrc/skinny.hip:
skinny_head_dual_kernel, csrc/select.hip: distill_final_kernel / distill_rows_kernel), built on tests/logprob_reference.py.

With t = teacher logit / temperature and s = student logit / temperature, per 16-column tile of a row:
    t_max, t_idx, t_sum and s_max, s_idx, s_sum     logprob_reference.tile_partials of each model
    cross = sum exp(t - t_max) ((t - t_max) - (s - s_max))  over the columns with t > -inf; +inf where such a column has s = -inf;
                                                    0 for a tile whose t_max is -inf
and per row, with Mt = max t_max, Zt = sum t_sum e^(t_max - Mt) (the same for the student):
    C  = sum over the tiles with t_max > -inf of e^(t_max - Mt) (cross + t_sum ((t_max - Mt) - (s_max - Ms)))   (+inf tiles: +inf)
    kl = C / Zt - log Zt + log Zs;   0 for a row with Mt = -inf and for a position j >= lengths[r].
The given next token's log-probabilities follow score_reference (the same ignore rules); kl_loss = temperature^2 sum(kl) / B is
KLDivLoss('batchmean') * temperature^2 and ce_loss the mean of -student_lp over the targets != 0.

Error bound of kl (device fp32 against this restatement applied to the same fp32 logits).  The rounding points:
  - the fp32 accumulator and the bias add are in the logits both sides start from (bounded in tests/logprob_reference.py's users);
    the multiplication by 1 / temperature is exact for the powers of two the tests use;
  - the two logs: -log Zt and -log Zs are the merged log-sum-exps of tests/test_logprob_gpu.py, 2e-5 nats each (derived there:
    the exp arguments, the ~24-deep summation tree, the merge's rescale, v_exp_f32 / v_log_f32, times 4) -> 4e-5, which is also
    the kernel's clamp DISTILL_CLAMP: a negative kl no further from 0 than the logs alone can push it becomes 0;
  - C / Zt = sum_v p_v d_v with p the teacher's softmax and d_v = (t_v - Mt) - (s_v - Ms).  Every term is a weight times a
    log-domain magnitude; the kernel forms it as e^(t - t_max) ((t - t_max) - (s - s_max)) in the tile and shifts by
    t_sum ((t_max - Mt) - (s_max - Ms)) in the merge.  A relative error eps on a weight, a product or a partial sum moves C / Zt
    by at most eps G with
        G = sum_v p_v (|t_v - t_max| + |s_v - s_max|) + sum_tiles P_tile (|t_max - Mt| + |s_max - Ms|),
    the teacher-weighted magnitude of everything that is ever multiplied or added (P_tile = the tile's teacher mass).  The eps
    are: the fast exp (argument subtraction, the log2 e scaling, v_exp_f32: 2 * 2^-24 |x| + ~1 ulp per weight, twice: tile and
    merge), three subtractions per d, the products, 4 + 2 adds in the tile, up to ~10 in the merge tree, and the division --
    a few dozen 2^-24 in all.  That factor is not taken from the device: DELTA_MEASURED is the worst |C / Zt (fp32) - C / Zt
    (fp64)| / G of kl_fp32 below -- the kernel's loops in numpy fp32, __expf as exp2(x * log2 e) -- on every input of
    tests/test_distill_gpu.py (tests/test_distill.py recomputes it; profiles/r20_distill_bound.txt records it), and the bound
    takes it times 4, as profiles/r16_encoder_kernels.txt did.
  bound_kl = 4e-5 + 4 * DELTA_MEASURED * G.   (G >= |C / Zt|, so the bound is relative where kl is large.)

``wrong`` names one deliberately wrong variant (tests/test_distill.py shows the GPU tests' inputs tell each from the right one):
  "wrong_centre"   the cross term's student part centred on the TEACHER's tile maximum
  "no_recentre"    the merge forgets the tile shift t_sum ((t_max - Mt) - (s_max - Ms))
  "swapped"        teacher and student exchanged
  "drop_tail"      the ragged last tile left out
  "temp_one"       the temperature applied to the teacher only
"""
import numpy as np

import logprob_reference as L
import score_reference as S

TILE = L.TILE
TOL_LOG = 2e-5                    # one merged log-sum-exp (tests/test_logprob_gpu.py)
CLAMP = 2 * TOL_LOG               # csrc/kernels.h: DISTILL_CLAMP
DELTA_MEASURED = 3.0e-7           # worst |A32 - A64| / G of kl_fp32 over the GPU tests' inputs, rounded up (see the docstring)
K_REL = 4 * DELTA_MEASURED


def _tiles(x):
    x = np.asarray(x, dtype=np.float64)
    M, N = x.shape
    nt = (N + TILE - 1) // TILE
    p = np.full((M, nt * TILE), -np.inf)
    p[:, :N] = x
    return p.reshape(M, nt, TILE)


def dual_partials(t, s, wrong=None):
    """scaled logits t, s [M][N] -> dict of the seven partials [M][ntiles] (fp64 / int64) and absx, the tile's share of G."""
    if wrong == "swapped":
        t, s = s, t
    if wrong == "drop_tail":
        N = np.asarray(t).shape[1]
        if N % TILE and N > TILE:
            t, s = np.asarray(t)[:, :N // TILE * TILE], np.asarray(s)[:, :N // TILE * TILE]
    t_max, t_idx, t_sum = L.tile_partials(t)
    s_max, s_idx, s_sum = L.tile_partials(s)
    tp, sp = _tiles(t), _tiles(s)
    with np.errstate(invalid="ignore", over="ignore"):
        live = tp > -np.inf
        dt = np.where(live, tp - t_max[..., None], 0.0)
        e = np.where(live, np.exp(dt), 0.0)
        centre = t_max if wrong == "wrong_centre" else s_max
        ds = np.where(live & (sp > -np.inf), sp - centre[..., None], 0.0)
        term = np.where(live, np.where(sp == -np.inf, np.inf, e * (dt - ds)), 0.0)
        absx = np.where(live & (sp > -np.inf), e * (np.abs(dt) + np.abs(np.where(live & (sp > -np.inf), sp - s_max[..., None], 0.0))), 0.0)
    return dict(t_max=t_max, t_idx=t_idx, t_sum=t_sum, s_max=s_max, s_idx=s_idx, s_sum=s_sum, cross=term.sum(-1), absx=absx.sum(-1))


def merge(p, wrong=None):
    """the partials of dual_partials -> dict: kl [M], G [M] (the bound's magnitude), Mt, Ms, lzt = -log Zt, lzs, top1s."""
    t_max, s_max = np.asarray(p["t_max"], np.float64), np.asarray(p["s_max"], np.float64)
    t_sum, s_sum, cross = np.asarray(p["t_sum"], np.float64), np.asarray(p["s_sum"], np.float64), np.asarray(p["cross"], np.float64)
    M = t_max.shape[0]
    kl, G = np.zeros(M), np.zeros(M)
    Mt, Ms = t_max.max(-1), s_max.max(-1)
    lzt, lzs = np.full(M, -np.inf), np.full(M, -np.inf)
    t1, s1 = np.zeros(M, np.int64), np.zeros(M, np.int64)
    absx = p.get("absx")
    for m in range(M):
        t1[m], lzt[m] = L.merge(t_max[m], p["t_idx"][m], t_sum[m])
        s1[m], lzs[m] = L.merge(s_max[m], p["s_idx"][m], s_sum[m])
        if Mt[m] == -np.inf:
            continue
        live = t_max[m] > -np.inf
        w = np.exp(t_max[m][live] - Mt[m])
        Zt = float((t_sum[m][live] * w).sum())
        cr = cross[m][live]
        if np.isinf(cr).any():
            kl[m] = np.inf
            continue
        at, as_ = t_max[m][live] - Mt[m], s_max[m][live] - Ms[m]
        shift = 0.0 if wrong == "no_recentre" else t_sum[m][live] * (at - as_)
        C = float((w * (cr + shift)).sum())
        kl[m] = max((C / Zt + lzt[m]) - lzs[m], 0.0) if (C / Zt + lzt[m]) - lzs[m] >= -CLAMP else (C / Zt + lzt[m]) - lzs[m]
        if absx is not None:
            G[m] = float((w * (np.asarray(absx, np.float64)[m][live] + t_sum[m][live] * (np.abs(at) + np.abs(as_)))).sum()) / Zt
    return dict(kl=kl, G=G, Mt=Mt, Ms=Ms, lzt=lzt, lzs=lzs, t_top1=t1, s_top1=s1)


def scaled(t_logits, s_logits, temperature, wrong=None):
    """fp32 logits -> (t, s) as the kernel scales them: one fp32 multiplication by the fp32 1 / temperature"""
    inv = np.float32(1.0) / np.float32(temperature)
    t = (np.asarray(t_logits, np.float32) * inv).astype(np.float64)
    s = np.asarray(s_logits, np.float32) * (np.float32(1.0) if wrong == "temp_one" else inv)
    return t, s.astype(np.float64)


def distill_logits(t_logits, s_logits, y, lengths=None, ignore_id=-1, temperature=1.0, wrong=None):
    """logits [R][T][V] of both models (fp32 values; finite or -inf), y int64 [R][T] -> dict: kl [R][T], G [R][T], kl_sum [R],
    count [R], t_top1 / s_top1 / agree [R][T], t_lp / s_lp [R][T - 1]."""
    tl, sl = np.asarray(t_logits), np.asarray(s_logits)
    R, T, V = tl.shape
    y = np.asarray(y, dtype=np.int64)
    t, s = scaled(tl.reshape(R * T, V), sl.reshape(R * T, V), temperature, wrong)
    mg = merge(dual_partials(t, s, wrong), wrong)
    if wrong == "swapped":
        t, s = s, t
    kl, G = mg["kl"].reshape(R, T).copy(), mg["G"].reshape(R, T).copy()
    live = np.ones((R, T), bool) if lengths is None else np.arange(T)[None, :] < np.asarray(lengths, np.int64)[:, None]
    kl[~live] = 0.0
    G[~live] = 0.0
    out = dict(kl=kl, G=G, t_top1=mg["t_top1"].reshape(R, T), s_top1=mg["s_top1"].reshape(R, T))
    out["agree"] = out["t_top1"] == out["s_top1"]
    out["kl_sum"] = np.array([sum(kl[r, j] for j in range(T) if live[r, j]) for r in range(R)], dtype=np.float64)
    out["count"] = live.sum(1).astype(np.int64)
    if T > 1:
        ok = S.counted(y, lengths, ignore_id, V)
        for name, x, Mx, lz in (("t_lp", t, mg["Mt"], mg["lzt"]), ("s_lp", s, mg["Ms"], mg["lzs"])):
            lp = np.zeros((R, T - 1))
            for r in range(R):
                for j in range(T - 1):
                    if ok[r, j]:
                        yt = x[r * T + j, y[r, j + 1]]
                        lp[r, j] = -np.inf if yt == -np.inf else (yt - Mx[r * T + j]) + lz[r * T + j]
            out[name] = lp
        out["counted"] = ok
    return out


def kl_loss(kl, B, temperature):
    """LOSS 2: KLDivLoss('batchmean') * temperature^2 over [B, T, V] logits"""
    return float(temperature) ** 2 * float(np.asarray(kl, np.float64).sum()) / B


def ce_loss(s_lp, y, counted=None):
    """LOSS 3: CrossEntropyLoss(ignore_index=0) of the student: the mean of -lp over the (counted) targets != 0"""
    tgt = np.asarray(y, np.int64)[..., 1:]
    ok = tgt != 0 if counted is None else (np.asarray(counted, bool) & (tgt != 0))
    return float(-(np.where(ok, np.asarray(s_lp, np.float64), 0.0)).sum() / max(int(ok.sum()), 1))


def bound_kl(G):
    """|device - fp64| allowed for kl (the docstring's derivation); G from merge / distill_logits"""
    return 2 * TOL_LOG + K_REL * np.asarray(G, np.float64)


# ---- the kernel's loops in fp32: how large is the factor in front of G? ---------------------------------------------------------

LOG2E = np.float32(1.4426950408889634)


def _fexp(x):
    """__expf: exp2(x * log2 e), every step rounded to fp32"""
    with np.errstate(under="ignore", invalid="ignore"):
        return np.exp2((np.asarray(x, np.float32) * LOG2E).astype(np.float32)).astype(np.float32)


def _tile_sum(v):
    """[.., 16] fp32 -> the tile's sum in the kernel's order: a lane's four columns ascending, then the xor 16 / 32 butterfly"""
    v = np.asarray(v, np.float32).reshape(*v.shape[:-1], 4, 4)
    lane = ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]
    return (lane[..., 0] + lane[..., 1]) + (lane[..., 2] + lane[..., 3])


def _merge_sum(v):
    """[nt] fp32 -> the merge's sum: thread tid takes tiles tid, tid + 256, ..; the 64-lane butterfly; waves 0 .. 3"""
    v = np.asarray(v, np.float32)
    pad = np.zeros((-len(v)) % 256, np.float32)
    acc = np.concatenate([v, pad]).reshape(-1, 256)
    th = acc[0].copy()
    for k in range(1, acc.shape[0]):
        th = th + acc[k]
    w = th.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :off] + w[:, off:2 * off]
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def kl_fp32(t, s):
    """scaled fp32 logits [M][N] (no +inf rows wanted here) -> A = C / Zt as the kernels form it, fp32 [M]"""
    t32, s32 = np.asarray(t, np.float32), np.asarray(s, np.float32)
    M, N = t32.shape
    nt = (N + TILE - 1) // TILE
    tp = np.full((M, nt * TILE), -np.inf, np.float32); tp[:, :N] = t32
    sp = np.full((M, nt * TILE), -np.inf, np.float32); sp[:, :N] = s32
    tp, sp = tp.reshape(M, nt, TILE), sp.reshape(M, nt, TILE)
    A = np.zeros(M, np.float32)
    with np.errstate(invalid="ignore"):
        t_max, s_max = tp.max(-1), sp.max(-1)
        live = tp > -np.inf
        dt = np.where(live, tp - t_max[..., None], np.float32(0))
        e = np.where(live, _fexp(dt), np.float32(0)).astype(np.float32)
        ds = np.where(live & (sp > -np.inf), sp - s_max[..., None], np.float32(0))
        t_sum = _tile_sum(e)
        cross = _tile_sum((e * (dt - ds).astype(np.float32)).astype(np.float32))
    for m in range(M):
        lv = t_max[m] > -np.inf
        Mt, Ms = t_max[m].max(), s_max[m].max()
        at = (t_max[m][lv] - Mt).astype(np.float32)
        w = _fexp(at)
        Zt = _merge_sum(t_sum[m][lv] * w)
        shift = (t_sum[m][lv] * (at - (s_max[m][lv] - Ms).astype(np.float32)).astype(np.float32)).astype(np.float32)
        C = _merge_sum(w * (cross[m][lv] + shift).astype(np.float32))
        A[m] = C / Zt
    return A


def delta_of(t, s):
    """worst |A32 - A64| / G over the rows of one input whose kl is finite"""
    p = dual_partials(t, s)
    mg = merge(p)
    fin = np.isfinite(mg["kl"]) & (mg["G"] > 0)
    if not fin.any():
        return 0.0
    A64 = mg["kl"] - mg["lzt"] + mg["lzs"]         # (rows the clamp touched have kl < 4e-5: not where the worst ratio lives)
    tt, ss = np.asarray(t)[fin], np.asarray(s)[fin]
    keep = np.isfinite(np.where(np.isinf(ss) & np.isfinite(tt), np.nan, 0.0)).all(1)
    A32 = kl_fp32(tt[keep], ss[keep]).astype(np.float64)
    return float((np.abs(A32 - A64[fin][keep]) / mg["G"][fin][keep]).max())


# ---- the inputs of tests/test_distill_gpu.py (made on the host, so that tests/test_distill.py sees the same ones) ---------------------

MS, NS, KS, TEMPS = (1, 16, 17, 37), (97, 197, 1000), ((128, 64), (768, 576), (1024, 576)), (1.0, 2.0)
NINF_MODES = (None, "teacher", "student", "both")


def e4m3_rows(Wf):
    """fp32 rows -> (e4m3 codes, the power-of-two row scale, the values the codes stand for); gpu_support.e4m3_rows on the host"""
    import torch
    wscale = torch.exp2(torch.ceil(torch.log2(Wf.abs().amax(dim=1) / 448.0)))
    W = (Wf / wscale[:, None]).to(torch.float8_e4m3fn)
    return W, wscale, W.float() * wscale[:, None]


def dual_inputs(M, N, Kt, Ks, fp8, seed=0, ninf=None):
    """Operands of the dual head whose logits have the shape of a softmax (gpu_support.softmax_head_inputs, for two models) -> dict of
    host tensors: Xt, Xs bf16; Wt (bf16, or e4m3 codes with wscale), Wt_bf16 (the bf16 matrix with the same values), Ws bf16;
    bt, bs fp32 [N].  ninf: -inf bias columns in the teacher, the student or both (the same columns), always with one whole tile."""
    import torch
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + 13 * N + Kt)
    Np = (N + 15) // 16 * 16
    out = {}
    for tag, K in (("t", Kt), ("s", Ks)):
        X = torch.randn(M, K, generator=g).bfloat16()
        Wf = torch.randn(Np, K, generator=g) * (3.0 / K ** 0.5)
        b = torch.randn(N, generator=g)
        for n in range(N, Np):                      # padding rows: a missing n < N guard would put e^large into the last tile
            Wf[n] = 4.0 * X[n % M].float()
        out["X" + tag], out["b" + tag], out["Wf" + tag] = X, b, Wf
    cols = torch.arange(1, N, 7)
    for tag in ("t", "s"):
        if ninf == "both" or ninf == {"t": "teacher", "s": "student"}[tag]:
            out["b" + tag][cols] = float("-inf")
            if N >= 32:
                out["b" + tag][16:32] = float("-inf")
    if fp8:
        out["Wt"], out["wscale"], vals = e4m3_rows(out.pop("Wft"))
        out["Wt_bf16"] = vals.bfloat16()
    else:
        out["Wt"] = out["Wt_bf16"] = out.pop("Wft").bfloat16()
        out["wscale"] = None
    out["Ws"] = out.pop("Wfs").bfloat16()
    return out


def host_logits(inp):
    """the two models' logits [M][N] of dual_inputs in fp64, rounded to fp32 (the device's differ by its accumulation order only)"""
    N = inp["bt"].shape[0]
    t = inp["Xt"].double() @ inp["Wt_bf16"].double()[:N].T + inp["bt"].double()
    s = inp["Xs"].double() @ inp["Ws"].double()[:N].T + inp["bs"].double()
    return t.float().numpy(), s.float().numpy()


def caption(M, N, seed=0):
    """one row of M ids whose targets exercise the ignore rules: (ids int64 [1][M], targets [M], lengths [1], ignore_id)"""
    rng = np.random.default_rng(seed + M + N)
    ids = rng.integers(1, N, size=M).astype(np.int64)
    ids[0] = 1
    if M > 4:
        ids[2] = N + 5                               # outside the vocabulary
        ids[3] = 0                                   # the ignore id
    targets = np.concatenate([ids[1:], [-1]]).astype(np.int64)
    return ids[None, :], targets, np.array([max(1, M - 2)], dtype=np.int32), 0
