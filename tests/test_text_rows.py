"""tests/text_rows_reference.py on the CPU: the restatement against torch.nn.functional and hand-worked cases, and the inputs of
tests/test_text_rows_gpu.py: a subtly wrong kernel (row_off ignored, the last slab left out, quick-GELU for GELU; for txt_block
the causal bound off by one, the last image key dropped, clip r for r / beams, two heads' part slots swapped) must miss a
case's tolerance by more than 10 x, and an fp32 implementation of the same operation must leave at most 2 % of a case's elements
off the correctly rounded value."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import text_rows_reference as R


def test_bf16_and_e4m3_formats_match_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4000) * np.exp2(rng.integers(-20, 20, 4000)), [0.0, 1.0, 1.00390625, 1.01171875, 2.0 ** -130]])
    x = x.astype(np.float32).astype(np.float64)
    assert np.array_equal(R.bf16_rne(x), torch.as_tensor(x, dtype=torch.float32).bfloat16().double().numpy())
    assert R.bf16_rne(1.00390625) == 1.0 and R.bf16_rne(1.01171875) == 1.015625          # ties to even, both ways
    codes = np.arange(256).astype(np.uint8)
    vals = R.e4m3_decode(codes)
    ok = (codes & 0x7F) != 0x7F                                                             # 0x7f / 0xff are NaN
    assert np.array_equal(R.e4m3_encode(vals[ok]), np.where(vals[ok] == 0, 0, codes[ok]) | (codes[ok] & 0x80))
    assert R.e4m3_decode(0x7E) == 448.0 and R.e4m3_decode(0x01) == 2.0 ** -9 and R.e4m3_decode(0x08) == 2.0 ** -6
    assert R.e4m3_encode(np.array([17.0]))[0] == R.e4m3_encode(np.array([16.0]))[0]        # 17 is a tie between 16 and 18: even mantissa
    assert R.e4m3_encode(np.array([19.0]))[0] == R.e4m3_encode(np.array([20.0]))[0]
    assert R.e4m3_encode(np.array([1000.0, -1000.0])).tolist() == [0x7E, 0xFE]
    if hasattr(torch, "float8_e4m3fn"):
        v = (rng.standard_normal(4000) * np.exp2(rng.integers(-9, 8, 4000))).clip(-448, 448).astype(np.float32)
        t = torch.as_tensor(v).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        mine = R.e4m3_encode(v.astype(np.float64))
        assert np.array_equal(mine & 0x7F, t & 0x7F)


def test_pack_frags_is_the_index_formula():
    for rows, K in ((16, 32), (48, 64), (32, 96)):
        src = np.arange(rows * K).reshape(rows, K)
        assert np.array_equal(R.pack_frags(src), R.pack_frags_by_formula(src))
    src = np.arange(16 * 32).reshape(16, 32)
    p = R.pack_frags(src).reshape(64, 8)
    assert p[0].tolist() == list(range(8)) and p[1].tolist() == list(range(32, 40)) and p[16].tolist() == list(range(8, 16))


def test_kv_quant_v_scale_rule_by_hand():
    D, H = 128, 2
    kv = np.zeros((3, 3 * D))
    kv[0, 2 * D] = 448.0            # exactly 448 * 2^0
    kv[0, 2 * D + 64] = 450.0       # just above: the next power of two
    kv[1, 2 * D] = 1.0              # 1 <= 448 * 2^-8 = 1.75, not <= 0.875
    kv[1, 2 * D + 64:] = 0.0        # a zero group: scale 1, codes 0
    kv[2, 2 * D] = 2.0 ** -120      # the exponent of the scale is floored at -126
    kv[2, 2 * D + 1] = -2.0 ** -123
    codes, scales, written = R.kv_quant_v(kv, D, H, 5)
    assert scales[0, 0] == 1.0 and scales[1, 0] == 2.0 and scales[0, 1] == 2.0 ** -8 and scales[1, 1] == 1.0
    assert codes[0, 0, 0] == 0x7E and codes[1, 0, 0] == R.e4m3_encode(np.array([225.0]))[0] and not codes[1, 1].any()
    assert scales[0, 2] == 2.0 ** -126 and R.e4m3_decode(codes[0, 2, 0]) == 64.0 and R.e4m3_decode(codes[0, 2, 1]) == -8.0
    assert written[:, :3].all() and not written[:, 3:].any() and not codes[:, 3:].any()
    for rows, (D, H) in ((7, (128, 2)), (33, (768, 12))):
        kv = R.kv_quant_inputs(rows, D, H, seed=rows + D)
        c, s, w = R.kv_quant_v(kv, D, H, rows + 5)
        v = kv[:, 2 * D:].reshape(rows, H, 64).transpose(1, 0, 2)
        amax = np.abs(v).max(axis=2)
        sc = s[:, :rows]
        nz = amax > 0
        assert (amax <= 448 * sc).all() and ((amax > 224 * sc) | (sc == 2.0 ** -126))[nz].all() and (sc[~nz] == 1).all()
        assert (np.abs(R.e4m3_decode(c[:, :rows]) * sc[:, :, None] - v) <= 2.0 ** -4 * np.maximum(np.abs(v), sc[:, :, None] * 2.0 ** -6)).all()
        assert (sc == 2.0 ** -126).sum() >= 2 and (~nz).sum() >= 1 and (amax == 448 * sc).any()      # the edges are in the inputs


def test_restatement_is_torch_functional():
    rng = np.random.default_rng(1)
    a = R.gemm_inputs(5, 21, 64, False, 7)
    X, W, b = (torch.as_tensor(a[k]) for k in ("X", "W", "bias"))
    for epi, fn in ((0, lambda y: y), (1, F.gelu), (2, F.relu)):
        y, bound = R.skinny(a["X"], a["W"], None, a["bias"], 21, epi)
        assert np.abs(y - fn(F.linear(X, W[:21], b)).numpy()).max() < 1e-12 and (bound > 0).all()
    q = R.ln_inputs(3, 128, 9, 5)
    y, _ = R.ln_reduce(**q)
    x = torch.as_tensor(q["slabs"].sum(0) + q["bias"] + q["resid"])
    want = F.layer_norm(x, (128,), torch.as_tensor(q["g"]), torch.as_tensor(q["b"]), q["eps"]).numpy()
    assert np.abs(y - want).max() < 1e-9
    e = R.embed_inputs(2, 64, 3)
    y, _ = R.prologue_rows(2, ids=e["ids"], T=1, t0=e["t0"], word=e["word"], pos=e["pos"], g=e["g"], b=e["b"], eps=e["eps"])
    ids = np.clip(e["ids"][:, 0], 0, e["vocab"] - 1)
    assert e["ids"].max() >= e["vocab"] and (e["ids"] == e["vocab"] - 1).any()
    x = torch.as_tensor(e["word"][ids] + e["pos"][e["t0"]])
    assert np.abs(y - F.layer_norm(x, (64,), torch.as_tensor(e["g"]), torch.as_tensor(e["b"]), e["eps"]).numpy()).max() < 1e-9
    f = R.ffn_inputs(3, 128, 128, False, 9)
    h64, hb, slabs, sb = R.ffn_txt(f["X"], f["W"], None, f["bias"], f["W2"], None)
    h = torch.as_tensor(R.bf16_rne(F.gelu(F.linear(torch.as_tensor(f["X"]), torch.as_tensor(f["W"]), torch.as_tensor(f["bias"]))).numpy()))
    assert np.abs(slabs.sum(0) - F.linear(h, torch.as_tensor(f["W2"])).numpy()).max() < 1e-9 and slabs.shape == (2, 3, 128)
    s, _ = R.splitk(f["X"], f["W"], None, 128, 4)
    assert np.abs(s.sum(0) - f["X"] @ f["W"].T).max() < 1e-12
    # by hand
    y, _ = R.skinny(np.array([[1.0, 2.0]]), np.array([[3.0, -1.0], [0.5, 0.5]]), np.array([2.0, 4.0]), np.array([1.0, -7.0]), 2, 2)
    assert y.tolist() == [[3.0, 0.0]]
    assert [R.orow(m, 3, 8, 2) for m in range(7)] == [2, 3, 4, 10, 11, 12, 18]
    assert abs(R.gelu(np.array([1.0]))[0] - 0.8413447460685429) < 1e-15


@pytest.mark.parametrize("M,N,K,fp8,epi,T,row_stride,row_off", R.SKINNY_CASES)
def test_skinny_inputs_tell_wrong_kernels_apart(M, N, K, fp8, epi, T, row_stride, row_off):
    a = R.gemm_inputs(M, N, K, fp8, seed=1000 + M + N + K)
    ref, bound = R.skinny(a["X"], a["W"], a["wscale"], a["bias"], N, epi)
    n_rows = ((M + T - 1) // T) * max(row_stride, T) + 2
    right = R.scatter_rows(ref, T, row_stride, row_off, n_rows, fill=0.0)
    tol = R.scatter_rows(bound, T, row_stride, row_off, n_rows, fill=bound.min())
    if row_off:
        wrong = R.scatter_rows(ref, T, row_stride, 0, n_rows, fill=0.0)
        assert (np.abs(wrong - right) > 10 * tol).any(), "row_off ignored would pass"
    if epi == 1:
        wrong, _ = R.skinny(a["X"], a["W"], a["wscale"], a["bias"], N, 1, R.quick_gelu)
        assert (np.abs(wrong - ref) > 10 * bound).any(), "quick-GELU would pass"
    nobias, _ = R.skinny(a["X"], a["W"], a["wscale"], np.full(N, a["bias"].mean()), N, epi)
    assert (np.abs(nobias - ref) > 10 * bound).any(), "the bias must depend on n"
    # ragged N: the padded weight rows give finite values, so a store without the n < N guard replaces the NaN poison the device
    # test asserts in columns >= N (and, at ldo = N, the next row's first columns by something else than that row's value)
    Np = (N + 15) // 16 * 16
    if Np > N:
        pad = a["X"] @ (a["W"][N:Np] * (1.0 if a["wscale"] is None else a["wscale"][N:Np, None])).T
        assert np.isfinite(pad).all()
        if M > 1:
            k = min(Np - N, N)
            assert (np.abs(pad[:-1, :k] - ref[1:, :k]) > 10 * bound[1:, :k]).any()
    # an fp32 implementation of the same operation: share of elements off the correctly rounded value
    emu = R.skinny_fp32(a["X"], a["W"], a["wscale"], a["bias"], N, epi)
    assert (np.abs(emu - ref) <= bound).all()
    assert R.flip_share(emu, ref) <= 0.02


@pytest.mark.parametrize("M,D,F_,fp8", R.FFN_CASES)
def test_ffn_inputs_tell_wrong_kernels_apart(M, D, F_, fp8):
    a = R.ffn_inputs(M, D, F_, fp8, seed=4000 + M + D + F_)
    h64, hb, slabs, sb = R.ffn_txt(a["X"], a["W"], a["wscale"], a["bias"], a["W2"], a["w2scale"])
    hq, _, wrong_slabs, _ = R.ffn_txt(a["X"], a["W"], a["wscale"], a["bias"], a["W2"], a["w2scale"], gelu_fn=R.quick_gelu)
    assert (np.abs(hq - h64) > 10 * hb).any() and (np.abs(wrong_slabs - slabs) > 10 * sb).any(), "quick-GELU would pass"
    total, tb = slabs.sum(0), sb.sum(0)
    assert (np.abs(slabs[:-1].sum(0) - total) > 10 * tb).any(), "a missing last slab would pass"
    if slabs.shape[0] > 1:                                    # slabs swapped: slices carry different weight
        assert (np.abs(slabs[0] - slabs[1]) > 10 * (sb[0] + sb[1])).any()
    emu = R.skinny_fp32(a["X"], a["W"], a["wscale"], a["bias"], F_, 1)
    assert (np.abs(emu - h64) <= hb).all()
    assert R.flip_share(emu, h64) <= 0.02


@pytest.mark.parametrize("M,D,nslab", R.LN_CASES + [(m, k, n) for m, k, kind, n in R.PROLOGUE_CASES if kind == 1])
def test_ln_inputs_tell_a_missing_slab_apart(M, D, nslab):
    q = R.ln_inputs(M, D, nslab, seed=D + nslab, hard_row=(M, D, nslab) in R.LN_CASES)
    y, bound = R.ln_reduce(**q)
    if nslab > 1:
        wrong, _ = R.ln_reduce(**q, nslab=nslab - 1)
        assert (np.abs(wrong - y) > 10 * bound).any(), "slab nslab - 1 left out would pass"
    nob, _ = R.ln_reduce(**dict(q, bias=np.zeros(D)))
    assert (np.abs(nob - y) > 10 * bound).any()
    # fp32 two-pass LayerNorm of the fp32 sum stays inside the bound (the hard row included)
    x = np.zeros((M, D), np.float32)
    for s in range(nslab):
        x = x + q["slabs"][s].astype(np.float32)
    x = x + (q["bias"].astype(np.float32) + q["resid"].astype(np.float32))
    mu = x.mean(axis=1, keepdims=True, dtype=np.float32)
    d = x - mu
    rstd = np.float32(1) / np.sqrt((d * d).mean(axis=1, keepdims=True, dtype=np.float32) + np.float32(q["eps"]))
    emu = d * rstd * q["g"].astype(np.float32) + q["b"].astype(np.float32)
    assert (np.abs(emu.astype(np.float64) - y) <= bound).all()
    assert bound.max() < 0.1 * np.abs(y).max()


@pytest.mark.parametrize("M,N,K,ksplit,fp8", R.SPLITK_CASES)
def test_splitk_inputs(M, N, K, ksplit, fp8):
    a = R.gemm_inputs(M, N, K, fp8, seed=3000 + M + N + K, guard=False)
    ks = ksplit or R.DEFAULT_KSPLIT[K]
    s, b = R.splitk(a["X"], a["W"], a["wscale"], N, ks)
    assert s.shape == (ks, M, N) and np.abs(s.sum(0) - a["X"] @ (a["W"][:N] * (1 if not fp8 else a["wscale"][:N, None])).T).max() < 1e-9
    if ks > 1:
        assert (np.abs(s[0] - s[ks - 1]) > 10 * (b[0] + b[ks - 1])).any()     # slabs in each other's place would show
    assert b.max() < 1e-3 * np.abs(s).max()


# ---- txt_block -----------------------------------------------------------------------------------------------------------------

def test_txt_block_restatement_is_sdpa_and_layer_norm():
    """fp64 scaled_dot_product_attention with an explicit mask over [image keys of the clip | text keys of the row], per head."""
    for case in ((128, 4, 2, 3, 2, 5, False, False, "n"), (128, 2, 1, 1, 0, 3, True, True, "n")):
        D, rows, beams, T, t0, S, _, _, _ = case
        q = R.txt_block_inputs(*case, seed=11)
        out = R.txt_block(q)
        H, M = q["H"], rows * T
        v_img = q["v_img"] if q["v_img"] is not None else q["kv_img"][:, 2 * D:]
        ctx = np.zeros((M, H, 64))
        for r in range(rows):
            clip = r // beams
            K = np.concatenate([q["kv_img"][clip * S:(clip + 1) * S, D:2 * D], q["kv_txt"][r, :t0 + T, D:2 * D]])
            V = np.concatenate([v_img[clip * S:(clip + 1) * S], q["kv_txt"][r, :t0 + T, 2 * D:]])
            Q = q["kv_txt"][r, t0:t0 + T, :D]
            mask = torch.ones(T, S + t0 + T, dtype=torch.bool)
            for j in range(T):
                mask[j, S + t0 + j + 1:] = False
            hd = lambda a: torch.as_tensor(a).reshape(a.shape[0], H, 64).transpose(0, 1)
            o = F.scaled_dot_product_attention(hd(Q), hd(K), hd(V), attn_mask=mask)          # [H][T][64], scale 1 / sqrt(64)
            ctx[r * T:(r + 1) * T] = o.transpose(0, 1).numpy()
        assert np.abs(ctx - out["ctx"]).max() < 1e-12
        cb = torch.as_tensor(R.bf16_rne(out["ctx"]))
        Wo = torch.as_tensor(q["Wo"])
        for h in range(H):
            assert np.abs(F.linear(cb[:, h], Wo[:, h * 64:(h + 1) * 64]).numpy() - out["part"][:, h]).max() < 1e-12
        x = F.linear(cb.reshape(M, D), Wo, torch.as_tensor(q["aob"])) + torch.as_tensor(q["xin"])
        want = F.layer_norm(x, (D,), torch.as_tensor(q["g1"]), torch.as_tensor(q["b1"]), q["eps"]).numpy()
        assert np.abs(want - out["x1"]).max() < 1e-9
        x1, _ = R.txt_x1(out["part"], q)
        assert np.abs(x1 - out["x1"]).max() < 1e-12
        assert np.isnan(q["kv_txt"][:, t0 + T:]).all() and np.isnan(q["kv_txt"][:, :t0, :D]).all()      # the poison a query must not read


def test_txt_block_by_hand():
    """One row, one image key, position 0, q = 0: both scores are 0, the context is the mean of the two V rows."""
    q = R.txt_block_inputs(128, 1, 1, 1, 0, 1, False, False, "equal", seed=3, identity=True)
    out = R.txt_block(q)
    want = 0.5 * (q["kv_img"][0, 256:] + q["kv_txt"][0, 0, 256:])
    assert np.array_equal(out["ctx"].reshape(-1), want)
    for h in range(2):                                            # identity slices: output n of head h is context element n % 64
        assert np.array_equal(out["part"][0, h], np.tile(R.bf16_rne(want[64 * h:64 * h + 64]), 2))
    assert np.array_equal(R.txt_block(q, variant="causal")["ctx"].reshape(-1), q["kv_img"][0, 256:])
    assert R.txt_variants(768, 6, 3, 1, 0, 5, False, False, "n")[-1] == "clip"


@pytest.mark.parametrize("i", range(len(R.TXT_CASES)))
def test_txt_block_inputs_tell_wrong_kernels_apart(i):
    case = R.TXT_CASES[i]
    q = R.txt_block_inputs(*case, seed=7000 + i)
    ref = R.txt_block(q)
    for k in ("kv_img", "kv_txt", "Wo"):
        v = q[k][~np.isnan(q[k])]
        assert np.array_equal(v, R.bf16_rne(v)), k                               # operands are bf16 values
    if q["v_img"] is not None:
        assert np.array_equal(q["v_img"], R.bf16_rne(q["v_img"]))                # code * scale is a bf16 value
    assert (ref["bound"] > 0).all() and np.isfinite(ref["part"]).all()
    for v in R.txt_variants(*case):
        wrong = R.txt_block(q, variant=v)
        assert (np.abs(wrong["part"] - ref["part"]) > 10 * ref["bound"]).any(), v + " would pass"
    # an fp32 implementation with the kernel's bf16 rounding of P stays inside the bound.  (No share of boundary flips is set for
    # the context: the rounding of P moves it by a good part of a bf16 ulp, not by an fp32 error, and it is no output; the bf16
    # output xsb is held to the rounding of the device's own xs exactly.)
    emu = R.txt_block(q, emulate=True)
    assert (np.abs(emu["part"] - ref["part"]) <= ref["bound"]).all()
    if case[8] == "peak_img" or case[8] == "peak_txt":
        assert R.txt_block(q)["ctx"].max() > 0                                  # (finite scores: no NaN from exp)
    x1, xb = R.txt_x1(emu["part"], q)
    assert xb.max() < 1e-4 and np.isfinite(x1).all()
