"""tests/encoder_kernels_reference.py on the CPU: each restatement against torch.nn.functional in fp64 and a hand-worked case, and the
inputs of tests/test_encoder_kernels_gpu.py: a subtly wrong kernel (a residual read with the output's leading dimension, the GELU on
the wrong side of the residual add, a clamped row written in the M tail; depthwise taps transposed, taken across a frame boundary, a
stride on one axis only; a bias table indexed (dx, dy), the next head's table, a window one pixel off, a dropped key; a causal bound
off by one, the next row's PAD mask, q_row_off ignored; a LayerNorm that divides by its lane count; a mean over HW - 1) must miss a
case's bound by more than 10 x somewhere, and an fp32 implementation of each kernel's own loop must stay inside the bound and leave
at most 2 % of a case's elements off the correctly rounded value.  The fp32 term delta of the two attention bounds is measured here
(encoder_kernels_reference.DELTA_*_MEASURED are held to what this file computes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_kernels_reference as E
from tinyvit_reference import Attention, attention_bias_idxs, _Ctx

T64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))


def _inside(emu, ref, bound, flips=True):
    assert (np.abs(emu - ref) <= bound).all()
    if flips:
        assert E.flip_share(emu, ref) <= 0.02


# ---- the restatements are the torch operations --------------------------------------------------------------------------------------

def test_gemm_restatement_is_torch_functional_and_by_hand():
    a = E.gemm_inputs(5, 12, 64, E.TV_RES, 3)
    A, W, b, r = (T64(a[k]) for k in ("A", "W", "bias", "res"))
    lin = F.linear(A, W, b)
    for epi, want in ((0, lin), (E.TV_GELU, F.gelu(lin)), (E.TV_RES, lin + r), (E.TV_RES | E.TV_RES_GELU, F.gelu(lin + r))):
        y, bound = E.tv_gemm(a["A"], a["W"], a["bias"], a["res"], epi)
        assert np.abs(y - want.numpy()).max() < 1e-12 and (bound > 0).all()
    y, _ = E.tv_gemm(np.array([[1.0, 2.0]]), np.array([[3.0, -1.0], [0.5, 0.5]]), np.array([1.0, -7.0]), np.array([[0.25, 6.0]]), E.TV_RES)
    assert y.tolist() == [[2.25, 0.5]]
    assert abs(E.erf_gelu32(np.array([1.0]))[0] - 0.8413447460685429) < 3e-7 and E.erf_gelu32(np.array([0.0]))[0] == 0.0
    assert E.gemm_strides(36, 64, True) == (72, 40, 48) and E.gemm_strides(36, 64, False) == (64, 36, 36)


def test_im2col_restatement_is_unfold_and_by_hand():
    for f32_nchw in (True, False):
        x = E.im2col_inputs(2, 4, 6, 3, f32_nchw, 5)
        nchw = T64(x) if f32_nchw else T64(x).permute(0, 3, 1, 2)
        want = F.unfold(nchw, 3, padding=1, stride=2).transpose(1, 2).reshape(2 * 2 * 3, 27).numpy()          # columns ci * 9 + ky * 3 + kx
        got = E.tv_im2col(x, f32_nchw, 32)
        assert np.array_equal(got[:, :27], E.bf16_rne(want)) and not got[:, 27:].any() and not np.signbit(got[:, 27:]).any()
        assert f32_nchw == (not np.array_equal(x, E.bf16_rne(x)))             # the fp32 form's values are not bf16 values
    x = np.arange(1.0, 5.0).reshape(1, 1, 2, 2)                               # one 2 x 2 frame [[1, 2], [3, 4]]: the patch around (0, 0)
    assert E.tv_im2col(x, True, 9).tolist() == [[0, 0, 0, 0, 1, 2, 0, 3, 4]]
    assert E.tv_to_nchw(np.arange(6.0).reshape(1, 3, 2)).tolist() == [[[0, 2, 4], [1, 3, 5]]]


def test_dwconv_restatement_is_conv2d_and_by_hand():
    for n, H, W, C, stride, g in E.DWCONV_CASES[1:4]:
        a = E.dwconv_inputs(n, H, W, C, 7)
        w = T64(a["w9"]).T.reshape(C, 1, 3, 3)                               # [9][C] -> the torch weight [C][1][ky][kx]
        want = F.conv2d(T64(a["x"]).permute(0, 3, 1, 2), w, T64(a["bias"]), stride, 1, groups=C)
        want = (F.gelu(want) if g else want).permute(0, 2, 3, 1).numpy()
        y, bound = E.tv_dwconv(a["x"], a["w9"], a["bias"], stride, g)
        assert y.shape == want.shape and np.abs(y - want).max() < 1e-12 and (bound > 0).all()
    x = np.arange(1.0, 5.0).reshape(1, 2, 2, 1)                                # [[1, 2], [3, 4]], taps 1 .. 9, stride 1
    y, _ = E.tv_dwconv(x, np.arange(1.0, 10.0).reshape(9, 1), np.array([0.5]), 1, False)
    assert y.reshape(-1).tolist() == [5 + 12 + 24 + 36 + 0.5, 4 + 10 + 21 + 32 + 0.5, 2 + 6 + 15 + 24 + 0.5, 1 + 4 + 12 + 20 + 0.5]


def test_ln_and_pool_restatements_are_torch_and_by_hand():
    q = E.ln_inputs(4, 160, 2)
    y, bound = E.tv_ln(**q)
    want = F.layer_norm(T64(q["x"]), (160,), T64(q["g"]), T64(q["b"]), q["eps"]).numpy()
    assert np.abs(y - want).max() < 1e-9 and (bound > 0).all()
    assert set(q["x"][-1]) == {256.0, 258.0} and np.array_equal(q["x"], E.bf16_rne(q["x"]))          # the hard row, in bf16 values
    y, _ = E.tv_ln(np.array([[1.0, 3.0] * 4]), np.full(8, 2.0), np.full(8, 0.5), 0.0)
    assert np.allclose(y, [[-1.5, 2.5] * 4], atol=1e-15)
    x = E.pool_inputs(2, 49, 64, 4)
    m, bound = E.tv_pool(x)
    assert np.abs(m - T64(x).mean(dim=1).numpy()).max() < 1e-14 and bound.max() < 1e-5
    assert E.tv_pool(np.array([[[1.0], [2.0], [6.0]]]))[0].tolist() == [[3.0]]


def test_bias_table_rule_is_the_first_appearance_order():
    for ws in (1, 2, 3, 7, 14):
        assert np.array_equal(E.bias_idx(ws), attention_bias_idxs(ws).numpy())
    assert E.bias_idx(2).tolist() == [[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]]
    assert E.bias_idx(2, swap=True)[0].tolist() == [0, 2, 1, 3]


def test_tv_attn_restatement_is_sdpa_and_the_reference_block():
    n, H, W, heads, ws = 2, 4, 6, 2, 2
    a = E.tv_attn_inputs(n, H, W, heads, ws, "n", 9)
    ctx = E.tv_attn(a["qkv"], a["ab"], n, H, W, heads, ws)
    N, C = ws * ws, heads * 32
    rows = E.window_rows(n, H, W, ws)
    t = T64(a["qkv"]).reshape(n * H * W, heads, 3, 32)[rows]                  # [windows][N][heads][3][32]
    q, k, v = (t[:, :, :, i].transpose(1, 2) for i in range(3))
    mask = T64(a["ab"])[:, attention_bias_idxs(ws)]                           # additive, [heads][N][N]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)               # scale 1 / sqrt(32)
    want = np.zeros_like(ctx)
    want[rows.reshape(-1)] = o.transpose(1, 2).reshape(-1, C).numpy()
    assert np.abs(ctx - want).max() < 1e-12
    # the window partition, the per-head interleave and the table through tinyvit_reference's Attention block (proj = identity) on the
    # windows TinyVitBlock.run cuts: LayerNorm and qkv act per pixel, so the block's own qkv rows are the kernel's input
    torch.manual_seed(0)
    blk = Attention(C, heads, ws).double()
    with torch.no_grad():
        blk.attention_biases.copy_(T64(a["ab"]))
        blk.proj.weight.copy_(torch.eye(C, dtype=torch.float64))
        blk.proj.bias.zero_()
        x = torch.randn(n, H, W, C, dtype=torch.float64)
        qkv = blk.qkv(F.layer_norm(x, (C,), blk.norm.weight, blk.norm.bias, blk.norm.eps)).reshape(n * H * W, 3 * C)
        tw = x.view(n, H // ws, ws, W // ws, ws, C).transpose(2, 3).reshape(-1, N, C)
        out = blk.run(tw, _Ctx()).view(n, H // ws, W // ws, ws, ws, C).transpose(2, 3).reshape(n * H * W, C)
    assert np.abs(E.tv_attn(qkv.numpy(), a["ab"], n, H, W, heads, ws) - out.numpy()).max() < 1e-12
    # by hand: one window of two equal keys -> the mean of their values whatever q is; a table that favours the own pixel by ln 3
    t = np.zeros((2, 1, 3, 32))
    t[0, 0, 2], t[1, 0, 2] = 1.0, 3.0
    ab = np.array([[np.log(3.0), 0.0, 0.0, 0.0]])
    got = E.tv_attn(np.tile(t.reshape(2, 96), (2, 1)), ab, 1, 2, 2, 1, 2)    # a 2 x 2 window: values 1, 3, 1, 3
    assert np.allclose(got[0], (3 * 1 + 3 + 1 + 3) / 6) and np.allclose(got[1], (1 + 3 * 3 + 1 + 3) / 6)


def test_attn_small_restatement_is_sdpa_and_by_hand():
    for case, with_ids in ((E.ATTN_SMALL_CASES[1], True), (E.ATTN_SMALL_CASES[4], True), (E.ATTN_SMALL_CASES[5], False)):
        a = E.attn_small_inputs(*case, with_ids, 21)
        rows, T, t0, nkeys, H, hd = case
        ctx = E.attn_small(a)
        for r in range(rows):
            keys = a["keys"]
            mask = torch.zeros(T, keys, dtype=torch.float64)
            for j in range(T):
                if nkeys == 0:
                    mask[j, t0 + j + 1:] = -np.inf
                if with_ids:
                    mask[j, torch.as_tensor(a["ids"][r, :keys] == a["pad_id"])] = -np.inf
            q = T64(a["q"][r, a["q_row_off"]:a["q_row_off"] + T]).transpose(0, 1)
            o = F.scaled_dot_product_attention(q, T64(a["k"][r]).transpose(0, 1), T64(a["v"][r]).transpose(0, 1), attn_mask=mask)
            want = o.transpose(0, 1).numpy()
            got = ctx[r * T:(r + 1) * T]
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert np.nanmax(np.abs(got - want)) < 1e-12
    a = E.attn_small_inputs(*E.ATTN_SMALL_CASES[0], True, 1)                  # one key, and it is PAD: NaN, as torch
    assert a["ids"][0, 0] == E.PAD_ID and np.isnan(E.attn_small(a)).all() and np.isnan(E.attn_small(a, fp32=True)).all()
    a = E.attn_small_inputs(*E.ATTN_SMALL_CASES[0], False, 1)                 # one key: the context is its value
    assert np.array_equal(E.attn_small(a)[0, 0], a["v"][0, 0, 0])
    hit = set()
    for case in E.ATTN_SMALL_CASES:                                            # the masks hit a first, a middle and a last key
        a = E.attn_small_inputs(*case, True, 2)
        for r in range(case[0]):
            i = int(np.flatnonzero(a["ids"][r, :a["keys"]] == E.PAD_ID)[0])
            hit.add("first" if i == 0 else "last" if i == a["keys"] - 1 else "middle")
    assert hit == {"first", "middle", "last"}


# ---- the inputs tell wrong kernels apart; an fp32 implementation stays inside the bound ---------------------------------------------

@pytest.mark.parametrize("M,N,K,epi", E.GEMM_CASES)
def test_gemm_inputs_tell_wrong_kernels_apart(M, N, K, epi):
    a = E.gemm_inputs(M, N, K, epi, seed=100 + M + N + K)
    ref, bound = E.tv_gemm(a["A"], a["W"], a["bias"], a["res"], epi)
    for k in ("A", "W"):
        assert np.array_equal(a[k], E.bf16_rne(a[k]))
    nobias, _ = E.tv_gemm(a["A"], a["W"], np.full(N, a["bias"].mean()), a["res"], epi)
    assert N == 4 or E.differs(nobias, ref, bound).any(), "the bias must depend on the column"
    if epi & E.TV_RES:
        lda, ldo, ldr = E.gemm_strides(N, K, True)
        resbuf = E.tv_gemm_buffer(a["res"], M + 1, ldr).reshape(-1)            # the residual as the device holds it, NaN in the gaps
        wrong_res = np.stack([resbuf[m * ldo:m * ldo + N] for m in range(M)])  # read with the output's leading dimension
        wrong, _ = E.tv_gemm(a["A"], a["W"], a["bias"], wrong_res, epi)
        assert E.differs(wrong, ref, bound).any(), "ldr taken as ldo would pass"
    if epi & E.TV_RES_GELU:
        wrong, _ = E.tv_gemm(a["A"], a["W"], a["bias"], a["res"], epi, variant="res_gelu_order")
        assert E.differs(wrong, ref, bound).any(), "the GELU in front of the residual add would pass"
    if M % 32:
        # rows M .. of the last tile clamped to row M - 1 and stored: finite values where the device test asserts its NaN poison
        rows = (M + 31) // 32 * 32
        right = E.tv_gemm_buffer(ref, rows, N)
        wrong = right.copy()
        wrong[M:] = ref[M - 1]
        assert E.differs(wrong, right, E.tv_gemm_buffer(bound, rows, N, fill=1.0)).any(), "a clamped row stored in the M tail would pass"
    _inside(E.tv_gemm_fp32(a["A"], a["W"], a["bias"], a["res"], epi), ref, bound)


@pytest.mark.parametrize("n,H,W,C,stride,g", E.DWCONV_CASES)
def test_dwconv_inputs_tell_wrong_kernels_apart(n, H, W, C, stride, g):
    a = E.dwconv_inputs(n, H, W, C, seed=200 + n + H + W + C)
    ref, bound = E.tv_dwconv(a["x"], a["w9"], a["bias"], stride, g)
    assert np.array_equal(a["x"], E.bf16_rne(a["x"])) and np.array_equal(a["w9"], E.f32(a["w9"]))
    for v in E.dwconv_variants(n, H, W, C, stride, g):
        wrong, _ = E.tv_dwconv(a["x"], a["w9"], a["bias"], stride, g, variant=v)
        assert E.differs(wrong, ref, bound).any(), v + " would pass"
    _inside(E.tv_dwconv_fp32(a["x"], a["w9"], a["bias"], stride, g), ref, bound)


def test_dwconv_cases_cover_every_variant():
    seen = set()
    for case in E.DWCONV_CASES:
        seen.update(E.dwconv_variants(*case))
    assert seen == {"taps_transposed", "no_frame_boundary", "stride_one_axis"}


@pytest.mark.parametrize("M,C", E.LN_CASES)
def test_ln_inputs_tell_a_lane_count_divisor_apart(M, C):
    q = E.ln_inputs(M, C, seed=300 + M + C)
    ref, bound = E.tv_ln(**q)
    lanes = 64 * 8 * ((C + 511) // 512)
    if lanes != C:
        wrong, _ = E.tv_ln(**q, divisor=lanes)
        assert E.differs(wrong, ref, bound).any(), "a divisor of 64 * 8 * ceil(C / 512) would pass"
    _inside(E.tv_ln_fp32(**q), ref, bound)
    assert bound.max() < 0.1 * np.abs(ref).max()


@pytest.mark.parametrize("n,HW,C", E.POOL_CASES)
def test_pool_inputs_tell_a_wrong_divisor_apart(n, HW, C):
    x = E.pool_inputs(n, HW, C, seed=400 + n + HW + C)
    ref, bound = E.tv_pool(x)
    if HW > 1:
        wrong, _ = E.tv_pool(x, divisor=HW - 1)
        assert E.differs(wrong, ref, bound).any(), "a divisor of HW - 1 would pass"
    _inside(E.tv_pool_fp32(x), ref, bound, flips=False)                        # an fp32 output: no bf16 rounding to flip


def _rel(emu, ref):
    return float(np.nanmax(np.abs(emu - ref) / np.abs(ref)))


@pytest.fixture(scope="module")
def measured():
    """The delta measurement (worst relative error of the fp32 restatement, per kernel) over the device test's inputs, once."""
    tv, small = {}, {}
    for i, case in enumerate(E.TV_ATTN_CASES):
        a = E.tv_attn_inputs(*case, seed=500 + i)
        tv[i] = (a, E.tv_attn(a["qkv"], a["ab"], *case[:5]), E.tv_attn_fp32(a["qkv"], a["ab"], *case[:5]))
    for i, case in enumerate(E.ATTN_SMALL_CASES):
        for with_ids in (False, True):
            a = E.attn_small_inputs(*case, with_ids, seed=600 + i)
            small[i, with_ids] = (a, E.attn_small(a), E.attn_small(a, fp32=True))
    return tv, small


def test_attention_deltas_are_the_measured_ones(measured):
    tv, small = measured
    d_tv = max(_rel(emu, ref) for _, ref, emu in tv.values())
    d_small = max(_rel(emu, ref) for _, ref, emu in small.values() if not np.isnan(ref).all())
    print(f"tv_attn: worst |fp32 - fp64| / |ctx| = {d_tv:.4g} (constant {E.DELTA_TV_ATTN_MEASURED:.4g}); "
          f"attn_small: {d_small:.4g} (constant {E.DELTA_ATTN_SMALL_MEASURED:.4g})")
    for i, (_, ref, emu) in tv.items():
        print(f"  tv_attn {E.TV_ATTN_CASES[i]}: {_rel(emu, ref):.4g}")
    for (i, ids), (_, ref, emu) in small.items():
        if not np.isnan(ref).all():
            print(f"  attn_small {E.ATTN_SMALL_CASES[i]} ids={ids}: {_rel(emu, ref):.4g}")
    # the constants are this measurement (to two digits, rounded up), not a device result
    assert d_tv <= E.DELTA_TV_ATTN_MEASURED <= 1.1 * d_tv
    assert d_small <= E.DELTA_ATTN_SMALL_MEASURED <= 1.1 * d_small
    # 4 x the measurement is far below the cap: the cap (a quarter of an ulp, 2^-10 .. 2^-9 of the value) never binds on these inputs
    assert 4 * max(E.DELTA_TV_ATTN_MEASURED, E.DELTA_ATTN_SMALL_MEASURED) < 2.0 ** -12


@pytest.mark.parametrize("i", range(len(E.TV_ATTN_CASES)))
def test_tv_attn_inputs_tell_wrong_kernels_apart(measured, i):
    case = E.TV_ATTN_CASES[i]
    a, ref, emu = measured[0][i]
    n, H, W, heads, ws, kind = case
    bound = E.attn_bound(ref, E.DELTA_TV_ATTN_MEASURED)
    assert np.array_equal(a["qkv"], E.bf16_rne(a["qkv"])) and np.abs(ref).min() >= 1.0          # no cancellation: |ctx| >= min |v|
    assert len(np.unique(a["ab"])) == a["ab"].size                                               # no two table entries alike
    for v in E.tv_attn_variants(*case):
        wrong = E.tv_attn(a["qkv"], a["ab"], n, H, W, heads, ws, variant=v)
        assert E.differs(wrong, ref, bound).any(), v + " would pass"
    _inside(E.bf16_rne(emu), ref, bound)
    if kind != "n":                                                                              # the scores do what the case is for
        rows = E.window_rows(n, H, W, ws)
        t = a["qkv"].reshape(n * H * W, heads, 3, 32)
        s = np.einsum("id,jd->ij", t[rows[0], 0, 0], t[rows[0], 0, 1]) * E.TV_ATTN_SCALE + a["ab"][0][E.bias_idx(ws)]
        d = np.diff(s, axis=1)
        assert (d > 0).all() if kind == "ascending" else (d < 0).all()


def test_tv_attn_cases_cover_every_variant_and_block_size():
    seen = set()
    for case in E.TV_ATTN_CASES:
        seen.update(E.tv_attn_variants(*case))
    assert seen == {"swap_dydx", "next_head_table", "window_shift", "last_key"}
    assert {(c[4] ** 2 + 63) // 64 * 64 for c in E.TV_ATTN_CASES} == {64, 192, 256}
    assert any(c[1] != c[2] for c in E.TV_ATTN_CASES) and {c[3] for c in E.TV_ATTN_CASES} >= {1, 2, 3, 5}


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("i", range(len(E.ATTN_SMALL_CASES)))
def test_attn_small_inputs_tell_wrong_kernels_apart(measured, i, with_ids):
    case = E.ATTN_SMALL_CASES[i]
    a, ref, emu = measured[1][i, with_ids]
    bound = E.attn_bound(ref, E.DELTA_ATTN_SMALL_MEASURED)
    for k in ("q", "k", "v"):
        assert np.array_equal(a[k], E.bf16_rne(a[k]))
    for v in E.attn_small_variants(*case, with_ids):
        wrong = E.attn_small(a, variant=v)
        assert E.differs(wrong, ref, bound).any(), v + " would pass"
    assert np.array_equal(np.isnan(emu), np.isnan(ref))
    ok = ~np.isnan(ref)
    if ok.any():
        _inside(E.bf16_rne(emu[ok]), ref[ok], bound[ok])


def test_attn_small_cases_cover_every_variant():
    seen = set()
    for case in E.ATTN_SMALL_CASES:
        seen.update(E.attn_small_variants(*case, True))
    assert seen == {"q_row_off", "causal_short", "mask_next_row"}
