"""The teacher's staging and layout kernels (csrc/preproc.hip, the plain row kernels of csrc/rowops.hip, the text embedding of
csrc/select.hip), each through its
handle-free gitcap_dbg_* hook on poisoned buffers, against tests/staging_reference.py: the fp32 frame transform under a counted
bound, the text embedding under ln_bound, everything else bit for bit.  Every launch is a few KB to a few MB."""
import ctypes

import numpy as np
import pytest
import torch

import staging_reference as R
from gpu_support import NAN, assert_tail, bf16_bits, close_to_fp64, f64, lib, poisoned, ptr, same_bits, stream, to_dev  # noqa: F401
from text_rows_reference import U32, bf16_ulp

pytestmark = pytest.mark.gpu

ERR_ARG = -1
SPARE = 16                      # elements behind what a launch may write
IPOISON = -777
BF, I32 = torch.bfloat16, torch.int32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def off_ptr(t, nbytes):
    """a pointer `nbytes` behind the start of t: a misaligned argument"""
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def untouched(buf, fill=NAN):
    assert_tail(buf, 0, fill)
    return True


def is_nan_bf16(bits):
    return (bits & 0x7fff) > 0x7f80


def assert_bf16_bits(dev_bits, ref_bits, what=""):
    """equal bit for bit; where the reference is a NaN the device holds a NaN (its payload is the instruction's)"""
    dev_bits, ref_bits = np.asarray(dev_bits), np.asarray(ref_bits)
    assert dev_bits.shape == ref_bits.shape, what
    n = is_nan_bf16(ref_bits)
    assert np.array_equal(is_nan_bf16(dev_bits), n), what
    assert np.array_equal(dev_bits[~n], ref_bits[~n]), what


def f32_bits_equal(t, ref32):
    return np.array_equal(host(t).view(np.uint32), np.ascontiguousarray(ref32, np.float32).view(np.uint32))


def tie_values(x32, rng):
    """some elements replaced by bf16 ties (round up and round down to even), +-inf-free; returns x32"""
    flat = x32.reshape(-1)
    idx = rng.choice(flat.size, size=max(4, flat.size // 16), replace=False)
    base = R.bf16_rne(flat[idx].astype(np.float64))
    flat[idx] = (base + 0.5 * bf16_ulp(base) * np.where(base >= 0, 1.0, -1.0)).astype(np.float32)     # exactly between two bf16 values
    return x32


# ---- the frame transform ------------------------------------------------------------------------------------------------------------

def run_preprocess(lib, frames_u8, crop):
    nf, H, W, _ = frames_u8.shape
    fr = dev(frames_u8)
    n = nf * 3 * crop * crop
    out = poisoned(n + SPARE, NAN)
    assert lib.gitcap_preprocess(ptr(fr), nf, H, W, ptr(out), crop, stream()) == 0
    torch.cuda.synchronize()
    assert_tail(out, n, NAN)
    return fr, host(out[:n]).reshape(nf, 3, crop, crop)


@pytest.mark.parametrize("i", range(len(R.PRE_CASES)), ids=lambda i: "x".join(map(str, R.PRE_CASES[i])))
def test_preprocess_fp32_within_the_counted_bound(lib, i):
    """|device - preprocess64| <= PRE_C 2^-24 magnitude, element by element (PRE_C: counted in staging_reference's docstring)"""
    nf, H, W, crop = R.PRE_CASES[i]
    frames = R.pre_case_frames(i)
    _, out = run_preprocess(lib, frames, crop)
    ref = np.stack([R.preprocess64(f, crop)[0] for f in frames])
    mag = np.stack([R.preprocess64(f, crop)[1] for f in frames])
    close_to_fp64(out, ref, R.PRE_C * U32 * mag, f"preprocess {nf}x{H}x{W} -> {crop}", flips=False)
    ratio = float((np.abs(out.astype(np.float64) - ref) / (U32 * mag)).max())
    print(f"preprocess {nf}x{H}x{W} -> {crop}: max |device - fp64| / (2^-24 magnitude) = {ratio:.2f}")


def test_preprocess_refuses_bad_arguments_before_any_launch(lib):
    fr = dev(R.frames_u8(1, 9, 16, 0))
    out = poisoned(3 * 64 + SPARE, NAN)
    for args in ((None, 1, 9, 16, ptr(out), 8), (ptr(fr), 1, 9, 16, None, 8), (ptr(fr), 0, 9, 16, ptr(out), 8), (ptr(fr), 1, 0, 16, ptr(out), 8),
                 (ptr(fr), 1, 9, 16, ptr(out), 0)):
        assert lib.gitcap_preprocess(*args, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert untouched(out)


PATCH_CASES = [(8, 4, 48), (8, 4, 64), (28, 14, 588), (28, 14, 640), (32, 16, 768)]


@pytest.mark.parametrize("crop,p,Kp", PATCH_CASES)
def test_preprocess_patches_are_the_rounded_fp32_form_in_patch_layout(lib, crop, p, Kp):
    for g, (H, W) in enumerate([(37, 53), (16, 9), (crop, crop)]):
        frames = R.frames_u8(2, H, W, 300 + g)
        fr, f32 = run_preprocess(lib, frames, crop)
        rows = 2 * (crop // p) ** 2
        pat = poisoned(rows * Kp + SPARE, NAN, BF)
        assert lib.gitcap_dbg_preprocess_patches(ptr(fr), 2, H, W, crop, p, Kp, ptr(pat), stream()) == 0
        torch.cuda.synchronize()
        assert_tail(pat, rows * Kp, NAN)
        got = bf16_bits(pat[:rows * Kp]).reshape(rows, Kp)
        ref = R.patch_rows(R.bf16_of_f32(f32), p, Kp)
        assert np.array_equal(got[:, :3 * p * p], ref[:, :3 * p * p]), (H, W)
        assert is_nan_bf16(got[:, 3 * p * p:]).all(), "the pad columns are never written"


def test_preprocess_patches_refuses_bad_arguments_before_any_launch(lib):
    fr = dev(R.frames_u8(1, 9, 16, 0))
    pat = poisoned(4 * 64 + SPARE, NAN, BF)
    bad = [(ptr(fr), 1, 9, 16, 8, 4, 49, ptr(pat)),              # Kp odd
           (ptr(fr), 1, 9, 16, 8, 4, 46, ptr(pat)),              # Kp < 3 p^2
           (ptr(fr), 1, 9, 16, 8, 3, 48, ptr(pat)),              # crop % p
           (ptr(fr), 1, 9, 16, 8, 0, 48, ptr(pat)),
           (ptr(fr), 1, 9, 16, 8, 4, 48, off_ptr(pat, 1)),
           (None, 1, 9, 16, 8, 4, 48, ptr(pat)), (ptr(fr), 1, 9, 16, 8, 4, 48, None)]
    for args in bad:
        assert lib.gitcap_dbg_preprocess_patches(*args, stream()) == ERR_ARG, args[1:7]
    torch.cuda.synchronize()
    assert untouched(pat)


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("crop", [8, 14, 28])
def test_preprocess_stem_rows_are_the_rounded_fp32_form_in_stem_layout(lib, crop, nf):
    H, W = 30, 41
    frames = R.frames_u8(nf, H, W, 400 + crop)
    fr, f32 = run_preprocess(lib, frames, crop)
    Ho = crop // 2
    rows = nf * Ho * Ho                                        # 3 x 7 x 7 = 147: not a multiple of the 64 rows of a workgroup
    col = poisoned(rows * 32 + SPARE, NAN, BF)
    assert lib.gitcap_dbg_preprocess_stem(ptr(fr), nf, H, W, crop, ptr(col), stream()) == 0
    torch.cuda.synchronize()
    assert_tail(col, rows * 32, NAN)
    got = bf16_bits(col[:rows * 32]).reshape(nf, Ho, Ho, 32)
    ref = R.stem_rows(R.bf16_of_f32(f32)).reshape(nf, Ho, Ho, 32)
    assert np.array_equal(got, ref)
    k = np.arange(27)
    assert (got[:, 0][..., k[(k % 9) // 3 == 0]] == 0).all(), "taps at iy = -1"
    assert (got[:, :, 0][..., k[k % 3 == 0]] == 0).all(), "taps at ix = -1"
    assert (got[..., 27:] == 0).all()
    assert (got[:, 1:, 1:, :27] != 0).any()


def test_preprocess_stem_refuses_bad_arguments_before_any_launch(lib):
    fr = dev(R.frames_u8(1, 9, 16, 0))
    col = poisoned(16 * 32 + SPARE, NAN, BF)
    bad = [(ptr(fr), 1, 9, 16, 8, off_ptr(col, 8)), (ptr(fr), 1, 9, 16, 7, ptr(col)), (ptr(fr), 0, 9, 16, 8, ptr(col)),
           (None, 1, 9, 16, 8, ptr(col)), (ptr(fr), 1, 9, 16, 8, None)]
    for args in bad:
        assert lib.gitcap_dbg_preprocess_stem(*args, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert untouched(col)


# ---- im2col, cast ---------------------------------------------------------------------------------------------------------------------

IM2COL_CASES = [(8, 4, 48), (8, 4, 64), (28, 14, 588), (28, 14, 592), (42, 14, 640), (32, 16, 768)]


@pytest.mark.parametrize("nf", [1, 2])
@pytest.mark.parametrize("img,p,Kp", IM2COL_CASES)
def test_im2col_is_the_rounded_frame_in_patch_layout_with_zero_pads(lib, img, p, Kp, nf):
    rng = np.random.default_rng(img * 1000 + Kp + nf)
    fr = tie_values(rng.standard_normal((nf, 3, img, img)).astype(np.float32), rng)
    fr[0, 1, img // 2, img - 1] = np.nan
    fr[nf - 1, 2, img - 1, 1] = -np.inf
    rows = nf * (img // p) ** 2
    pat = poisoned(rows * Kp + SPARE, NAN, BF)
    fr_t = dev(fr)                                                  # named: a temporary would be freed before the launch
    assert lib.gitcap_dbg_im2col(ptr(fr_t), nf, img, p, Kp, ptr(pat), stream()) == 0
    torch.cuda.synchronize()
    assert_tail(pat, rows * Kp, NAN)
    got = bf16_bits(pat[:rows * Kp]).reshape(rows, Kp)
    assert_bf16_bits(got, R.patch_rows(R.bf16_of_f32(fr), p, Kp, fill=0))
    assert (got[:, 3 * p * p:] == 0).all()


def test_im2col_refuses_bad_arguments_before_any_launch(lib):
    fr = poisoned(3 * 28 * 28 + SPARE, 1.0)
    pat = poisoned(4 * 640 + SPARE, NAN, BF)
    bad = [(ptr(fr), 1, 28, 14, 590 - 4, ptr(pat)),            # Kp < 3 p^2
           (ptr(fr), 1, 28, 14, 589, ptr(pat)),                # odd Kp on the 2-element path
           (ptr(fr), 1, 8, 4, 50, ptr(pat)),                   # Kp % 4 on the 4-element path
           (ptr(fr), 1, 28, 8, 192, ptr(pat)),                 # img % p
           (ptr(fr), 1, 9, 3, 28, ptr(pat)),                   # odd p
           (ptr(fr), 0, 8, 4, 48, ptr(pat)),
           (off_ptr(fr, 8), 1, 8, 4, 48, ptr(pat)), (ptr(fr), 1, 8, 4, 48, off_ptr(pat, 4)),       # 16 / 8 bytes on the 4-element path
           (off_ptr(fr, 2), 1, 28, 14, 588, ptr(pat)), (ptr(fr), 1, 28, 14, 588, off_ptr(pat, 2)),
           (None, 1, 8, 4, 48, ptr(pat)), (ptr(fr), 1, 8, 4, 48, None)]
    for args in bad:
        assert lib.gitcap_dbg_im2col(*args, stream()) == ERR_ARG, args[1:5]
    torch.cuda.synchronize()
    assert untouched(pat)


@pytest.mark.parametrize("n", [4, 1020, 1028])
def test_cast_bf16_rounds_to_nearest_even(lib, n):
    rng = np.random.default_rng(n)
    x = tie_values(rng.standard_normal(n).astype(np.float32) * np.float32(5.0), rng)
    x[:4] = [np.nan, np.inf, -np.inf, 1.00390625]                # 1 + 2^-8: a tie that rounds down to even
    out = poisoned(n + SPARE, NAN, BF)
    x_t = dev(x)
    assert lib.gitcap_dbg_cast_bf16(ptr(x_t), ptr(out), n, stream()) == 0
    torch.cuda.synchronize()
    assert_tail(out, n, NAN)
    got = bf16_bits(out[:n])
    assert_bf16_bits(got, R.bf16_of_f32(x))
    assert got[1] == 0x7f80 and got[2] == 0xff80 and got[3] == 0x3f80


def test_cast_bf16_refuses_bad_arguments_before_any_launch(lib):
    x = poisoned(64, 1.0)
    out = poisoned(64, NAN, BF)
    for args in ((ptr(x), ptr(out), 6), (ptr(x), ptr(out), 0), (off_ptr(x, 4), ptr(out), 8), (ptr(x), off_ptr(out, 2), 8), (None, ptr(out), 8),
                 (ptr(x), None, 8)):
        assert lib.gitcap_dbg_cast_bf16(*args, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert untouched(out)


# ---- e4m3 -> bf16 ---------------------------------------------------------------------------------------------------------------------

def dequant_inputs(rows, K):
    """rows / 5 rows per scale 2^e, e in DEQUANT_EXPONENTS; every block walks the 256 codes from 0"""
    per = rows // 5
    assert per * 5 == rows and per * K >= 256
    codes = np.tile((np.arange(per * K) % 256).astype(np.uint8).reshape(per, K), (5, 1))
    scale = np.repeat(np.exp2(np.array(R.DEQUANT_EXPONENTS, np.float64)), per)
    return codes, scale


def run_dequant(lib, codes, scale):
    rows, K = codes.shape
    out = poisoned(rows * K + SPARE, NAN, BF)
    c_t, s_t = dev(codes), dev(scale.astype(np.float32))
    assert lib.gitcap_dbg_dequant_fp8(ptr(c_t), ptr(s_t), ptr(out), rows, K, stream()) == 0
    torch.cuda.synchronize()
    assert_tail(out, rows * K, NAN)
    return out


DEQUANT_SHAPES = [(10, 128), (80, 16), (30, 48)]              # K = 16: one thread per row; K = 48: row edges inside a workgroup


@pytest.mark.parametrize("rows,K", DEQUANT_SHAPES)
def test_dequant_fp8_is_exact_on_every_code_under_every_scale(lib, rows, K):
    codes, scale = dequant_inputs(rows, K)
    got = bf16_bits(run_dequant(lib, codes, scale)[:rows * K]).reshape(rows, K)
    ref = R.dequant(codes, scale)
    nan = (codes & 0x7f) == 0x7f
    assert nan.sum() >= 10 and is_nan_bf16(got[nan]).all(), "the two NaN codes"
    assert np.array_equal(got[~nan], R.bits_of_bf16(ref[~nan]))
    assert (got[codes == 0x80] == 0x8000).all() and (got[codes == 0] == 0).all()


@pytest.mark.parametrize("n", [1, 3, 4])
def test_dequant_fp8_batch_equals_the_single_launches(lib, n):
    shapes = [(10, 128), (1, 16), (30, 48), (80, 16)][:n]     # 1280, 16 (a single chunk), 1440, 1280 values
    ins, singles, outs = [], [], []
    for rows, K in shapes:
        if rows % 5 == 0:
            codes, scale = dequant_inputs(rows, K)
        else:
            codes, scale = (np.arange(16, dtype=np.uint8) * 13 + 5).reshape(1, 16), np.array([2.0 ** -9])
        ins.append((dev(codes), dev(scale.astype(np.float32))))
        singles.append(run_dequant(lib, codes, scale))
        outs.append(poisoned(rows * K + SPARE, NAN, BF))
    arr = lambda ps: (ctypes.c_void_p * n)(*ps)
    i32 = lambda v: (ctypes.c_int32 * n)(*v)
    rc = lib.gitcap_dbg_dequant_fp8_batch(n, arr([c.data_ptr() for c, _ in ins]), arr([s.data_ptr() for _, s in ins]),
                                          arr([o.data_ptr() for o in outs]), i32([r for r, _ in shapes]), i32([k for _, k in shapes]), stream())
    torch.cuda.synchronize()
    assert rc == 0
    for (rows, K), one, out in zip(shapes, singles, outs):
        assert_tail(out, rows * K, NAN)                           # an entry shorter than the longest leaves its tail alone
        assert same_bits(out[:rows * K], one[:rows * K]), (rows, K)


def test_dequant_fp8_refuses_bad_arguments_before_any_launch(lib):
    codes, scale = dequant_inputs(10, 128)
    c, s = dev(codes), dev(scale.astype(np.float32))
    outs = [poisoned(1280 + SPARE, NAN, BF) for _ in range(5)]
    out = outs[0]
    for args in ((ptr(c), ptr(s), ptr(out), 10, 24), (ptr(c), ptr(s), ptr(out), 0, 128), (ptr(c), ptr(s), ptr(out), 10, 0),
                 (off_ptr(c, 8), ptr(s), ptr(out), 9, 128), (ptr(c), ptr(s), off_ptr(out, 8), 9, 128), (None, ptr(s), ptr(out), 10, 128),
                 (ptr(c), None, ptr(out), 10, 128), (ptr(c), ptr(s), None, 10, 128)):
        assert lib.gitcap_dbg_dequant_fp8(*args, stream()) == ERR_ARG

    def batch(n, rows, K, w8=None):
        arr = lambda ps: (ctypes.c_void_p * len(ps))(*ps)
        i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
        return lib.gitcap_dbg_dequant_fp8_batch(n, arr(w8 or [c.data_ptr()] * len(rows)), arr([s.data_ptr()] * len(rows)),
                                                arr([o.data_ptr() for o in outs[:len(rows)]]), i32(rows), i32(K), stream())
    assert batch(5, [10] * 5, [128] * 5) == ERR_ARG
    assert batch(0, [10], [128]) == ERR_ARG
    assert batch(2, [10, 10], [128, 24]) == ERR_ARG              # K % 16
    assert batch(2, [10, 0], [128, 128]) == ERR_ARG
    assert batch(2, [10, 10], [128, 128], w8=[c.data_ptr(), 0]) == ERR_ARG
    assert batch(2, [10, 9], [128, 128], w8=[c.data_ptr(), c.data_ptr() + 8]) == ERR_ARG
    torch.cuda.synchronize()
    for o in outs:
        assert untouched(o)


# ---- text embedding + LayerNorm -------------------------------------------------------------------------------------------------------

EMBED_CASES = [(1, 1, 0, 1, 64), (3, 5, 2, 8, 128), (2, 3, 0, 3, 576), (1, 7, 4, 9, 768), (5, 2, 1, 2, 1024), (1, 6, 0, 6, 260)]
VOCAB = 50
HARD_ID = 7


HARD_CASE = (3, 5, 2, 8, 128)


def embed_case(rows, T, t0, ld_ids, D, seed):
    """ids with -3, vocab, vocab + 5 and 2^40 among the valid ones (as far as the case has room), garbage in the columns T .. ld_ids - 1,
    and in HARD_CASE one hard row, row 0: word[HARD_ID] = 300 + 0.05 n(0, 1) at a position whose embedding is small (large mean, small
    variance)"""
    hard = (rows, T, t0, ld_ids, D) == HARD_CASE
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    word = f32(rng.standard_normal((VOCAB, D)))
    pos = f32(0.5 * rng.standard_normal((t0 + T + 1, D)))
    if hard:
        word[HARD_ID] = f32(300.0 + 0.05 * rng.standard_normal(D))
        pos[t0] = f32(0.01 * rng.standard_normal(D))
    ids = np.full((rows, ld_ids), 2 ** 50, np.int64)
    ids[:, T:] = np.where(rng.integers(0, 2, size=(rows, ld_ids - T)) == 1, 2 ** 50, -2 ** 45)
    ids[:, :T] = rng.integers(0, VOCAB, size=(rows, T))
    if hard:
        ids[0, 0] = HARD_ID
    specials = [-3, VOCAB, VOCAB + 5, 2 ** 40, VOCAB - 1, 0]
    slots = [i for i in range(rows * T) if i != 0]
    for i, v in zip(slots, specials):
        ids[i // T, i % T] = v
    g = f32(1.0 + 0.5 * np.sin(np.arange(D)))
    b = f32(0.3 * np.cos(np.arange(D) * 0.7))
    return ids, word, pos, g, b


def run_embed(lib, case, tensors, want_xf=True, want_xb=True):
    rows, T, t0, ld_ids, D = case
    ids, word, pos, g, b = tensors
    M = rows * T
    xf = poisoned(M * D + SPARE, NAN) if want_xf else None
    xb = poisoned(M * D + SPARE, NAN, BF) if want_xb else None
    rc = lib.gitcap_dbg_embed_text(ptr(ids), ld_ids, rows, T, t0, ptr(word), ptr(pos), ptr(g), ptr(b), 1e-5, D, VOCAB, ptr(xf), ptr(xb), stream())
    torch.cuda.synchronize()
    assert rc == 0
    for o in (xf, xb):
        if o is not None:
            assert_tail(o, M * D, NAN)
    return xf, xb


@pytest.mark.parametrize("case", EMBED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_embed_text_rows_against_fp64_layernorm(lib, case):
    """xf under ln_bound (one add, no slabs); xb under the same bound plus half a bf16 ulp, and off the correctly rounded value in at
    most 2 % of the elements -- counted over every row but the hard one: there ln_bound itself (0.03 at values of 3) exceeds half a
    bf16 ulp (0.008), so the rounded fp32 row may differ from the rounded fp64 row anywhere without being wrong.  The hard row's xb is
    held to the bound and, like every row, to being the rounding of the device's own xf."""
    rows, T, t0, ld_ids, D = case
    arrs = embed_case(*case, seed=sum(case))
    ids, word, pos, g, b = arrs
    tensors = tuple(dev(a) for a in arrs)
    xf, xb = run_embed(lib, case, tensors)
    M = rows * T
    tok = np.clip(ids[:, :T], 0, VOCAB - 1).reshape(-1)
    w64, p64 = word.astype(np.float64)[tok], np.tile(pos.astype(np.float64)[t0:t0 + T], (rows, 1))
    g64, b64 = g.astype(np.float64), b.astype(np.float64)
    ref = R.layernorm(w64 + p64, g64, b64, 1e-5)
    bound = R.ln_bound([], [w64, p64], g64, b64, 1e-5)
    xf_h = host(xf[:M * D]).reshape(M, D)
    close_to_fp64(xf_h, ref, bound, f"embed_text xf {case}", flips=False)
    xb_h, bb = f64(xb[:M * D]).reshape(M, D), bound + 0.5 * bf16_ulp(ref)
    easy = slice(1, None) if case == HARD_CASE else slice(None)
    close_to_fp64(xb_h[easy], ref[easy], bb[easy], f"embed_text xb {case}")
    close_to_fp64(xb_h, ref, bb, f"embed_text xb {case}, hard row included", flips=False)
    assert np.array_equal(bf16_bits(xb[:M * D]).reshape(M, D), R.bf16_of_f32(xf_h)), "xb is the rounded xf"
    # either output alone: the other one's bits do not change
    only_b = run_embed(lib, case, tensors, want_xf=False)[1]
    only_f = run_embed(lib, case, tensors, want_xb=False)[0]
    assert same_bits(only_b, xb) and same_bits(only_f, xf)


def test_embed_text_refuses_bad_arguments_before_any_launch(lib):
    case = (2, 3, 1, 4, 64)
    ids, word, pos, g, b = (dev(a) for a in embed_case(*case, seed=1))
    xf, xb = poisoned(6 * 64 + SPARE, NAN), poisoned(6 * 64 + SPARE, NAN, BF)
    ok = dict(ids=ptr(ids), ld_ids=4, rows=2, T=3, t0=1, word=ptr(word), pos=ptr(pos), gamma=ptr(g), beta=ptr(b), eps=1e-5, D=64, vocab=VOCAB,
              xf=ptr(xf), xb=ptr(xb))
    bad = [dict(D=62), dict(D=0), dict(D=1028), dict(ld_ids=2), dict(t0=-1), dict(vocab=0), dict(rows=0), dict(T=0), dict(ids=None), dict(word=None),
           dict(pos=None), dict(gamma=None), dict(beta=None), dict(xf=None, xb=None), dict(word=off_ptr(word, 4)), dict(pos=off_ptr(pos, 8)),
           dict(gamma=off_ptr(g, 4)), dict(beta=off_ptr(b, 4)), dict(xf=off_ptr(xf, 4)), dict(xb=off_ptr(xb, 2)), dict(ids=off_ptr(ids, 4))]
    for change in bad:
        assert lib.gitcap_dbg_embed_text(*{**ok, **change}.values(), stream()) == ERR_ARG, list(change)
    torch.cuda.synchronize()
    assert untouched(xf) and untouched(xb)


# ---- the frame window -------------------------------------------------------------------------------------------------------------------

WINDOW_SHAPES = [(B, N, D) for B in (1, 2) for N in (1, 5) for D in (64, 260, 768)]
F_RING = 3


@pytest.mark.parametrize("B,N,D", WINDOW_SHAPES)
def test_window_scatter_writes_the_wrapped_slots_and_nothing_else(lib, B, N, D):
    rng = np.random.default_rng(B * 1000 + N * 100 + D)
    size = B * F_RING * N * D
    for head in range(F_RING):
        for n in (1, 2, 3):
            src = rng.standard_normal((B, n, N, D)).astype(np.float32)
            ring = poisoned(size + SPARE, NAN)
            src_t = dev(src)
            assert lib.gitcap_dbg_window_scatter(ptr(src_t), ptr(ring), B, n, F_RING, head, N, D, stream()) == 0
            torch.cuda.synchronize()
            assert_tail(ring, size, NAN)
            ref = R.window_scatter(np.full((B, F_RING, N, D), np.nan, np.float32), src, head)
            assert f32_bits_equal(ring[:size], ref.reshape(-1)), (head, n)          # untouched slots keep the poison's bits


def test_window_scatter_grid_stride_loop_runs_more_than_once(lib):
    """70 x 1024 / 4 = 17920 pieces of 16 bytes per frame > 64 workgroups x 256"""
    B, n, N, D, head = 1, 2, 70, 1024, 2
    src = np.random.default_rng(5).standard_normal((B, n, N, D)).astype(np.float32)
    size = B * F_RING * N * D
    ring = poisoned(size + SPARE, NAN)
    src_t = dev(src)
    assert lib.gitcap_dbg_window_scatter(ptr(src_t), ptr(ring), B, n, F_RING, head, N, D, stream()) == 0
    torch.cuda.synchronize()
    assert_tail(ring, size, NAN)
    assert f32_bits_equal(ring[:size], R.window_scatter(np.full((B, F_RING, N, D), np.nan, np.float32), src, head).reshape(-1))


def test_window_scatter_refuses_bad_arguments_before_any_launch(lib):
    src = poisoned(4 * 5 * 64, 1.0)
    ring = poisoned(3 * 5 * 64 + SPARE, NAN)
    bad = [(ptr(src), ptr(ring), 1, 4, 3, 0, 5, 64), (ptr(src), ptr(ring), 1, 1, 3, 3, 5, 64), (ptr(src), ptr(ring), 1, 1, 3, -1, 5, 64),
           (ptr(src), ptr(ring), 1, 0, 3, 0, 5, 64), (ptr(src), ptr(ring), 0, 1, 3, 0, 5, 64), (ptr(src), ptr(ring), 1, 1, 3, 0, 5, 62),
           (ptr(src), ptr(ring), 1, 1, 3, 0, 0, 64), (off_ptr(src, 4), ptr(ring), 1, 1, 3, 0, 5, 64), (ptr(src), off_ptr(ring, 8), 1, 1, 3, 0, 5, 64),
           (None, ptr(ring), 1, 1, 3, 0, 5, 64), (ptr(src), None, 1, 1, 3, 0, 5, 64)]
    for args in bad:
        assert lib.gitcap_dbg_window_scatter(*args, stream()) == ERR_ARG, args[2:]
    torch.cuda.synchronize()
    assert untouched(ring)


def run_assemble(lib, ring_t, temporal_t, B, N, D, head, want_vis=True):
    rows = B * F_RING * N
    out = poisoned(rows * D + SPARE, NAN, BF)
    vis = poisoned(rows * D + SPARE, NAN) if want_vis else None
    assert lib.gitcap_dbg_window_assemble(ptr(ring_t), ptr(temporal_t), ptr(out), ptr(vis), B, F_RING, head, N, D, stream()) == 0
    torch.cuda.synchronize()
    assert_tail(out, rows * D, NAN)
    if want_vis:
        assert_tail(vis, rows * D, NAN)
    return out, vis


@pytest.mark.parametrize("B,N,D", WINDOW_SHAPES)
def test_window_assemble_adds_in_fp32_then_rounds(lib, B, N, D):
    rng = np.random.default_rng(B * 1000 + N * 100 + D + 1)
    ring = tie_values(rng.standard_normal((B, F_RING, N, D)).astype(np.float32), rng)
    temporal = rng.standard_normal((F_RING, D)).astype(np.float32)
    ring_t, temporal_t = dev(ring), dev(temporal)
    rows = B * F_RING * N                                          # 3, 6, 15, 30: never a multiple of the 4 rows of a workgroup
    assert rows % 4
    for head in range(F_RING):
        out, vis = run_assemble(lib, ring_t, temporal_t, B, N, D, head)
        s = R.window_assemble(ring, temporal, head)
        assert f32_bits_equal(vis[:rows * D], s.reshape(-1)), head
        assert np.array_equal(bf16_bits(out[:rows * D]).reshape(rows, D), R.bf16_of_f32(s)), head
        assert same_bits(run_assemble(lib, ring_t, temporal_t, B, N, D, head, want_vis=False)[0], out), "vis = NULL changes nothing"
        plain, pvis = run_assemble(lib, ring_t, None, B, N, D, head)
        s0 = R.window_assemble(ring, None, head)
        assert np.array_equal(bf16_bits(plain[:rows * D]).reshape(rows, D), R.bf16_of_f32(s0)) and f32_bits_equal(pvis[:rows * D], s0.reshape(-1))


def test_window_assemble_refuses_bad_arguments_before_any_launch(lib):
    ring, temporal = poisoned(3 * 5 * 64, 1.0), poisoned(3 * 64, 1.0)
    out, vis = poisoned(15 * 64 + SPARE, NAN, BF), poisoned(15 * 64 + SPARE, NAN)
    ok = (ptr(ring), ptr(temporal), ptr(out), ptr(vis), 1, 3, 0, 5, 64)
    bad = [ok[:6] + (3, 5, 64), ok[:6] + (-1, 5, 64), ok[:8] + (62,), ok[:8] + (1028,), ok[:7] + (0, 64), ok[:4] + (0, 3, 0, 5, 64),
           ok[:5] + (0, 0, 5, 64), (None,) + ok[1:], ok[:2] + (None,) + ok[3:], (off_ptr(ring, 4),) + ok[1:], ok[:1] + (off_ptr(temporal, 8),) + ok[2:],
           ok[:2] + (off_ptr(out, 4),) + ok[3:], ok[:3] + (off_ptr(vis, 4),) + ok[4:]]
    for args in bad:
        assert lib.gitcap_dbg_window_assemble(*args, stream()) == ERR_ARG, args[4:]
    torch.cuda.synchronize()
    assert untouched(out) and untouched(vis)


# ---- ragged batches ---------------------------------------------------------------------------------------------------------------------

RAGGED_COUNTS = [[1], [3, 1, 2], [2] * 256]


def run_tables(lib, counts, N):
    B, total = len(counts), sum(counts)
    off, ln, pos = (poisoned(n + SPARE, IPOISON, I32) for n in (B, B, total))
    rc = lib.gitcap_dbg_ragged_tables((ctypes.c_int32 * B)(*counts), B, N, ptr(off), ptr(ln), ptr(pos), total, stream())
    torch.cuda.synchronize()
    assert rc == 0
    for t, n in ((off, B), (ln, B), (pos, total)):
        assert_tail(t, n, IPOISON)                                 # entries behind B and behind the frame total keep the poison
    return off, ln, pos


@pytest.mark.parametrize("counts", RAGGED_COUNTS, ids=lambda c: f"{len(c)}clips")
def test_ragged_tables_equal_the_reference(lib, counts):
    N = 5
    off, ln, pos = run_tables(lib, counts, N)
    roff, rlen, rpos = R.ragged_tables(counts, N)
    B, total = len(counts), sum(counts)
    assert np.array_equal(host(off[:B]), roff) and np.array_equal(host(ln[:B]), rlen) and np.array_equal(host(pos[:total]), rpos)


def test_ragged_tables_refuses_bad_arguments_before_any_launch(lib):
    off, ln, pos = (poisoned(300 + SPARE, IPOISON, I32) for _ in range(3))
    c = lambda v: (ctypes.c_int32 * len(v))(*v)
    bad = [(c([1] * 257), 257, 5, ptr(off), ptr(ln), ptr(pos), 600), (c([1]), 0, 5, ptr(off), ptr(ln), ptr(pos), 600),
           (c([3, 0, 2]), 3, 5, ptr(off), ptr(ln), ptr(pos), 600), (c([3, 256, 2]), 3, 5, ptr(off), ptr(ln), ptr(pos), 600),
           (c([3, 1, 2]), 3, 5, ptr(off), ptr(ln), ptr(pos), 5),          # pos holds fewer entries than there are frames
           (c([3, 1, 2]), 3, 0, ptr(off), ptr(ln), ptr(pos), 600), (None, 3, 5, ptr(off), ptr(ln), ptr(pos), 600),
           (c([3, 1, 2]), 3, 5, None, ptr(ln), ptr(pos), 600), (c([3, 1, 2]), 3, 5, ptr(off), None, ptr(pos), 600),
           (c([3, 1, 2]), 3, 5, ptr(off), ptr(ln), None, 600), (c([3, 1, 2]), 3, 5, off_ptr(off, 2), ptr(ln), ptr(pos), 600)]
    for args in bad:
        assert lib.gitcap_dbg_ragged_tables(*args, stream()) == ERR_ARG, args[1:3]
    torch.cuda.synchronize()
    assert untouched(off, IPOISON) and untouched(ln, IPOISON) and untouched(pos, IPOISON)


@pytest.mark.parametrize("D", [64, 260, 768])
@pytest.mark.parametrize("counts,N", [([1], 3), ([3, 1, 2], 5), ([2] * 256, 1)], ids=["1clip", "3clips", "256clips"])
def test_ragged_temporal_adds_the_frames_own_position(lib, counts, N, D):
    rng = np.random.default_rng(len(counts) * 1000 + D)
    frames = sum(counts)
    rows = frames * N                                              # 3, 30, 512
    _, _, pos = run_tables(lib, counts, N)
    trows = max(counts) + 1
    ln = tie_values(rng.standard_normal((rows, D)).astype(np.float32), rng)
    temporal = rng.standard_normal((trows, D)).astype(np.float32)
    ln_t, temporal_t = dev(ln), dev(temporal)
    s = R.ragged_temporal(ln, temporal, R.ragged_tables(counts, N)[2], N)
    res = []
    for want_vis in (True, False):
        out = poisoned(rows * D + SPARE, NAN, BF)
        vis = poisoned(rows * D + SPARE, NAN) if want_vis else None
        assert lib.gitcap_dbg_ragged_temporal(ptr(ln_t), ptr(temporal_t), trows, ptr(pos), ptr(out), ptr(vis), frames, N, D, stream()) == 0
        torch.cuda.synchronize()
        assert_tail(out, rows * D, NAN)
        assert np.array_equal(bf16_bits(out[:rows * D]).reshape(rows, D), R.bf16_of_f32(s))
        if want_vis:
            assert_tail(vis, rows * D, NAN)
            assert f32_bits_equal(vis[:rows * D], s.reshape(-1))
        res.append(out)
    assert same_bits(res[0], res[1])


def test_ragged_temporal_refuses_bad_arguments_before_any_launch(lib):
    ln, temporal = poisoned(6 * 5 * 64, 1.0), poisoned(3 * 64, 1.0)
    pos = to_dev([0, 1, 2, 0, 0, 1], I32)
    wrong = to_dev([0, 1, 3, 0, 0, 1], I32)                        # a position behind the table
    neg = to_dev([0, -1, 2, 0, 0, 1], I32)
    out, vis = poisoned(30 * 64 + SPARE, NAN, BF), poisoned(30 * 64 + SPARE, NAN)
    ok = (ptr(ln), ptr(temporal), 3, ptr(pos), ptr(out), ptr(vis), 6, 5, 64)
    bad = [ok[:3] + (ptr(wrong),) + ok[4:], ok[:3] + (ptr(neg),) + ok[4:], ok[:2] + (2,) + ok[3:], ok[:8] + (62,), ok[:8] + (1028,), ok[:6] + (0, 5, 64),
           ok[:7] + (0, 64), (None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:3] + (None,) + ok[4:], ok[:4] + (None,) + ok[5:],
           (off_ptr(ln, 4),) + ok[1:], ok[:1] + (off_ptr(temporal, 4),) + ok[2:], ok[:4] + (off_ptr(out, 2),) + ok[5:], ok[:5] + (off_ptr(vis, 8),) + ok[6:]]
    for args in bad:
        assert lib.gitcap_dbg_ragged_temporal(*args, stream()) == ERR_ARG, args[6:]
    torch.cuda.synchronize()
    assert untouched(out) and untouched(vis)


# ---- gathers ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 1028])                       # 1028: the 1024-column stride loop runs twice, the second pass partial
def test_gather_hidden_is_the_caller_layout(lib, D):
    rng = np.random.default_rng(D)
    for B in (1, 2):
        for E in (1, 3):
            for S_img in (1, 5):
                for T in (1, 4):
                    istride, tstride = B * S_img * D + 8, B * T * D + 12          # entry strides larger than an entry
                    img = rng.standard_normal((E, istride)).astype(np.float32)
                    txt = rng.standard_normal((E, tstride)).astype(np.float32)
                    n = B * E * (S_img + T) * D
                    out = poisoned(n + SPARE, NAN)
                    img_t, txt_t = dev(img), dev(txt)
                    rc = lib.gitcap_dbg_gather_hidden(ptr(img_t), ptr(txt_t), ptr(out), E, B, S_img, T, D, istride, tstride, stream())
                    torch.cuda.synchronize()
                    assert rc == 0
                    assert_tail(out, n, NAN)
                    ref = R.gather_hidden(img[:, :B * S_img * D].reshape(E, B * S_img, D), txt[:, :B * T * D].reshape(E, B * T, D), B, S_img, T)
                    assert f32_bits_equal(out[:n], ref.reshape(-1)), (B, E, S_img, T)


def test_gather_hidden_refuses_bad_arguments_before_any_launch(lib):
    img, txt = poisoned(3 * 5 * 64 + 64, 1.0), poisoned(3 * 4 * 64 + 64, 1.0)
    out = poisoned(3 * 9 * 64 + SPARE, NAN)
    ok = (ptr(img), ptr(txt), ptr(out), 3, 1, 5, 4, 64, 5 * 64, 4 * 64)
    bad = [ok[:7] + (62,) + ok[8:], ok[:3] + (0,) + ok[4:], ok[:4] + (0,) + ok[5:], ok[:5] + (0,) + ok[6:], ok[:6] + (0,) + ok[7:], ok[:8] + (5 * 64 + 2, 4 * 64),
           ok[:8] + (5 * 64, 4 * 64 + 1), ok[:8] + (-4, 4 * 64), (None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:2] + (None,) + ok[3:],
           (off_ptr(img, 4),) + ok[1:], ok[:1] + (off_ptr(txt, 8),) + ok[2:], ok[:2] + (off_ptr(out, 4),) + ok[3:]]
    for args in bad:
        assert lib.gitcap_dbg_gather_hidden(*args, stream()) == ERR_ARG, args[3:]
    torch.cuda.synchronize()
    assert untouched(out)


@pytest.mark.parametrize("t_len", [1, 5])
@pytest.mark.parametrize("layers", [1, 3])
def test_gather_txt_rows_copies_the_filled_positions_of_the_source_rows(lib, layers, t_len):
    rows, Tmax, width = 4, 8, 24
    stride = rows * Tmax * width + 64                              # larger than one layer
    rng = np.random.default_rng(layers * 10 + t_len)
    src = rng.integers(0, 0x7f80, size=(layers, stride)).astype(np.uint16)          # any finite bf16 bit pattern
    src_rows = [2, 2, 0, 3]
    dst = poisoned(layers * stride + SPARE, NAN, BF)
    src_t, rows_t = dev(src.view(np.int16)).view(BF), to_dev(src_rows, I32)
    rc = lib.gitcap_dbg_gather_txt_rows(ptr(src_t), ptr(dst), ptr(rows_t), rows, t_len, Tmax, width, layers,
                                        stride, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert_tail(dst, layers * stride, NAN)
    poison = np.uint16(bf16_bits(poisoned(1, NAN, BF))[0])
    ref = np.full((layers, stride), poison, np.uint16)
    body = ref[:, :rows * Tmax * width].reshape(layers, rows, Tmax, width)
    R.gather_txt_rows(src[:, :rows * Tmax * width].reshape(layers, rows, Tmax, width), body, src_rows, t_len)
    ref[:, :rows * Tmax * width] = body.reshape(layers, -1)
    assert np.array_equal(bf16_bits(dst[:layers * stride]).reshape(layers, stride), ref)      # positions t_len .. Tmax - 1 and the gaps: poison


def test_gather_txt_rows_refuses_bad_arguments_before_any_launch(lib):
    rows, Tmax, width, layers = 4, 8, 24, 2
    stride = rows * Tmax * width + 64
    src = poisoned(layers * stride, 1.0, BF)
    dst = poisoned(layers * stride + SPARE, NAN, BF)
    sr, past, neg = to_dev([2, 2, 0, 3], I32), to_dev([2, 4, 0, 3], I32), to_dev([2, -1, 0, 3], I32)
    ok = (ptr(src), ptr(dst), ptr(sr), rows, 5, Tmax, width, layers, stride)
    bad = [ok[:4] + (9,) + ok[5:], ok[:4] + (-1,) + ok[5:], ok[:4] + (1, Tmax, 20, layers, rows * Tmax * 20 + 64),      # t_len * width % 8
           ok[:8] + (stride + 4,), ok[:8] + (rows * Tmax * width - 8,), ok[:3] + (0,) + ok[4:], ok[:7] + (0,) + ok[8:], ok[:6] + (0,) + ok[7:],
           ok[:2] + (ptr(past),) + ok[3:], ok[:2] + (ptr(neg),) + ok[3:],
           (ptr(dst),) + ok[1:], (None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:2] + (None,) + ok[3:], (off_ptr(src, 8),) + ok[1:],
           ok[:1] + (off_ptr(dst, 8),) + ok[2:]]
    for args in bad:
        assert lib.gitcap_dbg_gather_txt_rows(*args, stream()) == ERR_ARG, args[3:]
    torch.cuda.synchronize()
    assert untouched(dst)
