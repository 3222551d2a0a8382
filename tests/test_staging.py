"""tests/staging_reference.py kept honest without a GPU: the fp64 frame transform against ATen, its closed form, the row layouts
against torch's unfold, the table and gather functions against their index formulas, and the exactness of e4m3 x 2^k in bf16."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import staging_reference as R
from oracle.preprocess_oracle import image_transform
from text_rows_reference import U32, bf16_rne, e4m3_decode


@pytest.mark.parametrize("geom", R.PRE_GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_preprocess64_agrees_with_aten_on_small_geometries(geom):
    """max |aten - preprocess64| / (2^-24 magnitude) <= 32: twice the worst ratio measured on this list (ATen's fp32 weight arithmetic
    is not ours to bound term by term).  Measured on frames_u8(1, H, W, 100 + index), in the order of PRE_GEOMETRIES:
    9x16x8 5.6, 16x9x8 5.6, 11x11x8 1.6, 8x8x8 0.7, 5x7x8 5.1, 30x41x12 1.8, 37x53x28 10.0, 53x37x28 15.6, 29x28x28 1.1, 28x33x28 1.1,
    64x48x16 17.5, 17x16x16 0.9, 16x21x16 1.1, 100x300x32 2.2.  (Large frames do not belong here: at 240x320 -> 224 the ratio is
    about 300, the coordinate moving by an ulp near 200 in ATen's CPU build.)"""
    H, W, crop = geom
    img = R.frames_u8(1, H, W, 100 + R.PRE_GEOMETRIES.index(geom))[0]
    v, mag = R.preprocess64(img, crop)
    at = image_transform(torch.from_numpy(img), crop).numpy().astype(np.float64)
    assert at.shape == v.shape == mag.shape == (3, crop, crop)
    ratio = float((np.abs(at - v) / (U32 * mag)).max())
    print(f"{H}x{W}x{crop}: max |aten - fp64| / (2^-24 magnitude) = {ratio:.2f}")
    assert ratio <= 32.0


def test_identity_case_is_the_closed_form():
    img = R.frames_u8(1, 8, 8, 7)[0]
    v, mag = R.preprocess64(img, 8)
    p = img.astype(np.float64)[..., ::-1].transpose(2, 0, 1) / 255.0
    assert np.array_equal(v, (p - R.MEAN[:, None, None]) / R.STD[:, None, None])
    assert np.array_equal(mag, (p + R.MEAN[:, None, None]) / R.STD[:, None, None])
    # a wider frame whose resize is the identity: only the crop offset moves (33 - 28 = 5 -> left = round(2.5) = 2, half to even)
    img = R.frames_u8(1, 28, 33, 8)[0]
    assert R.geometry(28, 33, 28) == (28, 33, 0, 2) and R.geometry(53, 37, 28) == (40, 28, 6, 0) and R.geometry(30, 41, 12) == (12, 16, 0, 2)
    p = img.astype(np.float64)[:, 2:30, ::-1].transpose(2, 0, 1) / 255.0
    assert np.array_equal(R.preprocess64(img, 28)[0], (p - R.MEAN[:, None, None]) / R.STD[:, None, None])


def test_derived_constant_covers_every_frame_of_the_gpu_test():
    """PRE_C 2^-24 magnitude is at least the counted roundings, element by element, on the frames the GPU test launches"""
    worst = 0.0
    for i, (nf, H, W, crop) in enumerate(R.PRE_CASES):
        for img in R.pre_case_frames(i):
            c = float((R.preprocess_roundings(img, crop) / R.preprocess64(img, crop)[1]).max())
            worst = max(worst, c)
    print(f"largest counted roundings / magnitude over PRE_CASES: {worst:.1f} (PRE_C = {R.PRE_C})")
    assert worst <= R.PRE_C


def test_fp32_weights_stay_within_the_counted_horner_bound():
    """the evaluated fp32 weights (axis_taps) are within the half-ulp-per-intermediate count of the docstring: 24 u + the argument"""
    for n_src, n_new, off, crop in ((100, 32, 0, 32), (5, 8, 0, 8), (53, 40, 6, 28), (300, 96, 32, 32)):
        _, w, err = R.axis_taps(n_src, n_new, off, crop)
        assert np.allclose(w.sum(axis=1), 1.0, atol=1e-12)
        assert err.max() <= 26.0 and err.min() >= 0.5


@pytest.mark.parametrize("img,p,Kp", [(8, 4, 48), (8, 4, 64), (28, 14, 588), (42, 14, 640), (32, 16, 768)])
def test_patch_rows_are_unfold(img, p, Kp):
    fr = np.random.default_rng(img + Kp).standard_normal((2, 3, img, img)).astype(np.float32)
    rows = R.patch_rows(fr, p, Kp, fill=-7.0)
    ref = F.unfold(torch.from_numpy(fr), kernel_size=p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p).numpy()
    assert np.array_equal(rows[:, :3 * p * p], ref) and (rows[:, 3 * p * p:] == -7.0).all() and rows.shape == (2 * (img // p) ** 2, Kp)


@pytest.mark.parametrize("crop", [8, 14, 28])
def test_stem_rows_are_unfold(crop):
    fr = np.random.default_rng(crop).standard_normal((3, 3, crop, crop)).astype(np.float32)
    rows = R.stem_rows(fr)
    ref = F.unfold(torch.from_numpy(fr), kernel_size=3, stride=2, padding=1).transpose(1, 2).reshape(-1, 27).numpy()
    assert np.array_equal(rows[:, :27], ref) and (rows[:, 27:] == 0).all() and rows.shape == (3 * (crop // 2) ** 2, 32)


def test_ring_tables_and_gathers_follow_their_index_formulas():
    rng = np.random.default_rng(0)
    ring = np.full((2, 3, 2, 4), -1.0, np.float32)
    src = rng.standard_normal((2, 2, 2, 4)).astype(np.float32)
    R.window_scatter(ring, src, head=2)                                   # slots 2 and 0; slot 1 untouched
    assert np.array_equal(ring[:, 2], src[:, 0]) and np.array_equal(ring[:, 0], src[:, 1]) and (ring[:, 1] == -1.0).all()
    temporal = rng.standard_normal((3, 4)).astype(np.float32)
    out = R.window_assemble(ring, temporal, head=2).reshape(2, 3, 2, 4)
    for f in range(3):
        assert np.array_equal(out[:, f], ring[:, (2 + f) % 3] + temporal[f])
    assert np.array_equal(R.window_assemble(ring, None, 1).reshape(2, 3, 2, 4)[:, 2], ring[:, 0])
    off, ln, pos = R.ragged_tables([3, 1, 2], 5)
    assert off.tolist() == [0, 15, 20] and ln.tolist() == [15, 5, 10] and pos.tolist() == [0, 1, 2, 0, 0, 1]
    x = rng.standard_normal((6 * 5, 4)).astype(np.float32)
    t6 = rng.standard_normal((4, 4)).astype(np.float32)
    assert np.array_equal(R.ragged_temporal(x, t6, pos, 5)[17], x[17] + t6[0]) and np.array_equal(R.ragged_temporal(x, t6, pos, 5)[14], x[14] + t6[2])
    img = rng.standard_normal((3, 2 * 5, 4)).astype(np.float32)
    txt = rng.standard_normal((3, 2 * 4, 4)).astype(np.float32)
    g = R.gather_hidden(img, txt, B=2, S_img=5, T=4)
    assert g.shape == (2, 3, 9, 4) and np.array_equal(g[1, 2, 4], img[2, 9]) and np.array_equal(g[1, 0, 5], txt[0, 4])
    s = rng.standard_normal((3, 4, 8, 6)).astype(np.float32)
    d = R.gather_txt_rows(s, np.full_like(s, 9.0), [2, 2, 0, 3], 5)
    assert np.array_equal(d[:, 1, :5], s[:, 2, :5]) and np.array_equal(d[:, 2, :5], s[:, 0, :5]) and (d[:, :, 5:] == 9.0).all()


def test_every_e4m3_code_times_a_power_of_two_is_a_bf16_value():
    """the exactness claim of the dequantisation (csrc/common.h), independently of the kernel: bf16_rne is the identity"""
    codes = np.arange(256)
    ok = (codes & 0x7f) != 0x7f
    assert sorted(codes[~ok].tolist()) == sorted(R.E4M3_NAN_CODES)
    for e in R.DEQUANT_EXPONENTS:
        v = e4m3_decode(codes[ok]) * 2.0 ** e
        assert np.array_equal(bf16_rne(v), v), e
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), e
    d = R.dequant(codes[None, :], [2.0 ** -9])
    assert np.isnan(d[0, 0x7f]) and np.isnan(d[0, 0xff]) and d[0, 0x01] == 2.0 ** -18 and d[0, 0x7e] == 448 * 2.0 ** -9 and d[0, 0x80] == 0
    assert np.signbit(d[0, 0x80]) and not np.signbit(d[0, 0])


def test_bf16_bit_helpers_agree_with_torch():
    x = np.random.default_rng(3).standard_normal(4096).astype(np.float32) * np.float32(3.0)
    x[:8] = [np.nan, np.inf, -np.inf, 1.00390625, 1.01171875, -0.0, 3.3895314e38, 1e-40]        # NaN, infinities, two ties, -0, overflow, denormal
    ref = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_of_f32(x)
    assert np.array_equal(got[1:], ref[1:]) and (got[0] & 0x7fff) > 0x7f80 and (ref[0] & 0x7fff) > 0x7f80
    vals = torch.from_numpy(ref[1:].view(np.int16)).view(torch.bfloat16).double().numpy()
    assert np.array_equal(R.bits_of_bf16(vals), ref[1:])
