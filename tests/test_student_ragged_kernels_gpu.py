"""The variable-length forms of the student's two cross-attention kernels (csrc/student.hip: attn_small_kernel<true>,
cross_probs_kernel<true>) through gitcap_dbg_attn_small_varlen / gitcap_dbg_cross_probs_varlen: a row whose table entry says n keys
holds, bit for bit, what the plain launch (gitcap_dbg_attn_small / gitcap_dbg_cross_probs) writes at nkeys = n on that row's keys.
Nothing here has a tolerance but the sum of a row of probabilities: 1 within 1e-6, the fp32 sum of at most 64 terms."""
import ctypes

import pytest
import torch

from gpu_support import NAN, assert_tail, lib, poisoned, ptr, same_bits, stream  # noqa: F401

pytestmark = pytest.mark.gpu

H, T = 2, 2
TAIL = 24
# (key_len per decoder row, clip of every row): rows 3 and 4 are a beam pair on clip 1; every length of {1, 2, 6, 33, 64} occurs
CASES = [([1, 33, 6, 33, 33], [0, 1, 2, 1, 1]), ([64, 2, 1, 2, 2], [0, 1, 2, 1, 1]), ([6, 6, 64, 6, 6], [2, 1, 0, 1, 1])]
GAP = 3             # packed rows between two clips that no table points at (NaN)


def _packed(lens, clip, hd, seed):
    """-> q bf16 [rows * T][H * hd], kv bf16 [packed rows][2 * H * hd] (k | v side by side, NaN wherever no table points),
    key_off / key_len int32 [rows] (device), off (host list)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows, D = len(lens), H * hd
    clip_len = {}
    for n, c in zip(lens, clip):
        assert clip_len.setdefault(c, n) == n
    off_of, at = {}, GAP
    for c in sorted(clip_len):
        off_of[c] = at
        at += clip_len[c] + GAP
    kv = torch.full((at, 2 * D), NAN, device="cuda", dtype=torch.bfloat16)
    for c, n in clip_len.items():
        kv[off_of[c]:off_of[c] + n] = torch.randn(n, 2 * D, device="cuda", generator=g).bfloat16()
        kv[off_of[c] + n - 1, D:] *= 8.0                       # the last key weighs 8 x: a length short by one shows
    q = torch.randn(rows * T, D, device="cuda", generator=g).bfloat16()
    off = [off_of[c] for c in clip]
    return q, kv, torch.tensor(off, dtype=torch.int32, device="cuda"), torch.tensor(lens, dtype=torch.int32, device="cuda"), off


def _args(q, k, v, ldkv, keys_stride, nkeys, ctx, M, hd):
    from gitcap._lib import CDbgAttnSmallArgs
    D = H * hd
    return CDbgAttnSmallArgs(q.data_ptr(), D, T, T, 0, k.data_ptr(), v.data_ptr(), ldkv, keys_stride, nkeys, 0, None, 0, 0, ctx.data_ptr(), D,
                             M, H, hd)


@pytest.mark.parametrize("hd", [72, 16])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_attn_small_varlen_is_the_plain_kernel_row_by_row(lib, hd, case):
    lens, clip = CASES[case]
    rows, D = len(lens), H * hd
    q, kv, key_off, key_len, off = _packed(lens, clip, hd, 40 + case)
    ctx = poisoned(rows * T * D + TAIL, NAN, torch.bfloat16)
    g = _args(q, kv, kv[:, D:], 2 * D, 0, 0, ctx, rows * T, hd)
    assert lib.gitcap_dbg_attn_small_varlen(ctypes.byref(g), ptr(key_off), ptr(key_len), stream()) == 0
    torch.cuda.synchronize()
    assert_tail(ctx, rows * T * D, NAN)
    got = ctx[:rows * T * D].view(rows, T, D)
    assert bool(torch.isfinite(got.float()).all())              # nothing outside a clip was read
    for r, (n, o) in enumerate(zip(lens, off)):
        one = poisoned(T * D + TAIL, NAN, torch.bfloat16)
        keys = kv[o:o + n].contiguous()
        g1 = _args(q[r * T:(r + 1) * T].contiguous(), keys, keys[:, D:], 2 * D, n, n, one, T, hd)
        assert lib.gitcap_dbg_attn_small(ctypes.byref(g1), stream()) == 0
        torch.cuda.synchronize()
        assert_tail(one, T * D, NAN)
        assert same_bits(got[r].contiguous(), one[:T * D].view(T, D)), f"row {r}: {n} keys at {o}"


@pytest.mark.parametrize("hd", [72, 16])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_cross_probs_varlen_is_the_plain_kernel_row_by_row(lib, hd, case):
    lens, clip = CASES[case]
    rows, D, F = len(lens), H * hd, 64
    q, kv, key_off, key_len, off = _packed(lens, clip, hd, 60 + case)
    probs = poisoned(rows * T * H * F + TAIL, NAN)
    fm = poisoned(rows * T * F + TAIL, NAN)
    rc = lib.gitcap_dbg_cross_probs_varlen(ptr(q), ptr(kv), 2 * D, rows, T, H, hd, F, None, ptr(probs), ptr(fm), F, ptr(key_off), ptr(key_len),
                                           stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert_tail(probs, rows * T * H * F, NAN)
    assert_tail(fm, rows * T * F, NAN)
    got = probs[:rows * T * H * F].view(rows, T, H, F)
    mass = fm[:rows * T * F].view(rows, T, F)
    for r, (n, o) in enumerate(zip(lens, off)):
        p1 = poisoned(T * H * n + TAIL, NAN)
        f1 = poisoned(T * n + TAIL, NAN)
        keys = kv[o:o + n].contiguous()
        assert lib.gitcap_dbg_cross_probs(ptr(q[r * T:(r + 1) * T].contiguous()), ptr(keys), 2 * D, 1, T, H, hd, n, None, ptr(p1), ptr(f1), n,
                                          stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(got[r, :, :, :n].contiguous(), p1[:T * H * n].view(T, H, n)), f"row {r}: {n} keys at {o}"
        assert bool((got[r, :, :, n:] == 0).all()) and bool((mass[r, :, n:] == 0).all())        # exact zeros beyond the clip
        assert same_bits(mass[r, :, :n].contiguous(), f1[:T * n].view(T, n))
        assert float((got[r].sum(-1) - 1).abs().max()) <= 1e-6


def test_varlen_hooks_refuse_bad_tables(lib):
    lens, clip = CASES[0]
    rows, hd = len(lens), 16
    D = H * hd
    q, kv, key_off, key_len, _ = _packed(lens, clip, hd, 1)
    ctx = poisoned(rows * T * D, NAN, torch.bfloat16)
    g = _args(q, kv, kv[:, D:], 2 * D, 0, 0, ctx, rows * T, hd)
    for bad in (0, 65, -1):
        kl = key_len.clone()
        kl[2] = bad
        assert lib.gitcap_dbg_attn_small_varlen(ctypes.byref(g), ptr(key_off), ptr(kl), stream()) != 0
    ko = key_off.clone()
    ko[0] = -1
    assert lib.gitcap_dbg_attn_small_varlen(ctypes.byref(g), ptr(ko), ptr(key_len), stream()) != 0
    assert lib.gitcap_dbg_attn_small_varlen(ctypes.byref(g), None, ptr(key_len), stream()) != 0
    probs, fm = poisoned(rows * T * H * 6, NAN), poisoned(rows * T * 6, NAN)
    # lengths of up to 33 against F = 6
    assert lib.gitcap_dbg_cross_probs_varlen(ptr(q), ptr(kv), 2 * D, rows, T, H, hd, 6, None, ptr(probs), ptr(fm), 6, ptr(key_off), ptr(key_len),
                                             stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx.float()).all()) and bool(torch.isnan(probs).all())      # a refused call launched nothing
