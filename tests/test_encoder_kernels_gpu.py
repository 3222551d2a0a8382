"""The TinyViT encoder's kernels (csrc/tinyvit.hip) and the student decoder's attn_small (csrc/student.hip) on the MI355X, one kernel
at a time through the gitcap_dbg_tv_* / gitcap_dbg_attn_small hooks, against the fp64 restatement of tests/encoder_kernels_reference.py
on the same bf16 operands.

Tolerances are derived, not measured on the device (encoder_kernels_reference.py has the terms): half a bf16 ulp of the fp64 value
plus the fp32 error of what was rounded.  The one term no documentation gives, the fast exp of the two attention kernels, is measured
on the CPU with an fp32 restatement of each kernel's loop (4 x it, capped at a quarter of a bf16 ulp).  As a condition, at most 2 % of
a case's elements may differ from the correctly rounded reference at all; tests/test_encoder_kernels.py shows on the CPU that an fp32
implementation meets it on these inputs, and that subtly wrong kernels miss the bounds by more than 10 x.  im2col and to_nchw are exact.

Every output buffer is larger than what the kernel may write and filled with NaN (0xABAB for the exact bf16 outputs); pad columns of
strided operands hold NaN; what must not be written is checked after every launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import encoder_kernels_reference as E
from gpu_support import bf16_bits, close_to_fp64, f64, lib, ptr, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
POISON16 = 0xABAB - 0x10000              # 0xABAB as int16


def _nan(count, dtype=torch.bfloat16):
    return torch.full((count,), NAN, device="cuda", dtype=dtype)


def _strided(a, ld, rows=None):
    """a [M][N] -> device bf16 [rows][ld], NaN in the pad columns and rows"""
    return to_dev(E.tv_gemm_buffer(np.asarray(a), rows or a.shape[0], ld), torch.bfloat16)


# ---- tv_gemm ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, K, epi):
    a = E.gemm_inputs(M, N, K, epi, seed=100 + M + N + K)
    return a, E.tv_gemm(a["A"], a["W"], a["bias"], a["res"], epi)


def _gemm(lib, a, M, N, K, epi, lda, ldo, ldr, inplace=False):
    """-> the whole output buffer [M + 2][ldo] (bf16); its tail is checked here.  inplace: res == out (ldr = ldo), the buffer starts as
    the residual with NaN in its pad columns and rows."""
    A, W, bias = _strided(a["A"], lda), to_dev(a["W"], torch.bfloat16), to_dev(a["bias"], torch.float32)
    rows = M + 2
    out = _nan(rows * ldo + 32)
    res = None
    if inplace:
        assert ldr == ldo
        out[:rows * ldo] = _strided(a["res"], ldo, rows).reshape(-1)
        res = out
    elif epi & E.TV_RES:
        res = _strided(a["res"], ldr, M + 1)
    rc = lib.gitcap_dbg_tv_gemm(ptr(A), lda, ptr(W), ptr(bias), ptr(res), ldr, ptr(out), ldo, M, N, K, epi, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(out[rows * ldo:]).all())
    return out[:rows * ldo].view(rows, ldo)


def _gemm_written(buf, M, N):
    """rows >= M and columns >= N of every row are still poison -> the [M][N] block"""
    keep = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:M, :N] = True
    assert bool(torch.isnan(buf[~keep]).all()), "a store outside the rows / columns of the launch"
    return buf[:M, :N].contiguous()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("M,N,K,epi", E.GEMM_CASES)
def test_tv_gemm_against_fp64(lib, M, N, K, epi, wide):
    a, (ref, bound) = _gemm_case(M, N, K, epi)
    lda, ldo, ldr = E.gemm_strides(N, K, wide)
    got = _gemm_written(_gemm(lib, a, M, N, K, epi, lda, ldo, ldr), M, N)
    close_to_fp64(f64(got), ref, bound, f"tv_gemm M={M} N={N} K={K} epi={epi} lda={lda} ldo={ldo} ldr={ldr}")


@pytest.mark.parametrize("M,N,K,epi", [c for c in E.GEMM_CASES if c[3] & E.TV_RES])
def test_tv_gemm_in_place_residual_gives_the_same_bits(lib, M, N, K, epi):
    """res == out, as the encoder calls it; in both layouts, against the out-of-place launch."""
    a, _ = _gemm_case(M, N, K, epi)
    want = bf16_bits(_gemm_written(_gemm(lib, a, M, N, K, epi, K, N, N), M, N))
    for wide in (False, True):
        lda, ldo, _ = E.gemm_strides(N, K, wide)
        got = _gemm_written(_gemm(lib, a, M, N, K, epi, lda, ldo, ldo, inplace=True), M, N)
        assert np.array_equal(bf16_bits(got), want), wide


def test_tv_gemm_hook_rejects_bad_arguments(lib):
    x = torch.zeros(64 * 64, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(64, device="cuda")
    out = _nan(64 * 64)

    def rc(M=4, N=8, K=32, lda=32, ldo=8, ldr=8, epi=0, res=None, A=x, o=out):
        return lib.gitcap_dbg_tv_gemm(ptr(A), lda, ptr(x), ptr(b), ptr(res), ldr, ptr(o), ldo, M, N, K, epi, stream())

    assert rc(N=6) != 0 and rc(K=48, lda=48) != 0 and rc(lda=36) != 0 and rc(ldo=10) != 0 and rc(ldr=10, epi=E.TV_RES, res=x) != 0
    assert rc(epi=3) != 0 and rc(epi=E.TV_RES_GELU) != 0 and rc(epi=E.TV_GELU | E.TV_RES, res=x) != 0 and rc(epi=8) != 0
    assert rc(epi=E.TV_RES) != 0 and rc(epi=E.TV_RES | E.TV_RES_GELU) != 0                   # a residual epilogue without a residual
    assert rc(lda=24) != 0 and rc(ldo=4) != 0 and rc(ldr=4, epi=E.TV_RES, res=x) != 0 and rc(M=0) != 0 and rc(A=None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert rc() == 0 and rc(epi=E.TV_RES, res=x) == 0
    torch.cuda.synchronize()
    assert bool((out[:32] == 0).all()) and bool(torch.isnan(out[32:]).all())


# ---- tv_im2col / tv_to_nchw (exact) -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f32_nchw", [True, False])
@pytest.mark.parametrize("n,H,W,Cin,Kp", E.IM2COL_CASES)
def test_tv_im2col_is_exact(lib, n, H, W, Cin, Kp, f32_nchw):
    x = E.im2col_inputs(n, H, W, Cin, f32_nchw, seed=n + H + W + Cin)
    dx = to_dev(x, torch.float32 if f32_nchw else torch.bfloat16)
    count = n * (H // 2) * (W // 2) * Kp
    out = torch.full((count + 64,), POISON16, device="cuda", dtype=torch.int16)
    rc = lib.gitcap_dbg_tv_im2col(ptr(dx), int(f32_nchw), ptr(out), n, H, W, Cin, Kp, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out[count:] == POISON16).all())
    want = E.tv_im2col(x, f32_nchw, Kp)
    assert np.array_equal(out[:count].cpu().numpy().view(np.uint16).reshape(want.shape), bf16_bits(to_dev(want, torch.bfloat16)).reshape(want.shape))
    assert not out[:count].view(-1, Kp)[:, 9 * Cin:].any()                                  # the pad columns are +0, bit for bit


def test_tv_im2col_hook_rejects_bad_arguments(lib):
    x = torch.zeros(4096, device="cuda")
    out = torch.full((4096,), POISON16, device="cuda", dtype=torch.int16)
    rc = lambda n=1, H=4, W=4, Cin=3, Kp=32, i=x, o=out: lib.gitcap_dbg_tv_im2col(ptr(i), 1, ptr(o), n, H, W, Cin, Kp, stream())
    assert rc(H=3) != 0 and rc(W=5) != 0 and rc(Kp=26) != 0 and rc(Cin=4) != 0 and rc(n=0) != 0 and rc(i=None) != 0 and rc(o=None) != 0
    torch.cuda.synchronize()
    assert bool((out == POISON16).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not out[:4 * 32].any() and bool((out[4 * 32:] == POISON16).all())


@pytest.mark.parametrize("n,HW,C", E.NCHW_CASES)
def test_tv_to_nchw_is_exact(lib, n, HW, C):
    x = E.pool_inputs(n, HW, C, seed=400 + n + HW + C)
    out, dx = _nan(n * HW * C + 16, torch.float32), to_dev(x, torch.bfloat16)
    rc = lib.gitcap_dbg_tv_to_nchw(ptr(dx), ptr(out), n, HW, C, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(out[n * HW * C:]).all())
    assert np.array_equal(f64(out[:n * HW * C]).reshape(n, C, HW), E.tv_to_nchw(x))


# ---- tv_dwconv ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,H,W,C,stride,g", E.DWCONV_CASES)
def test_tv_dwconv_against_fp64(lib, n, H, W, C, stride, g):
    a = E.dwconv_inputs(n, H, W, C, seed=200 + n + H + W + C)
    count = n * (H // stride) * (W // stride) * C
    out = _nan(count + 64)
    x, w9, bias = to_dev(a["x"], torch.bfloat16), to_dev(a["w9"], torch.float32), to_dev(a["bias"], torch.float32)
    rc = lib.gitcap_dbg_tv_dwconv(ptr(x), ptr(w9), ptr(bias), ptr(out), n, H, W, C, stride, int(g), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(out[count:]).all())
    ref, bound = E.tv_dwconv(a["x"], a["w9"], a["bias"], stride, g)
    close_to_fp64(f64(out[:count]).reshape(ref.shape), ref, bound, f"tv_dwconv n={n} H={H} W={W} C={C} stride={stride} gelu={g}")


def test_tv_dwconv_hook_rejects_bad_arguments(lib):
    x = torch.zeros(4096, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(4096, device="cuda")
    out = _nan(4096)
    rc = lambda n=1, H=4, W=4, C=8, stride=1, i=x, o=out: lib.gitcap_dbg_tv_dwconv(ptr(i), ptr(w), ptr(w), ptr(o), n, H, W, C, stride, 0, stream())
    assert rc(C=12) != 0 and rc(C=4) != 0 and rc(stride=0) != 0 and rc(stride=3) != 0 and rc(stride=2, H=3) != 0 and rc(stride=2, W=5) != 0
    assert rc(n=0) != 0 and rc(i=None) != 0 and rc(o=None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert rc() == 0 and rc(stride=1, H=3, W=5) == 0
    torch.cuda.synchronize()
    assert bool((out[:128] == 0).all()) and bool(torch.isnan(out[128:]).all())


# ---- tv_ln ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,C", E.LN_CASES)
def test_tv_ln_against_fp64(lib, M, C):
    """The last row of a case with more than one has a mean of 257 and a spread of 1."""
    q = E.ln_inputs(M, C, seed=300 + M + C)
    out = _nan(M * C + 64)
    x, g, b = to_dev(q["x"], torch.bfloat16), to_dev(q["g"], torch.float32), to_dev(q["b"], torch.float32)
    rc = lib.gitcap_dbg_tv_ln(ptr(x), ptr(g), ptr(b), ptr(out), M, C, q["eps"], stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(out[M * C:]).all())
    ref, bound = E.tv_ln(**q)
    close_to_fp64(f64(out[:M * C]).reshape(M, C), ref, bound, f"tv_ln M={M} C={C}")


def test_tv_ln_hook_rejects_bad_arguments(lib):
    x = torch.zeros(8192, device="cuda", dtype=torch.bfloat16)
    g = torch.ones(4096, device="cuda")
    out = _nan(8192)
    rc = lambda M=2, C=32, i=x, o=out: lib.gitcap_dbg_tv_ln(ptr(i), ptr(g), ptr(g), ptr(o), M, C, 1e-5, stream())
    assert rc(C=12) != 0 and rc(C=2056) != 0 and rc(C=4096, M=1) != 0 and rc(M=0) != 0 and rc(C=0) != 0 and rc(i=None) != 0 and rc(o=None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool((out[:64] == 1).all()) and bool(torch.isnan(out[64:]).all())               # LN(0) gamma + beta = beta = 1


# ---- tv_pool -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,HW,C", E.POOL_CASES)
def test_tv_pool_against_fp64(lib, n, HW, C):
    x = E.pool_inputs(n, HW, C, seed=400 + n + HW + C)
    mem, dx = _nan(n * C + 16, torch.float32), to_dev(x, torch.bfloat16)
    rc = lib.gitcap_dbg_tv_pool(ptr(dx), ptr(mem), n, HW, C, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(mem[n * C:]).all())
    ref, bound = E.tv_pool(x)
    close_to_fp64(mem[:n * C].cpu().numpy().astype(np.float64).reshape(n, C), ref, bound + 1e-300, f"tv_pool n={n} HW={HW} C={C}", flips=False)


def test_tv_pool_and_to_nchw_hooks_reject_bad_arguments(lib):
    x = torch.zeros(4096, device="cuda", dtype=torch.bfloat16)
    out = _nan(4096, torch.float32)
    for fn in (lib.gitcap_dbg_tv_pool, lib.gitcap_dbg_tv_to_nchw):
        rc = lambda n=1, HW=4, C=32, i=x, o=out: fn(ptr(i), ptr(o), n, HW, C, stream())
        assert rc(n=0) != 0 and rc(HW=0) != 0 and rc(C=0) != 0 and rc(i=None) != 0 and rc(o=None) != 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
    assert lib.gitcap_dbg_tv_pool(ptr(x), ptr(out), 1, 4, 32, stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[:32] == 0).all()) and bool(torch.isnan(out[32:]).all())


# ---- tv_attn --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(E.TV_ATTN_CASES)))
def test_tv_attn_against_fp64(lib, i):
    """The hook expands the compact table with the function gitcap_tinyvit_finalize uses: the index rule is under test with the kernel."""
    n, H, W, heads, ws, kind = case = E.TV_ATTN_CASES[i]
    a = E.tv_attn_inputs(*case, seed=500 + i)
    count = n * H * W * heads * 32
    ctx = _nan(count + 64)
    qkv, ab = to_dev(a["qkv"], torch.bfloat16), to_dev(a["ab"], torch.float32)
    rc = lib.gitcap_dbg_tv_attn(ptr(qkv), ptr(ab), ptr(ctx), n, H, W, heads, ws, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(ctx[count:]).all())
    ref = E.tv_attn(a["qkv"], a["ab"], n, H, W, heads, ws)
    close_to_fp64(f64(ctx[:count]).reshape(ref.shape), ref, E.attn_bound(ref, E.DELTA_TV_ATTN_MEASURED), f"tv_attn {case}")


def test_tv_attn_hook_rejects_bad_arguments(lib):
    x = torch.zeros(16 * 96, device="cuda", dtype=torch.bfloat16)
    ab = torch.zeros(256, device="cuda")
    ctx = _nan(16 * 32 + 64)
    rc = lambda n=1, H=4, W=4, heads=1, ws=2, i=x, t=ab, o=ctx: lib.gitcap_dbg_tv_attn(ptr(i), ptr(t), ptr(o), n, H, W, heads, ws, stream())
    assert rc(ws=0) != 0 and rc(ws=15, H=15, W=15) != 0 and rc(ws=3) != 0 and rc(H=3, ws=3) != 0 and rc(W=6, ws=4) != 0
    assert rc(n=0) != 0 and rc(heads=0) != 0 and rc(i=None) != 0 and rc(t=None) != 0 and rc(o=None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool((ctx[:16 * 32] == 0).all()) and bool(torch.isnan(ctx[16 * 32:]).all())


# ---- attn_small ----------------------------------------------------------------------------------------------------------------------

def _attn_small(lib, a, **override):
    """One launch on the operands of E.attn_small_inputs: q in a ring of q_rows rows per text row (ldq = H hd + 8), k | v side by side
    in one buffer of keys + 2 rows per text row (ldkv = 2 H hd + 8; the rows behind the keys and the pad columns are NaN), ctx
    [M + 1][H hd + 4].  -> (status, ctx [M][H][hd] as fp64); the poison around ctx is checked here."""
    from gitcap._lib import CDbgAttnSmallArgs
    rows, T, H, hd, keys = a["rows"], a["T"], a["H"], a["hd"], a["keys"]
    D, M = H * hd, rows * T
    ldq, ldkv, ldc, kstride = D + 8, 2 * D + 8, D + 4, keys + 2
    q = _strided(a["q"].reshape(rows * a["q_rows"], D), ldq)
    kv = np.full((rows, kstride, ldkv), np.nan)
    kv[:, :keys, :D] = a["k"].reshape(rows, keys, D)
    kv[:, :keys, D:2 * D] = a["v"].reshape(rows, keys, D)
    kv = to_dev(kv, torch.bfloat16)
    ids = to_dev(a["ids"], torch.int64)
    ctx = _nan((M + 1) * ldc + 32)
    g = CDbgAttnSmallArgs()
    g.q, g.ldq, g.T, g.q_row_stride, g.q_row_off = ptr(q).value, ldq, T, a["q_rows"], a["q_row_off"]
    g.k, g.v, g.ldkv, g.keys_stride, g.nkeys, g.t0 = ptr(kv).value, ptr(kv).value + 2 * D, ldkv, kstride, a["nkeys"], a["t0"]
    g.ids, g.ld_ids, g.pad_id = (ptr(ids).value if ids is not None else None), keys + 2, a["pad_id"]
    g.ctx, g.ldc, g.M, g.H, g.hd = ptr(ctx).value, ldc, M, H, hd
    for k, v in override.items():
        setattr(g, k, v)
    rc = lib.gitcap_dbg_attn_small(ctypes.byref(g), stream())
    torch.cuda.synchronize()
    if rc != 0:
        assert bool(torch.isnan(ctx).all())
        return rc, None
    assert bool(torch.isnan(ctx[M * ldc:]).all())
    buf = ctx[:M * ldc].view(M, ldc)
    assert bool(torch.isnan(buf[:, D:]).all())
    return 0, f64(buf[:, :D]).reshape(M, H, hd)


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("i", range(len(E.ATTN_SMALL_CASES)))
def test_attn_small_against_fp64(lib, i, with_ids):
    """A query whose keys are all PAD gives NaN on both sides (case 0 with ids, and the first position of a row that starts with PAD)."""
    case = E.ATTN_SMALL_CASES[i]
    a = E.attn_small_inputs(*case, with_ids, seed=600 + i)
    rc, got = _attn_small(lib, a)
    assert rc == 0
    ref = E.attn_small(a)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN exactly where every key of a query is masked"
    ok = ~np.isnan(ref)
    if i == 0 and with_ids:
        assert not ok.any()
    else:
        close_to_fp64(got[ok], ref[ok], E.attn_bound(ref, E.DELTA_ATTN_SMALL_MEASURED)[ok], f"attn_small {case} ids={with_ids}")


def test_attn_small_hook_rejects_bad_arguments(lib):
    a = E.attn_small_inputs(2, 3, 5, 0, 2, 32, True, seed=1)
    for bad in (dict(hd=12), dict(hd=136), dict(hd=0), dict(nkeys=65), dict(nkeys=-1), dict(t0=62), dict(t0=-1), dict(T=0), dict(M=5),
                dict(M=0), dict(H=0), dict(ldq=32), dict(ldkv=132), dict(ldkv=56), dict(ldc=60), dict(ld_ids=7), dict(q=None), dict(k=None),
                dict(v=None), dict(ctx=None)):
        rc, _ = _attn_small(lib, a, **bad)
        assert rc != 0, bad
    assert lib.gitcap_dbg_attn_small(None, stream()) != 0
    assert _attn_small(lib, a)[0] == 0
