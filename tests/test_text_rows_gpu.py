"""The decoder's text-row kernels on the MI355X, one launcher at a time through the gitcap_dbg_* hooks, against the fp64 restatement
of tests/text_rows_reference.py on the same bf16 / e4m3 operands: pack_frags, kv_quant_v (exact), skinny with and without its row
prologue, skinny_splitk, ln_reduce, ffn_txt and txt_block (derived bounds), and the bitwise equalities their sources claim.

Tolerances are derived, not measured (text_rows_reference.py has the terms): a bf16 output may differ from the fp64 value by half a
bf16 ulp of that value plus the fp32 error of what was rounded -- gamma(K) sum|x||w| for the accumulator, one rounding for the bias,
the erf polynomial's 1.5e-7 for GELU.  Where the fp64 value lies within that fp32 error of a rounding boundary the device may round
the other way: the bound allows it, and as a condition (not a measurement) at most 2 % of a case's elements may differ from the
correctly rounded reference at all; test_text_rows.py shows on the CPU that an fp32 implementation stays under that share on these
inputs.  fp32 outputs (split-K slabs) carry the accumulator term alone.  A LayerNorm output is compared through ln_bound; its bf16
copy must be exactly the rounding of the device's own fp32 row.  Projections behind a row prologue and FC2 behind FC1 are judged on
the device's own bf16 operand bits, so that each stage is measured by itself.

txt_block is judged where a wrong key, clip or head shows undiluted: `part`, per head, against |Wo_h| (2^-8 |ctx| + 2^-8 sum_k p_k
|v_k| + delta) + gamma(64) |Wo_h| |ctx| -- the bf16 rounding of the context on either side of a boundary, the documented bf16
rounding of P in the PV product, the measured fp32 softmax term delta (4 x the measurement, capped at a quarter of a bf16 ulp of the
context, which is what governs here since the measurement, 0.0157, is taken behind the context's own rounding:
text_rows_reference.txt_delta, profiles/r11_text_row_kernels.txt), and the fp32 accumulator of the 64 products.  x1 is
compared with the exact fp64 LayerNorm of the device's own sum of partials (ln_bound with the reducer's summation order), which
isolates the reducer; xsb must be exactly the bf16 of xs.

Every output buffer is larger than what the kernel may write and filled with NaN (0xAB for codes); what must not be written is
checked after every launch."""
import ctypes

import numpy as np
import pytest
import torch

import text_rows_reference as R
from gpu_support import close_to_fp64, f64, lib, ptr, same_bits, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _weights(a, key="W", ckey="Wcodes", skey="wscale"):
    """device weight (bf16, or uint8 codes) and scale"""
    if a[ckey] is not None:
        return to_dev(a[ckey], torch.uint8), to_dev(a[skey], torch.float32)
    return to_dev(a[key], torch.bfloat16), None


def _pack(lib, W):
    rows, K = W.shape
    eb = W.element_size()
    n = rows * K
    buf = torch.full((n + 64,), 0x2B, device="cuda", dtype=torch.uint8) if eb == 1 else torch.full((n + 64,), NAN, device="cuda", dtype=torch.bfloat16)
    assert lib.gitcap_dbg_pack_frags(ptr(W), ptr(buf), rows, K, eb, stream()) == 0
    torch.cuda.synchronize()
    tail = buf[n:]
    assert bool((tail == 0x2B).all()) if eb == 1 else bool(torch.isnan(tail).all())
    return buf[:n]


# ---- pack_frags -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eb", [2, 1])
@pytest.mark.parametrize("rows16,K", [(16, 32), (48, 64), (16, 768), (48, 768), (48, 32)])
def test_pack_frags_is_the_index_formula(lib, rows16, K, eb):
    rng = np.random.default_rng(rows16 * K + eb)
    src = rng.integers(0, 256 if eb == 1 else 65536, size=(rows16, K)).astype(np.uint8 if eb == 1 else np.uint16)
    dsrc = torch.as_tensor(src.astype(np.int32)).to("cuda").to(torch.uint8) if eb == 1 else \
        torch.as_tensor(src.astype(np.int16)).to("cuda").view(torch.bfloat16)
    got = _pack(lib, dsrc)
    got = got.cpu().numpy() if eb == 1 else got.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, R.pack_frags(src))


# ---- kv_quant_v -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 7, 33])
@pytest.mark.parametrize("D,H", [(128, 2), (768, 12)])
def test_kv_quant_v_codes_and_scales_exact(lib, rows, D, H):
    pitch = rows + 5
    kv = R.kv_quant_inputs(rows, D, H, seed=rows + D)
    dkv = to_dev(kv, torch.bfloat16)
    assert np.array_equal(f64(dkv), kv)                                     # the inputs are bf16 values (denormals included)
    v8 = torch.full((H * pitch * 64 + 64,), 0xAB, device="cuda", dtype=torch.uint8)
    vs = torch.full((H * pitch + 16,), NAN, device="cuda")
    assert lib.gitcap_dbg_kv_quant_v(ptr(dkv), ptr(v8), ptr(vs), rows, D, H, pitch, stream()) == 0
    torch.cuda.synchronize()
    codes, scales, written = R.kv_quant_v(kv, D, H, pitch)
    g8 = v8[:H * pitch * 64].cpu().numpy().reshape(H, pitch, 64)
    gs = vs[:H * pitch].cpu().numpy().astype(np.float64).reshape(H, pitch)
    assert bool((v8[H * pitch * 64:] == 0xAB).all()) and bool(torch.isnan(vs[H * pitch:]).all())
    assert (g8[~written] == 0xAB).all() and np.isnan(gs[~written]).all()          # pitch > rows: nothing behind a head's rows
    assert np.array_equal(gs[written], scales[written])
    assert np.array_equal(g8[written], codes[written])
    val = R.e4m3_decode(g8[written]) * gs[written][:, None]
    assert np.isfinite(val).all() and np.array_equal(val, R.bf16_rne(val))       # code * scale is a bf16 value


# ---- skinny -----------------------------------------------------------------------------------------------------------------------

def _skinny(lib, *, X=None, W, Wpk=None, wscale=None, bias=None, M, N, K, epi, T=1, row_stride=1, row_off=0, ln=None, ldx=None):
    """-> out [n_rows][ldo] as fp64 with NaN where nothing was written (checked: the buffer's tail), and xf [M][K] for a prologue."""
    from gitcap._lib import CDbgSkinnyArgs
    n_rows = ((M + T - 1) // T) * max(row_stride, T) + 2
    ldo = (N + 3) // 4 * 4 + 8
    out = torch.full((n_rows * ldo + 32,), NAN, device="cuda", dtype=torch.bfloat16)
    a = CDbgSkinnyArgs()
    a.X = ptr(X).value if X is not None else None
    a.ldx = ldx or K
    a.W, a.Wpk = ptr(W).value, (ptr(Wpk).value if Wpk is not None else None)
    a.wscale = ptr(wscale).value if wscale is not None else None
    a.bias = ptr(bias).value if bias is not None else None
    a.M, a.N, a.K = M, N, K
    a.out, a.ldo, a.T, a.row_stride, a.row_off = ptr(out).value, ldo, T, row_stride, row_off
    xf = None
    if ln is not None:
        xf = torch.full((M * K + 16,), NAN, device="cuda")
        a.ln_kind = ln["kind"]
        for k in ("slabs", "bias", "resid", "ids", "word", "pos", "g", "b"):
            if ln.get(k) is not None:
                setattr(a, "ln_" + k, ptr(ln[k]).value)
        a.ln_nslab, a.ln_ld_ids, a.ln_T, a.ln_t0, a.ln_vocab = ln.get("nslab", 0), ln.get("ld_ids", 0), ln.get("T", 0), ln.get("t0", 0), ln.get("vocab", 0)
        a.ln_eps = ln["eps"]
        a.ln_xf = ptr(xf).value
    rc = lib.gitcap_dbg_skinny(ctypes.byref(a), epi, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(out[n_rows * ldo:]).all())
    if xf is not None:
        assert bool(torch.isnan(xf[M * K:]).all())
        xf = xf[:M * K].view(M, K)
    return out[:n_rows * ldo].view(n_rows, ldo), xf


@pytest.mark.parametrize("M,N,K,fp8,epi,T,row_stride,row_off", R.SKINNY_CASES)
def test_skinny_against_fp64(lib, M, N, K, fp8, epi, T, row_stride, row_off):
    a = R.gemm_inputs(M, N, K, fp8, seed=1000 + M + N + K)
    X, bias = to_dev(a["X"], torch.bfloat16), to_dev(a["bias"], torch.float32)
    W, ws = _weights(a)
    out, _ = _skinny(lib, X=X, W=W, wscale=ws, bias=bias, M=M, N=N, K=K, epi=epi, T=T, row_stride=row_stride, row_off=row_off)
    out_pk, _ = _skinny(lib, X=X, W=W, Wpk=_pack(lib, W), wscale=ws, bias=bias, M=M, N=N, K=K, epi=epi, T=T, row_stride=row_stride,
                        row_off=row_off)
    assert same_bits(out, out_pk)                                               # Wpk set versus unset: the same bits
    ref, bound = R.skinny(a["X"], a["W"], a["wscale"], a["bias"], N, epi)
    got = f64(out)
    want = R.scatter_rows(ref, T, row_stride, row_off, got.shape[0])
    mask = np.zeros(got.shape, bool)
    mask[:, :N] = ~np.isnan(want)
    assert np.isnan(got[~mask]).all(), "a store outside the rows / columns of the launch"      # rows between the scatter, columns >= N
    rows = [R.orow(m, T, row_stride, row_off) for m in range(M)]
    close_to_fp64(got[rows, :N], ref, bound, f"skinny M={M} N={N} K={K} fp8={fp8} epi={epi}")


@pytest.mark.parametrize("M,K,kind,nslab", R.PROLOGUE_CASES)
def test_skinny_row_prologue(lib, M, K, kind, nslab):
    """kind 1: the bits of ln_reduce followed by the plain launch, with the three-wave form on and off; both kinds against fp64."""
    N = 3 * K if K <= 128 else 2304
    a = R.gemm_inputs(M, N, K, False, seed=2000 + M + K + kind)
    W, bias = to_dev(a["W"], torch.bfloat16), to_dev(a["bias"], torch.float32)
    if kind == 1:
        q = R.ln_inputs(M, K, nslab, seed=K + nslab, hard_row=False)
        d = {k: to_dev(q[k], torch.float32) for k in ("slabs", "bias", "resid", "g", "b")}
        ln = dict(kind=1, nslab=nslab, eps=q["eps"], **d)
        xf0, xb0 = _ln_reduce(lib, d, nslab, q["eps"], M, K)
        plain, _ = _skinny(lib, X=xb0, W=W, bias=bias, M=M, N=N, K=K, epi=0, T=1, row_stride=3, row_off=1)
        for rows3 in (1, 0):
            old = lib.gitcap_dbg_config(11, rows3)
            try:
                out, xf = _skinny(lib, W=W, bias=bias, M=M, N=N, K=K, epi=0, T=1, row_stride=3, row_off=1, ln=ln)
            finally:
                lib.gitcap_dbg_config(11, old)
            assert same_bits(xf, xf0) and same_bits(out, plain), rows3
        want_x, bx = R.prologue_rows(1, **q)
    else:
        T = 2 if (M == 2 and K == 576) else 1
        q = R.embed_inputs(M, K, seed=K + M, T=T)
        ln = dict(kind=2, eps=q["eps"], ids=to_dev(q["ids"], torch.int64), ld_ids=T, T=T, t0=q["t0"], vocab=q["vocab"],
                  **{k: to_dev(q[k], torch.float32) for k in ("word", "pos", "g", "b")})
        out, xf = _skinny(lib, W=W, bias=bias, M=M, N=N, K=K, epi=0, T=1, row_stride=3, row_off=1, ln=ln)
        want_x, bx = R.prologue_rows(2, ids=q["ids"], T=T, t0=q["t0"], word=q["word"], pos=q["pos"], g=q["g"], b=q["b"], eps=q["eps"])
    close_to_fp64(f64(xf), want_x, bx, f"prologue kind {kind} M={M} K={K} nslab={nslab}: xf", flips=False)
    xb = R.bf16_rne(f64(xf))                                                 # the GEMM operand: the bf16 of the device's own row
    ref, bound = R.skinny(xb, a["W"], None, a["bias"], N, 0)
    got = f64(out)
    rows = [R.orow(m, 1, 3, 1) for m in range(M)]
    keep = np.zeros(got.shape, bool)
    keep[rows, :N] = True
    assert np.isnan(got[~keep]).all()
    close_to_fp64(got[rows, :N], ref, bound, f"prologue kind {kind} M={M} K={K}: projection")


def test_skinny_hook_rejects_bad_arguments(lib):
    from gitcap._lib import CDbgSkinnyArgs
    x = torch.zeros(16, 64, device="cuda", dtype=torch.bfloat16)
    a = CDbgSkinnyArgs()
    a.X, a.ldx, a.W, a.M, a.N, a.K, a.out, a.ldo, a.T, a.row_stride = ptr(x).value, 64, ptr(x).value, 1, 16, 64, ptr(x).value, 64, 1, 1
    assert lib.gitcap_dbg_skinny(ctypes.byref(a), 3, stream()) == -1       # the head has its own hook
    a.K = 96
    assert lib.gitcap_dbg_skinny(ctypes.byref(a), 0, stream()) == -1
    a.K, a.ln_kind = 64, 3
    assert lib.gitcap_dbg_skinny(ctypes.byref(a), 0, stream()) == -1
    assert lib.gitcap_dbg_skinny(None, 0, stream()) == -1
    assert lib.gitcap_dbg_pack_frags(ptr(x), ptr(x), 15, 64, 2, stream()) == -1
    assert lib.gitcap_dbg_kv_quant_v(ptr(x), ptr(x), ptr(x), 4, 128, 2, 3, stream()) == -1
    assert lib.gitcap_dbg_skinny_splitk(ptr(x), 64, ptr(x), None, None, 1, 16, 64, 3, ptr(x), 16, stream()) == -1
    assert lib.gitcap_dbg_ln_reduce(ptr(x), 65, ptr(x), ptr(x), ptr(x), ptr(x), 1e-5, 1, 64, ptr(x), ptr(x), stream()) == -1
    assert lib.gitcap_dbg_ffn_txt(ptr(x), 64, ptr(x), ptr(x), None, None, ptr(x), 1, 64, 64, ptr(x), stream()) == -1
    torch.cuda.synchronize()


# ---- split-K ---------------------------------------------------------------------------------------------------------------------

def _splitk(lib, X, W, Wpk, ws, M, N, K, ksplit, ks_eff, ldx=None):
    ldo = N + 4
    n = ks_eff * M * ldo
    # slabs are packed at stride M * ldo, so a store to rows >= M of slab s lands in slab s + 1 (and is compared there with that
    # slab's value); only behind the LAST slab is it poison: the tail holds the 16 - M % 16 rows a tile without the row guard
    # would write there
    slabs = torch.full((n + 16 * ldo,), NAN, device="cuda")
    rc = lib.gitcap_dbg_skinny_splitk(ptr(X), ldx or K, ptr(W), ptr(Wpk), ptr(ws), M, N, K, ksplit, ptr(slabs), ldo, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(slabs[n:]).all())                                # nothing behind row M - 1 of the last slab
    s = slabs[:n].view(ks_eff, M, ldo)
    assert bool(torch.isnan(s[:, :, N:]).all())
    return s[:, :, :N].contiguous()


@pytest.mark.parametrize("M,N,K,ksplit,fp8", R.SPLITK_CASES)
def test_splitk_slabs_against_fp64(lib, M, N, K, ksplit, fp8):
    a = R.gemm_inputs(M, N, K, fp8, seed=3000 + M + N + K, guard=False)
    X = to_dev(a["X"], torch.bfloat16)
    W, ws = _weights(a)
    ks = ksplit or R.DEFAULT_KSPLIT[K]
    got = _splitk(lib, X, W, None, ws, M, N, K, ksplit, ks)
    assert torch.equal(got, _splitk(lib, X, W, _pack(lib, W), ws, M, N, K, ksplit, ks))
    ref, bound = R.splitk(a["X"], a["W"], a["wscale"], N, ks)
    close_to_fp64(f64(got), ref, bound + 1e-300, f"splitk M={M} N={N} K={K} ksplit={ks} fp8={fp8}", flips=False)


# ---- ln_reduce -----------------------------------------------------------------------------------------------------------------

def _ln_reduce(lib, d, nslab, eps, M, D):
    xf = torch.full((M * D + 16,), NAN, device="cuda")
    xb = torch.full((M * D + 16,), NAN, device="cuda", dtype=torch.bfloat16)
    rc = lib.gitcap_dbg_ln_reduce(ptr(d["slabs"]), nslab, ptr(d["bias"]), ptr(d["resid"]), ptr(d["g"]), ptr(d["b"]), eps, M, D, ptr(xf), ptr(xb),
                                  stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(xf[M * D:]).all()) and bool(torch.isnan(xb[M * D:]).all())
    return xf[:M * D].view(M, D), xb[:M * D].view(M, D)


@pytest.mark.parametrize("M,D,nslab", R.LN_CASES)
def test_ln_reduce_against_fp64(lib, M, D, nslab):
    """Row 0 has a mean of 300 and a standard deviation of 0.05: a one-pass variance in fp32 would lose it."""
    q = R.ln_inputs(M, D, nslab, seed=D + nslab)
    d = {k: to_dev(q[k], torch.float32) for k in ("slabs", "bias", "resid", "g", "b")}
    xf, xb = _ln_reduce(lib, d, nslab, q["eps"], M, D)
    ref, bound = R.ln_reduce(**q)
    close_to_fp64(f64(xf), ref, bound, f"ln_reduce M={M} D={D} nslab={nslab}", flips=False)
    assert np.array_equal(f64(xb), R.bf16_rne(f64(xf)))                      # the bf16 copy is the rounding of the fp32 row


# ---- ffn_txt ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,D,F,fp8", R.FFN_CASES)
def test_ffn_txt_slabs(lib, M, D, F, fp8):
    """Bitwise the FC1 + GELU launch followed by the split-K launch with ksplit = F / 64; FC1 against fp64, FC2 against fp64 on the
    device's own h."""
    a = R.ffn_inputs(M, D, F, fp8, seed=4000 + M + D + F)
    X, b1 = to_dev(a["X"], torch.bfloat16), to_dev(a["bias"], torch.float32)
    W1, s1 = _weights(a)
    W2, s2 = _weights(a, "W2", "W2codes", "w2scale")
    W1pk, W2pk = _pack(lib, W1), _pack(lib, W2)
    ns = F // 64
    n = ns * M * D
    slabs = torch.full((n + 64,), NAN, device="cuda")
    rc = lib.gitcap_dbg_ffn_txt(ptr(X), D, ptr(W1pk), ptr(W2pk), ptr(s1), ptr(s2), ptr(b1), M, D, F, ptr(slabs), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(slabs[n:]).all())
    got = slabs[:n].view(ns, M, D)
    hbuf, _ = _skinny(lib, X=X, W=W1, Wpk=W1pk, wscale=s1, bias=b1, M=M, N=F, K=D, epi=1, T=M, row_stride=M, row_off=0)
    h = hbuf[:M, :F].contiguous()
    two = _splitk(lib, h, W2, W2pk, s2, M, D, F, ns, ns)
    assert torch.equal(got, two)
    h64, hb, ref, sb = R.ffn_txt(a["X"], a["W"], a["wscale"], a["bias"], a["W2"], a["w2scale"], h=f64(h))
    close_to_fp64(f64(h), h64, hb, f"ffn_txt M={M} D={D} F={F} fp8={fp8}: h")
    close_to_fp64(f64(got), ref, sb + 1e-300, f"ffn_txt M={M} D={D} F={F} fp8={fp8}: slabs", flips=False)


# ---- txt_block -------------------------------------------------------------------------------------------------------------------

CNT_POISON = 0x5EED


def _txt_operands(lib, q, packed):
    """The device operands of R.txt_block_inputs; the e4m3 image V comes from gitcap_dbg_kv_quant_v and must be the restatement's."""
    D, H = q["D"], q["H"]
    d = dict(kv_img=to_dev(q["kv_img"], torch.bfloat16), kv_txt=to_dev(q["kv_txt"], torch.bfloat16), aowpk=None, v8=None, vs=None,
             **{k: to_dev(q[k], torch.float32) for k in ("aob", "g1", "b1", "xin")})
    if q["Wcodes"] is not None:
        d["aow"], d["aoscale"] = to_dev(q["Wcodes"], torch.uint8), to_dev(q["aoscale"], torch.float32)
    else:
        d["aow"], d["aoscale"] = to_dev(q["Wo"], torch.bfloat16), None
        if packed:
            d["aowpk"] = _pack(lib, d["aow"])
    if q["v8"] is not None:
        keys, pitch = q["rows"] * q["S_img"], q["pitch"]
        v8 = torch.full((H * pitch * 64 + 64,), 0xAB, device="cuda", dtype=torch.uint8)
        vs = torch.full((H * pitch + 16,), NAN, device="cuda")
        assert lib.gitcap_dbg_kv_quant_v(ptr(d["kv_img"]), ptr(v8), ptr(vs), keys, D, H, pitch, stream()) == 0
        torch.cuda.synchronize()
        g8 = v8[:H * pitch * 64].cpu().numpy().reshape(H, pitch, 64)
        gs = vs[:H * pitch].cpu().numpy().astype(np.float64).reshape(H, pitch)
        assert np.array_equal(g8[:, :keys], q["v8"][:, :keys]) and np.array_equal(gs[:, :keys], q["vs"][:, :keys])
        assert (g8[:, keys:] == 0xAB).all() and np.isnan(gs[:, keys:]).all()          # v8_pitch > rows: poison behind a head's keys
        d["v8"], d["vs"] = v8, vs
    return d


def _txt_outputs(M, H, D):
    cnt = torch.full((M + 8,), CNT_POISON, device="cuda", dtype=torch.int32)
    cnt[:M] = 0
    return dict(part=torch.full((M * H * D + 64,), NAN, device="cuda"), cnt=cnt, xs=torch.full((M * D + 16,), NAN, device="cuda"),
                xsb=torch.full((M * D + 16,), NAN, device="cuda", dtype=torch.bfloat16))


def _txt_launch(lib, q, d, o, *, rows=None, T=None, t0=None, xin=None, nt_kv=0):
    """One launch on the operands d into the outputs o -> (part [M][H][D], xs [M][D], xsb [M][D]); tickets and poison checked."""
    from gitcap._lib import CDbgTxtBlockArgs
    D, H = q["D"], q["H"]
    rows, T, t0 = rows or q["rows"], T or q["T"], q["t0"] if t0 is None else t0
    M = rows * T
    a = CDbgTxtBlockArgs()
    a.kv_img, a.kv_txt = ptr(d["kv_img"]).value, ptr(d["kv_txt"]).value
    a.rows, a.beams, a.t0, a.T, a.Tmax, a.S_img, a.H, a.D = rows, q["beams"], t0, T, q["Tmax"], q["S_img"], H, D
    a.aow = ptr(d["aow"]).value
    a.aowpk = ptr(d["aowpk"]).value if d["aowpk"] is not None else None
    a.aoscale = ptr(d["aoscale"]).value if d["aoscale"] is not None else None
    a.aob, a.g1, a.b1 = ptr(d["aob"]).value, ptr(d["g1"]).value, ptr(d["b1"]).value
    a.xin = ptr(d["xin"] if xin is None else xin).value
    a.eps = q["eps"]
    a.part, a.cnt, a.xs, a.xsb = ptr(o["part"]).value, ptr(o["cnt"]).value, ptr(o["xs"]).value, ptr(o["xsb"]).value
    if d["v8"] is not None:
        a.v8_img, a.vs_img, a.v8_pitch = ptr(d["v8"]).value, ptr(d["vs"]).value, q["pitch"]
    a.nt_kv = nt_kv
    rc = lib.gitcap_dbg_txt_block(ctypes.byref(a), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((o["cnt"][:M] == 0).all()) and bool((o["cnt"][M:] == CNT_POISON).all())       # every ticket word is zero again
    assert bool(torch.isnan(o["part"][M * H * D:]).all()) and bool(torch.isnan(o["xs"][M * D:]).all()) and bool(torch.isnan(o["xsb"][M * D:]).all())
    return o["part"][:M * H * D].view(M, H, D).clone(), o["xs"][:M * D].view(M, D).clone(), o["xsb"][:M * D].view(M, D).clone()


@pytest.mark.parametrize("i", range(len(R.TXT_CASES)))
def test_txt_block_against_fp64(lib, i):
    """part per head and x1 against the restatement; xsb is the bf16 of xs; a second launch on the same buffers without touching
    cnt, and one with non-temporal K/V loads, give the same bits."""
    case = R.TXT_CASES[i]
    q = R.txt_block_inputs(*case, seed=7000 + i)
    M, H, D = q["rows"] * q["T"], q["H"], q["D"]
    d = _txt_operands(lib, q, packed=i % 2 == 0)
    o = _txt_outputs(M, H, D)
    part, xs, xsb = _txt_launch(lib, q, d, o)
    again = _txt_launch(lib, q, d, o)                                          # tickets left by the first launch
    assert same_bits(part, again[0]) and same_bits(xs, again[1]) and same_bits(xsb, again[2])
    nt = _txt_launch(lib, q, d, _txt_outputs(M, H, D), nt_kv=1)
    assert same_bits(part, nt[0]) and same_bits(xs, nt[1]) and same_bits(xsb, nt[2])
    if d["aowpk"] is not None:                                                 # fragment-major copy set versus unset
        un = _txt_launch(lib, q, dict(d, aowpk=None), _txt_outputs(M, H, D))
        assert same_bits(part, un[0]) and same_bits(xs, un[1])
    ref = R.txt_block(q)
    close_to_fp64(f64(part), ref["part"], ref["bound"], f"txt_block {case}: part", flips=False)
    x1, xb = R.txt_x1(f64(part), q)
    close_to_fp64(f64(xs), x1, xb, f"txt_block {case}: x1 from the device's partials", flips=False)
    assert np.array_equal(f64(xsb), R.bf16_rne(f64(xs)))


@pytest.mark.parametrize("D,rows,v8", [(768, 23, False), (128, 130, False), (768, 23, True)])
def test_txt_block_8_and_16_wave_workgroups_give_the_same_bits(lib, D, rows, v8):
    """More (row, head) units than the device has CUs: the launcher takes the 8-wave form unless switch 9 is off."""
    assert rows * (D // 64) > torch.cuda.get_device_properties(0).multi_processor_count
    q = R.txt_block_inputs(D, rows, 1, 1, 3, 33, False, v8, "n", seed=rows + D)
    d = _txt_operands(lib, q, packed=True)
    res = []
    for on in (1, 0):
        old = lib.gitcap_dbg_config(9, on)
        try:
            res.append(_txt_launch(lib, q, d, _txt_outputs(rows, q["H"], D)))
        finally:
            lib.gitcap_dbg_config(9, old)
    assert all(same_bits(x, y) for x, y in zip(*res))
    assert bool(torch.isfinite(res[0][1]).all())


@pytest.mark.parametrize("D", [128, 768])
def test_txt_block_row_is_independent_of_the_other_rows(lib, D):
    q = R.txt_block_inputs(D, 5, 1, 1, 4, 33, False, False, "n", seed=D + 5)
    d = _txt_operands(lib, q, packed=False)
    five = _txt_launch(lib, q, d, _txt_outputs(5, q["H"], D))
    one = _txt_launch(lib, q, d, _txt_outputs(1, q["H"], D), rows=1)
    assert all(same_bits(x[:1].contiguous(), y) for x, y in zip(five, one))


@pytest.mark.parametrize("D,v8", [(768, False), (128, True)])
def test_txt_block_cached_step_equals_teacher_forced_row(lib, D, v8):
    """T = 1 at t0 = t against row t of the teacher-forced launch (t0 = 0, T = 5) on the same K/V."""
    rows, T = 2, 5
    q = R.txt_block_inputs(D, rows, 1, T, 0, 33, False, v8, "n", seed=D + 17)
    d = _txt_operands(lib, q, packed=True)
    tf = _txt_launch(lib, q, d, _txt_outputs(rows * T, q["H"], D))
    for t in (0, 2, 4):
        sel = [r * T + t for r in range(rows)]
        step = _txt_launch(lib, q, d, _txt_outputs(rows, q["H"], D), T=1, t0=t, xin=d["xin"][sel].contiguous())
        assert all(same_bits(x[sel].contiguous(), y) for x, y in zip(tf, step)), t


def test_txt_block_hook_rejects_bad_arguments(lib):
    from gitcap._lib import CDbgTxtBlockArgs
    q = R.txt_block_inputs(128, 1, 1, 1, 0, 1, False, False, "n", seed=1)
    d = _txt_operands(lib, q, packed=False)
    o = _txt_outputs(1, 2, 128)

    def rc(**kw):
        a = CDbgTxtBlockArgs()
        a.kv_img, a.kv_txt, a.aow = ptr(d["kv_img"]).value, ptr(d["kv_txt"]).value, ptr(d["aow"]).value
        a.rows, a.beams, a.t0, a.T, a.Tmax, a.S_img, a.H, a.D = 1, 1, 0, 1, 3, 1, 2, 128
        a.aob, a.g1, a.b1, a.xin = (ptr(d[k]).value for k in ("aob", "g1", "b1", "xin"))
        a.part, a.cnt, a.xs, a.xsb = ptr(o["part"]).value, ptr(o["cnt"]).value, ptr(o["xs"]).value, ptr(o["xsb"]).value
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gitcap_dbg_txt_block(ctypes.byref(a), stream())

    assert rc(D=256, H=4) == -1 and rc(H=3) == -1 and rc(t0=3) == -1 and rc(beams=0) == -1 and rc(cnt=None) == -1
    assert rc(v8_img=ptr(d["aow"]).value) == -1 and rc(kv_img=ptr(d["kv_img"]).value + 2) == -1
    assert lib.gitcap_dbg_txt_block(None, stream()) == -1
    assert rc() == 0
    torch.cuda.synchronize()
