"""csrc/attnmap.hip through gitcap_dbg_attn_map on caller-built caches, against the fp64 restatement within the derived bound
(tests/attention_map_reference.py; tests/test_attention_map.py shows that these inputs tell wrong kernels apart)."""
import ctypes

import numpy as np
import pytest
import torch

import attention_map_reference as R
from gpu_support import NAN, lib, poisoned, ptr, same_bits, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

PAD_F, PAD_S = 3, 5         # leading dimensions beyond the widths: the columns there keep their poison


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in R.device_cases()}


@pytest.fixture(scope="module")
def refs(cases):
    return {n: R.maps_fp64(c, want_bound=True) for n, c in cases.items()}


def run(lib, case, patches=True, rows=None):
    """One call of the hook -> frame_mass [rows][T][Fmax], text_mass [rows][T], patch_map [rows][T][Smax] (device tensors); the
    poison around them is checked.  rows = (first, count): that slice of the case's rows (whole clips) as a launch of its own."""
    from gitcap._lib import CDbgAttnMapArgs
    r0, nr = rows or (0, case["rows"])
    rpc, T, N, Smax = case["rows_per_clip"], case["T"], case["N"], case["Smax"]
    Fmax = Smax // N
    assert r0 % rpc == 0 and nr % rpc == 0
    c0, nc = r0 // rpc, nr // rpc
    kv_txt = torch.from_numpy(np.ascontiguousarray(case["kv_txt"][:, r0:r0 + nr])).bfloat16().cuda()
    kv_img_np, off = case["kv_img"], case["off"]
    if off is None:
        kv_img_np = kv_img_np[:, c0 * case["S_img"]:(c0 + nc) * case["S_img"]]
    kv_img = torch.from_numpy(np.ascontiguousarray(kv_img_np)).bfloat16().cuda()
    ld_f, ld_s = Fmax + PAD_F, Smax + PAD_S
    fm, tm = poisoned((nr, T, ld_f), NAN), poisoned(nr * T + 16, NAN)
    pm = poisoned((nr, T, ld_s), NAN) if patches else None
    d_off = to_dev(None if off is None else off[c0:c0 + nc], torch.int32)
    d_len = to_dev(None if off is None else case["len"][c0:c0 + nc], torch.int32)
    d_lengths = to_dev(None if case["lengths"] is None else case["lengths"][r0:r0 + nr], torch.int32)
    a = CDbgAttnMapArgs(kv_txt.data_ptr(), kv_img.data_ptr(), case["L"], case["H"], case["D"], nr, rpc, T, case["Tmax"], N, case["S_img"],
                        Smax, kv_img.shape[1], d_off.data_ptr() if off is not None else None,
                        d_len.data_ptr() if off is not None else None, case["layer"],
                        d_lengths.data_ptr() if d_lengths is not None else None, fm.data_ptr(), ld_f, tm.data_ptr(),
                        pm.data_ptr() if patches else None, ld_s)
    rc = lib.gitcap_dbg_attn_map(ctypes.byref(a), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(fm[:, :, Fmax:]).all()) and bool(torch.isnan(tm[nr * T:]).all())
    if patches:
        assert bool(torch.isnan(pm[:, :, Smax:]).all())
    return fm[:, :, :Fmax].contiguous(), tm[:nr * T].view(nr, T).contiguous(), pm[:, :, :Smax].contiguous() if patches else None


def check(dev, ref, bound, what):
    dev = dev.double().cpu().numpy()
    assert not np.isnan(dev).any(), what
    ratio = float((np.abs(dev - ref) / bound).max())
    print(f"{what}: max |device - fp64| / bound = {ratio:.3f}")
    assert ratio <= 1.0, what
    assert (dev[ref == 0] == 0).all(), what + ": zeros are exact"


@pytest.mark.parametrize("name", [c["name"] for c in R.device_cases()])
def test_maps_against_fp64(lib, cases, refs, name):
    case = cases[name]
    fm, tm, pm = run(lib, case)
    rf, rt, rp, bf, bt, bp = refs[name]
    check(fm, rf, bf, name + " frame_mass")
    check(tm, rt, bt, name + " text_mass")
    check(pm, rp, bp, name + " patch_map")
    # rows sum to 1 within the sum of their elements' bounds (0 where the row is cut)
    total = fm.double().sum(-1).cpu().numpy() + tm.double().cpu().numpy()
    want = rf.sum(-1) + rt
    assert (np.abs(total - want) <= bf.sum(-1) + bt).all(), name
    # without the patch rows: the same masses, bit for bit
    fm2, tm2, _ = run(lib, case, patches=False)
    assert same_bits(fm, fm2) and same_bits(tm, tm2), name + ": two runs"


@pytest.mark.parametrize("name,rows", [("N197_F3_T17", (1, 1)), ("H12_layer0_T16_rpc2", (2, 2)), ("ragged_1_and_3_rpc2", (2, 2)),
                                       ("lengths_0_1_T", (1, 1))])
def test_a_row_alone_is_the_row_in_the_batch(lib, cases, name, rows):
    case = cases[name]
    fm, tm, pm = run(lib, case)
    fa, ta, pa = run(lib, case, rows=rows)
    r0, nr = rows
    if case["off"] is not None:         # the widths of a launch are its own longest clip's
        Fa, Sa = fa.shape[2], pa.shape[2]
        assert same_bits(fm[r0:r0 + nr, :, :Fa].contiguous(), fa) and same_bits(pm[r0:r0 + nr, :, :Sa].contiguous(), pa)
    else:
        assert same_bits(fm[r0:r0 + nr].contiguous(), fa) and same_bits(pm[r0:r0 + nr].contiguous(), pa)
    assert same_bits(tm[r0:r0 + nr].contiguous(), ta)


def test_hook_refuses_what_would_index_outside(lib, cases):
    from gitcap._lib import CDbgAttnMapArgs
    case = cases["N5_F1_T1_H1_L1"]
    kv_txt = torch.from_numpy(case["kv_txt"]).bfloat16().cuda()
    kv_img = torch.from_numpy(case["kv_img"]).bfloat16().cuda()
    out = poisoned(64, NAN)

    def rc(**kw):
        f = dict(kv_txt=kv_txt.data_ptr(), kv_img=kv_img.data_ptr(), L=1, H=1, D=64, rows=1, rows_per_clip=1, T=1, Tmax=3, N=5, S_img=5,
                 Smax=5, img_rows=5, off=None, len=None, layer=-1, lengths=None, frame_mass=out.data_ptr(), ld_f=1,
                 text_mass=out.data_ptr() + 128, patch_map=None, ld_s=0)
        f.update(kw)
        a = CDbgAttnMapArgs(*[f[n] for n, _ in CDbgAttnMapArgs._fields_])
        r = lib.gitcap_dbg_attn_map(ctypes.byref(a), stream())
        torch.cuda.synchronize()
        return r
    assert rc() == 0
    for bad in (dict(T=4), dict(layer=1), dict(layer=-2), dict(D=128), dict(ld_f=0), dict(img_rows=4), dict(N=2), dict(rows_per_clip=2),
                dict(Smax=10), dict(frame_mass=None), dict(patch_map=out.data_ptr() + 192, ld_s=4)):
        assert rc(**bad) == -1, bad


# ---- the student's read-out: cross_probs_kernel + cross_mean_kernel through gitcap_dbg_cross_probs ---------------------------------

@pytest.mark.parametrize("i", range(len(R.cross_cases())))
def test_cross_probs_against_fp64(lib, i):
    c = R.cross_cases()[i]
    F, rows, T, H, hd = c["F"], c["rows"], c["T"], c["H"], c["hd"]
    M = rows * T

    def run(r0, nr):
        q = torch.from_numpy(np.ascontiguousarray(c["q"][r0 * T:(r0 + nr) * T])).bfloat16().cuda()
        kv = torch.from_numpy(np.ascontiguousarray(c["kv"][r0:r0 + nr])).bfloat16().cuda()
        ln = to_dev(None if c["lengths"] is None else c["lengths"][r0:r0 + nr], torch.int32)
        probs, fm = poisoned(nr * T * H * F + 16, NAN), poisoned((nr, T, F + PAD_F), NAN)
        rc = lib.gitcap_dbg_cross_probs(ptr(q), ptr(kv), 2 * H * hd, nr, T, H, hd, F, ptr(ln), ptr(probs), ptr(fm), F + PAD_F, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert bool(torch.isnan(probs[nr * T * H * F:]).all()) and bool(torch.isnan(fm[:, :, F:]).all())
        return probs[:nr * T * H * F].view(nr * T, H, F).contiguous(), fm[:, :, :F].contiguous()
    p, fm = run(0, rows)
    rp, rf, bp, bf = R.cross_fp64(c)
    check(p, rp, bp, f"cross F={F} probs")
    check(fm, rf, bf + 2.0 ** -120, f"cross F={F} frame_mass")
    p2, fm2 = run(0, rows)
    assert same_bits(p, p2) and same_bits(fm, fm2)
    pa, fa = run(rows - 1, 1)                                       # a row alone
    assert same_bits(p[(rows - 1) * T:].contiguous(), pa) and same_bits(fm[rows - 1:].contiguous(), fa)
    assert lib.gitcap_dbg_cross_probs(ptr(p), ptr(p), 2 * H * hd, 1, 1, H, hd, 65, None, ptr(p), ptr(fm), 65, stream()) == -1
