"""The variable-length forms of attn_full and txt_block (ragged batches: gitcap_attach_frame_counts) against the plain hooks.

The yardstick is the existing kernel on one group / one clip alone: a group of the packed launch must give the same bits as
gitcap_dbg_attn_full(G = 1, S = len[g]) on its rows, a text row the same bits as gitcap_dbg_txt_block with S_img = len[clip] on
its clip's keys.  Outputs start as NaN poison, the packed buffers have gaps between the groups, and whatever lies outside a
group's or a unit's rows must still be poison afterwards."""
import ctypes

import pytest
import torch

from gpu_support import NAN, lib, poisoned, ptr, same_bits, stream  # noqa: F401

pytestmark = pytest.mark.gpu

ATTN_LENS = [1, 63, 64, 65, 97, 128, 129, 197, 394]


def _at(t, elems):
    """the address `elems` elements into tensor t"""
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def _i32(a):
    return torch.tensor(a, dtype=torch.int32, device="cuda")


# ---- attn_full ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,G", [(2, 12), (2, 9), (3, 16), (3, 9)])          # H * G % 8: 0, 2, 0, 3 (both branches of the id remap)
def test_attn_full_varlen_group_equals_the_group_alone(lib, H, G):
    gen = torch.Generator().manual_seed(100 * H + G)
    lens = [ATTN_LENS[i] for i in torch.randperm(len(ATTN_LENS), generator=gen).tolist()]
    lens += [ATTN_LENS[i] for i in torch.randint(0, len(ATTN_LENS), (G - len(ATTN_LENS),), generator=gen).tolist()]
    assert len(lens) == G and set(ATTN_LENS) <= set(lens)
    assert max(lens) == 394 and min(lens) == 1 and lens[0] != 394        # groups that need 1 of the longest group's 4 q-blocks
    gaps = torch.randint(0, 4, (G,), generator=gen).tolist()               # rows between the groups that belong to no group
    off, row = [], 2
    for n, g in zip(lens, gaps):
        off.append(row)
        row += n + g
    total = row + 3
    W = H * 64
    qkv = poisoned((total, 3 * W), NAN, torch.bfloat16)
    gd = torch.Generator(device="cuda").manual_seed(7 + G)
    for o, n in zip(off, lens):
        qkv[o:o + n] = torch.randn(n, 3 * W, device="cuda", generator=gd).bfloat16()
    ctx = poisoned((total, W), NAN, torch.bfloat16)
    assert lib.gitcap_dbg_attn_full_varlen(ptr(qkv), ptr(ctx), G, ptr(_i32(off)), ptr(_i32(lens)), H, stream()) == 0
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool, device="cuda")
    for g, (o, n) in enumerate(zip(off, lens)):
        ref = poisoned((n + 2, W), NAN, torch.bfloat16)
        assert lib.gitcap_dbg_attn_full(_at(qkv, o * 3 * W), ptr(ref), 1, n, H, stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(ref[n:].float()).all())
        assert bool(torch.isfinite(ref[:n].float()).all())
        assert same_bits(ctx[o:o + n].contiguous(), ref[:n].contiguous()), (g, o, n)
        inside[o:o + n] = True
    assert bool(torch.isnan(ctx[~inside].float()).all()), "rows outside every group were written"


def test_attn_full_varlen_hook_rejects_bad_arguments(lib):
    qkv = torch.zeros(8, 3 * 128, device="cuda", dtype=torch.bfloat16)
    ctx = torch.zeros(8, 128, device="cuda", dtype=torch.bfloat16)
    off, ln = _i32([0]), _i32([8])
    assert lib.gitcap_dbg_attn_full_varlen(ptr(qkv), ptr(ctx), 1, ptr(off), ptr(ln), 2, stream()) == 0
    assert lib.gitcap_dbg_attn_full_varlen(None, ptr(ctx), 1, ptr(off), ptr(ln), 2, stream()) == -1
    assert lib.gitcap_dbg_attn_full_varlen(ptr(qkv), ptr(ctx), 0, ptr(off), ptr(ln), 2, stream()) == -1
    assert lib.gitcap_dbg_attn_full_varlen(ptr(qkv), ptr(ctx), 1, None, ptr(ln), 2, stream()) == -1
    assert lib.gitcap_dbg_attn_full_varlen(ptr(qkv), ptr(ctx), 1, ptr(off), ptr(_i32([0])), 2, stream()) == -1     # an empty group
    torch.cuda.synchronize()


# ---- txt_block ---------------------------------------------------------------------------------------------------------------------

TXT_LENS = [17, 34, 64, 65, 197]
CNT_POISON = 0x5EED


def _txt_args(D, rows, beams, t0, T, Tmax, S_img, kv_img, kv_txt, w, xin, out, v8, vs, pitch):
    from gitcap._lib import CDbgTxtBlockArgs
    a = CDbgTxtBlockArgs()
    a.kv_img, a.kv_txt = kv_img.value, kv_txt.value
    a.rows, a.beams, a.t0, a.T, a.Tmax, a.S_img, a.H, a.D = rows, beams, t0, T, Tmax, S_img, D // 64, D
    a.aow, a.aowpk, a.aoscale = w["aow"].data_ptr(), None, None
    a.aob, a.g1, a.b1 = w["aob"].data_ptr(), w["g1"].data_ptr(), w["b1"].data_ptr()
    a.xin = xin.value
    a.eps = 1e-5
    a.part, a.cnt, a.xs, a.xsb = out["part"].data_ptr(), out["cnt"].data_ptr(), out["xs"].data_ptr(), out["xsb"].data_ptr()
    if v8 is not None:
        a.v8_img, a.vs_img, a.v8_pitch = v8.value, vs.value, pitch
    a.nt_kv = 0
    return a


def _txt_outputs(M, H, D):
    cnt = torch.full((M + 8,), CNT_POISON, device="cuda", dtype=torch.int32)
    cnt[:M] = 0
    return dict(part=poisoned(M * H * D + 64, NAN), cnt=cnt, xs=poisoned(M * D + 16, NAN), xsb=poisoned(M * D + 16, NAN, torch.bfloat16))


def _txt_check_tails(o, M, H, D):
    assert bool((o["cnt"][:M] == 0).all()) and bool((o["cnt"][M:] == CNT_POISON).all())
    assert bool(torch.isnan(o["part"][M * H * D:]).all()) and bool(torch.isnan(o["xs"][M * D:]).all())
    assert bool(torch.isnan(o["xsb"][M * D:].float()).all())


@pytest.mark.parametrize("v8", [False, True])
@pytest.mark.parametrize("t0,T", [(0, 1), (3, 1), (0, 4), (3, 4)])
@pytest.mark.parametrize("D,beams", [(128, 1), (128, 2), (768, 2)])
def test_txt_block_varlen_row_equals_its_clip_alone(lib, D, beams, t0, T, v8):
    H, clips = D // 64, len(TXT_LENS)
    rows, Tmax = clips * beams, t0 + T + 2
    M = rows * T
    lens = TXT_LENS[2:] + TXT_LENS[:2]                                     # the longest clip in the middle
    off, row = [], 0
    for n in lens:
        off.append(row)
        row += n
    total = row
    gd = torch.Generator(device="cuda").manual_seed(D + 10 * beams + t0 + T)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gd)
    kv_img = rnd(total, 3 * D).bfloat16()
    kv_img[:, :D] = NAN                                                    # the image rows' q is never read
    kv_txt = poisoned((rows, Tmax, 3 * D), NAN, torch.bfloat16)
    kv_txt[:, :t0 + T] = rnd(rows, t0 + T, 3 * D).bfloat16()
    w = dict(aow=(rnd(D, D) / D ** 0.5).bfloat16(), aob=rnd(D), g1=1 + 0.1 * rnd(D), b1=0.1 * rnd(D))
    xin = rnd(M, D)
    v8p = vsp = None
    pitch = total + 3
    if v8:
        v8p = torch.full((H * pitch * 64 + 64,), 0xAB, device="cuda", dtype=torch.uint8)
        vsp = poisoned(H * pitch + 16, NAN)
        assert lib.gitcap_dbg_kv_quant_v(ptr(kv_img), ptr(v8p), ptr(vsp), total, D, H, pitch, stream()) == 0
    out = _txt_outputs(M, H, D)
    a = _txt_args(D, rows, beams, t0, T, Tmax, 0, ptr(kv_img), ptr(kv_txt), w, ptr(xin), out,
                  ptr(v8p) if v8 else None, ptr(vsp) if v8 else None, pitch)
    assert lib.gitcap_dbg_txt_block_varlen(ctypes.byref(a), ptr(_i32(off)), ptr(_i32(lens)), stream()) == 0
    torch.cuda.synchronize()
    _txt_check_tails(out, M, H, D)
    assert bool(torch.isfinite(out["xs"][:M * D]).all())
    part, xs, xsb = out["part"][:M * H * D].view(M, H, D), out["xs"][:M * D].view(M, D), out["xsb"][:M * D].view(M, D)
    for c, (o, n) in enumerate(zip(off, lens)):
        m0, mc = c * beams * T, beams * T                                  # the clip's text rows: beams rows x T positions
        ref = _txt_outputs(mc, H, D)
        b = _txt_args(D, beams, beams, t0, T, Tmax, n, _at(kv_img, o * 3 * D), _at(kv_txt, c * beams * Tmax * 3 * D), w, _at(xin, m0 * D), ref,
                      _at(v8p, o * 64) if v8 else None, _at(vsp, o) if v8 else None, pitch)
        assert lib.gitcap_dbg_txt_block(ctypes.byref(b), stream()) == 0
        torch.cuda.synchronize()
        _txt_check_tails(ref, mc, H, D)
        assert same_bits(part[m0:m0 + mc].contiguous(), ref["part"][:mc * H * D].view(mc, H, D).contiguous()), (c, n)
        assert same_bits(xs[m0:m0 + mc].contiguous(), ref["xs"][:mc * D].view(mc, D).contiguous()), (c, n)
        assert same_bits(xsb[m0:m0 + mc].contiguous(), ref["xsb"][:mc * D].view(mc, D).contiguous()), (c, n)


def test_txt_block_varlen_hook_rejects_bad_arguments(lib):
    from gitcap._lib import CDbgTxtBlockArgs
    assert lib.gitcap_dbg_txt_block_varlen(None, None, None, stream()) == -1
    a = CDbgTxtBlockArgs()
    a.rows, a.beams = 1, 1
    assert lib.gitcap_dbg_txt_block_varlen(ctypes.byref(a), None, None, stream()) == -1                   # no tables
    t = _i32([0])
    assert lib.gitcap_dbg_txt_block_varlen(ctypes.byref(a), ptr(t), ptr(t), stream()) == -1               # tables, null operands
