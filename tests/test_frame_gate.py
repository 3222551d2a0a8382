"""Scene-change gate, the parts that need no device: known answers of the restatement the device is held to
(tests/frame_gate_reference.py), FrameGate's bookkeeping with the distance call replaced by that restatement, the argument
checks of gitcap_frame_change and of a gated stream, and the compile-time check of csrc/framegate.hip (which
tests/test_isa_lint.py's file list does not cover).  The device tests are in test_frame_gate_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import frame_gate_reference as R
from gitcap import _lib
from gitcap.framegate import FrameGate, frame_change, gated_frames
from gitcap.window import WindowSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("frame_change_kernel", "frame_change_finalize_kernel")


# ---------------------------------------------------------------------------------------------------- restatement, known answers
def test_identical_frames_are_at_distance_zero():
    f = np.random.default_rng(0).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    r = R.frame_change(f, f.copy(), 2)
    assert r["ssd"] == [0, 0] and r["mse"] == [0.0, 0.0] and r["chisq"] == [0.0, 0.0]
    assert np.array_equal(r["hist_frame"], r["hist_ref"]) and r["hist_ref"].sum(axis=1).tolist() == [37 * 53] * 2


def test_black_against_white_needs_more_than_32_bits():
    H, W = 480, 640
    black, white = np.zeros((1, H, W, 3), np.uint8), np.full((1, H, W, 3), 255, np.uint8)
    r = R.frame_change(white, black, 0)
    assert r["ssd"] == [H * W * 3 * 65025] and r["ssd"][0] > 2 ** 32
    assert r["mse"] == [65025.0]
    assert r["hist_ref"][0, 0] == H * W and r["hist_frame"][0, 255] == H * W
    assert r["chisq"] == [float(H * W)]                       # one bin: (HW - 0)^2 / HW; bin 255 has hist_ref = 0 and is skipped


def test_two_by_two_by_hand():
    # channel 2 of the reference frame: 0 0 5 7, of the frame: 0 5 5 9; channels 0 and 1 differ in one byte by 3
    ref = np.zeros((1, 2, 2, 3), np.uint8)
    frm = np.zeros((1, 2, 2, 3), np.uint8)
    ref[0, :, :, 2] = [[0, 0], [5, 7]]
    frm[0, :, :, 2] = [[0, 5], [5, 9]]
    frm[0, 1, 1, 0] = 3
    r = R.frame_change(frm, ref, 2)
    assert r["ssd"] == [25 + 4 + 9] and r["mse"] == [38.0 / 12.0]
    want_ref, want_frm = np.zeros(256, np.int64), np.zeros(256, np.int64)
    want_ref[[0, 5, 7]] = [2, 1, 1]
    want_frm[[0, 5, 9]] = [1, 2, 1]
    assert np.array_equal(r["hist_ref"][0], want_ref) and np.array_equal(r["hist_frame"][0], want_frm)
    # bins 0, 5, 7 of the reference: (2-1)^2/2 + (1-2)^2/1 + (1-0)^2/1; bin 9 (hist_ref = 0) is skipped
    assert r["chisq"] == [0.5 + 1.0 + 1.0]
    assert R.frame_change(frm, ref, 0)["chisq"] == [(4 - 3) ** 2 / 4.0]            # channel 0: reference has four zeros, the frame three
    assert R.frame_change(ref, frm, 0)["chisq"] == [1.0 / 3.0 + 1.0]               # not symmetric: (3-4)^2/3, then bin 3: (1-0)^2/1


def test_exact_mse_is_not_the_reference_s_uint8_arithmetic():
    """The documented deviation: the reference subtracts and squares uint8 arrays (frame_sampling_methods.py:237), which wraps
    modulo 256; the gate uses the exact integer definition."""
    a, b = np.full((1, 2, 2, 3), 10, np.uint8), np.full((1, 2, 2, 3), 250, np.uint8)
    wrapped = float(np.mean((a - b) ** 2))                     # 10 - 250 = 16 (mod 256), 16^2 = 0 (mod 256)
    assert wrapped == 0.0
    assert R.frame_change(a, b)["mse"] == [57600.0]


# ---------------------------------------------------------------------------------------------------- FrameGate bookkeeping
def _gate(metric, threshold, **kw):
    """A FrameGate whose distance call is the restatement: runs on CPU tensors."""
    g = FrameGate(metric, threshold, **kw)
    g.calls = 0

    def distance(frame, ref):
        g.calls += 1
        return R.distances(frame.numpy(), ref.numpy(), g.metric, g.channel)
    g._distance = distance
    return g


def _flat(B, value, H=4, W=4):
    return torch.full((B, 1, H, W, 3), value, dtype=torch.uint8)


def test_first_frame_is_admitted_and_the_comparison_is_strict():
    g = _gate("mse", 4.0)
    assert g.admit(_flat(1, 100)) == [0] and g.calls == 0                       # no reference frame yet: no distance call
    assert g.stats == {"pushed": 1, "looked_at": 1, "admitted": 1, "last_distance": None}
    assert g.admit(_flat(1, 102)) == [] and g.stats["last_distance"] == [4.0]   # 4.0 > 4.0 is false
    assert g.admit(_flat(1, 103)) == [0] and g.stats["last_distance"] == [9.0]
    assert g.stats["pushed"] == 3 and g.stats["looked_at"] == 3 and g.stats["admitted"] == 2
    assert FrameGate("mse", -1.0).threshold < 0                                 # distances are >= 0: admits everything
    g = _gate("hist", -1.0)
    assert [g.admit(_flat(1, 7)) for _ in range(3)] == [[0]] * 3


def test_reference_frame_is_replaced_on_admission_only():
    """A slow drift of sub-threshold steps is eventually admitted: each frame is 1 away from its predecessor (mse 1) but the
    distance is taken from the last ADMITTED frame."""
    g = _gate("mse", 8.5)
    got = [bool(g.admit(_flat(1, 50 + k))) for k in range(8)]
    assert got == [True, False, False, True, False, False, True, False]          # 3^2 = 9 > 8.5 at steps 3 and 6
    assert torch.equal(g._ref, _flat(1, 56)[:, 0])
    # the gate owns its reference frames: the caller may overwrite its buffer (a capture ring)
    g = _gate("mse", 8.5)
    buf = _flat(1, 10)
    g.admit(buf)
    buf.fill_(200)
    assert int(g._ref.max()) == 10
    assert g.admit(buf) == [0] and int(g._ref.min()) == 200


def test_every_third_frame():
    g = _gate("mse", 0.5, every=3)
    vals = [10, 99, 99, 10, 99, 99, 20, 99, 99, 20]                               # frames 0, 3, 6, 9 are looked at
    got = [bool(g.admit(_flat(1, v))) for v in vals]
    assert got == [True, False, False, False, False, False, True, False, False, False]
    assert g.stats["pushed"] == 10 and g.stats["looked_at"] == 4 and g.stats["admitted"] == 2 and g.calls == 3
    want, _ = R.admit_sequence([_flat(1, v)[:, 0].numpy() for v in vals], "mse", 0.5, every=3)
    assert want == [0, 6]


def test_any_clip_admits_all_clips():
    g = _gate("mse", 50.0)
    a = torch.cat([_flat(1, 10), _flat(1, 10)])
    assert g.admit(a) == [0]
    b = torch.cat([_flat(1, 11), _flat(1, 30)])                                   # clip 0: 1, clip 1: 400
    assert g.admit(b) == [0] and g.stats["last_distance"] == [1.0, 400.0]
    assert torch.equal(g._ref, b[:, 0])                                           # every clip's reference frame is replaced
    assert g.admit(torch.cat([_flat(1, 12), _flat(1, 31)])) == []                 # both clips 1 away now


def test_reset_stats_and_multi_frame_pushes():
    g = _gate("hist", 3.0, channel=1)
    vals = [5, 5, 9, 9, 9, 5]
    frames = torch.cat([_flat(2, v) for v in vals], dim=1)                        # [2,6,4,4,3]: one push, gated in order
    assert g.admit(frames) == [0, 2, 5]                                           # chi-square of a moved bin: 16^2/16 = 16 > 3
    assert g.stats == {"pushed": 6, "looked_at": 6, "admitted": 3, "last_distance": [16.0, 16.0]}
    want, looked = R.admit_sequence([frames[:, i].numpy() for i in range(6)], "hist", 3.0, channel=1)
    assert want == [0, 2, 5] and [i for i, _ in looked] == [1, 2, 3, 4, 5]
    g.reset()
    assert g.stats == {"pushed": 0, "looked_at": 0, "admitted": 0, "last_distance": None} and g._ref is None
    assert g.admit(frames[:, 3:5]) == [0]                                         # first frame after the reset
    with pytest.raises(ValueError):
        g.admit(_flat(2, 1, H=5))                                                 # another frame size without a reset
    for bad in (dict(metric="ssim", threshold=1), dict(metric="mse", threshold=1, channel=3),
                dict(metric="mse", threshold=1, every=0)):
        with pytest.raises(ValueError):
            FrameGate(**bad)


def test_gated_push_takes_camera_frames_only():
    g = _gate("mse", 1.0)
    sched = WindowSchedule(1, 6, 1)
    for bad in (torch.zeros((1, 3, 8, 8)), torch.zeros((1, 2, 16)), torch.zeros((1, 8, 8, 3)),      # fp32 frames, tokens, fp32 HWC
                torch.zeros((1, 8, 8, 4), dtype=torch.uint8), torch.zeros((8, 8, 3), dtype=torch.uint8),
                np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError):
            gated_frames(g, bad, sched, "cpu")
    with pytest.raises(ValueError):
        gated_frames(g, torch.zeros((2, 8, 8, 3), dtype=torch.uint8), sched, "cpu")   # two clips into a window opened for one
    with pytest.raises(ValueError):
        gated_frames(g, torch.zeros((1, 7, 8, 8, 3), dtype=torch.uint8), sched, "cpu")  # more than a window per push
    assert g.stats["pushed"] == 0
    x = torch.zeros((1, 3, 8, 8, 3), dtype=torch.uint8)
    x[:, 2] = 9
    out = gated_frames(g, x, sched, "cpu")
    assert out.shape == (1, 2, 8, 8, 3) and torch.equal(out, x[:, [0, 2]])
    assert gated_frames(g, x[:, 2], sched, "cpu") is None


@pytest.mark.parametrize("which", ["student", "git"])
def test_gated_streams_refuse_other_input_before_any_device_work(which):
    """The streams' push reaches gated_frames first: no model, library handle or device is touched."""
    if which == "student":
        from gitcap.student import StudentCaptionStream as Stream
    else:
        from gitcap.model import CaptionStream as Stream

    class _Model:
        _dev = "cpu"
    st = Stream.__new__(Stream)
    st._m, st._token = _Model(), object()
    st._m._window_owner = st._token
    st._gate, st._sched = _gate("mse", 1.0), WindowSchedule(1, 6, 1)
    for bad in (torch.zeros((1, 3, 8, 8)), torch.zeros((1, 2, 16)), torch.zeros((1, 8, 8, 3))):
        with pytest.raises(ValueError, match="uint8 camera frames"):
            st.push(bad)
    assert st._gate.stats["pushed"] == 0
    cam = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(AttributeError):
        st.push(cam)                                   # the first frame is admitted and goes on to the (absent) encoder
    assert st.push(cam) is None                        # an unchanged frame is rejected: nothing else is called
    assert st._gate.stats == {"pushed": 2, "looked_at": 2, "admitted": 1, "last_distance": [0.0]}


# ---------------------------------------------------------------------------------------------------- C ABI without a device
def test_frame_change_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()                       # a non-null host pointer: must never be dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda f, r, B, H, W, ch: lib.gitcap_frame_change(f, r, B, H, W, ch, p, None, None, None, None, None)
    for args in ((None, p, 1, 2, 2, 0), (p, None, 1, 2, 2, 0), (p, p, 0, 2, 2, 0), (p, p, 1, 0, 2, 0), (p, p, 1, 2, 0, 0),
                 (p, p, 1, 2, 2, -1), (p, p, 1, 2, 2, 3), (p, p, 1, 32768, 32768, 0)):
        assert call(*args) == -1, args
    with pytest.raises(ValueError):
        frame_change(torch.zeros((1, 4, 4, 3)), torch.zeros((1, 4, 4, 3)))
    with pytest.raises(_lib.GitcapError):
        frame_change(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), torch.zeros((1, 4, 4, 3), dtype=torch.uint8))   # no CPU path


def test_kernels_are_in_the_gfx950_code_object():
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS:
        assert k.encode() in blob, k


# ---------------------------------------------------------------------------------------------------- compile-time check
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs /opt/rocm/bin/hipcc")
def test_framegate_kernels_compile_without_scratch():
    """With the product flags of csrc/Makefile (tools/isa_waits.py: product_flags): every kernel of the file is found and none
    uses scratch memory.  Properties of the source, not of one compiler's schedule, so they hold on any hipcc."""
    from isa_waits import kernel_listings
    res, names = kernel_listings("framegate.hip", "_Z")
    assert len(res) == len(names) == len(KERNELS), names
    for k in KERNELS:
        assert sum(k in r[0] for r in res) == 1, (k, names)
    for name, vgprs, scratch, toks in res:
        print(f"framegate.hip: {name}: {vgprs} VGPRs, {scratch} B scratch")
        assert scratch == 0, f"framegate.hip: {name} uses {scratch} bytes of scratch"
        assert "xs" not in toks and "xl" not in toks, f"framegate.hip: {name} has scratch traffic"
