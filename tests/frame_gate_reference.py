"""Restatement of the scene-change gate in numpy int64 / Python floats, written from the definitions (include/gitcap.h:
gitcap_frame_change; gitcap/framegate.py: FrameGate), for tests/test_frame_gate.py and tests/test_frame_gate_gpu.py.

ssd and the histograms are integers, hence exact.  The two distances are fp64 with the device's operation order: one division
for the mean squared error; for the chi-square distance the bins in ascending order in a plain loop, one division and one
addition per bin with hist_ref > 0 (OpenCV's HISTCMP_CHISQR with the last kept frame as H1)."""
import numpy as np


def ssd(frame, ref):
    """Sum over all bytes of (frame - ref)^2, exact (Python int)."""
    d = np.asarray(frame).astype(np.int64) - np.asarray(ref).astype(np.int64)
    return int((d * d).sum())


def histogram(frame, channel):
    """int64 [256]: counts of the byte values of channel `channel` of a [H,W,3] frame."""
    return np.bincount(np.asarray(frame)[..., channel].reshape(-1), minlength=256).astype(np.int64)


def mse(frame, ref):
    return float(ssd(frame, ref)) / float(np.asarray(frame).size)


def chisq(hist_ref, hist_frame):
    acc = 0.0
    for i in range(256):
        hr, hf = int(hist_ref[i]), int(hist_frame[i])
        if hr > 0:
            d = hr - hf
            acc += float(d * d) / float(hr)
    return acc


def frame_change(frames, ref, channel=2):
    """frames, ref uint8 [B,H,W,3] -> dict of per-clip results, keyed as gitcap.framegate.frame_change."""
    frames, ref = np.asarray(frames), np.asarray(ref)
    assert frames.dtype == np.uint8 and ref.dtype == np.uint8 and frames.shape == ref.shape and frames.ndim == 4
    hf = np.stack([histogram(f, channel) for f in frames])
    hr = np.stack([histogram(r, channel) for r in ref])
    return {"ssd": [ssd(f, r) for f, r in zip(frames, ref)], "hist_frame": hf, "hist_ref": hr,
            "mse": [mse(f, r) for f, r in zip(frames, ref)], "chisq": [chisq(a, b) for a, b in zip(hr, hf)]}


def distances(frame, ref, metric, channel=2):
    """[B] floats: what FrameGate compares with its threshold."""
    r = frame_change(frame, ref, channel)
    return r["mse"] if metric == "mse" else r["chisq"]


def admit_sequence(frames, metric, threshold, channel=2, every=1):
    """frames: sequence of uint8 [B,H,W,3], in push order since a reset -> (indices admitted, [(index, [B] distances)] of the
    looked-at frames behind the first).  Every `every`-th frame is looked at, the first included; the first looked-at frame is
    admitted; a later one iff any clip's distance from the last admitted frame is > threshold; only admission replaces it."""
    ref, admitted, looked = None, [], []
    for i, f in enumerate(frames):
        if i % every:
            continue
        f = np.asarray(f)
        if ref is None:
            ref = f
            admitted.append(i)
            continue
        d = distances(f, ref, metric, channel)
        looked.append((i, d))
        if any(x > threshold for x in d):
            ref = f
            admitted.append(i)
    return admitted, looked
