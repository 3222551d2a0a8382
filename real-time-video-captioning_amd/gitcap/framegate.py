"""A scene-change gate in front of the live caption streams: is a pushed camera frame worth encoding?

The reference answers that on the host: its webcam loop takes every third frame (src/real_time_inference.py:48) and its
samplers keep a frame only when it differs enough from the last frame kept, by mean squared error or by the chi-square
distance of 256-bin histograms (src/utils/frame_sampling_methods.py:201-297).  Here the frames are already on the device as
uint8 before the encoder touches them, so the distances are computed there (``gitcap_frame_change``, csrc/framegate.hip) and
only B doubles per looked-at frame come back to the host.

Two deliberate differences from the reference's arithmetic: the mean squared error is the exact integer
definition (the reference squares uint8 differences, which wrap modulo 256, :237), and every frame is compared in the same
channel order (the reference's first kept frame is BGR, the later ones RGB, :230 / :235).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch

from . import _lib

OUTPUTS = ("ssd", "hist_frame", "hist_ref", "mse", "chisq")
METRICS = {"mse": "mse", "hist": "chisq"}


def frame_change(frames: torch.Tensor, ref: torch.Tensor, channel: int = 2, outputs: Sequence[str] = OUTPUTS) -> dict:
    """``gitcap_frame_change`` on device uint8 BGR frames ``[B,H,W,3]`` against reference frames of the same shape ->
    {"ssd": int64 [B], "hist_frame" / "hist_ref": int32 [B,256] (counts of channel `channel` of the BGR triple), "mse" /
    "chisq": float64 [B]}, device tensors, enqueued on the current stream (no synchronisation).  ``outputs`` names the ones
    wanted; the others are not computed into caller memory."""
    for t in (frames, ref):
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError("expected uint8 frames [B,H,W,3]")
        if t.device.type != "cuda":
            raise _lib.GitcapError("frame_change runs on the device only (no CPU path): pass device tensors")
    if frames.shape != ref.shape or frames.device != ref.device:
        raise ValueError(f"frames {tuple(frames.shape)} on {frames.device} and ref {tuple(ref.shape)} on {ref.device} differ")
    unknown = [o for o in outputs if o not in OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; known: {OUTPUTS}")
    lib = _lib.load()
    dev = frames.device
    frames, ref = frames.contiguous(), ref.contiguous()
    B, H, W = frames.shape[:3]
    shapes = {"ssd": ((B,), torch.int64), "hist_frame": ((B, 256), torch.int32), "hist_ref": ((B, 256), torch.int32),
              "mse": ((B,), torch.float64), "chisq": ((B,), torch.float64)}
    out = {o: torch.empty(shapes[o][0], dtype=shapes[o][1], device=dev) for o in OUTPUTS if o in outputs}
    ptr = [_lib.ptr(out.get(o)) for o in OUTPUTS]
    with torch.cuda.device(dev):
        rc = lib.gitcap_frame_change(_lib.ptr(frames), _lib.ptr(ref), B, H, W, int(channel), *ptr,
                                     ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise _lib.GitcapError(f"gitcap_frame_change failed (status {rc}): {B} frames {H}x{W}, channel {channel}")
    return out


class FrameGate:
    """Admits a pushed frame when it is far enough from the last frame admitted.

    ``metric``: "mse" (mean squared error over all bytes) or "hist" (chi-square distance of the histograms of channel
    ``channel`` of the BGR triple, the last admitted frame as H1; 2 = the red channel the reference histograms).  A looked-at
    frame is admitted iff its distance is strictly greater than ``threshold``; the first frame after a reset always is.
    ``every = k`` looks only at every k-th pushed frame (the first after a reset included) and drops the others unseen.
    The B clips of a stream advance in lockstep, so a frame is admitted for all clips iff any clip's distance exceeds the
    threshold, and every clip's reference frame is replaced then.  The reference frames are a device tensor the gate owns
    (copied on admission).  Each looked-at frame costs one launch and one copy of B doubles to the host."""

    def __init__(self, metric: str, threshold: float, channel: int = 2, every: int = 1):
        if metric not in METRICS:
            raise ValueError(f"metric {metric!r}: one of {sorted(METRICS)}")
        if channel not in (0, 1, 2):
            raise ValueError(f"channel {channel} outside 0..2 (of the BGR triple)")
        if int(every) < 1:
            raise ValueError(f"every={every} must be >= 1")
        self.metric, self.threshold, self.channel, self.every = metric, float(threshold), int(channel), int(every)
        self.reset()

    def reset(self):
        """Forget the reference frames and the counters: the next frame is looked at and admitted."""
        self._ref: Optional[torch.Tensor] = None
        self._pushed = self._looked = self._admitted = 0
        self._last: Optional[List[float]] = None

    @property
    def stats(self) -> dict:
        """Frames per clip pushed / looked at / admitted since the reset, and the last looked-at frame's distances [B]
        (None before the second looked-at frame)."""
        return {"pushed": self._pushed, "looked_at": self._looked, "admitted": self._admitted,
                "last_distance": None if self._last is None else list(self._last)}

    def _distance(self, frame: torch.Tensor, ref: torch.Tensor) -> List[float]:
        """The one device call: distances [B] of `frame` from `ref`, on the host."""
        key = METRICS[self.metric]
        return frame_change(frame, ref, self.channel, outputs=(key,))[key].tolist()

    def admit(self, frames: torch.Tensor) -> List[int]:
        """frames uint8 [B,n,H,W,3]: gates the n frames in order against the running reference -> indices of the admitted."""
        if frames.dim() != 5 or frames.dtype != torch.uint8 or frames.shape[-1] != 3:
            raise ValueError(f"expected uint8 frames [B,n,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
        keep = []
        for i in range(frames.shape[1]):
            idx = self._pushed
            self._pushed += 1
            if idx % self.every:
                continue
            frame = frames[:, i].contiguous()
            if self._ref is not None and (frame.shape != self._ref.shape or frame.device != self._ref.device):
                raise ValueError(f"frames {tuple(frame.shape)} on {frame.device} after frames {tuple(self._ref.shape)} on "
                                 f"{self._ref.device}; reset() first")
            self._looked += 1
            if self._ref is None:
                self._ref = frame.clone()
            else:
                self._last = [float(d) for d in self._distance(frame, self._ref)]
                if not any(d > self.threshold for d in self._last):
                    continue
                self._ref.copy_(frame)
            self._admitted += 1
            keep.append(i)
        return keep


def gated_frames(gate: FrameGate, frames, sched, device) -> Optional[torch.Tensor]:
    """What a gated stream does with a push: camera frames uint8 [B,H,W,3] or [B,n,H,W,3] (anything else raises ValueError
    before any device work) are moved to the device once and gated; -> the admitted frames [B,k,H,W,3] on the device, or None
    when there are none."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() not in (4, 5) or frames.shape[-1] != 3:
        what = f"{frames.dtype} {tuple(frames.shape)}" if torch.is_tensor(frames) else type(frames).__name__
        raise ValueError(f"a gated stream takes uint8 camera frames [B,H,W,3] or [B,n,H,W,3], got {what}")
    x = frames.unsqueeze(1) if frames.dim() == 4 else frames
    if min(x.shape[2], x.shape[3]) < 1:
        raise ValueError("empty frames")
    sched.check(x.shape[0], x.shape[1])
    x = x.to(device).contiguous()
    keep = gate.admit(x)
    if not keep:
        return None
    return x if len(keep) == x.shape[1] else x[:, keep].contiguous()
