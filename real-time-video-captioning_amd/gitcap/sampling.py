"""Frame sampling of whole decoded videos: from a video on the device to the ragged batch the decoding calls take.

The reference chooses the frames to caption with five samplers (src/utils/frame_sampling_methods.py): uniform, random from
bins, clustered, MSE difference and histogram scene change.  ``sample_frames`` offers the five under one call.  The two that
only count frames ("uniform", "bins") are index arithmetic on the host.  The three that look at the content run on the device
(csrc/framesample.hip) with every step enqueued at once and no host decision in between:

* "mse" / "hist": ``gitcap_frame_chain`` -- a frame is kept when it is far enough from the last frame kept; the reference frame
  is chosen on the device.  The arithmetic and its two differences from the reference are the scene-change gate's
  (gitcap/framegate.py: exact integer MSE, one channel order).
* "cluster": ``gitcap_frame_features`` (bilinear downsample), ``gitcap_kmeans`` (Lloyd), ``gitcap_frame_select`` (keep a frame
  when its cluster differs from the previous frame's).  Three deliberate differences: the downsample is fp32
  bilinear without cv2.resize's fixed-point rounding back to uint8; the initial centroids are the rows floor((j + 0.5) N / k)
  (or ``init``), not k-means++ with random_state = 42, which cannot be reproduced without sklearn -- so the method agrees with
  the reference in kind, not in labels; a cluster left empty keeps its centroid where sklearn relocates it.

The call synchronises once: one copy of B int32 (the numbers of selected frames) for the whole list of videos.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from . import _lib

METHODS = ("uniform", "bins", "cluster", "mse", "hist")
PARAMS = {"uniform": ("retention_rate",), "bins": ("num_bins", "seed"), "mse": ("threshold", "channel", "every"),
          "hist": ("threshold", "channel", "every"), "cluster": ("num_classes", "downsampling_ratio", "max_iter", "init")}
SAMPLER_PARAMS = tuple(sorted({p for ps in PARAMS.values() for p in ps}))


# ---- host arithmetic (needs neither a device nor the library) ---------------------------------------------------------------

def uniform_indices(N: int, retention_rate: float) -> List[int]:
    """The reference's uniform sampler (:62-72): every (N // int(N * rate))-th frame."""
    retained = int(N * retention_rate)
    if retained < 1:
        raise ValueError(f"retention_rate {retention_rate} keeps no frame of {N}")
    step = N // retained
    return [i for i in range(N) if i % step == 0]


def bin_indices(N: int, num_bins: int, generator: torch.Generator) -> List[int]:
    """The reference's bins sampler (:105-127): one frame drawn from each of num_bins bins of N // num_bins frames; an empty bin
    gives none.  Drawn from `generator`, so it agrees with the reference (numpy's global state) in distribution only."""
    if num_bins < 1:
        raise ValueError(f"num_bins={num_bins} must be >= 1")
    per = N // num_bins
    if per < 1:
        return []
    draws = torch.randint(0, per, (num_bins,), generator=generator).tolist()
    return [b * per + d for b, d in enumerate(draws)]


def thin(kept: Sequence[int], max_frames: int) -> List[int]:
    """kept[floor(j K / max_frames)], j = 0 .. max_frames - 1, when K = len(kept) > max_frames (gitcap_frame_select's rule)."""
    K = len(kept)
    if K <= max_frames:
        return list(kept)
    return [kept[j * K // max_frames] for j in range(max_frames)]


def default_init(N: int, k: int) -> List[int]:
    """The rows floor((j + 0.5) N / k): one per k-th of the video."""
    return [(2 * j + 1) * N // (2 * k) for j in range(k)]


def feature_size(H: int, W: int, ratio: float):
    """(h2, w2) = (int(H ratio), int(W ratio)), the reference's (:175-176)."""
    h2, w2 = int(H * ratio), int(W * ratio)
    if h2 < 1 or w2 < 1:
        raise ValueError(f"downsampling_ratio {ratio} leaves nothing of a {H}x{W} frame")
    return h2, w2


# ---- the selection ------------------------------------------------------------------------------------------------------------

@dataclass
class FrameSelection:
    """What ``sample_frames`` chose.  Per video b: ``indices[b]`` int64 device tensor [counts[b]], ascending; ``counts[b]`` a host
    int.  "mse" / "hist": ``distances[b]`` float64 [N_b] (NaN for frame 0 and frames not looked at).  "cluster": ``labels[b]``
    int32 [N_b], ``centroids[b]`` fp32 [k, D], ``iters[b]`` int32 [1] -- all on the device."""
    method: str
    videos: List[torch.Tensor]
    indices: List[torch.Tensor]
    counts: List[int]
    distances: Optional[List[torch.Tensor]] = None
    labels: Optional[List[torch.Tensor]] = None
    centroids: Optional[List[torch.Tensor]] = None
    iters: Optional[List[torch.Tensor]] = None
    _frames: Optional[List[torch.Tensor]] = field(default=None, repr=False)

    def frames(self) -> List[torch.Tensor]:
        """The selected frames, uint8 [F_b, H, W, 3] per video on the device: a ragged list for greedy_decode, infer, score and
        forward_image_enc."""
        if self._frames is None:
            self._frames = [v.index_select(0, i) for v, i in zip(self.videos, self.indices)]
        return self._frames


def _videos(videos, device) -> List[torch.Tensor]:
    vs = [videos] if torch.is_tensor(videos) else list(videos)
    if not vs:
        raise ValueError("no videos")
    out = []
    for v in vs:
        if not torch.is_tensor(v) or v.dtype != torch.uint8 or v.dim() != 4 or v.shape[-1] != 3 or min(v.shape[:3]) < 1:
            what = f"{v.dtype} {tuple(v.shape)}" if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"a video is a uint8 BGR tensor [N,H,W,3], got {what}")
        out.append(v.to(device).contiguous())
    return out


def _call(lib, name, *args):
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise _lib.GitcapError(f"{name} failed (status {rc})")


def sample_frames(videos, method: str, *, max_frames: Optional[int] = None, device=None, **params) -> FrameSelection:
    """Chooses the frames of each video.  ``videos``: one uint8 BGR tensor [N,H,W,3] or a list of them (sizes and lengths may
    differ; a host tensor is moved to the device once).  ``max_frames``: thin a longer selection to this many frames.

    method and its parameters:
      "uniform"  retention_rate                                          host index arithmetic
      "bins"     num_bins, seed=0                                        host indices from a seeded torch.Generator
      "mse"      threshold, channel=2, every=1                           gitcap_frame_chain
      "hist"     threshold, channel=2, every=1                           gitcap_frame_chain
      "cluster"  num_classes, downsampling_ratio=0.1, max_iter=100,      gitcap_frame_features, gitcap_kmeans,
                 init=None (row indices [k], or one list per video)      gitcap_frame_select
    """
    if method not in METHODS:
        raise ValueError(f"method {method!r}: one of {METHODS}")
    unknown = [p for p in params if p not in PARAMS[method]]
    if unknown:
        raise ValueError(f"{method!r} takes {PARAMS[method]}, not {unknown}")
    if max_frames is not None and int(max_frames) < 1:
        raise ValueError(f"max_frames={max_frames} must be >= 1")
    if device is None:
        first = videos if torch.is_tensor(videos) else (videos[0] if len(videos) else None)
        device = first.device if torch.is_tensor(first) and first.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    vs = _videos(videos, device)
    B = len(vs)
    limit = lambda N: N if max_frames is None else int(max_frames)

    if method in ("uniform", "bins"):
        if method == "uniform":
            kept = [uniform_indices(v.shape[0], float(params["retention_rate"])) for v in vs]
        else:
            g = torch.Generator().manual_seed(int(params.get("seed", 0)))
            kept = [bin_indices(v.shape[0], int(params["num_bins"]), g) for v in vs]
        kept = [thin(k, limit(v.shape[0])) for k, v in zip(kept, vs)]
        return FrameSelection(method, vs, [torch.tensor(k, dtype=torch.int64, device=device) for k in kept], [len(k) for k in kept])

    lib = _lib.load()
    counts = torch.empty((B,), dtype=torch.int32, device=device)
    idx = [torch.empty((v.shape[0],), dtype=torch.int64, device=device) for v in vs]
    sel = FrameSelection(method, vs, idx, [])
    with torch.cuda.device(device):
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        count_ptr = lambda b: ctypes.c_void_p(counts.data_ptr() + 4 * b)
        if method in ("mse", "hist"):
            thr, channel, every = float(params["threshold"]), int(params.get("channel", 2)), int(params.get("every", 1))
            if channel not in (0, 1, 2) or every < 1:
                raise ValueError(f"channel {channel} outside 0..2 or every={every} < 1")
            sel.distances = []
            for b, v in enumerate(vs):
                N, H, W = v.shape[:3]
                keep = torch.empty((N,), dtype=torch.uint8, device=device)
                dist = torch.empty((N,), dtype=torch.float64, device=device)
                _call(lib, "gitcap_frame_chain", _lib.ptr(v), N, H, W, int(method == "hist"), channel, thr, every, _lib.ptr(keep),
                      _lib.ptr(dist), st)
                _call(lib, "gitcap_frame_select", _lib.ptr(keep), None, N, limit(N), _lib.ptr(idx[b]), count_ptr(b), st)
                sel.distances.append(dist)
        else:
            k, ratio, max_iter = int(params["num_classes"]), float(params.get("downsampling_ratio", 0.1)), int(params.get("max_iter", 100))
            init = params.get("init")
            if max_iter < 1:
                raise ValueError(f"max_iter={max_iter} must be >= 1")
            sel.labels, sel.centroids, sel.iters = [], [], []
            for b, v in enumerate(vs):
                N, H, W = v.shape[:3]
                if not 1 <= k <= N:
                    raise ValueError(f"num_classes={k} outside [1, {N}] (video {b} has {N} frames)")
                h2, w2 = feature_size(H, W, ratio)
                D = h2 * w2 * 3
                rows = default_init(N, k) if init is None else init
                if not torch.is_tensor(rows) and len(rows) and not isinstance(rows[0], int):
                    rows = rows[b]
                rows = torch.as_tensor(rows).to(device=device, dtype=torch.int32).contiguous()
                if rows.shape != (k,):
                    raise ValueError(f"init holds {tuple(rows.shape)} rows for num_classes={k}")
                X = torch.empty((N, D), dtype=torch.float32, device=device)
                labels = torch.empty((N,), dtype=torch.int32, device=device)
                cent = torch.empty((k, D), dtype=torch.float32, device=device)
                iters = torch.empty((1,), dtype=torch.int32, device=device)
                _call(lib, "gitcap_frame_features", _lib.ptr(v), N, H, W, h2, w2, _lib.ptr(X), st)
                _call(lib, "gitcap_kmeans", _lib.ptr(X), N, D, k, _lib.ptr(rows), max_iter, _lib.ptr(labels), _lib.ptr(cent), _lib.ptr(iters), st)
                _call(lib, "gitcap_frame_select", None, _lib.ptr(labels), N, limit(N), _lib.ptr(idx[b]), count_ptr(b), st)
                sel.labels.append(labels)
                sel.centroids.append(cent)
                sel.iters.append(iters)
    sel.counts = counts.tolist()                          # the call's one synchronisation
    sel.indices = [i[:c] for i, c in zip(idx, sel.counts)]
    return sel


def caption_videos(model, videos, method: str, *, max_len: int, **kw):
    """Decoded videos -> captions: ``sample_frames(videos, method, max_frames=model._frame_limit(), ...)``, then the model's ragged
    ``greedy_decode`` on the selected frames.  ``kw``: the sampler's parameters (SAMPLER_PARAMS) and, everything else,
    greedy_decode's.  Videos of different frame sizes are decoded in one ragged batch per size (a batch shares its frame shape).
    -> (what greedy_decode returns, rows in the order of ``videos``; the FrameSelection)."""
    sampler = {p: kw.pop(p) for p in list(kw) if p in SAMPLER_PARAMS}
    sel = sample_frames(videos, method, max_frames=model._frame_limit(), device=model._dev, **sampler)
    if min(sel.counts) < 1:
        raise ValueError(f"{method!r} selected no frame of video {sel.counts.index(min(sel.counts))}")
    frames = sel.frames()
    groups = {}
    for b, f in enumerate(frames):
        groups.setdefault(tuple(f.shape[1:]), []).append(b)
    outs, order = [], []
    for members in groups.values():
        outs.append(model.greedy_decode([frames[b] for b in members], max_len=max_len, **kw))
        order += members
    back = torch.tensor(order).argsort()
    join = lambda parts: torch.cat(list(parts), 0)[back.to(parts[0].device)]
    if isinstance(outs[0], tuple):
        return tuple(join(p) for p in zip(*outs)), sel
    return join(outs), sel
