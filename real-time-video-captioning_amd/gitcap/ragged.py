"""Ragged batches: clips that differ in their number of frames (include/gitcap.h: gitcap_attach_frame_counts).

The library takes such a batch PACKED -- sum(counts) frames, clip-major, no padding -- plus the per-clip counts.  This module is
the host side of that layout and needs neither a device nor the library: what `src` / `frame_counts` mean, their checks, the
packing, and the way back from packed visual rows to the reference's padded (visual_features, visual_features_valid) pair."""
from typing import List, Optional, Sequence, Tuple

import torch


def check_counts(frame_counts, B: int, limit: int) -> List[int]:
    """frame_counts (a sequence or an int tensor) -> a list of B ints, each in [1, limit]; ValueError otherwise."""
    if isinstance(frame_counts, torch.Tensor):
        if frame_counts.dim() != 1 or frame_counts.dtype.is_floating_point or frame_counts.dtype == torch.bool:
            raise ValueError("frame_counts must be a 1-D integer tensor or a sequence of ints")
        frame_counts = frame_counts.tolist()
    counts = []
    for c in frame_counts:
        if isinstance(c, bool) or int(c) != c:
            raise ValueError(f"frame_counts must hold integers, got {c!r}")
        counts.append(int(c))
    if len(counts) != B:
        raise ValueError(f"frame_counts holds {len(counts)} counts for a batch of {B} clips")
    for b, c in enumerate(counts):
        if not 1 <= c <= limit:
            raise ValueError(f"clip {b} has {c} frames, outside [1, {limit}]")
    return counts


def clips(src, frame_counts, image_size: int, limit: int) -> Tuple[List[torch.Tensor], List[int], bool]:
    """The two input forms -> (one tensor [F_b, ...] per clip, the counts, raw).

    src: a padded tensor [B, Fmax, 3, S, S] (fp32, transformed) or [B, Fmax, H, W, 3] (uint8 BGR camera frames) with
    frame_counts [B] -- frames beyond a clip's count are ignored --, or a list of B tensors [F_b, 3, S, S] / [F_b, H, W, 3],
    whose counts are inferred (frame_counts, if given, must agree).  The clips are views: nothing is copied."""
    if isinstance(src, torch.Tensor):
        if frame_counts is None:
            raise ValueError("a padded tensor needs frame_counts")
        if src.dim() != 5:
            raise ValueError(f"expected padded frames [B, Fmax, ...], got {tuple(src.shape)}")
        counts = check_counts(frame_counts, src.shape[0], min(limit, src.shape[1]))
        parts = [src[b, :n] for b, n in enumerate(counts)]
    else:
        parts = list(src)
        if not parts or not all(isinstance(p, torch.Tensor) and p.dim() == 4 for p in parts):
            raise ValueError("expected a list of B tensors [F_b, 3, S, S] or [F_b, H, W, 3]")
        counts = check_counts([p.shape[0] for p in parts], len(parts), limit)
        if frame_counts is not None and check_counts(frame_counts, len(parts), limit) != counts:
            raise ValueError("frame_counts disagrees with the clips' own frame counts")
    if not counts:
        raise ValueError("empty batch")
    raw = parts[0].dtype == torch.uint8
    tail, dev = tuple(parts[0].shape[1:]), parts[0].device
    for p in parts:
        if (p.dtype == torch.uint8) != raw or tuple(p.shape[1:]) != tail or p.device != dev:
            raise ValueError("the clips of a batch must share dtype, frame shape and device")
    if raw:
        if tail[-1] != 3 or min(tail[0], tail[1]) < 1:
            raise ValueError(f"expected uint8 frames [F, H, W, 3], got {(counts[0],) + tail}")
    elif tail != (3, image_size, image_size):
        raise ValueError(f"expected frames [F, 3, {image_size}, {image_size}], got {(counts[0],) + tail}")
    return parts, counts, raw


def is_dense(counts: Sequence[int]) -> bool:
    return len(set(counts)) == 1


def dense(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    """Clips of equal length -> the dense [B, F, ...] tensor of the existing calls."""
    return torch.stack(list(parts), 0)


def pack(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    """Clip-major packed frames [sum(counts), ...] (one copy)."""
    return torch.cat(list(parts), 0)


def offsets(counts: Sequence[int], N: int = 1) -> List[int]:
    """off[b] = N * sum_{i<b} counts[i]: where clip b's frames (N = 1) or image rows (N = tokens per frame) start."""
    out, at = [], 0
    for c in counts:
        out.append(at * N)
        at += c
    return out


def unpack_rows(packed: torch.Tensor, counts: Sequence[int], N: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Packed visual rows [sum(counts) * N, D] -> (visual [B, Fmax * N, D], zero beyond a clip's rows; valid bool [B, Fmax * N]):
    the reference's visual_features / visual_features_valid pair."""
    B, S = len(counts), max(counts) * N
    vis = packed.new_zeros((B, S, packed.shape[-1]))
    valid = torch.zeros((B, S), dtype=torch.bool, device=packed.device)
    for b, (o, c) in enumerate(zip(offsets(counts, N), counts)):
        vis[b, :c * N] = packed[o:o + c * N]
        valid[b, :c * N] = True
    return vis, valid


def chunks(counts: Sequence[int], max_batch: int):
    """(b0, b1) clip ranges of at most max_batch clips."""
    return [(b0, min(len(counts), b0 + max_batch)) for b0 in range(0, len(counts), max_batch)]
