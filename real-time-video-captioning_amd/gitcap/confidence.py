"""One confidence number per caption from its per-token log-probabilities (greedy_decode(return_logprobs=True),
caption_stream(logprobs=True).last_logprobs), or from the dict ``score`` returns for a caption somebody else supplied."""
from __future__ import annotations

import torch


def caption_confidence(ids, logprobs: torch.Tensor = None, sep_token_id: int = None) -> torch.Tensor:
    """exp(mean log-probability) -- the geometric mean of the token probabilities -- over each row's tokens up to and including
    its first SEP, or over all of them when the row has none.  ``ids`` int64 [B, 1+steps] starting with CLS, ``logprobs`` fp32
    [B, steps] (column t belongs to ids[:, t + 1]).  -> fp32 [B] in [0, 1], on ``logprobs``' device.  Plain torch ops.
    ``caption_confidence(d)`` with the dict of ``GitCaptioner.score`` / ``StudentCaptioner.score``: exp(sum / count) over the
    positions that call counted, shaped as ``d["sum"]``; 1 where nothing was counted."""
    if isinstance(ids, dict):
        cnt = ids["count"].to(torch.float32)
        return torch.where(cnt > 0, torch.exp(ids["sum"].float() / cnt.clamp(min=1.0)), torch.ones_like(cnt))
    if logprobs is None or sep_token_id is None:
        raise ValueError("caption_confidence takes (ids, logprobs, sep_token_id) or the dict score() returns")
    if ids.dim() != 2 or logprobs.dim() != 2 or ids.shape[0] != logprobs.shape[0] or ids.shape[1] != logprobs.shape[1] + 1:
        raise ValueError(f"expected ids [B, 1+steps] and logprobs [B, steps], got {tuple(ids.shape)} and {tuple(logprobs.shape)}")
    B, steps = logprobs.shape
    if steps == 0:
        return torch.ones((B,), dtype=torch.float32, device=logprobs.device)
    is_sep = ids[:, 1:].to(logprobs.device) == sep_token_id
    # tokens to count: position of the first SEP + 1, or all of them
    first = torch.where(is_sep.any(dim=1), is_sep.int().argmax(dim=1) + 1, torch.full((B,), steps, device=logprobs.device))
    keep = torch.arange(steps, device=logprobs.device)[None, :] < first[:, None]
    total = torch.where(keep, logprobs.float(), torch.zeros((), device=logprobs.device)).sum(dim=1)
    return torch.exp(total / first.to(torch.float32))
