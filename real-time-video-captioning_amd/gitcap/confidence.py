"""One confidence number per greedy caption from its per-token log-probabilities (greedy_decode(return_logprobs=True),
caption_stream(logprobs=True).last_logprobs)."""
from __future__ import annotations

import torch


def caption_confidence(ids: torch.Tensor, logprobs: torch.Tensor, sep_token_id: int) -> torch.Tensor:
    """exp(mean log-probability) -- the geometric mean of the token probabilities -- over each row's tokens up to and including
    its first SEP, or over all of them when the row has none.  ``ids`` int64 [B, 1+steps] starting with CLS, ``logprobs`` fp32
    [B, steps] (column t belongs to ids[:, t + 1]).  -> fp32 [B] in [0, 1], on ``logprobs``' device.  Plain torch ops."""
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
