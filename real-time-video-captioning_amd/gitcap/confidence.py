"""One confidence number per caption from its per-token log-probabilities (greedy_decode(return_logprobs=True),
caption_stream(logprobs=True).last_logprobs), or from the dict ``score`` returns for a caption somebody else supplied."""
from __future__ import annotations

import torch


def caption_confidence(ids, logprobs: torch.Tensor = None, sep_token_id: int = None) -> torch.Tensor:
    """exp(mean log-probability) -- the geometric mean of the token probabilities -- over each row's tokens up to and including
    its first SEP, or over all of them when the row has none.  ``ids`` int64 [B, 1+steps] starting with CLS, ``logprobs`` fp32
    [B, steps] (column t belongs to ids[:, t + 1]).  -> fp32 [B] in [0, 1], on ``logprobs``' device.  Plain torch ops.
    ``caption_confidence(d)`` with the dict of ``GitCaptioner.score`` / ``StudentCaptioner.score``: exp(sum / count) over the
    positions that call counted, shaped as ``d["sum"]``; 1 where nothing was counted.  A dict that carries ``topk_logprobs``
    (``score(top_k=k)``, k >= 2) or ``logprobs`` [.., k] (``soft_labels``) gives a dict instead: ``confidence`` (the number above;
    absent without ``sum`` / ``count``) and ``margin`` fp32 [.., T-1], the per-token lp[.., 0] - lp[.., 1] in nats -- how far the
    model's best token is ahead of its runner-up; +inf where there is no rank 1."""
    if isinstance(ids, dict):
        conf = None
        if "count" in ids:
            cnt = ids["count"].to(torch.float32)
            conf = torch.where(cnt > 0, torch.exp(ids["sum"].float() / cnt.clamp(min=1.0)), torch.ones_like(cnt))
        top = ids.get("topk_logprobs", ids.get("logprobs") if "tail_logprob" in ids else None)
        if top is None:
            return conf
        out = dict(margin=top_margin(top))
        if conf is not None:
            out["confidence"] = conf
        return out
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


def top_margin(top_logprobs: torch.Tensor) -> torch.Tensor:
    """lp[..., 0] - lp[..., 1] of ranked log-probabilities [..., k]; +inf where rank 1 is missing (-inf padding, or k = 1)"""
    first = top_logprobs[..., 0].float()
    if top_logprobs.shape[-1] < 2:
        return torch.full_like(first, float("inf"))
    second = top_logprobs[..., 1].float()
    return torch.where(torch.isneginf(second), torch.full_like(first, float("inf")), first - second)


def frame_attribution(result) -> dict:
    """Which frame each token comes from, out of the dict ``GitCaptioner.attention`` / ``StudentCaptioner.attention`` returns (or a
    ``frame_attention`` tensor [.., T-1, F] itself).  -> dict: ``frame`` int64 [.., T-1], the frame with the largest attention mass
    per token (-1 at positions behind a row's length, whose masses are all zero); ``mean_mass`` fp32 [.., F], the caption-level
    mean mass per frame over the row's live positions (zeros for a row without any) -- frames near 0 are frames the decoder
    never looks at; ``image_share`` fp32 [..], the mean over the live positions of the mass on ALL frames (1 - the mass on the
    caption's own tokens): low values are tokens that come from the language prior.  Plain torch ops."""
    fa = result["frame_attention"] if isinstance(result, dict) else result
    if fa.dim() < 2:
        raise ValueError(f"expected frame_attention [.., T-1, F], got {tuple(fa.shape)}")
    fa = fa.float()
    total = fa.sum(dim=-1)
    ta = result.get("text_attention") if isinstance(result, dict) else None
    live = (total + ta.float() > 0) if ta is not None else (total > 0)
    if fa.shape[-1] == 0:
        frame = torch.full(fa.shape[:-1], -1, dtype=torch.int64, device=fa.device)
    else:
        frame = torch.where(live, fa.argmax(dim=-1), torch.full_like(total, -1, dtype=torch.int64))
    cnt = live.sum(dim=-1).clamp(min=1).to(torch.float32)
    mean_mass = torch.where(live[..., None], fa, torch.zeros_like(fa)).sum(dim=-2) / cnt[..., None]
    return dict(frame=frame, mean_mass=mean_mass, image_share=torch.where(live, total, torch.zeros_like(total)).sum(dim=-1) / cnt)
