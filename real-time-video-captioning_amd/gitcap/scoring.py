"""Scoring of given captions (include/gitcap.h: gitcap_score): what GitCaptioner.score and StudentCaptioner.score share -- the
argument handling in front of the C call and the dict behind it.  Plain torch ops on the handle's device; no host round trip."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib


def candidates(y: torch.Tensor, dev) -> tuple:
    """y [B, T] or [B, n, T] -> (ids int64 [B, n, T] on dev, had_n)."""
    if y.dim() not in (2, 3) or y.shape[-1] < 2 or y.shape[0] < 1 or (y.dim() == 3 and y.shape[1] < 1):
        raise ValueError(f"expected CLS-first ids [B, T] or [B, n, T] with T >= 2, got {tuple(y.shape)}")
    ids = y.to(device=dev, dtype=torch.int64)
    return (ids if y.dim() == 3 else ids[:, None]).contiguous(), y.dim() == 3


def row_lengths(ids: torch.Tensor, sep_token_id: int, until_sep: bool, lengths: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Valid tokens per row (CLS included), int32 [B, n] on ids' device, or None for all T: through the row's first SEP
    (until_sep), capped by the caller's ``lengths`` ([B] or [B, n]) when given."""
    B, n, T = ids.shape
    out = None
    if until_sep:
        is_sep = ids[:, :, 1:] == sep_token_id
        out = torch.where(is_sep.any(dim=2), is_sep.int().argmax(dim=2) + 2, torch.full((B, n), T, device=ids.device))
    if lengths is not None:
        ln = lengths.to(device=ids.device, dtype=torch.int64).reshape(B, -1).expand(B, n)
        out = ln if out is None else torch.minimum(out, ln)
    return None if out is None else out.to(torch.int32).contiguous()


class ScoreBuffers:
    """The five outputs of one gitcap_score / gitcap_student_score call over ``rows`` rows of T ids."""

    def __init__(self, rows: int, T: int, dev, top1: bool, top_k: int = 0):
        self.token_lp = torch.empty((rows, T - 1), dtype=torch.float32, device=dev)
        self.sum = torch.empty((rows,), dtype=torch.float32, device=dev)
        self.cnt = torch.empty((rows,), dtype=torch.int32, device=dev)
        self.top1_ids = torch.empty((rows, T - 1), dtype=torch.int64, device=dev) if top1 else None
        self.top1_lp = torch.empty((rows, T - 1), dtype=torch.float32, device=dev) if top1 else None
        # top_k: the k best tokens of every position and their log-probabilities (the one-shot attachment in front of the call)
        self.topk_ids = torch.empty((rows, T - 1, top_k), dtype=torch.int64, device=dev) if top_k else None
        self.topk_lp = torch.empty((rows, T - 1, top_k), dtype=torch.float32, device=dev) if top_k else None

    def attach_topk(self, call, name: str):
        """``call(name, ...)``: gitcap_attach_top_logprobs / gitcap_student_attach_top_logprobs, when top_k was asked for"""
        if self.topk_ids is not None:
            call(name, self.topk_ids.shape[2], _lib.ptr(self.topk_ids), _lib.ptr(self.topk_lp), self.topk_ids.shape[1])

    def args(self, T: int):
        """The output arguments of the C call, in its order."""
        return (_lib.ptr(self.token_lp), T - 1, _lib.ptr(self.sum), _lib.ptr(self.cnt), _lib.ptr(self.top1_ids), _lib.ptr(self.top1_lp))


def check_top_k(top_k) -> int:
    if not 0 <= int(top_k) <= 32:
        raise ValueError(f"top_k={top_k} outside 0..32")
    return int(top_k)


def result(chunks, B: int, n: int, had_n: bool, top1: bool, out_dev) -> dict:
    """ScoreBuffers of the chunks (clip-major rows) -> the dict ``score`` returns, shaped [B, (n,) ...] on out_dev."""
    def cat(field):
        t = torch.cat([getattr(c, field) for c in chunks], 0)
        t = t.view(B, n, *t.shape[1:]) if had_n else t
        return t.to(out_dev) if t.device != out_dev else t
    out = dict(token_logprobs=cat("token_lp"), sum=cat("sum"), count=cat("cnt"))
    if top1:
        out.update(top1_ids=cat("top1_ids"), top1_logprobs=cat("top1_lp"))
    if chunks[0].topk_ids is not None:
        out.update(topk_ids=cat("topk_ids"), topk_logprobs=cat("topk_lp"))
    return out


def soft_labels(teacher, x: torch.Tensor, y: torch.Tensor, k: int, lengths: Optional[torch.Tensor] = None) -> dict:
    """Offline distillation labels in the compact form: ONE ``teacher.score(x, y, top_k=k)`` call (GitCaptioner or
    StudentCaptioner) -> ``ids`` int64 and ``logprobs`` fp32 [B, (n,) T-1, k], the k best next tokens of every position of the
    teacher-forced captions ``y`` (-1 / -inf where a row has fewer), ``tail_logprob`` fp32 [B, (n,) T-1] = log1p(-sum exp(logprobs)),
    the log of the mass outside the k (the mass clamped at 0: -inf where the k tokens hold everything up to rounding), and
    ``mask`` bool [B, (n,) T-1], the positions ``score`` counted (targets inside the vocabulary, in front of the row's length)."""
    d = teacher.score(x, y, lengths=lengths, top_k=k)
    lp = d["topk_logprobs"]
    tail = torch.log1p(-torch.exp(lp.double()).sum(dim=-1).clamp(max=1.0)).float()
    # the positions score counted, decided from the ids the way the kernels decide it (target inside the vocabulary, in front of
    # the row's length: through its first SEP and the caller's lengths)
    ids, had_n = candidates(y, lp.device)
    V = getattr(teacher.cfg, "vocab_size", None) or teacher.cfg.vocab_length
    ln = row_lengths(ids, teacher.sep_token_id, True, lengths)
    tgt = ids[:, :, 1:]
    mask = (tgt >= 0) & (tgt < V) & (torch.arange(1, ids.shape[2], device=lp.device)[None, None, :] < ln[:, :, None])
    mask = mask if had_n else mask[:, 0]
    return dict(ids=d["topk_ids"], logprobs=lp, tail_logprob=tail, mask=mask)


def rerank_scores(score: dict, length_penalty: float) -> dict:
    """sum / count ** length_penalty -- the BeamHypotheses score of the reference's search -- per candidate [B, n], and the
    candidates' order, best first (ties: the lower index).  A candidate with nothing counted scores -inf."""
    cnt = score["count"].to(torch.float32)
    s = torch.where(cnt > 0, score["sum"] / cnt.clamp(min=1.0) ** length_penalty, torch.full_like(cnt, float("-inf")))
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    return dict(score, scores=s, order=order)
