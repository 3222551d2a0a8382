"""Teacher-student divergence of given captions on the device (include/gitcap.h: gitcap_distill): the two quantities
DistillationTrainer.training_step (src/models/model.py:919-935) runs on, forward only and without either model's logits tensor.
Plain torch ops on the handles' device; nothing goes through the host except what the caller reads."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib, scoring


class _Buffers:
    """The outputs of one gitcap_distill call over ``rows`` rows of T ids."""

    def __init__(self, rows: int, T: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.kl = torch.empty((rows, T), **f32)
        self.teacher_top1 = torch.empty((rows, T), dtype=torch.int64, device=dev)
        self.student_top1 = torch.empty((rows, T), dtype=torch.int64, device=dev)
        self.agreement = torch.empty((rows, T), dtype=torch.uint8, device=dev)
        self.teacher_logprobs = torch.empty((rows, T - 1), **f32)
        self.student_logprobs = torch.empty((rows, T - 1), **f32)
        self.kl_sum = torch.empty((rows,), **f32)
        self.count = torch.empty((rows,), dtype=torch.int32, device=dev)

    def cstruct(self, T: int) -> _lib.CDistillOut:
        p = lambda t: t.data_ptr()
        return _lib.CDistillOut(p(self.kl), T, p(self.teacher_top1), p(self.student_top1), p(self.agreement), p(self.teacher_logprobs),
                                p(self.student_logprobs), T - 1, p(self.kl_sum), p(self.count))


FIELDS = ("kl", "kl_sum", "count", "teacher_top1", "student_top1", "agreement", "teacher_logprobs", "student_logprobs")


@torch.no_grad()
def distill_report(teacher, student, x: torch.Tensor, y: torch.Tensor, *, temperature: float = 1.0,
                   lengths: Optional[torch.Tensor] = None, until_sep: bool = False, ignore_id: Optional[int] = None,
                   student_x: Optional[torch.Tensor] = None, frame_counts=None) -> dict:
    """How far the student's next-token distributions are from the teacher's on given captions.

    ``x``: frames [B,F,3,S,S] or the teacher's ``memory``; ``student_x``: the student's frames or memory [B,F,D] (default: ``x``
    through the student's own encoder, when ``x`` is frames and the student has one); ``y``: CLS-first ids [B, T] or [B, n, T].
    Positions behind a row's length (``lengths``, and / or its first SEP with ``until_sep``) are ignored.  -> dict on ``x``'s
    device, shaped [B, (n,) ...]: ``kl`` fp32 [.., T] = KL(softmax(teacher / temperature) || softmax(student / temperature)) per
    position in nats, ``kl_sum`` / ``count`` per row, ``teacher_top1`` / ``student_top1`` int64 [.., T] and ``agreement`` bool,
    ``teacher_logprobs`` / ``student_logprobs`` fp32 [.., T-1] of the given next tokens (score()'s ignore rules; at temperature 1
    score()'s bits), and two scalars: ``kl_loss`` = temperature^2 * kl.sum() / B -- the reference's LOSS 2
    (KLDivLoss('batchmean') * temperature^2) when nothing is ignored and n is 1 -- and ``ce_loss`` = the mean of -student_logprobs
    over the counted targets != 0, LOSS 3 (CrossEntropyLoss(ignore_index=0)).
    Clips go through in chunks of the smaller of the two handles' max_batch // n.
    frame_counts (``x`` / ``student_x`` padded [B, Fmax, ...]), or ``x`` / ``student_x`` as lists of B clips [F_b, ...]: clips that
    differ in length go to both models as they are (GitCaptioner.forward_image_enc, StudentCaptioner.score); a clip has at
    most min(the teacher's frame limit, the student's mem_tokens) frames."""
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature must be positive and finite, got {temperature}")
    if teacher._dev != student._dev:
        raise ValueError(f"teacher on {teacher._dev}, student on {student._dev}: both handles must live on one device")
    if teacher.cfg.vocab_size != student.cfg.vocab_length:
        raise ValueError(f"vocabularies differ: teacher {teacher.cfg.vocab_size}, student {student.cfg.vocab_length}")
    dev = teacher._dev
    teacher._drain()
    ids, had_n = scoring.candidates(y, dev)
    B, n, T = ids.shape
    rg = frame_counts is not None or not isinstance(x, torch.Tensor)         # a ragged batch: x is frames, packed by each model
    nclips = lambda v: v.shape[0] if isinstance(v, torch.Tensor) else len(v)
    if nclips(x) != B:
        raise ValueError("x and y disagree on the number of clips")
    if student_x is None:
        if not (rg or x.dim() == 5 or x.dtype == torch.uint8):
            raise ValueError("x is the teacher's memory: pass student_x (the student's frames or memory)")
        student_x = x
    if nclips(student_x) != B:
        raise ValueError("student_x and y disagree on the number of clips")
    if not rg and not isinstance(student_x, torch.Tensor):
        raise ValueError("student_x is a list of clips: pass x as one too, or frame_counts")
    out_dev = x.device if isinstance(x, torch.Tensor) else x[0].device
    if T > min(teacher.max_text_len, student.max_text_len + 1):
        raise ValueError(f"T={T} exceeds what the handles were created for")
    Bc = min(B, teacher.max_batch, student.max_batch // n)
    if Bc < 1 or Bc * n > teacher.max_batch * teacher.max_beams:
        raise ValueError(f"{n} candidates per clip exceed the rows the handles were created for")
    ln = scoring.row_lengths(ids, teacher.sep_token_id, until_sep, lengths)
    ign = -1 if ignore_id is None else int(ignore_id)
    frames = rg or x.dim() == 5
    chunks = []
    with torch.cuda.device(dev):
        for b0 in range(0, B, Bc):
            b1 = min(B, b0 + Bc)
            rows = (b1 - b0) * n
            fc = None if frame_counts is None else frame_counts[b0:b1]
            if rg:
                teacher.forward_image_enc(x[b0:b1], frame_counts=fc)
            elif frames:
                teacher.forward_image_enc(x[b0:b1])
            elif not (b0 == 0 and b1 == B and teacher._is_last_memory(x)):      # (as GitCaptioner.score: the handle may hold it already)
                mem = x[b0:b1].to(device=dev, dtype=torch.float32).contiguous()
                teacher._call("gitcap_set_visual", _lib.ptr(mem), mem.shape[0], mem.shape[1], teacher._stream())
                teacher._last_memory = None
                if b0 == 0 and b1 == B:
                    teacher._remember_memory(x)
            student._set_memory(student_x[b0:b1], fc if rg else None, n)
            buf = _Buffers(rows, T, dev)
            cid = ids[b0:b1].reshape(rows, T)
            cl = None if ln is None else ln[b0:b1].reshape(rows).contiguous()
            out = buf.cstruct(T)
            teacher._call("gitcap_distill", student._handle, _lib.ptr(cid), T, rows, n, T, _lib.ptr(cl), ign,
                          ctypes.c_float(float(temperature)), ctypes.byref(out), teacher._stream())
            chunks.append(buf)
    if B > Bc:
        teacher._last_memory = None

    def cat(field):
        t = torch.cat([getattr(c, field) for c in chunks], 0)
        t = t.view(B, n, *t.shape[1:]) if had_n else t
        return t.to(out_dev) if t.device != out_dev else t
    res = {f: cat(f) for f in FIELDS}
    res["agreement"] = res["agreement"].bool()
    res["kl_loss"] = float(temperature) ** 2 * res["kl"].sum() / B
    # LOSS 3: CrossEntropyLoss(ignore_index=0) -- the mean over the targets != 0 among the positions the call counted
    tgt = ids[:, :, 1:] if had_n else ids[:, 0, 1:]
    counted = (tgt != ign) & (tgt != 0) & (tgt >= 0) & (tgt < teacher.cfg.vocab_size)
    if ln is not None:
        j1 = torch.arange(1, T, device=dev)
        counted &= j1 < (ln if had_n else ln[:, 0])[..., None]
    counted = counted.to(out_dev)
    lp = res["student_logprobs"]
    res["ce_loss"] = -torch.where(counted, lp, torch.zeros_like(lp)).sum() / counted.sum().clamp(min=1)
    return res
