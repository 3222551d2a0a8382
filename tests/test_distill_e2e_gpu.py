"""gitcap.distill_report end to end (include/gitcap.h: gitcap_distill): both models' own forward_decoder logits pushed through
tests/distill_reference.py under its bound, score()'s bits at temperature 1, the refusals, and decoding left as it was."""
import dataclasses

import numpy as np
import pytest
import torch

import distill_reference as D
import score_reference as S
import gitcap
from gitcap._lib import GitcapError
from gitcap.config import git_tiny
from gitcap.student import StudentCaptioner
from gitcap.student_config import student_base, student_synthetic_weights, student_tiny
from gitcap.weights import synthetic_weights
from gpu_support import NAN, captioner_cls, close_to_fp64, mid768, same_bits  # noqa: F401
from oracle.git_oracle import make_frames

pytestmark = pytest.mark.gpu
T = 7


def _pair(captioner_cls, size):
    cfg = git_tiny(2) if size == "tiny" else mid768(2)
    scfg = dataclasses.replace(student_tiny() if size == "tiny" else student_base(), vocab_length=cfg.vocab_size)
    F = 2 if size == "tiny" else 3
    t = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=3, max_frames=F, max_text_len=T + 1, max_beams=2, stop="never")
    s = StudentCaptioner(cfg=scfg, weights=student_synthetic_weights(scfg, 0), device="cuda:0", max_batch=6, max_text_len=T + 1, stop="never")
    return t, s, cfg, scfg, F


@pytest.fixture(scope="module")
def tiny(captioner_cls):
    return _pair(captioner_cls, "tiny")


def _inputs(cfg, scfg, F, B, n, seed=5):
    g = torch.Generator().manual_seed(seed + 10 * B + n)
    frames = make_frames(B, F, cfg.image_size, 1234).cuda()
    smem = torch.randn(B, scfg.mem_tokens, scfg.d_model, generator=g).cuda()
    y = torch.randint(1, cfg.vocab_size, (B, n, T), generator=g)
    y[..., 0] = cfg.cls_token_id if hasattr(cfg, "cls_token_id") else 1
    y[0, 0, 3] = 0                                              # LOSS 3 ignores it
    lengths = torch.tensor([[T - (b + c) % 3 for c in range(n)] for b in range(B)])
    return frames, smem, y.cuda(), lengths


def _reference(t, s, frames, smem, y, lengths, tau, ignore_id=-1):
    B, n, _ = y.shape
    mem = t.forward_image_enc(frames)
    mem = mem[1] if isinstance(mem, (tuple, list)) else mem
    tl = torch.stack([t.forward_decoder(y[:, c], mem) for c in range(n)], 1).reshape(B * n, T, -1)
    sl = torch.stack([s.forward_decoder(y[:, c], smem) for c in range(n)], 1).reshape(B * n, T, -1)
    ln = None if lengths is None else lengths.reshape(-1).numpy()
    return D.distill_logits(tl.cpu().numpy(), sl.cpu().numpy(), y.reshape(B * n, T).cpu().numpy(), ln, ignore_id, tau)


def _check(t, s, cfg, scfg, F, B, n, tau, ragged):
    frames, smem, y, lengths = _inputs(cfg, scfg, F, B, n)
    lengths = lengths if ragged else None
    yy = y if n > 1 else y[:, 0]
    ln = None if lengths is None else (lengths if n > 1 else lengths[:, 0])
    ref = _reference(t, s, frames, smem, y, lengths, tau)
    got = gitcap.distill_report(t, s, frames, yy, temperature=tau, lengths=ln, student_x=smem)
    what = f"B={B} n={n} tau={tau} ragged={ragged}"
    shape = (B, n) if n > 1 else (B,)
    assert tuple(got["kl"].shape) == shape + (T,) and tuple(got["student_logprobs"].shape) == shape + (T - 1,)
    kl = got["kl"].reshape(B * n, T).cpu().numpy().astype(np.float64)
    close_to_fp64(kl, ref["kl"], D.bound_kl(ref["G"]), what + " kl", flips=False)
    assert np.array_equal(got["teacher_top1"].reshape(B * n, T).cpu().numpy(), ref["t_top1"]), what
    assert np.array_equal(got["student_top1"].reshape(B * n, T).cpu().numpy(), ref["s_top1"]), what
    assert np.array_equal(got["agreement"].reshape(B * n, T).cpu().numpy(), ref["agree"]), what
    assert np.array_equal(got["count"].reshape(-1).cpu().numpy(), ref["count"]), what
    bsum = D.bound_kl(ref["G"]).sum(1) + T * 2.0 ** -24 * np.abs(ref["kl"]).sum(1)
    close_to_fp64(got["kl_sum"].reshape(-1).cpu().numpy(), ref["kl_sum"], bsum, what + " kl_sum", flips=False)
    for k, r in (("teacher_logprobs", "t_lp"), ("student_logprobs", "s_lp")):
        close_to_fp64(got[k].reshape(B * n, T - 1).cpu().numpy(), ref[r], S.bound_lp(ref[r]), what + " " + k, flips=False)
    kl_loss = D.kl_loss(ref["kl"], B, tau)
    assert abs(float(got["kl_loss"]) - kl_loss) <= tau * tau * float(bsum.sum()) / B + 1e-6 * abs(kl_loss), what
    ce = D.ce_loss(ref["s_lp"], y.reshape(B * n, T).cpu().numpy(), ref["counted"])
    assert abs(float(got["ce_loss"]) - ce) <= float(S.bound_lp(ref["s_lp"]).max()) + 1e-6 * abs(ce), what
    if tau == 1.0:          # score()'s bits
        st = t.score(frames, yy, lengths=ln, until_sep=False)
        ss = s.score(smem, yy, lengths=ln, until_sep=False)
        assert same_bits(got["teacher_logprobs"].contiguous(), st["token_logprobs"].contiguous()), what
        assert same_bits(got["student_logprobs"].contiguous(), ss["token_logprobs"].contiguous()), what


@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_report_against_own_logits(tiny, B, n, tau):
    t, s, cfg, scfg, F = tiny
    _check(t, s, cfg, scfg, F, B, n, tau, ragged=(B + n) % 2 == 0)


def test_report_mid768_student_base(captioner_cls):
    t, s, cfg, scfg, F = _pair(captioner_cls, "mid")
    _check(t, s, cfg, scfg, F, 3, 2, 2.0, ragged=True)


def test_refusals_write_nothing(tiny, captioner_cls):
    t, s, cfg, scfg, F = tiny
    frames, smem, y, _ = _inputs(cfg, scfg, F, 2, 1)
    with pytest.raises(ValueError):
        gitcap.distill_report(t, s, frames, y[:, 0], temperature=0.0, student_x=smem)
    other = dataclasses.replace(student_tiny(), vocab_length=cfg.vocab_size - 100)
    s2 = StudentCaptioner(cfg=other, weights=student_synthetic_weights(other, 0), device="cuda:0", max_batch=6, max_text_len=T + 1, stop="never")
    with pytest.raises(ValueError):
        gitcap.distill_report(t, s2, frames, y[:, 0], student_x=smem)
    # the C call itself: poisoned outputs stay poisoned
    import ctypes
    from gitcap import _lib
    t.forward_image_enc(frames)
    ids = y[:, 0].contiguous()
    kl = torch.full((2, T), NAN, device="cuda")
    out = _lib.CDistillOut(kl.data_ptr(), T, None, None, None, None, None, 0, None, None)
    def call(st, temp, rows=2):
        return t._lib.gitcap_distill(t._handle, st._handle, _lib.ptr(ids), T, rows, 1, T, None, -1, ctypes.c_float(temp), ctypes.byref(out), t._stream())
    fresh = StudentCaptioner(cfg=scfg, weights=student_synthetic_weights(scfg, 0), device="cuda:0", max_batch=6, max_text_len=T + 1, stop="never")
    assert call(fresh, 1.0) == -2                               # GITCAP_ERR_STATE: before set_memory
    assert b"set_memory" in t._lib.gitcap_last_error(t._handle)
    s._call("gitcap_student_set_memory", _lib.ptr(smem), 2, s._stream())
    assert call(s2, 1.0) != 0                                   # vocabularies (and no memory)
    for temp in (0.0, -1.0, float("inf"), float("nan")):
        assert call(s, temp) == -1
    assert call(s, 1.0, rows=1) == -1                           # batch mismatch
    torch.cuda.synchronize()
    assert bool(torch.isnan(kl).all())
    assert call(s, 1.0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(kl).all())


def test_decoding_unchanged_and_workspace_counted(tiny):
    t, s, cfg, scfg, F = tiny
    frames, smem, y, _ = _inputs(cfg, scfg, F, 2, 1)
    before_t = t.greedy_decode(frames, max_len=T, stop="never").clone()
    before_s = s.greedy_decode(smem, max_len=T).clone()
    import ctypes
    ws0 = ctypes.c_int64()
    t._call("gitcap_workspace_bytes", ctypes.byref(ws0))
    gitcap.distill_report(t, s, frames, y[:, 0], temperature=2.0, student_x=smem)
    ws1 = ctypes.c_int64()
    t._call("gitcap_workspace_bytes", ctypes.byref(ws1))
    assert ws1.value >= ws0.value
    assert torch.equal(t.greedy_decode(frames, max_len=T, stop="never"), before_t)
    assert torch.equal(s.greedy_decode(smem, max_len=T), before_s)
