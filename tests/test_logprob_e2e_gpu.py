"""Per-token log-probabilities of greedy captions through the public surface (gitcap_attach_token_logprobs and its student twin,
greedy_decode(return_logprobs=True), caption_stream(logprobs=True)) on git_tiny and the tiny student, with the seeded weights the
fixtures of tests/golden/ were made with.

Reference: log_softmax of the model's own teacher-forced fp32 logits in fp64, gathered at the emitted ids, under the 2e-5 nats of
tests/test_logprob_gpu.py (the teacher-forced logits are bitwise those of the cached loop).  Everything else is torch.equal: the
values do not depend on the entry point, on the batch beside a row, or on a draft."""
import ctypes

import pytest
import torch

from gitcap.config import git_tiny
from gitcap.student_config import student_synthetic_weights, student_tiny
from gitcap.weights import synthetic_weights
from gpu_support import camera, captioner_cls, make_student_native, ptr, stream  # noqa: F401
from oracle.git_oracle import make_frames
from oracle.student_oracle import make_memory

pytestmark = pytest.mark.gpu

TOL = 2e-5
ERR_ARG = -1
STOP_NEVER = 0
MAX_LEN = 8
POISON = -4321.0


# ---- teacher --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def teacher(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=2, max_text_len=MAX_LEN, stop="never")
    fr = make_frames(2, 2, cfg.image_size, 1234).cuda()
    plain = m.greedy_decode(fr, max_len=MAX_LEN).clone()
    ids, lp = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True)
    return m, cfg, fr, plain, ids.clone(), lp.clone()


def _c_greedy(m, name, frames, B, extra=(), lp_ld=MAX_LEN + 2, attach=True):
    """One synchronous C greedy call on device frames with a poisoned attachment -> (rc, ids, lp).  lp is [B][MAX_LEN + 2] and is
    attached with its own row pitch; a smaller lp_ld (the error case) is what the library is told instead."""
    ids = torch.full((B, MAX_LEN + 1), -1, dtype=torch.int64, device="cuda")
    steps = torch.zeros(1, dtype=torch.int32, device="cuda")
    lp = torch.full((B, MAX_LEN + 2), POISON, device="cuda")
    assert lp_ld <= MAX_LEN + 2
    if attach:
        assert m._lib.gitcap_attach_token_logprobs(m._handle, ptr(lp), lp_ld) == 0
    rc = getattr(m._lib, name)(m._handle, ptr(frames), B, 2, *extra, MAX_LEN, STOP_NEVER, ptr(ids), ptr(steps), stream())
    torch.cuda.synchronize()
    return rc, ids, lp


@pytest.mark.parametrize("B", [1, 2])
def test_teacher_logprobs_vs_teacher_forced_logits(teacher, B):
    m, cfg, fr, plain, ids2, lp2 = teacher
    ids, lp = m.greedy_decode(fr[:B], max_len=MAX_LEN, return_logprobs=True)
    assert torch.equal(ids, plain[:B]) and torch.equal(ids, m.greedy_decode(fr[:B], max_len=MAX_LEN))    # the ids do not change
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (B, MAX_LEN) and lp.device == fr.device
    logits = m(fr[:B], ids[:, :-1])
    ref = torch.log_softmax(logits.double(), -1).gather(2, ids[:, 1:, None]).squeeze(-1)
    assert torch.equal(logits.argmax(-1), ids[:, 1:])
    err = (lp.double() - ref).abs().max().item()
    print(f"teacher B={B}: lp {lp.min().item():.4f} .. {lp.max().item():.4f}, max |device - fp64| {err:.3e}")
    assert err <= TOL and bool((lp <= 0).all())
    assert torch.equal(lp, lp2[:B])                                             # batch invariance: row 0 of B = 2 == B = 1
    # CPU frames in -> CPU results out
    ids_c, lp_c = m.greedy_decode(fr[:B].cpu(), max_len=MAX_LEN, return_logprobs=True)
    assert ids_c.device.type == lp_c.device.type == "cpu" and torch.equal(lp_c, lp.cpu()) and torch.equal(ids_c, ids.cpu())
    from gitcap import caption_confidence
    c = caption_confidence(ids, lp, cfg.sep_token_id)
    assert tuple(c.shape) == (B,) and bool(((c > 0) & (c <= 1)).all())


def test_teacher_logprobs_are_the_same_through_every_entry_point(teacher):
    m, cfg, fr, plain, ids2, lp2 = teacher
    from gitcap.preprocess import preprocess_frames
    cam = camera((2, 2, 80, 96, 3), 5).cuda()
    pre = preprocess_frames(cam, cfg.image_size).contiguous()
    # gitcap_greedy on the transformed frames == gitcap_greedy_raw on the camera frames
    rc, ids_a, lp_a = _c_greedy(m, "gitcap_greedy", pre, 2)
    assert rc == 0
    rc, ids_b, lp_b = _c_greedy(m, "gitcap_greedy_raw", cam, 2, extra=(80, 96))
    assert rc == 0
    assert torch.equal(ids_a, ids_b) and torch.equal(lp_a, lp_b)
    assert bool((lp_a[:, MAX_LEN:] == POISON).all()) and bool((lp_a[:, :MAX_LEN] <= 0).all())      # nothing behind max_len
    # two submissions in flight with distinct buffers
    bufs = []
    for x in (fr, pre):
        ids = torch.full((2, MAX_LEN + 1), -1, dtype=torch.int64, device="cuda")
        steps = torch.zeros(1, dtype=torch.int32, device="cuda")
        lp = torch.full((2, MAX_LEN + 3), POISON, device="cuda")
        tk = ctypes.c_int(-1)
        assert m._lib.gitcap_attach_token_logprobs(m._handle, ptr(lp), MAX_LEN + 3) == 0
        assert m._lib.gitcap_greedy_submit(m._handle, ptr(x), 2, 2, MAX_LEN, STOP_NEVER, ptr(ids), ptr(steps), stream(), ctypes.byref(tk)) == 0
        bufs.append((tk.value, ids, lp, steps))
    for tk, _, _, _ in bufs:
        assert m._lib.gitcap_greedy_wait(m._handle, tk, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs[0][1], ids2) and torch.equal(bufs[0][2][:, :MAX_LEN], lp2)
    assert torch.equal(bufs[1][1], ids_a) and torch.equal(bufs[1][2][:, :MAX_LEN], lp_a[:, :MAX_LEN])
    assert all(bool((b[2][:, MAX_LEN:] == POISON).all()) for b in bufs)
    # the frame window on the same frames (gitcap_window_greedy through caption_stream)
    s = m.caption_stream(batch=2, window=2, max_len=MAX_LEN, stop="never", logprobs=True)
    assert s.last_logprobs is None
    got = s.push(fr)
    assert torch.equal(got, ids2) and torch.equal(s.last_logprobs, lp2)
    with pytest.raises(ValueError):
        m.caption_stream(batch=2, window=2, max_len=MAX_LEN, beam_size=2, logprobs=True)


def test_teacher_attachment_is_one_shot_and_checked(teacher):
    m, cfg, fr, plain, ids2, lp2 = teacher
    lib, h = m._lib, m._handle
    # consumed by the first call: the second leaves a poisoned buffer alone
    rc, ids, lp = _c_greedy(m, "gitcap_greedy", fr, 2)
    assert rc == 0 and torch.equal(lp[:, :MAX_LEN], lp2)
    lp.fill_(POISON)
    rc, ids, _ = _c_greedy(m, "gitcap_greedy", fr, 2, attach=False)
    assert rc == 0 and torch.equal(ids, ids2) and bool((lp == POISON).all())
    # a pending attachment survives gitcap_encode, and is consumed by the greedy call behind it
    lp = torch.full((2, MAX_LEN), POISON, device="cuda")
    assert lib.gitcap_attach_token_logprobs(h, ptr(lp), MAX_LEN) == 0
    assert lib.gitcap_encode(h, ptr(fr), 2, 2, None, stream()) == 0
    rc, ids, _ = _c_greedy(m, "gitcap_greedy", fr, 2, attach=False)
    assert rc == 0 and torch.equal(lp, lp2)
    # NULL detaches
    lp.fill_(POISON)
    assert lib.gitcap_attach_token_logprobs(h, ptr(lp), MAX_LEN) == 0 and lib.gitcap_attach_token_logprobs(h, None, 0) == 0
    rc, ids, _ = _c_greedy(m, "gitcap_greedy", fr, 2, attach=False)
    assert rc == 0 and bool((lp == POISON).all())
    # ld < max_len: the ARG error at the consuming call, nothing written, and the attachment is consumed all the same
    rc, ids, lp = _c_greedy(m, "gitcap_greedy", fr, 2, lp_ld=MAX_LEN - 1)
    assert rc == ERR_ARG and bool((lp == POISON).all()) and bool((ids == -1).all())
    assert b"ld < max_len" in lib.gitcap_last_error(h)
    rc, ids, _ = _c_greedy(m, "gitcap_greedy", fr, 2, attach=False)
    assert rc == 0 and torch.equal(ids, ids2) and bool((lp == POISON).all())
    # bad attachments
    assert lib.gitcap_attach_token_logprobs(h, ptr(lp), 0) == ERR_ARG
    assert lib.gitcap_attach_token_logprobs(h, ctypes.c_void_p(lp.data_ptr() + 2), MAX_LEN) == ERR_ARG
    rc, ids, _ = _c_greedy(m, "gitcap_greedy", fr, 2, attach=False)             # neither left anything pending
    assert rc == 0 and bool((lp == POISON).all())


def test_teacher_workspace_grows_with_the_first_attach_only():
    from gitcap.model import GitCaptioner
    cfg = git_tiny(2)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=2, max_text_len=MAX_LEN, stop="never")
    fr = make_frames(1, 2, cfg.image_size, 1234).cuda()
    w0 = m.workspace_bytes()
    m.greedy_decode(fr, max_len=MAX_LEN)
    assert m.workspace_bytes() == w0
    m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True)
    w1 = m.workspace_bytes()
    assert w1 > w0
    m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True)
    assert m.workspace_bytes() == w1


# ---- student --------------------------------------------------------------------------------------------------------------------

S_LEN = 10


@pytest.fixture(scope="module")
def student():
    from gitcap.student import StudentCaptioner
    cfg = student_tiny()
    m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), device="cuda:0", max_batch=3, max_text_len=16, stop="never")
    mem = make_memory(3, cfg.mem_tokens, cfg.d_model, 43).cuda()
    plain = m.greedy_decode(mem, max_len=S_LEN).clone()
    ids, lp = m.greedy_decode(mem, max_len=S_LEN, return_logprobs=True)
    return m, cfg, mem, plain, ids.clone(), lp.clone()


@pytest.mark.parametrize("B", [1, 3])
def test_student_logprobs_vs_teacher_forced_logits(student, B):
    m, cfg, mem, plain, ids3, lp3 = student
    ids, lp = m.greedy_decode(mem[:B], max_len=S_LEN, return_logprobs=True)
    assert torch.equal(ids, plain[:B]) and tuple(lp.shape) == (B, S_LEN) and lp.dtype == torch.float32
    logits = m.forward_decoder(ids[:, :-1], mem[:B])
    ref = torch.log_softmax(logits.double(), -1).gather(2, ids[:, 1:, None]).squeeze(-1)
    err = (lp.double() - ref).abs().max().item()
    print(f"student B={B}: lp {lp.min().item():.4f} .. {lp.max().item():.4f}, max |device - fp64| {err:.3e}")
    assert err <= TOL
    assert torch.equal(lp, lp3[:B])
    assert torch.equal(m.greedy_decode(mem[:B], max_len=S_LEN), plain[:B])      # the plain call afterwards: its own graph


@pytest.mark.parametrize("B", [1, 3])
def test_student_logprobs_with_a_draft_are_those_without(student, B):
    m, cfg, mem, plain, ids3, lp3 = student
    ref, V = plain[:B], cfg.vocab_length

    def changed(col):
        d = ref.clone()
        d[:, col] = (d[:, col] + 1) % V
        return d
    for label, d, acc in (("accepted whole", ref, S_LEN), ("rejected at position 1", changed(1), 0),
                          ("rejected in the middle", changed(S_LEN // 2), S_LEN // 2 - 1)):
        ids, lp = m.greedy_decode(mem[:B], max_len=S_LEN, draft=d, return_logprobs=True)
        assert m.last_accepted == acc, label
        assert torch.equal(ids, ref) and torch.equal(lp, lp3[:B]), label
    # one-shot on this handle too: a draft call without the keyword returns ids only
    assert torch.equal(m.greedy_decode(mem[:B], max_len=S_LEN, draft=ref), ref)


def test_student_attachment_is_checked(student):
    m, cfg, mem, plain, ids3, lp3 = student
    lib, h = m._lib, m._handle
    lp = torch.full((3, S_LEN), POISON, device="cuda")
    ids = torch.full((3, S_LEN + 1), -1, dtype=torch.int64, device="cuda")
    steps = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.gitcap_student_attach_token_logprobs(h, ptr(lp), 0) == ERR_ARG
    assert lib.gitcap_student_attach_token_logprobs(h, ptr(lp), S_LEN - 1) == 0
    assert lib.gitcap_student_greedy(h, ptr(mem), 3, S_LEN, STOP_NEVER, ptr(ids), ptr(steps), stream()) == ERR_ARG
    assert lib.gitcap_student_greedy(h, ptr(mem), 3, S_LEN, STOP_NEVER, ptr(ids), ptr(steps), stream()) == 0      # consumed by the failure
    torch.cuda.synchronize()
    assert bool((lp == POISON).all()) and torch.equal(ids, plain)
    # ld > max_len: the columns behind max_len stay as they were
    wide = torch.full((3, S_LEN + 4), POISON, device="cuda")
    assert lib.gitcap_student_attach_token_logprobs(h, ptr(wide), S_LEN + 4) == 0
    assert lib.gitcap_student_greedy(h, ptr(mem), 3, S_LEN, STOP_NEVER, ptr(ids), ptr(steps), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :S_LEN], lp3) and bool((wide[:, S_LEN:] == POISON).all())


def test_student_stream_logprobs_with_carry():
    from gitcap import caption_confidence
    from gitcap.student import StudentCaptioner

    ma, mb = (make_student_native("tiny", max_batch=2, max_text_len=16) for _ in range(2))
    F, max_len, n = ma.cfg.mem_tokens, 8, ma.cfg.mem_tokens + 4
    cam = camera((1, n, 64, 80, 3), 3)
    cam[:, F:F + 3] = cam[:, F:F + 1]                   # a repeated frame: the carried draft is accepted for a while
    cam = cam.cuda()
    with pytest.raises(ValueError):
        ma.caption_stream(batch=1, max_len=max_len, beams=2, logprobs=True)
    sa = ma.caption_stream(batch=1, hop=1, max_len=max_len, stop="never", carry=True, logprobs=True)
    sb = mb.caption_stream(batch=1, hop=1, max_len=max_len, stop="never", logprobs=True)
    captions = 0
    for i in range(n):
        got, want = sa.push(cam[:, i]), sb.push(cam[:, i])
        assert (got is None) == (want is None)
        if got is None:
            continue
        captions += 1
        assert torch.equal(got, want) and torch.equal(sa.last_logprobs, sb.last_logprobs)
        assert tuple(sa.last_logprobs.shape) == (1, max_len) and sa.last_logprobs.device == got.device
        c = caption_confidence(got, sa.last_logprobs, ma.cfg.sep_token_id)
        assert bool(((c > 0) & (c <= 1)).all())
    assert captions == 5 and sa.stats()["draft_tokens"] > 0
    # CPU frames in: the log-probabilities are on the CPU as the caption is
    sc = ma.caption_stream(batch=1, hop=ma.cfg.mem_tokens, max_len=max_len, stop="never", logprobs=True)
    out = sc.push(cam[:, :F].cpu())
    assert out.device.type == "cpu" and sc.last_logprobs.device.type == "cpu"
