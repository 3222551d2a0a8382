"""Top-k token alternatives through the public surface (gitcap_attach_top_logprobs and its student twin; greedy_decode /
greedy_decode_async / caption_stream with top_logprobs=k; score(top_k=k); caption_confidence's margin; soft_labels) on git_tiny and
the tiny student with seeded weights.

Everything is exact: ids against the restatement's ranking (tests/top_logprobs_reference.py: logit descending, id ascending) of the
model's own teacher-forced fp32 logits for the same prefix -- bitwise the cached loop's logits --, rank 0 against the caption and
its token log-probabilities (==), and torch.equal between the entry points, between batch 1 and batch 3, and between the greedy
loop and score() of its caption."""
import numpy as np
import pytest
import torch

import top_logprobs_reference as T
from gitcap.config import git_tiny
from gitcap.student_config import student_synthetic_weights, student_tiny
from gitcap.weights import synthetic_weights
from gpu_support import camera, captioner_cls, make_student_native  # noqa: F401
from oracle.git_oracle import make_frames
from oracle.student_oracle import make_memory

pytestmark = pytest.mark.gpu

MAX_LEN = 8
K = 4


def _host_topk_ids(logits, k, banned=()):
    """[B, T, V] fp32 logits -> the restatement's ranking per position, int64 [B, T, k]"""
    lg = logits.float().cpu().numpy().copy()
    lg[..., list(banned)] = -np.inf
    out = np.full(lg.shape[:2] + (k,), -1, np.int64)
    for b in range(lg.shape[0]):
        for t in range(lg.shape[1]):
            r = T.ranked(lg[b, t])[:k]
            out[b, t, :len(r)] = r
    return torch.as_tensor(out)


def _check_ranks(ids, lp, top_ids, top_lp, k):
    B, n = lp.shape
    assert tuple(top_ids.shape) == tuple(top_lp.shape) == (B, n, k) and top_ids.dtype == torch.int64 and top_lp.dtype == torch.float32
    assert torch.equal(top_ids[..., 0], ids[:, 1:]) and torch.equal(top_lp[..., 0], lp)        # rank 0 = the caption, ==
    assert bool((top_lp[..., :-1] >= top_lp[..., 1:]).all()) and not bool(torch.isnan(top_lp).any())   # sorted


# ---- teacher --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def teacher(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=3, max_frames=2, max_text_len=MAX_LEN + 1, stop="never")
    fr = make_frames(3, 2, cfg.image_size, 1234).cuda()
    plain = m.greedy_decode(fr, max_len=MAX_LEN).clone()
    ids, lp, ti, tl = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True, top_logprobs=K)
    return m, cfg, fr, plain, ids.clone(), lp.clone(), ti.clone(), tl.clone()


def test_teacher_greedy_ranks(teacher):
    m, cfg, fr, plain, ids, lp, ti, tl = teacher
    assert torch.equal(ids, plain)                                              # the ids do not change
    ids2, lp2 = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True)      # nor the log-probabilities; one-shot: unattached again
    assert torch.equal(ids2, ids) and torch.equal(lp2, lp)
    _check_ranks(ids, lp, ti, tl, K)
    logits = m(fr, ids[:, :-1])
    assert torch.equal(ti.cpu(), _host_topk_ids(logits, K))
    # every rank's value, exactly: fp32 (logit - row maximum) + the winner's log-probability on the teacher-forced logits -- real,
    # non-exact weights, so a recompute whose accumulation order differed from the head's would not give these bits
    assert torch.equal(tl, (logits.gather(2, ti) - logits.max(-1, keepdim=True).values) + lp[..., None])
    ref = torch.log_softmax(logits.double(), -1).gather(2, ti)
    assert float((tl.double() - ref).abs().max()) <= 2e-5                       # (the bound of tests/test_logprob_gpu.py; the exact checks are above)
    only = m.greedy_decode(fr, max_len=MAX_LEN, top_logprobs=K)                 # without return_logprobs: (ids, top_ids, top_logprobs)
    assert len(only) == 3 and torch.equal(only[1], ti) and torch.equal(only[2], tl)
    for k in (1, 32):
        _, lpk, tik, tlk = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True, top_logprobs=k)
        kk = min(k, K)
        assert torch.equal(tik[..., :kk], ti[..., :kk]) and torch.equal(tlk[..., :kk], tl[..., :kk]) and torch.equal(lpk, lp)
    c_ids, c_lp, c_ti, c_tl = m.greedy_decode(fr.cpu(), max_len=MAX_LEN, return_logprobs=True, top_logprobs=K)
    assert c_ti.device.type == "cpu" and torch.equal(c_ti, ti.cpu()) and torch.equal(c_tl, tl.cpu())


def test_teacher_same_bits_from_every_entry_point(teacher):
    m, cfg, fr, plain, ids, lp, ti, tl = teacher
    # batch 1 against batch 3
    for b in range(3):
        _, _, t1, l1 = m.greedy_decode(fr[b:b + 1], max_len=MAX_LEN, return_logprobs=True, top_logprobs=K)
        assert torch.equal(t1, ti[b:b + 1]) and torch.equal(l1, tl[b:b + 1])
    # score() of the caption
    d = m.score(fr, ids, until_sep=False, return_top1=True, top_k=K)
    assert torch.equal(d["topk_ids"], ti) and torch.equal(d["topk_logprobs"], tl)
    assert torch.equal(d["topk_ids"][..., 0], d["top1_ids"]) and torch.equal(d["topk_logprobs"][..., 0], d["top1_logprobs"])
    assert "topk_ids" not in m.score(fr, ids, until_sep=False)                  # one-shot
    dn = m.score(fr[:1], torch.stack([ids[0], ids[1]])[None], until_sep=False, top_k=2)          # [B, n, T] candidates
    assert tuple(dn["topk_ids"].shape) == (1, 2, MAX_LEN, 2) and torch.equal(dn["topk_ids"][0, 0], ti[0, :, :2])
    # the window entry
    s = m.caption_stream(batch=3, window=2, max_len=MAX_LEN, stop="never", logprobs=True, top_logprobs=K)
    assert s.last_top_ids is None
    assert torch.equal(s.push(fr), ids)
    assert torch.equal(s.last_top_ids, ti) and torch.equal(s.last_top_logprobs, tl) and torch.equal(s.last_logprobs, lp)
    with pytest.raises(ValueError):
        m.caption_stream(batch=3, window=2, max_len=MAX_LEN, carry=True, top_logprobs=K)
    # pipelined: two submissions in flight
    futs = [m.greedy_decode_async(fr, max_len=MAX_LEN, top_logprobs=K), m.greedy_decode_async(fr[1:], max_len=MAX_LEN, top_logprobs=K),
            m.greedy_decode_async(fr, max_len=MAX_LEN)]
    a, b, c = (f.result() for f in futs)
    assert torch.equal(a[0], ids) and torch.equal(a[1], ti) and torch.equal(a[2], tl)
    assert torch.equal(b[0], ids[1:]) and torch.equal(b[1], ti[1:]) and torch.equal(b[2], tl[1:])
    assert torch.equal(c, ids)


def test_teacher_suppress_and_prompt(teacher):
    m, cfg, fr, plain, ids, lp, ti, tl = teacher
    banned = sorted({int(v) for v in ti[:, :, :2].flatten().tolist()})[:16]     # what the free run ranks first and second
    sid, slp, sti, stl = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True, top_logprobs=K, suppress_tokens=banned)
    _check_ranks(sid, slp, sti, stl, K)
    assert not bool(torch.isin(sti, torch.tensor(banned, device=sti.device)).any())
    assert torch.equal(sti.cpu(), _host_topk_ids(m(fr, sid[:, :-1]), K, banned))
    # a prompt: the forced positions carry the model's own ranks, the prompt's token is in the ids and its logprob column is 0
    prompt = torch.stack([torch.tensor([cfg.cls_token_id, 7, 9, 11]), torch.tensor([cfg.cls_token_id, 5, 3, 2]),
                          torch.tensor([cfg.cls_token_id, 8, 8, 8])]).cuda()
    pid, plp, pti, ptl = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True, top_logprobs=K, prompt=prompt)
    assert torch.equal(pid[:, :4], prompt) and bool((plp[:, :3] == 0).all())
    assert torch.equal(pti.cpu(), _host_topk_ids(m(fr, pid[:, :-1]), K))
    assert torch.equal(pti[:, 3:, 0], pid[:, 4:]) and torch.equal(ptl[:, 3:, 0], plp[:, 3:])     # free positions: rank 0 = the caption
    assert bool((ptl[:, :3] <= 0).all()) and bool(torch.isfinite(ptl).all())
    no_tk = m.greedy_decode(fr, max_len=MAX_LEN, prompt=prompt)
    assert torch.equal(no_tk, pid)                                              # the ids are those of the prompted call without it


def test_teacher_draft_refuses_the_attachment(teacher):
    from gitcap._lib import GitcapError
    m, cfg, fr, plain, ids, lp, ti, tl = teacher
    with pytest.raises(GitcapError, match="gitcap_attach_top_logprobs"):
        m.greedy_decode(fr, max_len=MAX_LEN, draft=ids, top_logprobs=K)
    assert torch.equal(m.greedy_decode(fr, max_len=MAX_LEN, draft=ids), ids)    # consumed: the next draft call runs, unattached
    assert torch.equal(m.greedy_decode(fr, max_len=MAX_LEN), ids)
    top = torch.zeros((3, 2, K), dtype=torch.int64, device="cuda")
    tlp = torch.zeros((3, 2, K), device="cuda")
    assert m._lib.gitcap_attach_top_logprobs(m._handle, 33, top.data_ptr(), tlp.data_ptr(), MAX_LEN) == -1
    assert m._lib.gitcap_attach_top_logprobs(m._handle, K, top.data_ptr(), tlp.data_ptr(), 2) == 0         # ld < max_len: refused by the call
    with pytest.raises(GitcapError, match="top-k"):
        m.greedy_decode(fr, max_len=MAX_LEN)
    assert torch.equal(m.greedy_decode(fr, max_len=MAX_LEN), ids)
    assert m._lib.gitcap_attach_top_logprobs(m._handle, K, top.data_ptr(), tlp.data_ptr(), 2) == 0
    assert m._lib.gitcap_attach_top_logprobs(m._handle, 0, None, None, 0) == 0                            # k = 0 clears
    assert torch.equal(m.greedy_decode(fr, max_len=MAX_LEN), ids)


def test_confidence_margin_and_soft_labels(teacher):
    from gitcap import caption_confidence, soft_labels
    m, cfg, fr, plain, ids, lp, ti, tl = teacher
    d = m.score(fr, ids, until_sep=False, top_k=K)
    c = caption_confidence(d)
    assert torch.equal(c["margin"], tl[..., 0] - tl[..., 1]) and bool((c["margin"] >= 0).all())
    assert torch.equal(c["confidence"], caption_confidence(m.score(fr, ids, until_sep=False)))
    one = dict(topk_logprobs=torch.tensor([[[-0.5, float("-inf")]]]))
    assert bool(torch.isposinf(caption_confidence(one)["margin"]).all())
    lengths = torch.tensor([MAX_LEN + 1, 4, 6])
    s = soft_labels(m, fr, ids, K, lengths=lengths)
    assert torch.equal(s["ids"], ti) and torch.equal(s["logprobs"], tl)
    want = torch.log1p(-torch.exp(tl.double()).sum(-1).clamp(max=1.0)).float()
    assert torch.equal(s["tail_logprob"], want) and bool((s["tail_logprob"] <= 0).all()) and not bool(torch.isnan(s["tail_logprob"]).any())
    sc = m.score(fr, ids, lengths=lengths)
    assert s["mask"].dtype == torch.bool and torch.equal(s["mask"].sum(-1).int(), sc["count"])
    assert torch.equal(caption_confidence(s)["margin"], c["margin"])


# ---- student --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def student():
    from gitcap.student import StudentCaptioner
    cfg = student_tiny()
    m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), device="cuda:0", max_batch=3, max_text_len=16, stop="never")
    mem = make_memory(3, cfg.mem_tokens, cfg.d_model, 43).cuda()
    plain = m.greedy_decode(mem, max_len=MAX_LEN).clone()
    ids, lp, ti, tl = m.greedy_decode(mem, max_len=MAX_LEN, return_logprobs=True, top_logprobs=K)
    return m, cfg, mem, plain, ids.clone(), lp.clone(), ti.clone(), tl.clone()


def test_student_ranks_and_entry_points(student):
    from gitcap._lib import GitcapError
    m, cfg, mem, plain, ids, lp, ti, tl = student
    assert torch.equal(ids, plain)
    _check_ranks(ids, lp, ti, tl, K)
    logits = m.forward_decoder(ids[:, :-1], mem)
    assert torch.equal(ti.cpu(), _host_topk_ids(logits, K))
    assert torch.equal(tl, (logits.gather(2, ti) - logits.max(-1, keepdim=True).values) + lp[..., None])      # exact, as for the teacher
    for b in range(3):                                                          # batch 1 against batch 3 (a graph of its own per B and k)
        _, _, t1, l1 = m.greedy_decode(mem[b:b + 1], max_len=MAX_LEN, return_logprobs=True, top_logprobs=K)
        assert torch.equal(t1, ti[b:b + 1]) and torch.equal(l1, tl[b:b + 1])
    _, _, t2, l2 = m.greedy_decode(mem, max_len=MAX_LEN, return_logprobs=True, top_logprobs=2)     # k is in the graph key
    assert torch.equal(t2, ti[..., :2]) and torch.equal(l2, tl[..., :2])
    assert torch.equal(m.greedy_decode(mem, max_len=MAX_LEN), ids)              # the plain graph is still the plain one
    d = m.score(mem, ids, until_sep=False, return_top1=True, top_k=K)
    assert torch.equal(d["topk_ids"], ti) and torch.equal(d["topk_logprobs"], tl) and torch.equal(d["topk_ids"][..., 0], d["top1_ids"])
    with pytest.raises(GitcapError, match="gitcap_attach_top_logprobs"):
        m.greedy_decode(mem, max_len=MAX_LEN, draft=ids, top_logprobs=K)
    assert torch.equal(m.greedy_decode(mem, max_len=MAX_LEN, draft=ids), ids)   # consumed by the refusal


def test_student_window_stream_carries_the_alternatives():
    m = make_student_native("tiny", max_batch=2, max_text_len=16)
    F = m.cfg.mem_tokens
    cam = camera((2, F, 64, 80, 3), 3).cuda()
    s = m.caption_stream(batch=2, hop=F, max_len=MAX_LEN, stop="never", logprobs=True, top_logprobs=K)
    assert s.last_top_ids is None
    out = s.push(cam)
    ids, lp, ti, tl = m.greedy_decode(cam, max_len=MAX_LEN, return_logprobs=True, top_logprobs=K)
    _check_ranks(ids, lp, ti, tl, K)
    assert torch.equal(out, ids) and torch.equal(s.last_logprobs, lp) and torch.equal(s.last_top_ids, ti) and torch.equal(s.last_top_logprobs, tl)
    with pytest.raises(ValueError):
        m.caption_stream(batch=1, max_len=MAX_LEN, carry=True, top_logprobs=K)


# ---- the window draft entry points at the C level, and soft_labels' mask on both models -------------------------------------------

def _attach(m, name, B):
    top = torch.zeros((B, MAX_LEN, K), dtype=torch.int64, device="cuda")
    tlp = torch.zeros((B, MAX_LEN, K), device="cuda")
    assert getattr(m._lib, name)(m._handle, K, top.data_ptr(), tlp.data_ptr(), MAX_LEN) == 0
    return top, tlp


def test_window_draft_entry_points_refuse_by_their_own_name(teacher, student):
    import ctypes
    out = torch.full((3, MAX_LEN + 1), -1, dtype=torch.int64, device="cuda")
    steps = torch.zeros(1, dtype=torch.int32, device="cuda")
    acc = (ctypes.c_int32 * 3)()
    m, ids = teacher[0], teacher[4]
    keep = _attach(m, "gitcap_attach_top_logprobs", 3)
    rc = m._lib.gitcap_window_greedy_draft(m._handle, ids.data_ptr(), MAX_LEN + 1, MAX_LEN, MAX_LEN, 0, None, out.data_ptr(), steps.data_ptr(),
                                           acc, None)
    msg = m._lib.gitcap_last_error(m._handle).decode()
    assert rc == -1 and msg.startswith("window_greedy_draft: top-k alternatives are attached (gitcap_attach_top_logprobs)"), msg
    assert bool((out == -1).all())                                              # nothing launched
    assert torch.equal(m.greedy_decode(teacher[2], max_len=MAX_LEN), ids)       # consumed: the next call is unattached
    s, sids = student[0], student[4]
    keep2 = _attach(s, "gitcap_student_attach_top_logprobs", 3)
    rc = s._lib.gitcap_student_window_greedy_draft(s._handle, sids.data_ptr(), MAX_LEN + 1, MAX_LEN, MAX_LEN, 0, out.data_ptr(), steps.data_ptr(),
                                                   acc, None)
    msg = s._lib.gitcap_student_last_error(s._handle).decode()
    assert rc == -1 and msg.startswith("student_window_greedy_draft: top-k alternatives are attached"), msg
    assert torch.equal(s.greedy_decode(student[2], max_len=MAX_LEN), sids)
    torch.cuda.synchronize()
    del keep, keep2


@pytest.mark.parametrize("which", ["teacher", "student"])
def test_soft_labels_mask_elementwise(teacher, student, which):
    """the mask against what score itself counted: a counted position has a log-probability below 0, an ignored one exactly 0"""
    from gitcap import soft_labels
    m, cfg, x, _, ids = (teacher if which == "teacher" else student)[:5]
    V = cfg.vocab_size if which == "teacher" else cfg.vocab_length
    y = ids.clone()
    y[0, 4] = cfg.sep_token_id                  # a first SEP: positions behind it are not counted
    y[1, -1] = V + 5                            # a target outside the vocabulary (the last column is a target only, never an input)
    y[2, 3] = -1 if which == "teacher" else V   # and one inside a row, on either side of the range
    lengths = torch.tensor([MAX_LEN + 1, MAX_LEN + 1, 6])
    for ln in (None, lengths):
        s = soft_labels(m, x, y, K, lengths=ln)
        d = m.score(x, y, lengths=ln)
        assert s["mask"].dtype == torch.bool and tuple(s["mask"].shape) == (3, MAX_LEN)
        assert torch.equal(s["mask"], d["token_logprobs"] != 0) and bool((d["token_logprobs"][s["mask"]] < 0).all())
        assert torch.equal(s["mask"].sum(-1).int(), d["count"])
        assert not bool(s["mask"][0, 4:].any()) and not bool(s["mask"][1, -1]) and not bool(s["mask"][2, 2])
        assert tuple(s["ids"].shape) == (3, MAX_LEN, K) and not bool(torch.isnan(s["tail_logprob"]).any())
    y3 = torch.stack([y, ids], 1)               # [B, n, T] candidates
    if which == "teacher":
        s = soft_labels(m, x[:1], y3[:1], 2)
        assert tuple(s["mask"].shape) == (1, 2, MAX_LEN) and torch.equal(s["mask"], m.score(x[:1], y3[:1])["token_logprobs"] != 0)
