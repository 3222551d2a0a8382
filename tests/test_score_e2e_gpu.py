"""Scoring of given captions through the public surface (GitCaptioner.score / rerank, StudentCaptioner.score, gitcap_score and
gitcap_student_score) on git_tiny and the tiny student, with the seeded weights the fixtures of tests/golden/ were made with.
B = 2, T <= 8.

Reference: log_softmax in fp64 of the SAME handle's teacher-forced fp32 logits (forward_decoder), gathered at the given ids,
under the bound derived in tests/test_score_gpu.py (score_reference.bound_lp / bound_sum).  The captured target logit is bit for
bit logits[r, j, y[r, j + 1]]; candidates [B, n, T] are bit for bit n separate [B, T] calls; the score of a greedy caption is bit
for bit the log-probabilities the greedy loop reported (cached == teacher-forced)."""
import numpy as np
import pytest
import torch

import score_reference as S
from gitcap.config import git_tiny
from gitcap.student_config import student_synthetic_weights, student_tiny
from gitcap.weights import synthetic_weights
from gpu_support import captioner_cls, ptr, stream  # noqa: F401
from oracle.git_oracle import make_frames
from oracle.student_oracle import make_memory

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -2
MAX_LEN = 8


def _check_against_logits(d, logits, y, lengths, ignore_id, V, what):
    """The dict of score() against fp64 log_softmax + gather of `logits` [R, T, V] under the ignore rules."""
    R, T = y.shape
    ref = torch.log_softmax(logits.double(), -1).cpu().numpy()
    yc = y.cpu().numpy()
    ok = S.counted(yc, lengths, ignore_id, V)
    want = np.zeros((R, T - 1))
    for r in range(R):
        for j in range(T - 1):
            if ok[r, j]:
                want[r, j] = ref[r, j, yc[r, j + 1]]
    got = d["token_logprobs"].double().cpu().numpy()
    err = np.abs(got - want)
    print(f"{what}: lp {want.min():.4f} .. {want.max():.4f}, max |device - fp64| {err.max():.3e}, counted {int(ok.sum())} of {ok.size}")
    assert (err <= S.bound_lp(want)).all()
    assert (got[~ok] == 0.0).all()
    assert d["count"].cpu().numpy().tolist() == ok.sum(1).tolist()
    gs = d["sum"].double().cpu().numpy()
    for r in range(R):
        assert abs(gs[r] - want[r][ok[r]].sum()) <= S.bound_sum(want[r][ok[r]])
    if "top1_ids" in d:
        assert torch.equal(d["top1_ids"], logits[:, :-1].argmax(-1))
        t1 = torch.log_softmax(logits.double(), -1)[:, :-1].max(-1).values
        assert float((d["top1_logprobs"].double() - t1).abs().max()) <= 2e-5


# ---- teacher --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def teacher(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=2, max_text_len=MAX_LEN, max_beams=3, stop="never")
    fr = make_frames(2, 2, cfg.image_size, 1234).cuda()
    ids, lp = m.greedy_decode(fr, max_len=MAX_LEN - 1, return_logprobs=True)         # [2, 8] ids: CLS + 7 tokens
    return m, cfg, fr, ids.clone(), lp.clone()


def _given(cfg, ids, seed):
    """Captions nobody decoded: random words, a SEP in row 0, an out-of-range id and a would-be ignore_id in row 1."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, cfg.vocab_size, tuple(ids.shape), generator=g).to(ids.device)
    y[y == cfg.sep_token_id] += 1                           # the only SEP is the one placed below
    y[:, 0] = ids[:, 0]
    y[0, 4] = cfg.sep_token_id
    y[1, 2] = cfg.vocab_size + 5
    y[1, 5] = 17
    return y


def test_teacher_score_vs_forward_decoder(teacher):
    m, cfg, fr, ids, _ = teacher
    y = _given(cfg, ids, 1)
    B, T = y.shape
    _, memory = m.forward_image_enc(fr)
    logits = m.forward_decoder(y, memory)
    d = m.score(memory, y, until_sep=False, return_top1=True)
    assert tuple(d["token_logprobs"].shape) == (B, T - 1) and d["sum"].dtype == torch.float32 and d["count"].dtype == torch.int32
    _check_against_logits(d, logits, y, None, -1, cfg.vocab_size, "teacher, all positions")
    # the captured target logits: bit for bit the logits tensor's elements
    tl = torch.zeros(B * T, device="cuda")
    assert m._lib.gitcap_dbg_score_target_logits(m._handle, ptr(tl), B * T, stream()) == 0
    torch.cuda.synchronize()
    tl = tl.view(B, T)
    for r in range(B):
        for j in range(T - 1):
            c = int(y[r, j + 1])
            if 0 <= c < cfg.vocab_size:
                assert tl[r, j].view(torch.int32) == logits[r, j, c].view(torch.int32), (r, j)
    # the ignore rules: through the first SEP, ignore_id, lengths; frames in place of memory
    d2 = m.score(fr, y, ignore_id=17, return_top1=True)
    ln = np.array([5, T])
    _check_against_logits(d2, logits, y, ln, 17, cfg.vocab_size, "teacher, until_sep + ignore_id")
    assert torch.equal(d2["top1_ids"], d["top1_ids"]) and torch.equal(d2["top1_logprobs"], d["top1_logprobs"])
    d3 = m.score(memory, y, until_sep=False, lengths=torch.tensor([1, 3]))
    _check_against_logits(d3, logits, y, np.array([1, 3]), -1, cfg.vocab_size, "teacher, lengths 1 and 3")
    assert d3["count"].tolist() == [0, 1] and float(d3["sum"][0]) == 0.0
    from gitcap import caption_confidence
    c = caption_confidence(d)
    assert tuple(c.shape) == (B,) and bool(((c > 0) & (c <= 1)).all())


def test_teacher_candidates_equal_separate_calls(teacher):
    m, cfg, fr, ids, _ = teacher
    cands = torch.stack([ids, _given(cfg, ids, 2), _given(cfg, ids, 3)], dim=1)      # [B, 3, T]
    _, memory = m.forward_image_enc(fr)
    d = m.score(memory, cands, return_top1=True)
    assert tuple(d["token_logprobs"].shape) == (2, 3, ids.shape[1] - 1) and tuple(d["sum"].shape) == (2, 3)
    for k in range(3):
        one = m.score(memory, cands[:, k].contiguous(), return_top1=True)
        for key in one:
            assert torch.equal(one[key], d[key][:, k]), (k, key)
    # one clip alone: the rows beside a row do not matter
    solo = m.score(fr[1:], cands[1:], return_top1=True)
    for key in solo:
        assert torch.equal(solo[key], d[key][1:]), key
    # both forms of the head kernel
    old = m._lib.gitcap_dbg_config(10, 0)
    try:
        single = m.score(memory, cands, return_top1=True)
    finally:
        m._lib.gitcap_dbg_config(10, old)
    for key in single:
        assert torch.equal(single[key], d[key]), key


def test_teacher_score_of_its_own_greedy_caption(teacher):
    m, cfg, fr, ids, lp = teacher
    d = m.score(fr, ids, until_sep=False, return_top1=True)
    assert torch.equal(d["top1_ids"], ids[:, 1:])
    # cached == teacher-forced, bit for bit: the greedy loop's own log-probabilities
    assert torch.equal(d["token_logprobs"], lp) and torch.equal(d["top1_logprobs"], lp)


def test_teacher_rerank_known_order(teacher):
    m, cfg, fr, ids, _ = teacher
    bad = ids.clone()
    bad[:, 3] = (bad[:, 3] + 1) % cfg.vocab_size                                    # one token corrupted
    r = m.rerank(fr, torch.stack([bad, ids], dim=1))
    assert r["order"].tolist() == [[1, 0], [1, 0]] and bool((r["scores"][:, 1] > r["scores"][:, 0]).all())
    r2 = m.rerank(fr, torch.stack([ids, bad], dim=1), length_penalty=1.0)
    assert r2["order"].tolist() == [[0, 1], [0, 1]]
    assert torch.equal(r2["sum"][:, 0], r["sum"][:, 1])
    want = r2["sum"] / r2["count"].float()
    assert torch.allclose(r2["scores"], want)


def test_teacher_score_error_paths(teacher):
    m, cfg, fr, ids, _ = teacher
    from gitcap.model import GitCaptioner
    fresh = GitCaptioner(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=2, max_text_len=MAX_LEN, stop="never")
    y = ids.contiguous()
    lp = torch.full((2, 7), -5.0, device="cuda")
    rc = fresh._lib.gitcap_score(fresh._handle, ptr(y), 8, 2, 1, 8, None, -1, ptr(lp), 7, None, None, None, None, stream())
    assert rc == ERR_STATE                                                          # before encode / set_visual
    m.forward_image_enc(fr)
    long_y = torch.zeros((2, MAX_LEN + 1), dtype=torch.int64, device="cuda")
    assert m._lib.gitcap_score(m._handle, ptr(long_y), MAX_LEN + 1, 2, 1, MAX_LEN + 1, None, -1, ptr(lp), 8, None, None, None, None, stream()) == ERR_ARG
    assert m._lib.gitcap_score(m._handle, ptr(y), 8, 2, 1, 1, None, -1, ptr(lp), 7, None, None, None, None, stream()) == ERR_ARG       # T < 2
    assert m._lib.gitcap_score(m._handle, ptr(y), 8, 2, 1, 8, None, -1, ptr(lp), 6, None, None, None, None, stream()) == ERR_ARG       # ld_lp < T - 1
    assert m._lib.gitcap_score(m._handle, ptr(y), 8, 3, 1, 8, None, -1, ptr(lp), 7, None, None, None, None, stream()) == ERR_ARG       # rows != clips * beams
    big = torch.zeros((8, 8), dtype=torch.int64, device="cuda")
    assert m._lib.gitcap_score(m._handle, ptr(big), 8, 8, 4, 8, None, -1, None, 0, None, None, None, None, stream()) == ERR_ARG      # rows > max_batch * max_beams
    torch.cuda.synchronize()
    assert bool((lp == -5.0).all())
    with pytest.raises(ValueError, match="max_text_len"):
        m.score(fr, long_y)
    with pytest.raises(ValueError, match="max_batch \\* max_beams = 6"):
        m.score(fr, torch.zeros((2, 4, 8), dtype=torch.int64))
    with pytest.raises(ValueError):
        m.score(fr, ids[:, :1])
    assert m._lib.gitcap_score(None, ptr(y), 8, 2, 1, 8, None, -1, ptr(lp), 7, None, None, None, None, None) == ERR_ARG


def test_teacher_score_reports_its_memory(teacher):
    m, cfg, fr, ids, _ = teacher
    from gitcap.model import GitCaptioner
    fresh = GitCaptioner(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=2, max_text_len=MAX_LEN, stop="never")
    before = fresh.workspace_bytes()
    fresh.score(fr, ids)
    grown = fresh.workspace_bytes() - before
    fresh.score(fr, ids)
    assert grown > 0 and fresh.workspace_bytes() - before == grown                  # first use only


# ---- student --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def student():
    from gitcap.student import StudentCaptioner
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cfg = student_tiny()
    m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), device="cuda:0", max_batch=6, max_text_len=MAX_LEN, stop="never")
    mem = make_memory(2, cfg.mem_tokens, cfg.d_model, 7).cuda()
    ids, lp = m.greedy_decode(mem, max_len=MAX_LEN - 1, return_logprobs=True)
    return m, cfg, mem, ids.clone(), lp.clone()


def _student_given(cfg, ids, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, cfg.vocab_length, tuple(ids.shape), generator=g).to(ids.device)
    y[:, 0] = ids[:, 0]
    y[y == cfg.pad_token_id] = 3                            # (PAD keys are masked by the student's self-attention: keep them out)
    y[y == cfg.sep_token_id] = 3                            # the only SEP is the one placed below
    y[0, 4] = cfg.sep_token_id
    y[1, 2] = cfg.vocab_length + 5
    return y


def test_student_score_vs_forward_decoder(student):
    m, cfg, mem, ids, _ = student
    y = _student_given(cfg, ids, 1)
    B, T = y.shape
    logits = m.forward_decoder(y, mem)
    d = m.score(mem, y, until_sep=False, return_top1=True)
    _check_against_logits(d, logits, y, None, -1, cfg.vocab_length, "student, all positions")
    tl = torch.zeros(B * T, device="cuda")
    assert m._lib.gitcap_student_dbg_score_target_logits(m._handle, ptr(tl), B * T, stream()) == 0
    torch.cuda.synchronize()
    tl = tl.view(B, T)
    for r in range(B):
        for j in range(T - 1):
            c = int(y[r, j + 1])
            if 0 <= c < cfg.vocab_length:
                assert tl[r, j].view(torch.int32) == logits[r, j, c].view(torch.int32), (r, j)
    d2 = m.score(mem, y, ignore_id=int(y[1, 5]))
    _check_against_logits(d2, logits, y, np.array([5, T]), int(y[1, 5]), cfg.vocab_length, "student, until_sep + ignore_id")


def test_student_candidates_equal_separate_calls(student):
    m, cfg, mem, ids, lp = student
    cands = torch.stack([ids, _student_given(cfg, ids, 2), _student_given(cfg, ids, 3)], dim=1)
    d = m.score(mem, cands, return_top1=True)
    for k in range(3):
        one = m.score(mem, cands[:, k].contiguous(), return_top1=True)
        for key in one:
            assert torch.equal(one[key], d[key][:, k]), (k, key)
    # its own greedy caption: the arg-max at every position, and the greedy loop's log-probabilities bit for bit
    own = m.score(mem, ids, until_sep=False, return_top1=True)
    assert torch.equal(own["top1_ids"], ids[:, 1:]) and torch.equal(own["token_logprobs"], lp)
    with pytest.raises(ValueError, match="max_batch"):
        m.score(mem, torch.zeros((2, 7, 4), dtype=torch.int64))
