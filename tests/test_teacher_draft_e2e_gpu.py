"""GitCaptioner.greedy_decode(draft=...), gitcap_greedy_draft / gitcap_window_greedy_draft, caption_stream(carry=True) and
gitcap.draft_and_verify on git_tiny with seeded weights (one case on GIT-base): ids, steps and the log-probabilities' bits equal the
plain call's, whatever the draft holds."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gitcap.config import git_base, git_tiny
from gitcap.weights import synthetic_weights
from gpu_support import captioner_cls, make_student, ptr, stream  # noqa: F401
from oracle.git_oracle import make_frames

pytestmark = pytest.mark.gpu

ERR_ARG = -1
B, F, L = 4, 2, 10
SEED = 1247
I32 = torch.int32


@pytest.fixture(scope="module")
def model(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=B, max_frames=F, max_text_len=12, stop="never")
    fr = make_frames(B, F, cfg.image_size, SEED).cuda()
    c, lp = m.greedy_decode(fr, max_len=L, return_logprobs=True)
    return m, cfg, fr, c.clone(), lp.clone()


def _check(m, fr, d, c, lp0, **kw):
    before = m.draft_stats()
    got, lp = m.greedy_decode(fr, max_len=L, draft=d, return_logprobs=True, **kw)
    assert torch.equal(got, c)
    assert torch.equal(lp.view(I32), lp0.view(I32))
    after = m.draft_stats()
    return m.last_accepted.tolist(), after[3] - before[3], after[1] - before[1]


def test_plain_caption_as_draft_is_accepted_whole(model):
    m, cfg, fr, c, lp0 = model
    acc, tail, offered = _check(m, fr, c, c, lp0)
    assert acc == [L] * B and tail == 0 and offered == B * L


def test_rows_rejected_at_their_own_position(model):
    m, cfg, fr, c, lp0 = model
    k = [1, 4, 2, 9]
    d = c.clone()
    for b, kb in enumerate(k):
        d[b, kb] = (d[b, kb] + 1) % cfg.vocab_size
    acc, tail, _ = _check(m, fr, d, c, lp0)
    assert acc == [kb - 1 for kb in k]
    assert tail == L - min(k)


def test_random_short_long_and_out_of_vocabulary_drafts(model):
    m, cfg, fr, c, lp0 = model
    g = torch.Generator().manual_seed(5)
    rnd = torch.randint(0, cfg.vocab_size, (B, L + 1), generator=g).cuda()
    _check(m, fr, rnd, c, lp0)
    acc, tail, offered = _check(m, fr, c[:, :2], c, lp0)                    # n = 1
    assert acc == [1] * B and tail == L - 1 and offered == B
    _check(m, fr, c, c, lp0)                                                # n = max_len
    acc, tail, _ = _check(m, fr, c[:, :6], c, lp0)                          # shorter than the caption
    assert acc == [5] * B and tail == L - 5
    bad = c.clone()
    bad[0, 3], bad[1, 1], bad[2, 5] = -1, cfg.vocab_size, 2 ** 40
    acc, _, _ = _check(m, fr, bad, c, lp0)
    assert acc == [2, 0, 4, L]
    acc, _, _ = _check(m, fr, torch.cat([c, c[:, 1:]], 1), c, lp0)          # longer than max_len: trimmed
    assert acc == [L] * B
    assert torch.equal(m.greedy_decode(fr.cpu(), max_len=L, draft=c.cpu()), c.cpu())


def test_stop_rules(model, captioner_cls):
    m, cfg, fr, c, lp0 = model
    w = dict(synthetic_weights(cfg, 0))
    w["head.b"] = w["head.b"].copy()
    w["head.b"][cfg.sep_token_id] = 1e4                                     # every row emits SEP at once
    ms = captioner_cls(cfg, w, max_batch=B, max_frames=F, max_text_len=12, stop="all_sep")
    plain, lp0s = ms.greedy_decode(fr, max_len=L, return_logprobs=True)
    assert tuple(plain.shape) == (B, 2)
    full = ms.greedy_decode(fr, max_len=L, stop="never")
    for d in (full, full[:, :3], torch.zeros_like(full)):
        before = ms.draft_stats()
        got, lp = ms.greedy_decode(fr, max_len=L, draft=d, return_logprobs=True)
        assert torch.equal(got, plain) and torch.equal(lp.view(I32), lp0s.view(I32))
        assert ms.draft_stats()[3] == before[3]                             # fired inside the covered part: no tail
        assert torch.equal(ms.greedy_decode(fr, max_len=L, stop="never", draft=d), full)
    # all_sep on the model that never fires: the whole loop
    got = m.greedy_decode(fr, max_len=L, stop="all_sep", draft=c[:, :4])
    assert torch.equal(got, m.greedy_decode(fr, max_len=L, stop="all_sep"))


def test_ragged_batch(model):
    m, cfg, fr, c, _ = model
    counts = [2, 1, 2, 1]
    plain, lp0 = m.greedy_decode(fr, max_len=L, frame_counts=counts, return_logprobs=True)
    d = plain.clone()
    d[1, 3] = (d[1, 3] + 1) % cfg.vocab_size
    got, lp = m.greedy_decode(fr, max_len=L, frame_counts=counts, draft=d, return_logprobs=True)
    assert torch.equal(got, plain) and torch.equal(lp.view(I32), lp0.view(I32))
    assert m.last_accepted.tolist() == [L, 2, L, L]


def test_forward_decoder_after_a_draft_call(model):
    m, cfg, fr, c, _ = model
    _, mem = m.forward_image_enc(fr)
    m.greedy_decode(fr, max_len=L)
    a = m.forward_decoder(c[:, :-1], mem)
    d = c.clone()
    d[2, 2] = (d[2, 2] + 1) % cfg.vocab_size
    m.greedy_decode(fr, max_len=L, draft=d)
    assert torch.equal(a, m.forward_decoder(c[:, :-1], mem))


def _c_greedy_draft(m, fr, d, n, ld, max_len, stop, acc=True):
    ids = torch.full((B, max_len + 1), -7, dtype=torch.int64, device="cuda")
    steps = torch.zeros(1, dtype=I32, device="cuda")
    a = (ctypes.c_int32 * B)()
    rc = m._lib.gitcap_greedy_draft(m._handle, ptr(fr), B, F, ptr(d), ld, n, max_len, stop, ptr(ids), ptr(steps), a if acc else None, stream())
    torch.cuda.synchronize()
    return rc, ids, steps, list(a)


def test_c_abi_and_errors(model):
    m, cfg, fr, c, _ = model
    lib, h = m._lib, m._handle
    ids0 = torch.full((B, L + 1), -7, dtype=torch.int64, device="cuda")
    steps0 = torch.zeros(1, dtype=I32, device="cuda")
    assert lib.gitcap_greedy(h, ptr(fr), B, F, L, 0, ptr(ids0), ptr(steps0), stream()) == 0
    d = c.clone()
    d[3, 6] = (d[3, 6] + 1) % cfg.vocab_size
    rc, ids, steps, acc = _c_greedy_draft(m, fr, d, L, L + 1, L, 0)
    assert rc == 0 and torch.equal(ids, ids0) and int(steps) == int(steps0) and acc == [L, L, L, 5]
    assert _c_greedy_draft(m, fr, d, L, L + 1, L, 0, acc=False)[0] == 0     # accepted_out is optional
    # the window forms
    assert lib.gitcap_window_reset(h, B, F) == 0
    assert lib.gitcap_window_push(h, ptr(fr), B, F, stream()) == 0
    w0, w1 = torch.full_like(ids0, -7), torch.full_like(ids0, -7)
    assert lib.gitcap_window_greedy(h, L, 0, None, ptr(w0), ptr(steps0), stream()) == 0
    a = (ctypes.c_int32 * B)()
    assert lib.gitcap_window_greedy_draft(h, ptr(d), L + 1, L, L, 0, None, ptr(w1), ptr(steps), a, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(w0, w1) and torch.equal(w0, ids0) and list(a) == [L, L, L, 5]
    # errors
    for n, ld, ml in ((0, L + 1, L), (L + 1, L + 2, L), (3, 3, L), (2, 3, 13)):
        assert _c_greedy_draft(m, fr, d, n, ld, ml, 0)[0] == ERR_ARG, (n, ld, ml)
    assert _c_greedy_draft(m, fr, d, 2, L + 1, L, 7)[0] == ERR_ARG
    assert lib.gitcap_greedy_draft(h, ptr(fr), B, F, None, L + 1, L, L, 0, ptr(ids), ptr(steps), None, stream()) == ERR_ARG
    assert lib.gitcap_greedy_draft(h, ptr(fr), B, F, ptr(d), L + 1, L, L, 0, None, ptr(steps), None, stream()) == ERR_ARG
    assert lib.gitcap_greedy_draft(None, ptr(fr), B, F, ptr(d), L + 1, L, L, 0, ptr(ids), ptr(steps), None, stream()) == ERR_ARG
    assert lib.gitcap_draft_stats(h, None) == ERR_ARG
    assert lib.gitcap_abi_version() == 1


def test_pending_prompt_and_constraints_are_refused_and_consumed(model):
    m, cfg, fr, c, lp0 = model
    from gitcap._lib import CConstraints
    lens = torch.full((B,), 3, dtype=I32, device="cuda")
    assert m._lib.gitcap_attach_prompt(m._handle, ptr(c), L + 1, ptr(lens), 3, 3) == 0
    assert _c_greedy_draft(m, fr, c, L, L + 1, L, 0)[0] == ERR_ARG
    assert "prompt or constraints" in m._lib.gitcap_last_error(m._handle).decode()
    assert torch.equal(m.greedy_decode(fr, max_len=L), c)                   # consumed: the next plain call is the plain call
    co = CConstraints()
    co.no_repeat_ngram_size = 2
    assert m._lib.gitcap_attach_constraints(m._handle, ctypes.byref(co)) == 0
    assert _c_greedy_draft(m, fr, c, L, L + 1, L, 0)[0] == ERR_ARG
    assert torch.equal(m.greedy_decode(fr, max_len=L), c)
    rc, ids, _, acc = _c_greedy_draft(m, fr, c, L, L + 1, L, 0)
    assert rc == 0 and torch.equal(ids, c) and acc == [L] * B
    with pytest.raises(ValueError):
        m.greedy_decode(fr, max_len=L, draft=c, prompt=c[:, :2])
    with pytest.raises(ValueError):
        m.greedy_decode(fr, max_len=L, draft=c, no_repeat_ngram_size=2)
    with pytest.raises(ValueError):
        m.greedy_decode(fr, max_len=L, draft=c[:2])
    with pytest.raises(ValueError):
        m.caption_stream(batch=1, carry=True, beam_size=2)


def test_fallback_beyond_the_accept_launch(captioner_cls):
    """B * n_draft cannot exceed slot 0's text-row workspace (max_batch * max_beams * max_text_len rows) while n_draft <= max_len
    <= max_text_len, so the plain-loop fallback is reached through its other condition: more than 63 draft positions."""
    cfg = git_tiny(2)
    n = 64
    assert cfg.max_text_pos >= n
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=F, max_text_len=n, stop="never")
    fr = make_frames(2, F, cfg.image_size, SEED).cuda()
    plain, lp0 = m.greedy_decode(fr, max_len=n, return_logprobs=True)
    got, lp = m.greedy_decode(fr, max_len=n, draft=plain, return_logprobs=True)
    assert torch.equal(got, plain) and torch.equal(lp.view(I32), lp0.view(I32))
    assert m.last_accepted.tolist() == [0, 0] and m.draft_stats() == (1, 0, 0, 0)
    got = m.greedy_decode(fr, max_len=n, draft=plain[:, :n])                # 63 positions: verified
    assert torch.equal(got, plain) and m.last_accepted.tolist() == [n - 1] * 2 and m.draft_stats()[:3] == (2, 2 * (n - 1), 2 * (n - 1))


@pytest.mark.parametrize("batch", [1, 2])
def test_caption_stream_carry(model, batch):
    m, cfg, fr, _, _ = model
    frames = make_frames(batch, 9, cfg.image_size, 77).cuda()
    frames[:, 5:] = frames[:, 4:5]                                          # the scene stands still: captions repeat
    outs = {}
    for carry in (False, True):
        s = m.caption_stream(batch=batch, window=2, hop=1, max_len=L, logprobs=True, carry=carry)
        before = m.draft_stats()
        caps = []
        for i in range(9):
            o = s.push(frames[:, i])
            if o is not None:
                caps.append((o.clone(), s.last_logprobs.clone()))
        outs[carry] = caps
        st = s.stats()
        after = m.draft_stats()
        assert st["captions"] == 8
        assert (after[1] - before[1], after[2] - before[2], after[3] - before[3]) == (st["draft_tokens"], st["accepted"], st["tail_steps"])
        if carry:
            assert after[0] - before[0] == 7 and st["draft_tokens"] == 7 * batch * L
            assert st["last"]["accepted"] == batch * L and st["last"]["tail_steps"] == 0      # the last windows hold equal frames
        else:
            assert after[0] == before[0] and st["draft_tokens"] == 0
    assert len(outs[True]) == 8
    for (a, alp), (b, blp) in zip(outs[False], outs[True]):
        assert torch.equal(a, b) and torch.equal(alp.view(I32), blp.view(I32))


def test_draft_and_verify(model):
    import gitcap
    m, cfg, fr, c, lp0 = model
    student = make_student("tiny", max_batch=B)                              # (its 97 words are ids of the teacher's 197 too)
    mem = torch.randn(B, student.cfg.mem_tokens, student.cfg.d_model, generator=torch.Generator().manual_seed(2)).cuda()
    res = gitcap.draft_and_verify(m, student, fr, max_len=L, student_src=mem, return_logprobs=True)
    assert torch.equal(res["draft"], student.greedy_decode(mem, max_len=L, stop="never"))
    assert torch.equal(res["ids"], c) and torch.equal(res["logprobs"].view(I32), lp0.view(I32))
    assert tuple(res["draft"].shape) == (B, L + 1) and tuple(res["accepted"].shape) == (B,)


def test_git_base_golden_clip(captioner_cls):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "hf_base_F6.npz"))
    cfg = git_base(6)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=6, max_text_len=20, stop="never")
    fr = make_frames(2, 6, cfg.image_size, int(g["frame_seed"])).cuda()
    plain, lp0 = m.greedy_decode(fr, max_len=20, return_logprobs=True)
    d = plain.clone()
    d[0, 7] = (d[0, 7] + 1) % cfg.vocab_size
    d[1, 15] = (d[1, 15] + 1) % cfg.vocab_size
    got, lp = m.greedy_decode(fr, max_len=20, draft=d, return_logprobs=True)
    assert torch.equal(got, plain) and torch.equal(lp.view(I32), lp0.view(I32))
    assert m.last_accepted.tolist() == [6, 14] and m.draft_stats() == (1, 40, 20, 13)
