"""The student's search that ends hypotheses at SEP on the device (include/gitcap.h: gitcap_student_attach_search,
gitcap_student_pool_beam_search), on the cases tests/test_student_search.py certifies: beam_search(eos=True) against
beam_search_host(eos=True), the window stream and the pool against beam_search, the refusals and the workspace."""
import ctypes
import functools

import pytest
import torch

import student_search_support as S
from gitcap import _lib

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -2            # include/gitcap.h: GITCAP_ERR_ARG, GITCAP_ERR_STATE

# |device score - host score|: the largest over the certified cases was 2.87e-06 on an MI355X (profiles/r33_student_search.txt): a few
# fp32 ulps of scores between -4 and -25 (fp32 log-softmax from chunk statistics against torch's, fp32 powf against Python floats).
# The bound is 4 x that, below the 1e-3 / 16 that the certified gap allows.
SCORE_TOL = 4 * 2.87e-06
assert SCORE_TOL < S.GAP_MIN / 16


@functools.lru_cache(maxsize=None)
def model():
    from gitcap.student import StudentCaptioner
    cfg, w = S.tiny_weights()
    return StudentCaptioner(cfg=cfg, weights=w, device="cuda:0", max_batch=S.CLIPS * S.K, max_text_len=S.MAX_LEN)


def call_args(case):
    m = model()
    inp, opts = S.INPUTS[case[0]], S.OPTS[case[1]]
    src = [t.cuda() for t in S.clip_memories(m.cfg, inp)]
    kw = dict(max_len=S.MAX_LEN, k=S.K, eos=True, **opts)
    if "min_length" in inp:
        kw["min_length"] = inp["min_length"]
    if "prompt" in inp:
        kw["prompt"] = S.prompt_rows(m.cfg, inp)
    return src, kw


@functools.lru_cache(maxsize=None)
def both(case):
    """(device result, host result) of one certified case, computed once"""
    src, kw = call_args(case)
    return model().beam_search(src, **kw), model().beam_search_host(src, **kw)


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "-".join(c))
def test_device_search_equals_the_host_search(case):
    dev, host = both(case)
    assert torch.equal(dev["predictions"], host["predictions"])
    assert torch.equal(dev["lengths"], host["lengths"])
    diff = float((dev["scores"] - host["scores"]).abs().max())
    print(case, "max |device - host| score", diff)
    assert diff <= SCORE_TOL


@pytest.mark.parametrize("case", [c for c in S.CASES if S.OPTS[c[1]].get("repetition_penalty", 1.0) == 1.0 and "min_length" not in S.INPUTS[c[0]]],
                         ids=lambda c: "-".join(c))
def test_scores_are_the_scored_sum_of_the_hypothesis(case):
    """scores * lengths ** length_penalty = the summed log-probabilities student.score gives the hypothesis with the token that
    finished it behind it (SEP, or at the last step whatever the candidate was: beam_search_host's last_tokens).  The cases without
    a penalty or a ban, whose scores are those of rewritten logits."""
    m = model()
    dev, host = both(case)
    src, kw = call_args(case)
    y = dev["predictions"].clone()
    n = y.shape[1]
    for b in range(S.CLIPS):
        for r in range(n):
            y[b, r, int(dev["lengths"][b, r])] = host["last_tokens"][b, r]
    lens = (dev["lengths"] + 1).to(torch.int64)
    plen = torch.tensor([len(p) for p in S.INPUTS[case[0]].get("prompt", [[]] * S.CLIPS)])[:, None].cuda()      # forced tokens beyond CLS carry no score
    sc = m.score(src, y, lengths=lens, until_sep=False)
    lp = sc["token_logprobs"]
    pos = torch.arange(lp.shape[-1], device=lp.device)[None, None, :]
    total = (lp * ((pos >= plen[:, :, None]) & (pos < (lens - 1)[:, :, None]))).sum(-1)
    want = dev["scores"].double() * dev["lengths"].double() ** kw.get("length_penalty", 1.0)
    diff = float((want - total.double()).abs().max())
    print(case, "max |score * len^lp - scored sum|", diff)
    assert diff <= SCORE_TOL


def test_defaults_are_the_plain_beam_search():
    m = model()
    src = [t.cuda() for t in S.clip_memories(m.cfg, {})]
    plain = m.beam_search(src, max_len=S.MAX_LEN, k=S.K)
    assert plain.shape == (S.CLIPS, S.MAX_LEN)
    assert torch.equal(plain, m.beam_search(src, max_len=S.MAX_LEN, k=S.K, eos=False, length_penalty=1.0, num_keep_best=1))
    assert torch.equal(plain, m.beam_search_host(torch.stack(src), max_len=S.MAX_LEN, k=S.K))
    with pytest.raises(ValueError):
        m.beam_search(src, max_len=S.MAX_LEN, k=S.K, num_keep_best=2)


def test_pool_with_beams_equals_beam_search_whichever_cameras_share_the_call():
    m = model()
    F, D = m.cfg.mem_tokens, m.cfg.d_model
    g = torch.Generator().manual_seed(5)
    fills = [1, F - 1, F + 2]                                   # camera 2 has wrapped its ring
    toks = [torch.randn(n, D, generator=g).cuda() for n in fills]
    opts = S.OPTS["C"]
    for eos in (True, False):
        pool = m.stream_pool(3, hop=10 ** 6, max_len=S.MAX_LEN, beams=S.K, **(dict(eos=True, **opts) if eos else {}))
        for s, t in enumerate(toks):
            for i in range(0, t.shape[0], F):
                pool.push(t[i:i + F], [s] * min(F, t.shape[0] - i))
        for group in ([0, 1, 2], [2], [1, 0]):
            out = pool.caption(group)
            for s in group:
                ref = m.beam_search([toks[s][-F:]], max_len=S.MAX_LEN, k=S.K, **(dict(eos=True, **opts) if eos else {}))
                if eos:
                    assert torch.equal(pool.last_predictions[s], ref["predictions"][0]) and torch.equal(out[s], ref["predictions"][0, 0])
                    assert torch.equal(pool.last_scores[s], ref["scores"][0]) and torch.equal(pool.last_lengths[s], ref["lengths"][0])
                else:
                    assert torch.equal(out[s], ref[0])
                assert pool.last_frames[s] == min(fills[s], F)


def test_window_stream_with_beams_equals_beam_search():
    from gpu_support import make_student_native
    m = make_student_native("tiny", max_batch=2 * S.K, max_text_len=S.MAX_LEN)
    F, size = m.cfg.mem_tokens, m.image_encoder.cfg.img_size
    frames = torch.randn(2, F + 1, 3, size, size, generator=torch.Generator().manual_seed(3)).cuda()
    opts = S.OPTS["B"]
    stream = m.caption_stream(batch=2, hop=1, max_len=S.MAX_LEN, beams=S.K, eos=True, **opts)
    for i in range(F + 1):
        out = stream.push(frames[:, i])
        if i < F - 1:
            assert out is None
            continue
        ref = m.beam_search(frames[:, i + 1 - F:i + 1], max_len=S.MAX_LEN, k=S.K, eos=True, **opts)
        assert torch.equal(out, ref["predictions"][:, 0]) and torch.equal(stream.last_predictions, ref["predictions"])
        assert torch.equal(stream.last_scores, ref["scores"]) and torch.equal(stream.last_lengths, ref["lengths"])


def test_greedy_family_refuses_and_consumes_the_attachment():
    m = model()
    lib, h = m._lib, m._handle
    B, L = 2, S.MAX_LEN - 1
    mem = torch.randn(B, m.cfg.mem_tokens, m.cfg.d_model).cuda()
    ids = torch.zeros((B, L + 1), dtype=torch.int64).cuda()
    ids[:, 0] = m.cfg.cls_token_id
    scores = torch.zeros((B, 1), dtype=torch.float32).cuda()
    fm = torch.zeros((B, L, m.cfg.mem_tokens), dtype=torch.float32).cuda()
    opt = _lib.CStudentSearchOptions(1, 1.0, 0, 1.0, scores.data_ptr(), None)
    acc = ctypes.c_int32(0)
    sid = (ctypes.c_int32 * B)(0, 1)
    seen = (ctypes.c_int32 * B)()
    p = _lib.ptr
    m.greedy_decode(mem, max_len=L)                              # (the handle holds a memory of B rows)
    assert lib.gitcap_student_pool_reset(h, 2) == 0
    calls = {
        "gitcap_student_greedy": lambda: lib.gitcap_student_greedy(h, p(mem), B, L, 0, p(ids), None, None),
        "gitcap_student_greedy_draft": lambda: lib.gitcap_student_greedy_draft(h, p(mem), B, p(ids), L + 1, 2, L, 0, p(ids), None, ctypes.byref(acc), None),
        "gitcap_student_window_greedy": lambda: lib.gitcap_student_window_greedy(h, L, 0, p(ids), None, None),
        "gitcap_student_window_greedy_partial": lambda: lib.gitcap_student_window_greedy_partial(h, L, 0, p(ids), None, ctypes.byref(acc), None),
        "gitcap_student_window_greedy_draft": lambda: lib.gitcap_student_window_greedy_draft(h, p(ids), L + 1, 2, L, 0, p(ids), None, ctypes.byref(acc), None),
        "gitcap_student_pool_greedy": lambda: lib.gitcap_student_pool_greedy(h, sid, B, L, 0, p(ids), None, seen, None),
        "gitcap_student_score": lambda: lib.gitcap_student_score(h, p(ids), L + 1, B, L + 1, None, -1, None, 0, p(scores), None, None, None, None),
        "gitcap_student_attention": lambda: lib.gitcap_student_attention(h, p(ids), L + 1, B, L, -1, None, p(fm), m.cfg.mem_tokens, None),
    }
    for name, call in calls.items():
        assert lib.gitcap_student_attach_search(h, ctypes.byref(opt)) == 0
        rc = call()
        assert rc in (ERR_ARG, ERR_STATE), (name, rc)
        assert b"gitcap_student_attach_search" in lib.gitcap_student_last_error(h), name
    # consumed: the same greedy call now runs, and a plain beam search is the plain one
    assert lib.gitcap_student_attach_search(h, ctypes.byref(opt)) == 0
    assert calls["gitcap_student_greedy"]() != 0
    assert calls["gitcap_student_greedy"]() == 0
    torch.cuda.synchronize()
    # what the attach itself and the consuming call refuse
    bad = _lib.CStudentSearchOptions(0, 1.0, 0, 1.0, scores.data_ptr(), None)
    assert lib.gitcap_student_attach_search(h, ctypes.byref(bad)) == ERR_ARG
    out = torch.zeros((1, 4, S.MAX_LEN), dtype=torch.int64).cuda()
    for n, pn, k in ((4, 0, 3), (1, 3, 2), (1, 0, 1), (1, 4, 5)):
        o = _lib.CStudentSearchOptions(n, 1.0, pn, 1.0, scores.data_ptr(), None)
        assert lib.gitcap_student_attach_search(h, ctypes.byref(o)) == 0
        assert lib.gitcap_student_beam_search(h, p(mem), 1, k, S.MAX_LEN, p(out), None) == ERR_ARG, (n, pn, k)


def test_a_handle_that_never_attaches_keeps_the_parents_workspace():
    from gitcap.student import StudentCaptioner
    cfg, w = S.tiny_weights()
    m = StudentCaptioner(cfg=cfg, weights=w, device="cuda:0", max_batch=S.CLIPS * S.K, max_text_len=S.MAX_LEN)
    src = [t.cuda() for t in S.clip_memories(cfg, {})]

    def ws():
        b = ctypes.c_int64(0)
        m._call("gitcap_student_workspace_bytes", ctypes.byref(b))
        return b.value

    m.beam_search(src, max_len=S.MAX_LEN, k=S.K)
    plain = ws()
    # the parent's beam workspace, buffer by buffer (csrc/student.hip: beam_workspace without search options)
    R, F, D, V, T, L = S.CLIPS * S.K, cfg.mem_tokens, cfg.d_model, cfg.vocab_length, S.MAX_LEN + 1, cfg.num_decoder_layers
    nch = (V + 2047) // 2048
    beam = 4 * R * F * D + 4 * R * 4 + 2 * 8 * R * (T + 1) + 4 * R * V + 2 * L * R * T * 3 * D + R * nch * (8 + 16 * 8)
    fresh = StudentCaptioner(cfg=cfg, weights=w, device="cuda:0", max_batch=S.CLIPS * S.K, max_text_len=S.MAX_LEN)
    b0 = ctypes.c_int64(0)
    fresh._call("gitcap_student_workspace_bytes", ctypes.byref(b0))
    assert plain - b0.value == beam
    m.beam_search(src, max_len=S.MAX_LEN, k=S.K, eos=True)
    grown = ws()
    assert grown - plain == R * (8 + 4 + 4 + 4) + 8 * R * T + 2 * 4 * R * 16          # words, done, hyp_len, hyp_score; hyp_ids; 16 candidate slots
    m.beam_search(src, max_len=S.MAX_LEN, k=S.K, eos=True, num_keep_best=3)
    assert ws() == grown
