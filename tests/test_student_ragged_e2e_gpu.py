"""Clips of different length on the student, end to end (gitcap_student_attach_frame_counts; StudentCaptioner's list / frame_counts
inputs) and captions of a live window that is not full yet (caption_stream(partial=True)).  The contract is exact: every clip of a
ragged call holds, bit for bit, what the clip yields alone on a second model built from the same weights with mem_tokens = F_b.  The
one comparison with a tolerance is forward_decoder against the bf16-emulating oracle, under the bound rule of tests/test_student.py
(restated in tests/test_student_ragged.py: e2e_bound)."""
import dataclasses

import pytest
import torch

import gitcap
from gitcap import _lib
from gitcap.student import StudentCaptioner
from gitcap.student_config import student_synthetic_weights, student_tiny
from gpu_support import camera, captioner_cls, make_student, make_student_native, same_bits  # noqa: F401
from test_student_ragged import LENS, e2e_bound, ragged_case

pytestmark = pytest.mark.gpu

L, K = 6, 2             # max_len, beams
KW = dict(max_batch=8, max_text_len=8, stop="never")


@pytest.fixture(scope="module")
def case():
    """The ragged model, one model per clip length (the same weights, mem_tokens = F_b), the clips as memory tokens, and what the
    ragged greedy call returns on them."""
    assert torch.cuda.is_available()
    cfg, w, y, mem = ragged_case()
    st = make_student("tiny", **KW)
    alone = {n: StudentCaptioner(cfg=dataclasses.replace(cfg, mem_tokens=n), weights=w, device="cuda:0", **KW) for n in set(LENS)}
    clips = [mem[b, :n].cuda() for b, n in enumerate(LENS)]
    out = st.greedy_decode(clips, max_len=L, return_logprobs=True, top_logprobs=3, return_attention=True)
    return dict(cfg=cfg, w=w, y=y.cuda(), mem=mem, st=st, alone=alone, clips=clips, out=out)


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b) if a.dtype == torch.int64 else same_bits(a.contiguous(), b.contiguous()), what


def test_greedy_each_clip_is_the_clip_alone(case):
    ids, lp, top_ids, top_lp, att = case["out"]
    F = case["cfg"].mem_tokens
    assert ids.shape == (3, L + 1) and att.shape == (3, L, F)
    for b, n in enumerate(LENS):
        one = case["alone"][n].greedy_decode(case["clips"][b][None], max_len=L, return_logprobs=True, top_logprobs=3, return_attention=True)
        for got, ref, what in zip((ids, lp, top_ids, top_lp), one, ("ids", "logprobs", "top_ids", "top_logprobs")):
            _eq(got[b:b + 1], ref, f"{what} of clip {b}")
        _eq(att[b:b + 1, :, :n], one[4], f"attention of clip {b}")
        assert bool((att[b, :, n:] == 0).all())
        assert float((att[b].sum(-1) - 1).abs().max()) < 1e-5


def test_permuted_clips_permute_the_results(case):
    perm = [2, 0, 1]
    got = case["st"].greedy_decode([case["clips"][p] for p in perm], max_len=L, return_logprobs=True, top_logprobs=3, return_attention=True)
    for g, ref in zip(got, case["out"]):
        _eq(g, ref[perm], "permuted")
    # the padded form with frame_counts is the list form
    pad = case["st"].greedy_decode(case["mem"].cuda(), max_len=L, return_logprobs=True, frame_counts=LENS)
    _eq(pad[0], case["out"][0], "padded ids")
    _eq(pad[1], case["out"][1], "padded logprobs")


def test_full_length_clips_are_the_dense_call(case):
    st, mem = case["st"], case["mem"].cuda()
    dense = st.greedy_decode(mem, max_len=L, return_logprobs=True)
    as_list = st.greedy_decode([mem[b] for b in range(3)], max_len=L, return_logprobs=True)
    _eq(as_list[0], dense[0], "ids")
    _eq(as_list[1], dense[1], "logprobs")
    _eq(st.beam_search([mem[b] for b in range(3)], max_len=L, k=K), st.beam_search(mem, max_len=L, k=K), "beam")


def test_score_attention_beam_draft_each_clip_is_the_clip_alone(case):
    st, clips, y = case["st"], case["clips"], case["y"]
    sc = st.score(clips, y, until_sep=False)
    cand = torch.stack([y, y.flip(0)], 1)                               # two candidates per clip
    sc2 = st.score(clips, cand, until_sep=False)
    at = st.attention(clips, y, until_sep=False)["frame_attention"]
    beam = st.beam_search(clips, max_len=L, k=K)
    ids, lp = case["out"][:2]
    drafted = st.greedy_decode(clips, max_len=L, draft=ids, return_logprobs=True)
    assert st.last_accepted == L
    _eq(drafted[0], ids, "draft ids")
    _eq(drafted[1], lp, "draft logprobs")
    wrong = ids.clone()
    wrong[:, 3] = (wrong[:, 3] + 1) % case["cfg"].vocab_length
    _eq(st.greedy_decode(clips, max_len=L, draft=wrong), ids, "ids behind a wrong draft")
    assert st.last_accepted == 2
    for b, n in enumerate(LENS):
        m1, c1 = case["alone"][n], clips[b][None]
        ref = m1.score(c1, y[b:b + 1], until_sep=False)
        for f in ("token_logprobs", "sum", "count"):
            _eq(sc[f][b:b + 1], ref[f], f"score {f} of clip {b}")
        ref2 = m1.score(c1, cand[b:b + 1], until_sep=False)
        _eq(sc2["sum"][b:b + 1], ref2["sum"], f"candidate sums of clip {b}")
        _eq(at[b:b + 1, :, :n], m1.attention(c1, y[b:b + 1], until_sep=False)["frame_attention"], f"attention of clip {b}")
        assert bool((at[b, :, n:] == 0).all())
        _eq(beam[b:b + 1], m1.beam_search(c1, max_len=L, k=K), f"beam of clip {b}")


def test_forward_decoder_against_the_clip_alone_and_the_oracle(case):
    st, clips, y = case["st"], case["clips"], case["y"]
    got = st.forward_decoder(y, clips)
    for b, n in enumerate(LENS):
        _eq(got[b:b + 1], case["alone"][n].forward_decoder(y[b:b + 1], clips[b][None]), f"logits of clip {b}")
        emu, bound = e2e_bound(case["cfg"], case["w"], y[b:b + 1].cpu(), case["mem"][b:b + 1, :n])
        err = (got[b:b + 1].cpu() - emu).abs().max().item()
        print(f"clip {b} ({n} frames): max |device - emulated oracle| = {err:.6f}, bound {bound:.4f}")
        assert err < bound


@pytest.fixture(scope="module")
def native():
    return make_student_native("tiny", **KW)


def test_caption_videos_is_greedy_on_the_sampled_frames(native):
    s = native.image_encoder.cfg.img_size
    videos = [camera((n, s + 6, s + 10, 3), 70 + n) for n in (3, 9, 14)]
    ids, sel = gitcap.caption_videos(native, videos, "uniform", max_len=L, retention_rate=0.5)
    assert len(set(sel.counts)) > 1 and max(sel.counts) <= native.cfg.mem_tokens
    _eq(ids, native.greedy_decode(sel.frames(), max_len=L), "caption_videos")
    for b, fr in enumerate(sel.frames()):                               # and a clip of frames is the clip alone (camera frames, packed encode)
        _eq(ids[b:b + 1], native.greedy_decode([fr], max_len=L), f"video {b}")


def test_stream_partial_captions_from_the_first_frame(native):
    s, F = native.image_encoder.cfg.img_size, native.cfg.mem_tokens
    frames = camera((F + 2, s, s, 3), 81)
    plain = native.caption_stream(batch=1, hop=1, max_len=L, logprobs=True)
    want = [plain.push(frames[i][None]) for i in range(F + 2)]
    want_lp = plain.last_logprobs
    assert all(w is None for w in want[:F - 1]) and want[F - 1] is not None and plain.last_frames == F
    part = native.caption_stream(batch=1, hop=1, max_len=L, logprobs=True, top_logprobs=2, partial=True)
    for i in range(F + 2):
        got = part.push(frames[i][None])
        n = min(i + 1, F)
        assert got is not None and part.last_frames == n
        ref = native.greedy_decode([frames[i + 1 - n:i + 1]], max_len=L, return_logprobs=True, top_logprobs=2)
        _eq(got, ref[0], f"caption after {i + 1} pushes")
        _eq(part.last_logprobs, ref[1], f"logprobs after {i + 1} pushes")
        _eq(part.last_top_ids, ref[2], f"top ids after {i + 1} pushes")
        if i >= F - 1:
            _eq(got, want[i], f"full window, push {i + 1}")
    _eq(part.last_logprobs, want_lp, "the last full window's logprobs")
    part.reset()
    assert part.push(frames[0][None]) is not None and part.last_frames == 1
    for bad in (dict(carry=True), dict(beams=2)):
        with pytest.raises(ValueError, match="partial=True is for greedy streams without carry"):
            native.caption_stream(batch=1, max_len=L, partial=True, **bad)


def test_distill_report_takes_ragged_clips(captioner_cls):
    from gitcap.config import git_tiny
    from gitcap.weights import synthetic_weights
    T = 5
    cfg = git_tiny(2)
    scfg = dataclasses.replace(student_tiny(), vocab_length=cfg.vocab_size)
    t = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=3, max_frames=2, max_text_len=T + 1, max_beams=2, stop="never")
    s = StudentCaptioner(cfg=scfg, weights=student_synthetic_weights(scfg, 0), device="cuda:0", max_batch=6, max_text_len=T + 1, stop="never")
    g = torch.Generator().manual_seed(3)
    lens = [1, 2, 1]
    frames = [torch.randn(n, 3, cfg.image_size, cfg.image_size, generator=g) for n in lens]
    smem = [2.0 * torch.randn(n, scfg.d_model, generator=g) for n in lens]
    y = torch.randint(1, cfg.vocab_size, (3, T), generator=g)
    y[:, 0] = cfg.cls_token_id
    got = gitcap.distill_report(t, s, frames, y, student_x=smem)
    ref = s.score(smem, y, until_sep=False)
    _eq(got["student_logprobs"], ref["token_logprobs"], "student columns")
    tref = t.score(frames, y, until_sep=False)
    _eq(got["teacher_logprobs"], tref["token_logprobs"], "teacher columns")
    assert bool(torch.isfinite(got["kl"]).all()) and float(got["kl"].min()) > -1e-5


def test_refusals_carry_their_messages(case):
    st, clips, mem = case["st"], case["clips"], case["mem"].cuda()
    F, D = case["cfg"].mem_tokens, case["cfg"].d_model
    with pytest.raises(ValueError, match=r"clip 1 has 0 frames, outside \[1, 6\]"):
        st.greedy_decode(mem, max_len=L, frame_counts=[1, 0, 6])
    with pytest.raises(ValueError, match=r"clip 0 has 7 frames, outside \[1, 6\]"):
        st.greedy_decode([torch.zeros(F + 1, D)], max_len=L)
    with pytest.raises(ValueError, match="frame_counts holds 2 counts for a batch of 3 clips"):
        st.greedy_decode(mem, max_len=L, frame_counts=[1, 2])
    with pytest.raises(ValueError, match="frame_counts disagrees with the clips' own frame counts"):
        st.greedy_decode(clips, max_len=L, frame_counts=[1, 4, 5])
    import ctypes
    c32 = lambda v: (ctypes.c_int32 * len(v))(*v)
    for bad, msg in (([1, 0, 6], r"clip 1 has 0 frames, outside \[1, 6\]"), ([F + 1], r"clip 0 has 7 frames, outside \[1, 6\]")):
        with pytest.raises(_lib.GitcapError, match=msg):
            st._call("gitcap_student_attach_frame_counts", c32(bad), len(bad))
    with pytest.raises(_lib.GitcapError, match="B outside"):
        st._call("gitcap_student_attach_frame_counts", c32([1] * 9), 9)
    # a sum that disagrees with the buffer: the counts say 3 clips, the call 2
    packed = torch.cat(clips, 0).contiguous()
    st._call("gitcap_student_attach_frame_counts", c32(LENS), 3)
    with pytest.raises(_lib.GitcapError, match="B = 2, but frame counts of 3 clips are attached"):
        st._call("gitcap_student_set_memory", _lib.ptr(packed), 2, st._stream())
    # the window family does not take counts, and the refusal consumes them
    for name, args in (("gitcap_student_window_reset", (1,)), ("gitcap_student_window_push", (_lib.ptr(packed), 1, 1, st._stream())),
                       ("gitcap_student_window_greedy", (L, 0, _lib.ptr(packed), None, st._stream())),
                       ("gitcap_student_window_greedy_partial", (L, 0, _lib.ptr(packed), None, None, st._stream())),
                       ("gitcap_student_window_beam_search", (K, L, _lib.ptr(packed), st._stream()))):
        st._call("gitcap_student_attach_frame_counts", c32(LENS), 3)
        with pytest.raises(_lib.GitcapError, match=r"per-clip frame counts are attached \(gitcap_student_attach_frame_counts\), which this call does not take"):
            st._call(name, *args)
    _eq(st.greedy_decode(mem, max_len=L), st.greedy_decode([mem[b] for b in range(3)], max_len=L), "nothing stayed attached")
    st._call("gitcap_student_window_reset", 1)
    with pytest.raises(_lib.GitcapError, match="no token pushed since the reset"):
        st._call("gitcap_student_window_greedy_partial", L, 0, _lib.ptr(packed), None, None, st._stream())
    st._call("gitcap_student_window_reset", 0)
