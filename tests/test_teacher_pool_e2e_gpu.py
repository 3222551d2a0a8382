"""The teacher's stream pool end to end (GitCaptioner.stream_pool; include/gitcap.h: gitcap_pool_*) on the tiny GIT: every caption
a camera gets from the pool is bit for bit the plain call on a one-clip list holding that camera's current frames -- ids,
log-probabilities, search predictions and scores --, whichever other cameras share the call."""
import ctypes

import pytest
import torch

from gitcap import _lib
from gitcap.config import git_tiny
from gitcap.weights import synthetic_weights
from oracle.git_oracle import make_frames
from gpu_support import camera, captioner_cls, ptr, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

F, L = 4, 6
ERR_ARG, ERR_STATE = -1, -2
LENS = [1, 2, F, F + 2]                                                 # frames pushed per camera; the last one wrapped its ring


@pytest.fixture(scope="module")
def model(captioner_cls):
    cfg = git_tiny(F)
    return captioner_cls(cfg, synthetic_weights(cfg, 5), max_batch=4, max_frames=F, max_text_len=8, max_beams=2, stop="never")


@pytest.fixture(scope="module")
def cams(model):
    """four cameras' frames [n, 3, S, S] on the device"""
    return [make_frames(1, n, model.cfg.image_size, 300 + c)[0].cuda() for c, n in enumerate(LENS)]


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a, b) if a.dtype == torch.int64 else same_bits(a.contiguous(), b.contiguous()), what


def _fill(pool, cams):
    """Push the cameras' frames interleaved, one frame per camera and push while it has one left."""
    out = {}
    for k in range(max(c.shape[0] for c in cams)):
        live = [c for c in range(len(cams)) if k < cams[c].shape[0]]
        out = pool.push(torch.stack([cams[c][k] for c in live], 0), live)
    return out


def _cut(ids, sep):
    hits = (ids[1:] == sep).nonzero()
    return int(hits[0]) + 1 if hits.numel() else ids.shape[0] - 1


@pytest.mark.parametrize("stop", ["never", "all_sep"])
def test_four_cameras_at_different_fill_levels_in_one_call(model, cams, stop):
    m = model
    pool = m.stream_pool(4, frames=F, hop=1, max_len=L, stop=stop, logprobs=True, top_logprobs=2)
    _fill(pool, cams)
    assert pool.counts() == [1, 2, F, F]
    ref = {}
    for c in range(4):
        ids, lp, ti, tl = m.greedy_decode([cams[c][-F:]], max_len=L, stop=stop, return_logprobs=True, top_logprobs=2)
        ref[c] = (ids[0], lp[0], ti[0], tl[0])
    for subset in ([0, 1, 2, 3], [3, 0], [2], [1, 3, 2], [3]):           # the same whichever subset of the others shares the call
        out = pool.caption(subset)
        assert list(out) == subset
        for c in subset:
            what = f"camera {c} in {subset} under {stop}"
            _eq(out[c], ref[c][0], "ids of " + what)
            if stop == "all_sep":
                assert out[c].shape[0] - 1 == _cut(out[c], m.cfg.sep_token_id), what
            _eq(pool.last_logprobs[c], ref[c][1], "logprobs of " + what)
            _eq(pool.last_top_ids[c], ref[c][2], "top ids of " + what)
            _eq(pool.last_top_logprobs[c], ref[c][3], "top logprobs of " + what)
            assert pool.last_frames[c] == min(LENS[c], F), what


def test_camera_frames_on_the_host(model):
    m = model
    cam = camera((3, 48, 64, 3), 310)
    pool = m.stream_pool(2, frames=F, max_len=L)
    out = pool.push(cam, [1, 1, 0])
    assert sorted(out) == [0, 1] and out[0].device.type == "cpu"
    _eq(out[1], m.greedy_decode([cam[:2]], max_len=L)[0], "two camera frames")
    _eq(out[0], m.greedy_decode([cam[2:]], max_len=L)[0], "one camera frame")


def test_equal_counts_are_the_lockstep_window_and_both_live_side_by_side(model):
    m = model
    fr = make_frames(3, F + 2, m.cfg.image_size, 320).cuda()
    cs = m.caption_stream(batch=3, window=F, hop=1, max_len=L)
    pool = m.stream_pool(3, frames=F, hop=1, max_len=L)                 # opening a pool leaves the window alone
    for k in range(F + 2):
        want = cs.push(fr[:, k])
        out = pool.push(fr[:, k].contiguous(), [0, 1, 2])
        assert sorted(out) == [0, 1, 2]
        got = torch.stack([out[c] for c in range(3)], 0)
        if k + 1 >= F:
            _eq(got, want, f"the full window after {k + 1} frames")
        else:                                                           # equal counts below F: the dense call on those frames
            assert want is None
            _eq(got, m.greedy_decode(fr[:, :k + 1], max_len=L), f"{k + 1} frames each")
    cs2 = m.caption_stream(batch=1, window=2, hop=2, max_len=L)         # and a new window leaves the pool alone
    assert pool.counts() == [F, F, F] and cs2.push(fr[:1, 0]) is None
    with pytest.raises(_lib.GitcapError, match="invalidated"):
        cs.push(fr[:, 0])


def test_more_due_streams_than_max_batch(captioner_cls, cams):
    cfg = git_tiny(F)
    m = captioner_cls(cfg, synthetic_weights(cfg, 5), max_batch=2, max_frames=F, max_text_len=8, stop="never")
    pool = m.stream_pool(4, frames=F, max_len=L, logprobs=True)
    for k in range(F + 2):                                              # at most max_batch * F frames per push: one camera at a time
        for c in range(4):
            if k < LENS[c]:
                out = pool.push(cams[c][k][None], [c])
                assert list(out) == [c]
    out = pool.caption([3, 1, 0, 2])                                    # two chunks of two
    for c in range(4):
        ids, lp = m.greedy_decode([cams[c][-F:]], max_len=L, return_logprobs=True)
        _eq(out[c], ids[0], f"camera {c}")
        _eq(pool.last_logprobs[c], lp[0], f"logprobs of camera {c}")


def test_drop_empties_one_stream_only(model, cams):
    m = model
    pool = m.stream_pool(4, frames=F, max_len=L)
    before = _fill(pool, cams)
    pool.drop(2)
    assert pool.counts() == [1, 2, 0, F] and 2 not in pool.last_frames
    with pytest.raises(_lib.GitcapError, match="stream 2 holds no frame"):
        pool.caption([0, 2])
    _eq(pool.caption([3])[3], before[3], "camera 3 behind the drop of camera 2")
    out = pool.push(cams[2][:1], [2])                                   # it starts again from an empty window
    _eq(out[2], m.greedy_decode([cams[2][:1]], max_len=L)[0], "camera 2 after the drop")


def test_beam_search_equals_infer_on_the_camera_s_frames(model, cams):
    m = model
    pool = m.stream_pool(4, frames=F, max_len=L, beam_size=2)
    _fill(pool, cams)
    out = pool.caption([2, 0, 3, 1])
    for c in range(4):
        want = m.infer([cams[c][-F:]], beam_size=2, max_steps=L)
        _eq(out[c], want["predictions"][0], f"predictions of camera {c}")
        _eq(pool.last_scores[c].reshape(1), want["logprobs"][0].reshape(1), f"score of camera {c}")


def test_constraints_and_a_prompt(model, cams):
    m = model
    rules = dict(no_repeat_ngram_size=1, min_length=4, suppress_tokens=[3, 5, 11])
    pool = m.stream_pool(4, frames=F, max_len=L, logprobs=True, **rules)
    _fill(pool, cams)
    out = pool.caption([0, 1, 2, 3])
    for c in range(4):
        ids, lp = m.greedy_decode([cams[c][-F:]], max_len=L, return_logprobs=True, **rules)
        _eq(out[c], ids[0], f"constrained camera {c}")
        _eq(pool.last_logprobs[c], lp[0], f"constrained logprobs of camera {c}")
    prompt = torch.tensor([17, 4, 29])
    pool = m.stream_pool(4, frames=F, max_len=L, prompt=prompt)
    _fill(pool, cams)
    out = pool.caption([3, 1, 0, 2])
    for c in range(4):
        _eq(out[c], m.greedy_decode([cams[c][-F:]], max_len=L, prompt=[prompt])[0], f"prompted camera {c}")


def test_refusals(model, cams):
    m = model
    lib, h, st = m._lib, m._handle, m._stream()
    pool = m.stream_pool(3, frames=F, max_len=L)
    ids = torch.empty((3, L + 1), dtype=torch.int64, device="cuda")
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    assert lib.gitcap_pool_greedy(h, i32(0), 1, L, 0, ptr(ids), None, None, st) == ERR_STATE          # an empty stream
    pool.push(cams[1], [0, 1])
    # attached frame counts: refused with the window calls' message, and consumed
    m._attach_counts([1, 1])
    with pytest.raises(_lib.GitcapError, match="window: per-clip frame counts are attached"):
        pool.caption([0, 1])
    want = pool.caption([0, 1])
    m._attach_counts([1])
    assert lib.gitcap_pool_push(h, ptr(cams[0]), i32(2), 1, st) == ERR_ARG and b"frame counts" in lib.gitcap_last_error(h)
    assert pool.counts() == [1, 1, 0]
    # an empty list, a repeated, an unknown or an empty stream: nothing is launched
    for sid, B, rc in ((i32(0), 0, ERR_ARG), (i32(0, 0), 2, ERR_ARG), (i32(0, 3), 2, ERR_ARG), (i32(1, -1), 2, ERR_ARG), (i32(0, 2), 2, ERR_STATE),
                       (i32(0, 1, 2, 0, 1), 5, ERR_ARG)):
        ids.fill_(-7)
        assert lib.gitcap_pool_greedy(h, sid, B, L, 0, ptr(ids), None, None, st) == rc, list(sid)
        torch.cuda.synchronize()
        assert bool((ids == -7).all())
    with pytest.raises(ValueError, match="named twice"):
        pool.caption([1, 1])
    with pytest.raises(_lib.GitcapError, match="stream 2 holds no frame"):
        pool.caption([2])
    # more than F frames to one stream in one push, a stream outside the pool, too many frames: a refused push changes nothing
    five = make_frames(1, F + 1, m.cfg.image_size, 330)[0].cuda()
    with pytest.raises(ValueError, match=f"at most {F} frames per stream"):
        pool.push(five, [0] * (F + 1))
    assert lib.gitcap_pool_push(h, ptr(five), i32(*[0] * (F + 1)), F + 1, st) == ERR_ARG and b"more than F" in lib.gitcap_last_error(h)
    assert lib.gitcap_pool_push(h, ptr(five), i32(0, 3), 2, st) == ERR_ARG
    assert lib.gitcap_pool_push(h, ptr(five), i32(0), 0, st) == ERR_ARG
    assert lib.gitcap_pool_push(h, ptr(five), i32(0), 4 * F + 1, st) == ERR_ARG
    assert lib.gitcap_pool_push(h, ctypes.c_void_p(five.data_ptr() + 4), i32(0), 1, st) == ERR_ARG
    assert lib.gitcap_pool_push(h, None, i32(0), 1, st) == ERR_ARG
    assert pool.counts() == [1, 1, 0]
    got = pool.caption([0, 1])
    for c in (0, 1):
        _eq(got[c], want[c], f"camera {c} behind the refused calls")
    assert lib.gitcap_pool_reset(h, 4097, F) == ERR_ARG and lib.gitcap_pool_reset(h, 2, F + 1) == ERR_ARG and lib.gitcap_pool_reset(h, 2, 0) == ERR_ARG
    # a second pool invalidates the first object; a released pool refuses its calls
    w_with = m.workspace_bytes()
    pool2 = m.stream_pool(1, frames=2, max_len=L)
    with pytest.raises(_lib.GitcapError, match="TeacherStreamPool was invalidated"):
        pool.counts()
    assert pool2.counts() == [0]
    assert lib.gitcap_pool_reset(h, 0, 0) == 0 and m.workspace_bytes() < w_with
    assert lib.gitcap_pool_greedy(h, i32(0), 1, L, 0, ptr(ids), None, None, st) == ERR_STATE
    assert lib.gitcap_pool_push(h, ptr(five), i32(0), 1, st) == ERR_STATE
    torch.cuda.synchronize()
