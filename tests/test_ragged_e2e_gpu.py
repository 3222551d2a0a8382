"""Ragged batches end to end (frame_counts=; include/gitcap.h: gitcap_attach_frame_counts): a clip inside a packed batch of clips
that differ in length must be BIT FOR BIT the clip captioned alone -- ids, log-probabilities, scores, visual rows -- through every
input form and entry point.  The clip alone is the path the parity tests hold to the HF goldens.

git_tiny(num_frames=8) has N = 17 image rows per frame, so the counts below put clips on both sides of the 64- and 128-key edges
of the two attention kernels (17, 34, 51, 68, 136 rows)."""
import ctypes

import pytest
import torch

from gpu_support import camera, captioner_cls, mid768, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

COUNTS = [1, 8, 3, 4, 8, 2]
MAX_LEN = 8


def _clips(cfg, counts, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 3, cfg.image_size, cfg.image_size, generator=g) for n in counts]


def _padded(clips):
    x = torch.full((len(clips), max(c.shape[0] for c in clips)) + tuple(clips[0].shape[1:]), float("nan"))
    for b, c in enumerate(clips):
        x[b, :c.shape[0]] = c
    return x


def _make(captioner_cls, cfg, **kw):
    from gitcap.weights import synthetic_weights
    kw = dict(dict(max_batch=len(COUNTS), max_frames=8, max_text_len=12, max_beams=3), **kw)
    return captioner_cls(cfg, synthetic_weights(cfg, seed=0), device="cuda:0", **kw)


@pytest.fixture(scope="module")
def tiny(captioner_cls):
    from gitcap.config import git_tiny
    cfg = git_tiny(num_frames=8)
    m = _make(captioner_cls, cfg)
    clips = [c.cuda() for c in _clips(cfg, COUNTS, 11)]
    alone = [m.greedy_decode(c[None], max_len=MAX_LEN, stop="never", return_logprobs=True) for c in clips]
    return m, cfg, clips, alone


def _same_as_alone(out, alone):
    ids, lp = out
    for b, (ai, al) in enumerate(alone):
        assert torch.equal(ids[b:b + 1].to(ai.device), ai), b
        assert same_bits(lp[b:b + 1].to(al.device).contiguous(), al.contiguous()), b


def test_greedy_padded_and_list_forms_equal_each_clip_alone(tiny):
    m, _, clips, alone = tiny
    _same_as_alone(m.greedy_decode(_padded(clips).cuda(), max_len=MAX_LEN, stop="never", return_logprobs=True, frame_counts=COUNTS), alone)
    _same_as_alone(m.greedy_decode(clips, max_len=MAX_LEN, stop="never", return_logprobs=True), alone)
    # host clips: packed once through the staging ring; results come back on the host
    ids, lp = m.greedy_decode([c.cpu() for c in clips], max_len=MAX_LEN, stop="never", return_logprobs=True)
    assert ids.device.type == "cpu"
    _same_as_alone((ids, lp), alone)
    _same_as_alone(m.greedy_decode(_padded(clips), max_len=MAX_LEN, stop="never", return_logprobs=True,
                                   frame_counts=torch.tensor(COUNTS)), alone)


def test_greedy_async_equals_each_clip_alone(tiny):
    m, _, clips, alone = tiny
    futs = [m.greedy_decode_async(clips, max_len=MAX_LEN, stop="never"),
            m.greedy_decode_async(_padded(clips), max_len=MAX_LEN, stop="never", frame_counts=COUNTS)]      # host-fed
    for f in futs:
        ids = f.result()
        for b, (ai, _) in enumerate(alone):
            assert torch.equal(ids[b:b + 1].to(ai.device), ai), b


def test_greedy_raw_camera_frames_equal_each_clip_alone(tiny):
    m = tiny[0]
    counts = [2, 1, 3]
    raw = [camera((n, 40, 48, 3), 50 + n) for n in counts]
    alone = [m.greedy_decode(r[None], max_len=MAX_LEN, stop="never", return_logprobs=True) for r in raw]
    _same_as_alone(m.greedy_decode(raw, max_len=MAX_LEN, stop="never", return_logprobs=True), alone)
    ids = m.greedy_decode_async([r.cuda() for r in raw], max_len=MAX_LEN, stop="never").result()
    for b, (ai, _) in enumerate(alone):
        assert torch.equal(ids[b:b + 1].cpu(), ai.cpu()), b


@pytest.mark.parametrize("beams", [1, 3])
def test_infer_equals_each_clip_alone(tiny, beams):
    m, _, clips, _ = tiny
    kw = dict(beam_size=beams, max_steps=MAX_LEN)
    got = m.infer(clips, **kw)
    fut = m.infer_async(_padded(clips).cuda(), frame_counts=COUNTS, visual_features=True, **kw).result()
    for b, c in enumerate(clips):
        ref = m.infer(c[None], **kw)
        for r in (got, fut):
            assert torch.equal(r["predictions"][b:b + 1], ref["predictions"]), b
            assert same_bits(r["logprobs"][b:b + 1].contiguous(), ref["logprobs"].contiguous()), b
    assert fut["visual_features_valid"].sum(1).tolist() == [17 * n for n in COUNTS]


def test_score_equals_each_clip_alone(tiny):
    m, _, clips, alone = tiny
    y = torch.cat([a[0] for a in alone], 0)
    got = m.score(clips, y)
    for b, c in enumerate(clips):
        ref = m.score(c[None], y[b:b + 1])
        assert same_bits(got["token_logprobs"][b:b + 1].contiguous(), ref["token_logprobs"].contiguous()), b
        assert same_bits(got["sum"][b:b + 1].contiguous(), ref["sum"].contiguous()) and int(got["count"][b]) == int(ref["count"][0])
    logits = m.forward(clips, y)
    for b, c in enumerate(clips):
        assert same_bits(logits[b:b + 1].contiguous(), m.forward(c[None], y[b:b + 1]).contiguous()), b


def test_forward_image_enc_gives_the_padded_pair(tiny):
    m, cfg, clips, _ = tiny
    N = cfg.tokens_per_frame
    vis, valid = m.forward_image_enc(_padded(clips).cuda(), frame_counts=COUNTS)
    assert vis.shape == (len(COUNTS), 8 * N, cfg.enc_width) and valid.shape == vis.shape[:2] and valid.dtype == torch.bool
    for b, c in enumerate(clips):
        ref = m.forward_image_enc(c[None])[1][0]
        n = c.shape[0] * N
        assert same_bits(vis[b, :n].contiguous(), ref.contiguous()), b
        assert bool((vis[b, n:] == 0).all()) and bool(valid[b, :n].all()) and not bool(valid[b, n:].any())


def test_ragged_prompt_and_ngram_ban(tiny):
    m, _, clips, _ = tiny
    prompt = [torch.tensor([5, 9]), torch.tensor([], dtype=torch.int64), torch.tensor([7]), torch.tensor([3, 4, 6]),
              torch.tensor([], dtype=torch.int64), torch.tensor([8])]
    for kw, rows in ((dict(prompt=prompt), True), (dict(no_repeat_ngram_size=2), False)):
        ids, lp = m.greedy_decode(clips, max_len=MAX_LEN, stop="never", return_logprobs=True, **kw)
        for b, c in enumerate(clips):
            one = dict(kw, prompt=[prompt[b]]) if rows else kw
            ri, rl = m.greedy_decode(c[None], max_len=MAX_LEN, stop="never", return_logprobs=True, **one)
            assert torch.equal(ids[b:b + 1], ri) and same_bits(lp[b:b + 1].contiguous(), rl.contiguous()), (b, kw.keys())


def test_e4m3_v_cache(captioner_cls):
    from gitcap.config import git_tiny
    cfg = git_tiny(num_frames=8)
    m = _make(captioner_cls, cfg, kv_cache="v_e4m3")
    clips = [c.cuda() for c in _clips(cfg, COUNTS, 12)]
    ids, lp = m.greedy_decode(clips, max_len=MAX_LEN, stop="never", return_logprobs=True)
    _same_as_alone((ids, lp), [m.greedy_decode(c[None], max_len=MAX_LEN, stop="never", return_logprobs=True) for c in clips])
    r3 = m.infer(clips, beam_size=3, max_steps=MAX_LEN)
    for b, c in enumerate(clips):
        ref = m.infer(c[None], beam_size=3, max_steps=MAX_LEN)
        assert torch.equal(r3["predictions"][b:b + 1], ref["predictions"]) and same_bits(r3["logprobs"][b:b + 1].contiguous(), ref["logprobs"].contiguous())


def test_mid768(captioner_cls):
    cfg = mid768()
    counts = [1, 3, 2, 3]
    m = _make(captioner_cls, cfg, max_batch=4, max_frames=3)
    clips = [c.cuda() for c in _clips(cfg, counts, 13)]
    out = m.greedy_decode(_padded(clips).cuda(), max_len=6, stop="never", return_logprobs=True, frame_counts=counts)
    _same_as_alone(out, [m.greedy_decode(c[None], max_len=6, stop="never", return_logprobs=True) for c in clips])


def test_equal_counts_take_the_dense_path(tiny):
    m, cfg, _, _ = tiny
    x = torch.stack(_clips(cfg, [3, 3, 3], 14)).cuda()
    ref = m.greedy_decode(x, max_len=MAX_LEN, stop="never", return_logprobs=True)
    for got in (m.greedy_decode(x, max_len=MAX_LEN, stop="never", return_logprobs=True, frame_counts=[3, 3, 3]),
                m.greedy_decode(list(x), max_len=MAX_LEN, stop="never", return_logprobs=True)):
        assert torch.equal(got[0], ref[0]) and same_bits(got[1].contiguous(), ref[1].contiguous())
    # the library's own equal-count branch: counts attached to a dense call
    ids = torch.empty((3, MAX_LEN + 1), dtype=torch.int64, device="cuda")
    m._attach_counts([3, 3, 3])
    m._call("gitcap_greedy", ctypes.c_void_p(x.data_ptr()), 3, 3, MAX_LEN, 0, ctypes.c_void_p(ids.data_ptr()), None, m._stream())
    torch.cuda.synchronize()
    assert torch.equal(ids, ref[0])


def test_reversing_the_clips_reverses_the_results(tiny):
    m, _, clips, alone = tiny
    _same_as_alone(m.greedy_decode(clips[::-1], max_len=MAX_LEN, stop="never", return_logprobs=True), alone[::-1])


def test_refusals_leave_the_handle_intact(tiny):
    from gitcap._lib import GitcapError
    m, cfg, clips, alone = tiny
    arr = lambda *c: (ctypes.c_int32 * len(c))(*c)
    for bad in ((1, 0, 2), (1, 9), (1, -3)):                               # a count of 0 / above the limit (num_frames = 8)
        with pytest.raises(GitcapError, match="frames, outside"):
            m._call("gitcap_attach_frame_counts", arr(*bad), len(bad))
    with pytest.raises(GitcapError):                                       # more clips than max_batch
        m._call("gitcap_attach_frame_counts", arr(*([1] * 7)), 7)
    x = torch.stack(_clips(cfg, [2, 2, 2], 15)).cuda()
    ids = torch.empty((3, MAX_LEN + 1), dtype=torch.int64, device="cuda")
    greedy = lambda B, F: m._call("gitcap_greedy", ctypes.c_void_p(x.data_ptr()), B, F, MAX_LEN, 0, ctypes.c_void_p(ids.data_ptr()), None, m._stream())
    m._attach_counts([2, 1])
    with pytest.raises(GitcapError, match="B differs"):                    # a B that disagrees with the call
        greedy(3, 2)
    m._attach_counts([2, 1, 1])
    with pytest.raises(GitcapError, match="largest"):                      # F is not the largest count
        greedy(3, 1)
    greedy(3, 2)                                                           # the refused calls consumed their attachments
    vis = torch.zeros((1, 17, cfg.enc_width), device="cuda")
    m._attach_counts([2, 1])
    with pytest.raises(GitcapError, match="frame counts are attached"):
        m._call("gitcap_set_visual", ctypes.c_void_p(vis.data_ptr()), 1, 17, m._stream())
    for name, args in (("gitcap_window_reset", (1, 2)), ("gitcap_window_push", (ctypes.c_void_p(x.data_ptr()), 1, 1, m._stream()))):
        m._attach_counts([2, 1])
        with pytest.raises(GitcapError, match="frame counts are attached"):
            m._call(name, *args)
    m._attach_counts([2, 1])
    with pytest.raises(GitcapError, match="frame counts are attached"):
        m._call("gitcap_window_greedy", MAX_LEN, 0, None, ctypes.c_void_p(ids.data_ptr()), None, m._stream())
    # hidden states of a ragged prefix have no [B][S_img] layout
    m._call("gitcap_hidden_states_enable", 1)
    try:
        m.forward(clips[:2], alone[0][0].repeat(2, 1))
        hid = torch.empty((2, cfg.dec_layers + 1, 17 * 8 + MAX_LEN + 1, cfg.dec_width), device="cuda")
        with pytest.raises(GitcapError, match="ragged"):
            m._call("gitcap_hidden_states_read", 2, 17 * 8, MAX_LEN + 1, ctypes.c_void_p(hid.data_ptr()), m._stream())
    finally:
        m._call("gitcap_hidden_states_enable", 0)
    with pytest.raises(ValueError):                                        # the Python layer refuses before anything is attached
        m.greedy_decode(clips, max_len=MAX_LEN, frame_counts=[1, 8, 3, 4, 8, 3])
    with pytest.raises(ValueError):
        m.greedy_decode(_padded(clips), max_len=MAX_LEN, frame_counts=[1, 8, 3, 0, 8, 2])
    # ... and the handle still gives the dense caption it gave before
    got = m.greedy_decode(clips[1][None], max_len=MAX_LEN, stop="never", return_logprobs=True)
    assert torch.equal(got[0], alone[1][0]) and same_bits(got[1].contiguous(), alone[1][1].contiguous())
