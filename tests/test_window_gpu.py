"""Sliding frame window (include/gitcap.h: gitcap_window_*; GitCaptioner.caption_stream): every caption of the window equals, bit
for bit, the full-clip call on the window's frames -- the ring keeps each frame's fp32 ln_post rows and only the temporal embedding
and the decoder's image prefix depend on the window."""
import ctypes

import numpy as np
import pytest
import torch

from gitcap.config import git_base, git_tiny
from gitcap.weights import quantize_weights_fp8, synthetic_weights
from oracle.git_oracle import make_frames
from gpu_support import captioner_cls, ptr  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_EXCHANGE = -1, -2, -5
STOP_NEVER, STOP_ALL_SEP = 0, 1
PUSHES = [1, 1, 2, 1, 3, 1, 6, 1, 1, 2, 1, 4]           # 24 frames: the 6-slot ring wraps four times


def _greedy(m, fr, max_len, mode=STOP_ALL_SEP):
    B, F = fr.shape[:2]
    ids = torch.empty((B, max_len + 1), dtype=torch.int64, device=m._dev)
    steps = torch.zeros((1,), dtype=torch.int32, device=m._dev)
    m._call("gitcap_greedy", ptr(fr), B, F, max_len, mode, ptr(ids), ptr(steps), m._stream())
    return ids, steps


def _encode(m, fr):
    B, F = fr.shape[:2]
    vis = torch.empty((B, F * m.cfg.tokens_per_frame, m.cfg.enc_width), dtype=torch.float32, device=m._dev)
    m._call("gitcap_encode", ptr(fr), B, F, ptr(vis), m._stream())
    return vis


def _push(m, fr):
    m._call("gitcap_window_push", ptr(fr), fr.shape[0], fr.shape[1], m._stream())


def _wgreedy(m, B, F, max_len, mode=STOP_ALL_SEP, want_vis=True):
    ids = torch.empty((B, max_len + 1), dtype=torch.int64, device=m._dev)
    steps = torch.zeros((1,), dtype=torch.int32, device=m._dev)
    vis = torch.empty((B, F * m.cfg.tokens_per_frame, m.cfg.enc_width), dtype=torch.float32, device=m._dev) if want_vis else None
    m._call("gitcap_window_greedy", max_len, mode, ptr(vis), ptr(ids), ptr(steps), m._stream())
    return ids, steps, vis


def _slide(m, pool, F, pushes, max_len, check_vis=True):
    """Push pool's frames in groups of `pushes`; after every push that fills the window compare with the full-clip calls."""
    B = pool.shape[0]
    m._call("gitcap_window_reset", B, F)
    at, checked = 0, 0
    for n in pushes:
        _push(m, pool[:, at:at + n].contiguous())
        at += n
        if at < F:
            continue
        got_ids, got_steps, got_vis = _wgreedy(m, B, F, max_len, want_vis=check_vis)
        win = pool[:, at - F:at].contiguous()
        ids, steps = _greedy(m, win, max_len)
        assert torch.equal(got_ids, ids), (at, got_ids, ids)
        assert torch.equal(got_steps, steps), at
        if check_vis:
            assert torch.equal(got_vis, _encode(m, win)), at
        checked += 1
    return checked


def test_sliding_window_equals_full_clip(captioner_cls):
    cfg = git_base(6)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=3, max_frames=6, max_text_len=8)
    pool = make_frames(2, sum(PUSHES), cfg.image_size, 31).cuda()
    assert _slide(m, pool, 6, PUSHES, 8) == len(PUSHES) - 4
    # a second reset with another size (fewer clips, fewer frames than the embeddings)
    assert _slide(m, pool[:1].contiguous(), 4, [2, 2, 1, 3, 1], 8) == 4
    # git_tiny, F = 2
    cfg = git_tiny(2)
    mt = captioner_cls(cfg, synthetic_weights(cfg, 1), max_batch=3, max_frames=2, max_text_len=8)
    pool = make_frames(3, 9, cfg.image_size, 32).cuda()
    assert _slide(mt, pool, 2, [1, 1, 2, 1, 1, 2, 1], 8) == 6


def test_raw_frames(captioner_cls):
    cfg = git_base(6)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=6, max_text_len=8)
    B, T, H, W = 2, 8, 480, 640
    raw = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)).cuda()
    S = cfg.image_size
    pre = torch.empty((B * T, 3, S, S), dtype=torch.float32, device="cuda")
    assert m._lib.gitcap_preprocess(ptr(raw), B * T, H, W, ptr(pre), S, m._stream()) == 0
    pre = pre.view(B, T, 3, S, S)
    got_raw, got_pre = [], []
    m._call("gitcap_window_reset", B, 6)
    for at in range(T):
        m._call("gitcap_window_push_raw", ptr(raw[:, at:at + 1].contiguous()), B, 1, H, W, m._stream())
        if at + 1 >= 6:
            got_raw.append(_wgreedy(m, B, 6, 8))
            win = raw[:, at + 1 - 6:at + 1].contiguous()
            ids = torch.empty((B, 9), dtype=torch.int64, device="cuda")
            steps = torch.zeros((1,), dtype=torch.int32, device="cuda")
            m._call("gitcap_greedy_raw", ptr(win), B, 6, H, W, 8, STOP_ALL_SEP, ptr(ids), ptr(steps), m._stream())
            assert torch.equal(got_raw[-1][0], ids) and torch.equal(got_raw[-1][1], steps), at
    m._call("gitcap_window_reset", B, 6)
    for at in range(0, T, 2):
        _push(m, pre[:, at:at + 2].contiguous())
        if at + 2 >= 6:
            got_pre.append(_wgreedy(m, B, 6, 8))
    # preprocess + push == raw push (windows ending at frames 6 and 8)
    for a, b in zip([got_raw[0], got_raw[2]], got_pre):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_beam_search(captioner_cls):
    cfg = git_base(6)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=6, max_text_len=10, max_beams=4)
    pool = make_frames(2, 8, cfg.image_size, 41).cuda()
    m._call("gitcap_window_reset", 2, 6)
    for at in range(8):
        _push(m, pool[:, at:at + 1].contiguous())
        if at + 1 < 6:
            continue
        dec = torch.empty((2, 10), dtype=torch.int64, device="cuda")
        lp = torch.empty((2,), dtype=torch.float32, device="cuda")
        vis = torch.empty((2, 6 * cfg.tokens_per_frame, cfg.enc_width), dtype=torch.float32, device="cuda")
        m._call("gitcap_window_beam_search", 4, 10, ctypes.c_float(0.6), 2, ptr(vis), ptr(dec), ptr(lp), m._stream())
        win = pool[:, at + 1 - 6:at + 1].contiguous()
        dec2, lp2 = torch.empty_like(dec), torch.empty_like(lp)
        m._call("gitcap_beam_search", ptr(win), 2, 6, 4, 10, ctypes.c_float(0.6), 2, ptr(dec2), ptr(lp2), m._stream())
        assert torch.equal(dec, dec2) and torch.equal(lp, lp2), at
        assert torch.equal(vis, _encode(m, win)), at


@pytest.mark.parametrize("mode", ["fp8_ffn", "v_e4m3"])
def test_modes(captioner_cls, mode):
    cfg = git_base(6)
    w = synthetic_weights(cfg, 0)
    if mode == "fp8_ffn":
        m = captioner_cls(cfg, quantize_weights_fp8(w), max_batch=2, max_frames=6, max_text_len=8, weight_dtype="fp8_e4m3",
                          compute="fp8_ffn")
    else:
        m = captioner_cls(cfg, w, max_batch=2, max_frames=6, max_text_len=8, kv_cache="v_e4m3")
    pool = make_frames(2, 9, cfg.image_size, 51).cuda()
    assert _slide(m, pool, 6, [3, 3, 1, 1, 1], 8) == 4


def test_isolation(captioner_cls):
    cfg = git_base(6)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=6, max_text_len=8, stop="all_sep")
    pool = make_frames(2, 8, cfg.image_size, 61).cuda()
    other = make_frames(2, 6, cfg.image_size, 62).cuda()
    want = [_greedy(m, pool[:, k - 6:k].contiguous(), 8) for k in (6, 7, 8)]
    m._call("gitcap_window_reset", 2, 6)
    _push(m, pool[:, :6].contiguous())
    _greedy(m, other, 8)                                            # synchronous call between pushes
    ids, steps, _ = _wgreedy(m, 2, 6, 8)
    assert torch.equal(ids, want[0][0]) and torch.equal(steps, want[0][1])
    f = m.greedy_decode_async(other, max_len=8)                    # pipelined submission between pushes
    _push(m, pool[:, 6:7].contiguous())
    f.result()
    m._call("gitcap_set_visual", ptr(_encode(m, other)), 2, 6 * cfg.tokens_per_frame, m._stream())
    ids, steps, _ = _wgreedy(m, 2, 6, 8)
    assert torch.equal(ids, want[1][0]) and torch.equal(steps, want[1][1])
    # a push leaves the current image (slot 0's K/V, text cache) alone: text_forward continues against it
    tok = torch.full((2, 3), cfg.cls_token_id, dtype=torch.int64, device="cuda")
    tok[:, 1:] = torch.tensor([[5, 9], [11, 3]], device="cuda")

    def logits_after(push):
        _encode(m, other)
        if push:
            m._call("gitcap_window_reset", 2, 6)
            _push(m, pool[:, 1:7].contiguous())
        lg = torch.empty((2, 3, cfg.vocab_size), dtype=torch.float32, device="cuda")
        m._call("gitcap_text_forward", ptr(tok), 3, 2, 1, 0, 3, ptr(lg), 1, None, 0, m._stream())
        return lg
    assert torch.equal(logits_after(False), logits_after(True))
    # push on one stream, caption on another: the library orders them by an event
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        _push(m, pool[:, 7:8].contiguous())
    with torch.cuda.stream(s2):
        ids, steps, _ = _wgreedy(m, 2, 6, 8)
    s2.synchronize()
    assert torch.equal(ids, want[2][0]) and torch.equal(steps, want[2][1])
    # the next push on s1 waits for s2's image prefix
    with torch.cuda.stream(s1):
        _push(m, pool[:, 2:3].contiguous())
    torch.cuda.synchronize()


def test_errors_and_workspace(captioner_cls):
    cfg = git_base(6)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=6, max_text_len=8)
    lib, h = m._lib, m._handle
    fr = make_frames(2, 6, cfg.image_size, 71).cuda()
    ids = torch.empty((2, 9), dtype=torch.int64, device="cuda")
    st = m._stream()
    assert lib.gitcap_window_push(h, ptr(fr), 2, 1, st) == ERR_STATE                     # no window yet
    assert lib.gitcap_window_greedy(h, 8, 0, None, ptr(ids), None, st) == ERR_STATE
    w0 = m.workspace_bytes()
    assert lib.gitcap_window_reset(h, 3, 6) == ERR_ARG                                  # > max_batch
    assert lib.gitcap_window_reset(h, 2, 7) == ERR_ARG                                  # > max_frames / num_frames
    assert lib.gitcap_window_reset(h, 2, 6) == 0
    assert m.workspace_bytes() >= w0 + 2 * 6 * cfg.tokens_per_frame * cfg.enc_width * 4
    assert lib.gitcap_window_push(h, ptr(fr), 1, 1, st) == ERR_ARG                        # B differs from the reset's
    assert lib.gitcap_window_push(h, ptr(fr), 2, 0, st) == ERR_ARG
    assert lib.gitcap_window_push(h, ptr(fr), 2, 7, st) == ERR_ARG
    assert lib.gitcap_window_push(h, None, 2, 1, st) == ERR_ARG
    assert lib.gitcap_window_push(h, ctypes.c_void_p(fr.data_ptr() + 4), 2, 1, st) == ERR_ARG
    assert lib.gitcap_window_push_raw(h, None, 2, 1, 480, 640, st) == ERR_ARG
    assert lib.gitcap_window_push(h, ptr(fr), 2, 5, st) == 0
    assert lib.gitcap_window_greedy(h, 8, 0, None, ptr(ids), None, st) == ERR_STATE     # 5 < F frames
    assert lib.gitcap_window_push(h, ptr(fr), 2, 1, st) == 0
    vis = torch.empty((2, 6 * cfg.tokens_per_frame + 1, cfg.enc_width), dtype=torch.float32, device="cuda")
    assert lib.gitcap_window_greedy(h, 8, 0, ctypes.c_void_p(vis.data_ptr() + 4), ptr(ids), None, st) == ERR_ARG
    assert lib.gitcap_window_greedy(h, 8, 0, None, ptr(ids), None, st) == 0
    assert lib.gitcap_window_reset(h, 2, 6) == 0                                        # empties it
    assert lib.gitcap_window_greedy(h, 8, 0, None, ptr(ids), None, st) == ERR_STATE
    assert lib.gitcap_window_reset(h, 0, 0) == 0
    assert m.workspace_bytes() == w0
    assert lib.gitcap_window_push(h, ptr(fr), 2, 1, st) == ERR_STATE                     # released
    torch.cuda.synchronize()


def test_caption_stream(captioner_cls):
    cfg = git_tiny(4)
    m = captioner_cls(cfg, synthetic_weights(cfg, 3), max_batch=2, max_frames=4, max_text_len=8, stop="never")
    pool = make_frames(2, 13, cfg.image_size, 81)
    for hop in (1, 3, 4):
        for dev in ("cpu", "cuda"):
            src = pool if dev == "cpu" else pool.cuda()
            cs = m.caption_stream(batch=2, hop=hop, max_len=8)
            since = None
            for k in range(13):
                got = cs.push(src[:, k])
                due = k + 1 >= 4 and (since is None or k + 1 - since >= hop)
                if not due:
                    assert got is None, (hop, k)
                    continue
                since = k + 1
                assert got is not None and got.device.type == dev, (hop, k)
                assert torch.equal(got, m.greedy_decode(src[:, k + 1 - 4:k + 1], max_len=8)), (hop, k)
    # several frames per push, reset, beam dict
    cs = m.caption_stream(batch=2, hop=1, max_len=8)
    assert cs.push(pool[:, :3]) is None
    assert torch.equal(cs.push(pool[:, 3:5]), m.greedy_decode(pool[:, 1:5], max_len=8))
    cs.reset()
    assert cs.push(pool[:, 5]) is None
    assert torch.equal(cs.push(pool[:, 6:9]), m.greedy_decode(pool[:, 5:9], max_len=8))
    with pytest.raises(ValueError):
        cs.push(pool[:1, 9])                                        # batch changes
    # a second stream invalidates the first
    cs2 = m.caption_stream(batch=1, window=2, hop=2, max_len=8)
    from gitcap._lib import GitcapError
    with pytest.raises(GitcapError):
        cs.push(pool[:, 9])
    assert cs2.push(pool[:1, 0]) is None
    assert torch.equal(cs2.push(pool[:1, 1]), m.greedy_decode(pool[:1, 0:2], max_len=8))
    mb = captioner_cls(cfg, synthetic_weights(cfg, 3), max_batch=2, max_frames=4, max_text_len=8, max_beams=2)
    csb = mb.caption_stream(batch=2, hop=2, max_len=6, beam_size=2, visual_features=True)
    assert csb.push(pool[:, 0:3]) is None
    r = csb.push(pool[:, 3])
    want = mb.infer_async(pool[:, 0:4], beam_size=2, max_steps=6, visual_features=True).result()
    assert torch.equal(r["predictions"], want["predictions"]) and torch.equal(r["logprobs"], want["logprobs"])
    assert torch.equal(r["visual_features"], want["visual_features"])


def test_exchange_failure_empties_the_window(captioner_cls):
    """As tests/test_pipeline_gpu.py: test_exchange_failure_poisons_submissions_in_flight, at a size whose image pass and prefix use
    the fused GEMM + LayerNorm epilogues: the window call after the failure returns GITCAP_ERR_EXCHANGE once, the window is empty,
    and a CaptionStream re-pushes the frames it kept and still returns the right caption."""
    from gitcap import _lib
    lib = _lib.load()
    cfg = git_base(6)
    w = synthetic_weights(cfg, 0)
    fr = make_frames(10, 7, cfg.image_size, 91)
    m = captioner_cls(cfg, w, max_batch=10, max_frames=6, max_text_len=8, stop="never")
    want = [m.greedy_decode(fr[:, k - 6:k].cuda(), max_len=8).cpu() for k in (6, 7)]
    m.poll_errors()
    frd = fr.cuda()
    ids = torch.empty((10, 9), dtype=torch.int64, device="cuda")
    old = lib.gitcap_dbg_config(6, 1)
    assert old == 0
    try:
        m._call("gitcap_window_reset", 10, 6)
        _push(m, frd[:, :6].contiguous())
        torch.cuda.synchronize()
        assert lib.gitcap_window_greedy(m._handle, 8, 0, None, ptr(ids), None, m._stream()) == ERR_EXCHANGE
        assert lib.gitcap_window_greedy(m._handle, 8, 0, None, ptr(ids), None, m._stream()) == ERR_STATE   # emptied
        _push(m, frd[:, :6].contiguous())                       # (the handle now runs the unfused launches)
        got, _, _ = _wgreedy(m, 10, 6, 8, mode=STOP_NEVER, want_vis=False)
        assert torch.equal(got.cpu(), want[0])
        m.poll_errors()
    finally:
        lib.gitcap_dbg_config(6, old)
    m2 = captioner_cls(cfg, w, max_batch=10, max_frames=6, max_text_len=8, stop="never")
    old = lib.gitcap_dbg_config(6, 1)
    try:
        cs = m2.caption_stream(batch=10, hop=1, max_len=8)
        assert torch.equal(cs.push(fr[:, :6]), want[0])          # CPU in: vouched, re-pushed and re-captioned after the failure
        assert torch.equal(cs.push(fr[:, 6]), want[1])
        m2.poll_errors()
    finally:
        lib.gitcap_dbg_config(6, old)
