"""Live captioning on the student, on the device: TinyViT from raw camera frames (gitcap_tinyvit_encode_raw), the memory-token
window (gitcap_student_window_*) and StudentCaptioner.caption_stream.

Every comparison is torch.equal: each new path is defined as bitwise equal to a composition of existing entry points
(gitcap_preprocess + gitcap_tinyvit_encode; gitcap_student_greedy / _beam_search on the window's tokens), and those are held to
the oracle by test_preprocess.py, test_tinyvit_gpu.py and test_student.py."""
import pytest
import torch

from gitcap.student_config import student_base, student_synthetic_weights, student_tiny
from gpu_support import camera, make_encoder, make_student, make_student_native, ptr, student_cfg
from oracle.student_oracle import make_memory

ERR_ARG, ERR_STATE = -1, -2
STOP_NEVER, STOP_ALL_SEP = 0, 1
GROUPS = [1, 1, 2, 1, 3, 1, 6, 1, 1, 2, 1, 4]          # 24 tokens through a ring of 6: it wraps four times


# ---------------------------------------------------------------------------------------------------- encode_raw
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(224, 224), (480, 640), (360, 300)])
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("name", ["tiny", "21m"])
def test_gpu_encode_raw_equals_preprocess_then_encode(name, n, H, W):
    from gitcap.preprocess import preprocess_frames
    enc = make_encoder(name)
    frames = camera((n, H, W, 3), 1000 * H + W + n)
    x = preprocess_frames(frames, crop=enc.cfg.img_size)
    want_maps, want_mem = enc(x), enc.memory(x[None])
    got_maps, got_mem = enc(frames), enc.memory(frames)               # CPU uint8 [n,H,W,3]: one clip
    assert got_mem.shape == (1, n, enc.out_dim) and torch.isfinite(got_mem).all()
    assert torch.equal(got_mem, want_mem)
    for a, b in zip(got_maps, want_maps):
        assert a.shape == b.shape and torch.equal(a, b)
    maps2, mem2 = enc.forward_with_memory(frames.cuda()[None])        # device uint8 [1,n,H,W,3]
    assert torch.equal(mem2, want_mem) and all(torch.equal(a, b) for a, b in zip(maps2, want_maps))


@pytest.mark.gpu
def test_gpu_encode_raw_refuses_bad_arguments():
    enc = make_encoder("tiny", max_frames=2)
    lib, h = enc._lib, enc._handle
    frames = camera((3, 80, 96, 3), 5).cuda()
    mem = torch.empty((3, enc.out_dim), dtype=torch.float32, device="cuda:0")
    call = lambda fr, n, H, W, m: lib.gitcap_tinyvit_encode_raw(h, fr, n, H, W, m, None, None)
    assert call(ptr(frames), 2, 80, 96, ptr(mem)) == 0
    for args in ((None, 2, 80, 96, ptr(mem)), (ptr(frames), 2, 80, 96, None), (ptr(frames), 0, 80, 96, ptr(mem)),
                 (ptr(frames), 3, 80, 96, ptr(mem)),                     # n > max_frames
                 (ptr(frames), 2, 0, 96, ptr(mem)), (ptr(frames), 2, 80, 0, ptr(mem))):   # no resized frame reaches the crop
        assert call(*args) == ERR_ARG, args
        assert lib.gitcap_tinyvit_last_error(h)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        enc.memory(torch.zeros((1, 2, 80, 96, 4), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------- the window in the C ABI
class _Win:
    """The window entry points of a StudentCaptioner's handle on device tensors."""

    def __init__(self, m):
        self.m, self.lib, self.h = m, m._lib, m._handle

    def stream(self):
        return self.m._stream()

    def reset(self, B):
        return self.lib.gitcap_student_window_reset(self.h, B)

    def push(self, mem, B=None, n=None):
        mem = mem.contiguous()
        return self.lib.gitcap_student_window_push(self.h, ptr(mem), mem.shape[0] if B is None else B,
                                                   mem.shape[1] if n is None else n, self.stream())

    def greedy(self, B, max_len, stop):
        ids = torch.full((B, max_len + 1), -1, dtype=torch.int64, device="cuda:0")
        steps = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
        rc = self.lib.gitcap_student_window_greedy(self.h, max_len, stop, ptr(ids), ptr(steps), self.stream())
        return rc, ids, steps

    def full_greedy(self, mem, max_len, stop):
        mem = mem.contiguous()
        B = mem.shape[0]
        ids = torch.full((B, max_len + 1), -1, dtype=torch.int64, device="cuda:0")
        steps = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
        rc = self.lib.gitcap_student_greedy(self.h, ptr(mem), B, max_len, stop, ptr(ids), ptr(steps), self.stream())
        assert rc == 0, self.err()
        return ids, steps

    def beam(self, B, k, max_len):
        ids = torch.full((B, max_len), -1, dtype=torch.int64, device="cuda:0")
        return self.lib.gitcap_student_window_beam_search(self.h, k, max_len, ptr(ids), self.stream()), ids

    def err(self):
        return self.lib.gitcap_student_last_error(self.h)


def _sep_friendly(cfg, seed):
    """Synthetic weights whose SEP logit is raised so that STOP_ALL_SEP ends some captions early (steps < max_len)."""
    w = dict(student_synthetic_weights(cfg, seed))
    w["linear.bias"] = w["linear.bias"].copy()
    w["linear.bias"][cfg.sep_token_id] += 1.5
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_gpu_sliding_window_equals_full_call(name, B):
    from gitcap.student import StudentCaptioner
    cfg = student_cfg(name)
    F, max_len = cfg.mem_tokens, 12
    m = StudentCaptioner(cfg=cfg, weights=_sep_friendly(cfg, 0), device="cuda:0", max_batch=6, max_text_len=16)
    w = _Win(m)
    toks = make_memory(B, sum(GROUPS), cfg.d_model, 17 + B).cuda()            # [B, 24, D]: the stream of tokens
    assert w.reset(B) == 0, w.err()
    pushed, checked, beams_checked = 0, 0, 0
    for gi, n in enumerate(GROUPS):
        assert w.push(toks[:, pushed:pushed + n]) == 0, w.err()
        pushed += n
        if pushed < F:
            continue
        window = toks[:, pushed - F:pushed].contiguous()
        for stop in (STOP_ALL_SEP, STOP_NEVER):
            rc, ids, steps = w.greedy(B, max_len, stop)
            assert rc == 0, w.err()
            want_ids, want_steps = w.full_greedy(window, max_len, stop)
            assert torch.equal(steps, want_steps), (gi, stop, steps, want_steps)
            assert torch.equal(ids, want_ids), (gi, stop)
            checked += 1
        if gi % 3 == 1:                                                       # a subset of the points: k = 2 and 3
            for k in (2, 3):
                rc, ids = w.beam(B, k, 9)
                assert rc == 0, w.err()
                assert torch.equal(ids, m.beam_search(window, max_len=9, k=k)), (gi, k)
                beams_checked += 1
    assert checked >= 16 and beams_checked >= 4
    # a second reset with another B: the ring is reallocated and starts empty
    B2 = 3 - B
    assert w.reset(B2) == 0, w.err()
    assert w.greedy(B2, max_len, STOP_NEVER)[0] == ERR_STATE
    toks2 = make_memory(B2, F + 2, cfg.d_model, 99).cuda()
    assert w.push(toks2[:, :F]) == 0 and w.push(toks2[:, F:]) == 0, w.err()
    rc, ids, steps = w.greedy(B2, max_len, STOP_NEVER)
    assert rc == 0, w.err()
    want_ids, want_steps = w.full_greedy(toks2[:, 2:], max_len, STOP_NEVER)
    assert torch.equal(ids, want_ids) and torch.equal(steps, want_steps)
    assert w.reset(0) == 0                                                    # releases the ring
    assert w.push(toks2[:, :1]) == ERR_STATE


@pytest.mark.gpu
def test_gpu_window_isolation():
    cfg = student_base()
    m = make_student("base", max_batch=4, max_text_len=12)
    w = _Win(m)
    F, B, T = cfg.mem_tokens, 2, 7
    mem0 = make_memory(B, F, cfg.d_model, 3).cuda()
    toks = make_memory(B, F + 3, cfg.d_model, 4).cuda()
    y = torch.randint(1, cfg.vocab_length, (B, T), generator=torch.Generator().manual_seed(1)).cuda()
    y[:, 0] = cfg.cls_token_id
    before = m.forward_decoder(y, mem0)                                       # set_memory(mem0) + forward_decoder

    def decoder_only():
        logits = torch.empty((B, T, cfg.vocab_length), dtype=torch.float32, device="cuda:0")
        assert m._lib.gitcap_student_forward_decoder(m._handle, ptr(y), T, B, T, ptr(logits), m._stream()) == 0, w.err()
        return logits

    assert w.reset(B) == 0
    for lo, hi in ((0, 4), (4, 6), (6, 9)):                                   # fill the ring and wrap it: pushes only
        assert w.push(toks[:, lo:hi]) == 0, w.err()
        assert torch.equal(decoder_only(), before)                            # the decoder still sees mem0
    rc, ids, _ = w.greedy(B, 6, STOP_NEVER)
    assert rc == 0, w.err()
    window = toks[:, 3:9].contiguous()
    after = decoder_only()                                                    # the handle now holds the window's memory
    assert torch.equal(after, m.forward_decoder(y, window))
    assert not torch.equal(after, before)
    # after a window beam search the handle holds B * k rows, as after the full call
    rc, _ = w.beam(B, 2, 5)
    assert rc == 0, w.err()
    y2 = y.repeat_interleave(2, dim=0).contiguous()
    logits = torch.empty((2 * B, T, cfg.vocab_length), dtype=torch.float32, device="cuda:0")
    assert m._lib.gitcap_student_forward_decoder(m._handle, ptr(y2), T, 2 * B, T, ptr(logits), m._stream()) == 0, w.err()
    assert torch.equal(logits, m.forward_decoder(y2, window.repeat_interleave(2, dim=0)))
    # pushes on a side stream, window calls on the current one: the two events order them
    side = torch.cuda.Stream()
    assert w.reset(B) == 0
    more = make_memory(B, 8, cfg.d_model, 6).cuda()
    torch.cuda.synchronize()
    for lo, hi in ((0, 6), (6, 7), (7, 8)):
        with torch.cuda.stream(side):
            assert w.push(more[:, lo:hi]) == 0, w.err()
        rc, ids, steps = w.greedy(B, 6, STOP_NEVER)
        assert rc == 0, w.err()
        want_ids, _ = w.full_greedy(more[:, hi - 6:hi], 6, STOP_NEVER)
        assert torch.equal(ids, want_ids), (lo, hi)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_window_errors():
    from gitcap.student import StudentCaptioner
    cfg = student_tiny()
    F = cfg.mem_tokens
    m = make_student("tiny", max_batch=4, max_text_len=8)
    w = _Win(m)
    toks = make_memory(2, F + 1, cfg.d_model, 1).cuda()
    def refused(rc, code):
        assert rc == code, (rc, code, w.err())
        assert w.err()                                                        # the message is not empty

    refused(w.push(toks[:, :1]), ERR_STATE)                                   # before any reset
    refused(w.greedy(2, 4, STOP_NEVER)[0], ERR_STATE)
    refused(w.beam(2, 2, 4)[0], ERR_STATE)
    refused(w.reset(5), ERR_ARG)                                              # B > max_rows
    refused(w.reset(-1), ERR_ARG)
    assert w.reset(2) == 0
    refused(w.lib.gitcap_student_window_push(w.h, None, 2, 1, w.stream()), ERR_ARG)
    refused(w.push(toks[:1, :1]), ERR_ARG)                                    # B differs from the reset's
    refused(w.push(toks[:, :1], n=0), ERR_ARG)
    refused(w.push(toks, n=F + 1), ERR_ARG)
    assert w.push(toks[:, :F - 1]) == 0
    refused(w.greedy(2, 4, STOP_NEVER)[0], ERR_STATE)                         # F - 1 tokens: not full
    refused(w.beam(2, 2, 4)[0], ERR_STATE)
    assert w.push(toks[:, F - 1:F]) == 0
    assert w.greedy(2, 4, STOP_NEVER)[0] == 0
    refused(w.lib.gitcap_student_window_greedy(w.h, 4, STOP_NEVER, None, None, w.stream()), ERR_ARG)
    refused(w.greedy(2, 0, STOP_NEVER)[0], ERR_ARG)
    refused(w.greedy(2, 9, STOP_NEVER)[0], ERR_ARG)                           # max_len > max_text_len
    refused(w.greedy(2, 4, 7)[0], ERR_ARG)                                    # unknown stop rule
    refused(w.lib.gitcap_student_window_beam_search(w.h, 2, 4, None, w.stream()), ERR_ARG)
    refused(w.beam(2, 3, 4)[0], ERR_ARG)                                      # B * k = 6 > max_rows
    refused(w.beam(2, 0, 4)[0], ERR_ARG)
    refused(w.beam(2, 2, 1)[0], ERR_ARG)                                      # max_len < 2
    refused(w.beam(2, 2, 10)[0], ERR_ARG)                                     # max_len > max_text_len + 1
    assert w.beam(2, 2, 9)[0] == 0
    assert w.reset(2) == 0                                                    # a reset empties the window
    refused(w.greedy(2, 4, STOP_NEVER)[0], ERR_STATE)
    torch.cuda.synchronize()
    # weights not finalized
    raw = StudentCaptioner(cfg=cfg, device="cuda:0", max_batch=2, max_text_len=8)
    w2 = _Win(raw)
    assert w2.reset(1) == 0
    assert w2.push(toks[:1, :1]) == ERR_STATE and w2.err()
    assert w2.greedy(1, 4, STOP_NEVER)[0] == ERR_STATE
    assert w2.beam(1, 2, 4)[0] == ERR_STATE


# ---------------------------------------------------------------------------------------------------- Python surface
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "21m"])
def test_gpu_caption_stream_end_to_end(name):
    from gitcap._lib import GitcapError
    from gitcap.preprocess import preprocess_frames
    m = make_student_native(name, max_batch=4, max_text_len=25)
    F, S = m.cfg.mem_tokens, m.image_encoder.cfg.img_size
    cam = camera((1, 14, 480, 640, 3), 77)                                   # one clip, 14 CPU camera frames
    x = preprocess_frames(cam, crop=S)                                        # [1,14,3,S,S] on the device
    # raw frames straight into the decode calls == the transformed frames
    assert torch.equal(m.greedy_decode(cam[:, :F], max_len=25, stop="never"),
                       m.greedy_decode(x[:, :F], max_len=25, stop="never").cpu())
    assert torch.equal(m.beam_search(cam[:, :F], max_len=8, k=2), m.beam_search(x[:, :F], max_len=8, k=2).cpu())
    fm_raw, mem_raw = m.forward_image_enc(cam[:, :F])
    fm_x, mem_x = m.forward_image_enc(x[:, :F])
    assert torch.equal(mem_raw, mem_x) and all(torch.equal(a, b) for a, b in zip(fm_raw, fm_x))
    # hop = 1: None five times, then a caption per frame, each the full call on the last six transformed frames
    st = m.caption_stream(hop=1, max_len=25, stop="never")
    for i in range(9):
        out = st.push(cam[:, i])
        if i < F - 1:
            assert out is None, i
            continue
        assert out.device.type == "cpu" and out.shape == (1, 26)
        assert torch.equal(out, m.greedy_decode(x[:, i - F + 1:i + 1], max_len=25, stop="never").cpu()), i
    st.reset()
    assert st.push(cam[:, 0]) is None
    # hop = 6 (the reference's tumbling loop): a caption every sixth push; the default stop rule truncates as greedy_decode
    st6 = m.caption_stream(hop=F, max_len=10)
    with pytest.raises(GitcapError):                                          # a second stream invalidated the first
        st.push(cam[:, 1])
    got = [st6.push(cam[:, i].cuda()) for i in range(2 * F)]
    assert [g is not None for g in got] == ([False] * (F - 1) + [True]) * 2
    for j in (1, 2):
        assert got[j * F - 1].device.type == "cuda"
        assert torch.equal(got[j * F - 1], m.greedy_decode(x[:, (j - 1) * F:j * F], max_len=10))
    # beams, several frames per push, transformed frames and memory tokens as input
    sb = m.caption_stream(hop=2, max_len=8, beams=2)
    assert sb.push(cam[:, 0:4]) is None and sb.push(x[:, 4]) is None          # [1,4,H,W,3] then [1,3,S,S]
    out = sb.push(m.image_encoder.memory(x[:, 5:7]))                          # tokens [1,2,D]: frames 1..6 form the window
    assert torch.equal(out, m.beam_search(x[:, 1:7], max_len=8, k=2))
    with pytest.raises(ValueError):
        sb.push(cam[:, :F + 1])                                               # more than a window per push
    with pytest.raises(ValueError):
        sb.push(torch.cat([cam[:, 0], cam[:, 0]]))                            # two clips into a stream opened for one
    with pytest.raises(ValueError):
        m.caption_stream(batch=3, beams=2)                                    # 6 rows > max_batch
    # two clips in lockstep
    cam2 = camera((2, F + 1, 120, 160, 3), 78)
    x2 = preprocess_frames(cam2, crop=S)
    s2 = m.caption_stream(batch=2, hop=1, max_len=12, stop="never")
    outs = [s2.push(cam2[:, i]) for i in range(F + 1)]
    assert all(o is None for o in outs[:F - 1])
    assert torch.equal(outs[F - 1], m.greedy_decode(x2[:, :F], max_len=12, stop="never").cpu())
    assert torch.equal(outs[F], m.greedy_decode(x2[:, 1:], max_len=12, stop="never").cpu())


@pytest.mark.gpu
def test_gpu_caption_stream_needs_the_native_encoder():
    from gitcap._lib import GitcapError
    m = make_student("tiny", max_batch=2, max_text_len=8)
    with pytest.raises(GitcapError, match="native"):
        m.caption_stream()
    with pytest.raises(GitcapError):
        m.greedy_decode(camera((1, 6, 48, 64, 3), 1), max_len=4)             # raw frames without an encoder
