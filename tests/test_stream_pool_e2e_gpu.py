"""The student's stream pool end to end (StudentCaptioner.stream_pool): uint8 camera frames through the native tiny encoder.  Every
caption a stream gets from the pool is bit for bit greedy_decode on a list holding that stream's last frames, cut behind the row's
own first SEP, whichever other streams were pushed to or captioned with it."""
import pytest
import torch

from gitcap import _lib
from gpu_support import camera, make_student_native, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

L = 6
KW = dict(max_batch=4, max_text_len=8)


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available()
    return make_student_native("tiny", **KW)


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a, b) if a.dtype == torch.int64 else same_bits(a.contiguous(), b.contiguous()), what


def cut(ids, sep):
    """Generated tokens of a CLS-first row up to and including its first SEP (all of them without one)."""
    hits = (ids[1:] == sep).nonzero()
    return int(hits[0]) + 1 if hits.numel() else ids.shape[0] - 1


def test_four_cameras_that_differ_in_length(native):
    m, F, s = native, native.cfg.mem_tokens, native.image_encoder.cfg.img_size
    lens = [3, 7, 1, F]
    cams = [camera((n, s, s, 3), 90 + c) for c, n in enumerate(lens)]
    # the fixed interleaving: pushes of one to four frames, a camera twice in one push, cameras out of order
    pushes = [[1], [3, 0, 1], [1, 1, 3], [2, 3, 0, 1], [3], [1, 0], [3, 1, 3]]
    assert [sum(p.count(c) for p in pushes) for c in range(4)] == lens
    pool = m.stream_pool(4, hop=1, max_len=L, logprobs=True, min_frames=1)
    at = [0, 0, 0, 0]
    captions = 0
    for p in pushes:
        frames = []
        for c in p:
            frames.append(cams[c][at[c]])
            at[c] += 1
        out = pool.push(torch.stack(frames, 0), p)
        assert sorted(out) == sorted(set(p))                 # hop = 1, min_frames = 1: every camera that got a frame
        for c, ids in out.items():
            n = min(at[c], F)
            ref_ids, ref_lp = m.greedy_decode([cams[c][at[c] - n:at[c]]], max_len=L, stop="never", return_logprobs=True)
            k = cut(ref_ids[0], m.cfg.sep_token_id)
            assert ids.device.type == "cpu"
            _eq(ids, ref_ids[0, :1 + k], f"camera {c} after {at[c]} frames")
            _eq(pool.last_logprobs[c], ref_lp[0, :k], f"logprobs of camera {c} after {at[c]} frames")
            assert pool.last_frames[c] == n
            captions += 1
    assert captions == sum(len(set(p)) for p in pushes) and pool.counts() == [3, F, 1, F]


def test_min_frames_of_a_full_window_is_the_single_stream(native):
    m, F, s = native, native.cfg.mem_tokens, native.image_encoder.cfg.img_size
    twin = make_student_native("tiny", **KW)                 # a second model from the same seed
    st = twin.caption_stream(batch=1, hop=1, max_len=L, logprobs=True)
    pool = m.stream_pool(2, hop=1, max_len=L, logprobs=True, min_frames=F)
    a, b = camera((F + 2, s, s, 3), 95), camera((F - 1, s, s, 3), 96)
    for i in range(F + 2):
        if i < F - 1:                                        # camera 1 never fills its window: no caption for it
            out = pool.push(torch.stack([b[i], a[i]], 0), [1, 0])
        else:
            out = pool.push(a[i][None], [0])
        want = st.push(a[i][None])
        if i < F - 1:
            assert out == {} and want is None
            continue
        assert sorted(out) == [0] and pool.last_frames[0] == F
        _eq(out[0], want[0], f"push {i + 1}")
        _eq(pool.last_logprobs[0], st.last_logprobs[0], f"logprobs of push {i + 1}")
    assert pool.counts() == [F, F - 1]


def test_more_due_streams_than_max_batch():
    m = make_student_native("tiny", max_batch=2, max_text_len=8)
    s = m.image_encoder.cfg.img_size
    pool = m.stream_pool(5, hop=1, max_len=L, stop="never", logprobs=True, top_logprobs=2)
    first = pool.push(camera((3, s, s, 3), 97), [4, 2, 4])   # streams at different fill levels
    assert sorted(first) == [2, 4]
    frames = camera((5, s, s, 3), 98)
    out = pool.push(frames, [3, 0, 4, 1, 2])
    assert sorted(out) == [0, 1, 2, 3, 4] and pool.counts() == [1, 1, 2, 1, 3]
    kept = {c: (out[c], pool.last_logprobs[c], pool.last_top_ids[c], pool.last_top_logprobs[c], pool.last_frames[c]) for c in out}
    for c in range(5):
        one = pool.caption([c], to_cpu=True)
        for got, ref, what in zip((one[c], pool.last_logprobs[c], pool.last_top_ids[c], pool.last_top_logprobs[c]), kept[c],
                                  ("ids", "logprobs", "top ids", "top logprobs")):
            _eq(got, ref, f"{what} of stream {c} alone")
        assert pool.last_frames[c] == kept[c][4]
    with pytest.raises(_lib.GitcapError, match="holds no token"):
        pool.drop(1) or pool.caption([1])


def test_a_stream_and_a_pool_live_side_by_side(native):
    m, F, s = native, native.cfg.mem_tokens, native.image_encoder.cfg.img_size
    cam = camera((F + 1, s, s, 3), 99)
    st = m.caption_stream(batch=1, hop=1, max_len=L, stop="never", partial=True)
    assert st.push(cam[0][None]) is not None
    pool = m.stream_pool(2, hop=1, max_len=L, stop="never")           # opening a pool leaves the stream alone ...
    for i in range(1, F + 1):
        got = st.push(cam[i][None])
        out = pool.push(cam[i][None], [1])
        n = min(i + 1, F)
        _eq(got, m.greedy_decode([cam[i + 1 - n:i + 1]], max_len=L, stop="never"), f"the stream after {i + 1} pushes")
        _eq(out[1], m.greedy_decode([cam[max(1, i + 1 - F):i + 1]], max_len=L, stop="never")[0], f"the pool after {i} pushes")
    st2 = m.caption_stream(batch=1, hop=1, max_len=L, stop="never", partial=True)      # ... and opening a stream leaves the pool alone
    assert st2.push(cam[0][None]) is not None
    assert pool.counts() == [0, F] and sorted(pool.push(cam[0][None], [0])) == [0]
    with pytest.raises(_lib.GitcapError, match="StudentCaptionStream was invalidated"):
        st.push(cam[0][None])                                                         # (a second stream still replaces the first)
    pool2 = m.stream_pool(1, max_len=L)
    with pytest.raises(_lib.GitcapError, match="StudentStreamPool was invalidated"):
        pool.counts()
    # a model that moves takes neither along
    if torch.cuda.device_count() >= 2:
        m.to("cuda:1")
        m.to("cuda:0")
    else:
        m._moved()                                           # what to() runs behind a real move
    with pytest.raises(_lib.GitcapError, match="StudentCaptionStream was invalidated"):
        st2.push(cam[0][None])
    with pytest.raises(_lib.GitcapError, match="StudentStreamPool was invalidated"):
        pool2.push(cam[0][None], [0])
