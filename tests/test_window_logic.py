"""Sliding caption window bookkeeping (gitcap/window.py: WindowSchedule, the part of GitCaptioner.caption_stream that decides which
frames form the window and when a caption is due).  CPU only."""
import pytest

from gitcap.window import WindowSchedule


def _run(window, hop, pushes):
    s = WindowSchedule(batch=2, window=window, hop=hop)
    due = []
    for n in pushes:
        if s.push(2, n):
            due.append(list(s.frames()))
    return s, due


def test_hop_one_captions_every_push_once_full():
    s, due = _run(6, 1, [1] * 9)
    assert due == [list(range(k - 6, k)) for k in range(6, 10)]
    assert s.full and list(s.frames()) == [3, 4, 5, 6, 7, 8]


def test_hop_equal_to_window_is_the_tumbling_loop():
    _, due = _run(6, 6, [1] * 18)
    assert due == [list(range(0, 6)), list(range(6, 12)), list(range(12, 18))]


def test_hop_three_and_pushes_of_several_frames():
    # pushes [1,1,2,1,3,1,6,1,1]: frames pushed 1 2 4 5 8 9 15 16 17
    s, due = _run(6, 3, [1, 1, 2, 1, 3, 1, 6, 1, 1])
    assert due == [list(range(2, 8)), list(range(9, 15))]
    assert s.pushed == 17 and s.since == 2 and list(s.frames()) == list(range(11, 17))


def test_window_before_full_and_wrap_around():
    s = WindowSchedule(batch=1, window=4, hop=1)
    assert not s.push(1, 3) and not s.full and list(s.frames()) == [0, 1, 2]
    assert s.push(1, 2) and list(s.frames()) == [1, 2, 3, 4]
    for k in range(5, 16):            # the ring wraps several times
        assert s.push(1, 1) and list(s.frames()) == list(range(k - 3, k + 1))
    assert s.push(1, 4) and list(s.frames()) == [16, 17, 18, 19]


def test_reset_empties_the_window():
    s = WindowSchedule(batch=1, window=2, hop=2)
    assert not s.push(1, 1) and s.push(1, 1)
    s.reset()
    assert not s.full and list(s.frames()) == []
    assert not s.push(1, 1) and s.push(1, 1) and list(s.frames()) == [0, 1]


def test_rejects_bad_pushes_and_batch_changes():
    s = WindowSchedule(batch=2, window=3, hop=1)
    with pytest.raises(ValueError):
        s.push(2, 4)                   # n > F
    with pytest.raises(ValueError):
        s.push(2, 0)
    with pytest.raises(ValueError):
        s.push(3, 1)                   # batch differs from the window's
    assert s.pushed == 0               # a refused push changes nothing
    with pytest.raises(ValueError):
        WindowSchedule(batch=1, window=0)
    with pytest.raises(ValueError):
        WindowSchedule(batch=1, window=2, hop=0)
