"""Bookkeeping of a sliding caption window (GitCaptioner.caption_stream): which frames form the window after a sequence of pushes
and when a caption is due.  Pure Python, no device: the frames themselves live in the library's ring (include/gitcap.h:
gitcap_window_*)."""
from __future__ import annotations


class WindowSchedule:
    """B clips advance in lockstep; each push appends n >= 1 frames per clip (n <= window).  A caption is due after a push once the
    window holds `window` frames and at least `hop` frames have arrived since the last caption (or since the reset).  hop = 1: a
    caption per new frame; hop = window: the reference's tumbling loop (src/real_time_inference.py:44-57: six frames, caption,
    clear).  partial: a caption is due once `hop` frames have arrived, full window or not (StudentCaptioner.caption_stream)."""

    def __init__(self, batch: int, window: int, hop: int = 1, partial: bool = False):
        if batch < 1 or window < 1 or hop < 1:
            raise ValueError(f"batch, window and hop must be >= 1 (got {batch}, {window}, {hop})")
        self.batch, self.window, self.hop = int(batch), int(window), int(hop)
        self.partial = bool(partial)
        self.reset()

    def reset(self):
        self.pushed = 0          # frames per clip pushed since the reset
        self.since = 0           # frames per clip pushed since the last caption

    def check(self, batch: int, n: int):
        """Raises ValueError if a push of n frames for `batch` clips is not one this window takes."""
        if batch != self.batch:
            raise ValueError(f"the window was opened for {self.batch} clips, got {batch}")
        if n < 1 or n > self.window:
            raise ValueError(f"a push takes 1..{self.window} frames per clip, got {n}")

    def push(self, batch: int, n: int) -> bool:
        """Record a push; -> True when a caption of the window is due now."""
        self.check(batch, n)
        self.pushed += n
        self.since += n
        if (self.partial or self.pushed >= self.window) and self.since >= self.hop:
            self.since = 0
            return True
        return False

    @property
    def full(self) -> bool:
        return self.pushed >= self.window

    def frames(self) -> range:
        """Indices (0 = the first frame pushed since the reset) of the frames the library's ring holds, oldest first: the caption
        window once it is full."""
        return range(max(0, self.pushed - self.window), self.pushed)


class PoolSchedule:
    """`streams` independent windows of `window` frames (StudentCaptioner.stream_pool): a push names the stream of each of its frames,
    any streams in any mix.  A stream is due once at least `hop` of its frames have arrived since its last caption (or since it was
    emptied) and it holds at least `min_frames` frames; min_frames = window is WindowSchedule's full-window rule, min_frames = 1 its
    partial one."""

    def __init__(self, streams: int, window: int, hop: int = 1, min_frames: int = 1):
        if streams < 1 or window < 1 or hop < 1:
            raise ValueError(f"streams, window and hop must be >= 1 (got {streams}, {window}, {hop})")
        if not 1 <= min_frames <= window:
            raise ValueError(f"min_frames={min_frames} outside 1..{window}")
        self.streams, self.window, self.hop, self.min_frames = int(streams), int(window), int(hop), int(min_frames)
        self.reset()

    def reset(self):
        self.held = [0] * self.streams       # frames a stream's window holds, 0..window
        self.since = [0] * self.streams      # frames arrived since the stream's last caption

    def check(self, ids):
        """Raises ValueError if a push whose frames go to streams `ids` is not one the pool takes."""
        ids = [int(s) for s in ids]
        if not ids:
            raise ValueError("a push takes at least one frame")
        for s in ids:
            if not 0 <= s < self.streams:
                raise ValueError(f"stream {s} outside 0..{self.streams - 1}")
        worst = max(set(ids), key=ids.count)
        if ids.count(worst) > self.window:
            raise ValueError(f"a push takes at most {self.window} frames per stream, got {ids.count(worst)} for stream {worst}")
        return ids

    def push(self, ids) -> list:
        """Record a push -> the streams that are due now, ascending.  They stay due until ``captioned`` says otherwise."""
        for s in self.check(ids):
            self.held[s] = min(self.held[s] + 1, self.window)
            self.since[s] += 1
        return [s for s in range(self.streams) if self.since[s] >= self.hop and self.held[s] >= self.min_frames]

    def captioned(self, ids):
        for s in ids:
            self.since[s] = 0

    def drop(self, s: int):
        self.held[s] = self.since[s] = 0
