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
