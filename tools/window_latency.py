"""Per-update wall time of a sliding caption window (include/gitcap.h: gitcap_window_*), GIT-base, F = 6, 20 greedy tokens:
  window  = push ONE new frame per clip + gitcap_window_greedy over the last 6
  full    = gitcap_greedy on the same 6 frames (what a sliding window costs without the ring)
Host clock around a device synchronise, warmed up, A/B interleaved, medians over ITERS (default 30) updates, B = 1 and 16.
Usage: python tools/window_latency.py [out.txt]    (the assembly kernel's own time: rocprofv3 --kernel-trace --stats -- python
tools/window_latency.py, row window_assemble_kernel)"""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-video-captioning_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gitcap.config import git_base  # noqa: E402
from gitcap.model import GitCaptioner  # noqa: E402
from gitcap.weights import synthetic_weights  # noqa: E402

F, MAX_LEN = 6, 20
ITERS = int(os.environ.get("ITERS", "30"))
WARMUP = 5


def P(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def main():
    cfg = git_base(F)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), max_batch=16, max_frames=F, max_text_len=MAX_LEN, stop="never")
    lines = [f"GIT-base, F = {F}, {MAX_LEN} greedy tokens (stop=never); host clock around torch.cuda.synchronize(), "
             f"{WARMUP} warm-up + {ITERS} interleaved updates, median [min .. max] ms"]
    for B in (1, 16):
        total = F + WARMUP + ITERS
        pool = torch.randn(B, total, 3, cfg.image_size, cfg.image_size, device="cuda")
        frames = [pool[:, k:k + 1].contiguous() for k in range(total)]          # one new frame per clip per update
        ids = torch.empty((B, MAX_LEN + 1), dtype=torch.int64, device="cuda")
        steps = torch.zeros((1,), dtype=torch.int32, device="cuda")
        st = m._stream()
        m._call("gitcap_window_reset", B, F)
        m._call("gitcap_window_push", P(pool[:, :F].contiguous()), B, F, st)
        tw, tf = [], []
        for k in range(F, total):
            win = pool[:, k + 1 - F:k + 1].contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m._call("gitcap_window_push", P(frames[k]), B, 1, st)
            m._call("gitcap_window_greedy", MAX_LEN, 0, None, P(ids), P(steps), st)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            wids = ids.clone()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            m._call("gitcap_greedy", P(win), B, F, MAX_LEN, 0, P(ids), P(steps), st)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            assert torch.equal(wids, ids), "window caption differs from the full-clip call"
            if k >= F + WARMUP:
                tw.append((t1 - t0) * 1e3)
                tf.append((t3 - t2) * 1e3)
        mw, mf = statistics.median(tw), statistics.median(tf)
        lines.append(f"B = {B:2d}: window update (push 1 frame + window_greedy) {mw:7.2f} [{min(tw):.2f} .. {max(tw):.2f}]   "
                     f"gitcap_greedy (6 frames) {mf:7.2f} [{min(tf):.2f} .. {max(tf):.2f}]   ratio {mw / mf:.3f}  (n = {len(tw)}, "
                     f"captions bitwise equal)")
    m._call("gitcap_window_reset", 0, 0)
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
