#!/usr/bin/env python3
"""What a draft costs and saves on the teacher's greedy call (its output is meant for profiles/r24_teacher_draft_bench.txt).

    python tools/teacher_draft_bench.py [--reps 5]

GIT-base (synthetic weights), 6 frames per clip, max_len = 20, stop = never, B = 1 and B = 16.  HIP events, p50 of `--reps` calls
after two warm-up calls, every call followed by a synchronisation.  Per batch size:
  image   forward_image_enc alone: the image pass every case below contains;
  plain   greedy_decode without a draft -- the yardstick; token loop = plain - image;
  whole   the draft is the plain caption: accepted whole, verify pass only;
  pos1    every row wrong at position 1: nothing accepted, the price of a useless verify pass;
  mid     every row wrong at position 10;
  ragged  row b wrong at position 1 + (5 b) % 19: the tail starts at the worst row's position.
Each case's ids are checked against the plain caption.  "loop" = the case's time - image."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def p50(fn, n, warm=2):
    ms = []
    for i in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    from oracle.git_oracle import make_frames

    F, L = 6, 20
    cfg = git_base(F)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=16, max_frames=F, max_text_len=L, stop="never")
    V = cfg.vocab_size
    for B in (1, 16):
        fr = make_frames(B, F, cfg.image_size, 11).cuda()
        cap = m.greedy_decode(fr, max_len=L)

        def wrong(cols):
            d = cap.clone()
            for b, c in enumerate(cols):
                d[b, c] = (d[b, c] + 1) % V
            return d

        drafts = dict(whole=cap, pos1=wrong([1] * B), mid=wrong([10] * B), ragged=wrong([1 + (5 * b) % 19 for b in range(B)]))
        image = p50(lambda: m.forward_image_enc(fr), args.reps)
        plain = p50(lambda: m.greedy_decode(fr, max_len=L), args.reps)
        print(f"B = {B:2d} x {F} frames: image pass {image:.3f} ms; plain call {plain:.3f} ms, token loop {plain - image:.3f} ms")
        for name, d in drafts.items():
            assert torch.equal(m.greedy_decode(fr, max_len=L, draft=d), cap), name
            acc = m.last_accepted.tolist()
            before = m.draft_stats()
            t = p50(lambda: m.greedy_decode(fr, max_len=L, draft=d), args.reps)
            tail = (m.draft_stats()[3] - before[3]) // (args.reps + 2)
            print(f"    {name:6s} call {t:.3f} ms, loop {t - image:.3f} ms = {100 * (t - image) / (plain - image):5.1f} % of the plain loop; "
                  f"accepted min {min(acc)} / max {max(acc)} of {L}, tail steps {tail}")


if __name__ == "__main__":
    main()
