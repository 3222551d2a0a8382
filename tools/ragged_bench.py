#!/usr/bin/env python3
"""What a ragged batch saves (its output is meant for profiles/r22_ragged_bench.txt).

    python tools/ragged_bench.py [--calls 5] [--warmup 2] [--seed 0]

GIT-base, sixteen clips whose frame counts are drawn once from 2..6 (seeded; the total is printed), a 20-step greedy caption
(image pass included), three ways:
  (a) ragged     one call with frame_counts: the packed batch, no padding
  (b) one by one sixteen calls, each clip alone
  (c) padded     every clip padded to six frames by repeating its last frame, one dense call (other captions: more frames)
HIP events around each way, p50 of `--calls` after `--warmup` unrecorded ones, the three alternating."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    cfg, B, Fmax, L = git_base(6), 16, 6, 20
    g = torch.Generator().manual_seed(args.seed)
    counts = torch.randint(2, Fmax + 1, (B,), generator=g).tolist()
    clips = [torch.randn(n, 3, cfg.image_size, cfg.image_size, generator=g).cuda() for n in counts]
    padded = torch.stack([torch.cat([c, c[-1:].expand(Fmax - c.shape[0], -1, -1, -1)], 0) for c in clips]).contiguous()
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=B, max_frames=Fmax, max_text_len=L + 1, max_beams=1, stop="never")
    ways = [("(a) ragged", lambda: m.greedy_decode(clips, max_len=L)),
            ("(b) one by one", lambda: [m.greedy_decode(c[None], max_len=L) for c in clips]),
            ("(c) padded to 6", lambda: m.greedy_decode(padded, max_len=L))]
    ra, rb = ways[0][1](), torch.cat(ways[1][1](), 0)
    assert torch.equal(ra, rb), "a clip of the ragged batch differs from the clip alone"
    t = {name: [] for name, _ in ways}
    for i in range(args.warmup + args.calls):
        for name, fn in ways:                                  # alternate
            ms = timed(fn)
            if i >= args.warmup:
                t[name].append(ms)
    print(f"tools/ragged_bench.py --calls {args.calls} --warmup {args.warmup} --seed {args.seed} on {torch.cuda.get_device_name(0)}")
    print(f"GIT-base, {B} clips, frame counts {counts}: {sum(counts)} frames in all ({B * Fmax} when padded to {Fmax}), "
          f"{L}-step greedy caption, image pass included; ids of (a) == ids of (b)")
    p50 = {name: statistics.median(v) for name, v in t.items()}
    for name, _ in ways:
        print(f"   {name:16s} p50 {p50[name]:8.3f} ms   min {min(t[name]):8.3f}   max {max(t[name]):8.3f}")
    print(f"   (a) / (b) = {p50['(a) ragged'] / p50['(b) one by one']:.3f}   (a) / (c) = {p50['(a) ragged'] / p50['(c) padded to 6']:.3f}   "
          f"frames (a) / (c) = {sum(counts) / (B * Fmax):.3f}", flush=True)


if __name__ == "__main__":
    main()
