#!/usr/bin/env python3
"""What a ragged batch saves on the student, and how soon a live stream shows its first caption (its output is meant for
profiles/r27_student_ragged_bench.txt).

    python tools/student_ragged_bench.py [--calls 5] [--warmup 2] [--seed 0]

1. The base student with its native TinyViT encoder, sixteen clips whose frame counts are drawn once from 2..6 (seeded), a 25-token
   greedy caption (encoder included), three ways:
     (a) ragged      one call on the list of clips: packed, no padding
     (b) one by one  sixteen calls, each clip alone
     (c) padded      every clip padded to six frames by repeating its last frame, one dense call (other captions: more frames)
2. One live stream (B = 1, hop = 1, no gate): the time from the push of the first frame after a reset to the first caption, with
   partial=True (one push) and partial=False (six pushes; frames arrive back to back, so this is the compute only -- at a camera's
   frame interval dt the full window adds 5 dt of waiting that partial=True does not have).
HIP events around each way, p50 of `--calls` after `--warmup` unrecorded ones, the ways alternating."""
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


def series(ways, calls, warmup):
    t = {name: [] for name, _ in ways}
    for i in range(warmup + calls):
        for name, fn in ways:                                  # alternate
            ms = timed(fn)
            if i >= warmup:
                t[name].append(ms)
    p50 = {name: statistics.median(v) for name, v in t.items()}
    for name, _ in ways:
        print(f"   {name:22s} p50 {p50[name]:8.3f} ms   min {min(t[name]):8.3f}   max {max(t[name]):8.3f}")
    return p50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights
    scfg, tcfg, B, L = student_base(), tinyvit_config("tiny_vit_21m_224"), 16, 25
    Fmax, S = scfg.mem_tokens, tcfg.img_size
    w = dict(student_synthetic_weights(scfg, 0))
    w.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=B * Fmax)
    m = StudentCaptioner(cfg=scfg, weights=w, image_encoder=enc, device="cuda:0", max_batch=B, max_text_len=L + 1, stop="never")
    g = torch.Generator().manual_seed(args.seed)
    counts = torch.randint(2, Fmax + 1, (B,), generator=g).tolist()
    clips = [torch.randn(n, 3, S, S, generator=g).cuda() for n in counts]
    padded = torch.stack([torch.cat([c, c[-1:].expand(Fmax - c.shape[0], -1, -1, -1)], 0) for c in clips]).contiguous()
    ways = [("(a) ragged", lambda: m.greedy_decode(clips, max_len=L)),
            ("(b) one by one", lambda: [m.greedy_decode([c], max_len=L) for c in clips]),
            ("(c) padded to 6", lambda: m.greedy_decode(padded, max_len=L))]
    ra, rb = ways[0][1](), torch.cat(ways[1][1](), 0)
    assert torch.equal(ra, rb), "a clip of the ragged batch differs from the clip alone"
    print(f"tools/student_ragged_bench.py --calls {args.calls} --warmup {args.warmup} --seed {args.seed} on {torch.cuda.get_device_name(0)}")
    print(f"base student + TinyViT-21M, {B} clips, frame counts {counts}: {sum(counts)} frames in all ({B * Fmax} when padded to {Fmax}), "
          f"{L}-token greedy caption, encoder included; ids of (a) == ids of (b)")
    p50 = series(ways, args.calls, args.warmup)
    print(f"   (a) / (b) = {p50['(a) ragged'] / p50['(b) one by one']:.3f}   (a) / (c) = {p50['(a) ragged'] / p50['(c) padded to 6']:.3f}   "
          f"frames (a) / (c) = {sum(counts) / (B * Fmax):.3f}")
    frames = torch.randint(0, 256, (Fmax, 1, 480, 640, 3), dtype=torch.uint8, generator=g).cuda()

    def first_caption(partial):
        stream = m.caption_stream(batch=1, hop=1, max_len=L, partial=partial)

        def run():
            stream.reset()
            for f in frames:
                if stream.push(f) is not None:
                    return
            raise AssertionError("no caption after a full window")
        return run
    print(f"live stream, B = 1, 480x640 uint8 frames on the device, hop = 1: reset -> first {L}-token caption, frames pushed back to back")
    live = [("partial=True  (1 push)", True), ("partial=False (6 pushes)", False)]
    t = {name: [] for name, _ in live}
    for name, partial in live:                                 # one live stream per model: each way opens its own, in turn
        run = first_caption(partial)
        for i in range(args.warmup + args.calls):
            ms = timed(run)
            if i >= args.warmup:
                t[name].append(ms)
    for name, _ in live:
        print(f"   {name:26s} p50 {statistics.median(t[name]):8.3f} ms   min {min(t[name]):8.3f}   max {max(t[name]):8.3f}", flush=True)


if __name__ == "__main__":
    main()
