#!/usr/bin/env python3
"""Sixteen cameras on one teacher: the stream pool against what a caller could do without it (its output is meant for
profiles/r30_teacher_pool_bench.txt).

    python tools/teacher_pool_bench.py [--calls 5] [--warmup 2] [--seed 0] [--ticks 8] [--lead 6]

GIT-base with windows of F = 6 frames, 16 cameras of 480x640 uint8 frames on the device, 20-token greedy captions.  Per
tick every camera contributes 0 or 1 admitted frame from a fixed seeded pattern (as behind per-camera scene-change gates), so the
cameras' windows sit at different fill levels and ring positions; every camera that got a frame is captioned (hop = 1,
min_frames = 1).  `--lead` ticks fill the windows unmeasured, then `--ticks` ticks are timed, three ways:
  (a) pool         one pool.push per tick: the admitted frames are encoded once, the due cameras captioned as one ragged batch
  (b) re-send      greedy_decode on the list of every due camera's whole window: every frame of a window is encoded again
  (c) one by one   the same, camera by camera
HIP events around every tick; a call is the sum over the timed ticks; p50 of `--calls` after `--warmup` unrecorded ones, the ways
alternating.  The encoder's share is measured on its own: one push that captions nothing (the packed encoder pass and the scatter)
of the frames (a) encodes per tick on average, and of the frames (b) does."""
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
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ticks", type=int, default=8)
    ap.add_argument("--lead", type=int, default=6)
    args = ap.parse_args()
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    C, L, F = 16, 20, 6
    cfg = git_base(F)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=C, max_frames=F, max_text_len=L + 1, stop="never")
    g = torch.Generator().manual_seed(args.seed)
    T = args.lead + args.ticks
    admit = torch.rand(T, C, generator=g) < 0.5                       # the fixed pattern: camera c has a frame at tick t
    admit[:, 0] = True                                                  # one camera whose gate admits everything ...
    admit[:args.lead, 1] = False                                        # ... and one that starts late
    admit[-1, :] |= ~admit[args.lead:].any(0)                           # every camera appears in the timed part
    frames = torch.randint(0, 256, (T, C, 480, 640, 3), dtype=torch.uint8, generator=g).cuda()
    ticks = [[c for c in range(C) if admit[t, c]] for t in range(T)]

    def windows_upto(t):
        """camera -> its last (up to F) admitted frames behind tick t"""
        return {c: [frames[u, c] for u in range(t + 1) if admit[u, c]][-F:] for c in range(C)}
    wins = [windows_upto(t) for t in range(T)]
    batches = [frames[t, cams].contiguous() if cams else None for t, cams in enumerate(ticks)]     # a tick's admitted frames, packed

    def run_pool():
        pool = m.stream_pool(C, frames=F, hop=1, max_len=L, min_frames=1)
        ms, outs = 0.0, []
        for t, cams in enumerate(ticks):
            if not cams:
                continue
            dt, out = timed(lambda: pool.push(batches[t], cams))
            if t >= args.lead:
                ms += dt
                outs.append(out)
        return ms, outs

    def run_resend(one_by_one):
        ms, outs = 0.0, []
        for t in range(args.lead, T):
            cams = ticks[t]
            if not cams:
                continue
            clips = [torch.stack(wins[t][c], 0) for c in cams]
            if one_by_one:
                dt, out = timed(lambda: [m.greedy_decode([cl], max_len=L) for cl in clips])
                out = torch.cat(out, 0)
            else:
                dt, out = timed(lambda: m.greedy_decode(clips, max_len=L))
            ms += dt
            outs.append(dict(zip(cams, out)))
        return ms, outs

    ways = [("(a) pool", run_pool), ("(b) re-send windows", lambda: run_resend(False)), ("(c) one by one", lambda: run_resend(True))]
    ref = [fn()[1] for _, fn in ways]
    for other in ref[1:]:
        assert len(other) == len(ref[0])
        for x, y in zip(ref[0], other):
            assert sorted(x) == sorted(y) and all(torch.equal(x[c], y[c]) for c in x), "a camera's caption differs between the ways"
    timed_ticks = [t for t in range(args.lead, T) if ticks[t]]
    n_cap = sum(len(ticks[t]) for t in timed_ticks)
    enc_a = n_cap
    enc_b = sum(len(wins[t][c]) for t in timed_ticks for c in ticks[t])
    print(f"tools/teacher_pool_bench.py --calls {args.calls} --warmup {args.warmup} --seed {args.seed} --ticks {args.ticks} --lead {args.lead} "
          f"on {torch.cuda.get_device_name(0)}")
    print(f"GIT-base, windows of {F} frames, {C} cameras, 480x640 uint8 frames on the device, {L}-token greedy captions, stop = never; "
          f"{len(timed_ticks)} timed ticks behind {args.lead} unmeasured ones: {n_cap} captions; frames encoded (a) {enc_a}, (b) and (c) {enc_b}; "
          f"fill levels at the first timed tick {[len(wins[args.lead][c]) for c in range(C)]}; the three ways' ids are equal")
    t = {name: [] for name, _ in ways}
    for i in range(args.warmup + args.calls):
        for name, fn in ways:                                           # alternate
            ms = fn()[0]
            if i >= args.warmup:
                t[name].append(ms)
    p50 = {name: statistics.median(v) for name, v in t.items()}
    for name, _ in ways:
        print(f"   {name:22s} p50 {p50[name]:9.3f} ms over the timed ticks   min {min(t[name]):9.3f}   max {max(t[name]):9.3f}   "
              f"{p50[name] / n_cap:7.3f} ms per caption   {p50[name] / len(timed_ticks):8.3f} ms per tick")
    print(f"   (a) / (b) = {p50['(a) pool'] / p50['(b) re-send windows']:.3f}   (a) / (c) = {p50['(a) pool'] / p50['(c) one by one']:.3f}   "
          f"(b) - (a) = {p50['(b) re-send windows'] - p50['(a) pool']:.3f} ms")
    # the encoder's share: one push that captions nothing (hop beyond reach), at the mean number of frames each way encodes per tick
    na, nb = max(1, round(enc_a / len(timed_ticks))), min(C * F, max(1, round(enc_b / len(timed_ticks))))
    flat = frames.view(T * C, 480, 640, 3)
    quiet = m.stream_pool(C, frames=F, hop=10 ** 9, max_len=L)
    e = {}
    for n in (na, nb):
        v = [timed(lambda: quiet.push(flat[:n], [i % C for i in range(n)]))[0] for _ in range(args.warmup + args.calls)][args.warmup:]
        e[n] = statistics.median(v)
    print(f"   encoder alone (a push that captions nothing: one packed pass and the scatter): {na} frames {e[na]:.3f} ms, {nb} frames {e[nb]:.3f} ms: per tick (b) encodes "
          f"{e[nb] - e[na]:.3f} ms more than (a), {(e[nb] - e[na]) * len(timed_ticks):.3f} ms over the timed ticks", flush=True)


if __name__ == "__main__":
    main()
