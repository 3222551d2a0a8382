#!/usr/bin/env python3
"""What the scene-change gate costs and saves on the live student path (profiles/r09_frame_gate.txt).

    python tools/frame_gate_bench.py [--pushes 60] [--reps 3] [--metric mse]

B = 1, 480x640 camera frames on the device, student 21m (synthetic weights), hop = 1, max_len = 25, stop = never.  In one
process, after a warm-up, p50 over `--pushes` pushes each, HIP-event and wall time (wall includes the synchronisation):
  (a) an ungated push that encodes and captions -- the yardstick, the code path without a gate;
  (b) a gated push that is admitted (a changing scene: every frame new);
  (c) a gated push that is rejected (the camera looks at a wall: the same frame again);
  (d) gitcap_frame_change alone (one output, no host read).
Repeated `--reps` times; the run-to-run spread of (a) is what (b) - (a) and (a) - (c) are held against: a difference inside
it is reported as "not resolved"."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, n, warm):
    """p50 (event ms, wall ms) of n calls of fn(i) after `warm` unrecorded ones; each call is followed by a synchronisation."""
    ev, wall = [], []
    for i in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn(i)
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warm:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return statistics.median(ev), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--metric", default="mse", choices=("mse", "hist"))
    args = ap.parse_args()

    from gitcap.framegate import METRICS, FrameGate, frame_change
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights

    tcfg, scfg = tinyvit_config("tiny_vit_21m_224"), student_base()
    weights = dict(student_synthetic_weights(scfg, 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=scfg.mem_tokens)
    m = StudentCaptioner(cfg=scfg, weights=weights, image_encoder=enc, device="cuda:0", max_batch=1, max_text_len=25, stop="never")
    F = scfg.mem_tokens
    pool = torch.randint(0, 256, (16, 1, 480, 640, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    threshold = 100.0 if args.metric == "mse" else 20.0     # random frames are ~1e4 (mse) / ~1e3 (hist) apart, a repeat is at 0

    def filled(gate):
        st = m.caption_stream(batch=1, hop=1, max_len=25, stop="never", gate=gate)
        for i in range(F):
            st.push(pool[i])
        return st

    rows = []
    for rep in range(args.reps):
        st = filled(None)
        a = timed(lambda i: st.push(pool[i % 16]), args.pushes, args.warmup)
        gate = FrameGate(args.metric, threshold)
        st = filled(gate)
        b = timed(lambda i: st.push(pool[(F + i) % 16]), args.pushes, args.warmup)
        assert gate.stats["admitted"] == gate.stats["pushed"], gate.stats
        gate = FrameGate(args.metric, threshold)
        st = filled(gate)
        same = pool[F - 1]
        outs = []
        c = timed(lambda i: outs.append(st.push(same)), args.pushes, args.warmup)
        assert all(o is None for o in outs) and gate.stats["admitted"] == F, gate.stats
        key = METRICS[args.metric]
        d = timed(lambda i: frame_change(pool[i % 16], pool[(i + 1) % 16], 2, outputs=(key,)), args.pushes, args.warmup)
        rows.append(dict(a=a, b=b, c=c, d=d))
        print(f"rep {rep}: p50 ms (HIP events / wall)  (a) ungated push {a[0]:.3f} / {a[1]:.3f}   (b) gated, admitted {b[0]:.3f} / {b[1]:.3f}"
              f"   (c) gated, rejected {c[0]:.3f} / {c[1]:.3f}   (d) frame_change alone {d[0]:.3f} / {d[1]:.3f}", flush=True)

    for k, what in ((0, "HIP events"), (1, "wall")):
        med = {x: statistics.median(r[x][k] for r in rows) for x in "abcd"}
        spread = max(r["a"][k] for r in rows) - min(r["a"][k] for r in rows)
        price, saved = med["b"] - med["a"], med["a"] - med["c"]
        res = lambda v: "resolved" if abs(v) > spread else "not resolved"
        print(f"{what}: (a) {med['a']:.3f} ms, spread of (a) over {args.reps} repetitions {spread:.3f} ms; "
              f"(b) - (a) = {price:+.3f} ms = {100 * price / med['a']:+.1f} % of (a) [{res(price)}]; "
              f"(c) = {med['c']:.3f} ms, (a) - (c) = {saved:.3f} ms [{res(saved)}]; (d) = {med['d']:.3f} ms")
    print(json.dumps({"metric": args.metric, "pushes": args.pushes, "reps": args.reps,
                      "p50_ms_event_wall": [{k: [round(x, 4) for x in v] for k, v in r.items()} for r in rows]}))


if __name__ == "__main__":
    main()
