#!/usr/bin/env python3
"""What the options of the device-resident search cost (its output is meant for docs/LAB_NOTEBOOK.md).

    python tools/search_options_bench.py [--calls 12] [--reps 3] [--batch 4] [--pipelined]

The BASELINE configs[4] shape: GIT-large, B clips x 10 frames, beam 4, 15 steps, e4m3-valued weights.  In one process, after a
warm-up, p50 over `--calls` batches each (HIP events; one synchronous infer per batch, or with --pipelined three infer_async in
flight and the time per batch of a run of `--calls` batches), the four variants alternating, repeated `--reps` times:
  plain                     no attachment: the launches of a handle that never attached;
  rp = 1.3                  the penalised chunk kernel in place of the plain one, 14 launches;
  n = 4                     the n-best step and finish kernels in place of the one-hypothesis ones;
  rp = 1.3, n = 4           both.
Reported: each variant's p50 per batch, its difference from plain, and the spread of the plain p50 over the repetitions."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

VARIANTS = (("plain", {}), ("rp1.3", dict(repetition_penalty=1.3)), ("n4", dict(num_keep_best=4)),
            ("rp1.3+n4", dict(repetition_penalty=1.3, num_keep_best=4)))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--pipelined", action="store_true")
    args = ap.parse_args()
    from gitcap.config import git_large
    from gitcap.model import GitCaptioner
    from gitcap.weights import quantize_weights_fp8, synthetic_weights
    B, beams, steps = args.batch, 4, 15
    cfg = git_large(10)
    m = GitCaptioner(cfg, quantize_weights_fp8(synthetic_weights(cfg, seed=0)), device="cuda:0", max_batch=B, max_frames=10,
                     max_text_len=20, max_beams=beams, weight_dtype="fp8_e4m3")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 10, 3, cfg.image_size, cfg.image_size, generator=g).cuda()
    kw = dict(beam_size=beams, max_steps=steps)

    def sync_call(opt):
        return lambda: m.infer(x, **kw, **opt)

    def pipe_run(opt):
        def run():
            pend = []
            for _ in range(args.calls):
                pend.append(m.infer_async(x, **kw, **opt))
                if len(pend) == 3:
                    pend.pop(0).result()
            while pend:
                pend.pop(0).result()
        return run

    want = {name: m.infer(x, **kw, **opt)["predictions"].clone() for name, opt in VARIANTS}       # (also the first attach: allocation)
    assert torch.equal(m.infer_async(x, **kw, **VARIANTS[3][1]).result()["predictions"], want["rp1.3+n4"])
    rows = []
    for rep in range(args.reps):
        row = {}
        for name, opt in VARIANTS:
            if args.pipelined:
                pipe_run(opt)()
                row[name] = statistics.median(event_ms(pipe_run(opt)) / args.calls for _ in range(3))
            else:
                fn = sync_call(opt)
                for _ in range(args.warmup):
                    fn()
                row[name] = statistics.median(event_ms(fn) for _ in range(args.calls))
        rows.append(row)
        print(f"rep {rep}: p50 ms per batch  " + "   ".join(f"{k} {v:.3f}" for k, v in row.items()), flush=True)
    assert torch.equal(m.infer(x, **kw)["predictions"], want["plain"])
    plain = [r["plain"] for r in rows]
    spread = max(plain) - min(plain)
    base = statistics.median(plain)
    mode = "three batches in flight" if args.pipelined else "one batch at a time"
    print(f"configs[4] shape, B = {B}, {mode}: plain {base:.3f} ms per batch = {1e3 * B / base:.1f} captions/s; spread of the plain p50 over "
          f"{len(rows)} repetitions {spread:.3f} ms")
    for name, _ in VARIANTS[1:]:
        v = statistics.median(r[name] for r in rows)
        print(f"  {name}: {v:.3f} ms per batch, {v - base:+.3f} ms = {100 * (v - base) / base:+.2f} % = {1e3 * (v - base) / (steps - 1):+.1f} us per "
              f"search step")
    print(json.dumps({"batch": B, "pipelined": args.pipelined, "calls": args.calls,
                      "rows": [{k: round(v, 4) for k, v in r.items()} for r in rows]}))


if __name__ == "__main__":
    main()
