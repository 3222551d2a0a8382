#!/usr/bin/env python3
"""What sampling on the device costs (its output is meant for docs/LAB_NOTEBOOK.md and profiles/).

    python tools/sampling_bench.py [--calls 12] [--reps 3] [--batch 16] [--pipelined] [--rows-only]

1. Per step, at the BASELINE configs[4] shape (B = 16, beams 4, V = 30522; 64 rows): the gitcap_sample_rows launch against the
   gitcap_beam_topk launch pair it replaces, on Gaussian logits; HIP events around `--calls` back-to-back calls, p50 and min..max over
   `--reps` repetitions, the variants alternating.
2. The whole search (GIT-large, B clips x 10 frames, beam 4, 15 steps, e4m3-valued weights), sampled against unsampled, as
   tools/search_options_bench.py measures the search options: p50 per batch, difference from plain, spread of the plain p50."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

VARIANTS = (("plain", {}), ("sample", dict(do_sample=True, seed=1)), ("top_k50", dict(do_sample=True, seed=1, top_k=50)),
            ("top_p0.9", dict(do_sample=True, seed=1, top_p=0.9)))
ROW_VARIANTS = (("beam_topk", None), ("sample", (0, 1.0)), ("top_k50", (50, 1.0)), ("top_p0.9", (0, 0.9)))


def rows_bench(args):
    import ctypes
    from gitcap import _lib
    lib = _lib.load()
    B, beams, V, pn = 16, 4, 30522, 2
    K = beams * pn
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B * beams, V, generator=g) * 2).cuda()
    bs = torch.zeros(B * beams, device="cuda")
    out_s, out_i = torch.empty(B * K, device="cuda"), torch.empty(B * K, device="cuda", dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(v):
        if v is None:
            rc = lib.gitcap_beam_topk(p(x), V, p(bs), B, beams, V, K, p(out_s), p(out_i), st)
        else:
            rc = lib.gitcap_sample_rows(p(x), V, p(bs), None, 0, 1, ctypes.c_float(1.0), B, beams, V, pn, ctypes.c_float(1.0), v[0],
                                        ctypes.c_float(v[1]), ctypes.c_uint64(1), p(out_s), p(out_i), None, None, st)
        assert rc == 0, rc

    res = {name: [] for name, _ in ROW_VARIANTS}
    for name, v in ROW_VARIANTS:
        for _ in range(args.warmup):
            call(v)
    for _ in range(args.reps):
        for name, v in ROW_VARIANTS:
            res[name].append(1e3 * event_ms(lambda: [call(v) for _ in range(args.calls)]) / args.calls)
    for name, _ in ROW_VARIANTS:
        t = res[name]
        print(f"rows, 64 x 30522: {name}: p50 {statistics.median(t):.1f} us per step ({min(t):.1f} .. {max(t):.1f} over {len(t)} repetitions)")
    print(json.dumps({"rows_us": {k: [round(x, 2) for x in v] for k, v in res.items()}}))


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--pipelined", action="store_true")
    ap.add_argument("--rows-only", action="store_true")
    args = ap.parse_args()
    rows_bench(args)
    if args.rows_only:
        return
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
    assert torch.equal(m.infer_async(x, **kw, **VARIANTS[3][1]).result()["predictions"], want["top_p0.9"])
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
