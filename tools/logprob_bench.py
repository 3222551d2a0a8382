#!/usr/bin/env python3
"""What asking for per-token log-probabilities costs on the two greedy paths (its output is meant for
profiles/r10_token_logprobs.txt).

    python tools/logprob_bench.py [--calls 40] [--reps 3] [--skip-teacher] [--skip-student]

In one process, after a warm-up, p50 over `--calls` calls each, HIP-event and wall time (wall includes the synchronisation),
attached (logprobs=True / return_logprobs=True) against not attached, alternating, repeated `--reps` times to show the spread:
  student: B = 1, 480x640 camera frames on the device, student 21m (synthetic weights), hop = 1, max_len = 25, stop = never --
           one window push per call (encoder + 25 token steps);
  teacher: GIT-base, 16 clips x 6 frames x 20 tokens, one synchronous greedy_decode per call (image pass + 20 token steps).
Every attached call returns the ids of the plain one (asserted).  Reported: the added time per caption and per token step."""
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
    """p50 (event ms, wall ms) of n calls of fn() after `warm` unrecorded ones; each call is followed by a synchronisation."""
    ev, wall = [], []
    for i in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warm:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return statistics.median(ev), statistics.median(wall)


def report(name, rows, captions, steps):
    for k, what in ((0, "HIP events"), (1, "wall")):
        off = statistics.median(r["off"][k] for r in rows)
        on = statistics.median(r["on"][k] for r in rows)
        spread = max(r["off"][k] for r in rows) - min(r["off"][k] for r in rows)
        add = on - off
        print(f"{name} {what}: not attached {off:.3f} ms, attached {on:.3f} ms, added {add:+.3f} ms per call = {100 * add / off:+.2f} % "
              f"= {1e3 * add / captions:+.2f} us per caption = {1e3 * add / steps:+.2f} us per token step; spread of the not-attached "
              f"p50 over {len(rows)} repetitions {spread:.3f} ms")


def student(args):
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights
    tcfg, scfg = tinyvit_config("tiny_vit_21m_224"), student_base()
    weights = dict(student_synthetic_weights(scfg, 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=scfg.mem_tokens)
    m = StudentCaptioner(cfg=scfg, weights=weights, image_encoder=enc, device="cuda:0", max_batch=1, max_text_len=25, stop="never")
    F, L = scfg.mem_tokens, 25
    frame = torch.randint(0, 256, (1, 480, 640, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    rows = []
    for rep in range(args.reps):
        row, caps = {}, {}
        for key, lp in (("off", False), ("on", True)):           # one live stream per model: fill, measure, then the other
            st = m.caption_stream(batch=1, hop=1, max_len=L, stop="never", logprobs=lp)
            for _ in range(F):
                caps[key] = st.push(frame)
            outs = []
            row[key] = timed(lambda: outs.append(st.push(frame)), args.calls, args.warmup)
            assert all(torch.equal(o, caps[key]) for o in outs)
        assert torch.equal(caps["on"], caps["off"])
        rows.append(row)
        print(f"student rep {rep}: p50 ms (HIP events / wall)  " + "   ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in row.items()), flush=True)
    report("student B=1, 25-token window push", rows, 1, L)
    return rows


def teacher(args):
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    from oracle.git_oracle import make_frames
    B, Fr, L = 16, 6, 20
    cfg = git_base(Fr)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=B, max_frames=Fr, max_text_len=L, stop="never")
    x = make_frames(B, Fr, cfg.image_size, 1234).cuda()
    want = m.greedy_decode(x, max_len=L).clone()
    rows = []
    for rep in range(args.reps):
        row = {}
        for key, lp in (("off", False), ("on", True)):
            outs = []
            row[key] = timed(lambda: outs.append(m.greedy_decode(x, max_len=L, return_logprobs=lp)), args.calls, args.warmup)
            assert all(torch.equal(o[0] if lp else o, want) for o in outs)
        rows.append(row)
        print(f"teacher rep {rep}: p50 ms (HIP events / wall)  " + "   ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in row.items()), flush=True)
    report("teacher 16 clips x 6 frames x 20 tokens, synchronous", rows, B, L)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--skip-teacher", action="store_true")
    ap.add_argument("--skip-student", action="store_true")
    args = ap.parse_args()
    out = {"calls": args.calls, "reps": args.reps}
    for name, fn, skip in (("student", student, args.skip_student), ("teacher", teacher, args.skip_teacher)):
        if not skip:
            out[name] = [{k: [round(v, 4) for v in r[k]] for k in r} for r in fn(args)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
