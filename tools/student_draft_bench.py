#!/usr/bin/env python3
"""What carrying the previous caption as a draft costs and saves on the live student path (its output is meant for
profiles/r10_student_draft.txt).

    python tools/student_draft_bench.py [--pushes 60] [--reps 3] [--plain-only]

B = 1, 480x640 camera frames on the device, student 21m (synthetic weights), hop = 1, max_len = 25, stop = never.  In one
process, after a warm-up, p50 over `--pushes` pushes each, HIP-event and wall time (wall includes the synchronisation).  Every
case pushes the same frame (a static scene), so the four differ in the decode only:
  (a) carry=False: the token loop from [CLS] for every caption -- the yardstick, the code path without a draft;
  (b) carry=True: the draft is the caption itself, accepted whole: encoder + one verify pass;
  (c) carry=True with the draft forced wrong at position 1: nothing accepted, the price of a useless verify pass;
  (d) carry=True with the draft forced wrong at position 13: half a loop behind the pass.
Repeated `--reps` times; the run-to-run spread of (a) is what (c) - (a) is held against, next to one token step's worth
(1/25 of the token loop of (a), the loop taken as (a) - (b) + one pass ~ (a) - (b)).  --plain-only runs (a) alone: the form that
also runs on a commit without `carry`, to show that the plain path did not move."""
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
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()

    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights

    tcfg, scfg = tinyvit_config("tiny_vit_21m_224"), student_base()
    weights = dict(student_synthetic_weights(scfg, 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=scfg.mem_tokens)
    m = StudentCaptioner(cfg=scfg, weights=weights, image_encoder=enc, device="cuda:0", max_batch=1, max_text_len=25, stop="never")
    F, L, V = scfg.mem_tokens, 25, scfg.vocab_length
    frame = torch.randint(0, 256, (1, 480, 640, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()

    def filled(**kw):
        st = m.caption_stream(batch=1, hop=1, max_len=L, stop="never", **kw)
        for _ in range(F):
            cap = st.push(frame)
        return st, cap

    def wrong_at(cap, col):
        d = cap.clone()
        d[:, col] = (d[:, col] + 1) % V
        return d

    rows = []
    for rep in range(args.reps):
        st, cap = filled()
        outs = []
        row = dict(a=timed(lambda i: outs.append(st.push(frame)), args.pushes, args.warmup))
        assert all(torch.equal(o, cap) for o in outs)
        if not args.plain_only:
            for key, col, accepted in (("b", None, L), ("c", 1, 0), ("d", 13, 12)):
                st, cap2 = filled(carry=True)
                assert torch.equal(cap2, cap)
                draft = cap if col is None else wrong_at(cap, col)
                outs = []

                def push(i):
                    st._prev = draft                                   # the draft this case is about, whatever the last caption was
                    outs.append(st.push(frame))
                    assert st.stats()["last"]["accepted"] == accepted, st.stats()

                row[key] = timed(push, args.pushes, args.warmup)
                assert all(torch.equal(o, cap) for o in outs)          # the same caption in every case
        rows.append(row)
        print(f"rep {rep}: p50 ms (HIP events / wall)  " + "   ".join(f"({k}) {v[0]:.3f} / {v[1]:.3f}" for k, v in row.items()), flush=True)

    for k, what in ((0, "HIP events"), (1, "wall")):
        med = {x: statistics.median(r[x][k] for r in rows) for x in rows[0]}
        spread = max(r["a"][k] for r in rows) - min(r["a"][k] for r in rows)
        line = f"{what}: (a) {med['a']:.3f} ms, spread of (a) over {args.reps} repetitions {spread:.3f} ms"
        if not args.plain_only:
            step = (med["a"] - med["b"]) / L
            price = med["c"] - med["a"]
            verdict = "inside the spread" if abs(price) <= spread else (
                "outside the spread by less than one token step" if abs(price) - spread <= step else "outside the spread by MORE than one token step")
            line += (f"; (b) {med['b']:.3f} ms = {100 * med['b'] / med['a']:.1f} % of (a); (c) {med['c']:.3f} ms, (c) - (a) = {price:+.3f} ms = "
                     f"{100 * price / med['a']:+.1f} % of (a) [{verdict}; one token step ~ {step:.3f} ms]; "
                     f"(d) {med['d']:.3f} ms = {100 * med['d'] / med['a']:.1f} % of (a)")
        print(line)
    print(json.dumps({"pushes": args.pushes, "reps": args.reps, "plain_only": args.plain_only,
                      "p50_ms_event_wall": [{k: [round(x, 4) for x in v] for k, v in r.items()} for r in rows]}))


if __name__ == "__main__":
    main()
