#!/usr/bin/env python3
"""What hard constraints cost (its output is meant for profiles/r21_constraints_bench.txt).

    python tools/constraints_bench.py [--calls 5] [--warmup 2] [--skip-large]

GIT-base, 16 clips x 6 frames, a 20-step greedy caption (greedy_decode, image pass included), alternating
  unattached        20 token steps
  attached          no_repeat_ngram_size = 3, min_length = 8, 16 suppressed ids: per step one ban-mask launch more and the BAN
                    form of the vocabulary head
and the image pass alone (forward_image_enc), so that the token loops can be told apart from it.  Then the configs[4] beam
shape (GIT-large, 10-frame clips, 16 clips, beam 4, 15 steps) with and without the same constraints: per ranked step one
ban-mask launch over the 64 beam rows and the BAN form of the chunk kernel.  HIP events, p50 of `--calls` calls after
`--warmup` unrecorded ones."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from prompt_bench import make, p50_events  # noqa: E402

CONS = dict(no_repeat_ngram_size=3, min_length=8, suppress_tokens=list(range(1, 17)))


def greedy(args):
    from gitcap.config import git_base
    cfg, B, L = git_base(6), 16, 20
    m, x = make(cfg, B, 6, L + 1, 1)
    cases = [("unattached", lambda: m.greedy_decode(x, max_len=L)),
             ("attached", lambda: m.greedy_decode(x, max_len=L, **CONS)),
             ("image pass alone", lambda: m.forward_image_enc(x))]
    t = {}
    for _ in range(2):                                                           # alternate
        for name, fn in cases:
            t[name] = p50_events(fn, args.calls, args.warmup)
    print(f"GIT-base, {B} clips x 6 frames, {L}-step greedy caption (image pass included)")
    for name, _ in cases:
        print(f"   {name:18s} p50 {t[name]:8.3f} ms   token loop {t[name] - t['image pass alone']:8.3f} ms")
    print(f"   attached / unattached: {t['attached'] / t['unattached']:.3f} of the call, "
          f"{(t['attached'] - t['image pass alone']) / (t['unattached'] - t['image pass alone']):.3f} of the token loop", flush=True)
    del m


def beam(args):
    from gitcap.config import git_large
    cfg, B, L = git_large(10), 16, 15
    m, x = make(cfg, B, 10, L, 4)
    kw = dict(beam_size=4, max_steps=L, length_penalty=0.6, per_node_beam_size=2, on_device=True)
    cases = [("unattached", lambda: m.infer(x, **kw)), ("attached", lambda: m.infer(x, **kw, **CONS))]
    t = {}
    for _ in range(2):
        for name, fn in cases:
            t[name] = p50_events(fn, args.calls, args.warmup)
    print(f"configs[4] shape (GIT-large), {B} clips x 10 frames, beam 4, {L} steps (image pass included)")
    for name, _ in cases:
        print(f"   {name:18s} p50 {t[name]:8.3f} ms")
    print(f"   attached / unattached: {t['attached'] / t['unattached']:.3f}", flush=True)
    del m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    print(f"tools/constraints_bench.py --calls {args.calls} --warmup {args.warmup} on {torch.cuda.get_device_name(0)}")
    greedy(args)
    if not args.skip_large:
        beam(args)


if __name__ == "__main__":
    main()
