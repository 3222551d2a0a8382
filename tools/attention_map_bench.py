#!/usr/bin/env python3
"""What asking for the attention maps costs (its output is meant for profiles/r26_attention_map_bench.txt).

    python tools/attention_map_bench.py [--calls 5] [--warmup 2]

In one process, after a warm-up, p50 over `--calls` calls each by HIP events, GIT-base with synthetic weights:
  greedy:    16 clips x 6 frames x 20 tokens, one synchronous greedy_decode per call, with and without return_attention;
  attention: attention(x, y) against score(x, y) on the same 16 x 21 ids (attention runs score's pass, then the two map launches),
             with and without the patch rows.
Every call with return_attention returns the ids of the plain one (asserted).
  student:   student base (synthetic weights), B = 1, memory given, 25 tokens: greedy with and without return_attention (one more
             teacher-forced pass), attention against score."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, n, warm):
    """p50 of the HIP-event ms of n calls of fn() after `warm` unrecorded ones; each call is followed by a synchronisation."""
    ev = []
    for i in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ev.append(a.elapsed_time(b))
    return statistics.median(ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    from oracle.git_oracle import make_frames
    B, Fr, L = 16, 6, 20
    cfg = git_base(Fr)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=B, max_frames=Fr, max_text_len=L + 1, stop="never")
    x = make_frames(B, Fr, cfg.image_size, 1234).cuda()
    want = m.greedy_decode(x, max_len=L).clone()
    res = {}
    for name, att in (("plain", False), ("return_attention", True), ("plain_again", False)):
        outs = []
        res["greedy_" + name] = timed(lambda: outs.append(m.greedy_decode(x, max_len=L, return_attention=att)), args.calls, args.warmup)
        assert all(torch.equal(o[0] if att else o, want) for o in outs)
    off = statistics.median([res["greedy_plain"], res["greedy_plain_again"]])
    on = res["greedy_return_attention"]
    print(f"greedy 16 clips x 6 frames x 20 tokens: plain {res['greedy_plain']:.3f} / {res['greedy_plain_again']:.3f} ms, "
          f"return_attention {on:.3f} ms, added {on - off:+.3f} ms = {100 * (on - off) / off:+.2f} %", flush=True)
    mem = m.forward_image_enc(x)[1]
    res["score"] = timed(lambda: m.score(mem, want, until_sep=False), args.calls, args.warmup)
    res["attention"] = timed(lambda: m.attention(mem, want, until_sep=False), args.calls, args.warmup)
    res["attention_patches"] = timed(lambda: m.attention(mem, want, patches=True, until_sep=False), args.calls, args.warmup)
    print(f"16 rows x 21 ids against the encoded memory: score {res['score']:.3f} ms, attention {res['attention']:.3f} ms, "
          f"attention(patches=True) {res['attention_patches']:.3f} ms", flush=True)
    student(args, res)
    print(json.dumps(res))


def student(args, res):
    """the student's 25-token call at B = 1 (memory given): greedy with and without return_attention, attention against score"""
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from oracle.student_oracle import make_memory
    cfg = student_base()
    m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), device="cuda:0", max_batch=1, max_text_len=25, stop="never")
    mem = make_memory(1, cfg.mem_tokens, cfg.d_model, 3).cuda()
    want = m.greedy_decode(mem, max_len=25).clone()
    for name, att in (("plain", False), ("return_attention", True), ("plain_again", False)):
        outs = []
        res["student_greedy_" + name] = timed(lambda: outs.append(m.greedy_decode(mem, max_len=25, return_attention=att)), args.calls, args.warmup)
        assert all(torch.equal(o[0] if att else o, want) for o in outs)
    res["student_score"] = timed(lambda: m.score(mem, want, until_sep=False), args.calls, args.warmup)
    res["student_attention"] = timed(lambda: m.attention(mem, want, until_sep=False), args.calls, args.warmup)
    print(f"student B = 1, 25 tokens: greedy plain {res['student_greedy_plain']:.3f} / {res['student_greedy_plain_again']:.3f} ms, "
          f"return_attention {res['student_greedy_return_attention']:.3f} ms; score {res['student_score']:.3f} ms, "
          f"attention {res['student_attention']:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
