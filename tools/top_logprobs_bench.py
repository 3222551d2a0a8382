#!/usr/bin/env python3
"""What asking for the top-k token alternatives costs (its output is meant for profiles/r25_top_logprobs_bench.txt).

    python tools/top_logprobs_bench.py [--calls 5] [--k 8] [--skip-teacher] [--skip-student] [--skip-score]

In one process, after a warm-up, p50 over `--calls` calls each by HIP events, attached against not attached:
  teacher: GIT-base, 16 clips x 6 frames x 20 tokens, one synchronous greedy_decode per call, top_logprobs = k and 32;
  student: B = 1, 480x640 camera frames on the device, student 21m (synthetic weights), hop = 1, max_len = 25 -- one window push
           per call (encoder + 25 token steps), top_logprobs = k;
  score:   GIT-base, 16 clips x 4 candidates x 21 positions (the shape of tools/score_bench.py), score(top_k=k) against
           forward_decoder + log_softmax + topk per candidate, with torch's peak allocation during each beside it.
Every attached call returns the ids of the plain one (asserted)."""
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


def line(name, off, on, steps):
    print(f"{name}: not attached {off:.3f} ms, attached {on:.3f} ms, added {on - off:+.3f} ms = {100 * (on - off) / off:+.2f} % "
          f"= {1e3 * (on - off) / steps:+.1f} us per token step", flush=True)


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
    out = {}
    for k in (0, args.k, 32, 0):
        outs = []
        ms = timed(lambda: outs.append(m.greedy_decode(x, max_len=L, top_logprobs=k)), args.calls, args.warmup)
        assert all(torch.equal(o[0] if k else o, want) for o in outs)
        out.setdefault(k, []).append(ms)
    off = statistics.median(out[0])
    print(f"teacher not attached, before / after the attached runs: {out[0][0]:.3f} / {out[0][1]:.3f} ms")
    for k in (args.k, 32):
        line(f"teacher 16 clips x 6 frames x 20 tokens, top_logprobs={k}", off, out[k][0], L)
    return {str(k): v for k, v in out.items()}


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
    res, caps = {}, {}
    for k in (0, args.k):                                         # one live stream per model: fill, measure, then the other
        st = m.caption_stream(batch=1, hop=1, max_len=L, stop="never", top_logprobs=k)
        for _ in range(F):
            caps[k] = st.push(frame)
        outs = []
        res[k] = timed(lambda: outs.append(st.push(frame)), args.calls, args.warmup)
        assert all(torch.equal(o, caps[k]) for o in outs)
    assert torch.equal(caps[0], caps[args.k])
    line(f"student B=1, 25-token window push, top_logprobs={args.k}", res[0], res[args.k], L)
    return {str(k): v for k, v in res.items()}


def score(args):
    """The shape of tools/score_bench.py (profiles/r18_score_bench.txt): 16 clips x 4 candidates x 21 positions = 64 rows, 1280 head rows."""
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    from oracle.git_oracle import make_frames
    B, n, T, Fr = 16, 4, 21, 6
    cfg = git_base(Fr)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=B, max_frames=Fr, max_text_len=T, max_beams=n, stop="never")
    x = make_frames(B, Fr, cfg.image_size, 1234).cuda()
    _, mem = m.forward_image_enc(x)
    y = torch.randint(1000, cfg.vocab_size, (B, n, T), generator=torch.Generator().manual_seed(3)).cuda()
    y[:, :, 0] = cfg.cls_token_id

    def fused():
        d = m.score(mem, y, until_sep=False, top_k=args.k)
        return d["topk_ids"], d["topk_logprobs"]

    def via_logits():
        out = []
        for c in range(n):                                          # forward_decoder takes [B, T]: one pass per candidate
            lp = torch.log_softmax(m.forward_decoder(y[:, c].contiguous(), mem), -1)[:, :-1]
            out.append(torch.topk(lp, args.k, dim=-1))
        return torch.stack([o.indices for o in out], 1), torch.stack([o.values for o in out], 1)

    a, b = fused(), via_logits()
    assert tuple(a[0].shape) == tuple(b[0].shape) == (B, n, T - 1, args.k)
    assert float((a[1].double() - b[1].double()).abs().max()) <= 1e-3          # (the same distributions; ties may order ids differently)
    res = {}
    for name, fn in (("score(top_k)", fused), ("logits + log_softmax + topk", via_logits), ("score()", lambda: m.score(mem, y, until_sep=False))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = timed(fn, args.calls, args.warmup)
        res[name] = (ms, (torch.cuda.max_memory_allocated() - base) / 1e6)
        print(f"score 16 clips x 4 candidates x 21 positions, k={args.k}: {name}: {ms:.3f} ms, peak torch allocation during the call "
              f"{res[name][1]:.1f} MB", flush=True)
    return {k: list(v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--skip-teacher", action="store_true")
    ap.add_argument("--skip-student", action="store_true")
    ap.add_argument("--skip-score", action="store_true")
    args = ap.parse_args()
    out = {"calls": args.calls, "k": args.k}
    for name, fn, skip in (("teacher", teacher, args.skip_teacher), ("student", student, args.skip_student), ("score", score, args.skip_score)):
        if not skip:
            out[name] = fn(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
