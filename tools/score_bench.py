#!/usr/bin/env python3
"""What scoring given captions costs against the only route there was before (its output is meant for
profiles/r18_score_bench.txt).

    python tools/score_bench.py [--calls 20] [--warmup 3] [--skip-large]

On one handle per shape, the image K/V already in place (forward_image_enc once, outside the timed region), alternating:
  fused:  GitCaptioner.score(memory, y)                        -- no logits tensor
  logits: forward_decoder(y, memory) -> torch.log_softmax -> gather -> masked sum
HIP events, p50 of `--calls` calls after `--warmup` unrecorded ones, and the peak device memory each route adds
(torch.cuda.max_memory_allocated: the library's own workspace is allocated by hipMalloc and reported through workspace_bytes).
Shapes: GIT-base, 16 clips x 6 frames, 21 positions, 1 and 4 candidates per clip; the configs[4] shape (GIT-large, 10-frame clips,
16 clips x 4 candidates x 15 positions).  The two routes' sums are compared (printed, and asserted within 1e-3 nats)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def p50_events(fn, n, warm):
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


def peak_added(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def shape(name, cfg, B, n, T, Fr, args):
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    from oracle.git_oracle import make_frames
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=B, max_frames=Fr, max_text_len=T, max_beams=n, stop="never")
    x = make_frames(B, Fr, cfg.image_size, 1234).cuda()
    _, memory = m.forward_image_enc(x)
    g = torch.Generator().manual_seed(3)
    y = torch.randint(1000, cfg.vocab_size, (B, n, T), generator=g).cuda()
    y[:, :, 0] = cfg.cls_token_id

    def fused():
        return m.score(memory, y, until_sep=False)["sum"]

    def logits_route():
        out = []
        for k in range(n):                                                       # forward_decoder takes [B, T]: one pass per candidate
            lg = m.forward_decoder(y[:, k].contiguous(), memory)
            lp = torch.log_softmax(lg, -1)[:, :-1].gather(2, y[:, k, 1:, None]).squeeze(-1)
            out.append(lp.sum(1))
        return torch.stack(out, 1)
    ws0 = m.workspace_bytes()
    a, peak_f = peak_added(fused)
    ws1 = m.workspace_bytes()
    b, peak_l = peak_added(logits_route)
    diff = float((a.double() - b.double()).abs().max())
    assert diff <= 1e-3, diff
    tf = tl = None
    for _ in range(2):                                                           # alternate
        tf = p50_events(fused, args.calls, args.warmup)
        tl = p50_events(logits_route, args.calls, args.warmup)
    print(f"{name}: {B} clips x {n} candidates x {T} positions, vocabulary {cfg.vocab_size}\n"
          f"   fused score            p50 {tf:8.3f} ms   peak torch memory added {peak_f / 1e6:8.2f} MB   library workspace added on first use {(ws1 - ws0) / 1e6:.2f} MB\n"
          f"   logits + log_softmax   p50 {tl:8.3f} ms   peak torch memory added {peak_l / 1e6:8.2f} MB\n"
          f"   ratio {tl / tf:.2f} x;  max |sum difference| {diff:.2e} nats", flush=True)
    del m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    from gitcap.config import git_base, git_large
    print(f"tools/score_bench.py --calls {args.calls} --warmup {args.warmup} on {torch.cuda.get_device_name(0)}")
    shape("GIT-base 16 x 1 x 21", git_base(6), 16, 1, 21, 6, args)
    shape("GIT-base 16 x 4 x 21", git_base(6), 16, 4, 21, 6, args)
    if not args.skip_large:
        shape("configs[4] shape (GIT-large)", git_large(10), 16, 4, 15, 10, args)


if __name__ == "__main__":
    main()
