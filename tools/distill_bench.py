"""distill_report against the two routes a user had before it, at 16 clips x 6 frames x 21 positions (GIT base + the base student):
  logits : forward_decoder of both models ([B * n * T, V] fp32 each) + torch softmax / log_softmax / kl_div
  scores : two score() calls -- the floor of the two forward passes with one single head each (no divergence comes out of it)
HIP events, p50 of 5 repetitions after a warm-up.  Usage: python tools/distill_bench.py [--out profiles/r20_distill_bench.txt]"""
import argparse
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")]


def p50(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--clips", type=int, default=16)
    args = ap.parse_args()
    import gitcap
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from gitcap.weights import synthetic_weights
    B, F, T, tau = args.clips, 6, 21, 2.0
    cfg = git_base(F)
    scfg = dataclasses.replace(student_base(), vocab_length=cfg.vocab_size)
    lines = [f"distill_report vs the logits route vs two score() calls: {B} clips x {F} frames x {T} positions, temperature {tau}, "
             f"V = {cfg.vocab_size}, teacher width {cfg.dec_width}, student width {scfg.d_model}; ms, p50 of 5 after a warm-up", ""]
    for n in (1, 4):
        t = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=B, max_frames=F, max_text_len=T + 1, max_beams=n, stop="never")
        s = StudentCaptioner(cfg=scfg, weights=student_synthetic_weights(scfg, 0), device="cuda:0", max_batch=B * n, max_text_len=T + 1, stop="never")
        g = torch.Generator().manual_seed(n)
        mem = t.forward_image_enc(torch.randn(B, F, 3, cfg.image_size, cfg.image_size, generator=g).cuda())[1]
        smem = torch.randn(B, scfg.mem_tokens, scfg.d_model, generator=g).cuda()
        y = torch.randint(1, cfg.vocab_size, (B, n, T), generator=g).cuda()
        yy = y if n > 1 else y[:, 0]

        def fused():
            return gitcap.distill_report(t, s, mem, yy, temperature=tau, student_x=smem)

        def logits():
            kl = 0
            for c in range(n):
                tl, sl = t.forward_decoder(y[:, c], mem), s.forward_decoder(y[:, c], smem)
                kl = kl + torch.nn.functional.kl_div(torch.log_softmax(sl / tau, -1), torch.softmax(tl / tau, -1), reduction="batchmean")
            return kl * tau * tau

        def scores():
            return t.score(mem, yy, until_sep=False), s.score(smem, yy, until_sep=False)

        torch.cuda.reset_peak_memory_stats()
        a = p50(fused); ma = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        b = p50(logits); mb = torch.cuda.max_memory_allocated()
        c = p50(scores)
        ref, got = float(logits()), float(fused()["kl_loss"])
        lines.append(f"n = {n}: distill_report {a:8.3f}   logits route {b:8.3f}   two score() calls {c:8.3f}   "
                     f"(peak torch allocations {ma / 2**20:.0f} / {mb / 2**20:.0f} MiB; kl_loss {got:.6f} vs torch {ref:.6f})")
        del t, s
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
