#!/usr/bin/env python3
"""What a prompt costs (its output is meant for profiles/r19_prompt_bench.txt).

    python tools/prompt_bench.py [--calls 20] [--warmup 3] [--skip-large]

GIT-base, 16 clips x 6 frames, a 20-step greedy caption (greedy_decode, image pass included), alternating four cases:
  unprompted        20 token steps
  shared 8 tokens   every row the same length: one 8-position pass + 12 token steps
  ragged 2..8       prompts of 2..8 tokens: one 2-position pass, forced arg-max launches up to position 7
  forced steps      the shared prompt with the multi-position pass switched off (gitcap_dbg_config(20, 0)): 20 token steps
and the image pass alone (forward_image_enc), so that the token loops can be told apart from it.  Then the configs[4] beam
shape (GIT-large, 10-frame clips, 16 clips, beam 4, 15 steps) with and without an 8-token prompt: the beam rows have no
multi-position pass, a prompt token costs one decoder step without the vocabulary head, the ranking and the K/V gather.
HIP events, p50 of `--calls` calls after `--warmup` unrecorded ones."""
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


def prompts(cfg, lengths, seed=3):
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randint(1000, cfg.vocab_size, (n,), generator=g) for n in lengths]
    for r in rows:
        r[0] = cfg.cls_token_id
    return rows


def make(cfg, B, Fr, T, beams):
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights
    from oracle.git_oracle import make_frames
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=B, max_frames=Fr, max_text_len=T, max_beams=beams, stop="never")
    return m, make_frames(B, Fr, cfg.image_size, 1234).cuda()


def greedy(args):
    from gitcap.config import git_base
    cfg, B, L = git_base(6), 16, 20
    m, x = make(cfg, B, 6, L + 1, 1)
    shared = torch.stack(prompts(cfg, [8] * B))
    ragged = prompts(cfg, [2 + b % 7 for b in range(B)])

    def no_prefill():
        old = m._lib.gitcap_dbg_config(20, 0)
        try:
            return m.greedy_decode(x, max_len=L, prompt=shared)
        finally:
            m._lib.gitcap_dbg_config(20, old)
    cases = [("unprompted", lambda: m.greedy_decode(x, max_len=L)),
             ("shared 8 tokens", lambda: m.greedy_decode(x, max_len=L, prompt=shared)),
             ("ragged 2..8", lambda: m.greedy_decode(x, max_len=L, prompt=ragged)),
             ("forced steps", no_prefill),
             ("image pass alone", lambda: m.forward_image_enc(x))]
    assert torch.equal(cases[1][1](), no_prefill())
    t = {}
    for _ in range(2):                                                           # alternate
        for name, fn in cases:
            t[name] = p50_events(fn, args.calls, args.warmup)
    print(f"GIT-base, {B} clips x 6 frames, {L}-step greedy caption (image pass included)")
    for name, _ in cases:
        print(f"   {name:18s} p50 {t[name]:8.3f} ms   token loop {t[name] - t['image pass alone']:8.3f} ms")
    print(f"   shared 8-token prompt / unprompted: {t['shared 8 tokens'] / t['unprompted']:.3f} of the call, "
          f"{(t['shared 8 tokens'] - t['image pass alone']) / (t['unprompted'] - t['image pass alone']):.3f} of the token loop", flush=True)
    del m


def beam(args):
    from gitcap.config import git_large
    cfg, B, L = git_large(10), 16, 15
    m, x = make(cfg, B, 10, L, 4)
    shared = torch.stack(prompts(cfg, [8] * B))
    kw = dict(beam_size=4, max_steps=L, length_penalty=0.6, per_node_beam_size=2, on_device=True)
    cases = [("unprompted", lambda: m.infer(x, **kw)), ("shared 8 tokens", lambda: m.infer(x, prompt=shared, **kw))]
    t = {}
    for _ in range(2):
        for name, fn in cases:
            t[name] = p50_events(fn, args.calls, args.warmup)
    print(f"configs[4] shape (GIT-large), {B} clips x 10 frames, beam 4, {L} steps (image pass included)")
    for name, _ in cases:
        print(f"   {name:18s} p50 {t[name]:8.3f} ms")
    print(f"   8-token prompt / unprompted: {t['shared 8 tokens'] / t['unprompted']:.3f} (7 forced steps: no head, no ranking, no gather)", flush=True)
    del m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    print(f"tools/prompt_bench.py --calls {args.calls} --warmup {args.warmup} on {torch.cuda.get_device_name(0)}")
    greedy(args)
    if not args.skip_large:
        beam(args)


if __name__ == "__main__":
    main()
