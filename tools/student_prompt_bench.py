#!/usr/bin/env python3
"""What a prompt costs on the student (its output is meant for profiles/r31_student_prompt_bench.txt).

    python tools/student_prompt_bench.py [--calls 5] [--warmup 2]

The base student (d_model 576, vocabulary 30522, 6 memory tokens), synthetic weights, memory tokens pushed directly (no image pass):
  push, B = 1            one token pushed into a caption_stream window, then its 25-token greedy caption: unprompted; with an
                         8-token prompt as one pass (8 positions in one forward, 17 token steps behind it); the same prompt as
                         forced token steps (gitcap_dbg_config(20, 0): 25 steps, the forced arg-max)
  pool, 16 cameras       one push of a token per camera and the 25-token captions of all 16 as one batch: unprompted, and with
                         ragged standing prompts of 2 .. 8 tokens (min length 2: two positions in one pass)
  beam_search, k = 3     B = 1, max_len 25: unprompted and with the 8-token prompt (7 forced bookkeeping steps)
HIP events, p50 of `--calls` calls after `--warmup` unrecorded ones; the cases of a group alternate."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from prompt_bench import p50_events  # noqa: E402

L = 25


def group(title, cases, args):
    t = {}
    for _ in range(2):                                                           # alternate
        for name, fn in cases:
            if isinstance(fn, tuple):                                            # (set-up outside the timed region, the timed call)
                fn[0]()
                fn = fn[1]
            t[name] = p50_events(fn, args.calls, args.warmup)
    print(title)
    base = t[cases[0][0]]
    for name, _ in cases:
        print(f"   {name:34s} p50 {t[name]:8.3f} ms   {t[name] / base:6.3f} x {cases[0][0]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from gitcap.tinyvit_config import tinyvit_synthetic_weights
    from gitcap.tinyvit import tinyvit_config
    cfg = student_base()
    weights = dict(student_synthetic_weights(cfg, 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tinyvit_config("tiny_vit_21m_224"), 0).items()})
    m = StudentCaptioner(cfg=cfg, weights=weights, image_encoder="native", device="cuda:0", max_batch=16, max_text_len=32, stop="never")
    g = torch.Generator().manual_seed(3)
    prompt8 = torch.randint(1000, cfg.vocab_length, (8,), generator=g)
    prompt8[0] = cfg.cls_token_id
    tok = torch.randn((16, 1, cfg.d_model), generator=g).cuda()

    def stream_case(prompt, one_pass=True):
        def run():
            old = m._lib.gitcap_dbg_config(20, 1 if one_pass else 0)
            try:
                st.prompt = prompt
                st.push(tok[:1])
            finally:
                m._lib.gitcap_dbg_config(20, old)
        return run
    st = m.caption_stream(batch=1, hop=1, max_len=L, stop="never")
    for _ in range(cfg.mem_tokens):
        st.push(tok[:1])
    group(f"caption_stream push, B = 1, {L}-token greedy caption",
          [("unprompted", stream_case(None)), ("8-token prompt, one pass", stream_case([prompt8])),
           ("8-token prompt, forced steps", stream_case([prompt8], False))], args)

    pool = m.stream_pool(16, hop=1, max_len=L, stop="never")
    cams = list(range(16))
    for _ in range(cfg.mem_tokens):
        pool.push(tok[:, 0], cams)

    def pool_case(prompted):
        def setup():                                # the standing prompts are set once; a pool call builds and attaches their table
            for c in cams:
                pool.set_prompt(c, prompt8[:2 + c % 7] if prompted else None)
        return setup, lambda: pool.push(tok[:, 0], cams)
    group(f"stream_pool push, 16 cameras, {L}-token greedy captions as one batch",
          [("unprompted", pool_case(False)), ("ragged prompts of 2 .. 8 tokens", pool_case(True))], args)

    mem = torch.randn((1, cfg.mem_tokens, cfg.d_model), generator=g).cuda()
    group(f"beam_search, B = 1, k = 3, max_len {L}",
          [("unprompted", lambda: m.beam_search(mem, max_len=L, k=3)),
           ("8-token prompt", lambda: m.beam_search(mem, max_len=L, k=3, prompt=[prompt8]))], args)


if __name__ == "__main__":
    main()
