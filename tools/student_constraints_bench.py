#!/usr/bin/env python3
"""What the student's hard constraints cost (its output is meant for profiles/r29_student_constraints_bench.txt).

    python tools/student_constraints_bench.py [--calls 5] [--warmup 2] [--seed 0]

The base student (576 wide, V = 30522) with its native TinyViT encoder; memory tokens are pushed, so that the encoder stays out of
the numbers.  Three shapes, each attached (no_repeat_ngram_size=2, min_length=4, suppress_tokens=[0]) against unattached, HIP events
around the call, p50 of `--calls` after `--warmup` unrecorded ones, per shape first all unattached calls, then all attached ones (a
model has one live stream and one pool at a time):
  (a) window   caption_stream(batch=1, hop=1): one token pushed into a full window and its 25-token greedy caption
  (b) pool     stream_pool(16): one token for each of 16 full cameras and their 16 captions, one pool call
  (c) beam     beam_search(k=3, max_len=25) of one clip
An attached call makes one 256-thread launch more per step (the rows' ban mask) and runs the BAN form of the head (greedy) or of
the candidate ranking (beam); (a) and (b) replay a captured loop of their own, the rules written to a device record ahead of it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

RULES = dict(no_repeat_ngram_size=2, min_length=4, suppress_tokens=[0])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights
    scfg, tcfg, C, L, K = student_base(), tinyvit_config("tiny_vit_21m_224"), 16, 25, 3
    F, D = scfg.mem_tokens, scfg.d_model
    w = dict(student_synthetic_weights(scfg, 0))
    w.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=C * F)
    m = StudentCaptioner(cfg=scfg, weights=w, image_encoder=enc, device="cuda:0", max_batch=C, max_text_len=L + 1, stop="never")
    g = torch.Generator().manual_seed(args.seed)
    n = args.warmup + args.calls
    tok = torch.randn(C, F + n, D, generator=g).cuda()                 # camera c's tokens, oldest first

    def window(kw):
        st = m.caption_stream(batch=1, hop=1, max_len=L, stop="never", **kw)
        assert st.push(tok[:1, :F - 1]) is None
        return [timed(lambda: st.push(tok[:1, F - 1 + i:F + i])) for i in range(n)]

    def pool(kw):
        pl = m.stream_pool(C, hop=1, max_len=L, stop="never", min_frames=F, **kw)
        ids = list(range(C))
        for f in range(F - 1):
            assert pl.push(tok[:, f].contiguous(), ids) == {}
        return [timed(lambda: pl.push(tok[:, F - 1 + i].contiguous(), ids)) for i in range(n)]

    def beam(kw):
        return [timed(lambda: m.beam_search(tok[:1, i:i + F].contiguous(), max_len=L, k=K, **kw)) for i in range(n)]

    print(f"tools/student_constraints_bench.py --calls {args.calls} --warmup {args.warmup} --seed {args.seed} on {torch.cuda.get_device_name(0)}")
    print(f"base student (d_model {D}, V {scfg.vocab_length}), memory tokens pushed (no encoder pass in the numbers), stop = never; "
          f"attached = {RULES}; p50 of {args.calls} after {args.warmup} warm-up calls, the two ways run back to back per shape")
    for name, fn, per in (("(a) window push + 25-token caption, B = 1", window, 1), (f"(b) pool push + {C} 25-token captions, one call", pool, C),
                          (f"(c) beam_search k = {K}, max_len = {L}, B = 1", beam, 1)):
        free, att = fn({}), fn(RULES)
        differs = sum(not torch.equal(torch.as_tensor(a[1][0] if isinstance(a[1], dict) else a[1]), torch.as_tensor(b[1][0] if isinstance(b[1], dict) else b[1]))
                      for a, b in zip(free, att))
        tf, ta = [x[0] for x in free[args.warmup:]], [x[0] for x in att[args.warmup:]]
        pf, pa = statistics.median(tf), statistics.median(ta)
        print(f"   {name:52s} unattached p50 {pf:8.3f} ms (min {min(tf):8.3f}, max {max(tf):8.3f})   attached p50 {pa:8.3f} ms "
              f"(min {min(ta):8.3f}, max {max(ta):8.3f})   attached - unattached = {pa - pf:+.3f} ms ({(pa - pf) / per:+.3f} ms per caption), "
              f"ratio {pa / pf:.3f}; the rules changed {differs} of {n} captions (camera 0's)", flush=True)


if __name__ == "__main__":
    main()
