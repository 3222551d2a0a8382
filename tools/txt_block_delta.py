"""Measures the fp32 softmax term delta of txt_block on the device (tests/text_rows_reference.py: DELTA_MEASURED): the largest
|ctx_device - ctx64| over TXT_CASES, the context recovered from `part` with identity slices for the output dense.

    python tools/txt_block_delta.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "real-time-video-captioning_amd"))

import text_rows_reference as R  # noqa: E402
import test_text_rows_gpu as G  # noqa: E402


def main():
    from gitcap import _lib
    lib = _lib.load()
    worst = excess = 0.0
    for i, case in enumerate(R.TXT_CASES):
        case = case[:6] + (False,) + case[7:]                    # identity slices are bf16
        q = R.txt_block_inputs(*case, seed=7000 + i, identity=True)
        M, H, D = q["rows"] * q["T"], q["H"], q["D"]
        d = G._txt_operands(lib, q, packed=False)
        part, _, _ = G._txt_launch(lib, q, d, G._txt_outputs(M, H, D))
        ctx_dev = G._np(part)[:, :, :64]
        ref = R.txt_block(q)
        err = np.abs(ctx_dev - ref["ctx"])
        ulps = float((err / R.bf16_ulp(ref["ctx"])).max())
        # what is left of it beside the two documented bf16 roundings (the context's own, and P's in the PV product)
        V = 2.0 ** -8 * np.abs(ref["ctx"])
        flips = float(np.mean(ctx_dev != R.bf16_rne(ref["ctx"])))
        print(f"{case}: max |ctx_device - ctx64| = {err.max():.6g} ({ulps:.3f} bf16 ulp of the value), "
              f"max over half-ulp rounding {np.maximum(err - V, 0).max():.6g}, off the correctly rounded value {flips:.4f}")
        worst = max(worst, float(err.max()))
        excess = max(excess, float(np.maximum(err - V, 0).max()))
    print(f"DELTA_MEASURED = {worst:.6g}   (beside the context's own rounding: {excess:.6g})")


if __name__ == "__main__":
    main()
