"""The fp64 restatement of the attention maps (tests/attention_map_reference.py) against a plain torch softmax, the measured part
of its bound, and the proof that the device test's inputs tell wrong kernels apart.  No GPU."""
import os

import numpy as np
import pytest
import torch

import attention_map_reference as R


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in R.device_cases()}


@pytest.fixture(scope="module")
def refs(cases):
    """fp64 maps and bounds of every device case, computed once"""
    return {n: R.maps_fp64(c, want_bound=True) for n, c in cases.items()}


def torch_maps(case):
    """softmax over [image ; causal text] scores in fp64 torch, head and layer mean, frame sums"""
    L, H, D, rows, T, N, Smax = (case[k] for k in ("L", "H", "D", "rows", "T", "N", "Smax"))
    layers = range(L) if case["layer"] < 0 else [case["layer"]]
    fm, tm, pm = torch.zeros(rows, T, Smax // N, dtype=torch.float64), torch.zeros(rows, T, dtype=torch.float64), torch.zeros(rows, T, Smax, dtype=torch.float64)
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    for r in range(rows):
        row0, S = R.clip_rows(case, r // case["rows_per_clip"])
        for l in layers:
            txt = torch.from_numpy(case["kv_txt"][l, r, :T].astype(np.float64))
            img = torch.from_numpy(case["kv_img"][l, row0:row0 + S].astype(np.float64))
            for h in range(H):
                q, kt, ki = txt[:, h * 64:h * 64 + 64], txt[:, D + h * 64:D + h * 64 + 64], img[:, D + h * 64:D + h * 64 + 64]
                s = torch.cat([q @ ki.T, q @ kt.T + mask], dim=1) / 8.0
                p = torch.softmax(s, dim=1)
                pm[r, :, :S] += p[:, :S]
                tm[r] += p[:, S:].sum(1)
        if case["lengths"] is not None:
            pm[r, int(case["lengths"][r]):] = 0
            tm[r, int(case["lengths"][r]):] = 0
    cnt = len(layers) * H
    pm, tm = pm / cnt, tm / cnt
    for r in range(rows):
        S = R.clip_rows(case, r // case["rows_per_clip"])[1]
        for f in range(S // N):
            fm[r, :, f] = pm[r, :, f * N:(f + 1) * N].sum(1)
    return fm.numpy(), tm.numpy(), pm.numpy()


def test_restatement_is_torch_softmax(cases, refs):
    for name, case in cases.items():
        fm, tm, pm = refs[name][:3]
        for a, b in zip((fm, tm, pm), torch_maps(case)):
            assert a.shape == b.shape and np.abs(a - b).max() < 1e-13, name
        total = fm.sum(-1) + tm
        live = np.ones_like(tm, bool)
        if case["lengths"] is not None:
            live = np.arange(case["T"])[None, :] < case["lengths"][:, None]
        assert np.abs(total[live] - 1.0).max() < 1e-13 and (total[~live] == 0).all(), name


def test_zeros_where_zeros_are_specified(cases, refs):
    c = cases["ragged_1_and_3_rpc2"]
    fm, tm, pm = refs[c["name"]][:3]
    assert (fm[:2, :, 1:] == 0).all() and (pm[:2, :, c["N"]:] == 0).all() and (fm[2:] > 0).all()
    c = cases["lengths_0_1_T"]
    fm, tm, pm = refs[c["name"]][:3]
    assert (fm[0] == 0).all() and (tm[0] == 0).all() and (fm[1, 1:] == 0).all() and (tm[1, 0] > 0) and (tm[2] > 0).all()


def measured_delta(cases, refs):
    worst = {}
    for name, case in cases.items():
        w = 0.0
        for v32, v64 in zip(R.maps_fp32(case), refs[name][:3]):
            big = v64 >= 2.0 ** -100
            if big.any():
                w = max(w, float((np.abs(v32 - v64)[big] / v64[big]).max()))
        worst[name] = w
    return worst


def test_measured_fp32_term_is_what_the_bound_uses(cases, refs):
    worst = measured_delta(cases, refs)
    for name, w in worst.items():
        print(f"{name}: worst |fp32 restatement - fp64| / value = {w:.3e}")
    assert max(worst.values()) <= R.DELTA_MEASURED
    assert max(worst.values()) >= R.DELTA_MEASURED / 64, "DELTA_MEASURED no longer describes the restatement"
    # the fp32 restatement itself sits inside the derived bound: the bound covers the kernel's rounding points
    for name, case in cases.items():
        for v32, v64, b in zip(R.maps_fp32(case), refs[name][:3], refs[name][3:]):
            assert (np.abs(v32 - v64) <= b).all(), name


@pytest.mark.parametrize("variant,name", [
    ("no_scale", "N197_F3_T17"), ("future_key", "N197_F3_T17"), ("future_key", "future_key"), ("frame_off_by_one", "N197_F3_T17"),
    ("wrong_clip", "H12_layer0_T16_rpc2"), ("wrong_clip", "ragged_1_and_3_rpc2"), ("drop_head", "N197_F3_T17"),
    ("drop_head", "H12_layer0_T16_rpc2"), ("drop_layer", "N197_F3_T17"), ("wrong_count", "N197_F3_T17"),
    ("wrong_count", "N5_F1_T1_H1_L1")])
def test_inputs_tell_wrong_kernels_apart(cases, refs, variant, name):
    fm, tm, pm, bf, bt, bp = refs[name]
    wf, wt, wp = R.maps_fp64(cases[name], variant=variant)
    miss = max(float((np.abs(wf - fm) / bf).max()), float((np.abs(wt - tm) / bt).max()))
    print(f"{variant} on {name}: worst |wrong - right| / bound = {miss:.3e}")
    assert miss > 100.0


def test_future_key_case_would_move_all_mass(cases, refs):
    wt = R.maps_fp64(cases["future_key"], variant="future_key")[1]
    assert (wt[:, :-1] > 0.99).all() and (np.abs(wt - refs["future_key"][1])[:, :-1].max() > 0.1)


def test_dominant_and_underflow_inputs(cases, refs):
    c = cases["dominant_underflow"]
    fm, tm, pm = refs[c["name"]][:3]
    # one head of row 0, position 2 puts its whole mass on key 7; the last frame's keys underflow there
    per_head = R.maps_fp64(dict(c, H=1, D=c["D"], layer=0), want_bound=False)
    assert per_head[2][0, 2, 7] > 0.999999 and per_head[2][0, 2, 2 * c["N"]:3 * c["N"]].max() < 2.0 ** -149


def test_restatement_on_the_oracles_own_q_and_k(golden_dir):
    """oracle/git_oracle.py's _attn, wrapped (not edited) to capture the q and k of a full pass over the hf_tiny fixture's frames and
    prefix: the restatement's maps on them against a plain torch softmax of the captured scores under the captured key limits."""
    from gitcap.config import git_tiny
    from gitcap.weights import synthetic_weights
    from oracle.git_oracle import GitOracle, make_frames
    cfg = git_tiny(2)
    g = np.load(os.path.join(golden_dir, "hf_tiny_F2.npz"))
    fr = make_frames(2, 2, cfg.image_size, int(g["frame_seed"]))
    orc = GitOracle(cfg, synthetic_weights(cfg, 0), emulate_bf16=True)
    _, mem = orc.forward_image_enc(fr)
    ids = torch.from_numpy(g["prefix_ids"])
    seen, inner = [], orc._attn
    orc._attn = lambda q, k, v, klimit: (seen.append((q.double(), k.double(), klimit)), inner(q, k, v, klimit))[1]
    orc.decoder_full(mem, ids)
    L, H, D = cfg.dec_layers, cfg.dec_heads, cfg.dec_width
    assert len(seen) == L
    B, T, S = ids.shape[0], ids.shape[1], mem.shape[1]
    N = S // 2
    kv_txt, kv_img = np.zeros((L, B, T, 3 * D), np.float32), np.zeros((L, B * S, 3 * D), np.float32)
    want_p = torch.zeros(B, T, S + T, dtype=torch.float64)
    for l, (q, k, klimit) in enumerate(seen):
        assert q.shape == (B, H, S + T, 64)
        kv_txt[l, :, :, :D] = q[:, :, S:].transpose(1, 2).reshape(B, T, D).numpy()
        kv_txt[l, :, :, D:2 * D] = k[:, :, S:].transpose(1, 2).reshape(B, T, D).numpy()
        kv_img[l, :, D:2 * D] = k[:, :, :S].transpose(1, 2).reshape(B * S, D).numpy()
        s = (q[:, :, S:] @ k.transpose(-1, -2)) / 8.0
        vis = torch.arange(S + T)[None, :] < klimit[S:, None]
        want_p += torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1).sum(1)
    want_p /= L * H
    assert (kv_txt == R.bf16_rne(kv_txt)).all() and (kv_img == R.bf16_rne(kv_img)).all()      # the oracle's q, k are bf16 values
    case = dict(name="oracle", L=L, H=H, D=D, rows=B, rows_per_clip=1, T=T, Tmax=T, N=N, S_img=S, Smax=S, img_rows=B * S, off=None,
                len=None, layer=-1, lengths=None, kv_txt=kv_txt, kv_img=kv_img)
    fm, tm, pm = R.maps_fp64(case)
    assert np.abs(pm - want_p[:, :, :S].numpy()).max() < 1e-13
    assert np.abs(tm - want_p[:, :, S:].sum(-1).numpy()).max() < 1e-13
    assert np.abs(fm - want_p[:, :, :S].reshape(B, T, 2, N).sum(-1).numpy()).max() < 1e-13


# ---- the student's read-out -----------------------------------------------------------------------------------------------------------

def test_cross_restatement_measured_term_and_wrong_kernels():
    worst = 0.0
    for c in R.cross_cases():
        p, fm, bp, bf = R.cross_fp64(c)
        rows, T, H, hd, F = c["rows"], c["T"], c["H"], c["hd"], c["F"]
        q = torch.from_numpy(c["q"].astype(np.float64)).reshape(rows, T, H, hd)
        k = torch.from_numpy(c["kv"][:, :, :H * hd].astype(np.float64)).reshape(rows, F, H, hd)
        want = torch.softmax(torch.einsum("rthd,rfhd->rthf", q, k) / hd ** 0.5, -1)
        assert np.abs(p - want.reshape(rows * T, H, F).numpy()).max() < 1e-14
        live = np.ones((rows, T), bool) if c["lengths"] is None else np.arange(T)[None, :] < c["lengths"][:, None]
        assert np.abs(fm.sum(-1)[live] - 1).max() < 1e-14 and (fm[~live] == 0).all()
        p32, fm32 = R.cross_fp32(c)
        assert (np.abs(p32 - p) <= bp).all() and (np.abs(fm32 - fm)[live] <= bf[live]).all()
        worst = max(worst, float((np.abs(p32 - p) / p).max()))
        for variant in ("no_scale", "next_row", "drop_head"):
            if variant == "next_row" and rows == 1:
                continue
            wp, wf, _, _ = R.cross_fp64(c, variant)
            miss = max(float((np.abs(wp - p) / bp).max()), float((np.abs(wf - fm)[live] / bf[live]).max()))
            print(f"cross F={F} {variant}: worst |wrong - right| / bound = {miss:.3e}")
            assert miss > 100.0 or (F == 1 and variant != "drop_head")       # one key: every softmax is 1
    print(f"cross: worst |fp32 restatement - fp64| / value = {worst:.3e}")
    assert R.DELTA_CROSS_MEASURED / 64 <= worst <= R.DELTA_CROSS_MEASURED
