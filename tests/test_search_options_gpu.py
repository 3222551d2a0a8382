"""The kernels behind gitcap_search_options on the MI355X, through their stateless hooks:

  a. gitcap_beam_topk_penalized against tests/search_options_reference.py (penalize in fp32 -> selection_reference.beam_candidates):
     indices exactly, scores within 1e-4 on inputs whose distinct candidate scores are more than 1e-3 apart -- the bar and the input
     condition of test_selection_gpu.py::test_beam_topk_vs_restatement; the fp32 penalty adds one rounding of a logit (~1e-6);
  b. gitcap_dbg_beam_step_nbest / _finish_nbest (with the penalised ranking) driven as a whole toy search against
     oracle.search_oracle.beam_search(num_keep_best=, repetition_penalty=);
  c. both, and the one-hypothesis hooks gitcap_dbg_beam_step / _finish, against tests/golden/device_search_options.npz: the bits the
     same hooks produced before the kernels behind them were unified (tools/gen_device_regression.py rewrites it).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import search_options_reference as S
import selection_reference as R
from gpu_support import beam_state, lib, ptr, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = S.topk_cases()


def _run_pen(lib, c, rp=None, pad=3, plain=False):
    x, beams, K = c["x"], c["beams"], c["K"]
    rows, V = x.shape
    B = rows // beams
    ld = V + pad
    buf = np.full((rows, ld), 1e30, np.float32)                    # row padding the kernel must not read
    buf[:, :V] = x
    d_x, d_bs, d_pre = to_dev(buf, torch.float32), to_dev(c["bs"], torch.float32), to_dev(c["prefix"], torch.int64)
    out_s = torch.full((B * K + 4,), float("nan"), device="cuda")
    out_i = torch.full((B * K + 4,), -5, device="cuda", dtype=torch.int32)
    if plain:
        rc = lib.gitcap_beam_topk(ptr(d_x), ld, ptr(d_bs), B, beams, V, K, ptr(out_s), ptr(out_i), stream())
    else:
        rc = lib.gitcap_beam_topk_penalized(ptr(d_x), ld, ptr(d_bs), ptr(d_pre), c["prefix"].shape[1], c["cur_len"],
                                            ctypes.c_float(c["rp"] if rp is None else rp), B, beams, V, K, ptr(out_s), ptr(out_i), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(out_s[B * K:]).all()) and bool((out_i[B * K:] == -5).all())
    return out_s[:B * K].view(B, K), out_i[:B * K].view(B, K)


@pytest.mark.parametrize("name", sorted(CASES))
def test_beam_topk_penalized_vs_restatement(lib, name):
    c = CASES[name]
    pre = c["prefix"][:, :c["cur_len"]]
    ws, wi, gap = S.expected_candidates(c["x"], c["bs"], pre, c["rp"], c["beams"], c["K"])
    assert float(gap.min()) > 1e-3, (name, gap)              # a condition on the INPUTS
    assert not (wi == R.SENTINEL).any()
    gs, gi = _run_pen(lib, c)
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy().astype(np.int64)
    print(name, "max |score - restatement| = %.3g, smallest input gap %.3g" % (np.abs(gs - ws).max(), gap.min()))
    assert np.array_equal(gi, wi), (name, gi, wi)
    assert np.allclose(gs, ws, rtol=0, atol=1e-4), (name, np.abs(gs - ws).max())


@pytest.mark.parametrize("name", ["edges_rp1.5", "signs", "vocab30522"])
def test_penalty_one_is_the_plain_ranking_bit_for_bit(lib, name):
    c = CASES[name]
    ps, pi = _run_pen(lib, c, plain=True)
    gs, gi = _run_pen(lib, c, rp=1.0)
    assert torch.equal(gi, pi) and torch.equal(gs.view(torch.int32), ps.view(torch.int32))


def test_beam_topk_penalized_refuses_bad_arguments(lib):
    V, beams, K = 300, 2, 4
    x = torch.zeros(2, V, device="cuda")
    bs = torch.zeros(2, device="cuda")
    pre = torch.zeros(2, 4, device="cuda", dtype=torch.int64)
    out_s = torch.full((8,), float("nan"), device="cuda")
    out_i = torch.full((8,), -5, device="cuda", dtype=torch.int32)

    def call(x=x, ld=V, bs=bs, pre=pre, ld_ids=4, cur_len=3, rp=1.5, B=1, beams=beams, V=V, K=K, out_s=out_s, out_i=out_i, pre_ptr=None):
        return lib.gitcap_beam_topk_penalized(ptr(x), ld, ptr(bs), pre_ptr if pre_ptr is not None else ptr(pre), ld_ids, cur_len,
                                              ctypes.c_float(rp), B, beams, V, K, ptr(out_s), ptr(out_i), stream())
    assert call(x=None) == -1 and call(bs=None) == -1 and call(out_s=None) == -1 and call(out_i=None) == -1
    assert call(pre=None) == -1                                                   # a penalty needs the prefix
    assert call(pre_ptr=ctypes.c_void_p(pre.data_ptr() + 4)) == -1                # int64 ids: 8-byte aligned
    assert call(cur_len=0) == -1 and call(cur_len=5) == -1                        # cur_len < 1, ld_ids < cur_len
    for rp in (0.0, -1.5, float("inf"), float("nan")):
        assert call(rp=rp) == -1, rp
    assert call(beams=17, B=1) == -1 and call(K=17) == -1 and call(B=0) == -1 and call(V=0) == -1
    big = 131073                                                                   # more than 64 chunks
    xb = torch.zeros(1, big, device="cuda")
    assert call(x=xb, ld=big, V=big, beams=1) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out_s).all()) and bool((out_i == -5).all())           # nothing was launched
    assert call(pre=None, rp=1.0) == 0                                            # rp 1: gitcap_beam_topk, the prefix is not read
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out_s[:K]).any()) and bool(torch.isnan(out_s[K:]).all())


# ---- b. the n-best bookkeeping: whole toy searches --------------------------------------------------------------------------

def _device_search(lib, table, beams, lp, n, rp, seen=None, old_hooks=False):
    """The toy search on the device: penalised ranking + n-best step per position, then the finish.  old_hooks: the one-hypothesis
    hooks gitcap_dbg_beam_step / _finish (n = 1, rp = 1 only).  -> (decoded [B][n][L], logprobs [B][n], per-step snapshots)"""
    B, V, L, K = S.TOY_B, S.TOY_V, S.TOY_MAXLEN, 2 * beams
    rows = B * beams
    t, bb1, bbn = beam_state(B, beams, n, L)
    d_table = table.cuda()
    clip = torch.arange(rows, device="cuda") // beams
    assert lib.gitcap_dbg_beam_init(ctypes.byref(bb1), B, beams, L, S.TOY_CLS, stream()) == 0
    t["hyp_len"].zero_()                                    # the init hook passes n = 1 (one slot per clip): all B * n are zeroed here
    ids = [t["ids0"], t["ids1"]]
    cs = torch.empty(B, K, device="cuda")
    ci = torch.empty(B, K, device="cuda", dtype=torch.int32)
    snaps, cur = [], 0
    for cur_len in range(1, L):
        if seen is not None and cur_len - 1 < len(seen):   # the oracle's step function saw exactly these prefixes
            assert torch.equal(ids[cur][:, :cur_len].cpu(), seen[cur_len - 1]), cur_len
        logits = d_table[clip, (cur_len - 1) % 8, t["words"] % V].contiguous()
        assert lib.gitcap_beam_topk_penalized(ptr(logits), V, ptr(t["beam_scores"]), ptr(ids[cur]), L, cur_len, ctypes.c_float(rp), B, beams, V,
                                              K, ptr(cs), ptr(ci), stream()) == 0
        torch.cuda.synchronize()
        assert bool(((ci >= 0) & (ci < beams * V)).all())
        if old_hooks:
            rc = lib.gitcap_dbg_beam_step(ctypes.byref(bb1), ptr(cs), ptr(ci), B, beams, K, V, cur_len, L, S.TOY_EOS, ctypes.c_float(lp), cur,
                                          stream())
        else:
            rc = lib.gitcap_dbg_beam_step_nbest(ctypes.byref(bbn), ptr(cs), ptr(ci), B, beams, K, V, cur_len, L, S.TOY_EOS,
                                                ctypes.c_float(lp), cur, stream())
        assert rc == 0
        torch.cuda.synchronize()
        cnt = (t["hyp_len"] > 0).sum(dim=1)
        for b in range(B):                                  # stored hypotheses fill the slots from 0, nothing behind them
            assert bool((t["hyp_len"][b, :cnt[b]] > 0).all()) and bool((t["hyp_len"][b, cnt[b]:] == 0).all())
        snaps.append({k: v.clone() for k, v in t.items()})
        cur ^= 1
    decoded = torch.full((B, n, L), -777, device="cuda", dtype=torch.int64)
    logprobs = torch.full((B, n), float("nan"), device="cuda")
    if old_hooks:
        rc = lib.gitcap_dbg_beam_finish(ctypes.byref(bb1), B, L, S.TOY_EOS, ptr(decoded), ptr(logprobs), stream())
    else:
        rc = lib.gitcap_dbg_beam_finish_nbest(ctypes.byref(bbn), B, L, S.TOY_EOS, ptr(decoded), ptr(logprobs), stream())
    assert rc == 0
    torch.cuda.synchronize()
    return decoded, logprobs, snaps


@pytest.fixture(scope="module")
def toy_table():
    return S.toy_table()


@pytest.mark.parametrize("cfg", S.toy_configs(), ids=lambda c: "n%d_b%d_lp%s_rp%s" % c)
def test_nbest_whole_search_vs_oracle(lib, toy_table, cfg):
    n, beams, lp, rp = cfg
    dec, lps, seen, log = S.toy_search(toy_table, beams, lp, n, rp)
    for b in range(S.TOY_B):                                # torch.topk defines no tie order: stored scores are apart
        v = sorted(x for x in lps[b].tolist() if x > -1e4)
        assert all(hi - lo > 1e-3 for lo, hi in zip(v, v[1:])), (cfg, b, v)
    if cfg == (3, 4, 0.6, 1.0):                             # what the tables were built for, on the oracle's run
        one = S.toy_search(toy_table, beams, lp, 1, rp)[3]
        assert max(log["short"]) >= 3 and sum(log["evicted"]) >= 1 and sum(log["rejected"]) >= 1
        assert one["done_at"][0] == 2 and log["done_at"][0] != 2
    decoded, logprobs, _ = _device_search(lib, toy_table, beams, lp, n, rp, seen)
    print(cfg, "max |logprob - oracle| = %.3g" % (logprobs.cpu() - lps).abs().max().item())
    assert torch.equal(decoded.cpu(), dec), (cfg, decoded.cpu(), dec)
    assert torch.allclose(logprobs.cpu(), lps, rtol=0, atol=1e-4), (cfg, logprobs.cpu(), lps)


@pytest.mark.parametrize("lp", [0.0, 0.6])
@pytest.mark.parametrize("beams", [1, 3, 4])
def test_nbest_hooks_with_one_slot_are_the_old_hooks_bit_for_bit(lib, toy_table, beams, lp):
    new = _device_search(lib, toy_table, beams, lp, 1, 1.0)
    old = _device_search(lib, toy_table, beams, lp, 1, 1.0, old_hooks=True)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1].view(torch.int32), old[1].view(torch.int32))
    for a, b in zip(new[2], old[2]):
        for k in a:
            ta, tb = a[k], b[k]
            if k == "hyp_ids":                              # columns behind a hypothesis's length are never written by either
                continue
            if ta.dtype == torch.float32:
                ta, tb = ta.view(torch.int32), tb.view(torch.int32)
            assert torch.equal(ta, tb), k
        ln = a["hyp_len"]
        for bb in range(S.TOY_B):
            assert torch.equal(a["hyp_ids"][bb, 0, :ln[bb, 0]], b["hyp_ids"][bb, 0, :ln[bb, 0]])


def test_nbest_hooks_refuse_bad_arguments(lib):
    from gitcap._lib import CDbgBeamBuffersNbest
    B, beams, L, K, V = 2, 2, 5, 4, 23
    t, _, bbn = beam_state(B, beams, 3, L)
    before = {k: v.clone() for k, v in t.items()}
    cs = torch.zeros(B, K, device="cuda")
    ci = torch.zeros(B, K, device="cuda", dtype=torch.int32)
    dec = torch.full((B, 3, L), -777, device="cuda", dtype=torch.int64)
    lp = torch.full((B, 3), float("nan"), device="cuda")
    step = lambda bb, cur_len=1, cur=0, beams=beams, K=K: lib.gitcap_dbg_beam_step_nbest(
        ctypes.byref(bb), ptr(cs), ptr(ci), B, beams, K, V, cur_len, L, 22, ctypes.c_float(0.6), cur, stream())
    for bad_n in (0, 17):
        bad = CDbgBeamBuffersNbest(*[getattr(bbn, f) for f, _ in CDbgBeamBuffersNbest._fields_[:-1]], bad_n)
        assert step(bad) == -1
        assert lib.gitcap_dbg_beam_finish_nbest(ctypes.byref(bad), B, L, 22, ptr(dec), ptr(lp), stream()) == -1
    assert step(bbn, cur_len=0) == -1 and step(bbn, cur_len=L) == -1 and step(bbn, cur=2) == -1
    assert step(bbn, beams=17) == -1 and step(bbn, K=17) == -1
    assert lib.gitcap_dbg_beam_finish_nbest(ctypes.byref(bbn), B, L, 22, None, ptr(lp), stream()) == -1
    torch.cuda.synchronize()
    for k in t:
        a, b = t[k], before[k]
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
    assert bool((dec == -777).all()) and bool(torch.isnan(lp).all())


def test_nbest_finish_orders_equal_scores_by_storage_and_pads_empty_ranks(lib):
    """Hand-made state: three stored hypotheses of four slots, two of them with the same score."""
    B, beams, n, L = 1, 1, 4, 6
    t, _, bbn = beam_state(B, beams, n, L)
    t["hyp_len"].copy_(torch.tensor([[2, 3, 1, 0]], dtype=torch.int32))
    t["hyp_score"].copy_(torch.tensor([[-1.5, -0.5, -1.5, 7.0]]))           # slot 3 is empty: its score is no score
    t["hyp_ids"][0, 0, :2] = torch.tensor([0, 4], device="cuda")
    t["hyp_ids"][0, 1, :3] = torch.tensor([0, 5, 6], device="cuda")
    t["hyp_ids"][0, 2, :1] = torch.tensor([0], device="cuda")
    dec = torch.full((B, n, L), -777, device="cuda", dtype=torch.int64)
    lp = torch.full((B, n), float("nan"), device="cuda")
    assert lib.gitcap_dbg_beam_finish_nbest(ctypes.byref(bbn), B, L, 22, ptr(dec), ptr(lp), stream()) == 0
    torch.cuda.synchronize()
    assert dec[0].tolist() == [[0, 5, 6, 22, 22, 22], [0, 4, 22, 22, 22, 22], [0, 22, 22, 22, 22, 22], [22] * 6]
    assert lp[0].tolist() == [-0.5, -1.5, -1.5, -1e5]


# ---- c. the recorded bits --------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _record(lib, toy_table):
    rec = {}
    for name in sorted(CASES):
        for tag, plain in (("pen", False), ("plain", True)):
            gs, gi = _run_pen(lib, CASES[name], plain=plain)
            rec["topk_%s_%s_idx" % (tag, name)] = gi.cpu().numpy()
            rec["topk_%s_%s_scores" % (tag, name)] = _bits(gs)
    runs = [("n%d_b%d_lp%s_rp%s" % c, c, False) for c in S.toy_configs()]
    runs += [("old_b%d_lp%s" % (c[1], c[2]), c, True) for c in S.toy_configs() if c[0] == 1 and c[3] == 1.0]
    for key, (n, beams, lp, rp), old in runs:
        decoded, logprobs, snaps = _device_search(lib, toy_table, beams, lp, n, rp, old_hooks=old)
        last = snaps[-1]
        rec["toy_%s_decoded" % key] = decoded.cpu().numpy()
        rec["toy_%s_logprobs" % key] = _bits(logprobs)
        rec["toy_%s_hyp_len" % key] = last["hyp_len"].cpu().numpy()
        rec["toy_%s_done" % key] = last["done"].cpu().numpy()
        rec["toy_%s_beam_scores" % key] = _bits(last["beam_scores"])
    return rec


def test_hooks_reproduce_the_recorded_parent_bits(lib, toy_table):
    """Every top-k case (penalised and plain) and every toy search (n-best hooks; the one-hypothesis hooks where n = 1, rp = 1):
    indices, ids and the bit patterns of every float equal the fixture.  GITCAP_WRITE_REGRESSION=dir writes it instead."""
    rec = _record(lib, toy_table)
    name = "device_search_options.npz"
    wdir = os.environ.get("GITCAP_WRITE_REGRESSION")
    if wdir:
        os.makedirs(wdir, exist_ok=True)
        np.savez_compressed(os.path.join(wdir, name), **rec)
        return
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    assert sorted(g.files) == sorted(rec)
    for k in sorted(rec):
        assert g[k].dtype == rec[k].dtype and np.array_equal(g[k], rec[k]), k
