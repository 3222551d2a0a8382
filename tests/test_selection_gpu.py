"""The token-selection kernels on the MI355X, each run alone through its gitcap_dbg_* hook and compared EXACTLY with the plain
restatement of tests/selection_reference.py (token ids and indices everywhere; values only where fp32 arithmetic is involved):

  a. the vocabulary head's per-tile arg-max partials (skinny.hip: logits_epilogue under both forms of the head kernel),
  b. argmax_final_kernel with and without its next-step embedding tail,
  c. draft_accept_kernel,
  d. beam_topk (chunks + merge),
  e. beam_init / beam_step / beam_finish driven as a whole search against oracle.search_oracle.beam_search.

Ties are exact by construction (identical operands give identical bits), never near-ties; everything else is kept far from a
tie, and for beam_topk that is asserted on the inputs (selection_reference.beam_candidates: gap) before the kernel is looked at."""
import ctypes

import numpy as np
import pytest
import torch

import selection_reference as R
from selection_reference import DRAFT_NT, DRAFT_SEP, draft_scenario, draft_scenarios
from oracle import search_oracle
from gpu_support import e4m3_rows, lib, ptr, run_vocab_head, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

NINF = float("-inf")
SENT = R.SENTINEL


# ---- a. vocabulary head -------------------------------------------------------------------------------------------------

def _tie_pairs(N):
    """Column pairs that hold identical weights and bias, one per level of the reduction: the two ends of the row, inside one
    lane's four columns, across lanes of a tile, across tiles."""
    t = ((N + 15) // 16 - 1) // 2
    pairs = [(0, N - 1), (16 * t + 4, 16 * t + 5), (16 * t + 9, 16 * t + 13), (2, 18)]
    assert all(0 <= a < b < N for a, b in pairs) and len({c for p in pairs for c in p}) == 8
    return pairs


def _head_inputs(M, N, K, variant, fp8, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Np = (N + 15) // 16 * 16
    ldx = K + 8 if M % 2 else K
    X = torch.randn(M, ldx, device="cuda", generator=g).bfloat16()
    Wf = torch.randn(Np, K, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(N, device="cuda", generator=g)
    pairs = _tie_pairs(N)
    ties = []
    for r in range(min(M, 4)):                      # row r's own tie: both columns hold bf16(X[r]), its largest logit by far
        n1, n2 = pairs[(r + variant) % 4]
        Wf[n1] = X[r, :K].float()
        Wf[n2] = X[r, :K].float()
        bias[n2] = bias[n1]
        ties.append((r, n1, n2))
    for i, n in enumerate(range(N, Np)):            # padding rows: a missing n < N guard would make them the arg-max
        Wf[n] = 4.0 * X[i % M, :K].float()
    if fp8:
        W, wscale, Weff = e4m3_rows(Wf)
    else:
        wscale = None
        W = Wf.bfloat16()
        Weff = W.float()
    return X, ldx, W, wscale, bias, Weff, ties


def _argmax_final(lib, val, idx, rows, nt):
    out = torch.full((rows,), -9, device="cuda", dtype=torch.int64)
    assert lib.gitcap_dbg_argmax_final(ptr(val), ptr(idx), nt, rows, 1, 0, ptr(out), 1, None, 0, -1, None, stream()) == 0
    return out.cpu().tolist()


def _head_check(lib, X, ldx, W, wscale, bias, Weff, M, N, K):
    """Both forms of the kernel: equal bits; partials == first arg-max of the logits the kernel wrote; logits ~ fp64 product;
    the token argmax_final makes of the partials == the first arg-max of the row.  Returns the logits (numpy)."""
    nt = (N + 15) // 16
    outs = [run_vocab_head(lib, X, ldx, W, wscale, bias, M, N, K, share=share)[:3] for share in (1, 0)]
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    logits, val, idx = outs[0]
    lg = logits.cpu().numpy()
    assert not np.isnan(lg).any()
    rv, ri = R.tile_partials(lg)
    assert np.array_equal(val.cpu().numpy().astype(np.float64), rv)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ri)
    ref = X[:, :K].double() @ Weff.double().t()[:, :N] + bias.double()
    assert torch.allclose(logits.double(), ref, rtol=1e-3, atol=1e-3), float((logits.double() - ref).abs().max())
    toks = _argmax_final(lib, val.contiguous(), idx.contiguous(), M, nt)
    assert toks == [R.argmax_partials(rv[m], ri[m]) for m in range(M)]
    assert toks == [int(np.argmax(lg[m])) for m in range(M)]                  # np.argmax: first occurrence
    return lg


def _head_case(lib, M, N, K, fp8=False):
    for variant in range(0, 4, min(M, 4)):          # fewer than four rows: rotate the kinds of tie over several launches
        X, ldx, W, wscale, bias, Weff, ties = _head_inputs(M, N, K, variant, fp8, seed=1000 * M + N + K + variant)
        lg = _head_check(lib, X, ldx, W, wscale, bias, Weff, M, N, K)
        for r, n1, n2 in ties:                      # the designed tie is there and is the row's maximum: the first column wins
            assert lg[r, n1] == lg[r, n2] == lg[r].max() and int(np.argmax(lg[r])) == min(n1, n2)
    # a row of equal logits (zero weights, constant bias; the padding columns would score 0 > -1.5): token 0
    Np = (N + 15) // 16 * 16
    W0 = torch.zeros(Np, K, device="cuda")
    ws0 = torch.ones(Np, device="cuda") if fp8 else None
    W0 = W0.to(torch.float8_e4m3fn) if fp8 else W0.bfloat16()
    bias0 = torch.full((N,), -1.5, device="cuda")
    lg = _head_check(lib, X, ldx, W0, ws0, bias0, torch.zeros(Np, K, device="cuda"), M, N, K)
    assert bool((lg == -1.5).all())


@pytest.mark.parametrize("K", [64, 128, 576, 768, 1024])
@pytest.mark.parametrize("N", [48, 64, 65, 997])
def test_vocab_head_partials(lib, N, K):
    """N = 48: three tiles, never the shared form; 64: the smallest shared launch; 65: a last tile with one valid column;
    997: a last workgroup with three active waves.  M = 1, 2 / 16, 17 / 33: one, two and three m-tiles (both LDS images)."""
    for M in (1, 2, 16, 17, 33):
        _head_case(lib, M, N, K)


@pytest.mark.parametrize("M,K", [(33, 768), (1, 576), (17, 1024), (2, 128), (16, 64)])
def test_vocab_head_partials_full_vocabulary(lib, M, K):
    _head_case(lib, M, 30522, K)


def test_vocab_head_partials_e4m3_weights(lib):
    for M in (1, 2, 16, 17, 33):
        _head_case(lib, M, 997, 128, fp8=True)


def test_vocab_head_rejects_bad_arguments(lib):
    x = torch.zeros(16, 64, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(64, device="cuda")
    i = torch.zeros(64, device="cuda", dtype=torch.int32)
    assert lib.gitcap_dbg_vocab_head(None, 64, ptr(x), None, None, 1, 16, 64, ptr(f), ptr(f), ptr(i), None) == -1
    assert lib.gitcap_dbg_vocab_head(ptr(x), 64, ptr(x), None, None, 1, 16, 96, ptr(f), ptr(f), ptr(i), None) == -1      # K not built
    assert lib.gitcap_dbg_vocab_head(ptr(x), 60, ptr(x), None, None, 1, 16, 64, ptr(f), ptr(f), ptr(i), None) == -1      # ldx < K
    assert lib.gitcap_dbg_vocab_head(ptr(x), 64, ptr(x), None, None, 1, 16, 64, ptr(f), ptr(f), None, None) == -1       # half a pair
    assert lib.gitcap_dbg_vocab_head(ptr(x), 64, ptr(x), ptr(f), None, 1, 16, 64, ptr(f), ptr(f), ptr(i), None) == -1     # e4m3 at K = 64


# ---- b. argmax_final ----------------------------------------------------------------------------------------------------

SEP = 5


def _partial_rows(nt, rng):
    """Hand-made rows of partials [(val, idx)]: unique maxima, exact ties at every distance the reduction has a level for, the
    winner at the first and at the last tile, equal rows, an empty row.  idx[t] = 16 t + 5 unless stated."""
    base = np.arange(nt, dtype=np.int64) * 16 + 5

    def fresh():
        return (rng.permutation(nt).astype(np.float32) / nt - 2.0), base.copy()       # distinct values in [-2, -1)
    rows = []
    v, i = fresh()
    rows.append((v, np.arange(nt, dtype=np.int64) * 16 + rng.integers(0, 16, nt)))
    v, i = fresh(); v[0] = 3.0; rows.append((v, i))
    v, i = fresh(); v[nt - 1] = 3.0; rows.append((v, i))
    # first and last tile; neighbouring lanes; two waves; one thread's next unrolled slot; one thread's second trip
    for d in (nt - 1, 1, 64, 256, 2048):
        if 0 < d < nt:
            for t in sorted({0, nt - 1 - d}):
                v, i = fresh(); v[t] = 3.0; v[t + d] = 3.0; rows.append((v, i))
    if nt > 300:                                    # three equal maxima: one thread (t, t + 256) and another wave (t + 70)
        v, i = fresh(); v[[7 + 256, 7 + 70, 7]] = 3.0; rows.append((v, i))
    rows.append((np.full(nt, 1.0, np.float32), base.copy()))                     # all equal: the first tile's index
    rows.append((np.full(nt, 1.0, np.float32), base[::-1].copy()))               # the stored index decides, not the position
    rows.append((np.full(nt, NINF, np.float32), np.full(nt, SENT, np.int64)))    # nothing above -inf: token 0
    return rows


def _argmax_final_case(lib, nt, D=0):
    rng = np.random.default_rng(nt + D)
    rows = _partial_rows(nt, rng)
    n = len(rows)
    stride, off, ld_out, step = 2, 1, 3, 2
    val = np.full((n * stride, nt), 9.0, np.float32)            # rows the launch must not read: larger values, index 7
    idx = np.full((n * stride, nt), 7, np.int64)
    for r, (v, i) in enumerate(rows):
        val[r * stride + off], idx[r * stride + off] = v, i
    want = [R.argmax_partials(v, i) for v, i in rows]
    assert want[1] == 5 and want[2] == 16 * (nt - 1) + 5 and want[-1] == 0 and want[-2] == 5 and want[-3] == 5
    d_val, d_idx = to_dev(val, torch.float32), to_dev(idx, torch.int32)
    out = torch.full((n, ld_out), -7, device="cuda", dtype=torch.int64)
    sep_cnt = to_dev([100, 200, 300, 400], torch.int32)
    emb = None
    if D:
        g = torch.Generator(device="cuda").manual_seed(D)
        vocab, position = 16 * nt, 3
        word = torch.randn(vocab, D, device="cuda", generator=g)
        pos = torch.randn(position + 2, D, device="cuda", generator=g)
        gamma, beta = torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)
        xf = torch.full((n + 1, D), float("nan"), device="cuda")
        xb = torch.full((n + 1, D), float("nan"), device="cuda", dtype=torch.bfloat16)
        from gitcap._lib import CDbgNextEmbed
        emb = CDbgNextEmbed(word.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, D, vocab, position,
                            xf.data_ptr(), xb.data_ptr())
    rc = lib.gitcap_dbg_argmax_final(ptr(d_val), ptr(d_idx), nt, n, stride, off, ptr(out), ld_out, ptr(sep_cnt), step, SEP,
                                     ctypes.byref(emb) if emb else None, stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    assert got[:, 0].tolist() == want
    assert bool((got[:, 1:] == -7).all())
    n_sep = sum(t == SEP for t in want)
    assert n_sep >= 2 and sep_cnt.cpu().tolist() == [100, 200, 300 + n_sep, 400]
    if D:
        x = word.double()[torch.tensor(want, device="cuda")] + pos.double()[position]
        ref = torch.nn.functional.layer_norm(x, (D,), gamma.double(), beta.double(), 1e-5)
        assert torch.allclose(xf[:n].double(), ref, rtol=1e-5, atol=1e-5), float((xf[:n].double() - ref).abs().max())
        assert torch.equal(xb[:n], xf[:n].bfloat16())
        assert bool(torch.isnan(xf[n]).all()) and bool(torch.isnan(xb[n].float()).all())


@pytest.mark.parametrize("nt", [1, 7, 8, 9, 257, 1908, 2049])
def test_argmax_final_hand_made_partials(lib, nt):
    """One thread; the 8-deep unroll; wave and workgroup boundaries; 1908 = the 30522-word vocabulary; a second trip of the
    256 * 8 loop.  Rows are read through row_stride / row_off, tokens written through ld_out; poison around both."""
    _argmax_final_case(lib, nt)


@pytest.mark.parametrize("D", [64, 576, 768, 1024])
@pytest.mark.parametrize("nt", [9, 257])
def test_argmax_final_next_embed(lib, nt, D):
    """NV = 1, 3, 3, 4 vectors per lane: xf == LayerNorm(word[token] + pos[position]) in fp64, xb == bf16(xf)."""
    _argmax_final_case(lib, nt, D)


# ---- c. draft_accept ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_draft_accept_vs_restatement(lib, B, n):
    rng = np.random.default_rng(100 * B + n)
    tok_scratch = torch.full((B * n,), -3, device="cuda", dtype=torch.int32)
    ticket = torch.zeros(1, device="cuda", dtype=torch.int32)
    seen_a = set()
    for a_rows, sep_at in draft_scenarios(B, n):          # every launch on the same ticket word
        tok, ids, val, idx = draft_scenario(B, n, a_rows, sep_at, rng)
        assert [R.argmax_partials(v, i) for v, i in zip(val, idx)] == tok.reshape(-1).tolist()
        want = R.draft_accept(tok, ids, DRAFT_SEP)
        assert want["a_r"] == a_rows                       # the inputs are what they were designed to be
        seen_a.add(want["a"])
        ld = ids.shape[1]
        d_ids = to_dev(ids, torch.int64)
        sep_cnt = torch.full((n + 2,), 77, device="cuda", dtype=torch.int32)
        host = (ctypes.c_int32 * 2)(-5, -5)
        d_val, d_idx = to_dev(val, torch.float32), to_dev(idx, torch.int32)
        rc = lib.gitcap_dbg_draft_accept(ptr(d_val), ptr(d_idx), DRAFT_NT, B, n, ptr(d_ids), ld, ptr(tok_scratch), ptr(ticket),
                                         ptr(sep_cnt), DRAFT_SEP, host, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert (host[0], host[1]) == want["host"]
        assert np.array_equal(d_ids.cpu().numpy(), want["ids"])          # rewritten columns, and everything else untouched
        assert sep_cnt.cpu().tolist() == want["sep_cnt"] + [77] * (n + 2 - want["covered"])
        assert tok_scratch.cpu().tolist() == tok.reshape(-1).tolist()
        assert int(ticket.item()) == 0
    assert {0, n} <= seen_a and (n < 2 or n // 2 in seen_a)


def test_draft_accept_fired_flag_cases(lib):
    """host[1]: SEP from all rows in one covered step -> 1; in different steps, or only beyond `covered` -> 0."""
    B, n = 2, 4
    for a_rows, sep_at, fired in [([4, 4], [(0, 1), (1, 1)], 1), ([4, 4], [(0, 1), (1, 2)], 0), ([1, 4], [(0, 2), (1, 2)], 0),
                                  ([1, 4], [(0, 1), (1, 1)], 1), ([1, 4], [(0, 0)], 0)]:
        rng = np.random.default_rng(7)
        tok, ids, val, idx = draft_scenario(B, n, a_rows, sep_at, rng)
        want = R.draft_accept(tok, ids, DRAFT_SEP)
        assert want["host"] == (min(a_rows), fired)
        d_ids = to_dev(ids, torch.int64)
        sep_cnt = torch.full((n + 2,), 77, device="cuda", dtype=torch.int32)
        scratch = torch.zeros(B * n, device="cuda", dtype=torch.int32)
        ticket = torch.zeros(1, device="cuda", dtype=torch.int32)
        host = (ctypes.c_int32 * 2)(-5, -5)
        d_val, d_idx = to_dev(val, torch.float32), to_dev(idx, torch.int32)
        assert lib.gitcap_dbg_draft_accept(ptr(d_val), ptr(d_idx), DRAFT_NT, B, n, ptr(d_ids), ids.shape[1], ptr(scratch), ptr(ticket),
                                           ptr(sep_cnt), DRAFT_SEP, host, stream()) == 0
        assert (host[0], host[1]) == want["host"] and np.array_equal(d_ids.cpu().numpy(), want["ids"])
        assert sep_cnt.cpu().tolist() == want["sep_cnt"] + [77] * (n + 2 - want["covered"])


# ---- d. beam_topk -------------------------------------------------------------------------------------------------------

def _bg(rng, rows, V):
    return rng.random((rows, V), dtype=np.float32) - 1.0           # background logits in [-1, 0)


def _spike(x, places, top=6.0, step=0.25):
    """places: (row, column) in the order of their logits top, top - step, ... (distinct: a collision is a mistake)"""
    assert len(set(places)) == len(places)
    for k, (r, v) in enumerate(places):
        x[r, v] = top - step * k


def _topk_cases():
    """name -> (logits [B*beams][V] fp32, beam_scores, beams, K).  Every case carries at least K + 1 spikes per clip where it
    is about winners, so the first K + 1 candidates are the designed ones."""
    rng = np.random.default_rng(2024)
    cases = {}
    # chunk edges: V around one 2048-logit chunk, two chunks, a short last chunk with empty slots
    for V, B, beams in [(2047, 2, 3), (2048, 2, 3), (2049, 2, 3), (4096, 2, 3), (2051, 1, 2)]:
        K = 8
        x = _bg(rng, B * beams, V)
        cols = []
        for c in (0, V - 1, 2047, 2048, 2046, 1, 2049, 2050, 255, 256, 1023, 300, 301, 1500, 700, 701, 2000):
            if c < V and c not in cols:
                cols.append(c)
        cols = cols[:K + 3]
        for b in range(B):
            _spike(x, [(b * beams + k % beams, cols[int(c)]) for k, c in enumerate(rng.permutation(len(cols)))])
        cases["edge_V%d" % V] = (x, rng.random(B * beams) - 1.0, beams, K)
    # 64 chunks
    V, beams, K = 131072, 2, 16
    x = _bg(rng, beams, V)
    cols = [0, V - 1, 2047, 2048, 129024, 129023, 65535, 65536, 4095, 4096, 100000, 77, 131071 - 256, 12345, 54321, 99999, 2, 3, 70000]
    _spike(x, [(k % beams, c) for k, c in enumerate(cols)], step=0.2)
    cases["nch64"] = (x, np.array([-0.3, 0.0]), beams, K)
    # all K winners inside one chunk, held by ONE thread (ids t + 256 q of chunk 1); K = 16: by two threads
    x = _bg(rng, 3, 4100)
    _spike(x, [(1, 2048 + 37 + 256 * q) for q in (3, 0, 7, 1, 6, 2, 5, 4)] + [(0, 9), (2, 4099), (1, 2048 + 38)])
    cases["one_thread_K8"] = (x, np.array([-0.5, 0.0, -0.25]), 3, 8)
    x = _bg(rng, 2, 6200)
    _spike(x, [(0, 2048 + (37 if q % 2 else 200) + 256 * (q // 2)) for q in rng.permutation(16)] + [(1, 0), (0, 5000), (1, 6199)], step=0.2)
    cases["two_threads_K16"] = (x, np.array([0.0, -0.1]), 2, 16)
    # -inf: a whole chunk, and scattered among valid logits; spikes next to masked columns
    x = _bg(rng, 4, 6144)
    x[0, 2048:4096] = NINF
    x[1][rng.random(6144) < 0.3] = NINF
    x[2, ::2] = NINF
    _spike(x, [(0, 2047), (1, 10), (0, 4096), (1, 6143), (0, 0), (1, 3000), (0, 6143), (1, 2048), (0, 1), (1, 4095)])
    _spike(x, [(2, 4097), (3, 2048), (2, 1), (3, 4095), (2, 6143), (3, 0), (2, 2049), (3, 6143), (2, 3), (3, 1000)])
    cases["neg_inf"] = (x, np.array([-0.2, 0.0, -0.4, -0.6, ]), 2, 8)
    # equal logits inside a row: one thread's registers, a chunk edge, the end of the row; then a second tied group
    x = _bg(rng, 2, 4100)
    x[0, [5, 5 + 256, 2047, 2048, 4099]] = 6.0
    x[1, [7, 8]] = 5.5
    x[0, 100], x[1, 200], x[0, 300] = 4.0, 3.5, 3.0
    cases["equal_logits"] = (x, np.array([0.0, -0.1]), 2, 8)
    cases["all_equal_row"] = (np.zeros((1, 300), np.float32), np.array([-1.0]), 1, 8)
    # two beams with identical rows and identical scores: the lower beam's candidate first, at every rank
    B, beams, V, K = 2, 3, 2500, 8
    x = _bg(rng, B * beams, V)
    for b in range(B):
        _spike(x, [(b * beams, int(c)) for c in rng.choice(V, 6, replace=False)], step=0.5)
        x[b * beams + 2] = x[b * beams]
        _spike(x, [(b * beams + 1, int(c)) for c in rng.choice(V, 3, replace=False)], top=4.1, step=0.5)
    cases["twin_beams"] = (x, np.array([-0.5, -1.0, -0.5, -0.25, -2.0, -0.25]), beams, K)
    # the first step of a search: identical rows, scores [0, -1e9, ...]: every candidate comes from beam 0
    B, beams, V, K = 3, 4, 2500, 8
    x = _bg(rng, B * beams, V)
    for b in range(B):
        _spike(x, [(b * beams, int(c)) for c in rng.choice(V, K + 3, replace=False)])
        x[b * beams + 1:(b + 1) * beams] = x[b * beams]
    cases["first_step"] = (x, np.tile(np.array([0.0, -1e9, -1e9, -1e9]), B), beams, K)
    # shapes
    for B, beams, K in [(5, 1, 1), (2, 3, 2), (3, 4, 8), (1, 16, 16), (2, 16, 1), (5, 4, 2)]:
        V = 2300
        x = _bg(rng, B * beams, V)
        for b in range(B):
            cols = rng.choice(V, K + 3, replace=False)
            _spike(x, [(b * beams + int(rng.integers(0, beams)), int(c)) for c in cols], step=0.3)
        cases["shape_B%d_b%d_K%d" % (B, beams, K)] = (x, -rng.random(B * beams), beams, K)
    # fewer than K candidates: the sentinel
    x = np.full((2, 64), NINF, np.float32)
    x[0, [3, 17, 40, 41, 63]] = [0.5, 2.0, -1.0, 1.0, 0.0]
    cases["few_finite_V64"] = (x, np.array([0.0, -1.0]), 1, 16)
    x = np.full((2, 2051), NINF, np.float32)
    x[0, [2048, 2049, 2050, 5, 1000]] = [1.0, 0.0, 2.0, 3.0, -1.0]
    cases["few_finite_V2051"] = (x, np.array([-0.5, 0.0]), 2, 16)
    return cases


TOPK_CASES = _topk_cases()


def _run_topk(lib, x, bs, beams, K, pad=3):
    rows, V = x.shape
    B = rows // beams
    ld = V + pad
    buf = np.full((rows, ld), 1e30, np.float32)                    # row padding the kernel must not read
    buf[:, :V] = x
    d_x, d_bs = to_dev(buf, torch.float32), to_dev(bs, torch.float32)
    out_s = torch.full((B * K + 4,), float("nan"), device="cuda")
    out_i = torch.full((B * K + 4,), -5, device="cuda", dtype=torch.int32)
    rc = lib.gitcap_beam_topk(ptr(d_x), ld, ptr(d_bs), B, beams, V, K, ptr(out_s), ptr(out_i), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(out_s[B * K:]).all()) and bool((out_i[B * K:] == -5).all())
    return out_s[:B * K].view(B, K).cpu().numpy(), out_i[:B * K].view(B, K).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name", sorted(TOPK_CASES))
def test_beam_topk_vs_restatement(lib, name):
    x, bs, beams, K = TOPK_CASES[name]
    bs32 = np.asarray(bs, np.float32)
    ws, wi, gap = R.beam_candidates(x, bs32, beams, K)
    assert float(gap.min()) > 1e-3, (name, gap)              # a condition on the INPUTS: apart from the exact ties nothing is close
    B = x.shape[0] // beams
    if name.startswith("few_finite"):
        assert (wi == SENT).any()
    else:
        assert not (wi == SENT).any()
    if name == "first_step":
        assert (wi < x.shape[1]).all()                       # every candidate from beam 0
    if name == "twin_beams":
        V = x.shape[1]
        assert all(wi[b, 1] == wi[b, 0] + 2 * V and ws[b, 1] == ws[b, 0] for b in range(B))
    if name == "one_thread_K8":
        assert sorted(wi[0].tolist()) == [4100 + 2048 + 37 + 256 * q for q in range(8)]
    gs, gi = _run_topk(lib, x, bs32, beams, K)
    assert np.array_equal(gi, wi), (name, gi, wi)
    live = wi != SENT
    assert np.allclose(gs[live], ws[live], rtol=0, atol=1e-4), (name, np.abs(gs[live] - ws[live]).max())
    assert bool((gs[~live] == NINF).all())


def test_beam_topk_refuses_more_than_64_chunks(lib):
    V = 131073
    x = torch.zeros(1, V, device="cuda")
    bs = torch.zeros(1, device="cuda")
    out_s = torch.full((8,), float("nan"), device="cuda")
    out_i = torch.full((8,), -5, device="cuda", dtype=torch.int32)
    assert lib.gitcap_beam_topk(ptr(x), V, ptr(bs), 1, 1, V, 8, ptr(out_s), ptr(out_i), stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out_s).all()) and bool((out_i == -5).all())          # nothing was launched


# ---- e. beam bookkeeping ------------------------------------------------------------------------------------------------

BEAM_V, BEAM_EOS, BEAM_CLS, BEAM_B, BEAM_MAXLEN = 23, 22, 0, 3, 7


def _beam_table(seed):
    """Logits by (clip, position % 8, last token): tests/test_search.py's _toy_step with one table per clip, so that the
    clips of a batch finish at different steps.  Clip 0: EOS is the best candidate of step 1 (the search of that clip is
    done at step 2); clip 2: EOS towers over every row of step 3; clip 1: plain (runs into the cut at max_len)."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(BEAM_B, 8, BEAM_V, BEAM_V, generator=g) * 2.0
    table[0, 0, BEAM_CLS, BEAM_EOS] = 12.0
    table[2, 2, :, BEAM_EOS] = 9.0
    return table


def _oracle_search(table, beams, lp, monkeypatch):
    """-> (decoded, logprobs, prefixes per step as the oracle's step function saw them, rejected, done_at)"""
    seen, log = [], {"rejected": 0, "kept": 0}

    class Hyp(search_oracle.BeamHypotheses):
        def add(self, hyp, s):
            before = len(self.hyp) and self.hyp[0][0]
            had = len(self.hyp)
            super().add(hyp, s)
            if had:
                log["rejected" if self.hyp[0][0] == before else "kept"] += 1

    monkeypatch.setattr(search_oracle, "BeamHypotheses", Hyp)
    clip = torch.arange(BEAM_B * beams) // beams

    def step(ids):
        seen.append(ids.clone())
        return table[clip, (ids.shape[1] - 1) % 8, ids[:, -1] % BEAM_V].clone()
    dec, lps, _ = search_oracle.beam_search(torch.full((BEAM_B, 1), BEAM_CLS), step, eos_index=BEAM_EOS, max_steps=BEAM_MAXLEN,
                                            beam_size=beams, per_node_beam_size=2, length_penalty=lp)
    return dec, lps, seen, log


@pytest.mark.parametrize("lp", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("beams", [1, 3, 4])
def test_beam_bookkeeping_whole_search_vs_oracle(lib, monkeypatch, beams, lp):
    from gitcap._lib import CDbgBeamBuffers
    B, V, L, K = BEAM_B, BEAM_V, BEAM_MAXLEN, 2 * beams
    rows = B * beams
    table = _beam_table(31 * beams)
    dec, lps, seen, log = _oracle_search(table, beams, lp, monkeypatch)
    d_table = table.cuda()
    clip = torch.arange(rows, device="cuda") // beams
    i64 = dict(device="cuda", dtype=torch.int64)
    i32 = dict(device="cuda", dtype=torch.int32)
    ids = [torch.full((rows, L), -777, **i64), torch.full((rows, L), -777, **i64)]
    words, hyp_ids = torch.full((rows,), -777, **i64), torch.full((B, L), -777, **i64)
    scores, hyp_score = torch.full((rows,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
    src_rows, done, hyp_len = torch.full((rows,), -777, **i32), torch.full((B,), -777, **i32), torch.full((B,), -777, **i32)
    bb = CDbgBeamBuffers(ids[0].data_ptr(), ids[1].data_ptr(), words.data_ptr(), hyp_ids.data_ptr(), scores.data_ptr(),
                         hyp_score.data_ptr(), src_rows.data_ptr(), done.data_ptr(), hyp_len.data_ptr())
    assert lib.gitcap_dbg_beam_init(ctypes.byref(bb), B, beams, L, BEAM_CLS, stream()) == 0
    torch.cuda.synchronize()
    assert ids[0][:, 0].tolist() == [BEAM_CLS] * rows and words.tolist() == [BEAM_CLS] * rows
    assert bool((ids[0][:, 1:] == -777).all()) and bool((ids[1] == -777).all())
    assert scores.tolist() == [0.0 if r % beams == 0 else -1e9 for r in range(rows)]
    assert src_rows.tolist() == list(range(rows)) and done.tolist() == [0] * B and hyp_len.tolist() == [0] * B
    assert hyp_score.tolist() == [0.0] * B
    cs = torch.empty(B, K, device="cuda")
    ci = torch.empty(B, K, **i32)
    cur, done_at = 0, {}
    for cur_len in range(1, L):
        assert torch.equal(ids[cur][:, :cur_len].cpu(), seen[cur_len - 1]) if cur_len - 1 < len(seen) else True
        logits = d_table[clip, (cur_len - 1) % 8, words % V].contiguous()
        assert lib.gitcap_beam_topk(ptr(logits), V, ptr(scores), B, beams, V, K, ptr(cs), ptr(ci), stream()) == 0
        torch.cuda.synchronize()
        assert bool(((ci >= 0) & (ci < beams * V)).all())               # never hand beam_step the sentinel
        old = ids[cur].clone()
        assert lib.gitcap_dbg_beam_step(ctypes.byref(bb), ptr(cs), ptr(ci), B, beams, K, V, cur_len, L, BEAM_EOS,
                                        ctypes.c_float(lp), cur, stream()) == 0
        torch.cuda.synchronize()
        new, src = ids[cur ^ 1], src_rows.long()
        assert bool(((src >= 0) & (src < rows)).all())
        assert torch.equal(new[:, :cur_len], old[src, :cur_len])        # the gathered prefixes
        assert torch.equal(new[:, cur_len], words) and bool((new[:, cur_len + 1:] == -777).all())
        assert torch.equal(ids[cur], old)                               # the source buffer is only read
        if cur_len < len(seen):                                         # the oracle's next step saw exactly these prefixes
            assert torch.equal(new[:, :cur_len + 1].cpu(), seen[cur_len])
        for b in range(B):
            if done[b].item() and b not in done_at:
                done_at[b] = cur_len
                # a finished clip is padded: (score 0, EOS, row 0)
            if b in done_at or cur_len + 1 == L:
                sl = slice(b * beams, (b + 1) * beams)
                assert words[sl].tolist() == [BEAM_EOS] * beams and src_rows[sl].tolist() == [0] * beams
                assert scores[sl].tolist() == [0.0] * beams
        cur ^= 1
    decoded = torch.full((B, L), -777, **i64)
    logprobs = torch.full((B,), float("nan"), device="cuda")
    assert lib.gitcap_dbg_beam_finish(ctypes.byref(bb), B, L, BEAM_EOS, ptr(decoded), ptr(logprobs), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(decoded.cpu(), dec)
    assert torch.allclose(logprobs.cpu(), lps.view(-1), rtol=0, atol=1e-4)
    # the table did what it was built for: EOS first in clip 0 (its search stops early), clips finish at different steps,
    # and a later hypothesis failed to beat the stored one somewhere
    assert dec[0].tolist() == [BEAM_CLS] + [BEAM_EOS] * (L - 1) and done_at.get(0) == 2
    assert int((dec[1] != BEAM_EOS).sum()) != int((dec[2] != BEAM_EOS).sum())
    if beams > 1:
        assert log["rejected"] >= 1
