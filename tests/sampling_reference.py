"""Plain fp64 restatements for sampling on the device (include/gitcap.h: gitcap_attach_sampling), the inputs the tests share, and
the bounds the GPU tests hold the kernel to.

The draw contract: Philox4x32-10 (Salmon et al., SC'11: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 /
0xBB67AE85, ten rounds), key = the two words of the seed, counter = (v // 4, row, cur_len, 0), lane v % 4 -> column v;
u = ((x >> 8) + 0.5) * 2^-24; key_v = z_v - log(-log u_v) over the kept columns of the filtered row z; the pn largest keys, descending,
ties to the smaller column, are the draws.  The filter itself is NOT restated: draw_rows calls
oracle.search_oracle.top_k_top_p_filtering(min_tokens_to_keep=2) on the fp64 row.

Bounds (eps = 2^-24, the unit roundoff of fp32; the device's logf / expf / log1pf are taken as 2 ulp, its divide and multiply as
correctly rounded; fp64 is exact by comparison):
  z        the penalty and the temperature are one fp32 rounding each:                      |dz| <= 2 eps |z|
  sums     a thread adds ceil(V / 1024) terms, the wave butterfly 6, the block 16; each term expf(z - M) carries 2 ulp of expf, one
           rounding of the difference and the error of its two operands:
           rel_sum = (ceil(V / 1024) + 22 + 2) eps + eps * range + 4 eps * zmax            (range = max z - min kept z, zmax = max |z|)
  key      E = -logf(u) or -log1pf(-(1 - u)) with u or 1 - u exact: 2 eps relative; logf(E): that plus 2 ulp of the result; one
           rounding of the difference:      key_bound = eps (2 |z| + 2 + 2 |log E| + |key|) <= eps (3 zmax + 2 + 3 * 17.33 + ...)
           (|log E| <= log(2^25) = 17.33).  Two keys closer than 2 * key_bound are undecidable.
  top_p    the kept test compares mass / Z with top_p: both sums carry rel_sum, the product top_p * Z one rounding:
           p_bound = 2 * rel_sum + eps.  A cumulative mass closer to top_p than p_bound is undecidable.
  top_k    the k'-th and (k'+1)-th largest values decide the cut; equal fp64 values come from equal inputs and stay equal in fp32;
           different ones closer than 2 * 2 eps * zmax may merge or swap: undecidable.
  score    (z_w - logZ) + beam_score, logZ = M + logf(S): rel_sum from S, 2 ulp of logf, one rounding per operation, dz:
           score_bound = rel_sum + eps (2 |log S| + |logZ| + |z_w - logZ| + |score| + 2 |z_w|);  logz_bound = rel_sum + eps (2 |log S| + |logZ|)
"""
import math

import numpy as np
import torch

from oracle import search_oracle

EPS = 2.0 ** -24
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint32 array [..., 4]; key: (k0, k1) -> uint32 [..., 4]."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(seed, row, cur_len, V):
    """u_v of one row at one step, fp64 (exact): [V]."""
    seed = int(seed) & (2 ** 64 - 1)
    nblk = (V + 3) // 4
    ctr = np.zeros((nblk, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(nblk)
    ctr[:, 1] = row
    ctr[:, 2] = cur_len
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:V]
    return ((x >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def _top(keys, n):
    """columns of the n largest keys, descending, ties to the smaller column; -inf keys are no candidates"""
    order = np.lexsort((np.arange(len(keys)), -keys))
    return [int(v) for v in order[:n] if keys[v] > -np.inf]


def filter_by_value(z, top_k, top_p):
    """The rule of include/gitcap.h stated by value (fp64): -> filtered row."""
    z = np.array(z, dtype=np.float64)
    V = len(z)
    if top_k > 0:
        kth = np.sort(z)[::-1][min(max(top_k, 2), V) - 1]
        z[z < kth] = -np.inf
    if top_p < 1.0:
        p = np.exp(z - z.max())
        p /= p.sum()
        keep = np.zeros(V, bool)
        for v in range(V):
            gt = z > z[v]
            keep[v] = z[v] > -np.inf and (gt.sum() < 3 or p[gt].sum() <= top_p)
        z[~keep] = -np.inf
    return z


def draw_rows(logits, beam_scores, prefix, rp, T, top_k, top_p, seed, cur_len, pn):
    """logits [rows, V]; prefix [rows, >= cur_len] ints or None.  -> dict of words [rows][<= pn], scores, kept, logz and, per row, the
    margins and bounds of the module docstring (key_margin / key_bound, cut_margin / cut_bound, score_bound, logz_bound)."""
    logits = np.asarray(logits)
    rows, V = logits.shape
    rp, T, top_p = float(np.float32(rp)), float(np.float32(T)), float(np.float32(top_p))
    out = dict(words=[], scores=[], kept=[], logz=[], key_margin=[], key_bound=[], cut_margin=[], cut_bound=[], score_bound=[],
               logz_bound=[], z=[])
    for r in range(rows):
        z = logits[r].astype(np.float64)
        if rp != 1.0:
            for t in set(int(i) for i in prefix[r][:cur_len]):
                if 0 <= t < V:
                    z[t] = z[t] * rp if z[t] < 0 else z[t] / rp
        if T != 1.0:
            z = z / T
        zf = search_oracle.top_k_top_p_filtering(torch.from_numpy(z)[None], top_k=top_k, top_p=top_p, min_tokens_to_keep=2)[0].numpy()
        kept = zf > -np.inf
        fin = z[z > -np.inf]
        zmax = float(np.abs(fin).max())
        m = float(zf.max())
        S = float(np.exp(zf[kept] - m).sum())
        logz = m + math.log(S)
        rel_sum = (math.ceil(V / 1024) + 24) * EPS + EPS * float(fin.max() - fin.min()) + 4 * EPS * zmax
        # the cut
        cut_margin, cut_bound = np.inf, 0.0
        s = np.sort(z)[::-1]
        if top_k > 0:
            kk = min(max(top_k, 2), V)
            if kk < V and s[kk - 1] > s[kk] > -np.inf:
                cut_margin, cut_bound = float(s[kk - 1] - s[kk]), 4 * EPS * zmax
            s = np.where(s >= s[kk - 1], s, -np.inf)
        if top_p < 1.0:
            p = np.exp(s - s[0])
            cum = np.cumsum(p / p.sum())
            d = float(np.abs(cum[2:] - top_p).min()) if V > 2 else np.inf
            pb = 2 * rel_sum + EPS
            if d / pb < cut_margin / max(cut_bound, 1e-300):
                cut_margin, cut_bound = d, pb
        # the draw
        E = -np.log(uniforms(seed, r, cur_len, V))
        key = np.where(kept, zf - np.log(E), -np.inf)
        words = _top(key, pn)
        ks = np.sort(key[kept])[::-1][:pn + 1]
        out["key_margin"].append(float(np.min(ks[:-1] - ks[1:])) if len(ks) > 1 else np.inf)
        out["key_bound"].append(EPS * (3 * zmax + 2 + 3 * 17.33 + 17.33))
        sc = [float((zf[w] - logz) + float(beam_scores[r])) for w in words]
        out["score_bound"].append([rel_sum + EPS * (2 * abs(math.log(S)) + abs(logz) + abs(zf[w] - logz) + abs(x) + 2 * abs(zf[w]))
                                   for w, x in zip(words, sc)])
        out["logz_bound"].append(rel_sum + EPS * (2 * abs(math.log(S)) + abs(logz)))
        out["words"].append(words); out["scores"].append(sc); out["kept"].append(int(kept.sum())); out["logz"].append(logz)
        out["cut_margin"].append(cut_margin); out["cut_bound"].append(cut_bound); out["z"].append(zf)
    return out


def decidable(d, r):
    """row r of a draw_rows result: (the filter's cut is decidable, the draws are decidable given the cut)"""
    return d["cut_margin"][r] > d["cut_bound"][r], d["key_margin"][r] > 2 * d["key_bound"][r]


def layout(words, scores, B, beams, pn, V):
    """rows of draws -> the candidates of include/gitcap.h: [B][K] flat indices and scores (model.py:548-552)."""
    K = beams * pn
    ci = np.zeros((B, K), np.int64)
    cs = np.zeros((B, K), np.float64)
    for b in range(B):
        for p in range(K):
            ci[b, p] = (p % beams) * V + words[b * beams + p // pn][p % pn]
            cs[b, p] = scores[b * beams + p // pn][p % pn]
    return ci, cs


def multinomial_from_philox(seed, cur_len=1):
    """A stand-in for torch.multinomial(probs [rows, V], num_samples, ...) that returns the contract's draws for successive steps
    (log p - log E orders as the keys do: log p = z - logZ)."""
    state = {"cur_len": cur_len}

    def multinomial(probs, num_samples, replacement=False, *, generator=None):
        p = probs.detach().cpu().double().numpy()
        rows, V = p.shape
        out = np.zeros((rows, num_samples), np.int64)
        with np.errstate(divide="ignore"):
            for r in range(rows):
                key = np.log(p[r]) - np.log(-np.log(uniforms(seed, r, state["cur_len"], V)))
                w = _top(key, num_samples)
                assert len(w) == num_samples, "fewer kept columns than draws"
                out[r] = w
        state["cur_len"] += 1
        return torch.from_numpy(out).to(probs.device)
    return multinomial


# ---- the bookkeeping for UNSORTED candidates (oracle/search_oracle.py:124-146), on the device's state, fp32 scores ----------------

class Book:
    """The beam state the device keeps (csrc/search.hip: BeamState) and one sampled step / the finish on it."""

    def __init__(self, B, beams, n, L, cls, eos, lp):
        self.B, self.beams, self.n, self.L, self.eos, self.lp = B, beams, n, L, eos, np.float32(lp)
        self.ids = [[cls] for _ in range(B * beams)]
        self.beam_scores = [np.float32(0.0 if r % beams == 0 else -1e9) for r in range(B * beams)]
        self.words = [cls] * (B * beams)
        self.src_rows = list(range(B * beams))
        self.done = [False] * B
        self.hyps = [[] for _ in range(B)]           # (score, ids) in storage order

    def _add(self, b, ids, s, cur_len):
        score = np.float32(s) / np.float32(cur_len) ** self.lp
        h = self.hyps[b]
        if len(h) < self.n:
            h.append((score, list(ids)))
            return
        e = min(range(len(h)), key=lambda i: (h[i][0], i))      # the earliest stored of equal minima
        if score > h[e][0]:
            del h[e]
            h.append((score, list(ids)))

    def step(self, cs, ci, V, cur_len):
        beams, pad = self.beams, (np.float32(0.0), self.eos, 0)
        new = []
        for b in range(self.B):
            h = self.hyps[b]
            if not self.done[b] and len(h) == self.n:
                best = max(np.float32(x) for x in cs[b])
                self.done[b] = bool(min(s for s, _ in h) >= best / np.float32(self.L - 1) ** self.lp)
            kept = []
            if not self.done[b]:
                for s, idx in zip(cs[b], ci[b]):
                    beam_id, word = divmod(int(idx), V)
                    if word == self.eos or cur_len + 1 == self.L:
                        self._add(b, self.ids[b * beams + beam_id][:cur_len], s, cur_len)
                    else:
                        kept.append((np.float32(s), word, b * beams + beam_id))
                    if len(kept) == beams:
                        break
            new += kept + [pad] * (beams - len(kept))
        self.beam_scores = [x[0] for x in new]
        self.words = [x[1] for x in new]
        self.src_rows = [x[2] for x in new]
        self.ids = [self.ids[x[2]][:cur_len] + [x[1]] for x in new]

    def finish(self):
        dec = np.full((self.B, self.n, self.L), self.eos, np.int64)
        lps = np.full((self.B, self.n), -1e5, np.float32)
        for b, h in enumerate(self.hyps):
            for k, i in enumerate(sorted(range(len(h)), key=lambda i: (-h[i][0], i))):
                dec[b, k, :len(h[i][1])] = h[i][1]
                lps[b, k] = h[i][0]
        return dec, lps


# ---- shared inputs ------------------------------------------------------------------------------------------------------------

_REF = {}


def gaussian_rows(seed, rows, V, scale):
    """Gaussian logits: scale 4 gives a peaked row, 0.25 a flat one."""
    return (np.random.default_rng(seed).standard_normal((rows, V)) * scale).astype(np.float32)


def row_cases():
    """The gitcap_sample_rows cases: the real vocabulary (30522) and the widest row the kernel holds (32768) or its tail (2048 +-1, 5),
    B x beams, pn, the filters, temperatures, a penalty with a repeating and an out-of-range prefix id, -inf columns, ld > V."""
    cases = []
    shapes = [(1, 1), (2, 4), (3, 2)]
    n = 0
    for V in (5, 2047, 2048, 2049, 30522, 32768):
        for top_k, top_p in ((0, 1.0), (1, 1.0), (5, 1.0), (V, 1.0), (V + 7, 1.0), (0, 0.9), (0, 0.5), (0, 1e-6), (5, 0.9)):
            B, beams = shapes[n % 3]
            pn = 2 if (top_p < 1.0 or 0 < top_k < 4 or n % 2 == 0 or beams * 4 > 16 or V < 8) else 4
            T = (1.0, 0.7, 2.0)[n % 3]
            rp = (1.0, 1.3)[(n // 3) % 2]
            scale = (4.0, 0.25)[(n // 2) % 2]
            if top_p < 1.0 and V > 4096:    # a flat row this wide has cumulative masses ~3e-5 apart, a few p_bounds: nearly every row
                scale = 6.0 * T             # would be undecidable on the reference alone; the top-p cases there use a row peaked after
                                            # the temperature (sigma 6: 0.9 of the mass lies in a few dozen columns)
            rows = B * beams
            cur_len = 1 + n % 5
            rng = np.random.default_rng(5000 + n)
            prefix = rng.integers(0, V, size=(rows, 6))
            prefix[:, 1] = prefix[:, 0]                       # a repeated token
            prefix[:, 2] = V + 3                              # outside the vocabulary
            prefix[-1, 0] = -1
            bs = rng.uniform(-5, 0, size=rows).astype(np.float32)
            for attempt in range(16):       # the first input seed whose rows are all decidable ON THE REFERENCE (module docstring)
                x = gaussian_rows(1000 + n + 1000 * attempt, rows, V, scale)
                if n % 4 == 1 and V > 8:
                    x[0, 1::3] = -np.inf
                c = dict(id="V%d_k%d_p%g_B%dx%d_pn%d_T%g_rp%g" % (V, top_k, top_p, B, beams, pn, T, rp), x=x, bs=bs, prefix=prefix,
                         cur_len=cur_len, B=B, beams=beams, pn=pn, T=T, rp=rp, top_k=top_k, top_p=top_p, seed=0x9E3779B97F4A7C15 + n,
                         pad=(0, 3)[n % 2])
                _REF.pop(c["id"], None)
                d = case_reference(c)
                if all(all(decidable(d, r)) for r in range(rows)):
                    break
            cases.append(c)
            n += 1
    return cases


def case_reference(c):
    """draw_rows of a case, computed once and shared."""
    if c["id"] not in _REF:
        _REF[c["id"]] = draw_rows(c["x"], c["bs"], c["prefix"], c["rp"], c["T"], c["top_k"], c["top_p"], c["seed"], c["cur_len"], c["pn"])
    return _REF[c["id"]]


# a toy decoder for whole searches: logits depend on (clip, step, last word); EOS is likely, so draws end beams early
TOY_V, TOY_EOS, TOY_CLS, TOY_B, TOY_L = 23, 22, 0, 3, 7


def toy_table(seed=77):
    t = np.random.default_rng(seed).standard_normal((TOY_B, 8, TOY_V, TOY_V)).astype(np.float32) * 1.5
    t[:, :, :, TOY_EOS] += 2.5
    t[1, 1:, :, TOY_EOS] += 4.0                              # clip 1: nearly every draw after step 1 is EOS
    return t


def toy_logits(table, words, beams, cur_len):
    clip = np.arange(len(words)) // beams
    return table[clip, (cur_len - 1) % 8, np.asarray(words) % TOY_V]


def toy_candidates(table, book, beams, pn, rp, T, top_k, top_p, seed, cur_len, forced=None):
    """The candidates of one toy step from the restated draw on `book`'s state: (ci [B][K], cs [B][K]); forced {(cur_len, row): words}
    replaces a row's draws (scores follow the words)."""
    x = toy_logits(table, book.words, beams, cur_len)
    d = draw_rows(x, book.beam_scores, book.ids, rp, T, top_k, top_p, seed, cur_len, pn)
    for (cl, r), w in (forced or {}).items():
        if cl == cur_len:
            d["words"][r] = list(w)
            d["scores"][r] = [float((d["z"][r][v] - d["logz"][r]) + float(book.beam_scores[r])) for v in w]
    return layout(d["words"], d["scores"], len(book.done), beams, pn, TOY_V)
