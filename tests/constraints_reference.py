"""Plain restatement of the three hard constraints of gitcap_attach_constraints (include/gitcap.h), written with loops and
comparisons only -- no tensor op that could hide an off-by-one:

  n-gram   (HF NoRepeatNGramLogitsProcessor): ban prefix[i + n - 1] for every i in 0 .. cur_len - n whose n - 1 tokens
           prefix[i .. i + n - 2] equal the last n - 1 tokens prefix[cur_len - n + 1 .. cur_len - 1];
  length   (HF MinLengthLogitsProcessor): ban sep_id while cur_len < min_length;
  suppress (HF SuppressTokensLogitsProcessor): ban the listed ids at every step.

Ids are compared as values; an id outside [0, V) bans nothing.  The ban mask is uint16 [rows][ld_mask]: bit c & 15 of word c >> 4
set = column c banned, ld_mask even and >= ceil(V / 16)."""
import numpy as np


def banned_columns(prefix, cur_len, n, min_length, sep_id, suppress, V):
    """-> the set of banned columns of one row; prefix: the row's ids, of which the first cur_len count."""
    out = set()
    if n >= 1:
        i = 0
        while i <= cur_len - n:
            same = True
            for j in range(n - 1):
                if int(prefix[i + j]) != int(prefix[cur_len - n + 1 + j]):
                    same = False
            if same:
                out.add(int(prefix[i + n - 1]))
            i += 1
    if cur_len < min_length:
        out.add(int(sep_id))
    for s in suppress:
        out.add(int(s))
    return {c for c in out if 0 <= c < V}


def mask_ld(V):
    w = (V + 15) // 16
    return w + (w & 1)


def ban_mask(prefixes, cur_len, n, min_length, sep_id, suppress, V, ld_mask=None):
    """-> uint16 [rows][ld_mask] for the rows of `prefixes` [rows][>= cur_len]."""
    ld = mask_ld(V) if ld_mask is None else ld_mask
    out = np.zeros((len(prefixes), ld), dtype=np.uint16)
    for r, p in enumerate(prefixes):
        for c in banned_columns(p, cur_len, n, min_length, sep_id, suppress, V):
            out[r, c >> 4] |= np.uint16(1 << (c & 15))
    return out


def mask_logits(logits, mask):
    """A copy of logits [rows][V] (numpy, any float type) with -inf at the columns the mask bans."""
    out = np.array(logits, copy=True)
    rows, V = out.shape
    for r in range(rows):
        for w in range((V + 15) // 16):
            word = int(mask[r, w])
            bit = 0
            while word:
                if word & 1 and w * 16 + bit < V:
                    out[r, w * 16 + bit] = -np.inf
                word >>= 1
                bit += 1
    return out


def repeats_ngram(ids, n):
    """True when the sequence holds the same n-gram twice."""
    seen = set()
    for i in range(len(ids) - n + 1):
        g = tuple(int(v) for v in ids[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False


# ---- the inputs the GPU test of the mask builder uses; tests/test_constraints.py shows that they tell the wrong builders apart ----

def builder_cases(V):
    """(name, prefixes int64 [rows][L], cur_len, n, min_length, sep_id, suppress).  Run IN ORDER on ONE buffer: the second and the
    third case have other, and fewer, bans than the one before."""
    L = 12
    a = np.array([[1, 0, 15, 16, V - 1, 0, 15, 7, 0, 15, 16, 3],            # 3-gram (0, 15, 16) thrice-started; columns 0, 15, 16, V - 1
                  [1, 5, 6, 5, 6, 5, 9, 9, 9, 2, 5, 6],
                  [1, -1, V, -1, V, 4, -1, V, 2, 2, 2, 2]], dtype=np.int64)   # ids outside the vocabulary
    b = np.array([[1, 16, 15, 0, 16, 15, V - 1, 16, 15, 3, 3, 3],
                  [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12],
                  [1, V - 1, V - 1, V - 1, V - 1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int64)
    return [
        ("ngram3 + min_length + suppress", a, 11, 3, 12, 2, [0, 15, 16, V - 1, -1, V, 15]),
        ("ngram2, another prefix", b, 9, 2, 0, 2, []),
        ("fewer bans", b, 6, 4, 6, 2, []),
        ("n = 1", a, 7, 1, 0, 2, [V - 1]),
        ("n larger than the prefix", a, 3, 5, 0, 2, []),
        ("cur_len + 1 == n", a, 3, 4, 0, 2, []),
        ("min_length at cur_len = m", a, 5, 0, 5, 2, []),
        ("min_length at cur_len = m - 1", a, 4, 0, 5, 2, []),
    ]
