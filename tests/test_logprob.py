"""The fp64 restatement of the token log-probability (tests/logprob_reference.py: tile partials + merge) against
torch.log_softmax gathered at the arg-max, and gitcap.caption_confidence on hand-made cases.  No GPU."""
import math

import numpy as np
import torch

import logprob_reference as L

NINF = float("-inf")


def _check(logits):
    """tokens == the first arg-max; lp == log_softmax(fp64)[token] (rows with nothing above -inf: token 0, lp -inf)."""
    x = torch.as_tensor(np.asarray(logits, dtype=np.float64))
    tok, lp = L.token_logprobs(x.numpy())
    for m in range(x.shape[0]):
        row = x[m]
        if bool((row == NINF).all()):
            assert tok[m] == 0 and lp[m] == NINF
            continue
        want_tok = int(np.argmax(row.numpy()))                          # np.argmax: first occurrence
        want = float(torch.log_softmax(row, 0)[want_tok])
        assert tok[m] == want_tok
        assert abs(lp[m] - want) <= 1e-12 * max(1.0, abs(want)), (m, lp[m], want)


def test_random_rows_and_ragged_last_tile():
    rng = np.random.default_rng(0)
    for N in (1, 10, 16, 17, 48, 65, 997, 4122):
        _check(rng.standard_normal((5, N)) * 3.0)


def test_exact_ties_for_the_maximum():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 200))
    x[0, [3, 7]] = 9.0              # inside one tile
    x[1, [5, 150]] = 9.0            # across tiles
    x[2, [199, 0]] = 9.0            # both ends
    x[3, :] = 1.25                  # all equal: token 0, lp = -log N
    _check(x)
    tok, lp = L.token_logprobs(x)
    assert tok.tolist() == [3, 5, 0, 0] and abs(lp[3] + math.log(200)) < 1e-12


def test_masked_columns_empty_tiles_and_the_empty_row():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((4, 100))
    x[0, 32:48] = NINF              # a whole tile
    x[0, [1, 50, 99]] = NINF        # scattered
    x[1, :96] = NINF                # only the ragged last tile is alive
    x[2, :] = NINF                  # nothing above -inf
    x[3, 1:] = NINF                 # one live logit: p = 1
    _check(x)
    val, idx, ssum = L.tile_partials(x)
    assert val[0, 2] == NINF and idx[0, 2] == L.SENTINEL and ssum[0, 2] == 0.0
    assert L.merge(val[2], idx[2], ssum[2]) == (0, NINF)
    assert L.merge(val[3], idx[3], ssum[3]) == (0, 0.0)


def test_peaked_row():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 4122))
    x[0, 1234] += 50.0
    x[1, 4121] += 50.0              # in the ragged last tile
    _check(x)
    tok, lp = L.token_logprobs(x)
    assert tok.tolist() == [1234, 4121] and (lp > -1e-15).all() and (lp <= 0).all()


def test_caption_confidence_hand_made():
    from gitcap import caption_confidence
    SEP = 102
    ids = torch.tensor([[101, 5, 6, SEP, 0, 0],         # first SEP at step 2: three tokens count
                        [101, 5, 6, 7, 8, 9],           # no SEP: all five
                        [101, SEP, SEP, 5, 6, 7],       # SEP at once: one token
                        [101, 5, 6, 7, 8, SEP]])        # SEP last
    p = torch.tensor([[0.5, 0.25, 0.125, 1e-9, 1e-9],
                      [0.5, 0.5, 0.5, 0.5, 0.5],
                      [0.9, 1e-9, 1e-9, 1e-9, 1e-9],
                      [1.0, 1.0, 1.0, 1.0, 1.0]])
    c = caption_confidence(ids, torch.log(p), SEP)
    want = torch.tensor([(0.5 * 0.25 * 0.125) ** (1 / 3), 0.5, 0.9, 1.0])
    assert c.dtype == torch.float32 and c.shape == (4,)
    assert torch.allclose(c, want, rtol=1e-6, atol=0)
    # a -inf token (the empty row) gives confidence 0; behind the first SEP it does not count
    lp = torch.log(p)
    lp[1, 2] = NINF
    lp[0, 4] = NINF
    c = caption_confidence(ids, lp, SEP)
    assert float(c[1]) == 0.0 and torch.allclose(c[0], want[0], rtol=1e-6, atol=0)
    # no steps: nothing to doubt
    assert caption_confidence(ids[:, :1], lp[:, :0], SEP).tolist() == [1.0] * 4
    try:
        caption_confidence(ids, lp[:, :3], SEP)
        assert False
    except ValueError:
        pass
