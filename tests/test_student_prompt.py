"""Prompted decoding on the student, on the CPU: what a prompted caption IS, stated on the oracle (oracle/student_oracle.py) with the
restatements of tests/student_prompt_reference.py -- all lengths 1 is the unprompted loop, a caption's own beginning as its prompt
reproduces it, a clip does not see the other clips' lengths --, that the end-to-end cases change what the model emits, and that
the cases tell three wrong restatements from the right one."""
import numpy as np
import pytest
import torch

import student_prompt_reference as P
from gitcap.student_config import student_synthetic_weights, student_tiny
from oracle.student_oracle import StudentOracle, make_memory


@pytest.fixture(scope="module")
def oracle():
    cfg = student_tiny()
    orc = StudentOracle(cfg, student_synthetic_weights(cfg, 0))
    mem = make_memory(P.B, cfg.mem_tokens, cfg.d_model, P.MEM_SEED)
    free = orc.greedy_decode(mem, P.L, stop="never")
    return orc, cfg, mem, free


@pytest.fixture(scope="module")
def cases(oracle):
    """case -> (prompts, the greedy yardstick's (ids, forced, logits)), computed once"""
    orc, cfg, mem, free = oracle
    out = {}
    for name, prompts in P.case_prompts(free.numpy(), cfg.vocab_length, cfg.cls_token_id).items():
        out[name] = (prompts, P.greedy_yardstick(orc.forward_decoder, mem, P.L, prompts, cfg.cls_token_id))
    return out


def test_all_lengths_one_is_the_unprompted_loop(oracle):
    orc, cfg, mem, free = oracle
    none = [[cfg.cls_token_id]] * P.B
    ids, forced, _ = P.greedy_yardstick(orc.forward_decoder, mem, P.L, none, cfg.cls_token_id)
    assert np.array_equal(ids, free.numpy()) and not forced.any()
    best = P.beam_yardstick(orc.forward_decoder, mem, P.L, P.K, none, cfg.cls_token_id)
    assert np.array_equal(best, orc.beam_search(mem, P.L, P.K).numpy())


@pytest.mark.parametrize("j", [2, 5, P.L])
def test_a_captions_own_beginning_reproduces_it(oracle, j):
    orc, cfg, mem, free = oracle
    prompts = [free[b, :j].tolist() for b in range(P.B)]
    ids, forced, _ = P.greedy_yardstick(orc.forward_decoder, mem, P.L, prompts, cfg.cls_token_id)
    assert np.array_equal(ids, free.numpy())
    assert forced[:, :j - 1].all() and not forced[:, j - 1:].any()


def test_the_cases_change_what_the_model_emits(oracle, cases):
    """A row with a prompt must hold, behind it, at least one token that differs from the free caption: a case that changes nothing
    proves nothing.  A row of CLS alone has no prompt and its caption is the free one (rows do not see each other)."""
    orc, cfg, mem, free = oracle
    for name, (prompts, (ids, forced, _)) in cases.items():
        for b, row in enumerate(prompts):
            n = len(row)
            assert ids[b, :n].tolist() == row, (name, b)
            assert forced[b].tolist() == [t + 1 < n for t in range(P.L)]
            if n == 1:
                assert np.array_equal(ids[b], free[b].numpy()), (name, b)
                continue
            assert all(ids[b, j] != free[b, j] or ids[b, j] == P.PAD for j in range(1, n)), (name, b)     # the prompt is not the free caption
            assert (ids[b, n:] != free[b, n:].numpy()).any(), (name, b, ids[b], free[b])
    assert P.PAD in cases["ragged"][0][2][1:]


def test_a_clip_does_not_depend_on_the_other_clips_lengths(oracle, cases):
    orc, cfg, mem, free = oracle
    prompts, (ids, _, _) = cases["ragged"]
    for b in range(P.B):
        one, _, _ = P.greedy_yardstick(orc.forward_decoder, mem[b:b + 1], P.L, prompts[b:b + 1], cfg.cls_token_id)
        assert np.array_equal(one[0], ids[b]), b
    best = P.beam_yardstick(orc.forward_decoder, mem, P.L, P.K, prompts, cfg.cls_token_id)
    for b in range(P.B):
        one = P.beam_yardstick(orc.forward_decoder, mem[b:b + 1], P.L, P.K, prompts[b:b + 1], cfg.cls_token_id)
        assert np.array_equal(one[0], best[b]), b
        assert best[b, :len(prompts[b])].tolist() == prompts[b]
    assert not np.array_equal(best, orc.beam_search(mem, P.L, P.K).numpy())


def test_a_prompted_beam_equals_the_reference_loop_started_from_the_prefix(oracle, cases):
    """The reference's loop (model.py:189-318) over one clip whose target starts as the prompt, against the lockstep yardstick."""
    orc, cfg, mem, free = oracle
    prompts, _ = cases["ragged"]
    best = P.beam_yardstick(orc.forward_decoder, mem, P.L, P.K, prompts, cfg.cls_token_id)
    k = P.K
    for b in range(P.B):
        m1 = mem[b:b + 1]
        tgt = torch.tensor([prompts[b]], dtype=torch.long)
        scores, top = torch.log_softmax(orc.forward_decoder(tgt, m1)[:, -1], -1).topk(k, -1)
        seqs = torch.cat([tgt.unsqueeze(1).expand(-1, k, -1), top.unsqueeze(-1)], -1)
        for _ in range(tgt.shape[1] + 1, P.L):
            lp = torch.log_softmax(orc.forward_decoder(seqs[0], m1.expand(k, -1, -1))[:, -1], -1)
            ts, ti = lp.topk(k, -1)
            cand = (scores[0][:, None] + ts).reshape(1, k * k)
            sel = cand.sort(dim=1, descending=True).indices[:, :k]
            seqs = torch.cat([seqs[:, (sel // k)[0]], ti.reshape(1, k * k).gather(1, sel).unsqueeze(-1)], -1)
            scores = cand.gather(1, sel)
        assert seqs[0, scores.argmax(-1)[0]].tolist() == best[b].tolist(), b


# ---- the cases tell wrong restatements from the right one ---------------------------------------------------------------------------------

def test_an_off_by_one_position_is_caught(oracle, cases):
    orc, cfg, mem, free = oracle
    for name, (prompts, (ids, _, _)) in cases.items():
        bad, _, _ = P.greedy_yardstick(orc.forward_decoder, mem, P.L, prompts, cfg.cls_token_id, wrong="pos")
        assert not np.array_equal(bad, ids), name


def test_unclamped_lengths_are_caught():
    prm, lens, max_len, cls = P.stage_inputs()
    ids0 = np.full((5, 12), -3, dtype=np.int64)
    good, _ = P.stage(prm, lens, 5, 1, max_len, cls, ids0)
    bad, _ = P.stage(prm, lens, 5, 1, max_len, cls, ids0, wrong="noclamp")
    assert not (good == 7777).any() and (bad == 7777).any()            # the column behind max_len
    assert good[0].tolist() == [cls] * 12 and good[3].tolist() == [cls] * 12
    assert good[1].tolist() == [cls] + prm[1, 1:4].tolist() + [cls] * 8
    assert good[2].tolist() == [cls] + prm[2, 1:11].tolist() + [cls] and good[4].tolist() == [cls] + prm[4, 1:11].tolist() + [cls]


def test_a_forced_step_that_permutes_is_caught():
    d = P.beam_step_inputs()
    args = (d["cand_scores"], d["cand_idx"], d["ids_cur"], np.full_like(d["ids_cur"], -3), np.arange(6, dtype=np.float32),
            np.full(6, -3, dtype=np.int32), d["B"], d["k"], d["V"], d["t"])
    pr = (d["prompt_ids"], d["lengths"], d["prompt_max_len"])
    good, bad = P.beam_step(*args, prompt=pr), P.beam_step(*args, prompt=pr, wrong="permute")
    assert good[2][:3].tolist() == [0, 1, 2] and bad[2][:3].tolist() == [2, 0, 2]
    assert not np.array_equal(good[0], bad[0])
    assert good[1][:3].tolist() == [0.0, 1.0, 2.0]                      # a forced clip's scores stay
    plain = P.beam_step(*args)
    assert np.array_equal(good[0][3:], plain[0][3:]) and np.array_equal(good[1][3:], plain[1][3:])      # the free clip is the plain step
