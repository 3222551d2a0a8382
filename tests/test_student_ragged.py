"""What "clips of different length" means for the student, on the CPU oracle: row b of a ragged batch is the decoder on its own F_b
memory tokens -- equivalently, on the padded memory with a -inf additive mask over the padding (the decoder has no positional or
temporal term on its memory) -- and the memories the GPU tests decode (tests/test_student_ragged_e2e_gpu.py: ragged_case) tell the
wrong kernels apart: each misreading of the two key tables moves the logits by more than the bound the e2e test grants the device."""
import pytest
import torch

from gitcap import ragged
from gitcap.student_config import student_synthetic_weights, student_tiny
from oracle.student_oracle import StudentOracle

LENS = [1, 4, 6]
TOL_EMU = 0.03          # tests/test_student.py: max |logit| error against the bf16-emulating oracle (logit std ~1)


def ragged_case(seed=5, T=6, scale=3.0):
    """-> cfg, weights, y int64 [3, T] (CLS first, no PAD), memory fp32 [3, 6, D]: clip b's tokens are memory[b, :LENS[b]]; what lies
    behind them is other finite data, as large."""
    cfg = student_tiny()
    g = torch.Generator().manual_seed(seed)
    mem = scale * torch.randn(len(LENS), cfg.mem_tokens, cfg.d_model, generator=g)
    y = torch.randint(cfg.pad_token_id + 1, cfg.vocab_length, (len(LENS), T), generator=g)
    y[:, 0] = cfg.cls_token_id
    return cfg, student_synthetic_weights(cfg, 0), y, mem


def e2e_bound(cfg, w, y, mem):
    """The bound rule of tests/test_student.py for device logits against the bf16-emulating oracle, restated: max(TOL_EMU *
    max(1, std), 1.5 * d), d = the distance of the emulated logits from the fp32 ones.  -> (emulated logits, bound)"""
    emu = StudentOracle(cfg, w, emulate_bf16=True).forward_decoder(y, mem)
    f32 = StudentOracle(cfg, w).forward_decoder(y, mem)
    d = (emu - f32).abs().max().item()
    return emu, max(TOL_EMU * max(1.0, emu.std().item()), 1.5 * d)


class MaskedOracle(StudentOracle):
    """The oracle with an additive mask [B, 1, 1, F] on the cross-attention scores (its own _attend is called with None there)."""
    mem_mask = None

    def _attend(self, q, k, v, mask):
        return super()._attend(q, k, v, self.mem_mask if mask is None else mask)


def test_ragged_is_the_padded_memory_under_a_minus_inf_mask():
    cfg, w, y, mem = ragged_case()
    alone = [StudentOracle(cfg, w).forward_decoder(y[b:b + 1], mem[b:b + 1, :n]) for b, n in enumerate(LENS)]
    orc = MaskedOracle(cfg, w)
    orc.mem_mask = torch.zeros(len(LENS), 1, 1, cfg.mem_tokens)
    for b, n in enumerate(LENS):
        orc.mem_mask[b, :, :, n:] = float("-inf")
    masked = orc.forward_decoder(y, mem)
    for b in range(len(LENS)):
        assert (masked[b] - alone[b][0]).abs().max().item() < 1e-4          # fp32: the order of the sums only
    # and the mask matters: without it the short clips read their padding
    plain = StudentOracle(cfg, w).forward_decoder(y, mem)
    assert (plain[0] - alone[0][0]).abs().max().item() > 0.1 and (plain[1] - alone[1][0]).abs().max().item() > 0.1
    assert (plain[2] - alone[2][0]).abs().max().item() < 1e-4


def test_the_memories_tell_wrong_kernels_apart():
    cfg, w, y, mem = ragged_case()
    F, k = cfg.mem_tokens, 2
    off = ragged.offsets(LENS)
    g = torch.Generator().manual_seed(99)
    packed = torch.cat([mem[b, :n] for b, n in enumerate(LENS)] + [3.0 * torch.randn(F + 1, cfg.d_model, generator=g)], 0)    # + what lies behind
    orc = StudentOracle(cfg, w)
    run = lambda b, o, n: orc.forward_decoder(y[b:b + 1], packed[None, o:o + n])[0]
    seen = set()
    for b, n in enumerate(LENS):
        right = run(b, off[b], n)
        _, bound = e2e_bound(cfg, w, y[b:b + 1], mem[b:b + 1, :n])
        wrong = {"key_len + 1": (off[b], n + 1), "the batch maximum": (off[b], max(LENS)), "clip b + 1's offset": (off[b] + n, n)}
        if n > 1:
            wrong["key_len - 1"] = (off[b], n - 1)
        for i in range(k):                              # beam row r = b * k + i reading clip r's entry instead of clip r // k's
            r = b * k + i
            if r != b and r < len(LENS):
                wrong[f"beam row {r} by r"] = (off[r], LENS[r])
        for what, (o, m) in wrong.items():
            if (o, m) == (off[b], n):
                continue                                # (the longest clip IS the batch maximum)
            moved = (run(b, o, m) - right).abs().max().item()
            print(f"clip {b} ({n} frames), {what}: logits move by {moved:.3f}, bound {bound:.3f}")
            assert moved > bound, (b, what)
            seen.add(what.split(" by ")[-1] if what.startswith("beam") else what)
    assert seen >= {"key_len + 1", "key_len - 1", "the batch maximum", "clip b + 1's offset", "r"}


def test_student_input_forms_and_refusals_need_no_device():
    """The host side of the ragged forms: counts are checked before anything touches the library."""
    with pytest.raises(ValueError, match="outside"):
        ragged.check_counts([1, 0, 6], 3, 6)
    with pytest.raises(ValueError, match="outside"):
        ragged.check_counts([7], 1, 6)
    from gitcap.window import WindowSchedule
    s = WindowSchedule(1, 6, hop=2, partial=True)
    assert [s.push(1, 1) for _ in range(7)] == [False, True, False, True, False, True, False]
    s = WindowSchedule(1, 6, hop=1)
    assert [s.push(1, 1) for _ in range(7)] == [False] * 5 + [True, True]
