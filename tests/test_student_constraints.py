"""Constrained decoding on the student without a GPU: (a) the header, the binding table, the library's exports and the Python entry
points carry the new surface; (b) what a constrained student caption IS, stated on the oracle (oracle/student_oracle.py) with the
restatement of tests/constraints_reference.py, and that the cases the GPU tests use bite on the tiny config; (c) the numpy packer
of the rule record against the restatement, on the inputs the GPU test uploads."""
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import constraints_reference as C
import student_constraints_support as S
from gitcap import _lib
from gitcap.student_config import student_synthetic_weights, student_tiny
from oracle.student_oracle import StudentOracle, make_memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYWORDS = ("no_repeat_ngram_size", "min_length", "suppress_tokens")


# ---- a. the surface ---------------------------------------------------------------------------------------------------------------

def test_header_bindings_and_exports_hold_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "gitcap.h")).read()
    for name in ("gitcap_student_attach_constraints", "gitcap_dbg_ban_mask_rec"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"int\s+gitcap_student_attach_constraints\s*\(\s*gitcap_student_t\s*\*\s*h\s*,\s*const\s+gitcap_constraints\s*\*\s*c\s*\)", text)
    assert len(_lib.SYMBOLS["gitcap_dbg_ban_mask_rec"][1]) == 10 and len(_lib.SYMBOLS["gitcap_student_attach_constraints"][1]) == 2
    assert "student model are not constrained" not in text
    so = os.path.join(ROOT, "real-time-video-captioning_amd", "gitcap", "libgitcap.so")
    if os.path.exists(so):                                  # once built: the exports
        names = open(so, "rb").read()
        for name in (b"gitcap_student_attach_constraints", b"gitcap_dbg_ban_mask_rec"):
            assert name + b"\0" in names, name


def test_python_entry_points_accept_the_keywords():
    from gitcap.student import StudentCaptioner
    for fn in ("greedy_decode", "beam_search", "beam_search_host", "caption_stream", "stream_pool"):
        sig = inspect.signature(getattr(StudentCaptioner, fn))
        for kw in KEYWORDS:
            assert kw in sig.parameters, (fn, kw)
        assert sig.parameters["no_repeat_ngram_size"].default == 0 and sig.parameters["min_length"].default == 0
        assert sig.parameters["suppress_tokens"].default is None


# ---- b. the yardstick on the oracle -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle():
    cfg = student_tiny()
    w = student_synthetic_weights(cfg, 0)
    mem = make_memory(S.B, cfg.mem_tokens, cfg.d_model, S.MEM_SEED)
    free = StudentOracle(cfg, w).greedy_decode(mem, S.L, stop="never")
    # SEP = a token the free caption emits early, so that min_length changes the caption
    cfg = dataclasses.replace(cfg, sep_token_id=int(free[0, 2]))
    orc = StudentOracle(cfg, w)
    free = orc.greedy_decode(mem, S.L, stop="never")
    return orc, cfg, mem, free


def test_free_yardsticks_are_the_oracles_own_loops(oracle):
    orc, cfg, mem, free = oracle
    ids, _ = S.greedy_yardstick(orc.forward_decoder, mem, S.L, {}, cfg.cls_token_id, cfg.sep_token_id, cfg.vocab_length)
    assert torch.equal(ids, free)
    beam = S.beam_yardstick(orc.forward_decoder, mem, S.L, S.K, {}, cfg.cls_token_id, cfg.sep_token_id, cfg.vocab_length)
    assert torch.equal(beam, orc.beam_search(mem, S.L, S.K))


@pytest.mark.parametrize("case", S.CASES)
def test_cases_bite_and_obey_the_rules_on_the_tiny_config(oracle, case):
    orc, cfg, mem, free = oracle
    V, sep = cfg.vocab_length, cfg.sep_token_id
    assert V == 97 and sep in free[0, 1:4].tolist()
    kw = S.case_kw(case, free)
    ids, rows = S.greedy_yardstick(orc.forward_decoder, mem, S.L, kw, cfg.cls_token_id, sep, V)
    assert not torch.equal(ids, free)
    assert rows.shape == (S.L, S.B, V) and np.isinf(rows).any()
    for b in range(S.B):
        assert S.obeys(ids[b], kw, sep), (kw, ids[b])
    assert not all(S.obeys(free[b], kw, sep) for b in range(S.B))       # the free captions break the rules: that is why the case bites
    beam = S.beam_yardstick(orc.forward_decoder, mem, S.L, S.K, kw, cfg.cls_token_id, sep, V)
    assert not torch.equal(beam, orc.beam_search(mem, S.L, S.K))
    for b in range(S.B):
        assert S.obeys(beam[b], kw, sep), (kw, beam[b])


# ---- c. the record ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [97, 30522, 131072])
def test_record_packer_agrees_with_the_restatement(V):
    for name, p, cur_len, n, m, sep, sup in C.builder_cases(V):
        rec = S.pack_record(n, m, sup, fill=5)              # (column 5 behind the list: read only by a wrong count)
        assert rec.dtype == np.int32 and rec.shape == (260,) and rec[3] == 0
        assert rec[:3].tolist() == [n, m, len(sup)] and rec[4:4 + len(sup)].tolist() == list(sup)
        assert S.unpack_record(rec) == (n, m, list(sup)), name
        assert np.array_equal(S.ban_mask_of_record(p, cur_len, rec, sep, V), C.ban_mask(p, cur_len, n, m, sep, sup, V)), name
    # the count word is clamped to the record
    ids = [V - 1 - (i % 7) for i in range(256)]
    for count, want in ((300, 256), (-4, 0), (1 << 30, 256)):
        n, m, sup = S.unpack_record(S.pack_record(0, 0, ids, n_suppress=count))
        assert len(sup) == want and sup == ids[:want]
