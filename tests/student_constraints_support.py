"""What the student's constrained-decoding tests share (tests/test_student_constraints.py on the CPU, the two *_gpu.py files on the
device): the numpy packer of the rule record gitcap_dbg_ban_mask_rec reads, the cases, and the yardsticks -- a greedy loop and the
reference-shaped beam loop over any ``forward_decoder(ids, memory) -> logits`` with constraints_reference.mask_logits in front of
the arg-max / the log-softmax.  The student's loops keep decoding behind a row's SEP and so do the yardsticks: the rules keep
applying there."""
import numpy as np
import torch

import constraints_reference as C

REC_HEADER, REC_MAX, REC_WORDS = 4, 256, 4 + 256
B, L, K = 3, 10, 3                  # clips, greedy steps, beams of the end-to-end cases
MEM_SEED = 31


def pack_record(n, min_length, suppress, fill=0, n_suppress=None):
    """-> int32 [4 + 256]: n, min_length, n_suppress, 0, the ids; the words behind the list hold `fill` (a reader that trusts a
    wrong count sees them).  n_suppress: the count word, when it is to differ from len(suppress)."""
    assert len(suppress) <= REC_MAX
    rec = np.full(REC_WORDS, fill, dtype=np.int32)
    rec[0], rec[1], rec[2], rec[3] = n, min_length, len(suppress) if n_suppress is None else n_suppress, 0
    rec[REC_HEADER:REC_HEADER + len(suppress)] = np.asarray(suppress, dtype=np.int32)
    return rec


def unpack_record(rec):
    """What the kernel reads of a record -> (n, min_length, the suppress list): the count clamped to 0..256."""
    rec = np.asarray(rec, dtype=np.int32)
    assert rec.shape == (REC_WORDS,)
    ns = min(max(int(rec[2]), 0), REC_MAX)
    return int(rec[0]), int(rec[1]), [int(v) for v in rec[REC_HEADER:REC_HEADER + ns]]


def ban_mask_of_record(prefixes, cur_len, rec, sep_id, V, ld_mask=None):
    n, m, sup = unpack_record(rec)
    return C.ban_mask(prefixes, cur_len, n, m, sep_id, sup, V, ld_mask)


# the teacher's four cases (tests/test_constraints_e2e_gpu.py); "own": tokens of the free captions
CASES = [dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2, min_length=6), dict(min_length=L + 1),
         dict(no_repeat_ngram_size=3, min_length=4, suppress_tokens="own")]


def case_kw(case, free):
    kw = dict(case)
    if kw.get("suppress_tokens") == "own":
        kw["suppress_tokens"] = sorted({int(free[0, 1]), int(free[1, 3]), int(free[2, 2])})
    return kw


def rules(kw):
    return kw.get("no_repeat_ngram_size", 0), kw.get("min_length", 0), list(kw.get("suppress_tokens", []))


def masked_last_logits(forward, ids, memory, kw, sep_id, V):
    """The logits of the last position of ids [rows][T] (a tensor) with -inf at the columns the rules ban -> numpy [rows][V]"""
    n, m, sup = rules(kw)
    lg = forward(ids, memory)[:, -1].float().cpu().numpy()
    return C.mask_logits(lg, C.ban_mask(ids.cpu().numpy(), ids.shape[1], n, m, sep_id, sup, V))


def greedy_yardstick(forward, memory, max_len, kw, cls_id, sep_id, V):
    """-> (ids int64 [B][1 + max_len], the masked rows of every step [max_len][B][V]); first arg-max, no stop"""
    ids = torch.full((memory.shape[0], 1), cls_id, dtype=torch.long)
    rows = []
    for _ in range(max_len):
        masked = masked_last_logits(forward, ids, memory, kw, sep_id, V)
        rows.append(masked)
        ids = torch.cat([ids, torch.as_tensor(masked.argmax(-1))[:, None]], dim=1)
    return ids, np.stack(rows, 0)


def beam_yardstick(forward, memory, max_len, k, kw, cls_id, sep_id, V):
    """oracle/student_oracle.py: beam_search (model.py:189-318), every row's banned logits -inf ahead of its log_softmax"""
    Bn = memory.shape[0]
    tgt = torch.full((Bn, 1), cls_id, dtype=torch.long)

    def logp(ids):
        return torch.log_softmax(torch.as_tensor(masked_last_logits(forward, ids, memory, kw, sep_id, V)), dim=-1)
    scores, top = logp(tgt).topk(k, dim=-1)
    seqs = torch.cat([tgt.unsqueeze(1).expand(-1, k, -1), top.unsqueeze(-1)], dim=-1)
    for _ in range(2, max_len):
        cand, toks = [], []
        for i in range(k):
            ts, ti = logp(seqs[:, i]).topk(k, dim=-1)
            cand.append(scores[:, i:i + 1] + ts)
            toks.append(ti)
        cand, toks = torch.cat(cand, dim=1), torch.cat(toks, dim=1)
        sel = cand.sort(dim=1, descending=True).indices[:, :k]
        seqs = torch.cat([seqs.gather(1, (sel // k).unsqueeze(-1).expand(-1, -1, seqs.shape[-1])), toks.gather(1, sel).unsqueeze(-1)], dim=-1)
        scores = cand.gather(1, sel)
    return seqs[torch.arange(Bn), scores.argmax(dim=-1)]


def obeys(seq, kw, sep_id):
    """One generated sequence (CLS first) against the rules themselves."""
    n, m, sup = rules(kw)
    seq = [int(v) for v in seq]
    return not (n and C.repeats_ngram(seq, n)) and not set(seq[1:]) & set(sup) and sep_id not in seq[1:m]
