"""TinyViT image encoder on the device (csrc/tinyvit.hip through gitcap.tinyvit.TinyViTEncoder) against the CPU
reference of tests/tinyvit_reference.py, and the student captioner from frames to a caption.

The bars below were fixed on the CPU before the first device run, by tools/tinyvit_tolerances.py on exactly these
inputs: the largest gap between the bf16-emulating reference with fp32 and with fp64 accumulation (what a different
summation order alone costs) and, end to end, plus the gap between the emulating and the fp32 reference; each bar is
3x the worst measured value.  Unit: per row (one pixel's channel vector / one frame's memory vector) max |d| / row RMS,
and mean |d| / mean row RMS (tinyvit_reference.row_error)."""
import pickle

import pytest
import torch

from gitcap.student_config import student_base, student_synthetic_weights, student_tiny
from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights, tinyvit_tiny
from oracle.student_oracle import StudentOracle
from tinyvit_reference import TinyViTReference, make_frames, row_error

# measured worst (max-row, mean): one stage on its own input 0.156 / 0.0040; memory end to end 0.064 / 0.0074
TOL_STAGE = (0.47, 0.0121)
TOL_E2E = (0.19, 0.022)
# token parity with the fp32 pipeline is asserted where its top-2 margin exceeds this: the encoder's bf16 rounding
# moved the student logits by <= 0.019 on the CPU, the decoder's by <= 0.10 (tests/test_student.py TOL_F32); 2x the sum
# of 3x the first and the second, rounded
NEAR_TIE_E2E = 0.3

CASES = [("tiny", (2, 2, 2), 12, 7), ("tiny", (2, 2, 1), 12, 7), ("21m", (2, 2, 2), 6, 8), ("21m", (2, 2, 1), 6, 8)]


def _cfg(name, ms):
    return tinyvit_tiny(ms) if name == "tiny" else tinyvit_config("tiny_vit_21m_224", ms)


def _encoder(cfg, w, max_frames=16):
    from gitcap.tinyvit import TinyViTEncoder
    return TinyViTEncoder(cfg, w, device="cuda:0", max_frames=max_frames)


@pytest.mark.gpu
@pytest.mark.parametrize("name,ms,n,seed", CASES)
def test_gpu_stages_and_memory_match_reference(name, ms, n, seed):
    cfg = _cfg(name, ms)
    w = tinyvit_synthetic_weights(cfg, 0)
    x = make_frames(n, cfg.img_size, seed)
    enc = _encoder(cfg, w)
    fm = [t.cpu() for t in enc(x)]
    mem = enc.memory(x.view(1, n, *x.shape[1:])).cpu()[0]
    emu = TinyViTReference(cfg, emulate_bf16=True).load_weights(w)
    f32 = TinyViTReference(cfg).load_weights(w)
    for i in range(4):
        want = emu.stage(0, emu.stem(x)) if i == 0 else emu.stage(i, fm[i - 1])
        assert fm[i].shape == want.shape
        err = row_error(fm[i], want)
        print(f"{name} {ms} stage {i}: {err}")
        assert torch.isfinite(fm[i]).all()
        assert err[0] < TOL_STAGE[0] and err[1] < TOL_STAGE[1], (i, err)
    # memory is the mean of the device's own stage-3 map, and close to the fp32 reference end to end
    assert torch.allclose(mem, fm[3].mean(dim=[2, 3]), rtol=1e-5, atol=1e-5)
    err = row_error(mem, f32.memory(x.view(1, n, *x.shape[1:]))[0])
    print(f"{name} {ms} memory vs fp32: {err}")
    assert err[0] < TOL_E2E[0] and err[1] < TOL_E2E[1], err


@pytest.mark.gpu
def test_gpu_batch_invariance_and_determinism():
    cfg = tinyvit_config("tiny_vit_21m_224")
    w = tinyvit_synthetic_weights(cfg, 1)
    enc = _encoder(cfg, w, max_frames=96)
    x = make_frames(96, cfg.img_size, 3).view(16, 6, 3, 224, 224)
    full = enc.memory(x)
    assert torch.equal(full, enc.memory(x))                                   # run to run
    for b, f in ((0, 0), (7, 3), (15, 5)):
        assert torch.equal(enc.memory(x[b:b + 1, f:f + 1]), full[b:b + 1, f:f + 1])    # alone vs inside n = 96
    fm_one = enc(x[7, 3:4])
    fm_all = enc(x.view(96, 3, 224, 224))
    for a, b in zip(fm_one, fm_all):
        assert torch.equal(a[0], b[7 * 6 + 3])


def _student_with_native(tcfg, scfg, tw, sw, **kw):
    from gitcap.student import StudentCaptioner
    weights = dict(sw)
    weights.update({"image_encoder.model." + k: v for k, v in tw.items()})
    name = "tiny_vit_21m_224.dist_in22k_ft_in1k" if tcfg.embed_dims[3] == 576 else None
    if name:
        return StudentCaptioner(name, cfg=scfg, weights=weights, image_encoder="native", device="cuda:0", **kw)
    from gitcap.tinyvit import TinyViTEncoder
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=kw.get("max_batch", 16) * scfg.mem_tokens)
    return StudentCaptioner(cfg=scfg, weights=weights, image_encoder=enc, device="cuda:0", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "21m"])
def test_gpu_student_frames_to_caption(name):
    tcfg = _cfg(name, (2, 2, 2))
    scfg = student_tiny() if name == "tiny" else student_base()
    tw, sw = tinyvit_synthetic_weights(tcfg, 0), student_synthetic_weights(scfg, 0)
    B = 2 if name == "tiny" else 1
    m = _student_with_native(tcfg, scfg, tw, sw, max_batch=4, max_text_len=25)
    x = make_frames(B * 6, tcfg.img_size, 9).view(B, 6, 3, tcfg.img_size, tcfg.img_size)
    ids = m.greedy_decode(x, max_len=25, stop="never")
    mem = m.image_encoder.memory(x)
    assert torch.equal(ids, m.greedy_decode(mem, max_len=25, stop="never").cpu())        # frames == the encoder's memory
    fm, mem2 = m.forward_image_enc(x)
    assert torch.equal(mem2, mem) and len(fm) == 4 and fm[3].shape[1] == scfg.d_model
    assert torch.equal(m.beam_search(x, max_len=8, k=2), m.beam_search(mem, max_len=8, k=2).cpu())
    assert torch.equal(m.beam_search_host(x, max_len=6, k=2), m.beam_search_host(mem, max_len=6, k=2).cpu())
    # tokens of the fp32 pipeline (reference encoder + StudentOracle), teacher-forced on the device's ids
    ref_mem = TinyViTReference(tcfg).load_weights(tw).memory(x)
    logits = StudentOracle(scfg, sw).forward_decoder(ids[:, :-1].cpu(), ref_mem)
    top2 = logits.topk(2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) > NEAR_TIE_E2E
    assert sure.float().mean().item() > 0.3
    assert torch.equal(logits.argmax(-1)[sure], ids[:, 1:].cpu()[sure])


@pytest.mark.gpu
def test_gpu_pickle_state_dict_and_errors():
    from gitcap._lib import GitcapError
    from gitcap.student import StudentCaptioner
    from gitcap.tinyvit import TinyViTEncoder
    tcfg, scfg = tinyvit_tiny(), student_tiny()
    tw, sw = tinyvit_synthetic_weights(tcfg, 2), student_synthetic_weights(scfg, 2)
    m = _student_with_native(tcfg, scfg, tw, sw, max_batch=2, max_text_len=8)
    x = make_frames(12, tcfg.img_size, 4).view(2, 6, 3, 64, 64)
    ids = m.greedy_decode(x, max_len=8, stop="never")
    m2 = pickle.loads(pickle.dumps(m))
    assert torch.equal(m2.greedy_decode(x, max_len=8, stop="never"), ids)
    sd = m.state_dict()
    assert {k for k in sd if k.startswith("image_encoder.model.")} == {"image_encoder.model." + k for k in tw}
    # a reference checkpoint with "stages.i" keys and the ignored buffers loads into the native encoder
    sd2 = {k.replace("stages_", "stages."): v for k, v in sd.items()}
    sd2["image_encoder.model.patch_embed.conv1.bn.num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=12)
    m3 = StudentCaptioner(cfg=scfg, image_encoder=enc, max_batch=2, max_text_len=8)
    m3.load_state_dict(sd2)
    assert torch.equal(m3.greedy_decode(x, max_len=8, stop="never"), ids)
    with pytest.raises(KeyError):                                               # missing encoder keys
        StudentCaptioner(cfg=scfg, image_encoder=TinyViTEncoder(tcfg, max_frames=12), max_batch=2,
                         max_text_len=8).load_state_dict({k: v for k, v in sd.items() if "stages_3" not in k})
    with pytest.raises(ValueError):                                             # wrong image size
        m.greedy_decode(torch.zeros(1, 6, 3, 32, 32), max_len=4)
    with pytest.raises(ValueError):                                             # n > max_frames
        m.image_encoder.memory(make_frames(18, 64, 1).view(3, 6, 3, 64, 64))
    with pytest.raises(ValueError, match="d_model"):                            # encoder width != d_model
        StudentCaptioner(cfg=student_base(), image_encoder=m.image_encoder)
    with pytest.raises(GitcapError):
        m.image_encoder.to("cpu")
    with pytest.raises(GitcapError):
        TinyViTEncoder(tcfg, device="cpu")
