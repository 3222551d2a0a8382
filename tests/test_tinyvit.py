"""TinyViT image encoder of the student captioner, host side (no GPU): configs, checkpoint keys, BatchNorm folding,
the attention-bias table, the test reference's attention, and the C ABI's refusal of bad configs."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gitcap import _lib
from gitcap.tinyvit_config import (CTinyViTConfig, canonical_key, fold_convnorm, folded_tensors,
                                   normalise_keys, tinyvit_config, tinyvit_shapes, tinyvit_synthetic_weights, tinyvit_tiny)
from tinyvit_reference import Attention, TinyViTReference, attention_bias_idxs


@pytest.mark.parametrize("name", ["tiny_vit_5m_224", "tiny_vit_11m_224", "tiny_vit_21m_224"])
def test_reference_state_dict_matches_shapes(name):
    cfg = tinyvit_config(name)
    ref = TinyViTReference(cfg)
    sd = {k: tuple(v.shape) for k, v in ref.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert sd == dict(tinyvit_shapes(cfg))
    assert not any("attention_bias_idxs" in k for k in ref.state_dict())           # non-persistent buffer


def test_config_names():
    assert tinyvit_config("tiny_vit_21m_224.dist_in22k_ft_in1k").embed_dims == (96, 192, 384, 576)
    assert tinyvit_config("tiny_vit_11m_224").num_heads == (2, 4, 8, 14)
    c5 = tinyvit_config("tiny_vit_5m_224")
    assert c5.embed_dims == (64, 128, 160, 320) and c5.num_heads == (2, 4, 5, 10)
    for c in (c5, tinyvit_config("tiny_vit_21m_224")):
        assert c.depths == (2, 2, 6, 2) and c.window_sizes == (7, 7, 14, 7) and c.merge_strides == (2, 2, 2)
        assert c.stage_maps() == (56, 28, 14, 7)
        c.validate()
    assert tinyvit_config("tiny_vit_21m_224", (2, 2, 1)).stage_maps() == (56, 28, 14, 14)
    for bad in ("tiny_vit_21m_384", "tiny_vit_21m", "vit_base", "tiny_vit_21m_224x"):
        with pytest.raises(ValueError):
            tinyvit_config(bad)
    tiny = tinyvit_tiny()
    assert tiny.embed_dims[3] == 64
    maps = tiny.stage_maps()
    assert any(maps[i] // tiny.window_sizes[i] > 1 for i in (1, 2, 3))            # a stage with several windows
    tinyvit_tiny((2, 2, 1)).validate()


def test_bias_index_table_hand_worked():
    # window 2: points (0,0) (0,1) (1,0) (1,1); offsets in order of first appearance: (0,0)=0 (0,1)=1 (1,0)=2 (1,1)=3
    assert attention_bias_idxs(2).tolist() == [[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]]
    t3 = attention_bias_idxs(3)
    # row 0 = point (0,0) against all points: offsets (0,0) (0,1) (0,2) (1,0) (1,1) (1,2) (2,0) (2,1) (2,2) -> 0..8
    assert t3[0].tolist() == list(range(9))
    # point (1,1) (index 4) against all: (1,1) (1,0) (1,1) (0,1) (0,0) (0,1) (1,1) (1,0) (1,1)
    assert t3[4].tolist() == [4, 3, 4, 1, 0, 1, 4, 3, 4]
    assert int(t3.max()) == 8 and torch.equal(t3, t3.t())


def test_reference_attention_equals_sdpa_with_bias():
    torch.manual_seed(0)
    C, heads, ws = 64, 2, 3
    att = Attention(C, heads, ws)
    with torch.no_grad():
        att.attention_biases.normal_()
    x = torch.randn(5, ws * ws, C)
    from tinyvit_reference import _Ctx
    got = att.run(x, _Ctx())
    xn = att.norm(x)
    q, k, v = att.qkv(xn).view(5, ws * ws, heads, 96).split([32, 32, 32], dim=3)
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=att.bias()[None])
    want = att.proj(o.transpose(1, 2).reshape(5, ws * ws, C))
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5)


def test_folded_convnorm_equals_conv_then_eval_bn():
    rng = np.random.default_rng(3)
    for groups, cin, cout, k in ((1, 8, 16, 3), (16, 16, 16, 3), (1, 32, 64, 1)):
        w = rng.standard_normal((cout, cin // groups, k, k)).astype(np.float32)
        g, b = rng.uniform(0.5, 2, cout).astype(np.float32), rng.normal(0, 0.5, cout).astype(np.float32)
        mu, var = rng.normal(0, 0.5, cout).astype(np.float32), rng.uniform(0.1, 2, cout).astype(np.float32)
        conv = torch.nn.Conv2d(cin, cout, k, 1, k // 2, groups=groups, bias=False)
        bn = torch.nn.BatchNorm2d(cout, eps=1e-5).eval()
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(w))
            bn.weight.copy_(torch.from_numpy(g)); bn.bias.copy_(torch.from_numpy(b))
            bn.running_mean.copy_(torch.from_numpy(mu)); bn.running_var.copy_(torch.from_numpy(var))
            x = torch.randn(2, cin, 7, 7, dtype=torch.float64)
            want = bn.double()(conv.double()(x))
            wf, bf = fold_convnorm(w, g, b, mu, var, 1e-5)
            got = F.conv2d(x, torch.from_numpy(wf).double(), torch.from_numpy(bf).double(), 1, k // 2, groups=groups)
        assert float((got - want).abs().max() / want.abs().max()) < 1e-5


def test_key_forms_are_normalised():
    assert canonical_key("image_encoder.model.stages_1.blocks.0.attn.qkv.weight") == "stages_1.blocks.0.attn.qkv.weight"
    assert canonical_key("model.stages.2.downsample.conv1.conv.weight") == "stages_2.downsample.conv1.conv.weight"
    assert canonical_key("patch_embed.conv1.bn.running_var") == "patch_embed.conv1.bn.running_var"
    assert canonical_key("stages.0.blocks.1.conv2.bn.num_batches_tracked") is None
    assert canonical_key("image_encoder.model.stages_1.blocks.0.attn.attention_bias_idxs") is None
    cfg = tinyvit_tiny()
    w = tinyvit_synthetic_weights(cfg, 0)
    dotted = {"image_encoder.model." + k.replace("stages_", "stages."): v for k, v in w.items()}
    dotted["image_encoder.model.stages.1.blocks.0.attn.attention_bias_idxs"] = np.zeros((16, 16))
    dotted["image_encoder.model.patch_embed.conv1.bn.num_batches_tracked"] = np.zeros(())
    out = normalise_keys(dotted)
    assert set(out) == set(tinyvit_shapes(cfg))


def test_synthetic_weights_and_folded_names():
    cfg = tinyvit_tiny()
    w = tinyvit_synthetic_weights(cfg, 0)
    assert all(np.abs(w[k]).min() > 0 for k in w if k.endswith("conv3.bn.weight"))     # the MBConv branch is live
    assert all(np.abs(w[k]).max() > 0 for k in w if k.endswith("attention_biases"))
    assert all(not np.allclose(w[k], 0) for k in w if k.endswith("running_mean"))
    fw = folded_tensors(cfg, w)
    assert "patch_embed.conv1.weight" in fw and "patch_embed.conv1.bias" in fw
    assert not any(".bn." in k or ".conv.weight" in k for k in fw)
    assert fw["stages_1.blocks.0.local_conv.weight"].shape == (32, 1, 3, 3)


def _create(cc):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.gitcap_tinyvit_create(ctypes.byref(cc), 0, ctypes.byref(h))
    return rc, lib.gitcap_tinyvit_last_error(None).decode(), h


@pytest.mark.parametrize("field,value,msg", [
    ("num_heads", (3, 6, 12, 16), "head_dim"),
    ("embed_dims", (96, 192, 384, 560), "multiples of 32"),
    ("window_sizes", (7, 7, 14, 6), "window"),
    ("merge_strides", (2, 2, 3), "merge_strides"),
    ("img_size", 226, "img_size"),
])
def test_bad_config_is_rejected_before_touching_the_device(field, value, msg):
    from dataclasses import replace
    cfg = replace(tinyvit_config("tiny_vit_21m_224"), **{field: value})
    with pytest.raises(ValueError):
        cfg.validate()
    rc, err, h = _create(CTinyViTConfig.from_config(cfg, 6))
    assert rc == -1 and not h.value and msg in err, (rc, err)
    lib = _lib.load()
    assert lib.gitcap_tinyvit_create(None, 0, ctypes.byref(h)) == -1


def test_good_config_gets_past_the_checks():
    """A valid config passes the checks: it is created on a GPU, and without one fails only at the device lookup."""
    rc, err, h = _create(CTinyViTConfig.from_config(tinyvit_config("tiny_vit_21m_224", (2, 2, 1)), 6))
    if rc == 0:
        _lib.load().gitcap_tinyvit_destroy(h)
    else:
        assert "no such HIP device" in err


def test_ctypes_struct_mirrors_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "gitcap.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"struct\s+gitcap_tinyvit_config\s*\{(.*?)\}\s*;", txt, flags=re.S).group(1), flags=re.S)
    names = [re.sub(r"\[.*\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert [f for f, _ in CTinyViTConfig._fields_] == names

