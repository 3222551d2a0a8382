"""Scene-change gate on the device: gitcap_frame_change against the numpy restatement (tests/frame_gate_reference.py), and the
gated caption streams of StudentCaptioner and GitCaptioner against ungated streams fed the frames the restatement admits.

ssd and the histograms are integers: exact equality.  mse and chisq: relative 1e-12 -- a bound, not a fit: at most 256 fp64
additions and one division per term, a few hundred units of 2^-53 ~ 1e-16, with two orders of room; and 0 must be exactly 0.
Captions are compared with torch.equal."""
import numpy as np
import pytest
import torch

import frame_gate_reference as R
from gitcap.config import git_tiny
from gitcap.student_config import student_base, student_synthetic_weights, student_tiny
from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights, tinyvit_tiny
from gitcap.weights import synthetic_weights
from gpu_support import ptr, stream

pytestmark = pytest.mark.gpu

ERR_ARG = -1
REL = 1e-12


def _near(got, want):
    return abs(got - want) <= REL * abs(want)          # want == 0: got must be exactly 0


def _check(frames, ref, channel, what):
    """frames, ref: uint8 numpy [B,H,W,3] -> runs the device call and holds all five outputs to the restatement."""
    from gitcap.framegate import frame_change
    want = R.frame_change(frames, ref, channel)
    got = frame_change(torch.from_numpy(frames).cuda(), torch.from_numpy(ref).cuda(), channel)
    torch.cuda.synchronize()
    assert got["ssd"].tolist() == want["ssd"], (what, got["ssd"].tolist(), want["ssd"])
    assert np.array_equal(got["hist_frame"].cpu().numpy().astype(np.int64), want["hist_frame"]), what
    assert np.array_equal(got["hist_ref"].cpu().numpy().astype(np.int64), want["hist_ref"]), what
    for key in ("mse", "chisq"):
        g = got[key].tolist()
        print(f"{what} {key}: device {g} restatement {want[key]}")
        assert all(_near(a, b) for a, b in zip(g, want[key])), (what, key, g, want[key])


@pytest.mark.parametrize("B", [1, 2, 7])
@pytest.mark.parametrize("H,W", [(224, 224), (480, 640), (360, 300), (37, 53), (1, 1)])
def test_frame_change_equals_the_restatement(H, W, B):
    rng = np.random.default_rng(100000 * H + 10 * W + B)
    shape = (B, H, W, 3)
    rand = lambda: rng.integers(0, 256, shape, dtype=np.uint8)
    one_byte = rand()
    one_byte_ref = one_byte.copy()
    for b in range(B):                                   # one byte per clip differs, anywhere in the frame
        i = int(rng.integers(0, H * W * 3))
        one_byte.reshape(B, -1)[b, i] ^= np.uint8(1 + rng.integers(0, 255))
    colour, colour_ref = np.empty(shape, np.uint8), np.empty(shape, np.uint8)
    colour[...] = np.array([17, 130, 255], np.uint8)     # one constant colour: every count in one bin
    colour_ref[...] = np.array([16, 0, 254], np.uint8)
    same = rand()
    cases = {"random": (rand(), rand()), "identical": (same, same.copy()),
             "white on black": (np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)),
             "one colour": (colour, colour_ref), "same colour": (colour, colour.copy()), "one byte": (one_byte, one_byte_ref)}
    ran = 0
    for channel in (0, 1, 2):
        for name, (f, r) in cases.items():
            _check(f, r, channel, f"{H}x{W} B={B} channel {channel} {name}")
            ran += 1
    assert ran == 18


def test_frame_change_at_any_alignment():
    """Frames that start off a 16-byte boundary (a scalar head and tail), and a pair whose addresses differ modulo 16 (no
    16-byte loads at all): the same numbers."""
    from gitcap.framegate import frame_change
    H, W, B = 61, 47, 2
    n = B * H * W * 3
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    want = R.frame_change(a.reshape(B, H, W, 3), b.reshape(B, H, W, 3), 1)
    ran = 0
    for off_f, off_r in ((0, 0), (1, 1), (5, 5), (15, 15), (0, 1), (3, 8), (16, 0), (7, 23)):
        buf_f = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        buf_r = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        assert buf_f.data_ptr() % 16 == 0 and buf_r.data_ptr() % 16 == 0
        f, r = buf_f[off_f:off_f + n].view(B, H, W, 3), buf_r[off_r:off_r + n].view(B, H, W, 3)
        f.copy_(torch.from_numpy(a).view(B, H, W, 3))
        r.copy_(torch.from_numpy(b).view(B, H, W, 3))
        assert f.is_contiguous() and f.data_ptr() % 16 == off_f % 16
        got = frame_change(f, r, 1)
        assert got["ssd"].tolist() == want["ssd"], (off_f, off_r)
        assert np.array_equal(got["hist_frame"].cpu().numpy(), want["hist_frame"]), (off_f, off_r)
        assert np.array_equal(got["hist_ref"].cpu().numpy(), want["hist_ref"]), (off_f, off_r)
        assert all(_near(x, y) for x, y in zip(got["chisq"].tolist(), want["chisq"])), (off_f, off_r)
        ran += 1
    assert ran == 8


def test_frame_change_null_outputs_and_bad_arguments():
    from gitcap import _lib
    from gitcap.framegate import OUTPUTS, frame_change
    lib = _lib.load()
    B, H, W = 2, 37, 53
    rng = np.random.default_rng(9)
    f_np, r_np = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    f, r = torch.from_numpy(f_np).cuda(), torch.from_numpy(r_np).cuda()
    want = R.frame_change(f_np, r_np, 2)
    full = frame_change(f, r, 2)
    st = stream()
    # every output alone (the other four null), through the binding; all null: accepted, nothing to do
    for key in OUTPUTS:
        one = frame_change(f, r, 2, outputs=(key,))
        assert list(one) == [key] and torch.equal(one[key], full[key]), key
    assert full["ssd"].tolist() == want["ssd"] and all(_near(a, b) for a, b in zip(full["chisq"].tolist(), want["chisq"]))
    assert frame_change(f, r, 2, outputs=()) == {}
    # a side stream: ordered on that stream, same numbers
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        on_side = frame_change(f, r, 2)
    side.synchronize()
    assert all(torch.equal(on_side[k], full[k]) for k in OUTPUTS)
    # bad arguments: refused, nothing is launched and the guard word behind the output stays
    out = torch.full((B + 1,), -7, dtype=torch.int64, device="cuda")
    call = lambda fp, rp, b, h, w, ch: lib.gitcap_frame_change(fp, rp, b, h, w, ch, ptr(out), None, None, None, None, st)
    for args in ((None, ptr(r), B, H, W, 2), (ptr(f), None, B, H, W, 2), (ptr(f), ptr(r), 0, H, W, 2), (ptr(f), ptr(r), -1, H, W, 2),
                 (ptr(f), ptr(r), B, 0, W, 2), (ptr(f), ptr(r), B, H, 0, 2), (ptr(f), ptr(r), B, H, W, 3), (ptr(f), ptr(r), B, H, W, -1)):
        assert call(*args) == ERR_ARG, args
    torch.cuda.synchronize()
    assert out.tolist() == [-7] * (B + 1)
    assert call(ptr(f), ptr(r), B, H, W, 2) == 0
    torch.cuda.synchronize()
    assert out.tolist() == want["ssd"] + [-7]
    with pytest.raises(ValueError):
        frame_change(f, r[:1], 2)
    with pytest.raises(_lib.GitcapError):
        frame_change(f, r, 5)


# ---------------------------------------------------------------------------------------------------- gated streams
_MODELS = {}


def _model(name):
    """tiny / 21m: StudentCaptioner with the native TinyViT encoder; git: GitCaptioner (git_tiny, 4 frames).  Built once."""
    if name not in _MODELS:
        if name == "git":
            from gitcap.model import GitCaptioner
            cfg = git_tiny(4)
            _MODELS[name] = GitCaptioner(cfg, synthetic_weights(cfg, 3), max_batch=2, max_frames=4, max_text_len=8, stop="never")
        else:
            from gitcap.student import StudentCaptioner
            from gitcap.tinyvit import TinyViTEncoder
            tcfg = tinyvit_tiny() if name == "tiny" else tinyvit_config("tiny_vit_21m_224")
            scfg = student_tiny() if name == "tiny" else student_base()
            weights = dict(student_synthetic_weights(scfg, 0))
            weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
            enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=2 * scfg.mem_tokens)
            _MODELS[name] = StudentCaptioner(cfg=scfg, weights=weights, image_encoder=enc, device="cuda:0", max_batch=2,
                                             max_text_len=12, stop="never")
    return _MODELS[name]


SIZES = {"tiny": (120, 160), "21m": (480, 640), "git": (60, 80)}
THRESHOLD = {"mse": 100.0, "hist": 20.0}
RANGES = ((0, 256), (0, 128), (128, 256), (64, 192))
# scene of each pushed frame, per clip: runs of repeated / near-repeated frames; clip 1 changes scene at other times than clip 0
SCENES = ([0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 4, 4, 5, 5, 5, 6, 6, 7, 8, 8, 9, 9],
          [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 6, 6, 6])
GROUPS = [1, 1, 2, 1, 3, 1, 1, 4, 1, 2, 1, 1, 2, 1]                         # frames per push: 22 in all


def _window(m):
    return m.cfg.mem_tokens if hasattr(m.cfg, "mem_tokens") else m.cfg.num_frames


def _stream(m, B, gate=None):
    return m.caption_stream(batch=B, hop=1, max_len=8, stop="never", gate=gate)


def _feed(name, B, seed):
    """uint8 [B,22,H,W,3] on the CPU: frame t of clip c shows scene SCENES[c][t]; the first frame of a run is the scene itself, a
    later one the scene with five bytes raised by one (a near-repeat)."""
    H, W = SIZES[name]
    out = np.empty((B, len(SCENES[0]), H, W, 3), np.uint8)
    for c in range(B):
        for t, s in enumerate(SCENES[c]):
            lo, hi = RANGES[s % 4]
            scene = np.random.default_rng(seed + 100 * s + c).integers(lo, hi, (H, W, 3), dtype=np.uint8)
            if t and SCENES[c][t - 1] == s:
                idx = np.random.default_rng(seed + 7 * t + c).integers(0, scene.size, 5)
                scene.reshape(-1)[idx] = np.minimum(scene.reshape(-1)[idx].astype(np.int64) + 1, 255).astype(np.uint8)
            out[c, t] = scene
    return torch.from_numpy(out)


def _pushes(feed):
    """The feed cut into pushes of GROUPS frames: a single frame goes in as [B,H,W,3], several as [B,n,H,W,3]."""
    t = 0
    for n in GROUPS:
        yield list(range(t, t + n)), (feed[:, t] if n == 1 else feed[:, t:t + n])
        t += n
    assert t == feed.shape[1]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return all(_same(a[k], b[k]) for k in a)
    return a.device == b.device and a.shape == b.shape and torch.equal(a, b)


CASES = [(n, B, metric) for n in ("tiny", "21m", "git") for B in (1, 2) for metric in ("mse", "hist")]


@pytest.mark.parametrize("name,B,metric", CASES)
def test_gate_that_admits_everything_changes_nothing(name, B, metric):
    from gitcap.framegate import FrameGate
    m = _model(name)
    feed = _feed(name, B, 11)
    gate = FrameGate(metric, -1.0)
    st = _stream(m, B, gate)
    got = [st.push(x) for _, x in _pushes(feed)]
    assert gate.stats["pushed"] == gate.stats["looked_at"] == gate.stats["admitted"] == feed.shape[1]
    st = _stream(m, B)
    want = [st.push(x) for _, x in _pushes(feed)]
    assert sum(w is not None for w in want) >= 8
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (i, g, w)
    # frames already on the device: the caption stays there
    st = _stream(m, B, gate)
    dev = [st.push(x.cuda()) for _, x in _pushes(feed)]
    for i, (g, w) in enumerate(zip(dev, want)):
        assert (g is None and w is None) or (g.device.type == "cuda" and torch.equal(g.cpu(), w)), i


@pytest.mark.parametrize("name,B,metric", CASES)
def test_gated_stream_captions_what_the_restatement_admits(name, B, metric):
    from gitcap.framegate import FrameGate
    m = _model(name)
    feed = _feed(name, B, 23)
    thr = THRESHOLD[metric]
    frames = [feed[:, t].numpy() for t in range(feed.shape[1])]
    admitted, looked = R.admit_sequence(frames, metric, thr, channel=2)
    # no decision near a rounding edge: every distance is at most half the threshold or at least twice it
    for t, dist in looked:
        assert all(d <= thr / 2 or d >= 2 * thr for d in dist), (t, dist, thr)
    rejected = [t for t, _ in looked if t not in admitted]
    assert len(admitted) >= _window(m) + 2 and len(rejected) >= 4, (admitted, rejected)
    if B == 2:                            # the any-clip rule is exercised: one clip far, the other near
        assert any(t in admitted and min(dist) <= thr / 2 for t, dist in looked)

    gate = FrameGate(metric, thr)
    kept = []
    inner = gate.admit
    gate.admit = lambda x: kept.append(inner(x)) or kept[-1]
    st = _stream(m, B, gate)
    got, seen = [], []
    for idx, x in _pushes(feed):
        got.append(st.push(x))
        seen += [idx[i] for i in kept[-1]]
        last = [d for t, d in looked if t <= idx[-1]]
        if last:                                         # the distances of the last looked-at frame, from the device
            dev = gate.stats["last_distance"]
            print(f"{name} B={B} {metric} frame {idx[-1]}: device {dev} restatement {last[-1]}")
            assert all(_near(a, b) for a, b in zip(dev, last[-1])), (idx, dev, last[-1])
    assert seen == admitted, (seen, admitted)
    assert gate.stats["pushed"] == feed.shape[1] and gate.stats["admitted"] == len(admitted)
    assert gate.stats["looked_at"] == len(looked) + 1

    st = _stream(m, B)                                   # ungated, fed only what the restatement admits, grouped as the pushes were
    captions = 0
    for (idx, _), g in zip(_pushes(feed), got):
        adm = [t for t in idx if t in admitted]
        if not adm:
            assert g is None, idx
            continue
        w = st.push(feed[:, adm])
        assert _same(g, w), (idx, adm, g, w)
        captions += w is not None
    assert captions >= 2


@pytest.mark.parametrize("name,B,metric", CASES)
def test_gate_above_every_distance_admits_one_frame(name, B, metric):
    from gitcap.framegate import FrameGate
    m = _model(name)
    feed = _feed(name, B, 31)
    H, W = SIZES[name]
    # mse <= 255^2.  chi-square: a term is (hr - hf)^2 / hr <= hr + hf^2 (hr >= 1), so the sum is <= P + P^2, P = H*W pixels
    thr = 65025.0 if metric == "mse" else float(H * W + (H * W) ** 2)
    gate = FrameGate(metric, thr)
    st = _stream(m, B, gate)
    outs = [st.push(x) for _, x in _pushes(feed)]
    assert all(o is None for o in outs)
    assert gate.stats["pushed"] == feed.shape[1] == gate.stats["looked_at"] and gate.stats["admitted"] == 1
    assert len(gate.stats["last_distance"]) == B
    st.reset()                                           # resets the gate: the next frame is admitted again
    assert gate.stats["pushed"] == 0 and st.push(torch.zeros_like(feed[:, 0])) is None and gate.stats["admitted"] == 1
    if metric == "mse":                                  # white against black reaches the bound and is still not above it
        assert st.push(torch.full_like(feed[:, 0], 255)) is None
        assert gate.stats["last_distance"] == [65025.0] * B and gate.stats["admitted"] == 1
    with pytest.raises(ValueError):
        st.push(torch.zeros((B, 3, 32, 32)))             # a gated stream takes camera frames only
