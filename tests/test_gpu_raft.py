"""GPU: RAFT2 / SEA-RAFT optical flow (csrc/raft.hip through the C ABI a3r_raft_*; default arithmetic since round 3: the
two-plane fp16 kernels, with the three-plane bf16 ones as the range fallback) against goldens produced by the
reference's own third_party/RAFT modules in the build container with the build's synthetic weights (tests/golden/raft.npz,
tests/golden/make_goldens.py --only raft; inputs are rebuilt here by align3r_amd.raft_weights.synthetic_raft_frames).

  * TINY configuration, 2 pairs 128 x 160, 3 iterations: every stage -- context network + init_conv, both feature maps, the four
    correlation-pyramid levels, the first heads, the first correlation lookup and motion features, hidden state and coarse flow after
    every iteration -- at max|a - b| / max|b| < 1e-4, and the final up-sampled flow at 1e-4;
  * RAFT_M (the configuration the reference's load_RAFT builds), called as the reference calls it (iters = 20, test_mode = True):
    first prediction and final flow, both at 1e-4 (measured: 2-5e-6 after 20 recurrent steps).

Both of the above run in BOTH arithmetics (A3R_RAFT = fh2, bf3): the fallback is compared with the reference, not only with itself
(measured: TINY stages <= 1.5e-6 fh2 / 1.9e-6 bf3; M after 20 iterations 2.7e-6 / 3.6e-6 fh2, 3.1e-6 / 4.9e-6 bf3).  Further
(tests/golden/raft_clip.<n>.npz, make_goldens.py --only raftclip):
  * RAFT_M at the sizes the pipeline runs, 288 x 512 (odd pyramid level in H) and 384 x 512, final flow at 1e-4: 6.0e-6 / 3.1e-6 fh2,
    6.7e-6 / 5.4e-6 bf3 (the reference's own fp32-versus-float64 difference: 2.7e-6 / 1.7e-6); B = 3 at 288 x 512 with the middle pair
    bitwise the B = 1 result;
  * small feature maps (fnet.final_conv x 2^-8 and x 2^-16): feature maps, the four correlation levels, the first lookup and motion
    features at 1e-4 of each tap's maximum.  Before the correlation operands got a per-image power-of-two scale (csrc/raft.hip) the fh2
    correlation taps measured 2.5e-5 (2^-8) and 5.7e-3 (2^-16, failing); now <= 7.8e-7 in both cases, bf3 <= 8.5e-7.
  * a ragged frame, 176 x 168 (tests/golden/raft_odd.<n>.npz, make_goldens.py --only raftodd): half-resolution width 84 (% 8 = 4) in
    the stems, a 22 x 21 eighth-resolution map (w % 4 = 1 in the depthwise convolution) with pyramid 22x21, 11x10, 5x5, 2x2: RAFT_TINY
    stage by stage and RAFT_M's final flow after 20 iterations, both arithmetics, at 1e-4.
What is pinned: every stage at 128 x 160 and at 176 x 168 in both arithmetics, the final flow at five sizes, the correlation path over
a 2^16 range of feature-map magnitudes.  The kernels of csrc/raft.hip that have no GEMM shape are pinned one by one against float64 at
their own tolerances, ragged tails, border arithmetic and second loop trips included, in tests/test_gpu_flow_kernels_f64.py (DESIGN
has the table).  Not pinned: intermediate stages of RAFT_M, level 0 of the correlation pyramid at 176 x 168 (462 x 462 values: its
GEMM is pinned at 128 x 160, its lookup operator by operator), and large (> 2^15) feature maps against the reference (the fallback
test checks those bitwise against bf3 only).
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, record_margin, rel_err
from align3r_amd.raft_weights import RAFT_M, RAFT_TINY, synthetic_raft_frames, synthetic_raft_state_dict

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "raft.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


ARITH = ["fh2", "bf3"]          # A3R_RAFT: the default two-plane fp16 kernels and the documented range fallback, both against the reference


def engine(monkeypatch, arith, cfg, sd):
    """A RaftEngine whose arithmetic is chosen as a user chooses it (A3R_RAFT, read when the engine is built)."""
    from align3r_amd.raft import RaftEngine
    monkeypatch.setenv("A3R_RAFT", arith)
    eng = RaftEngine(cfg, sd)
    assert eng.fh2 == (arith == "fh2")
    return eng


@pytest.mark.parametrize("arith", ARITH)
def test_raft_tiny_stages_and_flow(g, monkeypatch, arith):
    cfg = RAFT_TINY
    eng = engine(monkeypatch, arith, cfg, synthetic_raft_state_dict(cfg, 0))
    B, H, W, iters = 2, 128, 160, 3
    h, w, d = H // 8, W // 8, cfg.dim
    i1, i2 = synthetic_raft_frames(B, H, W, 7)
    ccp = (cfg.corr_channel + 31) // 32 * 32
    z = lambda *s: torch.zeros(*s, device="cuda")
    taps = dict(cnet=z(B, h, w, 2 * d), fmap=z(2 * B, h, w, 2 * d), flow_update0=z(B, h, w, 6), weight0=z(B, h, w, 576),
                lookup0=z(B, h, w, ccp), motion0=z(B, h, w, d))
    hl, wl = h, w
    for l in range(cfg.corr_levels):
        taps[f"corr_pyr{l}"] = z(B * h * w, hl, wl)
        hl, wl = hl // 2, wl // 2
    for it in range(iters):
        taps[f"net{it}"] = z(B, h, w, d)
        taps[f"flow8_{it}"] = z(B, h, w, 2)
    flow = eng.forward(dev(i1), dev(i2), iters=iters, taps=taps)
    t = {k: v.cpu().numpy() for k, v in taps.items()}
    m = {}
    m["cnet"] = rel_err(t["cnet"], g["t_cnet"])
    m["fmap1"] = rel_err(t["fmap"][:B], g["t_fmap1"])
    m["fmap2"] = rel_err(t["fmap"][B:], g["t_fmap2"])
    for l in range(cfg.corr_levels):
        m[f"corr_pyr{l}"] = rel_err(t[f"corr_pyr{l}"], g[f"t_corr_pyr{l}"][:, 0])
    m["flow_update0"] = rel_err(t["flow_update0"], g["t_flow_update0"])
    m["weight0"] = rel_err(t["weight0"], g["t_weight0"])
    m["lookup0"] = rel_err(t["lookup0"][..., :cfg.corr_channel], g["t_corr_lookup0"])
    assert not t["lookup0"][..., cfg.corr_channel:].any()           # the K padding of convc1 is zero-filled
    m["motion0"] = rel_err(t["motion0"], g["t_motion0"])
    for it in range(iters):
        m[f"net{it}"] = rel_err(t[f"net{it}"], g[f"t_net_{it}"])
        m[f"flow8_{it}"] = rel_err(t[f"flow8_{it}"], g[f"t_flow8_{it}"])
    m["flow"] = rel_err(flow.cpu().numpy(), g["t_flow"])
    record_margin("raft_tiny_vs_reference" + ("" if arith == "fh2" else "_" + arith), **m)
    bad = {k: v for k, v in m.items() if not v < TOL}
    assert not bad, bad
    assert eng.range_fallbacks == 0                                 # the arithmetic asked for is the one that was compared
    # zero iterations: the prediction from the context network alone (raft.py:213-220)
    f0 = eng.forward(dev(i1), dev(i2), iters=0)
    assert rel_err(f0.cpu().numpy(), g["t_flow_up_0"]) < TOL
    # batch invariance: pair 1 alone
    f1 = eng.forward(dev(i1[1:]), dev(i2[1:]), iters=iters)
    assert rel_err(f1.cpu().numpy(), flow[1:].cpu().numpy()) < 1e-5


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("tag,H,W,seed", [("m1", 128, 160, 11), ("m2", 160, 192, 13)])
def test_raft_m_as_the_reference_calls_it(g, monkeypatch, arith, tag, H, W, seed):
    """RAFT_M, iters = 20: the first iteration's prediction and the final flow (|flow| up to ~130 px with these random weights, 20
    recurrent steps) at 1e-4 of their maximum (measured: 2-5e-6; margins are recorded)."""
    from align3r_amd.raft import RAFT2
    monkeypatch.setenv("A3R_RAFT", arith)
    net = RAFT2(RAFT_M, synthetic_raft_state_dict(RAFT_M, 0)).to("cuda").eval()
    assert net._engine.fh2 == (arith == "fh2")
    i1, i2 = synthetic_raft_frames(1, H, W, seed)
    one = net(dev(i1), dev(i2), iters=1, test_mode=True)[1].cpu().numpy()
    out = net(dev(i1), dev(i2), iters=20, test_mode=True)
    assert isinstance(out, list) and len(out) == 2 and tuple(out[1].shape) == (1, 2, H, W)
    e1, e20 = rel_err(one, g[f"{tag}_flow_up_1"]), rel_err(out[1].cpu().numpy(), g[f"{tag}_flow"])
    record_margin(f"raft_m_{tag}_vs_reference" + ("" if arith == "fh2" else "_" + arith), flow_iter1=e1, flow_iter20=e20)
    assert e1 < TOL, e1
    assert e20 < TOL, e20
    assert net._engine.range_fallbacks == 0


def load_parts(stem):
    """tests/golden/<stem>.<n>.npz -> dict name -> array: a fixture written as numbered parts (no committed file above 1 MiB), an
    array larger than a part cut along its flattened length into `name@k` pieces (make_goldens.py:gen_raftclip)."""
    pieces, shapes, n = {}, {}, 0
    while os.path.exists(os.path.join(GOLDEN, f"{stem}.{n}.npz")):
        with np.load(os.path.join(GOLDEN, f"{stem}.{n}.npz")) as z:
            assert all(z[k].dtype in (np.float32, np.int64) for k in z.files)          # arrays only
            for k in z.files:
                name, idx = k.rsplit("@", 1)
                if idx == "shape":
                    shapes[name] = tuple(int(x) for x in z[k])
                else:
                    pieces.setdefault(name, {})[int(idx)] = z[k]
        n += 1
    assert n > 0 and set(pieces) == set(shapes), (stem, n)
    return {k: np.concatenate([pieces[k][i] for i in range(len(pieces[k]))]).reshape(shapes[k]) for k in shapes}


@pytest.fixture(scope="module")
def gc():
    """raft_clip (make_goldens.py --only raftclip).  low16's feature maps and correlation taps are low8's times 2^-8 / 2^-16 bit for bit
    in the fp32 reference (the generator asserts it), so they are stored once and rebuilt here by that exact multiplication."""
    g = load_parts("raft_clip")
    for k, p2 in dict(fmap1=-8, fmap2=-8, corr_pyr0=-16, corr_pyr1=-16, corr_pyr2=-16, corr_pyr3=-16, corr_lookup0=-16).items():
        g["low16_" + k] = g["low8_" + k] * np.float32(2.0 ** p2)
    return g


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("tag,H,W,seed", [("c288", 288, 512, 23), ("c384", 384, 512, 29)])
def test_raft_m_at_the_sizes_the_pipeline_runs(gc, monkeypatch, arith, tag, H, W, seed):
    """RAFT_M as the reference calls it at 288 x 512 (what the loader emits for 16:9 clips: the 1/8 map is 36 x 64 and the correlation
    pyramid 36, 18, 9, 4 -- an odd level in H) and 384 x 512 (BASELINE config 4, bench.py's raft_flow): widths 256 / 128 / 64 in the
    stems and strided convs, and other GEMM tiles than at the small test sizes.  Final flow at TOL = 1e-4 of max|flow| (156 / 180 px);
    the reference's own fp32-versus-float64 difference is 2.7e-6 / 1.7e-6 there (make_goldens.py:gen_raftclip)."""
    from align3r_amd.raft import RAFT2
    monkeypatch.setenv("A3R_RAFT", arith)
    net = RAFT2(RAFT_M, synthetic_raft_state_dict(RAFT_M, 0)).to("cuda").eval()
    assert net._engine.fh2 == (arith == "fh2")
    i1, i2 = synthetic_raft_frames(1, H, W, seed)
    out = net(dev(i1), dev(i2), iters=20, test_mode=True)
    assert isinstance(out, list) and len(out) == 2 and tuple(out[1].shape) == (1, 2, H, W)
    e = rel_err(out[1].cpu().numpy(), gc[f"{tag}_flow"])
    record_margin(f"raft_m_{tag}_vs_reference_{arith}", flow_iter20=e, max_abs_flow=float(np.abs(gc[f"{tag}_flow"]).max()))
    assert e < TOL, e
    assert net._engine.range_fallbacks == 0
    if H == 288:
        # batch invariance at this shape: the same pair in the middle of a batch of three is the B = 1 result bit for bit
        a1, a2 = synthetic_raft_frames(2, H, W, seed + 1)
        j1, j2 = np.stack([a1[0], i1[0], a1[1]]), np.stack([a2[0], i2[0], a2[1]])
        out3 = net(dev(j1), dev(j2), iters=20, test_mode=True)[1]
        assert tuple(out3.shape) == (3, 2, H, W)
        assert torch.equal(out3[1], out[1][0])
        assert not torch.equal(out3[0], out[1][0])


@pytest.fixture(scope="module")
def go():
    """raft_odd (make_goldens.py --only raftodd): one pair of 176 x 168 frames, frame seed 41"""
    return load_parts("raft_odd")


@pytest.mark.parametrize("arith", ARITH)
def test_raft_ragged_widths(go, monkeypatch, arith):
    """176 x 168: no width of this frame is a multiple of a kernel's column group -- 84 columns at half resolution (8 per thread in the
    stems), 21 at one eighth (4 per thread in the depthwise convolution, 8 in convf1) -- and the pyramid is 22x21, 11x10, 5x5, 2x2.
    RAFT_TINY, 3 iterations, every stored stage, and RAFT_M's final flow after 20 iterations, each at TOL of its own maximum."""
    from align3r_amd.raft import RAFT2
    cfg = RAFT_TINY
    eng = engine(monkeypatch, arith, cfg, synthetic_raft_state_dict(cfg, 0))
    B, H, W, iters = 1, 176, 168, 3
    h, w, d = H // 8, W // 8, cfg.dim
    i1, i2 = synthetic_raft_frames(B, H, W, 41)
    ccp = (cfg.corr_channel + 31) // 32 * 32
    z = lambda *s: torch.full(s, float("nan"), device="cuda")
    taps = dict(cnet=z(B, h, w, 2 * d), fmap=z(2 * B, h, w, 2 * d), lookup0=z(B, h, w, ccp), motion0=z(B, h, w, d))
    hl, wl = h, w
    for l in range(cfg.corr_levels):
        taps[f"corr_pyr{l}"] = z(B * h * w, hl, wl)
        hl, wl = hl // 2, wl // 2
    assert (hl * 2, wl * 2) == (2, 2)
    for it in range(iters):
        taps[f"net{it}"] = z(B, h, w, d)
        taps[f"flow8_{it}"] = z(B, h, w, 2)
    flow = eng.forward(dev(i1), dev(i2), iters=iters, taps=taps)
    t = {k: v.cpu().numpy() for k, v in taps.items()}
    assert all(np.isfinite(v).all() for v in t.values())            # every tap fully written
    m = dict(cnet=rel_err(t["cnet"], go["t_cnet"]), fmap1=rel_err(t["fmap"][:B], go["t_fmap1"]), fmap2=rel_err(t["fmap"][B:], go["t_fmap2"]))
    for l in range(1, cfg.corr_levels):
        m[f"corr_pyr{l}"] = rel_err(t[f"corr_pyr{l}"], go[f"t_corr_pyr{l}"])
    m["lookup0"] = rel_err(t["lookup0"][..., :cfg.corr_channel], go["t_corr_lookup0"])
    assert not t["lookup0"][..., cfg.corr_channel:].any()
    m["motion0"] = rel_err(t["motion0"], go["t_motion0"])
    for it in range(iters):
        m[f"net{it}"] = rel_err(t[f"net{it}"], go[f"t_net_{it}"])
        m[f"flow8_{it}"] = rel_err(t[f"flow8_{it}"], go[f"t_flow8_{it}"])
    m["flow"] = rel_err(flow.cpu().numpy(), go["t_flow"])
    assert eng.range_fallbacks == 0
    net = RAFT2(RAFT_M, synthetic_raft_state_dict(RAFT_M, 0)).to("cuda").eval()
    assert net._engine.fh2 == (arith == "fh2")
    out = net(dev(i1), dev(i2), iters=20, test_mode=True)[1]
    assert tuple(out.shape) == (1, 2, H, W)
    m["m_flow_iter20"] = rel_err(out.cpu().numpy(), go["m_flow"])
    record_margin(f"raft_ragged_vs_reference_{arith}", **m)
    bad = {k: v for k, v in m.items() if not v < TOL}
    assert not bad, bad
    assert net._engine.range_fallbacks == 0


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("tag,scale", [("low8", 2.0 ** -8), ("low16", 2.0 ** -16)])
def test_raft_small_feature_maps(gc, monkeypatch, arith, tag, scale):
    """A checkpoint whose feature maps are small: weight and bias of fnet.final_conv scaled by 2^-8 / 2^-16, so max|fmap| is 7.9e-3 /
    3.1e-5 and the correlation volume tops out at 6.5e-5 / 9.9e-10 -- where two fp16 planes stored at scale 1 stop being fp32-grade
    (csrc/fh2.h: absolute error 2^-25 / s below the band).  Every tap on the correlation path against the fp32 reference, each at
    TOL = 1e-4 of that tap's own maximum (the reference's fp32-versus-float64 noise on these taps is 3e-7 .. 1.5e-6).  The three-plane
    bf16 form has fp32's range: it passing shows the fixture is fair.
    The final flow is compared too, but it cannot see this path: max|flow| is 3.0419796 for low8 and 3.0419750 for low16 -- with the
    synthetic weights the flow hardly depends on the correlation volume (asserted below), so the taps are the assertion."""
    cfg = RAFT_TINY
    sd = dict(synthetic_raft_state_dict(cfg, 0))
    for k in ("fnet.final_conv.weight", "fnet.final_conv.bias"):
        sd[k] = sd[k] * np.float32(scale)
    eng = engine(monkeypatch, arith, cfg, sd)
    B, H, W, iters = 1, 128, 160, 3
    h, w, d = H // 8, W // 8, cfg.dim
    i1, i2 = synthetic_raft_frames(B, H, W, 31)
    ccp = (cfg.corr_channel + 31) // 32 * 32
    z = lambda *s: torch.zeros(*s, device="cuda")
    taps = dict(fmap=z(2 * B, h, w, 2 * d), lookup0=z(B, h, w, ccp), motion0=z(B, h, w, d))
    hl, wl = h, w
    for l in range(cfg.corr_levels):
        taps[f"corr_pyr{l}"] = z(B * h * w, hl, wl)
        hl, wl = hl // 2, wl // 2
    flow = eng.forward(dev(i1), dev(i2), iters=iters, taps=taps)
    t = {k: v.cpu().numpy() for k, v in taps.items()}
    m = dict(fmap1=rel_err(t["fmap"][:B], gc[f"{tag}_fmap1"]), fmap2=rel_err(t["fmap"][B:], gc[f"{tag}_fmap2"]))
    for l in range(cfg.corr_levels):
        m[f"corr_pyr{l}"] = rel_err(t[f"corr_pyr{l}"], gc[f"{tag}_corr_pyr{l}"])
    m["lookup0"] = rel_err(t["lookup0"][..., :cfg.corr_channel], gc[f"{tag}_corr_lookup0"])
    m["motion0"] = rel_err(t["motion0"], gc[f"{tag}_motion0"])
    m["flow"] = rel_err(flow.cpu().numpy(), gc[f"{tag}_flow"])
    record_margin(f"raft_tiny_{tag}_vs_reference_{arith}", max_abs_flow=float(np.abs(gc[f"{tag}_flow"]).max()), **m)
    bad = {k: v for k, v in m.items() if not v < TOL}
    assert not bad, bad
    assert eng.range_fallbacks == 0                                 # small maps are handled in the arithmetic asked for, not by a repeat
    # written down beside the test: the reference's final flows of the two cases agree to 2.7e-5 of their maximum although their
    # correlation volumes differ by a factor 2^16 -- inside what TOL allows, so a final-flow comparison alone could not tell a
    # correlation volume that is wrong by that factor from a right one
    assert rel_err(gc["low8_flow"], gc["low16_flow"]) < TOL


def test_raft_per_frame_feature_cache_is_bitwise_the_full_forward():
    """a3r_raft_encode + a3r_raft_forward_features against a3r_raft_forward: a frame's feature map does not depend on the batch it was
    encoded in nor on its partner, so the flow from cached per-frame features equals the full forward's bit for bit (what
    cloud_opt_flow.get_flow relies on when it encodes every frame once)."""
    from align3r_amd.raft import RaftEngine
    eng = RaftEngine(RAFT_TINY, synthetic_raft_state_dict(RAFT_TINY, 0))
    i1, i2 = synthetic_raft_frames(3, 128, 160, 17)
    frames = dev(np.concatenate([i1, i2]))                         # six frames
    fm_all = eng.encode(frames)                                    # one batch of six
    fm_one = torch.cat([eng.encode(frames[k:k + 1].contiguous()) for k in range(6)])
    assert torch.equal(fm_all, fm_one)                             # batch-invariant
    full = eng.forward(frames[:3].contiguous(), frames[3:].contiguous(), iters=4)
    cached = eng.forward(frames[:3].contiguous(), frames[3:].contiguous(), iters=4, fmaps=(fm_all[:3].contiguous(), fm_all[3:].contiguous()))
    assert torch.equal(full, cached)
    back = eng.forward(frames[3:].contiguous(), frames[:3].contiguous(), iters=4, fmaps=(fm_all[3:].contiguous(), fm_all[:3].contiguous()))
    assert torch.equal(back, eng.forward(frames[3:].contiguous(), frames[:3].contiguous(), iters=4))
    one = eng.forward(frames[1:2].contiguous(), frames[4:5].contiguous(), iters=4, fmaps=(fm_all[1:2].contiguous(), fm_all[4:5].contiguous()))
    assert torch.equal(one, cached[1:2])                           # a pair's flow does not depend on the batch it is computed in
    with pytest.raises(RuntimeError, match="fmap1"):
        eng.forward(frames[:3].contiguous(), frames[3:].contiguous(), fmaps=(fm_all[:2].contiguous(), fm_all[3:].contiguous()))


def test_raft_fp16_range_fallback(monkeypatch):
    """The default arithmetic stores activations as two fp16 planes with scale 1: a call whose activations reach 2^15 is detected by
    the range statistic (a3r_raft_range) and repeated on the three-plane bf16 kernels -- the result is bitwise that of an engine
    created with A3R_RAFT=bf3, never a silently saturated one.  Ordinary weights do not trigger it."""
    from align3r_amd.raft import RaftEngine
    sd = synthetic_raft_state_dict(RAFT_TINY, 0)
    i1, i2 = synthetic_raft_frames(1, 128, 160, 5)
    ok = RaftEngine(RAFT_TINY, sd)
    ok.forward(dev(i1), dev(i2), iters=2)
    assert ok.fh2 and ok.range_fallbacks == 0
    big = dict(sd)
    big["cnet.layer1.0.conv1.weight"] = sd["cnet.layer1.0.conv1.weight"] * np.float32(3e5)      # context features far beyond 65504
    e2 = RaftEngine(RAFT_TINY, big)
    out = e2.forward(dev(i1), dev(i2), iters=2)
    assert e2.range_fallbacks == 1
    monkeypatch.setenv("A3R_RAFT", "bf3")
    e3 = RaftEngine(RAFT_TINY, big)
    assert not e3.fh2
    ref = e3.forward(dev(i1), dev(i2), iters=2)
    assert torch.isfinite(ref).all() and torch.equal(out, ref)


def test_raft_errors_are_loud():
    from align3r_amd.raft import RAFT2, RaftEngine
    sd = synthetic_raft_state_dict(RAFT_TINY, 0)
    eng = RaftEngine(RAFT_TINY, sd)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        eng.forward(torch.zeros(1, 3, 100, 160, device="cuda"), torch.zeros(1, 3, 100, 160, device="cuda"))
    with pytest.raises(RuntimeError, match="too small"):
        eng.forward(torch.zeros(1, 3, 64, 96, device="cuda"), torch.zeros(1, 3, 64, 96, device="cuda"))
    bad = dict(sd)
    del bad["fnet.layer2.0.conv1.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        RaftEngine(RAFT_TINY, bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        RAFT2(RAFT_TINY, sd)(torch.zeros(1, 3, 128, 160), torch.zeros(1, 3, 128, 160), test_mode=True)


def test_cloud_opt_flow_computes_its_flow_with_the_hip_raft():
    """The reference's flow variant computes optical flow for every edge, both directions, inside its constructor
    (cloud_opt_flow/optimizer.py:118-154).  Same here when a flow network is given: the fields the aligner receives are exactly
    RaftEngine's outputs for (img_i * 255, img_j * 255, iters = 20) in chunks of 12, the forward-backward masks exist, and the
    flow-regularised alignment runs on them."""
    from align3r_amd.dust3r.cloud_opt_flow import global_aligner
    from align3r_amd.raft import RAFT2
    from test_gpu_api import _geom_scene
    N, H, W = 3, 128, 160
    edges, p1, p2, c, cams, depths, f = _geom_scene(N, H, W)
    a, b = synthetic_raft_frames(N, H, W, 21)
    frames = [torch.from_numpy(a[n] / 255.0 * 2 - 1) for n in range(N)]          # view['img'] is normalised to [-1, 1] (ImgNorm)
    dyn = [torch.zeros(H, W, dtype=torch.bool) for _ in range(N)]
    out = dict(view1=dict(idx=[i for i, j in edges], img=torch.stack([frames[i] for i, j in edges]), dynamic_mask=[dyn[i] for i, j in edges]),
               view2=dict(idx=[j for i, j in edges], img=torch.stack([frames[j] for i, j in edges]), dynamic_mask=[dyn[j] for i, j in edges]),
               pred1=dict(pts3d=torch.from_numpy(p1), conf=torch.from_numpy(c)),
               pred2=dict(pts3d_in_other_view=torch.from_numpy(p2), conf=torch.from_numpy(c)))
    net = RAFT2(RAFT_TINY, synthetic_raft_state_dict(RAFT_TINY, 0))
    torch.manual_seed(0)
    scene = global_aligner(out, "cuda", verbose=False, min_conf_thr=1.5, flow_loss_weight=0.01, flow_net=net, num_total_iter=20,
                           flow_loss_start_epoch=0.0)
    fij, fji = scene._flow_pair
    assert tuple(fij.shape) == (len(edges), 2, H, W) and fij.is_cuda
    imgs = np.stack(scene.imgs)                                                     # [N, H, W, 3] in [0, 1], as rgb() leaves them
    x = lambda idx: torch.from_numpy(imgs[idx]).float().permute(0, 3, 1, 2).contiguous().cuda() * 255
    ei, ej = [i for i, j in edges], [j for i, j in edges]
    want = net._engine.forward(x(ei), x(ej), iters=20)
    assert torch.equal(fij, want)
    assert torch.equal(fji, net._engine.forward(x(ej), x(ei), iters=20))
    vi = scene.flow_valid_mask_i
    assert tuple(vi.shape)[0] == len(edges) and vi.dtype in (torch.bool, torch.float32)
    loss = scene.compute_global_alignment(init="mst", niter=20, schedule="linear", lr=0.01)
    assert np.isfinite(loss)
    with pytest.raises(RuntimeError, match="no RAFT checkpoint"):
        global_aligner(out, "cuda", verbose=False, flow_loss_weight=0.01)


# ---- the C ABI itself (ctypes): weights are bound once, by a3r_raft_finalize (csrc/raft.hip, RaftW)
class _RawRaft:
    """One a3r_raft handle driven through the C ABI: create, set every weight of `weights`, finalize (rc kept), forward."""

    def __init__(self, weights):
        import ctypes as C
        from align3r_amd import _lib
        self.C, self.L, self.lib = C, _lib, _lib.load()
        cfg = RAFT_TINY
        c = _lib.RaftConfigC(cfg.initial_dim, (C.c_int * 3)(*cfg.block_dims), (C.c_int * 3)(*cfg.n_blocks), cfg.dim, cfg.radius,
                             cfg.corr_levels, cfg.num_blocks)
        self.handle = C.c_void_p()
        _lib.check(self.lib.a3r_raft_create(C.byref(c), C.byref(self.handle)), "a3r_raft_create")
        self.tensors = {}
        for name, arr in weights.items():
            self.set_weight(name, arr)
        self.packed = torch.empty(int(self.lib.a3r_raft_packed_bytes(self.handle)), dtype=torch.uint8, device="cuda")
        self.finalize_rc = self.finalize()

    def set_weight(self, name, arr):
        t = self.tensors[name] = dev(arr)
        shp = (self.C.c_int64 * t.dim())(*t.shape)
        self.L.check(self.lib.a3r_raft_set_weight(self.handle, name.encode(), self.L.ptr(t), t.dim(), shp), name)

    def finalize(self):
        rc = self.lib.a3r_raft_finalize(self.handle, self.L.ptr(self.packed), self.packed.numel(), self.L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def forward(self, i1, i2, iters=2):
        """(rc, flow)"""
        B, _, H, W = i1.shape
        ws = torch.empty(int(self.lib.a3r_raft_workspace_bytes(self.handle, B, H, W)), dtype=torch.uint8, device="cuda")
        flow = torch.zeros(B, 2, H, W, device="cuda")
        rc = self.lib.a3r_raft_forward(self.handle, self.L.ptr(i1), self.L.ptr(i2), B, H, W, iters, self.L.ptr(flow), self.L.ptr(ws),
                                       ws.numel(), None, self.L.stream_ptr())
        torch.cuda.synchronize()
        return rc, flow

    def error(self):
        return self.lib.a3r_last_error().decode(errors="replace")

    def close(self):
        self.lib.a3r_raft_destroy(self.handle)


@pytest.fixture(scope="module")
def raw():
    """(the weight set a3r_raft_set_weight takes for RAFT_TINY, one pair of 128 x 160 frames on the device); neither is modified."""
    from align3r_amd import _lib
    from align3r_amd.raft import engine_weights
    probe = _RawRaft({})
    width = _lib.load().a3r_raft_corr_width(probe.handle)
    probe.close()
    assert width == (RAFT_TINY.corr_channel + 31) // 32 * 32
    i1, i2 = synthetic_raft_frames(1, 128, 160, 31)
    return engine_weights(synthetic_raft_state_dict(RAFT_TINY, 0), RAFT_TINY, width), dev(i1), dev(i2)


@pytest.mark.parametrize("name", ["cnet.conv1.bias", "update_block.refine.1.norm.weight", "update_block.refine.0.dwconv.weight"])
def test_raft_finalize_reports_an_incomplete_weight_set(raw, name):
    """A bias, a norm weight, a depthwise weight left out: a3r_raft_finalize refuses and names it (before this was bound at finalize,
    a forward found it missing with earlier kernels already enqueued, and the depthwise launch did not look at all); the handle
    stays unfinalized, so a forward refuses too."""
    weights, i1, i2 = raw
    assert name in weights
    h = _RawRaft({k: v for k, v in weights.items() if k != name})
    try:
        assert h.finalize_rc != 0 and name in h.error()
        rc, _ = h.forward(i1, i2)
        assert rc != 0 and "has not been called" in h.error()
    finally:
        h.close()


def test_raft_set_weight_after_finalize_needs_a_new_finalize(raw):
    """The bound pointers of a finalized handle cannot go stale: a3r_raft_set_weight clears `finalized`, every forward refuses until
    a3r_raft_finalize has bound again, and the flow is then that of a fresh handle built with the changed weight, bit for bit."""
    weights, i1, i2 = raw
    name = "flow_head.2.bias"
    changed = dict(weights)
    changed[name] = (weights[name] + np.float32(0.25)).astype(np.float32)
    h, fresh = _RawRaft(weights), _RawRaft(changed)
    try:
        assert h.finalize_rc == 0 and fresh.finalize_rc == 0
        rc, before = h.forward(i1, i2)
        assert rc == 0, h.error()
        h.set_weight(name, changed[name])
        rc, _ = h.forward(i1, i2)
        assert rc != 0 and "has not been called" in h.error()
        assert h.finalize() == 0, h.error()
        rc, after = h.forward(i1, i2)
        assert rc == 0, h.error()
        rc, want = fresh.forward(i1, i2)
        assert rc == 0, fresh.error()
        assert torch.equal(after, want) and not torch.equal(after, before)
    finally:
        h.close()
        fresh.close()
