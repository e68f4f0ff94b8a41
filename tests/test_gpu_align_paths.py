"""GPU: the kernel forms of align.hip that the goldens never reach, each AlignEngine against AlignOracle on the same arrays --

  align_main_kernel<.., VEC = false>   P % 4 != 0 in all four (mono, L2) instantiations and modes 0 / 1 / 2, with train_pp,
                                       norm_pw_scale off and non-zero adaptors; P one below / above a chunk, P below a wave;
  align_main_kernel<.., VEC = true>    several chunks with a ragged last one, against the oracle (not only against itself);
  align_flow_kernel                    the scalar ego-flow pass (P % 4 != 0, and A3R_ALIGN_FLOW=v1 in a child process);
  align_flow_vec_kernel                more than 8 incident sides (batch rollover, odd tails), ragged last chunk, set dynamic
                                       masks, a pxl_thre that excludes pixels;
  align_flow_decide_kernel             kept / dropped a factor 2 either side of the threshold, the sticky flag, the start gate;
  align_depth_prior_kernel             P > 1024 (strided loops run more than once), the clamp branch, own dynamic weights.

The two forms of the ego-flow pass share one per-pixel body; test_flow_pass_bitwise_parent pins both, bit for bit, to what the
commit before that sharing computed (tests/golden/align_flow_parent.npz, written by make_goldens_align_flow_parent.py).

Problems come from tests/align_cases.py; tests/test_align_cases_cpu.py shows on the CPU that they are well posed (guard band
around pxl_thre, shares that bite).  Tolerances are those of tests/test_gpu_align.py and tests/test_oracle_align.py: first
loss 1e-6, gradients 1e-5 of the tensor max, trajectory losses 1e-5, states 1e-4, a term in isolation 1e-3.

Runtime of the whole file on one MI355X: not measured yet (DESIGN.md section 6.3 says what is still open); the problems have at
most 15 frames of 2080 pixels and one oracle evaluation of them takes well under a second."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases as ac
from conftest import REPO, record_margin, rel_err
from test_align_cases_cpu import FLOW_CASES, PRIOR_CASES, flow_case, make_oracle, oracle_flow_loss, prior_case
from test_gpu_align import _scene, host

pytestmark = pytest.mark.gpu

TOL = dict(loss=1e-6, grad=1e-5, losses=1e-5, state=1e-4, iso=1e-3, v1=1e-6)


@pytest.fixture(scope="module")
def Engine():
    from align3r_amd.aligner import AlignEngine
    return AlignEngine


def _check(case, margins):
    """Record, then assert every margin against the bound its prefix names."""
    record_margin("align_paths_" + case, **margins)
    for k, v in margins.items():
        assert np.isfinite(v) and v < TOL[k.split("_")[0]], (case, k, v, margins)


def _first_eval(o, a, epoch=9999, tag=""):
    lo, go = o.loss_grad(epoch)
    la, ga = a.loss_grad(epoch)
    assert set(go) == set(ga)
    m = {f"loss_{tag}first": abs(lo - la) / abs(lo)}
    for k in go:
        m[f"grad_{tag}{k}"] = rel_err(host(ga[k]).reshape(go[k].shape), go[k])
    return m, (lo, go), (la, ga)


def _trajectory(o, a, steps, lr, schedule, total=None):
    lo = np.asarray(o.run(steps, lr, schedule, total_iters=total))
    la = a.run(steps, lr, schedule, total_iters=total)
    m = dict(losses_run=rel_err(la, lo))
    for k in o.trainable():
        m[f"state_{k}"] = rel_err(host(a.params[k]).reshape(o.params[k].shape), o.params[k])
    return m


def _isolated(m, full, base, keys, tag):
    """A term in isolation: the difference of two gradients, engine against oracle."""
    (_, go1), (_, ga1) = full
    (_, go0), (_, ga0) = base
    for k in keys:
        ref = go1[k].astype(np.float64) - go0[k]
        mine = (host(ga1[k]).astype(np.float64) - host(ga0[k])).reshape(ref.shape)
        assert np.abs(ref).max() > 0, k
        m[f"iso_{tag}{k}"] = rel_err(mine, ref)


# ------------------------------------------------------------------------------------------------- main kernel
def _main_case(case, Engine, edges, N, H, W, mono, dist, seed=3, init_extra=None, **kw):
    """loss() == loss_grad() loss (mode 0 against mode 1), first evaluation, 20 cosine steps (mode 2)."""
    from oracle.align_ref import AlignOracle
    edges, p1, p2, w1, w2, m, init = _scene(edges, N, H, W, seed, mono)
    init.update(init_extra or {})
    args = ([i for i, j in edges], [j for i, j in edges], p1, p2, w1, w2, [(H, W)] * N)
    o = AlignOracle(*args, mono=m, dist=dist, **kw)
    a = Engine(*args, mono=m, dist=dist, train_adaptors=False, **kw)
    for eng in (o, a):
        eng.set_params(**init)
    margins, (lo, _), (la, _) = _first_eval(o, a)
    margins["loss_only_vs_grad"] = abs(float(a.loss().item()) - la) / abs(la)
    margins["loss_only_vs_oracle"] = abs(float(a.loss().item()) - lo) / abs(lo)
    margins.update(_trajectory(o, a, 20, 0.05, "cosine"))
    _check(case, margins)


CONFIGS = [(False, "l1"), (True, "l1"), (False, "l2"), (True, "l2")]


@pytest.mark.parametrize("mono,dist", CONFIGS, ids=[("mono_" if m else "") + d for m, d in CONFIGS])
@pytest.mark.parametrize("H,W", ac.RAGGED, ids=[f"{h}x{w}" for h, w in ac.RAGGED])
def test_main_ragged_vs_oracle(H, W, mono, dist, Engine):
    """P % 4 != 0: the !VEC main kernel, complete graph of 4 images."""
    _main_case(f"main_{H}x{W}_{'mono_' if mono else ''}{dist}", Engine, ac.complete_graph(4), 4, H, W, mono, dist)


@pytest.mark.parametrize("name", ["train_pp", "no_norm_pw_scale", "adaptors"])
def test_main_ragged_flags_vs_oracle(name, Engine):
    """37 x 41 on the degree-class graph with the flags that so far ran on the VEC instantiation only.  The adaptors are a fixed
    non-zero input (the oracle has no gradient for them)."""
    edges, N = ac.degree_class_graph()
    rng = np.random.default_rng(17)
    kw, extra = {}, {}
    if name == "train_pp":
        kw, extra = dict(train_pp=True), dict(im_pp=(0.05 * rng.standard_normal((N, 2))).astype(np.float32))
    elif name == "no_norm_pw_scale":
        kw = dict(norm_pw_scale=False)
    else:
        extra = dict(pw_adaptors=(2.0 * rng.standard_normal((len(edges), 2))).astype(np.float32))
    _main_case(f"main_37x41_deg_{name}", Engine, edges, N, 37, 41, False, "l1", init_extra=extra, **kw)


@pytest.mark.parametrize("mono", [False, True], ids=["plain", "mono"])
@pytest.mark.parametrize("H,W", ac.VEC_RAGGED, ids=[f"{h}x{w}" for h, w in ac.VEC_RAGGED])
def test_main_vec_ragged_last_chunk_vs_oracle(H, W, mono, Engine):
    """P % 4 == 0, P > 1024, P % 1024 != 0 on the degree-class graph."""
    edges, N = ac.degree_class_graph()
    _main_case(f"main_vec_{H}x{W}_{'mono' if mono else 'plain'}", Engine, edges, N, H, W, mono, "l1")


# ------------------------------------------------------------------------------------------------- ego-flow pass
def _engine(Engine, prob, **over):
    a = Engine(*prob["args"], **dict(prob["kw"], **over))
    a.set_params(**prob["init"])
    return a


def _flow_state(a):
    import ctypes as C
    from align3r_amd._lib import check
    st = np.zeros(5, np.float32)
    check(a.lib.a3r_align_flow_state(a.handle, st.ctypes.data_as(C.c_void_p)))
    return st


def _flow_keys(prob):
    return ["depth", "im_poses", "im_focals"] + (["im_pp"] if prob["kw"]["train_pp"] else [])


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_flow_biting_threshold_vs_oracle(name, Engine):
    """pxl_thre = 1.5 excludes most pixel components (guard-banded), 30 % dynamic pixels and one fully dynamic image: loss and
    every gradient with the flow term on and before its start iteration -- where the result must be that of the same problem built
    without flow -- and the flow term in isolation.  s*: scalar flow pass + !VEC main kernel consuming gflow; v*: vec forms."""
    prob = flow_case(name, True)
    o, a = make_oracle(prob), _engine(Engine, prob)
    m, ref_on, got_on = _first_eval(o, a, 9999, "on_")
    assert not a.flow_dropped and not o.flow_dropped and _flow_state(a)[3] == 0
    m["loss_only_on"] = abs(float(a.loss().item()) - ref_on[0]) / abs(ref_on[0])            # mode 0 with the flow variant on
    o_off = make_oracle(prob, flow=None)                                  # the same problem built without flow
    lo, go = o_off.loss_grad(0)
    la, ga = a.loss_grad(0)
    assert o.loss_grad(0)[0] == lo                                        # the oracle's own gate agrees
    m["loss_off_first"] = abs(lo - la) / abs(lo)
    for k in go:
        m[f"grad_off_{k}"] = rel_err(host(ga[k]).reshape(go[k].shape), go[k])
    assert abs(ref_on[0] - lo) / lo > 1e-4                                # the term is visible in the loss
    _isolated(m, (ref_on, got_on), ((lo, go), (la, ga)), _flow_keys(prob), "flow_")
    _check(f"flow_biting_{name}", m)


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_flow_loose_threshold_trajectory_vs_oracle(name, Engine):
    """pxl_thre = thre = 1e9: first evaluation, then 10 linear-schedule steps that cross the start gate at iteration 5."""
    prob = flow_case(name, False)
    o, a = make_oracle(prob), _engine(Engine, prob)
    m, _, _ = _first_eval(o, a, 9999, "on_")
    m.update(_trajectory(o, a, 10, 0.01, "linear", total=50))
    assert not a.flow_dropped and not o.flow_dropped
    _check(f"flow_loose_{name}", m)


@pytest.mark.parametrize("name", ["s37x41_win6_sf", "v36x44_deg_sf"], ids=["scalar", "vec"])
def test_flow_drop_decision(name, Engine):
    """thre a factor 2 either side of the flow loss L0 the oracle reports (fp32-against-float64 rounding cannot decide), and 0."""
    base = flow_case(name, True)
    L0 = oracle_flow_loss(make_oracle(base))
    assert L0 > 0
    o_off = make_oracle(base, flow=None)
    l_off, g_off = o_off.loss_grad()
    m = {}
    # kept
    for tag, thre in (("kept", 2 * L0), ("zero", 0.0)):
        prob = flow_case(name, True, thre=thre)
        o, a = make_oracle(prob), _engine(Engine, prob)
        mm, (lo, _), _ = _first_eval(o, a, 9999, tag + "_")
        m.update(mm)
        st = _flow_state(a)
        assert st[3] == 0 and st[4] == 0 and not a.flow_dropped and not o.flow_dropped, (tag, st)
        assert abs(st[2] - L0) / L0 < 1e-5, (st, L0)        # the reported fp32 flow loss: ~2e4 fp32 terms summed in a tree
        assert abs(lo - (l_off + prob["flow"]["weight"] * L0)) / lo < 1e-9           # the loss includes the term
    # dropped, and stays dropped
    prob = flow_case(name, True, thre=0.5 * L0)
    o, a = make_oracle(prob), _engine(Engine, prob)
    assert not a.flow_dropped                                            # nothing evaluated yet
    for visit in ("first", "again"):
        la, ga = a.loss_grad(9999)
        st = _flow_state(a)
        assert st[3] == 1 and st[4] == 1 and a.flow_dropped, (visit, st)
        m[f"loss_dropped_{visit}"] = abs(la - l_off) / l_off
        for k in g_off:
            m[f"grad_dropped_{visit}_{k}"] = rel_err(host(ga[k]).reshape(g_off[k].shape), g_off[k])
    lo, _ = o.loss_grad(9999)
    assert o.flow_dropped and lo == l_off
    m["loss_only_dropped"] = abs(float(a.loss().item()) - l_off) / l_off
    la, _ = a.loss_grad(0)                                               # before the start gate nothing is decided; the flag stays
    assert a.flow_dropped
    m["loss_dropped_gate"] = abs(la - l_off) / l_off
    _check(f"flow_drop_{name}", m)


# ------------------------------------------------------------------------------------------------- depth prior
@pytest.mark.parametrize("name", list(PRIOR_CASES))
def test_depth_prior_clamp_and_strides_vs_oracle(name, Engine):
    """P > 1024 with ragged (37 x 41) and exact-multiple-of-4 (40 x 52) tails, 10 % of the current and of the initial log-depths
    below the clamp, own dynamic weights; *_flow: the prior kernel and the flow kernels fill their workspaces in one launch
    sequence."""
    prob = prior_case(name)
    o, a = make_oracle(prob), _engine(Engine, prob)
    for eng in (o, a):
        eng.set_depth_prior(**prob["prior"])
    m, full_o, full_a = _first_eval(o, a, 9999, "prior_")
    m["loss_only_prior"] = abs(float(a.loss().item()) - full_o[0]) / abs(full_o[0])
    for eng in (o, a):
        eng.set_depth_prior(0.0)
    mm, base_o, base_a = _first_eval(o, a, 9999, "noprior_")
    m.update(mm)
    assert (full_o[0] - base_o[0]) / base_o[0] > 1e-4                     # the prior is visible in the loss
    m["iso_prior_value"] = abs((full_a[0] - base_a[0]) - (full_o[0] - base_o[0])) / (full_o[0] - base_o[0])
    _isolated(m, (full_o, full_a), (base_o, base_a), ["depth"], "prior_")
    diff = (host(full_a[1]["depth"]) - host(base_a[1]["depth"])).reshape(prob["clamped"].shape)
    assert np.all(diff[prob["clamped"]] == 0), "the clamp passes no gradient below eps: exact zeros"
    assert (diff[~prob["clamped"]] != 0).mean() > 0.99      # (a contribution can round away against the other terms)
    for k in ("pw_poses", "im_poses", "im_focals"):                      # the prior touches the depth maps only
        assert np.array_equal(host(full_a[1][k]), host(base_a[1][k])), k
    _check("prior_" + name, m)


# ------------------------------------------------------------------------------------------------- A3R_ALIGN_FLOW=v1
# (last in the file: if a child process ends abnormally, nothing else is started on the GPU after it)
_child_ended_badly = False

_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {tests!r}]
import numpy as np
from test_align_cases_cpu import flow_case
from align3r_amd.aligner import AlignEngine
prob = flow_case({name!r}, True)
a = AlignEngine(*prob["args"], **prob["kw"])
a.set_params(**prob["init"])
loss, g = a.loss_grad(9999)
np.savez({out!r}, loss=np.float64(loss), **{{k: v.detach().cpu().numpy() for k, v in g.items()}})
"""


def test_flow_v1_switch_at_vec_shape(Engine, tmp_path):
    """A3R_ALIGN_FLOW=v1 selects the scalar flow pass where the vec form would run (36 x 44).  The switch is read once per
    process, so the scalar run is one fresh child process, started after this process's own GPU work is done.  Against the oracle
    at the usual bounds, and against the vec form at 1e-6 of the tensor max ('to 7 digits')."""
    import torch
    name = "v36x44_deg_sf"
    assert os.environ.get("A3R_ALIGN_FLOW") != "v1"
    prob = flow_case(name, True)
    o, a = make_oracle(prob), _engine(Engine, prob)
    lo, go = o.loss_grad(9999)
    la, ga = a.loss_grad(9999)
    ga = {k: host(v).copy() for k, v in ga.items()}
    del a
    torch.cuda.synchronize()
    out = str(tmp_path / "v1.npz")
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), name=name, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, A3R_ALIGN_FLOW="v1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0 or not os.path.exists(out):
        global _child_ended_badly
        _child_ended_badly = True
        pytest.fail(f"the A3R_ALIGN_FLOW=v1 child process ended with status {r.returncode}:\n{r.stdout}", pytrace=False)
    c = np.load(out)
    m = dict(loss_v1_first=abs(float(c["loss"]) - lo) / abs(lo), v1_loss_vs_vec=abs(float(c["loss"]) - la) / abs(la))
    assert set(go) == set(ga) == set(c.files) - {"loss"}
    for k in go:
        m[f"grad_v1_{k}"] = rel_err(c[k].reshape(go[k].shape), go[k])
        m[f"v1_{k}_vs_vec"] = rel_err(c[k], ga[k])
    _check("flow_v1_switch_" + name, m)


# ------------------------------------------------------------------------------------------------- bitwise against the parent
def _flow_parent_generator():
    spec = importlib.util.spec_from_file_location("make_goldens_align_flow_parent",
                                                  os.path.join(REPO, "tests", "golden", "make_goldens_align_flow_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_PARENT = _flow_parent_generator()


@pytest.mark.parametrize("name", list(_PARENT.CASES))          # the case that needs a child process is the last one
def test_flow_pass_bitwise_parent(name, golden_dir, tmp_path):
    """Loss, every gradient tensor and the parameters after five steps with the flow term on are, byte for byte, those of the
    commit before the two flow kernels shared their per-pixel body: no tolerance.  The generator's own measure_case() runs the
    case, the v1_* one in a fresh child process under its own time limit (any non-zero status raises)."""
    global _child_ended_badly
    assert not _child_ended_badly, "not started: an earlier child process of this file ended abnormally"
    try:
        got = _PARENT.measure_case(name, str(tmp_path))
    except (RuntimeError, subprocess.TimeoutExpired):
        _child_ended_badly = True
        raise
    with np.load(os.path.join(golden_dir, "align_flow_parent.npz")) as z:
        want = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
    assert {"loss", "grad_depth", "grad_pw_poses", "grad_im_poses", "param_depth", "run_losses"} <= set(want)
    assert set(got) == set(want)
    differing = {}
    for k, w in want.items():
        g = np.asarray(got[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(np.frombuffer(g.tobytes(), np.uint8), np.frombuffer(w.tobytes(), np.uint8)):
            differing[k] = (int((g != w).sum()), float(np.abs(g.astype(np.float64) - w).max()))
    assert not differing, (name, "key: (elements that differ, largest difference)", differing)
