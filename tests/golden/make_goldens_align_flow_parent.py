"""Writes align_flow_parent.npz: what the aligner computes with the ego-flow term active, as the library selected by A3R_LIB
(default: the tree's own) computes it on the GPU.  The committed file pins the results of the commit BEFORE the two forms of the
ego-flow pass (align_flow_kernel, align_flow_vec_kernel) were put onto one per-pixel body:

    A3R_LIB=/path/to/that/commit/liba3r.so python tests/golden/make_goldens_align_flow_parent.py

Per case: loss_grad(9999) -- the loss and every gradient tensor, the [N,P] depth gradient included -- then five run() steps behind
the flow term's start gate (their losses, and every trained parameter after them), all stored in full.  The cases are the smallest
shapes at which each form can go wrong (tests/align_cases.py):

  vec_36x44_deg_sf      vector form on the degree-class graph: images with 17 / 16 / 9 / 8 / 7 / 2 / 1 incident edge sides, so the
                        batches of EB = 8 roll over and the two-sides-per-trip loop ends on an odd tail;
  vec_40x52_deg_pp      vector form, P = 2080 (P % 1024 != 0, P % 4 == 0): ragged last chunk;
  scalar_7x9_win6       scalar form (P % 4 == 3), P = 63: fewer pixels than a wave;
  scalar_25x41_win6     scalar form (P % 4 == 1), P = 1025: one pixel in the second chunk;
  v1_36x44_deg_sf       the first problem on the scalar form, selected by A3R_ALIGN_FLOW=v1.

Every problem has 30 % set dynamic-mask bytes, one fully dynamic image and pxl_thre = 1.5, which excludes pixels.

The A3R_ALIGN_FLOW switch is read once per process, so a v1_* case runs in a fresh child process: this file with `--one NAME OUT`
under the child's own time limit.  tests/test_gpu_align_paths.py imports CASES and measure_case() from here, so the test and the
golden cannot drift apart."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _dir in (TESTS, os.path.dirname(TESTS)):
    if _dir not in sys.path:
        sys.path.insert(0, _dir)

CHILD_TIMEOUT = 300      # seconds: one process start, one library load, one problem of at most 15 frames of 1584 pixels


def _win6(H, W):
    import align_cases as ac
    return ac.flow_problem(6, H, W, ac.window_graph(6), 7, dyn_frac=0.3, pxl_thre=1.5, thre=1e9, shared_focal=False, train_pp=False,
                           start_epoch=0.1)


def _named(name):
    from test_align_cases_cpu import flow_case
    return flow_case(name, True)


# case -> (problem builder, value of A3R_ALIGN_FLOW the case needs or None)
CASES = {
    "vec_36x44_deg_sf": (lambda: _named("v36x44_deg_sf"), None),
    "vec_40x52_deg_pp": (lambda: _named("v40x52_deg_pp"), None),
    "scalar_7x9_win6": (lambda: _win6(7, 9), None),
    "scalar_25x41_win6": (lambda: _win6(25, 41), None),
    "v1_36x44_deg_sf": (lambda: _named("v36x44_deg_sf"), "v1"),
}


def _measure_here(name):
    from align3r_amd.aligner import AlignEngine
    build, switch = CASES[name]
    assert os.environ.get("A3R_ALIGN_FLOW") == switch, (name, os.environ.get("A3R_ALIGN_FLOW"))
    prob = build()
    a = AlignEngine(*prob["args"], **prob["kw"])
    a.set_params(**prob["init"])
    loss, g = a.loss_grad(9999)
    out = {"loss": np.float64(loss)}
    out.update({"grad_" + k: v.detach().cpu().numpy() for k, v in g.items()})
    out["run_losses"] = a.run(5, 0.01, "linear", first_iter=5, total_iters=50)        # the flow term starts at iteration 5
    out.update({"param_" + k: a.params[k].detach().cpu().numpy() for k in a.trainable()})
    assert not a.flow_dropped
    return out


def measure_case(name, scratch_dir):
    """{key: array} of one case from the loaded library; a case that needs A3R_ALIGN_FLOW set runs in a fresh child process that
    leaves its arrays in scratch_dir."""
    switch = CASES[name][1]
    if os.environ.get("A3R_ALIGN_FLOW") == switch:
        return _measure_here(name)
    out = os.path.join(scratch_dir, name + ".npz")
    env = dict(os.environ)
    env.pop("A3R_ALIGN_FLOW", None)
    if switch is not None:
        env["A3R_ALIGN_FLOW"] = switch
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"the child process of case {name} ended with status {r.returncode}:\n{r.stdout}")
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        np.savez(sys.argv[3], **_measure_here(sys.argv[2]))
        sys.exit(0)
    import tempfile
    flat = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(CASES, key=lambda n: CASES[n][1] is not None):       # the child processes last
            for k, v in measure_case(name, tmp).items():
                assert np.all(np.isfinite(v)), (name, k)
                flat[f"{name}/{k}"] = v
    np.savez_compressed(os.path.join(HERE, "align_flow_parent.npz"), **flat)
    print(f"wrote {len(flat)} arrays of {len(CASES)} cases, {sum(v.nbytes for v in flat.values())} bytes before compression")
