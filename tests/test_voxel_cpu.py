"""CPU (no GPU): the voxel-grid restatement of tests/voxel_cases.py against a slow point-by-point checker, the conditions that keep
the shared cases from going vacuous, the properties of the mean, run_clip's new flags and the refusals of ops.voxel_downsample that
need no device."""
import numpy as np
import pytest
import torch

import voxel_cases as vc

SMALL = [c for c in vc.CASES if c[1] <= 1030]


def _same(a, b):
    assert a["dropped"] == b["dropped"]
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["count"], b["count"])
    assert a["xyz"].shape == b["xyz"].shape and a["xyz"].tobytes() == b["xyz"].tobytes()
    assert (a["rgb"] is None) == (b["rgb"] is None) and (a["rgb"] is None or np.array_equal(a["rgb"], b["rgb"]))


@pytest.mark.parametrize("case", SMALL, ids=vc.case_id)
def test_restatement_equals_the_point_by_point_checker(case):
    ref = vc.ref_case(case)
    xyz, voxel, priority, rgb = ref["xyz"], ref["voxel"], ref["priority"], ref["rgb"]
    for reduce in ("best", "mean"):
        _same(ref[reduce], vc.voxel_naive(xyz, voxel, priority, rgb, reduce, 1))
        _same(vc.voxel_ref(xyz, voxel, None, None, reduce, 2), vc.voxel_naive(xyz, voxel, None, None, reduce, 2))


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_the_cases_are_what_they_claim(case):
    kind, M, k = case
    ref = vc.ref_case(case)
    best = ref["best"]
    V = len(best["index"])
    assert best["xyz"].dtype == np.float32 and best["index"].dtype == np.int32 and best["count"].dtype == np.int32
    assert int(best["count"].sum()) + best["dropped"] == M and (np.diff(best["index"]) > 0).all()
    if kind in ("surface", "ties", "nan_prio", "runs") and M >= 65:
        print(f"{vc.case_id(case)}: V/M = {V / M:.3f}, largest count {best['count'].max()}")
        assert 0.05 <= V / M <= 0.5 and best["count"].max() >= 5
    if kind == "surface" and M >= 65:
        assert np.log2(ref["voxel"]) % 1 != 0                       # no power of two: the quotient rounds (M = 64 gives 0.5 and 1)
    if kind == "runs":
        inside, key, _, _ = vc.voxel_cells(ref["xyz"], ref["voxel"])
        same = inside[1:] & inside[:-1] & (key[1:] == key[:-1])
        assert best["dropped"] == max(M // 50, 1) and same.mean() >= 0.5      # most rows continue their neighbour's run
        assert M < 8193 or (same[63::64].any() and same[255::256].any())       # runs cross wave and workgroup borders
    if kind == "pile":
        assert V == 1 and best["count"][0] == M and best["index"][0] == 0 and best["dropped"] == 0
    if kind == "pile_prio":
        assert V == 1 and best["count"][0] == M and best["index"][0] == M - 1       # the last workgroup of the insert pass
    if kind == "spread":
        assert V == M and (best["count"] == 1).all() and np.array_equal(best["index"], np.arange(M))
    if kind == "edges":
        assert best["index"].tolist() == vc.EDGE_WINNERS and (best["count"] == 1).all() and best["dropped"] == vc.EDGE_DROPPED
        assert np.array_equal(vc.voxel_ref(ref["xyz"], ref["voxel"])["index"], vc.EDGE_WINNERS)
    if kind == "edges_rep":
        assert V == len(vc.EDGE_WINNERS) and best["dropped"] == 3 * vc.EDGE_DROPPED and sorted(best["count"].tolist()) == [3, 3, 3, 5, 5]
    if kind == "ties" and M >= 65:
        # voxels whose highest priority occurs more than once: the lowest row must win there
        inside, key, _, _ = vc.voxel_cells(ref["xyz"], ref["voxel"])
        tied = 0
        for i in best["index"][:200]:
            rows = np.flatnonzero(inside & (key == key[i]))
            top = rows[ref["priority"][rows] == ref["priority"][rows].max()]
            assert top[0] == i
            tied += len(top) > 1
        assert tied >= 5
    if kind == "nan_prio":
        pr = ref["priority"]
        assert np.isnan(pr[best["index"]]).any() and not np.isnan(pr[best["index"]]).all()
        inside, key, _, _ = vc.voxel_cells(ref["xyz"], ref["voxel"])
        mixed = [i for i in best["index"][:400] if np.isnan(pr[key == key[i]]).any() and not np.isnan(pr[key == key[i]]).all()]
        assert len(mixed) >= 1 or M < 200
        assert not np.isnan(pr[mixed]).any()                         # a NaN never wins against a number
    if kind == "empty":
        assert V == 0 and best["xyz"].shape == (0, 3)


@pytest.mark.parametrize("case", [c for c in vc.CASES if c[0] not in ("empty",)], ids=vc.case_id)
def test_a_mean_lies_inside_its_voxel_and_between_its_colours(case):
    ref = vc.ref_case(case)
    mean, voxel = ref["mean"], np.float64(ref["voxel"])
    inside, key, r, q = vc.voxel_cells(ref["xyz"], voxel)
    assert np.array_equal(mean["index"], ref["best"]["index"]) and np.array_equal(mean["count"], ref["best"]["count"])
    # The box to fp32 rounding.  An offset r - q lies in [0, 1) but may ROUND to 1 (x = -1e-30: r - q = 1 - 4e-30), so t <= 2^24 and
    # the centred mean (S + n / 2) / (n 2^24) lies in [2^-25, 1 + 2^-25]: the box widened upwards by half a fixed-point step,
    # voxel * 2^-25, which is a quarter of an fp32 ulp of the voxel edge.  The products and the fp32 rounding are monotone.
    lo, hi = (q[mean["index"]] * voxel).astype(np.float32), ((q[mean["index"]] + (1 + 2.0 ** -25)) * voxel).astype(np.float32)
    assert (mean["xyz"] >= lo).all() and (mean["xyz"] <= hi).all()
    rgb = ref["rgb"]
    for v, i in enumerate(mean["index"][:300]):
        rows = np.flatnonzero(inside & (key == key[i]))
        assert (mean["rgb"][v] >= rgb[rows].min(0)).all() and (mean["rgb"][v] <= rgb[rows].max(0)).all()
        pts = ref["xyz"][rows].astype(np.float64)
        exact = pts.mean(0)
        assert np.abs(mean["xyz"][v] - exact).max() <= voxel * 2.0 ** -23 + 2 * np.spacing(np.abs(pts).max().astype(np.float32))


@pytest.mark.parametrize("case", [c for c in vc.CASES if c[0] == "spread"], ids=vc.case_id)
def test_best_equals_mean_on_one_point_per_voxel(case):
    ref = vc.ref_case(case)
    a, b = ref["best"]["xyz"].astype(np.float64), ref["mean"]["xyz"].astype(np.float64)
    bound = ref["voxel"] * 2.0 ** -24 + np.spacing(np.abs(ref["best"]["xyz"]))          # the fixed-point step plus one fp32 ulp
    assert (np.abs(a - b) <= bound).all()
    assert np.array_equal(ref["best"]["rgb"], ref["mean"]["rgb"])


def test_run_clip_parses_the_voxel_flags(capsys):
    from align3r_amd.tool.run_clip import parse
    base = ["--images", "frames", "--weights", "w.pth", "--out", "out"]
    a = parse(base + ["--pointcloud", "s.ply"])
    assert a.pointcloud_voxel is None and a.pointcloud_reduce == "best" and a.pointcloud_min_count == 1
    a = parse(base + ["--pointcloud", "s.ply", "--pointcloud-voxel", "0.05", "--pointcloud-reduce", "mean", "--pointcloud-min-count", "2"])
    assert (a.pointcloud_voxel, a.pointcloud_reduce, a.pointcloud_min_count) == (0.05, "mean", 2)
    for mode in ("--hierarchical", "--flow-hierarchical"):
        assert parse(base + ["--pointcloud", "s.ply", "--pointcloud-voxel", "0.1", mode]).pointcloud_voxel == 0.1
    for bad, msg in ((["--pointcloud-voxel", "0.1"], "belongs to --pointcloud"),
                     (["--pointcloud", "s.ply", "--pointcloud-reduce", "mean"], "belongs to --pointcloud-voxel"),
                     (["--pointcloud", "s.ply", "--pointcloud-min-count", "2"], "belongs to --pointcloud-voxel"),
                     (["--pointcloud", "s.ply", "--pointcloud-voxel", "0"], "finite edge length"),
                     (["--pointcloud", "s.ply", "--pointcloud-voxel", "nan"], "finite edge length"),
                     (["--pointcloud", "s.ply", "--pointcloud-voxel", "0.1", "--pointcloud-min-count", "0"], "at least 1"),
                     (["--pointcloud", "s.ply", "--pointcloud-voxel", "0.1", "--pointcloud-reduce", "median"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse(base + bad)
        assert msg in capsys.readouterr().err


def test_voxel_downsample_refuses_bad_arguments_before_the_library(monkeypatch):
    from align3r_amd import _lib, ops

    def untouched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", untouched)
    xyz = torch.zeros((8, 3), dtype=torch.float32)
    ok = dict(voxel=0.5)
    with pytest.raises(ValueError, match="on the device"):
        ops.voxel_downsample(xyz, **ok)                                                  # a host tensor
    with pytest.raises(ValueError, match="torch tensor"):
        ops.voxel_downsample(xyz.numpy(), **ok)
    with pytest.raises(ValueError, match="xyz must be torch.float32"):
        ops.voxel_downsample(xyz.double(), **ok)
    for bad in (torch.zeros(8), torch.zeros((8, 4)), torch.zeros((2, 4, 3)), torch.zeros(())):
        with pytest.raises(ValueError, match="xyz has shape"):
            ops.voxel_downsample(bad, **ok)
    with pytest.raises(ValueError, match="xyz must be contiguous"):
        ops.voxel_downsample(torch.zeros((3, 8)).t(), **ok)
    with pytest.raises(ValueError, match="priority must be torch.float32"):
        ops.voxel_downsample(xyz, priority=torch.zeros(8, dtype=torch.float64), **ok)
    with pytest.raises(ValueError, match="priority has shape"):
        ops.voxel_downsample(xyz, priority=torch.zeros(7), **ok)
    with pytest.raises(ValueError, match="priority must be contiguous"):
        ops.voxel_downsample(xyz, priority=torch.zeros(16)[::2], **ok)
    with pytest.raises(ValueError, match="rgb must be torch.uint8"):
        ops.voxel_downsample(xyz, rgb=torch.zeros((8, 3)), **ok)
    with pytest.raises(ValueError, match="rgb has shape"):
        ops.voxel_downsample(xyz, rgb=torch.zeros((8, 4), dtype=torch.uint8), **ok)
    with pytest.raises(ValueError, match="rgb must be contiguous"):
        ops.voxel_downsample(xyz, rgb=torch.zeros((3, 8), dtype=torch.uint8).t(), **ok)
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and positive"):
            ops.voxel_downsample(xyz, voxel)
    for min_count in (0, -3, 1.5):
        with pytest.raises(ValueError, match="min_count"):
            ops.voxel_downsample(xyz, 0.5, min_count=min_count)
    with pytest.raises(ValueError, match="neither 'best' nor 'mean'"):
        ops.voxel_downsample(xyz, 0.5, reduce="median")
    for slots in (3, 12, -8, 2.5):
        with pytest.raises(ValueError, match="power of two"):
            ops.voxel_downsample(xyz, 0.5, slots=slots)
    for slots in (4, 8, 1 << 32):
        with pytest.raises(ValueError, match="must exceed the 8 points"):
            ops.voxel_downsample(xyz, 0.5, slots=slots)
    assert [ops.voxel_default_slots(M) for M in (0, 1, 2, 3, 8193, (1 << 30) + 1, (1 << 31) - 1)] == [1, 2, 4, 8, 32768, 1 << 31, 1 << 31]
