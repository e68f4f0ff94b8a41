"""CPU (no GPU): the host side of the point correspondences -- the mirror of find_reciprocal_matches / xy_grid against values recorded
from the reference (tests/golden/matches.npz, written by tests/golden/make_matches_golden.py), and the condition the GPU tests rest
on: on the tie-free clouds of tests/match_cases.py the float64 restatement brute() and the KD-tree route agree on every index."""
import os

import numpy as np
import pytest
import torch

import match_cases as mc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "matches.npz"))


@pytest.mark.parametrize("c, case", list(enumerate([("surface", 1000, 1337), ("uniform", 65, 257)])))
def test_host_route_equals_the_recorded_reference(gold, c, case):
    from align3r_amd.dust3r.utils.geometry import find_reciprocal_matches
    P1, P2 = mc.pair(*case)
    assert np.array_equal(P1, gold[f"P1_{c}"]) and np.array_equal(P2, gold[f"P2_{c}"])        # the fixture's inputs are the shared cases
    rec, nn2, count = find_reciprocal_matches(P1, P2)
    assert rec.dtype == bool and np.array_equal(rec, gold[f"reciprocal_{c}"])
    assert np.array_equal(nn2, gold[f"nn2_{c}"])
    assert int(count) == int(gold[f"count_{c}"]) == int(rec.sum())
    # CPU tensors with device=None take the host route as well
    rec_t, nn2_t, count_t = find_reciprocal_matches(torch.from_numpy(P1), torch.from_numpy(P2))
    assert np.array_equal(rec_t, rec) and np.array_equal(nn2_t, nn2) and count_t == count


@pytest.mark.parametrize("sizes", mc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", mc.TIE_FREE)
def test_brute_equals_the_host_route_on_tie_free_clouds(kind, sizes):
    from align3r_amd.dust3r.utils.geometry import find_reciprocal_matches
    ref = mc.brute_case(kind, *sizes)
    rec, nn2, count = find_reciprocal_matches(ref["P1"], ref["P2"])
    assert np.array_equal(nn2, ref["nn2_in_P1"])
    assert np.array_equal(rec, ref["reciprocal_in_P2"])
    assert int(count) == len(ref["pairs"])
    # the other direction: swap the roles
    _, nn1, _ = find_reciprocal_matches(ref["P2"], ref["P1"])
    assert np.array_equal(nn1, ref["nn1_in_P2"])


def test_brute_definition_on_ties_and_non_finite_points():
    """Guards the checker, not the library: brute() and reciprocal() of tests/match_cases.py on hand-worked ties, NaN / inf points and
    an empty data set -- the restatement every exact GPU comparison rests on."""
    D = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [-1, 0, 0]], np.float32)
    Q = np.array([[1, 0, 0], [0.5, 0, 0], [0, np.nan, 0], [-np.inf, 0, 0], [3e38, 0, 0]], np.float32)
    idx, d2 = mc.brute(Q, D)
    assert idx.tolist() == [1, 0, -1, -1, 0]                     # the lowest index of a tie; a non-finite query has no neighbour
    assert d2[0] == 0 and d2[1] == 0.25 and np.isposinf(d2[2]) and np.isposinf(d2[3])
    assert d2[4] == float(np.float32(3e38)) ** 2                 # far beyond the fp32 range of a square, finite in float64 (and a tie: 3e38 - 1 rounds to 3e38)
    idx, d2 = mc.brute(Q, D[:0])
    assert (idx == -1).all() and np.isposinf(d2).all()
    rec, pairs = mc.reciprocal(np.array([1, -1, 0]), np.array([2, 0]))
    assert rec.tolist() == [True, False, True] and pairs.tolist() == [[1, 0], [0, 2]]
    rec, pairs = mc.reciprocal(np.array([1, -1, 0]), np.array([1, 1]))
    assert rec.tolist() == [False, False, False] and pairs.shape == (0, 2)


def test_xy_grid_equals_the_recorded_reference(gold):
    from align3r_amd.dust3r.utils.geometry import xy_grid

    def same(got, want):
        got = got.numpy() if torch.is_tensor(got) else got
        return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)

    assert same(xy_grid(5, 3), gold["grid_np"])
    assert same(xy_grid(4, 2, origin=(3, 7)), gold["grid_origin"])
    assert same(xy_grid(3, 2, homogeneous=True), gold["grid_homog"])
    assert same(xy_grid(6, 4, device="cpu"), gold["grid_torch"])
    gx, gy = xy_grid(3, 2, device="cpu", unsqueeze=0, cat_dim=None)
    assert same(torch.stack([gx, gy]), gold["grid_planes"])
    g = xy_grid(5, 3)
    assert g[2, 4].tolist() == [4, 2]                            # out[j, i] = (i, j): x first


def test_lib_declares_the_match_symbols():
    from align3r_amd import _lib
    lib = _lib.load()
    for name in ("a3r_nn_chunks", "a3r_nn_workspace_bytes", "a3r_nn_search", "a3r_match_workspace_bytes", "a3r_reciprocal_matches"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # host-side sizing and refusals need no device
    assert lib.a3r_nn_chunks(1000, 1337, 7) == 7
    ch = lib.a3r_nn_chunks(1000, 1337, 0)
    assert 1 <= ch <= 64
    assert lib.a3r_nn_workspace_bytes(1000, 1337, 3) >= 1000 * 3 * 12
    assert lib.a3r_nn_workspace_bytes(0, 1337, 0) == 0 and lib.a3r_nn_workspace_bytes(1000, 0, 0) == 0
    assert lib.a3r_match_workspace_bytes(1000, 1337, 3) >= lib.a3r_nn_workspace_bytes(1337, 1000, 3) + 1000 * 4
    assert lib.a3r_nn_search(None, 1 << 31, None, 1, 0, None, 0, None, None, None) != 0
    assert b"2^31" in lib.a3r_last_error()
    assert lib.a3r_nn_search(None, 4, None, 4, 0, None, 0, None, None, None) != 0
    assert b"null" in lib.a3r_last_error()
    assert lib.a3r_nn_search(None, 4, None, 4, -1, None, 0, None, None, None) != 0
    assert b"chunks" in lib.a3r_last_error()


@pytest.mark.parametrize("mode", ["--hierarchical", "--flow-hierarchical"])
def test_run_clip_refuses_matches_with_the_hierarchical_modes(mode, capsys):
    from align3r_amd.tool.run_clip import parse
    base = ["--images", "frames", "--weights", "w.pth", "--out", "out", "--matches", "m"]
    with pytest.raises(SystemExit):
        parse(base + [mode])
    assert "--matches cannot be combined" in capsys.readouterr().err
    assert parse(base).matches == "m" and parse(base[:6]).matches is None
    assert parse(base + ["--flow"]).matches == "m"
