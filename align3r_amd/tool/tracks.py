"""Host-side helpers of the tracker (ops.track_points, csrc/track.hip): the plan that turns a list of frames into steps over the
scene's edges, the seed grid of run_clip --tracks, and the npz files tracks are kept in."""
from __future__ import annotations

import numpy as np

TRACK_KEYS = ("xy", "xyz", "pix", "state", "frames")


def plan_steps(edges, frames):
    """The steps [S,4] int32, rows (frame_from, frame_to, edge, reversed), that lead through `frames` in the order given (any order:
    backwards in time is a reversed list) over the graph `edges` = [(i, j), ...]: for every consecutive pair (a, b) the first edge
    (a, b) of the list, taken forwards (reversed = 0: its flow_ij leads from a to b); failing that the first edge (b, a), taken
    backwards (reversed = 1: its flow_ji does); a ValueError naming the pair when the graph holds neither."""
    first = {}
    for e, (i, j) in enumerate(edges):
        first.setdefault((int(i), int(j)), e)
    frames = [int(f) for f in frames]
    steps = np.zeros((max(len(frames) - 1, 0), 4), np.int32)
    for s, (a, b) in enumerate(zip(frames[:-1], frames[1:])):
        if (a, b) in first:
            steps[s] = (a, b, first[(a, b)], 0)
        elif (b, a) in first:
            steps[s] = (a, b, first[(b, a)], 1)
        else:
            raise ValueError(f"plan_steps: the graph has no edge between frames {a} and {b} (step {s} of the frame list)")
    return steps


def grid_seeds(shape, stride=8):
    """Seeds [M,2] float32 (x, y) on the pixels (stride * k, stride * l) of an image of shape (H, W), row-major."""
    H, W = int(shape[0]), int(shape[1])
    if stride < 1:
        raise ValueError(f"grid_seeds: stride = {stride} must be at least 1")
    ys, xs = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    return np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32)


def write_tracks_npz(path, tracks):
    """The dict of scene.get_tracks (xy, xyz, pix, state, frames; device tensors or arrays) as an uncompressed npz of host arrays
    with their own types; returns the path."""
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    missing = [k for k in TRACK_KEYS if k not in tracks]
    if missing:
        raise ValueError(f"write_tracks_npz: the tracks lack {missing}")
    np.savez(path, **{k: host(tracks[k]) for k in TRACK_KEYS})
    return path


def read_tracks_npz(path):
    """What write_tracks_npz wrote: a dict of numpy arrays, `frames` as a list of ints."""
    with np.load(path) as z:
        out = {k: z[k] for k in TRACK_KEYS}
    out["frames"] = [int(f) for f in out["frames"]]
    return out
