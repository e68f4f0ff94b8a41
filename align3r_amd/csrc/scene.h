// What the scene-out path (scene.hip) reads of an aligner handle (align.hip owns the handle and its transform builder).
#pragma once
#include "common.h"

namespace a3r {

struct SceneView {
    int N, P;
    const float* depth;     // [N, P] log-depth (plain form) or scale map (mono form): the handle's CURRENT parameters
    const float* mono;      // [N, P] mono depth maps, null in the plain form
    const float* img_xf;    // [N, 16] = [R | t] rows, then f, ppx, ppy, shift: written by build_transforms (align.hip)
    const int *imw, *imarea;
};

// Rebuilds the handle's per-image transforms from its current parameters on `st` (the prep kernel of a3r_align_pose_matrices and
// the iteration: one decoding of poses, focals -- shared_focal included --, principal points and shifts) and points `v` at them.
// Valid for fused and edge-shard handles: a shard holds a full replica of every buffer named here.
int align_scene_view(a3r_align_t a, hipStream_t st, SceneView* v, const char* who);

}  // namespace a3r
