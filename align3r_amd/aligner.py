"""AlignEngine: owner of one a3r_align handle (fused loss + gradient + Adam kernels) on one GPU.

Holds the stacked observation buffers of PointCloudOptimizer (dust3r/cloud_opt/optimizer.py:55-71),
the parameters and the Adam moments as device tensors and drives a3r_align_step.  The loop, the
schedules and the parameter names follow dust3r/cloud_opt/base_opt.py:424-464.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import AlignDesc, AlignFlowDesc, check, ptr, stream_ptr
from .obs16 import check_obs_dtype


def cosine_schedule(t, lr_start, lr_end):   # commons.py:123-125
    assert 0 <= t <= 1
    return lr_end + (lr_start - lr_end) * (1 + np.cos(t * np.pi)) / 2


def linear_schedule(t, lr_start, lr_end):   # commons.py:128-130
    assert 0 <= t <= 1
    return lr_start + (lr_end - lr_start) * t


def cycled_linear_schedule(t, lr_start, lr_end, num_cycles=2):   # cloud_opt_flow/commons.py:97-103
    assert 0 <= t <= 1
    cycle_t = t * num_cycles
    cycle_t = cycle_t - int(cycle_t)
    if t == 1:
        cycle_t = 1
    return linear_schedule(cycle_t, lr_start, lr_end)


def schedule_lr(schedule, t, lr, lr_min):
    """Learning rate of global_alignment_iter (cloud_opt/base_opt.py:451-457, cloud_opt_flow/base_opt.py:554-566)."""
    if schedule == "cosine":
        return cosine_schedule(t, lr, lr_min)
    if schedule == "linear":
        return linear_schedule(t, lr, lr_min)
    if schedule.startswith("cycle"):
        try:
            n = int(schedule[5:])
        except ValueError:
            n = 2
        return cycled_linear_schedule(t, lr, lr_min, num_cycles=n)
    raise ValueError(f"bad lr schedule={schedule!r}")


_PARAM_KEYS = ("pw_poses", "pw_adaptors", "depth", "shifts", "im_poses", "im_focals", "im_pp")


class _AlignEngineBase:
    """What the fused and the edge-sharded engine share: the graph, the uploaded observations, the flags and the bookkeeping of
    their handle states.  A state is anything with handle / params / adam / workspace / loss_history: the fused engine is its own
    single state, the sharded one has a _ShardReplica per shard (`_states`)."""

    def __init__(self, ei, ej, pred_i, pred_j, w_i, w_j, imshapes, mono, base_scale, pw_break, focal_break, norm_pw_scale, dist,
                 train_poses, train_focals, train_pp, train_adaptors, device, loss_capacity, shared_focal=False, obs_dtype="fp32",
                 pack_budget_bytes=1 << 30):
        self.obs_dtype = check_obs_dtype(obs_dtype)
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs a HIP device (there is no CPU fallback)")
        f32 = self._f32
        self.ei = np.ascontiguousarray(ei, dtype=np.int32)
        self.ej = np.ascontiguousarray(ej, dtype=np.int32)
        E, N = len(self.ei), len(imshapes)
        rows, pred_i, pred_j, w_i, w_j = self._select_rows(E, pred_i, pred_j, w_i, w_j)
        if self.obs_dtype == "fp32":
            self.w_i, self.w_j = f32(w_i).reshape(rows, -1), f32(w_j).reshape(rows, -1)
            P = self.w_i.shape[1]
            self.pred_i, self.pred_j = f32(pred_i).reshape(rows, P, 3), f32(pred_j).reshape(rows, P, 3)
        else:
            # packed fp16 records + one exponent per edge side (obs16.py); no fp32 copy of the observations is kept here
            P = torch.as_tensor(w_i).reshape(rows, -1).shape[1]
            self.pred_i = self.pred_j = self.w_i = self.w_j = None
            self.obs_i, self.exp_i = self._pack(pred_i, w_i, rows, P, pack_budget_bytes)
            self.obs_j, self.exp_j = self._pack(pred_j, w_j, rows, P, pack_budget_bytes)
        self.E, self.N, self.P = E, N, P
        self.imshapes = [tuple(int(v) for v in s) for s in imshapes]
        self.imw = np.asarray([w for h, w in self.imshapes], dtype=np.int32)
        self.imarea = np.asarray([h * w for h, w in self.imshapes], dtype=np.int32)
        self.pp0 = f32([(w / 2, h / 2) for h, w in self.imshapes])
        self.use_mono = mono is not None
        self.mono = f32(mono).reshape(N, P) if self.use_mono else None
        self.flags = dict(norm_pw_scale=bool(norm_pw_scale), dist_l2=(dist == "l2"), train_poses=bool(train_poses),
                          train_focals=bool(train_focals), train_pp=bool(train_pp), train_adaptors=bool(train_adaptors))
        self.base_scale, self.pw_break, self.focal_break = base_scale, pw_break, focal_break
        self.shared_focal = bool(shared_focal)
        self.flow = None
        self.prior = None             # AlignEngine.set_depth_prior(): dict(weight, init [N,P], dyn [N,P] uint8 | None, workspace)
        self.loss_capacity = loss_capacity
        self.total_area_i = float(sum(int(self.imarea[i]) for i in self.ei))       # the WHOLE graph's (optimizer.py:70-71)
        self.total_area_j = float(sum(int(self.imarea[j]) for j in self.ej))

    def _select_rows(self, E, pred_i, pred_j, w_i, w_j):
        """(number of observation rows to hold, the observations to upload): one row per edge of the graph here."""
        return E, pred_i, pred_j, w_i, w_j

    def _f32(self, a):
        return torch.as_tensor(a, dtype=torch.float32).to(self.device).contiguous()

    def _pack(self, pred, w, rows, P, budget_bytes):
        """One side's observations as (records [rows, P, 4] float16, exponents [rows] int32) on the device: uploaded and packed in
        row chunks of at most budget_bytes of fp32 rows (16 P bytes each), so the whole fp32 stack is never resident."""
        dev = self.device
        pred, w = torch.as_tensor(pred).reshape(rows, P, 3), torch.as_tensor(w).reshape(rows, P)
        obs = torch.empty(rows, P, 4, dtype=torch.float16, device=dev)
        exps = torch.empty(rows, dtype=torch.int32, device=dev)
        step = max(1, int(budget_bytes) // (16 * P))
        with torch.cuda.device(dev):
            for r0 in range(0, rows, step):
                r1 = min(rows, r0 + step)
                p32, w32 = (t[r0:r1].to(dev, torch.float32).contiguous() for t in (pred, w))
                check(self.lib.a3r_align_pack_obs(ptr(p32), ptr(w32), r1 - r0, P, ptr(obs[r0:r1]), ptr(exps[r0:r1]), stream_ptr()),
                      "a3r_align_pack_obs")
        return obs, exps

    @property
    def observation_bytes(self):
        """Device bytes of the observations held here: 32 per edge-pixel in fp32, 16 (+ 8 per edge for the exponents) packed."""
        held = (self.pred_i, self.pred_j, self.w_i, self.w_j) if self.obs_dtype == "fp32" else (self.obs_i, self.obs_j, self.exp_i, self.exp_j)
        return sum(t.numel() * t.element_size() for t in held)

    def decoded_observations(self):
        """(pred_i', pred_j', w_i', w_j') as fp32 tensors: the observations the loss is evaluated on.  With fp16 storage
        pred' = float(h) 2^-k and w' = float(h_w) (exact in fp32, obs16.py); with fp32 storage the tensors held here."""
        if self.obs_dtype == "fp32":
            return self.pred_i, self.pred_j, self.w_i, self.w_j
        # 2^-k from its bit pattern (|k| <= 100: a normal number); the product with an fp16 value is exact
        scale = lambda exps: (127 - exps).bitwise_left_shift(23).view(torch.float32)[:, None, None]
        dec = lambda obs, exps: (obs[..., :3].float() * scale(exps), obs[..., 3].float().contiguous())
        (pi, wi), (pj, wj) = dec(self.obs_i, self.exp_i), dec(self.obs_j, self.exp_j)
        return pi, pj, wi, wj

    def _alloc_state(self, st, workspace_bytes):
        """Zeroed parameters, Adam moments and loss history plus the workspace of one handle, as attributes of `st`."""
        E, N, P = self.E, self.N, self.P
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        st.params = dict(pw_poses=z(E, 8), pw_adaptors=z(E, 2), depth=z(N, P), shifts=z(N), im_poses=z(N, 7),
                         im_focals=z(1 if self.shared_focal else N), im_pp=z(N, 2))
        st.adam = dict(pw_poses=z(2, E, 8), depth=z(2, N, P), small=z(2, N, 16), pw_adaptors=z(2, E, 2))
        st.loss_history = z(self.loss_capacity)
        st.workspace = torch.empty(int(workspace_bytes), dtype=torch.uint8, device=self.device)
        st.handle = None

    def _fill_desc(self, params, adam, workspace, loss_history, row_slice):
        """The a3r_align_desc of one handle; row_slice selects its rows of the observation tensors held here (views)."""
        d = AlignDesc()
        d.E, d.N, d.P = self.E, self.N, self.P
        d.use_mono = int(self.use_mono)
        for k in ("norm_pw_scale", "dist_l2", "train_poses", "train_focals", "train_pp", "train_adaptors"):
            setattr(d, k, int(self.flags[k]))
        d.base_scale, d.pw_break, d.focal_break = self.base_scale, self.pw_break, self.focal_break
        d.total_area_i, d.total_area_j = self.total_area_i, self.total_area_j
        d.ei_host, d.ej_host = self.ei.ctypes.data, self.ej.ctypes.data
        d.imw_host, d.imarea_host = self.imw.ctypes.data, self.imarea.ctypes.data
        if self.obs_dtype == "fp32":
            d.pred_i, d.pred_j = self.pred_i[row_slice].data_ptr(), self.pred_j[row_slice].data_ptr()
            d.w_i, d.w_j = self.w_i[row_slice].data_ptr(), self.w_j[row_slice].data_ptr()
        else:
            d.obs_format = 1
            d.obs_i, d.obs_j = self.obs_i[row_slice].data_ptr(), self.obs_j[row_slice].data_ptr()
            d.obs_exp_i, d.obs_exp_j = self.exp_i[row_slice].data_ptr(), self.exp_j[row_slice].data_ptr()
        d.mono = self.mono.data_ptr() if self.use_mono else None
        d.pp0 = self.pp0.data_ptr()
        for k in _PARAM_KEYS:
            setattr(d, k, params[k].data_ptr())
        d.adam_pw_poses, d.adam_depth, d.adam_small, d.adam_pw_adaptors = (adam[k].data_ptr() for k in ("pw_poses", "depth", "small", "pw_adaptors"))
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel()
        d.loss_history, d.loss_capacity = loss_history.data_ptr(), self.loss_capacity
        return d

    def _destroy(self, st):
        if st.handle:
            h_old, st.handle = st.handle, None              # never leave a destroyed handle behind if a re-creation fails
            self.lib.a3r_align_destroy(h_old)

    def __del__(self):
        try:
            for st in self._states:
                self._destroy(st)
        except Exception:
            pass

    # ------------------------------------------------------------------ state
    def set_params(self, pw_poses=None, depth=None, im_poses=None, im_focals=None, shifts=None, im_pp=None,
                   pw_adaptors=None, reset_optimizer=True):
        for k, v in dict(pw_poses=pw_poses, depth=depth, im_poses=im_poses, im_focals=im_focals, shifts=shifts, im_pp=im_pp,
                         pw_adaptors=pw_adaptors).items():
            if v is not None:
                t = torch.as_tensor(v, dtype=torch.float32).to(self.device)
                if k == "im_focals" and self.shared_focal:
                    t = t.reshape(-1)[:1]          # one focal shared by all images (optimizer.py:56-58)
                for st in self._states:
                    st.params[k].copy_(t.reshape(st.params[k].shape))
        if reset_optimizer:
            for st in self._states:
                for t in st.adam.values():
                    t.zero_()
            self._create()     # step counter restarts with fresh Adam moments
        else:
            for st in self._states:
                check(self.lib.a3r_align_invalidate(st.handle))

    def set_trainable(self, **flags):
        """preset_pose / preset_focal / preset_principal_point semantics (optimizer.py:76-113)."""
        self.flags.update(flags)
        self._create()

    def trainable(self):
        t = ["pw_poses", "depth"]
        if self.flags["train_adaptors"]:
            t.append("pw_adaptors")
        if self.use_mono:
            t.append("shifts")
        if self.flags["train_poses"]:
            t.append("im_poses")
        if self.flags["train_focals"]:
            t.append("im_focals")
        if self.flags["train_pp"]:
            t.append("im_pp")
        return t

    @property
    def steps_done(self):
        return int(self.lib.a3r_align_steps_done(self._states[0].handle))

    def _lrs(self, niter, lr, schedule, lr_min, first_iter, total_iters):
        """The learning rates of run(): the schedule is evaluated here (float64, as the reference does), the iterations are
        enqueued by one native loop."""
        total = total_iters or niter
        return np.asarray([schedule_lr(schedule, it / total, lr, lr_min) for it in range(first_iter, first_iter + niter)], dtype=np.float32)

    def _grad_dict(self, g_pw, g_ad, g_depth, g_small):
        """Gradients of the trained parameters by name, from the [N,16] rows of the per-image parameters."""
        g_f = g_small[:, 7].sum().reshape(1) if self.shared_focal else g_small[:, 7]
        g = dict(pw_poses=g_pw, pw_adaptors=g_ad, depth=g_depth, im_poses=g_small[:, 0:7], im_focals=g_f, im_pp=g_small[:, 8:10],
                 shifts=g_small[:, 10])
        return {k: g[k] for k in self.trainable()}

    def pose_matrices(self):
        eM = torch.empty(self.E, 3, 4, device=self.device)
        iR = torch.empty(self.N, 3, 4, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_pose_matrices(self._states[0].handle, ptr(eM), ptr(iR), stream_ptr()), "a3r_align_pose_matrices")
        return eM, iR

    # ------------------------------------------------------------------ scene out (csrc/scene.hip)
    def points(self):
        """World points [N,P,3] of the current state (depth_to_pts3d of the reference, optimizer.py:244-251); zeros at the padding
        pixels of a mixed-shape scene.  The sharded engine reads replica 0 (the replicas are identical)."""
        out = torch.empty(self.N, self.P, 3, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_scene_points(self._states[0].handle, ptr(out), stream_ptr()), "a3r_align_scene_points")
        return out

    def _scene_inputs(self, conf, dyn, rgb):
        N, P, dev = self.N, self.P, self.device
        conf = torch.as_tensor(conf).to(dev, torch.float32).reshape(N, P).contiguous()
        if dyn is not None:
            dyn = torch.as_tensor(dyn).reshape(N, P).to(dev).ne(0).to(torch.uint8).contiguous()
        if rgb is not None:
            rgb = torch.as_tensor(rgb)
            if rgb.dtype != torch.uint8:
                raise TypeError(f"export_points: rgb must be uint8, got {rgb.dtype}")
            rgb = rgb.to(dev).reshape(N, P, 3).contiguous()
        ws = torch.empty(int(self.lib.a3r_align_scene_workspace_bytes(N, P)), dtype=torch.uint8, device=dev)
        return conf, dyn, rgb, ws

    def count_points(self, conf, thr, dyn=None):
        """(kept pixels of the scene, per-image counts [N] int32 on the device) under the rule of export_points."""
        conf, dyn, _, ws = self._scene_inputs(conf, dyn, None)
        counts = torch.empty(self.N, dtype=torch.int32, device=self.device)
        total = C.c_longlong(0)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_scene_count(self._states[0].handle, ptr(conf), float(thr), ptr(dyn), ptr(ws), ws.numel(), ptr(counts),
                                                 C.byref(total), stream_ptr()), "a3r_align_scene_count")
        return int(total.value), counts

    def export_points(self, conf, thr, dyn=None, rgb=None, with_index=False):
        """The scene compacted to the pixels with conf > thr (strict), dyn == 0 and finite coordinates, image-major and row-major:
        dict(xyz [M,3] float32, rgb [M,3] uint8 when `rgb` [N,P,3] uint8 is given, index [M] int32 = n * P + p with with_index).
        conf [N,P] (padding pixels of smaller images are never kept whatever it holds there); dyn [N,P], non-zero = dropped."""
        conf, dyn, rgb, ws = self._scene_inputs(conf, dyn, rgb)
        h, dev = self._states[0].handle, self.device
        total = C.c_longlong(0)
        with torch.cuda.device(dev):
            check(self.lib.a3r_align_scene_count(h, ptr(conf), float(thr), ptr(dyn), ptr(ws), ws.numel(), None, C.byref(total), stream_ptr()),
                  "a3r_align_scene_count")
            M = int(total.value)
            out = dict(xyz=torch.empty(M, 3, dtype=torch.float32, device=dev))
            if rgb is not None:
                out["rgb"] = torch.empty(M, 3, dtype=torch.uint8, device=dev)
            if with_index:
                out["index"] = torch.empty(M, dtype=torch.int32, device=dev)
            written = C.c_longlong(0)
            check(self.lib.a3r_align_scene_export(h, ptr(conf), float(thr), ptr(dyn), ptr(rgb), ptr(ws), ws.numel(), M, ptr(out["xyz"]),
                                                  ptr(out.get("rgb")), ptr(out.get("index")), C.byref(written), stream_ptr()),
                  "a3r_align_scene_export")
        assert written.value == M
        return out

    def _mesh_workspace(self):
        return torch.empty(int(self.lib.a3r_align_scene_mesh_workspace_bytes(self.N, self.P)), dtype=torch.uint8, device=self.device)

    def count_mesh(self, conf, thr, dyn=None, double_sided=False):
        """(V, F): the vertices and faces export_mesh would return."""
        conf, dyn, _, _ = self._scene_inputs(conf, dyn, None)
        ws = self._mesh_workspace()
        nv, nf = C.c_longlong(0), C.c_longlong(0)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_scene_mesh_count(self._states[0].handle, ptr(conf), float(thr), ptr(dyn), ptr(ws), ws.numel(),
                                                      int(bool(double_sided)), C.byref(nv), C.byref(nf), stream_ptr()),
                  "a3r_align_scene_mesh_count")
        return int(nv.value), int(nf.value)

    def export_mesh(self, conf, thr, dyn=None, rgb=None, double_sided=False):
        """The scene as a triangle mesh over the pixels export_points keeps (pts3d_to_trimesh / cat_meshes of the reference's
        dust3r/viz.py with every index replaced by the pixel's rank among the kept pixels; include/a3r.h has the definition):
        dict(xyz [V,3] float32 and rgb [V,3] uint8 -- bitwise those of export_points --, faces [F,3] int32 vertex ids, face_rgb [F,3]
        uint8; the colours when `rgb` [N,P,3] uint8 is given).  Two triangles per pixel quad, each kept where its three corner pixels
        are; double_sided adds every triangle wound backwards, in the reference's [A, A', B, B'] layout per image."""
        conf, dyn, rgb, _ = self._scene_inputs(conf, dyn, rgb)
        ws = self._mesh_workspace()
        h, dev, ds = self._states[0].handle, self.device, int(bool(double_sided))
        nv, nf = C.c_longlong(0), C.c_longlong(0)
        with torch.cuda.device(dev):
            check(self.lib.a3r_align_scene_mesh_count(h, ptr(conf), float(thr), ptr(dyn), ptr(ws), ws.numel(), ds, C.byref(nv), C.byref(nf),
                                                      stream_ptr()), "a3r_align_scene_mesh_count")
            V, F = int(nv.value), int(nf.value)
            out = dict(xyz=torch.empty(V, 3, dtype=torch.float32, device=dev))
            if rgb is not None:
                out["rgb"] = torch.empty(V, 3, dtype=torch.uint8, device=dev)
            out["faces"] = torch.empty(F, 3, dtype=torch.int32, device=dev)
            if rgb is not None:
                out["face_rgb"] = torch.empty(F, 3, dtype=torch.uint8, device=dev)
            check(self.lib.a3r_align_scene_mesh_export(h, ptr(conf), float(thr), ptr(dyn), ptr(rgb), ptr(ws), ws.numel(), ds, V, F,
                                                       ptr(out["xyz"]), ptr(out.get("rgb")), ptr(out["faces"]), ptr(out.get("face_rgb")),
                                                       C.byref(nv), C.byref(nf), stream_ptr()), "a3r_align_scene_mesh_export")
        assert (nv.value, nf.value) == (V, F)
        return out

    def clean_confidences(self, conf, tol=0.001, bad_conf=0.0):
        """clean_pointcloud of the reference (cloud_opt/base_opt.py:468-503) on the current state: a new [N,P] float32 device tensor
        in which conf[i,p] is clipped to bad_conf wherever another, more confident view sees the point of (i,p) in front of its own
        depth map by more than `tol` (images in order, each reading the finished rows below it; include/a3r.h has the rule).  The
        input is left untouched; padding entries and NaNs pass through."""
        N, P, dev = self.N, self.P, self.device
        out = torch.as_tensor(conf).to(dev, torch.float32).reshape(N, P).clone(memory_format=torch.contiguous_format)
        ws = torch.empty(int(self.lib.a3r_align_scene_clean_workspace_bytes(N, P)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(self.lib.a3r_align_scene_clean(self._states[0].handle, ptr(out), float(tol), float(bad_conf), ptr(ws), ws.numel(),
                                                 stream_ptr()), "a3r_align_scene_clean")
        return out


class AlignEngine(_AlignEngineBase):
    def __init__(self, ei, ej, pred_i, pred_j, w_i, w_j, imshapes, mono=None, base_scale=0.5, pw_break=20.0,
                 focal_break=20.0, norm_pw_scale=True, dist="l1", train_poses=True, train_focals=True, train_pp=False,
                 train_adaptors=False, device="cuda:0", loss_capacity=4096, shared_focal=False, temporal_smoothing_weight=0.0,
                 translation_weight=0.1, flow=None, obs_dtype="fp32", pack_budget_bytes=1 << 30):
        """obs_dtype: 'fp32', or 'fp16' = the observations are packed on upload (obs16.py: 16 bytes per edge-pixel instead of 32, in
        row chunks of at most pack_budget_bytes of fp32 rows); everything else stays fp32.
        flow (cloud_opt_flow variant): dict(flow_ij [E,2,P], flow_ji [E,2,P], dyn [N,P] bool, weight, thre, start_epoch,
        num_total_iter, pxl_thre) -- the optical-flow fields and dynamic masks are inputs (optimizer.py:104-116)."""
        super().__init__(ei, ej, pred_i, pred_j, w_i, w_j, imshapes, mono, base_scale, pw_break, focal_break, norm_pw_scale, dist,
                         train_poses, train_focals, train_pp, train_adaptors, device, loss_capacity, shared_focal=shared_focal,
                         obs_dtype=obs_dtype, pack_budget_bytes=pack_budget_bytes)
        E, N, P, dev = self.E, self.N, self.P, self.device
        self.tsw, self.trans_w = float(temporal_smoothing_weight), float(translation_weight)
        if flow is not None and flow.get("weight", 0) > 0:
            if self.use_mono or len(set(self.imshapes)) != 1:
                raise RuntimeError("the flow variant needs images of one shape and no mono-depth parameterisation")
            self.flow = dict(flow)
            self.flow["flow_ij"] = self._f32(flow["flow_ij"]).reshape(E, 2, P)
            self.flow["flow_ji"] = self._f32(flow["flow_ji"]).reshape(E, 2, P)
            self.flow["dyn"] = torch.as_tensor(np.ascontiguousarray(flow["dyn"])).reshape(N, P).to(dev, torch.uint8).contiguous()
        self.flow_variant = self.shared_focal or self.tsw > 0 or self.flow is not None
        self.train_masks = None       # set_train_masks(): dict(pose, focal, pp, depth) of [N] uint8 | None
        self.flow_workspace = (torch.empty(int(self.lib.a3r_align_flow_workspace_bytes(E, N, P)), dtype=torch.uint8, device=dev)
                               if self.flow_variant else None)
        self._alloc_state(self, self.lib.a3r_align_workspace_bytes(E, N, P))
        self._create()

    @property
    def _states(self):
        return (self,)

    def _create(self):
        self._destroy(self)
        d = self._fill_desc(self.params, self.adam, self.workspace, self.loss_history, slice(None))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_create(C.byref(d), C.byref(h), stream_ptr()), "a3r_align_create")
            if self.flow_variant:
                f = AlignFlowDesc()
                f.shared_focal = int(self.shared_focal)
                f.temporal_smoothing_weight, f.translation_weight = self.tsw, self.trans_w
                if self.flow is not None:
                    fl = self.flow
                    f.flow_loss_weight, f.flow_loss_thre, f.pxl_thre = fl["weight"], fl["thre"], fl["pxl_thre"]
                    bound = fl["num_total_iter"] * fl["start_epoch"]        # epoch >= num_total_iter * flow_loss_start_epoch
                    f.flow_start_iter = next(e for e in range(0, 1 << 30) if e >= bound)
                    f.H, f.W = self.imshapes[0]
                    f.flow_ij, f.flow_ji = fl["flow_ij"].data_ptr(), fl["flow_ji"].data_ptr()
                    f.dynamic_mask = fl["dyn"].data_ptr()
                f.workspace, f.workspace_bytes = self.flow_workspace.data_ptr(), self.flow_workspace.numel()
                check(self.lib.a3r_align_set_flow(h, C.byref(f), stream_ptr()), "a3r_align_set_flow")
            if self.prior is not None:
                pr = self.prior
                check(self.lib.a3r_align_set_depth_prior(h, float(pr["weight"]), pr["init"].data_ptr(),
                                                         pr["dyn"].data_ptr() if pr["dyn"] is not None else None,
                                                         pr["workspace"].data_ptr(), pr["workspace"].numel(), stream_ptr()),
                      "a3r_align_set_depth_prior")
        self.handle = h
        self._push_train_masks()

    def _push_train_masks(self, force=False):
        m = self.train_masks
        if m is None or (not force and all(v is None for v in m.values())):
            return
        arg = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_set_train_masks(self.handle, arg(m["pose"]), arg(m["focal"]), arg(m["pp"]), arg(m["depth"]),
                                                     stream_ptr()), "a3r_align_set_train_masks")

    def set_train_masks(self, pose=None, focal=None, pp=None, depth=None):
        """Per-image train masks ([N] booleans, True = trained; None = no per-image freeze, the train_* flag alone decides).
        A frozen group gets no Adam step and keeps its moments; loss_grad() returns exact zeros in its rows.  The masks survive
        set_params / set_trainable (the handle is re-created with them).  Every call replaces all four."""
        if focal is not None and self.shared_focal:
            raise ValueError("a per-image focal mask cannot be combined with shared_focal (one focal parameter for all images)")
        m = {}
        for k, v in dict(pose=pose, focal=focal, pp=pp, depth=depth).items():
            if v is not None:
                v = np.ascontiguousarray(np.asarray(v).astype(bool).astype(np.uint8)).reshape(-1)
                if v.shape[0] != self.N:
                    raise ValueError(f"train mask {k!r}: expected {self.N} entries, got {v.shape[0]}")
            m[k] = v
        self.train_masks = m
        self._push_train_masks(force=True)

    def set_depth_prior(self, weight, dyn=None, init=None):
        """depth_regularize_weight of the flow variant (optimizer.py:546-555).  `init`: [N,P] log-depth parameters to regularise
        towards (default: a copy of the current ones, which is what _set_init_depthmap captures); `dyn`: [N,P] dynamic masks."""
        if weight <= 0:
            self.prior = None
        else:
            if self.use_mono:
                raise RuntimeError("the depth prior belongs to the flow variant, which has no mono-depth parameterisation")
            init = self.params["depth"].clone() if init is None else torch.as_tensor(init, dtype=torch.float32).to(self.device).reshape(self.N, self.P).contiguous()
            if dyn is not None:
                dyn = torch.as_tensor(np.ascontiguousarray(dyn)).reshape(self.N, self.P).to(self.device, torch.uint8).contiguous()
            ws = torch.empty(int(self.lib.a3r_align_depth_prior_workspace_bytes(self.N, self.P)), dtype=torch.uint8, device=self.device)
            self.prior = dict(weight=float(weight), init=init, dyn=dyn, workspace=ws)
        with torch.cuda.device(self.device):
            pr = self.prior
            check(self.lib.a3r_align_set_depth_prior(self.handle, float(pr["weight"]) if pr else 0.0, pr["init"].data_ptr() if pr else None,
                                                     pr["dyn"].data_ptr() if pr and pr["dyn"] is not None else None,
                                                     pr["workspace"].data_ptr() if pr else None, pr["workspace"].numel() if pr else 0,
                                                     stream_ptr()), "a3r_align_set_depth_prior")

    # ------------------------------------------------------------------ compute
    def loss(self):
        out = torch.zeros(1, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_loss(self.handle, ptr(out), stream_ptr()), "a3r_align_loss")
        return out

    def loss_grad(self, epoch=9999):
        g_pw = torch.zeros_like(self.params["pw_poses"])
        g_ad = torch.zeros_like(self.params["pw_adaptors"])
        g_depth = torch.zeros_like(self.params["depth"])
        g_small = torch.zeros(self.N, 16, device=self.device)
        loss = torch.zeros(1, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_grad_full(self.handle, int(epoch), ptr(g_pw), ptr(g_ad), ptr(g_depth), ptr(g_small), ptr(loss),
                                               stream_ptr()), "a3r_align_grad")
        return float(loss.item()), self._grad_dict(g_pw, g_ad, g_depth, g_small)

    def step(self, lr, epoch=None):
        with torch.cuda.device(self.device):
            if epoch is None:
                check(self.lib.a3r_align_step(self.handle, float(lr), stream_ptr()), "a3r_align_step")
            else:
                check(self.lib.a3r_align_step_epoch(self.handle, float(lr), int(epoch), stream_ptr()), "a3r_align_step")

    @property
    def flow_dropped(self):
        """True once the flow term was dropped because its loss exceeded flow_loss_thre (self.flow_loss_flag)."""
        if self.flow is None:
            return False
        st = np.zeros(5, np.float32)
        check(self.lib.a3r_align_flow_state(self.handle, st.ctypes.data_as(C.c_void_p)))
        return bool(st[4] != 0)

    def run(self, niter, lr, schedule="cosine", lr_min=1e-6, first_iter=0, total_iters=None):
        """global_alignment_loop (base_opt.py:424-447) without per-iteration host syncs; returns the losses."""
        start = self.steps_done
        lrs = self._lrs(niter, lr, schedule, lr_min, first_iter, total_iters)
        with torch.cuda.device(self.device):
            check(self.lib.a3r_align_run(self.handle, lrs.ctypes.data_as(C.c_void_p), int(niter), int(first_iter), stream_ptr()), "a3r_align_run")
        return self.loss_history[start:start + niter].cpu().numpy().astype(np.float64)


class _ShardReplica:
    """One a3r_align_shard handle: the observation rows [e0, e1) and a full copy of the parameters, Adam moments and loss history."""

    def __init__(self, e0, e1):
        self.e0, self.e1 = int(e0), int(e1)
        self.handle = None


class ShardedAlignEngine(_AlignEngineBase):
    """Edge-sharded AlignEngine: every shard walks its own rows of the stacked observations, the additive partial results (one flat
    fp32 buffer: depth-parameter gradient map, per-image sums, per-edge sums) are summed, and every shard applies the same update
    to its replica of the parameters -- ONE reduction per iteration.  Two reducers:

      local_shards=K   K shard handles on this device, summed in a fixed order by a3r_align_shard_sum (bitwise reproducible);
      group=pg         one shard per rank of a torch.distributed group, exactly one all_reduce(SUM) of the buffer per iteration.

    Shard bounds are parallel.shard_rows(E, rank, world); shards that come out empty are skipped with local_shards and refused
    with group.  The observations are either the whole graph's [E, ...] (each shard takes a view of its rows) or, with group,
    this rank's rows only [e1 - e0, ...] (a rank's inference output is its shard).  Limits: plain cloud_opt only (no flow
    variant, no depth prior); the initial state comes through set_params.  obs_dtype='fp16': packed observations as in AlignEngine
    (every shard gets its rows of the records and of the exponent tables).  Same surface as AlignEngine: params, set_params,
    loss, loss_grad, step, run, steps_done, trainable, pose_matrices, points, export_points (replica 0)."""

    def __init__(self, ei, ej, pred_i, pred_j, w_i, w_j, imshapes, mono=None, base_scale=0.5, pw_break=20.0, focal_break=20.0,
                 norm_pw_scale=True, dist="l1", train_poses=True, train_focals=True, train_pp=False, train_adaptors=False,
                 device="cuda:0", loss_capacity=4096, local_shards=None, group=None, obs_dtype="fp32", pack_budget_bytes=1 << 30,
                 **unsupported):
        check_obs_dtype(obs_dtype)
        if unsupported.get("flow") is not None or unsupported.get("shared_focal") or unsupported.get("temporal_smoothing_weight", 0) > 0:
            raise NotImplementedError("ShardedAlignEngine: the flow variant (shared focal, temporal smoothing, ego-flow) is not edge-sharded")
        bad = set(unsupported) - {"flow", "shared_focal", "temporal_smoothing_weight", "translation_weight"}
        if bad:
            raise TypeError(f"ShardedAlignEngine: unexpected arguments {sorted(bad)}")
        if (local_shards is None) == (group is None):
            raise ValueError("ShardedAlignEngine: pass exactly one of local_shards=K and group=<process group>")
        self.group, self._local_shards = group, local_shards
        self._all_reduce = None
        if group is not None:
            from .parallel import GradientAllReduce
            self._all_reduce = GradientAllReduce(group)
        super().__init__(ei, ej, pred_i, pred_j, w_i, w_j, imshapes, mono, base_scale, pw_break, focal_break, norm_pw_scale, dist,
                         train_poses, train_focals, train_pp, train_adaptors, device, loss_capacity, obs_dtype=obs_dtype,
                         pack_budget_bytes=pack_budget_bytes)
        E, N, P = self.E, self.N, self.P
        self.n_floats = int(self.lib.a3r_align_shard_reduce_floats(E, N, P))
        self.replicas = []
        for e0, e1 in self.bounds:
            r = _ShardReplica(e0, e1)
            self._alloc_state(r, self.lib.a3r_align_shard_workspace_bytes(E, e1 - e0, N, P))
            r.buf = torch.zeros(self.n_floats, dtype=torch.float32, device=self.device)
            self.replicas.append(r)
        self.params = self.replicas[0].params           # the replicas hold identical values; this one is the public view
        self.loss_history = self.replicas[0].loss_history
        self._create()

    def _select_rows(self, E, pred_i, pred_j, w_i, w_j):
        """The shard bounds, and which rows of the observations are held here: the whole graph's [E, ...] or, with group, this
        rank's."""
        from .parallel import shard_rows
        group = self.group
        if group is not None:
            import torch.distributed as tdist
            world, rank = tdist.get_world_size(group), tdist.get_rank(group)
            e0, e1, _ = shard_rows(E, rank, world)
            if e0 >= e1:
                raise ValueError(f"ShardedAlignEngine: rank {rank} of {world} gets no edge of a graph with {E} edges; use fewer ranks")
            bounds = [(e0, e1)]
        else:
            K = int(self._local_shards)
            if K < 1:
                raise ValueError("ShardedAlignEngine: local_shards must be >= 1")
            bounds = [b[:2] for b in (shard_rows(E, r, K) for r in range(K)) if b[0] < b[1]]
        self.bounds = bounds
        rows = torch.as_tensor(w_i).shape[0]
        if rows == E:
            lo = 0
            if group is not None and not torch.as_tensor(w_i).is_cuda:      # upload this rank's rows only
                lo = bounds[0][0]
                pred_i, pred_j, w_i, w_j = (torch.as_tensor(t)[lo:bounds[0][1]] for t in (pred_i, pred_j, w_i, w_j))
        elif group is not None and rows == bounds[0][1] - bounds[0][0]:
            lo = bounds[0][0]
        else:
            raise ValueError(f"ShardedAlignEngine: {rows} observation rows for a graph with {E} edges (shards {bounds})")
        self._row0 = lo                          # graph edge of row 0 of the observation tensors held here
        return len(w_i), pred_i, pred_j, w_i, w_j

    @property
    def _states(self):
        return self.replicas

    def _create(self):
        for r in self.replicas:
            self._destroy(r)
            # the shard's rows of the tensors held here
            d = self._fill_desc(r.params, r.adam, r.workspace, r.loss_history, slice(r.e0 - self._row0, r.e1 - self._row0))
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                check(self.lib.a3r_align_shard_create(C.byref(d), r.e0, r.e1, C.byref(h), stream_ptr()), "a3r_align_shard_create")
            r.handle = h

    def set_depth_prior(self, weight, dyn=None, init=None):
        if weight > 0:
            raise NotImplementedError("ShardedAlignEngine: the depth prior belongs to the flow variant, which is not edge-sharded")

    @property
    def flow_dropped(self):
        return False

    # ------------------------------------------------------------------ compute
    def _partials(self):
        for r in self.replicas:
            check(self.lib.a3r_align_shard_partial(r.handle, ptr(r.buf), self.n_floats, stream_ptr()), "a3r_align_shard_partial")

    def _reduce(self):
        """The one reduction of an iteration; the reduced buffer is replica 0's."""
        if self._all_reduce is not None:
            self._all_reduce(self.replicas[0].buf)
        elif len(self.replicas) > 1:
            srcs = (C.c_void_p * len(self.replicas))(*[r.buf.data_ptr() for r in self.replicas])
            check(self.lib.a3r_align_shard_sum(ptr(self.replicas[0].buf), srcs, len(self.replicas), self.n_floats, stream_ptr()),
                  "a3r_align_shard_sum")
        return self.replicas[0].buf

    def loss_grad(self, epoch=9999):
        r0 = self.replicas[0]
        g_pw = torch.zeros_like(r0.params["pw_poses"])
        g_ad = torch.zeros_like(r0.params["pw_adaptors"])
        g_small = torch.zeros(self.N, 16, device=self.device)
        loss = torch.zeros(1, device=self.device)
        with torch.cuda.device(self.device):
            self._partials()
            red = self._reduce()
            check(self.lib.a3r_align_shard_grad(r0.handle, ptr(red), self.n_floats, ptr(g_pw), ptr(g_ad), ptr(g_small), ptr(loss),
                                                stream_ptr()), "a3r_align_shard_grad")
        g_depth = red[:self.N * self.P].reshape(self.N, self.P).clone()
        return float(loss.item()), self._grad_dict(g_pw, g_ad, g_depth, g_small)

    def loss(self):
        return torch.tensor([self.loss_grad()[0]], device=self.device)

    @property
    def collectives(self):
        """all-reduces issued so far (group form)."""
        return self._all_reduce.calls if self._all_reduce is not None else 0

    def _apply(self, red, lr):
        for r in self.replicas:
            check(self.lib.a3r_align_shard_apply(r.handle, ptr(red), self.n_floats, float(lr), stream_ptr()), "a3r_align_shard_apply")

    def step(self, lr, epoch=None):
        from .parallel import sharded_step
        with torch.cuda.device(self.device):
            sharded_step(self._partials, lambda _: self._reduce(), self._apply, lr)

    def run(self, niter, lr, schedule="cosine", lr_min=1e-6, first_iter=0, total_iters=None):
        start = self.steps_done
        if start + niter > self.loss_capacity:
            raise RuntimeError(f"loss_history too small ({start} + {niter} > {self.loss_capacity})")
        lrs = self._lrs(niter, lr, schedule, lr_min, first_iter, total_iters)
        if self.group is not None:
            for v in lrs:
                self.step(float(v))
        else:
            K = len(self.replicas)
            hs = (C.c_void_p * K)(*[r.handle.value for r in self.replicas])
            bufs = (C.c_void_p * K)(*[r.buf.data_ptr() for r in self.replicas])
            with torch.cuda.device(self.device):
                check(self.lib.a3r_align_shard_run_local(hs, K, bufs, self.n_floats, lrs.ctypes.data_as(C.c_void_p), int(niter), stream_ptr()),
                      "a3r_align_shard_run_local")
        return self.loss_history[start:start + niter].cpu().numpy().astype(np.float64)
