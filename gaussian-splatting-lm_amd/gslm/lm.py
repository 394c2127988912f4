"""Matrix-free Levenberg-Marquardt on the HIP rasterizer: the hot path of train_jvp.py's LM branch.

Reference semantics:
  * residual (batch_training_loss.py:10-17, disable_ssim=True):  r_b = m_b * clamp01(R_b) - gt_b, and
    the "ssim" slot aliases r, so the residual vector is [r; r]: loss = 2 ||r||^2, J^T J = 2 J_r^T J_r.
  * cgls_damped (conjugate_gradient.py:51-127) solves (J^T J + D) x = J^T b with b = -[r; r]
    (train_jvp.py:243), D the per-group diagonal of GaussianModelDampMatrix (train_jvp.py:229-235),
    xyz frozen by the param mask (train_jvp.py:221-227).
  * line search: alpha = 2, 1, ..., 1/16 on the validation views, keep the best (train_jvp.py:264-279).

MI355X design: the operator A = J^T J + D is applied by one fused HIP pass per view (gslm_matvec_view:
tangent preprocess -> JVP tile pass -> weight -> VJP tile pass -> gather-sum preprocess backward) on
geometry cached once per LM step (the sort is not redone per matvec).  CG runs on flat param-space
vectors with its scalars in device memory (gslm_dot / gslm_axpy_dev / gslm_xpby_dev): with
`check=False` an iteration has no host synchronisation at all.  CGLS on (J, D) and CG on A generate
the same iterates in exact arithmetic; the reference's restart schedule and stopping tests are kept.
"""
import copy
import ctypes
import math
import os

import torch

from gslm import _lib
from gslm._lib import check, lib
from gslm.params import GROUPS, ParamLayout, raw_gaussians

# train_jvp.py:229-235
STAGE_ALL = 7
STAGE_OVERWRITE = 8
MV_TAIL_CLEAN = 1  # gslm_matvec_opts.flags: GSLM_MV_TAIL_CLEAN
MV_SH_REST_PROJECTED = 2  # GSLM_MV_SH_REST_PROJECTED
MV_LEAN = 4  # GSLM_MV_LEAN
MV_EXPOSURE = 8  # GSLM_MV_EXPOSURE
MV_DAMP_VEC = 16  # GSLM_MV_DAMP_VEC
MV_DEPTH = 32  # GSLM_MV_DEPTH
MV_XYZ = 64  # GSLM_MV_XYZ (gslm_gather_views)
DIAG_TAIL_CLEAN = 1  # gslm_lm_diag_view flags: GSLM_DIAG_TAIL_CLEAN
DIAG_ACCUMULATE = 2  # GSLM_DIAG_ACCUMULATE
DIAG_SH_REST_PROJECTED = 4  # GSLM_DIAG_SH_REST_PROJECTED

DEFAULT_DAMP = {"xyz": 5e2, "features_dc": 5e-2, "features_rest": 5e-2, "scaling": 5e-2, "rotation": 5e-2,
                "opacity": 5e-2, "exposure": 1e1}


def _grown(buf, need, device, main=None, side=None):
    """The workspace `buf` when it holds `need` bytes, else a new one with 25 % + 4096 bytes of slack (a list that
    grows a little from one geometry to the next is not allocated again).  side: the stream that used the old
    buffer; it is freed on the stream `main`, which therefore waits for `side` first."""
    if buf is not None and buf.numel() >= need:
        return buf
    if buf is not None and side is not None:
        main.wait_stream(side)
    return _lib.u8(int(need * 1.25) + 4096, device)


class ViewRaster:
    """Primal forward of one view on raw GaussianModel leaves + the buffers the matvec reuses."""

    def __init__(self, view, device):
        self.view = view
        self.H, self.W = view.image_height, view.image_width
        self.device = device
        self.N = 0
        self.geom = self.binning = self.image = self.scratch = None
        # the scratch's gradient rows of never-blended entries hold the zeros of an earlier fused
        # product on the current geometry (GSLM_MV_TAIL_CLEAN): false after a forward or a backward
        self._active = None
        self._params = None
        self.tail_clean = False
        self.epoch = 0  # forwards so far: a right-hand side belongs to the geometry of one of them

    @property
    def tail_clean(self):
        return self._tail_clean

    @tail_clean.setter
    def tail_clean(self, value):
        self._tail_clean = bool(value)
        if not value:
            self._active = None  # the active list is the row map's: it lives exactly as long
            self._params = None  # ... and so does the list-order parameter block

    def active_list(self, P, stream):
        """(ids, Pa): the ascending int32 ids of the Gaussians that own a head row of this view's LM row map
        (gslm_active_list) and their number -- the Gaussians whose column of this view's J is not identically
        zero.  Needs the row map of an earlier product (tail_clean); built once per geometry (one read-back) and
        kept until the next forward or backward."""
        if not self.tail_clean or self.N is None:
            raise RuntimeError("active_list: no current LM row map (run a product or rhs() on this geometry first)")
        if self._active is None:
            dev = self.device
            ids = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
            rows = torch.empty(P + 1, dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            work = _lib.u8(lib.gslm_active_list_bytes(P), dev)
            check(lib.gslm_active_list(self.geom.data_ptr(), P, self.N, self.scratch.data_ptr(), self.scratch.numel(),
                                       work.data_ptr(), work.numel(), ids.data_ptr(), rows.data_ptr(),
                                       count.data_ptr(), stream), "gslm_active_list")
            n = int(count.item())
            self._active = (ids[:n], n)
            self.active_rows = rows[:n + 1]  # entry j's head rows: [rows[j], rows[j + 1])
        return self._active

    def list_words(self, stream):
        """(words, slots): copies of the sorted list's raw words (Gaussian id in the low 28 bits, quadrant mask in the
        top 4) and of the row map's slot of each entry (gslm_inspect_list) -- a diagnostic."""
        n = max(self.N, 1)
        words = torch.zeros(n, dtype=torch.int32, device=self.device)
        slots = torch.zeros(n, dtype=torch.int32, device=self.device)
        check(lib.gslm_inspect_list(self.binning.data_ptr(), self.binning.numel(), self.N, self.H, self.W,
                                    words.data_ptr(), slots.data_ptr(), stream), "gslm_inspect_list")
        return words[:self.N], slots[:self.N]

    def active_params(self, model, P, stream):
        """(block, pos): the list-order copy of the parameters the LM chains load per Gaussian (gslm_active_params)
        for active_list(), and the inverse map pos [P] (list row of a Gaussian, -1 off the list).  The block is a
        snapshot of the leaves, so it is keyed on them: built with the list (a forward or backward drops both) and
        again whenever a leaf was replaced or written in place since (the tensor objects and their version counters:
        _lib.tensor_token), which is checked here at every use -- a solve never reads a block older than its
        parameters."""
        ids, na = self.active_list(P, stream)
        leaves = (model._xyz, model._scaling, model._rotation, model._opacity)
        if self._params is None or not _lib.tokens_match(self._params[0], leaves):
            key = tuple(_lib.tensor_token(t) for t in leaves)
            dev = self.device
            block = _lib.u8(lib.gslm_active_params_bytes(na), dev)
            pos = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
            g = raw_gaussians(model)
            check(lib.gslm_active_params(ctypes.byref(g), self.geom.data_ptr(), P, ids.data_ptr() if na else None, na,
                                         block.data_ptr(), block.numel(), pos.data_ptr(), stream), "gslm_active_params")
            self._params = (key, block, pos)
        return self._params[1], self._params[2]

    def forward(self, g, stream, want_invdepth=True):
        """The full forward (the drop-in's gslm_preprocess + gslm_rasterize).  want_invdepth=False: the LM paths,
        which never read the inverse depth -- the blend then skips its accumulation (and its image)."""
        P = g.P
        dev = self.device
        self.tail_clean = False
        self.epoch += 1
        if self.geom is None or self.geom.numel() < lib.gslm_geom_bytes(P):
            self.geom = _lib.u8(lib.gslm_geom_bytes(P), dev)
            self.image = _lib.u8(lib.gslm_image_bytes(self.H, self.W), dev)
            self.color = torch.empty(3, self.H, self.W, dtype=torch.float32, device=dev)
            self.invdepth = torch.empty(1, self.H, self.W, dtype=torch.float32, device=dev)
            self.radii = torch.empty(P, dtype=torch.int32, device=dev)
        check(lib.gslm_preprocess(ctypes.byref(self.view), ctypes.byref(g), self.geom.data_ptr(), self.geom.numel(),
                                  self.radii.data_ptr(), stream), "gslm_preprocess")
        n = ctypes.c_int64(0)
        check(lib.gslm_num_rendered(self.geom.data_ptr(), P, ctypes.byref(n), stream), "gslm_num_rendered")
        self.N = int(n.value)
        self.binning = _grown(self.binning, lib.gslm_binning_bytes(self.N, self.H, self.W), dev)
        check(lib.gslm_rasterize(ctypes.byref(self.view), P, self.geom.data_ptr(), self.binning.data_ptr(),
                                 self.binning.numel(), self.N, self.image.data_ptr(), self.image.numel(),
                                 self.color.data_ptr(), self.invdepth.data_ptr() if want_invdepth else None, stream),
              "gslm_rasterize")
        self.scratch = _grown(self.scratch, lib.gslm_scratch_bytes(P, self.N), dev)
        return self.color

    def forward_dev(self, g, stream, want_invdepth=True, n_out=None):
        """forward() without the pair-count read-back between the preprocess and the binning (gslm_rasterize_dev):
        the binning workspace of an earlier forward() is used as a list of its capacity, the count stays on the
        device, and n_out (device or pinned uint32 address, or None) receives it in stream order.  The image is valid
        when the count fits `capacity()`.  The binning then serves this render only: an LM product on this view needs
        a forward() first (self.N is None until then)."""
        if self.binning is None or self.geom is None or self.geom.numel() < lib.gslm_geom_bytes(g.P):
            raise RuntimeError("forward_dev: the workspaces of an earlier forward() at this P are required")
        P = g.P
        self.tail_clean = False
        self.epoch += 1
        self.N = None
        check(lib.gslm_preprocess(ctypes.byref(self.view), ctypes.byref(g), self.geom.data_ptr(), self.geom.numel(),
                                  self.radii.data_ptr(), stream), "gslm_preprocess")
        check(lib.gslm_rasterize_dev(ctypes.byref(self.view), P, self.geom.data_ptr(), self.binning.data_ptr(),
                                     self.binning.numel(), self.image.data_ptr(), self.image.numel(),
                                     self.color.data_ptr(), self.invdepth.data_ptr() if want_invdepth else None,
                                     n_out, stream), "gslm_rasterize_dev")
        return self.color

    def capacity(self):
        """List capacity of the binning workspace (forward_dev renders at most this many pairs)."""
        return 0 if self.binning is None else int(lib.gslm_binning_capacity(self.binning.numel(), self.H, self.W))

    def product(self, g, vs, weight, mask_xyz, ys, opts, stream, what, active=None):
        """gslm_matvec_view_ex on this view's geometry, binning, image and scratch: the stages and flags of `opts`
        from the input grads struct vs (weight: the per-pixel weights, or the seed / J v image of the stage) into ys.
        active = (ids, na): vs and ys hold the listed Gaussians only -- gslm_matvec_view_active with this view's
        rows of the list.  The call alone: tail_clean and the flags are the caller's."""
        ws = (self.geom.data_ptr(), self.binning.data_ptr(), self.N, self.image.data_ptr(), self.scratch.data_ptr(),
              self.scratch.numel())
        if active is not None:
            ids, na = active
            check(lib.gslm_matvec_view_active(ctypes.byref(self.view), ctypes.byref(g), ctypes.byref(vs), weight,
                                              mask_xyz, *ws, ctypes.byref(ys), ctypes.byref(opts),
                                              ids.data_ptr() if na else None, self.active_rows.data_ptr(), na, stream),
                  what.replace("_ex", "_active"))
            return
        check(lib.gslm_matvec_view_ex(ctypes.byref(self.view), ctypes.byref(g), ctypes.byref(vs), weight, mask_xyz,
                                      *ws, ctypes.byref(ys), ctypes.byref(opts), stream), what)


class _ProductOpts:
    """The options every operator with a `layout`, `_damps`, `dot_scratch` and `mv_flags` builds around its products
    (LMProblem and its subclasses; gslm.parallel.GaussianShardedOperator on its shard's layout)."""

    def _opts(self, vr, stages, cg_ctl=None):
        """gslm_matvec_opts of a product on view vr: the stages, the layout's flag and GSLM_MV_TAIL_CLEAN while the
        view's scratch holds the row map of an earlier product on its geometry; cg_ctl: see matvec_dot."""
        opts = _lib.GslmMatvecOpts()
        opts.stages = stages
        opts.flags = (MV_TAIL_CLEAN if vr.tail_clean else 0) | self.mv_flags
        opts.cg_ctl = cg_ctl
        return opts

    def _dot_opts(self, opts, dot_out):
        """<v, y> fused into the gather: summed to the device double dot_out, or with None left as the gather's
        block partials in dot_scratch (the lean loop's dot_defer)."""
        opts.dot_vy = dot_out
        opts.dot_scratch = self.dot_scratch.data_ptr()
        opts.dot_scratch_bytes = self.dot_scratch.numel() * 8

    # pre = (s, beta_num, beta_den[, x, alpha_num, alpha_den]): before the product, [x += alpha v then]
    # v = s + beta v -- the CG direction update (and the deferred x update) of the previous iteration
    def _pre_opts(self, opts, v, pre):
        """Returns the grads struct of s, which opts points to: the caller keeps it alive for the call."""
        s, num, den = pre[:3]
        e0, e1 = self.layout.offsets["exposure"]
        ss = self.layout.grads_struct(s)
        opts.xpby_s = ctypes.addressof(ss)
        opts.beta_num, opts.beta_den = num, den
        if e1 > e0:
            opts.xpby_tail_v = v.data_ptr() + 4 * e0
            opts.xpby_tail_s = s.data_ptr() + 4 * e0
            opts.xpby_tail_n = e1 - e0
        if len(pre) > 3 and pre[3] is not None:
            x, anum, aden = pre[3:]
            opts.alpha_num, opts.alpha_den = anum, aden
            opts.xpby_x_offset = x.data_ptr() - v.data_ptr()
        return ss

    def _exposure_tail(self, v, y, damp=True, exposure_zero=False):
        """The exposure slice of y = [D v +] J^T W J v where J has no exposure column: D v, or zero.
        exposure_zero: the slices of v and y are zero already (matvec_dot) -- nothing is launched, as for an empty
        slice."""
        e0, e1 = self.layout.offsets["exposure"]
        if exposure_zero or e1 == e0:
            return
        dvec = self._damp_vec() if (damp and hasattr(self, "_damp_vec")) else None
        if dvec is not None:
            torch.mul(v[e0:e1], dvec[e0:e1], out=y[e0:e1])
        elif damp:
            torch.mul(v[e0:e1], float(self._damps[6]), out=y[e0:e1])
        else:
            y[e0:e1].zero_()


class _StageTimes:
    """stage_times of an operator whose product records `_mark(k)` between its STAGES."""

    _events = None  # HIP events recorded between the product's stages

    def _mark(self, k):
        if self._events is not None:
            self._events[k].record()

    def stage_times(self, v, reps=10):
        """Per-stage time of a product of direction v (ms, mean over `reps`): HIP events on the product's stream
        between the stages of STAGES (an exchange's all-to-alls include their wait)."""
        y = self.zeros()
        evs = []
        for _ in range(reps):
            self._events = [torch.cuda.Event(enable_timing=True) for _ in range(len(self.STAGES) + 1)]
            self.matvec_dot(v, y, None)
            evs.append(self._events)
            self._events = None
        torch.cuda.synchronize()
        out = {name: sum(e[k].elapsed_time(e[k + 1]) for e in evs) / reps for k, name in enumerate(self.STAGES)}
        out["total"] = sum(e[0].elapsed_time(e[-1]) for e in evs) / reps
        return out


def _exposure_index(model, cams):
    """train_exposure: each camera's row of model._exposure (model.exposure_mapping); ValueError for a model that
    renders with pretrained exposures or a camera without a row."""
    if getattr(model, "pretrained_exposures", None) is not None:
        raise ValueError("train_exposure: the model renders with pretrained exposures, which are not parameters")
    missing = [c.image_name for c in cams if c.image_name not in model.exposure_mapping]
    if missing:
        raise ValueError(f"train_exposure: no row of model._exposure for {missing} (model.exposure_mapping)")
    return [int(model.exposure_mapping[c.image_name]) for c in cams]


_ROBUST_KINDS = {"huber": _lib.GSLM_ROBUST_HUBER, "cauchy": _lib.GSLM_ROBUST_CAUCHY}


def robust_option(robust):
    """The `robust` option of LMProblem, LossEvaluator and lm_step checked: None, or (kind, delta) with kind "huber" or
    "cauchy" and delta a finite number > 0 -- returned as None or the pair (kind, float(delta)); ValueError otherwise."""
    if robust is None:
        return None
    ok = isinstance(robust, (tuple, list)) and len(robust) == 2 and isinstance(robust[0], str) \
        and robust[0] in _ROBUST_KINDS and isinstance(robust[1], (int, float)) and not isinstance(robust[1], bool)
    if not ok or not (math.isfinite(robust[1]) and robust[1] > 0):
        raise ValueError(f"robust must be None, ('huber', delta) or ('cauchy', delta) with a finite delta > 0, "
                         f"got {robust!r}")
    return (robust[0], float(robust[1]))


def _robust_struct(robust):
    """The gslm_robust block of a checked option (None: no block)."""
    return None if robust is None else _lib.GslmRobust(_ROBUST_KINDS[robust[0]], robust[1])


def depth_option(depth_weight):
    """The `depth_weight` option of LMProblem checked: None (no depth residual), or a finite number >= 0 -- returned as
    None or a float; ValueError otherwise."""
    if depth_weight is None:
        return None
    ok = isinstance(depth_weight, (int, float)) and not isinstance(depth_weight, bool)
    if not ok or not (math.isfinite(depth_weight) and depth_weight >= 0):
        raise ValueError(f"depth_weight must be None or a finite number >= 0, got {depth_weight!r}")
    return float(depth_weight)


def _depth_plane(t, what, H, W, device):
    """A depth target or mask checked: float32 [1, H, W] (ValueError otherwise), contiguous on `device`."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (1, H, W):
        got = (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what} must be float32 [1, {H}, {W}], got {got}")
    return t.to(device).contiguous()


def depth_targets(cams, invdepths, depth_masks, device):
    """Per camera (target, mask) of the depth residual, or None for a camera without one.  invdepths / depth_masks:
    explicit lists (as gts / alpha_masks; a None target: no depth term for that view, a None mask: every pixel), or
    None for the cameras' own fields -- invdepthmap where depth_reliable is set, and depth_mask."""
    if invdepths is not None and len(invdepths) != len(cams):
        raise ValueError(f"invdepths: one entry per camera ({len(cams)}), got {len(invdepths)}")
    if depth_masks is not None and len(depth_masks) != len(cams):
        raise ValueError(f"depth_masks: one entry per camera ({len(cams)}), got {len(depth_masks)}")
    out = []
    for b, c in enumerate(cams):
        if invdepths is not None:
            gt = invdepths[b]
        else:
            gt = c.invdepthmap if getattr(c, "depth_reliable", False) else None
        m = depth_masks[b] if depth_masks is not None else getattr(c, "depth_mask", None)
        if gt is None:
            out.append(None)
            continue
        H, W = c.image_height, c.image_width
        out.append((_depth_plane(gt, "an inverse-depth target", H, W, device),
                    None if m is None else _depth_plane(m, "a depth mask", H, W, device)))
    return out


class LMProblem(_ProductOpts):
    """The LM normal equations of one camera batch (one LM step's worth of cached geometry)."""

    def __init__(self, model, cams, bg, gts=None, alpha_masks=None, mask_xyz=True, damp=None, device="cuda",
                 ssim=False, lambda_dssim=0.2, sh_projection=False, train_exposure=False, damping="fixed",
                 marquardt_floor=0.0, robust=None, depth_weight=None, invdepths=None, depth_masks=None):
        """ssim=False: the residual train_jvp.py uses (disable_ssim=True, [r; r]); ssim=True: the
        [r1; r2] residual with the SSIM term (batch_training_loss.py:18-30, gslm_ssim_*).

        train_exposure: the residual is taken on the exposed colour C = R X[:3, :3] + X[:3, 3] of each camera's row
        X of model._exposure (render()'s use_trained_exp, gaussian_renderer/__init__.py:113-119), and the exposure
        rows of the batch's cameras are unknowns of the normal equations: J^T b and (J^T J + D) v carry them in the
        layout's exposure tail (GSLM_MV_EXPOSURE, gslm_lm_residual_exposure).  Single process, mask_xyz=True,
        ssim=False; every camera's image_name must be in model.exposure_mapping and the model must not carry
        pretrained exposures (they are not parameters) -- ValueError otherwise.  Both SH-rest layouts and the active
        list apply unchanged (the exposure rows ride in the flat tail); the lean CG loop does not.

        sh_projection: param-space vectors carry the SH-rest group as 3 coordinates per Gaussian along the
        view's unit basis direction (GSLM_MV_SH_REST_PROJECTED; one view only -- with one view the CG
        iterates of (J^T J + D) x = J^T b never leave that span).  True / False / "auto" (= one camera and
        SH degree > 0).  `expand` / `project` convert to and from the reference's layout (`full_layout`).

        damping: "fixed" (D = the seven absolute constants of `damp`, the reference's GaussianModelDampMatrix) or
        "marquardt": D = diag(d), d = lambda[group] max(diag(sum_b 2 J_b^T W_b J_b), marquardt_floor), with `damp` the
        per-group multiplier lambda -- it must be given (the defaults are absolute values and mean something else).
        d is built lazily, once after each evaluate(): diagonal(damp=False), then gslm_marquardt_scale, IN THE LAYOUT
        THE SOLVE RUNS IN.  With one view and sh_projection that is the projected layout, whose SH-rest diagonal is
        the quadratic form of Bh (x) e_c; on the full layout the SH-rest diagonal is Bh_k^2 times that, which is not
        a scalar on the group, so the projected layout's span argument does not hold for it and the two layouts
        define two different operators.  Each is a valid Marquardt scaling of its own coordinates.
        xyz and the exposure tail have no column in J: their d is lambda marquardt_floor, their right-hand side is
        zero and the iterates stay zero there.  The plain residual on the LM rows only: ValueError with ssim,
        train_exposure, mask_xyz=False, or the batched problem.  The lean CG loop does not run under it.
        set_damping_vector / damping_vector: a caller-supplied per-element D >= 0 in place of either.

        robust: None, ("huber", delta) or ("cauchy", delta) -- the loss is 2 sum rho(r^2) over the residual elements
        (Huber: r^2 where |r| <= delta, 2 delta |r| - delta^2 elsewhere; Cauchy: delta^2 log1p(r^2 / delta^2)), solved by
        iteratively reweighted least squares in the first-order Triggs form: evaluate() multiplies weights[b] and
        seeds[b] by rho'(r^2) at the linearisation point (gslm_lm_residual_robust) and `loss` is the robust loss, so
        rhs() is -1/2 grad loss, the products are 2 J^T (W rho') J + D and every consumer -- the active list, the lean
        loop, diagonal, cgls_jacobi, Marquardt damping, the batched problem and its union list -- runs unchanged;
        residuals[b] stay raw.  The plain residual on the LM rows only: ValueError with ssim, train_exposure or
        mask_xyz=False, and for anything that is not one of the three forms.  cgls_residual, which iterates on the raw
        residuals, refuses a robust problem.

        depth_weight: None, or lambda_d >= 0 -- the inverse-depth residual.  A view with a target
        (invdepths[b], or the camera's invdepthmap where depth_reliable is set; float32 [1, H, W]) and mask
        (depth_masks[b], or the camera's depth_mask; None = every pixel) adds lambda_d sum (m_d (D - Dgt))^2 to the
        loss, D the rendered inverse depth, and J_D^T W_d J_D, W_d = lambda_d m_d^2, to the products: its weights[b],
        seeds[b] and residuals[b] are [4, H, W], the fourth plane gslm_lm_residual_depth's, and its rhs() and products
        set GSLM_MV_DEPTH; the other views run the plain kernels.  On the LM rows 1/z is a constant, so J_D has columns
        in scaling, rotation and opacity only, zero for a Gaussian without a head row: the active list, the lean loop
        and the SH-rest projection apply unchanged.  depth_weight=0.0 is bitwise the problem without it.  The plain
        residual with the fixed damping only: ValueError with ssim, train_exposure, robust, damping="marquardt",
        set_damping_vector, diagonal (cgls_jacobi), cgls_residual, mask_xyz=False, the batched problem and the sharded
        ones."""
        self.depth_weight = depth_option(depth_weight)
        if self.depth_weight is None and (invdepths is not None or depth_masks is not None):
            raise ValueError("invdepths / depth_masks are the targets of depth_weight, which is None")
        if self.depth_weight is not None and (ssim or train_exposure or robust is not None or not mask_xyz or
                                              damping != "fixed"):
            raise ValueError("depth_weight runs the [r; r] residual on the LM rows with the fixed damping "
                             "(mask_xyz=True, no SSIM, no trained exposure, no robust loss, damping='fixed')")
        self.robust = robust_option(robust)
        if self.robust is not None and (ssim or train_exposure or not mask_xyz):
            raise ValueError("robust runs the [r; r] residual on the LM rows (mask_xyz=True, no SSIM, no trained "
                             "exposure)")
        self._robust = _robust_struct(self.robust)
        if damping not in ("fixed", "marquardt"):
            raise ValueError(f"damping must be 'fixed' or 'marquardt', got {damping!r}")
        self.damping = damping
        self.marquardt_floor = float(marquardt_floor)
        self._dvec = None  # the damping vector in this problem's layout (Marquardt's, or set_damping_vector's)
        if damping == "marquardt":
            if damp is None:
                raise ValueError("damping='marquardt': damp is the per-group multiplier lambda and must be given "
                                 "(DEFAULT_DAMP holds absolute values)")
            if ssim or train_exposure or not mask_xyz:  # (BatchedLMProblem refuses it itself)
                raise ValueError("damping='marquardt' runs the [r; r] residual on the LM rows of LMProblem "
                                 "(mask_xyz=True, no SSIM, no trained exposure, not the batched problem)")
            if not (self.marquardt_floor >= 0.0 and math.isfinite(self.marquardt_floor)):
                raise ValueError(f"marquardt_floor must be finite and >= 0, got {marquardt_floor!r}")
        elif self.marquardt_floor != 0.0:
            raise ValueError("marquardt_floor is an option of damping='marquardt'")
        self.model = model
        self.ssim, self.lambda_dssim = bool(ssim), float(lambda_dssim)
        if self.ssim and not mask_xyz:
            raise ValueError("the SSIM residual path runs on the LM rows (mask_xyz=True, train_jvp.py:221-227)")
        self.cams = cams
        self.device = device
        self.bg = bg
        self.mask_xyz = bool(mask_xyz)
        self.train_exposure = bool(train_exposure)
        if self.train_exposure:
            self._init_exposure(model, cams, device)
        P = model._xyz.shape[0]
        K = 1 + model._features_rest.shape[1]
        if sh_projection == "auto":
            sh_projection = len(cams) == 1 and K > 1 and model.active_sh_degree > 0
        if sh_projection and len(cams) != 1:
            raise ValueError("sh_projection is a single-view mode (the Krylov space of one view's J)")
        self.full_layout = ParamLayout(P, K, model._exposure.shape[0])
        self.layout = ParamLayout(P, K, model._exposure.shape[0], rest_projected=bool(sh_projection))
        self.mv_flags = MV_SH_REST_PROJECTED if self.layout.rest_projected else 0
        self.damp = DEFAULT_DAMP if damp is None else damp
        self._bounds, self._damps = self.layout.group_damp_arrays(self.damp)
        self.gts = [c.original_image.to(device) for c in cams] if gts is None else gts
        self.masks = [c.alpha_mask.to(device) for c in cams] if alpha_masks is None else alpha_masks
        self.views = [ViewRaster(_lib.view_from_camera(c, bg, model.active_sh_degree), device) for c in cams]
        # per view (target, mask) of the depth residual, None for a view without one (and always without depth_weight)
        self.depth = (depth_targets(cams, invdepths, depth_masks, device) if self.depth_weight is not None
                      else [None] * len(cams))
        self.stream = _lib.stream_handle(device)
        # >= 3 x 1024 doubles: gslm_cg_update_monitor's three partial sums
        self.dot_scratch = torch.empty(max(lib.gslm_dot_scratch_bytes(max(P, self.layout.numel)) // 8, 3 * 1024) + 8,
                                       dtype=torch.float64, device=device)
        self.weights = [None] * len(cams)
        self.residuals = [None] * len(cams)
        self.seeds = [None] * len(cams)
        self.ssim_state = [None] * len(cams)
        self._jv = [None] * len(cams)
        self._u = [None] * len(cams)
        self.res_scratch = torch.empty(lib.gslm_residual_scratch_bytes(1, 1) // 8, dtype=torch.float64,
                                       device=device)

    def _init_exposure(self, model, cams, device):
        if self.ssim or not self.mask_xyz:
            raise ValueError("train_exposure runs on the LM rows with the plain residual (mask_xyz=True, ssim=False)")
        self.exp_idx = _exposure_index(model, cams)
        X = model._exposure
        if X.dtype != torch.float32 or not X.is_contiguous() or X.shape[1:] != (3, 4):
            raise ValueError("train_exposure: model._exposure must be contiguous float32 [n, 3, 4]")
        self._exp_rhs = torch.zeros(X.numel(), dtype=torch.float32, device=device)  # the exposure rows of J^T b
        self._exp_u = [None] * len(cams)
        self._exp_scratch = torch.empty(lib.gslm_exposure_scratch_bytes(1, 1) // 8, dtype=torch.float64,
                                        device=device)
        seen = set()  # the first view of each camera writes that camera's rows of y (and adds D v there)
        self._exp_first = [not (i in seen or seen.add(i)) for i in self.exp_idx]
        rest = sorted(set(range(X.shape[0])) - seen)
        self._exp_rest = torch.tensor(rest, dtype=torch.long, device=device) if rest else None

    # -------------------------------------------------------------- residual (A8)
    def evaluate(self):
        """Primal forward of every view; residuals, per-pixel weights and the J^T b seeds from one fused
        epilogue per view (gslm_lm_residual); loss = 2 sum ||r||^2 (device double).  With `robust` the epilogue is
        gslm_lm_residual_robust: loss = 2 sum rho(r^2), weights and seeds times rho'."""
        live_masks()  # (a bad GSLM_LIVE_MASKS is refused before the geometry's row map reads it)
        if self.damping == "marquardt":
            self._dvec = None  # (the diagonal of the new weights: rebuilt on first use)
        g = raw_gaussians(self.model)
        loss = torch.zeros((), dtype=torch.float64, device=self.device)
        if self.train_exposure:
            self._exp_rhs.zero_()
        for b, vr in enumerate(self.views):
            dt = self.depth[b]
            R = vr.forward(g, self.stream, want_invdepth=dt is not None)
            planes = (4 if dt is not None else 3,) + tuple(R.shape[1:])  # (the fourth: the depth block's)
            if self.residuals[b] is None or tuple(self.residuals[b].shape) != planes:
                self.residuals[b] = R.new_empty(planes)
                self.weights[b] = R.new_empty(planes)
                self.seeds[b] = R.new_empty(planes)
                if self.train_exposure:
                    self._exp_u[b] = torch.empty_like(R)
            m = self.masks[b]
            gt = self.gts[b]
            if m is not None:
                m = m.to(torch.float32).contiguous()
                if m.numel() != vr.H * vr.W:
                    raise ValueError("alpha mask must be [1, H, W]")
            if gt.shape != R.shape or gt.dtype != torch.float32:
                raise ValueError(f"ground truth must be float32 {tuple(R.shape)}, got {gt.dtype} {tuple(gt.shape)}")
            gt = gt.contiguous()
            if self.ssim:
                if self.ssim_state[b] is None:
                    self.ssim_state[b] = _lib.u8(lib.gslm_ssim_state_bytes(vr.H, vr.W), self.device)
                    self._jv[b] = torch.empty_like(R)
                    self._u[b] = torch.empty_like(R)
                st = self.ssim_state[b]
                check(lib.gslm_ssim_residual(vr.H, vr.W, R.data_ptr(), gt.data_ptr(),
                                             None if m is None else m.data_ptr(), self.lambda_dssim, st.data_ptr(),
                                             st.numel(), None, None, self.seeds[b].data_ptr(), loss.data_ptr(),
                                             int(b > 0), self.stream), "gslm_ssim_residual")
                continue
            if self.train_exposure:
                # the same epilogue on the exposed colour; R stays in vr.color for the products.  The seed is dL/dR
                # (the exposure's transpose applied), so rhs() seeds the back-to-front pass as ever
                check(lib.gslm_lm_residual_exposure(
                    vr.H, vr.W, R.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(),
                    self.model._exposure.data_ptr() + 48 * self.exp_idx[b], self.residuals[b].data_ptr(),
                    self.weights[b].data_ptr(), self.seeds[b].data_ptr(),
                    self._exp_rhs.data_ptr() + 48 * self.exp_idx[b], self._exp_scratch.data_ptr(),
                    self._exp_scratch.numel() * 8, loss.data_ptr(), int(b > 0), self.stream),
                    "gslm_lm_residual_exposure")
                continue
            if self._robust is not None:
                check(lib.gslm_lm_residual_robust(
                    vr.H, vr.W, R.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(),
                    ctypes.byref(self._robust), self.residuals[b].data_ptr(), self.weights[b].data_ptr(),
                    self.seeds[b].data_ptr(), self.res_scratch.data_ptr(), self.res_scratch.numel() * 8,
                    loss.data_ptr(), int(b > 0), self.stream), "gslm_lm_residual_robust")
                continue
            check(lib.gslm_lm_residual(vr.H, vr.W, R.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(),
                                       self.residuals[b].data_ptr(), self.weights[b].data_ptr(),
                                       self.seeds[b].data_ptr(), self.res_scratch.data_ptr(),
                                       self.res_scratch.numel() * 8, loss.data_ptr(), int(b > 0), self.stream),
                  "gslm_lm_residual")
            if dt is not None:  # planes 0-2 above; plane 3 and the loss's depth term (stream order: one scratch)
                off = 12 * vr.H * vr.W
                check(lib.gslm_lm_residual_depth(
                    vr.H, vr.W, vr.invdepth.data_ptr(), dt[0].data_ptr(), None if dt[1] is None else dt[1].data_ptr(),
                    self.depth_weight, self.residuals[b].data_ptr() + off, self.weights[b].data_ptr() + off,
                    self.seeds[b].data_ptr() + off, self.res_scratch.data_ptr(), self.res_scratch.numel() * 8,
                    loss.data_ptr(), 1, self.stream), "gslm_lm_residual_depth")
        self.loss = loss
        return loss

    def num_rendered(self):
        return [v.N for v in self.views]

    # -------------------------------------------------------------- J^T b
    def rhs(self, out, fused=True):
        """out = J^T b = -2 sum_b J_b^T (m (.) 1[0<=R<=1] (.) r_b) in the flat layout (xyz zeroed; exposure zeroed,
        or with train_exposure the rows evaluate() summed: G[i][j] = sum R_i sC_j, G[j][3] = sum sC_j).

        fused: the LM path -- a back-to-front pass seeded with gslm_lm_residual's seed into the LM
        rows, then the LM gather (gslm_matvec_view_ex with pixel_seed); otherwise the drop-in
        gslm_backward (general rows, every parameter group)."""
        g = raw_gaussians(self.model)
        if fused and self.mask_xyz:
            ys = self.layout.grads_struct(out)
            for b, vr in enumerate(self.views):
                opts = self._opts(vr, 2 | 4 | (STAGE_OVERWRITE if b == 0 else 0))  # RENDER | GATHER
                opts.flags |= self._depth_flag(b)
                opts.pixel_seed = self.seeds[b].data_ptr()
                vr.product(g, ys, self.seeds[b].data_ptr(), 1, ys, opts, self.stream, "gslm_matvec_view_ex")
                vr.tail_clean = True
            if not self.views:
                out.zero_()
            e0, e1 = self.layout.offsets["exposure"]
            if self.train_exposure:
                out[e0:e1].copy_(self._exp_rhs)
            else:
                out[e0:e1].zero_()
            return self._mark_rhs(out)
        if self.layout.rest_projected or self.layout.rest_views:
            full = torch.zeros(self.full_layout.numel, dtype=torch.float32, device=self.device)
            self.rhs_full(full)
            return self._mark_rhs(self.project(full, out), fused=False)
        return self._mark_rhs(self.rhs_full(out), fused=False)

    def _depth_flag(self, b):
        """GSLM_MV_DEPTH for a view with a depth term (its weights and seeds are [4, H, W]), else 0."""
        return MV_DEPTH if self.depth[b] is not None else 0

    def _no_depth(self, what):
        if self.depth_weight is not None:
            raise ValueError(f"{what} does not carry the depth residual (depth_weight)")

    def _mark_rhs(self, out, fused=True):
        """Remember the J^T b this problem produced (exposure slice zeroed): cgls_fused may then skip the exposure
        slice's D v in every product without checking it (exposure_is_zero)."""
        self._rhs_token = _lib.tensor_token(out)
        # (the fused gather's J^T b is zero off the view's active list by construction: zero_off_active)
        self._rhs_epochs = [vr.epoch for vr in self.views] if fused else None
        return out

    def exposure_is_zero(self, g):
        """Whether the exposure slice of the right-hand side g is zero, so that every CG iterate's is (without
        train_exposure J has no exposure column): true without a device read for the rhs() this problem produced and
        nobody modified since; otherwise checked on the device (one host sync per solve).  Never with train_exposure."""
        if self.train_exposure:
            return False
        if self.rhs_is_mine(g):
            return True
        e0, e1 = self.layout.offsets["exposure"]
        return not bool(g[e0:e1].any())

    def rhs_is_mine(self, g):
        """g is the J^T b this problem's rhs() produced -- that tensor object itself -- unmodified since."""
        return _lib.token_matches(getattr(self, "_rhs_token", None), g)

    def rhs_full(self, out):
        """J^T b through the drop-in gslm_backward, in the reference's layout (full_layout)."""
        g = raw_gaussians(self.model)
        out.zero_()
        grads = self.full_layout.grads_struct(out, accumulate=True)
        for b, vr in enumerate(self.views):
            dL = self.seeds[b]  # -2 m 1[0 <= R <= 1] r, from gslm_lm_residual (plane 3: the depth block's seed)
            dD = dL.data_ptr() + 12 * vr.H * vr.W if self.depth[b] is not None else None
            check(lib.gslm_backward(ctypes.byref(vr.view), ctypes.byref(g), vr.geom.data_ptr(), vr.binning.data_ptr(),
                                    vr.N, vr.image.data_ptr(), dL.data_ptr(), dD, vr.scratch.data_ptr(),
                                    vr.scratch.numel(), ctypes.byref(grads), self.stream), "gslm_backward")
            vr.tail_clean = False
        self._apply_mask(out, self.full_layout)
        if self.train_exposure:
            e0, e1 = self.full_layout.offsets["exposure"]
            out[e0:e1].copy_(self._exp_rhs)
        return out

    # -------------------------------------------------------------- SH-rest projection (sh_projection)
    def _rest_convert(self, mode, src, dst, src_layout, dst_layout):
        if self.layout.K < 2:
            return
        g = raw_gaussians(self.model)
        a0 = src_layout.offsets["features_rest"][0]
        b0 = dst_layout.offsets["features_rest"][0]
        src_w = 3 * src_layout.shapes["features_rest"][1]
        dst_w = 3 * dst_layout.shapes["features_rest"][1]
        check(lib.gslm_sh_rest_project(ctypes.byref(self.views[0].view), ctypes.byref(g), mode,
                                       src.data_ptr() + 4 * a0, src_w, dst.data_ptr() + 4 * b0, dst_w, self.stream),
              "gslm_sh_rest_project")

    def _copy_other_groups(self, src, dst, src_layout, dst_layout):
        for name in GROUPS:
            if name == "features_rest":
                continue
            a0, a1 = src_layout.offsets[name]
            b0, b1 = dst_layout.offsets[name]
            dst[b0:b1].copy_(src[a0:a1])

    def expand(self, x, out=None):
        """A vector of this problem's layout in the reference's (full_layout); x itself when the layout carries the
        SH-rest group whole (neither projected nor in the batch's coordinates)."""
        if not (self.layout.rest_projected or self.layout.rest_views):
            return x
        out = torch.empty(self.full_layout.numel, dtype=torch.float32, device=x.device) if out is None else out
        self._copy_other_groups(x, out, self.layout, self.full_layout)
        self._rest_convert(0, x, out, self.layout, self.full_layout)
        return out

    def project(self, x_full, out=None):
        """full_layout -> this problem's layout (the orthogonal projection onto the views' SH-rest span)."""
        if not (self.layout.rest_projected or self.layout.rest_views):
            return x_full if out is None else out.copy_(x_full)
        out = torch.empty(self.layout.numel, dtype=torch.float32, device=x_full.device) if out is None else out
        self._copy_other_groups(x_full, out, self.full_layout, self.layout)
        self._rest_convert(1, x_full, out, self.full_layout, self.layout)
        return out

    def _apply_mask(self, vec, layout=None):
        o = (layout or self.layout).offsets
        if self.mask_xyz:
            vec[o["xyz"][0]:o["xyz"][1]].zero_()
        if not self.train_exposure:
            vec[o["exposure"][0]:o["exposure"][1]].zero_()

    # -------------------------------------------------------------- (J^T J + D) v
    def matvec(self, v, y, cg_ctl=None):
        """y = sum_b 2 J_b^T W_b J_b v + D v (fused per view; D v folded into the first view's gather)."""
        self.matvec_dot(v, y, None, cg_ctl=cg_ctl)
        return y

    # cgls_fused may pass exposure_zero=True (see matvec_dot) and the device CG control block (cg_ctl)
    supports_exposure_zero = True
    supports_cg_ctl = True

    def matvec_dot(self, v, y, dot_out, pre=None, exposure_zero=False, cg_ctl=None):
        """matvec, and when possible <v, y> -> device double* dot_out fused into the gather (single
        view; exposure components of v zero, as in every LM iterate).  Returns True if fused.
        pre = (s, beta_num_ptr, beta_den_ptr): first v <- s + beta v (the deferred CG direction
        update), fused into the first view's tangent kernel.
        exposure_zero: the caller guarantees that the exposure components of v (after pre) and of y are
        zero already -- true of every CG iterate (J has no exposure column, x0 = 0, y is the solver's own
        q) -- so y's exposure slice D v = 0 is left as it is (no elementwise launch per product).
        cg_ctl: device pointer of cgls_fused's CG control block (gslm_cg_monitor): once its stopping tests
        have fired the product's kernels return at once (gslm_matvec_opts.cg_ctl).
        With train_exposure nothing is fused (False): the gather's dot covers the Gaussian groups only, and
        <v, y> must include the exposure tail -- the caller takes its own dot over the whole vector."""
        fuse = dot_out is not None and len(self.views) == 1 and not self.train_exposure
        self.local_normal_matvec(v, y, damp=True, dot_out=dot_out if fuse else None, pre=pre,
                                 exposure_zero=exposure_zero, cg_ctl=cg_ctl)
        return fuse

    def local_normal_matvec(self, v, y, damp=False, dot_out=None, pre=None, exposure_zero=False, cg_ctl=None,
                            lean=None):
        """y = [D v +] sum over this problem's views of 2 J_b^T W_b J_b v  (overwrites y).
        pre, exposure_zero, cg_ctl: see matvec_dot.  lean: a GslmCgLean for an active_view()'s one product
        (_cgls_lean: GSLM_MV_LEAN)."""
        g = raw_gaussians(self.model)
        vs = self.layout.grads_struct(v)
        ys = self.layout.grads_struct(y)
        if pre is not None and not self.views:
            self._pre_without_views(v, pre)
            pre = None
        if not self.views:
            y.zero_()
            if damp:
                self.damp_add(v, y)
            return y
        last = len(self.views) - 1
        e0, e1 = self.layout.offsets["exposure"]
        dvec = self._damp_vec() if damp else None
        if dvec is not None and (lean is not None or self.ssim or self.train_exposure):
            raise ValueError("a damping vector runs the plain product (no lean loop, SSIM or trained exposure)")
        for b, vr in enumerate(self.views):
            opts = self._opts(vr, STAGE_ALL | (STAGE_OVERWRITE if b == 0 else 0), cg_ctl)
            opts.flags |= self._depth_flag(b)
            opts.damp7 = self._damps if (damp and b == 0 and dvec is None) else None
            if pre is not None and b == 0:
                ss = self._pre_opts(opts, v, pre)  # noqa: F841  (kept alive for the call)
            fuse = dot_out is not None and b == last
            if fuse or (lean is not None and lean.dot_defer):  # (deferred: <v, y> stays as the gather's partials)
                self._dot_opts(opts, dot_out if fuse else None)
            if self.ssim:
                self._ssim_product(b, vr, g, vs, ys, opts)
                continue
            if self.train_exposure:
                if lean is not None:
                    raise ValueError("the lean CG loop was written for a zero exposure tail")
                opts = self._exposure_opts(opts, b, vr, v, y, e0, damp)
            if dvec is not None and b == 0:  # D v with d per element, on the first view as damp7 is
                opts = _lib.extend_opts(opts, _lib.GslmMatvecOptsDamp, MV_DAMP_VEC)
                ds = self.layout.grads_struct(dvec)  # (kept alive for the call)
                opts.damp_vec = ctypes.addressof(ds)
            self._view_product(vr, g, vs, self.weights[b].data_ptr(), ys, opts, "gslm_matvec_view_ex", lean=lean)
            vr.tail_clean = True
        if self.train_exposure:
            # the batch's cameras' rows are written by their views (above); the other cameras' are D v alone
            if self._exp_rest is not None:
                vt, yt = v[e0:e1].view(-1, 12), y[e0:e1].view(-1, 12)
                yt[self._exp_rest] = vt[self._exp_rest] * (float(self._damps[6]) if damp else 0.0)
        else:
            self._exposure_tail(v, y, damp, exposure_zero)
        return y

    def _exposure_opts(self, opts, b, vr, v, y, e0, damp):
        """View b's options extended by its camera's exposure (GSLM_MV_EXPOSURE): X from the model, V and Y the
        camera's 12 floats of v's and y's exposure tail; the camera's first view writes Y and adds D V."""
        ext = _lib.extend_opts(opts, _lib.GslmMatvecOptsExposure, MV_EXPOSURE)
        k = self.exp_idx[b]
        x = ext.exposure
        x.exposure = self.model._exposure.data_ptr() + 48 * k
        x.v_rows = v.data_ptr() + 4 * (e0 + 12 * k)
        x.y_rows = y.data_ptr() + 4 * (e0 + 12 * k)
        x.color = vr.color.data_ptr()
        x.u_image = self._exp_u[b].data_ptr()
        x.scratch, x.scratch_bytes = self._exp_scratch.data_ptr(), self._exp_scratch.numel() * 8
        x.overwrite = int(self._exp_first[b])
        x.damp = float(self._damps[6]) if (damp and self._exp_first[b]) else 0.0
        return ext

    def _view_product(self, vr, g, vs, weight, ys, opts, what, lean=None):
        """ViewRaster.product of this problem on one view: on an active_view() (v and y hold the listed Gaussians
        only) the active-list form, with the lean loop's options when lean is given (GSLM_MV_LEAN)."""
        if lean is not None:
            opts = _lib.extend_opts(opts, _lib.GslmMatvecOptsLean, MV_LEAN)
            opts.lean = lean
        vr.product(g, vs, weight, int(self.mask_xyz), ys, opts, self.stream, what, active=self._active)

    def _pre_without_views(self, v, pre):
        s, num, den = pre[:3]
        if len(pre) > 3 and pre[3] is not None:
            x, anum, aden = pre[3:]
            check(lib.gslm_axpy_dev(v.numel(), anum, aden, 1.0, v.data_ptr(), x.data_ptr(), self.stream),
                  "gslm_axpy_dev")
        check(lib.gslm_xpby_dev(v.numel(), s.data_ptr(), num, den, v.data_ptr(), self.stream), "gslm_xpby_dev")

    def _ssim_product(self, b, vr, g, vs, ys, opts):
        """One view's J^T J v with the SSIM residual: J v (jv_out) -> image-space factor
        M (d1^2 + S^T c2^2 S) M (gslm_ssim_normal) -> seeded back-to-front pass + LM gather.
        opts carries this view's gather options (overwrite, damping, dot) and the fused xpby."""
        jv, u = self._jv[b], self._u[b]
        o1 = self._opts(vr, 1 | 2, opts.cg_ctl)  # TANGENT | RENDER (the flags are read by the active-list form only)
        o1.jv_out = jv.data_ptr()
        for f in ("xpby_s", "beta_num", "beta_den", "xpby_tail_v", "xpby_tail_s", "xpby_tail_n", "alpha_num",
                  "alpha_den", "xpby_x_offset"):
            setattr(o1, f, getattr(opts, f))
        self._view_product(vr, g, vs, jv.data_ptr(), ys, o1, "gslm_matvec_view_ex(jv)")
        check(lib.gslm_ssim_normal(vr.H, vr.W, self.gts[b].data_ptr(), self.ssim_state[b].data_ptr(), jv.data_ptr(),
                                   u.data_ptr(), self.stream), "gslm_ssim_normal")
        o2 = self._opts(vr, 2 | 4 | (opts.stages & STAGE_OVERWRITE), opts.cg_ctl)  # RENDER | GATHER
        o2.pixel_seed = u.data_ptr()
        for f in ("damp7", "dot_vy", "dot_scratch", "dot_scratch_bytes"):
            setattr(o2, f, getattr(opts, f))
        self._view_product(vr, g, vs, u.data_ptr(), ys, o2, "gslm_matvec_view_ex(seed)")
        vr.tail_clean = True

    # -------------------------------------------------------------- view-sharded exchange (gslm.parallel)
    def views_for(self, cams, pad_to=None):
        """ctypes array of the gslm_view of every camera in `cams` (the whole sharded batch), padded
        with copies of the last to `pad_to` entries (padded slots carry no screen data)."""
        vs = [_lib.view_from_camera(c, self.bg, self.model.active_sh_degree) for c in cams]
        vs += [vs[-1]] * max(0, (pad_to or len(vs)) - len(vs))
        arr = (_lib.GslmView * len(vs))()
        for k, vw in enumerate(vs):
            arr[k] = vw
        return arr

    def screen_products(self, v, screen, pre=None, cg_ctl=None):
        """screen[b] = this rank's view b's per-Gaussian screen-space sums S_b^T W_b J_b v (P x 8,
        GSLM_STAGE_SCREEN); pre as in matvec_dot (applied with the first view)."""
        if self.train_exposure:
            raise ValueError("the sharded exchanges do not carry trained exposure")
        self._no_depth("the sharded exchange")
        g = raw_gaussians(self.model)
        vs = self.layout.grads_struct(v)
        ys = self.layout.grads_struct(v)  # unused by the SCREEN stage
        e0, e1 = self.layout.offsets["exposure"]
        if pre is not None and not self.views:
            self._pre_without_views(v, pre)
        for b, vr in enumerate(self.views):
            opts = self._opts(vr, 1 | 2 | 16, cg_ctl)  # TANGENT | RENDER | SCREEN
            opts.screen_out = screen[b].data_ptr()
            if pre is not None and b == 0:
                ss = self._pre_opts(opts, v, pre)  # noqa: F841
            vr.product(g, vs, self.weights[b].data_ptr(), 1, ys, opts, self.stream, "gslm_matvec_view_ex")
            vr.tail_clean = True

    def gather_screen(self, views, screen_all, v, y, dot_out=None, chunk=16):
        """y = sum over all views b of C_b^T screen_all[b] + D v (exposure: D v only); <v, y> fused
        into dot_out when given."""
        g = raw_gaussians(self.model)
        vs = self.layout.grads_struct(v)
        ys = self.layout.grads_struct(y)
        n = len(views)
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            opts = _lib.GslmMatvecOpts()
            opts.stages = (STAGE_ALL | STAGE_OVERWRITE) if c0 == 0 else STAGE_ALL
            opts.damp7 = self._damps if c0 == 0 else None
            if dot_out is not None and c1 == n:
                self._dot_opts(opts, dot_out)
            check(lib.gslm_gather_screen(_lib.view_ptr(views, c0), c1 - c0, ctypes.byref(g),
                                         screen_all[c0].data_ptr(), ctypes.byref(vs), ctypes.byref(ys),
                                         ctypes.byref(opts), self.stream), "gslm_gather_screen")
        self._exposure_tail(v, y)
        return y

    def damp_add(self, v, y):
        dvec = self._damp_vec()
        if dvec is not None:
            y.addcmul_(dvec, v)
            return
        check(lib.gslm_damp_add(v.numel(), v.data_ptr(), self._bounds, self._damps, 7, y.data_ptr(), self.stream))

    # -------------------------------------------------------------- the damping vector (damping="marquardt")
    def _damp_vec(self):
        """The damping vector of this problem's products, or None (D is the seven constants): Marquardt's, built on
        first use after an evaluate(), or the one set_damping_vector holds."""
        if self._dvec is None and self.damping == "marquardt":
            self._dvec = self._marquardt_scale(self.diagonal(damp=False))
        return self._dvec

    def _marquardt_scale(self, diag, out=None):
        """lambda[group] max(diag, floor) (gslm_marquardt_scale); in place without `out`."""
        out = diag if out is None else out
        check(lib.gslm_marquardt_scale(diag.numel(), diag.data_ptr(), self._bounds, self._damps, 7,
                                       self.marquardt_floor, out.data_ptr(), self.stream), "gslm_marquardt_scale")
        return out

    def damping_vector(self):
        """The per-element damping d of the products (this problem's layout), or None under the seven constants.
        Under damping="marquardt" it needs a current evaluate() and is the vector the next solve uses."""
        return self._damp_vec()

    def set_damping_vector(self, d):
        """D = diag(d) for a caller-supplied d >= 0 in this problem's layout (a per-parameter trust region) in place
        of the seven constants or of Marquardt's vector; None returns to them.  The products, damp_add, the exposure
        tail, diagonal(damp=True) and the active list use it; the lean CG loop does not run.  Held until replaced --
        under damping="marquardt" until the next evaluate().  The plain residual on the LM rows of LMProblem only."""
        if d is None:
            self._dvec = None
            return
        self._no_depth("set_damping_vector")
        if self.ssim or self.train_exposure or not self.mask_xyz or self.layout.rest_views or self._active is not None:
            raise ValueError("set_damping_vector: the [r; r] residual on the LM rows of LMProblem (mask_xyz=True, no "
                             "SSIM, no trained exposure, not the batched problem or an active view)")
        if (not torch.is_tensor(d) or d.dtype != torch.float32 or d.shape != (self.layout.numel,) or
                not d.is_contiguous() or d.device != torch.zeros(0, device=self.device).device):
            raise ValueError(f"set_damping_vector: a contiguous float32 vector of {self.layout.numel} elements on "
                             f"{self.device}")
        if bool((d < 0).any()):
            raise ValueError("set_damping_vector: D must be >= 0")
        self._dvec = d

    # -------------------------------------------------------------- residual-space J and J^T (cgls_residual)
    def residual_masks(self):
        """Per view m (.) 1[0 <= R <= 1]: the Jacobian of r = m clamp01(R) - gt w.r.t. the render R."""
        out = []
        for b, vr in enumerate(self.views):
            R = vr.color
            inside = ((R >= 0) & (R <= 1)).to(torch.float32)
            m = self.masks[b]
            out.append(inside if m is None else inside * m.to(torch.float32).reshape(1, vr.H, vr.W))
        return out

    def jv_residual(self, v, rmasks, out):
        """out[b] = J_r,b v = m 1[0 <= R <= 1] (.) (d R_b / d theta) v  (the `matvec` of solver_functions.py:83-93,
        one copy of the [r; r] pair)."""
        if self.ssim or self.train_exposure:
            raise ValueError("jv_residual: the disable_ssim residual without trained exposure only")
        self._no_depth("jv_residual (the residual-space recursion)")
        g = raw_gaussians(self.model)
        vs = self.layout.grads_struct(v)
        for b, vr in enumerate(self.views):
            opts = _lib.GslmMatvecOpts()
            opts.stages = 1 | 2  # TANGENT | RENDER with jv_out: the colour tangent
            opts.flags = self.mv_flags
            opts.jv_out = out[b].data_ptr()
            vr.product(g, vs, out[b].data_ptr(), 1, vs, opts, self.stream, "gslm_matvec_view_ex(jv)")
            out[b].mul_(rmasks[b])
        return out

    def jt_residual(self, r, rmasks, out):
        """out = J^T [r; r] = 2 sum_b J_r,b^T r_b (the `matvec_T` of solver_functions.py:101-132), xyz and exposure
        groups zero.  Overwrites out."""
        if self.train_exposure:
            raise ValueError("jt_residual: the residual-space recursion does not carry trained exposure")
        self._no_depth("jt_residual (the residual-space recursion)")
        g = raw_gaussians(self.model)
        ys = self.layout.grads_struct(out)
        for b, vr in enumerate(self.views):
            seed = (2.0 * rmasks[b]) * r[b]
            opts = self._opts(vr, 2 | 4 | (STAGE_OVERWRITE if b == 0 else 0))  # RENDER | GATHER, seeded
            opts.pixel_seed = seed.data_ptr()
            vr.product(g, ys, seed.data_ptr(), 1, ys, opts, self.stream, "gslm_matvec_view_ex(seed)")
            vr.tail_clean = True
        if not self.views:
            out.zero_()
        self._apply_mask(out)
        return out

    # -------------------------------------------------------------- the active set (cgls_fused)
    _active = None  # (ids, Pa) on an active_view(): the layout's rows are the listed Gaussians

    def active_view(self):
        """This problem restricted to the Gaussians its one view can move (ViewRaster.active_list): a shallow copy
        whose layout is ParamLayout(Pa, ...) and whose products run gslm_matvec_view_active on the shared geometry.
        A Gaussian off the list has an exactly zero column of J, so A = J^T W J + D is D there, and a CG solve from
        x0 = 0 whose right-hand side is zero off the list keeps every vector exactly zero there: the solve on the
        listed rows is the same solve (either residual: the SSIM product runs the same per-Gaussian stages).  pack /
        unpack convert flat vectors.  None when it does not apply (several views, xyz unmasked, no current row
        map, nothing visible)."""
        if len(self.views) != 1 or not self.mask_xyz or self._active is not None:
            return None
        vr = self.views[0]
        if not vr.tail_clean or vr.N is None:
            return None
        ids, na = vr.active_list(self.layout.P, self.stream)
        if na == 0:
            return None  # (every vector of the solve is the exposure tail alone: nothing to save)
        return self._restricted(ids, na)

    def _restricted(self, ids, na):
        """The shallow copy of this problem whose vectors hold the na listed Gaussians only: the same layout kind
        over na rows, the damping arrays at its offsets."""
        act = copy.copy(self)
        act._active = (ids, na)
        act._full = self
        lay = self.layout
        act.layout = ParamLayout(na, lay.K, lay.n_exposure, rest_projected=lay.rest_projected,
                                 rest_views=lay.rest_views)
        act._bounds, act._damps = act.layout.group_damp_arrays(self.damp)
        dvec = self._damp_vec()
        if dvec is not None:
            act._dvec = act.pack(dvec)  # (once per solve: the listed rows of d)
        return act

    def _pack_args(self):
        lay = self._full.layout
        widths = [3, 3, 3 * lay.rest_rows if lay.K > 1 else 0, 3, 4, 1]
        return (ctypes.c_int32 * 6)(*widths), 6, lay.offsets["exposure"][1] - lay.offsets["exposure"][0]

    def pack(self, full):
        """The listed rows of a flat vector of the full problem's layout, in this view's layout."""
        ids, na = self._active
        w, n, tail = self._pack_args()
        out = torch.empty(self.layout.numel, dtype=torch.float32, device=full.device)
        check(lib.gslm_active_pack(full.data_ptr(), out.data_ptr(), ids.data_ptr(), na, self._full.layout.P, w, n, tail,
                                   self.stream), "gslm_active_pack")
        return out

    def unpack(self, vec):
        """A vector of this view's layout in the full problem's (zero off the list)."""
        ids, na = self._active
        w, n, tail = self._pack_args()
        out = torch.empty(self._full.layout.numel, dtype=torch.float32, device=vec.device)
        check(lib.gslm_active_unpack(vec.data_ptr(), out.data_ptr(), ids.data_ptr(), na, self._full.layout.P, w, n,
                                     tail, self.stream), "gslm_active_unpack")
        return out

    def zero_off_active(self, g):
        """Whether the full-layout right-hand side g is zero on every Gaussian off the list: true without a device
        read for the rhs() this problem produced and nobody modified since (the fused gather sums no rows for those
        Gaussians); otherwise checked on the device (one read-back)."""
        full = self._full
        if full.rhs_is_mine(g) and full._rhs_epochs == [vr.epoch for vr in full.views]:
            return True
        ids, na = self._active
        off = torch.ones(full.layout.P, dtype=torch.bool, device=g.device)
        off[ids.long()] = False
        for name, v in full.layout.views(g).items():
            if name != "exposure" and v.numel() and bool((v.reshape(full.layout.P, -1)[off] != 0).any()):
                return False
        return True

    # -------------------------------------------------------------- device scalar algebra
    def dot(self, a, b, out_slot, damped=False):
        if damped:
            check(lib.gslm_dot(a.data_ptr(), b.data_ptr(), self._bounds, self._damps, 7, a.numel(),
                               self.dot_scratch.data_ptr(), out_slot, self.stream))
        else:
            check(lib.gslm_dot(a.data_ptr(), b.data_ptr(), None, None, 0, a.numel(), self.dot_scratch.data_ptr(),
                               out_slot, self.stream))

    def zeros(self):
        return torch.zeros(self.layout.numel, dtype=torch.float32, device=self.device)

    # -------------------------------------------------------------- diag(J^T W J + D)  (cgls_jacobi)
    def diagonal(self, out=None, damp=True):
        """out = diag(sum_b 2 J_b^T W_b J_b [+ D]) in this problem's layout (projected when sh_projection selected
        it, else the reference's): gslm_lm_diag_view per view, the first overwriting and the others accumulating, D
        added once; the exposure tail is D alone.  Needs a current evaluate() (the weights); reuses each view's LM row
        map when it has one and builds it otherwise (the products after it then reuse it).  The plain residual on the
        LM rows only: ValueError with mask_xyz=False, ssim, train_exposure, or the batched problem's coordinates.
        With a damping vector (damping="marquardt", set_damping_vector) damp=True adds d: diag + d."""
        self._no_depth("diagonal (cgls_jacobi, Marquardt damping)")
        if (not self.mask_xyz or self.ssim or self.train_exposure or self.layout.rest_views or
                self._active is not None):
            raise ValueError("diagonal: the [r; r] residual on the LM rows (mask_xyz=True, no SSIM, no trained "
                             "exposure), in the full or the single-view projected layout")
        if any(w is None for w in self.weights):
            raise RuntimeError("diagonal: no current evaluate() (the per-pixel weights)")
        out = torch.empty(self.layout.numel, dtype=torch.float32, device=self.device) if out is None else out
        if damp and (self._dvec is not None or self.damping == "marquardt"):
            # D = diag(d): the diagonal of the matrix the products apply is diag + d
            self.diagonal(out, damp=False)
            if self._dvec is None:
                self._dvec = self._marquardt_scale(out, torch.empty_like(out))
            return out.add_(self._dvec)
        g = raw_gaussians(self.model)
        ys = self.layout.grads_struct(out)
        for b, vr in enumerate(self.views):
            flags = ((DIAG_TAIL_CLEAN if vr.tail_clean else 0) | (DIAG_ACCUMULATE if b else 0) |
                     (DIAG_SH_REST_PROJECTED if self.layout.rest_projected else 0))
            check(lib.gslm_lm_diag_view(ctypes.byref(vr.view), ctypes.byref(g), self.weights[b].data_ptr(), 1,
                                        vr.geom.data_ptr(), vr.binning.data_ptr(), vr.N, vr.image.data_ptr(),
                                        vr.scratch.data_ptr(), vr.scratch.numel(), ctypes.byref(ys),
                                        self._damps if (damp and b == 0) else None, flags, self.stream),
                  "gslm_lm_diag_view")
            vr.tail_clean = True
        if not self.views:
            for k, name in enumerate(GROUPS[:6]):
                o0, o1 = self.layout.offsets[name]
                out[o0:o1].fill_(float(self._damps[k]) if damp else 0.0)
        e0, e1 = self.layout.offsets["exposure"]
        out[e0:e1].fill_(float(self._damps[6]) if damp else 0.0)
        return out


class BatchedLMProblem(LMProblem, _StageTimes):
    """LMProblem over several views with one batched pass per product and per J^T b on one GPU (the reference's
    view batch, train_jvp.py --num_images): where LMProblem runs the whole fused product once per view -- the
    per-Gaussian tangent kernel over all P, and a gather that re-reads and re-writes all of y, V times -- this runs
      gslm_tangent_views   every view's tangent records in one pass over theta and p (per 16 views), with the fused
                           direction update and deferred x update of cgls_fused;
      RENDER (trec_in)     each view's fused J v -> J^T tile pass into its own head rows;
      gslm_gather_views    every view's row sums and chain per Gaussian, D v and <v, y>, y written once (per 16 views).
    With V <= GSLM_MAX_REST_VIEWS views (and 3 V < 3 (K - 1)) the SH-rest group of every vector is carried in the 3 V
    gslm_rest_basis coordinates of the views' span (GSLM_SHARD_REST=full keeps the reference's layout); `expand` /
    `project` convert to and from `full_layout`.  The forwards, residuals and the loss are LMProblem's own.
    mask_xyz=True and the disable_ssim residual only; BatchedXyzLMProblem is the batch with the positions free.

    With the positions free (BatchedXyzLMProblem, mask_xyz=False) the tangent records are [V][P][12],
    each view's RENDER stage runs unmasked into 48-byte head rows and the gather sets GSLM_MV_XYZ: the chain includes the means and
    y's xyz group is written with the others.  J is evaluated at the current theta, so the SH-rest coordinates stay
    valid.  rhs() is LMProblem's unmasked route (gslm_backward, then `project`), which drops the views' row maps: the
    first product rebuilds them.  ValueError with union_active=True (the list's kernels are masked forms) and, as on
    LMProblem, with robust."""

    XYZ_FREE = False  # (BatchedXyzLMProblem: True)

    CHUNK = 16  # views per gslm_tangent_views / gslm_gather_views call
    STAGES = ("tangent_views", "tile_passes", "gather_views")  # (_StageTimes.stage_times)

    def __init__(self, model, cams, bg, gts=None, alpha_masks=None, mask_xyz=True, damp=None, device="cuda",
                 ssim=False, lambda_dssim=0.2, sh_projection=False, union_active=False, damping="fixed",
                 marquardt_floor=0.0, robust=None, depth_weight=None, invdepths=None, depth_masks=None):
        if depth_weight is not None or invdepths is not None or depth_masks is not None:
            raise ValueError("BatchedLMProblem does not carry the depth residual (depth_weight is LMProblem's)")
        if damping != "fixed" or marquardt_floor != 0.0:
            raise ValueError("BatchedLMProblem runs the fixed damping (damping='marquardt' is LMProblem's)")
        if bool(mask_xyz) == self.XYZ_FREE:
            raise ValueError("BatchedLMProblem runs on the LM rows (mask_xyz=True, train_jvp.py:221-227) and "
                             "BatchedXyzLMProblem with the positions free (mask_xyz=False)")
        if not mask_xyz and union_active:
            raise ValueError("BatchedXyzLMProblem runs on all P Gaussians: union_active=True needs mask_xyz=True "
                             "(gslm_tangent_views_active / gslm_gather_views_active are masked forms)")
        if ssim:
            raise ValueError("BatchedLMProblem runs the disable_ssim residual")
        if len(cams) < 1:
            raise ValueError("BatchedLMProblem needs at least one view")
        if sh_projection not in (False, None, "auto"):
            raise ValueError("sh_projection is LMProblem's single-view mode; the batch carries SH-rest coordinates")
        super().__init__(model, cams, bg, gts=gts, alpha_masks=alpha_masks, mask_xyz=mask_xyz, damp=damp,
                         device=device, ssim=False, lambda_dssim=lambda_dssim, sh_projection=False, robust=robust)
        full = self.full_layout
        P, K, V = full.P, full.K, len(cams)
        self.rest_views = V if (K > 1 and V <= _lib.GSLM_MAX_REST_VIEWS and 3 * V < 3 * (K - 1)
                                and os.environ.get("GSLM_SHARD_REST", "coords") != "full") else 0
        if self.rest_views:
            self.layout = ParamLayout(P, K, full.n_exposure, rest_views=self.rest_views)
            self._bounds, self._damps = self.layout.group_damp_arrays(self.damp)
        self._views_arr = (_lib.GslmView * V)(*[vr.view for vr in self.views])
        # allocated once: every view's visibility words and tangent records, the SH-rest factors
        self._flags = torch.zeros(V, max(P, 1), dtype=torch.int32, device=device)
        self._trec_w = 8 if self.mask_xyz else 12  # floats per tangent record (gslm_tangent_views)
        self._trec = torch.zeros(V, max(P, 1), self._trec_w, dtype=torch.float32, device=device)
        rv = self.rest_views
        self._rest_n = P * rv * (rv + 1) // 2  # floats gslm_rest_basis writes
        self._rest_R = torch.zeros((self._rest_n + 255) // 256 * 256, dtype=torch.float32,
                                   device=device) if rv else None
        self._rest_ok = False
        self.union_active = bool(union_active)
        self._union = None  # (the views' epochs, ids, Pa, hrow, aflags): the union list of the current geometry

    def union_list(self):
        """(ids, Pa, hrow, aflags) of gslm_active_union: the ascending int32 ids of the Gaussians that own a head row
        in at least one view's LM row map, their number, every view's row offsets of the list ([V][P + 1]) and every
        view's gslm_view_flags words in list order ([V][P]).  Needs every view's row map (tail_clean: a product or
        rhs() on this geometry); built once per geometry (one read-back), kept until a view's forward or backward."""
        if any(not vr.tail_clean or vr.N is None for vr in self.views):
            self._union = None  # (the list is the row maps': it lives exactly as long)
            raise RuntimeError("union_list: a view has no current LM row map (run a product or rhs() first)")
        key = [vr.epoch for vr in self.views]
        if self._union is None or self._union[0] != key:
            V, P, dev = len(self.views), self.full_layout.P, self.device
            ids = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
            hrow = torch.empty(V, P + 1, dtype=torch.int32, device=dev)
            aflags = torch.empty(V, max(P, 1), dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            work = _lib.u8(lib.gslm_active_union_bytes(P), dev)
            check(lib.gslm_active_union(self._view_ws(0, V), V, P, work.data_ptr(), work.numel(), ids.data_ptr(),
                                        hrow.data_ptr(), aflags.data_ptr(), count.data_ptr(), self.stream),
                  "gslm_active_union")
            n = int(count.item())
            self._union = (key, ids[:n], n, hrow, aflags)
        return self._union[1:]

    def active_view(self):
        """With union_active=True: this problem restricted to the Gaussians at least one of its views can move
        (union_list; LMProblem.active_view's argument holds for the union, and the SH-rest coordinates are per
        Gaussian): a shallow copy whose layout is ParamLayout(Pa, ..., rest_views) and whose products run
        gslm_tangent_views_active / gslm_gather_views_active on the shared geometries.  None by default, without a
        current row map in every view, with nothing visible, and with GSLM_CG_ACTIVE=0."""
        if not self.union_active or self._active is not None or os.environ.get("GSLM_CG_ACTIVE", "1") == "0":
            return None
        if any(not vr.tail_clean or vr.N is None for vr in self.views):
            self._union = None
            return None
        ids, na, hrow, aflags = self.union_list()
        if na == 0:
            return None  # (every vector of the solve is the exposure tail alone: nothing to save)
        act = self._restricted(ids, na)
        act._union_bufs = (hrow, aflags)
        return act

    def evaluate(self):
        """LMProblem.evaluate (the same forwards and residual epilogues: the same loss bits); then, once per geometry,
        every view's visibility words; the SH-rest factors of the new geometry are recomputed on first use."""
        loss = super().evaluate()
        P = self.layout.P
        for b, vr in enumerate(self.views):
            check(lib.gslm_view_flags(vr.geom.data_ptr(), P, self._flags[b].data_ptr(), self.stream),
                  "gslm_view_flags")
        self._rest_ok = False
        return loss

    def _view_ws(self, c0, c1):
        ws = (_lib.GslmViewWs * (c1 - c0))()
        for k, vr in enumerate(self.views[c0:c1]):
            ws[k].geom, ws[k].scratch = vr.geom.data_ptr(), vr.scratch.data_ptr()
            ws[k].scratch_bytes, ws[k].num_rendered = vr.scratch.numel(), vr.N
        return ws

    def rest_basis(self):
        """gslm_rest_basis of the batch's views on the current geometry (None in the full layout)."""
        if not self.rest_views:
            return None
        if self._active is not None:
            return self._full.rest_basis()  # (the factors are the scene's [P]: the list's kernels read them by id)
        if not self._rest_ok:
            g = raw_gaussians(self.model)
            check(lib.gslm_rest_basis(self._views_arr, self.rest_views, ctypes.byref(g), self._rest_R.data_ptr(),
                                      self.stream), "gslm_rest_basis")
            self._rest_ok = True
        return self._rest_R

    # -------------------------------------------------------------- SH-rest coordinates
    def _rest_convert(self, mode, src, dst, src_layout, dst_layout):
        """gslm_rest_coords between the rest groups of two flat vectors (mode 0 expand, 1 project)."""
        g = raw_gaussians(self.model)
        a0 = src_layout.offsets["features_rest"][0]
        b0 = dst_layout.offsets["features_rest"][0]
        check(lib.gslm_rest_coords(self._views_arr, self.rest_views, ctypes.byref(g), self.rest_basis().data_ptr(),
                                   mode, src.data_ptr() + 4 * a0, 3 * src_layout.rest_rows, dst.data_ptr() + 4 * b0,
                                   3 * dst_layout.rest_rows, self.stream), "gslm_rest_coords")

    # -------------------------------------------------------------- the batched passes
    def _gather(self, g, vs, ys, damp, dot_out, cg_ctl):
        """gslm_gather_views over the views' head rows: y = [D v +] sum_b C_b^T rows_b, <v, y> with the last chunk."""
        V = len(self.views)
        R = self.rest_basis()
        for c0 in range(0, V, self.CHUNK):
            c1 = min(V, c0 + self.CHUNK)
            opts = _lib.GslmMatvecOpts()
            opts.stages = STAGE_ALL | (STAGE_OVERWRITE if c0 == 0 else 0)
            opts.damp7 = self._damps if (damp and c0 == 0) else None
            opts.cg_ctl = cg_ctl
            if not self.mask_xyz:
                opts.flags |= MV_XYZ  # the views' head rows are the unmasked RENDER stage's
            if R is not None:
                opts.rest_basis, opts.rest_views, opts.view_base = R.data_ptr(), self.rest_views, c0
            if dot_out is not None and c1 == V:
                self._dot_opts(opts, dot_out)
            vptr, ws = _lib.view_ptr(self._views_arr, c0), self._view_ws(c0, c1)
            if self._active is not None:  # v and y hold the union list's Gaussians only
                (ids, na), (hrow, aflags) = self._active, self._union_bufs
                P = self._full.full_layout.P
                check(lib.gslm_gather_views_active(vptr, ws, c1 - c0, ctypes.byref(g), ctypes.byref(vs),
                                                   ctypes.byref(ys), ids.data_ptr(), na,
                                                   hrow.data_ptr() + 4 * c0 * (P + 1), P + 1,
                                                   aflags.data_ptr() + 4 * c0 * P, P, ctypes.byref(opts), self.stream),
                      "gslm_gather_views_active")
                continue
            check(lib.gslm_gather_views(vptr, ws, c1 - c0, ctypes.byref(g), ctypes.byref(vs),
                                        ctypes.byref(ys), ctypes.byref(opts), self.stream), "gslm_gather_views")

    def rhs(self, out, fused=True):
        """out = J^T b in this problem's layout (xyz, exposure zeroed): per view the seeded back-to-front pass into
        its head rows, then one gslm_gather_views -- in coordinates it writes the coordinates of J^T b directly.
        mask_xyz=False: the seeded pass is a masked form, so J^T b is LMProblem's unmasked route -- gslm_backward into
        the reference's layout, then `project`; it drops the views' row maps (tail_clean False) and the first product
        rebuilds them."""
        if not self.mask_xyz:
            return LMProblem.rhs(self, out, fused=False)
        g = raw_gaussians(self.model)
        ys = self.layout.grads_struct(out)
        for b, vr in enumerate(self.views):
            opts = self._opts(vr, 2)  # RENDER, seeded
            opts.pixel_seed = self.seeds[b].data_ptr()
            vr.product(g, ys, self.seeds[b].data_ptr(), 1, ys, opts, self.stream, "gslm_matvec_view_ex(seed)")
            vr.tail_clean = True
        self._gather(g, ys, ys, False, None, None)
        e0, e1 = self.layout.offsets["exposure"]
        out[e0:e1].zero_()
        return self._mark_rhs(out)

    def matvec_dot(self, v, y, dot_out, pre=None, exposure_zero=False, cg_ctl=None):
        """LMProblem.matvec_dot; <v, y> is fused into the gather for any number of views (True with dot_out)."""
        self.local_normal_matvec(v, y, damp=True, dot_out=dot_out, pre=pre, exposure_zero=exposure_zero,
                                 cg_ctl=cg_ctl)
        return dot_out is not None

    def local_normal_matvec(self, v, y, damp=False, dot_out=None, pre=None, exposure_zero=False, cg_ctl=None):
        """y = [D v +] sum_b 2 J_b^T W_b J_b v (overwrites y); pre, exposure_zero, cg_ctl: see LMProblem.matvec_dot."""
        g = raw_gaussians(self.model)
        vs = self.layout.grads_struct(v)
        ys = self.layout.grads_struct(y)
        V, P = len(self.views), self._flags.shape[1]
        R = self.rest_basis()
        keep = []
        self._mark(0)
        # 1. every view's tangent records, one pass over the Gaussians per chunk (the direction update with the first)
        for c0 in range(0, V, self.CHUNK):
            c1 = min(V, c0 + self.CHUNK)
            opts = None
            if (pre is not None and c0 == 0) or R is not None or cg_ctl is not None:
                opts = _lib.GslmMatvecOpts()
                opts.cg_ctl = cg_ctl
                if pre is not None and c0 == 0:
                    keep.append(self._pre_opts(opts, v, pre))
                if R is not None:
                    opts.rest_basis, opts.rest_views, opts.view_base = R.data_ptr(), self.rest_views, c0
            vptr = _lib.view_ptr(self._views_arr, c0)
            if self._active is not None:  # v (and s, x of pre) hold the union list's Gaussians only
                (ids, na), aflags = self._active, self._union_bufs[1]
                check(lib.gslm_tangent_views_active(vptr, c1 - c0, ctypes.byref(g), ctypes.byref(vs), 1,
                                                    ids.data_ptr(), na, aflags.data_ptr() + 4 * c0 * P, P,
                                                    self._trec.data_ptr() + 32 * c0 * P, P,
                                                    None if opts is None else ctypes.byref(opts), self.stream),
                      "gslm_tangent_views_active")
                continue
            check(lib.gslm_tangent_views(vptr, c1 - c0, ctypes.byref(g), ctypes.byref(vs), int(self.mask_xyz),
                                         self._flags.data_ptr() + 4 * c0 * P, P,
                                         self._trec.data_ptr() + 4 * self._trec_w * c0 * P, P,
                                         None if opts is None else ctypes.byref(opts), self.stream),
                  "gslm_tangent_views")
        self._mark(1)
        # 2. each view's tile pass from its slice of the table, into its own head rows
        for b, vr in enumerate(self.views):
            opts = self._opts(vr, 2, cg_ctl)  # RENDER
            opts.trec_in = self._trec[b].data_ptr()
            vr.product(g, vs, self.weights[b].data_ptr(), int(self.mask_xyz), vs, opts, self.stream,
                       "gslm_matvec_view_ex")
            vr.tail_clean = True
        self._mark(2)
        # 3. every view's row sums and chain per Gaussian, y written once per chunk
        self._gather(g, vs, ys, damp, dot_out, cg_ctl)
        self._mark(3)
        self._exposure_tail(v, y, damp, exposure_zero)
        return y


class BatchedXyzLMProblem(BatchedLMProblem):
    """BatchedLMProblem with the positions free: xyz is a group of unknowns like the others (the reference keeps
    xyz_damp = 5e2 in GaussianModelDampMatrix for it).  Same passes per product -- one gslm_tangent_views, V tile
    passes, one gslm_gather_views -- in their unmasked forms (see BatchedLMProblem); the SH-rest coordinates apply
    unchanged.  mask_xyz must be False; union_active=True, robust, depth_weight, Marquardt damping and SSIM raise
    ValueError, and diagonal() / cgls_jacobi refuse the problem, as they refuse LMProblem(mask_xyz=False)."""

    XYZ_FREE = True

    def __init__(self, model, cams, bg, gts=None, alpha_masks=None, mask_xyz=False, **kw):
        super().__init__(model, cams, bg, gts=gts, alpha_masks=alpha_masks, mask_xyz=mask_xyz, **kw)


class NonFiniteError(AssertionError):
    """A NaN or Inf reached the normal equations.  The reference's only failure detection on the LM path is
    matvec_T's `assert not torch.isnan(self.gaussians._<group>.grad).any(), "NaN detected in gaussians._<group>.grad"`
    (solver/solver_functions.py:125-130), which aborts the step before the parameters move; this is raised at the
    same point of the fused solve (an AssertionError, with the reference's message), before update_params."""


CG_STOP_NONFINITE = 4  # gslm_cg_monitor's stop code (include/gslm.h GSLM_CG_STOP_NONFINITE)


def raise_nonfinite(prob, g, what="the normal-equations product (J^T J + D) p"):
    """Raises NonFiniteError naming the parameter groups of J^T b (= g) that hold a NaN / Inf, as the reference's
    asserts do; when J^T b is finite the failure came later in the solve (a product or the iterate)."""
    names = []
    try:
        for k, v in prob.layout.views(g).items():
            if k != "exposure" and v.numel() and not bool(torch.isfinite(v).all()):
                names.append(k)
    except (AttributeError, RuntimeError, TypeError):
        pass
    if names:
        raise NonFiniteError("; ".join(f"NaN detected in gaussians._{k}.grad" for k in names))
    raise NonFiniteError(f"NaN detected in {what} during CGLS (J^T b is finite)")


def _active_view_for(prob, g, callback):
    """The active-set view of cgls_fused's problem (LMProblem.active_view) when the solve may run on it, else None."""
    if callback is not None or os.environ.get("GSLM_CG_ACTIVE", "1") == "0":
        return None
    local = prob
    if not isinstance(local, LMProblem):
        from gslm import parallel
        # a view-sharded operator without collectives delegates every product to its local problem
        if not (isinstance(local, parallel.ShardedOperator) and not parallel.collectives_on(local.world_size)):
            return None
        local = local.local
        if not isinstance(local, LMProblem):
            return None
    if g.numel() != local.layout.numel:
        return None
    act = local.active_view()
    if act is None or not act.zero_off_active(g):
        return None
    return act


def _lean_applies(act, check_every, max_iter):
    """Whether cgls_fused's solve on the active view `act` takes the lean loop (_cgls_lean): benchmark mode (no
    stopping tests), the plain residual, scalars that stay on this device.  GSLM_CG_LEAN=0 keeps the loop below (the switch exists for A/B runs)."""
    if isinstance(act, BatchedLMProblem):
        return False  # (the lean loop is the single view's: act.views[0], its parameter block)
    if getattr(act, "train_exposure", False):
        return False  # (the lean kernels were written for a zero exposure tail)
    if getattr(act, "_dvec", None) is not None or getattr(act, "damping", "fixed") != "fixed":
        return False  # (a damping vector: the lean gather reads the seven constants)
    return (not check_every and max_iter >= 1 and not act.ssim and getattr(act, "allreduce_scalars", None) is None
            and os.environ.get("GSLM_CG_LEAN", "1") != "0")


def _cgls_lean(prob, act, g, max_iter, restart_iter):
    """cgls_fused's benchmark-mode loop on an active view with less work around the tile pass;
    x is bitwise that loop's.  Per iteration: tangent (with p = s + beta p and the deferred x += alpha p), tile
    pass, gather, update -- no finalising launch: the gather leaves delta and the update leaves gamma' as block
    partials, and the kernel that needs the scalar sums them (the update: delta, and after a start gamma_0; the next
    tangent kernel: gamma'; the solve's last launch: the last gamma'), one of its blocks storing the sum to the
    scalar's slot of sc.  The per-Gaussian kernels read the chains' parameters from the view's list-order block.
    One launch starts the solve from the full-layout g and one ends it in the full-layout x.  A restart
    (restart_iter < max_iter) runs cgls_fused's own flush -> matvec -> dot sequence on the packed g."""
    full = act._full
    vr = act.views[0]
    ids, Pa = act._active
    n = act.layout.numel
    dev, st = act.device, act.stream
    P = full.layout.P
    lo = (3 * Pa // 4) * 4  # (mask_xyz: the xyz group is zero in every iterate, as in cgls_fused)
    na = n - lo
    w, ng, tail = act._pack_args()
    block, pos = vr.active_params(act.model, P, st)
    sc = torch.zeros(16, dtype=torch.float64, device=dev)
    ptr = lambda i: sc.data_ptr() + 8 * i
    off = lambda t: t.data_ptr() + 4 * lo
    GAM, GAMN, DEL = 0, 1, 2
    NB = 1024  # DOT_BLOCKS: partials of a flat-vector dot
    x, s, p, q = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
    part_g0 = torch.empty(NB, dtype=torch.float64, device=dev)  # gamma_0's partials
    part_gn = torch.empty(NB, dtype=torch.float64, device=dev)  # gamma's: not the buffer delta's are in
    part_d = act.dot_scratch
    npd = (Pa + 255) // 256
    ids_ptr = ids.data_ptr() if Pa else None
    ez = prob.exposure_is_zero(g)
    check(lib.gslm_cg_start_active(g.data_ptr(), ids_ptr, Pa, P, w, ng, tail, lo, s.data_ptr(), p.data_ptr(),
                                   q.data_ptr(), x.data_ptr(), part_g0.data_ptr(), st), "gslm_cg_start_active")
    gam_part = part_g0.data_ptr()  # gamma still as partials (until the first update stores it)
    gp = None
    pend = pre = None
    iter_total = 0
    first = True
    while iter_total < max_iter:
        if not first:
            check(lib.gslm_axpy_dev(na, pend[0], pend[1], 1.0, off(p), off(x), st), "gslm_axpy_dev")
            pend = pre = None
            if gp is None:
                gp = act.pack(g)
            act.matvec(x, q)
            torch.sub(gp, q, out=s)
            p.copy_(s)
            act.dot(s[lo:], s[lo:], ptr(GAM))
            gam_part = None
        first = False
        for _ in range(restart_iter):
            lean = _lib.GslmCgLean()
            lean.dot_defer = 1
            lean.params = block.data_ptr()
            fpre = None
            if pre is not None:
                fpre = pre + (x, pend[0], pend[1])
                pend = None
                lean.beta_partials, lean.beta_np, lean.beta_store = part_gn.data_ptr(), NB, pre[1]
            act.local_normal_matvec(p, q, damp=True, pre=fpre, exposure_zero=ez, lean=lean)
            check(lib.gslm_cg_update_lean(na, ptr(GAM), gam_part, NB if gam_part else 0, part_d.data_ptr(), npd,
                                          ptr(DEL), off(p), off(q), off(s), part_gn.data_ptr(), st),
                  "gslm_cg_update_lean")
            gam_part = None
            pend = (ptr(GAM), ptr(DEL))  # alpha = gamma / delta, read before either slot is rewritten
            pre = (s, ptr(GAMN), ptr(GAM))  # beta = gamma' / gamma (gamma' stored to its slot by the kernel that sums it)
            GAM, GAMN = GAMN, GAM
            iter_total += 1
            if iter_total >= max_iter:
                break
    out = torch.empty(full.layout.numel, dtype=torch.float32, device=dev)
    check(lib.gslm_cg_end_active(x.data_ptr(), p.data_ptr(), pend[0], pend[1], lo, pos.data_ptr(), Pa, P, w, ng, tail,
                                 out.data_ptr(), part_gn.data_ptr(), NB, ptr(GAM), st), "gslm_cg_end_active")
    # what the solve left on the device (tests/test_gpu_cg_lean.py): the scalar slots and the partials behind them
    act._full._lean_state = {"sc": sc, "gamma": GAM, "delta": DEL, "gamma_partials": part_gn,
                             "delta_partials": part_d[:npd], "s": s, "p": p, "q": q, "lo": lo}
    return out, {"iters": iter_total, "residuals": []}


def cgls_fused(prob, g, max_iter=10, restart_iter=10, tol=1e-10, atol=0.0, check_every=True, verbose=False,
               callback=None, host_checks=None):
    """cgls_damped (conjugate_gradient.py:51-127) on the fused operator, x0 = 0.

    Returns (x, info).  check_every: the reference's stopping tests (delta < 1e-20, residual increase, gamma
    tolerance).  They run on the device by default (gslm_cg_monitor: a control block the update and product
    kernels test, one read-back at the end, no host synchronisation inside the loop -- the host enqueues the
    whole max_iter x restart_iter schedule and a stopped solve's remaining launches return at once);
    host_checks=True (or verbose / a callback, which need the values each iteration) reads the scalars back
    every iteration instead.  Both give the same iterates, stop and history.  With check_every=False the tests
    are skipped (benchmark mode); the iterates are identical while no test fires.

    A local single-view problem with the xyz mask is solved on the Gaussians its view can move (LMProblem.
    active_view: the rows of every CG vector that are exactly zero throughout are left out of the vectors, so the
    per-Gaussian kernels stream Pa rows instead of P); x comes back in the full layout.  GSLM_CG_ACTIVE=0 keeps
    the full vectors.  In benchmark mode that solve runs _cgls_lean's loop (same iterates bitwise, fewer launches;
    GSLM_CG_LEAN=0 keeps this function's).  Not taken with a callback (it sees the solver's own vectors), for several views or the
    Gaussian-sharded operators."""
    act = _active_view_for(prob, g, callback)
    if act is not None and _lean_applies(act, check_every, max_iter):
        return _cgls_lean(prob, act, g, max_iter, restart_iter)
    if act is not None:
        gp = act.pack(g)
        if prob.exposure_is_zero(g):
            act._mark_rhs(gp)  # (exposure_is_zero of the packed vector without a device read)
        x, info = cgls_fused(act, gp, max_iter=max_iter, restart_iter=restart_iter, tol=tol, atol=atol,
                             check_every=check_every, verbose=verbose, callback=None, host_checks=host_checks)
        return act.unpack(x), info
    n = prob.layout.numel
    dev = prob.device
    st = prob.stream
    # With the xyz mask (train_jvp.py:221-227) the xyz group is zero in every iterate: the vector
    # updates and dots run on [lo, n) only (lo rounded down to a float4 boundary for the update kernel).
    lo = (3 * prob.layout.P // 4) * 4 if getattr(prob, "mask_xyz", False) else 0
    na = n - lo
    off = lambda t: t.data_ptr() + 4 * lo
    sc = torch.zeros(16, dtype=torch.float64, device=dev)
    ptr = lambda i: sc.data_ptr() + 8 * i
    GAM, GAMN, DEL, XG, XS = 0, 1, 2, 3, 4  # gamma / gamma' ping-pong between slots 0 and 1
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    s = torch.empty_like(x)
    p = torch.empty_like(x)
    q = torch.zeros_like(x)
    if host_checks is None:
        host_checks = verbose or callback is not None
    on_device = check_every and not host_checks
    ctl = None
    if on_device:
        # [stop, iters, last_res, n_hist, history...] (gslm_cg_monitor)
        ctl = torch.full((4 + max_iter,), math.nan, dtype=torch.float64, device=dev)
        ctl[:4] = torch.tensor([0.0, 0.0, math.inf, 0.0], dtype=torch.float64)
        loss = prob.loss
        b2_dev = loss if (torch.is_tensor(loss) and loss.is_cuda and loss.dtype == torch.float64 and
                          loss.numel() == 1) else torch.tensor(float(loss), dtype=torch.float64, device=dev)
    cg_ctl = ctl.data_ptr() if ctl is not None else None
    ctl_kw = {"cg_ctl": cg_ctl} if (cg_ctl is not None and getattr(prob, "supports_cg_ctl", False)) else {}
    b2 = float(prob.loss) if (check_every and not on_device) else None  # ||b||^2 = loss
    iter_total, last_res, history = 0, math.inf, []
    # Benchmark mode defers x += alpha p into the next product's xpby pass (gslm_matvec_opts.alpha_num):
    # the update kernel then streams s and q only; the iterates are bitwise those of the undeferred loop.
    defer = not check_every and callback is None
    pend = None  # (alpha_num, alpha_den) of a deferred x update not yet applied
    # Gaussian-sharded operators (gslm.parallel.GaussianShardedOperator) hold a shard of every vector: each
    # dot / update pass leaves a per-shard partial that is summed over the ranks before it is used
    red = getattr(prob, "allreduce_scalars", None)

    def reduce(*slots):
        if red is not None:
            red(sc, slots)

    def flush():
        nonlocal pend
        if pend is not None:
            check(lib.gslm_axpy_dev(na, pend[0], pend[1], 1.0, off(p), off(x), st), "gslm_axpy_dev")
            pend = None

    # the products may leave y's exposure slice (D v there) unwritten only when g's is zero (exposure_zero)
    ez = {"exposure_zero": True} if (getattr(prob, "supports_exposure_zero", False) and
                                     prob.exposure_is_zero(g)) else {}
    first = True
    while iter_total < max_iter:
        if first:
            s.copy_(g)  # s0 = J^T b - D x0 with x0 = 0
            first = False
        else:
            flush()
            prob.matvec(x, q, **ctl_kw)
            torch.sub(g, q, out=s)
        p.copy_(s)
        prob.dot(s[lo:], s[lo:], ptr(GAM))
        reduce(GAM)
        stop = False
        pre = None
        for _ in range(restart_iter):
            # [p = s + beta p and the deferred x += alpha p, both fused into this product's tangent kernel]
            # q = A p and delta = <p, A p> (= |J p|^2 + p.D.p), fused into the gather when possible
            full = None if pre is None else pre + ((x, pend[0], pend[1]) if pend is not None else (None, None, None))
            if full is not None:
                pend = None
            # (q was allocated zero; with g's exposure slice zero every iterate's is: J has no exposure column
            # and x0 = 0)
            if not prob.matvec_dot(p, q, ptr(DEL), pre=full, **ez, **ctl_kw):
                prob.dot(p[lo:], q[lo:], ptr(DEL))
            reduce(DEL)
            if check_every and not on_device and not math.isfinite(sc[DEL].item()):
                raise_nonfinite(prob, g)
            if check_every and not on_device and sc[DEL].item() < 1e-20:
                if verbose:
                    print("Early termination: delta is too small.")
                stop = True
                break
            # [x += alpha p ;] s -= alpha q ; gamma' = <s, s> [; <x, g>, <x, s> for the monitor]  (one pass)
            if check_every:
                check(lib.gslm_cg_update_monitor(na, ptr(GAM), ptr(DEL), off(p), off(q), off(x), off(s), off(g),
                                                 prob.dot_scratch.data_ptr(), prob.dot_scratch.numel() * 8,
                                                 ptr(GAMN), ptr(XG), ptr(XS), cg_ctl, st))
                reduce(GAMN, XG, XS)
                if on_device:  # the stopping tests of :88-117 on the device (gslm_cg_monitor)
                    check(lib.gslm_cg_monitor(ptr(GAM), ptr(GAMN), ptr(DEL), ptr(XG), ptr(XS), b2_dev.data_ptr(),
                                              float(tol), float(atol), cg_ctl, max_iter, st), "gslm_cg_monitor")
            elif defer:
                check(lib.gslm_cg_update(na, ptr(GAM), ptr(DEL), off(p), off(q), None, off(s),
                                         prob.dot_scratch.data_ptr(), ptr(GAMN), st))
                pend = (ptr(GAM), ptr(DEL))  # alpha = gamma / delta, read before either slot is rewritten
                reduce(GAMN)
            else:
                check(lib.gslm_cg_update(na, ptr(GAM), ptr(DEL), off(p), off(q), off(x), off(s),
                                         prob.dot_scratch.data_ptr(), ptr(GAMN), st))
                reduce(GAMN)
            # beta = gamma' / gamma; after the slot swap below these are the GAM / GAMN slots
            pre = (s, ptr(GAMN), ptr(GAM))
            if check_every and not on_device:
                vals = sc[:5].tolist()
                if not all(math.isfinite(vals[k]) for k in (GAM, GAMN, XG, XS)):
                    raise_nonfinite(prob, g)
                res = b2 - vals[XG] - vals[XS]  # ||b - J x||^2 + x^T D x  (monitor of conjugate_gradient.py:103-104)
                history.append(res)
                if verbose:
                    print(f"[Iter {iter_total + 1}] res: {res:.2e}")
                if res > last_res:
                    stop = True
                    break
                last_res = res
                if vals[GAMN] < max(tol * math.sqrt(vals[GAM]), atol):
                    stop = True
                    break
            if callback is not None:
                callback(x, s, iter_total + 1)
            GAM, GAMN = GAMN, GAM
            iter_total += 1
            if iter_total >= max_iter:
                stop = True
                break
        if stop:
            break
    flush()
    if on_device:
        c = ctl.tolist()  # the solve's one read-back
        if int(c[0]) == CG_STOP_NONFINITE:  # (the monitor's inputs are all-reduced first: every rank raises here)
            raise_nonfinite(prob, g)
        iter_total, nh = int(c[1]), int(c[3])
        history = c[4:4 + min(nh, max_iter)]
        return x, {"iters": iter_total, "residuals": history, "stop": int(c[0])}
    return x, {"iters": iter_total, "residuals": history}


def cgls_jacobi(prob, g, max_iter=10, restart_iter=10, tol=1e-10, atol=0.0, check_every=True, verbose=False,
                diag=None):
    """cgls_fused's solve of (J^T J + D) x = g from x0 = 0 with the Jacobi preconditioner M = diag(J^T J + D)
    (LMProblem.diagonal): the reference's restart schedule and stopping tests (conjugate_gradient.py:51-127) with
    z = M^-1 s, gamma = <s, z> and p = z + beta p.  The monitor b^2 - <x, g> - <x, s> is the objective itself and
    does not change.  Returns (x, info).

    Scalars stay on the device (gslm_pcg_update, gslm_xpby_dev); with check_every=True the stopping tests read them
    back every iteration, with check_every=False the loop has no host synchronisation (one read-back after it, for
    the NaN check).  diag: the diagonal in prob's layout when the caller has it (entries <= 0 are not preconditioned
    against: z = 0 there); ones make this plain CG.  A local single-view problem is solved on its active list as in
    cgls_fused (the diagonal packed with g; GSLM_CG_ACTIVE=0 keeps the full vectors).  The lean loop is not
    involved.  The plain residual on the LM rows only (LMProblem.diagonal's ValueError otherwise)."""
    if not isinstance(prob, LMProblem) or prob.ssim or prob.train_exposure or not prob.mask_xyz or \
            prob.layout.rest_views:
        raise ValueError("cgls_jacobi: a local LMProblem with the [r; r] residual on the LM rows (mask_xyz=True, no "
                         "SSIM, no trained exposure, not the batched problem)")
    if diag is None:
        diag = prob.diagonal()
    act = _active_view_for(prob, g, None)
    if act is not None:
        gp = act.pack(g)
        if prob.exposure_is_zero(g):
            act._mark_rhs(gp)
        x, info = _pcg(act, gp, act.pack(diag), max_iter, restart_iter, tol, atol, check_every, verbose)
        return act.unpack(x), info
    return _pcg(prob, g, diag, max_iter, restart_iter, tol, atol, check_every, verbose)


def _pcg(prob, g, diag, max_iter, restart_iter, tol, atol, check_every, verbose):
    """cgls_jacobi's recursion on the vectors of `prob` (the problem itself or its active view)."""
    n = prob.layout.numel
    dev, st = prob.device, prob.stream
    lo = (3 * prob.layout.P // 4) * 4  # (mask_xyz: the xyz group is zero in every iterate, as in cgls_fused)
    na = n - lo
    off = lambda t: t.data_ptr() + 4 * lo
    sc = torch.zeros(16, dtype=torch.float64, device=dev)
    ptr = lambda i: sc.data_ptr() + 8 * i
    GAM, GAMN, DEL, XG, XS = 0, 1, 2, 3, 4
    x, q, z, minv = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(4))
    s, p = torch.empty_like(x), torch.empty_like(x)
    check(lib.gslm_precond_invert(na, off(diag), off(minv), st), "gslm_precond_invert")
    b2 = float(prob.loss) if check_every else None  # ||b||^2 = loss
    ez = {"exposure_zero": True} if prob.exposure_is_zero(g) else {}
    iter_total, last_res, history = 0, math.inf, []
    first = True
    while iter_total < max_iter:
        if first:
            s.copy_(g)  # s0 = J^T b - A x0 with x0 = 0
            first = False
        else:
            prob.matvec(x, q)
            torch.sub(g, q, out=s)
        torch.mul(s[lo:], minv[lo:], out=z[lo:])
        p.copy_(z)
        prob.dot(s[lo:], z[lo:], ptr(GAM))
        stop = False
        beta = None  # (num, den) of the direction update not yet applied
        for _ in range(restart_iter):
            if beta is not None:
                check(lib.gslm_xpby_dev(na, off(z), beta[0], beta[1], off(p), st), "gslm_xpby_dev")
            if not prob.matvec_dot(p, q, ptr(DEL), **ez):
                prob.dot(p[lo:], q[lo:], ptr(DEL))
            if check_every:
                delta = sc[DEL].item()
                if not math.isfinite(delta):
                    raise_nonfinite(prob, g)
                if delta < 1e-20:
                    if verbose:
                        print("Early termination: delta is too small.")
                    stop = True
                    break
            # x += alpha p ; s -= alpha q ; z = M^-1 s ; gamma' = <s, z>  (one pass)
            check(lib.gslm_pcg_update(na, ptr(GAM), ptr(DEL), off(p), off(q), off(x), off(s), off(minv), off(z),
                                      prob.dot_scratch.data_ptr(), ptr(GAMN), st), "gslm_pcg_update")
            beta = (ptr(GAMN), ptr(GAM))  # beta = gamma' / gamma; after the swap below the GAM / GAMN slots
            if check_every:
                prob.dot(x[lo:], g[lo:], ptr(XG))
                prob.dot(x[lo:], s[lo:], ptr(XS))
                vals = sc[:5].tolist()
                if not all(math.isfinite(vals[k]) for k in (GAM, GAMN, XG, XS)):
                    raise_nonfinite(prob, g)
                res = b2 - vals[XG] - vals[XS]  # the monitor of conjugate_gradient.py:103-104
                history.append(res)
                if verbose:
                    print(f"[Iter {iter_total + 1}] res: {res:.2e}")
                if res > last_res:
                    stop = True
                    break
                last_res = res
                if vals[GAMN] < max(tol * math.sqrt(max(vals[GAM], 0.0)), atol):
                    stop = True
                    break
            GAM, GAMN = GAMN, GAM
            iter_total += 1
            if iter_total >= max_iter:
                stop = True
                break
        if stop:
            break
    if not check_every and not all(math.isfinite(v) for v in sc[:3].tolist()):  # the solve's one read-back
        raise_nonfinite(prob, g)
    return x, {"iters": iter_total, "residuals": history, "precond": "jacobi"}


def cgls_residual(prob, max_iter=10, restart_iter=10, tol=1e-10, atol=0.0, verbose=False, callback=None):
    """cgls_damped (conjugate_gradient.py:51-127) in the reference's own recursion, on the HIP operator: residual-
    space r (one [3,H,W] image per view standing for the [r; r] pair, so its dots count twice), r -= alpha q with
    q = J p, a fresh s = J^T r - D x every iteration, and the residual monitor from a fresh J x -- two tangent
    passes and one seeded adjoint pass per iteration, where cgls_fused runs one fused (J^T J + D) p and updates s
    algebraically.  Equal iterates in exact arithmetic; this mode keeps long float32 solves on the reference's
    rounding path.  b = -[r; r] (train_jvp.py:243), x0 = 0.  Returns (x, info)."""
    if getattr(prob, "ssim", False):
        raise ValueError("cgls_residual: the disable_ssim residual only")
    if getattr(prob, "damping", "fixed") != "fixed" or getattr(prob, "_dvec", None) is not None:
        raise ValueError("cgls_residual: the seven damping constants only (no damping vector)")
    if getattr(prob, "train_exposure", False):
        raise ValueError("cgls_residual: the residual-space recursion does not carry trained exposure")
    if getattr(prob, "robust", None) is not None:
        raise ValueError("cgls_residual: the recursion iterates on the raw residuals, not a robust problem's "
                         "reweighted ones (cgls_fused / cgls_jacobi)")
    dev = prob.device
    rm = prob.residual_masks()
    b = [-r for r in prob.residuals]  # b = -[r; r]: one copy per view

    def dot2(u, v):  # <[u; u], [v; v]> over the views, reduced in float64 on the device (the .item() of :138-146)
        return 2.0 * sum(float((a.double() * c.double()).sum()) for a, c in zip(u, v))

    n = prob.layout.numel
    dvec = torch.empty(n, dtype=torch.float64, device=dev)
    bounds = list(prob._bounds)
    for k in range(7):
        dvec[bounds[k]:bounds[k + 1]] = float(prob._damps[k])

    def ddot(u, v):  # dot(x, y, damp) of GaussianModelState (gaussian_model_state.py:262-269)
        return float((u.double() * v.double() * dvec).sum())

    def Dx(x):
        return (x.double() * dvec).to(torch.float32)

    jv = [torch.empty_like(t) for t in b]
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    s = torch.empty_like(x)
    iter_total, last_res, history = 0, math.inf, []
    stop = False
    while iter_total < max_iter and not stop:
        prob.jv_residual(x, rm, jv)
        r = [bb - q for bb, q in zip(b, jv)]                         # r0 = b - A x0
        prob.jt_residual(r, rm, s)
        s -= Dx(x)                                                    # s0 = A^T r0 - D x0
        p = s.clone()
        gamma = float((s.double() * s.double()).sum())
        for _ in range(restart_iter):
            q = [t.clone() for t in prob.jv_residual(p, rm, jv)]      # q = A p
            delta = dot2(q, q) + ddot(p, p)
            if delta < 1e-20:
                if verbose:
                    print("Early termination: delta is too small.")
                stop = True
                break
            alpha = gamma / delta
            x += alpha * p
            r = [rr - alpha * qq for rr, qq in zip(r, q)]
            prob.jt_residual(r, rm, s)
            s -= Dx(x)                                                # s = A^T r - D x
            gamma_prev, gamma = gamma, float((s.double() * s.double()).sum())
            p = s + (gamma / gamma_prev) * p
            prob.jv_residual(x, rm, jv)
            cur = [bb - q for bb, q in zip(b, jv)]                   # cur_r = b - A x
            res = dot2(cur, cur) + ddot(x, x)
            history.append(res)
            if verbose:
                print(f"[Iter {iter_total + 1}] res: {res:.2e}")
            if res > last_res:
                stop = True
                break
            last_res = res
            if callback is not None:
                callback(x, s, iter_total + 1)
            if gamma < max(tol * math.sqrt(gamma_prev), atol):
                stop = True
                break
            iter_total += 1
            if iter_total >= max_iter:
                stop = True
                break
    return x, {"iters": iter_total, "residuals": history}


def loss_set_group():
    """Sets per blend pass of the line search (GSLM_LOSS_SET_GROUP, 1..8; default 1 = one pass per set).

    The variable was GSLM_LOSS_SETS until round 5, whose meaning changed between rounds (round 4: 1 = all sets; round
    5: 1 = per set): the old spelling is refused rather than silently read with either meaning, and so is a value
    outside 1..8."""
    if "GSLM_LOSS_SETS" in os.environ:
        raise ValueError("GSLM_LOSS_SETS is no longer read: set GSLM_LOSS_SET_GROUP=k (k sets per blend pass, 1..8; "
                         "1 = per set, the default; 8 = all sets in one pass)")
    raw = os.environ.get("GSLM_LOSS_SET_GROUP", "1")
    try:
        k = int(raw)
    except ValueError:
        k = 0
    if not 1 <= k <= 8:
        raise ValueError(f"GSLM_LOSS_SET_GROUP={raw!r}: sets per blend pass must be an integer in 1..8")
    return k


def live_masks():
    """Whether the LM row map refines the list's quadrant masks to the visits some pixel blends (GSLM_LIVE_MASKS,
    default 1; 0 = the binning's own masks, for A/B runs).  The library reads the variable at every row map; any
    value but "0" and "1" is refused here."""
    raw = os.environ.get("GSLM_LIVE_MASKS", "1")
    if raw not in ("0", "1"):
        raise ValueError(f"GSLM_LIVE_MASKS={raw!r}: 1 (refine the quadrant masks, the default) or 0")
    return raw == "1"


class LossEvaluator:
    """The line search's validation loss: `val_loss_func().loss_scalar` of train_jvp.py:258,268,279 (batch_training_loss
    with disable_ssim=True over the validation views: 2 sum_b ||m_b clamp01(R_b) - gt_b||^2) on the HIP forward.

    Per view: gslm_preprocess_ordered -> gslm_rasterize_loss (binning, then the blend with the residual's loss fused
    into its epilogue: no image is written).
      * Depth order: it depends on xyz alone, which the LM step freezes (train_jvp.py:221-227), so each view's order
        is sorted at its first evaluation and reused while model._xyz is the same tensor at the same version (the
        same point list, bitwise).
      * Batches: views run in batches of `batch` workspaces.  The first evaluation sizes the binnings: a batch's
        preprocesses are enqueued first and one gslm_num_rendered_many read-back sizes them all (one host round trip
        per batch).  With device_count=True later evaluations render through gslm_rasterize_loss_dev instead (the
        pair count stays on the device, no host round trip inside the evaluation); the counts land in one device
        array read once at the end, and a view whose count exceeded its slot's list capacity is rendered again
        exactly (its slot grown).
      * Streams: consecutive views of a batch run on `streams` HIP streams, so one view's short serial kernels
        (scans, the tile launch order, the loss reduction) and its blend's tail overlap another view's work.  Three
        by default: with the main stream that is the 4 hardware queues HIP gives a process (GPU_MAX_HW_QUEUES), and
        the LM step measured 91-93 ms at 3 side streams against 94-96 at 8 (profiles/r05/ab/val_streams_kept/; more
        queues or higher-priority streams were slower still).
    Each view's loss lands in its own device double; the total is their sum (view order fixed, so run to run the
    same).  `reduce`: a callable summing it over the ranks that hold the other views (gslm.parallel.allreduce_loss)."""

    def __init__(self, model, cams, bg, device="cuda", batch=8, gts=None, alpha_masks=None, reduce=None, streams=3,
                 device_count=False, train_exposure=False, fused_exposure=False, robust=None, depth_weight=None,
                 invdepths=None, depth_masks=None):
        """train_exposure: the loss is taken on the exposed colour of each camera's row of model._exposure, as
        LMProblem(train_exposure=True) takes it: 2 sum ||m clamp01(C) - gt||^2.  evaluate() then renders each view
        with the full forward and runs gslm_lm_residual_exposure in its loss-only mode (no fused loss epilogue, no
        side streams), and evaluate_points -- the union line search -- raises ValueError.
        fused_exposure (with train_exposure, without device_count -- else ValueError): the exposure is applied in the
        blend's loss epilogue instead (gslm_rasterize_loss_exposure: the same per-pixel residuals, summed per tile).
        evaluate() then takes its ordinary path -- batches, side streams, cached depth orders -- and evaluate_points
        is allowed: every set carries its own _exposure, and view i at set a uses row exp_idx[i] of it.
        robust: None, ("huber", delta) or ("cauchy", delta), as LMProblem takes it: the loss is 2 sum rho(r^2), summed
        in the blends' epilogues (gslm_rasterize_loss_robust and its slot and sets forms) -- batches, side streams
        and GSLM_LOSS_SET_GROUP as ever.  ValueError with device_count=True or train_exposure (neither blend has a
        robust form).
        depth_weight: None, or lambda_d >= 0 as LMProblem takes it, with the targets invdepths / depth_masks (default:
        the cameras' invdepthmap where depth_reliable is set, and depth_mask): a view with a target adds lambda_d sum
        (m_d (D - Dgt))^2, summed in the blend's epilogue (gslm_rasterize_loss_depth; evaluate_points through
        gslm_rasterize_loss_slot_depth per set -- there is no all-sets form, so GSLM_LOSS_SET_GROUP above 1 falls back to
        per set for those views); the other views run the plain blends.  ValueError with device_count=True,
        train_exposure or robust."""
        self.depth_weight = depth_option(depth_weight)
        if self.depth_weight is None and (invdepths is not None or depth_masks is not None):
            raise ValueError("invdepths / depth_masks are the targets of depth_weight, which is None")
        if self.depth_weight is not None and (device_count or train_exposure or robust is not None):
            raise ValueError("depth_weight: the device-count, exposure and robust blends have no depth form "
                             "(device_count=False, train_exposure=False, robust=None)")
        self.depth = (depth_targets(cams, invdepths, depth_masks, device) if self.depth_weight is not None
                      else [None] * len(cams))
        self.robust = robust_option(robust)
        if self.robust is not None and (device_count or train_exposure):
            raise ValueError("robust: the device-count blend and the exposure blends have no robust form "
                             "(device_count=False, train_exposure=False)")
        self._robust = _robust_struct(self.robust)
        self.model = model
        self.train_exposure = bool(train_exposure)
        self.fused_exposure = bool(fused_exposure)
        if self.fused_exposure and not self.train_exposure:
            raise ValueError("fused_exposure=True is an option of train_exposure=True")
        if self.fused_exposure and device_count:
            raise ValueError("fused_exposure=True: the device-count blend has no exposure form (device_count=False)")
        if self.train_exposure:
            self.exp_idx = _exposure_index(model, cams)
        if self.train_exposure and not self.fused_exposure:
            self._exp_scratch = torch.empty(lib.gslm_exposure_scratch_bytes(1, 1) // 8, dtype=torch.float64,
                                            device=device)
            self._exp_raster = {}  # (H, W) -> the ViewRaster whose workspaces the views of that size share
        # True: evaluations after the first render through gslm_rasterize_loss_dev (no count read-back per batch).
        # Measured at 50 1080p views, 8 streams: 0.347 ms per view against 0.339 with the per-batch read-back
        # (profiles/r03/val_loss_devcount.json) -- the read-back costs less than the capacity-sized tile sort
        self.device_count = device_count
        self.device = device
        self.reduce = reduce
        self.gts = [c.original_image.to(device) for c in cams] if gts is None else gts
        ms = [c.alpha_mask for c in cams] if alpha_masks is None else alpha_masks
        self.masks = [None if m is None else m.to(device=device, dtype=torch.float32).contiguous() for m in ms]
        self.views = [_lib.view_from_camera(c, bg, model.active_sh_degree) for c in cams]
        for vw, gt, m in zip(self.views, self.gts, self.masks):
            H, W = vw.image_height, vw.image_width
            if gt.shape != (3, H, W) or gt.dtype != torch.float32:
                raise ValueError(f"ground truth must be float32 (3, {H}, {W}), got {gt.dtype} {tuple(gt.shape)}")
            if m is not None and m.numel() != H * W:
                raise ValueError("alpha mask must be [1, H, W]")
        self.batch = max(1, min(int(batch), len(cams) or 1))
        nstr = max(1, min(int(streams), self.batch))
        self.streams = [torch.cuda.Stream(device) for _ in range(nstr)] if nstr > 1 else [None]
        self.slots = [dict(geom=None, binning=None) for _ in range(self.batch)]
        nb = max([lib.gslm_loss_scratch_bytes(v.image_height, v.image_width) for v in self.views] + [8])
        self.loss_scratch = [torch.empty(nb // 8 + 1, dtype=torch.float64, device=device) for _ in self.streams]
        self.num_rendered = [0] * len(cams)
        self._order_key, self._orders = None, [None] * len(cams)
        self._pos = [None] * len(cams)  # the depth orders' inverses (gslm_depth_positions), for evaluate_points
        # the shared binning of evaluate_points (gslm_union_*): per batch position k its sets' geometries, the union
        # geometry and the union list
        self.uslots = [[dict(geoms=[], ugeom=None) for _ in range(self.batch)] for _ in range(2)]
        self.ubins = [None] * self.batch
        self.sets_scratch = [None] * self.batch
        # the six points' blends: one pass per set over each union list (gslm_rasterize_loss_slot; loss_sets = 1), or
        # passes over groups of loss_sets sets each (gslm_rasterize_loss_sets) -- the same losses bitwise.  Per set is
        # the default: the all-sets pass wins when evaluate_points runs back to back (69.8 against 74.8 ms for the six
        # points over 50 views) but not inside lm_step, where it holds the CUs longer against the next batch's sorts
        # on the other streams (profiles/r04/ab/all_sets_default/, profiles/r05/ab/loss_set_groups/).
        # GSLM_LOSS_SET_GROUP=k (1..8) selects groups of k (1 = per set, 8 = all sets in one pass).
        self.loss_sets = loss_set_group()
        self.union_counts = []

    def _slot(self, k, P):
        sl = self.slots[k]
        if sl["geom"] is None or sl["geom"].numel() < lib.gslm_geom_bytes(P):
            sl["geom"] = _lib.u8(lib.gslm_geom_bytes(P), self.device)
        return sl

    def _stream(self, k):
        """(torch stream or None, hipStream_t) of batch position k."""
        st = self.streams[k % len(self.streams)]
        return st, (st.cuda_stream if st is not None else _lib.stream_handle(self.device))

    def _exposure_rows(self, holder, what="model"):
        """holder._exposure checked for the kernels (contiguous float32 [n, 3, 4] on the device): its data pointer;
        camera row r is the 12 floats at + 48 r."""
        X = getattr(holder, "_exposure", None)
        ref = self.model._exposure
        if (not torch.is_tensor(X) or X.dtype != torch.float32 or not X.is_contiguous() or X.shape != ref.shape
                or tuple(X.shape[1:]) != (3, 4) or X.device.type != torch.device(self.device).type):
            raise ValueError(f"fused_exposure: {what}._exposure must be contiguous float32 {tuple(ref.shape)} on "
                             f"{self.device}")
        return X.data_ptr()

    def _mask_ptr(self, i):
        m = self.masks[i]
        return None if m is None else m.data_ptr()

    def _refresh_orders(self, xyz, P):
        """Drop the cached depth orders (and their inverses) when xyz moved: another tensor object, version or size
        (_lib.tensor_token: the key holds xyz, so no later tensor can take its address while the orders live)."""
        key = self._order_key
        if key is None or key[1] != P or not _lib.token_matches(key[0], xyz):
            V = len(self.views)
            self._order_key, self._orders = (_lib.tensor_token(xyz), P), [None] * V
            self._pos = [None] * V

    def _preprocess_ordered(self, i, g, geom, sh):
        """gslm_preprocess_ordered of view i into the geometry workspace `geom` on stream sh: in the view's cached
        depth order (mode 2), or without one sorting and keeping the order (mode 1)."""
        mode = 2 if self._orders[i] is not None else 1
        if mode == 1:
            self._orders[i] = torch.empty(max(g.P, 1), dtype=torch.int32, device=self.device)
        check(lib.gslm_preprocess_ordered(ctypes.byref(self.views[i]), ctypes.byref(g), geom.data_ptr(), geom.numel(),
                                          None, self._orders[i].data_ptr(), mode, sh), "gslm_preprocess_ordered")

    def _total(self, losses):
        """The views' losses summed in view order (and over the ranks with `reduce`): a device double."""
        V = len(self.views)
        loss = losses[:V].sum() if V else losses[0]
        if self.reduce is not None:
            self.reduce(loss)
        return loss

    def _blend_loss(self, vw, P, sl, N, i, xrows, scr, out, sh):
        """gslm_rasterize_loss of view i from slot sl into the double at `out`; xrows (fused_exposure): the data
        pointer of the exposure rows, the blend then gslm_rasterize_loss_exposure with the camera's row; with `robust`
        gslm_rasterize_loss_robust."""
        mp = self._mask_ptr(i)
        dt = self.depth[i]
        if dt is not None:
            check(lib.gslm_rasterize_loss_depth(ctypes.byref(vw), P, sl["geom"].data_ptr(), sl["binning"].data_ptr(),
                                                sl["binning"].numel(), N, self.gts[i].data_ptr(), mp, dt[0].data_ptr(),
                                                None if dt[1] is None else dt[1].data_ptr(), self.depth_weight,
                                                scr.data_ptr(), scr.numel() * 8, out, 0, sh),
                  "gslm_rasterize_loss_depth")
        elif self._robust is not None:
            check(lib.gslm_rasterize_loss_robust(ctypes.byref(vw), P, sl["geom"].data_ptr(), sl["binning"].data_ptr(),
                                                 sl["binning"].numel(), N, self.gts[i].data_ptr(), mp,
                                                 ctypes.byref(self._robust), scr.data_ptr(), scr.numel() * 8, out, 0,
                                                 sh), "gslm_rasterize_loss_robust")
        elif xrows is None:
            check(lib.gslm_rasterize_loss(ctypes.byref(vw), P, sl["geom"].data_ptr(), sl["binning"].data_ptr(),
                                          sl["binning"].numel(), N, self.gts[i].data_ptr(), mp, scr.data_ptr(),
                                          scr.numel() * 8, out, 0, sh), "gslm_rasterize_loss")
        else:
            check(lib.gslm_rasterize_loss_exposure(ctypes.byref(vw), P, sl["geom"].data_ptr(), sl["binning"].data_ptr(),
                                                   sl["binning"].numel(), N, self.gts[i].data_ptr(), mp,
                                                   xrows + 48 * self.exp_idx[i], scr.data_ptr(), scr.numel() * 8, out,
                                                   0, sh), "gslm_rasterize_loss_exposure")

    def _render_exact(self, g, i, losses):
        """View i's loss into losses[i] with the count read back first (slot 0 grown as needed; main stream)."""
        P = g.P
        sl = self._slot(0, P)
        vw = self.views[i]
        main_h = torch.cuda.current_stream(self.device).cuda_stream
        self._preprocess_ordered(i, g, sl["geom"], main_h)  # (the order is the device-count render's)
        n = ctypes.c_int64(0)
        check(lib.gslm_num_rendered(sl["geom"].data_ptr(), P, ctypes.byref(n), main_h), "gslm_num_rendered")
        N = int(n.value)
        self.num_rendered[i] = N
        sl["binning"] = _grown(sl["binning"], lib.gslm_binning_bytes(N, vw.image_height, vw.image_width), self.device)
        self._blend_loss(vw, P, sl, N, i, None, self.loss_scratch[0], losses.data_ptr() + 8 * i, main_h)

    def evaluate(self):
        """Device double: the loss over this evaluator's views (summed over the ranks with `reduce`)."""
        if self.train_exposure and not self.fused_exposure:
            return self._evaluate_exposure()
        # fused_exposure: the blends read the cameras' rows of model._exposure on the device, in stream order
        xrows = self._exposure_rows(self.model) if self.fused_exposure else None
        g = raw_gaussians(self.model)
        P = g.P
        V = len(self.views)
        losses = torch.zeros(max(V, 1), dtype=torch.float64, device=self.device)
        main = torch.cuda.current_stream(self.device)
        main_h = main.cuda_stream
        self._refresh_orders(self.model._xyz, P)  # xyz moved: sort again
        # device-count renders' pair counts: allocated and zeroed on the main stream BEFORE the side streams wait on
        # it, so no stream's k_ranges count write can precede the zero fill
        counts = torch.zeros(max(V, 1), dtype=torch.int32, device=self.device)
        for st in self.streams:  # the parameters (and the zeroed losses and counts) as the main stream left them
            if st is not None:
                st.wait_stream(main)
        caps = {}  # view -> list capacity it was rendered with (device-count renders)
        for b0 in range(0, V, self.batch):
            idx = list(range(b0, min(V, b0 + self.batch)))
            slots = [self._slot(k, P) for k in range(len(idx))]
            if self.device_count and all(sl["binning"] is not None for sl in slots):
                # device-count renders: per view preprocess -> binning + blend + loss on its stream, no read-back
                for k, (sl, i) in enumerate(zip(slots, idx)):
                    vw = self.views[i]
                    _, sh = self._stream(k)
                    self._preprocess_ordered(i, g, sl["geom"], sh)
                    caps[i] = (k, int(lib.gslm_binning_capacity(sl["binning"].numel(), vw.image_height,
                                                                   vw.image_width)))
                    scr = self.loss_scratch[k % len(self.streams)]
                    check(lib.gslm_rasterize_loss_dev(ctypes.byref(vw), P, sl["geom"].data_ptr(), sl["binning"].data_ptr(),
                                                      sl["binning"].numel(), self.gts[i].data_ptr(), self._mask_ptr(i),
                                                      scr.data_ptr(), scr.numel() * 8, losses.data_ptr() + 8 * i, 0,
                                                      counts.data_ptr() + 4 * i, sh), "gslm_rasterize_loss_dev")
                continue
            for k, (sl, i) in enumerate(zip(slots, idx)):
                self._preprocess_ordered(i, g, sl["geom"], self._stream(k)[1])
            for st in self.streams:
                if st is not None:
                    main.wait_stream(st)
            geoms = (ctypes.c_void_p * len(idx))(*[sl["geom"].data_ptr() for sl in slots])
            Ps = (ctypes.c_int64 * len(idx))(*([P] * len(idx)))
            Ns = (ctypes.c_int64 * len(idx))()
            check(lib.gslm_num_rendered_many(geoms, Ps, len(idx), Ns, main_h), "gslm_num_rendered_many")
            for k, (sl, i) in enumerate(zip(slots, idx)):
                vw = self.views[i]
                H, W, N = vw.image_height, vw.image_width, int(Ns[k])
                self.num_rendered[i] = N
                st, sh = self._stream(k)
                # (an old buffer is freed on the main stream: after its last use on the view's)
                sl["binning"] = _grown(sl["binning"], lib.gslm_binning_bytes(N, H, W), self.device, main, st)
                self._blend_loss(vw, P, sl, N, i, xrows, self.loss_scratch[k % len(self.streams)],
                                 losses.data_ptr() + 8 * i, sh)
        for st in self.streams:
            if st is not None:
                main.wait_stream(st)
        if caps:
            ns = counts.tolist()  # the evaluation's one read-back
            for i in caps:
                self.num_rendered[i] = ns[i]
            for i, (k, cap) in caps.items():
                if ns[i] > cap:  # a list past its slot's capacity: this view again, exactly, on the main stream
                    self._render_exact(g, i, losses)
                    vw = self.views[i]
                    need = lib.gslm_binning_bytes(ns[i], vw.image_height, vw.image_width)
                    # and its slot's list grown for the next evaluation
                    self.slots[k]["binning"] = _grown(self.slots[k]["binning"], need, self.device)
        return self._total(losses)

    def _evaluate_exposure(self):
        """evaluate() with train_exposure: per view the forward, then the exposure residual's loss alone."""
        g = raw_gaussians(self.model)
        V = len(self.views)
        losses = torch.zeros(max(V, 1), dtype=torch.float64, device=self.device)
        X = self.model._exposure
        if X.dtype != torch.float32 or not X.is_contiguous():
            raise ValueError("train_exposure: model._exposure must be contiguous float32 [n, 3, 4]")
        stream = _lib.stream_handle(self.device)
        for i, vw in enumerate(self.views):
            key = (vw.image_height, vw.image_width)
            vr = self._exp_raster.get(key)
            if vr is None:
                vr = self._exp_raster[key] = ViewRaster(vw, self.device)
            vr.view = vw
            R = vr.forward(g, stream, want_invdepth=False)
            self.num_rendered[i] = vr.N
            check(lib.gslm_lm_residual_exposure(
                vr.H, vr.W, R.data_ptr(), self.gts[i].data_ptr(), self._mask_ptr(i),
                X.data_ptr() + 48 * self.exp_idx[i], None, None, None, None, self._exp_scratch.data_ptr(),
                self._exp_scratch.numel() * 8, losses.data_ptr() + 8 * i, 0, stream), "gslm_lm_residual_exposure")
        return self._total(losses)

    # ---- the line search's six points with one binning per view (include/gslm.h "shared binning", ABI 8) ----
    def _sets_scratch(self, k, n, H, W):
        """Batch position k's per-tile partials of the all-sets blend (its stream's own buffer)."""
        nb = lib.gslm_loss_sets_scratch_bytes(n, H, W)
        t = self.sets_scratch[k]
        if t is None or t.numel() * 8 < nb:
            t = self.sets_scratch[k] = torch.empty(nb // 8 + 1, dtype=torch.float64, device=self.device)
        return t

    def _uslot(self, par, k, n, P):
        """Batch position k's depth-space records (n sets, gslm_depth_records_bytes(P) = 64 B per Gaussian each) and
        union geometry (gslm_geom_bytes(P), ~112 B per Gaussian), of slot set `par` (two sets alternate over the
        batches: a batch's preprocesses overwrite the slots of the batch before the previous one).  Peak device memory
        of evaluate_points: 2 x batch x (64 n + 112) B per Gaussian (7.9 GB at 1M Gaussians, batch 8, n = 6; until
        round 5 every set held a whole geometry workspace: 12.5 GB), plus the snapshots' five moving leaves per point
        (param_snapshot) and one sort geometry; clear_val_cache() releases an evaluator lm_step kept."""
        sl = self.uslots[par][k]
        nr, nb = lib.gslm_depth_records_bytes(P), lib.gslm_geom_bytes(P)
        while len(sl["geoms"]) < n:
            sl["geoms"].append(None)
        for a in range(n):
            if sl["geoms"][a] is None or sl["geoms"][a].numel() < nr:
                sl["geoms"][a] = _lib.u8(nr, self.device)
        if sl["ugeom"] is None or sl["ugeom"].numel() < nb:
            sl["ugeom"] = _lib.u8(nb, self.device)
        return sl

    def _sort_geom(self, P):
        """The full geometry workspace of the depth sorts of evaluate_points (main stream only)."""
        t = getattr(self, "_sgeom", None)
        if t is None or t.numel() < lib.gslm_geom_bytes(P):
            t = self._sgeom = _lib.u8(lib.gslm_geom_bytes(P), self.device)
        return t

    def refresh_views(self, cams, bg, sh_degree):
        """Rebuild the views from the cameras (their matrices now) and drop the cached depth order of every view whose
        camera moved -- a kept evaluator (lm_step's _VAL_CACHE) then never renders with a stale pose."""
        for i, c in enumerate(cams):
            v = _lib.view_from_camera(c, bg, sh_degree)
            if bytes(v) != bytes(self.views[i]):
                self.views[i] = v
                self._orders[i] = None
                self._pos[i] = None

    def evaluate_points(self, sets):
        """The validation loss at each of n <= 8 parameter sets (snapshots sharing the model's frozen xyz: the six
        line-search points of train_jvp.py:262-277, param_snapshot), as a list of device doubles -- each bitwise equal
        to evaluate() with the model at that set.  Per view: the n sets' render records in depth space
        (gslm_preprocess_views with the view's depth positions: one pass over the Gaussians per set for the batch's
        views), ONE binning over the union of the sets' rects (gslm_union_geometry / gslm_union_binning: 4 mask bits
        per set and list entry, carried through the tile sort), then the n blends + losses through it
        (gslm_rasterize_loss_slot).  With fused_exposure every set also carries its _exposure (param_snapshot(model,
        exposure=True)) and the blends are the exposure forms, view i at set a under row exp_idx[i] of sets[a]._exposure.
        Pipelining: a batch's preprocesses, union geometries and pair-count read-back run on the main stream while the
        previous batch's binnings and blends run on the side streams (two alternating slot sets), so the read-back does
        not drain the device.  union_counts[i]: view i's union list length (the last call)."""
        if self.train_exposure and not self.fused_exposure:
            raise ValueError("evaluate_points renders no exposure: with train_exposure the line search is exact "
                             "(fused_exposure=True renders it in the blend's epilogue)")
        n = len(sets)
        if not 1 <= n <= 8:
            raise ValueError("evaluate_points takes 1..8 parameter sets")
        xs = [self._exposure_rows(st, f"sets[{a}]") for a, st in enumerate(sets)] if self.fused_exposure else None
        xyz = sets[0]._xyz
        if any(st._xyz is not xyz for st in sets):
            raise ValueError("evaluate_points: every set shares the frozen xyz tensor")
        gs = [raw_gaussians(st) for st in sets]
        P = gs[0].P
        V = len(self.views)
        main = torch.cuda.current_stream(self.device)
        main_h = main.cuda_stream
        self._refresh_orders(xyz, P)
        losses = [torch.zeros(max(V, 1), dtype=torch.float64, device=self.device) for _ in range(n)]
        self.union_counts = [0] * V
        side = [st for st in self.streams if st is not None]
        done = [None, None]  # per slot set: events after the side streams' last use of its slots
        for bi, b0 in enumerate(range(0, V, self.batch)):
            par = bi & 1
            idx = list(range(b0, min(V, b0 + self.batch)))
            if done[par] is not None:  # the batch before the previous one has finished with these slots
                for ev in done[par]:
                    main.wait_event(ev)
            slots = [self._uslot(par, k, n, P) for k in range(len(idx))]
            # 1. each view's depth order (sorted once while xyz is unchanged) and its inverse, the depth positions
            for k, i in enumerate(idx):
                if self._orders[i] is None:  # the depth sort (set 0's geometry; only the order is kept)
                    self._preprocess_ordered(i, gs[0], self._sort_geom(P), main_h)
                    self._pos[i] = None
                if self._pos[i] is None:
                    self._pos[i] = torch.empty(max(P, 1), dtype=torch.int32, device=self.device)
                    check(lib.gslm_depth_positions(self._orders[i].data_ptr(), P, self._pos[i].data_ptr(), main_h),
                          "gslm_depth_positions")
            # 2. the sets' render records in depth space: one pass over the Gaussians per set for the batch's views
            # (gslm_preprocess_views takes at most 8 views per call: a batch above 8 goes in chunks)
            for c0 in range(0, len(idx), 8):
                cidx = idx[c0:c0 + 8]
                vws = (_lib.GslmView * len(cidx))(*[self.views[i] for i in cidx])
                pos = (ctypes.c_void_p * len(cidx))(*[self._pos[i].data_ptr() for i in cidx])
                for a in range(n):
                    ge = (ctypes.c_void_p * len(cidx))(*[sl["geoms"][a].data_ptr() for sl in slots[c0:c0 + 8]])
                    check(lib.gslm_preprocess_views(vws, len(cidx), ctypes.byref(gs[a]), ge,
                                                    slots[0]["geoms"][a].numel(), pos, main_h), "gslm_preprocess_views")
            # 3. union geometries and their pair counts (main stream; the read-back waits for main only)
            for k, i in enumerate(idx):
                ge = (ctypes.c_void_p * n)(*[slots[k]["geoms"][a].data_ptr() for a in range(n)])
                check(lib.gslm_union_geometry(ctypes.byref(self.views[i]), P, ge, n, slots[k]["geoms"][0].numel(),
                                              slots[k]["ugeom"].data_ptr(), slots[k]["ugeom"].numel(), main_h),
                      "gslm_union_geometry")
            ugeoms = (ctypes.c_void_p * len(idx))(*[sl["ugeom"].data_ptr() for sl in slots])
            Ps = (ctypes.c_int64 * len(idx))(*([P] * len(idx)))
            Ns = (ctypes.c_int64 * len(idx))()
            check(lib.gslm_num_rendered_many(ugeoms, Ps, len(idx), Ns, main_h), "gslm_num_rendered_many")
            # 4. binning + the n blends of each view on its side stream
            for st in side:
                st.wait_stream(main)
            for k, (sl, i) in enumerate(zip(slots, idx)):
                vw = self.views[i]
                H, W, N = vw.image_height, vw.image_width, int(Ns[k])
                self.union_counts[i] = N
                st, sh = self._stream(k)
                # (an old list is freed on the main stream: after its last use on the view's)
                binning = self.ubins[k] = _grown(self.ubins[k], lib.gslm_union_binning_bytes(N, H, W), self.device,
                                                 main, st)
                ge =(ctypes.c_void_p * n)(*[sl["geoms"][a].data_ptr() for a in range(n)])
                sb = sl["geoms"][0].numel()
                check(lib.gslm_union_binning(ctypes.byref(vw), P, sl["ugeom"].data_ptr(), binning.data_ptr(),
                                             binning.numel(), N, ge, n, sb, sh), "gslm_union_binning")
                mp = self._mask_ptr(i)
                xoff = 48 * self.exp_idx[i] if xs is not None else 0
                dt = self.depth[i]
                if self.loss_sets > 1 and dt is None:  # groups of loss_sets sets, one pass over the union list each
                    gsz = min(self.loss_sets, n)
                    scr = self._sets_scratch(k, gsz, H, W)
                    for a0 in range(0, n, gsz):
                        na = min(gsz, n - a0)
                        gg = (ctypes.c_void_p * na)(*[sl["geoms"][a].data_ptr() for a in range(a0, a0 + na)])
                        lp = (ctypes.c_void_p * na)(*[losses[a].data_ptr() + 8 * i for a in range(a0, a0 + na)])
                        if xs is not None:
                            xp = (ctypes.c_void_p * na)(*[xs[a] + xoff for a in range(a0, a0 + na)])
                            check(lib.gslm_rasterize_loss_sets_exposure(
                                ctypes.byref(vw), P, gg, na, a0, sb, binning.data_ptr(), binning.numel(), N,
                                self.gts[i].data_ptr(), mp, xp, scr.data_ptr(), scr.numel() * 8, lp, 0, sh),
                                "gslm_rasterize_loss_sets_exposure")
                            continue
                        if self._robust is not None:
                            check(lib.gslm_rasterize_loss_sets_robust(
                                ctypes.byref(vw), P, gg, na, a0, sb, binning.data_ptr(), binning.numel(), N,
                                self.gts[i].data_ptr(), mp, ctypes.byref(self._robust), scr.data_ptr(),
                                scr.numel() * 8, lp, 0, sh), "gslm_rasterize_loss_sets_robust")
                            continue
                        check(lib.gslm_rasterize_loss_sets(ctypes.byref(vw), P, gg, na, a0, sb, binning.data_ptr(),
                                                           binning.numel(), N, self.gts[i].data_ptr(), mp,
                                                           scr.data_ptr(), scr.numel() * 8, lp, 0, sh),
                              "gslm_rasterize_loss_sets")
                    continue
                scr = self.loss_scratch[k % len(self.streams)]
                for a in range(n):
                    if dt is not None:  # (no all-sets form with depth: per set whatever loss_sets says)
                        check(lib.gslm_rasterize_loss_slot_depth(
                            ctypes.byref(vw), P, sl["geoms"][a].data_ptr(), sb, binning.data_ptr(), binning.numel(), N,
                            a, n, self.gts[i].data_ptr(), mp, dt[0].data_ptr(),
                            None if dt[1] is None else dt[1].data_ptr(), self.depth_weight, scr.data_ptr(),
                            scr.numel() * 8, losses[a].data_ptr() + 8 * i, 0, sh), "gslm_rasterize_loss_slot_depth")
                        continue
                    if xs is not None:
                        check(lib.gslm_rasterize_loss_slot_exposure(
                            ctypes.byref(vw), P, sl["geoms"][a].data_ptr(), sb, binning.data_ptr(), binning.numel(), N,
                            a, n, self.gts[i].data_ptr(), mp, xs[a] + xoff, scr.data_ptr(), scr.numel() * 8,
                            losses[a].data_ptr() + 8 * i, 0, sh), "gslm_rasterize_loss_slot_exposure")
                        continue
                    if self._robust is not None:
                        check(lib.gslm_rasterize_loss_slot_robust(
                            ctypes.byref(vw), P, sl["geoms"][a].data_ptr(), sb, binning.data_ptr(), binning.numel(), N,
                            a, n, self.gts[i].data_ptr(), mp, ctypes.byref(self._robust), scr.data_ptr(),
                            scr.numel() * 8, losses[a].data_ptr() + 8 * i, 0, sh), "gslm_rasterize_loss_slot_robust")
                        continue
                    check(lib.gslm_rasterize_loss_slot(ctypes.byref(vw), P, sl["geoms"][a].data_ptr(), sb,
                                                       binning.data_ptr(), binning.numel(), N, a, n, self.gts[i].data_ptr(),
                                                       mp, scr.data_ptr(), scr.numel() * 8,
                                                       losses[a].data_ptr() + 8 * i, 0, sh), "gslm_rasterize_loss_slot")
            if side:
                evs = []
                for st in side:
                    ev = torch.cuda.Event()
                    ev.record(st)
                    evs.append(ev)
                done[par] = evs
        for st in side:
            main.wait_stream(st)
        return [self._total(losses[a]) for a in range(n)]


_LS_GROUPS = ("_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


def param_snapshot(model, exposure=False):
    """A line-search point's parameters for LossEvaluator.evaluate_points: clones of the groups the LM step moves,
    the model's own (frozen) xyz tensor.  exposure=True also clones model._exposure, for an evaluator with
    fused_exposure (lm_step(train_exposure=True, val_exposure="fused")); without it the exposure group is not part
    of a snapshot."""
    import types
    ns = types.SimpleNamespace(_xyz=model._xyz, active_sh_degree=model.active_sh_degree)
    with torch.no_grad():
        for k in _LS_GROUPS + (("_exposure",) if exposure else ()):
            setattr(ns, k, getattr(model, k).detach().clone())
    return ns


def update_params(model, layout, step, scale, skip_xyz=False):
    """GaussianModel.update_step(scale * s) (gaussian_model.py:131-139) from a flat step.  skip_xyz: the step's xyz
    group is zero by construction (the LM step's param mask, train_jvp.py:221-227), so adding it would change no
    value -- it is left alone, which keeps model._xyz's version (the line search's cached depth orders)."""
    v = layout.views(step)
    with torch.no_grad():
        if not skip_xyz:
            model._xyz.add_(v["xyz"], alpha=scale)
        model._features_dc.add_(v["features_dc"], alpha=scale)
        model._features_rest.add_(v["features_rest"], alpha=scale)
        model._scaling.add_(v["scaling"], alpha=scale)
        model._rotation.add_(v["rotation"], alpha=scale)
        model._opacity.add_(v["opacity"], alpha=scale)
        model._exposure.add_(v["exposure"], alpha=scale)


_VAL_CACHE = {}  # lm_step's last validation evaluator: {"last": (key, evaluator)}


def clear_val_cache():
    """Release the validation evaluator lm_step keeps between LM steps (its workspaces -- evaluate_points' peak, see
    LossEvaluator._uslot -- the views' depth orders, and its references to the model and the validation cameras)."""
    _VAL_CACHE.clear()


def lm_step(model, cams, val_cams, bg, max_iter=2, restart_iter=1, damp=None, mask_xyz=True, check_every=True,
            verbose=False, device="cuda", sh_projection="auto", recursion="fused", exchange="auto", group=None,
            val_batch=8, timing=False, backend=None, line_search="union", val_at_start=False, cache_val=True,
            multiview="loop", union_active=False, train_exposure=False, val_exposure="forward", precond=None,
            damping="fixed", marquardt_floor=0.0, robust=None, depth_weight=None):
    """One LM step of train_jvp.py:237-289: loss, CGLS on the normal equations, backtracking line search.

    Single process: LMProblem over `cams` (with one training view the SH-rest group of the CG vectors is carried
    projected).  Under torch.distributed (several ranks, or GSLM_FORCE_COLLECTIVES=1 at one rank) the step runs
    sharded, every rank calling lm_step with the same arguments: the training views are split over the ranks
    (gslm.parallel.ShardedLMProblem -- Gaussian-sharded CG vectors when every rank holds as many views, else the
    replicated-vector exchanges), the step is gathered whole on every rank (gather_full), the validation views are
    split the same way and each line-search loss is one 8-byte all-reduce, and every rank applies the identical
    update_step -- the replicas stay bitwise equal.
    recursion: "fused" (cgls_fused, one fused (J^T J + D) p per iteration) or "cgls" (cgls_residual, the
    reference's residual-space recursion; single process only).  check_every: the reference's stopping tests,
    on the device (cgls_fused).  timing=True adds wall-clock phases (evaluate + J^T b, CG, line search) to the
    result, synchronising the device at their boundaries.
    line_search: "union" (xyz masked: the six points' parameters are formed first by the same update_step sequence
    and their validation losses come from ONE binning per view, LossEvaluator.evaluate_points -- bitwise the losses of
    the sequential renders; the final point, known only after them, is rendered as before) or "exact" (train_jvp.py's
    order: update, render, update, ...).  val_at_start: also report the validation loss at the starting parameters
    (one more evaluation, outside the reference's algorithm: it shows whether the step descends).  cache_val: keep the
    validation evaluator for the next LM step (its workspaces and cached depth orders; clear_val_cache() releases it;
    the views are rebuilt from the cameras every step, so a moved camera is rendered at its new pose).
    multiview: "loop" (LMProblem: the whole fused product once per training view) or "batched" (BatchedLMProblem: one
    tangent pass and one gather over the Gaussians for all the views, the SH-rest group in the views' coordinates;
    single process, recursion="fused", mask_xyz=True -- anything else raises ValueError; with one training view the
    existing path runs) or "batched_xyz" (BatchedXyzLMProblem: the same batch with the positions free; single process,
    recursion="fused" and mask_xyz=False, which must be passed -- anything else raises ValueError; the rest is what the
    loop's mask_xyz=False step does: the line search in the exact order and update_params with the xyz group).  The
    step comes back in the reference's layout in every case.
    union_active: multiview="batched" only (else ValueError): the batched solve runs on the Gaussians at least one
    training view can move (BatchedLMProblem(union_active=True)); off by default.
    train_exposure: the step also moves the exposure rows of the training cameras (LMProblem(train_exposure=True)),
    and the validation loss is taken under each validation camera's exposure (LossEvaluator(train_exposure=True)).
    Single process, multiview="loop", recursion="fused", mask_xyz=True -- anything else raises ValueError.  Off by
    default: nothing changes, and model._exposure is not touched.
    val_exposure (train_exposure=True only; any other string, or "fused" without it, raises ValueError): "forward"
    renders each validation view with the full forward and takes the exposure residual's loss of the image, one view
    after the other, and the line search runs in the exact order whatever line_search says.  "fused" applies the
    exposure in the loss blend's epilogue (LossEvaluator(fused_exposure=True)): the validation runs in batches over the
    side streams, and line_search="union" snapshots the six points with their exposure and evaluates them through one
    binning per view; line_search="exact" runs the fused evaluation seven times.
    precond: None (cgls_fused, today's step launch for launch) or "jacobi" (cgls_jacobi: CG preconditioned with
    diag(J^T J + D), LMProblem.diagonal; the result and its cg info report precond="jacobi").  Any other string raises
    ValueError, and so does "jacobi" with recursion="cgls", train_exposure=True, multiview="batched", a sharded run,
    mask_xyz=False or a backend (the SSIM residual, which lm_step does not run, is refused by cgls_jacobi itself).
    damping: "fixed" (today's step, launch for launch) or "marquardt" (LMProblem(damping="marquardt"): D = lambda
    max(diag(J^T W J), marquardt_floor) in the layout the solve runs in, `damp` the per-group lambda, which must be
    given).  The single-process step with multiview="loop", recursion="fused", mask_xyz=True, no trained exposure and
    no backend, with either precond -- anything else, another string, or a marquardt_floor without it raises
    ValueError.  The result reports `damping`.
    robust: None (today's step, launch for launch), ("huber", delta) or ("cauchy", delta): the step minimises
    2 sum rho(r^2) by iteratively reweighted least squares (LMProblem(robust=...)) and the line search takes the same
    robust loss on the validation views (LossEvaluator(robust=...)).  With either multiview, union_active, either
    precond, either damping and either line_search; ValueError for anything else than the three forms, and for a
    sharded run, a backend, recursion="cgls", train_exposure=True or mask_xyz=False.  The result reports `robust`.
    depth_weight: None (today's step, launch for launch) or lambda_d >= 0: the step also minimises the inverse-depth
    residual lambda_d sum (m_d (D - Dgt))^2 of every training camera that carries a target (invdepthmap with
    depth_reliable set, and depth_mask; LMProblem(depth_weight=...)), and the line search takes the combined loss on
    the validation cameras (LossEvaluator(depth_weight=...)).  The single-process step with multiview="loop",
    recursion="fused", mask_xyz=True, precond=None and damping="fixed", without trained exposure, a robust loss or a
    backend -- anything else, or a weight that is negative or not finite, raises ValueError.  The result reports
    `depth_weight`.
    backend: (problem_cls, evaluator_cls, solver) replacing (LMProblem, LossEvaluator, cgls_fused) -- the CPU
    multi-process tests run this same driver, sharding and reductions on the oracle restatement."""
    import time
    from gslm.parallel import ShardedLMProblem, allreduce_loss, collectives_on, shard_views, world
    rank, n = world()
    sharded = collectives_on(n)
    problem_cls, evaluator_cls, solver = backend if backend is not None else (LMProblem, LossEvaluator, cgls_fused)
    if multiview not in ("loop", "batched", "batched_xyz"):
        raise ValueError(f"multiview must be 'loop', 'batched' or 'batched_xyz', got {multiview!r}")
    if multiview == "batched":
        if sharded or backend is not None or recursion != "fused" or not mask_xyz:
            raise ValueError("multiview='batched' is the single-process HIP problem with recursion='fused' and "
                             "mask_xyz=True (multiview='batched_xyz' is the batch with the positions free)")
        if len(cams) > 1:
            problem_cls = BatchedLMProblem
    elif multiview == "batched_xyz":
        if sharded or backend is not None or recursion != "fused" or mask_xyz or union_active:
            raise ValueError("multiview='batched_xyz' is the single-process HIP problem with recursion='fused' and "
                             "mask_xyz=False, without union_active (the list's kernels are masked forms)")
        if len(cams) > 1:
            problem_cls = BatchedXyzLMProblem
    elif union_active:
        raise ValueError("union_active=True is an option of multiview='batched'")
    if train_exposure and (sharded or multiview != "loop" or recursion != "fused" or not mask_xyz):
        raise ValueError("train_exposure=True is the single-process step with multiview='loop', recursion='fused' "
                         "and mask_xyz=True")
    if val_exposure not in ("forward", "fused"):
        raise ValueError(f"val_exposure must be 'forward' or 'fused', got {val_exposure!r}")
    if val_exposure == "fused" and not train_exposure:
        raise ValueError("val_exposure='fused' is an option of train_exposure=True")
    if precond not in (None, "jacobi"):
        raise ValueError(f"precond must be None or 'jacobi', got {precond!r}")
    if precond == "jacobi":
        if (sharded or backend is not None or recursion != "fused" or not mask_xyz or train_exposure or
                multiview != "loop"):
            raise ValueError("precond='jacobi' is the single-process step with multiview='loop', recursion='fused', "
                             "mask_xyz=True and no trained exposure")
        solver = cgls_jacobi
    if damping not in ("fixed", "marquardt"):
        raise ValueError(f"damping must be 'fixed' or 'marquardt', got {damping!r}")
    if damping == "marquardt":
        if (sharded or backend is not None or recursion != "fused" or not mask_xyz or train_exposure or
                multiview != "loop"):
            raise ValueError("damping='marquardt' is the single-process step with multiview='loop', recursion='fused', "
                             "mask_xyz=True, no trained exposure and no backend")
        if damp is None:
            raise ValueError("damping='marquardt': damp is the per-group multiplier lambda and must be given")
    elif marquardt_floor != 0.0:
        raise ValueError("marquardt_floor is an option of damping='marquardt'")
    robust = robust_option(robust)
    if robust is not None and (sharded or backend is not None or recursion != "fused" or train_exposure or
                               not mask_xyz):
        raise ValueError("robust is the single-process step with recursion='fused', mask_xyz=True, no trained "
                         "exposure and no backend")
    depth_weight = depth_option(depth_weight)
    if depth_weight is not None and (sharded or backend is not None or recursion != "fused" or train_exposure or
                                     not mask_xyz or robust is not None or precond is not None or
                                     damping != "fixed" or (multiview == "batched" and len(cams) > 1)):
        raise ValueError("depth_weight is the single-process step with multiview='loop', recursion='fused', "
                         "mask_xyz=True, precond=None and damping='fixed': no trained exposure, robust loss or "
                         "backend")
    rob_kw = {"robust": robust} if robust is not None else {}
    if depth_weight is not None:
        rob_kw["depth_weight"] = depth_weight  # (the problem and the evaluator take it as they take `robust`)
    exp_kw = {"train_exposure": True} if train_exposure else {}
    damp_kw = {"damping": "marquardt", "marquardt_floor": marquardt_floor} if damping == "marquardt" else {}
    fused_exposure = val_exposure == "fused"
    t = {}
    clock = [time.perf_counter()]

    def lap(name):
        if timing:
            if torch.device(device).type == "cuda":
                torch.cuda.synchronize(device)
            now = time.perf_counter()
            t[name] = 1e3 * (now - clock[0])
            clock[0] = now

    if sharded:
        if recursion != "fused":
            raise ValueError("the sharded LM step runs cgls_fused")
        mine = [cams[i] for i in shard_views(len(cams), rank, n)]
        prob = ShardedLMProblem(model, mine, bg, group=group, all_cams=cams, exchange=exchange, mask_xyz=mask_xyz,
                                damp=damp, device=device, problem_cls=problem_cls)
    else:
        kw = {"union_active": True} if (union_active and problem_cls is BatchedLMProblem) else {}
        prob = problem_cls(model, cams, bg, mask_xyz=mask_xyz, damp=damp, device=device, sh_projection=sh_projection,
                           **kw, **exp_kw, **damp_kw, **rob_kw)
    start_loss = prob.evaluate()
    if recursion == "cgls":
        lap("evaluate_rhs_ms")
        s, info = cgls_residual(prob, max_iter=max_iter, restart_iter=restart_iter, verbose=verbose)
    elif recursion == "fused":
        g = prob.rhs(prob.zeros())
        lap("evaluate_rhs_ms")
        s, info = solver(prob, g, max_iter=max_iter, restart_iter=restart_iter, check_every=check_every,
                         verbose=verbose)
    else:
        raise ValueError(f"recursion must be 'fused' or 'cgls', got {recursion!r}")
    # the whole step in the reference's layout, identical on every rank
    s = prob.gather_full(s) if getattr(prob, "exchange", None) == "gaussian" else getattr(prob, "expand", lambda v: v)(s)
    if not bool(torch.isfinite(s).all()):
        # the reference's NaN asserts (solver_functions.py:125-130) on the step itself, before update_params touches the
        # model -- for solves without the device stopping tests (which raise inside cgls_fused, naming the groups);
        # s is the gathered step, the same on every rank, so every rank raises here and none waits in a collective
        raise NonFiniteError("NaN detected in the LM step (the CGLS solution)")
    start_loss = float(start_loss)
    del prob
    lap("cg_ms")
    full = ParamLayout(model._xyz.shape[0], 1 + model._features_rest.shape[1], model._exposure.shape[0])
    mine_val = [val_cams[i] for i in shard_views(len(val_cams), rank, n)] if sharded else val_cams
    # the validation evaluator (its workspaces and the views' cached depth orders) is kept from one LM step to the
    # next while the model, the validation cameras (held by it, so their ids stay theirs) and the settings are the same
    imgs = [(getattr(c, "original_image", None), getattr(c, "alpha_mask", None)) for c in mine_val]
    vkey = (id(model), model.active_sh_degree, tuple(id(c) for c in mine_val), tuple(id(t) for p in imgs for t in p),
            str(device), val_batch, evaluator_cls, sharded, id(group), bool(train_exposure), val_exposure, robust,
            depth_weight, tuple(id(getattr(c, k, None)) for c in mine_val for k in ("invdepthmap", "depth_mask")),
            tuple(float(x) for x in torch.as_tensor(bg).reshape(-1).tolist()))
    hit = _VAL_CACHE.get("last") if cache_val else None
    if hit is not None and hit[0] == vkey:
        val = hit[1]
        if hasattr(val, "refresh_views"):
            val.refresh_views(mine_val, bg, model.active_sh_degree)
    else:
        _VAL_CACHE.pop("last", None)
        val = evaluator_cls(model, mine_val, bg, device=device, batch=val_batch,
                            reduce=(lambda x: allreduce_loss(x, group)) if sharded else None, **exp_kw, **rob_kw,
                            **({"fused_exposure": True} if fused_exposure else {}),
                            # (GSLM_VAL_STREAMS: the side-stream count, an A/B override of LossEvaluator's default)
                            **({"streams": int(os.environ["GSLM_VAL_STREAMS"])} if "GSLM_VAL_STREAMS" in os.environ else {}))
        if cache_val:
            val.held = (model, list(mine_val), imgs)
            _VAL_CACHE["last"] = (vkey, val)
    val_start = float(val.evaluate()) if val_at_start else None
    if val_at_start:
        lap("val_start_ms")
    if line_search not in ("union", "exact"):
        raise ValueError(f"line_search must be 'union' or 'exact', got {line_search!r}")
    union = (line_search == "union" and mask_xyz and hasattr(val, "evaluate_points")
             and (fused_exposure or not train_exposure))
    # train_jvp.py:262-279: alpha = 2, 1, ..., 1/16 on the validation views, keep the best, step to it
    alpha = 2.0
    best_alpha, best_loss = alpha, math.inf
    trace = []
    update_params(model, full, s, alpha, skip_xyz=mask_xyz)
    if union:
        # the same update_step sequence, the six points' parameters kept; their losses from one binning per view
        points = []
        for _ in range(6):
            points.append((alpha, param_snapshot(model, exposure=fused_exposure)))
            new_alpha = alpha * 0.5
            update_params(model, full, s, new_alpha - alpha, skip_xyz=mask_xyz)
            alpha = new_alpha
        alphas = [a for a, _ in points]
        vls = [float(v) for v in val.evaluate_points([p for _, p in points])]
        del points
        for a, vl in zip(alphas, vls):
            trace.append((a, vl))
            if vl < best_loss:
                best_loss, best_alpha = vl, a
    else:
        for _ in range(6):
            vl = float(val.evaluate())
            trace.append((alpha, vl))
            if vl < best_loss:
                best_loss, best_alpha = vl, alpha
            new_alpha = alpha * 0.5
            update_params(model, full, s, new_alpha - alpha, skip_xyz=mask_xyz)
            alpha = new_alpha
    update_params(model, full, s, best_alpha - alpha, skip_xyz=mask_xyz)
    final = float(val.evaluate())
    lap("line_search_ms")
    out = dict(start_loss=start_loss, final_val_loss=final, best_alpha=best_alpha, cg=info, step=s, trace=trace,
               val_views=len(val_cams), ranks=n if sharded else 1, line_search="union" if union else "exact")
    if precond is not None:
        out["precond"] = precond
    if damping != "fixed":
        out["damping"] = damping
    if robust is not None:
        out["robust"] = robust
    if depth_weight is not None:
        out["depth_weight"] = depth_weight
    if val_at_start:
        out["val_start_loss"] = val_start
    if union and getattr(val, "union_counts", None):
        out["union_pairs"] = sum(val.union_counts)
    if timing:
        out["timing"] = t
    return out
