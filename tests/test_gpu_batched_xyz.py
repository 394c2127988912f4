"""gslm.lm.BatchedXyzLMProblem: the batched multi-view LM product with the positions free, and the kernel
under it, gslm_gather_views with GSLM_MV_XYZ (k_gather_views<., false, true>).

1. Against the float64 oracle (oracle.lm_ref.OracleLMProblem(mask_xyz=False)) on the scenes of
   tests/lm_batched_xyz_ref.py: loss, J^T b (expanded) and one product, in SH-rest coordinates and with
   GSLM_SHARD_REST=full, at 8 x the float32 oracle's own distance from the float64 one per group
   (lm_batched_xyz_ref.GPU_TOL).  The oracle test asserts that the xyz part of the direction alone makes up at least a
   quarter of the product in every group, so a dropped dmean or a lost xyz tangent cannot pass these bounds.
2. Against LMProblem(mask_xyz=False, sh_projection=False), the per-view loop, on the scenes of
   tests/test_gpu_batched_lm.py: the loss equal; J^T b, a product and three CG iterations at that file's 1e-6, 1e-5 and
   1e-4, measured as there but over the groups that file covers (everything but xyz); the xyz group, for which the
   project had no bound, at 8 x its float32 floor relative to the group's max.
3. gslm_gather_views with the flag against V accumulating gslm_matvec_view_ex(mask_xyz = 0, GATHER) calls on the same
   head rows: same row sums (block_sum_rows<3>), same chain, the views summed in index order where the loop adds them to
   y one by one -- rounding-level 1e-6 of each group's max in the full layout (whether the results are in fact bitwise
   equal is printed); in coordinates the SH-rest group is compared expanded, at the 1e-5 of tests/test_gpu_batched_lm.py.
4. The row-map protocol, the options that stay refused, and lm_step.

With GSLM_PARITY_MARGINS set to a file name every measured margin is appended to it as a JSON line."""
import copy
import ctypes
import functools
import json
import math
import os

import pytest
import torch

import lm_batched_xyz_ref as ref
import multiview_scene as ms
from gslm import _lib
from gslm._lib import lib
from gslm.cameras import orbit_cameras
from gslm.model import inverse_sigmoid, synthetic_gaussians
from gslm.params import ParamLayout, raw_gaussians

pytestmark = pytest.mark.gpu
DEV = "cuda"
RENDER, GATHER, OVERWRITE, ALL = 2, 4, 8, 7
TAIL_CLEAN, XYZ = 1, 64


def _record(case, **margins):
    print(case, " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in margins.items()))
    path = os.environ.get("GSLM_PARITY_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=case, **margins)) + "\n")


def _cuda(model, cams):
    model = copy.deepcopy(model).to(DEV)
    cams = [copy.deepcopy(c) for c in cams]
    for c in cams:
        c.to(DEV)
    return model, cams


# ------------------------------------------------------------------ 1. the float64 oracle
@pytest.mark.parametrize("rest", ["coords", "full"])
@pytest.mark.parametrize("name", ref.SCENES)
def test_loss_rhs_and_product_against_the_float64_oracle(name, rest, monkeypatch):
    from gslm.lm import BatchedXyzLMProblem
    monkeypatch.setenv("GSLM_SHARD_REST", rest)
    r = ref.oracle_results(name, True)
    model, cams, bg = ref.scene(name)
    model, cams = _cuda(model, cams)
    B = BatchedXyzLMProblem(model, cams, bg)
    assert B.rest_views == (ref.N_VIEWS if rest == "coords" else 0)
    assert not B.mask_xyz and B._trec.shape[-1] == 12
    L = B.full_layout
    loss = float(B.evaluate())
    eloss = abs(loss - r["loss"]) / r["loss"]
    g = B.expand(B.rhs(B.zeros())).cpu()
    eg = ref.group_errors(g, r["rhs"], L)
    vb = B.project(r["v"].float().to(DEV))
    y = B.expand(B.matvec(vb, B.zeros())).cpu()
    ey = ref.group_errors(y, r["y"], L)
    _record(f"oracle/{name}/{rest}", loss=eloss, **{f"rhs_{k}": v for k, v in eg.items()},
            **{f"product_{k}": v for k, v in ey.items()})
    assert eloss <= ref.GPU_TOL["loss"]
    for k in ref.GROUPS6:
        assert eg[k] <= ref.GPU_TOL["rhs"][k], ("rhs", k, eg[k])
        assert ey[k] <= ref.GPU_TOL["product"][k], ("product", k, ey[k])
    e0, e1 = L.offsets["exposure"]
    assert not g[e0:e1].any()


# ------------------------------------------------------------------ 2. the per-view loop
W, H = 96, 72
CASES = [(2, 6000), (5, 6001), (9, 2000)]


def _scene(nv, P):
    model = synthetic_gaussians(P, 3, seed=0, s0=0.03, n_cams=nv)
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(10 + i)) for i in range(nv)]
    cams = orbit_cameras(nv, W, H, seed=1, images=gts)
    model = model.to(DEV)
    for c in cams:
        c.to(DEV)
    return model, cams


def _direction(layout):
    """A generic direction with its xyz part (the exposure tail zero)."""
    v = torch.randn(layout.numel, generator=torch.Generator().manual_seed(3))
    a, b = layout.offsets["exposure"]
    v[a:b] = 0
    return v.to(DEV)


@functools.lru_cache(maxsize=None)
def _pair(nv, P):
    """(loop, batched, reference results of the loop): built and evaluated once per case, then only read."""
    from gslm.lm import BatchedXyzLMProblem, LMProblem, cgls_fused
    model, cams = _scene(nv, P)
    A = LMProblem(model, cams, torch.zeros(3), mask_xyz=False, sh_projection=False)
    B = BatchedXyzLMProblem(model, cams, torch.zeros(3))
    la, lb = A.evaluate(), B.evaluate()
    ga = A.rhs(A.zeros())
    v = B.expand(B.project(_direction(A.layout)))  # in the views' span, where every CG iterate lives
    out = {"loss": float(la), "loss_b": float(lb), "g": ga, "v": v, "y": A.matvec(v, A.zeros())}
    for ce in (False, True):
        out["x", ce] = cgls_fused(A, ga, max_iter=3, restart_iter=3, check_every=ce)[0]
    torch.cuda.synchronize()
    return A, B, out


def _split(layout, vec):
    """(the xyz group, everything else) of a vector of the reference's layout."""
    a, b = layout.offsets["xyz"]
    assert a == 0
    return vec[a:b], vec[b:]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("nv,P", CASES)
def test_layout_loss_rhs_and_product_match_the_loop(nv, P):
    A, B, r = _pair(nv, P)
    L = A.layout
    assert B.rest_views == (nv if nv <= 8 else 0)
    assert B.layout.numel == (L.numel - P * 3 * (15 - nv) if nv <= 8 else L.numel)
    assert B.full_layout.numel == L.numel and B.active_view() is None
    assert r["loss_b"] == r["loss"]  # the same forwards and residual epilogues
    g = B.rhs(B.zeros())
    assert B.exposure_is_zero(g)
    (gx, go), (rx, ro) = _split(L, B.expand(g)), _split(L, r["g"])
    assert float(rx.abs().max()) > 0  # J^T b has an xyz group
    y = B.expand(B.matvec(B.project(r["v"]), B.zeros()))
    (yx, yo), (sx, so) = _split(L, y), _split(L, r["y"])
    m = dict(rhs=_rel(go, ro), rhs_xyz=_rel(gx, rx), product=_rel(yo, so), product_xyz=_rel(yx, sx))
    # <v, y> comes fused for any V, the xyz group included
    dot = torch.zeros(1, dtype=torch.float64, device=DEV)
    vb = B.project(r["v"])
    yb = B.zeros()
    assert B.matvec_dot(vb, yb, dot.data_ptr()) is True
    scale = float((vb.double() * yb.double()).abs().sum())
    m["dot"] = abs(float(dot) - float((vb.double() * yb.double()).sum())) / scale
    a, b = B.layout.offsets["xyz"]
    m["dot_xyz_share"] = float((vb[a:b].double() * yb[a:b].double()).abs().sum()) / scale
    _record(f"loop/V{nv}_P{P}", **m)
    assert m["rhs"] <= 1e-6 and m["product"] <= 1e-5
    assert m["rhs_xyz"] <= ref.GPU_TOL["rhs"]["xyz"]
    assert m["product_xyz"] <= ref.GPU_TOL["product"]["xyz"]
    assert m["dot"] <= 1e-12
    assert m["dot_xyz_share"] > 0.1  # (a dot without the xyz group would miss the bound above by far)


@pytest.mark.parametrize("check_every", [False, True])
@pytest.mark.parametrize("nv,P", CASES)
def test_three_cg_iterations_match_the_loop(nv, P, check_every):
    from gslm.lm import cgls_fused
    A, B, r = _pair(nv, P)
    g = B.rhs(B.zeros())
    x, _ = cgls_fused(B, g, max_iter=3, restart_iter=3, check_every=check_every)
    (xx, xo), (rx, ro) = _split(A.layout, B.expand(x)), _split(A.layout, r["x", check_every])
    err = float((xo - ro).norm() / ro.norm())
    errx = _rel(xx, rx)
    _record(f"loop_cg/V{nv}_P{P}_check{int(check_every)}", solve=err, solve_xyz=errx)
    assert float(rx.abs().max()) > 0  # the solve moves xyz
    assert err <= 1e-4
    assert errx <= ref.GPU_TOL["solve"]["xyz"]


# ------------------------------------------------------------------ 3. the gather, through the C ABI
class Rig:
    """One geometry (forwards + residual weights of every view) and the buffers of one unmasked product's stages."""

    def __init__(self, P, V, D, coords, empty_at=None, mutate=None):
        model, cams = ms.scene(P, V, D)
        model = copy.deepcopy(model)
        if mutate is not None:
            with torch.no_grad():
                mutate(model)
        model = model.to(DEV)
        cams = [copy.deepcopy(c) for c in cams]
        if empty_at is not None:
            cams.insert(empty_at, ms.empty_camera())
        for c in cams:
            c.to(DEV)
        from gslm.lm import DEFAULT_DAMP, LMProblem
        self.P, self.V, self.D = P, len(cams), D
        self.prob = LMProblem(model, cams, torch.zeros(3), mask_xyz=False, sh_projection=False)
        self.prob.evaluate()
        self.st = self.prob.stream
        self.full = self.prob.full_layout
        self.K = self.full.K
        self.rv = self.V if coords else 0
        assert not coords or (self.K > 1 and self.V <= _lib.GSLM_MAX_REST_VIEWS)
        self.layout = ParamLayout(P, self.K, self.full.n_exposure, rest_views=self.rv)
        _, self.damps = self.full.group_damp_arrays(DEFAULT_DAMP)
        self.g = raw_gaussians(model)
        self.views = [vr.view for vr in self.prob.views]
        self.flags = torch.zeros(self.V, P, dtype=torch.int32, device=DEV)
        for b, vr in enumerate(self.prob.views):
            _lib.check(lib.gslm_view_flags(vr.geom.data_ptr(), P, self.flags[b].data_ptr(), self.st))
        self.R = None
        if self.rv:
            self.R = torch.zeros(P * self.rv * (self.rv + 1) // 2, dtype=torch.float32, device=DEV)
            _lib.check(lib.gslm_rest_basis(self._views(range(self.V)), self.rv, ctypes.byref(self.g),
                                           self.R.data_ptr(), self.st))
        self.trec = torch.zeros(self.V, P, 12, dtype=torch.float32, device=DEV)

    def _views(self, idx):
        idx = list(idx)
        return (_lib.GslmView * max(len(idx), 1))(*[self.views[b] for b in idx])

    def tiles(self):
        """[V, P] tile counts as the library holds them (gslm_inspect)."""
        out = torch.zeros(self.V, self.P, dtype=torch.int32, device=DEV)
        for b, vr in enumerate(self.prob.views):
            _lib.check(lib.gslm_inspect(vr.geom.data_ptr(), self.P, vr.binning.data_ptr(), vr.N, vr.H, vr.W,
                                        vr.image.data_ptr(), None, None, out[b].data_ptr(), None, None, None, self.st))
        torch.cuda.synchronize()
        return out.cpu()

    def block_rows(self, b):
        """Head rows of view b owned by each block of 256 consecutive Gaussians (gslm_inspect_rowmap; after render())."""
        vr, P = self.prob.views[b], self.P
        goff = torch.zeros(P, dtype=torch.int32, device=DEV)
        hscan = torch.zeros(vr.N + 1, dtype=torch.int32, device=DEV)
        _lib.check(lib.gslm_inspect_rowmap(vr.geom.data_ptr(), P, vr.N, vr.scratch.data_ptr(), vr.scratch.numel(),
                                           goff.data_ptr(), hscan.data_ptr(), self.st))
        torch.cuda.synchronize()
        tiles, goff, hscan = self.tiles()[b].long(), goff.cpu().long(), hscan.cpu().long()
        out = []
        for i0 in range(0, P, 256):
            il = min(i0 + 256, P) - 1
            out.append(int(hscan[goff[il] + tiles[il]] - hscan[goff[i0]]))
        return out

    def direction(self, seed=3):
        """In this rig's layout (coordinates or full), xyz included, the exposure tail zero."""
        v = torch.randn(self.layout.numel, generator=torch.Generator().manual_seed(seed))
        a, b = self.layout.offsets["exposure"]
        v[a:b] = 0
        return v.to(DEV)

    def expand(self, x):
        """A vector of this rig's layout in the reference's (gslm_rest_coords; x itself in the full layout)."""
        if not self.rv:
            return x
        out = torch.zeros(self.full.numel, dtype=torch.float32, device=DEV)
        for name in ref.GROUPS6 + ("exposure",):
            if name != "features_rest":
                (a0, a1), (b0, b1) = self.layout.offsets[name], self.full.offsets[name]
                out[b0:b1] = x[a0:a1]
        a0, b0 = self.layout.offsets["features_rest"][0], self.full.offsets["features_rest"][0]
        _lib.check(lib.gslm_rest_coords(self._views(range(self.V)), self.rv, ctypes.byref(self.g), self.R.data_ptr(), 0,
                                        x.data_ptr() + 4 * a0, 3 * self.layout.rest_rows, out.data_ptr() + 4 * b0,
                                        3 * self.full.rest_rows, self.st), "gslm_rest_coords")
        return out

    def render(self, v, trec_floats=12):
        """One unmasked product's stages up to the rows: every view's [P][12] tangent records, then per view the fused
        tile pass from its slice of the table into 48-byte head rows."""
        vs = self.layout.grads_struct(v)
        opts = _lib.GslmMatvecOpts()
        if self.R is not None:
            opts.rest_basis, opts.rest_views, opts.view_base = self.R.data_ptr(), self.rv, 0
        _lib.check(lib.gslm_tangent_views(self._views(range(self.V)), self.V, ctypes.byref(self.g), ctypes.byref(vs), 0,
                                          self.flags.data_ptr(), self.P, self.trec.data_ptr(), self.P,
                                          ctypes.byref(opts), self.st), "gslm_tangent_views")
        for b, vr in enumerate(self.prob.views):
            o = _lib.GslmMatvecOpts()
            o.stages = RENDER
            o.flags = TAIL_CLEAN if vr.tail_clean else 0
            o.trec_in = self.trec[b].data_ptr()
            _lib.check(lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(self.g), ctypes.byref(vs),
                                               self.prob.weights[b].data_ptr(), 0, vr.geom.data_ptr(),
                                               vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(),
                                               vr.scratch.numel(), ctypes.byref(vs), ctypes.byref(o), self.st),
                       "gslm_matvec_view_ex")
            vr.tail_clean = True

    def _opts(self, stages, damp, dot, ctl=None):
        o = _lib.GslmMatvecOpts()
        o.stages = stages
        o.damp7 = self.damps if damp else None
        if dot is not None:
            o.dot_vy = dot.data_ptr()
            o.dot_scratch = self.prob.dot_scratch.data_ptr()
            o.dot_scratch_bytes = self.prob.dot_scratch.numel() * 8
        o.cg_ctl = None if ctl is None else ctl.data_ptr()
        return o

    def ws(self, idx):
        idx = list(idx)
        ws = (_lib.GslmViewWs * max(len(idx), 1))()
        for k, b in enumerate(idx):
            vr = self.prob.views[b]
            ws[k].geom, ws[k].scratch = vr.geom.data_ptr(), vr.scratch.data_ptr()
            ws[k].scratch_bytes, ws[k].num_rendered = vr.scratch.numel(), vr.N
        return ws

    def gather_views(self, v, y, idx=None, overwrite=True, damp=True, dot=None, ctl=None):
        """gslm_gather_views with GSLM_MV_XYZ, in this rig's layout."""
        idx = list(range(self.V)) if idx is None else list(idx)
        vs, ys = self.layout.grads_struct(v), self.layout.grads_struct(y)
        o = self._opts(ALL | (OVERWRITE if overwrite else 0), damp, dot, ctl)
        o.flags = XYZ
        if self.R is not None:
            o.rest_basis, o.rest_views, o.view_base = self.R.data_ptr(), self.rv, idx[0]
        _lib.check(lib.gslm_gather_views(self._views(idx), self.ws(idx), len(idx), ctypes.byref(self.g),
                                         ctypes.byref(vs), ctypes.byref(ys), ctypes.byref(o), self.st),
                   "gslm_gather_views")
        return y

    def gather_loop(self, v_full, y_full, idx=None, overwrite=True, damp=True, dot=None):
        """The reference: one gslm_matvec_view_ex(mask_xyz = 0, GATHER) per view that rendered, accumulating into y (the
        first with OVERWRITE and the damping, the last with the dot), in the reference's layout."""
        idx = [b for b in (range(self.V) if idx is None else idx) if self.prob.views[b].N > 0]
        vs, ys = self.full.grads_struct(v_full), self.full.grads_struct(y_full)
        for k, b in enumerate(idx):
            vr = self.prob.views[b]
            first, last = k == 0, k == len(idx) - 1
            o = self._opts(GATHER | (OVERWRITE if (overwrite and first) else 0), damp and first, dot if last else None)
            o.flags = TAIL_CLEAN
            _lib.check(lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(self.g), ctypes.byref(vs),
                                               self.prob.weights[b].data_ptr(), 0, vr.geom.data_ptr(),
                                               vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(),
                                               vr.scratch.numel(), ctypes.byref(ys), ctypes.byref(o), self.st),
                       "gslm_matvec_view_ex(GATHER)")
        return y_full

    def compare(self, y, y_ref_full, what):
        """Per group, relative to the reference group's max: 1e-6 (1e-5 for the SH-rest group in coordinates)."""
        yf = self.expand(y)
        errs = ref.group_errors(yf.cpu(), y_ref_full.cpu(), self.full)
        bitwise = (not self.rv) and all(
            torch.equal(yf[a:b], y_ref_full[a:b]) for a, b in (self.full.offsets[k] for k in ref.GROUPS6))
        _record(what, bitwise=bool(bitwise), **errs)
        assert torch.isfinite(yf[:self.full.offsets["exposure"][0]]).all()
        for k, e in errs.items():
            assert e <= (1e-5 if (self.rv and k == "features_rest") else 1e-6), (what, k, e)
        return errs


def _prefill(layout, seed=5):
    return torch.randn(layout.numel, generator=torch.Generator().manual_seed(seed)).to(DEV)


GUARD = 64


def _nan_with_guards(n):
    """A NaN-filled vector of n floats between two guard bands (7.25) of one allocation."""
    buf = torch.full((n + 2 * GUARD,), 7.25, dtype=torch.float32, device=DEV)
    y = buf[GUARD:GUARD + n]
    y.fill_(math.nan)
    return buf, y


GATHER_CASES = [(P, V, mode) for P in (255, 256, 257) for V in (1, 2, 16)
                for mode in ("sh3_full", "sh3_coords", "sh0") if not (mode == "sh3_coords" and V > 8)]


@pytest.mark.parametrize("P,V,mode", GATHER_CASES)
def test_gather_views_xyz_matches_the_accumulating_single_view_gathers(P, V, mode):
    rig = Rig(P, V, 0 if mode == "sh0" else 3, coords=(mode == "sh3_coords"))
    none, some, every = ms.visibility_classes(rig.tiles())
    assert none >= 1 and every >= 1 and (V < 2 or some >= 1), (none, some, every)
    v = rig.direction()
    vf = rig.expand(v)
    rig.render(v)
    e0, e1 = rig.layout.offsets["exposure"]
    f0 = rig.full.offsets["exposure"][0]
    case = f"gather/P{P}_V{V}_{mode}"
    # OVERWRITE with damping over a NaN-filled y between guards, and the fused dot
    dot = torch.full((1,), math.nan, dtype=torch.float64, device=DEV)
    dot_ref = torch.full((1,), math.nan, dtype=torch.float64, device=DEV)
    y_ref = rig.gather_loop(vf, torch.full_like(vf, math.nan), dot=dot_ref)
    buf, y = _nan_with_guards(rig.layout.numel)
    rig.gather_views(v, y, dot=dot)
    torch.cuda.synchronize()
    assert torch.equal(buf[:GUARD], torch.full_like(buf[:GUARD], 7.25))
    assert torch.equal(buf[-GUARD:], torch.full_like(buf[-GUARD:], 7.25))
    assert torch.isfinite(y[:e0]).all() and torch.isnan(y[e0:e1]).all()  # (the exposure slice is the caller's)
    y = y.clone()
    y[e0:e1] = 0
    y_ref[f0:] = 0
    errs = rig.compare(y, y_ref, case + "/overwrite")
    host = float((v[:e0].double() * y[:e0].double()).sum())
    scale = float((v[:e0].double() * y[:e0].double()).abs().sum())
    _record(case + "/dot", dot=abs(float(dot) - host) / scale, dot_vs_loop=abs(float(dot) - float(dot_ref)) / scale)
    assert abs(float(dot) - host) <= 1e-12 * scale
    # accumulation, no damping (full layout: the loop has no coordinates to accumulate in)
    if not rig.rv:
        y0 = _prefill(rig.layout, seed=6)
        ya_ref = rig.gather_loop(vf, y0.clone(), overwrite=False, damp=False)
        ya = rig.gather_views(v, y0.clone(), overwrite=False, damp=False)
        assert torch.equal(ya[e0:e1], y0[e0:e1])
        rig.compare(ya, ya_ref, case + "/accumulate")
    # the two modes against each other: (accumulate onto zero, no damping) + D v = overwrite with damping
    yz = rig.gather_views(v, torch.zeros_like(v), overwrite=False, damp=False)
    xa, xb = rig.layout.offsets["xyz"]
    assert float(yz[xa:xb].abs().max()) > 0  # the rows reach y.xyz
    for k, name in enumerate(ref.GROUPS6):
        a, b = rig.layout.offsets[name]
        if b > a:
            yz[a:b] += float(rig.damps[k]) * v[a:b]
            assert _rel(yz[a:b], y[a:b]) <= 1e-6, name
    # reproducible: no atomics, a fixed order of every sum
    y2 = rig.gather_views(v, _prefill(rig.layout, seed=7))
    y2[e0:e1] = 0
    assert torch.equal(y, y2)


def test_two_eight_view_calls_equal_one_sixteen_view_call():
    rig = Rig(257, 16, 3, coords=False)
    v = rig.direction()
    rig.render(v)
    e0, e1 = rig.layout.offsets["exposure"]
    y16 = rig.gather_views(v, _prefill(rig.layout))
    y8 = rig.gather_views(v, _prefill(rig.layout, seed=8), idx=range(0, 8))
    dot = torch.zeros(1, dtype=torch.float64, device=DEV)
    rig.gather_views(v, y8, idx=range(8, 16), overwrite=False, damp=False, dot=dot)
    y16[e0:e1] = 0
    y8[e0:e1] = 0
    rig.compare(y8, y16, "gather/8+8_against_16")
    scale = float((v.double() * y8.double()).abs().sum())
    assert abs(float(dot) - float((v.double() * y8.double()).sum())) <= 1e-12 * scale


def _big_then_absent(model):
    """Gaussians 0..255 wide and faint (many head rows each, none occluded), 256..511 far outside every view."""
    model._scaling[:256] += math.log(6.0)
    model._opacity[:256] = inverse_sigmoid(torch.tensor(0.05))
    model._xyz[256:512] = torch.tensor([0.0, 0.0, 1000.0]) + torch.rand(256, 3, generator=torch.Generator().manual_seed(1))


@pytest.mark.parametrize("mode", ["sh3_full", "sh3_coords"])
def test_blocks_with_a_long_and_with_an_empty_row_range(mode):
    """A block whose head-row range exceeds GATHER_CHUNK = 512 rows (several LDS chunks of 48-byte rows) and a block
    that owns no row in any view, asserted on the library's own row map."""
    rig = Rig(600, 2, 3, coords=(mode == "sh3_coords"), mutate=_big_then_absent)
    v = rig.direction()
    rig.render(v)
    rows = [rig.block_rows(b) for b in range(rig.V)]
    print("head rows per block and view:", rows)
    assert all(r[0] > 512 for r in rows) and all(r[1] == 0 for r in rows) and all(r[2] > 0 for r in rows)
    vf = rig.expand(v)
    y_ref = rig.gather_loop(vf, torch.full_like(vf, math.nan))
    y = rig.gather_views(v, torch.full_like(v, math.nan))
    y[rig.layout.offsets["exposure"][0]:] = 0
    y_ref[rig.full.offsets["exposure"][0]:] = 0
    rig.compare(y, y_ref, f"gather/long_and_empty_blocks_{mode}")
    # the absent block's y is D v exactly
    for k, name in enumerate(ref.GROUPS6):
        a, b = rig.layout.offsets[name]
        w = (b - a) // rig.P
        sl = slice(a + 256 * w, a + 512 * w)
        assert torch.equal(y[sl], float(rig.damps[k]) * v[sl]), name


def test_empty_view_in_the_middle_is_skipped_and_not_read():
    rig = Rig(257, 3, 3, coords=False, empty_at=1)
    assert [vr.N > 0 for vr in rig.prob.views] == [True, False, True, True]
    v = rig.direction()
    rig.render(v)
    sc = rig.prob.views[1].scratch
    sc[:sc.numel() // 4 * 4].view(torch.float32).fill_(math.nan)  # nothing of it may be read
    e0, e1 = rig.layout.offsets["exposure"]
    y_all = rig.gather_views(v, _prefill(rig.layout))
    y_wo = rig.gather_views(v, _prefill(rig.layout, seed=9), idx=[0, 2, 3])
    y_all[e0:e1] = 0
    y_wo[e0:e1] = 0
    assert torch.isfinite(y_all).all()
    assert torch.equal(y_all, y_wo)
    y_ref = rig.gather_loop(v, torch.zeros_like(v))
    y_ref[e0:e1] = 0
    rig.compare(y_all, y_ref, "gather/empty_view_in_the_middle")
    # an all-empty call still writes D v, the xyz group included
    y_e = rig.gather_views(v, _prefill(rig.layout), idx=[1])
    for k, name in enumerate(ref.GROUPS6):
        a, b = rig.layout.offsets[name]
        assert torch.equal(y_e[a:b], float(rig.damps[k]) * v[a:b]), name


@pytest.mark.parametrize("mode", ["sh3_full", "sh3_coords"])
def test_stopped_solve_leaves_y_and_dot_untouched(mode):
    rig = Rig(257, 2, 3, coords=(mode == "sh3_coords"))
    v = rig.direction()
    rig.render(v)
    ctl = torch.tensor([1.0, 0.0, math.inf, 0.0], dtype=torch.float64, device=DEV)  # gslm_cg_monitor's block, stopped
    y0 = _prefill(rig.layout)
    dot = torch.full((1,), 123.5, dtype=torch.float64, device=DEV)
    y = rig.gather_views(v, y0.clone(), dot=dot, ctl=ctl)
    assert torch.equal(y, y0) and float(dot) == 123.5
    ctl[0] = 0.0  # running: the same call writes both
    y = rig.gather_views(v, y0.clone(), dot=dot, ctl=ctl)
    assert not torch.equal(y, y0) and float(dot) != 123.5


# ------------------------------------------------------------------ 4. protocol and options
def test_row_map_protocol_and_no_shared_state():
    from gslm.lm import BatchedLMProblem, BatchedXyzLMProblem
    model, cams = _scene(3, 3000)
    bg = torch.zeros(3)
    M = BatchedLMProblem(model, cams, bg)  # the masked problem on the same model
    M.evaluate()
    vm = _direction(M.layout)
    a, b = M.layout.offsets["xyz"]
    vm[a:b] = 0
    gm = M.rhs(M.zeros()).clone()
    ym = M.matvec(vm, M.zeros()).clone()

    B = BatchedXyzLMProblem(model, cams, bg)
    B.evaluate()
    assert not any(vr.tail_clean for vr in B.views)
    g = B.rhs(B.zeros())
    assert not any(vr.tail_clean for vr in B.views)  # gslm_backward drops the row maps
    assert B.rhs_is_mine(g) and B.exposure_is_zero(g)
    v = B.project(B.expand(_direction(B.layout)))
    y1 = B.matvec(v, B.zeros()).clone()
    assert all(vr.tail_clean for vr in B.views)  # the first product rebuilt them
    y2 = B.matvec(v, torch.full_like(y1, math.nan))  # the second reuses them (GSLM_MV_TAIL_CLEAN)
    e0, e1 = B.layout.offsets["exposure"]
    assert torch.equal(y1[:e0], y2[:e0])
    F = BatchedXyzLMProblem(model, cams, bg)  # a fresh problem: the same bits
    F.evaluate()
    y3 = F.matvec(v, F.zeros())
    assert torch.equal(y1, y3)
    # nothing of a product depends on what the record table or y held before
    B._trec.fill_(math.nan)
    assert torch.equal(B.matvec(v, torch.full_like(y1, math.nan))[:e0], y1[:e0])
    assert torch.equal(g, B.rhs(B.zeros()))

    # the masked problem gives the bits it gave before the unmasked ones ran
    assert torch.equal(gm, M.rhs(M.zeros()))
    assert torch.equal(ym, M.matvec(vm, M.zeros()))


def test_what_stays_refused():
    from gslm.lm import BatchedLMProblem, BatchedXyzLMProblem, cgls_jacobi, clear_val_cache, lm_step
    model, cams = _scene(3, 500)
    bg = torch.zeros(3)
    with pytest.raises(ValueError, match="union_active"):
        BatchedXyzLMProblem(model, cams, bg, union_active=True)
    with pytest.raises(ValueError, match="robust"):
        BatchedXyzLMProblem(model, cams, bg, robust=("huber", 0.1))
    with pytest.raises(ValueError, match="depth"):
        BatchedXyzLMProblem(model, cams, bg, depth_weight=1.0)
    with pytest.raises(ValueError, match="marquardt"):
        BatchedXyzLMProblem(model, cams, bg, damping="marquardt", damp=dict(DEFAULT_LAMBDA))
    with pytest.raises(ValueError, match="ssim"):
        BatchedXyzLMProblem(model, cams, bg, ssim=True)
    with pytest.raises(ValueError, match="BatchedXyzLMProblem"):
        BatchedLMProblem(model, cams, bg, mask_xyz=False)  # (the masked class keeps its refusal)
    with pytest.raises(ValueError, match="mask_xyz"):
        BatchedXyzLMProblem(model, cams, bg, mask_xyz=True)
    B = BatchedXyzLMProblem(model, cams, bg)
    B.evaluate()
    with pytest.raises(ValueError):
        cgls_jacobi(B, B.rhs(B.zeros()), max_iter=1, restart_iter=1)
    with pytest.raises(ValueError):
        B.diagonal()
    with pytest.raises(ValueError):
        lm_step(copy.deepcopy(model), cams[:2], cams[2:], bg, multiview="batched_xyz")  # (mask_xyz=False must be passed)
    kw = dict(mask_xyz=False, multiview="batched_xyz")
    for bad in (dict(union_active=True), dict(precond="jacobi"), dict(train_exposure=True), dict(robust=("huber", 0.1)),
                dict(depth_weight=1.0), dict(damping="marquardt", damp=dict(DEFAULT_LAMBDA)), dict(recursion="cgls")):
        with pytest.raises(ValueError):
            lm_step(copy.deepcopy(model), cams[:2], cams[2:], bg, **kw, **bad)
    clear_val_cache()


DEFAULT_LAMBDA = {"xyz": 1.0, "features_dc": 1.0, "features_rest": 1.0, "scaling": 1.0, "rotation": 1.0, "opacity": 1.0,
                  "exposure": 1.0}


def test_lm_step_batched_matches_loop_with_xyz_free():
    from gslm.lm import clear_val_cache, lm_step
    m, cams = _scene(7, 4000)
    m2 = copy.deepcopy(m)
    xyz0 = m._xyz.detach().clone()
    a = lm_step(m, cams[:3], cams[3:], torch.zeros(3), max_iter=3, restart_iter=3, multiview="loop", mask_xyz=False)
    b = lm_step(m2, cams[:3], cams[3:], torch.zeros(3), max_iter=3, restart_iter=3, multiview="batched_xyz",
                mask_xyz=False)
    clear_val_cache()
    err = float((a["step"] - b["step"]).norm() / a["step"].norm())
    moved = float((m2._xyz.detach() - xyz0).abs().max())
    _record("lm_step", step=err, moved=moved, alpha_loop=a["best_alpha"], alpha_batched=b["best_alpha"])
    assert a["line_search"] == b["line_search"] == "exact"
    assert a["best_alpha"] == b["best_alpha"]
    assert b["step"].numel() == a["step"].numel()  # the step comes back in the reference's layout
    assert err <= 1e-4
    assert moved > 0 and torch.isfinite(m2._xyz).all()
    x0, x1 = 0, 3 * xyz0.shape[0]
    assert float(b["step"][x0:x1].abs().max()) > 0
