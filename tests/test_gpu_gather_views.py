"""gslm_gather_views against what it fuses.

After one product's RENDER stages (gslm_tangent_views -> RENDER | SCREEN with trec_in, per view) every view's head
rows lie in its scratch and their per-Gaussian sums in a [V][P][8] table.  gslm_gather_views on the scratches must
give what gslm_gather_screen gives on the table: the two run the same row sums over the same 256-Gaussian partition
and the same chain, so the bound is the rounding-level 1e-6 of y's max that tests/test_gpu_dist.py uses for this
path; whether the results are in fact bitwise equal is printed per case.

Cases: P = 255, 256, 257 (a block edge at, just before and just after the last Gaussian) and 6001 (24 blocks, the
last one partial, row ranges longer than one LDS chunk); V = 1, 2, 5, 16; SH 3 in the full layout (every V) and in
gslm_rest_basis coordinates (V <= 8), SH 0 (no rest group).  Every scene holds a Gaussian no view sees, one every
view sees and, from two views on, one that only some see (asserted from the library's tile counts).
The dot's bound is that of tests/test_gpu_active_set.py: 1e-12 of sum |v_i y_i| against the float64 host sum."""
import copy
import ctypes
import math

import pytest
import torch

from gslm import _lib
from gslm._lib import lib
from gslm.lm import DEFAULT_DAMP, LMProblem
from gslm.params import ParamLayout, raw_gaussians
import multiview_scene as ms

pytestmark = pytest.mark.gpu
DEV = "cuda"
RENDER, SCREEN, OVERWRITE, ALL = 2, 16, 8, 7
TAIL_CLEAN = 1


class Rig:
    """One geometry (forwards + residual weights of every view) and the buffers of one product's stages."""

    def __init__(self, P, V, D, coords, empty_at=None):
        model, cams = ms.scene(P, V, D)
        model = copy.deepcopy(model).to(DEV)
        cams = [copy.deepcopy(c) for c in cams]
        if empty_at is not None:
            cams.insert(empty_at, ms.empty_camera())
        for c in cams:
            c.to(DEV)
        self.P, self.V, self.D = P, len(cams), D
        self.prob = LMProblem(model, cams, torch.zeros(3), sh_projection=False)
        self.prob.evaluate()
        self.st = self.prob.stream
        self.K = self.prob.full_layout.K
        self.rv = self.V if coords else 0
        assert not coords or (self.K > 1 and self.V <= _lib.GSLM_MAX_REST_VIEWS)
        self.layout = ParamLayout(P, self.K, self.prob.full_layout.n_exposure, rest_views=self.rv)
        _, self.damps = self.layout.group_damp_arrays(DEFAULT_DAMP)
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
        self.trec = torch.zeros(self.V, P, 8, dtype=torch.float32, device=DEV)
        self.screen = torch.zeros(self.V, P, 8, dtype=torch.float32, device=DEV)

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

    def direction(self, seed=3):
        v = torch.randn(self.layout.numel, generator=torch.Generator().manual_seed(seed))
        for grp in ("xyz", "exposure"):
            a, b = self.layout.offsets[grp]
            v[a:b] = 0
        return v.to(DEV)

    def render(self, v):
        """One product's stages up to the rows: every view's tangent records, then per view the fused tile pass from
        its slice of the table -- and the SCREEN stage's [P][8] sums, the reference path's input."""
        vs = self.layout.grads_struct(v)
        opts = _lib.GslmMatvecOpts()
        if self.R is not None:
            opts.rest_basis, opts.rest_views, opts.view_base = self.R.data_ptr(), self.rv, 0
        _lib.check(lib.gslm_tangent_views(self._views(range(self.V)), self.V, ctypes.byref(self.g), ctypes.byref(vs), 1,
                                          self.flags.data_ptr(), self.P, self.trec.data_ptr(), self.P,
                                          ctypes.byref(opts), self.st), "gslm_tangent_views")
        for b, vr in enumerate(self.prob.views):
            o = _lib.GslmMatvecOpts()
            o.stages = RENDER | (SCREEN if vr.N else 0)  # (no row map, hence no row sums, for a view that rendered nothing)
            o.flags = TAIL_CLEAN if vr.tail_clean else 0
            o.screen_out = self.screen[b].data_ptr()
            o.trec_in = self.trec[b].data_ptr()
            _lib.check(lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(self.g), ctypes.byref(vs),
                                               self.prob.weights[b].data_ptr(), 1, vr.geom.data_ptr(),
                                               vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(),
                                               vr.scratch.numel(), ctypes.byref(vs), ctypes.byref(o), self.st),
                       "gslm_matvec_view_ex")
            vr.tail_clean = True

    def opts(self, overwrite, damp, dot, ctl, view_base=0):
        o = _lib.GslmMatvecOpts()
        o.stages = ALL | (OVERWRITE if overwrite else 0)
        o.damp7 = self.damps if damp else None
        if dot is not None:
            o.dot_vy = dot.data_ptr()
            o.dot_scratch = self.prob.dot_scratch.data_ptr()
            o.dot_scratch_bytes = self.prob.dot_scratch.numel() * 8
        o.cg_ctl = None if ctl is None else ctl.data_ptr()
        if self.R is not None:
            o.rest_basis, o.rest_views, o.view_base = self.R.data_ptr(), self.rv, view_base
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
        idx = list(range(self.V)) if idx is None else list(idx)
        vs, ys = self.layout.grads_struct(v), self.layout.grads_struct(y)
        o = self.opts(overwrite, damp, dot, ctl, view_base=idx[0])
        _lib.check(lib.gslm_gather_views(self._views(idx), self.ws(idx), len(idx), ctypes.byref(self.g),
                                         ctypes.byref(vs), ctypes.byref(ys), ctypes.byref(o), self.st),
                   "gslm_gather_views")
        return y

    def gather_screen(self, v, y, idx=None, overwrite=True, damp=True, dot=None):
        idx = list(range(self.V)) if idx is None else list(idx)
        vs, ys = self.layout.grads_struct(v), self.layout.grads_struct(y)
        o = self.opts(overwrite, damp, dot, None, view_base=idx[0])
        table = self.screen[idx].contiguous()
        _lib.check(lib.gslm_gather_screen(self._views(idx), len(idx), ctypes.byref(self.g), table.data_ptr(),
                                          ctypes.byref(vs), ctypes.byref(ys), ctypes.byref(o), self.st),
                   "gslm_gather_screen")
        return y


def _prefill(layout, seed=5):
    return torch.randn(layout.numel, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


CASES = [(P, V, mode) for P in (255, 256, 257, 6001) for V in (1, 2, 5, 16)
         for mode in ("sh3_full", "sh3_coords", "sh0") if not (mode == "sh3_coords" and V > 8)]


@pytest.mark.parametrize("P,V,mode", CASES)
def test_gather_views_matches_rowsum_and_gather_screen(P, V, mode):
    rig = Rig(P, V, 0 if mode == "sh0" else 3, coords=(mode == "sh3_coords"))
    # the scene's conditions, from the library's own tile counts
    none, some, every = ms.visibility_classes(rig.tiles())
    assert none >= 1, "no Gaussian is invisible in every view"
    assert every >= 1, "no Gaussian is visible in every view"
    assert V < 2 or some >= 1, "no Gaussian is visible in some views only"
    v = rig.direction()
    rig.render(v)
    zeros = lambda: torch.zeros(rig.layout.numel, dtype=torch.float32, device=DEV)
    # OVERWRITE with damping and the fused dot
    dot = torch.full((1,), math.nan, dtype=torch.float64, device=DEV)
    y_ref = rig.gather_screen(v, zeros())
    y = rig.gather_views(v, _prefill(rig.layout), dot=dot)  # OVERWRITE: the prefill must not show
    e0, e1 = rig.layout.offsets["exposure"]
    y[e0:e1] = 0  # (the exposure slice belongs to the caller: neither gather writes it)
    err = _rel(y, y_ref)
    print(f"P {P} V {V} {mode}: overwrite+damp |diff| / max {err:.2e} bitwise {torch.equal(y, y_ref)}")
    assert torch.isfinite(y).all()
    assert err <= 1e-6
    host = float((v.double() * y.double()).sum())
    scale = float((v.double() * y.double()).abs().sum())
    print(f"  <v, y> device {float(dot)!r} host {host!r} |diff| / sum|v y| {abs(float(dot) - host) / scale:.2e}")
    assert abs(float(dot) - host) <= 1e-12 * scale
    # accumulate, no damping
    y0 = _prefill(rig.layout, seed=6)
    ya_ref = rig.gather_screen(v, y0.clone(), overwrite=False, damp=False)
    ya = rig.gather_views(v, y0.clone(), overwrite=False, damp=False)
    erra = _rel(ya, ya_ref)
    print(f"  accumulate |diff| / max {erra:.2e} bitwise {torch.equal(ya, ya_ref)}")
    assert erra <= 1e-6
    assert torch.equal(ya[e0:e1], y0[e0:e1])
    # the two modes against each other: (accumulate onto zero, no damping) + D v = overwrite with damping
    yz = rig.gather_views(v, zeros(), overwrite=False, damp=False)
    for k, name in enumerate(("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity")):
        a, b = rig.layout.offsets[name]
        yz[a:b] += float(rig.damps[k]) * v[a:b]
    assert _rel(yz, y) <= 1e-6
    # reproducible: no atomics, a fixed order of every sum
    y2 = rig.gather_views(v, _prefill(rig.layout, seed=7))
    y2[e0:e1] = 0
    assert torch.equal(y, y2)


@pytest.mark.parametrize("P", [257, 6001])
def test_two_eight_view_calls_equal_one_sixteen_view_call(P):
    rig = Rig(P, 16, 3, coords=False)
    v = rig.direction()
    rig.render(v)
    y16 = rig.gather_views(v, _prefill(rig.layout))
    y8 = rig.gather_views(v, _prefill(rig.layout, seed=8), idx=range(0, 8))
    rig.gather_views(v, y8, idx=range(8, 16), overwrite=False, damp=False)
    e0, e1 = rig.layout.offsets["exposure"]
    y16[e0:e1] = 0
    y8[e0:e1] = 0
    err = _rel(y8, y16)
    print(f"P {P}: 8 + 8 views against 16 |diff| / max {err:.2e} bitwise {torch.equal(y8, y16)}")
    assert err <= 1e-6
    # and the dot of the second call is the dot of the whole y
    dot = torch.zeros(1, dtype=torch.float64, device=DEV)
    y8b = rig.gather_views(v, _prefill(rig.layout, seed=8), idx=range(0, 8))
    rig.gather_views(v, y8b, idx=range(8, 16), overwrite=False, damp=False, dot=dot)
    y8b[e0:e1] = 0
    scale = float((v.double() * y8b.double()).abs().sum())
    assert abs(float(dot) - float((v.double() * y8b.double()).sum())) <= 1e-12 * scale


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


def test_view_that_rendered_nothing_is_skipped_and_not_read():
    rig = Rig(257, 3, 3, coords=False, empty_at=1)
    assert [vr.N > 0 for vr in rig.prob.views] == [True, False, True, True]
    assert int(rig.tiles()[1].sum()) == 0
    v = rig.direction()
    rig.render(v)
    sc = rig.prob.views[1].scratch
    sc[:sc.numel() // 4 * 4].view(torch.float32).fill_(math.nan)  # nothing of it may be read
    y_all = rig.gather_views(v, _prefill(rig.layout))
    y_wo = rig.gather_views(v, _prefill(rig.layout, seed=9), idx=[0, 2, 3])
    e0, e1 = rig.layout.offsets["exposure"]
    y_all[e0:e1] = 0
    y_wo[e0:e1] = 0
    assert torch.isfinite(y_all).all()
    assert torch.equal(y_all, y_wo)
    y_ref = rig.gather_screen(v, torch.zeros_like(y_all), idx=[0, 2, 3])
    assert _rel(y_all, y_ref) <= 1e-6
    # an all-empty call still writes D v
    y_e = rig.gather_views(v, _prefill(rig.layout), idx=[1])
    for k, name in enumerate(("features_dc", "features_rest", "scaling", "rotation", "opacity"), start=1):
        a, b = rig.layout.offsets[name]
        assert torch.equal(y_e[a:b], float(rig.damps[k]) * v[a:b])


def test_error_returns_write_nothing():
    rig = Rig(257, 2, 3, coords=True)
    v = rig.direction()
    rig.render(v)
    y0 = _prefill(rig.layout)
    y = y0.clone()
    vs, ys = rig.layout.grads_struct(v), rig.layout.grads_struct(y)
    views17 = (_lib.GslmView * 17)(*([rig.views[0]] * 17))
    ws17 = (_lib.GslmViewWs * 17)()
    for k in range(17):
        ws17[k] = rig.ws([0])[0]

    def call(views, ws, n, o):
        return lib.gslm_gather_views(views, ws, n, ctypes.byref(rig.g), ctypes.byref(vs), ctypes.byref(ys),
                                     ctypes.byref(o), rig.st)

    full = ParamLayout(rig.P, rig.K, rig.prob.full_layout.n_exposure)
    plain = _lib.GslmMatvecOpts()
    plain.stages = ALL | OVERWRITE
    for n in (0, 17):
        assert call(views17, ws17, n, rig.opts(True, True, None, None)) == _lib.GSLM_ERR_INVALID
        assert b"nviews" in lib.gslm_last_error()
    short = rig.ws([0, 1])
    short[1].scratch_bytes = lib.gslm_scratch_bytes(rig.P, rig.prob.views[1].N) - 1
    assert call(rig._views([0, 1]), short, 2, rig.opts(True, True, None, None)) == _lib.GSLM_ERR_CAPACITY
    o9 = rig.opts(True, True, None, None)
    o9.rest_views = 9
    assert call(rig._views([0, 1]), rig.ws([0, 1]), 2, o9) == _lib.GSLM_ERR_INVALID
    # a dot scratch that is too small, and group strides of another layout (the full one against these coordinates)
    od = rig.opts(True, True, torch.zeros(1, dtype=torch.float64, device=DEV), None)
    od.dot_scratch_bytes = lib.gslm_dot_scratch_bytes(rig.P) - 1
    assert call(rig._views([0, 1]), rig.ws([0, 1]), 2, od) == _lib.GSLM_ERR_CAPACITY
    yf = torch.zeros(full.numel, dtype=torch.float32, device=DEV)
    yfs = full.grads_struct(yf)
    assert lib.gslm_gather_views(rig._views([0, 1]), rig.ws([0, 1]), 2, ctypes.byref(rig.g), ctypes.byref(vs),
                                 ctypes.byref(yfs), ctypes.byref(rig.opts(True, True, None, None)),
                                 rig.st) == _lib.GSLM_ERR_INVALID
    assert lib.gslm_gather_views(None, rig.ws([0, 1]), 2, ctypes.byref(rig.g), ctypes.byref(vs), ctypes.byref(ys),
                                 ctypes.byref(plain), rig.st) == _lib.GSLM_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and not yf.any()
    # and the same arguments, valid, do write
    assert call(rig._views([0, 1]), rig.ws([0, 1]), 2, rig.opts(True, True, None, None)) == _lib.GSLM_OK
    assert not torch.equal(y, y0)
