"""A refused product call launches nothing.

Every GSLM_ERR_INVALID / GSLM_ERR_CAPACITY return of gslm_matvec_view_ex, gslm_matvec_view_active, gslm_gather_screen,
gslm_gather_views and gslm_tangent_views comes from the call's plan, which is built before the first launch
(include/gslm.h at gslm_matvec_opts).  Each case below arms what an early launch would move -- the fused direction
update p = s + (3/4) p with the deferred x += (3/2) p, on small integers -- hands the call NaN-filled outputs, and
asserts the code, a non-empty gslm_last_error() and, after a synchronize, the bits of p, x, y, jv_out, screen_out and
of the whole scratch workspace.  Cases 1 to 4 are the refusals that used to come after the tangent kernel (and the
tile pass); case 5 pairs one refusal that was always early with the accepted form of the same call, which returns 0,
moves p and writes y -- so the harness does see a launch.

Scenes: sh1_33x17 of test_gpu_lm_exposure.py (two tile columns, a ragged right edge, SH degree 1) for
gslm_matvec_view_ex, short_list_sh3 of test_gpu_cg_lean_direct.py for gslm_matvec_view_active, and the two-view rig
of test_gpu_gather_views.py's own error test for the multi-view calls."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_vector_algebra import _ints, _lib, _scalars, _slot

pytestmark = pytest.mark.gpu
DEV = "cuda"
TANGENT, RENDER, GATHER, ALL, OVERWRITE, SCREEN = 1, 2, 4, 7, 8, 16


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.uint8 else t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def _int_vec(n, seed):
    return torch.from_numpy(_ints(np.random.default_rng(seed), n)).to(DEV)


def _scene(entry):
    """(problem or active view, weight image, None or (ids, rows, na)) of an entry point's scene."""
    if entry == "ex":
        from test_gpu_lm_exposure import _tiles
        t = _tiles()["sh1_33x17"]
        assert t.vr.W > 16 and t.lay.K == 4  # more than one tile, an SH-rest group
        return t.prob, t.w, None
    from test_gpu_cg_lean_direct import _act
    prob, model, P, act = _act("short_list_sh3")
    assert prob.views[0].tail_clean and act.layout.K > 1
    ids, na = act._active
    return act, act.weights[0], (ids, act.views[0].active_rows, na)


class Call:
    """One call of gslm_matvec_view_ex / _active: integer s, p, x, NaN outputs, and the options a case edits."""

    def __init__(self, entry, xpby=True):
        L = _lib()
        self.pr, self.weight, self.active = _scene(entry)
        pr = self.pr
        self.vr, self.lay = pr.views[0], pr.layout
        n = self.lay.numel
        self.s, self.p, self.x = (_int_vec(n, 80 + k) for k in range(3))
        self.y = torch.full((n,), math.nan, device=DEV)
        self.jv = torch.full_like(self.vr.color, math.nan)
        self.screen = torch.full((self.lay.P, 8), math.nan, device=DEV)
        self.sc = _scalars(3.0, 4.0, 3.0, 2.0)
        self.dot = _scalars(-1.0)
        self.mask_xyz = 1
        self.vs, self.ys = self.lay.grads_struct(self.p), self.lay.grads_struct(self.y)
        o = self.o = L.GslmMatvecOpts()
        o.stages = ALL | OVERWRITE
        o.flags = pr.mv_flags | (1 if self.vr.tail_clean else 0)  # (GSLM_MV_TAIL_CLEAN: the active list needs it)
        self.ss = None
        if xpby:  # the fused direction update and the deferred x update, both armed
            sc = self.sc
            self.ss = pr._pre_opts(o, self.p, (self.s, _slot(sc, 0), _slot(sc, 1), self.x, _slot(sc, 2), _slot(sc, 3)))

    def with_dot(self):
        o, ds = self.o, self.pr.dot_scratch
        o.dot_vy, o.dot_scratch, o.dot_scratch_bytes = self.dot.data_ptr(), ds.data_ptr(), ds.numel() * 8

    def drop_group(self, name):
        """One group of v and of s NULL (a legal direction: the group is not moved)."""
        setattr(self.vs, name, None)
        setattr(self.ss, name, None)

    def watched(self):
        return dict(p=self.p, x=self.x, y=self.y, jv_out=self.jv, screen_out=self.screen, scratch=self.vr.scratch,
                    dot=self.dot)

    def run(self):
        from gslm.params import raw_gaussians
        L = _lib()
        vr = self.vr
        g = raw_gaussians(self.pr.model)
        args = (ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(self.vs), self.weight.data_ptr(), self.mask_xyz,
                vr.geom.data_ptr(), vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(),
                vr.scratch.numel(), ctypes.byref(self.ys), ctypes.byref(self.o))
        if self.active is not None:
            ids, rows, na = self.active
            st = L.lib.gslm_matvec_view_active(*args, ids.data_ptr(), rows.data_ptr(), na, self.pr.stream)
        else:
            st = L.lib.gslm_matvec_view_ex(*args, self.pr.stream)
        torch.cuda.synchronize()
        if st == 0 and (self.o.stages & RENDER):
            vr.tail_clean = True
        return st


def _assert_refused(what, watched, run, want):
    """run() returns `want`, leaves an error message, and every watched tensor keeps its bits."""
    L = _lib()
    before = {k: _bits(t).clone() for k, t in watched.items()}
    st = run()
    torch.cuda.synchronize()
    assert st == want, (what, st)
    assert L.lib.gslm_last_error(), what
    for k, t in watched.items():
        assert torch.equal(_bits(t), before[k]), (what, k)


def _refused(what, c, want=None):
    _assert_refused(what, c.watched(), c.run, _lib().GSLM_ERR_INVALID if want is None else want)


def _assert_accepted(c):
    p0, x0 = c.p.clone(), c.x.clone()
    assert c.run() == 0
    a, b = c.lay.offsets["xyz"]
    moved = torch.ones_like(p0, dtype=torch.bool)
    moved[a:b] = False  # (mask_xyz: the xyz group of p and x is left alone)
    e0 = c.lay.offsets["exposure"][0]
    assert torch.equal(c.p[moved], (c.s.double() + 0.75 * p0.double()).float()[moved])
    assert torch.equal(c.x[moved], (x0.double() + 1.5 * p0.double()).float()[moved])
    assert bool(torch.isfinite(c.y[:e0]).all()) and bool((c.y[:e0] != 0).any())


# ------------------------------------------------------------------------ 1..4: refusals that used to follow a launch
def test_jv_out_with_default_stages():
    """1. stages = 0 is GSLM_STAGE_ALL: jv_out with GATHER."""
    c = Call("ex")
    c.o.stages = 0
    c.o.jv_out = c.jv.data_ptr()
    _refused("jv_out, stages 0", c)


@pytest.mark.parametrize("form", ["no_screen_out_xpby", "no_screen_out", "mask_xyz_0"])
def test_screen_stage_without_its_arguments(form):
    """2. TANGENT | RENDER | SCREEN without screen_out, or without mask_xyz."""
    c = Call("ex", xpby=(form == "no_screen_out_xpby"))
    c.o.stages = TANGENT | RENDER | SCREEN
    if form == "mask_xyz_0":
        c.o.screen_out = c.screen.data_ptr()
        c.mask_xyz = 0
    _refused(form, c)


@pytest.mark.parametrize("entry", ["ex", "active"])
def test_output_of_another_layout(entry):
    """3. y.sh_rest_stride one more than the layout's."""
    c = Call(entry)
    c.ys.sh_rest_stride += 1
    _refused(entry, c)


@pytest.mark.parametrize("needs", ["damp7", "dot_vy"])
def test_damping_or_dot_with_a_null_group(needs):
    """4. damp7, or the fused dot, with one group of v (and of s) NULL."""
    c = Call("ex")
    if needs == "damp7":
        c.o.damp7 = c.pr._damps
    else:
        c.with_dot()
    c.drop_group("scales")
    _refused(needs, c)


# ------------------------------------------------------------- 5: an early refusal and the accepted form, per entry point
def test_matvec_view_ex_refusal_and_accepted_form():
    c = Call("ex")
    c.o.rest_basis = c.jv.data_ptr()
    _refused("rest_basis on gslm_matvec_view_ex", c)
    _assert_accepted(Call("ex"))


def test_matvec_view_active_refusal_and_accepted_form():
    c = Call("active")
    c.mask_xyz = 0
    _refused("gslm_matvec_view_active without mask_xyz", c)
    _assert_accepted(Call("active"))


def _rig():
    from test_gpu_gather_views import Rig
    rig = Rig(257, 2, 3, coords=True)
    v = rig.direction()
    rig.render(v)
    return rig, v


def _rig_scratches(rig):
    return {f"scratch{b}": vr.scratch for b, vr in enumerate(rig.prob.views)}


@pytest.mark.parametrize("entry", ["gather_views", "gather_screen"])
def test_multi_view_gather_refusal_and_accepted_form(entry):
    """gslm_gather_views with 17 views (test_gpu_gather_views.py), gslm_gather_screen with GSLM_MV_DAMP_VEC
    (test_oracle_lm_marquardt.py)."""
    L = _lib()
    rig, v = _rig()
    y = torch.full((rig.layout.numel,), math.nan, device=DEV)
    dot = _scalars(-1.0)
    vs, ys = rig.layout.grads_struct(v), rig.layout.grads_struct(y)
    views17 = (L.GslmView * 17)(*([rig.views[0]] * 17))
    ws17 = (L.GslmViewWs * 17)(*([rig.ws([0])[0]] * 17))
    table = rig.screen.contiguous()

    def call(n, o):
        views, ws = (views17, ws17) if n == 17 else (rig._views([0, 1]), rig.ws([0, 1]))
        if entry == "gather_views":
            return L.lib.gslm_gather_views(views, ws, n, ctypes.byref(rig.g), ctypes.byref(vs), ctypes.byref(ys),
                                           ctypes.byref(o), rig.st)
        return L.lib.gslm_gather_screen(views, n, ctypes.byref(rig.g), table.data_ptr(), ctypes.byref(vs),
                                        ctypes.byref(ys), ctypes.byref(o), rig.st)

    good = rig.opts(True, True, dot, None)
    bad = rig.opts(True, True, dot, None)
    n_bad = 2
    if entry == "gather_views":
        n_bad = 17
    else:
        bad.flags = 16
    watched = dict(v=v, y=y, dot=dot, **_rig_scratches(rig))
    _assert_refused(entry, watched, lambda: call(n_bad, bad), L.GSLM_ERR_INVALID)
    assert (b"nviews" if entry == "gather_views" else b"GSLM_MV_DAMP_VEC") in L.lib.gslm_last_error()
    assert call(2, good) == 0
    torch.cuda.synchronize()
    e0 = rig.layout.offsets["exposure"][0]
    assert bool(torch.isfinite(y[:e0]).all()) and bool((y[:e0] != 0).any()) and math.isfinite(dot.item())
    assert dot.item() != -1.0


def test_tangent_views_refusal_and_accepted_form():
    """gslm_tangent_views with 17 views (test_cabi.py), the fused direction update armed."""
    L = _lib()
    rig, _ = _rig()
    lay = rig.layout
    s, p, x = (_int_vec(lay.numel, 90 + k) for k in range(3))
    p0, x0 = p.clone(), x.clone()
    trec = torch.full((rig.V, rig.P, 8), math.nan, device=DEV)
    sc = _scalars(3.0, 4.0, 3.0, 2.0)
    vs, ss = lay.grads_struct(p), lay.grads_struct(s)
    o = L.GslmMatvecOpts()
    o.rest_basis, o.rest_views, o.view_base = rig.R.data_ptr(), rig.rv, 0
    o.xpby_s = ctypes.addressof(ss)
    o.beta_num, o.beta_den, o.alpha_num, o.alpha_den = (_slot(sc, k) for k in range(4))
    o.xpby_x_offset = x.data_ptr() - p.data_ptr()
    views17 = (L.GslmView * 17)(*([rig.views[0]] * 17))

    def call(n):
        views = views17 if n == 17 else rig._views(range(rig.V))
        return L.lib.gslm_tangent_views(views, n, ctypes.byref(rig.g), ctypes.byref(vs), 1, rig.flags.data_ptr(), rig.P,
                                        trec.data_ptr(), rig.P, ctypes.byref(o), rig.st)

    _assert_refused("17 views", dict(p=p, x=x, trec=trec), lambda: call(17), L.GSLM_ERR_INVALID)
    assert b"nviews" in L.lib.gslm_last_error()
    assert call(rig.V) == 0
    torch.cuda.synchronize()
    a, b = lay.offsets["xyz"]
    e0 = lay.offsets["exposure"][0]
    moved = torch.zeros_like(p0, dtype=torch.bool)
    moved[b:e0] = True  # (mask_xyz: the xyz group is left alone; the flat tail is not this call's)
    assert a == 0
    assert torch.equal(p[moved], (s.double() + 0.75 * p0.double()).float()[moved])
    assert torch.equal(x[moved], (x0.double() + 1.5 * p0.double()).float()[moved])
    seen = rig.flags < 0  # (bit 31: the Gaussian touches a tile of the view)
    assert bool(seen.any()) and bool(torch.isfinite(trec[seen]).all())
