"""The batched multi-view LM solve on the union of the views' active lists (BatchedLMProblem(union_active=True),
gslm_active_union / gslm_tangent_views_active / gslm_gather_views_active).

Scenes: the recipe of tests/multiview_scene.py at 96 x 72 -- a Gaussian no view sees (off the union list U by
construction), one every view sees and one only some see -- and sparse translucent scenes whose list has exactly 255,
256 or 257 entries.  Every scene asserts 0 < Pa < P and, from two views on, a listed Gaussian with an empty row range
in some view: without them the tests below would prove nothing.

Bounds.  The product on the list against the full product restricted to it: `==` (same per-element arithmetic, row-sum
order and view order).  <v, y>: 1e-12 of sum |v_i y_i|, the project's bound for this dot (another grouping of the same
float64 products).  Three CG iterations on the list against the same solve on the full vectors: 1e-4 in norm, the
bound tests/test_gpu_batched_lm.py uses for this solve against the per-view loop; the measured value and whether the
two were bitwise equal are printed."""
import copy
import ctypes
import functools
import math
import os

import pytest
import torch

from gslm import _lib
from gslm._lib import lib
import multiview_scene as ms

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENT = 64, 12345.0


class Rig:
    """One geometry: a BatchedLMProblem with union_active=True after evaluate() and rhs() (every view's row map
    exists), its active view and the union list."""

    def __init__(self, model, cams, full_env=False):
        from gslm.lm import BatchedLMProblem
        self.model = copy.deepcopy(model).to(DEV)
        self.cams = [copy.deepcopy(c).to(DEV) for c in cams]
        old = os.environ.get("GSLM_SHARD_REST")
        if full_env:  # (read by the constructor only; the rigs are cached, so no monkeypatch here)
            os.environ["GSLM_SHARD_REST"] = "full"
        try:
            self.U = BatchedLMProblem(self.model, self.cams, torch.zeros(3), union_active=True)
        finally:
            if full_env and old is None:
                del os.environ["GSLM_SHARD_REST"]
            elif full_env:
                os.environ["GSLM_SHARD_REST"] = old
        self.P, self.V = self.U.full_layout.P, len(self.cams)
        self.U.evaluate()
        self.g = self.U.rhs(self.U.zeros())
        self.act = self.U.active_view()
        assert self.act is not None
        self.ids, self.Pa = self.act._active
        self.hrow, self.aflags = self.act._union_bufs
        torch.cuda.synchronize()
        # the scene's conditions
        assert 0 < self.Pa < self.P, (self.Pa, self.P)
        h = self.hrow[:, :self.Pa + 1].long()
        self.empty_ranges = int(((h[:, 1:] == h[:, :-1]) & (torch.tensor([vr.N > 0 for vr in self.U.views],
                                                                           device=DEV)[:, None])).sum())
        assert self.V < 2 or self.empty_ranges > 0, "no listed Gaussian has an empty row range in some view"

    def off_list(self):
        off = torch.ones(self.P, dtype=torch.bool, device=DEV)
        off[self.ids.long()] = False
        return off

    def random_v(self, seed):
        """A vector of the problem's layout with xyz and exposure zero, as every LM iterate."""
        lay = self.U.layout
        v = torch.randn(lay.numel, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        for grp in ("xyz", "exposure"):
            a, b = lay.offsets[grp]
            v[a:b] = 0
        return v

    def restrict(self, v):
        """v with the rows off the list zeroed (a vector of the solve's invariant subspace)."""
        v = v.clone()
        off = self.off_list()
        for name, t in self.U.layout.views(v).items():
            if name != "exposure" and t.numel():
                t.view(self.P, -1)[off] = 0
        return v


@functools.lru_cache(maxsize=None)
def rig(P, V, D, full_env=False, empty_at=None):
    model, cams = ms.scene(P, V, D)
    cams = [copy.deepcopy(c) for c in cams]
    if empty_at is not None:
        cams.insert(empty_at, ms.empty_camera())
    return Rig(model, cams, full_env=full_env)


def _sparse_model(P, D, cams):
    """Translucent small Gaussians in the cameras' common field of view: no pixel saturates, so every blended entry
    is a head entry and moving a Gaussian out of every frustum changes nobody else's rows."""
    from gslm.model import inverse_sigmoid, synthetic_gaussians
    gen = torch.Generator().manual_seed(107)
    m = synthetic_gaussians(P, D, seed=3, s0=0.01, n_cams=len(cams))
    m._xyz.data[:] = torch.rand(P, 3, generator=gen) - 0.5
    m._opacity.data[:] = inverse_sigmoid(0.05 + 0.1 * torch.rand(P, 1, generator=gen))
    return m


FAR = lambda n: torch.tensor([0.0, 0.0, 1000.0]) + torch.arange(float(n))[:, None] * torch.tensor([0.0, 0.0, 1.0])


@functools.lru_cache(maxsize=None)
def boundary_rig(k, ends_active):
    """Two views, a list of exactly k entries.  Gaussian 1 sits at the origin (in both views), 2 far above the scene
    (in none), 3 where multiview_scene found a position only some views see; ends_active: Gaussians 0 and P - 1 are
    on the list (near the origin) or off it (far above the scene)."""
    P, D, V = 600, 3, 2
    ref_model, cams = ms.scene(P, V, D)
    m = _sparse_model(P, D, cams)
    m._xyz.data[1] = torch.tensor([0.0, 0.0, 0.0])
    m._xyz.data[2] = torch.tensor([0.0, 0.0, 900.0])
    m._xyz.data[3] = ref_model._xyz.data[P - 3]
    ends = torch.tensor([0, P - 1])
    m._xyz.data[ends] = torch.tensor([[0.02, 0.0, 0.0], [0.05, 0.05, 0.05]]) if ends_active else FAR(2)
    first = Rig(m, cams)
    keep = {1, 3} | ({0, P - 1} if ends_active else set())
    ids = first.ids.cpu().tolist()
    assert keep <= set(ids), (keep, "not all on the list")
    others = [i for i in ids if i not in keep]
    assert len(others) > k - len(keep), first.Pa
    drop = torch.tensor(others[k - len(keep):])
    m._xyz.data[drop] = FAR(len(drop)) + torch.tensor([0.0, 0.0, 10.0])
    return Rig(m, cams)


# ------------------------------------------------------------------------------------------------ 1. the list
LIST_RIGS = {"V1": (257, 1, 3), "V2": (6001, 2, 3), "V5": (6001, 5, 3), "V17_empty": (257, 16, 3, False, 8)}


@pytest.mark.parametrize("name", list(LIST_RIGS))
def test_union_list_is_the_union_of_the_views_lists(name):
    r = rig(*LIST_RIGS[name])
    U, P, Pa = r.U, r.P, r.Pa
    if name == "V17_empty":
        assert r.V == 17 and [vr.N > 0 for vr in U.views] == [True] * 8 + [False] + [True] * 8
    ids = r.ids.cpu().long()
    hrow, afl = r.hrow.cpu().long(), r.aflags.cpu()
    assert (ids[1:] > ids[:-1]).all()
    union = set()
    for b, vr in enumerate(U.views):
        h = hrow[b, :Pa + 1]
        if vr.N == 0:  # a camera looking away: all zeros, no workspace read
            assert not h.any() and not afl[b, :Pa].any()
            continue
        idb, nb = vr.active_list(P, U.stream)
        idb, rows = idb.cpu().long(), vr.active_rows.cpu().long()
        union |= set(idb.tolist())
        pos = torch.searchsorted(ids, idb)
        assert torch.equal(ids[pos], idb)  # every entry of the view's list is on the union list
        assert torch.equal(h[pos], rows[:-1]) and int(h[Pa]) == int(rows[-1])
        want = torch.zeros(Pa, dtype=torch.long)
        want[pos] = rows[1:] - rows[:-1]
        assert torch.equal(h[1:] - h[:-1], want)  # the view's own ranges, and empty ones everywhere else
        assert torch.equal(afl[b, :Pa], U._flags[b].cpu()[ids])
    assert ids.tolist() == sorted(union)
    print(f"{name}: P {P} Pa {Pa}, {r.empty_ranges} empty (entry, view) ranges")


# ------------------------------------------------------------------------------------------------ 2. the product
def _guarded(t):
    buf = torch.full((t.numel() + 2 * GUARD,), SENT, dtype=t.dtype, device=t.device)
    buf[GUARD:GUARD + t.numel()] = t
    return buf, buf[GUARD:GUARD + t.numel()]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all() and (buf[-GUARD:] == SENT).all())


def _product(prob, v, pre=None, damp=True, y0=None):
    """(y, <v, y>, v after the fused update, x after it, the guarded buffers) of one product with the dot fused.
    y0 None: y is NaN-filled (an overwriting product must not let it show); else the product accumulates onto it."""
    n = v.numel()
    x = None
    if pre is not None:  # x lives at a fixed offset from v: one buffer holds both
        s_, num, den, x0, anum, aden = pre
        vbuf, vx = _guarded(torch.cat([v, x0]))
        v, x = vx[:n], vx[n:]
        pre = (s_, num, den, x, anum, aden)
    else:
        vbuf, v = _guarded(v)
    ybuf, y = _guarded(torch.full_like(v, math.nan) if y0 is None else y0)
    e0, e1 = prob.layout.offsets["exposure"]
    y[e0:e1] = 0  # (exposure_zero: the slice belongs to the caller)
    dot = torch.full((1,), math.nan, dtype=torch.float64, device=DEV)
    prob.local_normal_matvec(v, y, damp=damp, dot_out=dot.data_ptr(), pre=pre, exposure_zero=True)
    torch.cuda.synchronize()
    assert _guards_intact(vbuf) and _guards_intact(ybuf), "a write landed outside the vectors"
    return y, float(dot), v, x


PRODUCT_RIGS = {
    "sh3_coords_V2": lambda: rig(6001, 2, 3),
    "sh3_coords_V5": lambda: rig(6001, 5, 3),
    "sh3_full_V9": lambda: rig(2000, 9, 3),
    "sh3_full_env_V2": lambda: rig(6001, 2, 3, True),
    "sh0_V2": lambda: rig(6001, 2, 0),
    "sh3_V16_one_chunk": lambda: rig(257, 16, 3),
    "sh3_V17_two_chunks": lambda: rig(257, 16, 3, False, 8),
    "k255_ends_on": lambda: boundary_rig(255, True), "k255_ends_off": lambda: boundary_rig(255, False),
    "k256_ends_on": lambda: boundary_rig(256, True), "k256_ends_off": lambda: boundary_rig(256, False),
    "k257_ends_on": lambda: boundary_rig(257, True), "k257_ends_off": lambda: boundary_rig(257, False),
}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(PRODUCT_RIGS))
def test_active_product_is_the_full_product_restricted(name, fused, monkeypatch):
    from gslm import lm
    r = PRODUCT_RIGS[name]()
    U, act = r.U, r.act
    lay = U.layout
    if name.startswith("k"):
        k = int(name[1:4])
        ids = r.ids.cpu().tolist()
        assert r.Pa == k
        on = name.endswith("ends_on")
        assert ((0 in ids) and (r.P - 1 in ids)) if on else ((0 not in ids) and (r.P - 1 not in ids))
    assert (lay.rest_views > 0) == ("coords" in name or name.startswith("k"))
    if "full" in name or "V1" in name:
        assert lay.rest_rows == 15 and act._pack_args()[0][2] == 45
    assert act.layout.P == r.Pa and act.layout.rest_views == lay.rest_views
    sc = torch.tensor([3.0, 7.0, 2.0, 5.0], dtype=torch.float64, device=DEV)  # beta = 3/7, alpha = 2/5
    ptr = lambda i: sc.data_ptr() + 8 * i
    off = r.off_list()
    for mode in ("overwrite_damp", "overwrite", "accumulate_damp", "accumulate"):
        damp = mode.endswith("damp")
        seed = 11 + len(mode)
        v = r.restrict(r.random_v(seed))
        pre_f = pre_a = None
        if fused:
            sv, xv = r.restrict(r.random_v(seed + 100)), r.restrict(r.random_v(seed + 200))
            pre_f = (sv, ptr(0), ptr(1), xv, ptr(2), ptr(3))
            pre_a = (act.pack(sv), ptr(0), ptr(1), act.pack(xv), ptr(2), ptr(3))
        y0f = y0a = None
        with monkeypatch.context() as mp:
            if mode.startswith("accumulate"):
                mp.setattr(lm, "STAGE_OVERWRITE", 0)  # every chunk's gather accumulates onto y
                y0f = r.random_v(seed + 300)
                y0a = act.pack(y0f)
            yf, df, vf, xf = _product(U, v, pre_f, damp=damp, y0=y0f)
            # the records of Gaussians off the list are never read: poison them before the product on the list
            U._trec[:, off] = math.nan
            ya, da, va, xa = _product(act, act.pack(v), pre_a, damp=damp, y0=y0a)
        assert torch.isfinite(ya).all()
        assert torch.equal(act.pack(yf), ya), (name, mode)
        if y0f is None:
            assert torch.equal(act.unpack(ya), r.restrict(yf))
        if fused:
            assert torch.equal(act.pack(vf), va) and torch.equal(act.pack(xf), xa)
        scale = float((vf.double() * yf.double()).abs().sum())
        print(f"{name} fused={fused} {mode}: Pa {r.Pa} of {r.P}; <v, y> full {df!r} active {da!r} "
              f"|diff| / sum|v y| {abs(df - da) / max(scale, 1e-300):.2e}")
        assert abs(df - da) <= 1e-12 * scale


# ------------------------------------------------------------------------------------------------ 3. rhs off the list
@pytest.mark.parametrize("name", ["sh3_coords_V5", "sh3_full_V9", "sh0_V2", "sh3_V17_two_chunks", "k256_ends_off"])
def test_rhs_is_zero_off_the_union_list(name):
    r = PRODUCT_RIGS[name]()
    g = r.U.rhs(r.U.zeros())
    off = r.off_list()
    assert int(off.sum()) == r.P - r.Pa > 0
    for grp, t in r.U.layout.views(g).items():
        if grp != "exposure" and t.numel():
            assert not bool((t.reshape(r.P, -1)[off] != 0).any()), grp  # +-0.0f only
    assert r.act.zero_off_active(g)  # ... so it is known without a read-back


# ------------------------------------------------------------------------------------------------ 4. the solve
@pytest.mark.parametrize("check_every", [False, True])
@pytest.mark.parametrize("name", ["sh3_coords_V2", "sh3_coords_V5", "sh3_full_V9", "k257_ends_on"])
def test_solve_on_the_union_list_matches_the_full_solve(name, check_every, monkeypatch):
    from gslm import lm
    r = PRODUCT_RIGS[name]()
    U = r.U
    F = lm.BatchedLMProblem(r.model, r.cams, torch.zeros(3))
    assert F.rest_views == U.rest_views
    F.evaluate()
    gf = F.rhs(F.zeros())
    assert lm._active_view_for(F, gf, None) is None
    xf, inf_f = lm.cgls_fused(F, gf, max_iter=3, restart_iter=3, check_every=check_every)
    gu = U.rhs(U.zeros())
    assert torch.equal(gu, gf)
    act = lm._active_view_for(U, gu, None)
    assert act is not None and act.layout.P == r.Pa
    assert not lm._lean_applies(act, check_every, 3)

    def no_lean(*a, **k):
        raise AssertionError("the lean loop is the single view's")

    monkeypatch.setattr(lm, "_cgls_lean", no_lean)
    xu, inf_u = lm.cgls_fused(U, gu, max_iter=3, restart_iter=3, check_every=check_every)
    assert inf_u["iters"] == inf_f["iters"] and inf_u.get("stop") == inf_f.get("stop")
    err = float((xu - xf).norm() / xf.norm())
    print(f"{name} check_every {check_every}: Pa {r.Pa} of {r.P}, iters {inf_u['iters']}, "
          f"|x - x_full| / |x_full| {err:.2e}, bitwise {torch.equal(xu, xf)}")
    assert err <= 1e-4
    off = r.off_list()
    for grp, t in U.layout.views(xu).items():
        if grp != "exposure" and t.numel():
            bits = t.reshape(r.P, -1)[off].contiguous().view(torch.int32)
            assert not bool(bits.any()), grp  # exactly +0.0f off U


def _close(a, b, tol):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-12)


def test_lm_step_union_active_matches_batched():
    """3 training and 4 validation views, at the tolerances of test_gpu_batched_lm.py::test_lm_step_batched_matches_loop."""
    from gslm.cameras import orbit_cameras
    from gslm.lm import clear_val_cache, lm_step
    from gslm.model import synthetic_gaussians
    W, H, nv, P = 96, 72, 7, 4000
    m = synthetic_gaussians(P, 3, seed=0, s0=0.03, n_cams=nv)
    with torch.no_grad():
        m._xyz[P - 2] = torch.tensor([0.0, 0.0, 1000.0])  # off every list
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(10 + i)) for i in range(nv)]
    cams = orbit_cameras(nv, W, H, seed=1, images=gts)
    m = m.to(DEV)
    for c in cams:
        c.to(DEV)
    m2 = copy.deepcopy(m)
    a = lm_step(m, cams[:3], cams[3:], torch.zeros(3), max_iter=3, restart_iter=3, multiview="batched")
    b = lm_step(m2, cams[:3], cams[3:], torch.zeros(3), max_iter=3, restart_iter=3, multiview="batched",
                union_active=True)
    clear_val_cache()
    print(f"lm_step: alpha {a['best_alpha']} / {b['best_alpha']}, final {a['final_val_loss']!r} / "
          f"{b['final_val_loss']!r}, step bitwise {torch.equal(a['step'], b['step'])}")
    assert a["best_alpha"] == b["best_alpha"]
    assert abs(a["final_val_loss"] - b["final_val_loss"]) <= 1e-4 * a["final_val_loss"]
    assert b["step"].numel() == a["step"].numel()
    for t1, t2 in zip(m.params(), m2.params()):
        assert _close(t2.detach(), t1.detach(), 1e-4)
    with pytest.raises(ValueError):
        lm_step(copy.deepcopy(m), cams[:3], cams[3:], torch.zeros(3), multiview="loop", union_active=True)
    clear_val_cache()


# ------------------------------------------------------------------------------------------------ 5. fallbacks, lifetime
def test_fallbacks_and_list_lifetime(monkeypatch):
    from gslm import lm
    from gslm.params import raw_gaussians
    model, cams = ms.scene(2000, 2, 3)
    model = copy.deepcopy(model).to(DEV)
    cams = [copy.deepcopy(c).to(DEV) for c in cams]
    D = lm.BatchedLMProblem(model, cams, torch.zeros(3))
    D.evaluate()
    D.rhs(D.zeros())
    assert D.active_view() is None  # off by default
    U = lm.BatchedLMProblem(model, cams, torch.zeros(3), union_active=True)
    U.evaluate()
    assert U.active_view() is None  # no row map yet
    g = U.rhs(U.zeros())
    a1 = U.active_view()
    assert a1 is not None and a1.active_view() is None
    ids1 = a1._active[0]
    assert U.active_view()._active[0] is ids1  # cached on the problem
    monkeypatch.setenv("GSLM_CG_ACTIVE", "0")
    assert U.active_view() is None and lm._active_view_for(U, g, None) is None
    monkeypatch.delenv("GSLM_CG_ACTIVE")
    assert lm._active_view_for(U, g, None) is not None
    # a forward on one view: its row map is gone, and so is the list
    U.views[1].forward(raw_gaussians(model), U.stream, want_invdepth=False)
    assert U.active_view() is None and U._union is None
    U.matvec(g, U.zeros())  # rebuilds the maps
    a2 = U.active_view()
    assert a2 is not None and a2._active[0] is not ids1 and torch.equal(a2._active[0], ids1)
    # evaluate(): every view's epoch moves, the list is rebuilt after the next rhs()
    U.evaluate()
    assert U.active_view() is None
    U.rhs(U.zeros())
    a3 = U.active_view()
    assert a3 is not None and a3._active[0] is not a2._active[0] and torch.equal(a3._active[0], ids1)
    # stage_times works on the active view
    t = a3.stage_times(a3.pack(g), reps=2)
    assert set(t) == set(lm.BatchedLMProblem.STAGES) | {"total"} and all(v >= 0 for v in t.values())


def test_nothing_visible_takes_the_full_path():
    from gslm import lm
    model, cams = ms.scene(300, 2, 3)
    model = copy.deepcopy(model)
    model._xyz.data[:] = FAR(300)
    model = model.to(DEV)
    cams = [copy.deepcopy(c).to(DEV) for c in cams]
    U = lm.BatchedLMProblem(model, cams, torch.zeros(3), union_active=True)
    U.evaluate()
    g = U.rhs(U.zeros())
    assert [vr.N for vr in U.views] == [0, 0]
    assert U.union_list()[1] == 0 and U.active_view() is None
    assert not g.any()


# ------------------------------------------------------------------------------------------------ 6. error returns
def test_error_returns_write_nothing():
    from gslm.params import raw_gaussians
    r = rig(6001, 2, 3)
    U, act, P, Pa = r.U, r.act, r.P, r.Pa
    g = raw_gaussians(U.model)
    views = (_lib.GslmView * 17)(*([U.views[0].view] * 17))
    ws = U._view_ws(0, 2)
    v = act.pack(r.restrict(r.random_v(5)))
    y0 = torch.randn_like(v)
    y = y0.clone()
    vs, ys = act.layout.grads_struct(v), act.layout.grads_struct(y)
    R = U.rest_basis()

    def opts(dot=None):
        o = _lib.GslmMatvecOpts()
        o.stages = 7 | 8
        o.rest_basis, o.rest_views = R.data_ptr(), U.rest_views
        if dot is not None:
            o.dot_vy, o.dot_scratch, o.dot_scratch_bytes = dot.data_ptr(), U.dot_scratch.data_ptr(), 0
        return o

    def gather(n=2, ws=ws, na=Pa, o=None, hs=P + 1):
        o = opts() if o is None else o
        return lib.gslm_gather_views_active(views, ws, n, ctypes.byref(g), ctypes.byref(vs), ctypes.byref(ys),
                                            r.ids.data_ptr(), na, r.hrow.data_ptr(), hs, r.aflags.data_ptr(), P,
                                            ctypes.byref(o), U.stream)

    INV, CAP = _lib.GSLM_ERR_INVALID, _lib.GSLM_ERR_CAPACITY
    assert gather(n=17) == INV and gather(n=0) == INV and gather(na=P + 1) == INV and gather(hs=Pa) == INV
    short = U._view_ws(0, 2)
    short[1].scratch_bytes = lib.gslm_scratch_bytes(P, U.views[1].N) - 1
    assert gather(ws=short) == CAP
    dot = torch.full((1,), 5.5, dtype=torch.float64, device=DEV)
    assert gather(o=opts(dot)) == CAP
    # the tangent pass: records untouched
    trec0 = U._trec.clone()
    tv = lambda n=2, mask=1, na=Pa: lib.gslm_tangent_views_active(
        views, n, ctypes.byref(g), ctypes.byref(vs), mask, r.ids.data_ptr(), na, r.aflags.data_ptr(), P,
        U._trec.data_ptr(), P, ctypes.byref(opts()), U.stream)
    assert tv(n=17) == INV and tv(mask=0) == INV and tv(na=P + 1) == INV and tv(na=-1) == INV
    # the list: outputs untouched
    ids = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    hrow = torch.full((2, P + 1), -7, dtype=torch.int32, device=DEV)
    afl = torch.full((2, P), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    work = _lib.u8(lib.gslm_active_union_bytes(P), DEV)
    au = lambda ws=ws, n=2, wb=work.numel(): lib.gslm_active_union(ws, n, P, work.data_ptr(), wb, ids.data_ptr(),
                                                                  hrow.data_ptr(), afl.data_ptr(), cnt.data_ptr(),
                                                                  U.stream)
    assert au(n=0) == INV and au(wb=work.numel() - 1) == CAP and au(ws=short) == CAP
    torch.cuda.synchronize()
    # (the table holds the NaN an earlier test planted off the list: compare the bits)
    assert torch.equal(y, y0) and float(dot) == 5.5 and torch.equal(U._trec.view(torch.int32), trec0.view(torch.int32))
    assert (ids == -7).all() and (hrow == -7).all() and (afl == -7).all() and int(cnt) == -7
    # and the same arguments, valid, do write
    assert au() == _lib.GSLM_OK and gather() == _lib.GSLM_OK
    torch.cuda.synchronize()
    assert int(cnt) == Pa and torch.equal(ids[:Pa], r.ids) and not torch.equal(y, y0)

