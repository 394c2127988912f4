"""GPU: the state lm_step keeps from one LM step to the next (gslm.lm._VAL_CACHE, cache_val=True -- the default, and the
path every step of a training run after the first takes) against fresh evaluators.

Every lm_step case is a sequence  step A -> event -> step B  run twice from identical starting state (deep copies of
one seeded scene, seeded events):
  * run K keeps the default cache_val=True throughout, so step B runs on step A's LossEvaluator: its workspaces, its
    union-binning slots, each view's cached depth order and inverse;
  * run F passes cache_val=False and calls clear_val_cache() before each step, so step B builds a fresh evaluator.
The fresh evaluator is the reference (it is pinned to the oracle elsewhere) and the claim is exactness: step B's trace,
best_alpha, final_val_loss, val_start_loss and every stepped leaf are compared with `==` / torch.equal, no tolerance.
Each case also asserts what the cache did (hit, re-sorted, dropped for one view, rebuilt), so that a case cannot pass
because the kept path quietly was not taken.

The events are the things a training loop does between two LM steps: nothing, xyz moved by torch, xyz moved by
FusedAdam / SparseGaussianAdam (which write through raw pointers: gslm_adam_step), pruning, densification, every leaf
replaced by a new tensor at the same size (the allocator may hand back the old address), a validation camera moved, a
validation image overwritten, the SH degree raised, another background.

The scene: 3000 SH-2 Gaussians large enough to overlap heavily (s0 = 0.05), 64x48 images, one training view, three
validation views at val_batch=2 (both slot sets of evaluate_points and a short last batch), random ground truths,
max_iter=2, restart_iter=1.

The last tests state the optimizer contract the depth-order key relies on: FusedAdam.step and SparseGaussianAdam.step
bump the version counter of every tensor they write, as torch.optim.Adam's in-place ops do.

What these cases found when they were written: the Adam steps bumped nothing, so the two Adam cases (and the
evaluator-level one) blended every validation view in the depth order of the old xyz and failed at `trace ==`, and
the contract tests failed at the version comparison and at the missing RuntimeError; the leaves placed over the old
storage failed at `trace ==` while the orders were keyed on xyz's address and version.  The other cases passed and
are regression tests.
"""
import copy
import functools
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
P0, W, H = 3000, 64, 48
LEAVES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
STEP_KW = dict(max_iter=2, restart_iter=1, val_batch=2, val_at_start=True)


@functools.lru_cache(maxsize=None)
def _base():
    """The scene on the host, built once: (model, [training camera], [3 validation cameras])."""
    from gslm.cameras import orbit_cameras
    from gslm.model import synthetic_gaussians
    m = synthetic_gaussians(P0, 2, seed=0, s0=0.05)
    cams = orbit_cameras(4, W, H, seed=7)
    for i, c in enumerate(cams):
        c.original_image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(60 + i))
    return m, cams[:1], cams[1:]


def _randn(shape, seed, scale=1.0):
    return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to(DEV)


class _Run:
    """One run of a sequence on its own deep copy of the scene: kept=True is run K, kept=False run F."""

    def __init__(self, kept, setup=None):
        from gslm import lm
        lm.clear_val_cache()
        m, train, val = _base()
        self.kept = kept
        self.m = copy.deepcopy(m).to(DEV)
        self.train = [copy.deepcopy(c).to(DEV) for c in train]
        self.val = [copy.deepcopy(c).to(DEV) for c in val]
        self.bg = torch.zeros(3)
        if setup is not None:
            setup(self.m)

    def step(self):
        from gslm import lm
        if not self.kept:
            lm.clear_val_cache()
        out = lm.lm_step(self.m, self.train, self.val, self.bg, cache_val=self.kept, **STEP_KW)
        if not self.kept:
            assert "last" not in lm._VAL_CACHE
        return out

    @property
    def evaluator(self):
        from gslm import lm
        return lm._VAL_CACHE["last"][1]


def _setup_adam(optimizer_type="default"):
    def setup(m):
        from gslm.train import OptimizationParams
        m.optimizer_type = optimizer_type
        m.training_setup(OptimizationParams(optimizer_type=optimizer_type))
    return setup


def _orders_of(ev):
    """(the order tensors themselves, copies of their contents, the inverse tensors themselves)."""
    assert all(o is not None for o in ev._orders) and all(p is not None for p in ev._pos)
    return list(ev._orders), [o.clone() for o in ev._orders], list(ev._pos)


def _p_sized_workspaces(ev):
    """Every workspace of the evaluator sized by P: evaluate()'s slot geometries, evaluate_points' records and union
    geometries in both slot sets, and the sort geometry."""
    ws = [sl["geom"] for sl in ev.slots] + [getattr(ev, "_sgeom", None)]
    for par in ev.uslots:
        for sl in par:
            ws += list(sl["geoms"]) + [sl["ugeom"]]
    return [t for t in ws if t is not None]


def _assert_same_step(bk, bf, mk, mf):
    """Step B of run K against step B of run F, bitwise."""
    assert bk["trace"] == bf["trace"]
    assert bk["best_alpha"] == bf["best_alpha"]
    assert bk["final_val_loss"] == bf["final_val_loss"]
    assert bk["val_start_loss"] == bf["val_start_loss"]
    assert bk["start_loss"] == bf["start_loss"]
    assert torch.equal(bk["step"], bf["step"])
    for name in LEAVES + ("_exposure",):
        assert torch.equal(getattr(mk, name), getattr(mf, name)), name


def _sequence(event, setup=None, after_event=None):
    """Run K and run F of  step A -> event(run) -> step B.  Returns (K, what run K observed, step B of K, step B of F);
    the two step Bs are compared here.  after_event(run K, what it observed): checks made on run K's model between
    the event and step B."""
    from gslm import lm
    K = _Run(True, setup)
    ak = K.step()
    ev = K.evaluator
    seen = dict(a=ak, ev=ev, orders=_orders_of(ev), num_rendered=list(ev.num_rendered),
                union_counts=list(ev.union_counts), ws=_p_sized_workspaces(ev),
                ws_bytes=[t.numel() for t in _p_sized_workspaces(ev)], P=K.m._xyz.shape[0])
    event(K)
    if after_event is not None:
        after_event(K, seen)
    bk = K.step()
    seen["ev_b"] = lm._VAL_CACHE["last"][1]
    F = _Run(False, setup)
    af = F.step()
    # (step A itself: the two runs start equal)
    assert ak["trace"] == af["trace"] and ak["final_val_loss"] == af["final_val_loss"]
    event(F)
    bf = F.step()
    _assert_same_step(bk, bf, K.m, F.m)
    lm.clear_val_cache()
    return K, seen, bk, bf


def _is_permutation(order, P):
    return order.numel() == P and torch.equal(torch.sort(order.long()).values, torch.arange(P, device=order.device))


# ------------------------------------------------------------------------------------------------ 1. nothing in between
def test_nothing_in_between_is_a_hit():
    K, seen, bk, _ = _sequence(lambda run: None)
    ev = seen["ev_b"]
    assert ev is seen["ev"]
    objs, _, pos = seen["orders"]
    for i in range(3):  # the orders and their inverses were not built again
        assert ev._orders[i] is objs[i] and ev._pos[i] is pos[i]
    # step A moved scales and opacities: the reused buffers saw other list lengths
    assert (list(ev.num_rendered) != seen["num_rendered"]) or (list(ev.union_counts) != seen["union_counts"])
    assert all(n > 0 for n in ev.num_rendered) and all(n > 0 for n in ev.union_counts)
    # step B starts where step A ended: the same parameters through the same evaluator
    assert bk["val_start_loss"] == seen["a"]["final_val_loss"]


# ------------------------------------------------------------------------------------------------ 2. xyz moved by torch
def _move_inplace(run):
    with torch.no_grad():
        run.m._xyz.add_(_randn(run.m._xyz.shape, 11, 0.3))


def _assert_resorted(ev, seen):
    objs, contents, _ = seen["orders"]
    for i in range(len(objs)):
        assert ev._orders[i] is not None
        assert ev._orders[i] is not objs[i] or not torch.equal(ev._orders[i], contents[i]), i
        assert not torch.equal(ev._orders[i], contents[i]), i  # (every move here changes every view's order)


def test_xyz_moved_in_place_by_torch():
    K, seen, _, _ = _sequence(_move_inplace)
    assert seen["ev_b"] is seen["ev"]
    _assert_resorted(seen["ev_b"], seen)


# ------------------------------------------------------------------------------------------------ 3, 4. moved by Adam
def _xyz_group(m):
    return next(g for g in m.optimizer.param_groups if g["name"] == "xyz")


def _move_fused_adam(run):
    """One FusedAdam step on xyz alone (the other groups have no gradient): the first Adam step moves every coordinate
    by lr g / (|g| + eps) = +-0.3."""
    m = run.m
    _xyz_group(m)["lr"] = 0.3
    m._xyz.grad = _randn(m._xyz.shape, 12)
    m.optimizer.step()
    m._xyz.grad = None


def _move_sparse_adam(run):
    """One SparseGaussianAdam step on the xyz of the ~60 % of Gaussians a seeded visibility mask selects.  It has no
    bias correction: the first step moves a coordinate by lr 0.1 g / (sqrt(0.001) |g| + eps) = +-3.16 lr, so lr = 0.1
    gives the +-0.3 of the dense case."""
    m = run.m
    P = m._xyz.shape[0]
    _xyz_group(m)["lr"] = 0.1
    m._xyz.grad = _randn(m._xyz.shape, 13)
    vis = (torch.rand(P, generator=torch.Generator().manual_seed(14)) < 0.6).to(DEV)
    m.optimizer.step(vis, P)
    m._xyz.grad = None


def _stale_order_is_visible(K, seen):
    """The case's own precondition, on run K's model after the move: (a) every validation view's fresh depth order
    differs from the one cached before the move, and (b) rendering in the old orders (permutations of 0..P-1 at the
    current P: a supported mode-2 call of gslm_preprocess_ordered) gives another loss than rendering fresh -- so an
    evaluator that kept them cannot pass the comparison with run F by luck."""
    from gslm.lm import LossEvaluator
    m, P = K.m, K.m._xyz.shape[0]
    _, old, _ = seen["orders"]
    fresh = LossEvaluator(m, K.val, K.bg, batch=2)
    loss_fresh = float(fresh.evaluate())
    for i in range(3):
        assert _is_permutation(old[i], P) and _is_permutation(fresh._orders[i], P)
        assert not torch.equal(fresh._orders[i], old[i]), i  # (a)
    stale = LossEvaluator(m, K.val, K.bg, batch=2)
    stale._refresh_orders(m._xyz, P)  # the key of the model as it is now ...
    stale._orders = [o.clone() for o in old]  # ... over the orders of xyz before the move
    loss_stale = float(stale.evaluate())
    for i in range(3):
        assert torch.equal(stale._orders[i], old[i])  # (it rendered in them: mode 2 leaves the order alone)
    print(f"loss fresh {loss_fresh!r}, in the stale orders {loss_stale!r}")
    assert loss_stale != loss_fresh  # (b)


def test_xyz_moved_by_fused_adam():
    K, seen, _, _ = _sequence(_move_fused_adam, setup=_setup_adam(), after_event=_stale_order_is_visible)
    assert seen["ev_b"] is seen["ev"]
    _assert_resorted(seen["ev_b"], seen)


def test_xyz_moved_by_sparse_adam():
    K, seen, _, _ = _sequence(_move_sparse_adam, setup=_setup_adam("sparse_adam"), after_event=_stale_order_is_visible)
    from gslm.optim import SparseGaussianAdam
    assert isinstance(K.m.optimizer, SparseGaussianAdam)
    assert seen["ev_b"] is seen["ev"]
    _assert_resorted(seen["ev_b"], seen)


# ------------------------------------------------------------------------------------------------ 5, 6. P changes
def _prune(run):
    P = run.m._xyz.shape[0]
    run.m.prune_points((torch.rand(P, generator=torch.Generator().manual_seed(15)) < 0.3).to(DEV))


def test_p_shrinks_by_pruning():
    K, seen, _, _ = _sequence(_prune, setup=_setup_adam())
    ev, P = seen["ev_b"], K.m._xyz.shape[0]
    assert ev is seen["ev"]
    assert 0.6 * P0 < P < 0.8 * P0
    for i in range(3):
        assert _is_permutation(ev._orders[i], P) and ev._pos[i].numel() == P
    # every P-sized workspace is step A's, at step A's (larger) size
    ws = _p_sized_workspaces(ev)
    assert len(ws) == len(seen["ws"])
    for a, b, nb in zip(ws, seen["ws"], seen["ws_bytes"]):
        assert a is b and a.numel() == nb


def _clone_rows(run):
    """densification_postfix on 500 cloned rows (densify_and_clone's call with a seeded selection)."""
    m = run.m
    P = m._xyz.shape[0]
    sel = torch.randperm(P, generator=torch.Generator().manual_seed(16))[:500].to(DEV)
    m.tmp_radii = torch.zeros(P, device=DEV)
    with torch.no_grad():
        m.densification_postfix(m._xyz[sel], m._features_dc[sel], m._features_rest[sel], m._opacity[sel],
                                m._scaling[sel], m._rotation[sel], m.tmp_radii[sel])
    m.tmp_radii = None


def test_p_grows_by_densification():
    from gslm._lib import lib
    K, seen, _, _ = _sequence(_clone_rows, setup=_setup_adam())
    ev, P = seen["ev_b"], K.m._xyz.shape[0]
    assert ev is seen["ev"] and P == P0 + 500
    for i in range(3):
        assert _is_permutation(ev._orders[i], P) and ev._pos[i].numel() == P
    # the workspaces regrew: none of step A's P-sized buffers holds the new P
    ws = _p_sized_workspaces(ev)
    assert len(ws) == len(seen["ws"])
    for a, b, nb in zip(ws, seen["ws"], seen["ws_bytes"]):
        assert a is not b and a.numel() > nb
    assert all(sl["geom"].numel() >= lib.gslm_geom_bytes(P) for sl in ev.slots)


# ------------------------------------------------------------------------------------------------ 7. leaves replaced
def _permuted_rows(m):
    P = m._xyz.shape[0]
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(17))
    host = {name: getattr(m, name).detach().cpu()[perm].contiguous() for name in LEAVES}
    torch.cuda.synchronize()
    return host


def _replace_leaves(run):
    """Every per-Gaussian leaf replaced by a row permutation of itself in a new Parameter: the values go to the host,
    the device tensors are dropped, the new ones are built.  Whether the allocator hands the old addresses back is
    its business (the test prints it); the new tensors are at version 0, as the old xyz is (the masked LM step never
    writes it)."""
    m = run.m
    host = _permuted_rows(m)
    old = {name: getattr(m, name).data_ptr() for name in LEAVES}
    for name in LEAVES:
        setattr(m, name, None)
    gc.collect()
    for name in LEAVES:
        setattr(m, name, torch.nn.Parameter(host[name].to(DEV)))
    run.addresses = [(name, old[name] == getattr(m, name).data_ptr(), getattr(m, name)._version) for name in LEAVES]


def _replace_leaves_in_the_old_storage(run):
    """The same event with the allocator's part decided: each new Parameter is placed over the storage of the leaf it
    replaces and filled through `.data`, so it is another tensor object at the old address with a version counter of
    its own at 0 -- what a freed and re-allocated block gives, every time.  xyz's old counter is at 0 too: its address
    and version do not tell the new tensor from the old one."""
    m = run.m
    host = _permuted_rows(m)
    assert m._xyz._version == 0
    run.addresses = []
    for name in LEAVES:
        old = getattr(m, name)
        new = torch.nn.Parameter(torch.empty(0, device=DEV))
        new.data = old.detach()
        new.data.copy_(host[name].to(DEV))
        setattr(m, name, new)
        assert new is not old and new.data_ptr() == old.data_ptr() and new._version == 0 and new.is_contiguous()
        run.addresses.append((name, True, new._version))
        del old
    torch.cuda.synchronize()


@pytest.mark.parametrize("event", [_replace_leaves, _replace_leaves_in_the_old_storage])
def test_every_leaf_replaced_at_the_same_size(event):
    K, seen, _, _ = _sequence(event)
    print("leaf, at the old address, version:", K.addresses)
    assert seen["ev_b"] is seen["ev"]
    assert K.m._xyz.shape[0] == seen["P"]
    _assert_resorted(seen["ev_b"], seen)


# ------------------------------------------------------------------------------------------------ 8. a camera moved
def _move_camera(run):
    """Validation camera 1 to another pose, its matrices rebuilt with in-place writes."""
    from gslm.cameras import orbit_cameras
    c, n = run.val[1], orbit_cameras(1, W, H, seed=99)[0]
    assert not torch.equal(n.world_view_transform, c.world_view_transform.cpu())
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        getattr(c, name).copy_(getattr(n, name).to(DEV))


def test_one_validation_camera_moved():
    K, seen, _, _ = _sequence(_move_camera)
    ev = seen["ev_b"]
    assert ev is seen["ev"]
    objs, contents, pos = seen["orders"]
    assert ev._orders[1] is not objs[1] and ev._pos[1] is not pos[1]
    assert not torch.equal(ev._orders[1], contents[1])
    for i in (0, 2):
        assert ev._orders[i] is objs[i] and ev._pos[i] is pos[i]


# ------------------------------------------------------------------------------------------------ 9. an image rewritten
def _overwrite_image(run):
    c = run.val[2]
    c.original_image.copy_(torch.rand(3, H, W, generator=torch.Generator().manual_seed(18)).to(DEV))


def test_one_validation_image_overwritten_in_place():
    K, seen, bk, _ = _sequence(_overwrite_image)
    ev = seen["ev_b"]
    assert ev is seen["ev"]
    objs, _, pos = seen["orders"]
    for i in range(3):
        assert ev._orders[i] is objs[i] and ev._pos[i] is pos[i]
    # the new image is what step B rendered against: it starts at the parameters step A ended at, at another loss
    assert ev.gts[2] is K.val[2].original_image
    assert bk["val_start_loss"] != seen["a"]["final_val_loss"]


# ------------------------------------------------------------------------------------------------ 10. the key misses
def _degree_one(m):
    m.active_sh_degree = 1


def test_sh_degree_raised_builds_a_new_evaluator():
    def event(run):
        run.m.oneupSHdegree()
        assert run.m.active_sh_degree == 2
    K, seen, _, _ = _sequence(event, setup=_degree_one)
    assert seen["ev_b"] is not seen["ev"]
    assert seen["ev"].views[0].sh_degree == 1 and seen["ev_b"].views[0].sh_degree == 2


def test_another_background_builds_a_new_evaluator():
    def event(run):
        run.bg = torch.tensor([0.2, 0.5, 0.7])
    K, seen, _, _ = _sequence(event)
    assert seen["ev_b"] is not seen["ev"]
    assert list(seen["ev_b"].views[0].bg) == [float(x) for x in torch.tensor([0.2, 0.5, 0.7])]


# ------------------------------------------------------------------------------------------------ one LossEvaluator
def _sets(m, seed, n=3):
    """n line-search points: snapshots after seeded in-place moves of every group but xyz (the model ends at the
    last), large enough that radii, rects and quadrant masks differ between the points."""
    from gslm.lm import param_snapshot
    sets = []
    for a in range(n):
        with torch.no_grad():
            m._scaling.add_(_randn(m._scaling.shape, seed + 10 * a, 0.2))
            m._opacity.add_(_randn(m._opacity.shape, seed + 10 * a + 1, 0.5))
            m._features_dc.add_(_randn(m._features_dc.shape, seed + 10 * a + 2, 0.1))
            m._rotation.add_(_randn(m._rotation.shape, seed + 10 * a + 3, 0.1))
        sets.append(param_snapshot(m))
    return sets


@pytest.mark.parametrize("mover", ["torch", "fused_adam"])
def test_one_evaluator_across_an_xyz_move(mover):
    """evaluate() -> evaluate_points(sets) -> xyz moved -> evaluate_points(sets2) -> evaluate() on ONE LossEvaluator,
    each result against an evaluator built for that call alone."""
    from gslm.lm import LossEvaluator
    run = _Run(True, _setup_adam() if mover == "fused_adam" else None)
    m, val, bg = run.m, run.val, run.bg

    def fresh():
        return LossEvaluator(m, val, bg, batch=2)

    ev = fresh()
    assert float(ev.evaluate()) == float(fresh().evaluate())
    sets = _sets(m, 100)
    assert [float(x) for x in ev.evaluate_points(sets)] == [float(x) for x in fresh().evaluate_points(sets)]
    old = [o.clone() for o in ev._orders]
    (_move_fused_adam if mover == "fused_adam" else _move_inplace)(run)
    sets2 = _sets(m, 200)
    assert all(s._xyz is m._xyz for s in sets2)
    ref = fresh()
    want = [float(x) for x in ref.evaluate_points(sets2)]
    for i in range(3):
        assert not torch.equal(ref._orders[i], old[i])  # the move changed every view's order
    assert [float(x) for x in ev.evaluate_points(sets2)] == want
    for i in range(3):
        assert torch.equal(ev._orders[i], ref._orders[i]), i
    assert float(ev.evaluate()) == float(fresh().evaluate())
    assert len(set(want)) == len(want)  # (the points differ)


# ------------------------------------------------------------------------------------------------ optimizer contract
def _optimizers():
    from gslm.optim import FusedAdam, SparseGaussianAdam
    N = 257

    def fused(groups):
        opt = FusedAdam(groups, lr=0.0, eps=1e-15)
        return opt, opt.step

    def sparse(groups):
        opt = SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
        vis = (torch.rand(N, generator=torch.Generator().manual_seed(5)) < 0.6).to(DEV)
        return opt, lambda: opt.step(vis, N)

    return {"fused": fused, "sparse": sparse}, N


@pytest.mark.parametrize("kind", ["fused", "sparse"])
def test_optimizer_step_bumps_the_versions_of_what_it_writes(kind):
    makers, N = _optimizers()
    p = torch.nn.Parameter(_randn((N, 3), 1))
    q = torch.nn.Parameter(_randn((N, 4), 2))  # never given a gradient
    opt, step = makers[kind]([{"params": [p], "lr": 0.01, "name": "p"}, {"params": [q], "lr": 0.01, "name": "q"}])
    p0, q0, v0 = p.detach().clone(), q.detach().clone(), (p._version, q._version)
    p.grad = _randn((N, 3), 3)
    step()
    assert not torch.equal(p.detach(), p0)
    assert p._version > v0[0]
    assert q._version == v0[1] and torch.equal(q.detach(), q0) and len(opt.state[q]) == 0
    st = opt.state[p]
    before = (p._version, st["exp_avg"]._version, st["exp_avg_sq"]._version)
    step()  # the moments exist now: their counters move with the parameter's
    after = (p._version, st["exp_avg"]._version, st["exp_avg_sq"]._version)
    assert all(a > b for a, b in zip(after, before)), (before, after)
    assert q._version == v0[1]


@pytest.mark.parametrize("kind", ["fused", "sparse"])
def test_backward_through_a_stepped_parameter_raises(kind):
    """y = f(p); opt.step(); y.backward() must not differentiate at the stepped values in silence: torch.optim.Adam
    (run here as the reference) raises, and so do the fused steps."""
    makers, N = _optimizers()

    def three_lines(make):
        p = torch.nn.Parameter(_randn((N, 3), 4))
        step = make([{"params": [p], "lr": 0.01, "name": "p"}])
        p.grad = _randn((N, 3), 6)
        y = (p * p).sum()
        step()
        y.backward()

    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        three_lines(lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15).step)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        three_lines(lambda groups: makers[kind](groups)[1])
