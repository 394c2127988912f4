"""The Python boundary of the drop-in rasterizer (diff_gaussian_rasterization/__init__.py: _RasterizeGaussians, _f32,
forward_buffers; gslm/_lib.py: _host_floats / _HOST_CACHE), on the call forms no other test hands it.

Every other test gives the kernels freshly built contiguous tensors.  Here:
  * input layouts: column-major means3D (X.t()), rotations / shs as slices of wider tensors, opacities as [P] and as
    [1, P].t(), scales as [P, 1].expand(P, 3) -- forward, backward and forward-AD jvp bitwise equal to the
    all-contiguous call, every leaf's gradient of the leaf's shape; the expanded scales' leaf gradient against the
    oracle's;
  * tangent layouts: _RasterizeGaussians.jvp handed transposed / expanded / sliced tangents, bitwise the contiguous ones
    (forward AD itself lays a tangent out like its primal, so only views of dual tensors bring other layouts);
  * cotangent forms: colour only, inverse depth only (grad_color is None), both, img.sum() (stride 0) and a permuted
    HWC cotangent, against the oracle's autograd gradients (oracle/torch_raster.py, 1e-4 of each tensor's max, the bar
    of tests/test_gpu_raster.py) and bitwise equal to the same values as fresh contiguous tensors (memo off, so the
    second call runs the kernels);
  * the settings host cache: hits, every kind of in-place write, another length, recycled ids and addresses, views of
    one [V, 4, 4] tensor, CPU tensors, the two switches, and a camera moved in place between two renders;
  * inputs on different devices: a ValueError that names the argument, raised before forward_buffers.
"""
import functools

import pytest
import torch
import torch.autograd.forward_ad as fwAD

from oracle import torch_raster as tr
from scenes import activated, gpu_settings, make_scene, oracle_settings

pytestmark = pytest.mark.gpu
DEV = "cuda"

SCENE_NAMES = ["tiny_300_sh2_40x33", "dense_2k_sh3_64x48"]
BG = (0.2, 0.5, 0.9)
KEYS = ("means3D", "opacities", "scales", "rotations", "shs")
VARIANTS = ["means3D_t", "rotations_slice", "shs_slice", "opacities_flat", "opacities_t", "scales_expand"]
ALL_TOGETHER = ("means3D_t", "rotations_slice", "shs_slice", "opacities_t", "scales_expand")


def _rel_err(a, b):
    scale = b.abs().max().clamp_min(1e-8)
    return ((a - b).abs().max() / scale).item()


@functools.lru_cache(maxsize=None)
def _case(name, iso):
    """(values, tangents, means2D tangent, camera, sh degree, colour cotangent, depth cotangent) of a scene, on the CPU;
    iso: every Gaussian's three scales (and their tangents) equal, so that they can be given as an expanded [P, 1]."""
    model, cams = make_scene(name)
    cam = cams[0]
    vals = activated(model)
    gen = torch.Generator().manual_seed(31)
    tang = {k: torch.randn(v.shape, generator=gen) for k, v in vals.items()}
    if iso:
        vals["scales"] = vals["scales"][:, :1].expand(-1, 3).contiguous()
        tang["scales"] = tang["scales"][:, :1].expand(-1, 3).contiguous()
    t_m2 = torch.randn(vals["means3D"].shape, generator=gen)
    H, W = int(cam.image_height), int(cam.image_width)
    dcol = torch.randn(3, H, W, generator=gen)
    ddep = torch.randn(1, H, W, generator=gen)
    return vals, tang, t_m2, cam, model.active_sh_degree, dcol, ddep


def _pack(vals, variants, seed):
    """Leaf tensors whose views (_view) hold `vals`; the columns a slice leaves out are filled with noise."""
    gen = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in vals.items()}
    P = vals["means3D"].shape[0]
    if "means3D_t" in variants:
        out["means3D"] = vals["means3D"].t().contiguous()
    if "rotations_slice" in variants:
        out["rotations"] = torch.cat([torch.randn(P, 1, generator=gen), vals["rotations"]], dim=1)
    if "shs_slice" in variants:
        out["shs"] = torch.cat([torch.randn(P, 1, 3, generator=gen), vals["shs"]], dim=1)
    if "opacities_flat" in variants:
        out["opacities"] = vals["opacities"].reshape(-1).clone()
    if "opacities_t" in variants:
        out["opacities"] = vals["opacities"].reshape(1, -1).clone()
    if "scales_expand" in variants:
        assert torch.equal(vals["scales"], vals["scales"][:, :1].expand(-1, 3))
        out["scales"] = vals["scales"][:, :1].contiguous()
    return out


def _view(leaves, variants):
    """What the rasterizer is handed."""
    a = dict(leaves)
    if "means3D_t" in variants:
        a["means3D"] = leaves["means3D"].t()
    if "rotations_slice" in variants:
        a["rotations"] = leaves["rotations"][:, 1:]
    if "shs_slice" in variants:
        a["shs"] = leaves["shs"][:, 1:]
    if "opacities_t" in variants:
        a["opacities"] = leaves["opacities"].t()
    if "scales_expand" in variants:
        a["scales"] = leaves["scales"].expand(-1, 3)
    return a


def _unpack_grads(g, variants):
    """Leaf gradients laid out as the contiguous call's; and the gradients of what a slice leaves out."""
    out, pad = dict(g), {}
    if "means3D_t" in variants:
        out["means3D"] = g["means3D"].t()
    if "rotations_slice" in variants:
        out["rotations"], pad["rotations"] = g["rotations"][:, 1:], g["rotations"][:, :1]
    if "shs_slice" in variants:
        out["shs"], pad["shs"] = g["shs"][:, 1:], g["shs"][:, :1]
    if "opacities_flat" in variants:
        out["opacities"] = g["opacities"].reshape(-1, 1)
    if "opacities_t" in variants:
        out["opacities"] = g["opacities"].t()
    if "scales_expand" in variants:
        del out["scales"]  # [P, 1]: a sum of the three columns, held to the oracle instead
    return out, pad


def _rast(st, a, m2):
    from diff_gaussian_rasterization import GaussianRasterizer
    return GaussianRasterizer(st)(means3D=a["means3D"], means2D=m2, shs=a["shs"], opacities=a["opacities"],
                                  scales=a["scales"], rotations=a["rotations"])


def _run(name, variants, iso):
    """Forward, backward (colour and depth cotangents) and forward-AD jvp with the inputs laid out per `variants`."""
    vals, tang, t_m2, cam, D, dcol, ddep = _case(name, iso)
    st = gpu_settings(cam, D, torch.tensor(BG))
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in _pack(vals, variants, 41).items()}
    args = _view(leaves, variants)
    for t in args.values():
        if not t.is_leaf:
            t.retain_grad()
    m2 = torch.zeros_like(vals["means3D"], device=DEV).requires_grad_(True)
    c, r, d = _rast(st, args, m2)
    torch.autograd.backward([c, d], [dcol.to(DEV), ddep.to(DEV)])
    out = dict(color=c.detach(), radii=r, invdepth=d.detach())
    arg_grads = {k: t.grad for k, t in args.items()} | {"means2D": m2.grad}
    leaf_grads = {k: t.grad for k, t in leaves.items()}
    with torch.no_grad(), fwAD.dual_level():
        tl = _pack(tang, variants, 43)
        dual = {k: fwAD.make_dual(leaves[k].detach(), tl[k].to(DEV)) for k in leaves}
        targs = _view(dual, variants)
        strides = {k: (fwAD.unpack_dual(t).primal.stride(), fwAD.unpack_dual(t).tangent.stride())
                   for k, t in targs.items()}
        tm2 = fwAD.make_dual(torch.zeros_like(vals["means3D"], device=DEV), t_m2.to(DEV))
        c, _, d = _rast(st, targs, tm2)
        out["color_tangent"] = fwAD.unpack_dual(c).tangent.clone()
        out["invdepth_tangent"] = fwAD.unpack_dual(d).tangent.clone()
    return out, arg_grads, leaf_grads, leaves, args, strides


@functools.lru_cache(maxsize=None)
def _contiguous_run(name, iso):
    out, arg_grads, _, _, args, _ = _run(name, (), iso)
    assert all(t.is_contiguous() for t in args.values())
    return out, arg_grads


@functools.lru_cache(maxsize=None)
def _oracle_scales_leaf_grad(name):
    """The oracle's gradient reaching s of scales = s.expand(P, 3), same cotangents as _run."""
    vals, _, _, cam, D, dcol, ddep = _case(name, True)
    a = {k: v.clone().requires_grad_(True) for k, v in vals.items()}
    s = vals["scales"][:, :1].clone().requires_grad_(True)
    c, _, d = tr.rasterize(a["means3D"], torch.zeros_like(a["means3D"]), a["opacities"],
                           oracle_settings(cam, D, torch.tensor(BG)), shs=a["shs"], scales=s.expand(-1, 3),
                           rotations=a["rotations"])
    torch.autograd.backward([c, d], [dcol, ddep])
    return s.grad.detach()


@pytest.mark.parametrize("name", SCENE_NAMES)
@pytest.mark.parametrize("variant", VARIANTS + ["all_together"])
def test_input_layouts_are_bitwise_the_contiguous_call(name, variant):
    variants = ALL_TOGETHER if variant == "all_together" else (variant,)
    iso = "scales_expand" in variants
    ref_out, ref_grads = _contiguous_run(name, iso)
    out, arg_grads, leaf_grads, leaves, args, strides = _run(name, variants, iso)
    # the variant is what it says: the Function sees that layout, primal and tangent
    for v, k in (("means3D_t", "means3D"), ("rotations_slice", "rotations"), ("shs_slice", "shs"),
                 ("scales_expand", "scales")):
        if v in variants:
            assert not args[k].is_contiguous()
            assert strides[k][0] == args[k].stride() and strides[k][1] == args[k].stride(), (k, strides[k])
    for k in ref_out:
        assert torch.equal(out[k], ref_out[k]), k
    assert float(ref_out["color_tangent"].abs().max()) > 0 and float(ref_out["invdepth_tangent"].abs().max()) > 0
    # the gradient the Function returns for each argument (means2D included)
    for k in ref_grads:
        assert arg_grads[k].shape == (args[k].shape if k in args else ref_grads[k].shape), k
        assert float(ref_grads[k].abs().max()) > 0, k
        assert torch.equal(arg_grads[k], ref_grads[k].reshape(arg_grads[k].shape)), f"gradient of {k}"
    # the gradient that reaches each leaf
    for k, t in leaves.items():
        assert leaf_grads[k].shape == t.shape, k
    back, pad = _unpack_grads(leaf_grads, variants)
    for k, g in back.items():
        assert torch.equal(g, ref_grads[k]), f"leaf gradient of {k}"
    for k, g in pad.items():
        assert not g.any(), f"{k}: the columns the slice leaves out have no gradient"
    if iso:
        ref = _oracle_scales_leaf_grad(name)
        got = leaf_grads["scales"].cpu()
        assert got.shape == ref.shape
        print(f"{name} {variant}: expanded scales leaf gradient rel err {_rel_err(got, ref):.3e}")
        assert _rel_err(got, ref) < 1e-4, f"expanded scales leaf gradient: rel err {_rel_err(got, ref):.3e}"


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_tangent_layouts_are_bitwise_the_contiguous_tangents(name):
    """_RasterizeGaussians.jvp on the node of one forward, with tangents in layouts forward AD can deliver through
    views of dual tensors.  The contiguous call is also bitwise what forward AD gives (_contiguous_run)."""
    from diff_gaussian_rasterization import _RasterizeGaussians
    vals, tang, t_m2, cam, D, _, _ = _case(name, True)
    st = gpu_settings(cam, D, torch.tensor(BG))
    a = {k: v.to(DEV).requires_grad_(True) for k, v in vals.items()}
    c, _, _ = _rast(st, a, torch.zeros_like(a["means3D"]))
    ctx = c.grad_fn
    T = {k: v.to(DEV) for k, v in tang.items()}
    T["means2D"] = t_m2.to(DEV)

    def jvp(t):
        with torch.no_grad():
            out = _RasterizeGaussians.jvp(ctx, t["means3D"], t["means2D"], t["shs"], None, None, t["opacities"],
                                          t["scales"], t["rotations"], None, None)
        return out[0], out[2]

    ref = jvp(T)
    fw, _ = _contiguous_run(name, True)
    assert torch.equal(ref[0], fw["color_tangent"]) and torch.equal(ref[1], fw["invdepth_tangent"])
    P = vals["means3D"].shape[0]
    wide = lambda t: torch.cat([torch.full_like(t[:, :1], 7.0), t], dim=1)[:, 1:]
    forms = {
        "means3D": T["means3D"].t().contiguous().t(),
        "means2D": T["means2D"].t().contiguous().t(),
        "scales": T["scales"][:, :1].contiguous().expand(-1, 3),
        "opacities": T["opacities"].reshape(1, P).clone().t(),
        "rotations": wide(T["rotations"]),
        "shs": wide(T["shs"]),
    }
    for k in ("means3D", "means2D", "scales", "rotations", "shs"):
        assert not forms[k].is_contiguous() and torch.equal(forms[k], T[k])
    assert forms["opacities"].stride() == (1, P)
    for k, t in list(forms.items()) + [("opacities_flat", T["opacities"].reshape(-1).clone())]:
        got = jvp(T | {k.replace("_flat", ""): t})
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), k
    got = jvp(forms)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), "all together"


# ---- cotangent forms

FORMS = ["colour", "invdepth", "both", "sum", "permuted"]


@functools.lru_cache(maxsize=None)
def _oracle_cotangent_grads(name):
    """The oracle's autograd gradients of every input for each cotangent form (one forward, four backward passes; the
    permuted cotangent holds the colour form's values)."""
    vals, _, _, cam, D, dcol, ddep = _case(name, False)
    a = {k: v.clone().requires_grad_(True) for k, v in vals.items()}
    a["means2D"] = torch.zeros_like(vals["means3D"], requires_grad=True)
    c, _, d = tr.rasterize(a["means3D"], a["means2D"], a["opacities"], oracle_settings(cam, D, torch.tensor(BG)),
                           shs=a["shs"], scales=a["scales"], rotations=a["rotations"])
    keys = list(a)

    def grads(outs, cots):
        g = torch.autograd.grad(outs, [a[k] for k in keys], cots, retain_graph=True, allow_unused=True)
        return {k: (torch.zeros_like(a[k]) if t is None else t.detach()) for k, t in zip(keys, g)}

    out = {"colour": grads([c], [dcol]), "invdepth": grads([d], [ddep]), "both": grads([c, d], [dcol, ddep]),
           "sum": grads([c.sum()], [torch.ones(())])}
    out["permuted"] = out["colour"]
    return out


@pytest.mark.parametrize("name", SCENE_NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_cotangent_forms(name, form, monkeypatch):
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_BWD_MEMO", False)  # the second call of a pair must run the kernels again
    seen = []
    inner = dgr._RasterizeGaussians._backward

    def recording(ctx, saved, grad_color, grad_invdepth):
        seen.append((grad_color, grad_invdepth))
        return inner(ctx, saved, grad_color, grad_invdepth)
    monkeypatch.setattr(dgr._RasterizeGaussians, "_backward", staticmethod(recording))

    vals, _, _, cam, D, dcol, ddep = _case(name, False)
    st = gpu_settings(cam, D, torch.tensor(BG))
    a = {k: v.to(DEV).requires_grad_(True) for k, v in vals.items()}
    a["means2D"] = torch.zeros_like(a["means3D"], requires_grad=True)
    keys = list(a)
    c, _, d = _rast(st, a, a["means2D"])
    dcol, ddep = dcol.to(DEV), ddep.to(DEV)

    def grads(outs, cots):
        g = torch.autograd.grad(outs, [a[k] for k in keys], cots, retain_graph=True, allow_unused=True)
        assert all(t is not None for t in g)
        return dict(zip(keys, g))

    if form == "colour":
        got, fresh = grads([c], [dcol]), grads([c], [dcol.clone()])
        assert seen[0][0] is not None and seen[0][1] is None
    elif form == "invdepth":
        got, fresh = grads([d], [ddep]), grads([d], [ddep.clone()])
        assert seen[0][0] is None and seen[0][1] is not None, "grad_color is None for a depth-only loss"
    elif form == "both":
        got, fresh = grads([c, d], [dcol, ddep]), grads([c, d], [dcol.clone(), ddep.clone()])
        assert seen[0][0] is not None and seen[0][1] is not None
    elif form == "sum":
        got = grads([c.sum()], [torch.ones((), device=DEV)])
        assert seen[0][0].stride() == (0, 0, 0), "img.sum().backward() brings a stride-0 cotangent"
        fresh = grads([c], [torch.ones_like(c)])
    else:
        hwc = dcol.permute(1, 2, 0).contiguous()
        got = grads([c], [hwc.permute(2, 0, 1)])
        assert not seen[0][0].is_contiguous() and torch.equal(seen[0][0], dcol)
        fresh = grads([c], [dcol.clone()])
    assert len(seen) == 2, "both calls of the pair ran the kernels"
    assert all(t is None or t.is_contiguous() for t in seen[1])
    ref = _oracle_cotangent_grads(name)[form]
    for k in keys:
        assert got[k].shape == a[k].shape and got[k].is_contiguous()
        assert torch.equal(got[k], fresh[k]), f"{form}: gradient of {k} differs from the fresh contiguous cotangent's"
        e = _rel_err(got[k].cpu(), ref[k])
        print(f"{name} {form}: grad {k} rel err {e:.3e}")
        assert e < 1e-4, f"{form}: grad {k}: rel err {e:.3e}"


# ---- the settings host cache

@pytest.fixture
def host_cache():
    from gslm import _lib
    was = _lib._HOST_CACHE_ON[0]
    _lib.set_host_cache(True)
    _lib.clear_host_cache()
    yield _lib
    _lib.clear_host_cache()
    _lib.set_host_cache(was)


def _floats(t, n):
    return [float(x) for x in t.detach().reshape(-1).cpu().tolist()][:n]


def _mat(seed):
    return torch.randn(4, 4, generator=torch.Generator().manual_seed(seed))


def test_host_cache_repeat_call_is_a_hit(host_cache):
    t = _mat(1).to(DEV)
    a = host_cache._host_floats(t, 16)
    assert a == _floats(t, 16) and len(host_cache._HOST_CACHE) == 1
    assert host_cache._host_floats(t, 16) is a, "a repeat call returns the cached list"
    assert host_cache._host_floats(t, 16) is a


@pytest.mark.parametrize("write", ["copy_", "index", "mul_"])
def test_host_cache_sees_in_place_writes(write, host_cache):
    t = _mat(2).to(DEV)
    before = host_cache._host_floats(t, 16)
    if write == "copy_":
        t.copy_(_mat(3))
    elif write == "index":
        t[3, :3] = torch.tensor([0.25, -1.5, 4.0], device=DEV)
    else:
        t.mul_(-2.0)
    after = host_cache._host_floats(t, 16)
    assert after == _floats(t, 16) and after != before
    assert host_cache._host_floats(t, 16) is after


def test_host_cache_keeps_lengths_apart(host_cache):
    t = _mat(4).to(DEV)
    full = _floats(t, 16)
    assert host_cache._host_floats(t, 16) == full
    assert host_cache._host_floats(t, 3) == full[:3]
    assert host_cache._host_floats(t, 16) == full
    c = torch.tensor([1.0, 2.0, 3.0, 4.0], device=DEV)
    assert host_cache._host_floats(c, 3) == [1.0, 2.0, 3.0]
    assert host_cache._host_floats(c, 4) == [1.0, 2.0, 3.0, 4.0]


def test_host_cache_with_recycled_ids_and_addresses(host_cache):
    """A tensor dies and another takes its place: the allocator hands out the same address and Python often the same
    id, and every read must still be the new tensor's values."""
    start = len(host_cache._HOST_CACHE)
    ids, ptrs, id_back, ptr_back = set(), set(), 0, 0
    for k in range(32):
        t = (_mat(100 + k) + k).to(DEV)
        want = _floats(t, 16)
        assert host_cache._host_floats(t, 16) == want, f"round {k}"
        id_back += id(t) in ids
        ptr_back += t.data_ptr() in ptrs
        ids.add(id(t))
        ptrs.add(t.data_ptr())
        del t
        assert len(host_cache._HOST_CACHE) == start
    print(f"recycled over 32 rounds: id {id_back} times, data_ptr {ptr_back} times")


def test_host_cache_views_of_one_tensor(host_cache):
    V = 5
    M = torch.stack([_mat(10 + b) for b in range(V)]).to(DEV)
    start = len(host_cache._HOST_CACHE)
    for _ in range(2):
        for b in range(V):
            assert host_cache._host_floats(M[b], 16) == _floats(M[b], 16), b  # a fresh view object per call
    assert len(host_cache._HOST_CACHE) == start, "entries of freed views are dropped"
    held = [M[b] for b in range(V)]
    for b in range(V):
        assert host_cache._host_floats(held[b], 16) == _floats(M[b], 16)
    assert len(host_cache._HOST_CACHE) == start + V
    M[1].mul_(3.0)  # a write through another view of the same storage: the version counter is shared
    M[4, 0, 0] = -9.0
    for b in range(V):
        assert host_cache._host_floats(held[b], 16) == _floats(M[b], 16), b
    del held
    assert len(host_cache._HOST_CACHE) == start


def test_host_cache_never_holds_cpu_tensors(host_cache):
    t = _mat(5)
    a = host_cache._host_floats(t, 16)
    assert a == _floats(t, 16) and len(host_cache._HOST_CACHE) == 0
    t.data.mul_(2.0)
    assert host_cache._host_floats(t, 16) == _floats(t, 16) != a
    assert host_cache._host_floats([1, 2, 3, 4], 3) == [1.0, 2.0, 3.0] and len(host_cache._HOST_CACHE) == 0


def test_host_cache_switches(host_cache):
    t, u = _mat(6).to(DEV), _mat(7).to(DEV)
    host_cache._host_floats(t, 16)
    host_cache._host_floats(u, 16)
    assert len(host_cache._HOST_CACHE) == 2
    host_cache.clear_host_cache()
    assert len(host_cache._HOST_CACHE) == 0
    assert host_cache._host_floats(t, 16) == _floats(t, 16) and len(host_cache._HOST_CACHE) == 1
    host_cache.set_host_cache(False)
    assert len(host_cache._HOST_CACHE) == 0
    before = host_cache._host_floats(t, 16)
    assert before == _floats(t, 16) and len(host_cache._HOST_CACHE) == 0, "nothing is cached while it is off"
    v = t._version
    t.data.copy_(_mat(8))  # a write the version counter does not see
    assert t._version == v
    after = host_cache._host_floats(t, 16)
    assert after == _floats(t, 16) and after != before
    host_cache.set_host_cache(True)
    assert host_cache._host_floats(t, 16) == after and len(host_cache._HOST_CACHE) == 1


def test_camera_moved_in_place_between_renders(host_cache):
    """Render, write another camera into the same settings tensors, render again: bitwise the render (and gradients) of
    freshly built settings."""
    model, cams = make_scene("tiny_300_sh2_40x33")
    D = model.active_sh_degree
    vals = {k: v.to(DEV) for k, v in activated(model).items()}
    dcol = _case("tiny_300_sh2_40x33", False)[5].to(DEV)

    def render(st):
        a = {k: v.clone().requires_grad_(True) for k, v in vals.items()}
        c, r, d = _rast(st, a, torch.zeros_like(a["means3D"]))
        c.backward(dcol)
        return [c.detach(), r, d.detach()] + [a[k].grad for k in KEYS]

    st = gpu_settings(cams[0], D, torch.tensor(BG))
    first = render(st)
    assert len(host_cache._HOST_CACHE) == 4
    fresh = [render(gpu_settings(cam, D, torch.tensor(BG))) for cam in cams]
    for x, y in zip(first, fresh[0]):
        assert torch.equal(x, y)
    assert not torch.equal(fresh[0][0], fresh[1][0])
    st.viewmatrix.copy_(cams[1].world_view_transform)
    st.projmatrix[:] = cams[1].full_proj_transform.to(DEV)
    st.campos.mul_(0).add_(cams[1].camera_center.to(DEV))
    moved = render(st)
    for x, y in zip(moved, fresh[1]):
        assert torch.equal(x, y)


# ---- inputs on different devices

@pytest.mark.parametrize("arg", ["means3D", "means2D", "shs", "dc", "colors_precomp", "opacities", "scales",
                                 "rotations", "cov3D_precomp"])
def test_mixed_devices_are_refused_before_the_library(arg, monkeypatch):
    import diff_gaussian_rasterization as dgr

    def reached(*_a, **_k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(dgr, "forward_buffers", reached)
    vals, _, _, cam, D, _, _ = _case("tiny_300_sh2_40x33", False)
    P = vals["means3D"].shape[0]
    inp = dict(means3D=vals["means3D"], means2D=torch.zeros(P, 3), opacities=vals["opacities"])
    if arg in ("colors_precomp", "cov3D_precomp"):
        inp.update(colors_precomp=torch.rand(P, 3), cov3D_precomp=torch.rand(P, 6))
    else:
        inp.update(scales=vals["scales"], rotations=vals["rotations"])
        if arg == "dc":
            inp.update(dc=vals["shs"][:, :1].contiguous(), shs=vals["shs"][:, 1:].contiguous())
        else:
            inp.update(shs=vals["shs"])
    inp = {k: (v if k == arg else v.to(DEV)) for k, v in inp.items()}
    assert not inp[arg].is_cuda and sum(v.is_cuda for v in inp.values()) == len(inp) - 1
    rast = dgr.GaussianRasterizer(gpu_settings(cam, D))
    with pytest.raises(ValueError, match=rf"\b{arg}\b"):
        rast(**inp)
    with pytest.raises(ValueError, match=rf"\b{arg}\b"):
        rast(**{k: v.clone().requires_grad_(True) for k, v in inp.items()})
