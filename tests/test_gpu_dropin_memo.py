"""The drop-in backward's memo for equal cotangents (diff_gaussian_rasterization/__init__.py,
_RasterizeGaussians.backward).

The reference's J^T v (solver_functions.py:101-132) runs two backward calls on one graph, one per half of the [r; r]
pair (loss_image_state.py:93-97); with disable_ssim both halves are the same image (batch_training_loss.py:15-17), so
the two cotangents are equal.  A call whose cotangent equals the previous call's (element for element) returns that
call's gradients.  Checked here through the reference's render() (gslm.train.render: activations in PyTorch, so the
returned gradients pass through autograd nodes and are accumulated into the leaves):
  * equal cotangents (a different tensor with the same values, as the reference's CG vectors are): every leaf's
    accumulated gradient bitwise that of the same two calls with the memo off;
  * a different cotangent on the second call, and a third call after the memo was used: bitwise as with it off
    (the memo is keyed on content and autograd never writes into the returned tensors).
Bitwise agreement with the memo off also holds for a memo that never fires or that answers when it must not, so:
  * it fires: the calls of _RasterizeGaussians._backward are counted (a counting wrapper put in its place);
  * it is safe: an input the Function saved, written in place between the two backward calls, raises autograd's
    "modified by an inplace operation" with the memo on as with it off (the saved tensors are read before the memo is
    looked at).  model._xyz is such an input (render() hands it over as it is).  model._opacity is not: the Function
    saves sigmoid(_opacity), and sigmoid's own backward reads its result, so a write to _opacity changes no tensor
    that this graph saved and raises nowhere, memo on or off -- that case is held to "same outcome as with the memo
    off", and the activated opacities handed to the Function directly are the case that must raise;
  * the inverse-depth cotangent is part of the key; the memo belongs to one graph; on leaf inputs AccumulateGrad gets
    the memo's tensors twice and must not write into them.
"""
import pytest
import torch

from scenes import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grads_of(model, calls, memo, monkeypatch):
    import diff_gaussian_rasterization as dgr
    from gslm.train import PipelineParams, render
    monkeypatch.setattr(dgr, "_BWD_MEMO", memo)
    cam = _grads_of.cam
    model.zero_grad()
    img = render(cam, model, PipelineParams(), torch.zeros(3, device=DEV))["render"]
    r = img - _grads_of.gt
    for k, v in enumerate(calls):
        r.backward(v, retain_graph=k + 1 < len(calls))
    return [None if t.grad is None else t.grad.detach().clone() for t in model.params()]


@pytest.mark.parametrize("pattern", ["equal", "different", "equal_then_different", "three_equal"])
def test_backward_memo_is_bitwise(pattern, monkeypatch):
    model, cams = make_scene("dense_2k_sh3_64x48")
    model = model.to(DEV)
    cam = cams[0].to(DEV)
    g = torch.Generator().manual_seed(11)
    shape = (3, int(cam.image_height), int(cam.image_width))
    _grads_of.cam = cam
    _grads_of.gt = torch.rand(shape, generator=g).to(DEV)
    v = torch.randn(shape, generator=g).to(DEV)
    w = torch.randn(shape, generator=g).to(DEV)
    calls = {"equal": [v, v.clone()],
             "different": [v, w],
             "equal_then_different": [v, v.clone(), w],
             "three_equal": [v, v.clone(), v.clone()]}[pattern]
    on = _grads_of(model, calls, True, monkeypatch)
    off = _grads_of(model, calls, False, monkeypatch)
    assert any(t is not None and t.abs().max() > 0 for t in off)
    for a, b in zip(on, off):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


# ---- does it fire, and is it safe

def _counting(monkeypatch):
    """Puts a counting wrapper in place of _RasterizeGaussians._backward (the kernels' side of backward)."""
    import diff_gaussian_rasterization as dgr
    inner = dgr._RasterizeGaussians._backward
    calls = []

    def counted(*args):
        calls.append(1)
        return inner(*args)
    monkeypatch.setattr(dgr._RasterizeGaussians, "_backward", staticmethod(counted))
    return calls


def _scene(seed=11):
    model, cams = make_scene("dense_2k_sh3_64x48")
    model = model.to(DEV)
    cam = cams[0].to(DEV)
    g = torch.Generator().manual_seed(seed)
    H, W = int(cam.image_height), int(cam.image_width)
    gt = torch.rand(3, H, W, generator=g).to(DEV)
    v = torch.randn(3, H, W, generator=g).to(DEV)
    w = torch.randn(3, H, W, generator=g).to(DEV)
    d = torch.randn(1, H, W, generator=g).to(DEV)
    d2 = torch.randn(1, H, W, generator=g).to(DEV)
    return model, cam, gt, v, w, d, d2


def _render(model, cam):
    from gslm.train import PipelineParams, render
    return render(cam, model, PipelineParams(), torch.zeros(3, device=DEV))


def _leaf_grads(model):
    return [None if t.grad is None else t.grad.detach().clone() for t in model.params()]


def _assert_same(on, off):
    assert any(t is not None and t.abs().max() > 0 for t in off)
    for a, b in zip(on, off):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


@pytest.mark.parametrize("memo", [True, False], ids=["memo_on", "memo_off"])
@pytest.mark.parametrize("pattern,expected", [("equal", 1), ("different", 2), ("equal_then_different", 2),
                                              ("three_equal", 1)])
def test_backward_memo_fires(pattern, expected, memo, monkeypatch):
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_BWD_MEMO", memo)
    calls = _counting(monkeypatch)
    model, cam, gt, v, w, _, _ = _scene()
    cots = {"equal": [v, v.clone()], "different": [v, w], "equal_then_different": [v, v.clone(), w],
            "three_equal": [v, v.clone(), v.clone()]}[pattern]
    r = _render(model, cam)["render"] - gt
    for k, c in enumerate(cots):
        r.backward(c, retain_graph=k + 1 < len(cots))
    assert len(calls) == (expected if memo else len(cots))


INPLACE = "modified by an inplace operation"


def _outcome_after_inplace_write(target, memo, monkeypatch):
    """Forward, backward(v), an in-place write to `target` under no_grad, backward(v.clone()): the RuntimeError's text,
    or the gradients if nothing raised."""
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_BWD_MEMO", memo)
    model, cam, gt, v, _, _, _ = _scene()
    if target == "opacities":  # the Function's own saved input: activated leaves handed to it directly
        from scenes import activated, gpu_settings
        a = {k: t.to(DEV).requires_grad_(True) for k, t in activated(model).items()}
        leaves = list(a.values())
        img, _, _ = dgr.GaussianRasterizer(gpu_settings(cam, model.active_sh_degree))(
            means3D=a["means3D"], means2D=torch.zeros_like(a["means3D"]), shs=a["shs"], opacities=a["opacities"],
            scales=a["scales"], rotations=a["rotations"])
        written = a["opacities"]
    else:
        leaves = model.params()
        img = _render(model, cam)["render"]
        written = getattr(model, target)
    r = img - gt
    r.backward(v, retain_graph=True)
    with torch.no_grad():
        written.mul_(0.5)
    try:
        r.backward(v.clone())
    except RuntimeError as e:
        return "raised", str(e)
    return "returned", [None if t.grad is None else t.grad.detach().clone() for t in leaves]


@pytest.mark.parametrize("target", ["_xyz", "_opacity", "opacities"])
def test_backward_memo_runs_the_version_check(target, monkeypatch):
    on = _outcome_after_inplace_write(target, True, monkeypatch)
    off = _outcome_after_inplace_write(target, False, monkeypatch)
    assert on[0] == off[0], f"memo on {on[0]}, memo off {off[0]}"
    if target == "_opacity":
        # no tensor this graph saved was written (module docstring): nothing to raise, and the same gradients
        assert off[0] == "returned"
        _assert_same(on[1], off[1])
    else:
        assert off[0] == "raised" and INPLACE in off[1], off[1]
        assert on[0] == "raised" and INPLACE in on[1], on[1]


def _depth_key_grads(pairs, memo, monkeypatch):
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_BWD_MEMO", memo)
    calls = _counting(monkeypatch)
    model, cam, gt, *_ = _scene()
    out = _render(model, cam)
    img, depth = out["render"] - gt, out["depth"]
    for k, (cv, cd) in enumerate(pairs):
        keep = k + 1 < len(pairs)
        if cd is None:
            torch.autograd.backward([img], [cv], retain_graph=keep)
        else:
            torch.autograd.backward([img, depth], [cv, cd], retain_graph=keep)
    return _leaf_grads(model), len(calls)


@pytest.mark.parametrize("case,expected", [("same_depth", 1), ("other_depth", 2), ("none_then_depth", 2),
                                           ("depth_then_none", 2)])
def test_backward_memo_keys_on_the_depth_cotangent(case, expected, monkeypatch):
    _, _, _, v, _, d, d2 = _scene()
    pairs = {"same_depth": [(v, d), (v.clone(), d.clone())], "other_depth": [(v, d), (v.clone(), d2)],
             "none_then_depth": [(v, None), (v.clone(), d)], "depth_then_none": [(v, d), (v.clone(), None)]}[case]
    on, n_on = _depth_key_grads(pairs, True, monkeypatch)
    off, n_off = _depth_key_grads(pairs, False, monkeypatch)
    assert n_on == expected and n_off == 2
    _assert_same(on, off)


def test_backward_memo_belongs_to_one_graph(monkeypatch):
    """Two forwards of different parameters, the same cotangent: each graph's own gradients."""
    import diff_gaussian_rasterization as dgr

    def run(memo):
        monkeypatch.setattr(dgr, "_BWD_MEMO", memo)
        calls = _counting(monkeypatch)
        model_a, cam, gt, v, *_ = _scene()
        model_b = _scene()[0]
        with torch.no_grad():
            model_b._xyz.add_(0.01)
            model_b._opacity.sub_(0.3)
        ra = _render(model_a, cam)["render"] - gt
        rb = _render(model_b, cam)["render"] - gt
        ra.backward(v)
        rb.backward(v.clone())
        return _leaf_grads(model_a), _leaf_grads(model_b), len(calls)

    a_on, b_on, n_on = run(True)
    a_off, b_off, n_off = run(False)
    assert n_on == 2 and n_off == 2
    _assert_same(a_on, a_off)
    _assert_same(b_on, b_off)
    assert not torch.equal(a_on[0], b_on[0])


def test_backward_memo_on_leaf_inputs(monkeypatch):
    """The rasterizer called on leaves, no activation nodes between: AccumulateGrad receives the memo's tensors on the
    second call.  The accumulated gradient is exactly twice the single call's and the memo's tensors are untouched."""
    import diff_gaussian_rasterization as dgr
    from scenes import activated, gpu_settings
    monkeypatch.setattr(dgr, "_BWD_MEMO", True)
    calls = _counting(monkeypatch)
    model, cam, _, v, _, d, _ = _scene()
    a = {k: t.to(DEV).requires_grad_(True) for k, t in activated(model).items()}
    a["means2D"] = torch.zeros_like(a["means3D"], requires_grad=True)
    img, _, depth = dgr.GaussianRasterizer(gpu_settings(cam, model.active_sh_degree))(
        means3D=a["means3D"], means2D=a["means2D"], shs=a["shs"], opacities=a["opacities"], scales=a["scales"],
        rotations=a["rotations"])
    ctx = img.grad_fn
    torch.autograd.backward([img, depth], [v, d], retain_graph=True)
    single = {k: t.grad.detach().clone() for k, t in a.items()}
    held = [t for t in ctx.bw_memo[2] if t is not None]
    copies = [t.clone() for t in held]
    assert len(held) == 6 and all(float(t.abs().max()) > 0 for t in held)
    for t in a.values():
        assert all(t.grad.data_ptr() != h.data_ptr() for h in held), "a leaf's .grad is one of the memo's tensors"
    torch.autograd.backward([img, depth], [v.clone(), d.clone()], retain_graph=True)
    assert len(calls) == 1
    for k, t in a.items():
        assert torch.equal(t.grad, 2 * single[k]), k
    for h, c in zip(held, copies):
        assert torch.equal(h, c)
    assert all(x is y for x, y in zip(held, [t for t in ctx.bw_memo[2] if t is not None]))
