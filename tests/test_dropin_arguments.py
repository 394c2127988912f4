"""The drop-in rasterizer's argument checks (diff_gaussian_rasterization/__init__.py), on CPU tensors only.

Every refusal here is raised before anything reaches the library, so these run without a GPU: forward_buffers is
replaced by a function that fails the test, and no tensor is ever on a device.
  * a float64 or float16 tensor in any argument: TypeError (whatever device the tensors are on);
  * float32 inputs that are not on a CUDA device: ValueError naming means3D;
  * GaussianRasterizer.forward's two "exactly one of" checks;
  * _same_cotangent, the memo's key comparison, on its five kinds of pairs.
"""
import pytest
import torch

P, K, H, W = 7, 4, 5, 6
ARGS = ("means3D", "means2D", "shs", "dc", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")


def _settings():
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=1, campos=torch.zeros(3), prefiltered=False,
        debug=False, antialiasing=False)


def _inputs(form):
    """CPU float32 inputs of one of the call forms that hold `arg`."""
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g)
    out = dict(means3D=r(P, 3), means2D=torch.zeros(P, 3), opacities=torch.rand(P, 1, generator=g))
    if form == "precomp":
        out.update(colors_precomp=torch.rand(P, 3, generator=g), cov3D_precomp=r(P, 6))
    else:
        out.update(scales=torch.rand(P, 3, generator=g), rotations=r(P, 4))
        if form == "dc_split":
            out.update(dc=r(P, 1, 3), shs=r(P, K - 1, 3))
        else:
            out.update(shs=r(P, K, 3))
    return out


def _form_of(arg):
    return {"dc": "dc_split", "colors_precomp": "precomp", "cov3D_precomp": "precomp"}.get(arg, "plain")


@pytest.fixture
def no_library(monkeypatch):
    import diff_gaussian_rasterization as dgr

    def reached(*_a, **_k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(dgr, "forward_buffers", reached)
    return dgr


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16], ids=["float64", "float16"])
@pytest.mark.parametrize("arg", ARGS)
def test_wrong_dtype_is_a_type_error(arg, dtype, no_library):
    inp = _inputs(_form_of(arg))
    inp[arg] = inp[arg].to(dtype)
    with pytest.raises(TypeError, match="float32") as e:
        no_library.GaussianRasterizer(_settings())(**inp)
    assert str(dtype) in str(e.value)


@pytest.mark.parametrize("form", ["plain", "dc_split", "precomp"])
def test_cpu_inputs_are_a_value_error(form, no_library):
    with pytest.raises(ValueError, match="means3D"):
        no_library.GaussianRasterizer(_settings())(**_inputs(form))
    with pytest.raises(ValueError, match="means3D"), torch.no_grad():
        no_library.GaussianRasterizer(_settings())(**_inputs(form))


def test_cpu_inputs_that_require_grad_are_a_value_error(no_library):
    inp = {k: v.requires_grad_(True) for k, v in _inputs("plain").items()}
    with pytest.raises(ValueError, match="means3D"):
        no_library.GaussianRasterizer(_settings())(**inp)


def test_exactly_one_colour_source(no_library):
    rast = no_library.GaussianRasterizer(_settings())
    inp = _inputs("plain")
    neither = {k: v for k, v in inp.items() if k != "shs"}
    with pytest.raises(Exception, match="one of either SHs or precomputed colors"):
        rast(**neither)
    with pytest.raises(Exception, match="one of either SHs or precomputed colors"):
        rast(colors_precomp=torch.rand(P, 3), **inp)
    # dc= counts as SH
    with pytest.raises(Exception, match="one of either SHs or precomputed colors"):
        rast(colors_precomp=torch.rand(P, 3), dc=torch.rand(P, 1, 3), **neither)


def test_exactly_one_covariance_source(no_library):
    rast = no_library.GaussianRasterizer(_settings())
    inp = _inputs("plain")
    msg = "one of either scale/rotation pair or precomputed 3D covariance"
    for drop in (("scales",), ("rotations",), ("scales", "rotations")):
        with pytest.raises(Exception, match=msg):
            rast(**{k: v for k, v in inp.items() if k not in drop})
    with pytest.raises(Exception, match=msg):
        rast(cov3D_precomp=torch.rand(P, 6), **inp)
    with pytest.raises(Exception, match=msg):
        rast(cov3D_precomp=torch.rand(P, 6), **{k: v for k, v in inp.items() if k != "rotations"})


def test_same_cotangent():
    from diff_gaussian_rasterization import _same_cotangent
    g = torch.Generator().manual_seed(5)
    a = torch.randn(3, H, W, generator=g)
    assert _same_cotangent(None, None) is True
    assert _same_cotangent(None, a) is False
    assert _same_cotangent(a, None) is False
    # a shape mismatch with the same elements, and one that broadcasts
    assert _same_cotangent(a, a.reshape(3, W, H)) is False
    assert _same_cotangent(a[:1], a[:1].expand(3, H, W)) is False
    assert _same_cotangent(torch.ones(1, H, W), torch.ones(3, H, W)) is False
    # a dtype mismatch with equal values
    z = torch.zeros(3, H, W)
    assert _same_cotangent(z, z.double()) is False
    assert _same_cotangent(z, z.half()) is False
    # equal values, different strides: permuted, stride 0, and a slice of a larger tensor
    hwc = a.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert hwc.stride() != a.stride() and _same_cotangent(a, hwc) is True
    one = torch.ones((), dtype=torch.float32).expand(3, H, W)
    assert one.stride() == (0, 0, 0) and _same_cotangent(one, torch.ones(3, H, W)) is True
    wide = torch.randn(3, H, W + 2, generator=g)
    assert _same_cotangent(wide[:, :, 1:-1], wide[:, :, 1:-1].clone()) is True
    # one element off
    b = a.clone()
    b[2, H - 1, W - 1] += 1e-3
    assert _same_cotangent(a, b) is False
    assert _same_cotangent(a, a.clone()) is True
