"""The SSIM kernels of csrc/ssim.hip against the float64 oracle, where the L1 term cannot mask their errors.

tests/test_gpu_ssim.py compares whole images by max|a - b| / max|b| at lambda_dssim = 0.2 on random inputs.  There
the L1 diagonal d1^2 = a^2 / (4 (|x - y| + 1e-6)) carries all of max|N jv| (4.8e-2 against a peak of 2.9e-5 and a median
of 5.6e-7 for the SSIM half S^T c2^2 S), so its 1e-4 bar is 16 % of the peak of the half that runs the two
convolutions.  Here:

* inputs keep |x - y| >= 0.02 everywhere (ssim_cases.gapped_case), so the reference is well conditioned: the float32
  oracle is within a quarter of every bar below on every case (tests/test_oracle_ssim_cases.py, CPU);
* lambda_dssim = 1 removes the L1 half and isolates k_ssim_eval's convolution, k_ssim_fwd and k_ssim_bwd;
  lambda_dssim = 0 removes the SSIM half; N_lambda = (1 - lambda) N_0 + lambda N_1, so a failure names one half;
* the metric is tile-local (ssim_cases.tile_rel): each 32x16 output tile against its own magnitude;
* shapes: images smaller than the 11-tap window in one or both axes, one tile exactly, one pixel past and short of it,
  3x3 tiles with 1-pixel last tiles, and 270 block partials into the 256-thread final reduction.

Bars (tests/test_gpu_ssim.py's): residuals and loss 1e-5, seed and operator 1e-4, under tile_rel against float64.
Worst GPU-vs-float64 values measured on the MI355X over all cases of this file (tile_rel; loss relative):
  r1 1.2e-7, r2 8.0e-7 (144x320, no mask), loss 2.7e-7, seed 1.3e-6 (17x33), N jv 2.5e-6 (1x40);
  linearity 3.9e-7 and symmetry 3.2e-7 at lambda_dssim = 1; x == gt: seed and N jv exactly 0;
  gslm.loss.ssim: value 3.6e-7, gradient 1.4e-6 of its max.
"""
import numpy as np
import pytest
import torch

import ssim_cases as sc
from margins import record
from oracle import ssim_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _np(t):
    return t.detach().cpu().double().numpy()


def _nan(H, W):
    return torch.full((3, H, W), float("nan"), device=DEV)


class View:
    """One view's device inputs and SSIM state."""

    def __init__(self, R, gt, m, H, W, mask_kind):
        from gslm import _lib
        self.H, self.W = H, W
        self.R, self.gt = R.to(DEV).contiguous(), gt.to(DEV).contiguous()
        self.m = None if mask_kind == "none" else m.to(DEV).contiguous()  # "none" takes the NULL-mask path
        self.st = _lib.u8(_lib.lib.gslm_ssim_state_bytes(H, W), DEV)

    def residual(self, lam, r1=True, r2=True, seed=True, loss=None, accumulate=0):
        from gslm import _lib
        H, W = self.H, self.W
        o1, o2, sd = (_nan(H, W) if on else None for on in (r1, r2, seed))
        if loss is None:
            loss = torch.full((), float("nan"), dtype=torch.float64, device=DEV)
        _lib.check(_lib.lib.gslm_ssim_residual(H, W, self.R.data_ptr(), self.gt.data_ptr(), _lib.ptr(self.m), lam,
                                               self.st.data_ptr(), self.st.numel(), _lib.ptr(o1), _lib.ptr(o2),
                                               _lib.ptr(sd), loss.data_ptr(), accumulate, _lib.stream_handle()))
        torch.cuda.synchronize()
        return o1, o2, sd, loss

    def normal(self, a):
        from gslm import _lib
        u = _nan(self.H, self.W)
        _lib.check(_lib.lib.gslm_ssim_normal(self.H, self.W, self.gt.data_ptr(), self.st.data_ptr(),
                                             a.data_ptr(), u.data_ptr(), _lib.stream_handle()))
        torch.cuda.synchronize()
        return u


def _gapped_view(H, W, mask_kind):
    R, gt, m, jv = sc.gapped(H, W, mask_kind)
    return View(R, gt, m, H, W, mask_kind), jv.to(DEV)


def _check_against_oracle(name, view, jv, lam, ref, quantities):
    r1, r2, loss, seed, njv = ref
    o1, o2, sd, lg = view.residual(lam)
    u = view.normal(jv)
    got = {"r1": (o1, r1, sc.BAR_RES), "r2": (o2, r2, sc.BAR_RES), "seed": (sd, seed, sc.BAR_OP),
           "Njv": (u, njv, sc.BAR_OP)}
    worst = {q: record(name, q, sc.tile_rel(_np(got[q][0]), got[q][1]), got[q][2]) for q in quantities}
    lerr = record(name, "loss", abs(lg.item() - loss) / loss, sc.BAR_RES)
    for q in quantities:
        assert worst[q] < got[q][2], (q, worst[q])
    assert lerr <= sc.BAR_RES
    return o1, o2, sd, u


@pytest.mark.parametrize("H,W,mask_kind,lam", sc.PURE_SSIM)
def test_pure_ssim_operator(H, W, mask_kind, lam):
    """lambda_dssim = 1: r1 is exactly 0 and r2, the loss, the seed and N jv are the SSIM half alone."""
    view, jv = _gapped_view(H, W, mask_kind)
    o1, _, _, _ = _check_against_oracle(f"pure_ssim[{H}x{W}-{mask_kind}]", view, jv, lam,
                                        sc.gapped_oracle(H, W, mask_kind, lam), ("r2", "seed", "Njv"))
    assert not o1.cpu().numpy().any()


@pytest.mark.parametrize("H,W,mask_kind,lam", sc.PURE_L1)
def test_pure_l1_operator(H, W, mask_kind, lam):
    """lambda_dssim = 0: r2 is exactly 0 and the seed and N jv are the L1 diagonal alone."""
    view, jv = _gapped_view(H, W, mask_kind)
    _, o2, _, _ = _check_against_oracle(f"pure_l1[{H}x{W}-{mask_kind}]", view, jv, lam,
                                        sc.gapped_oracle(H, W, mask_kind, lam), ("r1", "seed", "Njv"))
    assert not o2.cpu().numpy().any()


@pytest.mark.parametrize("H,W,mask_kind,lam", sc.MIXED)
def test_mixed_operator_at_tile_edges(H, W, mask_kind, lam):
    view, jv = _gapped_view(H, W, mask_kind)
    _check_against_oracle(f"mixed[{H}x{W}-{mask_kind}]", view, jv, lam, sc.gapped_oracle(H, W, mask_kind, lam),
                          ("r1", "r2", "seed", "Njv"))


@pytest.mark.parametrize("mask_kind,lam", sc.GATE)
def test_clamp_gate_at_exact_bounds(mask_kind, lam):
    """R = 0.0, 1.0 and -0.0 pass the gradient (torch.clamp's inclusive bounds, the kernel's gate plane);
    nextafter(0, -1) (a negative denormal) and nextafter(1, 2) do not, on every tile corner of a 33x65 image."""
    H, W = sc.GATE_HW
    R, gt, m, jv = sc.clamp_gate_case(mask_kind)
    view = View(R, gt, m, H, W, mask_kind)
    _, _, sd, u = _check_against_oracle(f"clamp_gate[{mask_kind}-{lam}]", view, jv.to(DEV), lam,
                                        sc.oracle(R, gt, m, jv, lam, torch.float64), ("seed", "Njv"))
    closed = ((R < 0) | (R > 1) | (m == 0).expand_as(R)).numpy()
    assert not _np(sd)[closed].any() and not _np(u)[closed].any()
    opened = ((R == 0) | (R == 1)) & (m > 0).expand_as(R)
    assert opened.any() and _np(sd)[opened.numpy()].all()


@pytest.mark.parametrize("H,W,mask_kind", sc.XEQ)
def test_x_equal_gt(H, W, mask_kind):
    """x == gt bit for bit: A == C and B == D in k_ssim_eval, so S = 1, d1 = c2 = 0, r = (a, b) sqrt(1e-6) and the
    seed and N jv vanish (measured: exactly 0 on the MI355X)."""
    lam = 0.2
    R, gt, m, jv = sc.xeq_case(H, W, mask_kind)
    view = View(R, gt, m, H, W, mask_kind)
    o1, o2, sd, lg = view.residual(lam)
    u = view.normal(jv.to(DEV))
    a, b = ssim_ref.image_weights(H, W, lam)
    assert np.abs(_np(o1) - a * 1e-3).max() <= 1e-6 * a * 1e-3
    assert np.abs(_np(o2) - b * 1e-3).max() <= 1e-6 * b * 1e-3
    want = 1e-6 * (a * a + b * b) * 3 * H * W
    assert abs(lg.item() - want) <= 1e-5 * want
    name = f"x_equal_gt[{H}x{W}-{mask_kind}]"
    bound = 1e-4 * a * a / 2
    assert record(name, "|seed|", np.abs(_np(sd)).max(), bound) < bound
    assert record(name, "|Njv|", np.abs(_np(u)).max(), bound) < bound


def test_loss_accumulates_over_views():
    """Two views into one loss_dev, accumulate = 0 then 1, from a poisoned loss_dev: the float64 sum.  accumulate = 0
    on both leaves the second loss alone."""
    H, W, lam = 17, 33, 0.2
    v1, _ = _gapped_view(H, W, "levels")
    v2, _ = _gapped_view(H, W, "none")
    l1, l2 = sc.gapped_oracle(H, W, "levels", lam)[2], sc.gapped_oracle(H, W, "none", lam)[2]
    assert abs(l1 - l2) > 1e-3 * l2  # two different views
    loss = torch.full((), float("nan"), dtype=torch.float64, device=DEV)
    v1.residual(lam, loss=loss, accumulate=0)
    assert abs(loss.item() - l1) <= 1e-5 * l1
    v2.residual(lam, loss=loss, accumulate=1)
    assert abs(loss.item() - (l1 + l2)) <= 1e-5 * (l1 + l2)
    loss.fill_(float("nan"))
    v1.residual(lam, loss=loss, accumulate=0)
    v2.residual(lam, loss=loss, accumulate=0)
    assert abs(loss.item() - l2) <= 1e-5 * l2


@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_normal_reuses_its_state(lam):
    """k_ssim_fwd overwrites the plane gslm_ssim_residual filled for the seed: N(jv) is bit-identical before and after
    N(other), and N is linear: N(2a + b) = 2 N(a) + N(b) to 1e-5 of its max."""
    H, W = 33, 65
    view, jv = _gapped_view(H, W, "levels")
    view.residual(lam)
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(3, H, W, generator=g).to(DEV), torch.randn(3, H, W, generator=g).to(DEV)
    first = view.normal(jv)
    na, nb = view.normal(a), view.normal(b)
    assert torch.equal(view.normal(jv), first)
    comb = _np(view.normal(2 * a + b))
    want = 2 * _np(na) + _np(nb)
    err = record(f"normal_linear[{lam}]", "N(2a+b)", np.abs(comb - want).max() / np.abs(comb).max(), 1e-5)
    assert err < 1e-5


def test_pure_ssim_operator_is_symmetric_and_psd():
    """<a, N a> >= 0 and <a, N b> = <N a, b> at lambda_dssim = 1, without the L1 diagonal to swamp them (the bar of
    test_ssim_normal_operator: 1e-4 of the larger side)."""
    H, W = 33, 65
    view, _ = _gapped_view(H, W, "levels")
    view.residual(1.0)
    g = torch.Generator().manual_seed(6)
    a, b = torch.randn(3, H, W, generator=g).to(DEV), torch.randn(3, H, W, generator=g).to(DEV)
    na, nb = view.normal(a).double(), view.normal(b).double()
    assert (a.double() * na).sum().item() > 0 and (b.double() * nb).sum().item() > 0
    lhs, rhs = (a.double() * nb).sum().item(), (na * b.double()).sum().item()
    err = record("pure_ssim_symmetry", "<a,Nb>-<Na,b>", abs(lhs - rhs) / max(abs(lhs), abs(rhs)), 1e-4)
    assert err <= 1e-4


def test_optional_outputs_do_not_change_the_others():
    H, W, lam = 17, 33, 0.2
    view, jv = _gapped_view(H, W, "binary")
    full = view.residual(lam)
    nfull = view.normal(jv)
    for skip in range(3):
        on = [i != skip for i in range(3)]
        part = view.residual(lam, r1=on[0], r2=on[1], seed=on[2])
        assert part[skip] is None
        for i in range(3):
            if on[i]:
                assert torch.equal(part[i], full[i])
        assert torch.equal(part[3], full[3])
        assert torch.equal(view.normal(jv), nfull)  # the state does not depend on which outputs were asked for


def test_error_returns_launch_nothing():
    from gslm import _lib
    H, W = 4, 5
    R, gt, m, jv = sc.gapped_case(H, W, 1, "none")
    Rg, gtg = R.to(DEV), gt.to(DEV)
    st = _lib.u8(_lib.lib.gslm_ssim_state_bytes(H, W), DEV)
    seed = torch.full((3, H, W), 7.0, device=DEV)
    loss = torch.full((), 123.0, dtype=torch.float64, device=DEV)

    def call(H=H, W=W, gt=gtg.data_ptr(), lam=0.2, nbytes=st.numel()):
        return _lib.lib.gslm_ssim_residual(H, W, Rg.data_ptr(), gt, None, lam, st.data_ptr(), nbytes, None, None,
                                           seed.data_ptr(), loss.data_ptr(), 0, _lib.stream_handle())

    bad = [dict(H=0), dict(W=0), dict(nbytes=st.numel() - 1), dict(lam=-0.1), dict(lam=1.1), dict(lam=float("nan")),
           dict(gt=None)]
    for kw in bad:
        with pytest.raises(_lib.GslmError):
            _lib.check(call(**kw), "gslm_ssim_residual")
    u = torch.full((3, H, W), 7.0, device=DEV)
    for kw in (dict(H=0), dict(gt=None), dict(jv=None)):
        args = dict(H=H, gt=gtg.data_ptr(), jv=seed.data_ptr())
        args.update(kw)
        with pytest.raises(_lib.GslmError):
            _lib.check(_lib.lib.gslm_ssim_normal(args["H"], W, args["gt"], st.data_ptr(), args["jv"], u.data_ptr(),
                                                 _lib.stream_handle()), "gslm_ssim_normal")
    torch.cuda.synchronize()
    assert (seed == 7.0).all() and (u == 7.0).all() and loss.item() == 123.0
    _lib.check(call(), "gslm_ssim_residual")  # the same arguments, valid, do run
    torch.cuda.synchronize()
    assert torch.isfinite(seed).all() and loss.item() != 123.0


# ---- gslm.loss.ssim: the mean path (k_ssim_mean, k_ssim_mean_bwd)

@pytest.mark.parametrize("lead", sc.MEAN_LEAD)
@pytest.mark.parametrize("H,W", sc.MEAN_SHAPES)
def test_mean_ssim_value_and_gradient(lead, H, W):
    """C = 1, 2, 3 and a (2, 3, H, W) batch, on images smaller than the window and around one tile; the bars of
    test_ssim_loss_matches_oracle (value 1e-6, gradient 1e-5 of its max), with an upstream gradient other than 1."""
    from gslm.loss import ssim
    x, y = sc.mean_case(lead, H, W)
    s64, g64 = sc.mean_oracle(x, y, torch.float64)
    xg = x.to(DEV).requires_grad_(True)
    s = ssim(xg, y.to(DEV))
    (sc.MEAN_UPSTREAM * s).backward()
    name = f"mean_ssim[{'x'.join(map(str, lead))}x{H}x{W}]"
    assert s.dtype == torch.float32 and s.shape == ()
    assert xg.grad.shape == x.shape and xg.grad.dtype == torch.float32
    assert record(name, "value", abs(s.item() - s64), 1e-6) < 1e-6
    gerr = record(name, "grad", np.abs(_np(xg.grad) - g64).max() / np.abs(g64).max(), 1e-5)
    assert gerr <= 1e-5


def test_mean_ssim_input_dtype_and_layout():
    """A float64 input and a non-contiguous (sliced) input give the float32 contiguous value, and a gradient of the
    input's dtype and shape."""
    from gslm.loss import ssim
    H, W = 17, 33
    x, y = sc.mean_case((3,), H, W)
    yg = y.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    s = ssim(xg, yg)
    (sc.MEAN_UPSTREAM * s).backward()
    xd = x.double().to(DEV).requires_grad_(True)
    sd = ssim(xd, yg.double())
    (sc.MEAN_UPSTREAM * sd).backward()
    assert sd.item() == s.item()
    assert xd.grad.dtype == torch.float64 and xd.grad.shape == x.shape
    assert torch.equal(xd.grad.float(), xg.grad)
    wide = torch.zeros(3, H, 2 * W)
    wide[..., ::2] = x
    xs = wide.to(DEV)[..., ::2].requires_grad_(True)
    assert not xs.is_contiguous() and torch.equal(xs.detach(), xg.detach())
    ywide = torch.zeros(3, 2 * H, W)
    ywide[:, ::2] = y
    ys = ywide.to(DEV)[:, ::2]
    assert not ys.is_contiguous()
    ss = ssim(xs, ys)
    (sc.MEAN_UPSTREAM * ss).backward()
    assert ss.item() == s.item()
    assert xs.grad.dtype == torch.float32 and xs.grad.shape == x.shape
    assert torch.equal(xs.grad, xg.grad)


@pytest.mark.parametrize("lead,H,W", [((3,), 17, 33), ((1,), 1, 1), ((2, 3), 5, 7)])
def test_mean_ssim_of_identical_images_is_one(lead, H, W):
    from gslm.loss import ssim
    x, _ = sc.mean_case(lead, H, W)
    xg = x.to(DEV)
    assert abs(ssim(xg, xg.clone()).item() - 1.0) <= 1e-6


def test_mean_ssim_rejects_cpu_tensors_and_mismatched_shapes():
    from gslm.loss import ssim
    x, y = sc.mean_case((3,), 5, 7)
    with pytest.raises(RuntimeError):
        ssim(x, y)
    with pytest.raises(ValueError):
        ssim(x.to(DEV), y[:, :4].to(DEV))
    with pytest.raises(ValueError):
        ssim(x.to(DEV), y[:2].to(DEV))
