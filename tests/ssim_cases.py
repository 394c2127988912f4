"""Inputs, float64 oracle and metric of the direct SSIM-operator tests (tests/test_gpu_ssim_operator.py on the GPU,
tests/test_oracle_ssim_cases.py as their conditioning guard on the CPU).  No GPU here.

Why gapped inputs: the L1 half of the image operator is the diagonal d1^2 = a^2 / (4 (|x - y| + 1e-6)), which spikes
wherever a pixel of x = m clamp01(R) lies close to the ground truth y.  On random inputs those spikes are 1000 times
the SSIM half S^T c2^2 S, they amplify the float32 rounding of |x - y| in the reference itself, and a global max-norm
bar is then pinned by the pixels that say least about the two convolutions.  `gapped_case` keeps |x - y| >= 0.02 at
every pixel (asserted, in float64), so the float32 oracle stays a factor of 4 inside every bar the GPU tests apply
(tests/test_oracle_ssim_cases.py), and `tile_rel` measures every 32x16 output tile of the kernel against its own
magnitude, so a wrong partial tile or halo cannot hide behind a large value elsewhere in the image.
"""
import functools

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from oracle import ssim_ref

TILE_W, TILE_H = 32, 16  # csrc/ssim.hip SS_TW, SS_TH

# Bars (tests/test_gpu_ssim.py's, applied under tile_rel against the float64 oracle).
BAR_RES = 1e-5   # r1, r2, loss
BAR_OP = 1e-4    # J^T b seed, image-space operator

# (H, W): the smallest shapes at which the tile and halo logic can go wrong.
SMALL = [(1, 1), (1, 40), (40, 1), (3, 5), (10, 11), (11, 10)]   # window larger than the image, one or both axes
TILE_EDGE = [(16, 32), (17, 33), (15, 31), (33, 65)]             # one tile, one past, one short; 3x3 tiles, 1-px last
MANY_PARTIALS = [(144, 320)]                                     # 9 x 10 x 3 = 270 partials > 256 threads
SHAPES = SMALL + TILE_EDGE + MANY_PARTIALS
MASKS = ["none", "binary", "levels"]

PURE_SSIM = [(H, W, mk, 1.0) for (H, W) in SHAPES for mk in MASKS]
PURE_L1 = [(H, W, "levels", 0.0) for (H, W) in SHAPES]
MIXED = [(H, W, mk, 0.2) for (H, W) in TILE_EDGE for mk in MASKS]
GATE = [("none", 0.2), ("binary", 0.2), ("none", 1.0)]           # clamp_gate_case(mask_kind), lambda
XEQ = [(17, 33, "levels"), (33, 65, "none"), (3, 5, "binary")]    # xeq_case(H, W, mask_kind)
MEAN_SHAPES = [(1, 1), (5, 7), (16, 32), (17, 33)]
MEAN_LEAD = [(1,), (2,), (3,), (2, 3)]                            # C = 1, 2, 3 and a (2, 3, H, W) batch


# Cases whose first seed fails the CPU guard: the 1x1 corner tile of 17x33 held a seed value 8.6e-4 of the image's
# max, under tile_rel's floor, where float32 rounding of 6e-8 of the max reads as 6e-5.
RESEED = {(17, 33, "binary"): 1}


def case_seed(H, W, mask_kind):
    return 1000 * H + W + 100000 * MASKS.index(mask_kind) + 1000000 * RESEED.get((H, W, mask_kind), 0)


def _mask(H, W, g, mask_kind):
    pick = torch.rand(1, H, W, generator=g)
    if mask_kind == "none":
        m = torch.ones(1, H, W)
    elif mask_kind == "binary":
        m = (pick < 0.7).float()
    elif mask_kind == "levels":
        m = torch.where(pick < 0.2, torch.zeros(()), torch.where(pick < 0.5, torch.full((), 0.5), torch.ones(())))
    else:
        raise ValueError(mask_kind)
    m[0, 0, 0] = 1.0  # never an all-zero mask (a 1x1 image would test nothing)
    return m


def assert_gap(R, gt, m, gap=1e-3):
    """|m clamp01(R) - gt| >= gap at every pixel, in float64 (where m == 0, x = 0 and gt >= gap)."""
    x = m.double() * R.double().clamp(0, 1)
    d = (x - gt.double()).abs().min().item()
    assert d >= gap, f"gap {d:.3e} < {gap:.1e}"
    return d


def gapped_case(H, W, seed, mask_kind):
    """R, gt, m, jv (float32, CPU) with x = m clamp01(R) at least 0.02 from gt everywhere.

    x is built first: gt in [0.1, 0.9], x = gt +- u with u in [0.02, 0.27], held inside [0, m] (the range m clamp01(.)
    can reach) by taking the other sign or the nearer end of the range, which never narrows the gap below u.  A fifth
    of the pixels sit at x = 0 with R < 0 and a fifth at x = m with R > 1, so the clamp gate is mixed.  Only then is
    R = x / m formed (exact: m is 0.5 or 1).  Where m == 0, x = 0, R is arbitrary and gt >= 0.1.

    Three choices keep the float32 oracle inside a quarter of the bars (its r2 error is the rounding of the
    variances K*(x x) - (K*x)^2 over 121 float32 taps, about 5e-6 of S on uniform images, divided by sqrt(1 - S)):
    gt = 0.1 + 0.8 rand^3 is dark with bright outliers (variance large against the squared mean), the sign moves x
    towards mid-grey (+ below 0.5, - above) and the out-of-range fifths are independent of gt (both lower the
    correlation of x with gt, so S stays away from 1)."""
    g = torch.Generator().manual_seed(seed)
    gt = 0.1 + 0.8 * torch.rand(3, H, W, generator=g) ** 3
    u = 0.02 + 0.25 * torch.rand(3, H, W, generator=g)
    plus = gt < 0.5
    m = _mask(H, W, g, mask_kind)
    mm = m.expand(3, H, W)
    plus = plus & (gt + u <= mm)
    x = torch.minimum(torch.where(plus, gt + u, gt - u).clamp(min=0.0), mm)
    side = torch.rand(3, H, W, generator=g)
    over = 0.01 + 0.3 * torch.rand(3, H, W, generator=g)
    free = torch.rand(3, H, W, generator=g) * 1.2 - 0.1
    low = side < 0.2
    high = (side > 0.8) & ((mm - gt).abs() >= 0.02)
    x = torch.where(low, torch.zeros(()), torch.where(high, mm, x))
    R = x / mm.clamp(min=0.5)
    R = torch.where(low, -over, torch.where(high, 1.0 + over, R))
    R = torch.where(mm > 0, R, free)
    jv = torch.randn(3, H, W, generator=g)
    assert_gap(R, gt, m, 0.02 - 1e-6)
    assert torch.equal(m * R.clamp(0, 1), torch.where(mm > 0, x, torch.zeros(())))
    if H * W >= 64:
        assert (R < 0).any() and (R > 1).any() and ((R >= 0) & (R <= 1)).any()
    return R, gt, m, jv


GATE_HW = (33, 65)


def clamp_gate_case(mask_kind):
    """A 33x65 gapped case whose R takes the exact values 0.0, 1.0, -0.0, nextafter(0, -1) and nextafter(1, 2) on the
    first and last row and column of every 32x16 tile (so on every tile corner).  clamp01 sends them to 0 or 1, at
    least 0.1 from gt; the gate M = m 1[0 <= R <= 1] is open for the first three and closed for the last two."""
    assert mask_kind in ("none", "binary")  # m = 0.5 would put x = 0.5 where gt may be
    H, W = GATE_HW
    R, gt, m, jv = gapped_case(H, W, 777 + MASKS.index(mask_kind), mask_kind)
    vals = torch.tensor([0.0, 1.0, -0.0, np.nextafter(np.float32(0), np.float32(-1)),
                         np.nextafter(np.float32(1), np.float32(2))], dtype=torch.float32)
    assert vals[3] < 0 and vals[4] > 1
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    edge = ((yy % TILE_H == 0) | (yy % TILE_H == TILE_H - 1) | (xx % TILE_W == 0) | (xx % TILE_W == TILE_W - 1))
    edge = edge | (yy == H - 1) | (xx == W - 1)
    cc = torch.arange(3).view(3, 1, 1)
    which = (yy + 2 * xx + cc) % 5
    R = torch.where(edge.expand(3, H, W), vals[which], R)
    assert_gap(R, gt, m, 0.02 - 1e-6)
    return R, gt, m, jv


def xeq_case(H, W, mask_kind):
    """x == gt bit for bit: gt = m clamp01(R) in float32, R random in [-0.1, 1.1]."""
    g = torch.Generator().manual_seed(4242 + case_seed(H, W, mask_kind))
    R = torch.rand(3, H, W, generator=g) * 1.2 - 0.1
    m = _mask(H, W, g, mask_kind)
    jv = torch.randn(3, H, W, generator=g)
    return R, m * R.clamp(0, 1), m, jv


def oracle(R, gt, m, jv, lam, dtype):
    """r1, r2, loss, seed = J_R^T b, N jv = J_R^T J_R jv of oracle.ssim_ref in `dtype` (numpy float64 arrays; loss a
    float).  The seed is autograd of -0.5 ||r||^2, N jv is forward-AD through clamp, mask, l1 and SSIM and then
    autograd.  In float64 the window is the float32 taps promoted (ssim_per_pixel's type_as): the kernel's taps."""
    R, gt, m, jv = (t.to(dtype) for t in (R, gt, m, jv))

    def res(Rt):
        return ssim_ref.ssim_residuals(Rt.clamp(0, 1) * m, gt, lam)

    with fwAD.dual_level():
        d1, d2 = res(fwAD.make_dual(R, jv))
        t1, t2 = fwAD.unpack_dual(d1).tangent, fwAD.unpack_dual(d2).tangent
    t1 = torch.zeros_like(R) if t1 is None else t1
    t2 = torch.zeros_like(R) if t2 is None else t2
    Rr = R.clone().requires_grad_(True)
    r1, r2 = res(Rr)
    half = 0.5 * ((r1 * r1).sum() + (r2 * r2).sum())
    seed = -torch.autograd.grad(half, Rr, retain_graph=True)[0]
    njv = torch.autograd.grad((r1 * t1).sum() + (r2 * t2).sum(), Rr)[0]
    loss = ((r1.detach().double() ** 2).sum() + (r2.detach().double() ** 2).sum()).item()
    f = lambda t: t.detach().double().numpy()
    return f(r1), f(r2), loss, f(seed), f(njv)


@functools.lru_cache(maxsize=None)
def gapped(H, W, mask_kind):
    return gapped_case(H, W, case_seed(H, W, mask_kind), mask_kind)


@functools.lru_cache(maxsize=None)
def gapped_oracle(H, W, mask_kind, lam, dtype=torch.float64):
    """The oracle of gapped(H, W, mask_kind), computed once and shared (do not write to the arrays)."""
    out = oracle(*gapped(H, W, mask_kind), lam, dtype)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def tile_rel(a, b):
    """max over the kernel's 32x16 output tiles and channels of max|a - b| on the tile over
    max(max|b| on the tile, 1e-3 max|b| globally)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    H, W = b.shape[-2:]
    a, b = a.reshape(-1, H, W), b.reshape(-1, H, W)
    d, mag = np.abs(a - b), np.abs(b)
    floor = 1e-3 * mag.max()
    if floor == 0.0:
        return 0.0 if d.max() == 0.0 else float("inf")
    worst = 0.0
    for y0 in range(0, H, TILE_H):
        for x0 in range(0, W, TILE_W):
            sl = (slice(None), slice(y0, y0 + TILE_H), slice(x0, x0 + TILE_W))
            worst = max(worst, float((d[sl].max(axis=(1, 2)) / np.maximum(mag[sl].max(axis=(1, 2)), floor)).max()))
    return worst


def mean_case(lead, H, W):
    """Independent x, y in [0, 1] of shape lead + (H, W) for gslm.loss.ssim.  (With y close to x, as in
    test_ssim_loss_matches_oracle, the gradient is a difference of terms of order 1 / C2 and the float32 oracle of a
    1x1 image is 7e-5 of the gradient's max from the float64 one; independent images keep it under 2e-6.)"""
    shape = tuple(lead) + (H, W)
    g = torch.Generator().manual_seed(31 * sum(shape) + len(shape))
    x = torch.rand(shape, generator=g)
    y = torch.rand(shape, generator=g)
    return x, y


MEAN_UPSTREAM = -0.37  # the loss is MEAN_UPSTREAM * ssim: an upstream gradient other than 1


def mean_oracle(x, y, dtype):
    """mean SSIM and the gradient of MEAN_UPSTREAM * mean in `dtype`; a leading batch folds into channel planes."""
    H, W = x.shape[-2:]
    xo = x.to(dtype).clone().requires_grad_(True)
    s = ssim_ref.ssim_per_pixel(xo.reshape(1, -1, H, W), y.to(dtype).reshape(1, -1, H, W)).mean()
    (MEAN_UPSTREAM * s).backward()
    return s.item(), xo.grad.double().numpy()
