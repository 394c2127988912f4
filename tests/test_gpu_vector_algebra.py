"""The device CG vector algebra (csrc/cg.hip) through the C ABI, against float64 references built from the inputs.

Exact cases: integer-valued float32 inputs in [-1000, 1000], step sizes 3/2 and 3/4 and group weights that are powers
of two (or 0).  Every product and every partial sum is then an integer multiple of 1/16 below 2^53 -- exact in double
in any summation order -- and every updated element a multiple of 1/4 below 2^14 -- exact in float with or without FMA
contraction -- so the kernels must reproduce the references with ==, and an element skipped, visited twice or weighted
with the wrong group's damping changes the result.  The sizes straddle each kernel's block (256), its float4 body
(n % 4), and one full grid-stride sweep (1024 x 256 elements in the dots, 1024 x 256 x 4 in the update, 4096 x 256 in
axpy / xpby / damp_add).

One rounding case per update kernel (alpha = 1/3 on normal inputs) holds the float arithmetic to its derived bound,
and the control-block cases pin what a stopped or early-terminated solve may touch.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gslm.params import GROUPS, ParamLayout

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

GUARD = 12345.0                        # the element past each vector: never written, and (NaN_PAD) never read
WEIGHTS = (0.0, 1.0, 2.0, 0.5, 4.0, 8.0, 0.25)
NB = 1024                              # DOT_BLOCKS of cg.hip: the partials per dot


def _lib():
    from gslm import _lib as L
    return L


def _ints(rng, n):
    return rng.integers(-1000, 1001, size=n).astype(np.float32)


def _dev(a, pad=1, fill=GUARD):
    """Device copy of a host vector with `pad` extra elements set to `fill` behind it."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.concatenate([a, np.full(pad, fill, dtype=a.dtype)])).cuda()


def _host(t, n):
    """(first n elements, the guard elements behind them) of a device vector."""
    h = t.cpu().numpy()
    return h[:n], h[n:]


def _scalars(*vals):
    return torch.tensor(list(vals), dtype=torch.float64, device="cuda")


def _slot(sc, i):
    return sc.data_ptr() + 8 * i


def _nan_scratch(nbytes):
    return torch.full((max(nbytes // 8, 1),), math.nan, dtype=torch.float64, device="cuda")


def _groups(bounds, damp):
    return (ctypes.c_int64 * len(bounds))(*bounds), (ctypes.c_double * max(len(damp), 1))(*damp)


def _group_weight(bounds, damp, n):
    """Per-element weight of gslm_dot / gslm_damp_add's groups: damp[k] on [bounds[k], min(bounds[k+1], n)), else 0."""
    w = np.zeros(n, dtype=np.float64)
    for k, d in enumerate(damp):
        lo, hi = min(bounds[k], n), min(bounds[k + 1], n)
        if hi > lo:
            w[lo:hi] = d
    return w


# ------------------------------------------------------------------------------------------------ gslm_dot
def _dot(a, b, n, bounds=None, damp=None, pad=1, fill=GUARD):
    L = _lib()
    ad, bd = _dev(a, pad, fill), _dev(b, pad, fill)
    scratch = _nan_scratch(L.lib.gslm_dot_scratch_bytes(n))
    out = _scalars(math.nan)
    if bounds is None:
        st = L.lib.gslm_dot(ad.data_ptr(), bd.data_ptr(), None, None, 0, n, scratch.data_ptr(), out.data_ptr(),
                            L.stream_handle())
    else:
        bo, da = _groups(bounds, damp)
        st = L.lib.gslm_dot(ad.data_ptr(), bd.data_ptr(), bo, da, len(damp), n, scratch.data_ptr(), out.data_ptr(),
                            L.stream_handle())
    torch.cuda.synchronize()
    return st, out.item()


@pytest.mark.parametrize("n", [0, 1, 3, 255, 256, 257, 262143, 262144, 262145, 1048583])
def test_dot_ungrouped_exact(n):
    rng = np.random.default_rng(100 + n)
    a, b = _ints(rng, n), _ints(rng, n)
    st, got = _dot(a, b, n)
    assert st == 0
    assert got == float(np.dot(a.astype(np.float64), b.astype(np.float64)))


def _layout_cases():
    cases = []
    for P, K in ((1, 1), (5, 4), (4443, 16), (17771, 16)):
        lay = ParamLayout(P, K, 1)
        cases.append((f"layout{P}x{K}", lay.numel, lay.bounds(), WEIGHTS))
    n = 1048583  # past one sweep of every kernel here
    cases += [
        ("empty_group", n, [0, 7, 7, 262151, 262152, 400003, 1048570, n], WEIGHTS[1:] + WEIGHTS[:1]),
        ("skipped_prefix", n, [13, 100, 300001, 300002, 524301, 786445, 1048577, n], WEIGHTS[::-1]),
        ("clipped_last", n, [0, 5, 262149, 262150, 600000, 600001, 1048575, n + 1000], (2.0, 0.0, 1.0, 8.0, 0.5, 4.0, 0.25)),
        ("group_past_n", 1000, [0, 100, 999, 1000, 1001, 5000, 5000, 6000], (1.0, 2.0, 4.0, 8.0, 0.5, 0.25, 2.0)),
        ("one_group", n, [3, n - 2], (4.0,)),
        ("one_group_small", 11, [2, 9], (0.5,)),
    ]
    return cases


LAYOUT_CASES = _layout_cases()
# what a group bound past n would read: NaN inside the allocation (the cases above reach at most 5000 elements past
# n), so a kernel that does not clip fails the comparison instead of reading foreign memory
NAN_PAD = 6000


@pytest.mark.parametrize("name,n,bounds,damp", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_dot_grouped_exact(name, n, bounds, damp):
    rng = np.random.default_rng(len(name) + n)
    a, b = _ints(rng, n), _ints(rng, n)
    st, got = _dot(a, b, n, bounds, damp, pad=NAN_PAD, fill=math.nan)
    assert st == 0
    w = _group_weight(bounds, damp, n)
    assert got == float(np.sum(w * a.astype(np.float64) * b.astype(np.float64)))


def test_dot_and_damp_add_refuse_nine_groups():
    L = _lib()
    t = torch.zeros(16, dtype=torch.float32, device="cuda")
    sc = _nan_scratch(L.lib.gslm_dot_scratch_bytes(16))
    out = _scalars(-1.0)
    bo, da = _groups(list(range(10)), [1.0] * 9)
    h = L.stream_handle()
    assert L.lib.gslm_dot(t.data_ptr(), t.data_ptr(), bo, da, 9, 16, sc.data_ptr(), out.data_ptr(), h) == L.GSLM_ERR_INVALID
    assert L.lib.gslm_damp_add(16, t.data_ptr(), bo, da, 9, t.data_ptr(), h) == L.GSLM_ERR_INVALID
    torch.cuda.synchronize()
    assert out.item() == -1.0


# ------------------------------------------------------------------------------------------------ gslm_damp_add
@pytest.mark.parametrize("name,n,bounds,damp", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_damp_add_exact(name, n, bounds, damp):
    L = _lib()
    rng = np.random.default_rng(7 * len(name) + n)
    x, y = _ints(rng, n), _ints(rng, n)
    xd, yd = _dev(x, NAN_PAD, math.nan), _dev(y)
    bo, da = _groups(bounds, damp)
    L.check(L.lib.gslm_damp_add(n, xd.data_ptr(), bo, da, len(damp), yd.data_ptr(), L.stream_handle()))
    torch.cuda.synchronize()
    got, guard = _host(yd, n)
    w = _group_weight(bounds, damp, n)
    ref = (y.astype(np.float64) + w * x.astype(np.float64)).astype(np.float32)  # exact: multiples of 1/4 below 2^14
    assert np.array_equal(got, ref)
    # outside every group (and inside a zero-weight one) y keeps its bits
    assert np.array_equal(got[w == 0].view(np.int32), y[w == 0].view(np.int32))
    assert guard[0] == GUARD


def test_damp_add_without_groups_adds_x():
    L = _lib()
    n = 1048583
    rng = np.random.default_rng(3)
    x, y = _ints(rng, n), _ints(rng, n)
    xd, yd = _dev(x), _dev(y)
    L.check(L.lib.gslm_damp_add(n, xd.data_ptr(), None, None, 0, yd.data_ptr(), L.stream_handle()))
    torch.cuda.synchronize()
    got, guard = _host(yd, n)
    assert np.array_equal(got, x + y) and guard[0] == GUARD


# ------------------------------------------------------------------------------------------------ axpy / xpby
SWEEP_N = [0, 1, 1048575, 1048576, 1048583]


@pytest.mark.parametrize("n", SWEEP_N)
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("with_den", [True, False])
def test_axpy_dev_exact(n, sign, with_den):
    """y += sign (num / den) x with num / den = 3 / 2, and den = NULL: a = *num = 3."""
    L = _lib()
    rng = np.random.default_rng(200 + n)
    x, y = _ints(rng, n), _ints(rng, n)
    xd, yd = _dev(x), _dev(y)
    sc = _scalars(3.0, 2.0)
    L.check(L.lib.gslm_axpy_dev(n, _slot(sc, 0), _slot(sc, 1) if with_den else None, sign, xd.data_ptr(),
                                yd.data_ptr(), L.stream_handle()))
    torch.cuda.synchronize()
    a = sign * (1.5 if with_den else 3.0)
    got, guard = _host(yd, n)
    assert np.array_equal(got, (y.astype(np.float64) + a * x.astype(np.float64)).astype(np.float32))
    assert guard[0] == GUARD
    assert np.array_equal(_host(xd, n)[0], x)


@pytest.mark.parametrize("n", SWEEP_N)
def test_xpby_dev_exact(n):
    """p = s + (3 / 4) p."""
    L = _lib()
    rng = np.random.default_rng(300 + n)
    s, p = _ints(rng, n), _ints(rng, n)
    sd, pd = _dev(s), _dev(p)
    sc = _scalars(3.0, 4.0)
    L.check(L.lib.gslm_xpby_dev(n, sd.data_ptr(), _slot(sc, 0), _slot(sc, 1), pd.data_ptr(), L.stream_handle()))
    torch.cuda.synchronize()
    got, guard = _host(pd, n)
    assert np.array_equal(got, (s.astype(np.float64) + 0.75 * p.astype(np.float64)).astype(np.float32))
    assert guard[0] == GUARD
    assert np.array_equal(_host(sd, n)[0], s) and _host(sd, n)[1][0] == GUARD


# ------------------------------------------------------------------------------------------------ gslm_cg_update[_monitor]
class _Update:
    """One gslm_cg_update / gslm_cg_update_monitor call on guarded device vectors."""

    def __init__(self, n, p, q, x, s, g, gam, dele, monitor, with_x=True, ctl=None, scratch=None):
        L = _lib()
        self.n = n
        # x == NULL: p must not be read either (NaN would reach nothing, but a read past a short p could fault)
        self.pd = _dev(p if with_x else np.full(n, np.nan, dtype=np.float32))
        self.qd, self.sd, self.gd = _dev(q), _dev(s), _dev(g)
        self.xd = _dev(x)
        self.sc = _scalars(gam, dele, math.nan, math.nan, math.nan)  # gamma, delta, gamma', <x, g>, <x, s>
        self.scratch = _nan_scratch(3 * NB * 8) if scratch is None else scratch
        self.ctl = None if ctl is None else torch.tensor(ctl, dtype=torch.float64, device="cuda")
        xp = self.xd.data_ptr() if with_x else None
        h = L.stream_handle()
        if monitor:
            self.status = L.lib.gslm_cg_update_monitor(
                n, _slot(self.sc, 0), _slot(self.sc, 1), self.pd.data_ptr(), self.qd.data_ptr(), xp, self.sd.data_ptr(),
                self.gd.data_ptr(), self.scratch.data_ptr(), self.scratch.numel() * 8, _slot(self.sc, 2),
                _slot(self.sc, 3), _slot(self.sc, 4), None if self.ctl is None else self.ctl.data_ptr(), h)
        else:
            self.status = L.lib.gslm_cg_update(
                n, _slot(self.sc, 0), _slot(self.sc, 1), self.pd.data_ptr(), self.qd.data_ptr(), xp, self.sd.data_ptr(),
                self.scratch.data_ptr(), _slot(self.sc, 2), h)
        torch.cuda.synchronize()
        self.x, self.x_guard = _host(self.xd, n)
        self.s, self.s_guard = _host(self.sd, n)
        self.gamn, self.xg, self.xs = self.sc.tolist()[2:]

    def inputs_untouched(self, p, q, g, with_x=True):
        ok = np.array_equal(_host(self.qd, self.n)[0], q) and np.array_equal(_host(self.gd, self.n)[0], g)
        if with_x:
            ok = ok and np.array_equal(_host(self.pd, self.n)[0], p)
        return ok and all(_host(t, self.n)[1][0] == GUARD for t in (self.pd, self.qd, self.gd))


UPDATE_N = [0, 1, 2, 3, 4, 5, 7, 1023, 1048576, 1048579, 1048581]


@pytest.mark.parametrize("n", UPDATE_N)
@pytest.mark.parametrize("monitor", [False, True])
@pytest.mark.parametrize("with_x", [True, False])
def test_cg_update_exact(n, monitor, with_x):
    """x += (3/2) p ; s -= (3/2) q ; gamma' = <s, s> [; <x, g>, <x, s>]: float4 body, scalar tail (n % 4 in 0..3), a
    second sweep past 1024 x 256 x 4 elements, and the x == NULL form that streams s and q only."""
    rng = np.random.default_rng(400 + n)
    p, q, x, s, g = (_ints(rng, n) for _ in range(5))
    u = _Update(n, p, q, x, s, g, 3.0, 2.0, monitor, with_x)
    assert u.status == 0
    d = lambda v: v.astype(np.float64)
    x_ref = d(x) + 1.5 * d(p)
    s_ref = d(s) - 1.5 * d(q)
    assert np.array_equal(u.s, s_ref.astype(np.float32))
    assert u.gamn == float(np.sum(s_ref * s_ref))
    if with_x:
        assert np.array_equal(u.x, x_ref.astype(np.float32))
        if monitor:
            assert u.xg == float(np.sum(x_ref * d(g)))
            assert u.xs == float(np.sum(x_ref * s_ref))
    else:
        assert np.array_equal(u.x.view(np.int32), x.view(np.int32))  # (the buffer was not passed at all)
    assert u.x_guard[0] == GUARD and u.s_guard[0] == GUARD
    assert u.inputs_untouched(p, q, g, with_x)


def test_cg_update_argument_checks():
    """A vector 4 bytes off a 16-byte boundary is refused (the float4 body), so is a monitor scratch below three
    sets of 1024 partials; neither launches anything."""
    L = _lib()
    n = 64
    t = [torch.zeros(n + 4, dtype=torch.float32, device="cuda") for _ in range(5)]
    sc = _scalars(3.0, 2.0, -1.0, -1.0, -1.0)
    scratch = _nan_scratch(3 * NB * 8)
    h = L.stream_handle()
    for bad in range(4):  # p, q, x, s
        ptrs = [v.data_ptr() + (4 if k == bad else 0) for k, v in enumerate(t[:4])]
        assert L.lib.gslm_cg_update(n, _slot(sc, 0), _slot(sc, 1), *ptrs, scratch.data_ptr(), _slot(sc, 2),
                                    h) == L.GSLM_ERR_INVALID, bad
    for bad in range(5):  # p, q, x, s, g
        ptrs = [v.data_ptr() + (4 if k == bad else 0) for k, v in enumerate(t)]
        assert L.lib.gslm_cg_update_monitor(n, _slot(sc, 0), _slot(sc, 1), *ptrs, scratch.data_ptr(), 3 * NB * 8,
                                            _slot(sc, 2), _slot(sc, 3), _slot(sc, 4), None, h) == L.GSLM_ERR_INVALID, bad
    ptrs = [v.data_ptr() for v in t]
    assert L.lib.gslm_cg_update_monitor(n, _slot(sc, 0), _slot(sc, 1), *ptrs, scratch.data_ptr(), 3 * NB * 8 - 1,
                                        _slot(sc, 2), _slot(sc, 3), _slot(sc, 4), None, h) == L.GSLM_ERR_CAPACITY
    torch.cuda.synchronize()
    assert sc.tolist()[2:] == [-1.0, -1.0, -1.0]
    assert all(not bool(v.any()) for v in t)


@pytest.mark.parametrize("monitor", [False, True])
def test_cg_update_rounding(monitor):
    """alpha = 1/3 on normal inputs, n = 1048579 (float4 body, a 3-element tail, two sweeps).

    Elements.  The kernel forms a32 = (float)(gamma / delta), then x_i + a32 p_i in float: either fl(x + fl(a32 p))
    -- fl(a32 p) = a32 p (1 + e1), the sum (x + a32 p (1 + e1)) (1 + e2), |e1|, |e2| <= 2^-24, so the error is at
    most 2^-24 |a32 p| + 2^-24 |x + a32 p| + 2^-48 |a32 p| -- or, contracted to an FMA, one rounding of the exact
    x + a32 p: at most 2^-24 |x + a32 p|.  Both are within 2^-24 (|a32 p| + |x + a32 p|) (1 + 2^-20) of the float64
    reference x + a32 p, whose own rounding (2^-53 relative) the factor 1 + 2^-20 absorbs too.  (No underflow: the
    products of N(0, 1) draws with 1/3 are far above 2^-126.)

    Sums.  gamma', <x, g> and <x, s> are sums of n products of two floats, each exact in double (24 + 24 bits).
    Summing n doubles in any order (thread-strided, then wave / block / final tree) errs by at most
    (n - 1) u / (1 - (n - 1) u) sum |t_i| with u = 2^-53, which is below n u sum |t_i| while n (n - 1) u <= 1
    (n < 9e7): the bound is n 2^-53 sum |t_i|.  The terms are built from the float vectors
    of the library's own arithmetic -- csrc/Makefile compiles with -ffp-contract=off, two roundings -- restated in
    numpy float32 from the inputs, so the bound covers the summation alone."""
    n = 1048579
    rng = np.random.default_rng(9)
    p, q, x, s, g = (rng.standard_normal(n).astype(np.float32) for _ in range(5))
    u = _Update(n, p, q, x, s, g, 1.0, 3.0, monitor)
    assert u.status == 0
    a32 = np.float32(np.float64(1.0) / np.float64(3.0))
    d = lambda v: v.astype(np.float64)
    ap, aq = np.float64(a32) * d(p), np.float64(a32) * d(q)
    x_ref, s_ref = d(x) + ap, d(s) - aq
    eps = 2.0 ** -24 * (1 + 2.0 ** -20)
    assert np.all(np.abs(d(u.x) - x_ref) <= eps * (np.abs(ap) + np.abs(x_ref)))
    assert np.all(np.abs(d(u.s) - s_ref) <= eps * (np.abs(aq) + np.abs(s_ref)))
    x32 = d(x + a32 * p)  # float32 arithmetic: two roundings
    s32 = d(s - a32 * q)
    sums = [(u.gamn, s32 * s32)]
    if monitor:
        sums += [(u.xg, x32 * d(g)), (u.xs, x32 * s32)]
    for got, terms in sums:  # (math.fsum: the correctly rounded sum, so the reference adds no summation error)
        assert abs(got - math.fsum(terms)) <= n * 2.0 ** -53 * math.fsum(np.abs(terms))
    assert u.x_guard[0] == GUARD and u.s_guard[0] == GUARD


# ------------------------------------------------------------------------------------------------ control block
def _ctl(stop=0.0, iters=0.0, last=math.inf, nh=0.0, hist=(math.nan, math.nan)):
    return [stop, iters, last, nh, *hist]


@pytest.mark.parametrize("n", [5, 1048579])
@pytest.mark.parametrize("case,stop,dele", [("stopped", 2.0, 2.0), ("delta_zero", 0.0, 0.0),
                                            ("delta_tiny", 0.0, 1e-21), ("delta_nan", 0.0, math.nan)])
def test_cg_update_monitor_leaves_a_stopped_solve_alone(n, case, stop, dele):
    rng = np.random.default_rng(500 + n)
    p, q, x, s, g = (_ints(rng, n) for _ in range(5))
    u = _Update(n, p, q, x, s, g, 3.0, dele, True, ctl=_ctl(stop=stop))
    assert u.status == 0
    assert np.array_equal(u.x.view(np.int32), x.view(np.int32))
    assert np.array_equal(u.s.view(np.int32), s.view(np.int32))
    c = u.ctl.tolist()
    assert c[:4] == [stop, 0.0, math.inf, 0.0]  # the update only reads the block


@pytest.mark.parametrize("n", [5, 1048579])
def test_cg_update_monitor_moves_above_the_delta_threshold(n):
    """delta = 1e-19 >= 1e-20: the step is taken (gamma = 1.5e-19: alpha rounds to 1.5f)."""
    rng = np.random.default_rng(600 + n)
    p, q, x, s, g = (_ints(rng, n) for _ in range(5))
    u = _Update(n, p, q, x, s, g, 1.5e-19, 1e-19, True, ctl=_ctl())
    assert np.float32(np.float64(1.5e-19) / np.float64(1e-19)) == np.float32(1.5)
    d = lambda v: v.astype(np.float64)
    x_ref, s_ref = d(x) + 1.5 * d(p), d(s) - 1.5 * d(q)
    assert np.array_equal(u.x, x_ref.astype(np.float32)) and np.array_equal(u.s, s_ref.astype(np.float32))
    assert (u.gamn, u.xg, u.xs) == (float(np.sum(s_ref * s_ref)), float(np.sum(x_ref * d(g))),
                                    float(np.sum(x_ref * s_ref)))


def _monitor(sc, ctl, tol=1e-10, atol=0.0, max_hist=2):
    """gslm_cg_monitor on host lists: sc = [gamma, gamma', delta, <x, g>, <x, s>, b2] -> the control block after."""
    L = _lib()
    scd = _scalars(*sc)
    cd = torch.tensor(ctl, dtype=torch.float64, device="cuda")
    L.check(L.lib.gslm_cg_monitor(_slot(scd, 0), _slot(scd, 1), _slot(scd, 2), _slot(scd, 3), _slot(scd, 4),
                                  _slot(scd, 5), tol, atol, cd.data_ptr(), max_hist, L.stream_handle()))
    torch.cuda.synchronize()
    assert scd.tolist() == [float(v) for v in sc] or any(math.isnan(v) for v in sc)  # the scalars are inputs only
    return cd.tolist()


def _same(a, b):
    """List equality with NaN == NaN."""
    return len(a) == len(b) and all((math.isnan(u) and math.isnan(v)) or u == v for u, v in zip(a, b))


@pytest.mark.parametrize("dele,stop", [(0.0, 1.0), (1e-21, 1.0), (math.nan, 4.0), (math.inf, 4.0)])
@pytest.mark.parametrize("n", [5, 1048579])
def test_delta_underflow_update_then_monitor(n, dele, stop):
    """The reference's early termination (delta < 1e-20 before x moves) on the device path: the update returns
    without writing partials, the finalisation sums whatever the scratch held (NaN here) into gamma', <x, g>, <x, s>,
    and the monitor must still report stop 1 -- it may not look at those three before delta.  A non-finite delta is
    stop 4."""
    L = _lib()
    rng = np.random.default_rng(700 + n)
    p, q, x, s, g = (_ints(rng, n) for _ in range(5))
    u = _Update(n, p, q, x, s, g, 3.0, dele, True, ctl=_ctl())
    assert u.status == 0
    b2 = _scalars(10.0)
    L.check(L.lib.gslm_cg_monitor(_slot(u.sc, 0), _slot(u.sc, 2), _slot(u.sc, 1), _slot(u.sc, 3), _slot(u.sc, 4),
                                  b2.data_ptr(), 1e-10, 0.0, u.ctl.data_ptr(), 2, L.stream_handle()))
    torch.cuda.synchronize()
    c = u.ctl.tolist()
    assert c[0] == stop and c[1] == 0.0 and c[2] == math.inf and c[3] == 0.0, c
    assert math.isnan(c[4]) and math.isnan(c[5])
    assert np.array_equal(_host(u.xd, n)[0].view(np.int32), x.view(np.int32))
    assert np.array_equal(_host(u.sd, n)[0].view(np.int32), s.view(np.int32))


def test_cg_monitor_nonfinite_gamma_wins_over_small_delta():
    """gamma and delta are both written before the update: either one non-finite is stop 4, also beside a small
    delta."""
    for gam in (math.nan, math.inf):
        c = _monitor([gam, 0.5, 0.0, 0.1, 0.1, 10.0], _ctl())
        assert c[0] == 4.0 and c[1] == 0.0 and c[3] == 0.0
    for k in (1, 3, 4):  # gamma', <x, g>, <x, s> beside a healthy delta
        sc = [1.0, 0.5, 2.0, 0.1, 0.1, 10.0]
        sc[k] = math.nan
        c = _monitor(sc, _ctl())
        assert c[0] == 4.0 and c[1] == 0.0 and c[3] == 0.0


def test_cg_monitor_table():
    """The stopping tests one by one; res = (b2 - <x, g>) - <x, s> = (10 - 2.5) - 1.25 = 6.25."""
    nan = math.nan
    # stop 1: delta small -- nothing else moves
    assert _same(_monitor([1.0, 0.5, 1e-21, 2.5, 1.25, 10.0], _ctl(iters=3.0, last=7.0, nh=1.0, hist=(7.0, nan))),
                 _ctl(1.0, 3.0, 7.0, 1.0, (7.0, nan)))
    # stop 2: the residual rose -- appended to the history first, last_res and iters kept
    assert _same(_monitor([1.0, 0.5, 2.0, 2.5, 1.25, 10.0], _ctl(iters=1.0, last=6.0, nh=1.0, hist=(6.0, nan))),
                 _ctl(2.0, 1.0, 6.0, 2.0, (6.0, 6.25)))
    # an equal residual is not a rise: continue
    assert _same(_monitor([1.0, 0.5, 2.0, 2.5, 1.25, 10.0], _ctl(iters=1.0, last=6.25, nh=1.0, hist=(6.25, nan))),
                 _ctl(0.0, 2.0, 6.25, 2.0, (6.25, 6.25)))
    # stop 3 by tol: gamma' = 1e-3 < 1e-2 sqrt(4) -- last_res updated, iters kept
    assert _same(_monitor([4.0, 1e-3, 2.0, 2.5, 1.25, 10.0], _ctl(), tol=1e-2),
                 _ctl(3.0, 0.0, 6.25, 1.0, (6.25, nan)))
    # gamma' = tol sqrt(gamma) exactly (0.5 * sqrt(4) = 1): not below, continue
    assert _same(_monitor([4.0, 1.0, 2.0, 2.5, 1.25, 10.0], _ctl(), tol=0.5),
                 _ctl(0.0, 1.0, 6.25, 1.0, (6.25, nan)))
    # stop 3 by atol: max(tol sqrt(gamma), atol) = atol
    assert _same(_monitor([4.0, 1.0, 2.0, 2.5, 1.25, 10.0], _ctl(), tol=1e-10, atol=1.5),
                 _ctl(3.0, 0.0, 6.25, 1.0, (6.25, nan)))
    # continue: iters += 1, last_res = res
    assert _same(_monitor([1.0, 0.5, 2.0, 2.5, 1.25, 10.0], _ctl(iters=4.0, last=8.0, nh=0.0)),
                 _ctl(0.0, 5.0, 6.25, 1.0, (6.25, nan)))
    # a stopped block is left alone, whatever the scalars say
    for stop in (1.0, 2.0, 3.0, 4.0):
        for sc in ([1.0, 0.5, 2.0, 2.5, 1.25, 10.0], [nan, nan, nan, nan, nan, 10.0]):
            assert _same(_monitor(sc, _ctl(stop, 2.0, 9.0, 1.0, (9.0, nan))), _ctl(stop, 2.0, 9.0, 1.0, (9.0, nan)))
    # a full history: the count still advances, the word behind the history keeps its value
    c = _monitor([1.0, 0.5, 2.0, 2.5, 1.25, 10.0], [0.0, 5.0, 8.0, 2.0, 9.0, 8.0, -77.0], max_hist=2)
    assert c == [0.0, 6.0, 6.25, 3.0, 9.0, 8.0, -77.0]
    c = _monitor([1.0, 0.5, 2.0, 2.5, 1.25, 10.0], [0.0, 0.0, math.inf, 0.0, -77.0], max_hist=0)
    assert c == [0.0, 1.0, 6.25, 1.0, -77.0]


# ------------------------------------------------------------------------------------------------ gslm_dot_finalize
# 2 = ceil(400 / 256) (the golden scene), 8 and 32 (the 2k / 8k test scenes), 3907 = ceil(1e6 / 256) (the benchmark)
@pytest.mark.parametrize("np_", [1, 2, 8, 32, 255, 256, 257, 2048, 2049, 3907, 5000])
def test_dot_finalize_exact(np_):
    L = _lib()
    rng = np.random.default_rng(800 + np_)
    part = rng.integers(-10 ** 9, 10 ** 9, size=np_).astype(np.float64)
    pd = _dev(part, 8, math.nan)
    out = _scalars(math.nan, GUARD)
    L.check(L.lib.gslm_dot_finalize(pd.data_ptr(), np_, out.data_ptr(), L.stream_handle()))
    torch.cuda.synchronize()
    assert out.tolist() == [float(np.sum(part)), GUARD]


# ------------------------------------------------------------------------------------------------ the solver's layouts
POW2_DAMP = dict(zip(GROUPS, (8.0, 0.5, 2.0, 0.25, 4.0, 1.0, 0.5)))


def _golden_problem(n_views):
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem
    from gslm.model import GaussianModel
    d = np.load(os.path.join(HERE, "golden", "solver_golden.npz"))
    _, D, W, H, _, nv = (int(v) for v in d["scene"])
    m = GaussianModel(D)
    m.set_params(*(torch.from_numpy(d[f"in_{k}"]).cuda() for k in GROUPS))
    m.active_sh_degree = D
    cams = orbit_cameras(nv, W, H, seed=1, images=[torch.from_numpy(d[f"gt{i}"]) for i in range(nv)])
    for c in cams:
        c.to("cuda")
    return LMProblem(m, cams[:n_views], torch.zeros(3), damp=POW2_DAMP)


def _synthetic_problem():
    """301 Gaussians, degree 1: numel = 23 * 301 + 12 = 6935 = 3 mod 4.  A 25-degree camera sees only the middle of
    the cube, so the active set is a proper subset."""
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem
    from gslm.model import synthetic_gaussians
    m = synthetic_gaussians(301, 1, seed=2, s0=0.06).to("cuda")
    cam = orbit_cameras(1, 40, 33, fovx_deg=25.0, seed=3,
                        images=[torch.rand(3, 33, 40, generator=torch.Generator().manual_seed(4))])[0]
    cam.to("cuda")
    return LMProblem(m, [cam], torch.zeros(3), damp=POW2_DAMP)


def _check_layout_algebra(prob, seed):
    """prob.dot(damped) and prob.damp_add against sum_k damp_k <a_k, b_k> and y + D v built from layout.offsets."""
    lay = prob.layout
    n = lay.numel
    rng = np.random.default_rng(seed)
    a, b, y = _ints(rng, n), _ints(rng, n), _ints(rng, n)
    w = np.zeros(n, dtype=np.float64)
    for k, grp in enumerate(GROUPS):
        lo, hi = lay.offsets[grp]
        w[lo:hi] = float(prob._damps[k])
        assert float(prob._damps[k]) == POW2_DAMP[grp]
    assert np.all(w > 0)  # the groups tile [0, n)
    ad, bd, yd = _dev(a, 0), _dev(b, 0), _dev(y)
    out = _scalars(math.nan, math.nan)
    prob.dot_scratch.fill_(math.nan)
    prob.dot(ad, bd, _slot(out, 0), damped=True)
    prob.dot(ad, bd, _slot(out, 1))
    prob.damp_add(ad, yd[:n])
    torch.cuda.synchronize()
    d = lambda v: v.astype(np.float64)
    assert out.tolist() == [float(np.sum(w * d(a) * d(b))), float(np.sum(d(a) * d(b)))]
    got, guard = _host(yd, n)
    assert np.array_equal(got, (d(y) + w * d(a)).astype(np.float32)) and guard[0] == GUARD


def test_layout_algebra_full_and_active():
    """The solver's own calls (LMProblem.dot / damp_add with its bounds and damping arrays) on the golden scene's
    layout, on its active-set view (ParamLayout(Pa): Pa, hence n % 4, the float4 floor lo = (3 Pa // 4) 4 of the xyz
    group and all seven bounds come from the data) and on a synthetic scene whose numel is 3 mod 4.  (The golden
    view moves all of its 400 Gaussians; the synthetic one 212 of 301.)"""
    mods = []
    for make, subset in ((lambda: _golden_problem(1), False), (_synthetic_problem, True)):
        prob = make()
        prob.evaluate()
        prob.rhs(prob.zeros())  # the row map the active list is read from
        act = prob.active_view()
        assert act is not None and 0 < act.layout.P <= prob.layout.P
        assert not subset or act.layout.P < prob.layout.P
        assert act.layout.numel == ParamLayout(act.layout.P, prob.layout.K, prob.layout.n_exposure).numel
        for k, pr in enumerate((prob, act)):
            _check_layout_algebra(pr, 900 + k)
            n = pr.layout.numel
            lo = (3 * pr.layout.P // 4) * 4  # cgls_fused's start of the updated range
            assert lo % 4 == 0 and 0 <= 3 * pr.layout.P - lo < 4
            mods.append(n % 4)  # (= (n - lo) % 4, the length the solver's update kernel sees)
            print(f"P = {pr.layout.P}: numel = {n} = {n % 4} mod 4, lo = {lo}")
    # the scalar tail of the vector kernels is reached through a real layout, not only through hand-made sizes
    assert any(m != 0 for m in mods), mods


@pytest.mark.parametrize("n_views", [1, 2])
def test_cgls_zero_rhs_stops_on_delta_on_both_paths(n_views):
    """J^T b = 0: the first delta = <p, A p> is 0 < 1e-20, the reference's early termination.  The device tests and
    the host tests must agree -- x = 0, no iteration, no history, stop 1 -- whatever the dot scratch held (NaN here:
    the early-returning update writes no partials).  One view solves on the active set, two on the full vectors."""
    from gslm.lm import cgls_fused
    prob = _golden_problem(n_views)
    prob.evaluate()
    prob.rhs(prob.zeros())
    g = prob.zeros()
    res = {}
    for host in (False, True):
        prob.dot_scratch.fill_(math.nan)
        x, info = cgls_fused(prob, g, max_iter=3, restart_iter=2, check_every=True, host_checks=host)
        torch.cuda.synchronize()
        assert x.numel() == prob.layout.numel and not bool(x.any())
        assert info["iters"] == 0 and list(info["residuals"]) == []
        res[host] = (x, info)
    assert res[False][1]["stop"] == 1
    assert torch.equal(res[False][0].view(torch.int32), res[True][0].view(torch.int32))
