"""The lean CG loop's entry points through the C ABI, each against a reference built from its inputs.

gslm_cg_start_active, gslm_cg_update_lean, gslm_cg_end_active, gslm_active_params and the GSLM_MV_LEAN options of
gslm_matvec_view_active run whenever cgls_fused(check_every=False) solves a single-view problem; tests/
test_gpu_cg_lean.py reaches them through whole solves only.  Here they are called one at a time, with the conventions
of tests/test_gpu_vector_algebra.py: integer-valued float32 inputs in [-1000, 1000] and step sizes 3/2 and 3/4, so
every updated element is a multiple of 1/4 below 2^14 (exact in float with or without FMA contraction) and every
partial sum an integer multiple of 1/16 below 2^53 (exact in double in any order) -- all comparisons are == ; outputs
start as NaN, so an element a kernel did not write fails; a guard element stands behind every output.  Scalars that
arrive as block partials are hand-made integer doubles whose sums give gamma / delta = 3K / 2K = 3/2 (beta = 3K / 4K),
so a missed or doubled partial changes the step and with it every element.

The layouts are those LMProblem._pack_args produces: the projected SH-rest group (3 floats per row), the full one at
SH 3 and SH 1 (45 and 9: the generic-width division of the start kernel, the end kernel's loop over more than four
floats of a row) and SH 0 (width 0: two groups share an offset).  The lists: one row, none, 255 / 256 / 257 rows (one
block of the per-Gaussian kernels, and one more), every row (the inverse map has no -1), the 2683 of 3001 of
tests/test_gpu_cg_lean.py, and 20000 rows at SH 3 (more than 4 x 1024 x 256 elements behind lo: the start kernel's
second sweep).  Partial counts straddle load_scalar's 8 x 256 loads in flight (2048 / 2049) and reach the benchmark's
3907.  The only non-integer cases are bitwise comparisons with the entry points these kernels claim to reproduce:
gslm_dot, gslm_cg_update(x = NULL) and gslm_axpy_dev + gslm_active_unpack.

Every argument-check case is one the host code refuses before a launch.  Not tested: the 64-bit branch of the start
kernel's divmod_w (an offset of 2^32 or more inside a group needs vectors of more than 4 G elements).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_cg_lean import layout_scene, scene
from test_gpu_vector_algebra import GUARD, NB, _dev, _host, _ints, _lib, _scalars, _slot

pytestmark = pytest.mark.gpu
DEV = "cuda"

LAYOUTS = {"sh3_projected": (3, 3, 3, 3, 4, 1), "sh3_full": (3, 3, 45, 3, 4, 1), "sh1_full": (3, 3, 9, 3, 4, 1),
           "sh0": (3, 3, 0, 3, 4, 1)}
LISTS = [(1, 1), (300, 0), (300, 255), (300, 256), (300, 257), (300, 300), (3001, 2683)]
BIG = (20011, 20000)  # at sh3_full: n - lo = 59 x 20000 + 12 - 60000 > 4 x 1024 x 256
KSUM = 1000003        # the hand-made partials sum to 3 KSUM, 2 KSUM or 4 KSUM


def _widths(w):
    return (ctypes.c_int32 * len(w))(*w)


def _ids(rng, P, na):
    return np.sort(rng.choice(P, size=na, replace=False)).astype(np.int32)


def _ids_dev(ids):
    """The list on the device, followed by 3 len + 16 entries of the valid id 0: a kernel that takes an element for
    another group's divides its offset by the wrong width and indexes past the list (by less than 14 / 3 of its
    length when the widths sum to 14) -- it then reads a valid row and fails the comparison, not foreign memory."""
    return _dev(ids, 3 * len(ids) + 16, 0)


def _lo(na):
    return (3 * na // 4) * 4  # _cgls_lean's start of the updated range (the masked xyz group, floored to a float4)


def _sizes(P, na, w, tail_n):
    """(length of a full-layout vector, of a list-layout one)."""
    return P * sum(w) + tail_n, na * sum(w) + tail_n


def _pack_ref(full, ids, P, w, tail_n):
    """The list layout of a full-layout host vector."""
    parts, po = [], 0
    for wk in w:
        parts.append(full[po:po + P * wk].reshape(P, wk)[ids].reshape(-1))
        po += P * wk
    parts.append(full[po:po + tail_n])
    return np.concatenate(parts)


def _unpack_ref(vec, ids, P, w, tail_n):
    """The full layout of a list-layout host vector, +0.0f off the list."""
    na, parts, ao = len(ids), [], 0
    for wk in w:
        grp = np.zeros((P, wk), dtype=np.float32)
        grp[ids] = vec[ao:ao + na * wk].reshape(na, wk)
        parts.append(grp.reshape(-1))
        ao += na * wk
    parts.append(vec[ao:ao + tail_n])
    return np.concatenate(parts)


def _nan_vec(n):
    return _dev(np.full(n, np.nan, dtype=np.float32))


def _partials_out(np_=NB):
    """np_ NaN doubles for a kernel's block partials, and the guard behind them."""
    return _dev(np.full(np_, np.nan), 1, GUARD)


def _hand_partials(rng, np_, total):
    """np_ integer doubles of magnitude up to 1e9 that sum to `total` (np_ x 1e9 < 2^53: exact in any order)."""
    part = rng.integers(-10 ** 9, 10 ** 9, size=np_).astype(np.float64)
    part[-1] += total - part.sum()
    assert part.sum() == total and (np_ == 1 or part[-1] != 0)
    return part


def _finalize(part_dev, np_):
    L = _lib()
    out = _scalars(math.nan)
    L.check(L.lib.gslm_dot_finalize(part_dev.data_ptr(), np_, out.data_ptr(), L.stream_handle()))
    torch.cuda.synchronize()
    return out.item()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ gslm_cg_start_active
class _Start:
    """One gslm_cg_start_active call: NaN-filled, guarded s, p, q, x and partials."""

    def __init__(self, g_full, ids, P, w, tail_n, lo, ngroups=None, na=None, null=None, widths=None):
        L = _lib()
        self.n_full, self.n = _sizes(P, len(ids), w, tail_n)
        self.gd, self.idd = _dev(g_full), _ids_dev(ids)
        self.vec = {k: _nan_vec(self.n) for k in "spqx"}
        self.part = _partials_out()
        ptr = {k: v.data_ptr() for k, v in self.vec.items()}
        ptr.update(g=self.gd.data_ptr(), ids=self.idd.data_ptr() if len(ids) else None, part=self.part.data_ptr())
        if null:
            ptr[null] = None
        self.status = L.lib.gslm_cg_start_active(
            ptr["g"], ptr["ids"], len(ids) if na is None else na, P, _widths(w) if widths is None else widths,
            len(w) if ngroups is None else ngroups, tail_n, lo, ptr["s"], ptr["p"], ptr["q"], ptr["x"], ptr["part"],
            L.stream_handle())
        torch.cuda.synchronize()

    def host(self, k):
        return _host(self.vec[k], self.n)

    def untouched(self):
        """Nothing written: the four vectors and the partials still NaN."""
        return (all(bool(torch.isnan(v[:self.n]).all()) for v in self.vec.values())
                and bool(torch.isnan(self.part[:NB]).all()))


def _check_start(P, na, w, seed):
    rng = np.random.default_rng(seed)
    ids = _ids(rng, P, na)
    for tail_n in (0, 12):
        n_full, n = _sizes(P, na, w, tail_n)
        g_full = _ints(rng, n_full)
        want = _pack_ref(g_full, ids, P, w, tail_n)
        assert want.shape == (n,)
        for lo in sorted({_lo(na), 0, n}):
            c = _Start(g_full, ids, P, w, tail_n, lo)
            assert c.status == 0, (tail_n, lo)
            ref = want.copy()
            ref[:lo] = 0
            for k in "sp":
                got, guard = c.host(k)
                assert _same_bits(got, ref) and guard[0] == GUARD, (k, tail_n, lo)
            for k in "qx":
                got, guard = c.host(k)
                assert _same_bits(got, np.zeros(n, dtype=np.float32)) and guard[0] == GUARD, (k, tail_n, lo)
            tail = ref[lo:].astype(np.float64)
            assert _finalize(c.part, NB) == float(np.sum(tail * tail)), (tail_n, lo)
            assert c.part[NB].item() == GUARD
            gh, gg = _host(c.gd, n_full)
            ih, ig = _host(c.idd, na)
            assert np.array_equal(gh, g_full) and gg[0] == GUARD and np.array_equal(ih, ids) and not ig.any()


@pytest.mark.parametrize("P,na", LISTS, ids=lambda v: str(v))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_cg_start_active_exact(layout, P, na):
    """s = p = the listed rows of g on [lo, n) and 0 on [0, lo), q = x = 0 on all of [0, n), gamma_0's partials; with
    and without the exposure tail; lo the solver's, 0 (the xyz group gathered too) and n (nothing gathered)."""
    _check_start(P, na, LAYOUTS[layout], 1000 + 7 * P + na + len(layout))


def test_cg_start_active_second_sweep():
    P, na = BIG
    w = LAYOUTS["sh3_full"]
    assert _sizes(P, na, w, 12)[1] - _lo(na) > 4 * NB * 256
    _check_start(P, na, w, 1100)


def test_cg_start_active_gamma_is_bitwise_gslm_dot():
    """Normal inputs: the finished gamma_0 is bitwise the one gslm_dot makes of the s the kernel wrote."""
    L = _lib()
    P, na, w, tail_n = 3001, 2683, LAYOUTS["sh3_full"], 12
    rng = np.random.default_rng(1200)
    ids = _ids(rng, P, na)
    n_full, n = _sizes(P, na, w, tail_n)
    g_full = rng.standard_normal(n_full).astype(np.float32)
    lo = _lo(na)
    c = _Start(g_full, ids, P, w, tail_n, lo)
    assert c.status == 0
    want = _pack_ref(g_full, ids, P, w, tail_n)
    want[:lo] = 0
    assert _same_bits(c.host("s")[0], want)
    got = _finalize(c.part, NB)
    scratch = _dev(np.full(L.lib.gslm_dot_scratch_bytes(n - lo) // 8, np.nan), 0)
    out = _scalars(math.nan)
    sp = c.vec["s"].data_ptr() + 4 * lo
    L.check(L.lib.gslm_dot(sp, sp, None, None, 0, n - lo, scratch.data_ptr(), out.data_ptr(), L.stream_handle()))
    torch.cuda.synchronize()
    assert math.isfinite(got) and got > 0.0
    assert np.float64(got).view(np.int64) == np.float64(out.item()).view(np.int64)


def test_cg_start_active_argument_checks():
    """Refused by the launcher before anything is written."""
    L = _lib()
    P, na, w, tail_n = 300, 257, LAYOUTS["sh3_projected"], 12
    rng = np.random.default_rng(1300)
    ids = _ids(rng, P, na)
    n_full, n = _sizes(P, na, w, tail_n)
    g_full = _ints(rng, n_full)
    nine = (ctypes.c_int32 * 9)(*([1] * 9))
    bad = [dict(ngroups=0), dict(ngroups=9, widths=nine), dict(widths=_widths((3, 3, -3, 3, 4, 1))), dict(na=P + 1),
           dict(lo=n + 1), dict(lo=-4), dict(tail_n=-1)]
    bad += [dict(null=k) for k in ("g", "ids", "s", "p", "q", "x", "part")]
    for kw in bad:
        args = dict(tail_n=tail_n, lo=_lo(na))
        args.update(kw)
        c = _Start(g_full, ids, P, w, args.pop("tail_n"), args.pop("lo"), **args)
        assert c.status == L.GSLM_ERR_INVALID, kw
        assert c.untouched(), kw
    assert _Start(g_full, ids, P, w, tail_n, _lo(na)).status == 0  # (the same call without a fault is accepted)


# ------------------------------------------------------------------------------------------------ gslm_cg_update_lean
class _UpdateLean:
    """One gslm_cg_update_lean call.  gam / dele: a host array of partials, or (gam only) the finished scalar."""

    def __init__(self, n, q, s, gam, dele, alias=None, misalign=None, null_del=False):
        L = _lib()
        self.n = n
        self.pd = _nan_vec(n + 4)  # x == NULL: p is not read, and may hold anything
        self.qd, self.sd = _dev(q, 5), _dev(s, 5)
        gam_is_part = isinstance(gam, np.ndarray)
        self.gam_part = _dev(gam, 8, math.nan) if gam_is_part else None
        self.del_part = _dev(dele, 8, math.nan)
        self.sc = _scalars(math.nan if gam_is_part else gam, math.nan, GUARD)  # gamma, delta
        self.out = _partials_out()
        out_ptr = {None: self.out, "gam": self.gam_part, "del": self.del_part}[alias].data_ptr()
        off = lambda k: 4 if misalign == k else 0
        self.status = L.lib.gslm_cg_update_lean(
            n, _slot(self.sc, 0), self.gam_part.data_ptr() if gam_is_part else None, len(gam) if gam_is_part else 0,
            None if null_del else self.del_part.data_ptr(), len(dele), _slot(self.sc, 1), self.pd.data_ptr() + off("p"),
            self.qd.data_ptr() + off("q"), self.sd.data_ptr() + off("s"), out_ptr, L.stream_handle())
        torch.cuda.synchronize()
        self.s, self.s_guard = _host(self.sd, n)


UPDATE_N = [1, 3, 4, 5, 1023, 1048576, 1048579]
DEL_NP = [1, 2, 11, 255, 256, 257, 2048, 2049, 3907]


@pytest.mark.parametrize("del_np", DEL_NP)
@pytest.mark.parametrize("n", UPDATE_N)
@pytest.mark.parametrize("gam_partials", [False, True])
def test_cg_update_lean_exact(gam_partials, n, del_np):
    """s -= (3/2) q with delta = 2K as del_np partials and gamma = 3K finished or as 1024 partials."""
    rng = np.random.default_rng(2000 + n + 13 * del_np)
    q, s = _ints(rng, n), _ints(rng, n)
    dele = _hand_partials(rng, del_np, 2 * KSUM)
    gam = _hand_partials(rng, NB, 3 * KSUM) if gam_partials else float(3 * KSUM)
    u = _UpdateLean(n, q, s, gam, dele)
    assert u.status == 0
    s_ref = s.astype(np.float64) - 1.5 * q.astype(np.float64)
    assert np.array_equal(u.s, s_ref.astype(np.float32)) and np.all(u.s_guard == GUARD)
    assert u.sc.tolist() == [float(3 * KSUM), float(2 * KSUM), GUARD]
    assert _finalize(u.out, NB) == float(np.sum(s_ref * s_ref))
    assert u.out[NB].item() == GUARD
    # q, p (all NaN: never read) and the partials it summed are as they were
    qh, qg = _host(u.qd, n)
    assert np.array_equal(qh, q) and np.all(qg == GUARD)
    assert bool(torch.isnan(u.pd[:-1]).all()) and u.pd[-1].item() == GUARD
    assert np.array_equal(u.del_part.cpu().numpy(), np.concatenate([dele, np.full(8, np.nan)]), equal_nan=True)
    if gam_partials:
        assert np.array_equal(u.gam_part.cpu().numpy(), np.concatenate([gam, np.full(8, np.nan)]), equal_nan=True)


def test_cg_update_lean_rounding_is_bitwise_cg_update():
    """alpha = 1/3 on normal inputs, n = 1048579: s and the finished gamma' are bitwise gslm_cg_update's with
    x == NULL (held to its derived bound by test_gpu_vector_algebra.test_cg_update_rounding), given gamma = 1 and
    delta = 3 as finished scalars where this call sums them from 1024 and 2049 partials."""
    L = _lib()
    n = 1048579
    rng = np.random.default_rng(2100)
    q, s = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    u = _UpdateLean(n, q, s, _hand_partials(rng, NB, 1), _hand_partials(rng, 2049, 3))
    assert u.status == 0 and u.sc.tolist()[:2] == [1.0, 3.0]
    pd, qd, sd = _nan_vec(n), _dev(q), _dev(s)
    sc = _scalars(1.0, 3.0, math.nan)
    scratch = _partials_out()
    L.check(L.lib.gslm_cg_update(n, _slot(sc, 0), _slot(sc, 1), pd.data_ptr(), qd.data_ptr(), None, sd.data_ptr(),
                                 scratch.data_ptr(), _slot(sc, 2), L.stream_handle()))
    torch.cuda.synchronize()
    ref, guard = _host(sd, n)
    assert not _same_bits(ref, s)  # (the reference moved)
    assert _same_bits(u.s, ref) and np.all(u.s_guard == GUARD)
    assert np.float64(_finalize(u.out, NB)).view(np.int64) == np.float64(sc.tolist()[2]).view(np.int64)


def test_cg_update_lean_argument_checks():
    """The new partials in a buffer the call sums, a vector 4 bytes off a 16-byte boundary, no delta partials:
    refused, nothing launched."""
    L = _lib()
    n = 64
    rng = np.random.default_rng(2200)
    q, s = _ints(rng, n), _ints(rng, n)
    gam, dele = _hand_partials(rng, NB, 3 * KSUM), _hand_partials(rng, NB, 2 * KSUM)
    bad = [dict(alias="gam"), dict(alias="del"), dict(misalign="p"), dict(misalign="q"), dict(misalign="s"),
           dict(null_del=True)]
    for kw in bad:
        u = _UpdateLean(n, q, s, gam, dele, **kw)
        assert u.status == L.GSLM_ERR_INVALID, kw
        assert np.array_equal(u.s, s), kw
        assert bool(torch.isnan(u.out[:NB]).all()) and bool(torch.isnan(u.sc[:2]).all()), kw
        assert np.array_equal(u.gam_part.cpu().numpy()[:NB], gam), kw
        assert np.array_equal(u.del_part.cpu().numpy()[:NB], dele), kw
    assert _UpdateLean(n, q, s, gam, dele).status == 0


# ------------------------------------------------------------------------------------------------ gslm_cg_end_active
def _pos(ids, P):
    pos = np.full(P, -1, dtype=np.int32)
    pos[ids] = np.arange(len(ids), dtype=np.int32)
    return pos


class _End:
    """One gslm_cg_end_active call on a NaN-filled, guarded full-layout output."""

    def __init__(self, x, p, pos, na, P, w, tail_n, lo, num=3.0, den=2.0, fin=None, fin_np=None, fin_slot=True,
                 null=None, ngroups=None, widths=None):
        L = _lib()
        self.n_full = _sizes(P, na, w, tail_n)[0]
        self.xd, self.pd, self.posd = _dev(x), _dev(p), _dev(pos, 1, -7)
        self.outd = _nan_vec(self.n_full)
        self.sc = _scalars(math.nan if num is None else num, math.nan if den is None else den, -1.0, GUARD)
        self.fin = None if fin is None else _dev(fin, 8, math.nan)
        ptr = dict(x=self.xd.data_ptr(), p=self.pd.data_ptr(), pos=self.posd.data_ptr(), out=self.outd.data_ptr())
        if null:
            ptr[null] = None
        self.status = L.lib.gslm_cg_end_active(
            ptr["x"], ptr["p"], None if num is None else _slot(self.sc, 0), None if den is None else _slot(self.sc, 1),
            lo, ptr["pos"], na, P, _widths(w) if widths is None else widths, len(w) if ngroups is None else ngroups,
            tail_n, ptr["out"], None if fin is None else self.fin.data_ptr(),
            (0 if fin is None else len(fin)) if fin_np is None else fin_np, _slot(self.sc, 2) if fin_slot else None,
            L.stream_handle())
        torch.cuda.synchronize()
        self.out, self.guard = _host(self.outd, self.n_full)
        self.fin_value = self.sc.tolist()[2]

    def inputs_untouched(self, x, p, pos):
        return (_same_bits(_host(self.xd, len(x))[0], x) and _same_bits(_host(self.pd, len(p))[0], p)
                and np.array_equal(self.posd.cpu().numpy(), np.concatenate([pos, [-7]]))
                and self.xd[-1].item() == GUARD and self.pd[-1].item() == GUARD and self.sc[3].item() == GUARD)


def _end_ref(x, p, a, lo, ids, P, w, tail_n):
    """x + a p on [lo, n), x before it, in the full layout (a = 3/2 or 3 on integers: exact)."""
    v = x.astype(np.float64)
    v[lo:] += a * p.astype(np.float64)[lo:]
    return _unpack_ref(v.astype(np.float32), ids, P, w, tail_n)


def _off_list_is_plus_zero(out, ids, P, w):
    off = np.ones(P, dtype=bool)
    off[ids] = False
    po = 0
    for wk in w:
        if np.any(_bits(out[po:po + P * wk].reshape(P, wk)[off]) != 0):
            return False
        po += P * wk
    return True


def _check_end(P, na, w, seed):
    rng = np.random.default_rng(seed)
    ids = _ids(rng, P, na)
    pos = _pos(ids, P)
    for tail_n in (0, 12):
        n = _sizes(P, na, w, tail_n)[1]
        x, p = _ints(rng, n), _ints(rng, n)  # nonzero on [0, lo) too: the branch m < lo must not add a p
        for lo in sorted({_lo(na), 0, n}):
            c = _End(x, p, pos, na, P, w, tail_n, lo)
            assert c.status == 0, (tail_n, lo)
            assert _same_bits(c.out, _end_ref(x, p, 1.5, lo, ids, P, w, tail_n)), (tail_n, lo)
            assert _off_list_is_plus_zero(c.out, ids, P, w), (tail_n, lo)
            assert c.guard[0] == GUARD and c.fin_value == -1.0 and c.inputs_untouched(x, p, pos)


@pytest.mark.parametrize("P,na", LISTS, ids=lambda v: str(v))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_cg_end_active_exact(layout, P, na):
    """out = x + (3/2) p at list elements m >= lo, x at m < lo (x and p are nonzero there), the tail likewise, and
    the bit pattern 0x00000000 in every float of a row off the list; no partials: the slot for their sum keeps its
    value."""
    _check_end(P, na, LAYOUTS[layout], 3000 + 7 * P + na + len(layout))


def test_cg_end_active_many_rows():
    _check_end(*BIG, LAYOUTS["sh3_full"], 3100)


@pytest.mark.parametrize("fin_np", [0, 1, 1024, 2049])
def test_cg_end_active_finishes_the_last_gamma(fin_np):
    P, na, w, tail_n = 300, 257, LAYOUTS["sh3_full"], 12
    rng = np.random.default_rng(3200 + fin_np)
    ids = _ids(rng, P, na)
    pos = _pos(ids, P)
    n, lo = _sizes(P, na, w, tail_n)[1], _lo(na)
    x, p = _ints(rng, n), _ints(rng, n)
    fin = _hand_partials(rng, fin_np, 3 * KSUM) if fin_np else np.zeros(0)
    c = _End(x, p, pos, na, P, w, tail_n, lo, fin=fin)
    assert c.status == 0
    assert c.fin_value == (float(3 * KSUM) if fin_np else 0.0)
    assert _same_bits(c.out, _end_ref(x, p, 1.5, lo, ids, P, w, tail_n)) and c.guard[0] == GUARD
    assert np.array_equal(c.fin.cpu().numpy(), np.concatenate([fin, np.full(8, np.nan)]), equal_nan=True)
    assert c.inputs_untouched(x, p, pos)


@pytest.mark.parametrize("layout", ["sh3_projected", "sh3_full", "sh0"])
def test_cg_end_active_without_a_step_and_without_a_denominator(layout):
    """num_dev == NULL: out = x (p is not read: NULL, or all NaN); den_dev == NULL: a = *num = 3."""
    P, na, w, tail_n = 300, 257, LAYOUTS[layout], 12
    rng = np.random.default_rng(3300)
    ids = _ids(rng, P, na)
    pos = _pos(ids, P)
    n, lo = _sizes(P, na, w, tail_n)[1], _lo(na)
    x, p = _ints(rng, n), _ints(rng, n)
    for kw, pv in ((dict(null="p"), p), (dict(), np.full(n, np.nan, dtype=np.float32))):
        c = _End(x, pv, pos, na, P, w, tail_n, lo, num=None, den=None, **kw)
        assert c.status == 0
        assert _same_bits(c.out, _unpack_ref(x, ids, P, w, tail_n)) and c.guard[0] == GUARD
        assert _off_list_is_plus_zero(c.out, ids, P, w)
    c = _End(x, p, pos, na, P, w, tail_n, lo, den=None)
    assert c.status == 0
    assert _same_bits(c.out, _end_ref(x, p, 3.0, lo, ids, P, w, tail_n)) and c.guard[0] == GUARD
    assert c.inputs_untouched(x, p, pos)


@pytest.mark.parametrize("layout", ["sh3_projected", "sh3_full", "sh0"])
def test_cg_end_active_rounding_is_bitwise_axpy_then_unpack(layout):
    """alpha = 1/3 on normal inputs: bitwise gslm_axpy_dev on [lo, n) followed by gslm_active_unpack."""
    L = _lib()
    P, na, w, tail_n = 3001, 2683, LAYOUTS[layout], 12
    rng = np.random.default_rng(3400)
    ids = _ids(rng, P, na)
    pos = _pos(ids, P)
    n_full, n = _sizes(P, na, w, tail_n)
    lo = _lo(na)
    x, p = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    c = _End(x, p, pos, na, P, w, tail_n, lo, num=1.0, den=3.0)
    assert c.status == 0
    xd, pd, idd, refd = _dev(x), _dev(p), _ids_dev(ids), _nan_vec(n_full)
    sc = _scalars(1.0, 3.0)
    h = L.stream_handle()
    L.check(L.lib.gslm_axpy_dev(n - lo, _slot(sc, 0), _slot(sc, 1), 1.0, pd.data_ptr() + 4 * lo,
                                xd.data_ptr() + 4 * lo, h))
    L.check(L.lib.gslm_active_unpack(xd.data_ptr(), refd.data_ptr(), idd.data_ptr(), na, P, _widths(w), len(w),
                                     tail_n, h))
    torch.cuda.synchronize()
    ref = _host(refd, n_full)[0]
    assert not _same_bits(ref, _unpack_ref(x, ids, P, w, tail_n))  # (the reference moved)
    assert _same_bits(c.out, ref) and c.guard[0] == GUARD
    assert _off_list_is_plus_zero(c.out, ids, P, w)


def test_cg_end_active_argument_checks():
    L = _lib()
    P, na, w, tail_n = 300, 257, LAYOUTS["sh3_projected"], 12
    rng = np.random.default_rng(3500)
    ids = _ids(rng, P, na)
    pos = _pos(ids, P)
    n, lo = _sizes(P, na, w, tail_n)[1], _lo(na)
    x, p = _ints(rng, n), _ints(rng, n)
    fin = _hand_partials(rng, 16, 3 * KSUM)
    nine = (ctypes.c_int32 * 9)(*([1] * 9))
    bad = [dict(ngroups=0), dict(ngroups=9, widths=nine), dict(widths=_widths((3, 3, 3, 3, -4, 1))), dict(na=P + 1),
           dict(null="x"), dict(null="out"), dict(null="p"), dict(null="pos"), dict(tail_n=-1), dict(lo=-4),
           dict(fin=fin, fin_np=-1), dict(fin=fin, fin_slot=False)]
    for kw in bad:
        args = dict(na=na, tail_n=tail_n, lo=lo)
        args.update(kw)
        c = _End(x, p, pos, args.pop("na"), P, w, args.pop("tail_n"), args.pop("lo"), **args)
        assert c.status == L.GSLM_ERR_INVALID, kw
        assert bool(torch.isnan(c.outd[:-1]).all()) and c.guard[0] == GUARD and c.fin_value == -1.0, kw
    assert _End(x, p, pos, na, P, w, tail_n, lo, fin=fin).status == 0


# ------------------------------------------------------------------------------------------------ gslm_active_params
@functools.lru_cache(maxsize=None)
def nothing_visible():
    """200 Gaussians at the camera centre: all culled, an empty list."""
    from gslm.lm import LMProblem
    from gslm.model import synthetic_gaussians
    from test_gpu_cg_lean import _camera
    cam = _camera().to(DEV)
    model = synthetic_gaussians(200, 3, seed=0, s0=0.03).to(DEV)
    with torch.no_grad():
        model._xyz[:] = cam.camera_center.to(DEV).view(1, 3)
    prob = LMProblem(model, [cam], torch.zeros(3), device=DEV, sh_projection="auto")
    prob.evaluate()
    prob.rhs(prob.zeros())
    return prob, model


def _geometry(name):
    """(problem, model, P) of a scene by name; a forward and J^T b have run (the geometry and the row map exist)."""
    if name == "nothing_visible":
        prob, model = nothing_visible()
        return prob, model, 200
    s = scene() if name == "sh3_projected_2683" else layout_scene(name)
    return s.prob, s.model, s.prob.layout.P


LISTED = ["sh3_projected_2683", "all_listed_sh2_full", "short_list_sh3", "sh0"]
SENTINEL = 0xAB


def _active_params(prob, model, P, ids, na, short=0, gauss=None, n_arg=None):
    """gslm_active_params into a block of exactly the bytes it asks for (`short` fewer), sentinel bytes in it and
    behind it; -> (status, block, pos with a guard entry)."""
    from gslm.params import raw_gaussians
    L = _lib()
    vr = prob.views[0]
    nbytes = L.lib.gslm_active_params_bytes(na)
    block = torch.full((nbytes + 256,), SENTINEL, dtype=torch.uint8, device=DEV)
    pos = torch.full((P + 1,), -7, dtype=torch.int32, device=DEV)
    g = raw_gaussians(model) if gauss is None else gauss
    st = L.lib.gslm_active_params(ctypes.byref(g), vr.geom.data_ptr(), P, ids.data_ptr() if na else None,
                                  na if n_arg is None else n_arg, block.data_ptr(), nbytes - short, pos.data_ptr(),
                                  prob.stream)
    torch.cuda.synchronize()
    return st, block, pos


@pytest.mark.parametrize("name", LISTED)
def test_active_params_block(name):
    """The arrays are the leaves indexed by the list, the clamp word is the geometry's, pos inverts the list, each
    array starts at a multiple of 256 bytes; nothing is written behind the bytes asked for."""
    L = _lib()
    prob, model, P = _geometry(name)
    vr = prob.views[0]
    ids, na = vr.active_list(P, prob.stream)
    if name == "all_listed_sh2_full":
        assert na == P
    elif name == "short_list_sh3":
        assert 0 < na < 256
    st, block, pos = _active_params(prob, model, P, ids, na)
    assert st == 0
    nbytes = L.lib.gslm_active_params_bytes(na)
    assert block.data_ptr() % 256 == 0
    idx = ids.long()
    leaves = (model._xyz, model._scaling, model._rotation, model._opacity)
    o = 0
    for k, width in enumerate((3, 3, 4, 1, 1)):
        assert o % 256 == 0
        got = block[o:o + 4 * width * na].view(torch.int32).reshape(na, width)
        if k < 4:
            assert torch.equal(got, leaves[k].detach()[idx].reshape(na, width).view(torch.int32)), k
        else:
            flags = torch.zeros(P, dtype=torch.int32, device=DEV)
            L.check(L.lib.gslm_view_flags(vr.geom.data_ptr(), P, flags.data_ptr(), prob.stream))
            torch.cuda.synchronize()
            assert bool((flags[idx] < 0).all())  # (bit 31: touches a tile, as every listed Gaussian does)
            assert torch.equal(got.reshape(-1), flags[idx] & 7)
        o = (o + 4 * width * na + 255) // 256 * 256
    assert o == nbytes
    assert bool((block[nbytes:] == SENTINEL).all())
    want = torch.full((P + 1,), -1, dtype=torch.int32, device=DEV)
    want[idx] = torch.arange(na, dtype=torch.int32, device=DEV)
    want[P] = -7
    assert torch.equal(pos, want)
    assert (na == P) == (not bool((pos[:P] < 0).any()))
    # the solver's own block (ViewRaster.active_params) is this one
    blk, ps = vr.active_params(model, P, prob.stream)
    torch.cuda.synchronize()
    used = torch.ones(nbytes, dtype=torch.bool, device=DEV)  # (the padding between two arrays is never written)
    o = 0
    for width in (3, 3, 4, 1, 1):
        e = o + 4 * width * na
        o = (e + 255) // 256 * 256
        used[e:o] = False
    assert torch.equal(blk[:nbytes][used], block[:nbytes][used]) and torch.equal(ps[:P], pos[:P])


def test_active_params_empty_list():
    """Nothing visible: pos is all -1, the status OK, the block untouched."""
    prob, model, P = _geometry("nothing_visible")
    ids, na = prob.views[0].active_list(P, prob.stream)
    assert na == 0 and prob.active_view() is None
    st, block, pos = _active_params(prob, model, P, ids, 0)
    assert st == 0
    assert bool((block == SENTINEL).all())
    assert bool((pos[:P] == -1).all()) and pos[P].item() == -7


def test_active_params_argument_checks():
    from gslm.params import raw_gaussians
    L = _lib()
    prob, model, P = _geometry("short_list_sh3")
    ids, na = prob.views[0].active_list(P, prob.stream)
    cooked = raw_gaussians(model)
    cooked.raw = 0
    for want, kw in ((L.GSLM_ERR_CAPACITY, dict(short=1)), (L.GSLM_ERR_INVALID, dict(n_arg=P + 1)),
                     (L.GSLM_ERR_INVALID, dict(gauss=cooked))):
        st, block, pos = _active_params(prob, model, P, ids, na, **kw)
        assert st == want, kw
        assert bool((block == SENTINEL).all()) and bool((pos == -7).all()), kw


# ------------------------------------------------------------------------------------------------ GSLM_MV_LEAN
def _act(name):
    prob, model, P = _geometry(name)
    act = prob.active_view()
    assert act is not None
    return prob, model, P, act


def _int_vec(act, seed):
    """An integer-valued vector of the active view's layout (every group, the exposure tail included)."""
    return torch.from_numpy(_ints(np.random.default_rng(seed), act.layout.numel)).to(DEV)


def _unit_vec(act, seed):
    """A normal vector of the active view's layout with xyz and exposure zero, as every LM iterate."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    v = torch.randn(act.layout.numel, device=DEV, generator=gen)
    for grp in ("xyz", "exposure"):
        a, b = act.layout.offsets[grp]
        v[a:b] = 0
    return v


def _nan_like(v):
    return torch.full_like(v, math.nan)


def _sevens(v):
    """A product's y before the call (overwritten where the product writes)."""
    return torch.full_like(v, 7.0)


def _block_of(prob, model, P):
    block, _ = prob.views[0].active_params(model, P, prob.stream)
    return block


@pytest.mark.parametrize("name", LISTED)
def test_lean_params_block_gives_the_same_product(name):
    """y with the chains' parameters read from the list-order block is bitwise y with them read by id."""
    L = _lib()
    prob, model, P, act = _act(name)
    v = _unit_vec(act, 41)
    y0, y1 = _sevens(v), _sevens(v)
    act.local_normal_matvec(v, y0, damp=True)
    lean = L.GslmCgLean()
    lean.params = _block_of(prob, model, P).data_ptr()
    act.local_normal_matvec(v, y1, damp=True, lean=lean)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y0).all()) and bool((y0 != 7.0).any())
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))


@pytest.mark.parametrize("name", LISTED)
def test_lean_dot_defer_leaves_the_partials(name):
    """dot_defer: the ceil(na / 256) doubles in dot_scratch are bitwise the partials the finishing call leaves
    there, and their gslm_dot_finalize is bitwise its <v, y>."""
    L = _lib()
    prob, model, P, act = _act(name)
    na = act.layout.P
    npd = (na + 255) // 256
    v = _unit_vec(act, 42)
    y0, y1 = _sevens(v), _sevens(v)
    dot = _scalars(math.nan)
    act.dot_scratch.fill_(math.nan)
    act.local_normal_matvec(v, y0, damp=True, dot_out=dot.data_ptr())
    torch.cuda.synchronize()
    part0 = act.dot_scratch.clone()
    assert bool(torch.isfinite(part0[:npd]).all()) and math.isfinite(dot.item())
    act.dot_scratch.fill_(math.nan)
    lean = L.GslmCgLean()
    lean.dot_defer = 1
    act.local_normal_matvec(v, y1, damp=True, lean=lean)
    torch.cuda.synchronize()
    part1 = act.dot_scratch.clone()
    assert torch.equal(part1[:npd].view(torch.int64), part0[:npd].view(torch.int64))
    assert bool(torch.isnan(part1[npd:]).all())  # nothing written behind the partials
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    assert np.float64(_finalize(part1, npd)).view(np.int64) == np.float64(dot.item()).view(np.int64)


@pytest.mark.parametrize("beta_np", [1, 1024, 2049])
@pytest.mark.parametrize("name", LISTED)
def test_lean_beta_partials(name, beta_np):
    """beta = 3K / 4K with the numerator as beta_np partials, alpha = 3 / 2 finished, integer s, p, x: the tangent
    stage writes p = s + (3/4) p and x + (3/2) p exactly (the masked xyz group of p and x keeps its bits), stores the
    numerator's exact sum, and the product is bitwise the one of the call that is handed the finished numerator."""
    L = _lib()
    prob, model, P, act = _act(name)
    lay = act.layout
    s, p, x = (_int_vec(act, 50 + k) for k in range(3))
    part = _dev(_hand_partials(np.random.default_rng(60 + beta_np), beta_np, 3 * KSUM), 8, math.nan)
    a0, a1 = lay.offsets["xyz"]
    d = lambda t: t.double()
    p_ref = (d(s) + 0.75 * d(p)).float()
    x_ref = (d(x) + 1.5 * d(p)).float()
    p_ref[a0:a1], x_ref[a0:a1] = p[a0:a1], x[a0:a1]
    res = []
    for with_part in (False, True):
        sc = _scalars(math.nan if with_part else 3 * KSUM, 4 * KSUM, 3.0, 2.0, GUARD)
        pv, xv, y = p.clone(), x.clone(), _sevens(p)
        lean = None
        if with_part:
            lean = L.GslmCgLean()
            lean.beta_partials, lean.beta_np, lean.beta_store = part.data_ptr(), beta_np, _slot(sc, 0)
        act.local_normal_matvec(pv, y, damp=True, pre=(s, _slot(sc, 0), _slot(sc, 1), xv, _slot(sc, 2), _slot(sc, 3)),
                                lean=lean)
        torch.cuda.synchronize()
        assert sc.tolist() == [float(3 * KSUM), float(4 * KSUM), 3.0, 2.0, GUARD]
        assert torch.equal(pv.view(torch.int32), p_ref.view(torch.int32)), with_part
        assert torch.equal(xv.view(torch.int32), x_ref.view(torch.int32)), with_part
        assert bool(torch.isfinite(y).all()) and bool((y != 7.0).any())
        res.append(y)
    assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32))
    assert bool(torch.isnan(part[beta_np:]).all()) and part[:beta_np].sum().item() == float(3 * KSUM)


def _raw_product(pr, v, y, opts, lean, active=True):
    """gslm_matvec_view_active (or _ex) with the options of LMProblem.local_normal_matvec's one product, extended by
    `lean` (GSLM_MV_LEAN); -> status."""
    from gslm import lm
    from gslm.params import raw_gaussians
    L = _lib()
    vr = pr.views[0]
    g = raw_gaussians(pr.model)
    vs, ys = pr.layout.grads_struct(v), pr.layout.grads_struct(y)
    ext = L.GslmMatvecOptsLean()
    opts.stages = lm.STAGE_ALL | lm.STAGE_OVERWRITE
    opts.flags = lm.MV_TAIL_CLEAN | pr.mv_flags | lm.MV_LEAN
    opts.damp7 = pr._damps
    ctypes.memmove(ctypes.addressof(ext.base), ctypes.addressof(opts), ctypes.sizeof(opts))
    ext.lean = lean
    args = (ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(vs), pr.weights[0].data_ptr(), 1, vr.geom.data_ptr(),
            vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(), vr.scratch.numel(),
            ctypes.byref(ys), ctypes.byref(ext))
    if active:
        ids, na = pr._active
        st = L.lib.gslm_matvec_view_active(*args, ids.data_ptr(), vr.active_rows.data_ptr(), na, pr.stream)
    else:
        st = L.lib.gslm_matvec_view_ex(*args, pr.stream)
    torch.cuda.synchronize()
    return st


def test_lean_option_argument_checks():
    """Each refused before a launch: y, p and x keep their bits."""
    L = _lib()
    prob, model, P, act = _act("short_list_sh3")
    assert prob.views[0].tail_clean
    s, p0, x0 = (_int_vec(act, 70 + k) for k in range(3))
    sc = _scalars(3.0, 4.0, 3.0, 2.0)
    other = _dev(_hand_partials(np.random.default_rng(71), 16, 3 * KSUM), 8, math.nan)
    scratch = act.dot_scratch

    def options(xpby, dot_vy=False, dot_scratch=False):
        o = L.GslmMatvecOpts()
        keep = None
        if xpby:
            keep = act._pre_opts(o, p, (s, _slot(sc, 0), _slot(sc, 1), x, _slot(sc, 2), _slot(sc, 3)))
        if dot_vy:
            o.dot_vy = dot.data_ptr()
        if dot_vy or dot_scratch:
            o.dot_scratch, o.dot_scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
        return o, keep

    def lean_of(**kw):
        le = L.GslmCgLean()
        for k, val in kw.items():
            setattr(le, k, val)
        return le

    cases = [
        ("MV_LEAN on gslm_matvec_view_ex", False, dict(xpby=False), dict()),
        ("dot_defer with dot_vy", True, dict(xpby=False, dot_vy=True), dict(dot_defer=1)),
        ("beta_partials == dot_scratch", True, dict(xpby=True, dot_scratch=True),
         dict(dot_defer=1, beta_partials=scratch.data_ptr(), beta_np=16)),
        ("beta_partials without xpby_s", True, dict(xpby=False), dict(beta_partials=other.data_ptr(), beta_np=16)),
        ("negative beta_np", True, dict(xpby=True), dict(beta_partials=other.data_ptr(), beta_np=-1)),
    ]
    for what, active, okw, lkw in cases:
        pr = act if active else prob
        p = p0.clone() if active else torch.from_numpy(_ints(np.random.default_rng(72), prob.layout.numel)).to(DEV)
        x, y, dot = x0.clone(), _nan_like(p), _scalars(-1.0)
        o, keep = options(**okw)
        st = _raw_product(pr, p, y, o, lean_of(**lkw), active)
        assert st == L.GSLM_ERR_INVALID, what
        assert bool(torch.isnan(y).all()) and dot.item() == -1.0, what
        if active:
            assert torch.equal(p, p0) and torch.equal(x, x0), what
    # the accepted form of the same call
    p, x, y = p0.clone(), x0.clone(), _sevens(p0)
    o, keep = options(xpby=True, dot_scratch=True)
    assert _raw_product(act, p, y, o, lean_of(dot_defer=1, beta_partials=other.data_ptr(), beta_np=16)) == 0
    assert bool(torch.isfinite(y).all()) and bool((y != 7.0).any()) and not torch.equal(p, p0)
