"""Device self-tests of the three binning primitives behind every image and every LM product, each against a numpy
restatement on the host and exact (integer kernels: every comparison is array_equal):

  gslm_selftest_sort        radix_sort_pairs (csrc/sort.hip): the tile sort, the depth sort (key_range), the union
                            binning's payload sort, the k-NN cell sort
  gslm_selftest_ranges      k_ranges (csrc/forward.hip): the per-tile [start, end) of the sorted list
  gslm_selftest_tile_order  k_tile_order / k_tile_order_xcd (csrc/forward.hip): the tile passes' launch order

The entry points are thin wrappers of the launchers the renders use, so the geometry tested is the shipped one.  Every
buffer a kernel may write is followed by guard words holding a sentinel, checked after the call.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5  # prefill of every output buffer and guard
GUARD = 64         # guard words behind each buffer
U32 = np.uint32


def _lib():
    from gslm import _lib
    return _lib


def _dev(a):
    """host uint32 array -> device tensor (int32 storage, same bits)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U32).view(np.int32).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(U32)


def _buf(n, init=None):
    """n words (init, or the sentinel) followed by the guard"""
    a = np.full(n + GUARD, SENT, U32)
    if init is not None:
        a[:n] = init
    return _dev(a)


def _ptr(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=6)
def _rand(n, seed):
    """n random words, shared between the cases that use the same (n, seed) and never written"""
    a = np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U32)
    a.setflags(write=False)
    return a


def _distinct(n):
    """n distinct words in no particular order (an odd multiplier is a bijection of the 32-bit words)"""
    return (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(U32)


# ------------------------------------------------------------------------------------------------------------ sort

def _call_sort(k0, v0, k1, v1, p0, p1, n, end_bit, iota, key_range, gather, n_dev, hist, hist_bytes):
    L = _lib()
    alt = ctypes.c_int32(-1)
    st = L.lib.gslm_selftest_sort(_ptr(k0), _ptr(v0), _ptr(k1), _ptr(v1), _ptr(p0), _ptr(p1), n, end_bit, int(iota),
                                  int(key_range), _ptr(gather), _ptr(n_dev), _ptr(hist), hist_bytes, ctypes.byref(alt),
                                  L.stream_handle())
    torch.cuda.synchronize()
    return st, alt.value


def _sort_case(keys, vals, end_bit, pay=None, iota=False, key_range=False, gather=None, n_dev=None):
    """Runs one sort and checks all of its outputs against numpy's stable argsort of the masked keys; returns the
    histogram workspace (host words) and its block count.  vals with iota: what v0 is filled with (never read)."""
    L = _lib()
    n = keys.size
    # with a gather table every value word a wrong sort could pick up (an unwritten slot's prefill, v0 under
    # iota_values) is a valid index: it then fails the comparisons below instead of reading outside the table
    vfill = np.full(n, SENT if gather is None else SENT % n, U32)
    assert gather is None or int(vals.max()) < n
    k0, v0, k1, v1 = _buf(n, keys), _buf(n, vals), _buf(n), _buf(n, vfill)
    p0, p1 = (_buf(n, pay), _buf(n)) if pay is not None else (None, None)
    hb = L.lib.gslm_selftest_sort_hist_bytes(n, int(pay is not None))
    assert hb % 8 == 0
    hist = _buf(hb // 4)
    g = None if gather is None else _dev(gather)
    nd = None if n_dev is None else _dev(np.array([n_dev], U32))
    st, alt = _call_sort(k0, v0, k1, v1, p0, p1, n, end_bit, iota, key_range, g, nd, hist, hb)
    L.check(st, "gslm_selftest_sort")

    c = n if n_dev is None else min(n, n_dev)
    mask = U32(0xFFFFFFFF if end_bit == 32 else (1 << end_bit) - 1)
    order = np.argsort(keys[:c] & mask, kind="stable")
    exp_v = order.astype(U32) if iota else vals[:c][order]
    exp_k = gather[exp_v] if gather is not None else keys[:c][order]
    passes = (end_bit + 7) // 8
    assert alt == passes % 2, (alt, passes)

    sent = np.full(n, SENT, U32)
    before = {"k0": keys, "v0": vals, "k1": sent, "v1": vfill, "p0": pay, "p1": sent}
    got = {"k0": _host(k0), "v0": _host(v0), "k1": _host(k1), "v1": _host(v1)}
    if pay is not None:
        got["p0"], got["p1"] = _host(p0), _host(p1)
    for name, a in got.items():
        assert np.array_equal(a[n:], np.full(GUARD, SENT, U32)), f"guard behind {name}"
        # nothing at or past the device count is ever written: the other buffer of a pair keeps its prefill there too
        assert np.array_equal(a[c:n], before[name][c:]), f"{name} written past the count"
    res = "1" if alt else "0"
    assert np.array_equal(got["v" + res][:c], exp_v), "values"
    assert np.array_equal(got["k" + res][:c], exp_k), "keys"
    if pay is not None:
        assert np.array_equal(got["p" + res][:c], pay[:c][order]), "payload"
    h = _host(hist)
    assert np.array_equal(h[hb // 4:], np.full(GUARD, SENT, U32)), "guard behind hist"
    if gather is not None:
        assert np.array_equal(_host(g), gather), "gather table written"
    return h[:hb // 4], (hb - 1040) // 1032


@pytest.mark.parametrize("end_bit", [1, 2, 7, 8, 9, 13, 15, 16, 17, 24, 25, 32])
def test_sort_bit_splits(end_bit):
    """Every pass count and odd split (digits of ceil(end_bit / passes) bits, the last one the rest: 9 = 5 + 4,
    17 = 6 + 6 + 5, 25 = 7 + 7 + 7 + 4): the sort is on bits [0, end_bit) alone, and the random bits above travel with
    their key.  The workspace's digit totals of the last pass (include/gslm.h) show the split itself: 13 bits end on a
    6-bit digit from bit 7, not a 5-bit one from bit 8."""
    n = 20_011
    keys, vals = _rand(n, 100 + end_bit), _rand(n, 200 + end_bit)
    hist, nb = _sort_case(keys, vals, end_bit)
    passes = (end_bit + 7) // 8
    per = -(-end_bit // passes)
    shift = per * (passes - 1)
    digits = (keys >> U32(shift)) & U32((1 << (end_bit - shift)) - 1)
    assert np.array_equal(hist[256 * nb:256 * nb + 256], np.bincount(digits, minlength=256).astype(U32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4_190_208, 4_190_209, 8_388_609])
def test_sort_sizes(n):
    """13-bit tile ids around the 64-key round, the wave quarter and the block of 2048; the switch to 16 keys per thread
    at 1023 * 4096 + 1 (2046 blocks of 2048 below it, 1024 blocks of 4096 with one key in the last at it); and 2049
    blocks of 4096, the second chunk of 2048 block counts in k_radix_scan."""
    _sort_case(_rand(n, 1), _rand(n, 2), 13)


@pytest.mark.parametrize("n", [2049, 4_190_209])
@pytest.mark.parametrize("pattern", ["equal", "alternating", "descending", "four"])
def test_sort_stability(n, pattern):
    """Equal digits across the 64-key rounds, the waves' quarters and the blocks keep their input order (the tile sort
    sorts on the tile id alone over a depth-ordered list).  The values are distinct, so any swap shows."""
    end_bit = 13
    if pattern == "equal":
        keys = np.full(n, 0x1ABC, U32)
    elif pattern == "alternating":  # two keys that differ in both digits of the 7 + 6 split
        keys = np.where(np.arange(n) & 1, U32(5), U32(4099)).astype(U32)
    elif pattern == "descending":   # strictly descending: three passes, and the whole list reversed across blocks
        keys, end_bit = np.arange(n - 1, -1, -1, dtype=U32), 24
    else:
        keys = np.array([0, 127, 128, 8191], U32)[_rand(n, 7) & U32(3)]
    vals = _distinct(n)
    _sort_case(keys, vals, end_bit)
    if pattern == "equal":  # (what _sort_case checked: the identity)
        assert np.array_equal(np.argsort(keys, kind="stable"), np.arange(n))


@pytest.mark.parametrize("n", [2049, 300_007])
@pytest.mark.parametrize("end_bit", [8, 13, 32])
@pytest.mark.parametrize("form", ["iota", "gather", "iota+gather"])
def test_sort_iota_values_and_last_gather(n, end_bit, form):
    """iota_values: the values are the indices and v0, filled with garbage here, is not read.  last_gather: the last
    pass leaves table[value] in each key slot (values a permutation of [0, n)); both together are the depth sort's
    form."""
    keys = _rand(n, 11)
    iota = "iota" in form
    vals = _rand(n, 12) % U32(n) if iota else np.random.default_rng(13).permutation(n).astype(U32)
    _sort_case(keys, vals, end_bit, iota=iota, gather=_rand(n, 14) if "gather" in form else None)


@pytest.mark.parametrize("n", [1, 2049, 300_007, 4_194_305])
@pytest.mark.parametrize("end_bit", [5, 13, 17])
def test_sort_payload(n, end_bit):
    """A payload word per pair (the union binning's set masks): blocks of 2048 at every size, so 4,194,305 pairs are
    2049 blocks (k_radix_scan's second chunk in the payload form); one, two and three passes."""
    _sort_case(_rand(n, 21), _rand(n, 22), end_bit, pay=_rand(n, 23))


@pytest.mark.parametrize("n,end_bit", [(5000, 5), (5000, 13), (4_190_209, 13)])
@pytest.mark.parametrize("count", [0, 1, 2048, 2049, "n-1", "n", "n+7"])
def test_sort_device_count(n, end_bit, count):
    """n a capacity, the count on the device: the first min(n, count) pairs are sorted and no buffer is written past
    them, at the small sizes and with 16 keys per thread."""
    count = {"n-1": n - 1, "n": n, "n+7": n + 7}.get(count, count)
    _sort_case(_rand(n, 31), _rand(n, 32), end_bit, n_dev=count)


def _range_keys(n, kmin, hi, frac, seed):
    """n keys in [kmin, hi] holding both ends (n >= 2; n == 1: kmin), a fraction of them then set to 0xFFFFFFFF"""
    rng = np.random.default_rng(seed)
    keys = (U32(kmin) + rng.integers(0, hi - kmin + 1, size=n, dtype=np.uint64).astype(U32)).astype(U32)
    keys[0] = kmin
    if n >= 2:
        keys[n // 2] = hi
    if frac >= 1.0:
        keys[:] = 0xFFFFFFFF
    elif frac > 0.0:
        keys[rng.random(n) < frac] = 0xFFFFFFFF
        if n >= 3:  # the ends stay
            keys[0], keys[n // 2] = kmin, hi
    return keys


@pytest.mark.parametrize("span", [0, 254, 255, 256, 65_535, 65_536, (1 << 24) - 1, 1 << 24])
@pytest.mark.parametrize("low", [0x00, 0x01, 0xFF])
def test_sort_key_range_spans(span, low):
    """The depth sort's form: spans that end on and just past each byte boundary, with a minimum whose low byte rotates
    pass 0's digits (or not), a tenth of the keys 0xFFFFFFFF.  The output is the plain 32-bit sort's."""
    kmin = 0x3F80_0000 + low
    keys = _range_keys(2049, kmin, kmin + span, 0.1, span % 1000 + low)
    _sort_case(keys, _rand(2049, 41), 32, iota=True, key_range=True)


@pytest.mark.parametrize("n", [1, 2049, 100_003])
@pytest.mark.parametrize("frac", [0.0, 0.1, 1.0])
def test_sort_key_range_sentinels(n, frac):
    """No, some and only 0xFFFFFFFF keys (frac 1: the all-0xFFFFFFFF list), one block and many."""
    keys = _range_keys(n, 0x3F80_0001, 0x3F81_0001, frac, n)
    _sort_case(keys, _rand(n, 42), 32, iota=True, key_range=True)


@pytest.mark.parametrize("kmin", [0, 1])
@pytest.mark.parametrize("frac", [0.0, 0.1])
def test_sort_key_range_full_width(kmin, frac):
    """Keys up to 0xFFFFFFFE from 0 and from 1: the 0xFFFFFFFF keys' sort value is the last one left."""
    keys = _range_keys(2049, kmin, 0xFFFFFFFE, frac, 50 + kmin)
    _sort_case(keys, _rand(2049, 43), 32, iota=True, key_range=True)


def test_sort_key_range_one_valid_key():
    keys = np.full(2049, 0xFFFFFFFF, U32)
    keys[1500] = 0x4012_3456
    _sort_case(keys, _rand(2049, 44), 32, iota=True, key_range=True)


@pytest.mark.parametrize("span", [0, 255, 65_536, 1 << 24])
@pytest.mark.parametrize("iota", [True, False])
def test_sort_key_range_last_gather(span, iota):
    """One to four working passes, the rest copies: the last pass gathers whether it sorts or copies.  Without
    iota_values the values come from v0 (a permutation here, the gather's indices)."""
    n = 100_003
    keys = _range_keys(n, 0x3F80_00FF, 0x3F80_00FF + span, 0.1, span % 1000)
    vals = _rand(n, 45) % U32(n) if iota else np.random.default_rng(46).permutation(n).astype(U32)
    _sort_case(keys, vals, 32, iota=iota, key_range=True, gather=_rand(n, 47))


def test_sort_argument_checks_launch_nothing():
    """Every refusal of gslm_selftest_sort, and the library's own of key_range beside a payload, a device count or fewer
    than 32 bits, with real buffers: the status, and no word of any buffer or guard changed."""
    L = _lib()
    INV, CAP = L.GSLM_ERR_INVALID, L.GSLM_ERR_CAPACITY
    n = 5000
    hb = L.lib.gslm_selftest_sort_hist_bytes(n, 1)
    assert hb >= L.lib.gslm_selftest_sort_hist_bytes(n, 0)
    names = ("k0", "v0", "k1", "v1", "p0", "p1", "hist", "gather", "n_dev")
    init = {"k0": _rand(n, 61), "v0": _rand(n, 62), "p0": _rand(n, 63), "gather": _rand(n, 64)}
    size = {"hist": hb // 4, "n_dev": 1}
    bufs = {k: _buf(size.get(k, n), init.get(k)) for k in names}
    snap = {k: _host(t).copy() for k, t in bufs.items()}

    def call(n=n, end_bit=13, iota=0, key_range=0, hist_bytes=hb, use=("k0", "v0", "k1", "v1", "hist")):
        a = {k: (bufs[k] if k in use else None) for k in names}
        return _call_sort(a["k0"], a["v0"], a["k1"], a["v1"], a["p0"], a["p1"], n, end_bit, iota, key_range,
                          a["gather"], a["n_dev"], a["hist"], hist_bytes)[0]

    base = ("k0", "v0", "k1", "v1", "hist")
    assert call(n=-1) == INV
    for end_bit in (0, 33, -5):
        assert call(end_bit=end_bit) == INV
    for drop in base:
        assert call(use=tuple(k for k in base if k != drop)) == INV, drop
    assert call(use=("k0", "k1", "hist"), iota=1) == INV  # iota_values spares v0, not v1
    assert call(use=base + ("p0",)) == INV
    assert call(use=base + ("p1",)) == INV
    assert call(hist_bytes=L.lib.gslm_selftest_sort_hist_bytes(n, 0) - 1) == CAP
    assert call(use=base + ("p0", "p1"), hist_bytes=hb - 1) == CAP
    assert call(end_bit=32, key_range=1, use=base + ("p0", "p1")) == INV
    assert b"key_range" in L.lib.gslm_last_error()
    assert call(end_bit=32, key_range=1, use=base + ("n_dev",)) == INV
    assert call(end_bit=24, key_range=1) == INV
    assert call(end_bit=24, key_range=1, iota=1, use=base + ("gather",)) == INV
    for k, t in bufs.items():
        assert np.array_equal(_host(t), snap[k]), k


# ---------------------------------------------------------------------------------------------------------- ranges

def _ranges_ref(keys, ntiles):
    ref = np.zeros((ntiles, 2), U32)
    present = np.unique(keys)
    ref[present, 0] = np.searchsorted(keys, present, side="left")
    ref[present, 1] = np.searchsorted(keys, present, side="right")
    return ref


def _ranges_case(keys_buf, n, ntiles, count=None):
    """keys_buf: the n keys and GUARD more words behind them (read by a kernel that looks past the list's end, so the
    caller picks them to make that show).  count: the device count form."""
    L = _lib()
    kd = _dev(keys_buf)
    out = _buf(2 * ntiles)
    nd = None if count is None else _dev(np.array([count], U32))
    no = None if count is None else _buf(1)
    L.check(L.lib.gslm_selftest_ranges(kd.data_ptr(), n, ntiles, _ptr(nd), _ptr(no), out.data_ptr(), L.stream_handle()),
            "gslm_selftest_ranges")
    torch.cuda.synchronize()
    c = n if count is None else min(n, count)
    got = _host(out)
    assert np.array_equal(got[2 * ntiles:], np.full(GUARD, SENT, U32)), "guard behind ranges"
    assert np.array_equal(got[:2 * ntiles].reshape(ntiles, 2), _ranges_ref(keys_buf[:c], ntiles))
    assert np.array_equal(_host(kd), keys_buf)
    if count is not None:
        h = _host(no)
        assert h[0] == count  # the device count itself, not capped at the capacity
        assert np.array_equal(h[1:], np.full(GUARD, SENT, U32))


def _ranges_keys(n, pattern):
    """(sorted tile ids [n], ntiles)"""
    if pattern == "gaps":  # 60 tiles, about a third of them absent (the first and the last too)
        ids = np.sort(np.random.default_rng(n).choice(np.arange(1, 59), size=40, replace=False))
        return np.sort(ids[np.random.default_rng(n + 1).integers(0, 40, size=n)]).astype(U32), 60
    if pattern == "one":
        return np.full(n, 17, U32), 23
    if pattern == "distinct":
        return (3 * np.arange(n) + 1).astype(U32), 3 * n + 2
    # run boundaries just before, on and just after the 4-key groups' edges, at the groups of a block's first and last
    # threads and the next block's first (1024 keys per block)
    cuts = sorted({4 * k + d for k in (1, 2, 5, 64, 255, 256, 257) for d in (-1, 0, 1)} | {2048})
    keys = 2 * np.searchsorted(np.array(cuts), np.arange(n), side="right")
    return keys.astype(U32), 2 * len(cuts) + 2


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 100_003])
@pytest.mark.parametrize("pattern", ["gaps", "one", "distinct", "boundaries"])
def test_ranges(n, pattern):
    """k_ranges' 16-byte loads, ragged tail and neighbour reads at every list length around the 4-key group and the
    1024-key block.  The words behind the list repeat its last key, so a read past the end would swallow the last
    run's end."""
    keys, ntiles = _ranges_keys(n, pattern)
    _ranges_case(np.concatenate([keys, np.full(GUARD, keys[-1], U32)]), n, ntiles)


@pytest.mark.parametrize("n", [1025, 100_003])
@pytest.mark.parametrize("pattern", ["gaps", "boundaries"])
@pytest.mark.parametrize("count", ["mid4", "mid", "n", "n+7", 0])
def test_ranges_device_count(n, pattern, count):
    """The count on the device: below n it cuts a run in the middle (at a multiple of 4 and not), and the keys past it
    are not part of the list -- here the cut run goes on for one more key, then random tile ids; n_out receives the
    count itself."""
    keys, ntiles = _ranges_keys(n, pattern)
    keys = np.concatenate([keys, np.full(GUARD, keys[-1], U32)])
    if count in ("mid4", "mid"):
        # a position inside a run (the key before and the key at it equal), from the middle of the list on
        inside = np.flatnonzero(keys[1:n] == keys[:n - 1]) + 1
        inside = inside[(inside >= n // 2) & ((inside % 4 == 0) == (count == "mid4"))]
        count = int(inside[0])
        keys[count + 1:n] = np.random.default_rng(5).integers(0, ntiles, size=n - count - 1)
    else:
        count = {"n": n, "n+7": n + 7}.get(count, count)
    _ranges_case(keys, n, ntiles, count)


# ------------------------------------------------------------------------------------------------------ tile order

def _bucket(n):
    """k_tile_order's bucket of a list length, restated: heaviest first, exact below 768, 32 wide above, saturating"""
    n = n.astype(np.int64)
    return 1023 - np.where(n < 768, n, np.minimum(1023, 768 + ((n - 768) >> 5)))


def _bands(lens):
    """k_tile_order_xcd's band of each tile, restated in Python integers"""
    wt = [int(x) + 1 for x in lens]
    total = sum(wt)
    out, pre = [], 0
    for w in wt:
        out.append(min(7, ((2 * pre + w) * 8) // (2 * total)))
        pre += w
    return np.array(out)


def _tile_lengths(ntiles, pattern):
    rng = np.random.default_rng(ntiles)
    lens = np.zeros(ntiles, np.int64)
    if pattern == "heavy":  # one heavy tile in an empty frame
        lens[ntiles // 2] = 20_000
    elif pattern == "random":  # mostly exact buckets, a tail in the 32-wide ones and one past 8928 (saturated)
        lens = rng.integers(0, 768, size=ntiles)
        tail = rng.random(ntiles)
        lens = np.where(tail < 0.10, rng.integers(768, 8928, size=ntiles), lens)
        lens = np.where(tail < 0.03, rng.integers(8928, 20_000, size=ntiles), lens)
        lens[0], lens[-1] = 8927, 8928
    elif pattern == "firstrow":  # all weight in the first tiles: the later bands come out empty or unequal
        lens[:max(1, ntiles // 100)] = 5000
    return lens


@pytest.mark.parametrize("ntiles", [1, 7, 8, 9, 1023, 1024, 1025, 8160, 32_400])
@pytest.mark.parametrize("pattern", ["zero", "heavy", "random", "firstrow"])
def test_tile_order(ntiles, pattern):
    """Both forms of the launch order, from list ranges and from a cost array: a permutation of the tiles (a dropped or
    doubled tile is a hole in the image), heaviest bucket first -- frame-wide in form 0; in form 1 inside each of the 8
    bands, which are dealt round-robin while every band has a tile left, the leftovers following band by band.  Above
    1024 tiles each thread walks a run of tiles.  The order inside a bucket is arbitrary (atomics), so properties."""
    L = _lib()
    lens = _tile_lengths(ntiles, pattern)
    starts = np.cumsum(lens) - lens
    ranges = _dev(np.stack([starts, starts + lens], axis=1).astype(U32).reshape(-1))
    cost = _dev(lens.astype(U32))
    bucket, band = _bucket(lens), _bands(lens)
    for form in (0, 1):
        for given in ("ranges", "cost"):
            out = _buf(ntiles)
            L.check(L.lib.gslm_selftest_tile_order(ranges.data_ptr() if given == "ranges" else None,
                                                   cost.data_ptr() if given == "cost" else None, ntiles, form,
                                                   out.data_ptr(), L.stream_handle()), "gslm_selftest_tile_order")
            torch.cuda.synchronize()
            got = _host(out)
            assert np.array_equal(got[ntiles:], np.full(GUARD, SENT, U32)), "guard behind order"
            order = got[:ntiles].astype(np.int64)
            assert np.array_equal(np.sort(order), np.arange(ntiles)), (form, given, "not a permutation")
            if form == 0:
                assert np.all(np.diff(bucket[order]) >= 0), (given, "bucket order")
                continue
            m = int(np.bincount(band, minlength=8).min())
            assert np.array_equal(band[order[:8 * m]], np.arange(8 * m) % 8), (given, "round-robin part")
            left = order[8 * m:]
            assert np.all(np.diff(band[left]) >= 0), (given, "leftovers band by band")
            for g in range(8):
                seq = np.concatenate([order[g:8 * m:8], left[band[left] == g]])
                assert np.all(np.diff(bucket[seq]) >= 0), (given, g, "bucket order inside the band")


def test_ranges_and_tile_order_argument_checks_launch_nothing():
    L = _lib()
    INV = L.GSLM_ERR_INVALID
    keys, out, cnt = _buf(100, np.zeros(100, U32)), _buf(24), _buf(1, np.array([5], U32))
    snap = [_host(t).copy() for t in (keys, out, cnt)]
    h = L.stream_handle()
    k, o, c = keys.data_ptr(), out.data_ptr(), cnt.data_ptr()
    rg, to = L.lib.gslm_selftest_ranges, L.lib.gslm_selftest_tile_order
    assert rg(k, -1, 12, None, None, o, h) == INV
    assert rg(k, 100, 0, None, None, o, h) == INV
    assert rg(None, 100, 12, None, None, o, h) == INV
    assert rg(k, 100, 12, None, None, None, h) == INV
    assert rg(k, 100, 12, None, c, o, h) == INV  # n_out without n_dev
    assert rg(k + 4, 96, 12, None, None, o, h) == INV  # the 16-byte loads
    assert to(k, None, 0, 0, o, h) == INV
    assert to(k, None, 12, 2, o, h) == INV
    assert to(k, None, 12, 0, None, h) == INV
    assert to(None, None, 12, 1, o, h) == INV
    torch.cuda.synchronize()
    for t, s in zip((keys, out, cnt), snap):
        assert np.array_equal(_host(t), s)
