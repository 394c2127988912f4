"""gslm_num_rendered_many: the pair counts of n preprocessed geometries from one read-back.

A kernel writes the counts into a pinned array of the calling host thread, 32 geometries per launch, the array grown on
demand.  gslm.lm never passes more than 8 geometries, so the second chunk's offset, a short last chunk, the growth, a
call below the capacity, the first allocation of a new host thread and a non-default stream run only here.  Seven small
scenes with pairwise distinct counts are cycled through the argument arrays (32 mod 7 != 0: a chunk written at the
wrong offset, or read from the wrong geometry, changes a value), and every element must equal gslm_num_rendered of the
same geometry.
"""
import ctypes
import threading

import pytest
import torch

from gslm.cameras import orbit_cameras
from gslm.model import synthetic_gaussians
from oracle import torch_raster as tr

pytestmark = pytest.mark.gpu

# (P, model seed, camera seed): seven different sizes in 200..900
SCENES = [(211, 0, 1), (307, 1, 2), (419, 2, 3), (523, 3, 4), (641, 4, 5), (757, 5, 6), (887, 6, 7)]
W, H, S0 = 64, 48, 0.05


def _oracle_count(P, seed, cam_seed):
    m = synthetic_gaussians(P, 0, seed=seed, s0=S0)
    cam = orbit_cameras(1, W, H, seed=cam_seed)[0]
    st = tr.settings_from_camera(cam, torch.zeros(3), 0)
    with torch.no_grad():
        pre = tr.preprocess(m.get_xyz, torch.zeros_like(m.get_xyz), m.get_opacity, m.get_features, None,
                            m.get_scaling, m.get_rotation, None, st)
    return int(pre["tiles_touched"].sum())


@pytest.fixture(scope="module")
def geoms():
    """The seven preprocessed geometries: (device buffers kept alive, addresses, Ps, gslm_num_rendered of each)."""
    from gslm import _lib
    from gslm.params import raw_gaussians
    lib = _lib.lib
    oracle = [_oracle_count(*s) for s in SCENES]
    assert all(c > 0 for c in oracle) and len(set(oracle)) == len(oracle), oracle
    keep, addr, Ps, single = [], [], [], []
    for P, seed, cam_seed in SCENES:
        m = synthetic_gaussians(P, 0, seed=seed, s0=S0).to("cuda")
        g = raw_gaussians(m)
        view = _lib.view_from_camera(orbit_cameras(1, W, H, seed=cam_seed)[0], torch.zeros(3), 0)
        nb = lib.gslm_geom_bytes(P)
        buf = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        _lib.check(lib.gslm_preprocess(ctypes.byref(view), ctypes.byref(g), buf.data_ptr(), nb, None,
                                       _lib.stream_handle()), "gslm_preprocess")
        n = ctypes.c_int64(-1)
        _lib.check(lib.gslm_num_rendered(buf.data_ptr(), P, ctypes.byref(n), _lib.stream_handle()))
        keep.append((m, buf))
        addr.append(buf.data_ptr())
        Ps.append(P)
        single.append(int(n.value))
    # the device's own counts are what the cycled arrays are checked against; they too must tell the scenes apart
    assert all(c > 0 for c in single) and len(set(single)) == len(single), single
    return keep, addr, Ps, single


def _many(geoms, n, stream=None, sentinel=-7):
    """gslm_num_rendered_many over the first n entries of the cycled arrays -> (status, out list with one spare)."""
    from gslm import _lib
    _, addr, Ps, _ = geoms
    k = len(addr)
    ga = (ctypes.c_void_p * max(n, 1))(*[addr[i % k] for i in range(n)])
    pa = (ctypes.c_int64 * max(n, 1))(*[Ps[i % k] for i in range(n)])
    out = (ctypes.c_int64 * (max(n, 0) + 1))(*([sentinel] * (max(n, 0) + 1)))
    st = _lib.lib.gslm_num_rendered_many(ga, pa, n, out, _lib.stream_handle() if stream is None else stream)
    return st, list(out)


def _expect(geoms, n, sentinel=-7):
    single = geoms[3]
    return [single[i % len(single)] for i in range(n)] + [sentinel]


def test_chunks_growth_and_reuse_on_one_thread(geoms):
    """1 (first allocation), 31 / 32 / 33 (a full chunk and one element past it), 64 / 70 (two full chunks; a short
    third), 100 (the pinned array grows again), then 5 (well below the capacity), in this order on one thread."""
    def run():
        for n in (1, 31, 32, 33, 64, 70, 100, 5):
            st, out = _many(geoms, n)
            assert st == 0, n
            assert out == _expect(geoms, n), n

    # a thread of its own, so the order of the allocations does not depend on which tests ran before
    err = []
    t = threading.Thread(target=lambda: _guard(run, err))
    t.start()
    t.join()
    assert not err, err[0]


def _guard(fn, err):
    try:
        fn()
    except BaseException as e:  # noqa: BLE001 (reported by the test's own thread)
        err.append(e)


def test_first_call_of_a_fresh_thread_spans_two_chunks(geoms):
    err = []

    def run():
        st, out = _many(geoms, 33)
        assert st == 0
        assert out == _expect(geoms, 33)

    t = threading.Thread(target=lambda: _guard(run, err))
    t.start()
    t.join()
    assert not err, err[0]


def test_non_default_stream(geoms):
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    st, out = _many(geoms, 40, stream=s.cuda_stream)
    assert st == 0
    assert out == _expect(geoms, 40)


def test_argument_checks(geoms):
    from gslm import _lib
    lib = _lib.lib
    st, out = _many(geoms, 0)
    assert st == 0 and out == [-7]
    st, out = _many(geoms, -1)
    assert st == _lib.GSLM_ERR_INVALID and out == [-7]
    _, addr, Ps, _ = geoms
    ga = (ctypes.c_void_p * 2)(*addr[:2])
    pa = (ctypes.c_int64 * 2)(*Ps[:2])
    out = (ctypes.c_int64 * 2)(-7, -7)
    h = _lib.stream_handle()
    assert lib.gslm_num_rendered_many(None, pa, 2, out, h) == _lib.GSLM_ERR_INVALID
    assert lib.gslm_num_rendered_many(ga, None, 2, out, h) == _lib.GSLM_ERR_INVALID
    assert lib.gslm_num_rendered_many(ga, pa, 2, None, h) == _lib.GSLM_ERR_INVALID
    assert list(out) == [-7, -7]
    assert lib.gslm_num_rendered_many(None, None, 0, None, h) == 0
