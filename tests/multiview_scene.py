"""The multi-view scenes of tests/test_gpu_gather_views.py: the recipe of tests/test_gpu_dist.py (seeded synthetic
Gaussians in [-1, 1]^3, orbit cameras at 96 x 72) with the last three Gaussians moved so that, whatever the seeded
draw gives at a small P, the per-Gaussian kernels meet a Gaussian no view sees, one every view sees and (from two
views on) one that some views see and others do not.  The choice is made and checked on the CPU oracle's preprocess
(oracle/torch_raster.py); the GPU tests assert the same three conditions again from the library's own tile counts."""
import functools
import math

import numpy as np
import torch

from gslm.cameras import Camera, look_at, orbit_cameras
from gslm.model import synthetic_gaussians
from oracle import torch_raster as tr
from scenes import activated, oracle_settings

W, H = 96, 72


def tiles_touched(model, cams, rows=None):
    """[len(cams), P] tile counts of the CPU oracle's preprocess (rows: of these Gaussians only)."""
    a = activated(model)
    if rows is not None:
        a = {k: v[rows] for k, v in a.items()}
    out = []
    for c in cams:
        st = oracle_settings(c, model.active_sh_degree)
        with torch.no_grad():
            pre = tr.preprocess(a["means3D"], torch.zeros_like(a["means3D"]), a["opacities"], a["shs"], None,
                                a["scales"], a["rotations"], None, st)
        out.append(pre["tiles_touched"])
    return torch.stack(out)


def visibility_classes(T):
    """(none, some, all): how many Gaussians touch a tile in no view, in some but not all, in every view."""
    n = (T > 0).sum(0)
    V = T.shape[0]
    return int((n == 0).sum()), int(((n > 0) & (n < V)).sum()), int((n == V).sum())


def empty_camera():
    """A camera outside the scene looking away from it: every Gaussian lies behind it (num_rendered == 0)."""
    R, T = look_at((50.0, 0.0, 0.0), target=(100.0, 0.0, 0.0))
    fovx = math.radians(60.0)
    fovy = 2 * math.atan(H / (2 * (W / (2 * math.tan(fovx / 2)))))
    return Camera(R, T, fovx, fovy, image=torch.rand(3, H, W, generator=torch.Generator().manual_seed(77)), uid=99)


@functools.lru_cache(maxsize=None)
def scene(P, nv, D):
    """(model, cams) on the CPU -- copy before moving them to the GPU.  Gaussian P-1 sits at the origin (in every
    view), P-2 far above the scene (in none), and with nv >= 2 Gaussian P-3 near the edge of view 0's frustum, at
    the first candidate position that the oracle sees in some views and not in all."""
    model = synthetic_gaussians(P, D, seed=0, s0=0.03, n_cams=nv)
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(10 + i)) for i in range(nv)]
    cams = orbit_cameras(nv, W, H, seed=1, images=gts)
    with torch.no_grad():
        model._xyz[P - 1] = torch.tensor([0.0, 0.0, 0.0])
        model._xyz[P - 2] = torch.tensor([0.0, 0.0, 1000.0])
    if nv >= 2:
        c0 = cams[0]
        tx, ty = math.tan(c0.FoVx * 0.5), math.tan(c0.FoVy * 0.5)
        inv = torch.linalg.inv(c0.world_view_transform.float())
        chosen = None
        for z in (0.6, 1.0, 1.5, 2.5, 4.0):
            for fx, fy in ((0.8, 0.0), (-0.8, 0.0), (0.0, 0.8), (0.0, -0.8), (0.8, 0.8), (-0.8, -0.8)):
                pv = torch.tensor([[fx * tx * z, fy * ty * z, z, 1.0]])
                with torch.no_grad():
                    model._xyz[P - 3] = (pv @ inv)[0, :3]  # row vectors: p_view = p_world @ V
                n = int((tiles_touched(model, cams, rows=slice(P - 3, P - 2)) > 0).sum())
                if 0 < n < nv:
                    chosen = (z, fx, fy)
                    break
            if chosen:
                break
        assert chosen is not None, "no candidate position is seen by some views only"
    none, some, every = visibility_classes(tiles_touched(model, cams))
    assert none >= 1 and every >= 1 and (nv < 2 or some >= 1), (P, nv, none, some, every)
    return model, cams
