"""Yardsticks of the batched multi-view LM problem with the positions free (gslm.lm.BatchedXyzLMProblem;
tests/test_oracle_batched_xyz.py, tests/test_gpu_batched_xyz.py).

scene(name)         the oracle-compared scenes, two views each: sh1_33x17 and sh3_40x33 (scenes.lm_bg_scene, generic
                    background) and tiny_300_sh2_40x33 (scenes.make_scene with random targets, black background).
span_basis          per Gaussian an orthonormal basis Q_i [K - 1, V] of span{B_rest(dir_{i,b})}, float64 (the space
                    gslm_rest_basis spans; the tests never compare its coordinates, only the projector Q Q^T).
direction           the tests' generic direction: randn in every group (xyz included, seed 4), the SH-rest rows a randn
                    (seed 5) projected onto the span; xyz_only keeps its xyz part alone.
oracle_results      loss, J^T b and (J^T J + D) v of oracle.lm_ref.OracleLMProblem(mask_xyz=False) in a given dtype,
                    computed once per (scene, dtype) and shared.

Bounds of the GPU comparison: 8 x the float32 oracle's own distance from the float64 one (F32_FLOOR, measured and
asserted by tests/test_oracle_batched_xyz.py::test_float32_floor), per group relative to the group's max, capped at
MAX_TOL -- the convention of tests/lm_diag_ref.py and tests/lm_depth_ref.py.  No bound comes from a GPU number."""
import functools

import torch

from gslm.cameras import orbit_cameras
from oracle import torch_raster as tr
from oracle.lm_ref import OracleLMProblem, cgls_ref
from scenes import BG_GENERIC, BG_ZERO, SCENES as PLAIN_SCENES, lm_bg_scene, make_scene, to_float64

SCENES = ("sh1_33x17", "sh3_40x33", "tiny_300_sh2_40x33")
GROUPS6 = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity")
N_VIEWS = 2
V_SEED, REST_SEED = 4, 5
CG_ITERS = 3
MAX_TOL = 1e-3
SPAN_TOL = 1e-5    # tests/test_oracle_properties.py::test_single_view_krylov_space_keeps_sh_rest_in_basis_span
XYZ_SHARE = 0.25   # the xyz-only image of the product, as a share of the generic product's group max

# float32 oracle vs float64 oracle (OracleLMProblem(mask_xyz=False) in both, the same float32-representable direction),
# max |x32 - x64| / max |x64| per group (relative for the loss), measured on sh1_33x17 | sh3_40x33 | tiny_300_sh2_40x33
# (tests/test_oracle_batched_xyz.py::test_float32_floor prints the measurements and asserts they stay below the floors;
# a floor is the largest of the three measurements with about 20 % of headroom):
#   loss                   2.6e-8  1.1e-8  3.2e-8
#   J^T b    xyz           2.1e-6  2.2e-6  1.1e-6      features_dc   3.8e-7  4.1e-7  4.7e-7
#            features_rest 3.1e-7  6.5e-7  7.2e-7      scaling       5.1e-7  3.9e-7  6.6e-7
#            rotation      5.3e-7  8.0e-7  1.3e-6      opacity       3.1e-7  5.0e-7  4.8e-7
#   product  xyz           3.5e-7  5.3e-7  2.2e-7      features_dc   5.4e-7  1.3e-6  1.6e-6
#            features_rest 5.7e-7  2.3e-6  1.3e-6      scaling       1.1e-6  1.1e-6  2.7e-6
#            rotation      1.9e-6  3.1e-6  4.2e-7      opacity       1.3e-6  1.6e-6  1.9e-6
#   solve    xyz           1.6e-6  2.6e-6  8.7e-7      features_dc   5.8e-7  2.9e-7  4.3e-7
#   (3 x 3   features_rest 4.6e-7  5.0e-7  6.7e-7      scaling       4.3e-7  4.3e-7  6.2e-7
#   cgls)    rotation      5.6e-7  8.7e-7  1.2e-6      opacity       3.7e-7  4.9e-7  3.3e-7
F32_FLOOR = {
    "loss": 3.8e-8,
    "rhs": {"xyz": 2.7e-6, "features_dc": 5.6e-7, "features_rest": 8.6e-7, "scaling": 7.9e-7, "rotation": 1.5e-6,
            "opacity": 6.0e-7},
    "product": {"xyz": 6.3e-7, "features_dc": 1.9e-6, "features_rest": 2.8e-6, "scaling": 3.2e-6, "rotation": 3.7e-6,
                "opacity": 2.3e-6},
    "solve": {"xyz": 3.1e-6, "features_dc": 7.0e-7, "features_rest": 8.0e-7, "scaling": 7.4e-7, "rotation": 1.5e-6,
              "opacity": 5.9e-7},
}


def _tol(f):
    return {k: min(8.0 * v, MAX_TOL) for k, v in f.items()} if isinstance(f, dict) else min(8.0 * f, MAX_TOL)


GPU_TOL = {q: _tol(f) for q, f in F32_FLOOR.items()}


def scene(name, f64=False):
    """(model, cams, bg) on the CPU, float32 (or float64 copies)."""
    if name in PLAIN_SCENES:
        model, _ = make_scene(name)
        _, _, W, H, _, _ = PLAIN_SCENES[name]
        cams = orbit_cameras(N_VIEWS, W, H, seed=1)
        for i, c in enumerate(cams):
            c.original_image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3 + i))
        bg = BG_ZERO
    else:
        model, cams = lm_bg_scene(name, n_views=N_VIEWS)
        bg = BG_GENERIC
    if f64:
        model, cams = to_float64(model, cams)
    return model, cams, torch.tensor(bg, dtype=torch.float64 if f64 else torch.float32)


def span_basis(model, cams):
    """Q [P, K - 1, V] float64, orthonormal columns spanning {B_rest(dir_{i,b})}_b of every Gaussian."""
    D = model.active_sh_degree
    K = (D + 1) ** 2
    cols = []
    for cam in cams:
        d = model._xyz.detach().double() - cam.camera_center.double()
        d = d / d.norm(dim=1, keepdim=True)
        eye = torch.eye(K, dtype=torch.float64).expand(d.shape[0], K, K)
        B = torch.stack([tr.eval_sh(D, eye[:, :, k:k + 1].expand(-1, -1, 3), d)[:, 0] for k in range(K)], 1)  # [P, K]
        cols.append(B[:, 1:])
    Q, _ = torch.linalg.qr(torch.stack(cols, 2))  # [P, K - 1, V]
    return Q


def off_span(vec, layout, Q):
    """(max |R - Q Q^T R|, max |R|) of the SH-rest rows R of a flat vector."""
    a, b = layout.offsets["features_rest"]
    R = vec[a:b].double().view(Q.shape[0], Q.shape[1], 3)
    resid = R - Q @ (Q.transpose(1, 2) @ R)
    return float(resid.abs().max()), float(R.abs().max())


def direction(layout, Q, xyz_only=False):
    """The generic direction (float32-representable float64): randn everywhere, the SH-rest rows in the span, the
    exposure tail zero; xyz_only: its xyz part alone."""
    v = torch.randn(layout.numel, generator=torch.Generator().manual_seed(V_SEED), dtype=torch.float64)
    a, b = layout.offsets["features_rest"]
    R = torch.randn(Q.shape[0], Q.shape[1], 3, generator=torch.Generator().manual_seed(REST_SEED), dtype=torch.float64)
    v[a:b] = (Q @ (Q.transpose(1, 2) @ R)).reshape(-1)
    e0, e1 = layout.offsets["exposure"]
    v[e0:e1] = 0
    if xyz_only:
        x0, x1 = layout.offsets["xyz"]
        w = torch.zeros_like(v)
        w[x0:x1] = v[x0:x1]
        v = w
    return v.float().double()


@functools.lru_cache(maxsize=None)
def oracle_results(name, f64):
    """{'loss', 'rhs', 'v', 'y' (= (J^T J + D) v), 'v_xyz', 'y_xyz' (= J^T J v_xyz, D v removed), 'x' (CG_ITERS
    iterations of oracle.lm_ref.cgls_ref from rhs), 'layout', 'Q'} of the
    oracle with the positions free, in float64 or float32 (the vectors come back in the oracle's dtype).  Computed
    once; the callers only read."""
    model, cams, bg = scene(name, f64)
    dt = torch.float64 if f64 else torch.float32
    op = OracleLMProblem(model, cams, bg, mask_xyz=False)
    Q = span_basis(model, cams)
    out = {"loss": float(op.evaluate()), "layout": op.layout, "Q": Q}
    out["rhs"] = op.rhs().to(dt)
    v = direction(op.layout, Q).to(dt)
    out["v"] = v
    out["y"] = op.matvec(v, torch.zeros(op.layout.numel, dtype=dt)).clone()
    vx = direction(op.layout, Q, xyz_only=True).to(dt)
    out["v_xyz"] = vx
    out["y_xyz"] = op.local_normal_matvec(vx, torch.zeros(op.layout.numel, dtype=dt), damp=False).clone()
    out["x"] = cgls_ref(op, out["rhs"], CG_ITERS, CG_ITERS)
    return out


def group_errors(got, ref, layout, groups=GROUPS6):
    """{group: max |got - ref| / max |ref|} in float64."""
    gv, rv = layout.views(got.double()), layout.views(ref.double())
    return {k: float((gv[k] - rv[k]).abs().max() / rv[k].abs().max().clamp_min(1e-300)) for k in groups
            if rv[k].numel()}


def group_max(vec, layout, groups=GROUPS6):
    v = layout.views(vec.double())
    return {k: float(v[k].abs().max()) for k in groups if v[k].numel()}
