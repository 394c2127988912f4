"""CPU: what the batched multi-view LM problem with the positions free rests on, checked on the oracle
(oracle.lm_ref.OracleLMProblem(mask_xyz=False)) for every scene tests/test_gpu_batched_xyz.py compares on.

1. The span claim with xyz free: J is evaluated at the current theta, so every view direction is fixed within a solve and
   the SH-rest rows of J^T b and of (J^T J + D) v, v in the views' span with a generic xyz part, stay in the span.
2. The xyz columns are not hidden: the image of the direction's xyz part alone is a large share of the product in every
   group, so a dropped or mis-chained dmean or a lost xyz tangent cannot pass the product bounds.
3. The float32 floors tests/lm_batched_xyz_ref.py records hold."""
import pytest

import lm_batched_xyz_ref as ref


@pytest.mark.parametrize("name", ref.SCENES)
def test_sh_rest_rows_stay_in_the_views_span_with_xyz_free(name):
    """Float32 oracle, the bound of test_single_view_krylov_space_keeps_sh_rest_in_basis_span (1e-5 of the group max).
    Measured on tiny_300_sh2_40x33: 2.0e-7 of a 3.59 max for J^T b, 1.1e-6 of a 14.5 max for the product."""
    r = ref.oracle_results(name, False)
    for what in ("rhs", "y", "x"):
        resid, scale = ref.off_span(r[what], r["layout"], r["Q"])
        print(f"{name} {what}: off-span {resid:.2e} of a group max of {scale:.3g}")
        assert scale > 0 and resid <= ref.SPAN_TOL * scale, (what, resid, scale)
    # the direction itself is in the span and has a generic xyz part
    resid, scale = ref.off_span(r["v"], r["layout"], r["Q"])
    assert resid <= 1e-6 * scale
    assert ref.group_max(r["v"], r["layout"])["xyz"] > 1.0


@pytest.mark.parametrize("name", ref.SCENES)
def test_the_xyz_columns_are_not_hidden(name):
    """J^T J applied to the xyz part of the direction alone (D v removed) against the generic product, per group."""
    r = ref.oracle_results(name, True)
    part, whole = ref.group_max(r["y_xyz"], r["layout"]), ref.group_max(r["y"], r["layout"])
    for k in ref.GROUPS6:
        print(f"{name} {k}: xyz-only {part[k]:.3g}, generic {whole[k]:.3g}")
        assert part[k] >= ref.XYZ_SHARE * whole[k], (k, part[k], whole[k])
    # and J^T b has an xyz group worth comparing
    g = ref.group_max(r["rhs"], r["layout"])
    assert g["xyz"] >= ref.XYZ_SHARE * max(v for k, v in g.items() if k != "xyz")


@pytest.mark.parametrize("name", ref.SCENES)
def test_float32_floor(name):
    r32, r64 = ref.oracle_results(name, False), ref.oracle_results(name, True)
    L = r64["layout"]
    e = abs(r32["loss"] - r64["loss"]) / r64["loss"]
    print(f"{name} loss {e:.2e}")
    assert e <= ref.F32_FLOOR["loss"]
    for what, key in (("rhs", "rhs"), ("product", "y"), ("solve", "x")):
        errs = ref.group_errors(r32[key], r64[key], L)
        print(f"{name} {what} " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert set(errs) == set(ref.GROUPS6)
        for k, v in errs.items():
            assert v <= ref.F32_FLOOR[what][k], (what, k, v)


def test_bounds_follow_the_convention():
    for what in ("rhs", "product", "solve"):
        for k, f in ref.F32_FLOOR[what].items():
            assert ref.GPU_TOL[what][k] == min(8.0 * f, ref.MAX_TOL) and 0 < f < ref.MAX_TOL / 8
    assert ref.GPU_TOL["loss"] == 8.0 * ref.F32_FLOOR["loss"]
