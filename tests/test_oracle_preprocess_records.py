"""CPU: what tests/test_gpu_preprocess_records.py relies on, measured and asserted on the oracle alone.

  * the float32 oracle's distance from the float64 record (chain_jacobian.record_fn) in the measure the GPU test uses,
    max over the visible Gaussians of |got - ref| / max(|ref|, median |ref|), for every case of the GPU test: the
    printed values are preprocess_layouts.FLOORS, and the GPU bounds are 8 x them;
  * the boundary exclusion of the discrete outputs: its share of P x views on every prefix (<= 0.5 %), and that the
    float32 oracle's tile count, rect, radius, clamp bits and visibility equal the float64 oracle's outside it;
  * the scene counts the alpha-threshold and depth-key tests rely on;
  * that the prefix sizes put every float4 residue into the last block for every SH-rest stride that has a tail;
  * stage_lead() of every layout, restated in Python on CPU tensors laid out the same way: a layout meant to be
    unstaged must not be staged by accident (nor the reverse).
"""
import ctypes

import pytest
import torch

import preprocess_layouts as pl


@pytest.mark.parametrize("case", pl.CASES, ids=pl.case_id)
def test_float32_floor(case):
    _, cams, o32s, o64s = pl.oracle_case(case)
    worst = torch.zeros(len(pl.OUT_NAMES), dtype=torch.float64)
    for b in range(len(cams)):
        o32, o64 = o32s[b], o64s[b]
        # the float32 oracle takes its own decisions; where they differ from float64's the Gaussian is in the exclusion
        # (asserted below), and a record exists on both sides only where both call it visible
        rows = o32["visible"] & o64["visible"]
        worst = torch.maximum(worst, pl.record_measure(o32["record"], o32, o64, rows))
        assert int(rows.sum()) > 0.5 * rows.numel()
    print(f"{pl.case_id(case)}: " + " ".join(f"{n}={float(x):.3e}" for n, x in zip(pl.OUT_NAMES, worst)))
    for o, name in enumerate(pl.OUT_NAMES):
        assert float(worst[o]) <= pl.FLOORS[pl.floor_key(name, case[2])], (name, float(worst[o]))


def test_bounds_are_rounding_level():
    """No GPU bound exceeds chain_jacobian.MAX_TOL (2e-4): a row read from the wrong slot is O(1) in this measure."""
    import chain_jacobian as cj
    assert pl.TOL_FACTOR == cj.TOL_FACTOR
    for name in pl.OUT_NAMES:
        for aa in (False, True):
            assert 0 < pl.record_tol(name, aa) <= cj.MAX_TOL, (name, aa)


@pytest.mark.parametrize("case", pl.CASES, ids=pl.case_id)
def test_exclusion_share_and_discrete_outputs(case):
    _, cams, o32s, o64s = pl.oracle_case(case)
    ex = [pl.excluded(o) for o in o64s]
    for P in pl.SIZES:
        n = sum(int(e[:P].sum()) for e in ex)
        print(f"{pl.case_id(case)} P={P}: {n} excluded of {P * len(cams)}")
        assert n <= pl.EXCLUDE_CAP * P * len(cams), (P, n)
    for b in range(len(cams)):
        keep = ~ex[b]
        o32, o64 = o32s[b], o64s[b]
        assert torch.equal(o32["visible"][keep], o64["visible"][keep])
        assert torch.equal((o32["depth"] > 0.2)[keep], (o64["depth"] > 0.2)[keep])
        vis = keep & o32["visible"]
        for k in ("tiles_touched", "radii", "rect", "clamped"):
            assert torch.equal(o32[k][vis], o64[k][vis]), (b, k)
        assert bool((o32["tiles_touched"][~o32["visible"]] == 0).all() and (o32["radii"][~o32["visible"]] == 0).all())


def test_alpha_threshold_scene_counts():
    """At least 5 visible Gaussians on each side of 255 o = 1 (o the float32 effective opacity) in each view: on the
    antialiasing case as it is, and on the plain (3, 3) case with every 16th opacity lowered."""
    for case, lowered in ((pl.CASES[-1], False), (pl.CASES[0], True)):
        _, cams, o32s, _ = pl.oracle_case(case, lowered)
        for b in range(len(cams)):
            vis = o32s[b]["visible"]
            o = o32s[b]["opacity"][vis]
            below = int((o * 255.0 <= 1.0).sum())
            above = int((o * 255.0 > 1.0).sum())
            print(f"{pl.case_id(case)} lowered={lowered} view {b}: 255 o <= 1 on {below}, > 1 on {above}")
            assert below >= 5 and above >= 5, (case, lowered, b, below, above)


@pytest.mark.parametrize("case", pl.CASES, ids=pl.case_id)
def test_depth_key_scene_counts(case):
    """At least 20 Gaussians in front of the near plane that their footprint culls (keyed, yet invisible) in each view.
    The scene has none behind the near plane: the mirrored copy (every 8th Gaussian reflected through the first
    camera's centre) puts at least 20 there."""
    model, cams, o32s, _ = pl.oracle_case(case)
    for b, o in enumerate(o32s):
        keyed_culled = int(((o["depth"] > 0.2) & ~o["visible"]).sum())
        print(f"{pl.case_id(case)} view {b}: keyed yet culled {keyed_culled}")
        assert keyed_culled >= 20
    o = pl._oracle(pl.mirrored_model(model, cams[0]), cams[0], case, torch.float32)
    behind = int((~(o["depth"] > 0.2)).sum())
    print(f"{pl.case_id(case)} mirrored: behind the near plane {behind}")
    assert behind >= 20 and not bool(o["visible"][~(o["depth"] > 0.2)].any())


def test_sizes_cover_every_float4_residue():
    """The last block's staged span is nv * stride floats, nv = P % 256 or 256; its tail is that modulo 4."""
    def residues(stride):
        return {(P % 256 or 256) * stride % 4 for P in pl.SIZES}
    for stride in (9, 45, 27):        # SH 1 leaf, SH 3 leaf, SH 2 features
        assert residues(stride) == {0, 1, 2, 3}, stride
    for stride in (24, 12, 48):       # SH 2 leaf, SH 1 features, SH 3 features: whole float4s at any size
        assert residues(stride) == {0}, stride
    # more than one block, with and without a tail, and a nearly full last block
    assert any(P > 256 and P % 256 for P in pl.SIZES) and any(P % 256 == 0 for P in pl.SIZES) and 255 in pl.SIZES


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("degree", [3, 2, 1, 0])
def test_stage_lead_of_every_layout(degree, raw):
    model, _, o32s, _ = pl.oracle_case((degree, degree, False, 1.0))
    for P in (1, 3, 258):
        vals = pl.model_values(model, P)
        for name in pl.LAYOUTS:
            L = pl.Layout(name, vals, raw, "cpu", colors=o32s[0]["rgb"][:P])
            want = pl.EXPECTED_LEAD[name] if degree > 0 else -1
            assert L.expected_lead() == want
            assert L.stage_lead() == want, (name, degree, P, L.stage_lead())
            # the same float values in every layout, read back through the pointers and strides the kernels get
            if name != "colors" and P <= 3:
                ref = torch.cat([vals["dc"].reshape(P, 3), vals["rest"].reshape(P, -1)], dim=1)

                def read(ptr, stride, n):
                    return torch.tensor([[ctypes.c_float.from_address(ptr + 4 * (i * stride + c)).value
                                          for c in range(n)] for i in range(P)])
                assert torch.equal(read(L.dc_ptr, L.dc_stride, 3), ref[:, :3])
                if L.M > 1:
                    assert torch.equal(read(L.rest_ptr, L.rest_stride, 3 * (L.M - 1)), ref[:, 3:])
                    if name == "padded":
                        assert torch.isnan(read(L.rest_ptr + 4 * 3 * (L.M - 1), L.rest_stride, 1)).all()
