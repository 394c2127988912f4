"""Test infrastructure: the LM normal equations under trained per-camera exposure on the CPU oracle, and the scenes
the exposure tests share (tests/test_oracle_lm_exposure.py, tests/test_gpu_lm_exposure.py).

ExposureOracleLMProblem is oracle.lm_ref.OracleLMProblem with render()'s exposure step
(gaussian_renderer/__init__.py:113-119) between the raw render and the clamp:
    C = matmul(R.permute(1, 2, 0), X[:3, :3]).permute(2, 0, 1) + X[:3, 3, None, None],   r = m clamp01(C) - gt
with X the camera's row of model._exposure, and a parameter mask that keeps the exposure rows.  Everything else --
J^T b through autograd, (J^T J + D) v through forward-AD then autograd, the damping -- is the base class's, so the
exposure columns of J come from torch's own differentiation of the lines above."""
import torch

from oracle import torch_raster as tr
from oracle.lm_ref import OracleLMProblem
from scenes import lm_bg_mask, lm_bg_scene

# the exposures of views 0 and 1 (row-major [i][k]: C_j = sum_i R_i X[i][j] + X[j][3])
X0 = [[0.90, 0.05, -0.03, 0.04], [-0.06, 1.10, 0.02, -0.02], [0.03, -0.04, 0.80, 0.03]]
X1 = [[1.15, -0.04, 0.02, -0.05], [0.03, 0.85, -0.05, 0.06], [-0.02, 0.06, 1.05, 0.01]]
# (scene name, occluders): checked on the CPU oracle -- with X0 / X1 no pixel-channel of C, covered or not, lies within
# 4e-5 of 0 or 1 in either view, for BG_ZERO and BG_GENERIC (exposure_stats; the tests assert 1e-5)
SCENES = {"sh1_33x17": False, "sh3_40x33": True}


def apply_exposure(raw, X):
    return torch.matmul(raw.permute(1, 2, 0), X[:3, :3]).permute(2, 0, 1) + X[:3, 3, None, None]


class ExposureOracleLMProblem(OracleLMProblem):
    def __init__(self, model, cams, bg, train_exposure=True, **kw):
        assert train_exposure
        super().__init__(model, cams, bg, **kw)
        assert not self.ssim

    def exposed(self, c):
        _, _, _, raw = tr.render_model(self.model, c, self.bg)
        return apply_exposure(raw, self.model._exposure[self.model.exposure_mapping[c.image_name]])

    def _residuals(self):
        return [self.exposed(c).clamp(0, 1) * c.alpha_mask - c.original_image for c in self.cams]

    def _mask(self, vec):
        if self.mask_xyz:
            a, b = self.layout.offsets["xyz"]
            vec[a:b] = 0
        return vec


class ExposureOracleLossEvaluator:
    """gslm.lm.LossEvaluator(train_exposure=True)'s interface on the oracle (evaluate() only: the exact line search)."""

    def __init__(self, model, cams, bg, device="cpu", batch=8, reduce=None, train_exposure=True):
        self.prob = ExposureOracleLMProblem(model, cams, bg)

    def evaluate(self):
        return self.prob.evaluate().clone()


def set_exposures(model, cams, rows=(X0, X1)):
    """model._exposure[i] = rows[i] for camera i (identity beyond), and the name -> row mapping render() uses."""
    names = [c.image_name for c in cams]
    assert len(set(names)) == len(names), names
    model.exposure_mapping = {n: i for i, n in enumerate(names)}
    with torch.no_grad():
        for i, X in enumerate(rows[:model._exposure.shape[0]]):
            model._exposure[i] = torch.tensor(X, dtype=model._exposure.dtype)
    return model


def exposure_scene(name, masked=True, n_views=2, rows=(X0, X1)):
    """(model, cams) on the CPU: lm_bg_scene(name, n_views, occluders as SCENES says), the exposures set, and with
    masked the fractional alpha masks of lm_bg_mask (view i's from seed i)."""
    model, cams = lm_bg_scene(name, n_views=n_views, occluders=SCENES[name])
    if masked:
        for i, c in enumerate(cams):
            c.alpha_mask = lm_bg_mask(name, seed=i)
    return set_exposures(model, cams, rows), cams


def exposure_stats(model, cams, bg):
    """Per view, on the oracle's exposed colour C: the shares of pixel-channels above 1 and below 0, and the number
    within 1e-5 of 0 or 1 (where the GPU's and the oracle's 1[0 <= C <= 1] could take different sides)."""
    op = ExposureOracleLMProblem(model, cams, torch.as_tensor(bg, dtype=model._xyz.dtype))
    out = []
    with torch.no_grad():
        for c in cams:
            C = op.exposed(c)
            near = ((C - 1).abs() < 1e-5) | (C.abs() < 1e-5)
            out.append(dict(above=float((C > 1).float().mean()), below=float((C < 0).float().mean()),
                            boundary=int(near.sum())))
    return out


def assert_exposure_scene(model, cams, bg):
    """No pixel-channel at a corner of the clamp, and the clamp's upper side live in every view."""
    stats = exposure_stats(model, cams, bg)
    for s in stats:
        assert s["boundary"] == 0, stats
        assert s["above"] > 0, stats
    return stats


def direction(layout, seed=9, tail=True):
    """A random direction with xyz zeroed (the LM mask) and, with tail, a nonzero exposure tail."""
    v = torch.randn(layout.numel, generator=torch.Generator().manual_seed(seed))
    a, b = layout.offsets["xyz"]
    v[a:b] = 0
    if not tail:
        a, b = layout.offsets["exposure"]
        v[a:b] = 0
    return v
