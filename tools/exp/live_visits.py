"""Experiment helper: what the live quadrant masks (k_quad_live, GSLM_LIVE_MASKS) remove at the bench config (1M
Gaussians SH 3, one 1080p view): the tile passes' wave-visits -- list entries whose mask holds quadrant q at a position
below the quadrant's bound, which both the J v pass and the VJP pass walk -- the head entries and the active list,
with the switch off and on, from the raw list words (gslm_inspect_list).  python tools/exp/live_visits.py"""
import json
import os
import sys

import torch

sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "gaussian-splatting-lm_amd")]
from gslm import _lib  # noqa: E402
from gslm.cameras import orbit_cameras  # noqa: E402
from gslm.lm import LMProblem  # noqa: E402
from gslm.model import synthetic_gaussians  # noqa: E402

W, H, P = 1920, 1080, 1_000_000
gy, gx = (H + 15) // 16, (W + 15) // 16
cams = orbit_cameras(1, W, H, seed=1)
model = synthetic_gaussians(P, 3, seed=0, s0=0.005, device="cpu", n_cams=1).to("cuda")
out = {}
for on in ("0", "1"):
    os.environ["GSLM_LIVE_MASKS"] = on
    prob = LMProblem(model, [c.to("cuda") for c in cams], torch.zeros(3), sh_projection="auto")
    prob.evaluate()
    prob.rhs(prob.zeros())  # builds the row map
    vr = prob.views[0]
    N = vr.N
    rg = torch.zeros(gy * gx * 2, dtype=torch.int32, device="cuda")
    nc = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    hscan = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.gslm_inspect(vr.geom.data_ptr(), P, vr.binning.data_ptr(), N, H, W, vr.image.data_ptr(),
                                     None, rg.data_ptr(), None, None, nc.data_ptr(), None, prob.stream))
    _lib.check(_lib.lib.gslm_inspect_rowmap(vr.geom.data_ptr(), P, N, vr.scratch.data_ptr(), vr.scratch.numel(),
                                            None, hscan.data_ptr(), prob.stream))
    words, _ = vr.list_words(prob.stream)
    _, pa = vr.active_list(P, prob.stream)
    torch.cuda.synchronize()
    # the quadrant bounds: the largest n_contrib of each tile's four 8 x 8 quadrants
    pad = torch.zeros(gy * 16, gx * 16, dtype=torch.int64, device="cuda")
    pad[:H, :W] = nc.view(H, W).long()
    neff = pad.view(gy, 2, 8, gx, 2, 8).amax(dim=(2, 5)).permute(0, 2, 1, 3).reshape(-1, 4)  # [tile, 2 qy + qx]
    r = rg.view(-1, 2).long()
    tid = torch.repeat_interleave(torch.arange(r.shape[0], device="cuda"), r[:, 1] - r[:, 0])
    pos = torch.arange(N, device="cuda") - r[tid, 0]
    mask = (words.long() >> 28) & 0xF
    visits = 0
    any_bit = torch.zeros(N, dtype=torch.bool, device="cuda")
    for q in range(4):
        hit = (((mask >> q) & 1) == 1) & (pos < neff[tid, q])
        visits += int(hit.sum())
        any_bit |= hit
    out["on" if on == "1" else "off"] = {"N": N, "wave_visits": visits, "head_entries": int(any_bit.sum()),
                                          "head_rows_hscan": int(hscan[N]), "Pa": int(pa)}
    del prob
a, b = out["off"], out["on"]
out["dead_share_of_visits"] = 1.0 - b["wave_visits"] / a["wave_visits"]
print(json.dumps(out))
