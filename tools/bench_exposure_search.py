#!/usr/bin/env python3
"""The LM step under trained exposure, by how its line search evaluates the validation views.

The scene and validation set of bench.py's `lm_step` measurement: 1M Gaussians, SH 3, one 1080p training view, 50
validation views (orbit seed 5), ground truth = the render of the perturbed model, here under the exposure X_GT; the
model starts from identity exposures, one row per camera.  lm_step(max_iter=10, restart_iter=10, timing=True), the
model restored after every step.  Modes, alternating in one process over --rounds rounds:
  plain        lm_step(): no exposure (the step bench.py times), for scale;
  forward      lm_step(train_exposure=True): the default -- per validation view the full forward, then
               gslm_lm_residual_exposure's loss, on one stream, seven evaluations in the exact order;
  fused_exact  val_exposure="fused", line_search="exact": the exposure in the loss blend's epilogue, batches over the
               side streams, seven evaluations;
  fused_union  val_exposure="fused", line_search="union": the six points through one binning per view.
Every mode keeps its own validation evaluator from step to step, as a training loop that stays in one mode does
(lm_step's cache holds one evaluator: the tool swaps the cache entry around each call).  One JSON line per step to
stdout and, with --out, to a file.  There is no fallback: without a GPU the tool fails.
--tree DIR times the package of another checkout (a build of the parent commit: --modes plain).

  python tools/bench_exposure_search.py --rounds 5 --out profiles/lm_exposure_search/runs.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_GT = [[0.90, 0.05, -0.03, 0.04], [-0.06, 1.10, 0.02, -0.02], [0.03, -0.04, 0.80, 0.03]]
MODES = {"plain": {}, "forward": {"train_exposure": True},
         "fused_exact": {"train_exposure": True, "val_exposure": "fused", "line_search": "exact"},
         "fused_union": {"train_exposure": True, "val_exposure": "fused", "line_search": "union"}}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s0", type=float, default=0.005)
    ap.add_argument("--val-views", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of " + ", ".join(MODES))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main():
    args = parse()
    modes = [m for m in args.modes.split(",") if m]
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode {m!r}")
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "gaussian-splatting-lm_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_exposure_search.py needs the GPU: a CPU run has no timing to report")
    from gslm import lm
    from gslm.cameras import orbit_cameras
    from gslm.model import synthetic_gaussians
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None

    def emit(line):
        s = json.dumps(dict(line, label=args.label, P=args.P, val_views=args.val_views, iters=args.iters))
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    W, H = args.width, args.height
    bg = torch.zeros(3)
    cams = [c.to(dev) for c in orbit_cameras(1, W, H, seed=1)]
    val = [c.to(dev) for c in orbit_cameras(args.val_views, W, H, seed=5)]
    for i, c in enumerate(val):  # (the two orbits name their cameras alike: one exposure row per camera needs names)
        c.image_name = f"val_{i:03d}"
    n_cams = 1 + len(val)
    pert = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=n_cams)
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        pert._features_dc += 0.01 * torch.randn(pert._features_dc.shape, generator=g2)
        pert._opacity += 0.01 * torch.randn(pert._opacity.shape, generator=g2)
        pert._scaling += 0.01 * torch.randn(pert._scaling.shape, generator=g2)
    pert.to(dev)
    X = torch.tensor(X_GT, device=dev)
    every = cams + val
    for c0 in range(0, len(every), 8):
        chunk = every[c0:c0 + 8]
        p = lm.LMProblem(pert, chunk, bg, device=dev)
        p.evaluate()
        for c, vr in zip(chunk, p.views):
            R = vr.color
            c.original_image = (torch.matmul(R.permute(1, 2, 0), X[:, :3]).permute(2, 0, 1) +
                                X[:, 3, None, None]).clamp(0, 1).contiguous()
        del p
    del pert
    torch.cuda.empty_cache()
    model = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=n_cams).to(dev)
    model.exposure_mapping = {c.image_name: i for i, c in enumerate(every)}
    assert len(model.exposure_mapping) == n_cams
    leaves = [t for t in model.params() if t is not model._xyz]  # xyz is masked: its version keeps the depth orders
    saved = [t.detach().clone() for t in leaves]
    caches = {}

    def step(m):
        lm._VAL_CACHE.clear()
        if m in caches:
            lm._VAL_CACHE["last"] = caches[m]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = lm.lm_step(model, cams, val, bg, max_iter=args.iters, restart_iter=args.iters, timing=True, **MODES[m])
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        caches[m] = lm._VAL_CACHE.get("last")
        with torch.no_grad():
            for t, s0 in zip(leaves, saved):
                t.copy_(s0)
        return ms, o

    for m in modes:  # workspaces, depth orders, clocks
        for _ in range(2):
            ms, o = step(m)
        emit({"kind": "warmup", "mode": m, "ms": ms, "line_search": o["line_search"]})
    for r in range(args.rounds):
        for m in modes:
            ms, o = step(m)
            emit({"kind": "lm_step", "round": r, "mode": m, "ms": ms, "phases_ms": o["timing"],
                  "line_search": o["line_search"], "best_alpha": o["best_alpha"], "final_val_loss": o["final_val_loss"],
                  "trace": [v for _, v in o["trace"]]})
    if out:
        out.close()


if __name__ == "__main__":
    main()
