"""Cost of the inverse-depth residual (LMProblem / lm_step with depth_weight) at the bench scene: 1M Gaussians SH 3,
one 1080p training view, 50 validation views, synthetic depth targets (the inverse depth of bench.py's perturbed
ground-truth model, every pixel).  bench.py itself is not touched: this builds the same scene and times, with and
without depth in one process (the plain path's kernels are the parent commit's, profiles/lm_depth/):

  cg      one CG iteration of cgls_fused in benchmark mode (the lean loop), HIP events around K iterations;
  step    lm_step, 10 iterations with the stopping tests and the 7-point line search, median of the reps
          (bench.py's time_lm_step, the model restored between reps).

    python tools/bench_lm_depth.py [--what cg|step|both] [--iters 20] [--reps 5] [--val-views 50] [--P 1000000]

--plain-only times the plain quantities alone and builds the scene without depth targets, so the same file also runs
against a tree from before the feature (copied into it) for an A/B of the plain path.

For the tile kernel alone run --what cg under `rocprofv3 --kernel-trace --stats -- python tools/bench_lm_depth.py ...`
and read k_render_matvec<false> against k_render_matvec_depth.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-lm_amd"), ROOT]

import torch  # noqa: E402


def scene(args, device):
    """bench.py's scene: the model, the training camera and the validation cameras with ground truth rendered from the
    perturbed model (seed 2) -- colour and, here, inverse depth."""
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem
    from gslm.model import synthetic_gaussians
    W, H = args.width, args.height
    bg = torch.zeros(3)
    cams = [c.to(device) for c in orbit_cameras(1, W, H, seed=1)]
    val = [c.to(device) for c in orbit_cameras(args.val_views, W, H, seed=5)]
    pert = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=1)
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        pert._features_dc += 0.01 * torch.randn(pert._features_dc.shape, generator=g2)
        pert._opacity += 0.01 * torch.randn(pert._opacity.shape, generator=g2)
        pert._scaling += 0.01 * torch.randn(pert._scaling.shape, generator=g2)
    pert.to(device)
    allc = cams + val
    for c0 in range(0, len(allc), 8):
        chunk = allc[c0:c0 + 8]
        if args.plain_only:
            p = LMProblem(pert, chunk, bg, device=device)
        else:  # (depth_weight = 0 with any target: evaluate() renders the inverse depth)
            zeros = [torch.zeros(1, H, W, device=device) for _ in chunk]
            p = LMProblem(pert, chunk, bg, device=device, depth_weight=0.0, invdepths=zeros)
        p.evaluate()
        for c, vr in zip(chunk, p.views):
            c.original_image = vr.color.clamp(0, 1).clone()
            if not args.plain_only:
                c.invdepthmap, c.depth_mask, c.depth_reliable = vr.invdepth.clone(), None, True
        del p
    del pert
    torch.cuda.empty_cache()
    model = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=1).to(device)
    return model, cams, val, bg


def time_cg(model, cams, bg, depth_weight, iters, reps, device):
    from gslm.lm import LMProblem, cgls_fused
    kw = {} if depth_weight is None else {"depth_weight": depth_weight}
    prob = LMProblem(model, cams, bg, device=device, sh_projection="auto", **kw)
    prob.evaluate()
    g = prob.rhs(prob.zeros())
    cgls_fused(prob, g, max_iter=3, restart_iter=3, check_every=False)  # warm-up: the row map, the list, workspaces
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cgls_fused(prob, g, max_iter=iters, restart_iter=iters, check_every=False)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    ms.sort()
    return {"ms_per_iteration": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "reps": reps, "iters": iters}


def time_step(model, cams, val, bg, depth_weight, reps, device):
    from gslm.lm import lm_step
    kw = {} if depth_weight is None else {"depth_weight": depth_weight}
    saved = [t.detach().clone() for t in model.params()]

    def restore():
        with torch.no_grad():
            for t, s0 in zip(model.params(), saved):
                if t is not model._xyz:
                    t.copy_(s0)

    out = lm_step(model, cams, val, bg, max_iter=10, restart_iter=10, device=device, **kw)  # warm-up
    restore()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = lm_step(model, cams, val, bg, max_iter=10, restart_iter=10, device=device, **kw)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        restore()
        torch.cuda.synchronize()
    ts.sort()
    return {"ms": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "reps": reps, "best_alpha": out["best_alpha"],
            "cg_iters": out["cg"]["iters"], "loss_start": out["start_loss"], "loss_final": out["final_val_loss"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("cg", "step", "both"), default="both")
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s0", type=float, default=0.005)
    ap.add_argument("--val-views", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth-weight", type=float, default=1.0)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    device = "cuda:0"
    if args.what == "cg":
        args.val_views = 0
    model, cams, val, bg = scene(args, device)
    res = {"P": args.P, "sh": args.sh, "size": [args.width, args.height], "val_views": args.val_views,
           "depth_weight": args.depth_weight}
    for name, w in (("plain", None),) + (() if args.plain_only else (("depth", args.depth_weight),)):
        if args.what in ("cg", "both"):
            res[f"cg_{name}"] = time_cg(model, cams, bg, w, args.iters, args.reps, device)
        if args.what in ("step", "both"):
            res[f"step_{name}"] = time_step(model, cams, val, bg, w, args.reps, device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
