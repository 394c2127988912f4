#!/usr/bin/env python3
"""Plain CG against Jacobi-preconditioned CG on the LM normal equations.

By default bench.py's scene: 1M Gaussians, SH 3, one 1080p view (--views 5: the five-view loop problem), the ground
truth rendered from the perturbed model.  Same scene, same g; per run and per max_iter in --iters the two modes
alternate in one process:
  plain    cgls_fused(check_every=False)   (one view: the active list and the lean loop, as the benchmark)
  jacobi   cgls_jacobi(check_every=False)  (LMProblem.diagonal once per solve, then gslm_pcg_update / gslm_xpby_dev)
`solve` lines: ms per solve (for jacobi including the diagonal) and ms per iteration; `diag` lines: ms of
LMProblem.diagonal alone (row map current), next to `product` lines (one (J^T J + D) v).  `quality` lines (once per
mode and max_iter): phi(x) = x^T A x / 2 - g^T x with one extra product and float64 sums, and |g - A x| / |g|.
`lm_step` lines: the line search's alpha and the validation loss after lm_step for precond=None and "jacobi" (--val
validation views; skipped with --val 0).  Each mode is settled first (untimed work >= 200 ms).  One JSON line per
measurement to stdout and, with --out, to a file.  There is no fallback: without a GPU the tool fails.

  python tools/bench_jacobi.py --runs 5 --out profiles/lm_jacobi/runs.jsonl
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s0", type=float, default=0.005)
    ap.add_argument("--views", type=int, default=1)
    ap.add_argument("--iters", type=int, nargs="+", default=[2, 5, 10], help="max_iter of the timed solves")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--val", type=int, default=4, help="validation views of the lm_step comparison (0: skip it)")
    ap.add_argument("--label", default="", help="copied into every line (e.g. the commit)")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main():
    args = parse()
    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-lm_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_jacobi.py needs the GPU: a CPU run has no timing to report")
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem, cgls_fused, cgls_jacobi, clear_val_cache, lm_step
    from gslm.model import synthetic_gaussians
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None

    def emit(line):
        line = dict(line, label=args.label, P=args.P, sh=args.sh, width=args.width, height=args.height,
                    views=args.views)
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    W, H = args.width, args.height
    nv = args.views + args.val
    cams = [c.to(dev) for c in orbit_cameras(nv, W, H, seed=1)]
    bg = torch.zeros(3)
    # ground truth as in bench.py: the render of the model with f_dc / opacity / scaling perturbed by N(0, 0.01^2)
    pert = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=nv)
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        pert._features_dc += 0.01 * torch.randn(pert._features_dc.shape, generator=g2)
        pert._opacity += 0.01 * torch.randn(pert._opacity.shape, generator=g2)
        pert._scaling += 0.01 * torch.randn(pert._scaling.shape, generator=g2)
    pert.to(dev)
    for c in cams:
        gt = LMProblem(pert, [c], bg, device=dev)
        gt.evaluate()
        c.original_image = gt.views[0].color.clamp(0, 1).clone()
        del gt
    del pert
    torch.cuda.empty_cache()
    model = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=nv).to(dev)
    train, val = cams[:args.views], cams[args.views:]

    prob = LMProblem(model, train, bg, device=dev, sh_projection="auto")
    prob.evaluate()
    g = prob.rhs(prob.zeros())
    torch.cuda.synchronize()
    emit({"kind": "scene", "num_rendered": [int(n) for n in prob.num_rendered()], "loss": float(prob.loss),
          "projected": bool(prob.layout.rest_projected)})

    def solve(mode, k):
        fn = cgls_fused if mode == "plain" else cgls_jacobi
        return fn(prob, g, max_iter=k, restart_iter=k, check_every=False)[0]

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    y = prob.zeros()
    for mode in ("plain", "jacobi"):
        t0 = time.perf_counter()
        n = 0
        while n < 2 or time.perf_counter() - t0 < 0.2:
            solve(mode, args.iters[-1])
            torch.cuda.synchronize()
            n += 1
        emit({"kind": "settle", "mode": mode, "calls": n, "ms": 1e3 * (time.perf_counter() - t0)})

    gd = g.double()
    gn = float(gd.norm())
    for k in args.iters:
        for mode in ("plain", "jacobi"):
            x = solve(mode, k)
            prob.matvec(x, y)
            xd, yd = x.double(), y.double()
            emit({"kind": "quality", "mode": mode, "max_iter": k, "phi": float(0.5 * (xd @ yd) - gd @ xd),
                  "residual_rel": float((gd - yd).norm()) / gn})

    d = prob.diagonal()
    v = prob.layout.views(d)
    emit({"kind": "diag_stats", **{f"{name}_median": float(t.median()) for name, t in v.items()
                                   if name not in ("xyz", "exposure") and t.numel()},
          **{f"{name}_max": float(t.max()) for name, t in v.items() if name not in ("xyz", "exposure") and t.numel()}})

    for r in range(args.runs):
        for k in args.iters:
            for mode in ("plain", "jacobi"):
                solve(mode, 2)  # warm-up of this mode's kernels right before its window
                torch.cuda.synchronize()
                a, b = events()
                a.record()
                solve(mode, k)
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b)
                emit({"kind": "solve", "run": r, "mode": mode, "max_iter": k, "ms": ms, "ms_per_iter": ms / k})
        for what, fn in (("diag", lambda: prob.diagonal(out=d)), ("product", lambda: prob.matvec(g, y))):
            fn()
            torch.cuda.synchronize()
            a, b = events()
            a.record()
            for _ in range(10):
                fn()
            b.record()
            torch.cuda.synchronize()
            emit({"kind": what, "run": r, "ms": a.elapsed_time(b) / 10})

    if args.val > 0:
        for precond in (None, "jacobi"):
            for k in args.iters:
                m = copy.deepcopy(model)
                clear_val_cache()
                res = lm_step(m, train, val, bg, max_iter=k, restart_iter=k, check_every=False, device=dev,
                              val_at_start=True, cache_val=False, precond=precond)
                emit({"kind": "lm_step", "mode": "plain" if precond is None else "jacobi", "max_iter": k,
                      "alpha": res["best_alpha"], "val_start": res["val_start_loss"], "val_final": res["final_val_loss"],
                      "train_start": res["start_loss"]})
                del m
        clear_val_cache()


if __name__ == "__main__":
    main()
