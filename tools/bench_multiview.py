#!/usr/bin/env python3
"""Multi-view LM products on one GPU: the per-view loop against the batched pass.

Times one CG iteration (cgls_fused, check_every=False: no host synchronisation inside the solve) of the same
problem -- by default 1M Gaussians, SH 3, 5 x 1080p views -- through
  loop     gslm.lm.LMProblem: the whole fused product once per view;
  gshard   a one-rank gslm.parallel.GaussianShardedOperator over LMProblem: the exchange's pipeline with device
           copies in place of its all-to-alls;
  batched  gslm.lm.BatchedLMProblem: gslm_tangent_views, V tile passes, gslm_gather_views;
  batched_active  BatchedLMProblem(union_active=True): the same solve on the Gaussians at least one view can move
           (DESIGN.md §4.5c); also emits Pa and P, and the one-off costs of the list, the pack and the unpack.
  loop_xyz, batched_xyz  `loop` and `batched` with the positions free (mask_xyz=False): the solve moves xyz too.
Every run times the requested modes one after the other in one process (HIP events around a whole solve, the device
synchronised at its end), after untimed solves of every mode that keep the GPU busy for >= 200 ms each (the clock
settle of bench.py).  One JSON line per (run, mode) and one per mode's stage times goes to stdout and, with --out, to
a file.  There is no fallback: without a GPU the tool fails.

  python tools/bench_multiview.py --runs 5 --out profiles/multiview_batched/runs.jsonl
  python tools/bench_multiview.py --P 5000000 --width 3840 --height 2160 --views 32 --iters 5 --runs 3 \
      --modes loop,batched --share-workspaces                  # BASELINE configs[4] whole on one GPU
  python tools/bench_multiview.py --modes loop --pkg <another checkout>/gaussian-splatting-lm_amd   # e.g. the parent
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s0", type=float, default=0.005)
    ap.add_argument("--iters", type=int, default=10, help="CG iterations per timed solve")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--stage-reps", type=int, default=10)
    ap.add_argument("--modes", default="loop,gshard,batched")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "gaussian-splatting-lm_amd"),
                    help="the package directory to import gslm from (its build/libgslm.so is loaded)")
    ap.add_argument("--share-workspaces", action="store_true",
                    help="the modes' problems share one set of per-view workspaces, weights and seeds (the same "
                         "geometry, so the same row maps): sizes whose workspaces fit the GPU only once")
    ap.add_argument("--label", default="", help="copied into every line (e.g. the commit)")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main():
    args = parse()
    sys.path.insert(0, args.pkg)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiview.py needs the GPU: a CPU run has no timing to report")
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem, cgls_fused
    from gslm.model import synthetic_gaussians
    dev = torch.device("cuda", 0)
    modes = [m for m in args.modes.split(",") if m]
    out = open(args.out, "a") if args.out else None

    def emit(line):
        line = dict(line, label=args.label, P=args.P, sh=args.sh, views=args.views, width=args.width,
                    height=args.height, iters=args.iters)
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    V, W, H = args.views, args.width, args.height
    cams = [c.to(dev) for c in orbit_cameras(V, W, H, seed=1)]
    bg = torch.zeros(3)
    # ground truth as in bench.py: the render of the model with f_dc / opacity / scaling perturbed by N(0, 0.01^2)
    pert = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=V)
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        pert._features_dc += 0.01 * torch.randn(pert._features_dc.shape, generator=g2)
        pert._opacity += 0.01 * torch.randn(pert._opacity.shape, generator=g2)
        pert._scaling += 0.01 * torch.randn(pert._scaling.shape, generator=g2)
    pert.to(dev)
    gt = LMProblem(pert, cams, bg, device=dev)
    gt.evaluate()
    for c, vr in zip(cams, gt.views):
        c.original_image = vr.color.clamp(0, 1).clone()
    del gt, pert
    torch.cuda.empty_cache()
    model = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=V).to(dev)

    probs = {}
    for m in modes:
        if m in ("loop", "loop_xyz"):
            p = LMProblem(model, cams, bg, device=dev, sh_projection=False, mask_xyz=(m == "loop"))
        elif m == "gshard":
            from gslm.parallel import GaussianShardedOperator
            p = GaussianShardedOperator(LMProblem(model, cams, bg, device=dev, sh_projection=False), all_cams=cams)
        elif m in ("batched", "batched_xyz"):
            from gslm import lm
            p = (lm.BatchedLMProblem if m == "batched" else lm.BatchedXyzLMProblem)(model, cams, bg, device=dev)
        elif m == "batched_active":
            from gslm.lm import BatchedLMProblem
            p = BatchedLMProblem(model, cams, bg, device=dev, union_active=True)
        else:
            raise SystemExit(f"unknown mode {m!r}")
        base = next(iter(probs.values()))[0] if (args.share_workspaces and probs) else None
        if base is None:
            p.evaluate()
        else:
            # the first problem's forwards, residual weights and seeds serve this one too; what it adds of its own
            # per geometry (BatchedLMProblem.evaluate: the views' visibility words) is done on the shared geometry
            for name in ("views", "weights", "residuals", "seeds", "loss"):
                setattr(p, name, getattr(base, name))
            if hasattr(p, "_flags"):
                from gslm._lib import check, lib
                for b, vr in enumerate(p.views):
                    check(lib.gslm_view_flags(vr.geom.data_ptr(), p.layout.P, p._flags[b].data_ptr(), p.stream),
                          "gslm_view_flags")
        probs[m] = (p, p.rhs(p.zeros()))
    torch.cuda.synchronize()
    first = probs[modes[0]][0]
    emit({"kind": "scene", "num_rendered": [int(n) for n in first.num_rendered()],
          "floats_per_gaussian": {m: p.layout.floats_per_gaussian for m, (p, _) in probs.items()}})

    def solve(m, iters):
        p, g = probs[m]
        return cgls_fused(p, g, max_iter=iters, restart_iter=iters, check_every=False)

    # clock settle: untimed solves of every mode, >= 200 ms each (the first call also allocates the CG vectors)
    for m in modes:
        t0 = time.perf_counter()
        n = 0
        while n < 2 or time.perf_counter() - t0 < 0.2:
            solve(m, args.iters)
            torch.cuda.synchronize()
            n += 1
        emit({"kind": "settle", "mode": m, "solves": n, "ms": 1e3 * (time.perf_counter() - t0)})

    xs = {}
    for r in range(args.runs):
        for m in modes:
            solve(m, 3)  # warm-up of this mode's kernels right before its window
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            x, _ = solve(m, args.iters)
            e1.record()
            torch.cuda.synchronize()
            xs[m] = x
            emit({"kind": "cg", "run": r, "mode": m, "ms_per_iter": e0.elapsed_time(e1) / args.iters})

    # the solves agree (each against the first mode that solves the same problem -- xyz masked or free -- in the
    # reference's layout)
    def full(m):
        p = probs[m][0]
        return p.gather_full(xs[m]) if getattr(p, "exchange", None) == "gaussian" else p.expand(xs[m])

    firsts = {}
    for m in modes:
        m0 = firsts.setdefault(m.endswith("_xyz"), m)
        if m0 != m:
            ref = full(m0)
            emit({"kind": "agreement", "mode": m, "against": m0, "rel_norm": float((full(m) - ref).norm() / ref.norm())})

    def timed(fn, reps):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1) / reps

    # per-stage times of one product (events between the stages), direction = the right-hand side
    for m in modes:
        p, g = probs[m]
        if m == "batched_active":
            # the list's size and what it costs once per geometry (the list) and once per solve (pack, unpack)
            def build():
                p._union = None
                return p.union_list()

            (_, Pa, _, _), t_list = timed(build, 5)
            act = p.active_view()
            if act is None:
                raise SystemExit("batched_active: no active view (GSLM_CG_ACTIVE=0, or nothing visible)")
            gp, t_pack = timed(lambda: act.pack(g), args.stage_reps)
            _, t_unpack = timed(lambda: act.unpack(gp), args.stage_reps)
            emit({"kind": "active", "mode": m, "Pa": int(Pa), "P_total": int(p.full_layout.P),
                  "ratio": Pa / max(p.full_layout.P, 1), "union_list_ms": t_list, "pack_ms": t_pack,
                  "unpack_ms": t_unpack})
            emit({"kind": "stages", "mode": m, "ms": act.stage_times(gp, reps=args.stage_reps)})
        elif hasattr(p, "stage_times"):
            emit({"kind": "stages", "mode": m, "ms": p.stage_times(g.clone(), reps=args.stage_reps)})
        else:
            y = p.zeros()
            v = g.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            p.matvec(v, y)
            e0.record()
            for _ in range(args.stage_reps):
                p.matvec(v, y)
            e1.record()
            torch.cuda.synchronize()
            emit({"kind": "stages", "mode": m, "ms": {"total": e0.elapsed_time(e1) / args.stage_reps}})
    if out:
        out.close()


if __name__ == "__main__":
    main()
