"""What mrt_render_adaptive buys at full size (DESIGN.md quotes the output).

For each scene: the uniform renders it is measured against (the cap's spp for
the time, `--truth` spp for the error), then for each threshold an adaptive
render to the cap: wall time, mean spp, rounds, the open-tile curve (from the
sample map: a tile with count c left after the round that reached c) and the
relative L2 of the resolved image against the truth. Threshold 0 closes almost
nothing: its time over the uniform render's is what running round by round
costs (a fill and a drain per round). Device buffers throughout; one JSON line
per measurement.

  python tools/adaptive_report.py --scenes sphere_grid,mesh_ply --cap 1024 \
      --thresholds 0,0.02,0.05,0.1 --steps 16,64
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "mass-raytrace_amd", REPO / "tools"):
    sys.path.insert(0, str(p))


def asset_dir(scene: str) -> Path:
    if scene.startswith("mesh") or scene.startswith("menger"):
        from gen_assets import ensure_assets

        return ensure_assets(REPO / "assets", mesh=scene.startswith("mesh"), textures=scene.endswith("textured"),
                             environment=scene.startswith("menger"))
    return REPO / "tests" / "golden"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="sphere_grid,mesh_ply")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--truth", type=int, default=4096, help="spp of the uniform render the error is measured against")
    ap.add_argument("--thresholds", default="0,0.02,0.05,0.1")
    ap.add_argument("--steps", default="16", help="step_spp values")
    ap.add_argument("--min-spp", type=int, default=0, help="min_spp (0: the step)")
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch  # before libmassrt (tests/conftest.py says why)

    torch.cuda.init()
    import massrt

    dev = torch.device("cuda", 0)
    W, H, n = a.width, a.height, a.width * a.height
    for scene in a.scenes.split(","):
        b = massrt.Builder(1).builtin(scene, float(massrt.ASPECT_RATIO), str(asset_dir(scene)))
        ctx = massrt.Context(0)
        ctx.upload(b)

        def buffers():
            return (torch.zeros(n * 3, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                    torch.zeros(n * 2, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))

        def uniform(spp, first):
            rgb, bo, _, _ = buffers()
            torch.cuda.synchronize()
            t = time.perf_counter()
            ctx.render_device(ctx.args(W, H, first, spp, a.seed), rgb.data_ptr(), bo.data_ptr())
            torch.cuda.synchronize()
            return time.perf_counter() - t, rgb

        uniform(16, 0)  # warm-up: buffers planned, kernels loaded
        # the truth from samples the adaptive renders do not use
        t_truth, truth = uniform(a.truth, a.cap)
        truth = truth / a.truth
        norm = float(torch.linalg.vector_norm(truth.double()))
        t_uni, uni = uniform(a.cap, 0)
        err_uni = float(torch.linalg.vector_norm((uni / a.cap - truth).double())) / norm
        print(json.dumps({"scene": scene, "uniform_spp": a.cap, "seconds": round(t_uni, 4), "rel_l2": err_uni,
                          "truth_spp": a.truth, "truth_seconds": round(t_truth, 3)}), flush=True)
        for step in [int(s) for s in a.steps.split(",")]:
            for thr in [float(t) for t in a.thresholds.split(",")]:
                mn = a.min_spp or step
                rgb, bo, mom, smp = buffers()
                res = torch.zeros(n * 3, device=dev)
                torch.cuda.synchronize()
                t = time.perf_counter()
                rep = ctx.render_adaptive_device(ctx.args(W, H, 0, a.cap, a.seed), rgb.data_ptr(), bo.data_ptr(),
                                                 mom.data_ptr(), smp.data_ptr(), min_spp=mn, step_spp=step,
                                                 threshold=thr, floor=a.floor)
                torch.cuda.synchronize()
                secs = time.perf_counter() - t
                ctx.adaptive_resolve_device(W, H, rgb.data_ptr(), smp.data_ptr(), res.data_ptr())
                torch.cuda.synchronize()
                err = float(torch.linalg.vector_norm((res - truth).double())) / norm
                counts = smp.cpu().numpy().astype(np.int64).reshape(H, W)[::8, ::8].reshape(-1)  # one pixel per tile
                done = [min(mn + step * r, a.cap) for r in range(rep["rounds"])]
                curve = [int((counts > d).sum()) for d in done[:-1]] + [rep["tiles_open"]]
                few = curve if len(curve) <= 16 else curve[:: max(1, len(curve) // 16)]
                print(json.dumps({"scene": scene, "threshold": thr, "min_spp": mn, "step_spp": step, "seconds": round(secs, 4),
                                  "vs_uniform": round(secs / t_uni, 3), "mean_spp": round(rep["samples"] / n, 2),
                                  "rounds": rep["rounds"], "tiles": rep["tiles"], "tiles_open": rep["tiles_open"],
                                  "rel_l2": err, "open_curve": few}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
