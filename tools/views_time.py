"""views_time — one mrt_render_views_device call against the loop of
mrt_set_camera + mrt_render_device calls over the same device buffers.

    python tools/views_time.py [--scenes sphere_grid,mesh_ply] [--out FILE.json]

Two sizes per scene: 64 views of 480x270 at 16 spp (animation frames) and 16
views of 1920x1080 at 14 spp. The cameras stand on a circle around the
built-in's look_at. Per contender 3 warm-ups, then 3 timed runs, the two
alternating within this process, each run between two HIP events on the
caller's stream (torch's current stream). Prints one JSON line per (scene,
size): both medians, min and max in ms, the ratio of the medians, and whether
the buffers of the two came out bit-identical.
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "mass-raytrace_amd", REPO / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

SIZES = [(64, 480, 270, 16), (16, 1920, 1080, 14)]
LOOK = {"sphere_grid": ((6.0, 8.0, 5.0), (0.0, 0.0, 0.0)), "mesh_ply": ((0.0, 3.2, 6.5), (0.0, -0.2, 0.0))}


def orbit(massrt, scene, n):
    (fx, fy, fz), at = LOOK[scene]
    dx, dz = fx - at[0], fz - at[2]
    views = []
    for v in range(n):
        phi = 2.0 * math.pi * v / n
        look_from = (at[0] + dx * math.cos(phi) + dz * math.sin(phi), fy, at[2] - dx * math.sin(phi) + dz * math.cos(phi))
        views.append(massrt.MrtView(massrt.make_camera(40.0, look_from, at), 1 + v))
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="sphere_grid,mesh_ply")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py), then libmassrt
    import massrt
    from gen_assets import ensure_assets

    assets = ensure_assets(REPO / "assets", mesh=True, textures=False, environment=False)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    for scene in a.scenes.split(","):
        ctx = massrt.Context(0, options=massrt.env_options())
        ctx.upload(massrt.Builder(1).builtin(scene, float(massrt.ASPECT_RATIO), assets))
        for V, W, H, spp in SIZES:
            views = orbit(massrt, scene, V)
            rgb = torch.zeros(V * W * H * 3, dtype=torch.float32, device=dev)
            bo = torch.zeros(V * W * H, dtype=torch.int32, device=dev)
            args = ctx.args(W, H, 0, spp, 0)

            def one_call():
                ctx.render_views_device(args, views, rgb.data_ptr(), bo.data_ptr(), stream)

            def loop():
                for v, view in enumerate(views):
                    ctx.set_camera(view.camera)
                    av = ctx.args(W, H, 0, spp, view.seed)
                    ctx.render_device(av, rgb.data_ptr() + v * W * H * 12, bo.data_ptr() + v * W * H * 4, stream)

            def timed(f):
                rgb.zero_()
                bo.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            ms = {"views": [], "loop": []}
            keep = {}
            for it in range(a.warmup + a.runs):
                for name, f in (("views", one_call), ("loop", loop)):
                    t = timed(f)
                    if it >= a.warmup:
                        ms[name].append(t)
                    if it == 0:
                        keep[name] = (rgb.clone(), bo.clone())
            same = bool(torch.equal(keep["views"][0].view(torch.int32), keep["loop"][0].view(torch.int32))
                        and torch.equal(keep["views"][1], keep["loop"][1]))
            line = {"scene": scene, "views": V, "width": W, "height": H, "spp": spp, "build": massrt.build_info(),
                    "bit_identical": same}
            for name, t in ms.items():
                line[name + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t), "runs": t}
            line["loop_over_views"] = line["loop_ms"]["median"] / line["views_ms"]["median"]
            lines.append(line)
            print(json.dumps(line), flush=True)
            del rgb, bo, keep
        ctx.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
