"""rays_time — mrt_render_rays_device on the camera's own rays against
mrt_render_device of that frame.

    python tools/rays_time.py [--scenes sphere_grid,mesh_ply] [--width 1920 --height 1080 --spp 16] [--out FILE.json]

Per scene the table holds the built-in camera's sample-0 ray of every pixel
(mrt_camera_rays: key = the pixel, skip = the ray's draws), on the device; one
call renders --spp samples of every entry, where the frame's call computes the
camera rays in its generation kernels. The two are not the same image (the
frame draws a new ray per sample), but the same number of paths through the
same scene from the same place. Per contender 2 warm-ups, then --runs timed
runs, the two alternating within this process, each run between two HIP events
on the caller's stream (torch's current stream). Prints one JSON line per
scene: both medians, min and max in ms, Msamples/s, and rays over frame.
--only rays|frame runs one contender alone (a build without the other).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "mass-raytrace_amd", REPO / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="sphere_grid,mesh_ply")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=("rays", "frame"), default=None)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py), then libmassrt
    import massrt
    from gen_assets import ensure_assets

    assets = ensure_assets(REPO / "assets", mesh=True, textures=False, environment=False)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    W, H, spp = a.width, a.height, a.spp
    n = W * H
    lines = []
    for scene in a.scenes.split(","):
        ctx = massrt.Context(0, options=massrt.env_options())
        b = massrt.Builder(1).builtin(scene, float(massrt.ASPECT_RATIO), assets)
        ctx.upload(b)
        rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        bo = torch.zeros(n, dtype=torch.int32, device=dev)
        contenders = []
        if a.only != "frame":
            _, cam = b.desc()
            e = massrt.camera_rays(cam, W, H, np.arange(n, dtype=np.uint32), seed=1, sample=0)
            d_rays = torch.from_numpy(e.view(np.uint8).copy()).to(dev)
            contenders.append(("rays", lambda: ctx.render_rays_device(d_rays.data_ptr(), n, 1, 0, spp, massrt.MAX_DEPTH,
                                                                      0, rgb.data_ptr(), bo.data_ptr(), stream)))
        if a.only != "rays":
            args = ctx.args(W, H, 0, spp, 1)
            contenders.append(("frame", lambda: ctx.render_device(args, rgb.data_ptr(), bo.data_ptr(), stream)))

        def timed(f):
            rgb.zero_()
            bo.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        ms = {name: [] for name, _ in contenders}
        for it in range(a.warmup + a.runs):
            for name, f in contenders:
                t = timed(f)
                if it >= a.warmup:
                    ms[name].append(t)
        line = {"scene": scene, "width": W, "height": H, "spp": spp, "build": massrt.build_info(),
                "tuning": ctx.tuning()}
        for name, t in ms.items():
            med = statistics.median(t)
            line[name + "_ms"] = {"median": med, "min": min(t), "max": max(t), "runs": t,
                                  "msamples_per_s": n * spp / med / 1e3}
        if len(ms) == 2:
            line["rays_over_frame"] = line["rays_ms"]["median"] / line["frame_ms"]["median"]
        lines.append(line)
        print(json.dumps(line), flush=True)
        del rgb, bo
        ctx.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
