"""A plain `bench.py --gpus 1 --steps N --warmup W` run: the result line it
prints, that it runs the headline scene only (everything else is `--full`'s),
and `--dump-outputs`: the image the last timed step left, bit for bit what the
same mrt_image_render calls give in this process. One small frame, one child
process (bench.py is the thing under test).
"""
import json
import subprocess
import sys

import numpy as np
import pytest

import massrt
from conftest import REPO

pytestmark = pytest.mark.gpu
W, H, SPP, STEPS, WARMUP = 96, 54, 8, 3, 1


def test_plain_run_line_and_dumped_outputs(golden_dir, tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--width", str(W), "--height", str(H), "--spp-per-step", str(SPP),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("Msamples/sec")
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    # value = samples of a step / the time of a step (both rounded to 3 decimals in the line)
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(W * H * SPP / line["ms_per_step"] / 1e3, rel=1e-2)
    # a plain run: the headline scene alone
    assert line["config"]["scene"] == "sphere_grid" and line["cpu_baseline"] is None
    assert not {"secondary", "c1", "c3", "c5", "dropin", "walks"} & set(line["config"])
    assert line["build"]["match"] is True

    rgb, bounces, passes = (np.load(out / f"{n}.npy") for n in ("rgb", "bounces", "passes"))
    assert sorted(p.name for p in out.iterdir()) == ["bounces.npy", "passes.npy", "rgb.npy"]
    assert rgb.dtype == np.float32 and rgb.shape == (H, W, 3)
    assert bounces.dtype == np.float64 and bounces.shape == (H, W) and passes.dtype == np.float64
    # the image accumulates every step, warmup included: the same calls here
    c = massrt.Context(0)
    try:
        b = massrt.Builder(1).builtin("sphere_grid", float(massrt.ASPECT_RATIO), golden_dir)
        c.upload(b)
        b.close()
        img = massrt.Image(c, W, H)
        for k in range(WARMUP + STEPS):
            img.render(1, k * SPP, SPP)
            img.gather()
        ergb, eb, ep = img.read()
        img.close()
    finally:
        c.close()
    assert passes.tolist() == [ep] == [(WARMUP + STEPS) * SPP]
    assert np.array_equal(bounces.ravel(), eb.astype(np.float64))
    assert np.array_equal(rgb.ravel().view(np.uint32), ergb.view(np.uint32))
