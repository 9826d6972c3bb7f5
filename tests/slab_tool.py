"""tools/slab_check (k_trace's two walks on the host, no GPU) compiled once per test session: the `slab_check`
fixture of tests/test_layout.py and tests/test_adversarial_worlds.py, and how the latter runs it on a world file."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

_built = {}


@pytest.fixture(scope="module")
def slab_check(tmp_path_factory):
    if "exe" not in _built:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # as the Makefile finds it
        if not shutil.which(hipcc):
            pytest.skip("hipcc missing")
        exe = tmp_path_factory.mktemp("slab") / "slab_check"
        lib = REPO / "mass-raytrace_amd" / "massrt"
        subprocess.run([hipcc, "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                        "-o", str(exe), str(REPO / "tools" / "slab_check.cpp"),
                        f"-L{lib}", "-lmassrt", f"-Wl,-rpath,{lib}"], check=True)
        _built["exe"] = exe
    return _built["exe"]


def run(exe, scene, *args, n=0, assets="-", timeout=600):
    """slab_check <scene> <n> <assets> args...; scene: a built-in scene's name or "@" and a world file's path."""
    return subprocess.run([str(exe), str(scene), str(n), str(assets), *[str(a) for a in args]], capture_output=True,
                          text=True, timeout=timeout)


def world_hits(exe, world_file, walk, rays, tmp_path):
    """(hits [n, 4] uint32, near_first [n] bool, {"fallbacks", "starts_ref"}) of `hits` / `hits-nf` on a world
    file, or the failed run (a nonzero exit status: `hits-nf` on a scene without near-first trees)."""
    rays_file, out_file, starts_file = tmp_path / "rays.f32", tmp_path / f"{walk}.u32", tmp_path / f"{walk}.u8"
    np.ascontiguousarray(rays, dtype=np.float32).tofile(rays_file)
    r = run(exe, f"@{world_file}", walk, rays_file, out_file, starts_file)
    if r.returncode != 0:
        return r
    line = [x for x in r.stdout.splitlines() if f" {walk}: " in x][0]
    stats = {k: int(line.split(f"{k} ")[1].split(",")[0]) for k in ("fallbacks", "starts_ref")}
    hits = np.fromfile(out_file, dtype=np.uint32).reshape(-1, 4)
    return hits, np.fromfile(starts_file, dtype=np.uint8).astype(bool), stats
