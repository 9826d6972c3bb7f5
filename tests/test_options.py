"""The context options and their per-scene rules on the host, no GPU
(csrc/host/options.h through tools/options_check.cpp): what mrt_set_option
rejects, and what derive_tuning makes of the options for a scene's facts —
the rules tests/test_gpu_frames.py::test_options_and_tuning sees on the GPU,
and those no scene of the GPU suite reaches (big worlds)."""
import shutil
import subprocess

import pytest

from conftest import REPO

# what the rules know of the benchmark scenes
SPHERE_GRID = ["nf_trees=1"]                                    # L2-resident, no instances
CUBE_FIELD = ["nf_trees=1", "instances=4096"]                   # > 1000 instances, small
MENGER = ["nf_trees=1", "instances=8000", "big=1"]              # big and instanced
MESH_PLY = ["nf_trees=1", "big=1"]                              # big solid


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = tmp_path_factory.mktemp("opt") / "options_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), str(REPO / "tools" / "options_check.cpp")],
                   check=True)

    def run(*args):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        return r.returncode, r.stdout

    return run


def tuning(check, *args):
    rc, out = check(*args)
    assert rc == 0, out
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def test_defaults_before_an_upload(check):
    t = tuning(check)
    assert t["queues"] == 2 and t["pool_paths"] == 384 << 20 and t["results_max"] == 1 << 31
    assert t["finish_paths"] == 500000 and t["finish_grid_div"] == 1 and t["mem_reserve"] == 4096 << 20
    assert t["trace_block"] == 256 and t["treelet_kb"] == 0 and t["shade_batch"] == 16 and t["wgs_per_cu"] == 0
    assert t["traversal"] == 0 and t["trace_prim_batch"] == 1 and t["trace_prim_run"] == 65  # no scene: no NF trees


def test_sphere_grid_rules(check):
    t = tuning(check, *SPHERE_GRID)  # traversal AUTO: the near-first walk and its own rules
    assert t["traversal"] == 1 and t["queues"] == 2
    assert t["trace_box_min"] == 20 and t["trace_chunk"] == 512 and t["shade_waves"] == 7
    assert t["shade_bin"] == 2 and t["trace_refill"] == 40
    assert t["trace_prim_run"] == 32 and t["trace_nf_batch"] == 40
    assert tuning(check, *SPHERE_GRID, "shade_bin=0")["shade_bin"] == 0
    t = tuning(check, *SPHERE_GRID, "traversal=0")  # forced reference walk
    assert t["traversal"] == 0 and t["trace_refill"] == 32 and t["shade_waves"] == 8 and t["shade_bin"] == 1
    assert t["trace_box_min"] == 24 and t["trace_chunk"] == 512 and t["trace_prim_run"] == 65
    t = tuning(check, *SPHERE_GRID, "traversal=1")
    assert t["traversal"] == 1 and t["trace_refill"] == 40 and t["shade_waves"] == 7
    t = tuning(check, *SPHERE_GRID, "traversal=0", "trace_box_min=40")
    assert t["trace_box_min"] == 40


def test_near_first_needs_trees_and_neither_treelet_nor_draws(check):
    assert tuning(check, "traversal=1")["traversal"] == 0
    assert tuning(check, *SPHERE_GRID, "traversal=1", "treelet=1")["traversal"] == 0
    assert tuning(check, *SPHERE_GRID, "traversal=1", "trav_rng=1")["traversal"] == 0


def test_instanced_small_rules(check):
    t = tuning(check, *CUBE_FIELD, "traversal=0")  # > 1000 instances: box run from 16 lanes, grabs of 128
    assert t["trace_box_min"] == 16 and t["trace_chunk"] == 128
    assert t["trace_refill"] == 32  # 12 only for a big instanced world (Menger)
    t = tuning(check, *CUBE_FIELD)
    assert t["traversal"] == 1 and t["trace_box_min"] == 16 and t["trace_chunk"] == 512 and t["trace_refill"] == 40


def test_menger_rules(check):
    t = tuning(check, *MENGER)  # big and instanced: the reference walk, refill 12
    assert t["traversal"] == 0 and t["trace_refill"] == 12
    assert t["trace_box_min"] == 16 and t["trace_chunk"] == 128 and t["shade_waves"] == 8 and t["shade_bin"] == 1
    assert tuning(check, *MENGER, "traversal=1")["traversal"] == 1  # the caller's choice still holds


def test_mesh_ply_rules(check):
    t = tuning(check, *MESH_PLY)  # big solid, near-first
    assert t["traversal"] == 1 and t["trace_refill"] == 32 and t["trace_chunk"] == 256 and t["trace_box_min"] == 20
    assert t["shade_waves"] == 7 and t["shade_bin"] == 2
    t = tuning(check, *MESH_PLY, "traversal=0")
    assert t["trace_refill"] == 32 and t["trace_chunk"] == 128 and t["trace_box_min"] == 32 and t["shade_waves"] == 7


def test_rejected_values(check):
    for name, bad in (("queues", 5), ("trace_block", 300), ("shade_waves", 6), ("trace_chunk", 8), ("trace_nf_batch", 0),
                      ("traversal", 2)):
        rc, out = check(f"{name}={bad}")
        assert rc == 1 and out.startswith("error: ") and name in out, (name, out)
    rc, out = check("no_such_knob=1")
    assert rc == 1 and "unknown option" in out, out


@pytest.mark.parametrize("facts", [SPHERE_GRID, SPHERE_GRID + ["traversal=0"]], ids=["near_first", "reference"])
def test_primitive_run_never_starts_below_the_batch(check, facts):
    """k_trace's primitive-run loop ends only when a pass finds the run over,
    so a pass that finds it on must step the lanes at a primitive: a run that
    is on (<= 64) has prim_run >= prim_batch, whatever the two options say."""
    rc, out = check("prim_sweep", *facts)
    assert rc == 0, out
    rows = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
    assert {(b, r) for b, r, _, _ in rows} == {(b, r) for b in range(1, 65) for r in [-1, *range(1, 66)]}
    for b, r, prim_batch, prim_run in rows:
        assert prim_batch == b, (b, r)
        assert prim_run > 64 or prim_run >= prim_batch, (b, r, prim_batch, prim_run)
        asked = r if r > 0 else (65 if "traversal=0" in facts else 32)  # otherwise the threshold is the caller's
        assert prim_run == (asked if asked > 64 else max(asked, b)), (b, r, prim_run)
