"""The record-stream layout (layout.h, upload.cpp relayout_blas) on the host,
no GPU: the same rays through the preorder stream (build_host_scene(..., sibling_layout=false)) and
through the default layout (BLAS regions with siblings together, every
successor explicit) find the same closest hits, t bits included, after the
same number of box tests; the early slab decision stays exact
(tools/slab_check.cpp, which runs k_trace's own walk code, compiled for the
host, one ray at a time); and both walks' closest hits equal the oracle's."""
import subprocess

import numpy as np
import pytest

import adversarial_rays
import massrt
import oracle
from conftest import GOLDEN
from ray_gen import camera_rays, random_rays
from slab_tool import slab_check  # noqa: F401 (the fixture: tools/slab_check compiled for the host)


@pytest.mark.parametrize("scene", ["cornell", "sphere_grid", "cube_field"])
def test_sibling_layout_walks_like_the_preorder_stream(slab_check, scene):
    r = subprocess.run([str(slab_check), scene, "20000", str(GOLDEN), "layout"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 of 20000 rays differ" in r.stdout, r.stdout


@pytest.mark.parametrize("scene", ["cornell", "sphere_grid", "cube_field"])
def test_stream_mode_treelet_sizes(slab_check, scene):
    """slab_check's `stream` mode (element counts and hashes of what the host builds, both layouts) and what
    upload.h states for build_treelet: budget 0 gives no treelet; a budget the whole stream fits gives a treelet
    of every record, its slot count the sum of the record sizes of rec_starts; slots_tl has the size of slots at
    every other budget. That sum is the preorder stream's length up to the near-first trees (its nf_first_slot):
    the preorder layout has no padding between records, and the sibling layout holds the same records.
    No hash is compared: they are bound to one toolchain."""
    r = subprocess.run([str(slab_check), scene, "0", str(GOLDEN), "stream"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words, value = {}, {}  # (layout, item, budget) -> 32-bit elements; a scalar's value
    for line in r.stdout.splitlines():
        name, layout, item, budget, n, digest, val = line.split()
        key = layout, item, None if budget == "-" else int(budget)
        assert name == scene and len(digest) == 16 and key not in words, line
        words[key] = int(n)
        if val != "-":
            value[key] = int(val)
    record_slots = value["preorder", "nf_first_slot", None]
    assert value["preorder", "nf_ok", None] == 1 and record_slots > 0
    for layout in ("sibling", "preorder"):
        n_words = words[layout, "slots", None]
        assert n_words % 4 == 0 and n_words // 4 > record_slots  # the near-first trees follow the records
        budgets = sorted(b for (lay, item, b) in words if lay == layout and item == "tlet")
        assert budgets == sorted({0, 64, 1536, 4992, n_words // 4}), budgets
        assert words[layout, "tlet", 0] == 0 and words[layout, "slots_tl", 0] == 0
        for b in budgets[1:]:
            assert words[layout, "slots_tl", b] == n_words, (layout, b)
            assert 0 < words[layout, "tlet", b] <= 4 * b, (layout, b)
        assert words[layout, "tlet", n_words // 4] == 4 * record_slots, layout


@pytest.mark.slow
def test_sibling_layout_mesh(slab_check, assets_dir):
    r = subprocess.run([str(slab_check), "mesh_ply", "20000", str(assets_dir), "layout"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and " 0 of 20000 rays differ" in r.stdout, r.stdout + r.stderr


def _bound(stdout: str):
    """(checks, worst dist/rho, over) from slab_check's `nf bound:` line."""
    line = [x for x in stdout.splitlines() if " nf bound: " in x][0]
    checks = int(line.split("nf bound: ")[1].split(" accepted")[0])
    worst = float(line.split("worst dist/rho ")[1].split(",")[0])
    over = int(line.split(" over;")[0].rsplit(", ", 1)[1])
    return checks, worst, over, line


@pytest.mark.parametrize("scene", ["cornell", "sphere_grid", "cube_field"])
def test_near_first_walk_finds_the_reference_hits(slab_check, scene):
    """The verified near-first walk (nf_tree.cpp's trees, walk_nf.h's steps,
    which tools/slab_check.cpp walk_nf runs on the host): on camera and bounce rays the
    same closest hits as the reference's left-first walk — primitive,
    container, t bits — with fewer record loads; the stack stays within
    kNfStack. Every hit the reference's tests accept lies within the walk's
    rounding margin rho of its box (nf_bound.h)."""
    r = subprocess.run([str(slab_check), scene, "30000", str(GOLDEN), "nf"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " nf: 0 of 30000 rays differ" in r.stdout, r.stdout
    loads = r.stdout.split("record loads ")[1].split(" (x")[0].split(" vs ")
    assert float(loads[0]) < float(loads[1]), r.stdout
    checks, worst, over, line = _bound(r.stdout)
    assert checks > 10000 and over == 0 and worst < 0.25, line


@pytest.mark.slow
@pytest.mark.parametrize("scene", ["mesh_ply", "menger_l3"])
def test_near_first_walk_mesh_and_menger(slab_check, assets_dir, scene):
    r = subprocess.run([str(slab_check), scene, "20000", str(assets_dir), "nf"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and " nf: 0 of 20000 rays differ" in r.stdout, r.stdout + r.stderr
    checks, worst, over, line = _bound(r.stdout)
    assert over == 0 and worst < 0.25, line
    if scene == "mesh_ply":  # normal cones (nf_bound.h nf_cone_rg): the generic term priced per node
        cones = [x for x in r.stdout.splitlines() if " nf cones: " in x][0]
        assert int(cones.split("nf cones: ")[1].split(" of")[0]) > 100_000, cones
        per_ray = float(r.stdout.split(" box tests ")[1].split(" vs")[0])
        assert per_ray < 42.0, r.stdout  # 64.6 with the worst-case |det| >= 1e-6 pricing, 43.7 before wild entries
        # the floor and the two thin light boxes are wild (nf_bound.h NfWild): each is entered only when the
        # ray meets its world box thickened by its own margin, so the walk enters fewer instances than the
        # reference's (3.0 per ray while the nodes above them never culled them)
        _wild_checked(r.stdout, 3)
        entries = float(r.stdout.split("instance entries per ray ")[1].split()[0])
        ref_entries = float(r.stdout.split("reference walk: instance entries per ray ")[1].split()[0])
        assert entries < ref_entries and entries < 1.0, r.stdout


def _wild_checked(stdout: str, n_wild: int):
    """slab_check's wild lines: n_wild wild instances, every accepted hit of one within its own margin of its
    world box (check_hit_wild), and rays that pass them by on that test."""
    assert f", {n_wild} wild instances" in stdout, stdout
    line = [x for x in stdout.splitlines() if " nf wild: " in x][0]
    assert int(line.split("nf wild: ")[1].split(" hits")[0]) > 100, line
    assert float(line.split("worst dist/rho ")[1]) < 0.25, line
    passed = float(stdout.split("nf wild instances passed by per ray ")[1].split()[0].rstrip(";"))
    assert passed > 0.1, stdout


def test_wild_instance_cornell(slab_check):
    """Cornell's thin light (cond |F||G| ~ 1.4e4: a wild instance, nf_tree.cpp wild()): its hits lie within its
    own instance term of its world box, which the walk tests at the wild leaf (walk_nf.h nf_wild_enter) instead of
    entering it on every ray; the closest hits stay the reference's."""
    r = subprocess.run([str(slab_check), "cornell", "30000", str(GOLDEN), "nf"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and " nf: 0 of 30000 rays differ" in r.stdout, r.stdout + r.stderr
    _wild_checked(r.stdout, 1)


@pytest.mark.slow
def test_near_first_grazing_rays_mesh_cones(slab_check, assets_dir):
    """The 1M-triangle mesh's generic triangles under the normal-cone bound
    (round 6): rays within 10^-8..10^-1.5 rad of a triangle's plane sit in
    the cone's grazing band, where each node falls back to the worst-case
    |det| >= 1e-6 term; every accepted hit still lies within the (cone-
    narrowed) rho of every NF node above it, and no closest hit differs."""
    r = subprocess.run([str(slab_check), "mesh_ply", "20000", str(assets_dir), "graze"], capture_output=True,
                       text=True, timeout=900)
    line = [x for x in r.stdout.splitlines() if " nf: " in x][0]
    assert " nf: 0 of 20000 rays differ" in line, line
    checks, worst, over, bline = _bound(r.stdout)
    assert checks > 20000 and over == 0 and worst < 0.25, bline
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("scene", ["cornell", "cube_field", "sphere_grid"])
def test_near_first_grazing_rays(slab_check, scene):
    """The near-first walk's hardest rays (massrt.h MRT_TRAVERSAL_*, DESIGN.md
    §4): nearly parallel to a triangle (10^-8 to 10^-1.5 rad), where
    Moller-Trumbore's computed t is least accurate. The walk thickens every
    box by its proven bound rho on how far a computed hit can lie outside its
    primitive's box (nf_bound.h): every accepted hit of the sample lies within
    rho of its box, with room to spare (worst dist/rho < 0.25), and no ray's
    closest hit differs."""
    r = subprocess.run([str(slab_check), scene, "100000", str(GOLDEN), "graze"], capture_output=True, text=True,
                       timeout=600)
    line = [x for x in r.stdout.splitlines() if " nf: " in x][0]
    assert " nf: 0 of 100000 rays differ" in line, line
    checks, worst, over, bline = _bound(r.stdout)
    assert checks > 100000 and over == 0 and worst < 0.25, bline
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("scene", ["sphere_grid"])
def test_near_first_tangent_rays(slab_check, scene):
    """Rays nearly tangent to a sphere from 1-400 radii (the sphere test's
    disc cancels there): the same hits as the reference walk, and every
    accepted hit within the sphere bound's rho of its box."""
    r = subprocess.run([str(slab_check), scene, "100000", str(GOLDEN), "tangent"], capture_output=True, text=True,
                       timeout=600)
    line = [x for x in r.stdout.splitlines() if " nf: " in x][0]
    assert " nf: 0 of 100000 rays differ" in line, line
    checks, worst, over, bline = _bound(r.stdout)
    assert checks > 100000 and over == 0 and worst < 0.25, bline


# ---- the walks' closest hits against the oracle, on the host ---------------------
# tests/test_gpu_parity.py's test_golden_rays_bit_exact and test_trace_rays_bit_exact
# without a GPU, on the code the GPU runs: slab_check's `hits` / `hits-nf` modes are
# k_rays_in -> the reference's / the near-first walk -> k_rays_out, one ray at a time.
SMALL = ["cornell", "sphere_grid", "cube_field"]
WALKS = ["hits", "hits-nf"]


def _host_hits(slab_check, scene, walk, rays, tmp_path):
    rays_file, out_file = tmp_path / "rays.f32", tmp_path / f"{walk}.u32"
    np.ascontiguousarray(rays, dtype=np.float32).tofile(rays_file)
    r = subprocess.run([str(slab_check), scene, "0", str(GOLDEN), walk, str(rays_file), str(out_file)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(out_file, dtype=np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("scene", SMALL)
def test_host_walks_golden_rays_bit_exact(slab_check, scene, tmp_path):
    g = np.load(GOLDEN / "oracle_golden.npz")
    for walk in WALKS:
        hits = _host_hits(slab_check, scene, walk, g["rays"], tmp_path)
        assert np.array_equal(hits, g[f"{scene}_hits"]), f"{walk}: {int((hits != g[f'{scene}_hits']).any(1).sum())} rays differ"


@pytest.mark.parametrize("scene", SMALL)
def test_host_walks_equal_the_oracle(slab_check, scene, tmp_path):
    """20,000 random and 20,000 camera rays: primitive, container, t bits and
    front face of both walks equal oracle.Scene.trace_rays."""
    aspect = float(massrt.ASPECT_RATIO)
    _, cam = massrt.Builder(1).builtin(scene, aspect, GOLDEN).desc()
    rays = np.concatenate([random_rays(20_000, 1), camera_rays(cam, 20_000, 2)])
    want = oracle.Scene(1).builtin(scene, aspect, GOLDEN).trace_rays(rays)
    assert int((want[:, 0] != 0).sum()) > 5_000  # the sample hits something
    for walk in WALKS:
        hits = _host_hits(slab_check, scene, walk, rays, tmp_path)
        assert np.array_equal(hits, want), f"{walk}: {int((hits != want).any(1).sum())} rays differ"


# ---- adversarial rays (tests/adversarial_rays.py): zero and tiny direction components, origins on box
# planes, box corners, triangle edges, sphere centres and tangents, |d| from 2^-120 to 2^100, origins up
# to 1e38 away, NaN and infinities. The reference's own arithmetic overflows on some of them and accepts
# hits whose t is NaN; both walks must return exactly what the oracle does.
@pytest.fixture(scope="module")
def adversarial():
    """scene -> (rays of all families, (family, begin, end) offsets, the oracle's hits), computed once per scene;
    the oracle's answers hold enough hits per family to prove something (adversarial_rays.check_floors)."""
    cache = {}

    def get(scene):
        if scene not in cache:
            aspect = float(massrt.ASPECT_RATIO)
            b = massrt.Builder(1).builtin(scene, aspect, GOLDEN)  # desc() points into the builder: kept until used
            rays, parts = adversarial_rays.split(adversarial_rays.families(*b.desc()))
            want = oracle.Scene(1).builtin(scene, aspect, GOLDEN).trace_rays(rays)
            cache[scene] = rays, parts, want
        return cache[scene]
    return get


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("scene", SMALL)
def test_host_walks_adversarial_rays(slab_check, adversarial, scene, walk, tmp_path):
    """Every family through one run of the host walk: all four words of every ray equal the oracle's."""
    rays, parts, want = adversarial(scene)
    assert {name for name, _, _ in parts} == {f.__name__ for f in adversarial_rays.FAMILIES}
    adversarial_rays.check_floors({name: want[a:e] for name, a, e in parts}, overflow=scene != "cube_field")
    hits = _host_hits(slab_check, scene, walk, rays, tmp_path)
    assert hits.shape == want.shape
    bad = [m for m in (adversarial_rays.first_difference(name, rays[a:e], hits[a:e], want[a:e]) for name, a, e in parts)
           if m]
    assert not bad, f"{walk} on {scene}:\n" + "\n".join(bad)
