"""Wild instances last, on the device (nf_tree.cpp, walk.h nf_start): the
wild instances' own tree is pushed to the bottom of a near-first ray's stack
and walked after everything else. The closest hits stay the oracle's —
primitive, container, t bits, front face — whatever the wild tree's shape, and
the walk enters a wild instance only where it can still hold the closest hit."""
import numpy as np
import pytest

import massrt
import oracle
from test_gpu_parity import ASPECT, RTOL, build_both, camera_rays, rel_l2

pytestmark = pytest.mark.gpu

NO_MAT = massrt.NO_MATERIAL


@pytest.fixture(scope="module")
def nf_ctx():
    c = massrt.Context(0, options={"traversal": massrt.TRAVERSAL_NEAR_FIRST})
    yield c
    c.close()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_sphere_grid_camera_rays_enter_the_ground_only_to_hit_it(nf_ctx, golden_dir):
    """Every camera ray of sphere_grid's view ends on a sphere or on the ground (the wild 1000x cube). With the
    wild leaf last its own box test runs at the sphere's t, so only the rays that hit the ground enter it; while
    it was a leaf of the world tree every ray did."""
    b = massrt.Builder(1).builtin("sphere_grid", ASPECT, golden_dir)
    o = oracle.Scene(1).builtin("sphere_grid", ASPECT, golden_dir)
    nf_ctx.upload(b)
    assert nf_ctx.tuning()["traversal"] == massrt.TRAVERSAL_NEAR_FIRST
    _, cam = b.desc()
    rays = camera_rays(cam, 60_000, 12)
    nf_ctx.reset_counters()
    gh, oh = nf_ctx.trace_rays(rays), o.trace_rays(rays)
    assert np.array_equal(gh, oh), f"{int((gh != oh).any(1).sum())} rays differ"
    in_container = int((oh[:, 1] >> 28 != 0).sum())
    entries = nf_ctx.counters()["instance_entries"]
    print(f"instance entries {entries}, rays whose hit has a container {in_container}, of {len(rays)}")
    assert 0 < in_container < len(rays)
    assert entries == in_container


def _slab(x, cube, k, mat):
    # wild by its condition number: 12 x 0.004 x 9 (nf_tree.cpp wild())
    x.add_instance(cube, (0.7 * k - 2.0, 0.3 * k - 0.6, -0.5 * k), (0.1 * k, 0.05, 0.02 * k), (12.0, 0.004, 9.0), mat)


def _only_wild(n):
    def scene(x, golden_dir):
        x.background(massrt.BG_SKY)
        lam = x.material(massrt.MAT_LAMBERTIAN, x.solid(0.6, 0.5, 0.4))
        glow = x.material(massrt.MAT_DIFFUSE_LIGHT, 0, 0.0, (4.0, 4.0, 4.0))
        cube = x.model_from_ply(golden_dir / "cube.ply", lam)
        for k in range(n):
            _slab(x, cube, k, glow if k % 2 else NO_MAT)
        x.build_bvh()
        x.camera(45.0, (0.5, 1.5, 7), (0, 0, 0), aspect=ASPECT)
    return scene


def _slabs_around_a_sphere(x, golden_dir):
    """Seen from the camera and from most random rays: a wild slab in front of the sphere (the wild instance is
    the closest hit, found last) and one behind it (the wild instance is occluded: its leaf test fails)."""
    x.background(massrt.BG_SKY)
    lam = x.material(massrt.MAT_LAMBERTIAN, x.solid(0.6, 0.5, 0.4))
    cube = x.model_from_ply(golden_dir / "cube.ply", lam)
    x.add_instance(cube, (0.0, 0.0, 2.5), (0.0, 0.0, 0.0), (3.0, 3.0, 0.001), NO_MAT)
    x.add_sphere(x.material(massrt.MAT_METAL, x.solid(0.8, 0.8, 0.8), 0.1), (0.0, 0.0, 0.0), 1.0)
    x.add_instance(cube, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0), (6.0, 6.0, 0.001), NO_MAT)
    x.build_bvh()
    x.camera(45.0, (0.3, 0.4, 9), (0, 0, 0), aspect=ASPECT)


def _mixed(order, n_cubes):
    """Six overlapping wild slabs added in `order`, n_cubes ordinary cubes and four spheres. With more than
    kNfWildFew (16) instances only the condition number makes an instance wild."""
    def scene(x, golden_dir):
        x.background(massrt.BG_SKY)
        lam = x.material(massrt.MAT_LAMBERTIAN, x.solid(0.6, 0.5, 0.4))
        glow = x.material(massrt.MAT_DIFFUSE_LIGHT, 0, 0.0, (4.0, 4.0, 4.0))
        cube = x.model_from_ply(golden_dir / "cube.ply", lam)
        for k in order:
            _slab(x, cube, k, glow if k % 2 else NO_MAT)
        for k in range(n_cubes):
            x.add_instance(cube, (1.1 * (k % 5) - 2.0, 0.2 + 0.9 * (k // 5), 1.0 - 0.4 * (k % 5)), (0.0, 0.13 * k, 0.0),
                           (0.4, 0.4, 0.4))
        for k in range(4):
            x.add_sphere(x.material(massrt.MAT_METAL, x.solid(0.8, 0.8, 0.8), 0.1), (k - 1.5, -0.2, 0.3 * k), 0.35)
        x.build_bvh()
        x.camera(45.0, (0.5, 1.5, 7), (0, 0, 0), aspect=ASPECT)
    return scene


WORLDS = {
    "one_wild_slab_alone": _only_wild(1),
    "only_wild_slabs": _only_wild(3),
    "slab_before_and_behind_a_sphere": _slabs_around_a_sphere,
    "six_slabs_cubes_spheres": _mixed(range(6), 5),
    "six_slabs_reversed": _mixed(range(5, -1, -1), 5),
    "six_slabs_shuffled": _mixed([3, 0, 5, 1, 4, 2], 5),
    "eighteen_instances": _mixed(range(6), 12),
}


@pytest.mark.parametrize("world", list(WORLDS))
def test_built_worlds_equal_the_oracle(nf_ctx, golden_dir, world):
    b, o = build_both(lambda x: WORLDS[world](x, golden_dir))
    nf_ctx.upload(b)
    assert nf_ctx.tuning()["traversal"] == massrt.TRAVERSAL_NEAR_FIRST
    r = np.random.default_rng(5)
    # from everywhere, and grazing the slabs (nearly in their y = const planes)
    o1, d1 = r.uniform(-4, 4, (30_000, 3)), r.normal(size=(30_000, 3))
    o2 = np.concatenate([r.uniform(-6, 6, (30_000, 1)), r.uniform(-1, 1, (30_000, 1)), r.uniform(-6, 6, (30_000, 1))], 1)
    d2 = np.concatenate([r.normal(size=(30_000, 1)), r.normal(size=(30_000, 1)) * 1e-3, r.normal(size=(30_000, 1))], 1)
    rays = np.concatenate([np.concatenate([o1, d1], 1), np.concatenate([o2, d2], 1)]).astype(np.float32)
    g, ob = nf_ctx.trace_rays(rays), o.trace_rays(rays)
    assert (ob[:, 1] >> 28 != 0).sum() > 3_000  # the sample hits the instances
    assert np.array_equal(g, ob), f"{int((g != ob).any(1).sum())} rays differ"
    rgb, bo = nf_ctx.render(64, 36, 0, 2, seed=8)
    orgb, obo = o.render(64, 36, 0, 2, seed=8)
    assert np.array_equal(bo, obo) and rel_l2(rgb, orgb) <= RTOL


@pytest.mark.parametrize("scene", ["sphere_grid", "cornell"])
def test_render_equals_the_reference_walk_bit_for_bit(nf_ctx, golden_dir, scene):
    b = massrt.Builder(1).builtin(scene, ASPECT, golden_dir)
    ref = massrt.Context(0, options={"traversal": massrt.TRAVERSAL_REFERENCE})
    try:
        ref.upload(b)
        a = ref.render(160, 90, 0, 4, seed=19)
    finally:
        ref.close()
    nf_ctx.upload(b)
    assert nf_ctx.tuning()["traversal"] == massrt.TRAVERSAL_NEAR_FIRST
    n = nf_ctx.render(160, 90, 0, 4, seed=19)
    assert _same(a[0], n[0]) and _same(a[1], n[1])
