"""Closest-hit parity on adversarial rays, on the device (tests/adversarial_rays.py
has the families; tests/test_layout.py runs the same rays through the host
build of the walks).

k_trace's two walks promise the reference's closest hit on EVERY ray:
primitive, container, t bits, front face. The rays here are the ones ordinary
generators never send: zero and subnormal direction components, origins on
box planes, box corners, triangle edges, sphere centres and tangents, |d| from
2^-120 to 2^100, origins up to 1e38 away (the reference's own sphere
arithmetic overflows there and accepts hits whose t is NaN), NaN and
infinities. The near-first walk is exact by a proof with a domain (no
overflow); nf_ray_ok sends a ray outside it to the reference
walk, and these tests are what holds it to that."""
import numpy as np
import pytest

import adversarial_rays as adv
import massrt
import oracle

pytestmark = pytest.mark.gpu
ASPECT = float(massrt.ASPECT_RATIO)
SMALL = ["cornell", "sphere_grid", "cube_field"]
CUSTOM = ["ties", "wild", "alpha_both"]
WALKS = {"reference": massrt.TRAVERSAL_REFERENCE, "near_first": massrt.TRAVERSAL_NEAR_FIRST}


@pytest.fixture(scope="module")
def contexts():
    c = {name: massrt.Context(0, options={"traversal": walk}) for name, walk in WALKS.items()}
    yield c
    for x in c.values():
        x.close()


def _build(world, golden_dir):
    if world in SMALL:
        return massrt.Builder(1).builtin(world, ASPECT, golden_dir), oracle.Scene(1).builtin(world, ASPECT, golden_dir)
    if world == "ties":  # coincident and touching primitives (tests/test_gpu_nearfirst.py test_random_worlds_with_ties)
        from test_bvh import random_world
        b, o = random_world(11, 400, ties=True)
        for x in (b, o):
            x.camera(50.0, (8, 6, 9), (0, 0, 0), aspect=ASPECT)
        return b, o
    if world == "wild":
        return adv.build_both(lambda x: adv.wild_world(x, golden_dir, ASPECT))
    return adv.build_both(lambda x: adv.alpha_world(x, "both", ASPECT))


@pytest.fixture(scope="module")
def worlds(golden_dir):
    """world -> (builder, the families' rays as one array, (family, begin, end) offsets, the oracle's hits): built,
    generated from the world's own desc() and traced by the oracle once, then shared and left unchanged."""
    cache = {}

    def get(world):
        if world not in cache:
            b, o = _build(world, golden_dir)
            rays, parts = adv.split(adv.families(*b.desc()))
            want = o.trace_rays(rays)
            want.setflags(write=False)
            rays.setflags(write=False)
            cache[world] = b, rays, parts, want
        return cache[world]
    return get


def _assert_equal(ctx, what, rays, parts, want):
    got = ctx.trace_rays(rays)
    assert got.shape == want.shape
    bad = [m for m in (adv.first_difference(name, rays[a:e], got[a:e], want[a:e]) for name, a, e in parts) if m]
    assert not bad, f"{what}:\n" + "\n".join(bad)


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("scene", SMALL)
def test_builtin_scenes(contexts, worlds, scene, walk):
    """Every family on the small built-in scenes: all four words of every ray equal the oracle's, on both walks."""
    b, rays, parts, want = worlds(scene)
    assert {name for name, _, _ in parts} == {f.__name__ for f in adv.FAMILIES}
    adv.check_floors({name: want[a:e] for name, a, e in parts}, overflow=scene != "cube_field")
    ctx = contexts[walk]
    ctx.upload(b)
    assert ctx.tuning()["traversal"] == WALKS[walk]
    _assert_equal(ctx, f"{walk} walk on {scene}", rays, parts, want)


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("world", CUSTOM)
def test_custom_worlds(contexts, worlds, world, walk):
    """Ties between coincident primitives; wild instances (thin 12 x 0.004 x 9 slabs: their own box test and
    margin, nf_bound.h nf_rho_wild, with its own rule for NaN and huge values); alpha-tested triangles entered
    through a Model and an Instance. The families come from each world's own boxes and primitives, so the far
    and the NaN origins meet the instance transform and the wild-box test. (`ties` is where a world triangle's
    NaN t first showed the device passing a ray's NaN on with another sign than the oracle's host: 12 of 4000
    rays, isect.h tri_t_nan.)"""
    b, rays, parts, want = worlds(world)
    adv.check_floors({name: want[a:e] for name, a, e in parts}, overflow=False)
    ctx = contexts[walk]
    ctx.upload(b)
    if world != "ties":  # as tests/test_gpu_nearfirst.py asserts for these worlds
        assert ctx.tuning()["traversal"] == WALKS[walk]
    _assert_equal(ctx, f"{walk} walk on {world}", rays, parts, want)


def test_treelet(contexts, worlds):
    """The LDS treelet's build of the walk (a budget of test_treelet_budgets_bit_exact's list) on sphere_grid's
    families: the plain context's hits."""
    b, rays, parts, want = worlds("sphere_grid")
    contexts["reference"].upload(b)
    plain = contexts["reference"].trace_rays(rays)
    c = massrt.Context(0, options={"trace_block": 256, "treelet_kb": 4})
    try:
        c.upload(b)
        _assert_equal(c, "treelet_kb 4 on sphere_grid", rays, parts, plain)
    finally:
        c.close()


def test_render_rays_with_odd_origins(contexts, golden_dir):
    """mrt_render_rays with a NaN component in three entries' origins and three origins 1e12 away (d = target
    - o): under the near-first walk the other entries' radiance and bounce bits are as without them, and the six
    odd entries bounce as often as under the reference walk."""
    from test_gpu_rays import SEED, bits, wall_rays
    cornell = massrt.Builder(1).builtin("cornell", ASPECT, golden_dir)
    e = wall_rays(64)
    odd = e.copy()
    nan_at, far_at = [5, 6, 33], [11, 40, 62]
    for k, i in enumerate(nan_at):
        odd["origin"][i, k] = np.nan
    rng = np.random.default_rng(9)
    for i in far_at:
        o = (1e12 * adv._unit(rng, 1)[0]).astype(np.float32)
        target = (np.float32([0.0, 5.0, 0.0]) + rng.uniform(-3.0, 3.0, 3)).astype(np.float32)
        odd["origin"][i] = o
        odd["direction"][i] = target - o
    bad = nan_at + far_at
    keep = np.setdiff1d(np.arange(e.size), bad)
    nf, ref = contexts["near_first"], contexts["reference"]
    nf.upload(cornell)
    assert nf.tuning()["traversal"] == massrt.TRAVERSAL_NEAR_FIRST
    good = nf.render_rays(e, seed=SEED, spp_count=2)
    got = nf.render_rays(odd, seed=SEED, spp_count=2)  # raises unless MRT_OK
    assert np.array_equal(bits(got[0]).reshape(-1, 3)[keep], bits(good[0]).reshape(-1, 3)[keep])
    assert np.array_equal(got[1][keep], good[1][keep])
    ref.upload(cornell)
    want = ref.render_rays(odd, seed=SEED, spp_count=2)
    assert np.array_equal(got[1][bad], want[1][bad]), (got[1][bad], want[1][bad])
    assert np.array_equal(got[1][keep], want[1][keep])
