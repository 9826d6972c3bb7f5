"""Volumes whose boundary is an instance or a model (fog boxes) on the device:
mrt_trace_rays and mrt_shade_rays against the composition over the CPU oracle
(tests/volume_ref.py), a furnace render through the whole k_trace -> k_shade
-> refill loop, and the cornell_smoke scene under every scheduling option."""
import ctypes as C

import numpy as np
import pytest

import massrt
import volume_ref as vr
from conftest import GOLDEN
from test_volume_targets import BEHIND, INSIDE, three_root_expectation

F = np.float32
INF = float("inf")
ALBEDO = (0.25, 0.5, 0.75)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


class MrtVolume(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("density", C.c_float), ("material", C.c_uint32)]


def fog(kind, albedo=ALBEDO, density=vr.DENSITY, spheres=False):
    b = massrt.Builder(1)
    cube = b.model_from_ply(GOLDEN / vr.CUBE, b.material(massrt.MAT_NONE))
    lam = b.material(massrt.MAT_LAMBERTIAN, b.solid(0.5, 0.5, 0.5))
    if spheres:
        b.add_sphere(lam, BEHIND[:3], BEHIND[3])
    if kind == "instance":
        b.add_volume_instance(cube, vr.INST_T, vr.INST_R, vr.INST_S, density, albedo)
    else:
        b.add_volume_model(cube, density, albedo)
    if spheres:
        b.add_sphere(lam, INSIDE[:3], INSIDE[3])
    b.camera(40.0, (0.3, 0.2, 5.0), vr.INST_T, aspect=float(massrt.ASPECT_RATIO))
    return b


@pytest.fixture(scope="module")
def cases():
    out = {}
    for kind, centre in (("instance", vr.INST_T), ("model", (0.0, 0.0, 0.0))):
        rays = vr.rays_about(centre)
        out[kind] = (rays, vr.Searches(GOLDEN, kind, rays))
    return out


@pytest.fixture(scope="module", params=[0, 24], ids=["global", "treelet24"])
def vctx(request):
    c = massrt.Context(0, options={"treelet_kb": request.param})
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("interval", vr.INTERVALS, ids=["open", "both-clips", "tmax-clip"])
@pytest.mark.parametrize("kind", ["instance", "model"])
def test_trace_rays_match_the_composition(vctx, cases, kind, interval):
    rays, s = cases[kind]
    vr.assert_not_empty(vr.volume_hits(rays, s, *vr.INTERVALS[0])[2], s)
    hit, t, cat = vr.volume_hits(rays, s, *interval)
    if interval != vr.INTERVALS[0]:
        vr.assert_clip_exercised(cat, s, *interval)
    vctx.upload(fog(kind))
    got = vctx.trace_rays(rays, *interval)
    assert np.array_equal(got, vr.expected_hits(hit, t))


@pytest.mark.gpu
def test_trace_rays_three_root_world(vctx, cases):
    rays, s = cases["instance"]
    want = three_root_expectation(rays, s, 0.001, INF)[0]
    vctx.upload(fog("instance", spheres=True))
    assert np.array_equal(vctx.trace_rays(rays), want)


@pytest.mark.gpu
def test_counters_count_both_searches(cases):
    """COUNT variants: every box and triangle test of both searches, one instance entry per search. The render's
    primary rays are not the composition's, so the check is the identity the reference obeys: an unbuilt world
    of one fog box enters its instance once per segment and once more per segment that found an entry."""
    c = massrt.Context(0)
    try:
        c.upload(fog("instance"))
        c.reset_counters()
        c.render(64, 36, 0, 2, seed=3, counters=True)
        k = c.counters()
        assert k["segments"] < k["instance_entries"] <= 2 * k["segments"]
        assert k["model_entries"] == 0 and k["triangle_tests"] > 0 and k["node_visits"] >= k["instance_entries"]
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["instance", "model"])
def test_shade_rays_on_volume_hits(vctx, cases, kind):
    rays, _ = cases[kind]
    b = fog(kind)
    d = b.desc_only()
    vol_material = C.cast(d.volumes, C.POINTER(MrtVolume))[0].material
    vctx.upload(b)
    out = vctx.shade_rays(rays, seed=7)
    v = out["prim"] == vr.VOLUME0
    assert v.sum() >= rays.shape[0] // 4 and np.all((out["prim"] == 0) | v)
    o = out[v]
    want = massrt.SHADE_FRONT_FACE | massrt.SHADE_SCATTERED
    assert np.all(o["flags"] & (massrt.SHADE_FRONT_FACE | massrt.SHADE_HAS_UV | massrt.SHADE_SCATTERED) == want)
    assert np.all(o["container"] == 0) and np.all(o["material"] == vol_material)
    assert np.array_equal(bits(o["normal"]), bits(np.broadcast_to(np.array([1, 0, 0], dtype=F), o["normal"].shape)))
    assert np.array_equal(bits(o["attenuation"]), bits(np.broadcast_to(np.array(ALBEDO, dtype=F), o["normal"].shape)))
    r = rays[v]
    point = (r[:, 0:3] + (r[:, 3:6] * o["t"][:, None]).astype(F)).astype(F)  # Ray::at: origin + direction * t
    assert np.array_equal(bits(o["point"]), bits(point))


@pytest.mark.gpu
def test_furnace():
    """A white world and an albedo-1 fog box: every path that ends on the background carries exactly 1, however
    often it scattered — unless the nested searches leak or lose state of the walk around them."""
    W, H, spp = 64, 36, 8
    # a unit cube (mean chord 2/3: optical depth 4/3 at density 2, so a path scatters a few times and the
    # bounce sum of 8 samples stays far below 50) filling most of a narrow view
    b = massrt.Builder(1)
    cube = b.model_from_ply(GOLDEN / vr.CUBE, b.material(massrt.MAT_NONE))
    b.add_volume_instance(cube, (0, 0, 0), vr.INST_R, (0.5, 0.5, 0.5), 2.0, (1, 1, 1))
    b.camera(30.0, (0.0, 0.0, 2.0), (0, 0, 0), aspect=float(massrt.ASPECT_RATIO))
    b.background(massrt.BG_SOLID, color=(1.0, 1.0, 1.0))
    c = massrt.Context(0)
    try:
        c.upload(b)
        rgb, bo = c.render(W, H, 0, spp, seed=11, max_depth=50)
    finally:
        c.close()
    rgb = rgb.reshape(-1, 3)
    in_depth = bo < 50  # no sample of the pixel can have used all 50 bounces
    print(f"furnace: {np.count_nonzero(in_depth)} of {W * H} pixels within depth, {np.count_nonzero(bo)} scattered, "
          f"largest bounce sum {bo.max()}, {np.count_nonzero(rgb[in_depth] != F(8.0))} values off 8.0")
    assert np.count_nonzero(in_depth) >= 0.99 * W * H
    assert np.count_nonzero(bo) >= 0.30 * W * H
    assert np.all(rgb[in_depth] == F(8.0))


@pytest.mark.gpu
def test_cornell_smoke_scheduling_invariants():
    W, H, spp = 64, 36, 4
    b = massrt.Builder(1).builtin("cornell_smoke", float(massrt.ASPECT_RATIO), GOLDEN)
    assert b.volume_targets()[1] == 2
    c = massrt.Context(0)
    try:
        c.upload(b)
        base = c.render(W, H, 0, spp, seed=5)
        assert np.isfinite(base[0]).all() and base[0].any()

        def same(got, what):
            assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(got[1], base[1]), what

        same(c.render(W, H, 0, spp, seed=5), "twice")
        for sb in (0, 1, 2):
            c.set_option("shade_bin", sb)
            same(c.render(W, H, 0, spp, seed=5), ("shade_bin", sb))
        c.set_option("shade_bin", -1)
        for q in (1, 2):
            c.set_option("queues", q)
            same(c.render(W, H, 0, spp, seed=5), ("queues", q))
        same(c.render(W, H, 0, spp, seed=5, flags=massrt.RENDER_SIMPLE_TRACE), "simple trace")
        acc = c.render(W, H, 0, spp, seed=5, shard_index=0, shard_count=2)
        same(c.render(W, H, 0, spp, seed=5, shard_index=1, shard_count=2, accum=acc), "two shards")
        # the pre-pass: a pixel whose primary hit is a fog box has the volume's fixed normal. Albedo 0 is the
        # black fog or, with a zero normal, a miss past the open front; albedo 1 with that normal is the white
        # fog alone (the white walls face -y, +y and +z, the wall that faces +x is red)
        albedo, normal = c.prepass(W, H, seed=5)
    finally:
        c.close()
    albedo, normal = albedo.reshape(-1, 3), normal.reshape(-1, 3)
    x = np.array([1, 0, 0], dtype=F)
    black = np.all(albedo == 0, axis=1) & np.any(normal != 0, axis=1)
    white = np.all(albedo == 1, axis=1)
    assert black.sum() >= 20 and np.all(normal[black] == x)
    assert np.count_nonzero(white & np.all(normal == x, axis=1)) >= 20
    walls = np.array([[1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, 1]], dtype=F)
    assert np.all(np.any(np.all(normal[white][:, None, :] == walls[None], axis=2), axis=1))


@pytest.mark.gpu
def test_device_build_bvh_agrees_with_the_host():
    """Both builders sort and join the volume's box like any other item, with the same draws."""
    def world(b):
        cube = b.model_from_ply(GOLDEN / vr.CUBE, b.material(massrt.MAT_NONE))
        lam = b.material(massrt.MAT_LAMBERTIAN, b.solid(0.5, 0.5, 0.5))
        for k in range(7):
            b.add_sphere(lam, (1.5 * k - 4.0, 0.3 * k, -0.7 * k), 0.4)
            if k % 3 == 0:
                b.add_volume_instance(cube, (0.9 * k - 2, 0.2, 0.5 * k), (0.1 * k, 0.7, 0.2), (1.0, 0.6, 0.8), 0.5, ALBEDO)
        b.add_volume_model(cube, 0.5, ALBEDO)
        return b

    c = massrt.Context(0)
    try:
        h, g = world(massrt.Builder(1)), world(massrt.Builder(1))
        h.build_bvh()
        g.build_bvh_device(c)
        dh, dg = h.desc_only(), g.desc_only()
        assert dh.n_nodes == dg.n_nodes and [dh.roots[k] for k in range(dh.n_roots)] == [dg.roots[k] for k in range(dg.n_roots)]
        nh = np.frombuffer(C.string_at(dh.nodes, dh.n_nodes * C.sizeof(massrt.MrtNode)), dtype=np.uint32)
        ng = np.frombuffer(C.string_at(dg.nodes, dg.n_nodes * C.sizeof(massrt.MrtNode)), dtype=np.uint32)
        assert np.array_equal(nh, ng)
        assert h.rand_f32() == g.rand_f32()  # the scene stream stands where the host build leaves it
    finally:
        c.close()


@pytest.mark.gpu
def test_upload_rejects_malformed_target_tables():
    b = fog("instance")
    b.add_volume((0, 0, 0), 1.0, 0.5, (1, 1, 1))
    d = b.desc_only()
    inst, model, sphere = massrt.REF_INSTANCE << 28, massrt.REF_MODEL << 28, massrt.REF_SPHERE << 28
    good = [(0, inst | 0)]
    c = massrt.Context(0)
    try:
        c.upload_desc(d, targets=good)
        for table, message in (([(5, inst | 0)], "volume index out of range"),
                               (good + [(1, model | 7)], "target index out of range"),
                               (good + [(1, sphere | 0)], "must be an instance or a model"),
                               (good + [(0, inst | 0)], "listed twice")):
            with pytest.raises(massrt.MassrtError, match=message):
                c.upload_desc(d, targets=table)
        c.upload_desc(d, targets=good)  # and the context still takes the well-formed scene
    finally:
        c.close()
