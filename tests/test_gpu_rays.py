"""mrt_render_rays: whole paths for rays the caller chose.

A camera sample is a ray plus a position in its stream, so the renderer's own
frames are the yardstick: entries built on the host from the oracle's path
stream (tests/rays_ref.py, numpy float32) must give the bits of mrt_render and
the oracle's answer — on scenes of every kernel variant, on both walks, through
the refill (more work items than pool slots) and through chunks of the results
slab. Then what the contract says about keys, positions, the device form and
the arguments."""
import ctypes as C

import numpy as np
import pytest

import massrt
import oracle
import rays_ref

pytestmark = pytest.mark.gpu
ASPECT = float(massrt.ASPECT_RATIO)
RTOL = 1e-4  # relative L2 on accumulated radiance (README "Parity")
MRT_OK, MRT_ERR_INVALID, MRT_ERR_STATE = 0, 1, 4
W, H, SPP, SEED = 48, 27, 4, 5
APERTURE = 0.1
COUNTED = ["samples", "segments", "node_visits", "sphere_tests", "triangle_tests", "closest_hits", "bounces"]


def composite(x):
    """A small world whose materials sit on composite surfaces (TextureBlend,
    SolidColorFallback): the EXT kernel variants. x: massrt.Builder or oracle.Scene."""
    warm = x.blend(massrt.BLEND_ADDITION, x.solid(0.5, 0.2, 0.1, 1.0), x.solid(0.2, 0.3, 0.1, 1.0))
    dark = x.blend(massrt.BLEND_DARKEN, x.solid(0.9, 0.4, 0.7, 1.0), x.solid(0.5, 0.8, 0.6, 1.0))
    back = x.fallback((0.2, 0.3, 0.4, 1.0), x.blend(massrt.BLEND_LIGHTEN, x.solid(0.1, 0.6, 0.2, 0.0), warm))
    x.background(massrt.BG_SKY)
    x.add_sphere(x.material(massrt.MAT_LAMBERTIAN, warm), (0.0, -100.5, 0.0), 100.0)
    x.add_sphere(x.material(massrt.MAT_METAL, dark, 0.2), (1.2, 0.0, 0.0), 0.5)
    x.add_sphere(x.material(massrt.MAT_LAMBERTIAN, back), (-1.1, 0.1, 0.3), 0.6)
    x.add_sphere(x.material(massrt.MAT_DIELECTRIC, 0, 1.5), (0.0, 0.0, 1.0), 0.4)
    x.add_sphere(x.material(massrt.MAT_DIFFUSE_LIGHT, 0, 0.0, (4.0, 4.0, 3.0)), (0.0, 2.5, -1.0), 0.7)
    x.build_bvh()
    vfov, look_from, look_at = VIEW["composite"]
    x.camera(vfov, look_from, look_at, aspect=ASPECT, aperture=APERTURE)
    return x


def fog(x):
    """Two constant-density spheres (Volume over a Sphere) between diffuse and
    metal ones: the traversal draws from the path's stream, which the oracle
    follows too (it has no fog boxes, so no cornell_smoke)."""
    x.background(massrt.BG_SKY)
    x.add_sphere(x.material(massrt.MAT_LAMBERTIAN, x.solid(0.6, 0.6, 0.5, 1.0)), (0.0, -100.5, 0.0), 100.0)
    x.add_sphere(x.material(massrt.MAT_METAL, x.solid(0.8, 0.7, 0.6, 1.0), 0.1), (1.3, 0.0, -0.4), 0.5)
    x.add_sphere(x.material(massrt.MAT_LAMBERTIAN, x.solid(0.2, 0.3, 0.8, 1.0)), (-1.2, 0.0, 0.2), 0.5)
    x.add_volume((0.0, 0.3, 0.6), 0.8, 0.9, (0.9, 0.9, 0.9))
    x.add_volume((0.4, 0.2, -1.6), 0.7, 2.5, (0.1, 0.1, 0.1))
    x.build_bvh()
    vfov, look_from, look_at = VIEW["fog"]
    x.camera(vfov, look_from, look_at, aspect=ASPECT, aperture=APERTURE)
    return x


# scene -> (vfov, look_from, look_at): the built-in's own view, here with a lens
VIEW = {"cornell": (37.0, (0.0, 5.0, 20.0), (0.0, 5.0, 0.0)),
        "cornell_smoke": (37.0, (0.0, 5.0, 20.0), (0.0, 5.0, 0.0)),  # traversal draws, no drain hand-off
        "sphere_grid": (40.0, (6.0, 8.0, 5.0), (0.0, 0.0, 0.0)),
        "cube_field": (40.0, (6.0, 8.0, 5.0), (0.0, 0.0, 0.0)),
        "composite": (40.0, (3.0, 2.0, 5.0), (0.0, 0.2, 0.0)),
        "fog": (40.0, (3.0, 2.0, 5.0), (0.0, 0.2, 0.0))}
SCENES = sorted(VIEW)
CUSTOM = {"composite": composite, "fog": fog}
ORACLE_SCENES = [s for s in SCENES if s != "cornell_smoke"]  # the oracle builds no fog boxes; `fog` stands in


def scene_camera(scene):
    vfov, look_from, look_at = VIEW[scene]
    return massrt.make_camera(vfov, look_from, look_at, aspect=ASPECT, aperture=APERTURE)


def build(scene, x, golden_dir):
    return CUSTOM[scene](x) if scene in CUSTOM else x.builtin(scene, ASPECT, golden_dir)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


@pytest.fixture(scope="module", params=["reference", "auto"])
def rctx(request):
    """A context per walk setting the issue names: the reference's walk, and AUTO (the default: per scene)."""
    walk = massrt.TRAVERSAL_REFERENCE if request.param == "reference" else massrt.TRAVERSAL_AUTO
    c = massrt.Context(0, options={"traversal": walk})
    yield c
    c.close()


@pytest.fixture(scope="module")
def entries():
    """The restatement's entries of every pixel of the 48 x 27 frame, per scene
    camera and sample, built once: {scene: [entries of sample 0..3]}."""
    cache, out = {}, {}
    for scene in SCENES:
        if VIEW[scene] not in cache:
            cam = scene_camera(scene)
            cache[VIEW[scene]] = [rays_ref.frame_entries(cam, W, H, SEED, s) for s in range(SPP)]
        out[scene] = cache[VIEW[scene]]
    assert any((e["skip"] > 4).any() for e in out["cornell"])  # rays whose stream starts after a rejected disk try
    return out


@pytest.fixture(scope="module")
def oracle_frames(golden_dir):
    """oracle.render_pixels of every pixel, samples 0..3, per scene, once."""
    out = {}
    for scene in ORACLE_SCENES:
        o = build(scene, oracle.Scene(1), golden_dir)
        vfov, look_from, look_at = VIEW[scene]
        o.camera(vfov, look_from, look_at, aspect=ASPECT, aperture=APERTURE)
        assert np.array_equal(bits(o.camera_fields()), bits(scene_camera(scene).fields())), scene
        out[scene] = o.render_pixels(W, H, np.arange(W * H, dtype=np.uint32), 0, SPP, seed=SEED)
    return out


def upload(c, scene, golden_dir):
    c.upload(build(scene, massrt.Builder(1), golden_dir))
    c.set_camera(scene_camera(scene))


def four_calls(c, per_sample, flags=0):
    """Sample s's entries with spp_begin = s, spp_count = 1, into one pair of buffers."""
    rgb, bo = np.zeros(W * H * 3, np.float32), np.zeros(W * H, np.uint32)
    for s, e in enumerate(per_sample):
        c.render_rays(e, seed=SEED, spp_begin=s, spp_count=1, flags=flags, rgb=rgb, bounces=bo)
    return rgb, bo


@pytest.mark.parametrize("scene", SCENES)
def test_camera_entries_give_the_frames_bits(rctx, scene, entries, golden_dir):
    """rgb and bounces bit for bit, and the counters of a counting run: samples,
    segments, primitive tests, closest hits and bounces on either walk, node
    visits on the reference's walk. On the near-first walk a frame does not
    repeat its own node visits: two identical counting renders of this 48 x 27 x
    4 frame gave 50365 and 50429 (composite), 1459716 and 1458471 (sphere_grid),
    732453 and 724630 (cornell), 2538578 and 2509658 (cube_field), with every
    other counter equal, where the reference's walk gave 33800, 2115891, 610673
    and 2787177 each time, for the frame and for its rays. That count depends
    on which rays share a wave there, so it has no frame's value to be held to."""
    upload(rctx, scene, golden_dir)
    frame = rctx.render(W, H, 0, SPP, seed=SEED)
    got = four_calls(rctx, entries[scene])
    assert same_bits(got, frame)
    assert frame[1].sum() > 0 and np.unique(frame[1]).size > 2
    # a counting run of each does the same work: per path nothing differs
    rctx.reset_counters()
    rctx.render(W, H, 0, SPP, seed=SEED, counters=True)
    want = rctx.counters()
    rctx.reset_counters()
    assert same_bits(four_calls(rctx, entries[scene], flags=massrt.RENDER_COUNTERS), frame)
    have = rctx.counters()
    assert have["samples"] == W * H * SPP
    reference_walk = rctx.tuning()["traversal"] == massrt.TRAVERSAL_REFERENCE
    for k in COUNTED:
        if k == "node_visits" and not reference_walk:
            continue
        assert have[k] == want[k], (k, have[k], want[k])
    assert have["instance_entries"] == want["instance_entries"] and have["shaded"] == want["shaded"]
    if massrt.lib().mrt_debug_build():  # MASSRT_LIB=dbg: no table, pool or slab index out of range
        assert rctx.debug_status()[3] == 0, rctx.debug_status()


@pytest.mark.parametrize("scene", ORACLE_SCENES)
def test_oracle_parity(rctx, scene, entries, oracle_frames, golden_dir):
    upload(rctx, scene, golden_dir)
    rgb, bo = four_calls(rctx, entries[scene])
    orgb, obo = oracle_frames[scene]
    assert np.array_equal(bo, obo), "bounce counts differ from the oracle"
    assert rel_l2(rgb, orgb) <= RTOL


@pytest.fixture(scope="module")
def grid(golden_dir):
    return massrt.Builder(1).builtin("sphere_grid", ASPECT, golden_dir)


@pytest.fixture(scope="module")
def cornell(golden_dir):
    return massrt.Builder(1).builtin("cornell", ASPECT, golden_dir)


def test_refill(rctx, grid):
    """92,160 entries against the smallest pool (65,536 paths): the rest can only come from k_refill<RayTable>."""
    w, h, depth = 480, 192, 8
    walk = rctx.get_option("traversal")
    c = massrt.Context(0, options={"traversal": walk, "pool_paths": 65536})
    try:
        c.upload(grid)
        cam = scene_camera("sphere_grid")
        c.set_camera(cam)
        assert c.tuning()["pool_paths"] == 65536 < w * h
        e = massrt.camera_rays(cam, w, h, np.arange(w * h, dtype=np.uint32), seed=SEED, sample=0)
        frame = c.render(w, h, 0, 1, seed=SEED, max_depth=depth)
        c.reset_kernel_stats()
        got = c.render_rays(e, seed=SEED, spp_begin=0, spp_count=1, max_depth=depth, flags=massrt.RENDER_TIME_KERNELS)
        ks = c.kernel_stats()
        assert ks["iterations"] > 1 and ks["shade_launches"] > 1, ks
        assert same_bits(got, frame)
        assert frame[1].max() <= depth and frame[1].sum() > 0
        if massrt.lib().mrt_debug_build():  # MASSRT_LIB=dbg: no table, pool or slab index out of range
            assert c.debug_status()[3] == 0, c.debug_status()
    finally:
        c.close()


def test_chunks(rctx, cornell):
    """One call of 5 samples over a slab of 4096 results (1296 entries: chunks of 3 + 2) = five calls of one."""
    walk = rctx.get_option("traversal")
    c = massrt.Context(0, options={"traversal": walk, "results_log2": 12})
    try:
        c.upload(cornell)
        cam = scene_camera("cornell")
        e = massrt.camera_rays(cam, W, H, np.arange(W * H, dtype=np.uint32), seed=SEED, sample=0)
        assert c.tuning()["results_max"] == 4096 and 2 * e.size < 4096 < 5 * e.size
        whole = c.render_rays(e, seed=SEED, spp_begin=2, spp_count=5)
        rgb, bo = np.zeros_like(whole[0]), np.zeros_like(whole[1])
        for s in range(2, 7):
            c.render_rays(e, seed=SEED, spp_begin=s, spp_count=1, rgb=rgb, bounces=bo)
        assert same_bits((rgb, bo), whole)
        rctx.upload(cornell)  # and the context with the default slab: one chunk
        assert same_bits(rctx.render_rays(e, seed=SEED, spp_begin=2, spp_count=5), whole)
    finally:
        c.close()


def wall_rays(n=96):
    """Rays from the Cornell camera's place into the box's back half: they hit the Lambertian walls."""
    rng = np.random.default_rng(3)
    e = np.zeros(n, dtype=massrt.PATH_RAY_DTYPE)
    e["origin"] = (0.0, 5.0, 20.0)
    e["direction"][:, 0] = rng.uniform(-4.0, 4.0, n)
    e["direction"][:, 1] = rng.uniform(-4.0, 4.0, n)
    e["direction"][:, 2] = -25.0
    e["key"] = np.arange(n) * 7 + 3
    e["skip"] = rng.integers(0, 9, n)
    return e


def test_keys_not_positions(rctx, cornell):
    rctx.upload(cornell)
    e = rays_ref.frame_entries(scene_camera("cornell"), W, H, SEED, 1)
    base = rctx.render_rays(e, seed=SEED, spp_begin=1, spp_count=2)
    perm = np.random.default_rng(1).permutation(e.size)
    got = rctx.render_rays(e[perm], seed=SEED, spp_begin=1, spp_count=2)
    assert np.array_equal(bits(got[0]).reshape(-1, 3), bits(base[0]).reshape(-1, 3)[perm])
    assert np.array_equal(got[1], base[1][perm])
    twice = rctx.render_rays(np.repeat(e, 2), seed=SEED, spp_begin=1, spp_count=2)
    pair = bits(twice[0]).reshape(-1, 2, 3)
    assert np.array_equal(pair[:, 0], pair[:, 1]) and np.array_equal(pair[:, 0], bits(base[0]).reshape(-1, 3))
    assert np.array_equal(twice[1].reshape(-1, 2)[:, 0], base[1]) and np.array_equal(twice[1][0::2], twice[1][1::2])
    # the stream is (seed, key, sample) after skip draws: each of the three matters to a diffuse bounce
    w = wall_rays()
    hits = rctx.trace_rays(np.concatenate([w["origin"], w["direction"]], 1))
    assert np.all(hits[:, 0] != 0)  # every ray meets a wall
    ref = rctx.render_rays(w, seed=SEED, spp_count=4)
    other_key, more_skip = w.copy(), w.copy()
    other_key["key"] += 1
    more_skip["skip"] += 1
    for name, res in (("key", rctx.render_rays(other_key, seed=SEED, spp_count=4)),
                      ("skip", rctx.render_rays(more_skip, seed=SEED, spp_count=4)),
                      ("seed", rctx.render_rays(w, seed=SEED + 1, spp_count=4))):
        changed = (bits(res[0]).reshape(-1, 3) != bits(ref[0]).reshape(-1, 3)).any(1) | (res[1] != ref[1])
        assert changed.mean() > 0.5, (name, changed.mean())
    assert same_bits(rctx.render_rays(w, seed=SEED, spp_count=4), ref)


def test_device_form(rctx, cornell):
    import torch

    walk = rctx.get_option("traversal")
    e = rays_ref.frame_entries(scene_camera("cornell"), W, H, SEED, 0)
    n = e.size
    pre_rgb = np.linspace(0.25, 3.0, n * 3, dtype=np.float32)
    pre_bo = ((np.arange(n) * 3) % 11 + 1).astype(np.uint32)
    c = massrt.Context(0, options={"traversal": walk})
    try:
        d, _ = cornell.desc()
        c.upload_desc(d)  # a scene, no camera
        want = c.render_rays(e, seed=SEED, spp_begin=0, spp_count=3, rgb=pre_rgb.copy(), bounces=pre_bo.copy())
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        assert side.cuda_stream != 0
        with torch.cuda.stream(side):
            d_rays = torch.from_numpy(e.view(np.uint8).copy()).to(dev)
            d_rgb = torch.from_numpy(pre_rgb.copy()).to(dev)
            d_bo = torch.from_numpy(pre_bo.astype(np.int32)).to(dev)
            assert d_rays.data_ptr() % 16 == 0 and d_rays.numel() == 32 * n
            c.render_rays_device(d_rays.data_ptr(), n, SEED, 0, 3, massrt.MAX_DEPTH, 0, d_rgb.data_ptr(),
                                 d_bo.data_ptr(), side.cuda_stream)
            # a skip the device form cannot refuse is clamped: it draws MRT_RAY_SKIP_MAX
            far = e.copy()
            far["skip"] = 2 ** 32 - 1
            d_far = torch.from_numpy(far.view(np.uint8).copy()).to(dev)
            d_rgb2 = torch.zeros(n * 3, dtype=torch.float32, device=dev)
            d_bo2 = torch.zeros(n, dtype=torch.int32, device=dev)
            c.render_rays_device(d_far.data_ptr(), n, SEED, 0, 1, massrt.MAX_DEPTH, 0, d_rgb2.data_ptr(),
                                 d_bo2.data_ptr(), side.cuda_stream)
        side.synchronize()
        got = (d_rgb.cpu().numpy(), d_bo.cpu().numpy().astype(np.uint32))
        assert same_bits(got, want)
        assert not np.array_equal(bits(got[0]), bits(pre_rgb))
        limit = e.copy()
        limit["skip"] = massrt.RAY_SKIP_MAX
        assert same_bits((d_rgb2.cpu().numpy(), d_bo2.cpu().numpy().astype(np.uint32)),
                         c.render_rays(limit, seed=SEED, spp_begin=0, spp_count=1))
        with pytest.raises(massrt.MassrtError, match="no camera"):
            c.render(W, H, 0, 1)
        with pytest.raises(massrt.MassrtError, match="16-byte aligned"):
            c.render_rays_device(d_rays.data_ptr() + 8, n - 1, SEED, 0, 1, massrt.MAX_DEPTH, 0, d_rgb.data_ptr(),
                                 d_bo.data_ptr(), side.cuda_stream)
    finally:
        c.close()
    # the context's camera is not changed either
    rctx.upload(cornell)
    rctx.set_camera(scene_camera("sphere_grid"))
    before = rctx.render(W, H, 0, 2, seed=9)
    assert same_bits(rctx.render_rays(e, seed=SEED, spp_begin=0, spp_count=3, rgb=pre_rgb.copy(), bounces=pre_bo.copy()),
                     want)
    assert same_bits(rctx.render(W, H, 0, 2, seed=9), before)


def test_arguments_and_state(rctx, cornell):
    L = massrt.lib()
    rctx.upload(cornell)
    e = wall_rays(64)
    good = rctx.render_rays(e, seed=SEED, spp_count=2)
    arr = e.ctypes.data_as(C.POINTER(massrt.MrtPathRay))
    rgb = np.full(e.size * 3, 0.5, np.float32)
    bo = np.full(e.size, 7, np.uint32)
    prgb, pbo = rgb.ctypes.data_as(C.POINTER(C.c_float)), bo.ctypes.data_as(C.POINTER(C.c_uint32))

    def call(rays=arr, n=e.size, spp_begin=0, spp_count=2, max_depth=massrt.MAX_DEPTH, flags=0, h=None):
        return L.mrt_render_rays(h or rctx.h, rays, n, SEED, spp_begin, spp_count, max_depth, flags, prgb, pbo)

    def refused(rc, code, text, h=None):
        assert rc == code and text in L.mrt_last_error(h or rctx.h).decode(), (rc, L.mrt_last_error(h or rctx.h))
        assert np.all(rgb == 0.5) and np.all(bo == 7)  # nothing was enqueued

    refused(call(rays=None), MRT_ERR_INVALID, "no rays")
    refused(call(n=0), MRT_ERR_INVALID, "no rays")
    refused(call(flags=massrt.RENDER_FUSED), MRT_ERR_INVALID, "render one camera")
    refused(call(flags=massrt.RENDER_SIMPLE_TRACE), MRT_ERR_INVALID, "render one camera")
    refused(call(spp_begin=2 ** 32 - 1, spp_count=1), MRT_ERR_INVALID, "sample index overflow")
    refused(call(spp_begin=2, spp_count=2 ** 32 - 2), MRT_ERR_INVALID, "sample index overflow")
    refused(L.mrt_render_rays(rctx.h, arr, e.size, SEED, 0, 2, 50, 0, None, pbo), MRT_ERR_INVALID, "null accumulation")
    refused(L.mrt_render_rays(rctx.h, arr, e.size, SEED, 0, 2, 50, 0, prgb, None), MRT_ERR_INVALID, "null accumulation")
    deep = e.copy()
    deep["skip"][40] = massrt.RAY_SKIP_MAX + 1
    refused(call(rays=deep.ctypes.data_as(C.POINTER(massrt.MrtPathRay))), MRT_ERR_INVALID, "entry 40 has skip 4097")
    # the device form refuses the same, on real device buffers that stay as they were
    import torch

    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(e[:4].view(np.uint8).copy()).to(dev)
    d_rgb, d_bo = torch.full((12,), 0.5, device=dev), torch.full((4,), 7, dtype=torch.int32, device=dev)
    pr, pc, pb = C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_rgb.data_ptr()), C.c_void_p(d_bo.data_ptr())

    def refused_dev(rc, code, text, h=None):
        refused(rc, code, text, h)
        torch.cuda.synchronize()
        assert bool((d_rgb == 0.5).all()) and bool((d_bo == 7).all())

    fresh = massrt.Context(0)
    try:
        refused(call(h=fresh.h), MRT_ERR_STATE, "no scene", h=fresh.h)
        refused_dev(L.mrt_render_rays_device(fresh.h, pr, 4, SEED, 0, 1, 50, 0, pc, pb, None), MRT_ERR_STATE, "no scene",
                    h=fresh.h)
    finally:
        fresh.close()
    refused_dev(L.mrt_render_rays_device(rctx.h, None, 4, SEED, 0, 1, 50, 0, pc, pb, None), MRT_ERR_INVALID, "no rays")
    refused_dev(L.mrt_render_rays_device(rctx.h, pr, 0, SEED, 0, 1, 50, 0, pc, pb, None), MRT_ERR_INVALID, "no rays")
    refused_dev(L.mrt_render_rays_device(rctx.h, pr, 4, SEED, 0, 1, 50, massrt.RENDER_FUSED, pc, pb, None),
                MRT_ERR_INVALID, "render one camera")
    refused_dev(L.mrt_render_rays_device(rctx.h, pr, 4, SEED, 2 ** 32 - 1, 1, 50, 0, pc, pb, None), MRT_ERR_INVALID,
                "sample index overflow")
    refused_dev(L.mrt_render_rays_device(rctx.h, pr, 4, SEED, 0, 1, 50, 0, None, pb, None), MRT_ERR_INVALID,
                "null accumulation")
    assert L.mrt_render_rays_device(rctx.h, pr, 4, SEED, 0, 0, 50, 0, pc, pb, None) == MRT_OK  # no samples: a no-op
    assert L.mrt_render_rays_device(rctx.h, pr, 4, SEED, 0, 1, 0, 0, pc, pb, None) == MRT_OK  # no depth: a no-op
    torch.cuda.synchronize()
    assert bool((d_rgb == 0.5).all()) and bool((d_bo == 7).all())
    # nothing to add: MRT_OK, the buffers as they were
    assert call(spp_count=0) == MRT_OK and call(max_depth=0) == MRT_OK
    assert np.all(rgb == 0.5) and np.all(bo == 7)
    # a skip at the limit itself is allowed; and after all the refusals a valid call gives the right bits
    deep["skip"][40] = massrt.RAY_SKIP_MAX
    rctx.render_rays(deep, seed=SEED, spp_count=1)
    assert same_bits(rctx.render_rays(e, seed=SEED, spp_count=2), good)


def test_any_ray_bits_are_accepted(rctx, cornell):
    """Ray values are not validated (as for mrt_trace_rays): NaN and zero
    directions return MRT_OK and leave the other entries' bits as they are."""
    rctx.upload(cornell)
    e = wall_rays(64)
    good = rctx.render_rays(e, seed=SEED, spp_count=2)
    odd = e.copy()
    bad = [5, 6, 33]
    odd["direction"][5] = (np.nan, np.nan, np.nan)
    odd["direction"][6] = (0.0, 0.0, 0.0)
    odd["direction"][33] = (0.0, np.nan, -1.0)
    got = rctx.render_rays(odd, seed=SEED, spp_count=2)  # raises unless MRT_OK
    keep = np.setdiff1d(np.arange(e.size), bad)
    assert np.array_equal(bits(got[0]).reshape(-1, 3)[keep], bits(good[0]).reshape(-1, 3)[keep])
    assert np.array_equal(got[1][keep], good[1][keep])
