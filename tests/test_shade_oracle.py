"""The oracle's one-step shading entry (oracle.Scene.shade_rays) and the cases
of tests/shade_cases.py, on the CPU alone.

Anchors: the new entry against the oracle's own walk (trace_rays), its
pre-pass, and answers worked out by hand. Coverage floors: the shared cases
reach what they are about (every material kind, both sides of the critical
angle, every texture size under either wrap, ...), by the oracle's count, so
that test_gpu_shade_probe.py compares the device on hits that exist.
"""
import ctypes as C

import numpy as np
import pytest

import massrt
import oracle
import shade_cases as sc

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    """name -> (case, oracle scene, rays, slices, records): computed once, read by every test."""
    out = {}
    for name, case in sc.CASES.items():
        o = oracle.Scene(3)
        case(o)
        rays, where = sc.all_rays(case.info)
        out[name] = (case, o, rays, where, o.shade_rays(rays, seed=sc.SEED))
    return out


def test_record_is_the_devices():
    assert sc.f32 is f32
    assert massrt.SHADE_DTYPE.itemsize == C.sizeof(massrt.MrtShadeOut) == 88
    o = oracle.Scene(1)
    o.add_sphere(o.material(massrt.MAT_LAMBERTIAN, o.solid(0.5, 0.5, 0.5)), (0, 0, 0), 1.0)
    o.build_bvh()
    rec = o.shade_rays(np.array([[0, 0, 3, 0, 0, 1], [0, 0, 3, 0, 0, -1]], dtype=f32))
    assert rec.dtype == massrt.SHADE_DTYPE
    assert not rec[:1].view(np.uint8).any()  # a miss is all zeros
    assert rec["prim"][1] == massrt.REF_SPHERE << 28 and rec["t"][1] == 2.0 and rec["material"][1] == 0


@pytest.mark.parametrize("name", list(sc.CASES))
def test_both_builders_number_the_materials_alike(name):
    """The device reports indices into the builder's interned table, the oracle into its list: the cases
    are written so that the two are one numbering (shade_cases docstring)."""
    case = sc.CASES[name]
    b, o = massrt.Builder(3), oracle.Scene(3)
    case(o)
    io = case.info
    case(b)
    ib = case.info
    assert io.mat == ib.mat
    d = b.desc_only()
    assert d.n_materials == len(ib.kinds) == len(io.kinds)
    for i in range(d.n_materials):
        m = d.materials[i]
        assert m.kind == ib.kinds[i] == io.kinds[i], i
        want = min(ib.params[i], f32(1.0)) if m.kind == massrt.MAT_METAL else ib.params[i]
        assert f32(m.param) == want, i
    for nm in ("mix1", "mix0", "mix035", "glow"):
        m = d.materials[ib.mat[nm]]
        assert m.kind == massrt.MAT_MIX and m.left < ib.mat[nm] and m.right < ib.mat[nm]
    assert d.materials[ib.mat["mix1"]].left == ib.mat["mix1_left"]
    assert d.materials[ib.mat["mix0"]].right == ib.mat["mix0_right"]
    assert d.n_volumes == ib.volumes


@pytest.mark.parametrize("name", list(sc.CASES))
def test_probe_walks_as_trace_rays_does(cases, name):
    """prim, container, t and front face are the walk's. The two entries key their streams differently, so
    where the traversal draws (a Volume, a Mix alpha test) only rays that stay clear of it are compared."""
    case, o, rays, _where, rec = cases[name]
    tr = o.trace_rays(rays)
    keep = sc.draws_nothing(rays, case.info) if case.rng_on else np.ones(rays.shape[0], dtype=bool)
    if case.rng_on:
        assert keep.sum() >= 1000 and (~keep).sum() >= 200
    mine = np.stack([rec["prim"], rec["container"], bits(rec["t"]),
                     ((rec["flags"] & massrt.SHADE_FRONT_FACE) != 0).astype(np.uint32)], 1)
    assert (tr[keep, 0] != 0).sum() >= 1000
    assert np.array_equal(mine[keep], tr[keep]), int((mine[keep] != tr[keep]).any(1).sum())


@pytest.mark.parametrize("name", list(sc.CASES))
def test_probe_equals_the_prepass(cases, name):
    """On the pre-pass rays (closed aperture) the probe's normal and its Lambertian attenuation are the
    pre-pass buffers: Camera::albedo_normal and one step of Camera::trace share intersect and scatter."""
    case, o, _rays, _where, _rec = cases[name]
    W, H = sc.PRE_W, sc.PRE_H
    rays = sc.prepass_rays(o.camera_fields(), W, H)
    albedo, normal = o.prepass(W, H, seed=sc.SEED)
    rec = o.shade_rays(rays, seed=sc.SEED)
    keep = sc.draws_nothing(rays, case.info) if case.rng_on else np.ones(W * H, dtype=bool)
    hit = keep & (rec["prim"] != 0)
    assert hit.sum() > W * H // 4
    assert np.array_equal(bits(rec["normal"])[keep], bits(normal.reshape(-1, 3))[keep])
    lam = hit & (case.info.kinds[np.where(hit, rec["material"], 0)] == massrt.MAT_LAMBERTIAN)
    assert lam.sum() > 200
    assert np.array_equal(bits(rec["attenuation"][lam]), bits(albedo.reshape(-1, 3)[lam]))


def test_hand_derived_spheres():
    """Radius 1/2 at integer centres, rays along the axes: every step is exact in f32."""
    o = oracle.Scene(1)
    colour = (0.9, 0.8, 0.7)
    metal = o.material(massrt.MAT_METAL, o.solid(*colour), 0.0)
    glass = o.material(massrt.MAT_DIELECTRIC, 0, 1.5)
    light = o.material(massrt.MAT_DIFFUSE_LIGHT, 0, 0.0, (4.0, 3.0, 2.5))
    lamb = o.material(massrt.MAT_LAMBERTIAN, o.solid(0.25, 0.5, 0.125))
    for k, m in enumerate((metal, glass, light, lamb)):
        o.add_sphere(m, (4.0 * k, 0.0, 0.0), 0.5)
    o.build_bvh()
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=f32)

    def towards(k, scale=1.0):  # from two radii out, straight at sphere k's centre
        c = np.array([4.0 * k, 0, 0], dtype=f32)
        return np.concatenate([c + axes * f32(2.0), -axes * f32(scale)], 1)

    S, F = massrt.SHADE_SCATTERED, massrt.SHADE_FRONT_FACE
    # fuzz-0 metal, normal incidence: straight back, the surface colour
    rec = o.shade_rays(towards(0))
    assert np.all(rec["t"] == 1.5) and np.all(rec["flags"] == S | F) and np.all(rec["material"] == metal)
    assert np.array_equal(rec["normal"], axes) and np.array_equal(rec["direction"], axes)
    assert np.array_equal(rec["point"], np.array([0, 0, 0], dtype=f32) + axes * f32(0.5))
    assert np.array_equal(bits(rec["attenuation"]), bits(np.tile(np.array(colour, dtype=f32), (6, 1))))
    assert not rec["emitted"].any() and not rec["uv"].any()
    # a DiffuseLight emits its colour and does not scatter
    rec = o.shade_rays(towards(2, 3.0))
    assert np.all(rec["t"] == 0.5) and np.all(rec["flags"] == F)
    assert np.array_equal(rec["emitted"], np.tile(np.array([4.0, 3.0, 2.5], dtype=f32), (6, 1)))
    assert not rec["attenuation"].any() and not rec["direction"].any()
    # a SOLID surface returns its colour
    rec = o.shade_rays(towards(3))
    assert np.all(rec["flags"] == S | F)
    assert np.array_equal(rec["attenuation"], np.tile(np.array([0.25, 0.5, 0.125], dtype=f32), (6, 1)))
    # glass from inside at 60 degrees (sin = 0.87 > 1 / 1.5): total internal reflection
    n = axes
    t = axes[[2, 3, 4, 5, 0, 1]]
    d = (f32(0.5) * n + f32(np.sqrt(0.75)) * t).astype(f32)
    p = np.array([4.0, 0, 0], dtype=f32) + f32(0.5) * n
    rays = np.concatenate([p - d * f32(0.25), d], 1)
    rec = o.shade_rays(rays)
    assert np.all(rec["flags"] == S) and np.all(rec["material"] == glass)  # back face
    assert np.array_equal(rec["attenuation"], np.ones((6, 3), dtype=f32))
    assert np.array_equal(bits(rec["direction"]), bits(sc.reflect(sc.unit32(d), rec["normal"])))
    assert np.allclose(rec["normal"], -n, atol=1e-6)


def test_hand_derived_textures_and_mixes(cases):
    """A 1x1 texture is its texel / 255 at any uv under either wrap; Mix ratio 1 always takes the left
    side, ratio 0 always the right, for emit and for scatter."""
    case, _o, _rays, _where, rec = cases["plain"]
    info = case.info
    hit = rec["prim"] != 0
    for wrap in sc.WRAPS:
        _p0, m = info.quads[(1, 1, wrap)]
        on = hit & (rec["material"] == m)
        assert on.sum() >= 200
        uv = rec["uv"][on]
        assert (uv < 0).any() and (uv > 1).any() and np.all((uv >= 0) & (uv <= 1), axis=1).any()
        texel = info.texels[(1, 1, wrap)][0, 0, :3].astype(f32) / f32(255.0)
        assert np.array_equal(bits(rec["attenuation"][on]), bits(np.tile(texel, (int(on.sum()), 1))))
    scattered = (rec["flags"] & massrt.SHADE_SCATTERED) != 0
    for name, colour in (("mix1", (0.1, 0.5, 0.9)), ("mix0", (0.3, 0.7, 0.6))):  # both sides are Lambertian there
        on = hit & (rec["material"] == info.mat[name])
        assert on.sum() >= 200
        assert scattered[on].all() and not rec["emitted"][on].any()
        assert np.array_equal(bits(rec["attenuation"][on]), bits(np.tile(np.array(colour, dtype=f32), (int(on.sum()), 1))))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_coverage_floors(cases, name):
    case, _o, rays, _where, rec = cases[name]
    got, want = sc.coverage(case.info, rays, rec), sc.floors(case)
    short = {k: (got[k], v) for k, v in want.items() if got[k] < v}
    assert not short, short


def test_lattice_reaches_both_sides_of_every_texel_boundary(cases):
    """Along the lattice rays the bilinear tap's integer column (row) takes every value and the fraction
    is zero on some hits, just above zero and just below one on others."""
    case, _o, _rays, where, rec = cases["plain"]
    rec = rec[where["lattice"]]
    for (w, h, wrap), (_p0, m) in case.info.quads.items():
        on = (rec["prim"] != 0) & (rec["material"] == m)
        for axis, n in ((0, w), (1, h)):
            if n == 1:
                continue
            uv = rec["uv"][on][:, axis].astype(np.float64)
            x = (uv - np.floor(uv) if wrap == massrt.WRAP_REPEAT else np.clip(uv, 0, 1)) * (n - 1)
            frac = x - np.floor(x)
            inner = (uv > 0) & (uv < 1) if wrap == massrt.WRAP_CLAMP else np.ones(uv.size, dtype=bool)
            assert set(np.floor(x[inner]).astype(int)) >= set(range(n - 1)), (w, h, wrap, axis)
            assert (frac[inner] < 1e-4).sum() >= 2 * (n - 1) and (frac[inner] > 1 - 1e-4).sum() >= 2 * (n - 1)


def test_cubemap_cameras_see_every_face():
    """The CubeMap with solid faces whose red is face + 1, through the oracle's own face selection: the
    three cameras of the background test put at least 30 pixels on each of the six faces."""
    seen = np.zeros(7, dtype=np.int64)
    for camera in sc.BG_CAMERAS:
        o = oracle.Scene(3)
        sc.background_case("cubemap", camera, index_faces=True)(o)
        rgb, _b = o.render(sc.BG_W, sc.BG_H, 0, 1, seed=sc.SEED, max_depth=1)
        red = rgb.reshape(-1, 3)[:, 0]
        assert np.all(red == np.round(red)) and red.max() <= 6
        seen += np.bincount(red.astype(np.int64), minlength=7)
    assert seen[0] >= 1  # the MAT_NONE sphere: a hit that neither emits nor scatters
    assert np.all(seen[1:] >= 30), seen
