"""EveMaterial and mapped normals on the device.

The oracle has no EveMaterial, so the yardstick is tests/eve_ref.py (numpy
float32 from the reference's text) through the shading probe
(Context.shade_rays): bit for bit on every hit. The probe itself is anchored
to the oracle-checked walk (Context.trace_rays) and to the pre-pass; one
statistical test ties the rendered image to an oracle scene that is equal in
distribution; the scheduling invariants hold bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import eve_ref
import massrt
from conftest import GOLDEN

f32 = np.float32
SOE = [[0.02, 0.02, 0.02], [0.2, 0.2, 0.2], [1.0, 1.0, 1.0], [0.5, 0.0, 0.0]]  # eve.rs:178-188
ORE = [[0.02, 0.02, 0.02], [0.1, 0.1, 0.1], [0.15, 0.26, 0.39], [0.85, 0.62, 0.2]]
GLOW = [0.5, 0.85, 2.0]
OVERRIDE = (0.3, 0.6, 0.9)

TRI = np.dtype([("a", "<f4", 3), ("b", "<f4", 3), ("c", "<f4", 3), ("na", "<f4", 3), ("nb", "<f4", 3),
                ("nc", "<f4", 3), ("uva", "<f4", 2), ("uvb", "<f4", 2), ("uvc", "<f4", 2), ("tangent", "<f4", 3),
                ("bitangent", "<f4", 3), ("material", "<u4"), ("flags", "<u4")])
INST = np.dtype([("fwd", "<f4", 16), ("inv", "<f4", 16), ("blas_root", "<u4"), ("material", "<u4")])
MAT = np.dtype([("kind", "<u4"), ("surface", "<u4"), ("param", "<f4"), ("emit", "<f4", 3), ("left", "<u4"),
                ("right", "<u4")])
SPH = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("material", "<u4")])


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def table(ptr, n, dtype, ctype):
    assert dtype.itemsize == C.sizeof(ctype)
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer((ctype * n).from_address(C.addressof(ptr.contents)), dtype=dtype).copy()


class Desc:
    """The builder's description as numpy tables (what the restatement is fed with)."""

    def __init__(self, b):
        d, ext = b.desc_only(), b.desc_ext()
        self.tri = table(d.triangles, d.n_triangles, TRI, massrt.MrtTriangle)
        self.inst = table(d.instances, d.n_instances, INST, massrt.MrtInstance)
        self.mat = table(d.materials, d.n_materials, MAT, massrt.MrtMaterial)
        self.sph = table(d.spheres, d.n_spheres, SPH, massrt.MrtSphere)
        self.tex = [np.ctypeslib.as_array(d.textures[i].rgba, shape=(d.textures[i].height, d.textures[i].width, 4)).copy()
                    for i in range(d.n_textures)]
        self.eve = [(e.normal_occlusion, e.albedo_roughness, e.pmdg, np.array(list(e.colors), dtype=f32).reshape(4, 3),
                     np.array(list(e.glow), dtype=f32)) for e in (ext.eve_materials[i] for i in range(ext.n_eve_materials))]


# ---- the test scene ---------------------------------------------------------

def barrel(nu=10, nv=10, center=(0.0, 0.0, 0.0), radius=1.0):
    """A lat-long sphere without its caps: nu * nv * 2 = 200 triangles {v, n, uv} x 3,
    smooth normals, uvs from (-1, -0.5) to (2, 1.5) (outside [0, 1] on every side)."""
    th = np.linspace(0.15 * np.pi, 0.85 * np.pi, nv + 1)
    ph = np.linspace(0.0, 2.0 * np.pi, nu + 1)

    def vert(i, j):
        n = np.array([np.sin(th[j]) * np.cos(ph[i]), np.cos(th[j]), np.sin(th[j]) * np.sin(ph[i])])
        return np.concatenate([np.asarray(center) + radius * n, n, [3.0 * i / nu - 1.0, 2.0 * j / nv - 0.5]])

    tris = []
    for i in range(nu):
        for j in range(nv):
            q = [vert(i, j), vert(i + 1, j), vert(i + 1, j + 1), vert(i, j + 1)]
            tris += [np.concatenate([q[0], q[1], q[2]]), np.concatenate([q[0], q[2], q[3]])]
    return np.array(tris, dtype=f32)


def quad(p0, du, dv, normal, uv_scale):
    p0, du, dv = (np.asarray(v, dtype=np.float64) for v in (p0, du, dv))
    c = [np.concatenate([p0 + a * du + b * dv, normal, [a * uv_scale, b * uv_scale]]) for a, b in
         ((0, 0), (1, 0), (1, 1), (0, 1))]
    return np.array([np.concatenate([c[0], c[1], c[2]]), np.concatenate([c[0], c[2], c[3]])], dtype=f32)


def textures(seed, shape):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=shape + (4,), dtype=np.uint8) for _ in range(3)]


def texel(*rgba):
    return np.array([[list(rgba)]], dtype=np.uint8)


def build_scene(b, eve=True, volume=False, aperture=0.0):
    """The same geometry for massrt.Builder and oracle.Scene (eve=False: Lambertian in place of every EveMaterial)."""
    def eve_mat(tex, colors, fallback):
        if not eve:
            return b.material(massrt.MAT_LAMBERTIAN, b.solid(*fallback))
        return b.eve_material(*[b.texture_rgba(t) for t in tex], colors, GLOW)

    big = eve_mat(textures(7, (7, 5)), SOE, (0.5, 0.5, 0.5))  # 5 wide, 7 high
    # 1x1 textures: roughness 1 -> ratio exactly 1; roughness 0 and dirt 0 -> ratio exactly 0
    rough = eve_mat([texel(128, 200, 128, 40), texel(200, 100, 50, 255), texel(60, 170, 30, 0)], ORE, (0.6, 0.4, 0.2))
    shiny = eve_mat([texel(128, 90, 128, 160), texel(220, 180, 140, 0), texel(200, 85, 0, 128)], ORE, (0.2, 0.4, 0.6))
    over = b.material(massrt.MAT_LAMBERTIAN, b.solid(*OVERRIDE))
    plain = b.material(massrt.MAT_LAMBERTIAN, b.solid(0.7, 0.7, 0.7))
    b.model(rough, quad((-5, -2, -5), (10, 0, 0), (0, 0, 10), (0, 1, 0), 2.5), add_to_world=True, shading=True)
    b.model(shiny, quad((-5, -2, -5), (10, 0, 0), (0, 7, 0), (0, 0, 1), 1.0), add_to_world=True, shading=True)
    m = b.model(big, barrel(), add_to_world=True, shading=True)
    b.add_instance(m, (3, 0, 0), (0.3, 0.5, 0.7), (1.0, 0.6, 1.4))
    b.add_instance(m, (-3, 0, 0), (0.1, -0.2, 0.0), (1.2, 1.2, 0.8), material=over)
    corners = barrel(center=(0, 0, 3)).reshape(-1, 3, 8)[:, :, :3].reshape(-1, 9)
    b.model(plain, corners, override=big, add_to_world=True)  # Triangle::new under an Eve override
    b.add_sphere(big, (0, 2.5, 0), 0.8)
    if volume:
        b.add_volume((0, 0, 0), 9.0, 0.05, (0.4, 0.4, 0.4))
    b.background(massrt.BG_SKY)
    b.camera(50.0, (0.5, 1.5, 9.0), (0, 0, 0), aspect=float(massrt.ASPECT_RATIO), aperture=aperture)
    b.build_bvh()
    return b


def probe_rays(n=4000, seed=3):
    """From outside towards the objects and from inside the meshes (back faces)."""
    rng = np.random.default_rng(seed)
    h = n // 2
    o = rng.uniform((-5, -1.8, -4.5), (5, 4, 6), size=(h, 3))
    d = rng.uniform((-4, -2, -4), (4, 3, 4), size=(h, 3)) - o
    centres = np.array([(0, 0, 0), (3, 0, 0), (-3, 0, 0), (0, 0, 3), (0, 2.5, 0)])
    oi = centres[rng.integers(0, len(centres), size=n - h)] + rng.uniform(-0.3, 0.3, size=(n - h, 3))
    di = rng.normal(size=(n - h, 3))
    return np.concatenate([np.concatenate([o, d], 1), np.concatenate([oi, di], 1)]).astype(f32)


@pytest.fixture(scope="module")
def scene():
    b = build_scene(massrt.Builder(1))
    return b, Desc(b), probe_rays()


def test_the_rays_reach_what_the_test_is_about(scene):
    """CPU pre-check with the oracle's walk over the same geometry under Lambertian."""
    import oracle

    b, desc, rays = scene
    hits = build_scene(oracle.Scene(1), eve=False).trace_rays(rays)
    prim, cont = hits[:, 0], hits[:, 1]
    tri = (prim >> 28) == massrt.REF_TRIANGLE
    own_eve = np.zeros(len(rays), dtype=bool)
    own_eve[tri] = desc.mat["kind"][desc.tri["material"][prim[tri] & 0x0FFFFFFF]] == massrt.MAT_EVE
    own_eve &= (desc.tri["flags"][np.where(tri, prim & 0x0FFFFFFF, 0)] & 1) != 0
    print(f"hits {int((prim != 0).sum())}, on Eve uv triangles {int(own_eve.sum())}, of them back faces "
          f"{int((own_eve & (hits[:, 3] == 0)).sum())}, instanced {int((own_eve & ((cont >> 28) == massrt.REF_INSTANCE)).sum())}")
    assert own_eve.sum() >= 1000
    assert (own_eve & (hits[:, 3] == 0)).sum() >= 100
    assert (own_eve & ((cont >> 28) == massrt.REF_INSTANCE)).sum() >= 100


def restate(desc, rays, out):
    """eve_ref over the probe's hits: per ray the expected uv, normal, front
    face, emission, and for Eve hits the SolidColor and the Mix ratio."""
    n = len(rays)
    o, d = rays[:, :3], rays[:, 3:]
    prim, cont = out["prim"], out["container"]
    pk, pi = prim >> 28, prim & 0x0FFFFFFF
    inst = (cont >> 28) == massrt.REF_INSTANCE
    ii = np.where(inst, cont & 0x0FFFFFFF, 0)
    ro, rd = o.copy(), d.copy()
    if inst.any():
        ro[inst] = eve_ref.transform(desc.inst["inv"][ii[inst]], o[inst], 1.0)
        rd[inst] = eve_ref.transform(desc.inst["inv"][ii[inst]], d[inst], 0.0)
    exp = {k: np.zeros((n, 3), dtype=f32) for k in ("normal", "emitted", "color")}
    exp["uv"] = np.zeros((n, 2), dtype=f32)
    exp["front"] = np.zeros(n, dtype=bool)
    exp["ratio"] = np.full(n, np.nan, dtype=f32)
    exp["has_uv"] = np.zeros(n, dtype=bool)
    exp["mapped"] = np.zeros(n, dtype=bool)
    outward = np.zeros((n, 3), dtype=f32)
    # spheres (geom.rs:77-91)
    s = pk == massrt.REF_SPHERE
    if s.any():
        sp = desc.sph[pi[s]]
        point = ro[s] + rd[s] * out["t"][s][:, None]
        outward[s] = (point - sp["center"]) / sp["radius"][:, None]
    # triangles
    t = pk == massrt.REF_TRIANGLE
    tr = desc.tri[pi[t]]
    nrm, uv = eve_ref.triangle_hit(tr, ro[t], rd[t], out["t"][t])
    has_uv = (tr["flags"] & 1) != 0
    exp["has_uv"][t] = has_uv
    exp["uv"][t] = np.where(has_uv[:, None], uv, 0)
    own = desc.mat[tr["material"]]
    mapped = has_uv & (own["kind"] == massrt.MAT_EVE)
    flat = outward.copy()
    flat[t] = nrm
    for rec in np.unique(own["surface"][mapped]):
        sel = mapped & (own["surface"] == rec)
        tan = eve_ref.normal_occlusion(desc.tex[desc.eve[rec][0]], uv[sel])
        nrm[sel] = eve_ref.mapped_normal(tr["tangent"][sel], tr["bitangent"][sel], nrm[sel], tan)
    outward[t] = nrm
    exp["mapped"][t] = mapped
    hit = prim != 0

    def world_normal(outw):
        front = np.zeros(n, dtype=bool)
        nn = np.zeros((n, 3), dtype=f32)
        front[hit], nn[hit] = eve_ref.face_normal(rd[hit], outw[hit])
        if inst.any():
            nn[inst] = eve_ref.instance_normal(desc.inst["fwd"][ii[inst]], nn[inst])
        return front, nn

    exp["front"], exp["normal"] = world_normal(outward)
    vol = pk == massrt.REF_VOLUME  # geom.rs:644-651: a fixed normal, the front face, no uv
    exp["front"][vol] = True
    exp["normal"][vol] = (1.0, 0.0, 0.0)
    exp["unmapped"] = world_normal(flat)[1]  # what a device without Material::normal would give
    # Hit::material's emission and scatter inputs
    m = desc.mat[np.where(hit, out["material"], 0)]
    e = hit & (m["kind"] == massrt.MAT_EVE) & exp["has_uv"]
    for rec in np.unique(m["surface"][e]):
        sel = e & (m["surface"] == rec)
        _, ar, pm, colors, glow = desc.eve[rec]
        exp["emitted"][sel] = eve_ref.emit(desc.tex[pm], glow, exp["uv"][sel])
        exp["color"][sel], exp["ratio"][sel] = eve_ref.color_ratio(desc.tex[ar], desc.tex[pm], colors, exp["uv"][sel])
    exp["eve"] = e
    exp["hit_kind"] = np.where(hit, m["kind"], 0xFFFFFFFF)
    return exp


@pytest.mark.gpu
def test_probe_equals_the_restatement_bit_for_bit(ctx, scene):
    b, desc, rays = scene
    ctx.upload(b)
    out = ctx.shade_rays(rays, seed=9)
    # the probe's walk is the oracle-checked one
    tr = ctx.trace_rays(rays)
    assert np.array_equal(out["prim"], tr[:, 0]) and np.array_equal(out["container"], tr[:, 1])
    assert np.array_equal(bits(out["t"]), tr[:, 2])
    assert np.array_equal(out["flags"] & 1, tr[:, 3])
    hit = out["prim"] != 0
    miss = out[~hit]
    assert not np.frombuffer(miss.tobytes(), dtype=np.uint8).any(), "a miss is all zeros"
    exp = restate(desc, rays, out)
    assert np.array_equal((out["flags"] & massrt.SHADE_HAS_UV) != 0, exp["has_uv"])
    assert np.array_equal(bits(out["uv"]), bits(exp["uv"]))
    assert np.array_equal((out["flags"] & 1) != 0, exp["front"])
    bad = (bits(out["normal"]) != bits(exp["normal"])).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} normals differ, first at ray {int(np.argmax(bad))}"
    assert np.array_equal(bits(out["emitted"]), bits(exp["emitted"]))
    scat = (out["flags"] & massrt.SHADE_SCATTERED) != 0
    ud = eve_ref.unit(rays[:, 3:])
    mirror = eve_ref.reflect(ud, out["normal"])
    lam_len = np.abs(eve_ref.length(out["direction"] - out["normal"]) - 1.0)

    # EveMaterial hits: Mix(ratio, Lambertian(color), Specular(1.8, color))
    e = exp["eve"]
    assert e.sum() >= 1000 and scat[e].all()
    assert np.any(exp["emitted"][e] != 0)
    is_one = (bits(out["attenuation"]) == bits(f32(1.0))).all(axis=1)
    is_color = (bits(out["attenuation"]) == bits(exp["color"])).all(axis=1)
    assert np.all(is_one[e] | is_color[e])
    assert not np.any(is_one[e] & is_color[e])
    spec = e & is_one
    lamb = e & is_color
    assert spec.sum() > 50 and lamb.sum() > 50, (int(spec.sum()), int(lamb.sum()))
    assert np.array_equal(bits(out["direction"][spec]), bits(mirror[spec]))
    same = (bits(out["direction"]) == bits(out["normal"])).all(axis=1)  # near_zero fallback (material.rs:207-209)
    assert np.all((lam_len[lamb] <= 1e-5) | same[lamb]), float(lam_len[lamb].max())
    # exact ratios: 1 always takes the Lambertian side; 0 leaves it to the Specular draw
    r1, r0 = e & (exp["ratio"] == 1.0), e & (exp["ratio"] == 0.0)
    assert r1.sum() > 100 and r0.sum() > 100, (int(r1.sum()), int(r0.sum()))
    assert lamb[r1].all()
    assert spec[r0].any() and lamb[r0].any()
    mid = e & (exp["ratio"] > 0.0) & (exp["ratio"] < 1.0)
    assert spec[mid].any() and lamb[mid].any()

    # a Lambertian override on Eve triangles: the mapped normal stays, the shading is the override's
    over = hit & exp["mapped"] & (exp["hit_kind"] == massrt.MAT_LAMBERTIAN)
    assert over.sum() > 50
    assert scat[over].all() and not out["emitted"][over].any()
    assert np.array_equal(bits(out["attenuation"][over]), np.broadcast_to(bits(np.array(OVERRIDE, dtype=f32)),
                                                                          (int(over.sum()), 3)))
    # the map is not flat: without it nearly every one of these normals would differ
    assert (bits(exp["normal"][exp["mapped"]]) != bits(exp["unmapped"][exp["mapped"]])).any(axis=1).mean() > 0.9

    # an Eve override on plain triangles, an Eve sphere: no uv, so no map, no scatter, no emission
    nouv = hit & (exp["hit_kind"] == massrt.MAT_EVE) & ~exp["has_uv"]
    tri_nouv = nouv & ((out["prim"] >> 28) == massrt.REF_TRIANGLE)
    sph_nouv = nouv & ((out["prim"] >> 28) == massrt.REF_SPHERE)
    assert tri_nouv.sum() > 50 and sph_nouv.sum() > 50, (int(tri_nouv.sum()), int(sph_nouv.sum()))
    assert not scat[nouv].any() and not exp["mapped"][nouv].any()
    for f in ("emitted", "attenuation", "direction", "uv"):
        assert not bits(out[f][nouv]).any(), f


def camera_rays(cam, W, H):
    """Camera::albedo_normal's rays with a closed aperture (world.rs:53-63,81-92)."""
    c = cam.fields()
    origin, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    x, y = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    u = (x.ravel() / f32(W - 1))[:, None]
    v = (y.ravel() / f32(H - 1))[:, None]
    d = (((llc + hor * u) + ver * v) - origin) - f32(0.0)
    return np.concatenate([np.broadcast_to(origin, d.shape), d], 1).astype(f32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "sphere_grid", "eve_test"])
def test_probe_equals_the_prepass(ctx, scene, name):
    W, H = 64, 36
    b = scene[0] if name == "eve_test" else massrt.Builder(1).builtin(name, float(massrt.ASPECT_RATIO), GOLDEN)
    d, cam = b.desc()
    cam.lens_radius = 0.0  # the pre-pass draws its lens sample from another stream than the probe
    ctx.upload_desc(d, b.desc_ext())
    ctx.set_camera(cam)
    albedo, normal = ctx.prepass(W, H, seed=4)
    out = ctx.shade_rays(camera_rays(cam, W, H), seed=4)
    hit = out["prim"] != 0
    assert hit.sum() > W * H // 4
    assert np.array_equal(bits(out["normal"]), bits(normal.reshape(-1, 3)))
    mats = table(d.materials, d.n_materials, MAT, massrt.MrtMaterial)
    lam = hit & (mats["kind"][np.where(hit, out["material"], 0)] == massrt.MAT_LAMBERTIAN)
    assert lam.any()
    assert np.array_equal(bits(out["attenuation"][lam]), bits(albedo.reshape(-1, 3)[lam]))


@pytest.mark.gpu
def test_eve_without_the_extension_is_rejected(ctx, scene):
    b = scene[0]
    with pytest.raises(massrt.MassrtError, match="eve material index out of range"):
        ctx.upload_desc(b.desc_only())
    empty = massrt.MrtSceneExt()
    with pytest.raises(massrt.MassrtError, match="eve material index out of range"):
        ctx.upload_desc(b.desc_only(), empty)
    ctx.upload(b)  # and the context still takes the scene with its table


@pytest.mark.gpu
def test_scheduling_invariants():
    """The image does not depend on the survivor grouping, the queue count, the
    shard split or the walk (the last on the scene without a Volume: a scene
    whose traversal draws keeps the reference's walk)."""
    W, H, spp = 64, 36, 8
    for volume in (False, True):
        b = build_scene(massrt.Builder(1), volume=volume)
        c = massrt.Context(0, options={"traversal": massrt.TRAVERSAL_REFERENCE})
        try:
            c.upload(b)
            base = c.render(W, H, 0, spp, seed=5)
            assert np.isfinite(base[0]).all() and base[0].any()
            for sb in (0, 1, 2):
                c.set_option("shade_bin", sb)
                got = c.render(W, H, 0, spp, seed=5)
                assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(got[1], base[1]), sb
            c.set_option("shade_bin", -1)
            for q in (1, 2):
                c.set_option("queues", q)
                got = c.render(W, H, 0, spp, seed=5)
                assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(got[1], base[1]), q
            acc = c.render(W, H, 0, spp, seed=5, shard_index=0, shard_count=2)
            acc = c.render(W, H, 0, spp, seed=5, shard_index=1, shard_count=2, accum=acc)
            assert np.array_equal(bits(acc[0]), bits(base[0])) and np.array_equal(acc[1], base[1])
            if not volume:
                c.set_option("traversal", massrt.TRAVERSAL_NEAR_FIRST)
                c.upload(b)
                assert c.tuning()["traversal"] == massrt.TRAVERSAL_NEAR_FIRST
                got = c.render(W, H, 0, spp, seed=5)
                assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(got[1], base[1])
        finally:
            c.close()


# ---- distribution against the oracle ------------------------------------------

def flat_uv(tris, uv=(0.3, 0.7)):
    """Every corner on one uv: uv_ab = uv_ac = 0, so tangent = bitangent = 0 (geom.rs:481-482)."""
    t = tris.reshape(-1, 3, 8).copy()
    t[:, :, 6:8] = uv
    return t.reshape(-1, 24)


def stat_scene(b, mats):
    """Instances only. With zero tangent frames the mapped normal is
    normal * tan.z, tan.z > 0: the same face and, after Instance::intersect's
    unit(), the same normal as without the map (up to rounding)."""
    floor = b.model(mats[0], flat_uv(quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0), 1.0)), shading=True)
    ball = b.model(mats[1], flat_uv(barrel()), shading=True)
    b.add_instance(floor, (0, -1, 0), (0, 0, 0), (6, 1, 6))
    b.add_instance(ball, (-1.3, 0, 0), (0.2, 0.1, 0.0), (1, 1, 1))
    b.add_instance(ball, (1.3, 0.1, 0.3), (0.0, 0.7, 0.3), (0.9, 1.1, 0.8), material=mats[0])
    b.background(massrt.BG_SKY)
    b.camera(45.0, (0.3, 1.8, 6.0), (0, -0.2, 0), aspect=float(massrt.ASPECT_RATIO))
    b.build_bvh()
    return b


# 1x1 textures: glow texel 0, dirt 0, so ratio = roughness = w / 255 and the colour does not depend on it
STAT_NO = texel(128, 150, 255, 110)
STAT_AR = [(200, 120, 90), (90, 160, 210)]
STAT_PMDG = [texel(100, 85, 0, 0), texel(30, 200, 0, 0)]
STAT_W = (51, 178)  # ratios 0.2 and 0.698


def gpu_stat_scene(flip):
    b = massrt.Builder(1)
    mats = [b.eve_material(b.texture_rgba(STAT_NO), b.texture_rgba(texel(*STAT_AR[k], 255 - STAT_W[k] if flip else STAT_W[k])),
                           b.texture_rgba(STAT_PMDG[k]), ORE, GLOW) for k in range(2)]
    return stat_scene(b, mats)


@pytest.mark.gpu
def test_image_distribution_equals_the_oracles_mix(ctx):
    """EveMaterial over constant texels against the oracle's
    Mix(ratio, Lambertian(color), Specular(1.8, color)) with eve_ref's color and
    ratio: Mix::emit draws once where EveMaterial::emit draws nothing, so the
    streams differ by a draw per bounce and the images agree in distribution
    only. And the statistic sees a swapped Mix: ratio -> 1 - ratio fails."""
    import oracle
    from test_statistical import batch_stats, block_z, check

    W, H = 64, 36
    o = oracle.Scene(1)
    mats = []
    for k in range(2):
        color, ratio = eve_ref.color_ratio(texel(*STAT_AR[k], STAT_W[k]), STAT_PMDG[k], ORE, np.zeros((1, 2), dtype=f32))
        assert 0.0 < ratio[0] < 1.0
        c = o.solid(*[float(v) for v in color[0]], 1.0)
        mats.append(o.mix(float(ratio[0]), o.material(massrt.MAT_LAMBERTIAN, c), o.material(massrt.MAT_SPECULAR, c, 1.8)))
    stat_scene(o, mats)
    n_ref = 1024
    m, v, bm, bv = batch_stats(lambda s0, n: o.render(W, H, s0, n, seed=31, threads=0), 32, 32)
    fix = {"width": W, "height": H, "n": n_ref, "mean": m, "var": v * n_ref, "bmean": bm, "bvar": bv * n_ref}

    def gpu(flip):
        ctx.upload(gpu_stat_scene(flip))
        return block_z(fix, batch_stats(lambda s0, n: ctx.render(W, H, s0, n, seed=32), 64, 64))

    z = gpu(False)
    print(f"max |z| {np.abs(z).max():.2f}, mean z^2 {np.mean(z * z):.3f} over {z.size} block values")
    check(z)
    zf = gpu(True)
    print(f"ratio -> 1 - ratio: max |z| {np.abs(zf).max():.2f}, mean z^2 {np.mean(zf * zf):.3f}")
    with pytest.raises(AssertionError):
        check(zf)


# ---- the built-in scene -------------------------------------------------------

@pytest.fixture(scope="module")
def eve_assets():
    from conftest import REPO
    from gen_assets import ensure_assets
    return ensure_assets(REPO / "assets", mesh=False, eve=True)


@pytest.mark.gpu
def test_builtin_eve(ctx, eve_assets, tmp_path):
    import subprocess
    from pathlib import Path
    from PIL import Image

    W, H, spp = 96, 54, 4
    b = massrt.Builder(1).builtin("eve", float(massrt.ASPECT_RATIO), eve_assets)
    ctx.upload(b)
    rgb, bo = ctx.render(W, H, 0, spp, seed=1)
    assert np.isfinite(rgb).all() and rgb.any() and bo.any()
    albedo, normal = ctx.prepass(W, H, seed=1)
    normal = normal.reshape(-1, 3)
    on = normal.any(axis=1)
    assert on.sum() > W * H // 10
    assert np.abs(eve_ref.length(normal[on]) - 1.0).max() < 1e-3
    # the probe on the camera's pixel-centre rays against the restatement
    _, cam = b.desc()
    rays = camera_rays(cam, W, H)
    out = ctx.shade_rays(rays, seed=6)
    exp = restate(Desc(b), rays, out)
    e = exp["eve"]
    assert e.sum() > 50, int(e.sum())  # the fleet is small in this frame and the Volume takes half the rays
    assert np.array_equal(bits(out["uv"]), bits(exp["uv"]))
    assert np.array_equal(bits(out["normal"]), bits(exp["normal"]))
    assert np.array_equal((out["flags"] & 1) != 0, exp["front"])
    assert np.array_equal(bits(out["emitted"]), bits(exp["emitted"]))
    att = bits(out["attenuation"])
    assert np.all((att[e] == bits(f32(1.0))).all(axis=1) | (att[e] == bits(exp["color"][e])).all(axis=1))
    # the C++ example renders the scene by name: the library's bytes
    exe = Path(massrt.__file__).parent / "mrt_render"
    png = tmp_path / "eve.png"
    r = subprocess.run([str(exe), "eve", str(W), str(H), str(spp), str(png), str(eve_assets)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(png).convert("RGB")), ctx.tonemap(W, H, rgb, bo, spp, massrt.DISPLAY_DEFAULT))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "eve_normal.png").convert("RGB")),
                          ctx.tonemap(W, H, normal, bo, spp, massrt.DISPLAY_NORMAL))
