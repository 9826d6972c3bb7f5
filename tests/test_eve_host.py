"""EveMaterial on the host: the builder's tangent frames against the numpy
restatement (tests/eve_ref.py), the OBJ group filter, Builder.eve_material's
argument checks, the scene extension it fills and the built-in "eve" scene
against scenes/eve.rs read by hand. (That plain mrt_upload_scene rejects an
MRT_MAT_EVE description needs a context, so it is in tests/test_gpu_eve.py.)"""
import numpy as np
import pytest

import eve_ref
import massrt

COLORS = [[0.02, 0.02, 0.02], [0.2, 0.2, 0.2], [1.0, 1.0, 1.0], [0.5, 0.0, 0.0]]
GLOW = [0.5, 0.85, 2.0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _eve(b, shape=(3, 2)):
    rng = np.random.default_rng(5)
    tex = [b.texture_rgba(rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)) for _ in range(3)]
    return b.eve_material(*tex, COLORS, GLOW)


def test_tangent_frames_equal_the_restatement():
    """Triangle::with_norms_and_uvs (geom.rs:474-482): random triangles, and uvs
    whose determinant is 0, tiny, huge or negative (the clamp of r to [-1, 1])."""
    rng = np.random.default_rng(11)
    n = 64
    t = rng.normal(size=(n, 3, 8)).astype(np.float32)
    t[0, :, 6:8] = [[0.25, 0.5]] * 3                      # one uv point: 1/0 -> +inf -> 1
    t[1, :, 6:8] = [[0, 0], [1, 1], [2, 2]]               # collinear uvs: det 0
    t[2, :, 6:8] = [[0, 0], [0, 1], [1, 0]]               # det -1
    t[3, :, 6:8] = [[0, 0], [1e-4, 0], [0, 1e-4]]         # 1/det = 1e8 -> 1
    t[4, :, 6:8] = [[0, 0], [0, 1e-4], [1e-4, 0]]         # -> -1
    t[5, :, 6:8] = [[0, 0], [40, 0], [0, 40]]             # |r| < 1 kept
    t[6, :, 6:8] = [[0.5, 0.5], [0.5, 0.5], [0.75, 0.5]]  # det -0.0 or +0.0 by sign of the products
    b = massrt.Builder(1)
    m = _eve(b)
    b.model(m, t.reshape(n, 24), add_to_world=True, shading=True)
    d = b.desc_only()
    assert d.n_triangles == n
    T = np.array([list(d.triangles[i].tangent) for i in range(n)], dtype=np.float32)
    B = np.array([list(d.triangles[i].bitangent) for i in range(n)], dtype=np.float32)
    # the builder keeps the triangles in the order given
    assert np.array_equal(np.array([list(d.triangles[i].a) for i in range(n)], dtype=np.float32), t[:, 0, :3])
    rt, rb = eve_ref.tangent_frame(t[:, 0, :3], t[:, 1, :3], t[:, 2, :3], t[:, 0, 6:8], t[:, 1, 6:8], t[:, 2, 6:8])
    assert np.array_equal(bits(T), bits(rt))
    assert np.array_equal(bits(B), bits(rb))
    assert np.all(np.isfinite(T[:7])) and np.all(np.isfinite(B[:7]))  # the clamp kept the degenerate ones finite


def test_plain_triangles_have_a_zero_frame():
    b = massrt.Builder(1)
    m = b.material(massrt.MAT_LAMBERTIAN, b.solid(1, 1, 1))
    b.model(m, np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], dtype=np.float32), add_to_world=True)
    t = b.desc_only().triangles[0]
    assert list(t.tangent) == [0, 0, 0] and list(t.bitangent) == [0, 0, 0]  # Triangle::new, geom.rs:463-464


OBJ = """\
v 0 0 0
v 1 0 0
v 0 1 0
vt 0 0
vt 1 0
vt 0 1
vn 0 0 1
f 1/1/1 2/2/1 3/3/1
o Hull
v 0 0 1
v 1 0 1
v 0 1 1
f 4/1/1 5/2/1 6/3/1
g Antenna
v 0 0 2
v 1 0 2
v 0 1 2
f 7/1/1 8/2/1 9/3/1
g
f 7/1/1 8/2/1 9/3/1
g Glass
f 7/2/1 8/3/1 9/1/1
f 1/1/1 5/2/1 9/3/1
o
f 4/3/1 5/1/1 6/2/1
o hull
f 1/1/1 2/2/1 3/3/1
"""


def test_load_obj_groups(tmp_path):
    """ObjLoader::with_filter (obj_loader.rs:348,394-397,431-436): groups set by
    `o` and by `g`; a line without a name changes nothing; faces before the
    first group are dropped; vertices of dropped groups still count."""
    p = tmp_path / "g.obj"
    p.write_text(OBJ)
    every = massrt.load_obj(p).reshape(-1, 3, 8)
    assert every.shape[0] == 8
    assert np.array_equal(massrt.load_obj_groups(p, []).reshape(-1, 3, 8), every)  # no groups: no filter
    z = lambda tris: [tuple(float(c[2]) for c in t) for t in tris]  # noqa: E731 - the corners' z name the vertices
    got = massrt.load_obj_groups(p, ["Hull", "Glass"]).reshape(-1, 3, 8)
    # Hull's face; not Antenna's two (the unnamed `g` keeps Antenna); Glass's two,
    # one of them over vertices of Antenna; the unnamed `o` keeps Glass; `hull` is another name
    assert z(got) == [(1, 1, 1), (2, 2, 2), (0, 1, 2), (1, 1, 1)]
    assert np.array_equal(got[1, :, 6:8], np.array([[1, 0], [0, 1], [0, 0]], dtype=np.float32))
    assert z(massrt.load_obj_groups(p, ["Antenna"]).reshape(-1, 3, 8)) == [(2, 2, 2), (2, 2, 2)]
    assert z(massrt.load_obj_groups(p, ["hull"]).reshape(-1, 3, 8)) == [(0, 0, 0)]
    assert massrt.load_obj_groups(p, ["Nothing"]).shape == (0, 24)
    with pytest.raises(massrt.MassrtError, match="cannot open"):
        massrt.load_obj_groups(tmp_path / "missing.obj", ["Hull"])


def test_eve_material_arguments():
    b = massrt.Builder(1)
    tex = b.texture_rgba(np.zeros((1, 1, 4), dtype=np.uint8))
    solid = b.solid(1, 1, 1)
    with pytest.raises(massrt.MassrtError, match="texture surfaces"):
        b.eve_material(tex, solid, tex, COLORS, GLOW)
    with pytest.raises(massrt.MassrtError, match="texture surfaces"):
        b.eve_material(b.ycbcr(tex, tex), tex, tex, COLORS, GLOW)
    with pytest.raises(massrt.MassrtError, match="out of range"):
        b.eve_material(tex, tex, 99, COLORS, GLOW)
    assert massrt.lib().mrt_builder_eve_material(b.h, tex, tex, tex, None, None) == -1  # -MRT_ERR_INVALID
    m = b.eve_material(tex, tex, tex, COLORS, GLOW)
    assert m >= 0


def test_scene_extension_holds_the_eve_table():
    """desc(): an MRT_MAT_EVE material whose `surface` names its record in
    mrt_scene_ext.eve_materials; equal EveMaterials share one record."""
    b = massrt.Builder(1)
    rng = np.random.default_rng(2)
    no, ar, pm = (b.texture_rgba(rng.integers(0, 256, size=(2, 2, 4), dtype=np.uint8)) for _ in range(3))
    m1 = b.eve_material(no, ar, pm, COLORS, GLOW)
    m2 = b.eve_material(no, ar, pm, COLORS, [1, 2, 3])
    m3 = b.eve_material(no, ar, pm, COLORS, GLOW)
    for k, m in enumerate((m1, m2, m3)):
        b.add_sphere(m, (3.0 * k, 0, 0), 1.0)
    lam = b.material(massrt.MAT_LAMBERTIAN, b.solid(1, 1, 1))
    b.add_sphere(lam, (0, 5, 0), 1.0)
    d, ext = b.desc_only(), b.desc_ext()
    assert ext.n_eve_materials == 2
    mats = [d.materials[d.spheres[k].material] for k in range(3)]
    assert [m.kind for m in mats] == [massrt.MAT_EVE] * 3
    assert [m.surface for m in mats] == [0, 1, 0]
    e0, e1 = ext.eve_materials[0], ext.eve_materials[1]
    assert len({e0.normal_occlusion, e0.albedo_roughness, e0.pmdg}) == 3 and e0.pmdg < d.n_textures
    assert np.array_equal(np.array(list(e0.colors), dtype=np.float32), np.array(COLORS, dtype=np.float32).ravel())
    assert list(e1.glow) == [1.0, 2.0, 3.0]
    # a scene without Eve materials has an empty table
    b2 = massrt.Builder(1)
    b2.add_sphere(b2.material(massrt.MAT_LAMBERTIAN, b2.solid(1, 1, 1)), (0, 0, 0), 1.0)
    b2.desc_only()
    assert b2.desc_ext().n_eve_materials == 0


def test_builtin_eve_mirrors_the_scene(tmp_path):
    """scenes/eve.rs:21-97 by hand. Draws of the scene stream: one axis per
    BvhNode::new call of the two hulls' Model::new (N(n) = 1 + N(n/2) + N(n - n/2),
    N(1) = N(2) = 1; 3136 kept triangles each), V3::rand() for the orca's
    rotation, then per fleet cell one f32::rand() for y and, as no cell lies
    within 50 of the camera, V3::rand() for its rotation: all 36 are kept; then
    World::build_bvh over 37 instances, the Volume and the sun."""
    import functools

    import oracle
    from conftest import REPO
    from gen_assets import ensure_assets

    assets = ensure_assets(REPO / "assets", mesh=False, eve=True)
    kept = massrt.load_obj_groups(assets / "eve" / "stratios.obj",
                                  ["Hull", "hull", "Glass", "glass", "DarkHull", "exhaust", "Exhaust"]).shape[0]
    assert kept == 3136 < massrt.load_obj(assets / "eve" / "stratios.obj").shape[0]  # EveFilter drops the Antenna
    b = massrt.Builder(1).builtin("eve", float(massrt.ASPECT_RATIO), assets)
    d, cam = b.desc()
    ext = b.desc_ext()
    assert (d.n_instances, d.n_volumes, d.n_spheres, d.n_triangles) == (37, 1, 1, 2 * kept)
    assert ext.n_eve_materials == 2 and d.background.kind == massrt.BG_CUBEMAP
    assert all(d.triangles[i].flags & 1 for i in (0, kept, 2 * kept - 1))
    assert d.materials[d.triangles[0].material].kind == massrt.MAT_EVE

    @functools.lru_cache(None)
    def nodes(n):
        return 1 if n <= 2 else 1 + nodes(n // 2) + nodes(n - n // 2)

    first = 2 * nodes(kept)
    total = first + 3 + 36 * 4 + nodes(37 + 1 + 1)
    _, f = oracle.wyrand(1, total + 1)
    assert b.rand_f32() == f[total]  # the scene stream stands where the reference's would
    one, two = np.float32(1.0), np.float32(2.0)
    # the orca (eve.rs:34-39), then the fleet in loop order (eve.rs:57-72)
    t0 = np.array(list(d.instances[0].fwd), dtype=np.float32)[12:15]
    assert np.array_equal(t0, np.array([-1250.0, 5.0, 0.0], dtype=np.float32))
    k = 1
    for xi in range(6):
        for zi in range(6):
            at = first + 3 + 4 * (k - 1)
            y = (f[at] * two - one) * np.float32(150.0)
            want = np.array([(np.float32(xi) - 3) * 190, y, (np.float32(zi) - 3) * 190], dtype=np.float32)
            got = np.array(list(d.instances[k].fwd), dtype=np.float32)
            assert np.array_equal(got[12:15], want), (xi, zi)
            k += 1
    c = cam.fields()
    assert np.array_equal(c[0:3], np.array([0.0, -20.0, 500.0], dtype=np.float32)) and c[18] == np.float32(0.1)
