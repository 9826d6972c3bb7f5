"""k_shade's loads: the lane's slot, the primitive's shading header and the
material record are each fetched once, in batches. Only when
memory is read changed, so every shading-header class — sphere, world
triangle, model with an override, instance with and without an override, a
Mix at the root and as an override, an emitting leaf, a texture — must still
match the oracle: bounces bit for bit, radiance within the suite's RTOL, in
every k_shade variant (7 / 8 waves, counting or not), with k_shade or the
drain shading the bounces, with and without the survivor key (which takes
the root material's kind from shade_step instead of loading it), through
the fused kernel and the pre-pass (which share resolve_hit and scatter)."""
import numpy as np
import pytest

import massrt
from test_gpu_parity import ASPECT, RTOL, build_both, rel_l2

pytestmark = pytest.mark.gpu
W, H, SPP, SEED = 64, 36, 8, 31


def _grid_tris(n, shading):
    """An n x n grid of quads over [-1, 1]^2 in the plane z = 0: 9 floats per
    triangle, or 24 ({v, n, uv} x 3) with normals that lean with x and uvs."""
    g = np.linspace(-1.0, 1.0, n + 1, dtype=np.float32)
    rows = []
    for i in range(n):
        for j in range(n):
            x0, x1, y0, y1 = g[i], g[i + 1], g[j], g[j + 1]
            for tri in ([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0]], [[x0, y0, 0], [x1, y1, 0], [x0, y1, 0]]):
                row = []
                for v in tri:
                    row += list(v)
                    if shading:
                        row += [0.2 * v[0], 0.1 * v[1], 1.0] + [v[0] * 0.7 + 0.5, v[1] * 0.7 + 0.5]
                rows.append(row)
    return np.array(rows, dtype=np.float32)


_TEX = np.random.default_rng(5).integers(0, 256, size=(16, 24, 4), dtype=np.uint8)
_TEX[..., 3] = 255  # opaque: no alpha test, the fused kernel accepts the scene
_PLAIN, _SHADED = _grid_tris(3, False), _grid_tris(4, True)


def _all_headers(x):
    x.background(massrt.BG_SKY)
    st = x.texture_rgba(_TEX, massrt.WRAP_REPEAT)
    grey, red, blue = x.solid(0.6, 0.6, 0.6, 1.0), x.solid(0.9, 0.3, 0.2, 1.0), x.solid(0.2, 0.3, 0.9, 1.0)
    lamb = x.material(massrt.MAT_LAMBERTIAN, grey)
    metal = x.material(massrt.MAT_METAL, red, 0.3)
    glass = x.material(massrt.MAT_DIELECTRIC, 0, 1.5)
    light = x.material(massrt.MAT_DIFFUSE_LIGHT, 0, 0.0, (4.0, 4.0, 3.0))
    glow = x.mix(0.4, lamb, x.mix(0.5, light, metal))  # nested: the inner Mix's leaf emits
    textured = x.material(massrt.MAT_LAMBERTIAN, st)
    over_mix = x.mix(0.3, x.material(massrt.MAT_METAL, blue, 0.1), x.material(massrt.MAT_LAMBERTIAN, red))
    over_model = x.material(massrt.MAT_METAL, grey, 0.05)
    x.add_sphere(lamb, (0, -100.5, -1), 100.0)
    for k, m in enumerate([lamb, metal, glass, light, glow]):
        x.add_sphere(m, (-2.0 + k, 0.0, -1.0 - 0.3 * (k % 2)), 0.45)
    x.add_triangle(x.material(massrt.MAT_LAMBERTIAN, blue), [-3.5, -0.5, -3.0, 3.5, -0.5, -3.0, 0.0, 2.5, -3.6])
    x.model(lamb, _PLAIN + np.float32([0.0, 1.4, -2.0] * 3), override=over_model, add_to_world=True)
    m = x.model(textured, _SHADED, add_to_world=False, shading=True)
    x.add_instance(m, (-1.6, 0.5, 0.4), (0.1, 0.6, 0.05), (0.7, 0.6, 1.0), over_mix)
    x.add_instance(m, (1.7, 0.4, 0.5), (-0.2, -0.5, 0.1), (0.8, 0.7, 1.0))
    x.build_bvh()
    x.camera(55.0, (0.0, 1.0, 4.0), (0.0, 0.2, -1.0), aspect=ASPECT)


@pytest.fixture(scope="module")
def headers():
    """The scene, a context of its own and the oracle's answers, computed once."""
    b, o = build_both(_all_headers)
    o.reset_counters()
    orgb, obo = o.render(W, H, 0, SPP, seed=SEED)
    oc = o.counters()
    oa, on = o.prepass(W, H, seed=2)
    for a in (orgb, obo, oa, on):
        a.setflags(write=False)
    c = massrt.Context(0)
    c.upload(b)
    yield {"ctx": c, "builder": b, "rgb": orgb, "bounces": obo, "counters": oc, "albedo": oa, "normal": on,
           "finish_default": c.get_option("finish_paths")}
    c.close()


@pytest.mark.parametrize("shade_bin", [0, 2])
@pytest.mark.parametrize("finish", [0, None])  # 0: k_shade, not the drain, shades every bounce
@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("waves", [7, 8])
def test_every_header_class_in_every_variant(headers, waves, counters, finish, shade_bin):
    c = headers["ctx"]
    c.set_option("shade_waves", waves)
    c.set_option("finish_paths", headers["finish_default"] if finish is None else finish)
    c.set_option("shade_bin", shade_bin)
    try:
        c.reset_counters()
        rgb, bo = c.render(W, H, 0, SPP, seed=SEED, counters=counters)
        gc = c.counters()
    finally:
        c.set_option("shade_waves", -1)
        c.set_option("finish_paths", headers["finish_default"])
        c.set_option("shade_bin", -1)
    print(f"waves {waves} counters {counters} finish {finish} bin {shade_bin}: "
          f"bounces differ {int((bo != headers['bounces']).sum())}, rel L2 {rel_l2(rgb, headers['rgb']):.3e}")
    assert np.array_equal(bo, headers["bounces"])
    assert rel_l2(rgb, headers["rgb"]) <= RTOL
    if counters:
        for k in ("samples", "segments", "closest_hits", "bounces"):
            assert gc[k] == headers["counters"][k], (k, gc[k], headers["counters"][k])


def test_fused_kernel_shares_the_step(headers):
    c = headers["ctx"]
    rgb, bo = c.render(W, H, 0, SPP, seed=SEED, flags=massrt.RENDER_FUSED)
    print(f"fused: bounces differ {int((bo != headers['bounces']).sum())}, rel L2 {rel_l2(rgb, headers['rgb']):.3e}")
    assert np.array_equal(bo, headers["bounces"])
    assert rel_l2(rgb, headers["rgb"]) <= RTOL


def test_prepass_shares_the_header(headers):
    ga, gn = headers["ctx"].prepass(W, H, seed=2)
    print(f"prepass: normals differ {int((gn != headers['normal']).sum())}, albedo differ {int((ga != headers['albedo']).sum())}")
    assert np.array_equal(gn, headers["normal"])
    assert np.array_equal(ga, headers["albedo"])


def test_33_materials_stay_per_lane():
    """33 spheres, 33 material records: more distinct records than half a
    wave has lanes, so a register copy of the record shared across lanes by
    mistake would shade some lane with its neighbour's material."""
    kinds = [massrt.MAT_LAMBERTIAN, massrt.MAT_METAL, massrt.MAT_DIELECTRIC]

    def scene(x):
        x.background(massrt.BG_SKY)
        for k in range(33):
            kind = kinds[k % 3]
            s = x.solid(0.15 + 0.025 * k, 0.95 - 0.02 * k, 0.3 + 0.015 * (k % 7), 1.0)
            m = x.material(kind, 0 if kind == massrt.MAT_DIELECTRIC else s, (0.0, 0.02 * (k % 9), 1.3 + 0.01 * k)[k % 3])
            i, j = k % 11, k // 11
            x.add_sphere(m, (-1.5 + 0.3 * i, -0.3 + 0.3 * j, -0.1 * ((i + j) % 3)), 0.16)
        x.build_bvh()
        x.camera(40.0, (0.0, 0.0, 3.5), (0.0, 0.0, 0.0), aspect=ASPECT)
    b, o = build_both(scene)
    c = massrt.Context(0, options={"finish_paths": 0})
    try:
        c.upload(b)
        rgb, bo = c.render(W, H, 0, SPP, seed=7)
    finally:
        c.close()
    orgb, obo = o.render(W, H, 0, SPP, seed=7)
    print(f"33 materials: bounces differ {int((bo != obo).sum())}, rel L2 {rel_l2(rgb, orgb):.3e}")
    assert np.array_equal(bo, obo)
    assert rel_l2(rgb, orgb) <= RTOL
