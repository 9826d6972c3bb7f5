"""Shared cases of the per-hit shading parity tests (test_shade_oracle.py on the
CPU, test_gpu_shade_probe.py on the device): four small worlds, one per
k_shade_rays<RNG, EXT> variant, the ray groups aimed at them, and the
background scenes.

A Case is a scene function for build_both (tests/test_gpu_parity.py): called
with a massrt.Builder or an oracle.Scene it builds the same world and leaves
what the tests need to know about it in `info`.

Material numbering. The probe reports Hit::material as an index: the device
into the table the host builder interns (first use first, a Mix behind its
children, equal records merged), the oracle into its list in call order (a
Volume's Isotrophic joins it when the volume is added). The cases create
every material right before its first use, children before their Mix, no two
equal, and add a volume after the last material, so the two numberings are
the same; test_shade_oracle.py checks that against the builder's table.
"""
import numpy as np

import massrt

f32 = np.float32
S = 3.0  # site spacing
R = 0.7  # sphere radius
TEX_SIZES = [(1, 1), (1, 7), (8, 4), (9, 5), (17, 3)]  # (width, height): each side of the 8x4 upload block
WRAPS = [massrt.WRAP_REPEAT, massrt.WRAP_CLAMP]
UV0, UV1 = (-1.0, -0.5), (2.0, 1.5)  # the quads' uv range
QUAD_W, QUAD_H = 1.5, 1.0
ULPS = (0, 1, 4, 64)
SEED = 7            # of every probe call of the two tests
PRE_W, PRE_H = 64, 36  # the pre-pass anchor's frame
COMPOSITES = ["ycbcr", "lighten", "darken", "addition", "subtraction", "fallback", "blend_fallback"]
KIND_NAMES = ["none", "lambertian", "metal", "dielectric", "diffuse_light", "specular", "isotrophic", "mix"]


def site(col, row):
    return np.array([S * col, 0.0, -S * row])


def quad(p0, du, dv, normal, nscale=1.0):
    """Two triangles {v, n, uv} x 3 over p0 + a du + b dv, uv from UV0 to UV1."""
    p0, du, dv = (np.asarray(v, dtype=np.float64) for v in (p0, du, dv))
    n = np.asarray(normal, dtype=np.float64) * nscale
    c = [np.concatenate([p0 + a * du + b * dv, n, [UV0[0] + a * (UV1[0] - UV0[0]), UV0[1] + b * (UV1[1] - UV0[1])]])
         for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
    return np.array([np.concatenate([c[0], c[1], c[2]]), np.concatenate([c[0], c[2], c[3]])], dtype=f32)


def grid(p0, du, dv, normal, n, uv_scale):
    """n x n quads (2 n^2 triangles) over p0 + a du + b dv, uv = (a, b) * uv_scale."""
    p0, du, dv = (np.asarray(v, dtype=np.float64) for v in (p0, du, dv))
    tris = []
    for i in range(n):
        for j in range(n):
            c = [np.concatenate([p0 + a * du + b * dv, normal, [a * uv_scale, b * uv_scale]])
                 for a, b in ((i / n, j / n), ((i + 1) / n, j / n), ((i + 1) / n, (j + 1) / n), (i / n, (j + 1) / n))]
            tris += [np.concatenate([c[0], c[1], c[2]]), np.concatenate([c[0], c[2], c[3]])]
    return np.array(tris, dtype=f32)


def barrel(center=(0.0, 0.0, 0.0), radius=R, nu=8, nv=5):
    """A lat-long sphere without its caps: 2 nu nv triangles, smooth normals, uvs from UV0 to UV1."""
    th = np.linspace(0.15 * np.pi, 0.85 * np.pi, nv + 1)
    ph = np.linspace(0.0, 2.0 * np.pi, nu + 1)

    def vert(i, j):
        n = np.array([np.sin(th[j]) * np.cos(ph[i]), np.cos(th[j]), np.sin(th[j]) * np.sin(ph[i])])
        return np.concatenate([np.asarray(center) + radius * n, n,
                               [UV0[0] + (UV1[0] - UV0[0]) * i / nu, UV0[1] + (UV1[1] - UV0[1]) * j / nv]])

    tris = []
    for i in range(nu):
        for j in range(nv):
            q = [vert(i, j), vert(i + 1, j), vert(i + 1, j + 1), vert(i, j + 1)]
            tris += [np.concatenate([q[0], q[1], q[2]]), np.concatenate([q[0], q[2], q[3]])]
    return np.array(tris, dtype=f32)


class Info:
    """What a Case's world holds, for the ray generators and the floors."""

    def __init__(self):
        self.kinds, self.params = [], []  # per material index
        self.mat = {}        # name -> material index
        self.spheres = []    # per sphere id: (name, centre, radius, material)
        self.targets = []    # (name, centre, radius, weight, closed): what the broad rays aim at
        self.quads = {}      # (width, height, wrap) -> (p0, material)
        self.comp_quads = {}  # composite name -> (p0, material)
        self.ycbcr_mats = []  # materials whose colour goes through powf(2.2)
        self.instances = {}  # name -> instance id
        self.drawers = []    # (centre, radius) bounding what makes the traversal draw
        self.volumes = 0
        self.pane = None     # (p0, du, dv) of the glass pane with normals of length 3


class Case:
    def __init__(self, name, volume=False, alpha_mix=False, composite=False):
        self.name, self.volume, self.alpha_mix, self.composite = name, volume, alpha_mix, composite
        self.rng_on = volume or alpha_mix  # the traversal draws: the k_shade_rays<true, .> variants
        self.info = None

    def __call__(self, x):
        I = Info()
        M = massrt

        def mat(name, kind, surface=0, param=0.0, emit=(0.0, 0.0, 0.0)):
            I.mat[name] = x.material(kind, surface, param, emit)
            I.kinds.append(kind), I.params.append(param)
            return I.mat[name]

        def mix(name, ratio, left, right):
            I.mat[name] = x.mix(ratio, left, right)
            I.kinds.append(M.MAT_MIX), I.params.append(ratio)
            return I.mat[name]

        def sphere(name, m, c, r=R, weight=1):
            x.add_sphere(m, c, r)
            I.spheres.append((name, np.asarray(c, dtype=np.float64), r, m))
            I.targets.append((name, np.asarray(c, dtype=np.float64), abs(r), weight, True))

        n_inst = 0
        x.background(M.BG_SKY)
        rng = np.random.default_rng(41)
        tex, I.texels = {}, {}
        for (w, h) in TEX_SIZES:
            for wrap in WRAPS:
                px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
                px[..., 3] = rng.integers(1, 255, size=(h, w))  # alpha strictly between 0 and 1
                I.texels[(w, h, wrap)] = px
                tex[(w, h, wrap)] = x.texture_rgba(px, wrap)

        # the ground: a large sphere under everything, below where any ray group starts
        x.add_sphere(mat("ground", M.MAT_LAMBERTIAN, x.solid(0.5, 0.5, 0.45)), (10.5, -1001.5, -6.0), 1000.0)
        I.spheres.append(("ground", np.array([10.5, -1001.5, -6.0]), 1000.0, I.mat["ground"]))

        # row 0: one sphere per plain material
        lamb = mat("lamb", M.MAT_LAMBERTIAN, x.solid(0.8, 0.3, 0.2))
        sphere("lamb", lamb, site(0, 0), weight=2)
        metal0 = mat("metal0", M.MAT_METAL, x.solid(0.9, 0.8, 0.7), 0.0)
        sphere("metal0", metal0, site(1, 0), weight=2)
        metal03 = mat("metal03", M.MAT_METAL, x.solid(0.7, 0.8, 0.9), 0.3)
        sphere("metal03", metal03, site(2, 0))
        metal1 = mat("metal1", M.MAT_METAL, x.solid(0.6, 0.9, 0.5), 1.0)
        sphere("metal1", metal1, site(3, 0))
        metal_over = mat("metal_over", M.MAT_METAL, x.solid(0.9, 0.5, 0.6), 1.7)  # the builders clamp it to 1
        sphere("metal_over", metal_over, site(4, 0))
        light = mat("light", M.MAT_DIFFUSE_LIGHT, 0, 0.0, (4.0, 3.0, 2.5))
        sphere("light", light, site(5, 0), weight=4)
        none = mat("none", M.MAT_NONE)
        sphere("none", none, site(6, 0), weight=4)
        iso = mat("iso", M.MAT_ISOTROPHIC, 0, 0.0, (0.4, 0.7, 0.3))
        sphere("iso", iso, site(7, 0), weight=4)

        # row 1: Dielectric and Specular at three indices, negative radii
        glass = {}
        for k, ior in enumerate((1.5, 1.0, 0.7)):
            glass[ior] = mat(f"glass{ior}", M.MAT_DIELECTRIC, 0, ior)
            sphere(f"glass{ior}", glass[ior], site(k, 1))
        for k, ior in enumerate((1.5, 1.0, 0.7)):
            m = mat(f"spec{ior}", M.MAT_SPECULAR, x.solid(0.2 + 0.2 * k, 0.5, 0.9 - 0.2 * k), ior)
            sphere(f"spec{ior}", m, site(3 + k, 1))
        sphere("neg_glass", glass[1.5], site(6, 1), -R, weight=3)
        sphere("neg_lamb", lamb, site(7, 1), -R, weight=3)

        # row 2: Mix at ratio 1, 0 and 0.35, a nested Mix over a light; the uv mesh
        mix_a = mat("mix1_left", M.MAT_LAMBERTIAN, x.solid(0.1, 0.5, 0.9))
        mix_b = mat("mix1_right", M.MAT_METAL, x.solid(0.5, 0.9, 0.1), 0.0)
        sphere("mix1", mix("mix1", 1.0, mix_a, mix_b), site(0, 2), weight=3)
        mix_c = mat("mix0_left", M.MAT_DIFFUSE_LIGHT, 0, 0.0, (2.0, 3.0, 4.0))
        mix_d = mat("mix0_right", M.MAT_LAMBERTIAN, x.solid(0.3, 0.7, 0.6))
        sphere("mix0", mix("mix0", 0.0, mix_c, mix_d), site(1, 2), weight=3)
        sphere("mix035", mix("mix035", 0.35, lamb, glass[1.5]), site(2, 2), weight=2)
        inner = mix("glow_inner", 0.25, metal03, glass[1.5])
        sphere("glow", mix("glow", 0.5, light, inner), site(3, 2), weight=6)

        bmat = mat("mesh", M.MAT_METAL, tex[(9, 5, M.WRAP_REPEAT)], 0.3)
        blas = x.model(bmat, barrel(), add_to_world=False, shading=True)
        rot, sc = (0.3, 0.5, 0.7), (1.0, 0.6, 1.3)
        x.add_instance(blas, site(4, 2), rot, sc)
        I.instances["plain"], n_inst = n_inst, n_inst + 1
        I.targets.append(("inst_plain", site(4, 2), 0.6, 5, True))
        ov_i = mat("inst_override", M.MAT_LAMBERTIAN, x.solid(0.3, 0.6, 0.9))
        x.add_instance(blas, site(5, 2), (0.1, -0.2, 0.4), (1.2, 1.1, 0.7), ov_i)
        I.instances["override"], n_inst = n_inst, n_inst + 1
        I.targets.append(("inst_override", site(5, 2), 0.6, 5, True))
        x.model(bmat, barrel(site(6, 2)), add_to_world=True, shading=True)
        I.targets.append(("model_plain", site(6, 2), R, 2, True))
        ov_m = mat("model_override", M.MAT_SPECULAR, x.solid(0.7, 0.4, 0.8), 1.5)
        x.model(bmat, barrel(site(7, 2)), override=ov_m, add_to_world=True, shading=True)
        I.targets.append(("model_override", site(7, 2), R, 2, True))

        # rows 3 and 4: one uv quad per (texture size, wrap), facing +z
        for k, key in enumerate(I.texels):
            p0 = np.array([1.0 + 2.0 * (k % 5), 0.25, -S * (3 + k // 5)])
            q = mat(f"quad{key}", M.MAT_LAMBERTIAN, tex[key])
            x.model(q, quad(p0, (QUAD_W, 0, 0), (0, QUAD_H, 0), (0, 0, 1)), add_to_world=True, shading=True)
            I.quads[key] = (p0, q)
            I.targets.append((f"quad{key}", p0 + (QUAD_W / 2, QUAD_H / 2, 0), 0.4, 1, False))

        # row 5: a glass pane whose vertex normals have length 3, as a mesh file may carry them: dot(-ud, n)
        # exceeds 1 by far, and without Dielectric::scatter's min(., 1) the reflectance 0.04 becomes negative
        p0 = np.array([1.0, 0.25, -S * 5])
        x.model(glass[1.5], quad(p0, (2.0, 0, 0), (0, 2.0, 0), (0, 0, 1), nscale=3.0), add_to_world=True, shading=True)
        I.pane = (p0, np.array([2.0, 0, 0]), np.array([0, 2.0, 0]))
        I.targets.append(("pane", p0 + (1.0, 1.0, 0), 0.8, 1, False))

        if self.composite:  # row 6: one uv quad per composite surface; row 7: some of them on spheres
            RP, CL = M.WRAP_REPEAT, M.WRAP_CLAMP
            yc = x.ycbcr(tex[(8, 4, RP)], tex[(9, 5, CL)])
            surf = {
                "ycbcr": yc,
                "lighten": x.blend(M.BLEND_LIGHTEN, tex[(17, 3, RP)], tex[(1, 7, CL)]),
                "darken": x.blend(M.BLEND_DARKEN, tex[(9, 5, RP)], x.solid(0.6, 0.5, 0.4, 0.5)),
                "addition": x.blend(M.BLEND_ADDITION, tex[(8, 4, CL)], tex[(1, 7, RP)]),
                "subtraction": x.blend(M.BLEND_SUBTRACTION, tex[(17, 3, CL)], tex[(9, 5, RP)]),
                "fallback": x.fallback((0.2, 0.3, 0.4, 1.0), tex[(8, 4, RP)]),
            }
            # texture, texture, texture on the operand stack before the first operator
            surf["blend_fallback"] = x.blend(M.BLEND_LIGHTEN, tex[(1, 1, CL)], x.fallback(
                (0.9, 0.1, 0.5, 0.7), x.blend(M.BLEND_DARKEN, tex[(1, 7, RP)], tex[(17, 3, RP)])))
            for k, name in enumerate(COMPOSITES):
                p0 = np.array([1.0 + 2.0 * k, 0.25, -S * 6])
                q = mat(f"comp_{name}", M.MAT_LAMBERTIAN, surf[name])
                x.model(q, quad(p0, (QUAD_W, 0, 0), (0, QUAD_H, 0), (0, 0, 1)), add_to_world=True, shading=True)
                I.comp_quads[name] = (p0, q)
                I.targets.append((f"comp_{name}", p0 + (QUAD_W / 2, QUAD_H / 2, 0), 0.4, 1, False))
            I.ycbcr_mats.append(I.mat["comp_ycbcr"])
            sphere("sph_ycbcr", I.mat["comp_ycbcr"], site(0, 7))  # spheres have no uv: sampled at (0, 0)
            sphere("sph_sub", mat("metal_sub", M.MAT_METAL, surf["subtraction"], 0.2), site(1, 7))
            sphere("sph_fallback", mat("spec_fallback", M.MAT_SPECULAR, surf["fallback"], 1.5), site(2, 7))
            sphere("sph_blend_fallback", I.mat["comp_blend_fallback"], site(3, 7))
            m = mat("metal_ycbcr", M.MAT_METAL, yc, 0.1)
            I.ycbcr_mats.append(m)
            sphere("sph_metal_ycbcr", m, site(4, 7))

        if self.alpha_mix:  # row -1: a Mix over cut-out textures: its alpha test draws during the walk
            arng = np.random.default_rng(11)
            cut = []
            for p in (0.3, 0.5):
                t = arng.integers(0, 256, size=(16, 24, 4), dtype=np.uint8)
                t[..., 3] = np.where(arng.random((16, 24)) < p, 0, 255)
                cut.append(x.texture_rgba(t, M.WRAP_REPEAT))
            ma = mat("alpha_left", M.MAT_LAMBERTIAN, cut[0])
            mb = mat("alpha_right", M.MAT_METAL, cut[1], 0.2)
            p0 = site(0, -1) + (-1.0, -1.0, 0.0)
            x.model(mix("alpha_mix", 0.4, ma, mb), grid(p0, (2.0, 0, 0), (0, 2.0, 0), (0, 0, 1), 4, 1.7),
                    add_to_world=True, shading=True)
            I.targets.append(("alpha_mix", site(0, -1), 0.9, 8, False))
            I.drawers.append((site(0, -1), np.sqrt(2.0)))

        if self.volume:  # row -1: a medium with a small sphere inside; its material is the table's last
            c = site(3, -1)
            sphere("in_volume", lamb, c, 0.4, weight=3)
            x.add_volume(c, 1.2, 0.8, (0.6, 0.7, 0.8))
            I.mat["volume"] = len(I.kinds)
            I.kinds.append(M.MAT_ISOTROPHIC), I.params.append(0.0)
            I.volumes = 1
            I.targets.append(("volume", c, 1.2, 5, False))
            I.drawers.append((c, 1.2))

        x.build_bvh()
        x.camera(60.0, (10.5, 5.0, 9.0), (10.5, 0.0, -6.0), aspect=float(M.ASPECT_RATIO), aperture=0.0)  # the pre-pass anchor's
        I.kinds, I.params = np.array(I.kinds, dtype=np.uint32), np.array(I.params, dtype=f32)
        self.info = I


CASES = {
    "plain": Case("plain"),
    "draws": Case("draws", volume=True, alpha_mix=True),
    "composite": Case("composite", composite=True),
    "both": Case("both", volume=True, composite=True),
}


# ---- ray groups ---------------------------------------------------------------

def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rays(o, d):
    return np.concatenate([o, d], 1).astype(f32)


def broad_rays(info, seed=5, per_weight=(60, 30)):
    """Towards every object from outside, and from inside the closed ones (back faces)."""
    rng = np.random.default_rng(seed)
    out = []
    for _name, c, r, weight, closed in info.targets:
        n = per_weight[0] * weight
        aim = c + rng.uniform(-0.8, 0.8, size=(n, 3)) * r
        up = _unit(rng.normal(size=(n, 3)))
        up[:, 1] = np.abs(up[:, 1])  # from above the ground
        o = c + up * rng.uniform(2.0, 6.0, size=(n, 1))
        out.append(_rays(o, (aim - o) * rng.uniform(0.2, 3.0, size=(n, 1))))  # directions are not unit length
        if closed:
            n = per_weight[1] * weight
            out.append(_rays(c + rng.uniform(-0.3, 0.3, size=(n, 3)) * r, rng.normal(size=(n, 3))))
    return np.concatenate(out)


def lattice_lines(width, height):
    """The u and v values where a texel or a wrap boundary lies, strictly inside the quads' uv range."""
    def lines(n, lo, hi):
        v = {float(m) for m in range(int(np.floor(lo)), int(np.ceil(hi)) + 1)}
        if n > 1:
            v |= {m + k / (n - 1) for m in range(int(np.floor(lo)), int(np.ceil(hi)) + 1) for k in range(n - 1)}
        return sorted(t for t in v if lo + 1e-6 < t < hi - 1e-6)
    return lines(width, UV0[0], UV1[0]), lines(height, UV0[1], UV1[1])


def _quad_rays(p0, uv, axis, rng):
    """Rays at the quad point with texture coordinates uv (n x 2): for every point and every k in ULPS the
    target moved by -k, +k ULP of its coordinate along `axis`, once head-on and once obliquely."""
    uv = np.asarray(uv, dtype=np.float64)
    a = (uv[:, 0] - UV0[0]) / (UV1[0] - UV0[0])
    b = (uv[:, 1] - UV0[1]) / (UV1[1] - UV0[1])
    p = (p0[None, :] + a[:, None] * np.array([QUAD_W, 0, 0]) + b[:, None] * np.array([0, QUAD_H, 0])).astype(f32)
    pts = []
    for k in sorted({s * u for u in ULPS for s in (-1, 1)}):
        q = p.copy()
        q[:, axis] = q[:, axis] + f32(k) * np.spacing(q[:, axis])
        pts.append(q)
    p = np.concatenate(pts)
    n = p.shape[0]
    front = p + np.array([0, 0, 1.5], dtype=f32)
    head_on = _rays(front, np.broadcast_to(np.array([0, 0, -1], dtype=f32), (n, 3)))
    o = front + np.concatenate([rng.uniform(-0.7, 0.7, size=(n, 2)), np.zeros((n, 1))], 1).astype(f32)
    return np.concatenate([head_on, _rays(o, p - o)])


def lattice_rays(info, seed=6, per_line=1, interior=120):
    """The texture lattice: both sides of every integer line and texel boundary of every (size, wrap) quad,
    and plain interior points, half of them inside [0, 1]^2."""
    rng = np.random.default_rng(seed)
    out = []

    def cross(n, lo, hi):  # the other coordinate: half inside [0, 1], half anywhere on the quad
        return np.where(rng.random(n) < 0.5, rng.uniform(0.02, 0.98, n), rng.uniform(lo + 0.02, hi - 0.02, n))

    for (w, h, _wrap), (p0, _m) in info.quads.items():
        us, vs = lattice_lines(w, h)
        u = np.repeat(us, per_line)
        out.append(_quad_rays(p0, np.stack([u, cross(u.size, UV0[1], UV1[1])], 1), 0, rng))
        v = np.repeat(vs, per_line)
        out.append(_quad_rays(p0, np.stack([cross(v.size, UV0[0], UV1[0]), v], 1), 1, rng))
        n = (20 if w * h == 1 else interior // 14)  # _quad_rays returns 14 rays per point; a 1x1 has few lines
        out.append(_quad_rays(p0, np.stack([cross(n, UV0[0], UV1[0]), cross(n, UV0[1], UV1[1])], 1), 0, rng))
    for _name, (p0, _m) in info.comp_quads.items():
        us, vs = lattice_lines(9, 5)
        out.append(_quad_rays(p0, np.stack([us, cross(len(us), UV0[1], UV1[1])], 1), 0, rng))
        out.append(_quad_rays(p0, np.stack([cross(len(vs), UV0[0], UV1[0]), vs], 1), 1, rng))
    return np.concatenate(out)


def _incidence_rays(c, r, theta, inside, rng, back=1.0):
    """Rays meeting the sphere (c, |r|) at angle theta to its normal, from inside or from outside."""
    n = _unit(rng.normal(size=(theta.size, 3)))
    t = _unit(np.cross(n, rng.normal(size=(theta.size, 3))))
    p = c + abs(r) * n
    ct, st = np.cos(theta)[:, None], np.sin(theta)[:, None]
    if inside:
        d = ct * n + st * t
        o = p - d * (abs(r) * ct)  # the chord's midpoint
    else:
        d = -ct * n + st * t
        o = p - d * back
    return _rays(o, d * rng.uniform(0.5, 2.0, size=(theta.size, 1)))


def sweep(ratio, rng, dense=250, wide=250):
    """Incidence angles: uniform up to grazing, and dense across the critical angle where there is one."""
    th = [rng.uniform(0.0, np.radians(89.9), wide)]
    if ratio > 1.0:
        th.append(np.arcsin(1.0 / ratio) + rng.uniform(-1.5e-3, 1.5e-3, dense) / np.sqrt(ratio * ratio - 1.0))
    return np.concatenate(th)


def dielectric_rays(info, seed=7):
    """Glass and Specular spheres from inside and outside: across the critical angle (ratio sin = 1), at
    normal incidence (cos reaches the min(., 1)) and at grazing incidence; the pane with over-long normals."""
    rng = np.random.default_rng(seed)
    sph = {s[0]: s for s in info.spheres}
    out = []
    for kind in ("glass", "spec"):
        for ior in (1.5, 1.0, 0.7):
            _n, c, r, _m = sph[f"{kind}{ior}"]
            out.append(_incidence_rays(c, r, sweep(ior, rng), True, rng))        # ratio = ior
            out.append(_incidence_rays(c, r, sweep(1.0 / ior, rng), False, rng))  # ratio = 1 / ior
        _n, c, r, _m = sph[f"{kind}1.5"]
        out.append(_incidence_rays(c, r, rng.uniform(np.radians(75.0), np.radians(89.5), 300), False, rng))
        out.append(_incidence_rays(c, r, np.zeros(300), False, rng))  # head-on
        out.append(_rays(np.broadcast_to(c, (100, 3)), rng.normal(size=(100, 3))))  # from the centre
    p0, du, dv = info.pane
    n = 800
    p = p0 + rng.uniform(0.05, 0.95, (n, 1)) * du + rng.uniform(0.05, 0.95, (n, 1)) * dv
    th, ph = rng.uniform(0.0, np.radians(75.0), n), rng.uniform(0.0, 2 * np.pi, n)
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], 1)
    d[n // 2:, 2] *= -1.0  # the second half from behind
    out.append(_rays(p - d, d))
    return np.concatenate(out)


def metal_rays(info, seed=8, n=500):
    """Grazing rays onto the fuzz-1 spheres: scattered and absorbed both occur; fuzz 0 and 0.3 for contrast."""
    rng = np.random.default_rng(seed)
    sph = {s[0]: s for s in info.spheres}
    out = []
    for name, lo, k in (("metal1", 60.0, n), ("metal_over", 60.0, n), ("metal03", 70.0, n // 2), ("metal0", 0.0, n // 2)):
        _n, c, r, _m = sph[name]
        out.append(_incidence_rays(c, r, rng.uniform(np.radians(lo), np.radians(89.5), k), False, rng))
    return np.concatenate(out)


def all_rays(info):
    """Every group in one array, with the slice of each."""
    groups = [("broad", broad_rays(info)), ("lattice", lattice_rays(info)), ("dielectric", dielectric_rays(info)),
              ("metal", metal_rays(info))]
    at, where = 0, {}
    for name, r in groups:
        where[name] = slice(at, at + r.shape[0])
        at += r.shape[0]
    return np.concatenate([r for _n, r in groups]), where


def draws_nothing(rays, info):
    """Rays whose line stays clear of everything that makes the traversal draw (a Volume, a Mix alpha test)."""
    o, d = rays[:, :3].astype(np.float64), _unit(rays[:, 3:].astype(np.float64))
    ok = np.ones(rays.shape[0], dtype=bool)
    for c, r in info.drawers:
        ok &= np.linalg.norm(np.cross(c - o, d), axis=1) > 1.01 * r
    return ok


def prepass_rays(fields, W, H):
    """Camera::albedo_normal's rays with a closed aperture (world.rs:53-63,81-92)."""
    c = np.asarray(fields, dtype=f32)
    origin, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    x, y = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    u = (x.ravel() / f32(W - 1))[:, None]
    v = (y.ravel() / f32(H - 1))[:, None]
    d = (((llc + hor * u) + ver * v) - origin) - f32(0.0)
    return np.concatenate([np.broadcast_to(origin, d.shape), d], 1).astype(f32)


# ---- what a record array says (the floors of both tests) ------------------------

def reflect(v, n):
    v, n = v.astype(f32), n.astype(f32)
    dot = ((v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) + v[:, 2] * n[:, 2])[:, None]
    return v - ((n * dot) * f32(2.0))


def unit32(v):
    v = v.astype(f32)
    return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]


def coverage(info, rays, rec):
    """Counts of what the hits in `rec` (shade_rays records of `rays`) reached: name -> count."""
    M = massrt
    hit = rec["prim"] != 0
    kind = np.where(hit, info.kinds[np.where(hit, rec["material"], 0)], 0xFF)
    scattered = (rec["flags"] & M.SHADE_SCATTERED) != 0
    front = (rec["flags"] & M.SHADE_FRONT_FACE) != 0
    has_uv = (rec["flags"] & M.SHADE_HAS_UV) != 0
    pk, pi = rec["prim"] >> 28, rec["prim"] & 0x0FFFFFFF
    c = {f"kind_{KIND_NAMES[k]}": int((kind == k).sum()) for k in range(8)}
    metal = kind == M.MAT_METAL
    c["metal_scattered"], c["metal_absorbed"] = int((metal & scattered).sum()), int((metal & ~scattered).sum())

    # Dielectric and Specular: ratio sin(theta) as Dielectric::scatter computes it (material.rs:299-305)
    ud = unit32(rays[:, 3:])
    n = rec["normal"].astype(f32)
    cos = np.minimum(((-ud[:, 0] * n[:, 0] + -ud[:, 1] * n[:, 1]) + -ud[:, 2] * n[:, 2]), f32(1.0))
    with np.errstate(invalid="ignore"):
        sin = np.sqrt(f32(1.0) - cos * cos)
    param = info.params[np.where(hit, rec["material"], 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(front, f32(1.0) / param, param).astype(f32)
        rs = ratio * sin
    # (a refracted direction is never this close to the mirrored one in these cases: ior 1 at 89.9 degrees
    # leaves 3.5e-3 between them)
    mirrored = np.all(np.abs(reflect(ud, n) - rec["direction"]) <= 1e-5, axis=1)
    glass = kind == M.MAT_DIELECTRIC
    c["glass_tir"] = int((glass & (rs > 1.0)).sum())
    c["glass_schlick"] = int((glass & ~(rs > 1.0) & mirrored).sum())
    c["glass_refracted"] = int((glass & ~(rs > 1.0) & ~mirrored).sum())
    c["glass_just_above"] = int((glass & (rs > 1.0) & (rs < 1.0 + 1e-3)).sum())
    c["glass_just_below"] = int((glass & (rs <= 1.0) & (rs > 1.0 - 1e-3)).sum())
    spec = kind == M.MAT_SPECULAR
    white = np.all(rec["attenuation"] == 1.0, axis=1)
    c["specular_mirror"] = int((spec & white & mirrored).sum())
    c["specular_inner"] = int((spec & scattered & ~white).sum())

    for name, (_p0, m) in info.comp_quads.items():
        c[f"composite_{name}"] = int((hit & has_uv & (rec["material"] == m)).sum())
    uv = rec["uv"]
    inside = np.all((uv >= 0.0) & (uv <= 1.0), axis=1)
    for key, (_p0, m) in info.quads.items():
        on = hit & has_uv & (rec["material"] == m)
        c[f"tex{key}_inside"], c[f"tex{key}_outside"] = int((on & inside).sum()), int((on & ~inside).sum())

    neg = [i for i, s in enumerate(info.spheres) if s[2] < 0]
    c["negative_radius"] = int((hit & (pk == M.REF_SPHERE) & np.isin(pi, neg)).sum())
    c["back_face"] = int((hit & ~front).sum())
    ck, ci = rec["container"] >> 28, rec["container"] & 0x0FFFFFFF
    c["instance_override"] = int((hit & (ck == M.REF_INSTANCE) & (ci == info.instances["override"])).sum())
    c["instance_plain"] = int((hit & (ck == M.REF_INSTANCE) & (ci == info.instances["plain"])).sum())
    c["emitted_and_scattered"] = int((hit & scattered & np.any(rec["emitted"] != 0.0, axis=1)).sum())
    c["volume"] = int((pk == M.REF_VOLUME).sum())
    c["alpha_mix"] = int((hit & (rec["material"] == info.mat.get("alpha_mix", 0xFFFFFFFF))).sum())
    return c


def floors(case):
    """name -> least count (the issue's coverage floors) for this case."""
    info = case.info
    f = {f"kind_{k}": 200 for k in KIND_NAMES}
    f.update(metal_scattered=200, metal_absorbed=200, glass_tir=200, glass_schlick=100, glass_refracted=200,
             glass_just_above=50, glass_just_below=50, specular_mirror=100, specular_inner=100, negative_radius=200,
             back_face=500, instance_override=200, instance_plain=200, emitted_and_scattered=50)
    for key in info.quads:
        f[f"tex{key}_inside"] = f[f"tex{key}_outside"] = 100
    for name in info.comp_quads:
        f[f"composite_{name}"] = 200
    if case.volume:
        f["volume"] = 200
    if case.alpha_mix:
        f["alpha_mix"] = 200
    return f


# ---- backgrounds ------------------------------------------------------------------

BG_CAMERAS = {"ppp": (1.0, 1.0, 1.0), "nnn": (-1.0, -1.0, -1.0), "px": (1.0, 0.0, 0.0)}
BG_W, BG_H = 32, 18
BG_ROTATION = (0.05, 0.1, -0.2)


def background_case(kind, camera="ppp", index_faces=False):
    """A world of one small MAT_NONE sphere under background `kind` ("solid", "sky", "cubemap"), seen through
    a vfov-100 camera at the origin. index_faces: the CubeMap's faces are solids whose red is face + 1."""
    M = massrt

    def scene(x):
        rng = np.random.default_rng(17)
        if kind == "solid":
            x.background(M.BG_SOLID, 0, (0.25, 0.5, 0.75))
        elif kind == "sky":
            x.background(M.BG_SKY)
        elif index_faces:
            x.background_cubemap([x.solid(k + 1.0, 0.0, 0.0, 1.0) for k in range(6)], BG_ROTATION)
        else:
            t = [x.texture_rgba(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8), wrap)
                 for (w, h, wrap) in ((9, 5, M.WRAP_REPEAT), (8, 4, M.WRAP_CLAMP), (17, 3, M.WRAP_REPEAT), (5, 6, M.WRAP_CLAMP))]
            faces = [t[0], t[1], x.solid(0.3, 0.6, 0.9, 1.0), x.blend(M.BLEND_LIGHTEN, t[2], x.solid(0.4, 0.1, 0.2, 1.0)),
                     x.fallback((0.2, 0.3, 0.4, 1.0), t[3]), t[2]]
            x.background_cubemap(faces, BG_ROTATION)
        x.add_sphere(x.material(M.MAT_NONE), (1.0, 1.0, 1.0), 0.2)
        x.build_bvh()
        x.camera(100.0, (0.0, 0.0, 0.0), BG_CAMERAS[camera], aspect=float(M.ASPECT_RATIO), aperture=0.0)
    return scene


BG_CASES = [("solid", "ppp"), ("sky", "ppp"), ("cubemap", "ppp"), ("cubemap", "nnn"), ("cubemap", "px")]
