"""Adversarial geometry, as data: worlds at the edges of the near-first walk's per-scene hypotheses
(nf_tree.cpp: the domain gates, tri_bound's choice between the coordinate-plane and the generic bound,
degenerate triangles, the wild() split), beside adversarial_rays.py's rays, which probe the per-ray half.

A world is a list of plain ops over float32 values drawn from np.random.default_rng(seed):
    ("sphere", c, r)   ("tri", abc)   ("model", tris [n, 9], add_to_world)
    ("instance", model: its number among the world's models, t, rot, scale)   ("camera", vfov, look_from, look_at)
apply() drives a massrt.Builder or an oracle.Scene with them, write() puts them into a text file for
tools/slab_check (`@file`: the same calls through the C ABI, with the same builder seed: the reference's closest
hit on a 0/0 slab depends on the tree, and the tree on the builder's draws). WORLDS names them with the verdict
nf_tree.cpp must reach: BUILT, or a substring of the nf_note of a scene that keeps the reference walk. Every
world has a dozen ordinary spheres and at most 500 objects.

The |inv translation| <= 2^44 gate (kNfInvShiftMax) has no world: with every world box within 2^28 and
|inv| <= 2^16 the inverse translation is at most 2^28 * 2^16 = 2^44, so it cannot fail while the others hold."""
import numpy as np

import massrt

SEED = 3  # the builders' seed (adversarial_rays.build_both's)
# The short families' directions are the plain ones times 2^k (adversarial_rays.short). A ray starts near first while
# kw1 |d| and ko1 |d| <= 2^-8 and aw0 + aw1 |d| <= 2^-4 (nf_bound.h nf_ray_ok); slab_check's `bound:` line gives
# kw1 2.6e-3 and ko1 4.7e-3 for slivers, kw1 2.5e-3 for near_plane (so |d| <= 0.8 and 1.5 there) and 0 for the
# others, whose `corners` rays are as long as the scene: up to 2^29 in edge_in, which 2^-17 brings within the
# gate's 2^28 too, far above its 2^-50.
SHORT_K = -17
BUILT = None
F = np.float32


def _f(v):
    return np.asarray(v, dtype=np.float32)


def _unit(rng, n=1):
    v = rng.normal(size=(n, 3))
    return _f(v / np.linalg.norm(v, axis=1, keepdims=True))


def _tri(a, ab, ac):
    """a, a + ab, a + ac in float32."""
    a, ab, ac = _f(a), _f(ab), _f(ac)
    return np.concatenate([a, a + ab, a + ac]).astype(np.float32)


def _ordinary_spheres(rng, span=3.0, n=12):
    return [("sphere", _f(rng.uniform(-span, span, 3)), float(F(rng.uniform(0.2, 0.5)))) for _ in range(n)]


# a ground under the small things: a sphere has no generic term, and a family aimed at slivers still hits something
GROUND = ("sphere", _f([0.0, -4100.0, 0.0]), 4096.0)


def _camera(look_from=(0.5, 1.5, 8.0), look_at=(0.0, 0.0, 0.0)):
    return ("camera", 45.0, _f(look_from), _f(look_at))


def _cube():
    """The 12 triangles of [-1, 1]^3 (axis-structured, every one)."""
    t = []
    for k in range(3):
        j, l = (k + 1) % 3, (k + 2) % 3
        for s in (-1.0, 1.0):
            p = np.zeros((4, 3), dtype=np.float32)
            p[:, k] = s
            p[:, j] = [-1, 1, 1, -1]
            p[:, l] = [-1, -1, 1, 1]
            t += [np.concatenate([p[0], p[1], p[2]]), np.concatenate([p[0], p[2], p[3]])]
    return np.array(t, dtype=np.float32)


# ---- in-domain worlds -------------------------------------------------------------------------------
def _sliver_tris(rng, span, counts):
    """Triangles about U(-span, span)^3; counts: (small, needles, slivers, collinear, repeated, ordinary)."""
    out = []
    at = lambda: _f(np.round(rng.uniform(-span, span, 3) * 1024) / 1024)  # multiples of 2^-10: a + e below is exact
    for _ in range(counts[0]):  # edges ~1e-3: |ab x ac| ~ 1e-6, the reference's |det| cut for a unit ray
        out.append(_tri(at(), 1e-3 * _unit(rng)[0], 1e-3 * _unit(rng)[0]))
    for _ in range(counts[1]):  # needles
        out.append(_tri(at(), 0.05 * _unit(rng)[0], 1e-6 * _unit(rng)[0]))
    for _ in range(counts[2]):  # slivers: ac = 2 ab + noise
        ab = 0.03 * _unit(rng)[0]
        out.append(_tri(at(), ab, 2 * ab + _f(1e-7 * rng.normal(size=3))))
    for _ in range(counts[3]):  # collinear, exactly: e a multiple of 2^-16
        e = _f(np.round(0.03 * _unit(rng)[0] * 65536) / 65536)
        out.append(_tri(at(), e, 2 * e))
    for k in range(counts[4]):  # a repeated vertex: (a, a, c), (a, b, b), (a, b, a)
        e1, e2 = 0.03 * _unit(rng)[0], 0.03 * _unit(rng)[0]
        out.append(_tri(at(), *[(0 * e1, e2), (e1, e1), (e1, 0 * e1)][k % 3]))
    for _ in range(counts[5]):  # ordinary, edges 0.01-0.03
        out.append(_tri(at(), rng.uniform(0.01, 0.03) * _unit(rng)[0], rng.uniform(0.01, 0.03) * _unit(rng)[0]))
    return out


def slivers():
    """Small generic triangles (|ab||ac| <= 1.8e-3, so that rays of |d| ~ 1 still pass the kappa gate): edges
    ~1e-3, needles, slivers, collinear and repeated-vertex triangles (zero area: `poisoned` cones), ordinary ones
    of edge 0.01-0.03; in the world and in a BLAS entered as a Model and through three Instances, one mirrored."""
    rng = np.random.default_rng(101)
    ops = _ordinary_spheres(rng) + [GROUND]
    ops += [("tri", t) for t in _sliver_tris(rng, 2.0, (25, 20, 20, 10, 9, 60))]
    ops.append(("model", np.array(_sliver_tris(rng, 1.0, (15, 10, 10, 6, 6, 40))), True))
    ops.append(("instance", 0, _f([2.5, 0.5, -1.0]), _f([0.3, 0.2, 0.1]), _f([0.9, 1.1, 1.0])))
    ops.append(("instance", 0, _f([-2.5, -0.5, 0.5]), _f([0.0, 1.0, 0.4]), _f([1.2, 0.8, 1.0])))
    ops.append(("instance", 0, _f([0.0, 2.0, 1.5]), _f([0.5, 0.0, 0.2]), _f([-1.0, 1.0, 0.9])))  # mirrored
    return ops + [_camera()]


NEAR_PLANE_TINY = (0.0, 1.4e-45, -1.4e-45, 1e-30, -1e-30, 1e-10, -1e-10, 6e-8, -6e-8, 1e-7, -1e-7)


def near_plane():
    """Edges of 0.03. For each axis k: a_k = 0 and ab_k, ac_k from {0, +-1.4e-45 (the smallest subnormal), +-1e-30,
    +-1e-10, +-6e-8, +-1e-7} times the edge (the subnormal as it is), each zero or not independently; a_k ordinary
    and b_k, c_k zero, one or two ulps from it; and triangles exactly on a coordinate plane whose in-plane normal
    nearly cancels, ac = ab (1 + 2^-j) + 0.03 * 2^-m e_l for j, m in 8..21 (tri_bound's `beta < 0.5` and
    `kap > kNfKappaMax` exits to the generic bound)."""
    rng = np.random.default_rng(102)
    ops = _ordinary_spheres(rng) + [GROUND]
    e = F(0.03)

    def in_plane(k):
        a, ab, ac = _f(rng.uniform(-2, 2, 3)), e * _f(rng.uniform(0.5, 1, 3)), e * _f(rng.uniform(0.5, 1, 3))
        ab *= rng.choice(_f([-1, 1]), 3)
        ac[(k + 1) % 3] *= F(-1)  # not parallel: the in-plane normal does not cancel
        return a, ab, ac

    tiny = [F(v) if abs(v) < 1e-40 else F(v) * e for v in NEAR_PLANE_TINY]
    for k in range(3):
        for i, v in enumerate(tiny):
            for vb, vc in ((v, F(0)), (F(0), v), (v, v), (v, tiny[(i + 3) % len(tiny)])):
                a, ab, ac = in_plane(k)
                a[k], ab[k], ac[k] = 0.0, vb, vc
                ops.append(("tri", _tri(a, ab, ac)))
        for sb in range(-2, 3):  # b_k, c_k: sb, sc ulps from a_k
            for sc in range(-2, 3):
                a, ab, ac = in_plane(k)
                t = _tri(a, ab, ac)
                for at, steps in ((3 + k, sb), (6 + k, sc)):
                    t[at] = a[k]
                    for _ in range(abs(steps)):
                        t[at] = np.nextafter(t[at], F(np.inf if steps > 0 else -np.inf))
                ops.append(("tri", t))
    for n, j in enumerate(range(8, 22)):
        for m in (j, 29 - j):
            k = n % 3
            a, ab, ac = in_plane(k)
            ab[k] = ac[k] = 0.0
            ac = ab * F(1 + 2.0 ** -j)
            ac[(k + 2) % 3] += e * F(2.0 ** -m)
            t = _tri(a, ab, ac)
            t[3 + k] = t[6 + k] = a[k]
            ops.append(("tri", t))
    return ops + [_camera()]


def radii():
    """Spheres only (no generic term): radii 2^-59, 2^-56, ... 2^10 about the origin, each centred within three
    radii of it (the s51 / r_min term; no box of theirs is flat, see out_flat), a negative radius, and one of
    radius 2^12 as the ground."""
    rng = np.random.default_rng(103)
    ops = _ordinary_spheres(rng)
    for k in range(-59, 11, 3):
        ops.append(("sphere", _f(2.0 ** k * rng.uniform(-3, 3, 3)), float(2.0 ** k)))
    ops.append(("sphere", _f([1.0, 0.5, 2.0]), -0.4))
    ops.append(GROUND)
    return ops + [_camera((0.5, 3.0, 12.0))]


def big_flat():
    """Axis-structured triangles only, and no generic one (a mix with generic triangles of edge 2^18 sends every
    ray to the reference walk, kw1 |d| > 2^-8, and proves nothing about the near-first one): right-angled
    triangles on coordinate planes with edges 2^0 .. 2^20 about the origin, and ones of edge 2^-10 on planes
    2^20 from it."""
    rng = np.random.default_rng(104)
    ops = _ordinary_spheres(rng)

    def flat(k, plane, at, edge):
        a, ab, ac = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        j, l = (k + 1) % 3, (k + 2) % 3
        a[k], a[j], a[l] = plane, at[0], at[1]
        ab[j], ac[l] = edge * rng.choice([-1.0, 1.0]), edge * rng.choice([-1.0, 1.0])
        t = _tri(a, ab, ac)
        assert t[k] == t[3 + k] == t[6 + k]
        return ("tri", t)

    for n in range(84):
        edge = 2.0 ** (n % 21)
        ops.append(flat(n % 3, rng.uniform(-4, 4) * (1 if n % 21 < 8 else edge / 64), rng.uniform(-4, 4, 2), edge))
    for n in range(36):
        ops.append(flat(n % 3, 2.0 ** 20 * (-1) ** (n // 3), rng.uniform(-2, 2, 2), 2.0 ** -10))
    for n in range(60):  # near the spheres, of edge 0.25 .. 2
        ops.append(flat(n % 3, rng.uniform(-3, 3), rng.uniform(-3, 3, 2), 2.0 ** (n % 4 - 2)))
    return ops + [_camera()]


INSTANCES_WILD = 2  # the (1.6e-5, 2, 2) scale and the slab: an instance is wild once gamma_3 |F||G| > 2^-14,
#                     |F||G| > 341 (nf_tree.cpp inst_term, wild); theirs are 1.8e5 and 1.4e6, the others' < 20


def instances():
    """The cube under 20 random transforms (negative scales among them), a rotation of exactly pi (matrix
    entries of ~1e-8 and ~1e-16), the scale (1.6e-5, 2, 2) (|inv| = 6.25e4: just inside 2^16), a 1000 x 0.001 x
    1000 slab, and a translation of 2^20."""
    rng = np.random.default_rng(105)
    ops = _ordinary_spheres(rng)
    ops.append(("model", _cube(), False))
    for _ in range(20):
        s = rng.uniform(0.3, 2.0, 3) * rng.choice([-1.0, 1.0], 3, p=[0.3, 0.7])
        ops.append(("instance", 0, _f(rng.normal(size=3) * 3), _f(rng.normal(size=3)), _f(s)))
    ops.append(("instance", 0, _f([1.0, 0.5, -2.0]), _f([np.pi, 0.0, 0.0]), _f([0.7, 0.7, 0.7])))
    ops.append(("instance", 0, _f([-1.0, 1.0, 2.0]), _f([0.0, np.pi, np.pi]), _f([0.5, 0.6, 0.7])))
    ops.append(("instance", 0, _f([2.0, -1.0, 1.0]), _f([0.2, 0.1, 0.0]), _f([1.6e-5, 2.0, 2.0])))
    ops.append(("instance", 0, _f([0.0, -3.0, 0.0]), _f([0.0, 0.0, 0.0]), _f([1000.0, 0.001, 1000.0])))
    ops.append(("instance", 0, _f([2.0 ** 20, 0.0, 0.0]), _f([0.1, 0.2, 0.3]), _f([1.0, 1.0, 1.0])))
    return ops + [_camera()]


# ---- the gates' edges: one world inside every gate, and twins of it with one number changed ------------
EDGE_FACE_IN = float(2.0 ** 28 * (1 - 2.0 ** -16))


def _edge(big_sphere=((2.0 ** 27, 0.0, 0.0), 2.0 ** 26), thin_scale=1.6e-5, far_vertex=4000.0, small_r=2.0 ** -60,
          small_c=(0.0, 0.0, 0.0), face=EDGE_FACE_IN):
    rng = np.random.default_rng(106)
    ops = _ordinary_spheres(rng)
    for n in range(72):  # enough ordinary boxes that few rays start at the far ones' corners
        k = n % 3
        a, ab, ac = _f(rng.uniform(-3, 3, 3)), np.zeros(3, np.float32), np.zeros(3, np.float32)
        ab[(k + 1) % 3], ac[(k + 2) % 3] = rng.uniform(0.3, 1.0), rng.uniform(0.3, 1.0)
        ops.append(("tri", _tri(a, ab, ac)))
    ops.append(("sphere", _f(big_sphere[0]), float(F(big_sphere[1]))))
    ops.append(("tri", _f([face, 0, 0, face, 1, 0, face, 0, 1])))  # a box face at `face`
    ops.append(("sphere", _f(small_c), float(small_r)))
    ops.append(("model", _cube(), False))
    ops.append(("instance", 0, _f([2.0, -1.0, 1.0]), _f([0.2, 0.1, 0.0]), _f([thin_scale, 2.0, 2.0])))
    far = _f([[0, 0, 0, far_vertex, 0, 0, 0, 0, 1], [0, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, far_vertex, 0, 0, 0, 1, 0]])
    ops.append(("model", far, False))
    ops.append(("instance", 1, _f([-2.0, 0.0, 0.0]), _f([0.0, 0.3, 0.0]), _f([1e-3, 1e-3, 1e-3])))
    return ops + [_camera()]


def edge_in():
    """Just inside every gate: a sphere at (2^27, 0, 0) of radius 2^26, a box face at 2^28 (1 - 2^-16), the
    instance scale (1.6e-5, 2, 2), a mesh with a vertex 4000 from its origin instanced at scale 1e-3, a sphere
    of radius exactly 2^-60, at the origin, where its box is not flat (out_flat). (A face at exactly 2^28 is
    out_face: the gate looks at the padded box.)"""
    return _edge()


def out_box():
    return _edge(big_sphere=((2.0 ** 28, 0.0, 0.0), 1.0))


def out_inf():
    """The sphere's box overflows to infinity."""
    return _edge(big_sphere=((3e38, 0.0, 0.0), 3e38))


def out_face():
    """A triangle's face at exactly 2^28: its near-first box is padded outward (nf_tree.cpp pad_box), past 2^28."""
    return _edge(face=2.0 ** 28)


def out_inst():
    return _edge(thin_scale=1e-5)


def out_mesh():
    return _edge(far_vertex=4200.0)


def out_small():
    return _edge(small_r=2.0 ** -61)


def out_zero():
    return _edge(small_r=0.0)


def out_flat():
    """The sphere of radius 2^-60 away from the origin, alone in its node of the reference's tree: the node's box
    is the point (0.5, 0.25, 1). A ray through it with d_y = 0 and o_y = 0.25 has 0/0 on both y planes of that
    box, which min/max pass over, and hits the sphere; the boxes above with y_min = 0.25 have 0/0 and an
    infinity there and are missed by the reference, which never reaches the sphere. The near-first walk checks
    the winner's parent box only (walk_nf.h nf_finish) and returned the sphere on 31 + 2 + 13 rays of the `axis`,
    `on_plane` and `spheres` families before nf_tree.cpp declined such scenes."""
    return _edge(small_c=(0.5, 0.25, 1.0))


NOTE_BOX, NOTE_INST = "a world box outside", "an instance transform outside"
NOTE_MESH, NOTE_SMALL, NOTE_FLAT = "an instanced mesh outside", "a sphere too small", "a sphere in a flat reference box"
WORLDS = {
    "slivers": (slivers, BUILT), "near_plane": (near_plane, BUILT), "radii": (radii, BUILT),
    "big_flat": (big_flat, BUILT), "instances": (instances, BUILT), "edge_in": (edge_in, BUILT),
    "out_box": (out_box, NOTE_BOX), "out_inf": (out_inf, NOTE_BOX), "out_face": (out_face, NOTE_BOX),
    "out_inst": (out_inst, NOTE_INST), "out_mesh": (out_mesh, NOTE_MESH), "out_small": (out_small, NOTE_SMALL),
    "out_zero": (out_zero, NOTE_SMALL), "out_flat": (out_flat, NOTE_FLAT),
}
IN_DOMAIN = [name for name, (_, verdict) in WORLDS.items() if verdict is BUILT]
OUT_OF_DOMAIN = [name for name in WORLDS if name not in IN_DOMAIN]


# ---- the ops' two consumers ----------------------------------------------------------------------------------
def apply(x, ops):
    """Drives x, a massrt.Builder or an oracle.Scene, with the ops; the tree is built after the last of them."""
    x.background(massrt.BG_SKY)
    mat = x.material(massrt.MAT_LAMBERTIAN, x.solid(0.5, 0.5, 0.5))
    models, camera = [], None
    for op in ops:
        if op[0] == "sphere":
            x.add_sphere(mat, op[1], op[2])
        elif op[0] == "tri":
            x.add_triangle(mat, op[1])
        elif op[0] == "model":
            models.append(x.model(mat, op[1], add_to_world=op[2]))
        elif op[0] == "instance":
            x.add_instance(models[op[1]], op[2], op[3], op[4])
        elif op[0] == "camera":
            camera = op
        else:
            raise ValueError(op[0])
    x.build_bvh()
    x.camera(camera[1], camera[2], camera[3], aspect=float(massrt.ASPECT_RATIO))
    return x


def build_both(name):
    import oracle
    ops = WORLDS[name][0]()
    return apply(massrt.Builder(SEED), ops), apply(oracle.Scene(SEED), ops)


def write(path, ops, seed=SEED):
    """The ops as tools/slab_check reads them (its load_world): words and C hex floats."""
    hexf = lambda v: " ".join(float(F(x)).hex() for x in np.asarray(v, dtype=np.float32).reshape(-1))
    lines = [f"seed {seed}"]
    for op in ops:
        if op[0] == "model":
            lines.append(f"model {int(op[2])} {len(op[1])}")
            lines += [hexf(t) for t in op[1]]
        elif op[0] == "instance":
            lines.append(f"instance {op[1]} {hexf(op[2])} {hexf(op[3])} {hexf(op[4])}")
        elif op[0] == "camera":
            lines.append(f"camera {hexf([op[1]])} {hexf(op[2])} {hexf(op[3])}")
        else:
            lines.append(f"{op[0]} {hexf(op[1])}" + (f" {hexf([op[2]])}" if op[0] == "sphere" else ""))
    path.write_text("\n".join(lines) + "\n")
    return path
