"""Adversarial ray families, as data: deterministic numpy generators shared by
the host-walk tests (tests/test_layout.py) and the GPU tests
(tests/test_gpu_adversarial.py), beside ray_gen.py's ordinary rays.

families(desc, cam) takes the scene's own geometry (Builder.desc(): node
boxes, spheres, triangles, instances, the camera) and returns name -> [n, 6]
float32 rays (origin, direction). Every family is a place where a closest-hit
walk can go wrong without ordinary rays noticing: zero and subnormal direction
components, origins on box planes (0/0 in the slab test), rays through box
corners and along shared triangle edges, directions of 2^-120 to 2^100,
origins up to 1e38 from the scene (where the reference's own sphere arithmetic
overflows and accepts a hit with t = NaN), NaN and infinite values, rays
grazing a triangle's plane and passing a sphere at nearly its radius. short()
gives every family again with directions of 2^k.

The custom worlds the GPU tests walk (random_world is tests/test_bvh.py's) are
built here too, so that their rays come from the same desc() the walk sees."""
import ctypes as C

import numpy as np

import massrt
from ray_gen import camera_rays

N_FAMILY = 2000  # rays per family (the last block of a family is cut to fit)
SCALE_K = (-120, -60, -51, -50, -49, -30, -12, 12, 30, 60, 100)  # -51..-49: around the gate's d2 >= 2^-100
TINY = (1e-40, -1e-40, 1.4e-45, 1e-30, -1e-25)
FAR_BIG_K = tuple(range(3, 20))
FAR_UNIT_K = (3, 6, 9, 12, 19, 20, 25, 30, 38)


# ---- the scene's geometry, in world space ----------------------------------------
def _table(ptr, n, struct):
    """A desc array as [n, words] uint32 (a copy)."""
    words = C.sizeof(struct) // 4
    if n == 0:
        return np.zeros((0, words), dtype=np.uint32)
    raw = (C.c_uint32 * (n * words)).from_address(C.addressof(ptr.contents))
    return np.frombuffer(raw, dtype=np.uint32).reshape(n, words).copy()


def _subtree(nodes, root):
    """Node ids and leaf refs below node ref `root`."""
    ids, leaves, stack = [], [], [int(root)]
    while stack:
        r = stack.pop()
        k, i = r >> 28, r & 0x0FFFFFFF
        if k == massrt.REF_NODE:
            ids.append(i)
            stack += [int(nodes[i, 6]), int(nodes[i, 7])]
        elif k != massrt.REF_NONE:
            leaves.append((k, i))
    return ids, leaves


def _xform(fwd, p):
    """Points p [n, 3] through a column-major 4x4 (in double, rounded once)."""
    m = fwd.astype(np.float64).reshape(4, 4).T  # m[r, c]
    return (p.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32)


def _corners(box):
    b = np.asarray(box, dtype=np.float32).reshape(-1, 6)
    pick = np.array([[(c >> k) & 1 for k in range(3)] for c in range(8)])  # 0: min, 1: max
    return np.where(pick[None, :, :] == 1, b[:, None, 3:], b[:, None, :3])  # [n, 8, 3]


def geometry(desc, cam):
    """World-space geometry of a built scene: `boxes` [n, 6] (the world tree's
    and the models' node boxes, and each instance's BLAS boxes as the hull of
    their transformed corners), `spheres` [n, 4] (centre, |radius|), `tris`
    [n, 9] (instanced triangles through the instance's forward matrix), `cam`
    (the camera), `centre` (the median primitive position: where rays aim)."""
    nodes = _table(desc.nodes, desc.n_nodes, massrt.MrtNode)
    sph = _table(desc.spheres, desc.n_spheres, massrt.MrtSphere)
    tri = _table(desc.triangles, desc.n_triangles, massrt.MrtTriangle)[:, :9].copy().view(np.float32)
    inst = _table(desc.instances, desc.n_instances, massrt.MrtInstance)
    model = _table(desc.models, desc.n_models, massrt.MrtModel)
    node_box = nodes[:, :6].copy().view(np.float32)
    boxes, tris, spheres = [], [], []
    blas = {}  # blas root -> (node ids, triangle ids)

    def blas_of(root):
        if root not in blas:
            ids, leaves = _subtree(nodes, (massrt.REF_NODE << 28) | root)
            blas[root] = (ids, [i for k, i in leaves if k == massrt.REF_TRIANGLE])
        return blas[root]

    for r in range(desc.n_roots):
        ids, leaves = _subtree(nodes, desc.roots[r])
        boxes.append(node_box[ids])
        for k, i in leaves:
            if k == massrt.REF_SPHERE:
                spheres.append(i)
            elif k == massrt.REF_TRIANGLE:
                tris.append(tri[i:i + 1])
            elif k == massrt.REF_MODEL:
                nid, tid = blas_of(int(model[i, 0]))
                boxes.append(node_box[nid])
                tris.append(tri[tid])
            elif k == massrt.REF_INSTANCE:
                fwd = inst[i, :16].copy().view(np.float32)
                nid, tid = blas_of(int(inst[i, 32]))
                c = _xform(fwd, _corners(node_box[nid]).reshape(-1, 3)).reshape(-1, 8, 3)
                boxes.append(np.concatenate([c.min(1), c.max(1)], 1))
                tris.append(_xform(fwd, tri[tid].reshape(-1, 3)).reshape(-1, 9))
    boxes = np.concatenate(boxes) if boxes else np.zeros((0, 6), np.float32)
    boxes = boxes[np.isfinite(boxes).all(1)]
    tris = np.concatenate(tris) if tris else np.zeros((0, 9), np.float32)
    s = sph[spheres, :4].copy().view(np.float32) if spheres else np.zeros((0, 4), np.float32)
    s[:, 3] = np.abs(s[:, 3])
    pts = np.concatenate([tris.reshape(-1, 3), s[:, :3]])
    centre = np.median(pts, 0).astype(np.float32) if len(pts) else np.zeros(3, np.float32)
    return {"boxes": boxes, "spheres": s, "tris": tris, "cam": cam, "centre": centre}


# ---- building blocks ---------------------------------------------------------------
def _rays(o, d):
    o = np.broadcast_to(np.asarray(o, dtype=np.float32), np.asarray(d).shape)
    return np.concatenate([o, np.asarray(d, dtype=np.float32)], 1).astype(np.float32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _targets(g, n, rng):
    """n points on the scene's primitives: sphere centres and points inside triangles."""
    out = []
    if len(g["tris"]):
        t = g["tris"][rng.integers(0, len(g["tris"]), n)]
        u, v = rng.random((n, 1), dtype=np.float32), rng.random((n, 1), dtype=np.float32)
        flip = (u + v) > 1
        u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
        out.append(t[:, 0:3] + u * (t[:, 3:6] - t[:, 0:3]) + v * (t[:, 6:9] - t[:, 0:3]))
    if len(g["spheres"]):
        out.append(g["spheres"][rng.integers(0, len(g["spheres"]), n), :3])
    p = np.concatenate(out)
    return p[rng.permutation(len(p))[:n]].astype(np.float32)


def _origins(g, n, rng, span=6.0):
    return (g["centre"] + rng.uniform(-span, span, (n, 3))).astype(np.float32)


def ordinary(g, n, seed):
    """Ordinary rays: half from the camera into its frustum, half from random
    origins about the scene aimed at its primitives."""
    rng = np.random.default_rng(seed)
    a = camera_rays(g["cam"], n // 2, seed + 1)
    o = _origins(g, n - n // 2, rng)
    return np.concatenate([a, _rays(o, _targets(g, n - n // 2, rng) - o)])


def _along_axes(g, n, rng, fill):
    """Rays through a primitive point p whose direction has one or two
    components replaced by fill(count): the origin lies back along the
    components that are kept, so the ray still passes (nearly) through p."""
    p = _targets(g, n, rng)
    d = rng.uniform(0.5, 2.0, (n, 3)).astype(np.float32) * rng.choice(np.float32([-1, 1]), (n, 3))
    replaced = np.zeros((n, 3), dtype=bool)
    replaced[np.arange(n), rng.integers(0, 3, n)] = True
    two = rng.random(n) < 0.5
    replaced[np.arange(n)[two], rng.integers(0, 3, n)[two]] = True  # the same axis again: still one
    kept = np.where(replaced, np.float32(0), d)
    back = rng.uniform(0.5, 8.0, (n, 1)).astype(np.float32)
    o = (p - kept * back).astype(np.float32)
    d = np.where(replaced, fill((n, 3)), d).astype(np.float32)
    return _rays(o, d)


def blocks(values, n):
    """The value of each of n rays of a family laid out in equal blocks, one per value."""
    return np.repeat(np.asarray(values), -(-n // len(values)))[:n]


# ---- the families ------------------------------------------------------------------
def axis(g, n, seed):
    rng = np.random.default_rng(seed)
    return _along_axes(g, n, rng, lambda shape: rng.choice(np.float32([0.0, -0.0]), shape))


def tiny_comp(g, n, seed):
    rng = np.random.default_rng(seed)
    return _along_axes(g, n, rng, lambda shape: rng.choice(np.float32(TINY), shape))


def on_plane(g, n, seed):
    """Origin component k on a plane of a node box and direction component k
    zero: the slab test's (plane - o) / d is 0/0 there. The ray runs in that
    plane through a point of the box's face."""
    rng = np.random.default_rng(seed)
    b = g["boxes"][rng.integers(0, len(g["boxes"]), n)]
    k = rng.integers(0, 3, n)
    rows = np.arange(n)
    face = (b[:, :3] + rng.random((n, 3), dtype=np.float32) * (b[:, 3:] - b[:, :3])).astype(np.float32)
    plane = np.where(rng.random(n) < 0.5, b[rows, k], b[rows, 3 + k])
    d = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    d[rows, k] = rng.choice(np.float32([0.0, -0.0]), n)
    o = (face - d * rng.uniform(0.0, 6.0, (n, 1)).astype(np.float32)).astype(np.float32)
    o[rows, k] = plane
    return _rays(o, d)


def corners(g, n, seed):
    rng = np.random.default_rng(seed)
    c = _corners(g["boxes"])
    i, j = rng.integers(0, len(c), n), rng.integers(0, len(c), n)
    a, b = c[i, rng.integers(0, 8, n)], c[j, rng.integers(0, 8, n)]
    down = (a[:, 1] < b[:, 1])[:, None]  # from the higher corner: towards the ground, where the scenes have one
    a, b = np.where(down, b, a), np.where(down, a, b)
    return _rays(a, b - a)


def tri_edges(g, n, seed):
    """At triangle vertices and at points 0.25 and 0.5 along edges (shared by
    the neighbouring triangle in a mesh), from the camera and from random origins."""
    rng = np.random.default_rng(seed)
    t = g["tris"][rng.integers(0, len(g["tris"]), n)].reshape(n, 3, 3)
    e = rng.integers(0, 3, n)
    a, b = t[np.arange(n), e], t[np.arange(n), (e + 1) % 3]
    f = rng.choice(np.float32([0.0, 0.25, 0.5]), (n, 1))
    p = (a + f * (b - a)).astype(np.float32)
    o = _origins(g, n, rng)
    o[: n // 2] = g["cam"].fields()[0:3]
    return _rays(o, p - o)


def spheres(g, n, seed):
    """Aimed at a sphere's centre; from the centre; tangent at the top point
    (y = centre_y + r, d.y = 0)."""
    rng = np.random.default_rng(seed)
    s = g["spheres"][rng.integers(0, len(g["spheres"]), n)]
    c, r = s[:, :3], s[:, 3:4]
    m = n // 3
    o = _origins(g, n, rng)
    d = (c - o).astype(np.float32)
    o[m:2 * m] = c[m:2 * m]
    d[m:2 * m] = rng.normal(size=(m, 3))
    flat = rng.normal(size=(n - 2 * m, 3)).astype(np.float32)
    flat[:, 1] = 0.0
    top = c[2 * m:] + np.concatenate([np.zeros_like(r), r, np.zeros_like(r)], 1)[2 * m:]
    o[2 * m:] = top - flat * rng.uniform(0.5, 4.0, (n - 2 * m, 1)).astype(np.float32)
    o[2 * m:, 1] = top[:, 1]
    d[2 * m:] = flat
    return _rays(o, d)


def scales(g, n, seed):
    r = ordinary(g, n, seed)
    with np.errstate(over="ignore", under="ignore"):
        r[:, 3:] = r[:, 3:] * np.ldexp(np.float32(1), blocks(SCALE_K, n))[:, None].astype(np.float32)
    return r


def _far(g, n, seed, ks):
    rng = np.random.default_rng(seed)
    k = blocks(ks, n)
    o = (g["centre"].astype(np.float64) + _unit(rng, n) * (10.0 ** k)[:, None]).astype(np.float32)
    target = (g["centre"] + rng.uniform(-3.0, 3.0, (n, 3))).astype(np.float32)
    return o, target


def far_big_d(g, n, seed):
    """Origin 10^k from the scene, k = blocks(FAR_BIG_K, n), d = target - origin in float32."""
    o, target = _far(g, n, seed, FAR_BIG_K)
    return _rays(o, target - o)


def far_unit_d(g, n, seed):
    """The same kind of origin, k = blocks(FAR_UNIT_K, n), with a unit direction towards the target."""
    o, target = _far(g, n, seed, FAR_UNIT_K)
    d = target.astype(np.float64) - o.astype(np.float64)
    return _rays(o, d / np.linalg.norm(d, axis=1, keepdims=True))


def _one_slot(g, n, seed, lo, hi, values):
    rng = np.random.default_rng(seed)
    r = ordinary(g, n, seed + 100)
    r[np.arange(n), lo + np.arange(n) % (hi - lo)] = rng.choice(np.float32(values), n)
    return r


def nan_origin(g, n, seed):
    """NaN in origin slot i % 3 of ray i."""
    return _one_slot(g, n, seed, 0, 3, [np.nan])


def nan_direction(g, n, seed):
    return _one_slot(g, n, seed, 3, 6, [np.nan])


def inf(g, n, seed):
    return _one_slot(g, n, seed, 0, 6, [np.inf, -np.inf])


def zero_d(g, n, seed):
    r = ordinary(g, n, seed)
    r[:, 3:] = np.random.default_rng(seed).choice(np.float32([0.0, -0.0]), (n, 3))
    return r


def _perpendicular(w):
    """Unit vectors perpendicular to the unit vectors w [n, 3] (float64)."""
    e = np.where((np.abs(w[:, 0]) < 0.9)[:, None], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    t = np.cross(w, e)
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def graze(g, n, seed):
    """Through a random point of a triangle (one with a normal) at 10^U(-8, -1.5) rad to its plane, either
    side, the origin 0.5-20 back along the ray; |d| in 0.5-2. Where Moller-Trumbore's t is least accurate and
    the reference's |det| >= 1e-6 cut decides (tools/slab_check.cpp `graze`, here from the scene's world-space
    triangles). Computed in float64 and rounded once."""
    return graze_with_triangles(g, n, seed)[0]


def graze_with_triangles(g, n, seed):
    """graze()'s rays and each ray's triangle [n, 3, 3] (float64)."""
    rng = np.random.default_rng(seed)
    t = g["tris"].astype(np.float64).reshape(-1, 3, 3)
    nn = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ln = np.linalg.norm(nn, axis=1)
    ok = np.flatnonzero(ln > 0)
    i = ok[rng.integers(0, len(ok), n)]
    t, nn = t[i], nn[i] / ln[i, None]
    b1, b2 = rng.random((n, 1)), rng.random((n, 1))
    flip = (b1 + b2) > 1
    b1, b2 = np.where(flip, 1 - b1, b1), np.where(flip, 1 - b2, b2)
    p = t[:, 0] + b1 * (t[:, 1] - t[:, 0]) + b2 * (t[:, 2] - t[:, 0])
    t1 = _perpendicular(nn)
    t2 = np.cross(nn, t1)
    phi = rng.uniform(0.0, 2.0 * np.pi, (n, 1))
    th = 10.0 ** rng.uniform(-8.0, -1.5, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    d = rng.uniform(0.5, 2.0, (n, 1)) * (np.cos(th) * (np.cos(phi) * t1 + np.sin(phi) * t2) + np.sin(th) * nn)
    back = rng.uniform(0.5, 20.0, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    return _rays((p - d * back).astype(np.float32), d), t


def family_seed(f, seed=1):
    """The seed families() passes to family f."""
    return seed + 1000 * FAMILIES.index(f)


def tangent(g, n, seed):
    """Past a sphere at r (1 +- 10^U(-7, -1)) from its centre, from 1-400 radii before the nearest point;
    |d| in 0.5-2. Where the sphere test's discriminant cancels (tools/slab_check.cpp `tangent`). Half pass
    outside. Computed in float64 and rounded once."""
    rng = np.random.default_rng(seed)
    s = g["spheres"][rng.integers(0, len(g["spheres"]), n)].astype(np.float64)
    c, r = s[:, :3], s[:, 3:4]
    w = _unit(rng, n)
    off = r * (1.0 + rng.choice([-1.0, 1.0], (n, 1)) * 10.0 ** rng.uniform(-7.0, -1.0, (n, 1)))
    t1 = _perpendicular(w)
    back = r * 10.0 ** rng.uniform(0.0, 2.6, (n, 1))
    d = t1 * rng.uniform(0.5, 2.0, (n, 1))
    return _rays((c + w * off - t1 * back).astype(np.float32), d)


FAMILIES = (axis, on_plane, corners, tri_edges, spheres, scales, tiny_comp, far_big_d, far_unit_d, nan_origin,
            nan_direction, inf, zero_d, graze, tangent)
# the families aimed at the scene's own boxes and primitives with finite, ordinary-sized values
GEOMETRIC = ("axis", "on_plane", "corners", "tri_edges", "spheres", "tiny_comp", "graze", "tangent")


def families(desc, cam, n=N_FAMILY, seed=1):
    """name -> [n, 6] float32 rays, from the scene's own geometry. A family
    whose primitives the scene lacks (spheres, tangent; tri_edges, graze) is left out."""
    g = geometry(desc, cam)
    out = {}
    for k, f in enumerate(FAMILIES):
        if (f in (spheres, tangent) and not len(g["spheres"])) or (f in (tri_edges, graze) and not len(g["tris"])):
            continue
        r = f(g, n, seed + 1000 * k)
        assert r.shape == (n, 6) and r.dtype == np.float32, f.__name__
        out[f.__name__] = r
    return out


def short(name_rays: dict, k: int):
    """Every family again as `family/short`: the same origins, directions times 2^k. With generic triangles in
    the scene a ray walks near first only while kw1 |d| <= 2^-8 (nf_bound.h nf_ray_ok), which |d| ~ 1 fails
    once some |ab||ac| reaches ~3e-3: the short rays are the ones that take the near-first walk there."""
    out = {}
    for name, r in name_rays.items():
        s = r.copy()
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            s[:, 3:] = np.ldexp(r[:, 3:], k)
        out[f"{name}/short"] = s
    return out


def split(name_rays: dict):
    """The families as one array and (name, begin, end) offsets into it."""
    at, parts = 0, []
    for name, r in name_rays.items():
        parts.append((name, at, at + len(r)))
        at += len(r)
    return np.concatenate(list(name_rays.values())), parts


# ---- what a family must contain to prove anything (on the oracle's answer alone) --------
# Floors well under the measured shares (DESIGN.md §4 lists those): a family
# that hits nothing would pass any comparison.
# corners: 48.3% on cube_field and 48.5% on sphere_grid with these generators (many leaf boxes stand on the
# ground plane, and a ray between two such corners runs in it), so its floor is half of that.
# graze: 95.5 / 66.5 / 99.5% on cornell / sphere_grid / cube_field and 71.2% or more on adversarial_worlds.py's
# worlds; tangent (half of its rays pass outside their sphere by construction, and may hit something else):
# 99.5 / 99.3 / 57.0% and 69.0% or more. Each floor is half of the smallest share.
HIT_FLOOR = {"nan_origin": 0.25, "tri_edges": 0.5, "spheres": 0.5, "corners": 0.25, "axis": 0.2, "on_plane": 0.2,
             "tiny_comp": 0.2, "graze": 0.33, "tangent": 0.28}


def is_nan_t(hits):
    return (hits[:, 0] != 0) & ((hits[:, 2] & 0x7FFFFFFF) > 0x7F800000)


def check_floors(want: dict, overflow: bool):
    """The oracle's own answers `want` (name -> [n, 4]) hold enough hits per
    family; overflow: the scene is one whose spheres make far_big_d's inf - inf
    discriminant a hit with t = NaN on many rays (cornell, sphere_grid)."""
    for name, floor in HIT_FLOOR.items():
        if name in want:
            share = float((want[name][:, 0] != 0).mean())
            assert share >= floor, f"{name}: the oracle hits {share:.1%} of the rays, under {floor:.0%}"
    for name in GEOMETRIC:  # short(): the same rays with t_min = 0.001 so much nearer the origin
        if f"{name}/short" in want:
            share = float((want[f"{name}/short"][:, 0] != 0).mean())
            assert share >= 0.2, f"{name}/short: the oracle hits {share:.1%} of the rays, under 20%"
    n = len(want["far_unit_d"])
    far = blocks(FAR_UNIT_K, n) >= 20
    share = float((want["far_unit_d"][far, 0] != 0).mean())
    assert share >= 0.15, f"far_unit_d, k >= 20: the oracle hits {share:.1%}, under 15%"
    if overflow:
        big = blocks(FAR_BIG_K, len(want["far_big_d"])) >= 10
        share = float(is_nan_t(want["far_big_d"][big]).mean())
        assert share >= 0.10, f"far_big_d, k >= 10: the oracle's t is NaN on {share:.1%}, under 10%"


def first_difference(name, rays, got, want):
    """None, or the assertion text: the family, how many rays differ, the first with both answers."""
    bad = np.flatnonzero((got != want).any(1))
    if not len(bad):
        return None
    i = int(bad[0])
    fmt = lambda h: " ".join(f"{int(x):08x}" for x in h)
    return (f"{name}: {len(bad)} of {len(rays)} rays differ; first, ray {i} = {rays[i].tolist()} "
            f"(bits {fmt(rays[i].view(np.uint32))}): got {fmt(got[i])}, the oracle {fmt(want[i])}")


# ---- the custom worlds of the GPU tests ------------------------------------------------
def build_both(fn, seed=3):
    import oracle
    b, o = massrt.Builder(seed), oracle.Scene(seed)
    fn(b)
    fn(o)
    return b, o


def wild_world(x, golden_dir, aspect):
    """Thin slabs scaled 1:3000 (wild instances, nf_tree.cpp wild()) crossing
    each other, non-wild cubes and spheres. x: massrt.Builder or oracle.Scene."""
    x.background(massrt.BG_SKY)
    lam = x.material(massrt.MAT_LAMBERTIAN, x.solid(0.6, 0.5, 0.4))
    glow = x.material(massrt.MAT_DIFFUSE_LIGHT, 0, 0.0, (4.0, 4.0, 4.0))
    cube = x.model_from_ply(golden_dir / "cube.ply", lam)
    for k in range(6):  # wild: 12 x 0.004 x 9
        x.add_instance(cube, (0.7 * k - 2.0, 0.3 * k - 0.6, -0.5 * k), (0.1 * k, 0.05, 0.02 * k), (12.0, 0.004, 9.0),
                       glow if k % 2 else massrt.NO_MATERIAL)
    for k in range(5):  # ordinary
        x.add_instance(cube, (1.1 * k - 2.0, 0.2, 1.0 - 0.4 * k), (0.0, 0.13 * k, 0.0), (0.4, 0.4, 0.4))
    for k in range(4):
        x.add_sphere(x.material(massrt.MAT_METAL, x.solid(0.8, 0.8, 0.8), 0.1), (k - 1.5, -0.2, 0.3 * k), 0.35)
    x.build_bvh()
    x.camera(45.0, (0.5, 1.5, 7), (0, 0, 0), aspect=aspect)


def alpha_plane(rng):
    """A texture with holes in its alpha and an 8 x 8 grid of quads (128 triangles with normals and uvs) over it."""
    tex = rng.integers(0, 256, size=(16, 24, 4), dtype=np.uint8)
    tex[..., 3] = np.where(rng.random((16, 24)) < 0.3, 0, 255)
    grid = np.linspace(-2, 2, 9, dtype=np.float32)
    tris = []
    for i in range(8):
        for j in range(8):
            x0, x1, y0, y1 = grid[i], grid[i + 1], grid[j], grid[j + 1]
            for tri in ([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0]], [[x0, y0, 0], [x1, y1, 0], [x0, y1, 0]]):
                row = []
                for v in tri:
                    row += list(v) + [0, 0, 1] + [v[0] * 0.3 + 0.5, v[1] * 0.3 + 0.5]
                tris.append(row)
    return tex, np.array(tris, dtype=np.float32)


def alpha_world(x, variant, aspect):
    """Alpha-tested triangles in a BLAS entered through a Model and/or an
    Instance (variant: model, instance, both), and a glass sphere."""
    tex, tris = alpha_plane(np.random.default_rng(7))
    st = x.texture_rgba(tex, massrt.WRAP_REPEAT)
    x.background(massrt.BG_SKY)
    mt = x.material(massrt.MAT_LAMBERTIAN, st)
    m = x.model(mt, tris, add_to_world=variant in ("model", "both"), shading=True)
    if variant in ("instance", "both"):
        x.add_instance(m, (0.5, 0.2, -1.5), (0.1, 0.2, 0.05), (1.2, 0.8, 1.0), x.material(massrt.MAT_METAL, st, 0.3))
    x.add_sphere(x.material(massrt.MAT_DIELECTRIC, 0, 1.4), (0.3, 0.1, 1.0), 0.5)
    x.build_bvh()
    x.camera(45.0, (0.5, 0.8, 6), (0, 0, 0), aspect=aspect)
