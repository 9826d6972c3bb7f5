"""Per-hit shading parity: the device's shading probe (Context.shade_rays,
k_shade_rays<RNG, EXT>) against the oracle's one-step entry
(oracle.Scene.shade_rays) on the cases of tests/shade_cases.py — every field
of every record bit for bit: the hit, point, normal, uv, material, emission,
attenuation and the scattered direction.

The one exception is the attenuation of a YCbCr surface, whose powf(., 2.2)
is ocml's on the device and glibc's in the oracle: within rtol 1e-5 / atol
1e-6 there, the bound test_composite_surfaces_and_cubemap_parity holds the
same quantity to (largest distance seen on the MI355X: 1 ULP).

Backgrounds are not in a probe record (a miss is zeros), so they are compared
through 1-spp renders of depth 1, whose radiance is the background's value.
"""
import numpy as np
import pytest

import massrt
import oracle
import shade_cases as sc

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def refs():
    """name -> (case, builder, rays, oracle records): the oracle's side, computed once for both walks."""
    out = {}
    for name, case in sc.CASES.items():
        b, o = massrt.Builder(3), oracle.Scene(3)
        case(b)
        case(o)
        rays, _where = sc.all_rays(case.info)
        out[name] = (case, b, rays, o.shade_rays(rays, seed=sc.SEED))
    return out


def words(rec, field):
    return np.ascontiguousarray(rec[field]).view(np.uint32).reshape(rec.shape[0], -1)


def ulp_distance(a, b):
    """Between non-negative floats: the difference of their bit patterns."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def assert_records_equal(case, got, ref):
    info = case.info
    hit = ref["prim"] != 0
    kind = np.where(hit, info.kinds[np.where(hit, ref["material"], 0)], 0)
    ycbcr = hit & np.isin(ref["material"], info.ycbcr_mats)
    problems = []
    for field in massrt.SHADE_DTYPE.names:
        differ = (words(got, field) != words(ref, field)).any(1)
        if field == "attenuation":
            differ &= ~ycbcr
        if differ.any():
            i = int(np.flatnonzero(differ)[0])
            what = sc.KIND_NAMES[kind[i]] if hit[i] else "miss"
            problems.append(f"{field}: {int(differ.sum())} rays differ, first ray {i} ({what}): "
                            f"device {got[field][i]} oracle {ref[field][i]}")
    assert not problems, "\n".join(problems)
    if ycbcr.any():
        a, b = got["attenuation"][ycbcr], ref["attenuation"][ycbcr]
        print(f"{case.name}: YCbCr attenuation on {int(ycbcr.sum())} hits, largest distance "
              f"{int(ulp_distance(a, b).max())} ULP, {int((ulp_distance(a, b) != 0).sum())} components differ")
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6)


def assert_floors(case, rays, rec):
    got, want = sc.coverage(case.info, rays, rec), sc.floors(case)
    short = {k: (got[k], v) for k, v in want.items() if got[k] < v}
    assert not short, short


@pytest.mark.parametrize("name", list(sc.CASES))
def test_shading_is_the_oracles_bit_for_bit(ctx, refs, name):
    case, b, rays, ref = refs[name]
    ctx.upload(b)
    got = ctx.shade_rays(rays, seed=sc.SEED)
    assert_floors(case, rays, got)  # a device that loses hits does not pass on an empty set
    assert_records_equal(case, got, ref)


def test_probe_sits_behind_either_walk(ctx, refs):
    """The plain case again on a context of its own with the reference's walk: equal bytes."""
    _case, b, rays, _ref = refs["plain"]
    ctx.upload(b)
    got = ctx.shade_rays(rays, seed=sc.SEED)
    other = massrt.Context(0, options={"traversal": massrt.TRAVERSAL_REFERENCE})
    try:
        other.upload(b)
        again = other.shade_rays(rays, seed=sc.SEED)
    finally:
        other.close()
    assert got.tobytes() == again.tobytes()


def test_backgrounds_bit_exact(ctx):
    """One sample, closed aperture, depth 1, a world of one small MAT_NONE sphere: a missing path's
    radiance is 0 + 1 * background(d) on the device and what trace returns in the oracle. BG_SOLID,
    BG_SKY, and a CubeMap (texture under each wrap, solid, Blend, Fallback, texture; rotated) from three
    cameras that see all six faces (test_shade_oracle.py counts them)."""
    for kind, camera in sc.BG_CASES:
        b, o = massrt.Builder(3), oracle.Scene(3)
        scene = sc.background_case(kind, camera)
        scene(b)
        scene(o)
        ctx.upload(b)
        rgb, bo = ctx.render(sc.BG_W, sc.BG_H, 0, 1, seed=sc.SEED, max_depth=1)
        orgb, obo = o.render(sc.BG_W, sc.BG_H, 0, 1, seed=sc.SEED, max_depth=1)
        assert orgb.any() and np.unique(orgb.reshape(-1, 3), axis=0).shape[0] > (1 if kind == "solid" else 100)
        assert np.array_equal(bo, obo), (kind, camera)
        differ = (rgb.view(np.uint32) != orgb.view(np.uint32)).reshape(-1, 3).any(1)
        assert not differ.any(), (kind, camera, int(differ.sum()), int(np.flatnonzero(differ)[0]))
