"""The near-first walk's per-scene hypotheses on the device (tests/adversarial_worlds.py has the worlds,
tests/test_adversarial_worlds.py runs them through the host build of the walks).

nf_tree.cpp decides per scene whether k_trace may walk near first: every gate has a world just inside it and
twins one number outside, and the in-domain worlds hold the triangles a bound can be wrong on (slivers, needles,
zero-area triangles, triangles a rounding from a coordinate plane), spheres of radius 2^-59 to 2^12, wild and
mirrored instances. On the device nf_sqrt_up, nf_min, the cones' rcp and the wild box test are other instructions
than on the host, and subnormal edges meet the device's arithmetic: every ray of every adversarial family, plain
and with directions of 2^k (the rays that walk near first where generic triangles are large), must come back with
the oracle's four words on both walks."""
import numpy as np
import pytest

import adversarial_rays as adv
import adversarial_worlds as aw
import massrt

pytestmark = pytest.mark.gpu
WALKS = {"reference": massrt.TRAVERSAL_REFERENCE, "near_first": massrt.TRAVERSAL_NEAR_FIRST}


@pytest.fixture(scope="module")
def contexts():
    c = {name: massrt.Context(0, options={"traversal": walk}) for name, walk in WALKS.items()}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def worlds():
    """name -> (builder, the families' rays, plain and short, as one array, (family, begin, end) offsets, the
    oracle's hits): made once, shared, left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            b, o = aw.build_both(name)
            with np.errstate(all="ignore"):  # out_inf: the sphere at 3e38
                plain = adv.families(*b.desc())
            rays, parts = adv.split({**plain, **adv.short(plain, aw.SHORT_K)})
            want = o.trace_rays(rays)
            for a in (rays, want):
                a.setflags(write=False)
            cache[name] = b, rays, parts, want
        return cache[name]
    return get


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("name", list(aw.WORLDS))
def test_world(contexts, worlds, name, walk):
    """Uploaded under option NEAR_FIRST an in-domain world walks near first and an out-of-domain twin keeps the
    reference walk; either way, and under option REFERENCE, all four words of every ray equal the oracle's."""
    b, rays, parts, want = worlds(name)
    ctx = contexts[walk]
    ctx.upload(b)
    built = aw.WORLDS[name][1] is aw.BUILT
    assert ctx.tuning()["traversal"] == (WALKS[walk] if built else massrt.TRAVERSAL_REFERENCE)
    got = ctx.trace_rays(rays)
    assert got.shape == want.shape
    bad = [m for m in (adv.first_difference(n, rays[a:e], got[a:e], want[a:e]) for n, a, e in parts) if m]
    assert not bad, f"{walk} walk on {name}:\n" + "\n".join(bad)


@pytest.mark.parametrize("name", ["instances", "radii"])
def test_render_equals_the_reference_walk(contexts, worlds, name):
    """Camera rays and their bounces, whole paths: no generic term in these two worlds, so they walk near first
    (tests/test_adversarial_worlds.py: every plain geometric family starts there). A 64 x 36 render of 2 samples
    per pixel is bit-identical between the walks, bounce counts included."""
    b = worlds(name)[0]
    out = {}
    for walk, ctx in contexts.items():
        ctx.upload(b)
        assert ctx.tuning()["traversal"] == WALKS[walk]
        ctx.reset_counters()
        out[walk] = ctx.render(64, 36, 0, 2, seed=5, counters=True) + (ctx.counters(),)
    (ra, ba, _), (rn, bn, cn) = out["reference"], out["near_first"]
    print(f"{name}: vnf_fallbacks {cn['vnf_fallbacks']} of {cn['segments']} segments")
    assert int((bn > 0).sum()) > 64 * 36 // 4  # the paths meet the world
    assert np.array_equal(ba, bn)
    assert np.array_equal(ra.view(np.uint32), rn.view(np.uint32))
