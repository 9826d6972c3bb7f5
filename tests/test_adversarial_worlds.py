"""The near-first walk's per-scene hypotheses, on the host (tests/adversarial_worlds.py has the worlds,
tests/test_gpu_adversarial_worlds.py runs them on the device).

nf_tree.cpp builds the near-first trees only for a scene inside the domain its rounding bound is proven on, and
chooses each triangle's bound (coordinate-plane or generic), the cones and the wild instances. Here every gate
has a world just inside it and a twin just outside, and the triangles are the ones a bound can be wrong on:
slivers, needles, zero-area triangles, triangles a rounding from a coordinate plane. For each world: both Python
builders agree on the tree; through tools/slab_check (k_trace's walks compiled for the host, the world from a
file) the verdict is the expected one, both walks return the oracle's four words on every adversarial family,
plain and with directions of 2^k (adversarial_rays.short: the rays that do walk near first where generic
triangles make kw1 |d| > 2^-8 for |d| ~ 1), and no accepted hit lies further than rho from its box."""
import numpy as np
import pytest

import adversarial_rays as adv
import adversarial_worlds as aw
import slab_tool
from slab_tool import slab_check  # noqa: F401 (the fixture)
from test_bvh import assert_same_tree

SHORT_K = aw.SHORT_K


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    """name -> the world built by both builders, its file, the families' rays (plain and short) from the world's
    own desc() with the oracle's hits: made once, shared, left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            b, o = aw.build_both(name)
            with np.errstate(all="ignore"):  # out_inf: the sphere at 3e38
                plain = adv.families(*b.desc())
            rays, parts = adv.split({**plain, **adv.short(plain, SHORT_K)})
            want = o.trace_rays(rays)
            for a in (rays, want):
                a.setflags(write=False)
            path = aw.write(tmp_path_factory.mktemp(name) / "world.txt", aw.WORLDS[name][0]())
            cache[name] = {"b": b, "o": o, "file": path, "rays": rays, "parts": parts, "want": want}
        return cache[name]
    return get


def _differences(what, w, got):
    assert got.shape == w["want"].shape
    bad = [m for m in (adv.first_difference(name, w["rays"][a:e], got[a:e], w["want"][a:e]) for name, a, e in w["parts"])
           if m]
    assert not bad, f"{what}:\n" + "\n".join(bad)


def _bound_line(stdout):
    """(accepted hits checked, worst dist/rho, hits over rho) of slab_check's `nf bound:` line."""
    line = [x for x in stdout.splitlines() if " nf bound: " in x][0]
    return (int(line.split("nf bound: ")[1].split(" accepted")[0]), float(line.split("worst dist/rho ")[1].split(",")[0]),
            int(line.split(" over;")[0].rsplit(", ", 1)[1]), line)


@pytest.mark.parametrize("name", list(aw.WORLDS))
def test_builders_agree_and_families_hit(worlds, name):
    """Both Python builders build the same tree, and the oracle's own answers hold enough hits per family, the
    short ones included, for a comparison to prove something."""
    w = worlds(name)
    assert_same_tree(w["b"], w["o"])
    assert w["b"].rand_f32() == w["o"].rand_f32()
    d = w["b"].desc_only()
    assert d.n_spheres + d.n_triangles + d.n_instances + d.n_models <= 500
    names = {n for n, _, _ in w["parts"]}
    assert {"spheres", "tangent", "spheres/short", "tangent/short"} <= names
    adv.check_floors({n: w["want"][a:e] for n, a, e in w["parts"]}, overflow=False)


@pytest.mark.parametrize("name", aw.OUT_OF_DOMAIN)
def test_out_of_domain_twin_keeps_the_reference_walk(slab_check, worlds, name, tmp_path):
    """One number past a gate: the scene gets the stated nf_note and no near-first trees (`hits-nf` is refused), and
    the reference walk still returns the oracle's hits on every family."""
    w = worlds(name)
    r = slab_tool.run(slab_check, f"@{w['file']}", "nf")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no near-first trees (" in r.stdout and aw.WORLDS[name][1] in r.stdout, r.stdout
    refused = slab_tool.world_hits(slab_check, w["file"], "hits-nf", w["rays"][:16], tmp_path)
    assert not isinstance(refused, tuple) and refused.returncode != 0 and aw.WORLDS[name][1] in refused.stderr
    hits, _, _ = slab_tool.world_hits(slab_check, w["file"], "hits", w["rays"], tmp_path)
    _differences(f"hits on {name}", w, hits)


@pytest.fixture(scope="module")
def built(slab_check, worlds, tmp_path_factory):
    """name -> an in-domain world's runs of the tool: `hits`, `hits-nf` (with the rays that started near first) and
    `bound`, once."""
    cache = {}

    def get(name):
        if name not in cache:
            w, tmp = worlds(name), tmp_path_factory.mktemp(f"{name}_runs")
            runs = {walk: slab_tool.world_hits(slab_check, w["file"], walk, w["rays"], tmp) for walk in ("hits", "hits-nf")}
            rays_file = tmp / "rays.f32"  # written by world_hits
            runs["bound"] = slab_tool.run(slab_check, f"@{w['file']}", "bound", rays_file)
            cache[name] = runs
        return cache[name]
    return get


@pytest.mark.parametrize("name", aw.IN_DOMAIN)
def test_in_domain_world_walks_equal_the_oracle(worlds, built, name):
    """The trees are built, and both host walks return the oracle's four words on every family, plain and short.
    The comparison is about the near-first walk: at least 90% of the rays of every short geometric family started
    on it (a condition on the inputs, met by the choice of SHORT_K)."""
    w, runs = worlds(name), built(name)
    for walk in ("hits", "hits-nf"):
        assert isinstance(runs[walk], tuple), runs[walk].stdout + runs[walk].stderr  # hits-nf refused: not built
    near_first, stats = runs["hits-nf"][1], runs["hits-nf"][2]
    shares = {n: float(near_first[a:e].mean()) for n, a, e in w["parts"]}
    print(f"{name}: fallbacks {stats['fallbacks']}, starts_ref {stats['starts_ref']} of {len(near_first)}; "
          "started near first: " + ", ".join(f"{n} {s:.1%}" for n, s in shares.items()))
    for fam in adv.GEOMETRIC:
        if f"{fam}/short" in shares:
            assert shares[f"{fam}/short"] >= 0.9, f"{fam}/short: {shares[f'{fam}/short']:.1%} started near first"
    assert stats["starts_ref"] == int((~near_first).sum())
    for walk in ("hits", "hits-nf"):
        _differences(f"{walk} on {name}", w, runs[walk][0])


@pytest.mark.parametrize("name", aw.IN_DOMAIN)
def test_in_domain_world_hits_lie_within_rho(worlds, built, name):
    """The proof's claim (nf_bound.h) on the world's rays that start near first: every hit the
    reference's tests accept, at any t, lies within rho of its primitive's near-first box, of every node above it
    with its cone, and of its container's world box (a wild instance's within its own margin). DESIGN.md §4
    records the worst dist/rho per world."""
    r = built(name)["bound"]
    assert " bound: " in r.stdout, r.stdout + r.stderr
    n = len(worlds(name)["rays"])
    assert f" nf: 0 of {n} rays differ" in r.stdout, r.stdout + r.stderr
    checks, worst, over, line = _bound_line(r.stdout)
    print(line)
    assert checks > 10000 and over == 0 and worst <= 1.0, line
    assert r.returncode == 0, r.stdout + r.stderr


def test_slivers_graze_rays_sit_at_the_det_cut(worlds):
    """The reference accepts a triangle only if |det| = |d . (ab x ac)| >= 1e-6: at least 5% of the `graze` rays
    of `slivers` have that product (in float64, with the world-space triangle the ray was aimed at) within a
    factor 4 of the cut, so the cut decides on rays of the sample, either way."""
    w = worlds("slivers")
    a, e = next((a, e) for n, a, e in w["parts"] if n == "graze")
    rays, t = adv.graze_with_triangles(adv.geometry(*w["b"].desc()), e - a, adv.family_seed(adv.graze))
    assert np.array_equal(rays.view(np.uint32), w["rays"][a:e].view(np.uint32))  # the family's rays
    normals = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    det = np.abs((rays[:, 3:].astype(np.float64) * normals).sum(1))
    near = float(((det >= 0.25e-6) & (det <= 4e-6)).mean())
    assert near >= 0.05, f"{near:.1%} of the graze rays have |d . N| within [0.25e-6, 4e-6]"


def _tri_edges(b):
    d = b.desc_only()
    t = adv._table(d.triangles, d.n_triangles, aw.massrt.MrtTriangle)[:, :9].copy().view(np.float32)
    return t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3]  # float32, as upload.cpp forms ab and ac


def _generic_counts(stdout):
    line = [x for x in stdout.splitlines() if " bound: aw0 " in x][0]
    counts = line.split("generic triangles ")[1]  # "<n> off every coordinate plane, <m> on one"
    return int(counts.split(" off ")[0]), int(counts.split("plane, ")[1].split(" on ")[0])


def test_near_plane_generic_count(worlds, built):
    """tri_bound may use the coordinate-plane bound only for ab_k == ac_k == 0 exactly: the triangles with a
    nonzero ab_k or ac_k on every axis, a subnormal included, are counted here in numpy and must be the ones
    the tool reports as generic off every coordinate plane. Of the exactly planar ones, those whose in-plane
    normal nearly cancels take the generic bound too (tri_bound's exits)."""
    ab, ac = _tri_edges(worlds("near_plane")["b"])
    off_plane = int(((ab != 0) | (ac != 0)).all(1).sum())
    tiny = int((((ab != 0) | (ac != 0)).all(1) & ((np.abs(ab) < 1e-30) & (ab != 0) | (np.abs(ac) < 1e-30) & (ac != 0)).any(1)).sum())
    # the world holds what it is for: 3 axes x (11 values x 4 pairs - 3 of two zeros + 25 ulp pairs - 1 of two zeros)
    assert off_plane == 195 and tiny >= 30, (off_plane, tiny)
    generic, planar_generic = _generic_counts(built("near_plane")["bound"].stdout)
    assert generic == off_plane, (generic, off_plane)
    assert 0 < planar_generic <= 28, planar_generic  # of the 28 nearly cancelling ones


def test_big_flat_has_no_generic_triangle(built):
    assert _generic_counts(built("big_flat")["bound"].stdout) == (0, 0)


def test_instances_wild_count(built):
    """The (1.6e-5, 2, 2) scale and the 1000 x 0.001 x 1000 slab are wild, no other instance is
    (adversarial_worlds.INSTANCES_WILD says why)."""
    _, _, _, line = _bound_line(built("instances")["bound"].stdout)
    assert f", {aw.INSTANCES_WILD} wild instances" in line, line
