"""Volume::intersect over an Instance or a Model target (geom.rs:611-655),
composed from the CPU oracle, which itself knows sphere volumes only.

An oracle scene holding nothing but the target, unbuilt, makes
World::intersect (world.rs:131-144) the target's own intersect. So:

  enter = trace_rays(rays, -inf, +inf)            closest hit by t, may be negative
  exit  = trace_rays(ray_i, enter_i + 0.0001, +inf)   one call per ray (t_min differs)
  steps 3-6 in numpy float32, the draw from oracle.path_rng(0, i, 0xFFFFFFFE, 1)
  (the stream mrt_trace_rays documents), ln from the host libm logf (the
  device's table is built from that function; numpy's float32 log need not
  round alike).

The oracle's counters over those two traces are what the reference executes
for the volume test: every BoundingBox::hit, every Triangle::intersect, one
Instance::intersect / Model::intersect per search."""
import ctypes
import ctypes.util

import numpy as np

import massrt
import oracle

F = np.float32
INF = float("inf")
CUBE = "cube.ply"
# the instance target of the parity tests
INST_T, INST_R, INST_S = (0.3, 0.2, -0.5), (0.4, 0.7, 0.2), (1.0, 0.6, 0.8)
DENSITY = 0.5
INTERVALS = [(0.001, INF), (0.7, 1.5), (0.001, 0.8)]
VOLUME0 = massrt.REF_VOLUME << 28

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x) -> np.ndarray:
    return np.array([_libm.logf(float(v)) for v in np.asarray(x, dtype=F)], dtype=F)


def rays_about(centre, n=4096, seed=3) -> np.ndarray:
    """Half from a radius-4 shell aimed at the box (normal scatter 0.45 about its
    centre), a quarter from inside radius 0.3, a quarter from the shell in
    random directions; direction lengths 0.3 to 3."""
    g = np.random.default_rng(seed)
    c = np.asarray(centre, dtype=np.float64)

    def unit(k):
        v = g.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    h, q = n // 2, n // 4
    o = np.concatenate([c + 4.0 * unit(h), c + 0.3 * g.random((q, 1)) * unit(q), c + 4.0 * unit(n - h - q)])
    d = np.concatenate([(c + 0.45 * g.normal(size=(h, 3))) - o[:h], unit(q), unit(n - h - q)])
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(0.3, 3.0, size=(n, 1))
    return np.concatenate([o, d], axis=1).astype(F)


def target_scene(golden, kind) -> oracle.Scene:
    """An oracle scene holding only the target: unbuilt, so World::intersect is target.intersect."""
    o = oracle.Scene(1)
    m = o.material(massrt.MAT_NONE)
    if kind == "instance":
        o.add_instance(o.model_from_ply(golden / CUBE, m), INST_T, INST_R, INST_S)
    else:
        o.model_from_ply(golden / CUBE, m, add_to_world=True)
    return o


class Searches:
    """enter / exit of every ray over the whole line, and the oracle's counters for both traces."""

    def __init__(self, golden, kind, rays):
        o = target_scene(golden, kind)
        o.reset_counters()
        n = rays.shape[0]
        e = o.trace_rays(rays, -INF, INF)
        self.has_enter = e[:, 0] != 0
        self.enter = e[:, 2].copy().view(F)
        self.has_exit = np.zeros(n, dtype=bool)
        self.exit = np.zeros(n, dtype=F)
        past = (self.enter + F(0.0001)).astype(F)  # one f32 add
        for i in np.flatnonzero(self.has_enter):
            x = o.trace_rays(rays[i:i + 1], float(past[i]), INF)
            self.has_exit[i] = x[0, 0] != 0
            self.exit[i] = x[0, 2:3].view(F)[0]
        self.counters = o.counters()


def volume_hits(rays, s: Searches, t_min, t_max, density=DENSITY):
    """Steps 3-6 for every ray against [t_min, t_max] (scalars or per-ray arrays):
    (hit mask, t float32, categories). Categories: 'miss' the target is not hit,
    'degenerate' the enter >= exit return, 'pass' the ray went through, 'hit'."""
    n = rays.shape[0]
    t_min = np.broadcast_to(np.asarray(t_min, dtype=F), (n,))
    t_max = np.broadcast_to(np.asarray(t_max, dtype=F), (n,))
    both = s.has_enter & s.has_exit
    with np.errstate(all="ignore"):
        enter = np.where(s.enter < t_min, t_min, s.enter).astype(F)
        exit_ = np.where(s.exit > t_max, t_max, s.exit).astype(F)
        ordered = both & ~(enter >= exit_)
        enter = np.where(enter < F(0), F(0), enter).astype(F)
        d = rays[:, 3:6]
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
        f = np.array([oracle.path_rng(0, int(i), 0xFFFFFFFE, 1)[1][0] for i in range(n)], dtype=F)
        dist = (logf(f) * (F(-1.0) / F(density))).astype(F)
        inside = ((exit_ - enter).astype(F) * length).astype(F)
        hit = ordered & ~(dist > inside)
        t = (enter + (dist / length).astype(F)).astype(F)
    cat = np.where(~both, "miss", np.where(~ordered, "degenerate", np.where(hit, "hit", "pass")))
    return hit, np.where(hit, t, F(0)).astype(F), cat


def assert_not_empty(cat, s: Searches):
    """No parity test may pass on an empty case."""
    n = cat.size
    frac = {k: float(np.count_nonzero(cat == k)) / n for k in ("hit", "pass", "miss", "degenerate")}
    inside = float(np.count_nonzero(s.has_enter & (s.enter < 0))) / n
    print(f"volume hits {frac['hit']:.3f} pass {frac['pass']:.3f} miss {frac['miss']:.3f} "
          f"enter>=exit {frac['degenerate']:.4f} start inside {inside:.3f}")
    assert frac["hit"] >= 0.25 and frac["pass"] >= 0.25 and frac["miss"] >= 0.20 and inside >= 0.15, (frac, inside)
    assert np.count_nonzero(cat == "degenerate") >= 1, frac


def assert_clip_exercised(cat, s: Searches, t_min, t_max):
    """The clipped intervals (step 3). The same rays as the open interval, whose
    conditions assert_not_empty checks; clipped to [0.7, 1.5] or [0.001, 0.8] most
    of them take the enter >= exit return by construction (t is in units of a
    direction of length 0.3 to 3, the shell is 4 away), so the shares differ.
    What must not be empty here: every outcome keeps at least 2 % of the rays
    (80 of 4096: a clip applied wrongly to any of them shows), and so does
    each clip that the interval adds, counted over the rays it binds on
    without emptying their interval."""
    n = cat.size
    both = s.has_enter & s.has_exit
    for k in ("hit", "pass", "miss", "degenerate"):
        assert np.count_nonzero(cat == k) >= 0.02 * n, (k, np.count_nonzero(cat == k))
    lo = np.count_nonzero(both & (s.enter < F(t_min)) & (s.exit > F(t_min)) & (cat != "degenerate"))
    hi = np.count_nonzero(both & (s.exit > F(t_max)) & (s.enter < F(t_max)) & (cat != "degenerate"))
    print(f"t_min clips {lo} rays, t_max clips {hi} rays")
    assert lo >= 0.02 * n
    assert t_max == INF or hi >= 0.02 * n


def expected_hits(hit, t) -> np.ndarray:
    """mrt_trace_rays' columns for a world holding only the volume: prim, container, t bits, front_face."""
    out = np.zeros((hit.size, 4), dtype=np.uint32)
    out[hit, 0] = VOLUME0
    out[:, 2] = np.where(hit, t, F(0)).astype(F).view(np.uint32)
    out[hit, 3] = 1
    return out
