"""numpy float32 restatement of mrt_render_adaptive's contract (include/massrt.h):
the per-sample terms, the tile decision with its slot and tree order, the round
schedule and the report. No code is shared with the library: the tests compare
the two bit for bit.

All arithmetic is float32 on arrays (numpy neither contracts nor reorders):
  per sample   y = (r + g) + b;  m1 += y;  m2 += y * y;  n += 1
  per pixel    nf = float32(n); L = nf * m2 - m1 * m1; q = m1 + nf * floor;
               R = (tau2 * (nf - 1)) * (q * q),  tau2 = threshold * threshold
  per tile     slot i = (y % 8) * 8 + (x % 8), absent slots +0; L and R summed by
               the tree k = 32, 16, .., 1: v[i] = v[i] + v[i + k], i < k;
               closed iff every present pixel has n >= 2 and L_sum <= R_sum
"""
import numpy as np

TILE = 8
F = np.float32


def tile_pixels(W, H, shard_index=0, shard_count=1):
    """[T, 64] pixel p = y * W + x of each slot of each tile of the shard (frame
    tiles t with t % count == index, in raster order), -1 where a tile hangs
    over the frame's edge."""
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles = np.arange(shard_index, tx * ty, shard_count)
    i = np.arange(TILE * TILE)
    x = (tiles[:, None] % tx) * TILE + i[None, :] % TILE
    y = (tiles[:, None] // tx) * TILE + i[None, :] // TILE
    return np.where((x < W) & (y < H), y * W + x, -1).astype(np.int64)


def tree_sum(v):
    """[T, 64] float32 -> [T]: the contract's tree, in float32."""
    v = v.astype(F).copy()
    k = 32
    while k:
        v[:, :k] = v[:, :k] + v[:, k:2 * k]
        k //= 2
    return v[:, 0]


def pixel_terms(m1, m2, n, threshold, floor):
    with np.errstate(all="ignore"):
        tau2 = F(threshold) * F(threshold)
        nf = n.astype(F)
        L = nf * m2 - m1 * m1
        q = m1 + nf * F(floor)
        R = (tau2 * (nf - F(1.0))) * (q * q)
    return L.astype(F), R.astype(F)


def tiles_open(W, H, moments, samples, threshold, floor, shard_index=0, shard_count=1):
    """uint8 [T]: 1 = open, for every tile of the shard in shard order."""
    mom = np.asarray(moments, F).reshape(-1, 2)
    n = np.asarray(samples, np.uint32).reshape(-1)
    pix = tile_pixels(W, H, shard_index, shard_count)
    present = pix >= 0
    p = np.where(present, pix, 0)
    L, R = pixel_terms(mom[p, 0], mom[p, 1], n[p], threshold, floor)
    L = np.where(present, L, F(0.0)).astype(F)
    R = np.where(present, R, F(0.0)).astype(F)
    with np.errstate(all="ignore"):
        ls, rs = tree_sum(L), tree_sum(R)
        closed = np.all(~present | (n[p] >= 2), axis=1) & (ls <= rs)
    return (~closed).astype(np.uint8)


def schedule(min_spp, step_spp, cap):
    """[(first, count)] per round if every tile stays open: round 0 the minimum,
    then steps, the last one what is left of the cap. `first` counts from spp_begin."""
    out, done = [(0, min_spp)], min_spp
    while done < cap:
        c = min(step_spp, cap - done)
        out.append((done, c))
        done += c
    return out


def run(W, H, frames_rgb, frames_b, min_spp, step_spp, cap, threshold, floor, shard_index=0, shard_count=1,
        state=None):
    """The whole call over per-sample frames: frames_rgb[k] (W*H*3 float32) and
    frames_b[k] (W*H uint32) are what sample spp_begin + k adds, k < cap.
    state = (rgb, bounces, moments, samples) continues an estimate (copied).
    Returns a dict: rgb, bounces, moments, samples, open (tiles open after each
    round) and the report."""
    npx = W * H
    if state is None:
        rgb, bo = np.zeros((npx, 3), F), np.zeros(npx, np.uint32)
        mom, n = np.zeros((npx, 2), F), np.zeros(npx, np.uint32)
    else:
        rgb, bo = state[0].astype(F).reshape(npx, 3).copy(), state[1].astype(np.uint32).copy()
        mom, n = state[2].astype(F).reshape(npx, 2).copy(), state[3].astype(np.uint32).copy()
    pix = tile_pixels(W, H, shard_index, shard_count)
    running = np.ones(pix.shape[0], bool)
    done, rounds, total, curve = 0, 0, 0, []
    while True:
        count = min_spp if rounds == 0 else min(step_spp, cap - done)
        sel = pix[running]
        sel = sel[sel >= 0]
        for k in range(done, done + count):
            s = np.asarray(frames_rgb[k], F).reshape(npx, 3)[sel]
            rgb[sel] = rgb[sel] + s
            bo[sel] += np.asarray(frames_b[k], np.uint32)[sel]
            y = (s[:, 0] + s[:, 1]) + s[:, 2]
            mom[sel, 0] = mom[sel, 0] + y
            mom[sel, 1] = mom[sel, 1] + y * y
            n[sel] += 1
        total += int(sel.size) * count
        done += count
        rounds += 1
        running &= tiles_open(W, H, mom, n, threshold, floor, shard_index, shard_count).astype(bool)
        curve.append(int(running.sum()))
        if not running.any() or done == cap:
            break
    report = {"rounds": rounds, "spp_reached": done, "tiles": int(pix.shape[0]), "tiles_open": curve[-1],
              "samples": total}
    return {"rgb": rgb.reshape(-1), "bounces": bo, "moments": mom.reshape(-1), "samples": n, "open": curve,
            "report": report}


def resolve(rgb, samples):
    """out[3p+c] = (1 / float32(samples[p])) * rgb[3p+c], zeros where the count is 0."""
    n = np.asarray(samples, np.uint32)
    with np.errstate(all="ignore"):
        scale = np.where(n > 0, F(1.0) / n.astype(F), F(0.0)).astype(F)
    out = scale[:, None] * np.asarray(rgb, F).reshape(-1, 3)
    return np.where(n[:, None] > 0, out, F(0.0)).astype(F).reshape(-1)


def per_tile_counts(W, H, samples):
    """The sample count of every tile of the frame (its pixels share one)."""
    pix = tile_pixels(W, H)
    n = np.asarray(samples)[np.where(pix >= 0, pix, pix.max(axis=1, keepdims=True))]
    assert np.all(n == n[:, :1])
    return n[:, 0]


def check_not_vacuous(counts, lo, hi):
    """The issue's non-vacuity: at least 3 distinct per-tile sample counts each
    held by at least 2 tiles, some tile at `lo` and some at `hi`."""
    vals, held = np.unique(counts, return_counts=True)
    assert int((held >= 2).sum()) >= 3, dict(zip(vals.tolist(), held.tolist()))
    assert lo in vals and hi in vals, vals


# ---- the decision's test inputs (CPU and GPU tests share them) --------------

def random_moments(W, H, seed):
    """Moments of plausible estimates, tile by tile from calm to noisy, so both
    outcomes occur: per pixel n in [2, 64], mean mu in [0.05, 2], a relative
    deviation per tile over 2.5 decades; m1 = n mu, m2 = n (mu^2 + sd^2)."""
    rng = np.random.default_rng(seed)
    npx = W * H
    n = rng.integers(2, 65, npx).astype(np.uint32)
    mu = rng.uniform(0.05, 2.0, npx)
    tx = (W + TILE - 1) // TILE
    p = np.arange(npx)
    tile = (p // W // TILE) * tx + (p % W) // TILE
    rel = 10.0 ** rng.uniform(-1.0, 1.5, tile.max() + 1)
    sd = rel[tile] * mu * rng.uniform(0.5, 1.5, npx)
    mom = np.stack([n * mu, n * (mu * mu + sd * sd)], axis=1).astype(F)
    return mom.reshape(-1), n


def decision_cases(W, H, seed=5):
    """[(name, moments, samples, threshold, floor)] for a W x H frame: random
    moments under three rules, and a calm frame (n = 16, y = 1 +- a little:
    every tile closes at threshold 0.2) with one thing changed in one pixel of
    its first and of its last tile."""
    cases = []
    mom, n = random_moments(W, H, seed)
    for thr, fl in ((0.2, 0.01), (0.05, 0.0), (1.0, 0.5)):
        cases.append((f"random thr {thr} floor {fl}", mom, n, thr, fl))
    npx = W * H
    calm_m = np.tile(np.array([16.0, 16.01], F), npx)
    calm_n = np.full(npx, 16, np.uint32)
    cases.append(("calm", calm_m, calm_n, 0.2, 0.01))

    def changed(name, m1=None, m2=None, cnt=None, thr=0.2, fl=0.01):
        m, c = calm_m.copy(), calm_n.copy()
        for p in (min(W - 1, 3) + min(H - 1, 2) * W, npx - 1):
            if m1 is not None:
                m[2 * p] = m1
            if m2 is not None:
                m[2 * p + 1] = m2
            if cnt is not None:
                c[p] = cnt
        cases.append((name, m, c, thr, fl))

    changed("n 0 in one slot", 0.0, 0.0, 0)
    changed("n 1 in one slot", 1.0, 1.0, 1)
    changed("n 2 in one slot", 2.0, 2.001, 2)
    for name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        changed(f"m1 {name}", m1=v)
        changed(f"m2 {name}", m2=v)
    changed("a noisy pixel", m2=4000.0)
    # zero variance everywhere: m2 = m1^2 / n exactly, L = 0 in every pixel
    zero_m = np.tile(np.array([16.0, 16.0], F), npx)
    cases.append(("zero variance", zero_m, calm_n, 0.2, 0.01))
    cases.append(("zero variance, threshold 0", zero_m, calm_n, 0.0, 0.01))
    cases.append(("calm, threshold 0", calm_m, calm_n, 0.0, 0.01))
    cases.append(("calm, floor 0", calm_m, calm_n, 0.2, 0.0))
    cases.append(("random, threshold 0", mom, n, 0.0, 0.0))
    # L slightly negative from rounding: n = 3, m2 one ulp below m1^2 / n
    m1 = F(0.3)
    neg_m = np.tile(np.array([m1, np.nextafter(F(m1 * m1 / F(3.0)), F(0.0))], F), npx)
    neg_n = np.full(npx, 3, np.uint32)
    assert (F(3.0) * neg_m[1] - m1 * m1) < 0
    cases.append(("L slightly negative", neg_m, neg_n, 0.2, 0.01))
    cases.append(("L slightly negative, threshold 0", neg_m, neg_n, 0.0, 0.0))
    return cases
