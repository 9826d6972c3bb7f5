"""The wavefront loop's integer decisions on the host, no GPU (csrc/host/loop.h
through tools/loop_check.cpp): k_reserve's refill and gap-closing plan, the
sizes plan_buffers gives the pool and the results slab, the split of a chunk's
first paths over the queues, and what a queue does with a status read. The
kernels and render.hip call the same functions; on the GPU only whole renders
see them (tests/test_gpu_frames.py::test_shade_bin_is_bit_identical)."""
import shutil
import subprocess

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = tmp_path_factory.mktemp("loop") / "loop_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), str(REPO / "tools" / "loop_check.cpp")],
                   check=True)

    def run(mode):
        r = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-400:]
        return [ln.split() for ln in r.stdout.splitlines()]

    return run


def test_refill_keeps_every_path_once_and_the_pool_contiguous(check):
    """k_reserve + k_refill on a model pool: bottom survivors in [0, lo), top
    survivors in [cap - hi, cap), then the plan applied as k_refill does it —
    the move and the fill run in one launch, unordered, so their slot ranges
    must not meet at all."""
    rows = [tuple(int(x) for x in r) for r in check("refill")]
    seen = set()
    for cap, lo, hi, G, work, want, slot, count, base, mv, src, dst, active in rows:
        case = (cap, lo, hi, G, work)
        seen.add(case)
        assert want == cap - lo - hi, case
        issued = want > 0 and work < G  # the counter is advanced only while it is below G
        assert base == (work if issued else G), case
        assert count == (min(want, G - work) if work < G else 0), case
        assert base + count <= G, case
        assert active <= cap, case
        pool = [None] * cap
        for i in range(lo):
            pool[i] = ("s", i)
        for i in range(hi):
            pool[cap - hi + i] = ("s", lo + i)
        before = list(pool)
        srcs, dsts, fills = range(src, src + mv), range(dst, dst + mv), range(slot, slot + count)
        assert not set(srcs) & set(dsts), case  # sources and destinations are disjoint
        assert not set(fills) & (set(srcs) | set(dsts)), case
        for a, b in zip(srcs, dsts):
            assert 0 <= a < cap and 0 <= b < cap, case
            assert before[a] is not None and before[b] is None, case  # a live path onto a free slot
            pool[b], pool[a] = before[a], None
        for j, i in enumerate(fills):
            assert 0 <= i < cap and before[i] is None, case  # no fill lands on a live slot
            pool[i] = ("w", base + j)
        # the pool stays contiguous: every survivor and every new work item once in [0, active), nothing past it
        want_set = {("s", i) for i in range(lo + hi)} | {("w", base + j) for j in range(count)}
        assert None not in pool[:active] and len(set(pool[:active])) == active and set(pool[:active]) == want_set, case
        assert all(p is None for p in pool[active:]), case
    want_cases = {(cap, lo, hi, G, work) for cap in range(1, 11) for lo in range(cap + 1) for hi in range(cap - lo + 1)
                  for G in range(1, 2 * cap + 3) for work in range(G + cap + 2)}
    assert seen == want_cases and len(rows) == len(want_cases) == 95946


def test_sizes_shrink_the_pool_first_and_fit_the_budget(check):
    rows = check("sizes")
    assert rows[0][0] == "const"
    path_bytes, floor = int(rows[0][1]), int(rows[0][2])
    assert path_bytes == 16 * (2 * 5 + 1) and floor == 64 << 20  # two state sets of 5 x 16 B + the hit; 64M paths

    def pool_bytes(K, P):  # 256-B aligned sections: at most 4096 B of padding per queue
        return (path_bytes * -(-P // K) + 4096) * K

    plans = [tuple(int(x) for x in r[1:]) for r in rows if r[0] == "plan"]
    assert len(plans) > 10000
    n_unchanged = n_pool_shrunk = n_chunk_shrunk = n_nofit = 0
    for n_pix, spp, pool_paths, K, budget, need_pool, P, chunk, fits, pb in plans:
        case = (n_pix, spp, pool_paths, K, budget, need_pool)
        assert K in (1, 2, 3, 4) and pb == pool_bytes(K, P), case
        P0 = min(n_pix * spp, pool_paths) if need_pool else 0
        need = (pool_bytes(K, P) if P else 0) + 16 * n_pix * chunk
        assert 1 <= chunk <= spp and P <= P0 and P <= n_pix * chunk, case
        assert (P > 0) == bool(need_pool), case  # need_pool = false plans no pool; a pool never shrinks to nothing
        if (pool_bytes(K, P0) if P0 else 0) + 16 * n_pix * spp <= budget:  # room for everything: unchanged
            assert (P, chunk, fits) == (P0, spp, 1), case
            n_unchanged += 1
        if chunk < spp:  # the samples per chunk shrink only once the pool is at its floor
            assert P <= floor, case
            n_chunk_shrunk += 1
        if P < P0 and chunk == spp:
            assert P >= floor, case  # the pool alone never goes below the floor
            n_pool_shrunk += 1
        if fits:
            assert need <= budget, case
        else:  # only when not even one sample per pixel fits beside the smallest pool
            assert need > budget and chunk == 1 and P <= floor and P <= n_pix, case
            n_nofit += 1
    assert min(n_unchanged, n_pool_shrunk, n_chunk_shrunk, n_nofit) > 100  # the grid reaches every branch

    chunks = [tuple(int(x) for x in r[1:]) for r in rows if r[0] == "chunk"]
    assert len(chunks) >= 50
    for spp_count, results_max, n_pix, first in chunks:
        assert first == max(1, min(spp_count, results_max // n_pix)), (spp_count, results_max, n_pix)
        assert 1 <= first <= spp_count and (first == 1 or first * n_pix <= results_max)


def test_queue_shares_sum_and_fit_each_queue(check):
    rows = [tuple(int(x) for x in r) for r in check("share")]
    assert {(K, P) for K, P, *_ in rows} == {(K, P) for K in range(1, 5) for P in range(1, 41)}
    for K, P, n0, *shares in rows:
        per_q = -(-P // K)  # ensure_pool: a queue's capacity
        assert len(shares) == K and sum(shares) == n0 and all(0 <= s <= per_q for s in shares), (K, P, n0, shares)
        base, running = 0, []  # the fork's running sum: queue k starts at work item `base`
        for k in range(K):
            running.append(n0 * (k + 1) // K - base)
            base += running[-1]
        assert shares == running, (K, P, n0)
    assert any(n0 < K for K, P, n0, *_ in rows) and any(n0 == K * -(-P // K) for K, P, n0, *_ in rows)


def test_status_rule(check):
    rows = check("status")
    assert rows[0][0] == "const"
    batch, max_it = int(rows[0][1]), int(rows[0][2])
    assert batch > 0 and batch % 2 == 0  # a status read sees the live pool in active[0]
    assert max_it == 64 * 1024
    seqs = {}
    for r in rows[1:]:
        seqs.setdefault(int(r[0]), []).append(r)
    assert len(seqs) >= 50
    ends = set()
    for sid, steps in seqs.items():
        bound, exhausted = -1, 0
        for n, r in enumerate(steps):
            G, finish_paths, a0, _a1, short, work = (int(x) for x in r[1:7])
            step, new_bound, new_exh, finished = r[7], int(r[8]), int(r[9]), int(r[10])
            case = (sid, n, r)
            if short:  # any nonzero shade_short fails, and changes nothing
                assert step == "shade_short" and (new_bound, new_exh, finished) == (bound, exhausted, 0), case
            else:
                assert new_exh == (1 if exhausted or work >= G else 0), case  # sticky, and only from the counter
                assert (new_bound == -1) == (not new_exh), case  # unbounded until the counter is seen exhausted
                if work >= G:
                    assert new_bound == (a0 if bound == -1 else min(bound, a0)), case  # never rises
                else:
                    assert new_bound == bound, case
                if work < G:
                    assert step == "go_on", case  # never finishes while work is left
                elif a0 > finish_paths:
                    assert step == "go_on", case
                else:  # a hand-off launch only for 0 < active0 <= finish_paths
                    assert step == ("hand_off" if a0 > 0 else "finished"), case
                if finish_paths == 0:
                    assert step != "hand_off" and (step == "finished") == (work >= G and a0 == 0), case
                assert finished == (step in ("hand_off", "finished")), case
            bound, exhausted = new_bound, new_exh
        assert all(r[7] == "go_on" for r in steps[:-1])  # a sequence ends with its queue
        ends.add(steps[-1][7])
    assert ends == {"hand_off", "finished", "shade_short"}


def test_nothing_to_add_is_any_zero_factor(check):
    """A render adds nothing exactly when it has no samples, no depth or no list entries: the one rule every entry
    point asks before it plans or enqueues anything."""
    rows = [tuple(int(x) for x in r) for r in check("nothing")]
    vals = (0, 1, 7, 2 ** 32 - 1)
    assert {r[:3] for r in rows} == {(s, d, n) for s in vals for d in vals for n in vals} and len(rows) == 64
    for spp, depth, n, nothing in rows:
        assert nothing == (1 if 0 in (spp, depth, n) else 0), (spp, depth, n)
