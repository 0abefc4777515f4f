"""The cut pool at tree nodes: Scorer.pool_separate_points at P LP points in one call against a loop of P calls with one point each,
the same function on the same handle.

    python tools/pool_points.py [--points 8 64 256] [--max-return 256] [--repeats 5] [--rows 262144] [--out profiles/pool_points.txt]

Host to host (numpy points in, views of the pinned block out), per call and per point; the median of --repeats blocks with the
smallest and the largest block behind it.  Two kinds of pool:
  * the pool a 4-round spar070-050-1 dim-3 run with pool_max_age = 2 leaves behind (strategy 1, share 0.1): the eigen-cuts of a root
    run, 9 entries each.  The points are the run's last LP point moved a tenth of the way towards seeded random McCormick points: what
    the LP points of nodes near the root look like
  * a synthetic pool of --rows rows of 20 entries (the longest eigen-cut row) on the same columns, both senses, right-hand sides placed
    around the activity at a base point; the points are perturbations of the base point.  Once with about half the rows violated
    (more than the workgroup's list holds: the radix select runs, the pool is walked ten times per point) and once with about one
    row in a hundred violated (they fit the list: one walk)
select_passes and n_violated are listed per line (medians over the points).

Needs a GPU.  Nothing is asserted: the file is a measurement."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
INST = os.path.join(ROOT, "tests", "golden", "instances", "spar070-050-1.in")


def timed(fn, repeats, budget_s=0.25):
    """-> ms per call: (median, min, max) over `repeats` blocks of as many calls as fit budget_s"""
    fn()
    t = time.perf_counter()
    fn()
    one = time.perf_counter() - t
    reps = max(1, min(200, int(budget_s / max(one, 1e-6))))
    blocks = []
    for _ in range(repeats):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        blocks.append(1e3 * (time.perf_counter() - t) / reps)
    return float(np.median(blocks)), min(blocks), max(blocks)


def table(sc, make_points, Ps, max_return, repeats):
    lines = ["      P | batched ms/call            us/point | loop ms/call               us/point | loop / batched | select_passes | violated (median)"]
    for P in Ps:
        pts = make_points(P)
        out = sc.pool_separate_points(pts, max_return)
        rows = [pts[p:p + 1] for p in range(P)]

        def loop():
            for r in rows:
                sc.pool_separate_points(r, max_return)
        b = timed(lambda: sc.pool_separate_points(pts, max_return), repeats)
        lo = timed(loop, repeats)
        lines.append("   %4d | %9.4f (%9.4f .. %9.4f) %9.2f | %9.4f (%9.4f .. %9.4f) %9.2f | %14.2f | %13d | %d"
                     % (P, b[0], b[1], b[2], 1e3 * b[0] / P, lo[0], lo[1], lo[2], 1e3 * lo[0] / P, lo[0] / b[0],
                        int(np.median([o["select_passes"] for o in out])), int(np.median([o["n_violated"] for o in out]))))
    return lines


def synthetic_block(rng, m, ncols, base, shifts):
    """m rows of 20 distinct columns each (numpy, vectorised): rhs = activity at base - sense * shift * ||row||"""
    ln = 20
    cols = np.argsort(rng.random((m, 64)), axis=1)[:, :ln] * (ncols // 64) + rng.integers(0, ncols // 64, size=(m, ln))
    vals = rng.standard_normal((m, ln))
    sense = np.where(rng.random(m) < 0.5, 1, -1).astype(np.int32)
    act = np.sum(vals * base[cols], axis=1)
    shift = shifts[np.arange(m) % len(shifts)] * np.sqrt(np.sum(vals * vals, axis=1))
    ptr = np.arange(m + 1, dtype=np.int32) * ln
    return ptr, cols.reshape(-1).astype(np.int32), vals.reshape(-1), act - sense * shift, sense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--max-return", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_points.txt"))
    args = ap.parse_args()
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    lines = ["# tools/pool_points.py --points %s --max-return %d --repeats %d --rows %d: ms per call, us per point; median over the blocks (min .. max)"
             % (" ".join(map(str, args.points)), args.max_return, args.repeats, args.rows),
             "# batched = pool_separate_points(P points, %d); loop = P x pool_separate_points(1 point, %d) on the same handle; states = all"
             % (args.max_return, args.max_return), ""]

    def flush():
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    # 1. the pool a root run leaves behind
    cs = pkg.CutSolver()
    cs.cut_select_algo(INST, 3, 0.1, strat=1, nb_rounds_cuts=4, pool_max_age=2)
    sc = cs.pool_loop.pool
    st = sc.pool_state()
    n = cs._nb_vars
    last = np.array(cs._my_prob.get_values())

    def near_root(P):
        return np.stack([0.9 * last + 0.1 * harness.random_mccormick_point(n, np.random.default_rng(100 + p)) for p in range(P)])
    lines.append("spar070-050-1 dim 3, 4 rounds, pool_max_age 2: %d rows (%d in the LP, %d parked), %d entries each"
                 % (st["n"], int(np.sum(st["state"] == 0)), int(np.sum(st["state"] == 1)), int(np.median(st["nnz"]))))
    lines.extend(table(sc, near_root, args.points, args.max_return, args.repeats))
    lines.append("")
    flush()

    # 2. synthetic pools on the same columns
    ncols = n * (n + 1) // 2 + n
    for name, shifts in (("about half the rows violated", np.array([0.0, 0.1, -0.1, 0.001, -0.001])),
                         ("about one row in a hundred violated", np.array([0.1] * 99 + [-0.1]))):
        rng = np.random.default_rng(1)
        base = rng.random(ncols)
        sc.pool_create(args.rows)
        done = 0
        while done < args.rows:
            m = min(65536, args.rows - done)
            sc.pool_add(*synthetic_block(rng, m, ncols, base, shifts))
            done += m

        def near_base(P):
            return base[None, :] + 0.01 * np.random.default_rng(7).standard_normal((P, ncols))
        lines.append("synthetic: %d rows of 20 entries, %s" % (args.rows, name))
        lines.extend(table(sc, near_base, args.points, args.max_return, args.repeats))
        lines.append("")
        flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
