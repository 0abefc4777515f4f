"""Diverse selection in the cutting-plane loop: CutSolver.cut_select_algo with and without the parallelism filter
(max_parallel in {0.9, 0.5}) on BoxQP instances under tests/golden/instances, and the device time of a filtered round next to the
plain round of the same quota.

    python tools/diverse_rounds.py [--instances spar020-100-1 spar040-030-1 spar070-050-1] [--dims 3] [--strats 1 4]
                                   [--rounds 4] [--sel 0.1] [--pool-factor 4] [--out profiles/diverse_rounds.txt]

Per run and round: the LP bound after the round's solve, the rows the round added, the seconds of that LP solve (HiGHS,
harness.LinearRelaxation) and of the separation, and the walk's counts (pool, examined, not violated, rejected as parallel).
Then, per instance and strategy: host-to-host milliseconds of Scorer.round_csr_diverse and of Scorer.round_csr at the same quota
and LP point (a random McCormick point), median of --repeats after one warm-up call each.

Needs a GPU.  Nothing is asserted: the file is a measurement."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
FILTERS = (None, 0.9, 0.5)


def loop_lines(path, dim, strat, sel, rounds, pool_factor):
    from sdpcutsel_via_nn_amd.cut_solver import CutSolver
    lines = []
    for mp in FILTERS:
        solver = CutSolver()
        logs = []
        out = solver.cut_select_algo(path, dim, sel, strat=strat, nb_rounds_cuts=rounds, max_parallel=mp, pool_factor=pool_factor,
                                     on_round=lambda r, log: logs.append(log))
        log, cuts, n_cand = logs[-1], out[4], out[6]
        quota = CutSolver.selection_size(sel, n_cand)
        lines.append("  filter %-9s candidates %d quota %d" % ("none" if mp is None else "cos<=%.1f" % mp, n_cand, quota))
        lines.append("    %5s %14s %6s %9s %9s   %s" % ("round", "bound", "rows", "LP s", "sep s", "pool / examined / not violated / parallel"))
        for r in range(len(log.bounds)):
            info = ""
            if mp is not None and 1 <= r <= len(solver.diverse_log):
                d = solver.diverse_log[r - 1]
                info = "%d / %d / %d / %d (strategy %d)" % (d["pool"], d["examined"], d["skipped_nonviolated"], d["rejected_parallel"], d["strat"])
            lines.append("    %5d %14.4f %6d %9.3f %9.4f   %s" % (r, -log.bounds[r], cuts[r] if r < len(cuts) else 0, log.solve_s[r],
                                                                 log.separation_s[r - 1] if r >= 1 else 0.0, info))
        lines.append("    total rows %d, LP seconds %.3f, separation seconds %.4f" % (sum(cuts), sum(log.solve_s), sum(log.separation_s)))
    return lines


def timing_lines(path, dim, strats, sel, pool_factor, repeats):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi, harness
    from sdpcutsel_via_nn_amd.cut_solver import CutSolver
    inst = harness.parse_boxqp(path)
    n = inst["nb_vars"]
    sc = pkg.Scorer(0)
    lines = []
    try:
        sc.set_builtin_networks(5)
        sc.set_instance(n, np.asarray(inst["Q_arr"], dtype=np.float64))
        n_cand = sc.set_candidates_cover(inst["adj"], dim)
        quota = CutSolver.selection_size(sel, n_cand)
        pool = int(min(max(pool_factor * quota, quota), _capi.DIVERSE_MAX_POOL))
        vv = harness.random_mccormick_point(n, np.random.default_rng(7))

        def median_ms(fn):
            fn()
            ms = []
            for _ in range(repeats):
                t = time.perf_counter()
                fn()
                ms.append(1e3 * (time.perf_counter() - t))
            return float(np.median(ms))
        for strat in strats:
            plain = median_ms(lambda: sc.round_csr(strat, quota, point=vv))
            cells = []
            for mp in (1.0, 0.9, 0.5):
                ms = median_ms(lambda: sc.round_csr_diverse(vv, strat, quota, mp, pool_size=pool))
                r = sc.round_csr_diverse(vv, strat, quota, mp, pool_size=pool)
                cells.append("cos<=%.1f %8.3f ms (%d rows, examined %d)" % (mp, ms, r["rhs"].shape[0], r["info"]["examined"]))
            lines.append("  strategy %d  candidates %8d quota %5d pool %5d | round_csr %8.3f ms | round_csr_diverse: %s"
                         % (strat, n_cand, quota, pool, plain, "; ".join(cells)))
    finally:
        sc.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", nargs="+", default=["spar020-100-1", "spar040-030-1", "spar070-050-1"])
    ap.add_argument("--timing-instances", nargs="*", default=["spar020-100-1", "spar040-030-1", "spar070-050-1", "spar125-075-1"])
    ap.add_argument("--dims", nargs="+", type=int, default=[3])
    ap.add_argument("--strats", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sel", type=float, default=0.1)
    ap.add_argument("--pool-factor", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_rounds.txt"))
    args = ap.parse_args()
    inst_dir = os.path.join(ROOT, "tests", "golden", "instances")
    lines = ["# diverse selection (cut_select_algo(..., max_parallel=, pool_factor=%d)), selection share %.2f, %d rounds; LP: HiGHS"
             % (args.pool_factor, args.sel, args.rounds),
             "# bound = upper bound of the maximisation after the round's LP solve (round 0: the McCormick relaxation)"]

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lines.append("# device time of one round, host to host, median of %d after a warm-up; LP point: a random McCormick point" % args.repeats)
    for name in args.timing_instances:
        for dim in args.dims:
            lines.append("%s dim %d" % (name, dim))
            got = timing_lines(os.path.join(inst_dir, name + ".in"), dim, args.strats, args.sel, args.pool_factor, args.repeats)
            lines += got
            print("\n".join([lines[-len(got) - 1]] + got), flush=True)
            flush()
    for name in args.instances:
        for dim in args.dims:
            for strat in args.strats:
                lines.append("%s dim %d strategy %d" % (name, dim, strat))
                lines += loop_lines(os.path.join(inst_dir, name + ".in"), dim, strat, args.sel, args.rounds, args.pool_factor)
                print("\n".join(lines[-(3 * (args.rounds + 4)):]), flush=True)
                flush()


if __name__ == "__main__":
    main()
