"""All violated eigen-cuts of a selected set in the cutting-plane loop: CutSolver.cut_select_algo with one cut per set (today's
round), with cuts_per_set = 5 under the row budget (at most `quota` rows per round, fewer sets) and under the set budget (`quota`
sets, all the cuts they offer) on BoxQP instances under tests/golden/instances, and the time of a multi-cut round next to the
plain round of the same quota.

    python tools/multi_cuts.py [--instances spar020-100-1 spar040-030-1 spar070-050-1] [--dims 3 4 5] [--strats 1 4] [--rounds 4]
                               [--sel 0.1] [--repeats 9] [--out profiles/multi_cuts.txt]

Per run and round: the LP bound after the round's solve, the rows the round added, the seconds of that LP solve (HiGHS,
harness.LinearRelaxation) and of the separation, and the round's record of CutSolver.multi_log (entries used, violated eigenvalues
per entry, whether the quota dropped a row).
Then, per instance, dim and strategy: host-to-host milliseconds (a host clock around a call that ends in the round's host wait) of
Scorer.round_csr and of Scorer.round_csr_multi at the same quota and LP point (a random McCormick point).  The forms are timed in
the same process, ALTERNATING call by call after a warm-up of each, --repeats calls each: median and (min .. max) per form, so the
run-to-run spread stands next to every difference.

Needs a GPU.  Nothing is asserted: the file is a measurement."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
FORMS = (("one cut per set", 1, None), ("5 per set, row budget", 5, None), ("5 per set, set budget", 5, "sets"))


def loop_lines(path, dim, strat, sel, rounds):
    from sdpcutsel_via_nn_amd.cut_solver import CutSolver
    lines = []
    for label, m, rq in FORMS:
        solver = CutSolver()
        logs = []
        out = solver.cut_select_algo(path, dim, sel, strat=strat, nb_rounds_cuts=rounds, cuts_per_set=m, row_quota=rq,
                                     on_round=lambda r, log: logs.append(log))
        log, cuts, n_cand = logs[-1], out[4], out[6]
        quota = CutSolver.selection_size(sel, n_cand)
        lines.append("  %-24s candidates %d quota %d" % (label, n_cand, quota))
        lines.append("    %5s %14s %6s %9s %9s   %s" % ("round", "bound", "rows", "LP s", "sep s", "entries used / last entry | n_neg histogram 0..5 | quota hit"))
        mlog = getattr(solver, "multi_log", None) or []
        for r in range(len(log.bounds)):
            info = ""
            if m > 1 and 1 <= r <= len(mlog):
                d = mlog[r - 1]
                info = "%d / %d | %s | %s (strategy %d)" % (d["entries_used"], d["last_entry"], " ".join(str(c) for c in d["n_neg_hist"]),
                                                           "yes" if d["quota_hit"] else "no", d["strat"])
            lines.append("    %5d %14.4f %6d %9.3f %9.4f   %s" % (r, log.bounds[r], cuts[r] if r < len(cuts) else 0, log.solve_s[r],
                                                                 log.separation_s[r - 1] if r >= 1 else 0.0, info))
        lines.append("    total rows %d, LP seconds %.3f, separation seconds %.4f" % (sum(cuts), sum(log.solve_s), sum(log.separation_s)))
    return lines


def timing_lines(path, dim, strats, sel, repeats):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
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
        vv = harness.random_mccormick_point(n, np.random.default_rng(7))
        for strat in strats:
            forms = [("round_csr", lambda: sc.round_csr(strat, quota, point=vv)),
                     ("multi m=1", lambda: sc.round_csr_multi(vv, strat, quota, 1)),
                     ("multi m=5 rows", lambda: sc.round_csr_multi(vv, strat, quota, 5)),
                     ("multi m=5 sets", lambda: sc.round_csr_multi(vv, strat, quota, 5, row_quota="sets"))]
            for _, fn in forms:
                for _ in range(3):
                    fn()
            ms = [[] for _ in forms]
            for _ in range(repeats):
                for j, (_, fn) in enumerate(forms):      # alternating: every form sees the same neighbours on the machine
                    t = time.perf_counter()
                    fn()
                    ms[j].append(1e3 * (time.perf_counter() - t))
            rows = [sc.round_csr(strat, quota, point=vv)["rhs"].shape[0]] + [fn()["rhs"].shape[0] for _, fn in forms[1:]]
            cells = ["%s %7.3f ms (%.3f .. %.3f; %d rows)" % (name, float(np.median(v)), min(v), max(v), r)
                     for (name, _), v, r in zip(forms, ms, rows)]
            lines.append("  strategy %d  candidates %8d quota %5d | %s" % (strat, n_cand, quota, " | ".join(cells)))
    finally:
        sc.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", nargs="+", default=["spar020-100-1", "spar040-030-1", "spar070-050-1"])
    ap.add_argument("--timing-instances", nargs="*", default=["spar020-100-1", "spar040-030-1", "spar070-050-1", "spar125-075-1"])
    ap.add_argument("--dims", nargs="+", type=int, default=[3, 4, 5])
    ap.add_argument("--timing-dims", nargs="+", type=int, default=[3, 4])
    ap.add_argument("--strats", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sel", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_cuts.txt"))
    args = ap.parse_args()
    inst_dir = os.path.join(ROOT, "tests", "golden", "instances")
    lines = ["# all violated eigen-cuts (cut_select_algo(..., cuts_per_set=, row_quota=)), selection share %.2f, %d rounds; LP: HiGHS" % (args.sel, args.rounds),
             "# bound = LP value after the round's solve (round 0: the McCormick relaxation); a higher bound is a tighter one"]

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lines.append("# time of one round, host to host: %d alternating calls per form after a warm-up, median (min .. max); LP point: a random McCormick point"
                 % args.repeats)
    for name in args.timing_instances:
        for dim in args.timing_dims:
            lines.append("%s dim %d" % (name, dim))
            got = timing_lines(os.path.join(inst_dir, name + ".in"), dim, args.strats, args.sel, args.repeats)
            lines += got
            print("\n".join([lines[-len(got) - 1]] + got), flush=True)
            flush()
    for name in args.instances:
        for dim in args.dims:
            for strat in args.strats:
                lines.append("%s dim %d strategy %d" % (name, dim, strat))
                got = loop_lines(os.path.join(inst_dir, name + ".in"), dim, strat, args.sel, args.rounds)
                lines += got
                print("\n".join([lines[-len(got) - 1]] + got), flush=True)
                flush()


if __name__ == "__main__":
    main()
