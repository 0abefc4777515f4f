"""Cut pool in the cutting-plane loop: CutSolver.cut_select_algo without a pool (the loop as it was: the baseline) and with
pool_max_age in {2, 4} on BoxQP instances under tests/golden/instances.

    python tools/cut_pool.py [--runs spar070-050-1:5 spar125-075-1:3 spar125-075-1:4] [--strats 1 4] [--ages none 2 4]
                             [--rounds 5] [--sel 0.1] [--budget-s 600] [--out profiles/cut_pool.txt]

Per run and round: the LP bound after the round's solve, the rows of the LP that was solved, the seconds of that solve (HiGHS,
harness.LinearRelaxation), the rows the round added and -- with a pool -- the rows that left and returned, the rows parked
afterwards and the milliseconds of the pool step, host to host.  A run whose LP seconds pass --budget-s is stopped after the
round that passed it and says so; the file is rewritten after every run, so a killed tool leaves what it measured.

Needs a GPU.  Nothing is asserted: the file is a measurement."""
import argparse
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


class _Stop(Exception):
    pass


def run_lines(path, dim, strat, age, sel, rounds, budget_s):
    from sdpcutsel_via_nn_amd.cut_solver import CutSolver
    solver = CutSolver()
    logs = []

    def on_round(r, log):
        logs.append(log)
        if sum(log.solve_s) > budget_s and r < rounds:
            raise _Stop()
    stopped = False
    try:
        solver.cut_select_algo(path, dim, sel, strat=strat, nb_rounds_cuts=rounds, pool_max_age=age, on_round=on_round)
    except _Stop:
        stopped = True
    log = logs[-1]
    plog = getattr(solver, "pool_log", None) if age is not None else None
    lines = ["  pool_max_age %-4s" % ("none" if age is None else age),
             "    %5s %14s %8s %9s %7s %7s %7s %8s %9s" % ("round", "bound", "LP rows", "LP s", "added", "left", "back", "parked", "step ms")]
    final = solver._my_prob.linear_constraints.get_num()
    added_all = [c["sdp"] + c.get("tri", 0) for c in log.counts]
    for r in range(len(log.bounds)):
        added = added_all[r] if r < len(added_all) else 0
        if plog is not None and r < len(plog):
            rec = plog[r]
            lines.append("    %5d %14.4f %8d %9.3f %7d %7d %7d %8d %9.3f" % (r, -log.bounds[r], rec["lp_rows"], log.solve_s[r], rec["added"],
                                                                            rec["leave"], rec["enter"], rec["parked"], rec["step_ms"]))
        else:
            lines.append("    %5d %14.4f %8d %9.3f %7d" % (r, -log.bounds[r], final - sum(added_all[r:]), log.solve_s[r], added))
    lines.append("    LP rows at the end %d, LP seconds %.3f, separation seconds %.4f%s"
                 % (final, sum(log.solve_s), sum(log.separation_s),
                    "   STOPPED after round %d: LP seconds passed the budget, later rounds not measured" % (len(log.bounds) - 1) if stopped else ""))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", nargs="+", default=["spar070-050-1:5", "spar125-075-1:3", "spar125-075-1:4"], help="instance:dim")
    ap.add_argument("--strats", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--ages", nargs="+", default=["none", "2", "4"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sel", type=float, default=0.1)
    ap.add_argument("--budget-s", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_pool.txt"))
    a = ap.parse_args()
    lines = ["# cut pool (cut_select_algo(..., pool_max_age=, pool_drop_age=10, pool_return=None)), selection share %.2f, %d rounds; LP: HiGHS" % (a.sel, a.rounds),
             "# bound = upper bound of the maximisation after the round's LP solve (round 0: the McCormick relaxation); LP rows = rows of the LP",
             "# that solve saw (with a pool; the plain loop only grows); left / back = rows the pool step took out of / returned to the LP",
             "# before the round's separation; step ms = the pool step, host to host.  pool_max_age none = the loop without a pool"]
    for run in a.runs:
        name, dim = run.split(":")
        path = os.path.join(ROOT, "tests", "golden", "instances", name + ".in")
        for strat in a.strats:
            lines.append("%s dim %s strategy %d" % (name, dim, strat))
            for age in a.ages:
                lines += run_lines(path, int(dim), strat, None if age == "none" else int(age), a.sel, a.rounds, a.budget_s)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
                print("\n".join(lines[-(a.rounds + 4):]), flush=True)


if __name__ == "__main__":
    main()
