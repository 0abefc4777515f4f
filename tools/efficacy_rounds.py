"""Efficacy ranking (strategy 6) measured on one MI355X: what its scoring launch and its round cost next to the feasibility round
of the same handle, and what the ranking buys in bound per round next to strategies 1, 2 and 4.

    python tools/efficacy_rounds.py [--part a b] [--instances spar040-030-1 spar070-050-1 spar125-075-1] [--rounds 4] [--sel 0.1]
                                    [--repeats 21] [--out profiles/efficacy_rounds.txt]

(a) Per list -- the bench list (10^6 three-variable Philox candidates on n = 1000) and the dim-4 cover of spar125-075-1 at the LP
    point a recorded run separated at in round 3 (tests/golden/rounds_spar125_075_1_d4_s4.npz) -- in ALTERNATING order, medians of
    --repeats after a warm-up of each:
      eff launch   Scorer.score(EFF) + synchronize on a list whose lambda_min is scored already (the efficacy kernel and its launch)
      eig launch   Scorer.score(EIG) + synchronize after set_point (the eigenvalue kernel, for scale)
      round 6 / 1  Scorer.round_csr(strategy, quota, point=...) host to host: point up, scores, selection, rows
    and the share of candidates that are not violated (their lanes leave before the eigenvector).
(b) CutSolver.cut_select_algo at share --sel for --rounds rounds under strategies 1, 2, 4, 6 (w = 0) and 6 (w = 0.1), each with and
    without max_parallel = 0.5, on the dim-3 covers: the bound after every round and the rows added.

Needs a GPU.  Nothing is asserted: the file is a measurement."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
INST = os.path.join(ROOT, "tests", "golden", "instances")
EIG, EFF = 1, 8


def timing_lines(label, sc, vv, quota, repeats):
    def timed(fn, prep=None):
        if prep:
            prep()
        sc.synchronize()
        t = time.perf_counter()
        fn()
        sc.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def eig_prep():
        sc.set_point(vv)

    def eff_prep():
        sc.set_point(vv)
        sc.score(EIG)
    runs = {"eff launch": (lambda: sc.score(EFF), eff_prep), "eig launch": (lambda: sc.score(EIG), eig_prep),
            "round 6": (lambda: sc.round_csr(6, quota, point=vv), None), "round 1": (lambda: sc.round_csr(1, quota, point=vv), None)}
    ms = {k: [] for k in runs}
    for k, (fn, prep) in runs.items():
        timed(fn, prep)                      # warm-up (allocations, the first launch of a kernel)
    for _ in range(repeats):                 # alternating: every pass runs each of them once
        for k, (fn, prep) in runs.items():
            ms[k].append(timed(fn, prep))
    sc.set_point(vv)
    sc.score(EFF)
    eff = sc.get_efficacy()[0]
    r6, r1 = sc.round_csr(6, quota, point=vv), sc.round_csr(1, quota, point=vv)
    return ["%s: %d candidates, quota %d, not violated %.1f %%" % (label, sc.N, quota, 100.0 * float((eff <= 0).mean()))] + \
           ["    %-10s median %8.3f ms   min %8.3f   max %8.3f   (%d samples)" % (k, float(np.median(v)), min(v), max(v), len(v)) for k, v in ms.items()] + \
           ["    rows of the head: strategy 6 %d, strategy 1 %d" % (r6["rhs"].shape[0], r1["rhs"].shape[0])]


def part_a(repeats):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness, synthetic
    lines = []
    sc = pkg.Scorer(0)
    try:
        n = 1000
        Q_arr, _, _ = synthetic.make_instance(n, 7)
        sc.set_instance(n, np.asarray(Q_arr, dtype=np.float64))
        sc.set_candidates_philox(3, 1000000, seed=7)
        vv = harness.random_mccormick_point(n, np.random.default_rng(7))
        lines += timing_lines("bench list (Philox, k = 3, n = 1000, random McCormick point)", sc, vv, 5000, repeats)
        inst = harness.parse_boxqp(os.path.join(INST, "spar125-075-1.in"))
        sc.set_instance(inst["nb_vars"], np.asarray(inst["Q_arr"], dtype=np.float64))
        sc.set_candidates_cover(inst["adj"], 4)
        z = np.load(os.path.join(ROOT, "tests", "golden", "rounds_spar125_075_1_d4_s4.npz"))
        lines += timing_lines("spar125-075-1 dim-4 cover at the recorded LP point of round 3", sc, np.array(z["r03_vars"], dtype=np.float64), 5000, repeats)
    finally:
        sc.close()
    return lines


CONFIGS = ((1, {}), (2, {}), (4, {}), (6, {}), (6, {"objpar_weight": 0.1}))


def part_b(name, sel, rounds):
    from sdpcutsel_via_nn_amd.cut_solver import CutSolver
    lines = ["%s dim 3, share %.2f: bound after the LP solve of round 0 .. %d | rows added per round | LP s | separation s" % (name, sel, rounds)]
    for strat, kw in CONFIGS:
        for mp in (None, 0.5):
            solver, logs = CutSolver(), []
            out = solver.cut_select_algo(os.path.join(INST, name + ".in"), 3, sel, strat=strat, nb_rounds_cuts=rounds, max_parallel=mp,
                                         on_round=lambda r, log: logs.append(log), **kw)
            log = logs[-1]
            tag = "strategy %d%s%s" % (strat, " w=0.1" if kw else "", " cos<=0.5" if mp is not None else "")
            lines.append("    %-26s %s | %s | %.2f | %.4f" % (tag, " ".join("%.3f" % -b for b in log.bounds), " ".join(str(c) for c in out[4][1:]),
                                                              sum(log.solve_s), sum(log.separation_s)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["a", "b"])
    ap.add_argument("--instances", nargs="+", default=["spar040-030-1", "spar070-050-1", "spar125-075-1"])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sel", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "efficacy_rounds.txt"))
    args = ap.parse_args()
    lines = ["# efficacy ranking (strategy 6, SDPCUT_EFF): one MI355X; times host to host in ms, alternating runs, medians of %d" % args.repeats,
             "# bound = upper bound of the maximisation after the round's LP solve (round 0: the McCormick relaxation); LP: HiGHS"]

    def flush(new):
        lines.extend(new)
        print("\n".join(new), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if "a" in args.part:
        flush(part_a(args.repeats))
    if "b" in args.part:
        for name in args.instances:
            flush(part_b(name, args.sel, args.rounds))


if __name__ == "__main__":
    main()
