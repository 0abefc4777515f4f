"""Node boxes in cutting-plane rounds at the nodes of a small branch-and-bound tree: the bound per round and the time per round of
the boxed optimality measure (Scorer.set_box) next to today's behaviour at a node -- the same node LP, the unit-box measure.

    python tools/node_rounds.py [--instances spar040-030-1 spar070-050-1 spar125-075-1] [--dim 3] [--strats 2 4] [--rounds 4]
                                [--sel 0.1] [--out profiles/node_rounds.txt]

Nodes: the two children of the root after branching on the variable with the largest X_ii - x_i^2 at the root LP point (at x_i,
kept 2^-10 away from the bounds), then each child branched once more the same way at its own LP point: 2 + 4 nodes per instance.
Per node and strategy both modes run --rounds rounds on their own copy of the node relaxation (harness.boxqp_relaxation(inst, lb,
ub)), alternating round by round in one process: "boxed" with the node's box set on its handle, "ignored" on a handle without a
box.  Recorded per round: the LP bound after the round's solve, the rows added, and the milliseconds of Scorer.round_csr, host to
host (LP point in, CSR block out).  The comparison is between the two modes of the same list in the same run.

Needs a GPU.  Nothing is asserted: the file is a measurement."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
MIN_WIDTH = 2.0 ** -10


def solve_node(inst, lb, ub):
    from sdpcutsel_via_nn_amd import harness
    lp = harness.boxqp_relaxation(inst, lb, ub)
    lp.solve()
    return lp, np.asarray(lp.get_values(), dtype=np.float64)


def branch(inst, lb, ub, vv):
    """-> (i, value): the variable with the largest X_ii - x_i^2 at the LP point and where it is split; None if no split fits"""
    n = inst["nb_vars"]
    L = n * (n + 1) // 2
    idx = np.arange(n)
    x = vv[L:]
    gap = vv[n * idx - idx * (idx - 1) // 2] - x * x
    gap[ub - lb < 4 * MIN_WIDTH] = -np.inf
    i = int(np.argmax(gap))
    if not np.isfinite(gap[i]):
        return None
    return i, float(np.clip(x[i], lb[i] + MIN_WIDTH, ub[i] - MIN_WIDTH))


def nodes_of(inst):
    """[(name, lb, ub)]: depth 1 (2 nodes) and depth 2 (4 nodes)"""
    n = inst["nb_vars"]
    out, frontier = [], [("", np.zeros(n), np.ones(n))]
    for depth in (1, 2):
        nxt = []
        for name, lb, ub in frontier:
            _, vv = solve_node(inst, lb, ub)
            b = branch(inst, lb, ub, vv)
            if b is None:
                continue
            i, val = b
            for side in ("L", "R"):
                l2, u2 = lb.copy(), ub.copy()
                if side == "L":
                    u2[i] = val
                else:
                    l2[i] = val
                nxt.append(("%s%s(x%d@%.4f)" % (name + "/" if name else "", side, i, val), l2, u2))
        out += nxt
        frontier = nxt
    return out


def node_lines(inst, scorers, quota, name, lb, ub, strat, rounds):
    lines = ["  node %s  strategy %d" % (name, strat)]
    modes = ("boxed", "ignored")
    scorers[0].set_box(lb, ub)
    lps = [solve_node(inst, lb, ub) for _ in modes]
    cur = [strat, strat]
    rec = [[(-lps[m][0].get_objective_value(), 0, 0.0, strat)] for m in range(2)]
    for _ in range(rounds):
        for m in range(2):      # the two modes alternate
            lp, vv = lps[m]
            t = time.perf_counter()
            r = scorers[m].round_csr(cur[m], quota, point=vv)
            ms = (time.perf_counter() - t) * 1e3
            rows = int(r["rhs"].shape[0])
            used = cur[m]
            if cur[m] == 4:
                cur[m] = r["new_strat"]
            if rows:
                lp.linear_constraints.add_csr(r["indptr"].astype(np.int64), r["indices"].astype(np.int64), r["values"].copy(), r["rhs"].copy(), "G")
            lp.solve()
            lps[m] = (lp, np.asarray(lp.get_values(), dtype=np.float64))
            rec[m].append((-lp.get_objective_value(), rows, ms, used))
    scorers[0].clear_box()
    lines.append("    %5s | %14s %6s %9s %5s | %14s %6s %9s %5s" % (("round",) + ("bound", "rows", "round ms", "strat") * 2))
    lines.append("    %5s | %-37s | %-37s" % ("", modes[0], modes[1]))
    for r in range(rounds + 1):
        a, b = rec[0][r], rec[1][r]
        lines.append("    %5d | %14.4f %6d %9.3f %5d | %14.4f %6d %9.3f %5d" % ((r,) + a + b))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", nargs="+", default=["spar040-030-1", "spar070-050-1", "spar125-075-1"])
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--strats", nargs="+", type=int, default=[2, 4])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sel", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_rounds.txt"))
    args = ap.parse_args()
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    from sdpcutsel_via_nn_amd.cut_solver import CutSolver
    lines = ["node boxes: bound (as the loop reports it, -LP value) and Scorer.round_csr milliseconds per round, boxed measure against the",
             "unit-box measure on the same node LP; dim %d, sel %g, %d rounds" % (args.dim, args.sel, args.rounds), ""]
    for name in args.instances:
        inst = harness.parse_boxqp(os.path.join(ROOT, "tests", "golden", "instances", name + ".in"))
        scorers = [pkg.Scorer(0), pkg.Scorer(0)]
        try:
            for sc in scorers:
                sc.set_builtin_networks(5)
                sc.set_instance(inst["nb_vars"], np.asarray(inst["Q_arr"], dtype=np.float64))
                n_cand = sc.set_candidates_cover(inst["adj"], args.dim)
            quota = CutSolver.selection_size(args.sel, n_cand)
            lines.append("%s: n %d, candidates %d, quota %d" % (name, inst["nb_vars"], n_cand, quota))
            for node, lb, ub in nodes_of(inst):
                for strat in args.strats:
                    lines += node_lines(inst, scorers, quota, node, lb, ub, strat, args.rounds)
            lines.append("")
        finally:
            for sc in scorers:
                sc.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
