"""Branch and cut on the batched node calls, and the node evaluation call itself.

    python tools/tree_search.py [--instances spar020-100-1 spar040-030-1 spar070-050-1] [--limits 10 15 20] [--max-nodes 2000]
                                [--strats 1 2 4] [--sel 0.1] [--batch 16] [--repeats 5] [--out profiles/tree_search.txt]

1. Scorer.node_eval_points at P = 8 / 64 / 256 points of spar040-030-1 (the root LP point moved a tenth of the way towards seeded
   random McCormick points, node boxes of random widths around them): per point, host to host, against the numpy twin on the same
   input and against a loop of P one-point calls on the same handle; medians of --repeats blocks.
2. The six tiny dense instances of the tests (tests/boxqp_truth.py) with the configuration of tests/test_gpu_tree.py: nodes, status,
   bounds against the exact optimum.
3. CutSolver.branch_and_cut on the --instances, each under its --limits seconds and --max-nodes, for the --strats with node boxes on
   and off and the triangle inequalities of the node's box or of the root's: nodes, status, final gap, and the seconds of the LP
   solves, the separation calls and the evaluation calls.

Needs a GPU.  Nothing is asserted: the file is a measurement.  A part that was not run says so."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
INSTANCES = os.path.join(ROOT, "tests", "golden", "instances")


def timed(fn, repeats, budget_s=0.2):
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


def close(cs):
    for b in (getattr(cs, "_gpu_bindings", None) or {}).values():
        b.drain()
        b.scorer.close()
    for a in ("_gpu_tri", "_gpu_tri_points"):
        if getattr(cs, a, None) is not None:
            getattr(cs, a).close()


def eval_lines(repeats, Ps):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness, nodeeval
    inst = harness.parse_boxqp(os.path.join(INSTANCES, "spar040-030-1.in"))
    n = inst["nb_vars"]
    lp = harness.boxqp_relaxation(inst)
    lp.solve()
    root = np.array(lp.get_values())
    obj = np.array(lp.obj)
    sc = pkg.Scorer(0)
    sc.set_instance(n, np.asarray(inst["Q_arr"], dtype=np.float64))
    sc.set_objective(obj)
    lines = ["node_eval_points on spar040-030-1 (n = %d), max_sweeps 50, rule 1: ms per call, us per point; median over %d blocks (min .. max)" % (n, repeats),
             "      P | device ms/call             us/point | twin ms/call               us/point | loop of 1-point calls ms   us/point | sweeps (median)"]
    try:
        for P in Ps:
            pts = np.stack([0.9 * root + 0.1 * harness.random_mccormick_point(n, np.random.default_rng(100 + p)) for p in range(P)])
            rng = np.random.default_rng(P)
            x = pts[:, -n:]
            lb = np.clip(x - 0.02 - 0.3 * rng.random((P, n)), 0.0, 1.0)
            ub = np.clip(x + 0.02 + 0.3 * rng.random((P, n)), 0.0, 1.0)
            bx = np.stack([lb, ub], axis=1)
            out = sc.node_eval_points(pts, bx)
            rows = [(pts[p:p + 1], bx[p:p + 1]) for p in range(P)]

            def loop():
                for a, b in rows:
                    sc.node_eval_points(a, b)
            d = timed(lambda: sc.node_eval_points(pts, bx), repeats)
            t = timed(lambda: nodeeval.node_eval_points(obj, pts, bx), repeats)
            lo = timed(loop, repeats)
            lines.append("   %4d | %9.4f (%9.4f .. %9.4f) %9.2f | %9.3f (%9.3f .. %9.3f) %9.2f | %9.4f (%9.4f .. %9.4f) %9.2f | %d"
                         % (P, d[0], d[1], d[2], 1e3 * d[0] / P, t[0], t[1], t[2], 1e3 * t[0] / P, lo[0], lo[1], lo[2], 1e3 * lo[0] / P,
                            int(np.median(out["sweeps"]))))
    finally:
        sc.close()
    return lines


def tiny_lines(tmp):
    import boxqp_truth as bt
    import sdpcutsel_via_nn_amd as pkg
    lines = ["the six tiny dense instances (tests/boxqp_truth.py), dim 3, strategy 2 with up to 10 cuts, node boxes, box triangles, batch 8, rounds 2, cap 400 nodes",
             "    n seed | status      nodes |          lower          upper          truth | lp failures | lp s  separate s  evaluate s"]
    for n, seed in bt.PROTOTYPES:
        inst, truth, _ = bt.truth_of(n, seed)
        path = os.path.join(tmp, "tiny_%d_%d.in" % (n, seed))
        bt.write_boxqp(path, inst)
        cs = pkg.CutSolver()
        try:
            r = cs.branch_and_cut(path, 3, 10, strat=2, batch=8, max_nodes=400)
        finally:
            close(cs)
        lines.append("   %2d %4d | %-10s %6d | %14.9f %14.9f %14.9f | %11d | %5.2f %10.2f %10.2f"
                     % (n, seed, r.status, r.nodes, r.lower, r.upper, truth, r.lp_failures, r.seconds["lp"], r.seconds["separate"], r.seconds["evaluate"]))
    return lines


def tree_lines(name, limit, args, flush):
    import sdpcutsel_via_nn_amd as pkg
    path = os.path.join(INSTANCES, name + ".in")
    lines = ["%s: at most %g s and %d nodes per run; dim 3, sel %g, batch %d, rounds 2, up to 1000 triangle rows per node and round" % (name, limit, args.max_nodes, args.sel, args.batch),
             "  strat boxes tri_box | status      nodes |      value (file's sense)          bound        gap |   lp s  separate s  evaluate s    total s"]
    for strat in args.strats:
        for boxes in (True, False):
            for tri_box in (True, False):
                cs = pkg.CutSolver()
                try:
                    r = cs.branch_and_cut(path, 3, args.sel, strat=strat, boxes=boxes, triangle_box=tri_box, batch=args.batch, max_nodes=args.max_nodes,
                                          time_limit=limit)
                finally:
                    close(cs)
                v, b = r.instance_bounds
                s = r.seconds
                lines.append("  %5d %5s %7s | %-10s %6d | %25.6f %14.6f %10.3e | %6.2f %11.2f %11.2f %10.2f"
                             % (strat, "on" if boxes else "off", "on" if tri_box else "off", r.status, r.nodes, v, b, r.gap, s["lp"], s["separate"], s["evaluate"], s["total"]))
                flush(lines)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", nargs="*", default=["spar020-100-1", "spar040-030-1", "spar070-050-1"])
    ap.add_argument("--limits", nargs="*", type=float, default=[10.0, 15.0, 20.0])
    ap.add_argument("--max-nodes", type=int, default=2000)
    ap.add_argument("--strats", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--sel", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", nargs="*", type=int, default=[8, 64, 256])
    ap.add_argument("--no-tiny", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_search.txt"))
    args = ap.parse_args()
    import tempfile
    done = ["# tools/tree_search.py " + " ".join(sys.argv[1:]), ""]

    def flush(pending=()):
        with open(args.out, "w") as f:
            f.write("\n".join(done + list(pending)) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    done += (eval_lines(args.repeats, args.points) if args.points else ["node_eval_points timing: not run"]) + [""]
    flush()
    if args.no_tiny:
        done += ["the six tiny instances: not run", ""]
    else:
        with tempfile.TemporaryDirectory() as tmp:
            done += tiny_lines(tmp) + [""]
    flush()
    for k, name in enumerate(args.instances):
        limit = args.limits[min(k, len(args.limits) - 1)]
        done += tree_lines(name, limit, args, flush) + [""]
        flush()
    if not args.instances:
        done += ["tree runs on the spar instances: not run", ""]
        flush()
    print("\n".join(done))


if __name__ == "__main__":
    main()
