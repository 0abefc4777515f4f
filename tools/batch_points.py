#!/usr/bin/env python3
"""GPU box: what a separation round costs per LP point when P points of one instance are handed over in ONE call
(Scorer.round_csr_points) against the same P points through a loop of single-point rounds (Scorer.round_csr).

Lists: the spar020-100-1 dim-3 cover (1051 three-variable candidates) and the spar040-030-1 dim-5 cover (sizes 2..5 mixed).
P in {1, 8, 64, 256}, strategies 1 and 4, sel_size = 10 % of the list.  Times are host to host (time.perf_counter around the call,
which ends in the device wait), in ms per call and us per point.

Method: both forms are warmed up at every shape (first launches load code objects); then `--repeats` blocks, each block timing the
batched form and the loop form one after the other (alternating, so that drift of the box hits both), `--calls` calls per timing.
Reported: the median over the blocks and their min .. max (the run-to-run spread on this box during this run).

--boxes: every point lies in a node box of its own (a tree search's open nodes).  batched = round_csr_points(P points, boxes=),
loop = P x (set_box, round_csr(point=p)) on the same handle -- what separate_points(..., boxes=) did before the boxed entry points
existed.  Lists: the dim-3 covers of spar020-100-1 and spar040-030-1; P in {8, 64, 256}; strategies 2 and 4 (strategy 1 reads no
box).  Boxes: per variable a seeded interval of width 0.05 .. 1 inside [0, 1]; points: McCormick-feasible points of the unit box
carried into the box (nodebox.inverse_tables).

--diverse: the filtered round (max_parallel 0.5, sel 100, pool 400; strategies 1, 4 and 6) over P in {8, 64, 256} points of the dim-3
covers of spar020-100-1 and spar040-030-1, without and with a box per point.  batched = round_csr_points_diverse(P points[, boxes=]),
loop = P x ([set_box,] round_csr_diverse(point p)) on the same handle.  Strategy 4 with sel < pool is served by the loop inside the
call (csrc/batch_route.h); a further row times it with sel = pool = 400, where it takes the one-wait route.  Behind each list: the
plain round_csr_points at P = 64 and sel 100, the price of the filter; --plain-only times that alone, and --root DIR takes the
package from another checkout (the parent commit's, built), so that the same tool gives the value before and after a change.

--triangles: the triangle inequalities (Scorer.tri_round_csr_points, Scorer.tri_round_csr), medians of --repeats (default 5) blocks:
  * the batch call against the loop it replaces on the same handle -- P x (set_point, tri_separate, the numpy build of the rows of
    GpuCutSelectionMixin._separate_and_add_triangle), timed together -- at P in {8, 64, 256} McCormick points and heads of 4096
    entries, over the triangle lists (dim-independent) of spar020-100-1, spar040-030-1 and spar070-050-1, without and with a box
    per point (the loop then is P x (set_box, tri_round_csr): there is no older way to a node's rows);
  * tri_round_csr against set_point + tri_separate + the numpy build at one point, spar125-075-1, 10 000 rows;
  * at the depth-1 / depth-2 nodes of tools/node_rounds.py (spar020-100-1, spar040-030-1): the violated inequalities at the node's
    LP point with the unit box's facets and with the node's, and the bound after 4 rounds of cut_select_algo(strat 1, triangle_on)
    with triangle_box off and on.

usage: tools/batch_points.py [--boxes | --diverse | --triangles] [--repeats R] [--calls C] [--loop-only] [--plain-only] [--root DIR] [--out [FILE]]
  --boxes       the boxed batch against the loop of set_box + single-point rounds
  --diverse     the filtered batch against the loop of single-point filtered rounds (default --repeats 5)
  --loop-only   time the single-point loop only (runs on a library without the batched entry points: the parent commit's)
  --out         also write the table to FILE (default profiles/batch_points.txt; with --boxes profiles/boxed_points.txt; with
                --diverse profiles/diverse_points.txt; with --triangles profiles/tri_points.txt)"""
import argparse
import gc
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv[1:-1] else ROOT
sys.path.insert(0, PKG_ROOT)
import sdpcutsel_via_nn_amd as pkg  # noqa: E402
from sdpcutsel_via_nn_amd import _capi, harness, networks, nodebox  # noqa: E402

INST = os.path.join(ROOT, "tests", "golden", "instances")
LISTS = (("spar020-100-1 dim 3", "spar020-100-1.in", 3), ("spar040-030-1 dim 5", "spar040-030-1.in", 5))
POINTS = (1, 8, 64, 256)
BOXED_LISTS = (("spar020-100-1 dim 3", "spar020-100-1.in", 3), ("spar040-030-1 dim 3", "spar040-030-1.in", 3))
BOXED_POINTS = (8, 64, 256)


def seeded_box(n, seed):
    """-> [2, n]: per variable an interval of width 0.05 .. 1 inside the unit interval"""
    rng = np.random.default_rng(7000 + seed)
    w = rng.uniform(0.05, 1.0, n)
    lb = rng.uniform(0.0, 1.0, n) * (1.0 - w)
    return np.stack([lb, np.minimum(lb + w, 1.0)])


def timed(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls


def median_cell(times, P):
    a = np.array(times) * 1e3
    return "%8.4f (%7.4f .. %7.4f) %8.2f" % (np.median(a), a.min(), a.max(), np.median(a) * 1e3 / P)


def diverse_main(args):
    """--diverse / --plain-only: see the module's docstring"""
    sel, pool, mp = 100, 400, 0.5
    lines = ["# tools/batch_points.py --diverse%s --repeats %d: ms per call, us per point; median over the blocks (min .. max)"
             % (" --plain-only" if args.plain_only else "", args.repeats),
             "# batched = round_csr_points_diverse(P points[, boxes=]); loop = P x ([set_box,] round_csr_diverse(point=p)); sel %d, pool %d, "
             "max_parallel %.1f" % (sel, pool, mp),
             "# package: %s" % ("this checkout" if PKG_ROOT == ROOT else "another checkout (--root)")]
    for title, fname, dim in BOXED_LISTS:
        inst = harness.parse_boxqp(os.path.join(INST, fname))
        S, ks, N = _capi.enumerate_cover(inst["adj"], dim)
        n = inst["nb_vars"]
        sc = pkg.Scorer(0)
        for k in (2, 3, 4, 5):
            sc.set_network(k, *networks.load_network(k))
        sc.set_instance(n, inst["Q_arr"])
        sc.set_candidates(S, ks)
        pts_all = np.stack([harness.random_mccormick_point(n, np.random.default_rng(100 + i)) for i in range(max(BOXED_POINTS))])
        boxes_all = np.stack([seeded_box(n, i) for i in range(max(BOXED_POINTS))])
        bpts_all = np.stack([nodebox.inverse_tables(None, pts_all[i], boxes_all[i, 0], boxes_all[i, 1])[1] for i in range(max(BOXED_POINTS))])
        lines.append("")
        lines.append("%s: %d candidates" % (title, N))
        if not args.plain_only:
            sc.set_objective(np.concatenate([np.asarray(inst["Q_arr"], dtype=np.float64), np.asarray(inst["c"], dtype=np.float64)]))
            sc.set_efficacy_weight(0.1)
            lines.append("  strat  sel boxed    P | batched ms/call          us/point | loop ms/call             us/point | loop / batched | one-wait points")
            for strat, q in ((1, sel), (4, sel), (4, pool), (6, sel)):
                for boxed in (False, True):
                    for P in BOXED_POINTS:
                        pts = np.ascontiguousarray((bpts_all if boxed else pts_all)[:P])
                        rows = [pts[p] for p in range(P)]
                        bx = np.ascontiguousarray(boxes_all[:P]) if boxed else None
                        calls = args.calls or max(4, 1024 // P)

                        def loop():
                            for p, v in enumerate(rows):
                                if bx is not None:
                                    sc.set_box(bx[p, 0], bx[p, 1])
                                sc.round_csr_diverse(v, strat, q, mp, pool_size=pool)
                            if bx is not None:
                                sc.clear_box()

                        def batched():
                            sc.round_csr_points_diverse(pts, strat, q, mp, pool_size=pool, boxes=bx)

                        f0 = sc.get_stat(_capi.STAT_DIVERSE_POINTS_FAST)
                        batched()
                        fast = sc.get_stat(_capi.STAT_DIVERSE_POINTS_FAST) - f0
                        for f in (batched, loop):
                            timed(f, max(2, calls // 4))
                        t = {"batched": [], "loop": []}
                        for _ in range(args.repeats):
                            for f in (batched, loop):
                                t[f.__name__].append(timed(f, calls))
                        lines.append("  %5d %4d %5s %4d | %s | %s | %14.2f | %d of %d" % (strat, q, "yes" if boxed else "no", P, median_cell(t["batched"], P),
                                                                                 median_cell(t["loop"], P), np.median(t["loop"]) / np.median(t["batched"]), fast, P))
                        print(lines[-1], flush=True)
            lines.append("  points redone through the single-point round: %d" % sc.get_stat(_capi.STAT_POINTS_REDONE))
            sc.set_objective(None)
        # the price of the filter: the plain batched round of the same points
        lines.append("  plain round_csr_points, P = 64, sel %d:" % sel)
        pts = np.ascontiguousarray(pts_all[:64])
        for strat in (1, 4):
            def plain():
                sc.round_csr_points(pts, strat, sel)
            timed(plain, 16)
            t = [timed(plain, 64) for _ in range(args.repeats)]
            lines.append("  %5d %4d %5s %4d | %s" % (strat, sel, "no", 64, median_cell(t, 64)))
            print(lines[-1], flush=True)
        sc.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def triangles_main(args):
    """--triangles: see the module's docstring"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import node_rounds
    from tri_rows_numpy import numpy_rows as numpy_tri_rows      # the one copy of the loop's host build
    head = 4096
    lines = ["# tools/batch_points.py --triangles --repeats %d: ms per call, us per point; median over the blocks (min .. max)" % args.repeats,
             "# batched = tri_round_csr_points(P points, %d[, boxes=]); loop = P x (set_point, tri_separate(%d), numpy rows); with boxes: P x (set_box, "
             "tri_round_csr)" % (head, head)]

    def handle(fname):
        inst = harness.parse_boxqp(os.path.join(INST, fname))
        sc = pkg.Scorer(0)
        sc.set_instance(inst["nb_vars"], inst["Q_arr"])
        tri, _ = sc.tri_preprocess(inst["adj"])
        return inst, sc, np.asarray(tri, dtype=np.int64)

    for fname in ("spar020-100-1.in", "spar040-030-1.in", "spar070-050-1.in"):
        inst, sc, tri64 = handle(fname)
        n = inst["nb_vars"]
        pts_all = np.stack([harness.random_mccormick_point(n, np.random.default_rng(100 + i)) for i in range(max(BOXED_POINTS))])
        boxes_all = np.stack([seeded_box(n, i) for i in range(max(BOXED_POINTS))])
        bpts_all = np.stack([nodebox.inverse_tables(None, pts_all[i], boxes_all[i, 0], boxes_all[i, 1])[1] for i in range(max(BOXED_POINTS))])
        lines.append("")
        lines.append("%s: %d triples, %d inequalities" % (fname[:-3], tri64.shape[0], 4 * tri64.shape[0]))
        lines.append("  boxed    P | batched ms/call          us/point | loop ms/call             us/point | loop / batched | one-wait points | violated (median)")
        for boxed in (False, True):
            for P in BOXED_POINTS:
                pts = np.ascontiguousarray((bpts_all if boxed else pts_all)[:P])
                bx = np.ascontiguousarray(boxes_all[:P]) if boxed else None
                calls = args.calls or max(4, 512 // P)

                def loop():
                    for p in range(P):
                        if bx is not None:
                            sc.set_box(bx[p, 0], bx[p, 1])
                            sc.tri_round_csr(head, point=pts[p])
                        else:
                            sc.set_point(pts[p])
                            ent, _, _ = sc.tri_separate(head)
                            numpy_tri_rows(tri64, n, ent)
                    if bx is not None:
                        sc.clear_box()

                def batched():
                    return sc.tri_round_csr_points(pts, head, boxes=bx)

                f0 = sc.get_stat(_capi.STAT_TRI_POINTS_FAST)
                nviol = int(np.median([r["n_violated"] for r in batched()]))
                fast = sc.get_stat(_capi.STAT_TRI_POINTS_FAST) - f0
                for f in (batched, loop):
                    timed(f, max(2, calls // 4))
                t = {"batched": [], "loop": []}
                for _ in range(args.repeats):
                    for f in (batched, loop):
                        t[f.__name__].append(timed(f, calls))
                lines.append("  %5s %4d | %s | %s | %14.2f | %d of %d | %d" % ("yes" if boxed else "no", P, median_cell(t["batched"], P), median_cell(t["loop"], P),
                                                                          np.median(t["loop"]) / np.median(t["batched"]), fast, P, nviol))
                print(lines[-1], flush=True)
        sc.close()

    inst, sc, tri64 = handle("spar125-075-1.in")
    n = inst["nb_vars"]
    vv = harness.random_mccormick_point(n, np.random.default_rng(100))

    def device_rows():
        return sc.tri_round_csr(10000, point=vv)

    def host_rows():
        sc.set_point(vv)
        ent, _, _ = sc.tri_separate(10000)
        numpy_tri_rows(tri64, n, ent)

    rows = device_rows()["n_rows"]
    for f in (device_rows, host_rows):
        timed(f, 8)
    t = {"device_rows": [], "host_rows": []}
    for _ in range(args.repeats):
        for f in (device_rows, host_rows):
            t[f.__name__].append(timed(f, args.calls or 32))
    lines.append("")
    lines.append("spar125-075-1: %d triples, one point, %d rows" % (tri64.shape[0], rows))
    lines.append("  tri_round_csr                          ms/call | %s" % median_cell(t["device_rows"], 1))
    lines.append("  set_point + tri_separate + numpy rows  ms/call | %s" % median_cell(t["host_rows"], 1))
    print("\n".join(lines[-3:]), flush=True)
    sc.close()

    lines.append("")
    lines.append("nodes of tools/node_rounds.py: violated inequalities at the node's LP point, bound after 4 rounds (strategy 1, dim 3, sel 0.1, triangle_on)")
    lines.append("  instance        node                                   | violated unit-box  node-box | bound triangle_box off            on")
    for fname in ("spar020-100-1.in", "spar040-030-1.in"):
        inst, sc, _ = handle(fname)
        for name, lb, ub in node_rounds.nodes_of(inst):
            _, vv = node_rounds.solve_node(inst, lb, ub)
            unit = sc.tri_round_csr(0, point=vv)["n_violated"]
            sc.set_box(lb, ub)
            node = sc.tri_round_csr(0, point=vv)["n_violated"]
            sc.clear_box()
            bound = []
            for on in (False, True):
                out = pkg.CutSolver().cut_select_algo(os.path.join(INST, fname), 3, 0.1, strat=1, nb_rounds_cuts=4, triangle_on=True, box=(lb, ub),
                                                      triangle_box=on)
                bound.append(out[0][-1])
            lines.append("  %-15s %-38s | %17d %9d | %24.6f %13.6f" % (fname[:-3], name, unit, node, bound[0], bound[1]))
            print(lines[-1], flush=True)
        sc.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=0)
    ap.add_argument("--diverse", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--calls", type=int, default=0, help="calls per timing (default: about 4096 points' worth, at least 8)")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--boxes", action="store_true")
    ap.add_argument("--triangles", action="store_true")
    ap.add_argument("--out", nargs="?", const="", default=None)
    args = ap.parse_args()
    diverse = args.diverse or args.plain_only
    args.repeats = args.repeats or (5 if diverse or args.triangles else 9)
    if args.triangles:
        if args.out == "":
            args.out = os.path.join(ROOT, "profiles", "tri_points.txt")
        gc.collect()
        gc.freeze()
        return triangles_main(args)
    if args.out == "":
        args.out = os.path.join(ROOT, "profiles", "diverse_points.txt" if diverse else "boxed_points.txt" if args.boxes else "batch_points.txt")
    if diverse:
        gc.collect()
        gc.freeze()
        return diverse_main(args)
    lines = ["# tools/batch_points.py%s --repeats %d%s: ms per call, us per point; median over the blocks (min .. max)"
             % (" --boxes" if args.boxes else "", args.repeats, " --loop-only" if args.loop_only else ""),
             "# batched = round_csr_points(P points, boxes=); loop = P x (set_box, round_csr(point=p)); sel_size = 10 % of the list"
             if args.boxes else "# batched = round_csr_points(P points); loop = P x round_csr(point=p); sel_size = 10 % of the list"]
    gc.collect()
    gc.freeze()
    for title, fname, dim in (BOXED_LISTS if args.boxes else LISTS):
        inst = harness.parse_boxqp(os.path.join(INST, fname))
        S, ks, N = _capi.enumerate_cover(inst["adj"], dim)
        n = inst["nb_vars"]
        sc = pkg.Scorer(0)
        for k in (2, 3, 4, 5):
            sc.set_network(k, *networks.load_network(k))
        sc.set_instance(n, inst["Q_arr"])
        sc.set_candidates(S, ks)
        sel = max(1, int(0.1 * N))
        pts_all = np.stack([harness.random_mccormick_point(n, np.random.default_rng(100 + i)) for i in range(max(POINTS))])
        boxes_all = None
        if args.boxes:
            boxes_all = np.stack([seeded_box(n, i) for i in range(max(POINTS))])
            pts_all = np.stack([nodebox.inverse_tables(None, pts_all[i], boxes_all[i, 0], boxes_all[i, 1])[1] for i in range(max(POINTS))])
        sizes = ", ".join("%d of %d" % (int((ks == k).sum()), k) for k in (2, 3, 4, 5) if (ks == k).any())
        lines.append("")
        lines.append("%s: %d candidates (%s), head %d" % (title, N, sizes, sel))
        lines.append("  strat    P | batched ms/call          us/point | loop ms/call             us/point | loop / batched")
        for strat in ((2, 4) if args.boxes else (1, 4)):
            for P in (BOXED_POINTS if args.boxes else POINTS):
                pts = np.ascontiguousarray(pts_all[:P])
                rows = [pts[p] for p in range(P)]
                bx = np.ascontiguousarray(boxes_all[:P]) if args.boxes else None
                calls = args.calls or max(8, 4096 // P)

                def loop():
                    if bx is None:
                        for v in rows:
                            sc.round_csr(strat, sel, point=v)
                    else:
                        for p, v in enumerate(rows):
                            sc.set_box(bx[p, 0], bx[p, 1])
                            sc.round_csr(strat, sel, point=v)
                        sc.clear_box()

                def batched():
                    sc.round_csr_points(pts, strat, sel, boxes=bx)

                forms = [loop] if args.loop_only else [batched, loop]
                for f in forms:                      # warm-up at this shape
                    timed(f, max(4, calls // 4))
                t = {f.__name__: [] for f in forms}
                for _ in range(args.repeats):
                    for f in forms:
                        t[f.__name__].append(timed(f, calls))

                def cell(name):
                    a = np.array(t[name]) * 1e3
                    return "%8.4f (%7.4f .. %7.4f) %8.2f" % (np.median(a), a.min(), a.max(), np.median(a) * 1e3 / P)
                if args.loop_only:
                    lines.append("  %5d %4d | %-40s | %s |" % (strat, P, "-", cell("loop")))
                else:
                    ratio = np.median(t["loop"]) / np.median(t["batched"])
                    lines.append("  %5d %4d | %s | %s | %6.2f" % (strat, P, cell("batched"), cell("loop"), ratio))
                print(lines[-1], flush=True)
        if not args.loop_only:
            lines.append("  points redone through the single-point round: %d, selection fallbacks: %d"
                         % (sc.get_stat(_capi.STAT_POINTS_REDONE), sc.get_stat(_capi.STAT_SELECT_FALLBACKS)))
        sc.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
