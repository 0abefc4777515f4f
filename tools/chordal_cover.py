"""Covers on the chordal extension for the BoxQP instances under tests/golden/instances: our counts for ch_ext 1 (P^bar(E)_3) and
ch_ext 2 (bar(P*_3)) under the default elimination order next to the published nb_subproblems (the reference orders with
cvxopt's AMD, so the counts differ), the fill, and the host-to-host time of the device enumeration
(Scorer.set_candidates_cover(..., ch_ext=c): extension on the host + upload + count, scan and write kernels + the wait).

    python tools/chordal_cover.py [--out profiles/chordal_cover.txt] [--repeats 5]

Needs a GPU.  Nothing asserts the times; the counts are checked against the host enumeration."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chordal_cover.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi, harness
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "published_chordal_counts.csv")) as f:
        published = {r["filename"]: (int(r["nb_subproblems_PbarE3"]), int(r["nb_subproblems_barP3star"])) for r in csv.DictReader(f)}
    lines = ["# covers on the chordal extension, dim 3; order: greedy minimum degree (ours) vs cvxopt AMD (published)",
             "# time: host-to-host ms of Scorer.set_candidates_cover(adj, 3, ch_ext=c), median of %d after one warm-up call" % args.repeats,
             "%-16s %5s %6s %6s | %9s %9s %8s | %9s %9s %8s | %9s %8s" % ("instance", "n", "edges", "fill", "PbarE3", "published", "ms", "barP3star",
                                                                          "published", "ms", "P^E_3", "ms")]
    for path in sorted(glob.glob(os.path.join(golden, "instances", "spar*.in"))):
        name = os.path.basename(path)[:-3]
        inst = harness.parse_boxqp(path)
        n, adj = inst["nb_vars"], inst["adj"]
        fill = _capi.chordal_extension(adj)[2]
        sc = pkg.Scorer(0)
        sc.set_instance(n, inst["Q_arr"])
        cells = {}
        for c in (1, 2, 0):
            want = _capi.enumerate_cover(adj, 3, ch_ext=c)[2]
            sc.set_candidates_cover(adj, 3, ch_ext=c)
            ms = []
            for _ in range(args.repeats):
                t = time.perf_counter()
                got = sc.set_candidates_cover(adj, 3, ch_ext=c)
                ms.append(1e3 * (time.perf_counter() - t))
            if got != want:
                raise SystemExit("%s ch_ext %d: device %d, host %d" % (name, c, got, want))
            cells[c] = (got, float(np.median(ms)))
        sc.close()
        pub = published.get(name, (-1, -1))
        lines.append("%-16s %5d %6d %6d | %9d %9d %8.3f | %9d %9d %8.3f | %9d %8.3f"
                     % (name, n, int(np.triu(adj, 1).sum()), fill, cells[1][0], pub[0], cells[1][1], cells[2][0], pub[1], cells[2][1],
                        cells[0][0], cells[0][1]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
