"""Time one round of dense eigen-cuts (strategy 0) at recorded LP points: the device round host to host (sdpcut_dense_round:
point upload, eigensolver, row assembly into pinned memory, one wait), its two kernels by HIP events, the sweep count -- and, on
the same box, the only way to these cuts without the library: cut_select_qp.py:757-786 restated (numpy.linalg.eigh plus the
per-entry Python comprehension) on the host CPU.

    python tools/dense_round.py [--reps 30] [--warmup 5] [--out profiles/NAME.json]

Prints one JSON line per point; medians over --reps repetitions after --warmup discarded ones."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

POINTS = [("spar070-050-1", 70, "rounds_spar070_050_1_d5_s4.npz", "r01"), ("spar070-050-1", 70, "rounds_spar070_050_1_d5_s4.npz", "r12"),
          ("spar125-075-1", 125, "rounds_spar125_075_1_d3_s2.npz", "r01"), ("spar125-075-1", 125, "rounds_spar125_075_1_d3_s2.npz", "r12")]


def host_reference(vv, n):
    """cut_select_qp.py:757-786 without the LP object -> number of cuts"""
    L = n * (n + 1) // 2
    X_vals, x_vals = list(vv[0:L]), list(vv[L:])
    mat = np.zeros((n + 1, n + 1))
    mat[0, 0] = 1
    mat[0, 1:] = x_vals
    iu = np.triu_indices(n)
    mat[iu[0] + 1, iu[1] + 1] = X_vals
    eigvals, evecs = np.linalg.eigh(mat, "U")
    rows, rhs = [], []
    for ix in range(n):
        if eigvals[ix] < -1e-15:
            v = evecs.T[ix]
            rows.append(([x + L for x in range(n)] + list(range(L)),
                         [v[a] * v[b] * 2 if a != b else v[a] * v[b] for a in range(n + 1) for b in range(max(a, 1), n + 1)]))
            rhs.append(-v[0] * v[0])
    return len(rows)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi, dense
    lines = []
    for inst, n, fname, rnd in POINTS:
        vv = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", fname))[rnd + "_vars"], dtype=np.float64)
        sc = pkg.Scorer(0)
        sc.set_instance(n, np.zeros(n * (n + 1) // 2))
        res = sc.dense_round(vv)
        nb, sweeps = res["n_rows"], res["sweeps"]
        dev = median_ms(lambda: sc.dense_round(vv), args.reps, args.warmup)
        sc.set_option(_capi.OPT_TIMING, 2)
        eig_ms, rows_ms = [], []
        for _ in range(args.reps):
            sc.dense_round(vv)
            a, b = sc.last_timing()
            eig_ms.append(a)
            rows_ms.append(b)
        sc.set_option(_capi.OPT_TIMING, 0)
        eig_only = median_ms(lambda: sc.dense_eig(), args.reps, args.warmup)
        sc.close()
        assert host_reference(vv, n) == nb
        host = median_ms(lambda: host_reference(vv, n), args.host_reps, 1)
        t0 = time.perf_counter()
        for _ in range(args.host_reps):
            np.linalg.eigh(dense.lifted_matrix(vv, n), "U")
        host_eigh = (time.perf_counter() - t0) * 1e3 / args.host_reps
        line = dict(instance=inst, point=rnd, n=n, rows=nb, row_len=n + n * (n + 1) // 2, sweeps=sweeps, reps=args.reps,
                    device_round_ms=dict(median=dev[0], min=dev[1], max=dev[2]), eig_kernel_ms=statistics.median(eig_ms),
                    rows_kernel_ms=statistics.median(rows_ms), device_eig_only_ms=eig_only[0],
                    host_reference_ms=dict(median=host[0], min=host[1], max=host[2], reps=args.host_reps), host_eigh_ms=host_eigh)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
