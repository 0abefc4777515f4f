"""Rate of the exact-SDP optimality measure on the device, host to host: candidates per second of score(SDP) on the four golden
covers (point already on the device; the call, then a wait for the handle's stream) and of sdp_batch per k (inputs up, solve,
value and gap down) on the 4096 golden inputs tiled to --batch.  The reference's per-candidate MOSEK call takes 0.63-1.43 ms
(the paper's table2.csv).

    python tools/exact_sdp_rate.py [--reps 20] [--warmup 3] [--batch 262144] [--out profiles/exact_sdp_rate.txt]

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  One JSON line per step; medians over --reps repetitions after --warmup."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
COVERS = ["spar020_100_1_d3", "spar020_100_1_d4", "spar040_030_1_d5", "spar030_060_1_d3"]
STEP_LIMIT_S = 120


def median_s(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def step_cover(tag, reps, warmup):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    z = np.load(os.path.join(GOLDEN, "inst_boxqp.npz"))
    sc = pkg.Scorer(0)
    sc.set_instance(int(z[tag + "_nb_vars"]), z[tag + "_Q_arr"])
    sc.set_candidates(z[tag + "_set_inds"], z[tag + "_k"])
    sc.set_point(z[tag + "_mck_vars"])

    def once():
        sc.score(_capi.SDP)
        sc.synchronize()
    s = median_s(once, reps, warmup)
    N = int(z[tag + "_k"].shape[0])
    ks = np.bincount(z[tag + "_k"], minlength=6)[2:].tolist()
    return dict(step="score_sdp", cover=tag, candidates=N, per_size=ks, ms=s * 1e3, candidates_per_s=N / s, us_per_candidate=s / N * 1e6,
                unconverged=sc.get_stat(_capi.STAT_SDP_UNCONVERGED))


def step_batch(k, count, reps, warmup):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    inp = np.load(os.path.join(GOLDEN, "nn_k%d.npz" % k))["inputs"]
    inp = np.ascontiguousarray(np.tile(inp, ((count + inp.shape[0] - 1) // inp.shape[0], 1))[:count])
    sc = pkg.Scorer(0)
    s = median_s(lambda: sc.sdp_batch(k, inp), reps, warmup)
    return dict(step="sdp_batch", k=k, candidates=count, ms=s * 1e3, candidates_per_s=count / s, us_per_candidate=s / count * 1e6,
                unconverged=sc.get_stat(_capi.STAT_SDP_UNCONVERGED))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--out")
    ap.add_argument("--step", help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        kind, arg = a.step.split(":")
        res = step_cover(arg, a.reps, a.warmup) if kind == "cover" else step_batch(int(arg), a.batch, a.reps, a.warmup)
        print(json.dumps(res))
        return 0
    lines = []
    for step in ["cover:" + t for t in COVERS] + ["batch:%d" % k for k in (2, 3, 4, 5)]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--warmup", str(a.warmup), "--batch", str(a.batch)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S, universal_newlines=True)
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: stopping" % (step, STEP_LIMIT_S), file=sys.stderr)
            return 1
        if p.returncode != 0:
            print("step %s failed with status %d: stopping" % (step, p.returncode), file=sys.stderr)
            return 1
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
