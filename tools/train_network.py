"""Train the optimality estimator's networks on the device: sample (networks.sample_table1), label (Scorer.sdp_batch), train
(networks.train with the Scorer as back end) for k = 2..5 at the reference's architectures (train_NNs.m:35-40).

    python tools/train_network.py [--samples 16384] [--epochs 300] [--reps 20] [--ks 2,3,4,5] [--out profiles/train_network.txt]

Per k one JSON line: ms per gradient evaluation (a train_loss_grad call over the training part, host to host, median of --reps),
ms per SCG iteration (wall time of train() / iterations: two gradient evaluations, one forward pass over the validation part and
the host's vector arithmetic), the final validation MSE and the SHIPPED network's MSE on the same validation samples, both in the
trained network's normalised units.  Every k runs in a child process of its own under its own time limit; the first step that
fails or runs out of time ends the run (nothing more is started on the device)."""
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
HIDDEN = {2: (50, 50, 50), 3: (50, 50, 50), 4: (64, 64, 64), 5: (64, 64, 64, 64)}      # train_NNs.m:35-40
STEP_LIMIT_S = 240


def step(k, samples, epochs, reps, seed):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import networks
    sc = pkg.Scorer(0)
    X = networks.sample_table1(k, samples, seed=seed)
    t0 = time.perf_counter()
    t = sc.sdp_batch(k, X)[0]
    label_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    widths, params, rep = networks.train(k, X, t, hidden=HIDDEN[k], scorer=sc, epochs=epochs, seed=seed)
    train_s = time.perf_counter() - t0
    first, n_tr = rep["split"]["train"]
    times = []
    for i in range(reps + 3):
        t0 = time.perf_counter()
        sc.train_loss_grad(k, widths, params, first, n_tr)
        if i >= 3:
            times.append(time.perf_counter() - t0)
    v0, n_va = rep["split"]["val"]
    Xv, tv = X[rep["perm"]][v0:v0 + n_va], t[rep["perm"]][v0:v0 + n_va]
    shipped = networks.forward_twin(k, *networks.load_network(k), Xv)
    sc.set_network(k, widths, params)      # the result is a network the library accepts
    own = sc.nn_batch(k, Xv)
    y_gain = params[-2]
    sc.close()
    return dict(k=k, hidden=list(HIDDEN[k]), samples=samples, train_samples=n_tr, label_ms=label_s * 1e3,
                ms_per_grad_eval=statistics.median(times) * 1e3, ms_per_scg_iteration=train_s / max(rep["iterations"], 1) * 1e3,
                iterations=rep["iterations"], grad_evals=rep["grad_evals"], stop=rep["stop"], best_iteration=rep["best_iteration"],
                val_mse=rep["best_val_loss"], val_mse_from_nn_batch=float(np.mean(((own - tv) * y_gain) ** 2)),
                shipped_val_mse=float(np.mean(((shipped - tv) * y_gain) ** 2)), test_mse=rep["test_loss"],
                unclamped_ok=rep["unclamped_ok"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ks", default="2,3,4,5")
    ap.add_argument("--out")
    ap.add_argument("--step", type=int, help="internal: run one k in this process")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, a.samples, a.epochs, a.reps, a.seed)))
        return 0
    lines = []
    for k in [int(v) for v in a.ks.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(k), "--samples", str(a.samples), "--epochs", str(a.epochs),
               "--reps", str(a.reps), "--seed", str(a.seed)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S, universal_newlines=True)
        except subprocess.TimeoutExpired:
            print("k = %d ran out of its %d s: stopping" % (k, STEP_LIMIT_S), file=sys.stderr)
            return 1
        if p.returncode != 0:
            print("k = %d failed with status %d: stopping" % (k, p.returncode), file=sys.stderr)
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
