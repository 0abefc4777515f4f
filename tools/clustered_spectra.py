#!/usr/bin/env python3
"""Accuracy of lambda_min and of the cut rows at multiple and nearly multiple smallest eigenvalues, measured against exact spectra.

Walks the inputs of tests/spectra_cases.py through the checks of tests/test_gpu_clustered_spectra.py without stopping at a missed
bound and prints, per family and k, the maxima of four quantities for LAPACK (numpy.linalg.eigvalsh / eigh) and for every device
path: |lambda - mu| / s, the residual ||M B - rho B||_max / max(||M||_max, 1), 1 - <B, P_cluster> and the orthogonality defect
<B_r, B_s> of two rows of one entry.  Needs the GPU.

    python tools/clustered_spectra.py > profiles/clustered_spectra.txt
"""
import contextlib
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(make_scorer=None):
    import spectra_cases as sc
    import test_gpu_clustered_spectra as t
    from oracle import cutsel_oracle as oracle
    if make_scorer is None:
        import sdpcutsel_via_nn_amd as pkg
        make_scorer = lambda: pkg.Scorer(0)      # noqa: E731
    t.STRICT = False
    h = make_scorer()
    h.set_builtin_networks(5)
    broken = []
    for k in sc.KS:
        for fn, args in ((t.test_lambda_min_against_the_exact_spectrum, (h, k)),
                         (t.test_single_cut_rows_against_the_exact_eigenspaces, (h, oracle, k)),
                         (t.test_multi_cut_rows_against_the_exact_eigenspaces, (h, k)),
                         (t.test_eig_batch_against_the_exact_spectrum, (h, k))):
            t0 = time.time()
            try:
                with contextlib.redirect_stdout(sys.stderr):
                    fn(*args)
            except AssertionError as e:
                broken.append((fn.__name__, k, repr(e)[:400]))
            print("# %s[%d]: %.1f s" % (fn.__name__, k, time.time() - t0), file=sys.stderr, flush=True)
    h.close()
    per, fam = sc.lapack_maxima()
    bound = t.resid_bounds()
    print("Clustered spectra: maxima per family and k against the exact spectrum (tools/clustered_spectra.py)")
    print("inputs: tests/spectra_cases.py, %s matrices; s = 1 + 2 sum|x| + 2 sum|X|" % ", ".join("k=%d: %d" % (k, len(sc.cases(k))) for k in sc.KS))
    print("residual bound of the tests (32 x LAPACK's family maximum): %s; documented bound of the inverse iteration: 1e-12"
          % ", ".join("%s %.2e" % (f, bound[f]) for f in sorted(bound)))
    print()
    print("%-3s %-2s %-22s %12s %12s %12s %12s" % ("fam", "k", "path", "|lam-mu|/s", "residual", "1-<B,P>", "<B_r,B_s>"))
    paths = sorted({p for p, _, _ in t.MEASURED})
    for f in sc.FAMILIES:
        for k in sc.KS:
            if (f, k) not in per:
                continue
            print("%-3s %-2d %-22s %12.2e %12.2e %12.2e %12.2e" % ((f, k, "LAPACK") + per[(f, k)]))
            for p in paths:
                if (p, f, k) in t.MEASURED:
                    print("%-3s %-2d %-22s %12.2e %12.2e %12.2e %12.2e" % ((f, k, p) + tuple(t.MEASURED[(p, f, k)])))
    print()
    print("bounds missed: %d" % len(t.MISSED))
    for m in t.MISSED[:200]:
        print("  ", m)
    print("checks that stopped: %d" % len(broken))
    for b in broken:
        print("  ", b)
    return len(t.MISSED) + len(broken)


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
