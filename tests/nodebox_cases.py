"""Instances, seeded boxes and LP points of the node-box tests (test_node_box_cpu.py, test_gpu_node_box.py).  A plain module: no
fixtures, no GPU.

Instances: spar020-100-1 at dim 3 (n = 20, 1051 sets, one size class) and spar040-030-1 at dim 5 (142 sets, k = 2..5 mixed).
Boxes: per variable one of four kinds in turn from a seeded permutation -- the unit interval, l = 0 with u < 1, a random interior
interval, and the minimum width 2^-10 -- so every box holds all four.  Points: random_mccormick_point mapped into the box by the
inverse transform (a McCormick-feasible point of the node); `outside=True` moves one x_i out of its bounds by 1e-9."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances")
CASES = {"spar020": ("spar020-100-1.in", 3), "mixed": ("spar040-030-1.in", 5)}
MIN_WIDTH = 2.0 ** -10


def instance(case):
    from sdpcutsel_via_nn_amd import harness
    inst = harness.parse_boxqp(os.path.join(INST, CASES[case][0]))
    return inst, CASES[case][1]


def random_box(n, seed):
    """-> (lb, ub): kinds 0 unit, 1 l = 0 only, 2 interior, 3 minimum width, each on about a quarter of the variables"""
    rng = np.random.default_rng(1000 + seed)
    kind = rng.permutation(n) % 4
    lb, ub = np.zeros(n), np.ones(n)
    for i in range(n):
        if kind[i] == 1:
            ub[i] = rng.uniform(0.25, 0.9)
        elif kind[i] == 2:
            w = rng.uniform(0.05, 0.5)
            lb[i] = rng.uniform(0.0, 1.0 - w)
            ub[i] = lb[i] + w
        elif kind[i] == 3:
            lb[i] = np.floor(rng.uniform(0.0, 1.0 - MIN_WIDTH) * 1024.0) / 1024.0      # a multiple of 2^-10: u - l is exactly 2^-10
            ub[i] = lb[i] + MIN_WIDTH
    assert np.all(ub - lb >= MIN_WIDTH) and np.all(lb >= 0) and np.all(ub <= 1) and (ub - lb).min() == MIN_WIDTH
    return lb, ub


def point_in_box(n, lb, ub, seed, outside=False):
    """a McCormick-feasible point of the unit box carried into [lb, ub] by the inverse transform"""
    from sdpcutsel_via_nn_amd import harness, nodebox
    vb = harness.random_mccormick_point(n, np.random.default_rng(seed))
    _, vv = nodebox.inverse_tables(None, vb, lb, ub)
    if outside:
        L = n * (n + 1) // 2
        i = int(np.argmax(ub - lb < 1.0))      # a variable with a proper bound
        vv = vv.copy()
        vv[L + i] = lb[i] - 1e-9
    return vv


def child_box(inst, depth=1):
    """the box of the `depth`-th left-right-... child below the root: branch on the variable with the largest X_ii - x_i^2 at the
    node's LP point, at x_i (kept 2^-10 away from the bounds) -> (lb, ub, LP value of the root relaxation)"""
    from sdpcutsel_via_nn_amd import harness
    n = inst["nb_vars"]
    L = n * (n + 1) // 2
    lb, ub = np.zeros(n), np.ones(n)
    root = None
    for level in range(depth):
        lp = harness.boxqp_relaxation(inst, lb, ub)
        lp.solve()
        if root is None:
            root = lp.get_objective_value()
        vv = np.asarray(lp.get_values())
        x = vv[L:]
        diag = n * np.arange(n) - np.arange(n) * (np.arange(n) - 1) // 2
        i = int(np.argmax(vv[diag] - x * x))
        cut = float(np.clip(x[i], lb[i] + MIN_WIDTH, ub[i] - MIN_WIDTH))
        if level % 2 == 0:
            ub[i] = cut
        else:
            lb[i] = cut
    return lb, ub, root
