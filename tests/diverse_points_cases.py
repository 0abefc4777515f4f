"""Lists, LP points and (strategy, sel, pool) cases of the filtered batched round (tests/test_gpu_diverse_points.py), and the numpy
twins their premises are checked with on the CPU (tests/test_diverse_points_cpu.py).  A plain module: no fixtures, no GPU.

Lists: the dim-3 covers of spar020-100-1 (1051 candidates) and spar040-030-1 (243 candidates).  Points: McCormick-feasible points
-- random ones (harness.random_mccormick_point) and blends t * random + (1 - t) * (a point of the same x that violates nothing): the
weight sets how many candidates are violated, from most of the list down to none, so a walk by a measure that ranks every
candidate (strategies 2, 4, 6) meets entries that are not violated -- and the McCormick vertex x = 0.5 of the existing diverse
tests (tied scores and cosines).  Boxes: tests/nodebox_cases.py.

The twins: lambda_min and the cut rows from numpy.linalg.eigh, the optimality measure from networks.forward_twin, the efficacy score
from efficacy.measure, the rankings from the oracle's closed forms (strategy 6: efficacy.ranking), the walk from
diversity.greedy_filter.  They decide premises (counts that are > 0, where a walk ends), not bits."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
INST = os.path.join(ROOT, "tests", "golden", "instances")
LISTS = {"spar020": ("spar020-100-1.in", 3, 1051), "spar040": ("spar040-030-1.in", 3, 243)}
NEG = -1e-15
MP = 0.5
EFF_W = 0.1      # the weight of the objective parallelism in the strategy-6 cases

# (list, strategy, sel, pool_size) of the fast-route comparisons; every one holds the premises of test_diverse_points_cpu.py at
# max_parallel = 0.5.  Strategy 4 takes the one-wait route only with sel = pool (csrc/batch_route.h).
CASES = (
    ("spar020", 1, 40, 129), ("spar020", 1, 64, 512), ("spar020", 2, 50, 129), ("spar020", 2, 100, 512),
    ("spar020", 4, 129, 129), ("spar020", 4, 512, 512), ("spar020", 6, 30, 129), ("spar020", 6, 100, 512),
    ("spar040", 1, 20, 65), ("spar040", 2, 30, 129), ("spar040", 4, 243, 512), ("spar040", 6, 60, 512),
)
# pools at the edges of the walk's blocks: (list, strategy, sel, pool_size)
EDGE_CASES = tuple((lst, s, sel, pool) for lst in ("spar020", "spar040") for s in (1, 2, 6) for sel, pool in ((1, 1), (10, 63), (64, 64), (20, 65), (63, 65)))
N_POINTS = 8


@functools.lru_cache(maxsize=None)
def load(name):
    """-> (n, Q_arr, S int32 [N, 5], ks int32 [N], LP objective [Q_arr | c])"""
    from sdpcutsel_via_nn_amd import _capi, harness
    fname, dim, N = LISTS[name]
    inst = harness.parse_boxqp(os.path.join(INST, fname))
    S, ks, _ = _capi.enumerate_cover(inst["adj"], dim)
    S, ks = np.ascontiguousarray(S, dtype=np.int32), np.ascontiguousarray(ks, dtype=np.int32)
    assert S.shape[0] == N
    Q = np.asarray(inst["Q_arr"], dtype=np.float64)
    return inst["nb_vars"], Q, S, ks, np.concatenate([Q, np.asarray(inst["c"], dtype=np.float64)])


def mccormick_vertex(n, Q_arr):
    X = np.where(Q_arr < 0, 0.5, 0.0)
    iu = np.triu_indices(n)
    X[iu[0] == iu[1]] = 0.5
    return np.concatenate([X, np.full(n, 0.5)])


def blend_point(n, seed, t):
    """t * (a random McCormick point) + (1 - t) * (x x^T of the same x with the diagonal half way to the secant X_ii = x_i): both
    are McCormick-feasible and the set is convex; the second violates nothing, so t sets how many candidates are violated"""
    from sdpcutsel_via_nn_amd import harness
    vv = harness.random_mccormick_point(n, np.random.default_rng(seed))
    L = n * (n + 1) // 2
    x = vv[L:]
    iu = np.triu_indices(n)
    base = x[iu[0]] * x[iu[1]]
    base[iu[0] == iu[1]] += 0.5 * (x - x * x)
    return np.concatenate([t * vv[:L] + (1.0 - t) * base, x])


# blend weights of the eight points of a list: from every second candidate violated down to none at all
BLENDS = (1.0, 1.0, 0.7, 0.5, 0.4, 0.35, 0.3, 0.2)


@functools.lru_cache(maxsize=None)
def points(name):
    """[N_POINTS, L + n]: row p blends seed 700 + p with weight BLENDS[p]"""
    n = load(name)[0]
    return np.stack([blend_point(n, 700 + p, BLENDS[p]) for p in range(N_POINTS)])


def many_points(name, P):
    """P points for the one large batch: the eight above, then random ones"""
    n = load(name)[0]
    return np.stack([points(name)[p] if p < N_POINTS else blend_point(n, 700 + p, BLENDS[p % N_POINTS]) for p in range(P)])


def boxes_and_points(name, P, seed0=900):
    """P boxes of width >= 2^-10 (box 0: the unit box) and a McCormick-feasible point of each, as tests/test_gpu_boxed_points.py"""
    import nodebox_cases as nc
    n = load(name)[0]
    boxes = np.stack([np.stack((np.zeros(n), np.ones(n)))] + [np.stack(nc.random_box(n, seed0 + p)) for p in range(1, P)])
    pts = np.stack([nc.point_in_box(n, boxes[p, 0], boxes[p, 1], seed0 + p) for p in range(P)])
    return boxes, pts


# ------------------------------------------------------------------------------------------------------------ twins
def rows_twin(n, S, ks, vv):
    """-> (lam [N], coef [N, 20], cols int64 [N, 20]) of every candidate at vv: the eigenvector of the smallest eigenvalue of the
    lifted matrix, components of magnitude <= 1e-15 zeroed, v_i v_j on the x columns and the diagonal, 2 v_i v_j off it"""
    N = ks.shape[0]
    L = n * (n + 1) // 2
    lam, coef, cols = np.zeros(N), np.zeros((N, 20)), np.full((N, 20), -1, dtype=np.int64)
    for k in np.unique(ks):
        k = int(k)
        sel = np.flatnonzero(ks == k)
        s = S[sel, :k].astype(np.int64)
        ia, ib = np.triu_indices(k)
        pos = n * s[:, ia] - s[:, ia] * (s[:, ia] + 1) // 2 + s[:, ib]
        A = np.zeros((sel.shape[0], k + 1, k + 1))
        A[:, 0, 0] = 1.0
        A[:, 0, 1:] = A[:, 1:, 0] = vv[L + s]
        A[:, ia + 1, ib + 1] = vv[pos]
        A[:, ib + 1, ia + 1] = vv[pos]
        w, V = np.linalg.eigh(A)
        v = V[:, :, 0]
        v = np.where(np.abs(v) <= 1e-15, 0.0, v)
        lam[sel] = w[:, 0]
        m = 0
        for i in range(k + 1):
            for j in range(max(i, 1), k + 1):
                coef[sel, m] = (2.0 if i != j else 1.0) * v[:, i] * v[:, j]
                m += 1
        cols[sel, :k] = L + s
        cols[sel, k:k + pos.shape[1]] = pos
    return lam, coef, cols


@functools.lru_cache(maxsize=None)
def _net(k):
    from sdpcutsel_via_nn_amd import networks
    return networks.load_network(k)


def measure_twin(n, Q_arr, S, ks, vv, box=None):
    """obj_improve of every candidate (the MLP's estimate, float64 twin), inside ``box`` = (lb, ub) on the transformed tables"""
    from sdpcutsel_via_nn_amd import networks, nodebox
    if box is not None:
        Q_arr, vv = nodebox.transform_tables(Q_arr, vv, box[0], box[1])
    L = n * (n + 1) // 2
    out = np.zeros(ks.shape[0])
    for k in np.unique(ks):
        k = int(k)
        sel = np.flatnonzero(ks == k)
        s = S[sel, :k].astype(np.int64)
        ia, ib = np.triu_indices(k)
        pos = n * s[:, ia] - s[:, ia] * (s[:, ia] + 1) // 2 + s[:, ib]
        q = Q_arr[pos]
        me = k * np.abs(q).max(axis=1)
        me[me == 0.0] = 1.0
        q = q / me[:, None]
        sm = (q * vv[:L][pos]).sum(axis=1)
        w, p = _net(k)
        y = networks.forward_twin(k, w, p, np.concatenate([vv[L:][s], q], axis=1))
        out[sel] = (-sm) * me + y * me
    return out


def ranking_twin(strat, sel, lam, obj=None, escore=None):
    """candidate ids in the order sdpcut_rank(strat, sel_size = sel) lists them (strategy 1: the violated ones only)"""
    from oracle import cutsel_oracle
    from sdpcutsel_via_nn_amd import efficacy
    if strat == 6:
        return efficacy.ranking(escore)
    return np.asarray(cutsel_oracle.rank_arrays(strat, obj, lam, sel)[0], dtype=np.int64)


def walk_twin(name, strat, sel, pool_size, vv, max_parallel=MP, box=None):
    """the filtered round of one point by the twins -> info dict of diversity.greedy_filter plus accepted (``closest`` kept)"""
    from sdpcutsel_via_nn_amd import diversity, efficacy
    n, Q, S, ks, lpobj = load(name)
    lam, coef, cols = rows_twin(n, S, ks, vv)
    obj = measure_twin(n, Q, S, ks, vv, box) if strat in (2, 4) else None
    esc = efficacy.measure(lam, coef, cols, ks, lpobj, EFF_W)[2] if strat == 6 else None
    ids = ranking_twin(strat, sel, lam, obj, esc)[:pool_size]
    el = diversity.eligible_rows(lam[ids], ks[ids], coef[ids])
    keep, info = diversity.greedy_filter(S[ids], ks[ids], coef[ids], el, sel, max_parallel, return_info=True)
    info["accepted"] = int(keep.sum())
    return info
