"""The cut loop at a node with the node's triangle inequalities (cut_select_algo(box=, triangle_on=True, triangle_box=True)) on
spar020-100-1: every triangle row the loop hands to the LP is the twin's (sdpcutsel_via_nn_amd/triangles.py) and certified by
its checker; the default (triangle_box=False) is the run without the argument, byte for byte; separate_triangles_points."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PATH = os.path.join(GOLDEN, "instances", "spar020-100-1.in")
ROUNDS, SEL = 3, 0.1


def node_box(n):
    """a depth-2 node: two variables halved, one towards each side"""
    lb, ub = np.zeros(n), np.ones(n)
    ub[3], lb[11] = 0.5, 0.5
    return lb, ub


def run(**kw):
    """-> (the call's tuple, the LP's rows as (values, columns, lengths, rhs), [(LP point, first row, rows)] of the boxed triangle steps, solver)"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd.cut_solver import _lp_point
    cs = pkg.CutSolver()
    steps = []
    inner = cs._separate_and_add_triangle_node

    def spy(sel_size, vars_values):
        first = cs._my_prob.linear_constraints.get_num()
        nb = inner(sel_size, vars_values)
        steps.append((np.array(_lp_point(vars_values), dtype=np.float64), first, nb))
        return nb

    cs._separate_and_add_triangle_node = spy
    out = cs.cut_select_algo(PATH, 3, SEL, strat=1, nb_rounds_cuts=ROUNDS, triangle_on=True, box=node_box(20), **kw)
    store = cs._my_prob.linear_constraints
    return out, store.csr_parts(0) + (store.rhs_from(0),), steps, cs


def test_every_triangle_row_of_the_node_loop_is_certified():
    from sdpcutsel_via_nn_amd import triangles
    out, (val, col, lens, rhs), steps, cs = run(triangle_box=True)
    n = 20
    box = node_box(n)
    tri, dens = triangles.preprocess(cs._gpu_dense_adj())
    assert np.array_equal(tri, cs._gpu_tri_triples) and len(steps) >= 1 and out[5] == [s[2] for s in steps]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    total, scaled = 0, False
    for vv, first, nb in steps:
        full = triangles.round_csr(tri, dens, n, vv, cs._TRI_CUTS_PER_ROUND_MAX, box=box)
        nv = full["n_violated"]
        want = max(min(cs._TRI_CUTS_PER_ROUND_MIN, int(np.floor(SEL * nv))), min(cs._TRI_CUTS_PER_ROUND_MAX, nv))      # :844-845
        assert nb == want == min(nv, 4 * tri.shape[0])
        res = triangles.round_csr(tri, dens, n, vv, nb, box=box)
        lo, hi = ptr[first], ptr[first + nb]
        assert val[lo:hi].tobytes() == res["values"].tobytes() and np.array_equal(col[lo:hi], res["indices"])
        assert np.array_equal(lens[first:first + nb], np.diff(res["indptr"])) and rhs[first:first + nb].tobytes() == res["rhs"].tobytes()
        assert triangles.check_round(tri, dens, n, vv, nb, res, box=box)
        total += nb
        scaled = scaled or bool(np.any(np.abs(val[lo:hi]) > 1.0))
    # the node's facets are not the unit box's: rows over a halved variable carry 1 / d = 2
    assert total > 0 and scaled


def test_the_default_is_the_run_without_the_argument():
    a, rows_a, steps_a, _ = run()
    b, rows_b, steps_b, _ = run(triangle_box=False)
    assert not steps_a and not steps_b
    assert a[0] == b[0] and a[4] == b[4] and a[5] == b[5] and a[6] == b[6]
    for x, y in zip(rows_a, rows_b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert sum(a[5]) > 0


def test_separate_triangles_points():
    """the mixin's batched call: one (csr, n_violated) per point, the twin's rows, with and without boxes; a finished boxed run's
    triangle handle is not involved"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness, triangles
    inst = harness.parse_boxqp(PATH)
    n = inst["nb_vars"]
    cs = pkg.CutSolver()
    cs._nb_vars, cs._nb_lifted, cs._Q_arr, cs._Q_adj = n, inst["nb_lifted"], inst["Q_arr"], inst["adj"]
    tri, dens = triangles.preprocess(cs._gpu_dense_adj())
    rng = np.random.default_rng(8)
    pts = np.stack([harness.random_mccormick_point(n, rng) for _ in range(4)])
    boxes = np.stack([np.stack(node_box(n))] * 4)
    boxes[1, 1, 7] = 0.25
    for bx in (None, boxes):
        got = cs.separate_triangles_points(pts, 300, boxes=bx)
        assert len(got) == 4
        for p, (csr, nv) in enumerate(got):
            want = triangles.round_csr(tri, dens, n, pts[p], 300, box=None if bx is None else (bx[p, 0], bx[p, 1]))
            assert nv == want["n_violated"]
            for a, k in zip(csr, ("indptr", "indices", "values", "rhs")):
                assert a.dtype == want[k].dtype and a.tobytes() == want[k].tobytes(), (p, k)
