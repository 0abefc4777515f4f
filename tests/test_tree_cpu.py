"""The branch-and-cut driver (sdpcutsel_via_nn_amd/tree.py) on its CPU backends: the numpy twin of node evaluation, and dense
eigen-cuts from numpy's eigh (tests/tree_helpers.py), against the exact optimum of six tiny dense instances
(tests/boxqp_truth.py).  No GPU."""
import numpy as np
import pytest

import boxqp_truth as bt
import tree_helpers as th

# Nodes the driver needs here with its defaults (rounds = 2, rule 1, rho 0.2) and the dense eigen-cuts, measured with the driver
# itself: (n, seed) -> (batch = 1, batch = 8).  The caps of the test are twice these.
NODES = {(5, 1): (7, 7), (6, 1): (3, 3), (6, 2): (17, 17), (8, 1): (5, 5), (8, 2): (1, 1), (10, 1): (11, 11)}


def test_truth_checks_itself_and_handles_singular_faces():
    # f = (x0 - x1)^2 - 0.5 (x0 + x1) + x2: the face with x0, x1 free is singular with a residual; the optimum is at x0 = x1 = 1
    n, Q_arr, c = 3, np.array([1.0, -2.0, 0.0, 1.0, 0.0, 0.0]), np.array([-0.5, -0.5, 1.0])
    v, x = bt.boxqp_truth(n, Q_arr, c)
    assert v == -1.0 and x.tolist() == [1.0, 1.0, 0.0]
    # f = (x0 - x1)^2: a continuum of stationary points on a singular face, value 0
    v, x = bt.boxqp_truth(2, np.array([1.0, -2.0, 1.0]), np.zeros(2))
    assert v == 0.0 and x[0] == x[1]
    # an interior minimiser: (x0 - 0.3)^2 + (x1 - 0.7)^2 - 0.58
    v, x = bt.boxqp_truth(2, np.array([1.0, 0.0, 1.0]), np.array([-0.6, -1.4]))
    assert abs(v + 0.58) < 1e-15 and np.allclose(x, [0.3, 0.7], atol=1e-15)
    # a free value within rounding of a bound: the minimiser of (x0 - (1 + 1e-12))^2 is clipped onto x0 = 1
    v, x = bt.boxqp_truth(1, np.array([1.0]), np.array([-2.0 * (1.0 + 1e-12)]))
    assert x.tolist() == [1.0] and v == 1.0 - 2.0 * (1.0 + 1e-12)


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("n, seed", bt.PROTOTYPES)
def test_driver_closes_the_tiny_instances(n, seed, batch):
    from sdpcutsel_via_nn_amd import tree
    inst, truth, _ = bt.truth_of(n, seed)
    need = NODES[(n, seed)][batch == 8]
    res = tree.branch_and_cut(inst, th.eigen_separator(n), batch=batch, max_nodes=2 * need)
    print("n %d seed %d batch %d: %s, %d nodes (measured %d), lower %.9f upper %.9f truth %.9f" % (n, seed, batch, res.status, res.nodes, need,
                                                                                                  res.lower, res.upper, truth))
    th.check_result(res, truth)
    assert res.status == "optimal"
    assert abs(res.upper - truth) <= 1e-7 * max(1.0, abs(truth))
    assert res.gap <= 1e-6 and res.sign == 1.0 and res.instance_bounds == (res.upper, res.lower)
    assert res.x.shape == (n,) and np.all((res.x >= 0.0) & (res.x <= 1.0))
    M, _, c = bt.dense(n, inst["Q_arr"], inst["c"])
    assert abs(bt.f_value(M, c, res.x)[0] - res.upper) <= 1e-12 * max(1.0, abs(truth)) * n * n
    assert set(res.seconds) == {"lp", "separate", "evaluate", "total"} and res.lp_failures == 0


def test_mccormick_only_ends_at_the_node_limit_with_a_valid_bound():
    """Without cuts the n = 6, seed 2 instance is still open at the cap: status node_limit, and the bound is still a bound.  (This
    driver's node relaxations -- the secant and both tangents of every variable's own bounds -- close the tree without cuts after
    73 nodes at batch 8; the cap of 20 stops it well before that.  With the eigen-cuts it needs 17.)"""
    from sdpcutsel_via_nn_amd import tree
    inst, truth, _ = bt.truth_of(6, 2)
    res = tree.branch_and_cut(inst, batch=8, max_nodes=20)
    th.check_result(res, truth)
    assert res.status == "node_limit" and 20 <= res.nodes <= 21
    assert res.lower < truth - 1e-3 and res.gap > 1e-6
    assert res.seconds["separate"] >= 0.0 and res.iterations >= 1


def test_time_limit_and_arguments():
    from sdpcutsel_via_nn_amd import tree
    inst, truth, _ = bt.truth_of(10, 1)
    ticks = iter(range(10 ** 6))
    res = tree.branch_and_cut(inst, batch=1, time_limit=40.0, clock=lambda: float(next(ticks)))      # a clock that advances by itself
    th.check_result(res, truth)
    assert res.status == "time_limit" and res.nodes >= 1
    with pytest.raises(ValueError):
        tree.branch_and_cut(inst, batch=0)
    with pytest.raises(ValueError):
        tree.branch_and_cut(inst, batch=129)


def test_a_failed_lp_never_prunes(monkeypatch):
    """the first five LPs that carry cut rows report a failure: those nodes are solved again with McCormick rows only, keep their
    parent's bound (the root: -inf) and are counted; nothing is pruned by them and the answer is still right"""
    from sdpcutsel_via_nn_amd import harness, tree
    inst, truth, _ = bt.truth_of(6, 2)
    real = harness.LinearRelaxation.solve
    left = [5]

    def solve(self):
        if len(self.linear_constraints._blocks) > 1 and left[0] > 0:
            left[0] -= 1
            raise RuntimeError("HiGHS: injected")
        return real(self)
    monkeypatch.setattr(harness.LinearRelaxation, "solve", solve)
    res = tree.branch_and_cut(inst, th.eigen_separator(6), batch=4, max_nodes=400)
    th.check_result(res, truth)
    assert res.log[0][1] == -np.inf      # the root failed: it has no bound of its own
    assert res.lp_failures == 5 and res.status == "optimal" and abs(res.upper - truth) <= 1e-7 * abs(truth)


def test_leaves_stay_in_the_global_bound():
    """an evaluate that never offers a branching variable: the root is a leaf, the run ends open_leaves with the root's bound"""
    from sdpcutsel_via_nn_amd import tree
    inst, truth, _ = bt.truth_of(6, 2)
    twin = tree.twin_evaluate(inst)

    def evaluate(points, boxes):
        r = dict(twin(points, boxes))
        r["branch_var"] = np.full_like(r["branch_var"], -1)
        return r
    res = tree.branch_and_cut(inst, evaluate=evaluate)
    th.check_result(res, truth)
    assert res.status == "open_leaves" and res.nodes == 1 and res.leaves == 1 and res.lower < truth < res.upper + 1e-9


def test_the_global_bound_counts_every_open_node(monkeypatch):
    """Scripted LP values and incumbents, no LP at all: root 0; its children 1.0 and 4.9995; the children of the first 4.9999 each
    with an incumbent of 5.0 (gap_tol 1e-3: the cutoff becomes 4.995).  The node at 4.9995 is then still open -- within the gap of
    the incumbent, not yet closed -- and the global bound of that iteration is 4.9995, not 4.9999; the log never decreases."""
    from sdpcutsel_via_nn_amd import tree
    n = 4
    inst = dict(nb_vars=n, Q_arr=np.zeros(n * (n + 1) // 2), c=np.ones(n), adj=np.ones((n, n), dtype=bool))
    lp_values = iter([0.0, 1.0, 4.9995, 4.9999, 4.9999])
    incumbents = iter([10.0, 10.0, 10.0, 5.0, 5.0])

    def solve(node, inst_, res, clock):
        node.point = np.zeros(n * (n + 1) // 2 + n)
        return next(lp_values)

    def evaluate(points, boxes):
        P = points.shape[0]
        depth = int(np.sum(boxes[0, 1] - boxes[0, 0] < 1.0))      # one more variable halved per level
        f = np.array([next(incumbents) for _ in range(P)])
        return dict(x_local=np.zeros((P, n)), f_point=f, f_local=f, sweeps=np.zeros(P, np.int32), moves=np.zeros(P, np.int32),
                    branch_var=np.full(P, depth, np.int32), branch_score=np.ones(P), branch_val=np.full(P, 0.5))
    monkeypatch.setattr(tree, "_solve", solve)
    res = tree.branch_and_cut(inst, evaluate=evaluate, batch=1, rounds=0, gap_tol=1e-3)
    assert [(k, lo, up) for k, lo, up in res.log] == [(1, 0.0, 10.0), (3, 1.0, 10.0), (5, 4.9995, 5.0), (5, 4.9995, 5.0)]
    assert res.status == "optimal" and res.lower == 4.9995 and res.upper == 5.0 and res.nodes == 5
    lows = [lo for _, lo, _ in res.log]
    assert lows == sorted(lows)


def test_the_leaf_rule_follows_the_evaluate_callable():
    """a rule-0 evaluate under the driver's default branch_rule = 1: scores X_ii - x_i^2 <= 1e-9 must not make leaves"""
    from sdpcutsel_via_nn_amd import tree
    inst, truth, _ = bt.truth_of(6, 2)
    calls = []
    ev0 = tree.twin_evaluate(inst, branch_rule=0)

    def evaluate(points, boxes):
        r = dict(ev0(points, boxes))
        r["branch_score"] = np.minimum(r["branch_score"], 1e-12)      # tiny rule-0 scores, still branchable
        calls.append(points.shape[0])
        return r
    evaluate.branch_rule = 0
    res = tree.branch_and_cut(inst, th.eigen_separator(6), evaluate, batch=4, max_nodes=400)
    th.check_result(res, truth)
    assert res.status == "optimal" and res.leaves == 0 and abs(res.upper - truth) <= 1e-7 * abs(truth)
