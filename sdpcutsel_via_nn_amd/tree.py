"""A small best-first branch and cut for BoxQP, strung together from the batched node calls.

    min f(x) = sum_{i <= j} a_ij x_i x_j + sum_i c_i x_i      0 <= x <= 1

in the LP's minimising form: ``inst = dict(nb_vars, Q_arr = a packed, c, adj)`` as ``harness.parse_boxqp`` returns it (a BoxQP file
maximises: its values are the negatives, ``sign = -1``).  A node is a box ``l <= x <= u``; its relaxation is
``harness.boxqp_relaxation(inst, l, u)`` plus the cut rows its parent ended with, which are valid in the child because its box lies
inside the parent's.  Two callables do everything between the LP solves, each for ALL nodes of a batch in one call:

    separate(points [k, L + n], boxes [k, 2, n]) -> list of k CSR blocks (indptr, indices, values, rhs), rows ``>=``, or None
    evaluate(points, boxes) -> the dict of ``nodeeval.node_eval_points``

The defaults are "no cuts" and the numpy twin, so the driver runs without a GPU; :func:`gpu_backends` builds the pair from a bound
``CutSolver`` (``separate_points``, ``separate_triangles_points``, ``evaluate_points``).

What is NOT here: a global cut pool, node-valid rows in pools, strong branching, fixed variables (a variable narrower than
4 * BOX_MIN_WIDTH is never branched on; a node without a candidate is a leaf whose bound stays in the global bound), LP solves in
parallel.
"""
import heapq
import time

import numpy as np

from . import harness, nodeeval

LEAF_SCORE = 1e-9       # rule 1: sum_j |a_ij| |X_ij - x_i x_j| at or below this for every i -- X = x x^T on the pattern


class TreeResult(object):
    """What :func:`branch_and_cut` returns.  ``lower`` / ``upper`` / ``x``: the proven bound, the incumbent's value and the
    incumbent, in the LP's minimising form; ``sign``: the instance's own sense (-1: the file maximises and its values are
    ``sign * lower`` / ``sign * upper``).  ``status``: "optimal" (lower >= upper - gap_tol max(1, |upper|)), "node_limit",
    "time_limit" or "open_leaves" (the tree ended on leaves that cannot be branched and are not closed).  ``nodes``: node LPs
    built (the root is one).  ``log``: per iteration (nodes so far, lower, upper) -- lower never decreases, upper never increases.
    ``seconds``: dict lp / separate / evaluate / total.  ``lp_failures``: nodes whose LP did not solve to optimality with the
    carried rows and were solved again with McCormick rows only."""

    def __init__(self):
        self.lower, self.upper, self.x = -np.inf, np.inf, None
        self.status, self.nodes, self.sign = "node_limit", 0, 1.0
        self.log, self.seconds = [], dict(lp=0.0, separate=0.0, evaluate=0.0, total=0.0)
        self.lp_failures, self.leaves, self.iterations = 0, 0, 0
        self.incumbents = []      # (nodes so far, value, x, box [2, n] of the node it came from)

    @property
    def gap(self):
        """(upper - lower) / max(1, |upper|)"""
        return (self.upper - self.lower) / max(1.0, abs(self.upper))

    @property
    def instance_bounds(self):
        """(value of the incumbent, proven bound) in the instance's own sense"""
        return self.sign * self.upper, self.sign * self.lower


class _Node(object):
    __slots__ = ("lb", "ub", "bound", "var", "val", "rows", "depth", "lp", "point", "failed")

    def __init__(self, lb, ub, bound, rows, depth):
        self.lb, self.ub, self.bound, self.rows, self.depth = lb, ub, bound, rows, depth
        self.var, self.val, self.lp, self.point, self.failed = -1, 0.0, None, None, False


def no_cuts(points, boxes):
    return [None] * len(points)


def twin_evaluate(inst, max_sweeps=50, branch_rule=1, rho=0.2):
    """the default ``evaluate``: the numpy twin on the instance's own objective"""
    obj = np.concatenate([np.asarray(inst["Q_arr"], dtype=np.float64), np.asarray(inst["c"], dtype=np.float64)])

    def evaluate(points, boxes):
        return nodeeval.node_eval_points(obj, points, boxes, max_sweeps=max_sweeps, branch_rule=branch_rule, rho=rho)
    evaluate.branch_rule = branch_rule
    return evaluate


def _concat_csr(blocks):
    """CSR blocks (or None) -> one block, or None"""
    blocks = [b for b in blocks if b is not None and len(b[3])]
    if not blocks:
        return None
    if len(blocks) == 1:
        return blocks[0]
    indptr, off = [np.zeros(1, np.int64)], 0
    for b in blocks:
        p = np.asarray(b[0], dtype=np.int64)
        indptr.append(p[1:] + off)
        off += int(p[-1])
    return (np.concatenate(indptr), np.concatenate([np.asarray(b[1], dtype=np.int64)[:int(b[0][-1])] for b in blocks]),
            np.concatenate([np.asarray(b[2], dtype=np.float64)[:int(b[0][-1])] for b in blocks]),
            np.concatenate([np.asarray(b[3], dtype=np.float64) for b in blocks]))


def gpu_backends(solver, strat=2, sel_size=100, triangles=True, triangle_box=True, boxes=True, tri_cuts=1000, max_sweeps=50,
                 branch_rule=1, rho=0.2):
    """(separate, evaluate) on the device from a bound ``CutSolver`` (instance, candidate list, networks, ``_my_prob``): one
    ``separate_points`` round of strategy ``strat`` with ``sel_size`` cuts per node -- with the nodes' boxes if ``boxes`` --, the
    triangle inequalities of ``separate_triangles_points`` behind it if ``triangles`` (at most ``tri_cuts`` per node; those of the
    node's box if ``triangle_box``, else the root's), and ``evaluate_points``."""
    def separate(points, bxs):
        res = solver.separate_points(strat, points, sel_size, boxes=bxs if boxes else None)
        out = [tuple(np.array(a) for a in r[0]) for r in res]
        if triangles:
            tri = solver.separate_triangles_points(points, tri_cuts, boxes=bxs if triangle_box else None)
            out = [_concat_csr([a, t[0]]) for a, t in zip(out, tri)]
        return out

    def evaluate(points, bxs):
        return solver.evaluate_points(points, boxes=bxs, max_sweeps=max_sweeps, branch_rule=branch_rule, rho=rho)
    evaluate.branch_rule = branch_rule
    return separate, evaluate


def _solve(node, inst, res, clock):
    """Build (if needed) and solve the node's LP -> its value, or None after a failure: the node was then solved again with
    McCormick rows only and keeps its parent's bound."""
    t = clock()
    try:
        if node.lp is None:
            node.lp = harness.boxqp_relaxation(inst, node.lb, node.ub)
            for b in node.rows:
                node.lp.linear_constraints.add_csr(b[0], b[1], b[2], b[3], "G")
        try:
            node.lp.solve()
            node.point = np.asarray(node.lp.get_values(), dtype=np.float64)
            return float(node.lp.get_objective_value())
        except RuntimeError:
            # a status other than optimal never prunes: McCormick rows only, the parent's bound, counted
            res.lp_failures += 1
            node.failed, node.rows = True, []
            node.lp = harness.boxqp_relaxation(inst, node.lb, node.ub)
            node.lp.solve()      # (the McCormick relaxation of a box is feasible and bounded: a failure here is an error)
            node.point = np.asarray(node.lp.get_values(), dtype=np.float64)
            return None
    finally:
        res.seconds["lp"] += clock() - t


def branch_and_cut(inst, separate=None, evaluate=None, batch=64, rounds=2, gap_tol=1e-6, max_nodes=10000, time_limit=None,
                   branch_rule=1, rho=0.2, max_sweeps=50, sign=None, clock=time.perf_counter):
    """Best-first branch and cut (the module's docstring states the problem and the two callables) -> :class:`TreeResult`.
    Per iteration: the up to ``batch`` open nodes with the lowest bounds are branched on their stored (variable, value); every
    child's LP is built and solved, ``rounds`` times separated (one ``separate`` call for all children) and solved again, and
    evaluated once (one ``evaluate`` call).  A child's bound is max(parent's bound, LP value); the incumbent is the best f_local
    seen, with its x.  A node is closed when its bound reaches ``upper - gap_tol max(1, |upper|)``; a node without a branching
    variable, or (rule 1) with a score at most LEAF_SCORE, is a leaf: it is not branched and its bound stays in the global bound.
    ``branch_rule`` / ``rho`` / ``max_sweeps`` configure the default ``evaluate``.  The leaf test has to know which rule the scores
    come from: it reads ``evaluate.branch_rule`` where the callable has that attribute (:func:`twin_evaluate` and
    :func:`gpu_backends` set it) and takes the ``branch_rule`` argument otherwise -- pass the rule of a callable of your own."""
    n = int(inst["nb_vars"])
    if not 1 <= int(batch) <= nodeeval.MAX_POINTS // 2:
        raise ValueError("batch must be 1 .. %d: both children of every popped node go through one call" % (nodeeval.MAX_POINTS // 2))
    if separate is None:
        separate = no_cuts
    if evaluate is None:
        evaluate = twin_evaluate(inst, max_sweeps=max_sweeps, branch_rule=branch_rule, rho=rho)
    rule = getattr(evaluate, "branch_rule", branch_rule)      # the rule the scores come from: the callable's own, if it says
    res = TreeResult()
    res.sign = float(inst.get("sign", 1.0) if sign is None else sign)
    t_start = clock()
    heap, tick = [], 0            # (bound, tick, node)
    closed_floor = np.inf         # the lowest bound of a node closed by bound or left as a leaf
    open_leaf_floor = np.inf

    def cutoff():
        return res.upper - gap_tol * max(1.0, abs(res.upper))

    def process(nodes):
        """solve, separate, evaluate the nodes of a batch; close them or push them"""
        nonlocal tick, closed_floor, open_leaf_floor
        values = [_solve(nd, inst, res, clock) for nd in nodes]
        for _ in range(int(rounds)):
            act = [k for k, nd in enumerate(nodes) if not nd.failed]
            if not act:
                break
            pts = np.stack([nodes[k].point for k in act])
            bxs = np.stack([np.stack([nodes[k].lb, nodes[k].ub]) for k in act])
            t = clock()
            csrs = separate(pts, bxs)
            res.seconds["separate"] += clock() - t
            for k, csr in zip(act, csrs):
                if csr is None or len(csr[3]) == 0:
                    continue
                nd = nodes[k]
                blk = tuple(np.array(a) for a in csr)
                nd.rows = nd.rows + [blk]
                nd.lp.linear_constraints.add_csr(blk[0], blk[1], blk[2], blk[3], "G")
                values[k] = _solve(nd, inst, res, clock)
        pts = np.stack([nd.point for nd in nodes])
        bxs = np.stack([np.stack([nd.lb, nd.ub]) for nd in nodes])
        t = clock()
        ev = evaluate(pts, bxs)
        res.seconds["evaluate"] += clock() - t
        res.nodes += len(nodes)
        for k, nd in enumerate(nodes):
            if values[k] is not None and not nd.failed:
                nd.bound = max(nd.bound, values[k])
            f = float(ev["f_local"][k])
            if f < res.upper:
                res.upper, res.x = f, np.array(ev["x_local"][k])
                res.incumbents.append((res.nodes, f, res.x, bxs[k].copy()))
            nd.var, nd.val = int(ev["branch_var"][k]), float(ev["branch_val"][k])
            nd.lp = nd.point = None
            if nd.var < 0 or (rule == 1 and float(ev["branch_score"][k]) <= LEAF_SCORE):
                nd.var = -1
        for nd in nodes:      # (after the batch: every node sees the batch's incumbent)
            if nd.bound >= cutoff():
                closed_floor = min(closed_floor, nd.bound)
            elif nd.var < 0:
                res.leaves += 1
                open_leaf_floor = min(open_leaf_floor, nd.bound)
            else:
                tick += 1
                heapq.heappush(heap, (nd.bound, tick, nd))

    def note():
        # every open node counts, also one whose bound has come within the gap of the incumbent and is about to be closed
        lo = min([res.upper, closed_floor, open_leaf_floor] + [h[0] for h in heap])
        res.lower = lo
        res.log.append((res.nodes, lo, res.upper))

    process([_Node(np.zeros(n), np.ones(n), -np.inf, [], 0)])
    note()
    while True:
        while heap and heap[0][0] >= cutoff():      # closed by an incumbent found since they were pushed
            closed_floor = min(closed_floor, heapq.heappop(heap)[0])
        if not heap:
            res.status = "optimal" if open_leaf_floor >= cutoff() else "open_leaves"
            break
        if res.nodes >= max_nodes:
            res.status = "node_limit"
            break
        if time_limit is not None and clock() - t_start >= time_limit:
            res.status = "time_limit"
            break
        children = []
        while heap and len(children) < 2 * int(batch) and res.nodes + len(children) < max_nodes:
            bound, _, nd = heapq.heappop(heap)
            if bound >= cutoff():
                closed_floor = min(closed_floor, bound)
                continue
            for side in (0, 1):
                lb, ub = nd.lb.copy(), nd.ub.copy()
                if side == 0:
                    ub[nd.var] = nd.val
                else:
                    lb[nd.var] = nd.val
                children.append(_Node(lb, ub, nd.bound, list(nd.rows), nd.depth + 1))
        if children:
            process(children)
        res.iterations += 1
        note()
    note()
    res.seconds["total"] = clock() - t_start
    return res
