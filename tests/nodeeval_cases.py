"""The committed cases of node evaluation (tests/test_nodeeval_cpu.py: the twin against long double and the checker;
tests/test_gpu_node_eval.py: the device against the twin, byte for byte).

A case is a dict: name, n, obj [L + n] = [a packed | c], points [P, L + n], boxes [P, 2, n] or None, max_sweeps, branch_rule, rho.
The objectives are integers in [-50, 50] as the tree tests' instances have them, unless the case sets them by hand.

    sizes          n = 1, 2, 3, 63, 64, 65, 125, 128, 129 and 200 (above 128, no multiple of 64): one, two, three and four entries per
                   lane, with and without a partial last round; boxed, both rules
    points         P = 1, 3 and 256 (n = 3 boxed, n = 65 on the unit box)
    diagonal       a_ii positive, negative and zero in one instance
    endpoint_tie   a_ii < 0 with phi(l) = phi(u) (the tie goes to l) and a coordinate whose phi is 0 everywhere (never moves)
    argmax_tie     equal scores under both rules: the lowest index wins; with variable 0 too narrow, variable 1
    on_bounds      x on a bound, one ulp inside, one ulp outside and 1e-7 outside, on a node box and on the unit box
    widths         widths exactly BOX_MIN_WIDTH, 4 BOX_MIN_WIDTH and one ulp below it; the narrow variables carry the largest scores
    all_narrow     every variable too narrow: branch_var = -1, score 0
    rounded_value  l + m rounded across a binade: the value moves by an ulp so that both children keep BOX_MIN_WIDTH
    sweeps         max_sweeps 0, 1 and 50 on one instance
    exact_product  X = x x^T exactly (x in eighths): score 0 under both rules
    sparse         most a_ij zero
"""
import numpy as np

MIN_WIDTH = 2.0 ** -10
KEYS = ("x_local", "f_point", "f_local", "sweeps", "moves", "branch_var", "branch_score", "branch_val")


def pos(n, i, j):
    return i * n - i * (i - 1) // 2 + (j - i)


def int_objective(n, rng, density=1.0, diag=None):
    L = n * (n + 1) // 2
    a = rng.integers(-50, 51, size=L).astype(np.float64)
    if density < 1.0:
        a[rng.random(L) > density] = 0.0
    c = rng.integers(-50, 51, size=n).astype(np.float64)
    if diag is not None:
        for i, v in enumerate(diag):
            a[pos(n, i, i)] = v
    obj = np.concatenate([a, c])
    if not obj.any():
        obj[-1] = 1.0
    return obj


def random_boxes(n, P, rng):
    lb = rng.random((P, n)) * 0.6
    ub = np.minimum(lb + 0.05 + rng.random((P, n)) * 0.5, 1.0)
    return np.stack([lb, ub], axis=1)


def points_in(n, P, rng, boxes=None, noise=0.05, outside=0.0):
    """LP-like points: x inside the box (a fraction `outside` of the entries 1e-7 beyond a bound), X = x x^T + noise"""
    lb, ub = (np.zeros((P, n)), np.ones((P, n))) if boxes is None else (boxes[:, 0], boxes[:, 1])
    x = lb + rng.random((P, n)) * (ub - lb)
    if outside:
        out = rng.random((P, n)) < outside
        side = rng.random((P, n)) < 0.5
        x = np.where(out & side, lb - 1e-7, np.where(out & ~side, ub + 1e-7, x))
    iu = np.triu_indices(n)
    X = x[:, iu[0]] * x[:, iu[1]] + noise * rng.random((P, iu[0].shape[0]))
    return np.concatenate([X, x], axis=1)


def case(name, n, obj, points, boxes, max_sweeps=50, branch_rule=1, rho=0.2):
    pts = np.ascontiguousarray(points, dtype=np.float64)
    assert pts.shape[1] == n * (n + 1) // 2 + n and obj.shape == (pts.shape[1],)
    return dict(name=name, n=n, obj=np.ascontiguousarray(obj, dtype=np.float64), points=pts,
                boxes=None if boxes is None else np.ascontiguousarray(boxes, dtype=np.float64), max_sweeps=max_sweeps, branch_rule=branch_rule,
                rho=rho)


def build_cases():
    out = []
    # sizes
    for k, n in enumerate((1, 2, 3, 63, 64, 65, 125, 128, 129, 200)):
        rng = np.random.default_rng(1000 + n)
        bx = random_boxes(n, 3, rng)
        out.append(case("size%d_rule%d" % (n, k % 2), n, int_objective(n, rng), points_in(n, 3, rng, bx, outside=0.1), bx, branch_rule=k % 2))
    rng = np.random.default_rng(7)
    bx = random_boxes(129, 2, rng)
    out.append(case("size129_rule1", 129, int_objective(129, rng), points_in(129, 2, rng, bx), bx, branch_rule=1, rho=0.5))
    # points
    rng = np.random.default_rng(11)
    out.append(case("P1", 5, int_objective(5, rng), points_in(5, 1, rng), None))
    bx = random_boxes(3, 256, rng)
    out.append(case("P256_n3_boxed", 3, int_objective(3, rng), points_in(3, 256, rng, bx, outside=0.2), bx, branch_rule=0, rho=0.01))
    out.append(case("P256_n65_unit", 65, int_objective(65, rng), points_in(65, 256, rng, None, outside=0.05), None, max_sweeps=4))
    # diagonal signs
    rng = np.random.default_rng(12)
    bx = random_boxes(6, 4, rng)
    out.append(case("diagonal", 6, int_objective(6, rng, diag=[5, -5, 0, 12, -7, 0]), points_in(6, 4, rng, bx), bx))
    # endpoint tie: coordinate 0 has a = -2, s = 2 on [0, 1]: phi(0) = phi(1) = 0 -> l; coordinate 1 has phi = 0 everywhere
    obj = np.array([-2.0, 0.0, 0.0, 2.0, 0.0])
    pts = np.array([[0.3, 0.2, 0.3, 0.5, 0.5], [0.0, 0.0, 0.0, 1.0, 0.25], [1.0, 0.0, 0.0, 0.0, 1.0]])
    out.append(case("endpoint_tie", 2, obj, pts, None))
    # the same with a box whose endpoints tie: a = -2, s = 3 on [0.5, 1]: phi(0.5) = (-1 + 3) 0.5 = 1, phi(1) = (-2 + 3) 1 = 1
    obj = np.array([-2.0, 0.0, 0.0, 3.0, 0.0])
    bx = np.array([[[0.5, 0.0], [1.0, 1.0]]] * 2)
    out.append(case("endpoint_tie_boxed", 2, obj, np.array([[0.5, 0.3, 0.2, 0.75, 0.5], [0.5, 0.3, 0.2, 0.5, 0.5]]), bx))
    # argmax ties
    n = 5
    L = n * (n + 1) // 2
    obj = np.concatenate([np.full(L, 3.0), np.full(n, -1.0)])
    pts = np.concatenate([np.full(L, 0.5), np.full(n, 0.5)])[None, :].repeat(2, axis=0)
    bx = np.stack([np.stack([np.zeros(n), np.ones(n)]), np.stack([np.zeros(n), np.ones(n)])])
    bx[1, 1, 0] = 3 * MIN_WIDTH      # point 1: variable 0 is too narrow -> variable 1
    pts[1, L] = 0.001
    for rule in (0, 1):
        out.append(case("argmax_tie_rule%d" % rule, n, obj, pts, bx, branch_rule=rule))
    # x on, next to and outside the bounds
    n = 8
    rng = np.random.default_rng(13)
    obj = int_objective(n, rng)
    L = n * (n + 1) // 2
    for name, l, u in (("node", 0.25, 0.75), ("unit", 0.0, 1.0)):
        x = np.array([l, np.nextafter(l, 1.0), np.nextafter(l, -1.0), l - 1e-7, u + 1e-7, u, np.nextafter(u, 2.0), np.nextafter(u, 0.0)])
        X = rng.random(L)
        bx = np.stack([np.full(n, l), np.full(n, u)])[None]
        out.append(case("on_bounds_" + name, n, obj, np.concatenate([X, x])[None], bx if name == "node" else None))
        out.append(case("on_bounds_%s_sweeps0" % name, n, obj, np.concatenate([X, x])[None], bx if name == "node" else None, max_sweeps=0))
    # widths: exactly MIN_WIDTH, 4 MIN_WIDTH, one ulp below 4 MIN_WIDTH, wide; the narrow ones have the largest X_ii - x_i^2
    n = 4
    L = n * (n + 1) // 2
    rng = np.random.default_rng(14)
    obj = int_objective(n, rng)
    lb = np.full(n, 0.25)
    ub = np.array([0.25 + MIN_WIDTH, 0.25 + 4 * MIN_WIDTH, np.nextafter(0.25 + 4 * MIN_WIDTH, 0.0), 0.75])
    assert ub[1] - lb[1] == 4 * MIN_WIDTH and ub[2] - lb[2] < 4 * MIN_WIDTH and ub[0] - lb[0] == MIN_WIDTH
    x = np.array([0.25, 0.2501, 0.2502, 0.5])
    X = np.zeros(L)
    for i, g in enumerate((0.9, 0.2, 0.8, 0.1)):
        X[pos(n, i, i)] = x[i] * x[i] + g
    for rule in (0, 1):
        for rho in (0.2, 0.5, 0.001):
            out.append(case("widths_rule%d_rho%g" % (rule, rho), n, obj, np.concatenate([X, x])[None], np.stack([lb, ub])[None], branch_rule=rule, rho=rho))
    ub2 = np.array([0.25 + MIN_WIDTH, np.nextafter(0.25 + 4 * MIN_WIDTH, 0.0), 0.25 + 2 * MIN_WIDTH, 0.25 + 3 * MIN_WIDTH])
    out.append(case("all_narrow", n, obj, np.concatenate([X, x])[None], np.stack([lb, ub2])[None]))
    # rounded_value: l = 0.5 - 3 * 2^-54 and m = MIN_WIDTH: l + m crosses into [0.5, 1), is rounded down, and (l + m) - l comes out
    # one ulp below MIN_WIDTH -- the value has to move up by an ulp for the left child to be a box set_box accepts
    n = 3
    L = n * (n + 1) // 2
    l0 = 0.5 - 3 * 2.0 ** -54
    assert (l0 + MIN_WIDTH) - l0 < MIN_WIDTH
    lb, ub = np.array([l0, 0.0, 0.25]), np.array([l0 + 0.01, 1.0, 0.75])
    x = np.array([l0, 0.5, 0.5])
    X = np.zeros(L)
    for i, g in enumerate((0.9, 0.1, 0.2)):
        X[pos(n, i, i)] = x[i] * x[i] + g
    out.append(case("rounded_value", n, int_objective(n, np.random.default_rng(18)), np.concatenate([X, x])[None], np.stack([lb, ub])[None], branch_rule=0,
                    rho=0.001))
    # max_sweeps
    rng = np.random.default_rng(15)
    obj = int_objective(8, rng)
    bx = random_boxes(8, 5, rng)
    pts = points_in(8, 5, rng, bx)
    for ms in (0, 1, 50):
        out.append(case("sweeps%d" % ms, 8, obj, pts, bx, max_sweeps=ms))
    # X = x x^T exactly
    n = 6
    rng = np.random.default_rng(16)
    x = rng.integers(0, 9, size=(3, n)) / 8.0
    iu = np.triu_indices(n)
    pts = np.concatenate([x[:, iu[0]] * x[:, iu[1]], x], axis=1)
    for rule in (0, 1):
        out.append(case("exact_product_rule%d" % rule, n, int_objective(n, rng), pts, None, branch_rule=rule))
    # sparse
    rng = np.random.default_rng(17)
    bx = random_boxes(40, 3, rng)
    out.append(case("sparse", 40, int_objective(40, rng, density=0.2), points_in(40, 3, rng, bx), bx))
    return out


CASES = build_cases()
IDS = [c["name"] for c in CASES]


def twin(c):
    from sdpcutsel_via_nn_amd import nodeeval
    return nodeeval.node_eval_points(c["obj"], c["points"], c["boxes"], max_sweeps=c["max_sweeps"], branch_rule=c["branch_rule"], rho=c["rho"])


_TWIN = {}


def twin_cached(c):
    """the twin's result of a committed case, computed once and shared (read-only)"""
    if c["name"] not in _TWIN:
        r = twin(c)
        for a in r.values():
            a.setflags(write=False)
        _TWIN[c["name"]] = r
    return _TWIN[c["name"]]


def same_bytes(a, b):
    """two results equal byte for byte, shapes and dtypes included"""
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.nonzero((x != y) | (np.signbit(x) != np.signbit(y)) if x.dtype.kind == "f" else (x != y))
            raise AssertionError("%s differs at %s: %r != %r" % (k, [b_[:5] for b_ in bad], x[bad][:5], y[bad][:5]))
