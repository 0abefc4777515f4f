"""The numpy twin of node evaluation (sdpcutsel_via_nn_amd/nodeeval.py) on the committed cases (tests/nodeeval_cases.py): against a
long-double restatement that shares no code with it, f_local <= f_point, the invariant checker on the twin's output and on mutants
of it, and the refusals.  No GPU."""
import numpy as np
import pytest

import nodeeval_cases as nc

LD = np.longdouble
EPS = 2.0 ** -53


def reference(c):
    """Plain loops in long double, point by point: projection, f, the scores of the rule.  The local search is not restated here --
    it is sequential decisions, which only equal arithmetic can follow; the checker's stationarity test covers its result."""
    n, P = c["n"], c["points"].shape[0]
    L = n * (n + 1) // 2
    a = [[LD(c["obj"][nc.pos(n, min(i, j), max(i, j))]) for j in range(n)] for i in range(n)]
    out = []
    for p in range(P):
        pt = c["points"][p]
        l = [0.0] * n if c["boxes"] is None else c["boxes"][p, 0]
        u = [1.0] * n if c["boxes"] is None else c["boxes"][p, 1]
        x = [LD(min(max(pt[L + i], l[i]), u[i])) for i in range(n)]
        f = sum(a[i][j] * x[i] * x[j] for i in range(n) for j in range(i, n)) + sum(LD(c["obj"][L + i]) * x[i] for i in range(n))
        mag = sum(abs(a[i][j] * x[i] * x[j]) for i in range(n) for j in range(i, n)) + sum(abs(LD(c["obj"][L + i]) * x[i]) for i in range(n))
        X = lambda i, j: LD(pt[nc.pos(n, min(i, j), max(i, j))])      # noqa: E731
        if c["branch_rule"] == 0:
            g = [X(i, i) - x[i] * x[i] for i in range(n)]
            gmag = [abs(X(i, i)) + x[i] * x[i] for i in range(n)]
        else:
            g = [sum(abs(a[i][j]) * abs(X(i, j) - x[i] * x[j]) for j in range(n)) for i in range(n)]
            gmag = [sum(abs(a[i][j]) * (abs(X(i, j)) + abs(x[i] * x[j])) for j in range(n)) for i in range(n)]
        out.append(dict(x=x, f=f, mag=mag, g=g, gmag=gmag, cand=[u[i] - l[i] >= 4 * nc.MIN_WIDTH for i in range(n)], l=l, u=u))
    return out


SMALL = [c for c in nc.CASES if c["n"] <= 65 and c["points"].shape[0] <= 5]


@pytest.mark.parametrize("c", SMALL, ids=[c["name"] for c in SMALL])
def test_twin_against_long_double(c):
    r = nc.twin_cached(c)
    n = c["n"]
    for p, ref in enumerate(reference(c)):
        bound = (n + 4) * EPS * ref["mag"]      # a sum of n(n+3)/2 products in any order with partial sums of at most n + 2 terms each... see nodeeval.f_longdouble
        assert abs(LD(r["f_point"][p]) - ref["f"]) <= bound, (p, r["f_point"][p], ref["f"])
        v = int(r["branch_var"][p])
        if not any(ref["cand"]):
            assert v == -1 and r["branch_score"][p] == 0.0
            continue
        assert ref["cand"][v]
        gb = [(n + 4) * EPS * m for m in ref["gmag"]]
        assert abs(LD(r["branch_score"][p]) - ref["g"][v]) <= gb[v]
        assert all(ref["g"][v] + gb[v] >= ref["g"][i] - gb[i] for i in range(n) if ref["cand"][i])
        # the lowest index among the candidates that tie exactly in the twin's own arithmetic is covered by the hand-built cases
        w = c["rho"] * (ref["u"][v] - ref["l"][v])
        m = max(w, nc.MIN_WIDTH)
        want = min(max(float(ref["x"][v]), ref["l"][v] + m), ref["u"][v] - m)
        while want - ref["l"][v] < nc.MIN_WIDTH:      # the rounded sum left the left child an ulp short (the rounded_value case)
            want = float(np.nextafter(want, 2.0))
        while ref["u"][v] - want < nc.MIN_WIDTH:
            want = float(np.nextafter(want, -1.0))
        assert r["branch_val"][p] == want and want - ref["l"][v] >= nc.MIN_WIDTH
        if c["max_sweeps"] == 0:
            assert np.array_equal(r["x_local"][p], np.array([float(t) for t in ref["x"]]))


@pytest.mark.parametrize("c", nc.CASES, ids=nc.IDS)
def test_local_search_descends_and_checker_accepts_the_twin(c):
    from sdpcutsel_via_nn_amd import nodeeval
    r = nc.twin_cached(c)
    fl, bl = nodeeval.f_longdouble(c["obj"], r["x_local"])
    L = c["n"] * (c["n"] + 1) // 2
    lb, ub = (0.0, 1.0) if c["boxes"] is None else (c["boxes"][:, 0], c["boxes"][:, 1])
    fp, bp = nodeeval.f_longdouble(c["obj"], np.clip(c["points"][:, L:], lb, ub))
    assert np.all(fl <= fp + bl + bp)                       # f_local <= f_point up to the rounding bound of the two sums
    assert np.all(np.abs(r["f_local"] - fl) <= bl) and np.all(np.abs(r["f_point"] - fp) <= bp)
    assert np.all(r["sweeps"] <= c["max_sweeps"]) and np.all((r["moves"] == 0) | (r["sweeps"] > 0))
    assert np.all((r["sweeps"] == c["max_sweeps"]) | (r["sweeps"] >= 1))       # a search that ended by itself ran its last, empty sweep
    assert nodeeval.check_node_eval(r, c["obj"], c["points"], c["boxes"], c["branch_rule"], c["rho"], c["max_sweeps"]) == []


def test_hand_built_answers():
    by = {c["name"]: c for c in nc.CASES}
    r = nc.twin_cached(by["endpoint_tie"])
    assert r["x_local"][:, 0].tolist() == [0.0, 1.0, 0.0] and r["moves"].tolist() == [1, 0, 0] and r["sweeps"].tolist() == [2, 1, 1]
    r = nc.twin_cached(by["endpoint_tie_boxed"])
    assert r["x_local"][:, 0].tolist() == [0.5, 0.5] and r["moves"].tolist() == [1, 0]
    for rule in (0, 1):
        assert nc.twin_cached(by["argmax_tie_rule%d" % rule])["branch_var"].tolist() == [0, 1]
        r = nc.twin_cached(by["exact_product_rule%d" % rule])
        assert r["branch_var"].tolist() == [0, 0, 0] and r["branch_score"].tolist() == [0.0] * 3
        # variable 1 on [0.25, 0.25 + 4 w], w = BOX_MIN_WIDTH, x_1 = 0.2501 below l + m: m = max(rho 4 w, w) and the value is l + m
        for rho, m in ((0.2, nc.MIN_WIDTH), (0.5, 2 * nc.MIN_WIDTH), (0.001, nc.MIN_WIDTH)):
            r = nc.twin_cached(by["widths_rule%d_rho%g" % (rule, rho)])
            assert r["branch_var"].tolist() == [1] and r["branch_val"].tolist() == [0.25 + m]
    c = by["rounded_value"]
    r = nc.twin_cached(c)
    l, u = c["boxes"][0, 0, 0], c["boxes"][0, 1, 0]
    assert (l + nc.MIN_WIDTH) - l < nc.MIN_WIDTH      # the plain formula's value would leave the left child too narrow
    assert r["branch_var"].tolist() == [0] and r["branch_val"][0] == np.nextafter(l + nc.MIN_WIDTH, 1.0)
    assert r["branch_val"][0] - l >= nc.MIN_WIDTH and u - r["branch_val"][0] >= nc.MIN_WIDTH
    r = nc.twin_cached(by["all_narrow"])
    assert r["branch_var"].tolist() == [-1] and r["branch_score"].tolist() == [0.0] and r["branch_val"].tolist() == [0.0]
    a, b, c50 = (nc.twin_cached(by["sweeps%d" % k]) for k in (0, 1, 50))
    assert a["sweeps"].tolist() == [0] * 5 and b["sweeps"].tolist() == [1] * 5 and np.all(c50["f_local"] <= b["f_local"]) and np.all(b["f_local"] <= a["f_local"])
    for name in ("on_bounds_node", "on_bounds_unit"):
        c = by[name + "_sweeps0"]
        l, u = (0.25, 0.75) if "node" in name else (0.0, 1.0)
        x = nc.twin_cached(c)["x_local"][0]
        assert x.tolist() == [l, np.nextafter(l, 1.0), l, l, u, u, u, np.nextafter(u, 0.0)]


def mutants(c, r):
    """(what, mutated result): each breaks one invariant"""
    n = c["n"]
    lb = np.zeros(n) if c["boxes"] is None else c["boxes"][0, 0]
    ub = np.ones(n) if c["boxes"] is None else c["boxes"][0, 1]

    def mut(**kw):
        m = {k: np.array(v) for k, v in r.items()}
        for k, (idx, val) in kw.items():
            m[k][idx] = val
        return m
    yield "leaves the box", mut(x_local=((0, 0), ub[0] + 1e-9))
    yield "not stationary", mut(x_local=((0, 1), 0.5 * (lb[1] + ub[1]) if abs(r["x_local"][0, 1] - 0.5 * (lb[1] + ub[1])) > 1e-3 else lb[1]))
    yield "f_local", mut(f_local=(0, r["f_local"][0] + 1e-6 * max(1.0, abs(r["f_local"][0]))))
    yield "f_point", mut(f_point=(0, r["f_point"][0] - 1e-6 * max(1.0, abs(r["f_point"][0]))))
    v = int(r["branch_var"][0])
    yield "branch_score", mut(branch_score=(0, r["branch_score"][0] * 1.001 + 1e-6))
    yield "not the argmax", mut(branch_var=(0, (v + 1) % n))
    yield "child too narrow", mut(branch_val=(0, lb[v] + 0.5 * nc.MIN_WIDTH))
    yield "no candidate", mut(branch_var=(0, -1))


@pytest.mark.parametrize("name", ["diagonal", "sweeps50", "sparse"])
def test_checker_rejects_mutants(name):
    from sdpcutsel_via_nn_amd import nodeeval
    c = {c["name"]: c for c in nc.CASES}[name]
    r = nc.twin_cached(c)
    args = (c["obj"], c["points"], c["boxes"], c["branch_rule"], c["rho"], c["max_sweeps"])
    assert nodeeval.check_node_eval(r, *args) == []
    for what, m in mutants(c, r):
        bad = nodeeval.check_node_eval(m, *args)
        assert bad and all(b.startswith("point 0") for b in bad), (what, bad)


def test_checker_on_capped_and_uncapped_searches():
    """a search cut off by max_sweeps = 1 is not stationary: the checker says so when told nothing about a cap, and skips the test
    for the capped points when told"""
    from sdpcutsel_via_nn_amd import nodeeval
    c = {c["name"]: c for c in nc.CASES}["sweeps1"]
    r = nc.twin_cached(c)
    assert nodeeval.check_node_eval(r, c["obj"], c["points"], c["boxes"], max_sweeps=1) == []
    assert any("stationary" in b for b in nodeeval.check_node_eval(r, c["obj"], c["points"], c["boxes"]))


def test_refusals():
    from sdpcutsel_via_nn_amd import nodeeval
    c = {c["name"]: c for c in nc.CASES}["diagonal"]
    ok = dict(obj=c["obj"], points=c["points"], boxes=c["boxes"], max_sweeps=5, branch_rule=1, rho=0.2)

    def refused(**kw):
        with pytest.raises(ValueError):
            nodeeval.node_eval_points(**dict(ok, **kw))
    nodeeval.node_eval_points(**ok)
    for bad in (np.nan, np.inf):
        for key, idx in (("obj", 3), ("points", (1, 2)), ("boxes", (0, 1, 2))):
            a = c[key].copy()
            a[idx] = bad
            refused(**{key: a})
    for l, u in ((-1e-9, 0.5), (0.5, 1.0 + 1e-9), (0.5, 0.5), (0.6, 0.5)):
        b = c["boxes"].copy()
        b[2, 0, 5], b[2, 1, 5] = l, u
        refused(boxes=b)
    for rho in (0.0, -0.1, 0.5000001, np.nan):
        refused(rho=rho)
    for rule in (-1, 2, 0.5):
        refused(branch_rule=rule)
    for ms in (-1, 1.5):
        refused(max_sweeps=ms)
    refused(points=c["points"][:, :-1])
    refused(points=np.zeros((257, c["points"].shape[1])), boxes=None)
    refused(boxes=c["boxes"][:3])
    refused(obj=c["obj"][:-1])
    n = 1025
    refused(obj=np.ones(n * (n + 1) // 2 + n), points=np.zeros((1, n * (n + 1) // 2 + n)), boxes=None)
    b = c["boxes"].copy()      # narrower than BOX_MIN_WIDTH is not refused: never a candidate
    b[0, 1, :] = b[0, 0, :] + 2.0 ** -12
    assert nodeeval.node_eval_points(**dict(ok, boxes=b))["branch_var"][0] == -1
