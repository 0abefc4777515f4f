"""Node evaluation on the device (sdpcut_node_eval_points; csrc/node_eval.hip) against its numpy twin (sdpcutsel_via_nn_amd/nodeeval.py),
byte for byte on every committed case (tests/nodeeval_cases.py): the twin restates the device's arithmetic operation by operation,
so nothing here has a tolerance.  Then the invariant checker on the device's output, the counter, the handle's state -- the call is
read-only -- and the refusals."""
import os

import numpy as np
import pytest

import nodeeval_cases as nc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances", "spar020-100-1.in")


@pytest.fixture(scope="module")
def handles():
    """one Scorer per instance size, shared by the cases of that size"""
    import sdpcutsel_via_nn_amd as pkg
    made = {}

    def get(n, obj):
        if n not in made:
            made[n] = pkg.Scorer(0)
            made[n].set_instance(n, np.ascontiguousarray(obj[:n * (n + 1) // 2]))
        made[n].set_objective(obj)
        return made[n]
    yield get
    for s in made.values():
        s.close()


def device(sc, c, **kw):
    return sc.node_eval_points(c["points"], c["boxes"], max_sweeps=c["max_sweeps"], branch_rule=c["branch_rule"], rho=c["rho"], **kw)


@pytest.mark.parametrize("c", nc.CASES, ids=nc.IDS)
def test_device_equals_twin(handles, c):
    from sdpcutsel_via_nn_amd import _capi, nodeeval
    sc = handles(c["n"], c["obj"])
    before = sc.get_stat(_capi.STAT_NODE_EVAL_POINTS)
    got = device(sc, c)
    nc.same_bytes(got, nc.twin_cached(c))
    assert sc.get_stat(_capi.STAT_NODE_EVAL_POINTS) == before + c["points"].shape[0]
    assert nodeeval.check_node_eval(got, c["obj"], c["points"], c["boxes"], c["branch_rule"], c["rho"], c["max_sweeps"]) == []
    view = device(sc, c, copy=False)      # the strided view of the pinned block holds the same bytes
    assert np.array_equal(view["x_local"], got["x_local"]) and not view["x_local"].flags.writeable


def test_expected_answers_of_the_hand_built_cases(handles):
    """what the cases were built to show, on the device's output"""
    by = {c["name"]: c for c in nc.CASES}
    r = device(handles(2, by["endpoint_tie"]["obj"]), by["endpoint_tie"])
    assert r["x_local"][0, 0] == 0.0 and r["x_local"][1, 0] == 1.0 and r["moves"].tolist() == [1, 0, 0]      # the tie goes to l; phi = 0: no move
    r = device(handles(2, by["endpoint_tie_boxed"]["obj"]), by["endpoint_tie_boxed"])
    assert r["x_local"][:, 0].tolist() == [0.5, 0.5] and r["moves"].tolist() == [1, 0]
    for rule in (0, 1):
        c = by["argmax_tie_rule%d" % rule]
        assert device(handles(c["n"], c["obj"]), c)["branch_var"].tolist() == [0, 1]
        c = by["exact_product_rule%d" % rule]
        r = device(handles(c["n"], c["obj"]), c)
        assert r["branch_var"].tolist() == [0, 0, 0] and r["branch_score"].tolist() == [0.0, 0.0, 0.0]
        c = by["widths_rule%d_rho0.2" % rule]
        assert device(handles(c["n"], c["obj"]), c)["branch_var"].tolist() == [1]      # 0 and 2 are too narrow whatever their score
    c = by["all_narrow"]
    r = device(handles(c["n"], c["obj"]), c)
    assert r["branch_var"].tolist() == [-1] and r["branch_score"].tolist() == [0.0] and r["branch_val"].tolist() == [0.0]
    c = by["sweeps0"]
    r = device(handles(c["n"], c["obj"]), c)
    L = c["n"] * (c["n"] + 1) // 2
    assert np.array_equal(r["x_local"], np.clip(c["points"][:, L:], c["boxes"][:, 0], c["boxes"][:, 1])) and r["f_local"].tobytes() == r["f_point"].tobytes()


# ------------------------------------------------------------------------------------------ the handle's state is untouched
@pytest.fixture(scope="module")
def spar():
    from sdpcutsel_via_nn_amd import harness
    inst = harness.parse_boxqp(INST)
    n = inst["nb_vars"]
    rng = np.random.default_rng(5)
    obj = np.concatenate([inst["Q_arr"], inst["c"]])
    bx = nc.random_boxes(n, 4, rng)
    pts = nc.points_in(n, 4, rng, bx)
    lp = harness.boxqp_relaxation(inst)
    lp.solve()
    return dict(inst=inst, n=n, obj=obj, boxes=bx, points=pts, lp_point=np.asarray(lp.get_values(), dtype=np.float64),
                want=None)


def fresh(spar):
    import sdpcutsel_via_nn_amd as pkg
    sc = pkg.Scorer(0)
    sc.set_builtin_networks(5)
    sc.set_instance(spar["n"], np.asarray(spar["inst"]["Q_arr"], dtype=np.float64))
    sc.set_candidates_cover(spar["inst"]["adj"], 3)
    sc.set_objective(spar["obj"])
    return sc


def evaluate(sc, spar):
    from sdpcutsel_via_nn_amd import nodeeval
    got = sc.node_eval_points(spar["points"], spar["boxes"])
    if spar["want"] is None:
        spar["want"] = nodeeval.node_eval_points(spar["obj"], spar["points"], spar["boxes"])
    nc.same_bytes(got, spar["want"])


def same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            assert a[k] == b[k], k
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def prepare_scored(sc, spar):
    from sdpcutsel_via_nn_amd import _capi
    sc.set_point(spar["lp_point"])
    sc.score(_capi.EIG | _capi.NN)


def after_scored(sc, spar):
    e, o = sc.get_scores()
    return dict(eig=e, obj=o, **{"round_" + k: v for k, v in sc.round_csr(4, 40, copy=True).items()})


def prepare_pending(sc, spar):
    sc.round_csr_begin(2, 40, point=spar["lp_point"])


def after_pending(sc, spar):
    return sc.round_csr_end(copy=True)


def prepare_box(sc, spar):
    sc.set_box(spar["boxes"][1, 0], spar["boxes"][1, 1])
    sc.set_point(spar["lp_point"])


def after_box(sc, spar):
    from sdpcutsel_via_nn_amd import _capi
    sc.score(_capi.EIG | _capi.NN)
    e, o = sc.get_scores()
    lb, ub = sc.box
    Qb, vb = sc.box_tables()
    return dict(eig=e, obj=o, lb=lb, ub=ub, Q_box=Qb, vars_box=vb)


def prepare_pool(sc, spar):
    r = sc.round_csr(1, 60, point=spar["lp_point"], copy=True)
    sc.pool_create(200)
    sc.pool_add(r["indptr"], r["indices"], r["values"], r["rhs"])


def after_pool(sc, spar):
    out = {"state_" + k: v for k, v in sc.pool_state().items()}
    for p, d in enumerate(sc.pool_separate_points(spar["points"], 50, copy=True)):
        out.update({"sep%d_%s" % (p, k): v for k, v in d.items()})
    return out


@pytest.mark.parametrize("prepare, after", [(prepare_scored, after_scored), (prepare_pending, after_pending), (prepare_box, after_box),
                                            (prepare_pool, after_pool)], ids=["scored_point", "pending_round", "set_box", "live_pool"])
def test_the_call_leaves_the_handle_as_it_was(spar, prepare, after):
    """after each kind of state: the call (its own answer still the twin's), then the next existing call -- equal to the same call
    on a handle that never evaluated a node"""
    a, b = fresh(spar), fresh(spar)
    try:
        prepare(a, spar)
        evaluate(a, spar)
        evaluate(a, spar)
        got = after(a, spar)
        prepare(b, spar)
        same_dict(got, after(b, spar))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(spar):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    sc = fresh(spar)
    try:
        pts, bx = spar["points"], spar["boxes"]
        prepare_scored(sc, spar)
        want = after_scored(sc, spar)
        count = sc.get_stat(_capi.STAT_NODE_EVAL_POINTS)

        def refused(points=pts, boxes=bx, **kw):
            with pytest.raises(ValueError):
                sc.node_eval_points(points, boxes, **kw)
        for bad in (np.nan, np.inf, -np.inf):
            p2 = pts.copy()
            p2[2, 7] = bad
            refused(points=p2)
            p2 = pts.copy()
            p2[3, -1] = bad
            refused(points=p2)
            b2 = bx.copy()
            b2[1, 0, 3] = bad
            refused(boxes=b2)
        for l, u in ((-1e-9, 0.5), (0.5, 1.0 + 1e-9), (0.5, 0.5), (0.6, 0.5)):
            b2 = bx.copy()
            b2[2, 0, 5], b2[2, 1, 5] = l, u
            refused(boxes=b2)
        for rho in (0.0, -0.1, 0.5000001, np.nan, np.inf):
            refused(rho=rho)
        for rule in (-1, 2, 7):
            refused(branch_rule=rule)
        refused(max_sweeps=-1)
        refused(points=pts[:, :-1])
        refused(points=np.zeros((257, pts.shape[1])), boxes=None)
        refused(boxes=bx[:3])
        assert sc.get_stat(_capi.STAT_NODE_EVAL_POINTS) == count
        b2 = bx.copy()      # narrower than BOX_MIN_WIDTH is NOT refused: never a candidate
        b2[0, 1, :] = b2[0, 0, :] + 2.0 ** -12
        assert sc.node_eval_points(pts, b2)["branch_var"][0] == -1
        evaluate(sc, spar)
        same_dict(after_scored(sc, spar), want)
        # without an objective: a state error, and the handle goes on
        sc.set_objective(None)
        with pytest.raises(pkg.SdpCutError):
            sc.node_eval_points(pts, bx)
        sc.set_objective(spar["obj"])
        evaluate(sc, spar)
    finally:
        sc.close()


def test_more_than_1024_variables_are_refused():
    import sdpcutsel_via_nn_amd as pkg
    n = 1025
    L = n * (n + 1) // 2
    sc = pkg.Scorer(0)
    try:
        sc.set_instance(n, np.ones(L))
        sc.set_objective(np.ones(L + n))
        with pytest.raises(ValueError):
            sc.node_eval_points(np.zeros((1, L + n)))
    finally:
        sc.close()


def test_the_largest_size_served():
    """n = 1024, sixteen entries per lane: one sweep, the device against the twin"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import nodeeval
    n = 1024
    rng = np.random.default_rng(21)
    obj = nc.int_objective(n, rng, density=0.05)
    pts = nc.points_in(n, 2, rng)
    sc = pkg.Scorer(0)
    try:
        sc.set_instance(n, np.ascontiguousarray(obj[:n * (n + 1) // 2]))
        sc.set_objective(obj)
        nc.same_bytes(sc.node_eval_points(pts, None, max_sweeps=1), nodeeval.node_eval_points(obj, pts, None, max_sweeps=1))
    finally:
        sc.close()


def test_evaluate_points_follows_the_scorers_objective(spar):
    """CutSolver.evaluate_points hands the bound LP's objective to the scorer once -- and again after anybody else has set another
    vector, cleared it, or set the instance anew on that scorer"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import nodeeval
    cs = pkg.CutSolver()
    try:
        res = cs.branch_and_cut(INST, 3, 5, strat=1, triangles=False, max_nodes=1)
        assert res.nodes == 1
        sc = cs._gpu_bind().scorer
        want = spar["want"] or nodeeval.node_eval_points(spar["obj"], spar["points"], spar["boxes"])
        assert sc.objective_key == spar["obj"].tobytes()
        nc.same_bytes(cs.evaluate_points(spar["points"], spar["boxes"]), want)
        other = spar["obj"][::-1].copy()
        sc.set_objective(other)
        assert sc.objective_key == other.tobytes()
        nc.same_bytes(sc.node_eval_points(spar["points"], spar["boxes"]), nodeeval.node_eval_points(other, spar["points"], spar["boxes"]))
        nc.same_bytes(cs.evaluate_points(spar["points"], spar["boxes"]), want)
        sc.set_objective(None)
        assert sc.objective_key is None
        nc.same_bytes(cs.evaluate_points(spar["points"], spar["boxes"]), want)
        sc.set_instance(spar["n"], np.asarray(spar["inst"]["Q_arr"], dtype=np.float64))
        assert sc.objective_key is None
        nc.same_bytes(cs.evaluate_points(spar["points"], spar["boxes"]), want)
        nc.same_bytes(cs.evaluate_points(spar["points"], spar["boxes"], obj=other), nodeeval.node_eval_points(other, spar["points"], spar["boxes"]))
    finally:
        for b in (cs._gpu_bindings or {}).values():
            b.scorer.close()
