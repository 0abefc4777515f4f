"""Batched rounds on the device: sdpcut_score_points / sdpcut_round_csr_points against the single-point path on a SECOND handle with
the same instance, candidates and networks (round_csr(point=p); set_point + score + get_scores).  Every comparison is
np.array_equal on every field: the arithmetic of a candidate does not depend on the launch that hosts it, and all selection
routes share keys and tie rules."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances")
ARRAYS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
N_VARS = 20
LIST_SIZES = (1, 15, 16, 17, 63, 64, 65, 4096)


@pytest.fixture(scope="module")
def pair():
    """(batched handle, single-point handle) with the four shipped networks"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import networks
    scs = []
    for _ in range(2):
        sc = pkg.Scorer(0)
        for k in (2, 3, 4, 5):
            sc.set_network(k, *networks.load_network(k))
        scs.append(sc)
    yield tuple(scs)
    for sc in scs:
        sc.close()


def bind(pair, n, Q_arr, set_inds, ks):
    for sc in pair:
        sc.drop_pending()
        sc.set_instance(n, np.asarray(Q_arr, dtype=np.float64))
        sc.set_candidates(set_inds, ks)


def generic_points(n, count, seed0=1000):
    from sdpcutsel_via_nn_amd import harness
    return np.stack([harness.random_mccormick_point(n, np.random.default_rng(seed0 + i)) for i in range(count)])


def synthetic_list(k, N, seed=7):
    from sdpcutsel_via_nn_amd import synthetic
    Q_arr, _, rng = synthetic.make_instance(N_VARS, seed)
    s = synthetic.random_index_sets(N_VARS, k, N, rng)
    pad = np.full((N, 5), -1, dtype=np.int32)
    pad[:, :k] = s
    return Q_arr, pad, np.full(N, k, dtype=np.int32)


def assert_same_round(got, want, what=""):
    """every field of a round: the arrays (dtype, shape -- n_out, n_rows and nnz are their lengths -- and values), n_total,
    new_strat, counters"""
    assert set(got) == set(want), what
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f)
    assert (got["n_total"], got["new_strat"], got["counters"]) == (want["n_total"], want["new_strat"], want["counters"]), what


def stats(sc):
    from sdpcutsel_via_nn_amd import _capi
    return sc.get_stat(_capi.STAT_POINTS_REDONE), sc.get_stat(_capi.STAT_SELECT_FALLBACKS)


def real_cover(name, dim):
    """(n, Q_arr, set_inds, ks) of a BoxQP cover or of the objective cover of a QCQP instance"""
    from sdpcutsel_via_nn_amd import _capi, harness
    path = os.path.join(INST, name)
    if name.endswith(".in"):
        inst = harness.parse_boxqp(path)
        S, ks, _ = _capi.enumerate_cover(inst["adj"], dim)
    else:
        inst = harness.parse_osil(path)
        (S, ks), _ = harness.qcqp_covers(inst, dim, _capi.enumerate_cover)
    return inst["nb_vars"], inst["Q_arr"], np.ascontiguousarray(S), np.ascontiguousarray(ks), inst


# ------------------------------------------------------------------------------------------ 1. score shapes
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_score_points_shapes(pair, k):
    """tile-of-16 and strip-of-32/64 edges of the MFMA kernel, first / middle / last row of the grid's point axis; EIG only (the
    eigenvalue kernel), NN only and both"""
    from sdpcutsel_via_nn_amd import _capi
    batch, single = pair
    pts = generic_points(N_VARS, 17)
    before = stats(batch)
    for N in LIST_SIZES:
        Q_arr, S, ks = synthetic_list(k, N)
        bind(pair, N_VARS, Q_arr, S, ks)
        for eig, obj in ((True, False), (False, True), (True, True)):
            flags = (_capi.EIG if eig else 0) | (_capi.NN if obj else 0)
            ref_e, ref_o = np.empty((17, N)), np.empty((17, N))
            for p in range(17):
                single.set_point(pts[p])
                single.score(flags)
                e, o = single.get_scores(eig=eig, obj=obj)
                if eig:
                    ref_e[p] = e
                if obj:
                    ref_o[p] = o
            for P in (1, 2, 3, 17):
                e, o = batch.score_points(pts[:P], eig=eig, obj=obj)
                assert (e is None) == (not eig) and (o is None) == (not obj)
                if eig:
                    assert e.shape == (P, N) and np.array_equal(e, ref_e[:P]), (k, N, P, flags)
                if obj:
                    assert o.shape == (P, N) and np.array_equal(o, ref_o[:P]), (k, N, P, flags)
    assert stats(batch) == before


# ------------------------------------------------------------------------------------------ 2. round sizes
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_round_points_sizes(pair, k):
    batch, single = pair
    pts = generic_points(N_VARS, 17, seed0=2000)
    before = stats(batch)
    for N in LIST_SIZES:
        Q_arr, S, ks = synthetic_list(k, N)
        bind(pair, N_VARS, Q_arr, S, ks)
        for strat in (1, 2, 4):
            for sel in sorted(set(min(s, N) for s in (1, 7, 512))):
                ref = [single.round_csr(strat, sel, point=pts[p], copy=True) for p in range(17)]
                for P in (1, 3, 17):
                    got = batch.round_csr_points(pts[:P], strat, sel)
                    assert len(got) == P
                    for p in range(P):
                        assert_same_round(got[p], ref[p], (k, N, strat, sel, P, p))
    assert stats(batch) == before      # 7: generic points never leave the one-launch route, and nothing fell back


# ------------------------------------------------------------------------------------------ 3. real covers
@pytest.mark.parametrize("name,dim", [("spar020-100-1.in", 3), ("spar040-030-1.in", 5), ("q_20_4_25_1.osil", 3)])
def test_round_points_real_covers(pair, name, dim):
    batch, single = pair
    n, Q_arr, S, ks, _ = real_cover(name, dim)
    N = S.shape[0]
    if name == "spar020-100-1.in":
        assert N == 1051
    if name == "spar040-030-1.in":
        assert set(np.unique(ks).tolist()) == {2, 3, 4, 5}
    assert 1 <= N <= 4096
    bind(pair, n, Q_arr, S, ks)
    sel = max(1, int(np.floor(0.1 * N)))
    pts = generic_points(n, 5, seed0=3000)
    before = stats(batch)
    for strat in (1, 2, 4):
        ref = [single.round_csr(strat, sel, point=pts[p], copy=True) for p in range(5)]
        got = batch.round_csr_points(pts, strat, sel)
        for p in range(5):
            assert_same_round(got[p], ref[p], (name, strat, p))
    e, o = batch.score_points(pts)
    for p in range(5):
        single.set_point(pts[p])
        single.score(3)
        re, ro = single.get_scores()
        assert np.array_equal(e[p], re) and np.array_equal(o[p], ro)
    assert stats(batch) == before


# ------------------------------------------------------------------------------------------ 4. combined strategy, both regimes
def test_combined_both_regimes_in_one_batch(pair):
    """a batch with a point that has at least sel_size strong candidates (the scan stops there: + BIG_M) and one with fewer (every
    entry visited), found by seed search on the single-point path: random McCormick points (seeds 0..31), then blends of such
    points with the PSD point x x^T or with the LP vertex of the McCormick relaxation (seeds 32..63).  The strong count of every point is read off a
    single-point round whose quota nobody reaches (sel_size = N: every entry visited, counters["strong"] is the count); sel_size
    of the test is the largest count found (512 at most), so the point that has it is in the strong regime and every point with fewer is not.
    Fails -- does not skip -- if the two seed ranges hold no two points with different counts."""
    from sdpcutsel_via_nn_amd import harness
    batch, single = pair
    n, Q_arr, S, ks, inst = real_cover("spar020-100-1.in", 3)
    N = S.shape[0]
    bind(pair, n, Q_arr, S, ks)
    iu = np.triu_indices(n)
    lp = harness.boxqp_relaxation(inst)
    lp.solve()
    vertex = np.array(lp.get_values(), dtype=np.float64)

    def point(seed):
        rng = np.random.default_rng(seed)
        vv = harness.random_mccormick_point(n, rng)
        if seed >= 32:
            t = 0.03 * (seed - 31)
            if seed % 2:      # towards the relaxation's own LP vertex (McCormick feasible, like every blend with it)
                vv = t * vv + (1 - t) * vertex
            else:             # towards the PSD point x x^T of its own x
                x = vv[iu[0].shape[0]:]
                vv = t * vv + (1 - t) * np.concatenate([(x[:, None] * x[None, :])[iu], x])
        return vv

    pts_all = [point(seed) for seed in range(64)]
    strong = [single.round_csr(4, N, point=vv)["counters"]["strong"] for vv in pts_all]
    print("strong candidates by seed:", strong)
    sel = min(max(strong), 512)      # (a head of at most 512 entries: the one-launch route)
    assert sel >= 1 and min(strong) < sel, "seed ranges 0..31 / 32..63 did not yield both regimes: %s" % strong
    i_strong, i_few = strong.index(max(strong)), strong.index(min(strong))
    pts = np.stack([pts_all[i_few], pts_all[i_strong], pts_all[i_few], pts_all[i_strong]])
    refs = [single.round_csr(4, sel, point=vv, copy=True) for vv in pts]
    assert refs[1]["counters"]["strong"] == sel > refs[0]["counters"]["strong"]      # the two regimes on the single-point path
    got = batch.round_csr_points(pts, 4, sel)
    for p in range(4):
        assert_same_round(got[p], refs[p], p)
        assert got[p]["new_strat"] == refs[p]["new_strat"] and got[p]["counters"] == refs[p]["counters"]
    assert got[1]["counters"]["strong"] == sel > got[0]["counters"]["strong"]


# ------------------------------------------------------------------------------------------ 5. structured points
def test_structured_points(pair):
    from sdpcutsel_via_nn_amd import _capi, harness
    batch, single = pair
    n, Q_arr, S, ks, inst = real_cover("spar020-100-1.in", 3)
    bind(pair, n, Q_arr, S, ks)
    L = n * (n + 1) // 2
    sel = 105
    # the McCormick vertex: X of the relaxation's LP solution, x = 0.5 (round 1 of every BoxQP run; masses of equal scores)
    lp = harness.boxqp_relaxation(inst)
    lp.solve()
    vv = np.array(lp.get_values(), dtype=np.float64)
    vv[L:] = 0.5
    for strat in (1, 2, 4):
        redone0 = batch.get_stat(_capi.STAT_POINTS_REDONE)
        ref = single.round_csr(strat, sel, point=vv, copy=True)
        got = batch.round_csr_points(np.stack([vv, vv, vv]), strat, sel)
        for p in range(3):
            assert_same_round(got[p], ref, (strat, p))
            assert_same_round(got[p], got[0], (strat, p))
        # (a void every-entry-visited tie group is the one thing the fallback may absorb: the single-point path leaves its fast
        # route for it too)
        assert 0 <= batch.get_stat(_capi.STAT_POINTS_REDONE) - redone0 <= 3
    # a PSD point, X = x x^T, between two generic ones: nothing is violated there
    x = np.random.default_rng(5).uniform(0.0, 1.0, n)
    psd = np.concatenate([(x[:, None] * x[None, :])[np.triu_indices(n)], x])
    g = generic_points(n, 2, seed0=5000)
    pts = np.stack([g[0], psd, g[1]])
    ref = [single.round_csr(1, sel, point=p, copy=True) for p in pts]
    got = batch.round_csr_points(pts, 1, sel)
    for p in range(3):
        assert_same_round(got[p], ref[p], p)
    assert got[1]["idx"].shape[0] == 0 and got[1]["rhs"].shape[0] == 0 and got[1]["values"].shape[0] == 0      # n_out, n_rows, nnz
    assert got[1]["n_total"] == ref[1]["n_total"] and got[1]["counters"] == ref[1]["counters"]


# ------------------------------------------------------------------------------------------ 6. loop route
@pytest.mark.parametrize("case", ["n4097", "sel513", "sel0", "exact_head"])
def test_loop_route(pair, case):
    from sdpcutsel_via_nn_amd import _capi
    batch, single = pair
    N = 4097 if case == "n4097" else 4096
    sel = {"n4097": 100, "sel513": 513, "sel0": 0, "exact_head": 100}[case]
    Q_arr, S, ks = synthetic_list(3, N)
    bind(pair, N_VARS, Q_arr, S, ks)
    pts = generic_points(N_VARS, 3, seed0=6000)
    if case == "exact_head":
        for sc in pair:
            sc.set_option(_capi.OPT_EXACT_HEAD, 1)
    try:
        for strat in (1, 2, 4):
            ref = [single.round_csr(strat, sel, point=p, copy=True) for p in pts]
            got = batch.round_csr_points(pts, strat, sel)
            for p in range(3):
                assert_same_round(got[p], ref[p], (case, strat, p))
            if case == "exact_head" and strat != 1:
                assert batch.get_stat(_capi.STAT_EXACT_HEAD) == single.get_stat(_capi.STAT_EXACT_HEAD)
    finally:
        for sc in pair:
            sc.set_option(_capi.OPT_EXACT_HEAD, 0)


# ------------------------------------------------------------------------------------------ 8. state
def test_state_after_a_batched_call(pair):
    from sdpcutsel_via_nn_amd import _capi
    batch, single = pair
    Q_arr, S, ks = synthetic_list(3, 300)
    bind(pair, N_VARS, Q_arr, S, ks)
    pts = generic_points(N_VARS, 4, seed0=8000)
    for call in (lambda: batch.round_csr_points(pts[:3], 4, 30), lambda: batch.score_points(pts[:3])):
        batch.set_point(pts[3])
        batch.score(_capi.EIG)
        call()
        with pytest.raises(_capi.SdpCutError, match="set_point first"):      # SDPCUT_ESTATE: no current point
            batch.score(_capi.EIG)
        assert batch.get_stat(_capi.STAT_SCORED) == 0
        # a single-point round at a fresh point is what it is on the other handle
        assert_same_round(batch.round_csr(4, 30, point=pts[3], copy=True), single.round_csr(4, 30, point=pts[3], copy=True))
    # between the halves of a single-point round both batched calls are refused, and the pending round still ends correctly
    want = single.round_csr(1, 30, point=pts[2], copy=True)
    batch.round_csr_begin(1, 30, point=pts[2])
    with pytest.raises(_capi.SdpCutError, match="pending"):
        batch.round_csr_points(pts[:2], 1, 30)
    with pytest.raises(_capi.SdpCutError, match="pending"):
        batch.score_points(pts[:2])
    assert_same_round(batch.round_csr_end(copy=True), want)
    # refusals
    for strat in (0, 3, -1, 5, _capi.PART_STRONG, _capi.PART_COMBALL):
        with pytest.raises(ValueError, match="strategies 1 .*2 .*4"):
            batch.round_csr_points(pts[:2], strat, 30)
    with pytest.raises(ValueError):
        batch.round_csr_points(pts[:2], 1, -1)
    lib, h = batch._lib, batch._h
    import ctypes
    dp = pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = (_capi.RoundCsr * 2)()
    e = np.empty((2, 300))
    ep = e.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.sdpcut_round_csr_points(h, 0, dp, pts.shape[1], 1, 30, out) == -1
    assert b"256" in lib.sdpcut_last_error(h)
    assert lib.sdpcut_round_csr_points(h, 257, dp, pts.shape[1], 1, 30, out) == -1
    assert lib.sdpcut_round_csr_points(h, 2, None, pts.shape[1], 1, 30, out) == -1
    assert lib.sdpcut_round_csr_points(h, 2, dp, pts.shape[1], 1, 30, None) == -1
    assert lib.sdpcut_round_csr_points(h, 2, dp, pts.shape[1] - 1, 1, 30, out) == -1
    assert lib.sdpcut_score_points(h, 2, dp, pts.shape[1], _capi.SDP, ep, None) == -1
    assert lib.sdpcut_score_points(h, 2, dp, pts.shape[1], _capi.EIG | _capi.SDP, ep, None) == -1
    assert lib.sdpcut_score_points(h, 2, dp, pts.shape[1], 0, ep, ep) == -1
    assert lib.sdpcut_score_points(h, 2, dp, pts.shape[1], _capi.EIG, None, ep) == -1
    # no instance / no candidates: SDPCUT_ESTATE
    import sdpcutsel_via_nn_amd as pkg
    fresh = pkg.Scorer(0)
    try:
        fresh.nb_vars = N_VARS
        with pytest.raises(_capi.SdpCutError, match="set_instance"):
            fresh.round_csr_points(pts[:2], 1, 30)
        fresh.set_instance(N_VARS, Q_arr)
        with pytest.raises(_capi.SdpCutError, match="set_candidates"):
            fresh.score_points(pts[:2])
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------ 9. Python surface
def test_python_surface(pair):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    batch, single = pair
    n, Q_arr, S, ks, _ = real_cover("spar020-100-1.in", 3)
    bind(pair, n, Q_arr, S, ks)
    pts = generic_points(n, 3, seed0=9000)
    sel = 105
    one = single.round_csr(4, sel, point=pts[0])
    many = batch.round_csr_points(pts, 4, sel)
    assert list(one) == list(many[0])                       # the same keys in the same order
    for f in ARRAYS:
        assert many[0][f].dtype == one[f].dtype and many[0][f].ndim == one[f].ndim, f
        assert not many[0][f].flags.owndata                 # copy=False: views into the block
    detached = batch.round_csr_points(pts, 4, sel, copy=True)
    assert all(detached[1][f].flags.owndata for f in ARRAYS)
    assert isinstance(many[0]["n_total"], int) and isinstance(many[0]["new_strat"], int) and isinstance(many[0]["counters"], dict)
    assert all(isinstance(v, int) for v in many[0]["counters"].values()) and list(many[0]["counters"]) == list(one["counters"])

    # separate_points: per node what _gpu_add_csr takes; added to a row store it gives the rows of the single-point path
    class LP(object):
        def __init__(self):
            self.linear_constraints = harness._RowStore()

    cs = pkg.CutSolver()
    sets = [[int(v) for v in S[i, :ks[i]]] for i in range(S.shape[0])]
    agg = [(s, [n * s[a] - s[a] * (s[a] + 1) // 2 + s[b] for a in range(len(s)) for b in range(a, len(s))], None, None) for s in sets]
    cs.set_instance(n, Q_arr, agg, dim=3)
    try:
        for strat in (1, 4):
            nodes = cs.separate_points(strat, pts, sel)
            assert len(nodes) == 3
            for p, (csr, n_total, new_strat, counters) in enumerate(nodes):
                ref = single.round_csr(strat, sel, point=pts[p], copy=True)
                assert (n_total, new_strat, counters) == (ref["n_total"], ref["new_strat"], ref["counters"])
                a, b = LP(), LP()
                cs._my_prob = a
                assert cs._gpu_add_csr(csr, harness.SparsePair) == ref["rhs"].shape[0]
                cs._my_prob = b
                cs._gpu_add_csr((ref["indptr"], ref["indices"], ref["values"], ref["rhs"]), harness.SparsePair)
                for x, y in zip(a.linear_constraints.csr_parts(), b.linear_constraints.csr_parts()):
                    assert np.array_equal(x, y)
                assert a.linear_constraints.rhs == b.linear_constraints.rhs and a.linear_constraints.senses == b.linear_constraints.senses
                assert a.linear_constraints.get_num() == ref["rhs"].shape[0] > 0
    finally:
        for bnd in cs._gpu_bindings.values():
            bnd.scorer.close()
