"""The covers on a chordal extension enumerated on the device (sdpcut_set_candidates_cover_ch: ch_ext 1, 2, -1) against the host
twin (sdpcut_enumerate_cover_ch, itself pinned to numpy twins and counts in tests/test_chordal_cpu.py), rounds on such a list,
and cut_select_algo(..., ch_ext=c) end to end."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import sdpcutsel_via_nn_amd as p
    return p


def _random_graph(n, dens, seed):
    rng = np.random.default_rng(seed)
    A = np.triu(rng.uniform(size=(n, n)) < dens, 1)
    return A | A.T


def _rule2_graph():
    """A 5-cycle 0..4, a 4-cycle 5..8 and the lone edge (9, 10), 12 vertices.  Under the default order the 5-cycle is filled with
    (1,4) and (2,4) and the 4-cycle with (6,8).  Under ch_ext = 2: the pair (1,2) SURVIVES although the extension has the
    triangle (1,2,4) -- that one has a single original edge --, the lone edge survives, the fill edges give no pair, and the
    pairs of the 4-cycle VANISH into the triangles (5,6,8) and (6,7,8), each with two original edges."""
    A = np.zeros((12, 12), dtype=bool)
    for a, b in [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (5, 6), (6, 7), (7, 8), (5, 8), (9, 10)]:
        A[a, b] = A[b, a] = True
    return A


def _instance(name):
    from sdpcutsel_via_nn_amd import harness
    return harness.parse_boxqp(os.path.join(GOLDEN, "instances", name))


def _cases():
    out = [("n%d" % n, _random_graph(n, dens, 7 * n), None) for n, dens in ((7, 0.6), (64, 0.2), (65, 0.2), (130, 0.08), (300, 0.03))]
    out.append(("n100_dense", _random_graph(100, 0.97, 3), None))          # > 64 forward triangles per edge: the 64-lane rounds repeat
    out.append(("rule2", _rule2_graph(), None))
    out.append(("spar070-050-1", None, "spar070-050-1.in"))
    return out


CASES = _cases()


@pytest.mark.parametrize("name,A,inst_name", CASES, ids=[c[0] for c in CASES])
def test_device_list_equals_host_twin(pkg, name, A, inst_name):
    """list order: the sets read back with get_candidates; the per-size SoA buckets (what the score kernels read): the scores of
    the enumerated list equal, bit for bit, those of the same list uploaded with set_candidates"""
    from sdpcutsel_via_nn_amd import _capi, harness
    if inst_name:
        inst = _instance(inst_name)
        A, n, Q_arr = inst["adj"], inst["nb_vars"], inst["Q_arr"]
    else:
        n = A.shape[0]
        rng = np.random.default_rng(n)
        L = n * (n + 1) // 2
        Q_arr = rng.uniform(0.5, 2.0, size=L) * rng.choice([-1.0, 1.0], size=L)
    vv = harness.random_mccormick_point(n, np.random.default_rng(4))
    sc, sc2 = pkg.Scorer(0), pkg.Scorer(0)
    try:
        for s in (sc, sc2):
            s.set_builtin_networks(5)
            s.set_instance(n, Q_arr)
        for c in (1, 2, -1):
            S, ks, N = _capi.enumerate_cover(A, 3, ch_ext=c)
            if name == "n100_dense":          # some edge has more than 64 sets: a second round of 64 lanes
                assert np.unique(S[:, :2], axis=0, return_counts=True)[1].max() > 64
            if name == "rule2" and c == 2:
                pairs = [tuple(r[:2]) for r, k in zip(S.tolist(), ks.tolist()) if k == 2]
                assert pairs == [(1, 2), (9, 10)] and N == 2 + 4            # survivors; the 4-cycle's pairs are gone
            assert sc.set_candidates_cover(A, 3, ch_ext=c) == N and sc.N == N, (name, c)
            S2, ks2 = sc.get_candidates(np.arange(N))
            assert np.array_equal(ks2, ks) and np.array_equal(S2, S), (name, c)
            sc.set_point(vv)
            sc.score(_capi.EIG | _capi.NN)
            eig, obj = sc.get_scores()
            sc2.set_candidates(S, ks)
            sc2.set_point(vv)
            sc2.score(_capi.EIG | _capi.NN)
            eig2, obj2 = sc2.get_scores()
            assert np.array_equal(eig, eig2) and np.array_equal(obj, obj2), (name, c)
    finally:
        sc.close()
        sc2.close()


def test_count_only_call_and_refusals(pkg):
    from sdpcutsel_via_nn_amd import _capi
    A = _random_graph(65, 0.2, 9)
    S1, ks1, N1 = _capi.enumerate_cover(A, 3, ch_ext=1)
    N2 = _capi.enumerate_cover(A, 3, ch_ext=2)[2]
    sc = pkg.Scorer(0)
    try:
        with pytest.raises(pkg.SdpCutError, match="set_instance first"):
            sc.set_candidates_cover(np.zeros((0, 0)), 3, ch_ext=-1)
        sc.set_instance(65, np.ones(65 * 66 // 2))
        assert sc.set_candidates_cover(A, 3, ch_ext=1) == N1 and sc.N == N1
        for c, N in ((2, N2), (-1, 65 * 64 * 63 // 6), (1, N1)):
            assert sc.set_candidates_cover(A, 3, max_subs=N, ch_ext=c) == N and sc.N == N1          # count only: the list stays
            S, ks = sc.get_candidates(np.arange(N1))
            assert np.array_equal(S, S1) and np.array_equal(ks, ks1)
        assert sc.set_candidates_cover(A, 3, max_subs=N2 + 1, ch_ext=2) == N2 and sc.N == N2
        with pytest.raises(ValueError):
            sc.set_candidates_cover(A, 4, ch_ext=2)
        with pytest.raises(ValueError):
            sc.set_candidates_cover(A, 3, ch_ext=3)
        assert sc.N == N2
        # ch_ext = 1 at dim 4: the cover of the extended pattern
        S4, ks4, N4 = _capi.enumerate_cover(A, 4, ch_ext=1)
        assert sc.set_candidates_cover(A, 4, ch_ext=1) == N4
        S, ks = sc.get_candidates(np.arange(N4))
        assert np.array_equal(S, S4) and np.array_equal(ks, ks4)
    finally:
        sc.close()


def test_rounds_on_the_extended_cover(pkg):
    """feasibility and combined rounds on the ch_ext = 2 cover of spar040-030-1: same head and rows as the same handle loaded with
    that list through set_candidates"""
    from sdpcutsel_via_nn_amd import _capi, harness
    inst = _instance("spar040-030-1.in")
    n = inst["nb_vars"]
    S, ks, N = _capi.enumerate_cover(inst["adj"], 3, ch_ext=2)
    assert N == 1090
    vv = harness.random_mccormick_point(n, np.random.default_rng(12))
    sc = pkg.Scorer(0)
    try:
        sc.set_builtin_networks(5)
        sc.set_instance(n, inst["Q_arr"])
        assert sc.set_candidates_cover(inst["adj"], 3, ch_ext=2) == N
        mine = {strat: sc.round_csr(strat, 109, point=vv, copy=True) for strat in (1, 4)}
        sc.set_candidates(S, ks)
        for strat in (1, 4):
            ref = sc.round_csr(strat, 109, point=vv, copy=True)
            assert ref["idx"].shape[0] > 0
            for key, val in ref.items():
                if isinstance(val, np.ndarray):
                    assert np.array_equal(mine[strat][key], val), (strat, key)
                else:
                    assert mine[strat][key] == val, (strat, key)
    finally:
        sc.close()


@pytest.mark.parametrize("c,n_cand", [(0, 1051), (1, 1105), (2, 1105)])
def test_cut_select_algo_with_ch_ext(pkg, c, n_cand):
    from sdpcutsel_via_nn_amd import _capi
    path = os.path.join(GOLDEN, "instances", "spar020-100-1.in")
    inst = _instance("spar020-100-1.in")
    n = inst["nb_vars"]
    cs = pkg.CutSolver()
    rows_m = []
    out = cs.cut_select_algo(path, 3, 0.1, strat=1, nb_rounds_cuts=2, ch_ext=c,
                             on_round=lambda r, log: rows_m.append(cs._my_prob.linear_constraints.get_num()) if r == 0 else None)
    bounds, nb_cuts = out[0], out[4]
    assert out[-1] == n_cand
    edges = int(np.triu(inst["adj"], 1).sum())
    ext, _, fill = _capi.chordal_extension(inst["adj"])
    assert fill == 3
    # McCormick rows: on the EXTENDED pattern with ch_ext 1 and 2 (cut_select_qp.py:396), on the original one otherwise
    assert rows_m == [2 * n + 3 * (edges + (fill if c else 0))]
    assert np.array_equal(np.asarray(cs._Q_adj) != 0, ext if c else inst["adj"])
    # at most the quota of cuts per round; cuts only remove points, so the bound cannot get worse (up to the LP solver's tolerance)
    assert nb_cuts[0] == 0 and 0 < nb_cuts[1] <= int(np.floor(0.1 * n_cand))
    assert bounds[0] + 1e-6 >= bounds[1] and bounds[1] + 1e-6 >= bounds[2]


def test_cut_select_algo_refuses_other_flags(pkg):
    path = os.path.join(GOLDEN, "instances", "spar020-100-1.in")
    with pytest.raises(AssertionError, match="Chordal extension flags"):
        pkg.CutSolver().cut_select_algo(path, 3, 0.1, strat=1, nb_rounds_cuts=2, ch_ext=3)
