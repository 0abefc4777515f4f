"""SDPCUT_OPT_SKIP_NONVIOLATED (csrc/score_mfma.hip: score_mfma_skip_kernel): a fused combined round that runs the MLP for violated
candidates only must return what the round that scores everybody returns, bit for bit.

Every case runs the same calls on two handles over the same list -- option value 2 (skip whatever the list length) and 0 (never)
-- and compares the bytes of everything they return: ids, scores, lambda_min, rows, counters, new_strat, and afterwards both
arrays of get_scores in full.

The LP point makes the violated candidates known by construction: n = 40, x uniform in [0.2, 0.8], X = x x^T with +0.05 on the
first 20 diagonal entries and -0.05 on the last 20.  A 3-variable set is non-violated exactly when all its variables are among
the first 20: 1 140 of the 9 880 sets, lambda_min in [0.020, 0.041] by the CPU oracle, at most -0.031 for all the others; 52 sets
are strong (violated with a positive measure) and no non-violated set has a positive measure (so nb_positive is the same either
way).  test_the_pattern_is_what_the_lists_assume asserts all of that with the oracle.  A second point with the same pattern
(_point_with_positive_nonviolated) gives 33 non-violated sets a positive measure and pins the one documented difference, nb_positive.

Lists hold 12 352 .. 14 000 candidates: the score kernels count for the selection -- and so may skip -- only where a fresh
selection would run the key pass and the fused radix kernel (csrc/topk_route.h: tk_fuse_ok), which for the combined strategy
starts above 12 288 candidates.  With option value 2 score_plan_skip hands each of the ~50 waves about four strips; the lists are
laid out strip by strip so that the waves' queues meet every fill the kernel distinguishes (asserted from the restated plan,
tests/skip_plan.py)."""
import itertools

import numpy as np
import pytest

import skip_plan

pytestmark = pytest.mark.gpu

N_VARS = 40
FIELDS = ("idx", "score", "lam", "rhs", "coef", "ks")
CSR_FIELDS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
STRIP_FILLS = (0, 1, 16, 17, 31, 32, 33, 64)


def _point(seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.2, 0.8, N_VARS)
    X = np.outer(x, x)
    d = np.arange(20)
    X[d, d] += 0.05
    X[d + 20, d + 20] -= 0.05
    return np.concatenate([X[np.triu_indices(N_VARS)], x])


ALL_SETS = np.array(list(itertools.combinations(range(N_VARS), 3)), dtype=np.int32)
NONVIOL = (ALL_SETS < 20).all(axis=1)


class _World(object):
    """the instance, the oracle's view of the 9 880 sets at the two LP points, and the device's CU count"""

    def __init__(self, oracle):
        import torch
        from sdpcutsel_via_nn_amd import synthetic
        self.Q, _, _ = synthetic.make_instance(N_VARS, 7)
        self.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        L = N_VARS * (N_VARS + 1) // 2
        self.points = {s: _point(s) for s in (3, 0)}
        self.eig, self.obj = {}, {}
        for s, vv in self.points.items():
            self.eig[s] = oracle.eigmin_batch(3, vv[L:][ALL_SETS], vv[:L][oracle.triu_positions(ALL_SETS, N_VARS)])
            self.obj[s] = oracle.opt_score_batch(3, ALL_SETS, N_VARS, vv, self.Q)
        self.strong = np.flatnonzero((self.obj[3] > 0) & ~NONVIOL)


@pytest.fixture(scope="module")
def world(oracle):
    return _World(oracle)


def test_the_pattern_is_what_the_lists_assume(world):
    assert int(NONVIOL.sum()) == 1140
    for s in world.points:
        e = world.eig[s]
        assert 0.017 <= e[NONVIOL].min() and e[NONVIOL].max() <= 0.044 and e[~NONVIOL].max() <= -0.031, s
        assert not ((world.obj[s] > 0) & NONVIOL).any(), s
    e = world.eig[3]
    assert 0.0199 <= e[NONVIOL].min() and e[NONVIOL].max() <= 0.0414
    assert world.strong.size == 52


def _layout(world, kind, seed=0):
    """-> (index into ALL_SETS of every candidate, violated flag of every candidate)"""
    rng = np.random.default_rng(seed)
    viol_pool, free_pool = np.flatnonzero(~NONVIOL), np.flatnonzero(NONVIOL)
    if kind == "none":
        flags = np.zeros(12352 + 17, dtype=bool)
    else:
        n = {"fills": 12352 + 41, "runs": 13000 + 7}[kind]
        flags = np.zeros(n, dtype=bool)
        strips = n // 64
        if kind == "fills":
            fills = rng.choice(STRIP_FILLS, size=strips)
        else:      # runs of all-violated and of none-violated strips within ONE wave (it takes every W-th strip), and alternating ones
            W = 4 * skip_plan.skip_plan(n, world.n_cu, True)["grid"]
            g, r = np.arange(strips) % W, np.arange(strips) // W
            fills = np.where(g < W // 3, 64, np.where(g < 2 * W // 3, 0, np.where(r % 2 == 0, 64, 0)))
        for s, f in enumerate(fills):
            flags[64 * s + rng.permutation(64)[:f]] = True
        flags[64 * strips:] = rng.uniform(size=n - 64 * strips) < 0.5
    which = np.where(flags, rng.choice(viol_pool, size=flags.shape[0]), rng.choice(free_pool, size=flags.shape[0]))
    # every strong set at least once, and one of them at several positions
    at = np.flatnonzero(flags)
    if at.size:
        spots = rng.choice(at, size=world.strong.size + 6, replace=False)
        which[spots[:world.strong.size]] = world.strong
        which[spots[world.strong.size:]] = world.strong[0]
    return which, flags


class _Pair(object):
    """the same list on two handles: option value 2 (a) and 0 (b)"""

    def __init__(self, world, which, opt=2, n_vars=N_VARS, sets=None, ks=None):
        import sdpcutsel_via_nn_amd as lib
        from sdpcutsel_via_nn_amd import _capi
        self.which = which
        if sets is None:
            sets = np.full((which.shape[0], 5), -1, dtype=np.int32)
            sets[:, :3] = ALL_SETS[which]
            ks = np.full(which.shape[0], 3, dtype=np.int32)
        self.N = sets.shape[0]
        self.handles = []
        for value in (opt, 0):
            sc = lib.Scorer(0)
            sc.set_builtin_networks(5)
            sc.set_instance(n_vars, world.Q)
            sc.set_candidates(sets, ks)
            sc.set_option(_capi.OPT_SKIP_NONVIOLATED, value)
            self.handles.append(sc)
        self.a, self.b = self.handles

    def close(self):
        for sc in self.handles:
            sc.close()

    def both(self, run, point=None):
        """run(scorer) on both handles, each at a fresh point (nothing scored: the round scores for itself)"""
        out = []
        for sc in self.handles:
            if point is not None:
                sc.set_point(point)
            out.append(run(sc))
        return out


@pytest.fixture(scope="module")
def pairs(world):
    made = {}

    def get(kind):
        if kind not in made:
            which, flags = _layout(world, kind)
            made[kind] = (_Pair(world, which), flags)
        return made[kind]
    yield get
    for p, _ in made.values():
        p.close()


def _same(a, b, fields, what):
    for f in fields:
        assert a[f].shape == b[f].shape and a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), (what, f)
    assert a["n_total"] == b["n_total"] and a["new_strat"] == b["new_strat"] and a["counters"] == b["counters"], (what, a["counters"], b["counters"])


def _stats(sc):
    from sdpcutsel_via_nn_amd import _capi
    return sc.get_stat(_capi.STAT_NN_SKIPPED), sc.get_stat(_capi.STAT_NN_COMPLETIONS)


def _scores_equal(pair, what):
    (ea, oa), (eb, ob) = pair.a.get_scores(), pair.b.get_scores()
    assert ea.tobytes() == eb.tobytes() and oa.tobytes() == ob.tobytes(), what
    return eb, ob


def test_the_queues_meet_every_fill(world, pairs):
    """what the lists are for, from the restated plan: strips with each of the fills, waves whose violated total leaves each
    remainder, runs of full and of empty strips within one wave"""
    _, flags = pairs("fills")
    p = skip_plan.skip_plan(flags.shape[0], world.n_cu, True)
    _, seen = skip_plan.passes(flags, p)
    assert max(len(s) for s in seen) >= 4
    assert set(STRIP_FILLS) <= set(c for s in seen for c in s)
    assert {0, 1, 16, 17, 31} <= set(sum(s) % 32 for s in seen)
    assert any(sum(s[:i]) % 32 + s[i] >= 64 for s in seen for i in range(len(s)))      # two passes behind one strip
    _, flags = pairs("runs")
    _, seen = skip_plan.passes(flags, skip_plan.skip_plan(flags.shape[0], world.n_cu, True))
    assert any(s[:3] == [64, 64, 64] for s in seen) and any(s[:3] == [0, 0, 0] for s in seen)
    assert any(64 in s and 0 in s for s in seen)


@pytest.mark.parametrize("auto_regime", [1, 0])
@pytest.mark.parametrize("kind", ["fills", "runs", "none"])
def test_same_round_either_way(world, pairs, kind, auto_regime):
    from sdpcutsel_via_nn_amd import _capi
    pair, flags = pairs(kind)
    n_viol = int(flags.sum())
    n_strong = int(np.isin(pair.which, world.strong).sum())
    assert (n_strong >= 52) == (kind != "none")
    for sc in pair.handles:
        sc.set_option(_capi.OPT_AUTO_REGIME, auto_regime)
    try:
        # strong regime: at most n_strong entries wanted; every entry visited: more than that
        for sel, strong_regime in ((20, True), (min(52, n_strong), True), (n_strong + 50, False), (5000, False)):
            if sel < 1:
                continue
            strong_regime = strong_regime and n_strong >= sel
            for call, fields in (("select_round", FIELDS), ("round_csr", CSR_FIELDS)):
                done0 = _stats(pair.a)[1]
                a, b = pair.both(lambda sc: getattr(sc, call)(4, sel, copy=True), point=world.points[3])
                _same(a, b, fields, (kind, sel, call))
                assert b["counters"]["nb_violated"] == n_viol
                skipped, done = _stats(pair.a)
                # (the stat is the LAST scoring launch's: the completion behind a round that visits every entry skipped nobody)
                assert skipped == (pair.N - n_viol if strong_regime else 0), (kind, sel, call)
                assert done - done0 == (0 if strong_regime else 1), (kind, sel, call, strong_regime)
                assert pair.a.get_stat(_capi.STAT_SCORED) == pair.b.get_stat(_capi.STAT_SCORED) == (_capi.EIG | _capi.NN)
                assert _stats(pair.b) == (0, 0)
                eig, obj = _scores_equal(pair, (kind, sel, call))
                assert _stats(pair.a) == (0, done0 + 1)      # get_scores completed the measure, or the round had
                assert np.array_equal(eig < -1e-15, flags)
                assert int(((obj > 0) & flags).sum()) == n_strong and not (obj[~flags] > 0).any()
    finally:
        for sc in pair.handles:
            sc.set_option(_capi.OPT_AUTO_REGIME, 1)


def test_repeated_sets_get_the_same_bits(world, pairs):
    pair, flags = pairs("fills")
    pair.both(lambda sc: sc.select_round(4, 20), point=world.points[3])
    _, obj = _scores_equal(pair, "repeats")
    order = np.argsort(pair.which, kind="stable")
    w, o = pair.which[order], obj[order]
    same_set = w[1:] == w[:-1]
    assert same_set.sum() > 1000 and np.array_equal(o[1:][same_set], o[:-1][same_set])
    assert (pair.which == world.strong[0]).sum() >= 7


@pytest.mark.parametrize("strat", [1, 2])
def test_other_strategies_after_a_skipped_round(world, pairs, strat):
    from sdpcutsel_via_nn_amd import _capi
    pair, flags = pairs("fills")
    a, b = pair.both(lambda sc: sc.select_round(4, 20), point=world.points[3])
    _same(a, b, FIELDS, "first")
    done0 = _stats(pair.a)[1]
    for sel in (300, 5000):
        a, b = pair.both(lambda sc: sc.select_round(strat, sel))      # same point: the eigenvalues stand, the measure is partial
        _same(a, b, FIELDS, (strat, sel))
    assert _stats(pair.a)[1] - done0 == 1      # (strategy 1 as well: its nb_positive counts by the measure)
    ra, rb = pair.both(lambda sc: sc.rank(strat, 300, max_out=300))
    assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() and ra[2:] == rb[2:]
    ra, rb = pair.both(lambda sc: sc.rank(4, 20, max_out=2000))      # the ranking beyond the head reads the whole measure
    assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() and ra[2:] == rb[2:]
    assert _stats(pair.a)[1] - done0 == 1
    _scores_equal(pair, strat)


def test_a_new_point_scores_again(world, pairs):
    pair, flags = pairs("fills")
    a, b = pair.both(lambda sc: sc.select_round(4, 20), point=world.points[3])
    _same(a, b, FIELDS, "point 3")
    done0 = _stats(pair.a)[1]
    a, b = pair.both(lambda sc: sc.select_round(4, 20), point=world.points[0])
    _same(a, b, FIELDS, "point 0")
    assert _stats(pair.a) == (pair.N - int(flags.sum()), done0)
    assert not np.array_equal(a["score"], pair.a.select_round(4, 20, point=world.points[3])["score"])
    pair.b.set_point(world.points[3])
    pair.b.select_round(4, 20)
    eig, obj = _scores_equal(pair, "back at point 3")
    ref = world.obj[3][pair.which]      # (the tolerances of smoke())
    assert np.all(np.abs(obj - ref) <= 1e-9 * np.maximum(np.abs(ref), 1.0)) and np.abs(eig - world.eig[3][pair.which]).max() <= 2e-13


def test_sharded_round_with_one_rank(world, pairs):
    import torch
    from sdpcutsel_via_nn_amd.distributed import DeviceOps, ShardedSelector
    which, flags = _layout(world, "fills", seed=1)
    pair = _Pair(world, which)
    n_strong = int(np.isin(which, world.strong).sum())
    try:
        sels = [ShardedSelector(DeviceOps(sc, torch.device("cuda", 0)), pair.N) for sc in pair.handles]
        for sel_size, path in ((20, "common"), (n_strong + 50, "comball")):
            out = []
            done0 = _stats(pair.a)[1]
            for sc, sel in zip(pair.handles, sels):
                sc.set_point(world.points[3])
                out.append(sel.select_round(4, sel_size))
            a, b = out
            for f in ("ids", "scores", "mine", "lam", "coef", "rhs", "ks"):
                assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), (path, f)
            assert a["new_strat"] == b["new_strat"] and a["n_total"] == b["n_total"] and a["counters"] == b["counters"], path
            assert sels[0].path_counts[path] == sels[1].path_counts[path] >= 1 and sels[0].path_counts["unfused"] == 0
            if path == "common":
                assert _stats(pair.a) == (pair.N - int(flags.sum()), done0)
            else:
                assert _stats(pair.a) == (0, done0 + 1)
            _scores_equal(pair, path)
    finally:
        for sc in pair.handles:
            sc.set_stream(None)
        pair.close()


def test_mixed_list_stays_on_the_launch_over_all_classes(world):
    """only 3-variable candidates have a skipping kernel, and only a list of that one class uses it: a mixed list is scored by the
    launch over all classes as before, whatever the option says"""
    which, _ = _layout(world, "fills", seed=2)
    sets = np.full((which.shape[0], 5), -1, dtype=np.int32)
    sets[:, :3] = ALL_SETS[which]
    ks = np.full(which.shape[0], 3, dtype=np.int32)
    sets[::7, 2] = -1
    ks[::7] = 2
    pair = _Pair(world, which, sets=sets, ks=ks)
    try:
        a, b = pair.both(lambda sc: sc.select_round(4, 20), point=world.points[3])
        _same(a, b, FIELDS, "mixed")
        assert _stats(pair.a) == (0, 0)
        _scores_equal(pair, "mixed")
    finally:
        pair.close()


def test_production_plan_just_above_the_threshold(world):
    """option value 1, the default: a list just above the 65 536 candidates from which score_plan cuts strips of 64 on 256 CUs"""
    from sdpcutsel_via_nn_amd import _capi
    n = 32 * world.n_cu * 8 + 77
    rng = np.random.default_rng(5)
    which = rng.integers(0, ALL_SETS.shape[0], size=n)
    flags = ~NONVIOL[which]
    assert skip_plan.skip_applies(n, world.n_cu, 3, 1) and not skip_plan.skip_applies(n - 77, world.n_cu, 3, 1)
    pair = _Pair(world, which, opt=1)
    n_strong = int(np.isin(which, world.strong).sum())
    assert n_strong >= 250
    try:
        for sel in (250, 5000):      # the strong regime, then every entry visited
            done0 = _stats(pair.a)[1]
            a, b = pair.both(lambda sc: sc.round_csr(4, sel, copy=True), point=world.points[3])
            _same(a, b, CSR_FIELDS, sel)
            assert b["counters"]["strong"] == (sel if n_strong >= sel else n_strong)
            assert _stats(pair.a) == ((n - int(flags.sum()), done0) if n_strong >= sel else (0, done0 + 1))
            _scores_equal(pair, ("production", sel))
    finally:
        pair.close()


def _point_with_positive_nonviolated():
    """x as above (seed 0); X = x x^T + 0.1 b b^T + 0.01 I on the first 20 variables (b standard normal: positive definite, with
    off-diagonal structure) and - 0.05 on the last 20 diagonal entries.  The violated pattern is the same by construction; by the
    CPU oracle lambda_min >= 0.0038 on the non-violated sets and <= -0.031 on the others, 110 sets are strong and 33 NON-violated
    sets have a positive measure (up to 5.4)."""
    rng = np.random.default_rng(0)
    x = rng.uniform(0.2, 0.8, N_VARS)
    X = np.outer(x, x)
    b = rng.normal(size=(20, 1))
    X[:20, :20] += 0.1 * (b @ b.T) + 0.01 * np.eye(20)
    d = np.arange(20, 40)
    X[d, d] -= 0.05
    return np.concatenate([X[np.triu_indices(N_VARS)], x])


def test_nb_positive_of_a_skipped_round_counts_violated_candidates_only(world, oracle):
    """the one documented difference (include/sdpcut.h): where a NON-violated candidate has a positive measure, nb_positive of a
    skipped round in its strong regime is the number of positive measures among the violated candidates -- the others were not
    evaluated -- and everything else is the same, bit for bit"""
    vv = _point_with_positive_nonviolated()
    L = N_VARS * (N_VARS + 1) // 2
    eig = oracle.eigmin_batch(3, vv[L:][ALL_SETS], vv[:L][oracle.triu_positions(ALL_SETS, N_VARS)])
    obj = oracle.opt_score_batch(3, ALL_SETS, N_VARS, vv, world.Q)
    assert eig[NONVIOL].min() >= 0.003 and eig[~NONVIOL].max() <= -0.03
    assert int(((obj > 0) & NONVIOL).sum()) == 33 and int(((obj > 0) & ~NONVIOL).sum()) == 110
    which = np.concatenate([np.arange(ALL_SETS.shape[0]), np.random.default_rng(9).integers(0, ALL_SETS.shape[0], size=2600)])
    pair = _Pair(world, which)
    try:
        a, b = pair.both(lambda sc: sc.select_round(4, 100), point=vv)
        for f in FIELDS:
            assert a[f].tobytes() == b[f].tobytes(), f
        assert a["n_total"] == b["n_total"] and a["new_strat"] == b["new_strat"] == 4
        assert _stats(pair.a) == (int(NONVIOL[which].sum()), 0)
        e, o = _scores_equal(pair, "positive non-violated")
        viol, pos = e < -1e-15, o > 0
        assert np.array_equal(viol, ~NONVIOL[which]) and int((pos & ~viol).sum()) >= 33
        assert b["counters"] == dict(nb_violated=int(viol.sum()), strong=100, violated=100, nb_positive=int(pos.sum()))
        assert a["counters"] == dict(nb_violated=int(viol.sum()), strong=100, violated=100, nb_positive=int((pos & viol).sum()))
    finally:
        pair.close()


def test_the_exact_measure_after_a_skipped_round(world):
    """strategy 3 (SDPCUT_OPT_EXACT_SDP) ranks by the exact measure, which has an array of its own: a round and a ranking by it at
    the point of a skipped round are those of option 0, complete nothing, leave the MLP's measure partial and its array alone"""
    from sdpcutsel_via_nn_amd import _capi
    which, flags = _layout(world, "fills", seed=3)
    pair = _Pair(world, which)
    try:
        for sc in pair.handles:
            sc.set_option(_capi.OPT_EXACT_SDP, 1)
        a, b = pair.both(lambda sc: sc.select_round(4, 20), point=world.points[3])
        _same(a, b, FIELDS, "combined")
        before = _stats(pair.a)
        assert before == (pair.N - int(flags.sum()), 0)
        a, b = pair.both(lambda sc: sc.select_round(3, 300))      # scores the exact measure, then strategy 2 on it
        _same(a, b, FIELDS, "strategy 3 round")
        assert a["new_strat"] == 3
        ra, rb = pair.both(lambda sc: sc.rank(3, 0, max_out=500))
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() and ra[2:] == rb[2:]
        (sa, ga), (sb, gb) = pair.both(lambda sc: sc.get_sdp_scores())
        assert sa.tobytes() == sb.tobytes() and ga.tobytes() == gb.tobytes()
        assert np.array_equal(ra[1], np.sort(sa)[::-1][:500])      # the ranking's scores ARE the exact measure
        assert _stats(pair.a) == before
        want = _capi.EIG | _capi.NN | _capi.SDP
        assert pair.a.get_stat(_capi.STAT_SCORED) == pair.b.get_stat(_capi.STAT_SCORED) == want
        _scores_equal(pair, "after strategy 3")      # the MLP's measure: completed now, once
        assert _stats(pair.a) == (0, 1)
        (sa2, _), = [pair.a.get_sdp_scores()]
        assert sa2.tobytes() == sa.tobytes()
    finally:
        pair.close()
