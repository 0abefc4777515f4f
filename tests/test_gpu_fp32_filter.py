"""SDPCUT_OPT_FP32_FILTER (csrc/score_mfma.hip: score_mfma_filter_kernel): the skipping launch of a fused combined round first runs
the network in fp32 for the violated candidates and the fp64 pass only for those the fp32 result cannot rule out.  A round must
return what it returns with the option off, and with SDPCUT_OPT_SKIP_NONVIOLATED off, bit for bit; and the bound the filter
decides by -- |y32 - y64| <= filter_margin -- must hold on the real instructions (sdpcut_filter_audit).

The construction is that of tests/test_gpu_skip_nonviolated.py, imported: n = 40, the pattern point, 9 880 three-variable sets,
lists of 12 352 .. 14 000 candidates under SDPCUT_OPT_SKIP_NONVIOLATED = 2.  The oracle is the float64 numpy twin of the network
(networks.forward_twin) on the candidate's inputs; test_the_pattern_holds_all_three_kinds holds it to the C oracle."""
import numpy as np
import pytest

import skip_plan
import test_gpu_skip_nonviolated as base

pytestmark = pytest.mark.gpu

N_VARS = base.N_VARS
ALL_SETS, NONVIOL = base.ALL_SETS, base.NONVIOL
FIELDS, CSR_FIELDS = base.FIELDS, base.CSR_FIELDS
PASS_FILLS = (0, 1, 16, 17, 31, 32)      # survivors of ONE fp32 pass of 32
WAVE_FILLS = (0, 33, 64)                 # survivors a wave hands to ring 2 in all


def _measure(oracle, sets, n_vars, vv, Q):
    """float64 twin on every set -> (y64 unmapped network output, max_elem, obj = -S max_elem + y max_elem)"""
    from sdpcutsel_via_nn_amd import networks
    L = n_vars * (n_vars + 1) // 2
    pos = oracle.triu_positions(sets, n_vars)
    q = Q[pos]
    me = 3.0 * np.abs(q).max(axis=1)
    me[me == 0.0] = 1.0
    q = q / me[:, None]
    S = (q * vv[:L][pos]).sum(axis=1)
    y = networks.forward_twin(3, *networks.load_network(3), np.concatenate([vv[L:][sets], q], axis=1))
    return y, me, (-S) * me + y * me


class _World(base._World):
    def __init__(self, oracle):
        from sdpcutsel_via_nn_amd import networks
        super().__init__(oracle)
        self.margin = networks.filter_margin(3, *networks.load_network(3))
        self.y, self.me, self.obj_twin = {}, {}, {}
        for s, vv in self.points.items():
            self.y[s], self.me[s], self.obj_twin[s] = _measure(oracle, ALL_SETS, N_VARS, vv, self.Q)
        self.r = {s: self.obj_twin[s] / self.me[s] for s in self.points}      # obj / max_elem: what the margin is held against


@pytest.fixture(scope="module")
def world(oracle):
    return _World(oracle)


def _handles(world, which, configs, sets=None, ks=None, net=None):
    """one Scorer per (SKIP_NONVIOLATED, FP32_FILTER) in configs over the same list"""
    import sdpcutsel_via_nn_amd as lib
    from sdpcutsel_via_nn_amd import _capi
    if sets is None:
        sets = np.full((which.shape[0], 5), -1, dtype=np.int32)
        sets[:, :3] = ALL_SETS[which]
        ks = np.full(which.shape[0], 3, dtype=np.int32)
    out = []
    for skip, filt in configs:
        sc = lib.Scorer(0)
        sc.set_builtin_networks(5)
        if net is not None:
            sc.set_network(3, *net)
        sc.set_instance(N_VARS, world.Q)
        sc.set_candidates(sets, ks)
        sc.set_option(_capi.OPT_SKIP_NONVIOLATED, skip)
        sc.set_option(_capi.OPT_FP32_FILTER, filt)
        out.append(sc)
    return out


THREE = ((2, 1), (2, 0), (0, 1))      # filtering | skipping only | scoring everybody


def _round(handles, call, strat, sel, point):
    out = []
    for sc in handles:
        if point is not None:
            sc.set_point(point)
        out.append(getattr(sc, call)(strat, sel, copy=True))
    return out


def _all_same(outs, fields, what):
    for o in outs[1:]:
        base._same(outs[0], o, fields, what)


def _scores_same(handles, what):
    got = [sc.get_scores() for sc in handles]
    for e, o in got[1:]:
        assert e.tobytes() == got[0][0].tobytes() and o.tobytes() == got[0][1].tobytes(), what
    return got[0]


def _evaluated(sc):
    from sdpcutsel_via_nn_amd import _capi
    return sc.get_stat(_capi.STAT_NN_EVALUATED)


def test_the_pattern_holds_all_three_kinds(world):
    """strong < within the margin < within twice the margin < half the violated sets, at both points; and the twin is the oracle"""
    m = world.margin
    viol = ~NONVIOL
    assert 0.01 < m < 0.05
    for s in world.points:
        ref = world.obj[s]
        assert np.all(np.abs(world.obj_twin[s] - ref) <= 1e-9 * np.maximum(np.abs(ref), 1.0)), s
        strong = int((viol & (world.r[s] > 0)).sum())
        within = int((viol & (world.r[s] > -m)).sum())
        within2 = int((viol & (world.r[s] > -2 * m)).sum())
        print("point %d: %d violated, %d strong, %d within the margin, %d within twice the margin" % (s, viol.sum(), strong, within, within2))
        assert 0 < strong < within < within2 < viol.sum() // 2, (s, strong, within, within2)
    assert int((viol & (world.r[3] > 0)).sum()) == world.strong.size == 52


@pytest.fixture(scope="module")
def lists(world):
    made = {}

    def get(kind):
        if kind not in made:
            which, flags = base._layout(world, kind)
            made[kind] = (_handles(world, which, THREE), which, flags)
        return made[kind]
    yield get
    for hs, _, _ in made.values():
        for sc in hs:
            sc.close()


def _bounds(world, which, flags, s=3):
    """what SDPCUT_STAT_NN_EVALUATED of a filtering launch must lie between, from the oracle: every violated candidate with a positive
    measure is evaluated, and nobody with obj64 <= -2 margin max_elem is (|obj32 - obj64| <= margin max_elem)"""
    r = world.r[s][which]
    return int((flags & (r > 0)).sum()), int((flags & (r > -2 * world.margin)).sum())


@pytest.mark.parametrize("auto_regime", [1, 0])
@pytest.mark.parametrize("kind", ["fills", "runs"])
def test_same_round_either_way(world, lists, kind, auto_regime):
    """tests 1 and 3 of the issue: the head at exactly the strong count (a dropped strong candidate shows), a head larger than it
    (the round completes and runs again), and the evaluated count between its two bounds"""
    from sdpcutsel_via_nn_amd import _capi
    handles, which, flags = lists(kind)
    n_strong = int(np.isin(which, world.strong).sum())
    lo, hi = _bounds(world, which, flags)
    assert lo == n_strong and hi < int(flags.sum()) // 2
    for sc in handles:
        sc.set_option(_capi.OPT_AUTO_REGIME, auto_regime)
    try:
        for sel, strong_regime in ((n_strong, True), (n_strong + 50, False)):
            for call, fields in (("select_round", FIELDS), ("round_csr", CSR_FIELDS)):
                done0 = handles[0].get_stat(_capi.STAT_NN_COMPLETIONS)
                outs = _round(handles, call, 4, sel, world.points[3])
                _all_same(outs, fields, (kind, sel, call))
                done = handles[0].get_stat(_capi.STAT_NN_COMPLETIONS) - done0
                ev = [_evaluated(sc) for sc in handles]
                print(kind, auto_regime, sel, call, "evaluated", ev, "bounds", lo, hi, "violated", int(flags.sum()))
                if strong_regime:
                    assert done == 0
                    assert lo <= ev[0] <= hi, (ev[0], lo, hi)
                    assert ev[1] == int(flags.sum()) and ev[2] == which.shape[0]
                    assert handles[0].get_stat(_capi.STAT_NN_SKIPPED) == which.shape[0] - int(flags.sum())
                else:
                    assert done == 1 and ev == [which.shape[0]] * 3
                _scores_same(handles, (kind, sel, call))
    finally:
        for sc in handles:
            sc.set_option(_capi.OPT_AUTO_REGIME, 1)


def _ring2(viol, surv, p):
    """The two rings of score_mfma_body (FILTER) followed wave by wave: fp32 passes take the 32 oldest entries of ring 1 while it
    holds 32, the last strip drains it.  -> (survivors of every fp32 pass, survivors per wave, violated per wave)"""
    per_pass, per_wave, viol_wave = [], [], []
    for mine in skip_plan.wave_strips(viol.shape[0], p):
        queue = []
        tot = 0
        for a, e in mine:
            queue += list(surv[a:e][viol[a:e]])
            while len(queue) >= 32:
                per_pass.append(int(sum(queue[:32])))
                tot += per_pass[-1]
                queue = queue[32:]
        if queue:
            per_pass.append(int(sum(queue)))
            tot += per_pass[-1]
        per_wave.append(tot)
        viol_wave.append(int(sum(int(viol[a:e].sum()) for a, e in mine)))
    return per_pass, per_wave, viol_wave


def _fill_layout(world, seed=4):
    """A list whose survivors are known from the oracle alone: every violated candidate is either strong (survives by the proof) or
    lies below -2 margin (cannot survive).  Laid out per WAVE: wave g gets WAVE target survivors spread over its strips so that
    single passes meet each of PASS_FILLS, one wave has every violated candidate surviving, one has none."""
    rng = np.random.default_rng(seed)
    viol = ~NONVIOL
    sure_in = np.flatnonzero(viol & (world.r[3] > 0))
    sure_out = np.flatnonzero(viol & (world.r[3] < -2 * world.margin))
    free = np.flatnonzero(NONVIOL)
    n = 12352 + 23
    p = skip_plan.skip_plan(n, world.n_cu, True)
    which = rng.choice(free, size=n)
    vflag = np.zeros(n, dtype=bool)
    sflag = np.zeros(n, dtype=bool)
    waves = skip_plan.wave_strips(n, p)
    pass_targets = list(PASS_FILLS) + [32, 1, 32, 0, 17]
    for g, mine in enumerate(waves):
        if g == 0:        # every violated candidate survives, whole strips
            plan = [(e - a, e - a) for a, e in mine]
        elif g == 1:      # violated, none survives
            plan = [(e - a, 0) for a, e in mine]
        elif g == 2:      # 33 survivors in all
            plan = [(min(40, e - a), 33 if i == 0 else 0) for i, (a, e) in enumerate(mine)]
        elif g == 3:      # 64
            plan = [(e - a, min(32, e - a) if i < 2 else 0) for i, (a, e) in enumerate(mine)]
        else:             # whole passes: 32 violated per strip, a chosen number of them surviving; the rest left to chance
            t = pass_targets[(g - 4) % len(pass_targets)]
            rest = (g - 4) >= len(pass_targets)
            plan = [(min(32, e - a), min(t, e - a) if i == 0 else (int(rng.integers(0, min(32, e - a) + 1)) if rest else 0))
                    for i, (a, e) in enumerate(mine)]
        for (a, e), (nv, ns) in zip(mine, plan):
            at = a + np.sort(rng.permutation(e - a)[:nv])
            vflag[at] = True
            which[at] = rng.choice(sure_out, size=nv)
            s_at = rng.permutation(at)[:ns]
            sflag[s_at] = True
            which[s_at] = rng.choice(sure_in, size=ns)
    # a strip no wave's plan touched stays non-violated
    return which, vflag, sflag, p


def test_ring_fills(world):
    """test 2 of the issue: the survivors' queue meets every fill the kernel distinguishes (asserted from the restated plan), and the
    evaluated count is EXACTLY the number of sure survivors"""
    from sdpcutsel_via_nn_amd import _capi
    which, vflag, sflag, p = _fill_layout(world)
    assert np.array_equal(vflag, ~NONVIOL[which])
    per_pass, per_wave, viol_wave = _ring2(vflag, sflag, p)
    assert set(PASS_FILLS) <= set(per_pass), sorted(set(per_pass))
    assert set(WAVE_FILLS) <= set(per_wave), sorted(set(per_wave))
    assert {0, 1, 16, 17, 31} <= set(w % 32 for w in per_wave), sorted(set(w % 32 for w in per_wave))
    assert any(s == v > 64 for s, v in zip(per_wave, viol_wave)) and any(s == 0 and v > 64 for s, v in zip(per_wave, viol_wave))
    handles = _handles(world, which, THREE)
    try:
        n_strong = int(sflag.sum())
        for sel in (n_strong, 20):
            outs = _round(handles, "round_csr", 4, sel, world.points[3])
            _all_same(outs, CSR_FIELDS, ("ring fills", sel))
            assert outs[0]["counters"]["strong"] == sel
            assert _evaluated(handles[0]) == n_strong and _evaluated(handles[1]) == int(vflag.sum())
        _scores_same(handles, "ring fills")
    finally:
        for sc in handles:
            sc.close()


def _audit(world, oracle, n_vars, Q, sets, vv, what):
    """-> the largest |y32 - y64| / margin over the list"""
    import sdpcutsel_via_nn_amd as lib
    sc = lib.Scorer(0)
    try:
        sc.set_builtin_networks(5)
        sc.set_instance(n_vars, Q)
        pad = np.full((sets.shape[0], 5), -1, dtype=np.int32)
        pad[:, :3] = sets
        sc.set_candidates(pad, np.full(sets.shape[0], 3, dtype=np.int32))
        sc.set_point(vv)
        m = sc.filter_margin(3)
        assert abs(m - world.margin) <= 0.02 * world.margin      # the C side against the numpy restatement
        y32 = sc.filter_audit()
    finally:
        sc.close()
    y64, _, _ = _measure(oracle, sets, n_vars, vv, Q)
    ratio = float(np.abs(y32 - y64).max() / m)
    print("filter audit, %s: %d candidates, max |y32 - y64| = %.3g = %.3g of the margin %.4g" % (what, sets.shape[0], ratio * m, ratio, m))
    return ratio


def test_the_bound_holds_on_the_device(world, oracle):
    """test 4 of the issue: |y32 - y64| <= filter_margin for every candidate of four lists, y32 from the device function stage F runs"""
    from sdpcutsel_via_nn_amd import synthetic
    L = N_VARS * (N_VARS + 1) // 2
    worst = []
    for s, vv in world.points.items():
        worst.append(_audit(world, oracle, N_VARS, world.Q, ALL_SETS, vv, "pattern point %d" % s))
    wl = synthetic.make_workload(nb_vars=100, k=3, count=4096, seed=7)
    worst.append(_audit(world, oracle, 100, wl["Q_arr"], wl["set_inds"][:, :3].astype(np.int32), wl["vars_values"], "n = 100, seed 7"))
    rng = np.random.default_rng(21)
    x = rng.integers(0, 2, size=N_VARS).astype(np.float64)      # x on its bounds, X = x x^T
    X = np.outer(x, x)
    worst.append(_audit(world, oracle, N_VARS, world.Q, ALL_SETS, np.concatenate([X[np.triu_indices(N_VARS)], x]), "x on its bounds"))
    Qs = np.where(rng.uniform(size=L) < 0.5, -7.0, 7.0)         # every |Q| equal: every |q| = 1/k
    worst.append(_audit(world, oracle, N_VARS, Qs, ALL_SETS, world.points[0], "|q| = 1/k"))
    assert max(worst) <= 1.0, worst


def test_outside_the_box_bypasses_the_filter(world, oracle):
    """test 5 of the issue: x = 1 + 1e-7 and x = -1e-7 are inside the +-3 clamp and outside the box the margin was derived on: the
    candidates that hold such a variable go to the fp64 pass whatever their fp32 measure"""
    rng = np.random.default_rng(0)
    x = rng.uniform(0.2, 0.8, N_VARS)
    out_vars = (5, 25, 30)
    x[5], x[25], x[30] = 1.0 + 1e-7, -1e-7, 1.0 + 1e-7
    X = np.outer(x, x)
    d = np.arange(20)
    X[d, d] += 0.05
    X[d + 20, d + 20] -= 0.05
    vv = np.concatenate([X[np.triu_indices(N_VARS)], x])
    L = N_VARS * (N_VARS + 1) // 2
    eig = oracle.eigmin_batch(3, vv[L:][ALL_SETS], vv[:L][oracle.triu_positions(ALL_SETS, N_VARS)])
    assert eig[NONVIOL].min() > 1e-3 and eig[~NONVIOL].max() < -1e-3
    _, me, obj = _measure(oracle, ALL_SETS, N_VARS, vv, world.Q)
    which = np.concatenate([np.arange(ALL_SETS.shape[0]), np.random.default_rng(9).integers(0, ALL_SETS.shape[0], size=2600)])
    viol = ~NONVIOL[which]
    outside = np.isin(ALL_SETS[which], out_vars).any(axis=1)
    r = (obj / me)[which]
    lo = int((viol & (outside | (r > 0))).sum())
    hi = int((viol & (outside | (r > -2 * world.margin))).sum())
    n_strong = int((viol & (r > 0)).sum())
    assert int((viol & outside).sum()) > 1000 and n_strong >= 20 and hi < int(viol.sum())
    handles = _handles(world, which, THREE)
    try:
        outs = _round(handles, "round_csr", 4, 20, vv)
        _all_same(outs, CSR_FIELDS, "outside the box")
        ev = _evaluated(handles[0])
        print("outside the box: evaluated", ev, "bounds", lo, hi, "violated", int(viol.sum()))
        assert lo <= ev <= hi, (ev, lo, hi)
        _scores_same(handles, "outside the box")
    finally:
        for sc in handles:
            sc.close()


def test_what_must_not_filter(world):
    """test 6 of the issue: a user network that is not filter_ok, a mixed list, strategy 2, a boxed round -- each reports the
    evaluations its launch makes without the option, and identical outputs"""
    from sdpcutsel_via_nn_amd import _capi, networks
    which, flags = base._layout(world, "fills", seed=5)
    two = ((2, 1), (2, 0))
    # a network of the shipped shape, clamp-free, whose margin lies above the cut-off (output weights doubled)
    widths, params = networks.load_network(3)
    _, offs, _ = networks.check_network(3, widths, params)
    p = params.copy()
    p[offs[3][0]:offs[3][1]] *= 2.0
    assert networks.unclamped_ok(3, widths, p) and not networks.filter_ok(3, widths, p)
    handles = _handles(world, which, two, net=(widths, p))
    try:
        assert all(np.isnan(sc.filter_margin(3)) for sc in handles)
        outs = _round(handles, "select_round", 4, 20, world.points[3])
        _all_same(outs, FIELDS, "user network")
        # (the violated candidates if this network's round stays in its strong regime, everybody if it had to complete: the same
        # on both handles, and never a filtered count)
        ev = [_evaluated(sc) for sc in handles]
        assert ev[0] == ev[1] and ev[0] in (int(flags.sum()), which.shape[0]), ev
        _scores_same(handles, "user network")
    finally:
        for sc in handles:
            sc.close()
    # a mixed list: the launch over all classes
    sets = np.full((which.shape[0], 5), -1, dtype=np.int32)
    sets[:, :3] = ALL_SETS[which]
    ks = np.full(which.shape[0], 3, dtype=np.int32)
    sets[::7, 2] = -1
    ks[::7] = 2
    handles = _handles(world, which, two, sets=sets, ks=ks)
    try:
        outs = _round(handles, "select_round", 4, 20, world.points[3])
        _all_same(outs, FIELDS, "mixed")
        assert [_evaluated(sc) for sc in handles] == [which.shape[0]] * 2
        _scores_same(handles, "mixed")
    finally:
        for sc in handles:
            sc.close()
    handles = _handles(world, which, two)
    try:
        assert all(abs(sc.filter_margin(3) - world.margin) <= 0.02 * world.margin for sc in handles)
        # strategy 2 ranks by the measure of every candidate
        outs = _round(handles, "select_round", 2, 300, world.points[3])
        _all_same(outs, FIELDS, "strategy 2")
        assert [_evaluated(sc) for sc in handles] == [which.shape[0]] * 2
        # a boxed round scores in two launches, nothing fused
        lb, ub = np.zeros(N_VARS), np.ones(N_VARS)
        ub[::3] = 0.9
        for sc in handles:
            sc.set_box(lb, ub)
        outs = _round(handles, "select_round", 4, 20, world.points[3])
        _all_same(outs, FIELDS, "boxed")
        assert [_evaluated(sc) for sc in handles] == [which.shape[0]] * 2
        _scores_same(handles, "boxed")
    finally:
        for sc in handles:
            sc.close()
