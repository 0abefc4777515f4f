"""The margin PER CANDIDATE of the fp32 filter on the device (csrc/score_mfma.hip: filter_cand_margin; the derivation is in
csrc/net_pack.h at net_filter_slope_terms).  sdpcut_filter_audit_margins returns, from the device function stage F runs, the fp32
output and the margin of every candidate:  |y32 - y64| <= m <= sdpcut_get_filter_margin  must hold for each of them, and m must be
the twin's value up to what the fp32 activations can move it.  Rounds under the option must stay what they are without it, bit for
bit, and evaluate in fp64 no more than the twin's margins allow.

Lists: the pattern list of tests/test_gpu_skip_nonviolated.py (n = 40, 9 880 sets, points 0 and 3), the 4096 synthetic sets
(n = 100, seed 7), lists of 1, 17, 48 and 257 sets, "fills" and "runs"; the shipped network and the three tail networks of
tests/filter_tail_nets.py."""
import numpy as np
import pytest

import filter_tail_nets
import test_gpu_fp32_filter as f32
import test_gpu_skip_nonviolated as base

pytestmark = pytest.mark.gpu

N_VARS, ALL_SETS = base.N_VARS, base.ALL_SETS
SMALL = (1, 17, 48, 257)
NETS = ("shipped",) + filter_tail_nets.NAMES
TIE = 1e-9      # an eigenvalue this close to its threshold, or a measure this close to zero, may fall on either side on the device


def _net(name):
    from sdpcutsel_via_nn_amd import networks
    return networks.load_network(3) if name == "shipped" else filter_tail_nets.tail_network(name)


class _Case(object):
    """one list of 3-variable sets at one point, seen by the oracle under one network: lambda_min, max_elem, obj64 / max_elem, the
    network's inputs, the twin's margin of every candidate and the slack the device's margin may show against it"""

    def __init__(self, oracle, name, n_vars, Q, sets, vv):
        from sdpcutsel_via_nn_amd import networks
        self.net_name, self.n_vars, self.Q, self.sets, self.vv = name, n_vars, Q, sets, vv
        self.net = _net(name)
        L = n_vars * (n_vars + 1) // 2
        pos = oracle.triu_positions(sets, n_vars)
        self.eig = oracle.eigmin_batch(3, vv[L:][sets], vv[:L][pos])
        q = Q[pos]
        me = 3.0 * np.abs(q).max(axis=1)
        me[me == 0.0] = 1.0
        self.inputs = np.concatenate([vv[L:][sets], q / me[:, None]], axis=1)
        _, self.me, obj = filter_tail_nets.measure(oracle, self.net, sets, n_vars, vv, Q)
        self.r = obj / self.me
        self.m0 = networks.filter_margin(3, *self.net)
        self.m_twin = networks.filter_margin_at(3, self.net[0], self.net[1], self.inputs)
        G, _, _, e = networks.filter_margin_terms(3, *self.net)
        self.m_slack = 2.0 * float((G[:e.shape[0]] * e).sum())      # 1 - a^2 moves by at most 2 e_j per neuron

    def scorer(self):
        import sdpcutsel_via_nn_amd as lib
        sc = lib.Scorer(0)
        sc.set_builtin_networks(5)
        if self.net_name != "shipped":
            sc.set_network(3, *self.net)
        sc.set_instance(self.n_vars, self.Q)
        pad = np.full((self.sets.shape[0], 5), -1, dtype=np.int32)
        pad[:, :3] = self.sets
        sc.set_candidates(pad, np.full(self.sets.shape[0], 3, dtype=np.int32))
        return sc


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> list of (what, _Case), made once per network and shared by the tests"""
    from sdpcutsel_via_nn_amd import synthetic
    Q, _, _ = synthetic.make_instance(N_VARS, 7)
    points = {s: base._point(s) for s in (3, 0)}
    wl = synthetic.make_workload(nb_vars=100, k=3, count=4096, seed=7)
    rng = np.random.default_rng(5)
    order = rng.permutation(ALL_SETS.shape[0])
    made = {}

    def get(name):
        if name not in made:
            out = [("pattern point %d" % s, _Case(oracle, name, N_VARS, Q, ALL_SETS, vv)) for s, vv in points.items()]
            out.append(("synthetic", _Case(oracle, name, 100, wl["Q_arr"], wl["set_inds"][:, :3].astype(np.int32), wl["vars_values"])))
            for n in SMALL:
                out.append(("%d sets" % n, _Case(oracle, name, N_VARS, Q, ALL_SETS[order[:n]], points[3])))
            made[name] = out
        return made[name]
    return get


@pytest.mark.parametrize("name", NETS)
def test_the_margin_of_every_candidate(cases, name):
    """|y32 - y64| <= m <= sdpcut_get_filter_margin with y64 from sdpcut_nn_batch, and |m - m_twin| <= 2 sum_j G_j e_j + 2^-8 m_twin"""
    for what, c in cases(name):
        sc = c.scorer()
        try:
            sc.set_point(c.vv)
            m0 = sc.filter_margin(3)
            y32, m = sc.filter_audit_margins()
            y32_alone = sc.filter_audit()
            y64 = sc.nn_batch(3, c.inputs)
        finally:
            sc.close()
        assert abs(m0 - c.m0) <= 1e-9 * c.m0, (name, what)
        assert y32.tobytes() == y32_alone.tobytes(), (name, what)
        err = np.abs(y32 - y64)
        dm = np.abs(m - c.m_twin)
        print("%s, %s: %d candidates, max |y32 - y64| = %.3g, m in %.4g .. %.4g (a priori %.4g), max |y32 - y64| / m = %.3g, "
              "max |m - m_twin| = %.3g (allowed %.3g)" % (name, what, m.shape[0], err.max(), m.min(), m.max(), m0, (err / m).max(),
                                                          dm.max(), (c.m_slack + 2.0 ** -8 * c.m_twin).min()))
        assert np.all(np.isfinite(m)) and np.all(m > 0.0), (name, what)
        assert np.all(err <= m), (name, what, float((err / m).max()))
        assert np.all(m <= m0), (name, what)
        assert np.all(dm <= c.m_slack + 2.0 ** -8 * c.m_twin), (name, what, float(dm.max()))


FILTERS_FROM = 12352      # the shortest list of the existing filter tests: above the one-workgroup selection (TK_SMALLSEL_N = 12288),
#                           below which a round's scoring launch is not the fused one and nothing skips or filters


def _round_checks(c, which, flags, what, sel=None, filtering=True):
    """strategy 4 through round_csr and select_round on the list c.sets[which]: the filtering handle against the same list with
    SDPCUT_OPT_FP32_FILTER = 0 -- head, scores, rows, new_strat, counters and the score arrays byte for byte -- and, where the
    launch filters, the evaluated count against the oracle -> the evaluated count (None where the strong class is not known
    exactly or is empty: the round then completes the measure, and the count is the list's length)"""
    import sdpcutsel_via_nn_amd as lib
    from sdpcutsel_via_nn_amd import _capi
    r, eig, m_twin = c.r[which], c.eig[which], c.m_twin[which]
    viol_sure = eig < -TIE if flags is None else flags
    viol_may = eig < TIE if flags is None else flags
    # (a positive measure survives whatever its last bits are on the device: the bounds themselves need no slack)
    lo = int((viol_sure & (r > 0.0)).sum())
    hi = int((viol_may & (r > -2.0 * m_twin)).sum())
    n_strong = int((viol_may & (r > -TIE)).sum())
    fits = lo == n_strong and lo >= 1      # the strong class is known exactly: a head inside it stays in the strong regime
    if sel is None:
        sel = min(lo, 20) if fits else min(5, which.shape[0])
    pad = np.full((which.shape[0], 5), -1, dtype=np.int32)
    pad[:, :3] = c.sets[which]
    handles = []
    for filt in (1, 0):
        sc = lib.Scorer(0)
        sc.set_builtin_networks(5)
        if c.net_name != "shipped":
            sc.set_network(3, *c.net)
        sc.set_instance(c.n_vars, c.Q)
        sc.set_candidates(pad, np.full(which.shape[0], 3, dtype=np.int32))
        sc.set_option(_capi.OPT_SKIP_NONVIOLATED, 2)
        sc.set_option(_capi.OPT_FP32_FILTER, filt)
        handles.append(sc)
    ev = None
    try:
        for call, fields in (("round_csr", base.CSR_FIELDS), ("select_round", base.FIELDS)):
            done0 = handles[0].get_stat(_capi.STAT_NN_COMPLETIONS)
            outs = f32._round(handles, call, 4, sel, c.vv)
            f32._all_same(outs, fields, (c.net_name, what, call))
            done = handles[0].get_stat(_capi.STAT_NN_COMPLETIONS) - done0
            ev = [f32._evaluated(sc) for sc in handles]
            print("%s, %s, %s: %d candidates, head %d, evaluated %s, bounds %d .. %d, completions %d"
                  % (c.net_name, what, call, which.shape[0], sel, ev, lo, hi, done))
            if not filtering:
                assert ev[0] == ev[1], (c.net_name, what, call, ev)
            elif fits and sel <= lo:
                assert done == 0, (c.net_name, what, call)
                # the handle without the filter evaluated the violated candidates: the skipping launch ran on both
                assert int(viol_sure.sum()) <= ev[1] <= int(viol_may.sum()), (c.net_name, what, call, ev[1])
                assert lo <= ev[0] <= hi, (c.net_name, what, call, ev[0], lo, hi)
            f32._scores_same(handles, (c.net_name, what, call))
    finally:
        for sc in handles:
            sc.close()
    return ev[0] if filtering and fits and sel <= lo else None


@pytest.mark.parametrize("name", NETS)
def test_rounds_on_the_audited_lists(cases, name):
    """Every audited list as it is -- all of them are short enough for the one-workgroup selection, whose round scores in a launch
    that neither skips nor filters: same round, same evaluations -- and repeated until the fused launch serves it, where the
    filter decides: the bounds on the evaluated count are those of the list, times the repeats."""
    for what, c in cases(name):
        n = c.sets.shape[0]
        assert n < FILTERS_FROM
        _round_checks(c, np.arange(n), None, what, filtering=False)
        reps = -(-FILTERS_FROM // n)
        ev = _round_checks(c, np.tile(np.arange(n), reps), None, "%s x %d" % (what, reps))
        if name == "shipped" and what == "synthetic":
            # fewer fp64 evaluations than the a-priori rule gives on this list in the CPU replay
            a_priori = int(((c.eig < -TIE) & (c.r > -c.m0)).sum())
            assert ev is not None and ev < reps * a_priori, (ev, reps, a_priori)


@pytest.mark.parametrize("kind", ["fills", "runs"])
def test_rounds_on_fills_and_runs(oracle, cases, kind):
    """the lists of tests/test_gpu_fp32_filter.py: the head at exactly the strong count, where a dropped strong candidate shows"""
    world = f32._World(oracle)
    which, flags = base._layout(world, kind)
    c = dict(cases("shipped"))["pattern point 3"]
    n_strong = int(np.isin(which, world.strong).sum())
    ev = _round_checks(c, which, flags, kind, sel=n_strong)
    assert ev is not None and n_strong <= ev
