"""The staging of the mapped inputs in the skipping and the filtering kernel (csrc/score_mfma.hip: the loop between lambda_min and
the passes of score_mfma_body) reads its launch constants -- the input mapping and, for the filter, NetDev::filter_box -- from LDS,
and the box test of the nine features is one branch-free expression.  Nothing a round returns may move, and the bypass bit must be
the one the short-circuit test gave: set exactly when one of the candidate's mapped inputs lies outside its interval of the box.

The construction is that of tests/test_gpu_fp32_filter.py, imported: n = 40, the pattern point (tests/test_gpu_skip_nonviolated.py),
the 9 880 three-variable sets repeated to just past the 12 288 candidates from which the fused launch serves a combined round,
SDPCUT_OPT_SKIP_NONVIOLATED = 2.  Only the three x features of a candidate can leave the box with the LP point (the six q features
are Q / (3 max |Q|), inside [-1/3, 1/3] for every instance), one per member position: a variable J on the wrong side of a bound by
1e-6 -- 1000 times what networks.filter_box widens the domain's image by -- is feature 0 of the sets it leads, feature 1 of those
where it is the middle member and feature 2 of those it ends."""
import numpy as np
import pytest

import filter_tail_nets
import test_gpu_fp32_filter as f32
import test_gpu_skip_nonviolated as base

pytestmark = pytest.mark.gpu

N_VARS = base.N_VARS
ALL_SETS, NONVIOL = base.ALL_SETS, base.NONVIOL
FIELDS, CSR_FIELDS = base.FIELDS, base.CSR_FIELDS
THREE = f32.THREE                        # filtering | skipping only | scoring everybody
BOUNDARY_LENGTHS = (12352, 12353, 12415)      # 193 whole strips of 64; one candidate in the 194th; 63
J = 24                                   # leads 105 sets, is the middle member of 360 and the last of 276; all of them violated
SEL = 20


@pytest.fixture(scope="module")
def world(oracle):
    return f32._World(oracle)


def _repeated(n, seed, pool=None):
    """every set once, then draws from `pool` (default: all sets) up to n candidates"""
    rng = np.random.default_rng(seed)
    pool = np.arange(ALL_SETS.shape[0]) if pool is None else pool
    return np.concatenate([np.arange(ALL_SETS.shape[0]), rng.choice(pool, size=n - ALL_SETS.shape[0])])


def _sure_list(world, r, n, seed, allowed=None, extra=()):
    """A list whose fp64 evaluations are known from the oracle alone, as _fill_layout of test_gpu_fp32_filter.py builds it: of the
    `allowed` sets every strong one (violated, r = obj / max_elem > 0: survives by the proof) once, then `extra`, then draws from the
    violated sets with r <= -2 margin (cannot survive) and, an eighth, from the non-violated ones without a positive measure; shuffled"""
    rng = np.random.default_rng(seed)
    allowed = np.ones(ALL_SETS.shape[0], dtype=bool) if allowed is None else allowed
    strong = np.flatnonzero(allowed & ~NONVIOL & (r > 0))
    out = np.flatnonzero(allowed & ~NONVIOL & (r <= -2 * world.margin))
    free = np.flatnonzero(allowed & NONVIOL & (r <= 0))      # (a non-violated candidate with a positive measure moves nb_positive)
    rest = n - strong.size - len(extra)
    which = np.concatenate([strong, np.asarray(extra, dtype=np.int64), rng.choice(out, size=rest - rest // 8), rng.choice(free, size=rest // 8)])
    return rng.permutation(which)


def _pattern_point(x):
    """the LP point of base._point for a given x: X = x x^T, +0.05 on the first 20 diagonal entries, -0.05 on the last 20"""
    X = np.outer(x, x)
    d = np.arange(20)
    X[d, d] += 0.05
    X[d + 20, d + 20] -= 0.05
    return np.concatenate([X[np.triu_indices(N_VARS)], x])


def _base_x():
    return np.random.default_rng(3).uniform(0.2, 0.8, N_VARS)      # x of base._point(3) = world.points[3]


def _oracle_view(world, oracle, vv, which):
    """-> (violated flag, obj / max_elem) of every candidate of the list at point vv, the pattern asserted with the oracle"""
    L = N_VARS * (N_VARS + 1) // 2
    eig = oracle.eigmin_batch(3, vv[L:][ALL_SETS], vv[:L][oracle.triu_positions(ALL_SETS, N_VARS)])
    assert eig[NONVIOL].min() > 1e-3 and eig[~NONVIOL].max() < -1e-3
    _, me, obj = f32._measure(oracle, ALL_SETS, N_VARS, vv, world.Q)
    return ~NONVIOL[which], (obj / me)[which]


def _rounds_same(handles, vv, what):
    """select_round and round_csr on the three handles at vv: everything they return byte for byte, then both score arrays in full
    -> SDPCUT_STAT_NN_EVALUATED of the filtering handle's round_csr launch"""
    ev = None
    for call, fields in (("select_round", FIELDS), ("round_csr", CSR_FIELDS)):
        outs = f32._round(handles, call, 4, SEL, vv)
        f32._all_same(outs, fields, (what, call))
        ev = [f32._evaluated(sc) for sc in handles]
    f32._scores_same(handles, what)
    return ev


@pytest.mark.parametrize("n", BOUNDARY_LENGTHS)
def test_byte_identity_at_strip_boundaries(world, n):
    """a list that ends on a strip boundary, one candidate behind it and one short of the next: the filtering launch against the
    skipping one and against the launch that scores everybody"""
    which = _repeated(n, seed=n)
    flags = ~NONVIOL[which]
    assert which.shape[0] == n > 12288 and int(np.isin(which, world.strong).sum()) >= SEL
    lo, hi = f32._bounds(world, which, flags)
    handles = f32._handles(world, which, THREE)
    try:
        ev = _rounds_same(handles, world.points[3], ("boundary", n))
        print("boundary", n, "evaluated", ev, "bounds", lo, hi, "violated", int(flags.sum()))
        assert lo <= ev[0] <= hi and ev[1] == int(flags.sum()) and ev[2] == n
    finally:
        for sc in handles:
            sc.close()


@pytest.fixture(scope="module")
def bypass_list(world):
    """12 353 candidates: every set that holds J four times, and of the sets without J only those whose fate the oracle decides --
    the strong ones, sets the filter must drop, non-violated ones.  (x_J enters the inputs of no set without J: their measures are
    the same at the three points below.)"""
    holds = (ALL_SETS == J).any(axis=1)
    which = _sure_list(world, world.r[3], 12353, seed=5, allowed=~holds, extra=np.tile(np.flatnonzero(holds), 4))
    handles = f32._handles(world, which, THREE)
    yield which, handles
    for sc in handles:
        sc.close()


def test_inside_the_box_nobody_bypasses(world, bypass_list):
    """the pattern point itself, every x in [0.2, 0.8]: the evaluated count inside the oracle's bounds, which lie below the number
    of violated candidates that hold J"""
    which, handles = bypass_list
    flags = ~NONVIOL[which]
    lo, hi = f32._bounds(world, which, flags)
    assert which.shape[0] == 12353 and np.array_equal(base._point(3), _pattern_point(_base_x()))
    assert lo >= SEL and hi < int((flags & (ALL_SETS[which] == J).any(axis=1)).sum())
    ev = _rounds_same(handles, world.points[3], "inside")
    print("inside: evaluated", ev, "bounds", lo, hi, "violated", int(flags.sum()))
    assert lo <= ev[0] <= hi, (ev[0], lo, hi)


@pytest.mark.parametrize("value", [1.0 + 1e-6, -1e-6])
def test_the_bypass_bit_feature_by_feature(world, oracle, bypass_list, value):
    """x_J outside [0, 1] by 1e-6: every violated candidate that holds J -- as its first, second or third member -- is evaluated in
    fp64 whatever its fp32 measure.  A test dropped, overwritten or taken from another feature when the nine are merged loses the
    candidates of one position: each position alone holds more candidates that the filter would drop (measure below -2 margin)
    than there are candidates without J that may survive, so the count falls below the number of violated candidates with J."""
    which, handles = bypass_list
    x = _base_x()
    x[J] = value
    vv = _pattern_point(x)
    viol, r = _oracle_view(world, oracle, vv, which)
    sets = ALL_SETS[which]
    holds = (sets == J).any(axis=1)
    assert np.array_equal(r[~holds], world.r[3][which][~holds])
    others_hi = int((viol & ~holds & (r > -2 * world.margin)).sum())
    for pos in range(3):
        droppable = int((viol & (sets[:, pos] == J) & (r <= -2 * world.margin)).sum())
        assert droppable > others_hi, (pos, droppable, others_hi)
    lo = int((viol & (holds | (r > 0))).sum())
    hi = int((viol & (holds | (r > -2 * world.margin))).sum())
    assert int((viol & (r > 0)).sum()) >= SEL and lo == hi < int(viol.sum())
    ev = _rounds_same(handles, vv, ("bypass", value))
    # what the device itself says of the list: violated candidates with J at each position
    eig, _ = handles[2].get_scores()
    got_sets = handles[2].get_candidates(np.arange(which.shape[0]))[0][:, :3]
    dev_viol = eig < -1e-15
    for pos in range(3):
        assert int((dev_viol & (got_sets[:, pos] == J)).sum()) > 0, pos
    n_hold = int((dev_viol & (got_sets == J).any(axis=1)).sum())
    print("bypass x_J = %r: evaluated" % value, ev, "violated with J", n_hold, "bounds", lo, hi, "others that may survive", others_hi)
    assert n_hold == int((viol & holds).sum())
    assert ev[0] >= n_hold, (ev[0], n_hold)
    assert lo <= ev[0] <= hi, (ev[0], lo, hi)


def test_domain_corners_do_not_bypass(world, oracle):
    """variables at exactly 0.0 and exactly 1.0 map onto the ends of the box (inclusive bounds, widened by 1e-9): no candidate
    bypasses on their account.  On a list of sure candidates the oracle's bounds coincide: a single bypass among the more than 1000
    droppable candidates that hold a corner variable shows"""
    x = _base_x()
    zeros, ones = (2, 22, 31), (7, 27, 38)
    x[list(zeros)] = 0.0
    x[list(ones)] = 1.0
    vv = _pattern_point(x)
    _, r_sets = _oracle_view(world, oracle, vv, np.arange(ALL_SETS.shape[0]))
    which = _sure_list(world, r_sets, 12353, seed=11)
    viol, r = ~NONVIOL[which], r_sets[which]
    corner = np.isin(ALL_SETS[which], zeros + ones).any(axis=1)
    world.r["corners"] = r_sets      # (the oracle's bounds by the helper of test_gpu_fp32_filter.py, at this point)
    lo, hi = f32._bounds(world, which, viol, s="corners")
    assert which.shape[0] == 12353 and SEL <= lo == hi and int((viol & corner & (r <= -2 * world.margin)).sum()) > 1000
    handles = f32._handles(world, which, THREE)
    try:
        ev = _rounds_same(handles, vv, "corners")
        print("corners: evaluated", ev, "bounds", lo, hi, "violated", int(viol.sum()), "of them with a corner variable", int((viol & corner).sum()))
        assert lo <= ev[0] <= hi, (ev[0], lo, hi)
    finally:
        for sc in handles:
            sc.close()


def _clamped_net():
    """the "speaks" network of filter_tail_nets with one first-layer bias at 60: neuron 0 of layer 1 saturates, the network is no
    longer provably clamp-free (nor filtering) and still depends on every input"""
    from sdpcutsel_via_nn_amd import networks
    widths, params = filter_tail_nets.tail_network("speaks")
    params = params.copy()
    networks.split_params(3, widths, params)[4][0][0] = 60.0
    return widths, params


def test_the_skipping_kernel_on_a_clamped_user_network(world, oracle):
    """a user network that does not filter (clamped: score_mfma_skip_kernel with the tansig clamps reads the mapping from LDS too):
    skipping against scoring everybody on a 12 353-candidate list.  (The list leaves out the non-violated sets this network gives a
    positive measure: nb_positive is the one documented difference of a skipping round.)"""
    from sdpcutsel_via_nn_amd import networks
    net = _clamped_net()
    assert not networks.unclamped_ok(3, *net) and not networks.filter_ok(3, *net)
    _, _, obj = filter_tail_nets.measure(oracle, net, ALL_SETS, N_VARS, world.points[3], world.Q)
    assert np.abs(obj).min() > 1e-3
    which = _repeated(12353, seed=12353, pool=np.flatnonzero(~NONVIOL | (obj <= 0)))
    which = which[~(NONVIOL & (obj > 0))[which]]
    which = np.concatenate([which, which[:12353 - which.shape[0]]])
    flags = ~NONVIOL[which]
    assert which.shape[0] == 12353 and int((flags & (obj[which] > 0)).sum()) >= SEL
    handles = f32._handles(world, which, ((2, 1), (0, 1)), net=net)
    try:
        assert all(np.isnan(sc.filter_margin(3)) for sc in handles)
        ev = _rounds_same(handles, world.points[3], "clamped user network")
        print("clamped user network: evaluated", ev, "violated", int(flags.sum()))
        # (the skipping launch served the round: it evaluated the violated candidates and nobody else)
        assert ev == [int(flags.sum()), which.shape[0]], ev
    finally:
        for sc in handles:
            sc.close()
