"""The VALU tail of the fp32 filter's pass (csrc/score_mfma.hip: filter_pass_f32 runs neurons 48 and 49 of every hidden layer on the
VALU, the other 48 on the matrix core), on the device:
  1. the shipped network's audit: every |y32 - y64| inside the margin, and the largest no more than four times what the pass with
     all four row tiles on the matrix core gave on the same lists (1.00e-5, profiles/fp32_filter_ab.txt: a reordering changes
     roundings, a wrong term changes magnitudes; re-measured side by side, profiles/fp32_tail_ab.txt: 1.003e-5 then, 9.38e-6 now);
  2. the audit of the three tail networks of tests/filter_tail_nets.py, in which a dropped, swapped or misplaced tail neuron moves
     the output by more than ten margins (tests/test_filter_tail_cpu.py), on the same lists and on lists of 1, 17, 48 and 257
     candidates (partial tiles, stale padding columns);
  3. rounds with those networks: filtering, skipping only and scoring everybody return the same bytes, and the number of fp64
     evaluations of the filtering launch lies between its two bounds from the float64 twin.
The lists and helpers are those of tests/test_gpu_fp32_filter.py and tests/test_gpu_skip_nonviolated.py, imported."""
import numpy as np
import pytest

import filter_tail_nets as ftn
import test_gpu_fp32_filter as fp
import test_gpu_skip_nonviolated as base

pytestmark = pytest.mark.gpu

N_VARS = base.N_VARS
ALL_SETS, NONVIOL = base.ALL_SETS, base.NONVIOL
PARENT_AUDIT_MAX = 1.00e-5      # largest |y32 - y64| of the four-tile pass on the lists of test 1 (profiles/fp32_filter_ab.txt, section 2)
SHORT = (1, 17, 48, 257)


@pytest.fixture(scope="module")
def world(oracle):
    return base._World(oracle)


@pytest.fixture(scope="module")
def synth():
    from sdpcutsel_via_nn_amd import synthetic
    return synthetic.make_workload(nb_vars=100, k=3, count=4096, seed=7)


def _lists(world, synth):
    """(what, n_vars, Q, sets, point) of the audits"""
    out = [("pattern point %d" % s, N_VARS, world.Q, ALL_SETS, vv) for s, vv in world.points.items()]
    out.append(("n = 100, seed 7", 100, synth["Q_arr"], synth["set_inds"][:, :3].astype(np.int32), synth["vars_values"]))
    return out


def _audit(oracle, net, n_vars, Q, sets, vv):
    """-> (y32 of the device's fp32 pass, y64 of the float64 twin, the device's margin); net = None: the shipped network"""
    import sdpcutsel_via_nn_amd as lib
    from sdpcutsel_via_nn_amd import networks
    sc = lib.Scorer(0)
    try:
        sc.set_builtin_networks(5)
        if net is not None:
            sc.set_network(3, *net)
        sc.set_instance(n_vars, Q)
        pad = np.full((sets.shape[0], 5), -1, dtype=np.int32)
        pad[:, :3] = sets
        sc.set_candidates(pad, np.full(sets.shape[0], 3, dtype=np.int32))
        sc.set_point(vv)
        m = sc.filter_margin(3)
        y32 = sc.filter_audit()
    finally:
        sc.close()
    y64 = ftn.measure(oracle, net if net is not None else networks.load_network(3), sets, n_vars, vv, Q)[0]
    return y32, y64, m


def test_shipped_network_audit(world, synth, oracle):
    from sdpcutsel_via_nn_amd import networks
    want = networks.filter_margin(3, *networks.load_network(3))
    worst = 0.0
    for what, n_vars, Q, sets, vv in _lists(world, synth):
        y32, y64, m = _audit(oracle, None, n_vars, Q, sets, vv)
        assert abs(m - want) <= 0.02 * want
        err = float(np.abs(y32 - y64).max())
        print("shipped network, %s: %d candidates, max |y32 - y64| = %.3g = %.3g of the margin %.6f" % (what, sets.shape[0], err, err / m, m))
        assert np.isfinite(y32).all() and err <= m, (what, err, m)
        worst = max(worst, err)
    print("shipped network: largest |y32 - y64| %.3g, the four-tile pass had %.3g" % (worst, PARENT_AUDIT_MAX))
    assert worst <= 4.0 * PARENT_AUDIT_MAX, worst


@pytest.mark.parametrize("name", ftn.NAMES)
def test_tail_network_audit(world, synth, oracle, name):
    from sdpcutsel_via_nn_amd import networks
    net = ftn.tail_network(name)
    want = networks.filter_margin(3, *net)
    cases = _lists(world, synth)
    rng = np.random.default_rng(5)
    for n in SHORT:      # short lists: a partial tile, a lone tile, padding columns that hold what the pass before left
        cases.append(("%d sets" % n, N_VARS, world.Q, ALL_SETS[rng.choice(ALL_SETS.shape[0], size=n, replace=False)], world.points[3]))
    for what, n_vars, Q, sets, vv in cases:
        y32, y64, m = _audit(oracle, net, n_vars, Q, sets, vv)
        assert abs(m - want) <= 0.02 * want, (name, m, want)
        assert y32.shape == y64.shape and np.isfinite(y32).all(), (name, what)
        err = float(np.abs(y32 - y64).max())
        print("%s, %s: %d candidates, max |y32 - y64| = %.3g = %.3g of the margin %.4g" % (name, what, sets.shape[0], err, err / m, m))
        assert err <= m, (name, what, err, m)


@pytest.mark.parametrize("name", ftn.NAMES)
def test_tail_network_rounds(world, oracle, name):
    from sdpcutsel_via_nn_amd import _capi, networks
    net = ftn.tail_network(name)
    m = networks.filter_margin(3, *net)
    vv = world.points[3]
    _, me, obj = ftn.measure(oracle, net, ALL_SETS, N_VARS, vv, world.Q)
    r = obj / me
    for kind in ("fills", "runs"):
        which, flags = base._layout(world, kind)
        n_viol = int(flags.sum())
        lo, hi = int((flags & (r[which] > 0)).sum()), int((flags & (r[which] > -2 * m)).sum())
        n_strong = lo
        print("%s, %s: %d candidates, %d violated, %d strong, %d within two margins" % (name, kind, which.shape[0], n_viol, lo, hi))
        # what the lists must hold for the counts below to say something (from the twin alone)
        assert lo >= 10 or name == "heard", (name, kind, lo)
        assert lo >= 1
        assert hi < n_viol // 2 or name == "both", (name, kind, hi, n_viol)
        handles = fp._handles(world, which, fp.THREE, net=net)
        try:
            assert all(abs(sc.filter_margin(3) - m) <= 0.02 * m for sc in handles)
            for sel in (20, n_strong):
                for call, fields in (("round_csr", base.CSR_FIELDS), ("select_round", base.FIELDS)):
                    done0 = handles[0].get_stat(_capi.STAT_NN_COMPLETIONS)
                    outs = fp._round(handles, call, 4, sel, vv)
                    done = handles[0].get_stat(_capi.STAT_NN_COMPLETIONS) - done0
                    ev = [fp._evaluated(sc) for sc in handles]
                    # In these networks non-violated candidates have positive measures, and nb_positive of a skipping round in its
                    # strong regime counts the violated ones only (include/sdpcut.h; pinned by test_gpu_skip_nonviolated.py): that
                    # counter is held to the scores themselves, everything else to the bytes of the filtering handle.
                    fp._all_same(outs[:2], fields, (name, kind, sel, call))
                    eig, obj_dev = handles[2].get_scores()
                    assert np.array_equal(eig < -1e-15, flags)
                    want_pos = int((obj_dev > 0).sum()), int(((obj_dev > 0) & flags).sum())
                    assert want_pos[0] >= want_pos[1] > 0
                    assert outs[2]["counters"]["nb_positive"] == want_pos[0]
                    assert outs[0]["counters"]["nb_positive"] == (want_pos[1] if done == 0 else want_pos[0]), (outs[0]["counters"], want_pos, done)
                    everybody = dict(outs[2], counters=dict(outs[2]["counters"], nb_positive=outs[0]["counters"]["nb_positive"]))
                    base._same(outs[0], everybody, fields, (name, kind, sel, call, "scoring everybody"))
                    print(name, kind, sel, call, "evaluated", ev, "bounds", lo, hi, "completions", done)
                    if sel <= n_strong:      # the head is filled from the strong class: the filtering launch's own count stands
                        assert done == 0
                        assert lo <= ev[0] <= hi, (name, kind, sel, ev[0], lo, hi)
                        assert ev[1] == n_viol and ev[2] == which.shape[0]
                    else:                    # fewer strong candidates than the head asks for: the round completes everybody
                        assert done == 1 and ev == [which.shape[0]] * 3
                    fp._scores_same(handles, (name, kind, sel, call))
        finally:
            for sc in handles:
                sc.close()
