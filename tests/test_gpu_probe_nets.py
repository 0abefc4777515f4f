"""The premises of the fp32 filter's margin and of the fp64 fast tansig, one at a time, on the device: the probe networks of
tests/probe_nets.py (their own premises are held without a GPU by tests/test_probe_nets_cpu.py).

Family A  |y32 - y64| <= m <= sdpcut_get_filter_margin on networks whose margin per candidate is 13 .. 26 u (u = 2^-24): the 13 u
          charged for v_exp_f32 / v_rcp_f32, tested at a resolution of 13 u; a saturated activation is exactly +-1.
Family B  |y32 - y64| <= the premise-level bound of the accumulation chain (rounding counts gamma(m_j), conversions, two
          activations behind it) on a matrix-core row and a tail row, for coherent, random and sorted terms.
Family C  every fp64 kernel within its documented per-activation constant of the long double reference at chosen arguments,
          clamp-free and clamped, with the neurons that share the reciprocal of tansig4 saturated either way.
One round  a strategy-4 round on a Family A network whose measures lie within +-64 u of zero, filter on and off, byte for byte.

y64 is the long double reference (networks.forward_twin in np.longdouble; for a one-path network its closed form).  Every figure is
printed (run with -s); profiles/premise_probes.txt records what an MI355X gave."""
import numpy as np
import pytest

import probe_nets as pn
import test_gpu_filter_slope_margin as fsm
import user_nets
from sdpcutsel_via_nn_amd import _capi, networks

pytestmark = pytest.mark.gpu

U = pn.U
LD = np.longdouble
KERNELS = (("mfma", _capi.KERNEL_MFMA), ("valu", _capi.KERNEL_VALU), ("simple", _capi.KERNEL_SIMPLE))


class _FilterList(object):
    """one handle over a probe list of 3-variable candidates: set_network, set_point, filter_audit_margins per network"""

    def __init__(self, n, Q, sets, vv):
        import sdpcutsel_via_nn_amd as lib
        self.vv = vv
        self.sc = lib.Scorer(0)
        try:
            self.sc.set_builtin_networks(5)
            self.sc.set_instance(n, Q)
            self.sc.set_candidates(*user_nets.padded(sets))
        except Exception:
            self.sc.close()
            raise

    def audit(self, p):
        """-> (y32, m, a-priori margin) of network p on the list"""
        self.sc.set_network(3, *p.net)
        self.sc.set_point(self.vv)
        m0 = self.sc.filter_margin(3)
        y32, m = self.sc.filter_audit_margins()
        return y32, m, m0

    def close(self):
        self.sc.close()


def _twin_margins(p, inputs):
    """the twin's margin of every candidate and the slack rule of test_gpu_filter_slope_margin.py: the device's margin may differ
    by 2 sum_j G_j e_j (1 - a^2 moves by at most 2 e_j per neuron) and 2^-8 of the twin's"""
    m_twin = networks.filter_margin_at(3, p.widths, p.params, inputs)
    G, _, _, e = networks.filter_margin_terms(3, *p.net)
    return m_twin, 2.0 * float((G[:e.shape[0]] * e).sum()) + 2.0 ** -8 * m_twin


def _check_margins(p, y32, m, m0, y64, inputs):
    """|y32 - y64| <= m <= the a-priori margin, the a-priori margin is the twin's, m is the twin's up to the slack -> |y32 - y64|"""
    err = np.abs(y32.astype(LD) - y64).astype(np.float64)
    m_twin, slack = _twin_margins(p, inputs)
    want0 = networks.filter_margin(3, *p.net)
    assert abs(m0 - want0) <= 1e-9 * want0, p.name
    assert np.all(np.isfinite(y32)) and np.all(np.isfinite(m)) and np.all(m > 0.0), p.name
    assert np.all(err <= m), (p.name, float((err / m).max()), float(err.max() / U))
    assert np.all(m <= m0), p.name
    assert np.all(np.abs(m - m_twin) <= slack), (p.name, float(np.abs(m - m_twin).max() / U))
    return err


def _bucket_names(edges, what):
    return ["%s = 0" % what] + ["%g < %s <= %g" % (edges[i - 1], what, edges[i]) for i in range(1, len(edges))]


def test_family_a_one_fp32_activation_at_a_time():
    """Layer-3 probes: 85 + 49 networks x 1024 candidates, margins of 13 .. 26 u.  At |b3| >= 39 the output is exactly +-1.0.  Layer-1
    probes: the one-term chain z1 = fl32(fl32(c w1) v32) and three activations at slope <= 1.  The largest |y32 - y64| in u per
    bucket of |z| of the probed activation is printed: the hardware's activation error as this repository first measured it."""
    n, Q, sets, vv, inputs, x, v = pn.a_points()
    lst = _FilterList(n, Q, sets, vv)
    worst = {name: np.zeros(len(pn.Z_BUCKETS) + 1) for name in ("A3", "A3w", "A1")}
    ratio = {name: 0.0 for name in worst}
    try:
        for p in pn.family_a3() + pn.family_a3_wide():
            y32, m, m0 = lst.audit(p)
            err = _check_margins(p, y32, m, m0, pn.closed_form(p, x), inputs)
            assert np.all(m <= 26.0 * U * (1.0 + 2.0 ** -7)), (p.name, float(m.max() / U))
            if abs(p.b3) >= 39.0:      # the premise Family B builds on: a saturated activation is exact
                assert np.all(y32 == np.sign(p.b3)), (p.name, float(np.abs(y32 - np.sign(p.b3)).max()))
            b = pn.bucket(pn.C * p.b3)
            worst[p.family][b] = max(worst[p.family][b], err.max() / U)
            ratio[p.family] = max(ratio[p.family], float((err / m).max()))
        for p in pn.family_a1():
            y32, m, m0 = lst.audit(p)
            err = _check_margins(p, y32, m, m0, pn.closed_form(p, x), inputs)
            z1 = pn.predict_z1(p.path[1][0], v)
            buckets = np.searchsorted(pn.Z_BUCKETS, np.abs(z1.astype(np.float64)), side="left")
            for b in np.unique(buckets):
                worst["A1"][b] = max(worst["A1"][b], err[buckets == b].max() / U)
            ratio["A1"] = max(ratio["A1"], float((err / m).max()))
    finally:
        lst.close()
    for name, what in (("A3", "layer-3 probes"), ("A3w", "layer-3 probes, link 2 = 1"), ("A1", "layer-1 probes")):
        print("%s: max |y32 - y64| / m = %.3f; max |y32 - y64| in u per bucket: " % (what, ratio[name])
              + ", ".join("%s: %.2f" % (t, e) for t, e in zip(_bucket_names(pn.Z_BUCKETS, "|z|"), worst[name])))
    assert ratio["A3"] > 0.0 and ratio["A3w"] > 0.0


def test_family_b_the_fp32_accumulation_chain():
    """|y32 - y64| <= the premise-level bound (saturated layer exact, gamma(m_j) and conversions of the probed row, 13 u and a
    one-term chain for each of the two activations behind it) and <= m; observed / bound per pattern, matrix-core and tail rows"""
    n, Q, sets, vv, inputs = pn.b_points()
    lst = _FilterList(n, Q, sets, vv)
    seen = {}
    try:
        for p in pn.family_b():
            y32, m, m0 = lst.audit(p)
            with np.errstate(over="ignore"):
                y64 = networks.forward_twin(3, p.widths, p.params, inputs, dtype=LD)
            err = _check_margins(p, y32, m, m0, y64, inputs)
            bound = pn.premise_bound(p)
            emu, delta = pn.chain_error(p)
            where = "tail" if p.chain[0] >= 48 else "mfma"
            print("%s: |y32 - y64| = %.1f u, premise-level bound %.1f u (%.3f), emulated chain %.1f u, m = %.1f u"
                  % (p.name, err.max() / U, bound / U, err.max() / bound, emu, m.max() / U))
            assert np.all(err <= bound), (p.name, float(err.max() / U), bound / U)
            seen.setdefault((p.pattern, where), []).append(float(err.max() / bound))
    finally:
        lst.close()
    for key, r in sorted(seen.items()):
        print("observed / bound, %s on %s rows: %.3f .. %.3f" % (key + (min(r), max(r))))


@pytest.mark.parametrize("variant", ("clamp-free", "clamped"))
@pytest.mark.parametrize("k", (2, 3, 4, 5))
def test_family_c_one_fp64_activation_at_a_time(k, variant):
    """score(NN) under the MFMA, the VALU and the simple kernel and nn_batch on the same inputs, each within probe_nets.c_allowance
    of the long double reference for its documented per-activation bound; no subnormal, infinite or NaN score anywhere, the
    companion-saturated cases included"""
    import sdpcutsel_via_nn_amd as lib
    n, Q, sets, vv, inputs, x = pn.c_points(k)
    free, clamped = pn.family_c(k)
    nets = free if variant == "clamp-free" else clamped
    worst = {}
    tightest = {}
    sc = lib.Scorer(0)
    try:
        sc.set_network(k, *nets[0].net)
        sc.set_instance(n, Q)
        sc.set_candidates(*user_nets.padded(sets))
        for p in nets:
            assert networks.unclamped_ok(k, *p.net) == (variant == "clamp-free")
            sc.set_network(k, *p.net)
            ref = pn.closed_form(p, x)
            n_probe = np.abs(pn.path_activations(p, x)[p.probe][0].astype(np.float64))
            buckets = np.searchsorted(pn.N_BUCKETS, n_probe, side="left")
            got = {}
            for name, variant_id in KERNELS:
                sc.set_option(_capi.OPT_KERNEL, variant_id)
                sc.set_point(vv)
                sc.score(_capi.NN)
                got[name] = sc.get_scores(eig=False)[1]
            got["nn_batch"] = sc.nn_batch(k, inputs)
            for name, obj in got.items():
                allow = pn.c_allowance(p, x, name)
                err = np.abs(obj.astype(LD) - ref).astype(np.float64)
                assert np.all(np.isfinite(obj)), (p.name, name)
                assert np.all((obj == 0.0) | (np.abs(obj) >= np.finfo(np.float64).tiny)), (p.name, name)
                for b in np.unique(buckets):
                    key = (name, int(b))
                    worst[key] = max(worst.get(key, 0.0), float(err[buckets == b].max()))
                at = int(np.argmax(err / allow))
                tightest[name] = max(tightest.get(name, 0.0), float(err[at] / allow[at]))
                assert np.all(err <= allow), (p.name, name, float(x[at]), float(err[at]), float(allow[at]))
    finally:
        sc.close()
    names = _bucket_names(pn.N_BUCKETS, "|n|")
    for name in ("mfma", "valu", "simple", "nn_batch"):
        print("k %d %s, %s (bound %.2g per activation): max error / allowance %.3f; max |obj - ref| per bucket: " %
              (k, variant, name, pn.ACT_BOUND[pn.KERNEL_ACT[name]], tightest[name])
              + ", ".join("%s: %.2e" % (names[b], worst[(name, b)]) for b in range(len(names)) if (name, b) in worst))


class _RoundCase(object):
    """what _round_checks of test_gpu_filter_slope_margin.py reads of a case, for a probe network"""

    def __init__(self, oracle, p, n, Q, sets, vv, inputs, x):
        self.net_name, self.net, self.n_vars, self.Q, self.sets, self.vv = p.name, p.net, n, Q, sets, vv
        L = n * (n + 1) // 2
        self.eig = oracle.eigmin_batch(3, vv[L:][sets], vv[:L][oracle.triu_positions(sets, n)])
        self.r = pn.closed_form(p, x).astype(np.float64)      # max_elem = 1, S = 0: obj / max_elem is the network's output
        self.m_twin = networks.filter_margin_at(3, p.widths, p.params, inputs)


def test_one_round_where_a_margin_of_13_u_decides(oracle):
    """A strategy-4 round_csr / select_round on the round-check network, its list tiled to 13 312 candidates (above FILTERS_FROM),
    with the filter on and off: head, scores, rows and counters byte for byte, and STAT_NN_EVALUATED inside the bounds the twin's
    margins give.  Every candidate is violated, the measures run over +-64 u: the filter drops a good part of the list on a margin
    of 13 u, and a strong candidate lost to it would change the head."""
    p = pn.round_net()
    n, Q, sets, vv, inputs, x, v = pn.round_points()
    c = _RoundCase(oracle, p, n, Q, sets, vv, inputs, x)
    assert np.all(c.eig < -fsm.TIE) and np.all(np.abs(c.r) > fsm.TIE)
    assert np.all(c.m_twin <= 26.0 * U)
    strong = int((c.r > 0).sum())
    may_drop = int((c.r < -2.0 * c.m_twin).sum())
    band = int(((c.r <= 0) & (c.r >= -2.0 * c.m_twin)).sum())
    print("round check: %d candidates, measures %.2f .. %.2f u, %d strong, %d below -2 m, %d in between; m_twin %.2f .. %.2f u"
          % (c.r.shape[0], c.r.min() / U, c.r.max() / U, strong, may_drop, band, c.m_twin.min() / U, c.m_twin.max() / U))
    assert strong >= 100 and may_drop >= 20 and band >= 100
    reps = -(-fsm.FILTERS_FROM // sets.shape[0])
    which = np.tile(np.arange(sets.shape[0]), reps)
    ev = fsm._round_checks(c, which, None, "probe list x %d" % reps)
    assert ev is not None and reps * strong <= ev <= reps * (sets.shape[0] - may_drop)
    assert ev < which.shape[0]      # real drops
