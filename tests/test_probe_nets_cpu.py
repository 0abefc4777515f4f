"""The premises of the probes of tests/probe_nets.py themselves, without a GPU, so that tests/test_gpu_probe_nets.py cannot be
vacuous: every network lands in the kernel variant it is meant for, the library's own margin is as tight on the probe inputs as the
probes claim (the caps are conditions on the INPUTS, chosen from the formula of the derivation), the restated premise-level bound is
the twin's bound term for term, a float32 emulation of the accumulation chain stays inside it and really exercises it, and the
long double reference of a one-path network is its closed form.  Every figure is printed (run with -s); profiles/premise_probes.txt
records them."""
import numpy as np
import pytest

import probe_nets as pn
import user_nets
from sdpcutsel_via_nn_amd import networks

U = pn.U


@pytest.fixture(scope="module")
def a_list():
    return pn.a_points()


@pytest.fixture(scope="module")
def fam():
    return {"A3": pn.family_a3(), "A3w": pn.family_a3_wide(), "A1": pn.family_a1(), "B": pn.family_b(), "round": [pn.round_net()]}


def test_grids_and_rows_cover_what_they_must(fam, a_list):
    """b3: at least 48 values inside (-40, 40), 0, the powers of two of 2^z, |z| up to 115; the mapped inputs exact in fp32 with a
    full significand; the first link no power of two; the probed rows: first and last row of every 16-row tile, every register slot
    of a C/D fragment, both tail rows, and the last row below H of every shipped shape"""
    g = np.array(pn.B3_GRID)
    assert g.shape[0] >= 48 and 0.0 in g and np.all(np.abs(g) < 40.0) and abs(pn.C) * np.abs(g).max() > 115.0
    for m in (1, 2, 3):
        for s in (-1.0, 1.0):
            assert np.any(g == s * m * pn.LN2H)
            assert abs(2.0 ** (pn.C * s * m * pn.LN2H) - 2.0 ** (-s * m)) < 1e-12
    x, v = a_list[5], a_list[6]
    bits = np.abs(v.astype(np.float32)).view(np.uint32)
    assert np.all(bits & 1 == 1) and np.all(v.astype(np.float32).astype(np.float64) == v) and np.all((x - 0.5) * pn.A_GAIN == v)
    for w1 in (pn.W1,) + pn.A1_LINKS:
        wt = np.float32(pn.C * w1)
        assert np.frexp(abs(w1))[0] != 0.5 and np.frexp(abs(float(wt)))[0] != 0.5
    assert int(np.float32(pn.C * pn.W1).view(np.uint32)) & 0xFFF != 0      # a shortened operand (19 bits or fewer) changes it
    want = {0, 15, 16, 31, 32, 47, 48, 49} | {0, 1, 2, 3}
    for layer in range(3):
        assert want <= {p.path[0][layer] for p in fam["A3"]}, layer
    assert want <= {p.path[0][0] for p in fam["A1"]}
    assert {r % 4 for r in pn.ROWS_MFMA} == {0, 1, 2, 3}
    for k, (H, nh) in user_nets.SHAPES.items():
        free, clamped = pn.family_c(k)
        for nets in (free, clamped):
            assert any(H - 1 in p.path[0] for p in nets) and any(0 in p.path[0] for p in nets), k
        shared = [pn.companion_rows(H, r) for r in (0, 17, 34, 47)]
        assert shared == [[4, 8, 12], [21, 25, 29], [38, 42, 46], [35, 39, 43]]
    assert pn.companion_rows(50, 48) is None and pn.companion_rows(50, 49) is None and pn.companion_rows(64, 63) == [51, 55, 59]


def test_every_network_lands_in_its_variant(fam):
    for name in ("A3", "A3w", "A1", "B", "round"):
        for p in fam[name]:
            assert networks.unclamped_ok(p.k, *p.net) and networks.filter_ok(p.k, *p.net), p.name
    for k in user_nets.SHAPES:
        free, clamped = pn.family_c(k)
        assert len(free) >= 12 and len(clamped) >= 12
        for p in free:
            assert networks.unclamped_ok(k, *p.net), p.name
        for p in clamped:
            assert not networks.unclamped_ok(k, *p.net) and user_nets.net_bound(k, *p.net) > 40.0, p.name
    # one live path: every other weight is zero
    for p in fam["A3"] + fam["A3w"] + fam["A1"] + pn.family_c(5)[0]:
        _, _, _, Ws, _, _ = networks.split_params(p.k, p.widths, p.params)
        assert [int(np.count_nonzero(W)) for W in Ws] == [1] * len(Ws), p.name


def test_family_a_margin_caps(fam, a_list):
    """Layer-3 probes: the twin's margin of every candidate is <= 26 u, twice the activation charge (13 .. 19.5 u is what the
    formula gives).  Layer-1 probes: <= 3 x 13 u plus the chain, conversion and input terms of the three one-term layers, which is
    the a-priori margin restated.  The round check's network: <= 26 u as well."""
    inputs = a_list[4]
    lo, hi = np.inf, 0.0
    for p in fam["A3"] + fam["A3w"] + fam["round"]:
        m = networks.filter_margin_at(3, p.widths, p.params, inputs)
        m0 = networks.filter_margin(3, *p.net)
        lo, hi = min(lo, m.min()), max(hi, m.max())
        print("%s: margin per candidate %.2f .. %.2f u, a priori %.2f u" % (p.name, m.min() / U, m.max() / U, m0 / U))
        assert np.all(m <= 26.0 * U) and np.all(m >= 13.0 * U), (p.name, m.max() / U)
    print("layer-3 probes: margin per candidate %.2f .. %.2f u over %d networks" % (lo / U, hi / U, len(fam["A3"]) + len(fam["A3w"])))
    z3 = pn.C * (pn.path_activations(fam["A3w"][30], a_list[5])[2][0]).astype(np.float64)
    assert np.unique(z3.astype(np.float32)).shape[0] >= 512      # the wide set really spreads the argument of exp2
    for p in fam["A1"]:
        m = networks.filter_margin_at(3, p.widths, p.params, inputs)
        m0 = networks.filter_margin(3, *p.net)
        extra = pn.premise_bound(p, charge=0.0, saturated_exact=False)
        cap = 3.0 * 13.0 * U * (1.0 + 2.0 ** -10) + extra
        print("%s: margin per candidate %.2f .. %.2f u, a priori %.2f u, cap %.2f u (3 x 13 u + %.2f u)"
              % (p.name, m.min() / U, m.max() / U, m0 / U, cap / U, extra / U))
        assert np.all(m <= cap * (1.0 + 1e-12)), (p.name, m.max() / U, cap / U)
        assert abs(m0 - cap) <= 1e-12 * cap, p.name


def test_the_restated_bound_is_the_twin_s(fam):
    """premise_layers with the twin's own premises (13 u, no exact saturation) is networks._filter_layers term for term: a rounding
    count or the charge changed in the derivation shows here"""
    for p in fam["A3"][::7] + fam["A3w"][::7] + fam["A1"][::3] + fam["B"]:
        e = networks._filter_layers(3, p.widths, p.params)
        mine = pn.premise_layers(p, saturated_exact=False)[-1][1]
        assert np.all(np.abs(mine - e) <= 1e-12 * e), (p.name, float(np.abs(mine - e).max() / U))
        assert abs(pn.premise_bound(p, saturated_exact=False) - networks.filter_margin(3, *p.net)) <= 1e-12 * networks.filter_margin(3, *p.net)
    widths, params = networks.load_network(3)
    p = pn.Net("shipped", 3, widths, params)
    e = networks._filter_layers(3, widths, params)
    assert np.all(np.abs(pn.premise_layers(p, saturated_exact=False)[-1][1] - e) <= 1e-12 * e)


def test_family_b_bounds_and_the_emulated_chain(fam):
    """the premise-level bound (saturated layer exact) is below the twin's own e of the output's neuron; a float32 emulation of the
    chain in the documented k-step order stays inside the chain's share of it; on the coherent pattern it reaches a tenth of it"""
    ratios = {}
    for p in fam["B"]:
        row, w, s, b2 = p.chain
        assert abs(b2) + np.abs(w).sum() < 40.0
        _, _, _, Ws, _, _ = networks.split_params(3, p.widths, p.params)
        r3 = int(np.flatnonzero(Ws[3][0])[0])
        e_twin = networks.filter_margin_terms(3, *p.net)[3][r3]
        e_mine = pn.premise_layers(p, saturated_exact=True)[-1][1][r3]
        assert 26.0 * U < e_mine <= e_twin, p.name
        n2 = float((w * s).sum() + b2)
        assert abs(n2) < 1e-3, (p.name, n2)      # z ~ 0: slope 1
        err, delta = pn.chain_error(p)
        where = "tail" if row >= 48 else "mfma"
        print("%s: emulated chain error %.1f u, chain bound %.1f u (%.3f), premise-level bound %.1f u, twin's e %.1f u"
              % (p.name, err, delta, err / delta, pn.premise_bound(p) / U, e_twin / U))
        assert err <= delta, p.name
        ratios.setdefault((p.pattern, where), []).append(err / delta)
    for key, r in sorted(ratios.items()):
        print("emulated / bound, %s on %s rows: %.3f .. %.3f" % (key + (min(r), max(r))))
    for where in ("mfma", "tail"):
        assert min(ratios[("coherent", where)]) >= 0.1, ratios[("coherent", where)]


def test_the_fp32_prediction_of_a_one_term_path(a_list):
    """z1 = fl32(fl32(c w1) v32) is a pure function on the host: the float32 product is the exact product rounded once, and it lies
    within the one-term chain bound of c w1 v"""
    v = a_list[6]
    for w1 in (pn.W1,) + pn.A1_LINKS:
        z1 = pn.predict_z1(w1, v)
        wt = np.float32(pn.C * w1)
        exact = np.float64(wt) * v                      # 24 x 24 bits: exact in float64
        assert z1.dtype == np.float32 and np.array_equal(z1, exact.astype(np.float32))
        assert np.array_equal(z1, pn.predict_z1(w1, v.copy()))
        assert np.any(z1.astype(np.float64) != exact)      # the rounding is real: the product needs more than 24 bits
        bound = abs(float(wt)) * np.abs(v) * pn.gamma(1) + abs(float(wt) - pn.C * w1) * np.abs(v)
        assert np.all(np.abs(z1.astype(np.float64) - pn.C * w1 * v) <= bound * (1.0 + 1e-9))


def test_the_reference_of_a_one_path_network_is_its_closed_form(fam, a_list):
    """networks.forward_twin in long double against T(w3 T(w2 T(w1 v + b1) + b2) + b3), bit for bit"""
    inputs, x = a_list[4], a_list[5]
    for p in fam["A3"][::9] + fam["A3w"][::9] + fam["A1"][::4] + fam["round"]:
        ref = networks.forward_twin(3, p.widths, p.params, inputs, dtype=np.longdouble)
        assert np.array_equal(ref, pn.closed_form(p, x)), p.name
    for k in user_nets.SHAPES:
        _, _, _, _, inputs, x = pn.c_points(k)
        free, clamped = pn.family_c(k)
        for p in free[::13] + clamped[::11]:
            with np.errstate(over="ignore"):
                ref = networks.forward_twin(k, p.widths, p.params, inputs[::8], dtype=np.longdouble)
            assert np.array_equal(ref, pn.closed_form(p, x[::8])), p.name
            assert np.all(np.isfinite(ref.astype(np.float64)))


def test_family_c_allowances(fam):
    """the allowance is a few 1e-15 where the probed activation is sensitive and never below the kernel's documented bound"""
    for k in (3, 5):
        _, _, _, _, _, x = pn.c_points(k)
        free, clamped = pn.family_c(k)
        for p in free + clamped:
            for kernel in ("mfma", "valu", "simple"):
                a = pn.c_allowance(p, x, kernel)
                act = pn.ACT_BOUND[pn.KERNEL_ACT[kernel]]
                assert np.all(a >= act) and np.all(a <= 2.2 * len(p.path[0]) * act + 1e-14), (p.name, kernel, a.max())
