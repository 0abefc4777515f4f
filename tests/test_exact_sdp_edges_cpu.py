"""Exact-SDP measure at the inputs an LP actually produces (tests/sdp_inputs.py): x on, next to and outside its bounds, tied and
one-signed weights, nearly positive semidefinite weight matrices -- the numpy twin (exact_sdp.solve) and the solver body of the
kernels compiled for the host (csrc/exact_sdp.h through test_exact_sdp_cpu.host_solver), without a device.  Every returned (lam, Y)
passes the independent certificate check, the k = 2 values bracket a closed-form optimum computed in long double, and a lane that
does not converge says so.

Measured by these tests (python -m pytest tests/test_exact_sdp_edges_cpu.py -s prints them), seed 21, k = 2..5 together; the device
column is what test_gpu_exact_sdp_edges.py printed on an MI355X:
  worst certificate violation in units (SLACK_UNITS = 3.4; the slack of a family is max(SLACK_UNITS, 4 x the twin's worst on it)):
                  twin   header  device
    near_bounds   0.65   1.29    0.74
    on_bounds     1.01   0.92    1.10
    outside       0.94   0.98    1.05
    sign_q        0.40   0.41    0.54
    neg_q         0.97   1.11    0.77
    all_minus     0.29   0.44    0.43
    near_psd      0.98   0.80    0.80
    one_weight    1.55   1.65    2.45
    tiny_q        0      0       0       (weights below 1e-9: judged against the check's absolute floor, eps)
    vertex        0.57   0.72    0.55
    graded_sign   0.27   0.31    0.31
    late          0.75   0.89    1.09
    unitQ         0.41   0.43    0.59
  before certificate_check judged dual feasibility in the solver's scaled units the twin's and the header's worst were 2.6e15
  (near_bounds), 3.2e15 (graded_sign), 3.1e15 (late) and 12.8 (near_psd) units: 1-2 of 256, 9 of 1893 and 1-2 of 256 rejected
  largest iteration count of a converged input: 91 (k = 5, near_bounds), twin, header and device alike (ITER_CAP = 138)
  unconverged, all of them in `vertex`: k = 4 twin 2, header 3, device 2 of 256 (largest gap at the cap 1.9e-3); k = 5 twin 1,
  header 1, device 0 of 256 (6.9e-4); none for k = 2, 3; none in any other family
  k = 2: worst excess of `value` over the closed-form p*, or of p* over `upper`, 13 families + 4096 golden inputs: 1.9e-16"""
import numpy as np
import pytest

import sdp_inputs
from conftest import golden_nn
from sdpcutsel_via_nn_amd import exact_sdp
from test_exact_sdp_cpu import host_solver      # noqa: F401  (the fixture, by import)

KS = sdp_inputs.KS
VERTEX_SHARE = 0.02      # of a `vertex` family may end unconverged (the twin alone shows 0.6 %, the header 0.2 %; which tied input
#                          stalls depends on last-bit rounding)
CLOSED_FORM_BOUND = 1e-15


@pytest.fixture(scope="module")
def runs(host_solver):      # noqa: F811
    """{k: {family: (inputs, twin result, header result)}}, solved once"""
    z = sdp_inputs.golden_boxqp()
    out = {}
    for k in KS:
        out[k] = {}
        for name, inp in sdp_inputs.families(k, z=z).items():
            h = host_solver(k, inp)
            h["converged"] = h["converged"].astype(bool)
            out[k][name] = (inp, exact_sdp.solve(k, inp), h)
    return out


def _may_stall(k, name):
    return name == "vertex" and k >= 4


def test_premises(runs):
    """the families hold what they were built for, so that a re-seed cannot empty one"""
    for name in ("near_bounds", "graded_sign", "late"):      # finding 1; over the sizes together (k = 5 shows it once in thousands)
        for who in (1, 2):
            n = {k: int(sdp_inputs.tiny_d_zero_answers(k, runs[k][name][0], runs[k][name][who]).sum()) for k in KS}
            print("%-12s %s: zero-iteration answers with a tiny d_i and lambda_min(C) < -1e-3, per k: %s" % (name, ("twin", "header")[who - 1], n))
            assert sum(n.values()) >= 1
    for k in KS:                                              # finding 2
        inp, t, _ = runs[k]["near_psd"]
        C, _ = sdp_inputs.problem(k, inp)
        assert (sdp_inputs.zero_answers(t) & (np.linalg.eigvalsh(C)[:, 0] < 0)).any()
    for k in (4, 5):                                          # finding 3
        t = runs[k]["vertex"][1]
        assert (~t["converged"]).any() and np.all(t["iters"][~t["converged"]] == exact_sdp.ITER_CAP)


def test_closed_form_agrees_with_a_grid():
    """the k = 2 reference against brute force: no point of a 401 x 401 grid of the box lies below it, and one comes close"""
    inp = np.vstack([sdp_inputs.drawn_families(2)[n][:8] for n in ("near_bounds", "sign_q", "neg_q", "near_psd", "vertex")])
    p = sdp_inputs.closed_form_k2(inp).astype(np.float64)
    x, C, xqx = exact_sdp.unpack(2, inp)
    r = np.sqrt(np.maximum(x - x * x, 0.0))
    g = np.linspace(0.0, 1.0, 401)
    u, v = r[:, 0, None, None] * g[None, :, None], r[:, 1, None, None] * g[None, None, :]
    f = C[:, 0, 0, None, None] * u * u + C[:, 1, 1, None, None] * v * v - 2 * np.abs(C[:, 0, 1, None, None]) * u * v
    best = xqx + f.reshape(inp.shape[0], -1).min(axis=1)
    assert np.all(p <= best + 1e-15) and np.all(best - p <= 1e-5)


def test_k2_values_bracket_the_closed_form(runs, host_solver):      # noqa: F811
    cases = {name: (inp, t, h) for name, (inp, t, h) in runs[2].items()}
    g = golden_nn(2)["inputs"]
    assert g.shape[0] == 4096
    cases["golden"] = (g, exact_sdp.solve(2, g), host_solver(2, g))
    worst = 0.0
    for name, (inp, t, h) in cases.items():
        p = sdp_inputs.closed_form_k2(inp)
        for r in (t, h):
            lo = float((r["value"].astype(sdp_inputs.LD) - p).max())
            up = float((p - (r["value"].astype(sdp_inputs.LD) + r["gap"].astype(sdp_inputs.LD))).max())
            worst = max(worst, lo, up)
            assert lo <= CLOSED_FORM_BOUND and up <= CLOSED_FORM_BOUND, (name, lo, up)
    print("k = 2: worst excess of value over p* or of p* over upper, twin and header, 13 families + 4096 golden inputs: %.2e" % worst)


@pytest.mark.parametrize("k", KS)
def test_certificates(runs, k):
    for name, (inp, t, h) in runs[k].items():
        C, d = sdp_inputs.problem(k, inp)
        slack, worst_t = sdp_inputs.family_slack(k, inp, t)
        ch = exact_sdp.certificate_check(C, d, h["lam"], h["Y"], slack_units=slack)
        print("k = %d %-12s worst violation in units: twin %.3f, header %.3f (slack %.2f)" % (k, name, worst_t, ch["worst_units"], slack))
        assert exact_sdp.certificate_check(C, d, t["lam"], t["Y"])["ok"].all(), name      # the twin inside SLACK_UNITS itself
        assert ch["ok"].all(), name
        for r in (t, h):      # the certificate IS the proof: the value it implies is the value returned
            xqx = exact_sdp.unpack(k, inp)[2]
            assert np.abs(xqx - (d * r["lam"]).sum(axis=1) - r["value"]).max() <= 1e-14


@pytest.mark.parametrize("k", KS)
def test_certificate_check_still_refutes(runs, k):
    """the check has not gone lax on these inputs: 0.9 lam and 1.1 Y are rejected wherever the solver moved and the returned
    bracket proves them wrong (sdp_inputs.assert_refuted: everywhere on eight families, somewhere on every other)"""
    for name, (inp, t, h) in runs[k].items():
        slack, _ = sdp_inputs.family_slack(k, inp, t)
        for who, r in (("twin", t), ("header", h)):
            moved, by_lam, by_Y = sdp_inputs.assert_refuted(k, inp, r, slack, name)
            print("k = %d %-12s %-6s moved %4d: 0.9 lam refuted on %4d, 1.1 Y on %4d" % (k, name, who, moved, by_lam, by_Y))
            assert moved < 16 or (by_lam >= 1 and by_Y >= 1), name


def test_a_bound_above_the_closed_form_is_refuted(runs):
    """the zero-iteration answers of finding 1 (k = 2): the check accepts lam = 0 -- value = p* to 1e-15 by the closed form -- and
    rejects any lam that would put the lower bound 1e-12 above p*, on whichever index it is placed"""
    seen = 0
    cases = [runs[2][n][:2] for n in ("near_bounds", "graded_sign", "late")] + [(sdp_inputs.reproducers()["tiny_d"][1], None)]
    for inp, t in cases:
        t = exact_sdp.solve(2, inp) if t is None else t
        w = np.flatnonzero(sdp_inputs.tiny_d_zero_answers(2, inp, t))
        if w.size == 0:
            continue
        seen += w.size
        inp, lam, Y = inp[w], t["lam"][w], t["Y"][w]
        C, d = sdp_inputs.problem(2, inp)
        assert exact_sdp.certificate_check(C, d, lam, Y)["ok"].all()
        p = sdp_inputs.closed_form_k2(inp)
        xqx = exact_sdp.unpack(2, inp)[2]
        need = (xqx.astype(sdp_inputs.LD) - p - sdp_inputs.LD(1e-12)).astype(np.float64)      # d^T lam of such a bound
        for i in (np.argmin(np.where(d > 0, d, np.inf), axis=1), np.argmax(d, axis=1)):
            wrong = np.zeros_like(lam)
            wrong[np.arange(w.size), i] = need / d[np.arange(w.size), i]
            lower = xqx - (d * wrong).sum(axis=1)
            assert np.all(lower.astype(sdp_inputs.LD) - p >= 0.9e-12)
            assert not exact_sdp.certificate_check(C, d, wrong, Y)["ok"].any()
    assert seen >= 2


@pytest.mark.parametrize("k", KS)
def test_convergence_is_reported_honestly(runs, k):
    for name, (inp, t, h) in runs[k].items():
        bad_t, bad_h = ~t["converged"], ~h["converged"]
        assert np.array_equal(bad_t, sdp_inputs.stalled(t)) and np.array_equal(bad_h, sdp_inputs.stalled(h)), name
        if _may_stall(k, name):
            print("k = %d vertex: unconverged twin %d, header %d of %d; largest gap at the cap %.2e"
                  % (k, bad_t.sum(), bad_h.sum(), inp.shape[0], max(t["gap"][bad_t].max(initial=0.0), h["gap"][bad_h].max(initial=0.0))))
            assert bad_t.sum() <= VERTEX_SHARE * inp.shape[0] and bad_h.sum() <= VERTEX_SHARE * inp.shape[0]
        else:
            assert not bad_t.any() and not bad_h.any(), name
        sdp_inputs.assert_unconverged_honest(t, bad_t)
        sdp_inputs.assert_unconverged_honest(h, bad_h)
        assert np.all(t["value"] <= t["upper"])
        sdp_inputs.assert_agree(t, bad_t, h, bad_h)


def test_iteration_counts_stay_under_the_cap(runs):
    most = {}
    for k in KS:
        for name, (inp, t, h) in runs[k].items():
            for who, r in (("twin", t), ("header", h)):
                conv = r["converged"]
                assert np.all(r["iters"] <= exact_sdp.ITER_CAP) and np.all(r["iters"][conv & (r["gap"] > 0)] <= exact_sdp.ITER_CAP)
                m = int(r["iters"][conv].max(initial=0))
                if m > most.get(who, (0,))[0]:
                    most[who] = (m, k, name)
    print("largest iteration count of a converged input: %s (ITER_CAP %d)" % (most, exact_sdp.ITER_CAP))


def test_reproducers(host_solver):      # noqa: F811
    rep = sdp_inputs.reproducers()
    # finding 1
    k, inp = rep["tiny_d"]
    for r in (exact_sdp.solve(k, inp), host_solver(k, inp)):
        C, d = sdp_inputs.problem(k, inp)
        c = exact_sdp.certificate_check(C, d, r["lam"], r["Y"])
        assert r["iters"][0] == 0 and np.all(r["lam"] == 0.0) and c["ok"].all() and c["dual_min_unscaled"][0] < -0.3
        assert abs(float(r["value"][0] - sdp_inputs.closed_form_k2(inp)[0])) <= CLOSED_FORM_BOUND
    # finding 3: the lower bound is the optimum 15/64; the twin's upper bound stalls, and says so
    k, inp = rep["tied_k4"]
    t, h = exact_sdp.solve(k, inp), host_solver(k, inp)
    assert not t["converged"][0] and t["iters"][0] == exact_sdp.ITER_CAP and t["gap"][0] > 1e-6
    assert 0 <= 15 / 64 - t["value"][0] <= exact_sdp.GAP_TOL and 15 / 64 <= t["upper"][0]
    assert h["value"][0] <= 15 / 64 + 1e-15 <= h["value"][0] + h["gap"][0] + 2e-15
    for name in ("tied_k5_a", "tied_k5_b"):
        k, inp = rep[name]
        t, h = exact_sdp.solve(k, inp), host_solver(k, inp)
        h["converged"] = h["converged"].astype(bool)
        assert not t["converged"][0] and t["iters"][0] == exact_sdp.ITER_CAP
        C, d = sdp_inputs.problem(k, inp)
        assert exact_sdp.certificate_check(C, d, t["lam"], t["Y"])["ok"].all() and exact_sdp.certificate_check(C, d, h["lam"], h["Y"])["ok"].all()
        sdp_inputs.assert_agree(t, ~t["converged"], h, ~h["converged"])
