"""Exact-SDP measure on the device at the inputs an LP actually produces (tests/sdp_inputs.py; the CPU side of the same assertions
is test_exact_sdp_edges_cpu.py): sdp_batch for k = 2..5 on every family against the numpy twin, the independent certificate check
and the k = 2 closed form; SDPCUT_STAT_SDP_UNCONVERGED against the lanes that say so themselves; a candidate's result as a function
of its own input alone, bit for bit, whatever shares its wave; score(SDP) and strategy 3 on the golden covers at the `late` and
`unitQ` points.

Measured by these tests on an MI355X (python -m pytest -m gpu tests/test_gpu_exact_sdp_edges.py -s prints them), seed 21:
  worst certificate violation of the device over k = 2..5, in units (SLACK_UNITS = 3.4): near_bounds 0.74, on_bounds 1.10,
  outside 1.05, sign_q 0.54, neg_q 0.77, all_minus 0.43, near_psd 0.80, one_weight 2.45, tiny_q 0, vertex 0.55, graded_sign 0.31,
  late 1.09, unitQ 0.59 (the twin's and the header's: the docstring of test_exact_sdp_edges_cpu.py)
  largest iteration count of a converged lane: 91 (k = 5: near_bounds, one_weight, graded_sign), the twin's count
  unconverged lanes: `vertex` k = 4: 2 of 256 (the twin 2), k = 5: 0 of 256 (the twin 1); no other family, no k = 2, 3; of the 1025
  tied k = 4 inputs test_stat_counts_the_last_valid_lane_of_a_partial_wave searches, the device ends 5 at the cap
  k = 2: worst excess of the device's value over the closed-form p*, or of p* over its upper bound: 1.9e-16
  score(SDP) on the four covers: worst |device - twin| 7.5e-13 at `late` (the device forms d = x - x x with one rounding, numpy
  with two: inside the two gaps), 8.9e-16 at `unitQ`; no candidate over the tolerance, SDPCUT_STAT_SDP_UNCONVERGED 0
  the whole file: 4.4 s, 2.5 s of it the twin's solves"""
import numpy as np
import pytest

import sdp_inputs
from sdpcutsel_via_nn_amd import _capi, exact_sdp
from test_exact_sdp_cpu import cover_inputs
from test_exact_sdp_edges_cpu import CLOSED_FORM_BOUND, VERTEX_SHARE, _may_stall

pytestmark = pytest.mark.gpu
KS = sdp_inputs.KS


@pytest.fixture(scope="module")
def runs():
    """{k: {family: (inputs, twin result, device result, SDPCUT_STAT_SDP_UNCONVERGED after that batch)}}, solved once"""
    import sdpcutsel_via_nn_amd as pkg
    z = sdp_inputs.golden_boxqp()
    sc = pkg.Scorer(0)
    out = {}
    for k in KS:
        out[k] = {}
        for name, inp in sdp_inputs.families(k, z=z).items():
            r = sc.sdp_batch(k, inp, want_certificate=True)
            out[k][name] = (inp, exact_sdp.solve(k, inp), r, sc.get_stat(_capi.STAT_SDP_UNCONVERGED))
    sc.close()
    return out


@pytest.mark.parametrize("k", KS)
def test_sdp_batch_certificates_and_twin(runs, k):
    for name, (inp, t, r, stat) in runs[k].items():
        C, d = sdp_inputs.problem(k, inp)
        slack, worst_t = sdp_inputs.family_slack(k, inp, t)
        c = exact_sdp.certificate_check(C, d, r["lam"], r["Y"], slack_units=slack)
        bad, bad_t = sdp_inputs.stalled(r), ~t["converged"]
        conv = ~bad
        print("k = %d %-12s certificate worst %.3f units (twin %.3f, slack %.2f); iterations of a converged lane max %d (twin %d); unconverged %d (twin %d)"
              % (k, name, c["worst_units"], worst_t, slack, r["iters"][conv].max(initial=0), t["iters"][~bad_t].max(initial=0), bad.sum(), bad_t.sum()))
        assert c["ok"].all(), name
        xqx = exact_sdp.unpack(k, inp)[2]
        # the value the certificate implies.  (The device contracts d = x - x x into one fma, rounded once; numpy rounds x x first:
        # the two d differ by up to eps / 2, and lam = l / d carries the device's.)
        implied = xqx - (d * r["lam"]).sum(axis=1)
        assert np.all(np.abs(implied - r["value"]) <= 1e-14 + 0.5 * np.finfo(np.float64).eps * r["lam"].sum(axis=1)), name
        sdp_inputs.assert_refuted(k, inp, r, slack, name)
        # convergence, honestly reported
        assert stat == bad.sum(), name
        assert np.all(r["iters"] <= exact_sdp.ITER_CAP) and np.all(r["iters"] >= 0)
        assert np.all(r["gap"][conv] <= exact_sdp.GAP_TOL * np.maximum(1.0, np.abs(r["value"][conv])))
        if _may_stall(k, name):
            assert bad.sum() <= VERTEX_SHARE * inp.shape[0]
        else:
            assert not bad.any(), name
        sdp_inputs.assert_unconverged_honest(r, bad)
        sdp_inputs.assert_agree(r, bad, t, bad_t)


def test_k2_values_bracket_the_closed_form(runs):
    worst = 0.0
    for name, (inp, t, r, _) in runs[2].items():
        p = sdp_inputs.closed_form_k2(inp)
        lo = float((r["value"].astype(sdp_inputs.LD) - p).max())
        up = float((p - (r["value"].astype(sdp_inputs.LD) + r["gap"].astype(sdp_inputs.LD))).max())
        worst = max(worst, lo, up)
        assert lo <= CLOSED_FORM_BOUND and up <= CLOSED_FORM_BOUND, (name, lo, up)
    print("k = 2: worst excess of the device's value over p* or of p* over its upper bound: %.2e" % worst)


def test_a_bound_above_the_closed_form_is_refuted(runs):
    """the device's own zero-iteration answers at a tiny d_i (finding 1): accepted, and a lam 1e-12 above p* is not"""
    seen = 0
    for name in ("near_bounds", "graded_sign", "late"):
        inp, _, r, _ = runs[2][name]
        w = np.flatnonzero(sdp_inputs.tiny_d_zero_answers(2, inp, r))
        seen += w.size
        if w.size == 0:
            continue
        inp, Y = inp[w], r["Y"][w]
        C, d = sdp_inputs.problem(2, inp)
        assert exact_sdp.certificate_check(C, d, r["lam"][w], Y)["ok"].all()
        p = sdp_inputs.closed_form_k2(inp)
        xqx = exact_sdp.unpack(2, inp)[2]
        need = (xqx.astype(sdp_inputs.LD) - p - sdp_inputs.LD(1e-12)).astype(np.float64)
        for i in (np.argmin(np.where(d > 0, d, np.inf), axis=1), np.argmax(d, axis=1)):
            wrong = np.zeros((w.size, 2))
            wrong[np.arange(w.size), i] = need / d[np.arange(w.size), i]
            assert not exact_sdp.certificate_check(C, d, wrong, Y)["ok"].any()
    assert seen >= 1


def _device_stall():
    """(k, input) of a lane the DEVICE ends at the cap: the tied reproducers and the vertex families of a few seeds"""
    import sdpcutsel_via_nn_amd as pkg
    pool = {4: [sdp_inputs.reproducers()["tied_k4"][1]], 5: [sdp_inputs.reproducers()[n][1] for n in ("tied_k5_a", "tied_k5_b")]}
    for seed in range(sdp_inputs.SEED, sdp_inputs.SEED + 4):
        for k in (4, 5):
            pool[k].append(sdp_inputs.drawn_families(k, seed)["vertex"])
    sc = pkg.Scorer(0)
    try:
        for k in (4, 5):
            inp = np.vstack(pool[k])
            bad = np.flatnonzero(sdp_inputs.stalled(sc.sdp_batch(k, inp, want_certificate=True)))
            print("k = %d: the device ends %d of %d tied inputs at the cap" % (k, bad.size, inp.shape[0]))
            if bad.size:
                return k, inp[bad[0]]
    finally:
        sc.close()
    return None


def test_stat_counts_the_last_valid_lane_of_a_partial_wave():
    import sdpcutsel_via_nn_amd as pkg
    found = _device_stall()
    assert found is not None, "no tied input stalls on the device: the premise of this test is gone"
    k, row = found
    easy = sdp_inputs.drawn_families(k)["sign_q"]
    sc = pkg.Scorer(0)
    for count in (1, 64, 69, 128, 129):      # the stalled lane last: alone, closing a full wave, and the last valid lane of a partial one
        inp = np.vstack([easy[:count - 1], row[None]])
        r = sc.sdp_batch(k, inp, want_certificate=True)
        bad = sdp_inputs.stalled(r)
        assert bad[-1] and bad.sum() == 1 and sc.get_stat(_capi.STAT_SDP_UNCONVERGED) == 1, count
        v, g = sc.sdp_batch(k, inp)
        assert sc.get_stat(_capi.STAT_SDP_UNCONVERGED) == 1 and np.array_equal(v, r["value"]) and np.array_equal(g, r["gap"])
    r = sc.sdp_batch(k, easy[:69], want_certificate=True)      # and the count is of the last solve only
    assert sc.get_stat(_capi.STAT_SDP_UNCONVERGED) == 0 and not sdp_inputs.stalled(r).any()
    sc.close()


def _bits(r):
    return [np.ascontiguousarray(r[key]).view(np.int64 if r[key].dtype == np.float64 else np.int32) for key in ("value", "gap", "lam", "Y", "iters")]


@pytest.mark.parametrize("k", KS)
def test_result_is_a_function_of_the_input_alone(runs, k):
    """A wave loops until its slowest lane is done and lanes past `count` re-read the last input: neither the company a candidate
    keeps nor its place in the batch may change one bit of its result."""
    import sdpcutsel_via_nn_amd as pkg
    inp = np.vstack([runs[k]["near_bounds"][0], runs[k]["vertex"][0]])
    n = inp.shape[0]
    ref = {key: np.concatenate([runs[k]["near_bounds"][2][key], runs[k]["vertex"][2][key]]) for key in ("value", "gap", "lam", "Y", "iters")}
    sc = pkg.Scorer(0)
    whole = sc.sdp_batch(k, inp, want_certificate=True)
    for a, b in zip(_bits(whole), _bits(ref)):      # against the two families solved on their own
        assert np.array_equal(a, b)
    perm = np.random.default_rng(k).permutation(n)
    shuffled = sc.sdp_batch(k, inp[perm], want_certificate=True)
    for a, b in zip(_bits(shuffled), _bits(ref)):
        assert np.array_equal(a, b[perm])
    v, g = sc.sdp_batch(k, inp[perm])
    assert np.array_equal(v.view(np.int64), ref["value"][perm].view(np.int64)) and np.array_equal(g.view(np.int64), ref["gap"][perm].view(np.int64))
    for size in (1, 63, 64, 65, 129):
        for lo in range(0, n, size):
            w = np.arange(lo, min(lo + size, n))
            part = sc.sdp_batch(k, inp[w], want_certificate=True)
            for a, b in zip(_bits(part), _bits(ref)):
                assert np.array_equal(a, b[w]), (size, lo)
            v, g = sc.sdp_batch(k, inp[w])
            assert np.array_equal(v.view(np.int64), ref["value"][w].view(np.int64)) and np.array_equal(g.view(np.int64), ref["gap"][w].view(np.int64))
    sc.close()


@pytest.mark.parametrize("which", sdp_inputs.COVER)
@pytest.mark.parametrize("tag", sdp_inputs.COVER_TAGS)
def test_score_sdp_on_the_covers(golden_boxqp, tag, which):
    import sdpcutsel_via_nn_amd as pkg
    z = golden_boxqp
    Q, vv = sdp_inputs.cover_case(z, tag, which)
    N = z[tag + "_k"].shape[0]
    sc = pkg.Scorer(0)
    sc.set_option(_capi.OPT_EXACT_SDP, 1)
    sc.set_instance(int(z[tag + "_nb_vars"]), Q)
    sc.set_candidates(z[tag + "_set_inds"], z[tag + "_k"])
    sc.set_point(vv)
    sc.score(_capi.SDP)
    sdp, gap = sc.get_sdp_scores()
    stat = sc.get_stat(_capi.STAT_SDP_UNCONVERGED)
    ids, score, total, new_strat, _ = sc.rank(3, 0)
    ids_h, score_h, _, _, _ = sc.rank(3, 0, max_out=100)
    sc.close()
    meas, tgap, pstar, me = np.zeros(N), np.zeros(N), np.zeros(N), np.ones(N)
    for k, (m, inp, negSM, me_k) in cover_inputs(sdp_inputs.cover_view(z, tag, which), tag, which).items():
        t = exact_sdp.solve(k, inp)
        meas[m], tgap[m], me[m] = negSM + t["value"] * me_k, t["gap"] * me_k, me_k
        pstar[m] = (sdp[m] - negSM) / me_k      # the device's own p* in normalised units, for its tolerance
    over = gap > exact_sdp.GAP_TOL * np.maximum(1.0, np.abs(pstar))
    print("%s %s: %d candidates, worst |device - twin| %.3e, device gap max %.3e, over the tolerance %d (stat %d)"
          % (tag, which, N, np.abs(sdp - meas).max(), gap.max(), over.sum(), stat))
    assert np.all(np.abs(sdp - meas) <= gap * me + tgap + 1e-12 * np.maximum(1.0, np.abs(meas)))
    assert stat == over.sum()
    order = np.argsort(-sdp, kind="stable")
    assert total == N and new_strat == 3 and np.array_equal(ids, order) and np.array_equal(score, sdp[order])
    assert np.array_equal(ids_h, order[:100]) and np.array_equal(score_h, sdp[order[:100]])
