"""Inputs for the exact-SDP edge tests (test_exact_sdp_edges_cpu.py, test_gpu_exact_sdp_edges.py): the [x | Q_slice] an LP actually
hands the solver -- x on, next to and just outside its bounds, tied and one-signed weights, nearly positive semidefinite weight
matrices, weights down to 1e-300 -- as deterministic families, the golden covers at two hostile points, the explicit reproducers
the families were built around, and the closed-form optimum for k = 2 in long double.  A plain module: no fixtures, no GPU.

Every family draws q = uniform(-1, 1) / k and interior x = uniform(0.05, 0.95) unless its line says otherwise; 10^j has j a uniform
INTEGER of the stated range.
  near_bounds   each x_i independently becomes eps, 1 - eps or stays interior, eps = 10^j, j in -16 .. -3
  on_bounds     the same pattern with eps = 0
  outside       -eps and 1 + eps
  sign_q        q_ij = +-1/k at random
  neg_q         q = -|q|
  all_minus     every q_ij = -1/k
  near_psd      C = P - (lambda_min(P) + 10^j) I, j in -16 .. -4, P a random Gram matrix scaled to max|.| = 1/k; q_ii = C_ii, q_ij = 2 C_ij
  one_weight    a single +-1/k entry, the rest 0
  tiny_q        q scaled by 10^j, j in -300 .. -9
  vertex        x = 0.5, q_ij in {0, +-1/k} at random
  graded_sign   the x of near_bounds with the q of sign_q
  late          every size-k candidate of the golden covers at their `rnd` point with 60 % of the x coordinates moved to the nearer
                bound plus noise from {0, +-1e-9, 1e-12, 1e-16} (the x an LP returns late in a run)
  unitQ         the same candidates at the `mck` point with Q_arr replaced by its sign (unit-weight instances)
The drawn families hold N = 256 inputs; the two cover families hold what the four covers have of that size (k = 2: 9, k = 3: 1893, k = 4: 4152, k = 5: 1)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble

N = 256
KS = (2, 3, 4, 5)
SEED = 21
COVER_TAGS = ("spar020_100_1_d3", "spar020_100_1_d4", "spar040_030_1_d5", "spar030_060_1_d3")
DRAWN = ("near_bounds", "on_bounds", "outside", "sign_q", "neg_q", "all_minus", "near_psd", "one_weight", "tiny_q", "vertex", "graded_sign")
COVER = ("late", "unitQ")
LATE_NOISE = (0.0, 1e-9, -1e-9, 1e-12, 1e-16)
LATE_SHARE = 0.6


def _m(k):
    return k * (k + 1) // 2


def _q(rng, k, n=N):
    return rng.uniform(-1.0, 1.0, size=(n, _m(k))) / k


def _x(rng, k, n=N):
    return rng.uniform(0.05, 0.95, size=(n, k))


def _pow10(rng, lo, hi, shape):
    return 10.0 ** rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def _bound_pattern(rng, k, eps_of):
    """x with each coordinate at eps, at 1 - eps or interior, a third each; eps_of(shape) -> eps per coordinate (signed)"""
    x = _x(rng, k)
    where = rng.integers(0, 3, size=x.shape)
    eps = eps_of(x.shape)
    return np.where(where == 0, eps, np.where(where == 1, 1.0 - eps, x))


def _sign_q(rng, k):
    return rng.choice([-1.0, 1.0], size=(N, _m(k))) / k


def _near_psd(rng, k):
    ia, ib = np.triu_indices(k)
    q = np.empty((N, _m(k)))
    for i in range(N):
        G = rng.normal(size=(k, k))
        P = G @ G.T
        P = P / (k * np.abs(P).max())
        C = P - (np.linalg.eigvalsh(P)[0] + 10.0 ** int(rng.integers(-16, -3))) * np.eye(k)
        q[i] = np.where(ia == ib, C[ia, ib], 2.0 * C[ia, ib])
    return q


def drawn_families(k, seed=SEED):
    """{name: inputs [N, k(k+3)/2]} of the drawn families, one generator per family so that a family does not move when another does"""
    out = {}
    for f, name in enumerate(DRAWN):
        rng = np.random.default_rng([seed, k, f])
        if name == "near_bounds":
            x, q = _bound_pattern(rng, k, lambda s: _pow10(rng, -16, -3, s)), _q(rng, k)
        elif name == "on_bounds":
            x, q = _bound_pattern(rng, k, lambda s: np.zeros(s)), _q(rng, k)
        elif name == "outside":
            x, q = _bound_pattern(rng, k, lambda s: -_pow10(rng, -16, -3, s)), _q(rng, k)
        elif name == "sign_q":
            x, q = _x(rng, k), _sign_q(rng, k)
        elif name == "neg_q":
            x, q = _x(rng, k), -np.abs(_q(rng, k))
        elif name == "all_minus":
            x, q = _x(rng, k), np.full((N, _m(k)), -1.0 / k)
        elif name == "near_psd":
            x, q = _x(rng, k), _near_psd(rng, k)
        elif name == "one_weight":
            x, q = _x(rng, k), np.zeros((N, _m(k)))
            q[np.arange(N), rng.integers(0, _m(k), size=N)] = rng.choice([-1.0, 1.0], size=N) / k
        elif name == "tiny_q":
            x, q = _x(rng, k), _q(rng, k) * _pow10(rng, -300, -9, (N, 1))
        elif name == "vertex":
            x, q = np.full((N, k), 0.5), rng.integers(-1, 2, size=(N, _m(k))).astype(np.float64) / k
        elif name == "graded_sign":
            x, q = _bound_pattern(rng, k, lambda s: _pow10(rng, -16, -3, s)), _sign_q(rng, k)
        out[name] = np.ascontiguousarray(np.hstack([x, q]))
    return out


# ---- the golden covers at two hostile points -------------------------------------------------------------------------------------
def golden_boxqp():
    return np.load(os.path.join(GOLDEN, "inst_boxqp.npz"))


def cover_case(z, tag, which, seed=SEED):
    """-> (Q_arr, vars_values) of golden cover `tag` at the `late` or `unitQ` point"""
    n = int(z[tag + "_nb_vars"])
    L = n * (n + 1) // 2
    Q = np.array(z[tag + "_Q_arr"], dtype=np.float64)
    if which == "unitQ":
        return np.sign(Q), np.array(z[tag + "_mck_vars"], dtype=np.float64)
    assert which == "late"
    rng = np.random.default_rng([seed, COVER_TAGS.index(tag), 99])
    vv = np.array(z[tag + "_rnd_vars"], dtype=np.float64)
    x = vv[L:]
    move = rng.random(n) < LATE_SHARE
    noise = rng.choice(LATE_NOISE, size=n)
    vv[L:] = np.where(move, np.where(x < 0.5, noise, 1.0 - noise), x)
    return Q, vv


def cover_view(z, tag, which, seed=SEED):
    """what test_exact_sdp_cpu.cover_inputs reads of a cover, at that point: cover_inputs(view, tag, which)"""
    Q, vv = cover_case(z, tag, which, seed)
    return {tag + "_nb_vars": z[tag + "_nb_vars"], tag + "_Q_arr": Q, tag + "_set_inds": z[tag + "_set_inds"], tag + "_k": z[tag + "_k"],
            tag + "_%s_vars" % which: vv}


def cover_families(k, seed=SEED, z=None):
    """{late, unitQ: inputs [*, k(k+3)/2]}: the size-k candidates of the four golden covers, cover after cover"""
    from test_exact_sdp_cpu import cover_inputs
    z = golden_boxqp() if z is None else z
    out = {}
    for which in COVER:
        parts = []
        for tag in COVER_TAGS:
            co = cover_inputs(cover_view(z, tag, which, seed), tag, which)
            if k in co:
                parts.append(co[k][1])
        out[which] = np.ascontiguousarray(np.vstack(parts))
    return out


def families(k, seed=SEED, z=None):
    out = drawn_families(k, seed)
    out.update(cover_families(k, seed, z))
    return out


# ---- the explicit reproducers ----------------------------------------------------------------------------------------------------
TINY_D = (2, [0.35, 1e-16], [0.5, -0.18, -0.32])      # zero iterations, lam = 0, C + Diag(lam) has lambda_min -0.33 on the active indices
TIED_K4 = (4, [0.5] * 4, [0.25, -0.25, 0, 0.25, 0, 0.25, 0.25, 0.25, 0, 0.25])      # p* = 15/64; the twin's upper bound stalls
# two analogues for k = 5 found by scanning the `vertex` generator (the twin ends at the cap on both), in units of 1/5
TIED_K5_A = (5, [0.5] * 5, [v / 5 for v in (-1, 1, 1, 0, 0, -1, 1, 0, 0, 1, 0, -1, 0, 1, 1)])
TIED_K5_B = (5, [0.5] * 5, [v / 5 for v in (-1, 0, 1, -1, 0, -1, 0, 0, -1, 1, 0, 0, 1, 1, 1)])


def reproducers():
    """{name: (k, inputs [1, k(k+3)/2])}"""
    return {name: (k, np.array([list(x) + list(q)], dtype=np.float64))
            for name, (k, x, q) in dict(tiny_d=TINY_D, tied_k4=TIED_K4, tied_k5_a=TIED_K5_A, tied_k5_b=TIED_K5_B).items()}


# ---- an independent optimum for k = 2 ----------------------------------------------------------------------------------------------
def closed_form_k2(inputs):
    """p* of [x0 x1 | q00 q01 q11] in long double.  With u = sqrt(Y00), v = sqrt(Y11) and Y01 = -sign(q01) u v (the best a positive
    semidefinite Y allows) the inner problem is min c00 u^2 + c11 v^2 - |q01| u v over the box [0, r0] x [0, r1], r = sqrt(d): a
    quadratic form is minimised over a box at the origin, at a corner or on one of the two far edges, where it is a parabola in one
    variable -- the three non-origin corners, the two clipped stationary points of the edges u = r0 and v = r1, and 0."""
    a = np.asarray(inputs, dtype=np.float64).astype(LD)
    x0, x1, q00, q01, q11 = (a[:, i] for i in range(5))
    zero = LD(0)
    r0, r1 = np.sqrt(np.maximum(x0 - x0 * x0, zero)), np.sqrt(np.maximum(x1 - x1 * x1, zero))
    b = np.abs(q01)
    f = lambda u, v: q00 * u * u + q11 * v * v - b * u * v      # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        vs = np.where(q11 > 0, np.clip(b * r0 / (2 * q11), zero, r1), r1)      # edge u = r0
        us = np.where(q00 > 0, np.clip(b * r1 / (2 * q00), zero, r0), r0)      # edge v = r1
    inner = np.minimum.reduce([np.zeros_like(x0), f(r0, zero * r1), f(zero * r0, r1), f(r0, r1), f(r0, vs), f(us, r1)])
    return q00 * x0 * x0 + q01 * x0 * x1 + q11 * x1 * x1 + inner


# ---- what both test files assert of a solver's results ---------------------------------------------------------------------------
def problem(k, inputs):
    """-> (C [n, k, k], d [n, k]) as certificate_check takes them"""
    from sdpcutsel_via_nn_amd import exact_sdp
    x, C, _ = exact_sdp.unpack(k, inputs)
    return C, np.maximum(x - x * x, 0.0)


def family_slack(k, inputs, twin):
    """slack of a family in units: max(SLACK_UNITS, 4 x the twin's own worst violation on it), the rule SLACK_UNITS was set by
    -> (slack, the twin's worst)"""
    from sdpcutsel_via_nn_amd import exact_sdp
    C, d = problem(k, inputs)
    worst = exact_sdp.certificate_check(C, d, twin["lam"], twin["Y"])["worst_units"]
    return max(exact_sdp.SLACK_UNITS, 4.0 * worst), worst


def stalled(r):
    """lanes that ended at the cap with the gap above the tolerance (what SDPCUT_STAT_SDP_UNCONVERGED counts)"""
    from sdpcutsel_via_nn_amd import exact_sdp
    return (r["iters"] == exact_sdp.ITER_CAP) & (r["gap"] > exact_sdp.GAP_TOL * np.maximum(1.0, np.abs(r["value"])))


def zero_answers(r):
    """answers of the positive-semidefinite shortcut: no iteration, lam = 0"""
    return (r["iters"] == 0) & (r["lam"] == 0.0).all(axis=1)


def tiny_d_zero_answers(k, inputs, r):
    """premise 1: zero-iteration answers with some 0 < d_i <= 1e-14 whose C (+ Diag(0)) has lambda_min < -1e-3 on the active indices"""
    C, d = problem(k, inputs)
    act = d > 0
    mask = act[:, :, None] & act[:, None, :]
    lm = np.linalg.eigvalsh(np.where(mask, C, np.eye(k)[None]))[:, 0]
    return zero_answers(r) & (act & (d <= 1e-14)).any(axis=1) & (lm < -1e-3)


TIGHT = ("on_bounds", "outside", "sign_q", "neg_q", "all_minus", "one_weight", "vertex", "unitQ")


def assert_refuted(k, inputs, r, slack, name):
    """The check has not gone lax: 0.9 lam and 1.1 Y are rejected wherever the solver moved and the answer is tight.
    A solver that stops at an ABSOLUTE gap of 1e-9 returns a slack lam where the whole problem is smaller than that (d_i of 1e-10, C
    within 1e-12 of positive semidefinite: d^T lam <= 1e-9): 0.9 lam is then feasible too and must be accepted, and where Y = 0 is
    the primal answer 1.1 Y is the same certificate.  So the refutation is demanded where it is provable from the returned bracket
    alone: an accepted lam' proves  xqx - d^T lam' - k s_A <= p* <= upper  (certificate_check), so 0.9 lam has to go wherever
    0.1 d^T lam > gap + k s_A, and 1.1 Y breaks weak duality by 0.1 |<C, Y>| - gap, so it has to go wherever that exceeds s.
    On the families of TIGHT -- weights of full size on the active indices -- that is every converged input the solver moved on."""
    from sdpcutsel_via_nn_amd import exact_sdp
    eps = np.finfo(np.float64).eps
    C, d = problem(k, inputs)
    n = inputs.shape[0]
    moved = (r["iters"] > 0) & ~stalled(r)
    rr = np.sqrt(d)
    A, l = C * rr[:, :, None] * rr[:, None, :], d * r["lam"]
    s_A = slack * eps * (np.sqrt((A * A).sum(axis=(1, 2))) + np.abs(l).max(axis=1))
    s = slack * eps * (np.sqrt((C * C).sum(axis=(1, 2))) + np.abs(r["lam"]).max(axis=1))
    ia, ib = np.triu_indices(k)
    Ym = np.zeros((n, k, k))
    Ym[:, ia, ib] = r["Y"]
    Ym[:, ib, ia] = r["Y"]
    must_lam = moved & (0.1 * l.sum(axis=1) > r["gap"] + k * s_A)
    must_Y = moved & (0.1 * np.abs((C * Ym).sum(axis=(1, 2))) > r["gap"] + s)
    if name in TIGHT:
        assert np.array_equal(must_lam, moved) and np.array_equal(must_Y, moved), name
    assert not exact_sdp.certificate_check(C, d, 0.9 * r["lam"], r["Y"], slack_units=slack)["ok"][must_lam].any(), name
    assert not exact_sdp.certificate_check(C, d, r["lam"], 1.1 * r["Y"], slack_units=slack)["ok"][must_Y].any(), name
    return int(moved.sum()), int(must_lam.sum()), int(must_Y.sum())


def assert_unconverged_honest(r, bad):
    """an unconverged answer sits at the cap, says so through its gap, and is still a bracket"""
    from sdpcutsel_via_nn_amd import exact_sdp
    assert np.all(r["iters"][bad] == exact_sdp.ITER_CAP)
    assert np.all(r["gap"][bad] > exact_sdp.GAP_TOL * np.maximum(1.0, np.abs(r["value"][bad])))
    assert np.all(r["gap"] >= 0)      # value <= upper = value + gap


def assert_agree(a, bad_a, b, bad_b):
    """two implementations on the same inputs: within the two gaps where both converged (both values bracket p* from below within
    their own gaps), each lower bound under the other's upper bound otherwise"""
    both = ~bad_a & ~bad_b
    assert np.all(np.abs(a["value"] - b["value"])[both] <= (a["gap"] + b["gap"])[both] + 1e-15)
    assert np.all(a["value"] <= b["value"] + b["gap"] + 1e-12) and np.all(b["value"] <= a["value"] + a["gap"] + 1e-12)
