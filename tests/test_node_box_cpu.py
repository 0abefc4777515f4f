"""Node boxes without a GPU: the numpy twin of csrc/box.hip (sdpcutsel_via_nn_amd/nodebox.py), the algebra it rests on, the node's
McCormick block (harness.mccormick_csr_box) and the refusals.

Rounding bound of the twin against the same map in long double (a priori, eps = 2^-53 the unit roundoff; |X_ij| <= 1, 0 <= l < 1,
|x| <= 1 + 1e-9, so every product below is at most 1 in magnitude):
    t1 = fl(l_i x_j)          |err| <= eps                 a = fl(X_ij - t1)   |a| <= 1  (X_ij in [0, 1], t1 in [0, 1))
    t2 = fl(l_j x_i)          |err| <= eps                 b = fl(a - t2)      |b| <= 2
    t3 = fl(l_i l_j)          |err| <= eps                 c = fl(b + t3)      |c| <= 2
  the roundings of a, b, c add eps |a| + eps |b| + eps |c| <= eps + 2 eps + 2 eps, together with the three products 8 eps absolute on
  the numerator; the quotient r = fl(c / fl(d_i d_j)) adds two relative roundings, 2 eps |X'| (+ eps^2 terms):
      |dX'_ij| <= 8 eps / (d_i d_j) + 3 eps max(1, |X'_ij|)
  and x' = fl(fl(x - l) / d) has two relative roundings of a value of magnitude <= (1 + 1e-9) / d_i:
      |dx'_i| <= 2 eps / d_i
  (both times a factor 1 + 2^-8 on the bound: it covers the eps^2 terms, the 1e-9 excursion of one x_i and the long double
  reference's own rounding, which is 2^-11 of the float64 one per operation).  Q' = fl(Q fl(d_i d_j)): |dQ'| <= 2 eps |Q'| likewise.
"""
import os

import numpy as np
import pytest

import nodebox_cases as nc

EPS = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -8
LD = np.longdouble


def _tables(case, seed, outside=False):
    inst, _ = nc.instance(case)
    n = inst["nb_vars"]
    lb, ub = nc.random_box(n, seed)
    vv = nc.point_in_box(n, lb, ub, seed, outside=outside)
    return inst, n, lb, ub, vv


@pytest.mark.parametrize("case,seed,outside", [("spar020", 1, False), ("spar020", 2, True), ("mixed", 3, False), ("mixed", 4, True)])
def test_twin_against_long_double(case, seed, outside):
    from sdpcutsel_via_nn_amd import nodebox
    inst, n, lb, ub, vv = _tables(case, seed, outside)
    L = n * (n + 1) // 2
    Q = np.asarray(inst["Q_arr"], dtype=np.float64)
    Qb, vb = nodebox.transform_tables(Q, vv, lb, ub)
    assert Qb.dtype == np.float64 and vb.dtype == np.float64
    Qr, vr = nodebox.transform_tables(Q.astype(LD), vv.astype(LD), lb.astype(LD), ub.astype(LD))
    assert Qr.dtype == LD and vr.dtype == LD
    i, j = np.triu_indices(n)
    d = ub - lb
    dd = (d[i] * d[j])
    errX = np.abs(vb[:L].astype(LD) - vr[:L]).astype(np.float64)
    boundX = (8.0 * EPS / dd + 3.0 * EPS * np.maximum(1.0, np.abs(vb[:L]))) * SLACK
    errx = np.abs(vb[L:].astype(LD) - vr[L:]).astype(np.float64)
    boundx = 2.0 * EPS / d * SLACK
    errQ = np.abs(Qb.astype(LD) - Qr).astype(np.float64)
    boundQ = 2.0 * EPS * np.abs(Qb) * SLACK
    print("%s seed %d: max err / bound  X' %.3f  x' %.3f  Q' %.3f" % (case, seed, (errX / boundX).max(), (errx / boundx).max(),
                                                                      (errQ / np.maximum(boundQ, 1e-300)).max()))
    assert np.all(errX <= boundX) and np.all(errx <= boundx) and np.all(errQ <= boundQ)
    # the premises of the bound, and that the point is the node's (x' in [0, 1] up to the one excursion)
    assert vv[:L].min() >= 0.0 and vv[:L].max() <= 1.0 and np.abs(vv[L:]).max() <= 1.0 + 1e-9
    assert vb[L:].min() >= (-1e-9 / nc.MIN_WIDTH * SLACK if outside else 0.0) and vb[L:].max() <= 1.0 + 4 * EPS / d.min()
    assert (vb[L:].min() < 0.0) == outside


@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_unit_box_is_the_identity_bit_for_bit(case):
    from sdpcutsel_via_nn_amd import harness, nodebox
    inst, _ = nc.instance(case)
    n = inst["nb_vars"]
    Q = np.asarray(inst["Q_arr"], dtype=np.float64)
    vv = harness.random_mccormick_point(n, np.random.default_rng(5))
    Qb, vb = nodebox.transform_tables(Q, vv, np.zeros(n), np.ones(n))
    assert np.array_equal(Qb, Q) and np.array_equal(vb, vv)
    assert np.array_equal(Qb.view(np.uint64), Q.view(np.uint64))
    Q2, v2 = nodebox.inverse_tables(Qb, vb, np.zeros(n), np.ones(n))
    assert np.array_equal(Q2, Q) and np.array_equal(v2, vv)


def _lifted(vv, n):
    L = n * (n + 1) // 2
    M = np.zeros((n + 1, n + 1))
    M[0, 0] = 1.0
    M[0, 1:] = M[1:, 0] = vv[L:]
    i, j = np.triu_indices(n)
    M[1 + i, 1 + j] = vv[:L]
    M[1 + j, 1 + i] = vv[:L]
    return M


def _feasible_scaled_point(n, rng, x=None):
    """x' in (0, 1)^n and X' = x' x'^T + S R S with R a correlation matrix and S_ii^2 <= x'_i - x'_i^2: lifted matrix PSD, X'_ii <= x'_i"""
    x = rng.uniform(0.05, 0.95, n) if x is None else x
    G = rng.standard_normal((n, n + 3))
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    s = np.sqrt(rng.uniform(0.0, 1.0, n) * (x - x * x))
    X = np.outer(x, x) + (G @ G.T) * np.outer(s, s)
    i, j = np.triu_indices(n)
    return np.concatenate([X[i, j], x])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_algebra_of_the_reexpression(seed):
    from sdpcutsel_via_nn_amd import nodebox
    inst, _ = nc.instance("spar020")
    n = inst["nb_vars"]
    L = n * (n + 1) // 2
    Q = np.asarray(inst["Q_arr"], dtype=np.float64)
    lb, ub = nc.random_box(n, seed)
    rng = np.random.default_rng(seed)
    vb1 = _feasible_scaled_point(n, rng)
    vb2 = _feasible_scaled_point(n, rng, x=vb1[L:])
    assert np.abs(vb1[:L] - vb2[:L]).max() > 1e-3
    Qb, _ = nodebox.transform_tables(Q, None, lb, ub)
    diag = n * np.arange(n) - np.arange(n) * (np.arange(n) - 1) // 2
    f = []
    for vb in (vb1, vb2):
        assert np.linalg.eigvalsh(_lifted(vb, n)).min() >= -1e-12 and np.all(vb[diag] <= vb[L:] + 1e-15)
        _, vv = nodebox.inverse_tables(None, vb, lb, ub)
        x = vv[L:]
        assert np.all(x >= lb) and np.all(x <= ub)
        assert np.linalg.eigvalsh(_lifted(vv, n)).min() >= -1e-12                       # the lifted matrix stays PSD (a congruence)
        assert np.all(vv[diag] <= (lb + ub) * x - lb * ub + 1e-14)                      # the node's secant
        f.append(float(Q @ vv[:L]) - float(Qb @ vb[:L]))
    # <Q, X> - <Q', X'> does not depend on X': the same affine function of x for both
    assert abs(f[0] - f[1]) <= 1e-12 * np.abs(Q).sum()
    i, j = np.triu_indices(n)
    x = lb + (ub - lb) * vb1[L:]
    affine = float(Q @ (lb[i] * x[j] + lb[j] * x[i] - lb[i] * lb[j]))
    assert abs(f[0] - affine) <= 1e-12 * np.abs(Q).sum()


@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_mccormick_box_on_the_unit_box_is_mccormick_csr(case):
    from sdpcutsel_via_nn_amd import harness
    inst, _ = nc.instance(case)
    n = inst["nb_vars"]
    a = harness.mccormick_csr(n, inst["adj"])
    b = harness.mccormick_csr_box(n, inst["adj"], np.zeros(n), np.ones(n))
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y)
    # and the relaxation built from it
    la, lb_ = harness.boxqp_relaxation(inst), harness.boxqp_relaxation(inst, np.zeros(n), np.ones(n))
    for x, y in zip(la.linear_constraints.csr_parts(), lb_.linear_constraints.csr_parts()):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("case,seed", [("spar020", 1), ("mixed", 2), ("mixed", 3)])
def test_mccormick_box_rows_hold_on_the_box(case, seed):
    from sdpcutsel_via_nn_amd import harness
    inst, _ = nc.instance(case)
    n = inst["nb_vars"]
    L = n * (n + 1) // 2
    lb, ub = nc.random_box(n, seed)
    indptr, indices, values, rhs = harness.mccormick_csr_box(n, inst["adj"], lb, ub)
    m = rhs.shape[0]
    rows = np.repeat(np.arange(m), np.diff(indptr))
    n_edges = int(np.triu(np.asarray(inst["adj"]) != 0, 1).sum())
    li, lj = lb[np.nonzero(np.triu(np.asarray(inst["adj"]) != 0, 1))[0]], lb[np.nonzero(np.triu(np.asarray(inst["adj"]) != 0, 1))[1]]
    assert m == 2 * n + 2 * int((lb > 0).sum()) + int((ub < 1).sum()) + 3 * n_edges + int(((li > 0) | (lj > 0)).sum())
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(n)
    diag = n * np.arange(n) - np.arange(n) * (np.arange(n) - 1) // 2
    # the secant rows: +1 on a diagonal X_ii and one more entry
    first = indices[indptr[:-1]]
    secant = np.flatnonzero(np.isin(first, diag) & (values[indptr[:-1]] == 1.0) & (np.diff(indptr) == 2))
    assert secant.shape[0] == n
    pts = [lb.copy(), ub.copy()]
    pts += [np.where(rng.random(n) < 0.5, lb, ub) for _ in range(6)]                     # vertices
    pts += [lb + (ub - lb) * rng.random(n) for _ in range(6)]                             # interior points
    for p, x in enumerate(pts):
        v = np.concatenate([np.outer(x, x)[iu], x])
        act = np.bincount(rows, weights=values * v[indices], minlength=m)
        assert np.all(act <= rhs + 1e-12), (p, float((act - rhs).max()))
        if p < 8:      # every coordinate sits on a bound: the secants are tight
            assert np.abs(act[secant] - rhs[secant]).max() <= 1e-12


def test_node_lp_is_at_least_the_root_lp():
    from sdpcutsel_via_nn_amd import harness
    inst, _ = nc.instance("spar020")
    for depth in (1, 2):
        lb, ub, root = nc.child_box(inst, depth)
        assert (ub - lb).min() < 1.0
        lp = harness.boxqp_relaxation(inst, lb, ub)
        lp.solve()
        node = lp.get_objective_value()
        print("depth %d: root LP %.6f, node LP %.6f" % (depth, root, node))
        assert node >= root - 1e-7 * max(1.0, abs(root))      # (HiGHS' feasibility tolerance; the model minimises)


def test_check_box_refuses_what_the_library_refuses():
    from sdpcutsel_via_nn_amd import nodebox
    n = 6
    lb, ub = np.zeros(n), np.ones(n)
    out = nodebox.check_box(n, lb, ub)
    assert np.array_equal(out[0], lb) and np.array_equal(out[1], ub)
    ok = nodebox.check_box(n, np.full(n, 0.5), np.full(n, 0.5 + 2.0 ** -10))      # the minimum width itself is served
    assert ok[0].dtype == np.float64

    def bad(i_lb=None, i_ub=None, shape=None):
        l, u = lb.copy(), ub.copy()
        if i_lb is not None:
            l[2] = i_lb
        if i_ub is not None:
            u[2] = i_ub
        if shape:
            l = l[:shape]
        with pytest.raises(ValueError):
            nodebox.check_box(n, l, u)

    bad(i_lb=-1e-12)                        # l < 0
    bad(i_ub=1.0 + 1e-12)                   # u > 1
    bad(i_lb=float("nan"))
    bad(i_ub=float("nan"))
    bad(i_lb=float("-inf"))
    bad(i_ub=float("inf"))
    bad(i_lb=0.5, i_ub=0.5)                 # a fixed variable
    bad(i_lb=0.6, i_ub=0.4)                 # l > u
    bad(i_lb=0.5, i_ub=0.5 + 2.0 ** -11)    # below the minimum width
    bad(shape=5)
    assert nodebox.BOX_MIN_WIDTH == 2.0 ** -10
    hdr = open(os.path.join(nc.ROOT, "include", "sdpcut.h")).read()
    import re
    assert float(re.search(r"#define SDPCUT_BOX_MIN_WIDTH ([0-9.eE+-]+)", hdr).group(1)) == nodebox.BOX_MIN_WIDTH


def test_new_entry_points_are_declared_bound_and_refuse_a_null_handle():
    """the host-only argument checks: a NULL handle is SDPCUT_EINVAL before anything touches a device"""
    import ctypes
    from sdpcutsel_via_nn_amd import _capi, build
    build.build(verbose=False)
    lib = _capi.load_library()
    names = ("sdpcut_set_box", "sdpcut_get_box", "sdpcut_get_box_tables")
    hdr = open(os.path.join(nc.ROOT, "include", "sdpcut.h")).read()
    for name in names:
        assert name in _capi.SIGNATURES and ("int %s(" % name) in hdr
    z = (ctypes.c_double * 4)()
    flag = ctypes.c_int(7)
    assert lib.sdpcut_set_box(None, z, z) == -1
    assert lib.sdpcut_get_box(None, z, z, ctypes.byref(flag)) == -1 and flag.value == 7
    assert lib.sdpcut_get_box_tables(None, z, z) == -1
    for meth in ("set_box", "clear_box", "box", "box_tables"):
        assert hasattr(_capi.Scorer, meth)
