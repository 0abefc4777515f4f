"""Dense eigen-cuts (strategy 0), the parts that need no GPU: the numpy twin of the device eigensolver against numpy.linalg.eigh,
the row layout against a restatement of the reference's generator, the binding, and the loop's acceptance of strat=0.

`reference_dense_rows` is the checker of this module and of tests/test_gpu_dense.py: cut_select_qp.py:757-786 restated on
numpy.linalg.eigh(A, "U") -- the reference's own arithmetic, entry by entry, without the LP object."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

EPS = 2.0 ** -52
NEG = -1e-15

# Constant of the eigenvalue bound |lambda - lambda_numpy| <= C eps ||A||_F: 4 x the largest error measured over the matrices of
# dense_points(), in units of eps F (rotation order and fused roundings move it).  The numpy twin's largest error is 7.94 (generated
# point, n = 127; test_twin_against_eigh prints every figure).  The kernel's own figure on an MI355X is printed by
# tests/test_gpu_dense.py::test_eigenvalues_and_row_count; it had NOT been measured when this constant was set (DESIGN.md section 5,
# "Dense eigen-cuts"), so C rests on the twin alone: the twin runs the kernel's rotations in the kernel's order and differs from it
# only in roundings (no fused multiply-add, IEEE sqrt and division).  A kernel figure above 7.94 moves C to 4 x that figure.
# The algorithm is wrong, not the constant, if C > 8 D: at the two smallest orders (D = 3: 24) the bound used is min(C, 8 D).
MEASURED_TWIN_EPS_F = 7.94
C_EIG = 4.0 * MEASURED_TWIN_EPS_F


def c_eig(D):
    return min(C_EIG, 8.0 * D)


def dense_points():
    """(name, n, LP point) of every matrix the issue lists: generated McCormick-feasible points (seed 7, the C2 generator) at
    n = 2, 3, 62, 63, 127, the golden points of spar020 / spar040 and four recorded LP points of the reference's own runs."""
    from sdpcutsel_via_nn_amd import synthetic
    out = [("gen%03d" % n, n, synthetic.make_instance(n, 7)[1]) for n in (2, 3, 62, 63, 127)]
    z = np.load(os.path.join(GOLDEN, "inst_boxqp.npz"))
    out += [("spar020_" + p, 20, z["spar020_100_1_d3_%s_vars" % p]) for p in ("mck", "rnd", "psd")]
    out.append(("spar040_mck", 40, z["spar040_030_1_d5_mck_vars"]))
    for f, n in (("rounds_spar070_050_1_d5_s4.npz", 70), ("rounds_spar125_075_1_d3_s2.npz", 125)):
        z = np.load(os.path.join(GOLDEN, f))
        out += [("spar%03d_%s" % (n, r), n, z[r + "_vars"]) for r in ("r01", "r12")]
    return out


def reference_dense_rows(vars_values, n):
    """cut_select_qp.py:757-786 in other words -> (A, eigvals, evecs, cols, rows [nb, row_len], rhs [nb])."""
    L = n * (n + 1) // 2
    X_vals, x_vals = vars_values[:L], vars_values[L:L + n]
    mat = np.zeros((n + 1, n + 1))
    mat[0, 0] = 1
    mat[0, 1:] = x_vals
    r_, c_ = np.triu_indices(n)
    mat[r_ + 1, c_ + 1] = X_vals
    eigvals, evecs = np.linalg.eigh(mat, "U")
    rows, rhs = [], []
    for ix in range(n):                                   # never the largest eigenvalue (:773)
        if eigvals[ix] < NEG:
            v = evecs.T[ix]
            rows.append([v[a] * v[b] * 2 if a != b else v[a] * v[b] for a in range(n + 1) for b in range(max(a, 1), n + 1)])
            rhs.append(-v[0] * v[0])
    cols = [x + L for x in range(n)] + list(range(L))
    A = np.triu(mat) + np.triu(mat, 1).T
    return A, eigvals, evecs, np.array(cols), np.array(rows).reshape(len(rows), n + L), np.array(rhs)


POINTS = None


def points():
    global POINTS
    if POINTS is None:
        POINTS = dense_points()
    return POINTS


@pytest.fixture(scope="module")
def references():
    """the restated reference at every point, computed once"""
    return {name: reference_dense_rows(vv, n) for name, n, vv in points()}


NAMES = ["gen002", "gen003", "gen062", "gen063", "gen127", "spar020_mck", "spar020_rnd", "spar020_psd", "spar040_mck",
         "spar070_r01", "spar070_r12", "spar125_r01", "spar125_r12"]
# rows the reference generates at the points where no eigenvalue lies near the threshold (checked: none within 1e-9 of zero)
EXACT_ROWS = {"spar020_mck": 11, "spar020_psd": 0, "spar070_r01": 35, "spar070_r12": 27, "spar125_r01": 62, "spar125_r12": 61}


def test_points_are_the_listed_ones(references):
    assert [p[0] for p in points()] == NAMES
    for name, nb in EXACT_ROWS.items():
        A, w = references[name][0], references[name][1]
        assert references[name][4].shape[0] == nb
        assert np.abs(w).min() > 1e-9
    w40 = references["spar040_mck"][1]
    assert np.abs(w40).min() < 1e-15          # the threshold case: an eigenvalue that is zero to rounding


@pytest.mark.parametrize("name", NAMES)
def test_twin_against_eigh(references, name):
    """The kernel's algorithm in numpy (same ordering, same stop rule, same sort): eigenvalues within C eps F of LAPACK's, residual
    and orthogonality of the vectors, the row count within the band the eigenvalue bound allows, and convergence well inside the cap."""
    from sdpcutsel_via_nn_amd import dense
    A, w = references[name][0], references[name][1]
    D = A.shape[0]
    F = np.linalg.norm(A)
    lam, V, sweeps = dense.jacobi_twin(A)
    C = c_eig(D)
    err = np.abs(lam - w).max() / (EPS * F)
    print("%s: D %d sweeps %d max |d lambda| %.2f eps F" % (name, D, sweeps, err))
    assert C <= 8 * D
    assert err <= C
    assert sweeps < dense.MAX_SWEEPS and sweeps <= 12
    assert np.abs(A @ V - V * lam).max() <= C * EPS * F
    assert np.abs(V.T @ V - np.eye(D)).max() <= 4 * D * EPS
    G = C * EPS * F
    nb = dense.count_rows(lam)
    assert np.count_nonzero(w[:-1] < NEG - G) <= nb <= np.count_nonzero(w[:-1] < NEG + G)
    if name in EXACT_ROWS:
        assert nb == EXACT_ROWS[name]


def test_tournament_visits_every_pair_once():
    from sdpcutsel_via_nn_amd import dense
    for m in (4, 6, 64, 126, 128):
        seen = set()
        for step in range(m - 1):
            p, q = dense.tournament_pairs(m, step)
            assert p.shape[0] == m // 2 and np.all(p < q)
            assert sorted(np.concatenate([p, q]).tolist()) == list(range(m))      # disjoint: everybody plays once per step
            seen.update(zip(p.tolist(), q.tolist()))
        assert len(seen) == m * (m - 1) // 2


@pytest.mark.parametrize("name", ["gen002", "gen003", "spar020_mck", "spar070_r12"])
def test_layout_against_restated_reference(references, name):
    """row_cols / row_values / lifted_matrix = the reference's column list, its comprehension and its matrix, exactly"""
    from sdpcutsel_via_nn_amd import dense
    n, vv = next((p[1], p[2]) for p in points() if p[0] == name)
    A, w, V, cols, rows, rhs = references[name]
    assert np.array_equal(dense.lifted_matrix(vv, n), A)
    assert np.array_equal(dense.row_cols(n), cols) and dense.row_len(n) == cols.shape[0]
    k = 0
    for ix in range(n):
        if w[ix] < NEG:
            val, r = dense.row_values(V[:, ix])
            assert np.array_equal(val, rows[k]) and r == rhs[k]
            k += 1
    assert k == rows.shape[0]


def test_binding_declares_both_functions():
    from sdpcutsel_via_nn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    for name in ("sdpcut_dense_round", "sdpcut_dense_eig"):
        assert name in _capi.SIGNATURES
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M)
    assert [f[0] for f in _capi.DenseRound._fields_] == ["dim", "n_rows", "sweeps", "reserved", "row_len", "eigvals", "cols", "values", "rhs"]
    assert int(re.search(r"#define SDPCUT_DENSE_MAX_VARS (\d+)", hdr).group(1)) == 127
    lib = _capi.load_library()
    assert hasattr(lib, "sdpcut_dense_round") and hasattr(lib, "sdpcut_dense_eig")
    assert callable(_capi.Scorer.dense_round) and callable(_capi.Scorer.dense_eig)


def test_mangled_name_resolves_to_the_mixin():
    """the reference's loop calls self.__gen_dense_eigcuts inside class CutSolver (cut_select_qp.py:166): on a composed class that
    name must be the mixin's method"""
    import sdpcutsel_via_nn_amd as pkg
    M = pkg.GpuCutSelectionMixin
    assert M._CutSolver__gen_dense_eigcuts is M._gen_dense_eigcuts

    class CutSolver(object):
        def __gen_dense_eigcuts(self, vars_values=None): raise AssertionError("CPU dense generation reached")
        def via_loop(self): return self.__gen_dense_eigcuts

    class mod: pass
    mod.CutSolver = CutSolver
    G, _ = pkg.make_dropin_classes(mod)
    assert G().via_loop().__func__ is M._gen_dense_eigcuts


def test_strategy_zero_is_accepted_and_fails_only_for_want_of_a_device():
    """cut_select_algo(strat=0) passes the argument checks (strategy 3 still does not) and gets as far as creating its handle"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    path = os.path.join(GOLDEN, "instances", "spar020-100-1.in")
    cs = pkg.CutSolver()
    with pytest.raises(AssertionError):
        cs.cut_select_algo(path, 3, 0.1, strat=3)
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if have_gpu:
        out = cs.cut_select_algo(path, 3, 0.1, strat=0, nb_rounds_cuts=0)
        assert out[-1] == 1051
    else:
        with pytest.raises(_capi.SdpCutError, match="sdpcut_create failed"):
            cs.cut_select_algo(path, 3, 0.1, strat=0, nb_rounds_cuts=1)
