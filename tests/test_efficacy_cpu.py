"""The numpy twin of the efficacy measure (sdpcutsel_via_nn_amd/efficacy.py) on its own, and what the GPU tests assume about
their inputs (tests/efficacy_cases.py).  No device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import efficacy_cases as ec  # noqa: E402
from sdpcutsel_via_nn_amd import efficacy  # noqa: E402


def random_rows(k, count, seed):
    """violated rows of size k: a random symmetric lifted matrix with a negative lambda_min, the row of its eigenvector on made-up
    distinct columns, and a point z on those columns -> (lam [c], coef [c, 20], cols [c, 20], ks [c], rhs [c], z [c, M])"""
    rng = np.random.default_rng([k, seed])
    M = k + k * (k + 1) // 2
    lam, coef, cols, rhs, zs = np.zeros(count), np.zeros((count, 20)), np.full((count, 20), -1, dtype=np.int64), np.zeros(count), np.zeros((count, M))
    got = 0
    while got < count:
        x = rng.uniform(0, 1, k)
        X = rng.uniform(0, 1, (k, k))
        X = (X + X.T) / 2
        A = np.block([[np.ones((1, 1)), x[None, :]], [x[:, None], X]])
        w, V = np.linalg.eigh(A)
        if not w[0] < -1e-3:
            continue
        v = V[:, 0]
        lam[got] = w[0]
        coef[got, :M] = ec.row_of(v)
        cols[got, :M] = rng.permutation(400)[:M]
        rhs[got] = -v[0] * v[0]
        iu = np.triu_indices(k)
        zs[got] = np.concatenate([x, X[iu]])
        got += 1
    return lam, coef, cols, np.full(count, k, dtype=np.int32), rhs, zs


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_efficacy_is_the_distance_to_the_cut(k):
    """z + eff coef / ||coef||, restricted to the row's columns, meets the cut with equality.  lam is the row's own violation
    a.z - rhs (long double, rounded once): for an exact unit eigenvector that IS lambda_min, and the property under test is the
    measure's, not an eigensolver's."""
    _, coef, cols, ks, rhs, zs = random_rows(k, 200, 1)
    M = k + k * (k + 1) // 2
    ld = np.longdouble
    lam = np.array([float(np.sum(coef[t, :M].astype(ld) * zs[t].astype(ld)) - ld(rhs[t])) for t in range(200)])
    assert np.all(lam < -1e-4)
    eff, objpar, escore = efficacy.measure(lam, coef, cols, ks)
    assert np.all(eff > 0) and np.all(objpar == 0.0) and np.array_equal(eff, escore)
    for t in range(lam.shape[0]):
        a, z = coef[t, :M].astype(ld), zs[t].astype(ld)
        nrm = np.sqrt(np.sum(a * a))
        moved = z + ld(eff[t]) * a / nrm
        tol = (M + 4) * ld(2.0) ** -52 * (1 + np.max(np.abs(z)) * np.sum(np.abs(a))) / nrm
        assert abs(np.sum(a * moved) - ld(rhs[t])) / nrm <= tol, (k, t)


def test_sign_rule_at_the_edges():
    coef = np.zeros((5, 20))
    coef[:, :5] = [0.6, 0.0, -0.8, 0.0, 0.0]
    cols = np.tile(np.arange(20), (5, 1))
    ks = np.full(5, 2, dtype=np.int32)
    lam = np.array([-1e-15, -1.0000000000000002e-15, 0.0, 0.25, -0.5])
    eff, objpar, escore = efficacy.measure(lam, coef, cols, ks)
    assert eff[0] == 0.0 and not np.signbit(eff[0])            # lam = -1e-15 exactly: not violated (the test is lam < -1e-15)
    assert eff[1] == 1.0000000000000002e-15 / 1.0              # the next double below: violated, ||coef|| = 1
    assert eff[2] == 0.0 and not np.signbit(eff[2])            # lam = 0: +0, not -0
    assert eff[3] == -0.25                                     # min(-lam, 0)
    assert eff[4] == 0.5
    assert np.array_equal(eff > 0, lam < -1e-15)
    assert np.array_equal(escore, eff) and np.all(objpar == 0.0)
    # a zero row is not a cut whatever lam says
    e0, p0, s0 = efficacy.measure(np.array([-0.5]), np.zeros((1, 20)), cols[:1], ks[:1], obj=np.ones(20), w=0.3)
    assert (e0[0], p0[0], s0[0]) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_objective_parallelism(k):
    lam, coef, cols, ks, rhs, zs = random_rows(k, 100, 2)
    M = k + k * (k + 1) // 2
    rng = np.random.default_rng(k)
    obj = rng.normal(size=400)
    eff, objpar, escore = efficacy.measure(lam, coef, cols, ks, obj=obj, w=0.1)
    assert np.all((objpar >= 0.0) & (objpar <= 1.0)) and objpar.max() > 0.0
    assert np.array_equal(escore, eff + 0.1 * objpar)
    # a row proportional to the objective on its columns, zeros elsewhere: parallelism 1
    for t in range(5):
        o = np.zeros(400)
        o[cols[t, :M]] = -3.0 * coef[t, :M]
        _, p, _ = efficacy.measure(lam[t:t + 1], coef[t:t + 1], cols[t:t + 1], ks[t:t + 1], obj=o)
        assert abs(p[0] - 1.0) <= 4 * 2.0 ** -52
    # invariant to the scale of obj (powers of two exactly, others to rounding)
    _, p2, _ = efficacy.measure(lam, coef, cols, ks, obj=4.0 * obj)
    assert np.array_equal(p2, objpar)
    _, p3, _ = efficacy.measure(lam, coef, cols, ks, obj=-7.3 * obj)
    # (absolute: sum |coef obj| <= ||coef|| ||obj||, so M products, M sums, two norms and a division move objpar by <= (M + 4) ulp of 1)
    assert np.max(np.abs(p3 - objpar)) <= (M + 4) * 2.0 ** -52
    # w = 0: the same escore with and without an objective
    e_a, _, s_a = efficacy.measure(lam, coef, cols, ks)
    e_b, _, s_b = efficacy.measure(lam, coef, cols, ks, obj=obj, w=0.0)
    assert np.array_equal(s_a, s_b) and np.array_equal(e_a, e_b) and np.array_equal(s_a, e_a)
    for bad in (np.zeros(400), np.full(400, np.nan)):
        with pytest.raises(ValueError):
            efficacy.measure(lam, coef, cols, ks, obj=bad)
    for w in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            efficacy.measure(lam, coef, cols, ks, w=w)


def test_ranking_breaks_ties_by_ascending_index():
    escore = np.array([0.0, 0.5, 0.25, 0.5, 0.0, -1.0, 0.25, 0.5])
    assert efficacy.ranking(escore).tolist() == [1, 3, 7, 2, 6, 0, 4, 5]
    assert efficacy.objective_norm(np.array([3.0, 4.0])) == 5.0


def test_check_round_sees_a_row_that_is_not_violated():
    lam, coef, cols, ks, rhs, zs = random_rows(3, 4, 3)
    # one row per candidate on its own point: checked one at a time
    for t in range(4):
        p = np.zeros(400)
        p[cols[t, :9]] = zs[t]
        eff = efficacy.measure(lam[t:t + 1], coef[t:t + 1], cols[t:t + 1], ks[t:t + 1])[0]
        args = (p, [0, 9], cols[t, :9], coef[t, :9], rhs[t:t + 1])
        assert efficacy.check_round(*args, eff=eff, lam=lam[t:t + 1], quota=1) == []
        assert efficacy.check_round(*args, quota=0)                                   # over the quota
        assert efficacy.check_round(p, [0, 9], cols[t, :9], -coef[t, :9], -rhs[t:t + 1])     # the row reversed: satisfied, not violated
        assert efficacy.check_round(*args, eff=eff * 1.001, lam=lam[t:t + 1])          # a wrong efficacy


# ------------------------------------------------------------------------------------------ what the GPU tests assume
def test_inputs_of_the_gpu_tests():
    gen = ec.generic_cases()
    viol_total = excluded = 0
    for c in gen:
        lam, eff, sep = ec.truth(c)
        viol = lam < ec.NEG
        viol_total += int(viol.sum())
        excluded += int((viol & ~sep).sum())
        if c.N >= 1000 and c.name.startswith("mixed"):
            assert set(np.unique(c.ks).tolist()) == {2, 3, 4, 5}
            waves = [viol[a:a + 64] for a in range(0, c.N - 63, 64)]
            assert sum(1 for w in waves if 0 < w.sum() < 64) >= 3            # waves that mix violated and non-violated lanes
    assert viol_total > 1000
    assert excluded <= 0.01 * viol_total, (excluded, viol_total)              # the gap rule excludes at most 1 % on the generic lists
    st = {c.name: c for c in ec.structured_cases(clustered=False)}      # (the clustered spectra have tests of their own)
    lam, _, _ = ec.truth(st["mixed/psd"])
    assert np.all(lam > 1e-3)                                                 # entirely non-violated
    lam, _, sep = ec.truth(st["mixed/vertex"])
    assert (lam < ec.NEG).sum() > 100
