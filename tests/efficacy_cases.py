"""Inputs of the efficacy tests (tests/test_gpu_efficacy.py), built from committed fixtures only, and the numpy truth they are
compared with.  No device is needed here: tests/test_efficacy_cpu.py checks on the CPU what the GPU tests assume about these
inputs (every size class present, waves that mix violated and non-violated lanes, the gap rule excluding at most 1 %)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
INST = os.path.join(GOLDEN, "instances")
NEG = -1e-15
LENGTHS = (1, 63, 64, 65, 1000)      # one lane, a wave less one, a wave, a wave plus one, many waves


class Case(object):
    """one candidate list at one LP point: n, Q_arr, S int32 [N, 5], ks int32 [N], point [X packed | x], obj (the instance's LP
    objective [Q_arr | c]) and whether the list is a generic one (test 2 applies) or a structured one (test 1 only)"""

    def __init__(self, name, n, Q_arr, S, ks, point, obj, generic):
        self.name, self.n, self.Q_arr, self.point, self.obj, self.generic = name, int(n), np.asarray(Q_arr, dtype=np.float64), point, obj, generic
        self.S, self.ks = np.ascontiguousarray(S, dtype=np.int32), np.ascontiguousarray(ks, dtype=np.int32)

    @property
    def N(self):
        return self.ks.shape[0]

    def prefix(self, count):
        return Case("%s[:%d]" % (self.name, count), self.n, self.Q_arr, self.S[:count], self.ks[:count], self.point, self.obj, self.generic)


@functools.lru_cache(maxsize=None)
def instance(name):
    from sdpcutsel_via_nn_amd import harness
    return harness.parse_boxqp(os.path.join(INST, name))


@functools.lru_cache(maxsize=None)
def cover(name, dim):
    from sdpcutsel_via_nn_amd import _capi
    S, ks, _ = _capi.enumerate_cover(instance(name)["adj"], dim)
    return np.ascontiguousarray(S, dtype=np.int32), np.ascontiguousarray(ks, dtype=np.int32)


def lp_objective(inst):
    return np.concatenate([np.asarray(inst["Q_arr"], dtype=np.float64), np.asarray(inst["c"], dtype=np.float64)])


@functools.lru_cache(maxsize=None)
def mixed_sets(name="spar040-030-1.in"):
    """1024 index sets on one instance, shuffled: its dim-3, dim-4 and dim-5 covers (531 sets, some of them in two covers: equal
    scores) filled up with random subsets of 2 .. 5 variables -- every k in every stretch of the list"""
    parts = [cover(name, d) for d in (3, 4, 5)]
    S, ks = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    rng = np.random.default_rng(606)
    n = instance(name)["nb_vars"]
    extra = 1024 - ks.shape[0]
    assert extra > 0
    ke = rng.integers(2, 6, extra).astype(np.int32)
    Se = np.full((extra, 5), -1, dtype=np.int32)
    for i in range(extra):
        Se[i, :ke[i]] = np.sort(rng.choice(n, int(ke[i]), replace=False))
    S, ks = np.concatenate([S, Se]), np.concatenate([ks, ke])
    order = rng.permutation(ks.shape[0])
    return S[order], ks[order]


def random_point(n, seed):
    from sdpcutsel_via_nn_amd import harness
    return harness.random_mccormick_point(n, np.random.default_rng(seed))


def mccormick_vertex(inst):
    """the optimum of the McCormick relaxation of a BoxQP instance: x = 0.5, X_ii = 0.5, X_ij in {0, 0.5} by the sign of q_ij"""
    n = inst["nb_vars"]
    Q = np.asarray(inst["Q_arr"], dtype=np.float64)
    X = np.where(Q < 0, 0.5, 0.0)
    iu = np.triu_indices(n)
    X[iu[0] == iu[1]] = 0.5
    return np.concatenate([X, np.full(n, 0.5)])


def psd_point(n, seed):
    """X = x x^T + a small PSD term (0.01 I): the Schur complement of every lifted sub-matrix is 0.01 I, nothing is violated"""
    x = np.random.default_rng(seed).uniform(0.05, 0.95, n)
    X = np.outer(x, x) + 0.01 * np.eye(n)
    return np.concatenate([X[np.triu_indices(n)], x])


def recorded_point(fixture, round_no):
    """the LP point round ``round_no`` of a recorded run separated at (tests/golden/rounds_*.npz)"""
    z = np.load(os.path.join(GOLDEN, fixture))
    return np.array(z["r%02d_vars" % round_no], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def generic_cases():
    """random interior points on the mixed list (N = 1, 63, 64, 65, 1000) and recorded LP points after round 2"""
    inst = instance("spar040-030-1.in")
    S, ks = mixed_sets()
    obj = lp_objective(inst)
    out = []
    for count in LENGTHS:
        c = Case("mixed/rnd", inst["nb_vars"], inst["Q_arr"], S, ks, random_point(inst["nb_vars"], 7 + count), obj, True)
        out.append(c.prefix(min(count, c.N)))
    for fixture, name, dim in (("rounds_spar070_050_1_d5_s4.npz", "spar070-050-1.in", 5), ("rounds_spar125_075_1_d3_s2.npz", "spar125-075-1.in", 3)):
        i2 = instance(name)
        S2, ks2 = cover(name, dim)
        take = np.random.default_rng(3).permutation(ks2.shape[0])[:1000]      # (a thousand candidates of the cover: seconds, not minutes, of numpy truth)
        take.sort()
        out.append(Case("lp3/" + name, i2["nb_vars"], i2["Q_arr"], S2[take], ks2[take], recorded_point(fixture, 3), lp_objective(i2), True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def structured_cases(clustered=True):
    """the all-non-violated list, the McCormick vertex x = 0.5 and the clustered spectra (tests/spectra_cases.py): test 1 only --
    lambda_min is multiple or nearly so there, a vector of the eigenspace is not unique and no independent truth exists for it"""
    import spectra_cases
    inst = instance("spar040-030-1.in")
    S, ks = mixed_sets()
    obj = lp_objective(inst)
    n = inst["nb_vars"]
    out = [Case("mixed/psd", n, inst["Q_arr"], S[:1000], ks[:1000], psd_point(n, 5), obj, False),
           Case("mixed/vertex", n, inst["Q_arr"], S[:1000], ks[:1000], mccormick_vertex(inst), obj, False)]
    for k in (spectra_cases.KS if clustered else ()):
        p = spectra_cases.packed(k)
        o = p["orders"]["mixed"]
        L = p["n"] * (p["n"] + 1) // 2
        ob = np.concatenate([np.asarray(p["Q_arr"], dtype=np.float64), np.linspace(-1.0, 1.0, p["n"])])
        assert ob.shape[0] == L + p["n"]
        out.append(Case("clustered/k%d" % k, p["n"], p["Q_arr"], o["S"], o["ks"], np.asarray(p["point"], dtype=np.float64), ob, False))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------ numpy truth
def lifted(case, i):
    """[[1, x^T], [x, X]] of candidate i of a case"""
    k, n = int(case.ks[i]), case.n
    s = case.S[i, :k].astype(np.int64)
    L = n * (n + 1) // 2
    A = np.empty((k + 1, k + 1))
    A[0, 0] = 1.0
    A[0, 1:] = A[1:, 0] = case.point[L + s]
    for a in range(k):
        for b in range(a, k):
            A[1 + a, 1 + b] = A[1 + b, 1 + a] = case.point[n * s[a] - s[a] * (s[a] + 1) // 2 + s[b]]
    return A


def row_of(v):
    """the cut coefficients of an eigenvector (cut_select_qp.py:744-746): |v_i| <= 1e-15 zeroed, v_i v_j, doubled off the diagonal"""
    v = np.where(np.abs(v) <= 1e-15, 0.0, v)
    D = v.shape[0]
    return np.array([(2.0 if i != j else 1.0) * v[i] * v[j] for i in range(D) for j in range(max(i, 1), D)])


def truth(case):
    """-> (lam [N], eff [N], separated bool [N]) from numpy.linalg.eigh: eff = -lam / ||coef(v)|| for lam < -1e-15; separated where
    lambda_min is at least 1e-6 ||A||_F away from the next eigenvalue (numpy.linalg.eigvalsh)"""
    N = case.N
    lam, eff, sep = np.zeros(N), np.zeros(N), np.zeros(N, dtype=bool)
    for i in range(N):
        A = lifted(case, i)
        w = np.linalg.eigvalsh(A)
        sep[i] = (w[1] - w[0]) >= 1e-6 * np.linalg.norm(A)
        ww, V = np.linalg.eigh(A)
        lam[i] = ww[0]
        if ww[0] < NEG:
            eff[i] = -ww[0] / np.linalg.norm(row_of(V[:, 0]))
    return lam, eff, sep
