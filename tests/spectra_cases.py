"""Lifted matrices [[1, x^T], [x, X]] of order D = k + 1 (k = 2..5) with a multiple or nearly multiple smallest eigenvalue and KNOWN
truth: the exact spectrum (fractions.Fraction) and the orthogonal projector onto every eigenvalue cluster (test infrastructure of
tests/test_spectra_cases_cpu.py and tests/test_gpu_clustered_spectra.py; no GPU).

Families
  A  exact dyadic.  Q = a product of two or three reflectors I - 2 u u^T / (u^T u), u with two or four entries +-1 (u^T u a power of
     two), random column signs and order; Lambda dyadic.  M = Q Lambda Q^T is formed in Fraction arithmetic, the large eigenvalue is
     the one that makes M_00 = 1, and a draw is rejected unless that eigenvalue and every entry of M is a double: spectrum and
     eigenspaces are then known without any solver.  D = 3 admits only reflectors with two ones, whose products are signed
     permutations: the family is left out for k = 2.
  B  generic clusters.  Haar Q, nominal gaps 1e-16 .. 1e-3 (one per decade), two- and three-fold; symmetrised, divided by M_00, M_00
     set to 1.  Truth: mpmath.eigsy of the ROUNDED matrix at 60 digits; the gaps used are the actual ones.
  C  LP noise on structured vertices.  x = 0.5, X in {0, 0.5}, every entry moved by a random multiple (|m| <= 8) of 2^-50: the
     couplings that decide on which side of -1e-15 a zero eigenvalue falls.  Truth from mpmath.

Clusters.  The cluster of an eigenvalue is every eigenvalue within TAU = 1e-6 of it; it QUALIFIES for projector assertions when
everything else is at least SEP = 1e-3 away from all of its members.  Gaps between TAU and SEP are part of the prescribed cases
(2^-10 in A, the nominal 1e-5, 1e-4, 1e-3 in B): their lambda_min is a cluster of its own that does not qualify; tests that want
the projector there use the bound that follows from a residual (see near_ok).

Packing.  One LP point per k over DISJOINT index sets: 40 variables carry a generic McCormick point (the lanes that converge in
three evaluations), then every matrix gets k fresh variables -- twice, so that every matrix has a twin at other indices.  Two list
orders over the same point: "sorted" (family by family, the twin right behind the first copy: whole waves of 64 are clustered) and
"mixed" (every clustered lane among three generic ones, the twins in a second pass).
"""
import functools
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TAU = 1e-6            # the separation from which the project compares vectors (tests/test_gpu_round3.py)
SEP = 1e-3            # a qualifying cluster is this far from the rest of the spectrum
NEG = -1e-15          # _THRES_NEG_EIGVAL
LAM_TOL = 3e-15       # |lambda - mu| / s (tests/test_gpu_round4.py, test_lambda_min_on_points_outside_the_lp_box)
PER_FAMILY = 64       # matrices per (k, family)
GENERIC_VARS = 40
KS = (2, 3, 4, 5)
FAMILIES = ("A", "B", "C")
_SHIFT = 240          # mpmath values are kept as Fractions over 2^240


class Case(object):
    """M float64 [D, D]; spectrum: ascending Fractions; vectors float64 [D, D] (columns, truth to double rounding, exact for A);
    members[j]: indices of the cluster of eigenvalue j; proj[j]: its projector; qualifies[j]; sep[j]: distance of the cluster of j
    from the rest; s = 1 + 2 sum|x| + 2 sum|X| (the project's scale of a lifted matrix); gap: mu_1 - mu_0 as a float."""

    def __init__(self, k, family, tag, M, spectrum, vectors):
        self.k, self.family, self.tag = int(k), family, tag
        self.M = np.ascontiguousarray(M, dtype=np.float64)
        D = self.k + 1
        assert self.M.shape == (D, D) and np.array_equal(self.M, self.M.T) and self.M[0, 0] == 1.0
        order = sorted(range(D), key=lambda j: spectrum[j])
        self.spectrum = [spectrum[j] for j in order]
        self.vectors = np.asarray(vectors, dtype=np.float64)[:, order]
        mu = self.spectrum
        self.members, self.proj, self.qualifies, self.sep = [], [], [], []
        for j in range(D):
            mem = [i for i in range(D) if abs(mu[i] - mu[j]) <= TAU]
            rest = [i for i in range(D) if i not in mem]
            sep = min([float(abs(mu[i] - mu[m])) for i in rest for m in mem] or [np.inf])
            V = self.vectors[:, mem]
            self.members.append(mem)
            self.proj.append(V @ V.T)
            self.sep.append(sep)
            self.qualifies.append(sep >= SEP)
        iu = np.triu_indices(self.k)
        self.x = self.M[0, 1:].copy()
        self.X = self.M[1:, 1:][iu].copy()
        self.s = 1.0 + 2.0 * float(np.abs(self.x).sum()) + 2.0 * float(np.abs(self.X).sum())
        self.gap = float(mu[1] - mu[0])

    def near_ok(self, j, residual=1e-12):
        """the cluster of eigenvalue j is far enough from the rest for ANY vector with the documented residual r = 1e-12 max(||M||, 1)
        to lie in it to 1e-9: 1 - <B, P> = sin^2 <= (r / sep)^2 (Davis-Kahan), asked to be <= 1e-10; holds from sep ~ 1e-7 ||M|| on"""
        return (residual * max(float(np.abs(self.M).max()), 1.0) / self.sep[j]) ** 2 <= 1e-10


# ------------------------------------------------------------------------------------------------------------ exact helpers
def frac(v):
    return Fraction(float(v))


def frac_matrix(A):
    A = np.asarray(A, dtype=np.float64)
    return [[Fraction(float(A[i, j])) for j in range(A.shape[1])] for i in range(A.shape[0])]


def representable(q):
    try:
        return Fraction(float(q)) == q
    except OverflowError:
        return False


def fmatmul(A, B):
    n, m, p = len(A), len(B), len(B[0])
    return [[sum(A[i][t] * B[t][j] for t in range(m)) for j in range(p)] for i in range(n)]


def to_int(A):
    """a matrix of doubles -> (rows of Python ints Z, shift) with A = Z 2^-shift exactly"""
    import math
    A = np.asarray(A, dtype=np.float64)
    shift = 0
    for v in A.ravel():
        if v != 0.0:
            shift = max(shift, 53 - math.frexp(float(v))[1])
    one = 1 << shift
    return [[int(Fraction(float(v)) * one) for v in row] for row in A], shift


def row_measures(B, M, mu, P=None):
    """Exact (integer arithmetic) measures of a row's matrix B against the lifted matrix M and the true eigenvalue mu (Fraction):
    -> dict(trace |tr B - 1|, idem ||B B - B||_F, rho <B, M> (Fraction), lam_err |rho - mu|, resid ||M B - rho B||_max /
    max(||M||_max, 1), proj <B, P> in doubles)."""
    import math
    D = M.shape[0]
    ZB, sb = to_int(B)
    ZM, sm = to_int(M)
    ob = 1 << sb
    tr = abs(Fraction(sum(ZB[i][i] for i in range(D)) - ob, ob))
    sq = 0
    for i in range(D):
        for j in range(D):
            t = sum(ZB[i][t] * ZB[t][j] for t in range(D)) - ZB[i][j] * ob
            sq += t * t
    idem = math.sqrt(float(Fraction(sq, ob ** 4)))
    rho = Fraction(sum(ZB[i][j] * ZM[i][j] for i in range(D) for j in range(D)), 1 << (sb + sm))
    # M B - rho B over the common denominator 2^(sb + sm) den(rho)
    rn, rd = rho.numerator, rho.denominator
    worst = 0
    for i in range(D):
        for j in range(D):
            t = sum(ZM[i][t] * ZB[t][j] for t in range(D)) * rd - rn * ZB[i][j] * (1 << sm)
            worst = max(worst, abs(t))
    resid = float(Fraction(worst, rd << (sb + sm))) / max(float(np.abs(M).max()), 1.0)
    out = dict(trace=float(tr), idem=idem, rho=rho, lam_err=float(abs(rho - mu)), resid=resid)
    if P is not None:
        out["proj"] = float((np.asarray(B) * P).sum())
    return out


def vector_residual(M, v):
    """||M v - rho(v) v||_inf / max(||M||_max, 1) about the vector's own Rayleigh quotient, exactly"""
    D = M.shape[0]
    ZM, sm = to_int(M)
    Zv, sv = to_int(np.asarray(v, dtype=np.float64).reshape(1, D))
    z = Zv[0]
    Mv = [sum(ZM[i][j] * z[j] for j in range(D)) for i in range(D)]          # over 2^(sm + sv)
    vv = sum(t * t for t in z)                                                # over 2^(2 sv)
    vMv = sum(z[i] * Mv[i] for i in range(D))                                 # over 2^(sm + 2 sv)
    worst = max(abs(Mv[i] * vv - vMv * z[i]) for i in range(D))               # (M v - rho v) vv over 2^(sm + 3 sv)
    r = Fraction(worst, vv << (sm + sv))
    return float(r) / max(float(np.abs(M).max()), 1.0)


# ------------------------------------------------------------------------------------------------------------ family A
GAPS_A = [Fraction(0)] + [Fraction(1, 1 << e) for e in (52, 44, 36, 34, 33, 30, 20, 10)]
LAM0_A = [Fraction(-1, 4), Fraction(-1, 1 << 20), Fraction(-1, 1 << 40), Fraction(0), Fraction(1, 8)]
TRIPLE_GAPS_A = [Fraction(0)] + [Fraction(1, 1 << e) for e in (52, 44, 34, 33, 30)]
_REST_A = [Fraction(1, 4), Fraction(3, 8), Fraction(1, 2), Fraction(5, 8), Fraction(3, 4)]


def _reflector(D, rng, ones):
    """I - 2 u u^T / (u^T u) with `ones` entries +-1; ones = 5 stands for (2, 1, 1, 1, 1) up to signs and places, u^T u = 8"""
    u = [0] * D
    for n, i in enumerate(rng.choice(D, ones, replace=False)):
        u[int(i)] = int(rng.choice([-1, 1])) * (2 if ones == 5 and n == 0 else 1)
    uu = sum(t * t for t in u)
    assert uu & (uu - 1) == 0
    return [[Fraction(int(i == j)) - Fraction(2 * u[i] * u[j], uu) for j in range(D)] for i in range(D)]


def family_a_draw(D, lam0, gap, fold, rng):
    """one draw -> (M float64, spectrum Fractions, Q float64) or None when the draw is rejected"""
    count = int(rng.integers(2, 4))
    pool = [2, 4, 5] if D >= 5 else [2, 4]
    kinds = [int(rng.choice(pool[1:]))] + [int(rng.choice(pool)) for _ in range(count - 1)]
    Q = _reflector(D, rng, kinds[0])
    for ones in kinds[1:]:
        Q = fmatmul(Q, _reflector(D, rng, ones))
    perm = [int(p) for p in rng.permutation(D)]
    sign = [int(s) for s in rng.choice([-1, 1], D)]
    Q = [[Q[i][perm[j]] * sign[j] for j in range(D)] for i in range(D)]
    if all(abs(q) in (0, 1) for row in Q for q in row):
        return None                                   # a signed permutation: M would be diagonal
    lam = [lam0 + gap * j for j in range(fold)]
    rest = [_REST_A[int(i)] for i in rng.choice(len(_REST_A), D - 1 - fold, replace=False)]
    lam += rest
    q0 = Q[0][D - 1]
    if q0 == 0:
        return None
    big = (1 - sum(Q[0][j] ** 2 * lam[j] for j in range(D - 1))) / q0 ** 2
    if big < 1 or not representable(big):
        return None
    lam.append(big)
    M = [[sum(Q[i][t] * Q[j][t] * lam[t] for t in range(D)) for j in range(D)] for i in range(D)]
    if not all(representable(m) for row in M for m in row):
        return None
    return np.array([[float(m) for m in row] for row in M]), lam, np.array([[float(q) for q in row] for row in Q])


def _specs_a(D):
    specs = [(l0, g, 2) for g in GAPS_A for l0 in LAM0_A]
    if D >= 4:
        specs += [(l0, g, 3) for g in TRIPLE_GAPS_A for l0 in LAM0_A[:3]] + [(Fraction(0), Fraction(0), 3)]
    return specs[:PER_FAMILY]


def family_a(k, seed=0, tries=300):
    D = k + 1
    if D < 4:
        return []
    out = []
    for n, (lam0, gap, fold) in enumerate(_specs_a(D)):
        rng = np.random.default_rng([seed, k, n])
        for _ in range(tries):
            got = family_a_draw(D, lam0, gap, fold, rng)
            if got is not None:
                M, lam, Q = got
                tag = "A k%d lam0 %s gap %s x%d" % (k, lam0, ("2^-%d" % (gap.denominator.bit_length() - 1)) if gap else "0", fold)
                out.append(Case(k, "A", tag, M, lam, Q))
                break
    return out            # (a prescription without an exact draw is left out: tests/test_spectra_cases_cpu.py says which must be there)


# ------------------------------------------------------------------------------------------------------------ mpmath truth
def mp_truth(M):
    """-> (ascending Fractions, float64 eigenvector columns) of the symmetric matrix of doubles M, mpmath.eigsy at 60 digits"""
    import mpmath
    with mpmath.workdps(60):
        E, Q = mpmath.eigsy(mpmath.matrix(M.tolist()))
        D = M.shape[0]
        lam = [Fraction(int(mpmath.nint(mpmath.ldexp(E[j], _SHIFT))), 1 << _SHIFT) for j in range(D)]
        V = np.array([[float(Q[i, j]) for j in range(D)] for i in range(D)])
    return lam, V


# ------------------------------------------------------------------------------------------------------------ family B
NOMINAL_GAPS_B = [10.0 ** -e for e in range(16, 2, -1)]


def _haar(D, rng):
    Z = rng.normal(size=(D, D))
    Q, R = np.linalg.qr(Z)
    return Q * np.sign(np.diag(R))


def family_b(k, seed=0):
    D = k + 1
    rng = np.random.default_rng([seed, k, 66])
    folds = (2, 3) if D >= 4 else (2,)
    # (a three-fold cluster spaced by 1e-6 straddles TAU: its lambda_min has neither a qualifying cluster nor one of its own)
    specs = [(g, f) for f in folds for g in NOMINAL_GAPS_B if not (f == 3 and g == 1e-6)]
    lam0s = [-0.3, -0.05, -1e-3, -1e-8, 0.0, 0.05]
    out = []
    n = 0
    while len(out) < PER_FAMILY:
        g, fold = specs[n % len(specs)]
        lam0 = lam0s[(n // len(specs) + n) % len(lam0s)]
        n += 1
        for _ in range(200):
            ev = [lam0 + g * j for j in range(fold)]
            rest = np.sort(rng.choice(np.arange(0.15, 0.95, 0.1), D - 1 - fold, replace=False) + rng.uniform(-0.02, 0.02, D - 1 - fold))
            ev = np.array(ev + rest.tolist() + [float(rng.uniform(1.5, 3.0))])
            Q = _haar(D, rng)
            M = (Q * ev) @ Q.T
            M = 0.5 * (M + M.T)
            if not 0.25 <= M[0, 0] <= 4.0:
                continue
            M = M / M[0, 0]
            M = 0.5 * (M + M.T)
            M[0, 0] = 1.0
            lam, V = mp_truth(M)
            c = Case(k, "B", "B k%d lam0 %g nominal gap %.0e x%d" % (k, lam0, g, fold), M, lam, V)
            if c.qualifies[0] or (c.sep[0] > TAU and len(c.members[0]) == 1):
                out.append(c)
                break
        else:
            raise AssertionError("no family B matrix for gap %g" % g)
    return out


# ------------------------------------------------------------------------------------------------------------ family C
def family_c(k, seed=0):
    """structured vertices with LP noise; three quarters of them (k >= 3) with a nearly multiple lambda_min by LAPACK's account"""
    D = k + 1
    rng = np.random.default_rng([seed, k, 67])
    iu = np.triu_indices(k)
    out, seen = [], set()
    want_clustered = 0 if k == 2 else (3 * PER_FAMILY) // 4
    n_cl = 0
    for _ in range(200000):
        if len(out) == PER_FAMILY:
            break
        X = rng.choice([0.0, 0.5], size=iu[0].shape[0])
        x = np.full(k, 0.5)
        X = X + rng.integers(-8, 9, size=X.shape[0]) * 2.0 ** -50
        x = x + rng.integers(-8, 9, size=k) * 2.0 ** -50
        M = np.zeros((D, D))
        M[0, 0] = 1.0
        M[0, 1:] = M[1:, 0] = x
        M[iu[0] + 1, iu[1] + 1] = X
        M[iu[1] + 1, iu[0] + 1] = X
        w = np.linalg.eigvalsh(M)
        clustered = bool(w[1] - w[0] <= 1e-9)
        if k > 2 and (n_cl >= want_clustered if clustered else len(out) - n_cl >= PER_FAMILY - want_clustered):
            continue
        d = np.diff(w)
        if ((d > 1e-7) & (d < 2e-3)).any() or M.tobytes() in seen:
            continue
        seen.add(M.tobytes())
        lam, V = mp_truth(M)
        c = Case(k, "C", "C k%d #%d" % (k, len(out)), M, lam, V)
        if all(c.qualifies):
            out.append(c)
            n_cl += len(c.members[0]) > 1
    assert len(out) == PER_FAMILY, (k, len(out))
    return out


# ------------------------------------------------------------------------------------------------------------ all of it
@functools.lru_cache(maxsize=None)
def cases(k):
    """the matrices of size k, family by family (A, B, C)"""
    return tuple(family_a(k) + family_b(k) + family_c(k))


def lapack_yardstick(case):
    """LAPACK's own error on a case -> (|eigvalsh(M, 'U')[0] - mu_0| / s and the residual of column 0 of eigh, both in exact
    arithmetic; 1 - <v v^T, P> of that column; the largest <B_r, B_s> = (v_r . v_s)^2 of two columns of eigh)"""
    w = np.linalg.eigvalsh(case.M, "U")
    _, V = np.linalg.eigh(case.M)
    G = (V.T @ V - np.eye(V.shape[0])) ** 2
    return (float(abs(frac(w[0]) - case.spectrum[0])) / case.s, vector_residual(case.M, V[:, 0]),
            1.0 - float(V[:, 0] @ case.proj[0] @ V[:, 0]) / float(V[:, 0] @ V[:, 0]), float(G.max()))


@functools.lru_cache(maxsize=None)
def lapack_maxima():
    """-> {(family, k): (lambda error / s, residual, 1 - <B, P>, orthogonality defect)} and {family: the maxima over k}: the first
    two are the yardstick of the device bounds"""
    per, fam = {}, {}
    for k in KS:
        for c in cases(k):
            y = lapack_yardstick(c)
            for key, d in (((c.family, k), per), (c.family, fam)):
                d[key] = tuple(max(a, b) for a, b in zip(d.get(key, (0.0,) * 4), y))
    return per, fam


# ------------------------------------------------------------------------------------------------------------ packing
@functools.lru_cache(maxsize=None)
def packed(k):
    """-> dict(n, L, point [X packed | x], Q_arr, cases, orders = {"sorted" | "mixed": dict(S int32 [N, 5], ks int32 [N], case int64
    [N]: index into cases or -1 for a generic candidate, copy int64 [N]: 0 / 1 for the two copies of a matrix)}, var0 int64 [cases, 2]:
    first variable of either copy)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sdpcutsel_via_nn_amd import harness
    cs = cases(k)
    C = len(cs)
    n = GENERIC_VARS + 2 * C * k
    L = n * (n + 1) // 2
    rng = np.random.default_rng([k, 68])
    point = np.zeros(L + n)
    g = harness.random_mccormick_point(GENERIC_VARS, rng)
    gi = np.triu_indices(GENERIC_VARS)
    point[n * gi[0] - gi[0] * (gi[0] + 1) // 2 + gi[1]] = g[:gi[0].shape[0]]
    point[L:L + GENERIC_VARS] = g[gi[0].shape[0]:]
    var0 = np.zeros((C, 2), dtype=np.int64)
    ia, ib = np.triu_indices(k)
    for c, case in enumerate(cs):
        for r in range(2):
            v0 = GENERIC_VARS + (2 * c + r) * k
            var0[c, r] = v0
            a, b = v0 + ia, v0 + ib
            point[n * a - a * (a + 1) // 2 + b] = case.X
            point[L + v0:L + v0 + k] = case.x
    Q_arr = np.round(rng.normal(size=L) * 20) * (rng.uniform(size=L) < 0.3)

    def special(c, r):
        return [int(var0[c, r]) + i for i in range(k)], c, r

    def generic():
        return sorted(int(v) for v in rng.choice(GENERIC_VARS, k, replace=False)), -1, 0
    sorted_list = [special(c, r) for c in range(C) for r in range(2)]
    mixed = []
    slots = [(c, 0) for c in rng.permutation(C)] + [(c, 1) for c in rng.permutation(C)]
    for c, r in slots:
        at = int(rng.integers(0, 4))
        four = [generic() for _ in range(3)]
        four.insert(at, special(int(c), r))
        mixed += four
    orders = {}
    for name, lst in (("sorted", sorted_list), ("mixed", mixed)):
        S = np.full((len(lst), 5), -1, dtype=np.int32)
        for i, (s, _, _) in enumerate(lst):
            S[i, :k] = s
        orders[name] = dict(S=S, ks=np.full(len(lst), k, dtype=np.int32), case=np.array([c for _, c, _ in lst], dtype=np.int64),
                            copy=np.array([r for _, _, r in lst], dtype=np.int64))
    return dict(n=n, L=L, point=point, Q_arr=Q_arr, cases=cs, orders=orders, var0=var0)
