"""The band rule of SDPCUT_OPT_EXACT_HEAD (csrc/exact_band.h), compiled alone with the host compiler: the band contains the exact
head for every (approximate, exact) score pair within the asserted error bound, the retry / give-up decisions at the capacity
edges, zero-band membership at the bound and one ulp beyond it.  CPU only: the header is plain C++."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

EXACT, RETRY, GIVE_UP = 0, 1, 2
LDSK = 8192

WRAPPER = r"""
#include "exact_band.h"
extern "C" {
double w_eps(double obj, double me) { return eb_eps(obj, me); }
double w_bound(double q) { return eb_max_elem_bound(q); }
int w_zero(double obj, double me) { return eb_zero_band(obj, me); }
long w_margin(long cap) { return eb_margin(cap); }
long w_first(long n, long cap) { return eb_first_band(n, cap); }
int w_head_ok(long n, long cap) { return eb_head_ok(n, cap); }
double w_delta(double a, double b, double me, int bigm) { return eb_delta(a, b, me, bigm != 0); }
int w_holds(double a, double b, double me, int bigm) { return eb_band_holds(a, b, me, bigm != 0); }
int w_decide(long n, long cls, long band, int holds) { return eb_decide(n, cls, band, holds != 0); }
long w_ldsk() { return EB_LDSK; }
long w_zbmax() { return EB_ZB_MAX; }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("exact_band")
    src = d / "band.cpp"
    src.write_text(WRAPPER)
    so = d / "band.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    L = ctypes.CDLL(str(so))
    D, I, G = ctypes.c_double, ctypes.c_int, ctypes.c_long
    for name, res, args in (("w_eps", D, [D, D]), ("w_bound", D, [D]), ("w_zero", I, [D, D]), ("w_margin", G, [G]), ("w_first", G, [G, G]),
                            ("w_head_ok", I, [G, G]), ("w_delta", D, [D, D, D, I]), ("w_holds", I, [D, D, D, I]),
                            ("w_decide", I, [G, G, G, I]), ("w_ldsk", G, []), ("w_zbmax", G, [])):
        getattr(L, name).restype = res
        getattr(L, name).argtypes = args
    return L


def test_error_bound_and_margins(lib):
    assert lib.w_ldsk() == LDSK and lib.w_zbmax() == 1024
    assert lib.w_eps(2.0, 100.0) == 1e-9 * 2.0
    assert lib.w_eps(-0.05, 100.0) == 1e-9 * (1e-3 * 100.0)
    assert lib.w_bound(0.0) == 1.0 and lib.w_bound(0.1) == 1.0 and lib.w_bound(100.0) == 500.0      # max_elem = k max|Q| or 1
    assert lib.w_margin(100) == 256 and lib.w_margin(2048) == 256 and lib.w_margin(5000) == 625
    assert lib.w_first(10 ** 6, 5000) == 5625 and lib.w_first(5100, 5000) == 5100 and lib.w_first(1051, 105) == 361
    # head limit: the first band must fit the merge
    assert lib.w_head_ok(10 ** 6, 5000) and lib.w_head_ok(10 ** 6, 7282) and not lib.w_head_ok(10 ** 6, 7283)
    assert not lib.w_head_ok(10 ** 6, 9000) and lib.w_head_ok(8192, 8192) and not lib.w_head_ok(8193, 8192)


@pytest.mark.parametrize("bigm", [0, 1])
@pytest.mark.parametrize("scale,me", [(1.0, 500.0), (1e-3, 5.0), (300.0, 500.0), (1e-4, 1.0)])
def test_band_contains_the_exact_head(lib, bigm, scale, me):
    """(approximate, exact) pairs with |delta| <= eps: whenever the rule says the band holds, the exact top-cap lies inside the
    approximate top-band; spacings around the bound so that both verdicts occur"""
    rng = np.random.default_rng(5 + bigm)
    seen = set()
    for trial in range(300):
        n, cap = 400, 40
        band = cap + int(rng.integers(1, 60))
        exact = rng.standard_normal(n) * scale
        if trial % 3 == 0:      # a dense cluster around the threshold: spacings of the order of eps
            thr = np.sort(exact)[::-1][cap]
            cl = rng.choice(n, 120, replace=False)
            exact[cl] = thr + rng.standard_normal(120) * 4.0 * lib.w_eps(thr + (1000.0 if bigm else 0.0), me)
        eps = np.array([lib.w_eps(v, me) for v in exact])
        approx = exact + rng.uniform(-1.0, 1.0, n) * eps
        if bigm:      # keys of the every-entry-visited regime: obj + BIG_M, rounded (monotone)
            k_exact, k_approx = exact + 1000.0, approx + 1000.0
        else:
            k_exact, k_approx = exact, approx
        oa = np.argsort(-k_approx, kind="stable")
        oe = np.argsort(-k_exact, kind="stable")
        holds = lib.w_holds(float(k_approx[oa[cap - 1]]), float(k_approx[oa[band - 1]]), me, bigm)
        seen.add(bool(holds))
        if holds:
            assert set(oe[:cap].tolist()) <= set(oa[:band].tolist()), (trial, band)
            # ... and ranking the band by the exact keys gives the exact head, ties by index
            b = np.sort(oa[:band])
            assert np.array_equal(b[np.argsort(-k_exact[b], kind="stable")][:cap], oe[:cap])
    assert seen == {True, False}


def test_band_rule_needs_a_strict_gap(lib):
    me = 500.0
    assert not lib.w_holds(1.0, 1.0, me, 0)                       # equal keys at both ends: never proven
    d = lib.w_delta(1.0, 1.0, me, 0)
    assert d >= 2.0 * lib.w_eps(1.0, me)
    assert not lib.w_holds(1.0, 1.0 - d, me, 0) and lib.w_holds(1.0, 1.0 - 1.01 * d, me, 0)
    assert lib.w_delta(1.0, 0.5, me, 1) >= 2.0 * lib.w_eps(1001.0, me) + 2.0 ** -42      # + BIG_M and the rounding of the sum


def test_retry_and_give_up_at_the_capacity_edges(lib):
    n = 10 ** 6
    assert lib.w_decide(n, n, 5625, 1) == EXACT
    assert lib.w_decide(n, n, 5625, 0) == RETRY                   # first band failed: the widest one
    assert lib.w_decide(n, n, LDSK, 0) == GIVE_UP                  # the widest failed too
    assert lib.w_decide(n, n, LDSK - 1, 0) == RETRY
    assert lib.w_decide(n, n, LDSK, 1) == EXACT
    assert lib.w_decide(n, 5625, 5625, 0) == EXACT                 # the whole class was re-scored: nothing to prove
    assert lib.w_decide(n, 5626, 5625, 0) == RETRY
    assert lib.w_decide(6000, 6000, 5625, 0) == RETRY and lib.w_decide(6000, 6000, 6000, 0) == EXACT
    assert lib.w_decide(361, 361, 361, 0) == EXACT                 # short list: band = list
    assert lib.w_decide(20000, 20000, 356, 0) == RETRY and lib.w_decide(20000, 20000, LDSK, 0) == GIVE_UP


def test_zero_band_membership_at_the_bound(lib):
    me = 500.0
    e = lib.w_eps(0.0, me)
    assert e == 1e-9 * (1e-3 * me)
    up = float(np.nextafter(e, np.inf))
    for s in (1.0, -1.0):
        assert lib.w_zero(s * e, me) and not lib.w_zero(s * up, me)
        assert lib.w_zero(s * 0.0, me) and lib.w_zero(s * e / 3, me)
    assert not lib.w_zero(1.0, me) and not lib.w_zero(-1e-9, me)
