"""The filtered batched round (sdpcut_round_csr_points_diverse, sdpcut_efficacy_points), the parts that need no device: the route
function of csrc/batch_route.h compiled alone, the premises of the GPU cases (tests/diverse_points_cases.py) by the numpy twins,
and the argument refusals that are decided before anything touches a device.

One premise is wanted of every case and strategy 1 cannot have it: skipped_nonviolated > 0.  The ranking of strategy 1 lists the
violated candidates only, and the row of a violated candidate is not zero (a unit eigenvector of a negative eigenvalue of
[[1, x^T], [x, X]] has a non-zero component beyond the first), so every pool entry of strategy 1 is eligible and the count is 0 at
every point.  test_premises asserts exactly that for strategy 1 and the > 0 for strategies 2, 4 and 6."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import diverse_points_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
NAMES = ("sdpcut_efficacy_points", "sdpcut_round_csr_points_diverse")
FAST, LOOP = 1, 2

WRAPPER = r"""
#include "batch_route.h"
extern "C" {
// in: N, sel, pool, strat, exact_head, shard, nb_vars, n_points -> out: batch_route_diverse, batch_route_diverse_boxed
void diverse_rows(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + 8 * i;
        out[2 * i] = batch_route_diverse(a[0], a[1], a[2], (int)a[3], a[4] != 0, a[5] != 0);
        out[2 * i + 1] = batch_route_diverse_boxed(a[0], a[1], a[2], (int)a[3], a[4] != 0, a[5] != 0, a[6], a[7]);
    }
}
int mode_of(int strat) { return batch_mode(strat); }
int mode_diverse_of(int strat) { return batch_mode_diverse(strat); }
int route_of(int64_t N, int64_t cap, int strat, int exact, int shard) { return batch_route(N, cap, strat, exact != 0, shard != 0); }
int route_boxed_of(int64_t N, int64_t cap, int strat, int exact, int shard, int64_t nv, int64_t P) { return batch_route_boxed(N, cap, strat, exact != 0, shard != 0, nv, P); }
int64_t box_budget(void) { return BATCH_BOX_BUDGET_BYTES; }
int64_t box_bytes(int64_t nv, int64_t P) { return batch_box_table_bytes(nv, P); }
int max_pool(void) { return BATCH_DIVERSE_MAX_POOL; }
}
"""


@pytest.fixture(scope="module")
def route_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_route_diverse")
    src, so = d / "wrap.cpp", d / "wrap.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    i64p = ctypes.POINTER(ctypes.c_int64)
    i64 = ctypes.c_int64
    lib.diverse_rows.argtypes = [ctypes.c_long, i64p, i64p]
    lib.route_of.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.route_boxed_of.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, i64, i64]
    lib.box_budget.restype = lib.box_bytes.restype = i64
    lib.box_bytes.argtypes = [i64, i64]
    return lib


def _routes(lib, rows):
    a = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.zeros((a.shape[0], 2), dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.diverse_rows(a.shape[0], a.ctypes.data_as(i64p), out.ctypes.data_as(i64p))
    return out[:, 0], out[:, 1]


# ------------------------------------------------------------------------------------------ 1. ABI
def test_abi_carries_the_entry_points():
    from sdpcutsel_via_nn_amd import _capi, build
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    declared = set(re.findall(r"^int\s*(sdpcut_\w+)\s*\(", hdr, flags=re.M))
    c = ctypes
    dp = c.POINTER(c.c_double)
    for name in NAMES:
        assert name in declared and name in _capi.SIGNATURES, name
        assert _capi.SIGNATURES[name][:4] == [c.c_void_p, c.c_int32, dp, c.c_int64]
    assert _capi.SIGNATURES[NAMES[0]][4:] == [dp, dp, dp]
    assert _capi.SIGNATURES[NAMES[1]][4:] == [dp, dp, c.c_int64, c.c_int, c.c_int64, c.c_int64, c.c_double, c.POINTER(_capi.RoundCsr),
                                              c.POINTER(_capi.DiverseInfo)]
    enums = " ".join(re.findall(r"enum\s*\{([^}]*)\}", hdr))
    stats = dict((k, int(v)) for k, v in re.findall(r"(SDPCUT_STAT_\w+)\s*=\s*(-?\d+)", enums))
    assert stats["SDPCUT_STAT_DIVERSE_POINTS_FAST"] == _capi.STAT_DIVERSE_POINTS_FAST == 17
    assert stats["SDPCUT_STAT_INJECTED"] == _capi.STAT_INJECTED == 18      # (the test-only statistic of SDPCUT_OPT_INJECT_GIVEUP came after it)
    assert sorted(stats.values()) == list(range(1, 19))      # new codes, nothing renumbered
    assert (stats["SDPCUT_STAT_POINTS_REDONE"], stats["SDPCUT_STAT_NN_EVALUATED"]) == (13, 16)
    so = build.build(verbose=False)
    exported = set(ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if ln.strip())
    for name in NAMES:
        assert name in exported, name


# ------------------------------------------------------------------------------------------ 2. routes
NS = (1, 64, 512, 513, 4096, 4097)
POOLS = (1, 64, 512, 513)
STRATS = (1, 2, 4, 6, 0, 3, 5)


def test_route_diverse(route_lib):
    """FAST exactly when: a served strategy, N <= 4096, pool = min(pool_size, N) in 1 .. 512, exact head off, no shard -- and, for
    strategy 4, min(sel, N) == pool (its quota stays sel: with sel < pool the one-workgroup selection is another list).  Boxed: plus
    the box tables within the budget for the strategies that read them (2 and 4)."""
    assert route_lib.max_pool() == 512
    budget = route_lib.box_budget()
    assert budget == 256 << 20
    rows = []
    for N, pool, strat, exact, shard in itertools.product(NS, POOLS, STRATS, (0, 1), (0, 1)):
        for sel in sorted({1, max(1, pool // 2), pool}):
            for nv, P in ((20, 8), (125, 256), (400, 256)):
                rows.append((N, sel, pool, strat, exact, shard, nv, P))
    got, got_boxed = _routes(route_lib, rows)
    a = np.array(rows)
    N, sel, pool, strat, exact, shard, nv, P = a.T
    p_eff, s_eff = np.minimum(pool, N), np.minimum(sel, N)
    served = np.isin(strat, (1, 2, 4, 6))
    want = served & (N <= 4096) & (p_eff >= 1) & (p_eff <= 512) & (exact == 0) & (shard == 0) & ((strat != 4) | (s_eff >= p_eff))
    assert np.array_equal(got, np.where(want, FAST, LOOP))
    fits = np.array([route_lib.box_bytes(int(v), int(q)) <= budget for v, q in zip(nv, P)])
    assert fits.any() and not fits.all()
    want_boxed = want & (fits | np.isin(strat, (1, 6)))
    assert np.array_equal(got_boxed, np.where(want_boxed, FAST, LOOP))
    for s in (1, 2, 4, 6):
        assert ((got == FAST) & (strat == s)).any() and ((got == LOOP) & (strat == s)).any()
    assert ((got == LOOP) & (strat == 4) & (sel < pool) & (N <= 4096) & (pool <= 512) & (exact == 0) & (shard == 0) & (sel < N)).any()


def test_existing_routes_keep_refusing_strategy_6(route_lib):
    assert [route_lib.mode_of(s) for s in (1, 2, 4, 6, 0, 3, 5, -1)] == [1, 2, 5, 0, 0, 0, 0, 0]
    assert [route_lib.mode_diverse_of(s) for s in (1, 2, 4, 6, 0, 3, 5, -1)] == [1, 2, 5, 2, 0, 0, 0, 0]
    for N, cap in itertools.product(NS, POOLS):
        for exact, shard in itertools.product((0, 1), (0, 1)):
            assert route_lib.route_of(N, min(cap, N), 6, exact, shard) == LOOP
            assert route_lib.route_boxed_of(N, min(cap, N), 6, exact, shard, 20, 8) == LOOP
    assert route_lib.route_of(1051, 105, 2, 0, 0) == FAST and route_lib.route_boxed_of(1051, 105, 4, 0, 0, 20, 8) == FAST


# ------------------------------------------------------------------------------------------ 3. premises of the GPU cases
@pytest.fixture(scope="module")
def walks():
    """{case: [info of the walk at each of the eight points]} at max_parallel = 0.5, by the twins"""
    return {case: [dc.walk_twin(case[0], case[1], case[2], case[3], dc.points(case[0])[p]) for p in range(dc.N_POINTS)]
            for case in dc.CASES}


def test_lists_and_points():
    for name, (_, _, N) in dc.LISTS.items():
        n, Q, S, ks, obj = dc.load(name)
        assert S.shape == (N, 5) and obj.shape == (n * (n + 1) // 2 + n,)
        pts = dc.points(name)
        L = n * (n + 1) // 2
        iu = np.triu_indices(n)
        viol = []
        for vv in pts:      # McCormick-feasible
            x, X = vv[L:], vv[:L]
            assert np.all(X <= np.minimum(x[iu[0]], x[iu[1]]) + 1e-15) and np.all(X >= np.maximum(0.0, x[iu[0]] + x[iu[1]] - 1.0) - 1e-15)
            viol.append(int((dc.rows_twin(n, S, ks, vv)[0] < dc.NEG).sum()))
        assert max(viol) > N // 2 and min(viol) == 0 and 0 < sorted(viol)[2] < 129      # many, none, and fewer than a pool


def test_premises(walks):
    assert {c[1] for c in dc.CASES} == {1, 2, 4, 6} and {c[0] for c in dc.CASES} == set(dc.LISTS)
    for case, infos in walks.items():
        assert all(i["closest"] > 1e-9 for i in infos), case      # no pair at the threshold: device and twin decide alike
        assert max(i["rejected_parallel"] for i in infos) > 0, case
        if case[1] == 1:
            assert all(i["skipped_nonviolated"] == 0 for i in infos), case      # (see the module's docstring)
        else:
            assert max(i["skipped_nonviolated"] for i in infos) > 0, case
        for i in infos:
            assert i["examined"] == i["accepted"] + i["skipped_nonviolated"] + i["rejected_parallel"]


def test_walks_end_at_a_block_end_and_inside_a_block(walks):
    at_end = [(c, p) for c, infos in walks.items() for p, i in enumerate(infos)
              if i["accepted"] == c[2] and i["examined"] % 64 == 0 and i["examined"] < i["pool"]]
    inside = [(c, p) for c, infos in walks.items() for p, i in enumerate(infos)
              if i["accepted"] == c[2] and i["examined"] % 64 != 0 and i["examined"] < i["pool"]]
    assert at_end and inside, (at_end, inside)
    assert (("spar040", 1, 20, 65), 1) in at_end      # examined = 64: the quota fills with the last entry of the first block


# ------------------------------------------------------------------------------------------ 4. refusals without a device
def test_refusals_without_a_device():
    from sdpcutsel_via_nn_amd import _capi, build
    build.build(verbose=False)
    lib = _capi.load_library()
    pts = np.zeros((2, 9))
    dp = pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out, info = (_capi.RoundCsr * 2)(), (_capi.DiverseInfo * 2)()
    assert lib.sdpcut_efficacy_points(None, 2, dp, 9, dp, None, None) == -1
    assert lib.sdpcut_round_csr_points_diverse(None, 2, dp, 9, None, None, 0, 1, 1, 1, 0.5, out, info) == -1
    sc = _capi.Scorer.__new__(_capi.Scorer)      # no handle: the argument checks come first
    sc.nb_vars, sc.N = 3, 4
    good = np.zeros((2, 9))
    for bad in (np.zeros(9), np.zeros((2, 8)), np.zeros((0, 9)), np.zeros((257, 9))):
        with pytest.raises(ValueError):
            sc.round_csr_points_diverse(bad, 1, 1, 0.5)
        with pytest.raises(ValueError):
            sc.efficacy_points(bad)
    for kw in (dict(strat=0), dict(strat=3), dict(strat=5), dict(max_parallel=-0.01), dict(max_parallel=1.01), dict(max_parallel=float("nan")),
               dict(sel_size=0), dict(sel_size=10, pool_size=9), dict(pool_size=_capi.DIVERSE_MAX_POOL + 1)):
        args = dict(strat=1, sel_size=2, max_parallel=0.5, pool_size=None)
        args.update(kw)
        with pytest.raises(ValueError):
            sc.round_csr_points_diverse(good, args["strat"], args["sel_size"], args["max_parallel"], pool_size=args["pool_size"])
    bx = np.zeros((2, 2, 3))
    bx[:, 1] = 1.0
    bx[1, 1, 2] = bx[1, 0, 2] + 2.0 ** -11      # narrower than 2^-10
    with pytest.raises(ValueError, match="point 1"):
        sc.round_csr_points_diverse(good, 2, 1, 0.5, boxes=bx)
    with pytest.raises(ValueError):
        sc.round_csr_points_diverse(good, 2, 1, 0.5, boxes=bx[:1])
    sc._h = None
