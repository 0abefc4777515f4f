"""The work split of the skipping score kernel (csrc/score_plan.h: score_plan_skip, score_skip_applies) against its restatement
(tests/skip_plan.py), and score_plan itself at the inputs tests/test_score_plan.py pins: unchanged by the new rule next to it.
CPU only: the header is plain C++ and is compiled alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import skip_plan
import test_score_plan as parent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

SKIP_OUT = ("grid", "strip", "rr_end", "tail_nhi", "tail_hi", "tail_lo", "pf_mloc", "spread")

WRAPPER = r"""
#include "score_plan.h"
extern "C" void skip_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + 6 * i;
        int64_t *o = out + 8 * i;
        const ScorePlan p = score_plan_skip(a[0], (int)a[1], (int)a[2], a[3], a[4], a[5] != 0);
        o[0] = p.grid; o[1] = p.strip; o[2] = p.rr_end; o[3] = p.tail_nhi; o[4] = p.tail_hi; o[5] = p.tail_lo; o[6] = p.pf_mloc; o[7] = p.spread;
    }
}
extern "C" void applies_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) out[i] = score_skip_applies(in[4 * i], (int)in[4 * i + 1], (int)in[4 * i + 2], (int)in[4 * i + 3]);
}
extern "C" void plan_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + 6 * i;
        int64_t *o = out + 8 * i;
        const ScorePlan p = score_plan(a[0], (int)a[1], (int)a[2], a[3], a[4], a[5] != 0);
        o[0] = p.grid; o[1] = p.strip; o[2] = p.rr_end; o[3] = p.tail_nhi; o[4] = p.tail_hi; o[5] = p.tail_lo; o[6] = p.pf_mloc; o[7] = p.spread;
    }
}
extern "C" int constants(int *out) { out[0] = SDPCUT_SKIP_BLOCKS_PER_CU; out[1] = SDPCUT_SKIP_FORCED_STRIPS; out[2] = SDPCUT_SKIP_KMASK; return 3; }
"""

P64 = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_plan_skip")
    src = d / "skip.cpp"
    src.write_text(WRAPPER)
    so = d / "skip.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _call(fn, cases, ncols_out):
    cases = np.ascontiguousarray(cases, dtype=np.int64)
    out = np.full((cases.shape[0], ncols_out), -99, dtype=np.int64)
    fn(ctypes.c_long(cases.shape[0]), cases.ctypes.data_as(P64), out.ctypes.data_as(P64))
    return out


def _sizes():
    ns = list(range(1, 301))
    for n_cu in (1, 8, 256):
        rnd = n_cu * skip_plan.BLOCKS_PER_CU * 4 * 64      # one round of the full launch
        for R in (1, 2, 7, 15):
            ns += [R * rnd + d for d in (-65, -17, -16, -15, -1, 0, 1, 15, 16, 17, 63, 64, 65)]
            ns += [R * rnd + f * rnd // 100 for f in (3, 25, 50, 63, 90, 99)]
    ns += [4095, 4096, 4097, 12352, 65535, 65536, 65537, 65600, 10 ** 5, 524287, 10 ** 6, 1000003, 1681784, 2 * 10 ** 6]
    return sorted(set(n for n in ns if 1 <= n <= 2 * 10 ** 6))


def test_constants_match_the_restatement(lib):
    c = (ctypes.c_int * 3)()
    assert lib.constants(c) == 3
    assert (c[0], c[1]) == (skip_plan.BLOCKS_PER_CU, skip_plan.FORCED_STRIPS)
    assert c[0] in (2, 4, 8) and c[2] == 1 << 3      # the sizes that are switched on: 3-variable candidates


@pytest.mark.parametrize("n_cu", [1, 8, 256])
def test_every_candidate_exactly_once(lib, n_cu):
    ns = _sizes()
    cases = np.array([(n, n_cu, 3, n, 5000, force) for n in ns for force in (0, 1)], dtype=np.int64)
    out = _call(lib.skip_batch, cases, 8)
    split = several = 0
    for c, o in zip(cases, out):
        n, force = int(c[0]), bool(c[5])
        got = dict(zip(SKIP_OUT, (int(v) for v in o)))
        want = skip_plan.skip_plan(n, n_cu, force)
        assert {k: got[k] for k in want} == want, (n, n_cu, force, got, want)
        assert got["spread"] == 0 and got["grid"] >= 1
        seen, longest = skip_plan.visits(n, got)
        assert seen.min() == 1 and seen.max() == 1, (n, n_cu, force, got)
        assert longest <= 64
        per_wave = [len(m) for m in skip_plan.wave_strips(n, got)]
        assert min(per_wave) >= 1 or n < 64 * 4 * got["grid"]      # no wave of a launched workgroup idles, short lists apart
        if force and n >= 64 * 64:
            assert max(per_wave) >= 3, (n, got)                    # option value 2: a wave gets several strips however short the list
            several += 1
        split += got["rr_end"] < n
    assert split > 0 and several > 0


def test_fewer_longer_lived_waves_than_the_plain_plan(lib):
    """the 10^6-candidate benchmark list on 256 CUs: one resident generation, the last partial round split evenly"""
    a = _call(lib.skip_batch, [(10 ** 6, 256, 3, 10 ** 6, 5000, 0)], 8)[0]
    got = dict(zip(SKIP_OUT, (int(v) for v in a)))
    W = 256 * skip_plan.BLOCKS_PER_CU * 4
    R, rem = divmod(10 ** 6, W * 64)
    tiles = -(-rem // 16)
    assert got["grid"] == W // 4 and got["rr_end"] == R * W * 64
    assert got["tail_lo"] == tiles // W and got["tail_hi"] == tiles // W + 1
    assert got["tail_nhi"] * got["tail_hi"] + (W - got["tail_nhi"]) * got["tail_lo"] >= tiles
    assert got["pf_mloc"] == parent._mloc_restated(5000, -(-10 ** 6 // got["grid"]), 10 ** 6) > 0


def test_where_the_skipping_kernel_applies(lib):
    cases = [(n, n_cu, K, opt) for n_cu in (1, 8, 256) for K in (2, 3, 4, 5) for opt in (0, 1, 2)
             for n in (0, 1, 4096, 32 * n_cu * 8, 32 * n_cu * 8 + 1, 10 ** 6, 59000 * n_cu * skip_plan.BLOCKS_PER_CU - 1,
                       59000 * n_cu * skip_plan.BLOCKS_PER_CU)]
    out = _call(lib.applies_batch, np.array(cases, dtype=np.int64), 1)[:, 0]
    for c, o in zip(cases, out):
        assert bool(o) == skip_plan.skip_applies(*c), c
    assert out.any() and not out.all()
    # where it applies by default the plain plan cuts strips of 64 and the fine histogram stays in use
    for (n, n_cu, K, opt), o in zip(cases, out):
        if o and opt == 1:
            plain = _call(lib.plan_batch, [(n, n_cu, K, n, 5000, 1)], 8)[0]
            skip = _call(lib.skip_batch, [(n, n_cu, K, n, 5000, 0)], 8)[0]
            assert plain[1] == 64 and skip[6] > 0, (n, n_cu)


def test_score_plan_unchanged(lib):
    """score_plan at the inputs of tests/test_score_plan.py, against the restatement there"""
    cases = np.array([(n, n_cu, K, nt(n), fk, fu) for (n, n_cu) in parent.PLAN_GRID for (K, nt, fk, fu) in parent.PLAN_VARIANTS], dtype=np.int64)
    out = _call(lib.plan_batch, cases, 8)
    for c, o in zip(cases, out):
        want = parent._plan_restated(*[int(v) for v in c])
        assert dict(zip(parent.PLAN_OUT, (int(v) for v in o))) == want, c
    a = _call(lib.plan_batch, [(10 ** 6, 256, 3, 10 ** 6, 0, 0)], 8)[0]
    assert dict(zip(parent.PLAN_OUT, a)) == dict(grid=2048, strip=64, rr_end=524288, tail_nhi=5156, tail_hi=4, tail_lo=3, pf_mloc=0, spread=0)
