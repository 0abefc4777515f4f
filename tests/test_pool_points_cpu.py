"""The pool at tree nodes without a device: the numpy twin's pool_separate_points / pool_drop (sdpcutsel_via_nn_amd/cutpool.py) against
the invariant checker and against the step it restates, the layout header compiled alone, and the refusals that need no device.
The pools are tests/pool_points_cases.py."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import pool_points_cases as pc
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")


def twin(cap=8192):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    return CutPoolTwin(cap, pc.NCOLS)


def checked(tw, points, max_return, viol_tol=1e-6, states="all"):
    from sdpcutsel_via_nn_amd.cutpool import check_separation
    before = tw.pool_state()
    out = tw.pool_separate_points(points, max_return, viol_tol=viol_tol, states=states)
    after = tw.pool_state()
    assert all(np.array_equal(before[f], after[f]) for f in pc.STATE) and before["next_serial"] == after["next_serial"]
    assert check_separation(before, points, viol_tol, states, max_return, out)
    return out


# ------------------------------------------------------------------------------------------ 1. the twin against the checker
@pytest.mark.parametrize("b", range(8))
def test_byte_families(b):
    tw = twin()
    keys = pc.byte_family(b, 600)
    tw.pool_add(*pc.single_rows(keys))
    pts = np.stack([pc.zero_point()] * 2)
    for mr in (0, 1, 7, 600):
        out = checked(tw, pts, mr, viol_tol=0.0)
        want = sorted(((-k, i) for i, k in enumerate(keys)))[:mr]
        for o in out:      # the keys ARE the right-hand sides: the expected order needs no arithmetic at all
            assert o["n_violated"] == 600 and list(o["serial"]) == [i for _, i in want] and list(o["key"]) == [-k for k, _ in want]


def test_tie_runs_inf_keys_and_thresholds():
    tw = twin()
    keys = pc.tie_runs()
    tw.pool_add(*pc.single_rows(keys))
    z = pc.zero_point()[None, :]
    o = checked(tw, z, 7)[0]
    assert list(o["key"]) == [3.0] * 3 + [2.0] * 4 and list(o["serial"]) == [2, 7, 13, 0, 3, 4, 6]
    o = checked(tw, z, 4096)[0]
    assert o["n_violated"] == 18 and list(o["serial"][-5:]) == [1, 5, 10, 14, 17]
    tw = twin()
    blk, nv = pc.inf_keys()
    tw.pool_add(*blk)
    o = checked(tw, z, 4096, viol_tol=0.0)[0]
    assert o["n_violated"] == nv and list(o["serial"]) == [1, 5, 3, 0] and list(o["key"]) == [np.inf, np.inf, 1e300, 5.0]
    for vt in (1e-6, 0.0):
        tw = twin()
        tw.pool_add(*pc.single_rows(pc.threshold(vt)))
        o = checked(tw, z, 4096, viol_tol=vt)[0]
        assert o["n_violated"] == 3 and list(o["serial"]) == [0, 3, 6] and np.all(o["key"] == np.nextafter(vt, np.inf))


@pytest.mark.parametrize("states", ["all", "parked", "lp"])
def test_mixed_pool_every_state_mask(states):
    tw = twin()
    base, rng = pc.mixed_pool([tw], 240)
    st = tw.pool_state()
    assert set(st["nnz"].tolist()) == set(pc.LENGTHS) and set(st["sense"].tolist()) == {1, -1} and set(st["state"].tolist()) == {0, 1}
    pts = pc.points_near(rng, base, 3)
    for mr in (0, 5, 4096):
        out = checked(tw, pts, mr, states=states)
    mask = {"all": [0, 1], "parked": [1], "lp": [0]}[states]
    pos = {int(s): i for i, s in enumerate(st["serial"])}
    for o in out:
        assert o["n_violated"] > 0 and all(st["state"][pos[int(s)]] in mask for s in o["serial"])
    both = tw.pool_separate_points(pts, 4096, states="all")
    parts = [tw.pool_separate_points(pts, 4096, states=s) for s in ("parked", "lp")]
    for p in range(3):
        assert both[p]["n_violated"] == parts[0][p]["n_violated"] + parts[1][p]["n_violated"]


# ------------------------------------------------------------------------------------------ 2. the twin against the step
def test_parked_separation_is_what_a_step_would_enter():
    tw = twin()
    base, rng = pc.mixed_pool([tw], 300)
    for mr in (0, 3, 40, 4096):
        pt = pc.points_near(rng, base, 1)
        before = tw.pool_state()
        o = tw.pool_separate_points(pt, mr, viol_tol=1e-6, states="parked")[0]
        after = tw.pool_state()
        assert all(np.array_equal(before[f], after[f]) for f in pc.STATE)
        # max_age beyond reach: no LP row is parked by the step, which examines the rows parked before it anyway
        s = copy.deepcopy(tw).pool_step(pt[0], tight_tol=1e-9, viol_tol=1e-6, max_age=10 ** 6, drop_age=10 ** 6, max_return=mr)
        assert o["n_violated"] == s["n_violated"] > 3
        for f, g in (("serial", "enter"), ("key", "enter_key"), ("indptr", "enter_indptr"), ("indices", "enter_indices"),
                     ("values", "enter_values"), ("rhs", "enter_rhs"), ("sense", "enter_sense")):
            assert o[f].dtype == s[g].dtype and np.array_equal(o[f], s[g]), f


# ------------------------------------------------------------------------------------------ 3. pool_drop
DROPS = {"none": lambda s: [], "all": lambda s: s, "first": lambda s: s[:1], "last": lambda s: s[-1:], "alternating": lambda s: s[::2],
         "unknown": lambda s: [-5, 10 ** 12, int(s[-1]) + 1], "duplicates_unsorted": lambda s: [s[7], s[3], s[7], s[3], s[100], -1]}


@pytest.mark.parametrize("pattern", sorted(DROPS))
def test_drop_equals_a_rebuild_of_the_survivors(pattern):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    tw = twin()
    base, rng = pc.mixed_pool([tw], 150)
    tw.pool_drop([4, 5])                       # (serials no longer ascend by one)
    st = tw.pool_state()
    ser = [int(s) for s in DROPS[pattern](st["serial"])]
    gone = tw.pool_drop(np.array(ser, dtype=np.int64))
    keep = ~np.isin(st["serial"], ser)
    assert gone == int((~keep).sum()) == {"none": 0, "all": 148, "first": 1, "last": 1, "alternating": 74, "unknown": 0, "duplicates_unsorted": 3}[pattern]
    # from scratch: a fresh pool given the surviving rows with the serials, states and ages they had
    fresh = CutPoolTwin(8192, pc.NCOLS)
    rows = np.flatnonzero(keep)
    if rows.size:
        lens = st["nnz"][rows]
        ptr = np.concatenate([[0], np.cumsum(lens)])
        fresh.pool_add(ptr, np.concatenate([st["cols"][r, :st["nnz"][r]] for r in rows]), np.concatenate([st["vals"][r, :st["nnz"][r]] for r in rows]),
                       st["rhs"][rows], st["sense"][rows])
        fresh.serial, fresh.state, fresh.age = st["serial"][rows].copy(), st["state"][rows].copy(), st["age"][rows].copy()
    fresh.next_serial = st["next_serial"]
    pc.same_state(tw.pool_state(), fresh.pool_state())
    pts = pc.points_near(rng, base, 2)
    a, b = tw.pool_separate_points(pts, 50), fresh.pool_separate_points(pts, 50)
    for x, y in zip(a, b):
        assert all(np.array_equal(x[f], y[f]) for f in pc.OUT) and x["n_violated"] == y["n_violated"]
    assert tw.pool_add(*pc.single_rows([1.0])) == st["next_serial"]      # serials are never reused


# ------------------------------------------------------------------------------------------ 4. the layout header, compiled alone
LAYOUT_MAIN = r"""
#include "pool_points_layout.h"
#include <stdio.h>
int main(void)
{
    const long caps[] = {0, 1, 7, 63, 64, 65, 1000, 4096};
    for (int i = 0; i < 8; ++i) {
        const PoolPointsLayout y = pool_points_layout(caps[i]);
        printf("%ld %zu %zu %zu %zu %zu %zu %zu %zu\n", caps[i], y.serial, y.key, y.rhs, y.values, y.indptr, y.sense, y.indices, y.slice);
    }
    printf("limits %d %d %d %d %zu\n", POOL_POINTS_ROW_LD, POOL_POINTS_MAX_RETURN, POOL_POINTS_LIST, POOL_POINTS_HDR_BYTES, POOL_POINTS_MAX_BLOCK_BYTES);
    printf("fits %d %d %d %d\n", pool_points_block_fits(4096, 240), pool_points_block_fits(4096, 241), pool_points_block_fits(4095, 241),
           pool_points_block_fits(0, 256));
    printf("bytes %zu\n", pool_points_block_bytes(4096, 256));
    return 0;
}
"""


def test_layout_header_alone(tmp_path):
    from sdpcutsel_via_nn_amd import _capi
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(LAYOUT_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    for ln in lines[:8]:
        cap, serial, key, rhs, values, indptr, sense, indices, slice_ = (int(t) for t in ln.split())
        ld = _capi.ROW_LD
        # header | serial | key | rhs | values | indptr | sense | indices: disjoint, without gaps, in this order
        assert serial == 64 and key == serial + 8 * cap and rhs == key + 8 * cap and values == rhs + 8 * cap
        assert indptr == values + 8 * ld * cap and sense == indptr + 4 * (cap + 1) and indices == sense + 4 * cap
        end = indices + 4 * ld * cap
        assert end <= slice_ < end + 64 and slice_ % 64 == 0 and values % 8 == 0
        assert slice_ == _capi.pool_sep_slice_bytes(cap)
    assert lines[8].split()[1:] == [str(_capi.ROW_LD), str(_capi.POOL_SEP_MAX_RETURN), str(pc.LIST), "64", str(_capi.POOL_SEP_MAX_BLOCK_BYTES)]
    assert _capi.POOL_SEP_MAX_BLOCK_BYTES == 256 * 1024 * 1024
    # the 256 MiB rule: 4096 rows per point fit up to 240 points
    assert lines[9].split()[1:3] == ["1", "0"] and 240 * 1114240 <= 256 * 2 ** 20 < 241 * 1114240 and _capi.pool_sep_slice_bytes(4096) == 1114240
    fits = [str(int(P * _capi.pool_sep_slice_bytes(cap) <= _capi.POOL_SEP_MAX_BLOCK_BYTES)) for cap, P in ((4096, 240), (4096, 241), (4095, 241), (0, 256))]
    assert lines[9].split()[1:] == fits
    assert int(lines[10].split()[1]) == 256 * _capi.pool_sep_slice_bytes(4096) > _capi.POOL_SEP_MAX_BLOCK_BYTES
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    assert "#define SDPCUT_POOL_SEP_MAX_RETURN %d\n" % _capi.POOL_SEP_MAX_RETURN in hdr
    assert "#define SDPCUT_POOL_SEP_LP %du\n" % _capi.POOL_SEP_LP in hdr and "#define SDPCUT_POOL_SEP_PARKED %du\n" % _capi.POOL_SEP_PARKED in hdr


# ------------------------------------------------------------------------------------------ 5. refusals that need no device
def test_refusals_without_a_device():
    from sdpcutsel_via_nn_amd import _capi
    tw = twin()
    tw.pool_add(*pc.single_rows(pc.tie_runs()))
    before = tw.pool_state()
    z = pc.zero_point()[None, :]
    for kw in (dict(max_return=-1), dict(max_return=4097), dict(max_return=1.5), dict(viol_tol=-1e-9), dict(viol_tol=float("nan")),
               dict(viol_tol=float("inf")), dict(states="none"), dict(states=3), dict(states="LP")):
        with pytest.raises(ValueError):
            tw.pool_separate_points(z, **dict(dict(max_return=4), **kw))
    for pts in (np.zeros((0, pc.NCOLS)), np.zeros((257, pc.NCOLS)), np.zeros((2, pc.NCOLS - 1)), np.zeros(pc.NCOLS)):
        with pytest.raises(ValueError):
            tw.pool_separate_points(pts, 4)
    for bad in ([[1, 2]], [1.5], ["a"]):
        with pytest.raises(ValueError):
            tw.pool_drop(bad)
    assert tw.pool_drop([]) == 0 and tw.pool_drop(np.zeros(0)) == 0
    after = tw.pool_state()
    assert all(np.array_equal(before[f], after[f]) for f in pc.STATE)
    # the 256 MiB rule names the product and the limit
    with pytest.raises(ValueError, match=r"256 points x \d+ bytes \(4096 rows each\) = \d+ bytes exceeds the limit of 268435456 bytes"):
        _capi.check_pool_sep_args(256, 4096, 1e-6, "all", 5000)
    assert _capi.check_pool_sep_args(256, 4096, 1e-6, "all", 100) == (4096, 1e-6, 3)      # (a small pool caps the slices)
    assert _capi.check_pool_sep_args(1, 0, 0.0, "lp", 0) == (0, 0.0, 1) and _capi.check_pool_sep_args(1, 0, 0.0, "parked", 0)[2] == 2
    # an empty pool returns zeros for every point
    out = twin().pool_separate_points(np.zeros((3, pc.NCOLS)), 9)
    assert len(out) == 3 and all(o["n_violated"] == 0 and o["serial"].size == 0 and list(o["indptr"]) == [0] for o in out)
