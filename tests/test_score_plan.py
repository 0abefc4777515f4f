"""The rules of a scoring launch (csrc/score_plan.h: score_plan, pf_mloc_rule, score_form) against restatements written from the
comments of the kernel and from the launchers as they were before the rules had a header -- not generated from the header.
CPU only: the header is plain C++."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

EINVAL, ESTATE = -1, -4                       # include/sdpcut.h
EIG, NN = 1, 2
MFMA, SIMPLE, VALU = 0, 1, 2
FEAS, OPT, STRONG, COMBAUTO = 1, 2, 3, 5      # topk_route.h (COMBAUTO: a mode the score kernels have no histogram variant for)
FORM_EIG, FORM_ONE, FORM_SIDE, FORM_SEQ = 1, 2, 3, 4
MSG_NONE, MSG_NO_NETWORK, MSG_NO_VARIANT, MSG_MEASURE = 0, 1, 2, 3
MESSAGES = {MSG_NO_NETWORK: "no network set for this candidate size",
            MSG_NO_VARIANT: "score: no histogram variant for this selection mode",
            MSG_MEASURE: "score: the selection mode ranks by a measure this launch does not compute"}

PLAN_IN = ("n", "n_cu", "K", "n_total", "fuse_k", "fused")
PLAN_OUT = ("grid", "strip", "rr_end", "tail_nhi", "tail_hi", "tail_lo", "pf_mloc", "spread")
FORM_IN = ("variant", "flags", "fuse", "fuse_mode", "eig_kernel", "one_launch", "side_streams", "side_choice", "timing", "n_total",
           "n2", "n3", "n4", "n5", "set2", "set3", "set4", "set5", "shape2", "shape3", "shape4", "shape5", "unc2", "unc3", "unc4", "unc5")
FORM_OUT = ("err", "msg", "fused", "form", "calibrate", "timed", "first", "last", "kbig", "nclasses")

WRAPPER = r"""
#include <string.h>
#include "score_plan.h"
extern "C" void plan_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + %d * i;
        int64_t *o = out + %d * i;
        const ScorePlan p = score_plan(a[0], (int)a[1], (int)a[2], a[3], a[4], a[5] != 0);
        o[0] = p.grid; o[1] = p.strip; o[2] = p.rr_end; o[3] = p.tail_nhi; o[4] = p.tail_hi; o[5] = p.tail_lo; o[6] = p.pf_mloc; o[7] = p.spread;
    }
}
extern "C" void mloc_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) out[i] = pf_mloc_rule(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
}
extern "C" void form_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + %d * i;
        int64_t *o = out + %d * i;
        ScoreFormIn r;
        r.variant = (int)a[0]; r.flags = (uint32_t)a[1]; r.fuse = a[2] != 0; r.fuse_mode = (int)a[3];
        r.eig_kernel = a[4] != 0; r.one_launch = a[5] != 0; r.side_streams = (int)a[6]; r.side_choice = (int)a[7]; r.timing = (int)a[8];
        r.n_total = a[9];
        for (int k = 2; k <= 5; ++k) {
            r.n[k] = a[10 + k - 2]; r.net_set[k] = a[14 + k - 2] != 0; r.shape_ok[k] = a[18 + k - 2] != 0; r.unclamped_ok[k] = a[22 + k - 2] != 0;
        }
        const ScoreForm f = score_form(r);
        o[0] = f.err; o[1] = f.msg; o[2] = f.fused; o[3] = f.form; o[4] = f.calibrate; o[5] = f.timed; o[6] = f.first; o[7] = f.last;
        o[8] = f.kbig; o[9] = f.nclasses;
    }
}
extern "C" int shapes(int *out)      /* NetShape<K>, net_shape_is, mfma_cols */
{
    out[0] = NetShape<2>::H; out[1] = NetShape<2>::NH; out[2] = NetShape<3>::H; out[3] = NetShape<3>::NH;
    out[4] = NetShape<4>::H; out[5] = NetShape<4>::NH; out[6] = NetShape<5>::H; out[7] = NetShape<5>::NH;
    int ok = 0;
    for (int k = 1; k <= 6; ++k)
        for (int w = 49; w <= 64; ++w)
            for (int nh = 2; nh <= 5; ++nh) ok += net_shape_is(k, w, nh);
    return 100 * ok + 10 * mfma_cols(3) + (int)pf_score_k(3);
}
extern "C" int message_is(int msg, const char *text) { return strcmp(score_form_msg(msg), text) == 0; }
""" % (len(PLAN_IN), len(PLAN_OUT), len(FORM_IN), len(FORM_OUT))

P64 = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_plan")
    src = d / "plan.cpp"
    src.write_text(WRAPPER)
    so = d / "plan.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _call(fn, cases, ncols_out):
    cases = np.ascontiguousarray(cases, dtype=np.int64)
    out = np.full((cases.shape[0], ncols_out), -99, dtype=np.int64)
    fn(ctypes.c_long(cases.shape[0]), cases.ctypes.data_as(P64), out.ctypes.data_as(P64))
    return out


# ---- the work split ------------------------------------------------------------------------------------------------------------
def _n_values(n_cu):
    ns = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]
    ns += [32 * n_cu * 8 + d for d in (-17, -1, 0, 1, 17)]
    rnd = n_cu * 8 * 4 * 64      # candidates of one round-robin round of a full grid
    for R in (1, 2, 3):
        ns += [R * rnd + d for d in (-17, -1, 0, 1, 17)]
        for pct in (87, 89, 90, 91, 95, 99):
            ns += [R * rnd + pct * rnd // 100 + d for d in (-1, 0, 1, 5)]
    return sorted(set(n for n in ns if n >= 1))


PLAN_GRID = [(n, n_cu) for n_cu in (1, 4, 256) for n in _n_values(n_cu)]
# (K, n_total as a function of n, fuse_k, fused): 3-variable lists count the fine histogram, 2-variable ones do not
PLAN_VARIANTS = [(3, lambda n: n, 5000, 1), (3, lambda n: 3 * n + 7, 5000, 1), (3, lambda n: n, 16384, 1), (3, lambda n: n, 0, 1),
                 (3, lambda n: n, 5000, 0), (2, lambda n: n, 5000, 1)]


def _mloc_restated(head_k, per_wg, n_total):
    """24 + 8 x the expected share of the head, as pf_mloc_for had it (and, with the guards in this order, the eigenvalue launch)"""
    if head_k <= 0 or per_wg >= 60000 or n_total < 1:
        return 0
    m = 24.0 + 8.0 * (float(head_k) * float(per_wg) / float(n_total))
    return 60000 if m > 60000.0 else int(m + 0.999)


def _plan_restated(n, n_cu, K, n_total, fuse_k, fused):
    """launch_score_k before the split: grid_for, the strip-32 rule, set_balanced_tail, pf_mloc_for, spread"""
    strip = 64
    grid = max(1, min(-(-n // 256), n_cu * 8))
    if n <= 32 * n_cu * 4 * 2:
        strip = 32
        grid = (-(-n // 32) + 3) // 4
    rr_end, nhi, hi, lo = n, 0, 0, 0
    if strip == 64:
        W = grid * 4
        rnd = W * 64
        R, rem = divmod(n, rnd)
        tiles = -(-rem // 16)
        if R >= 1 and 100 * rem >= 90 * rnd:
            lo = tiles // W
            rr_end, hi = R * rnd, lo + 1
            nhi = (tiles - lo * W + 3) // 4 * 4
    mloc = _mloc_restated(fuse_k, -(-n // grid), n_total) if (fused and K == 3) else 0
    spread = int(mloc > 0 and n <= grid * 4 * strip)
    return dict(grid=grid, strip=strip, rr_end=rr_end, tail_nhi=nhi, tail_hi=hi, tail_lo=lo, pf_mloc=mloc, spread=spread)


def _walk(n, p, spread):
    """The strip loop of score_mfma_body for every wave of the launch at once: how often each candidate is visited, and the longest
    strip.  Wave w of workgroup b is wave gw = 4 b + w of the launch (spread: w * grid + b); it takes the strips of p.strip
    candidates gw, gw + W, gw + 2 W ... below rr_end (W = 4 grid waves), each cut at rr_end, and then its tail strip
    [t_start, t_end): tail_hi (the first tail_nhi waves) or tail_lo column tiles of 16 candidates from rr_end on, cut at n."""
    grid, strip, rr_end = int(p["grid"]), int(p["strip"]), int(p["rr_end"])
    nhi, hi, lo = int(p["tail_nhi"]), int(p["tail_hi"]), int(p["tail_lo"])
    b, w = np.meshgrid(np.arange(grid, dtype=np.int64), np.arange(4, dtype=np.int64), indexing="ij")
    gw = (w * grid + b if spread else b * 4 + w).ravel()
    wstride = grid * 4 * strip
    c_first = gw * strip
    t_tiles = np.where(gw < nhi, hi, lo)
    t_start = np.minimum(rr_end + 16 * np.where(gw < nhi, gw * hi, nhi * hi + (gw - nhi) * lo), n)
    t_end = np.minimum(t_start + 16 * t_tiles, n)
    tail = c_first >= rr_end
    s0 = np.where(tail, t_start, c_first)
    more = np.where(tail, t_start < t_end, True)
    diff = np.zeros(n + 1, dtype=np.int64)
    longest, strips = 0, 0
    while more.any():
        lim = np.where(tail, t_end, np.minimum(s0 + strip, rr_end))
        a, e = s0[more], lim[more]
        assert np.all(a <= e) and np.all(a >= 0) and np.all(e <= n)
        longest = max(longest, int((e - a).max()))
        strips += a.size
        np.add.at(diff, a, 1)
        np.add.at(diff, e, -1)
        nx_rr = ~tail & (s0 + wstride < rr_end)
        nx_tail = ~tail & ~nx_rr
        nx_more = nx_rr | (nx_tail & (t_start < t_end))
        s0 = np.where(nx_rr, s0 + wstride, t_start)
        tail = tail | nx_tail
        more = more & nx_more
    return np.cumsum(diff[:n]), longest


@pytest.fixture(scope="module")
def plans(lib):
    cases = np.array([(n, n_cu, K, nt(n), fk, fu) for (n, n_cu) in PLAN_GRID for (K, nt, fk, fu) in PLAN_VARIANTS], dtype=np.int64)
    return cases, _call(lib.plan_batch, cases, len(PLAN_OUT))


def test_every_candidate_exactly_once(plans):
    cases, out = plans
    nv = len(PLAN_VARIANTS)
    strip32 = balanced = spreads = 0
    for i in range(0, cases.shape[0], nv):      # (the split does not depend on the variant: walk the first, which may spread)
        n = int(cases[i, 0])
        p = dict(zip(PLAN_OUT, out[i]))
        assert np.array_equal(out[i:i + nv, :6], np.tile(out[i, :6], (nv, 1)))
        assert p["grid"] >= 1 and p["strip"] in (32, 64)
        forms = {int(p["spread"])}
        if n <= p["grid"] * 4 * p["strip"]:
            forms.add(1)
        for spread in sorted(forms):
            visits, longest = _walk(n, p, spread)
            assert visits.min() == 1 and visits.max() == 1, (n, int(cases[i, 1]), spread, p)
            assert longest <= 64, (n, int(cases[i, 1]), spread, longest)
        strip32 += p["strip"] == 32
        balanced += p["rr_end"] < n
        spreads += 1 in forms
    assert strip32 > 0 and balanced > 0 and spreads > 0      # the grid reaches the strip-32 and the balanced-tail branches
    assert balanced == 138


def test_plan_against_the_restated_rules(lib, plans):
    cases, out = plans
    for c, o in zip(cases, out):
        want = _plan_restated(*[int(v) for v in c])
        got = dict(zip(PLAN_OUT, (int(v) for v in o)))
        assert got == want, (dict(zip(PLAN_IN, c)), got, want)
    assert (out[:, 6] > 0).any() and (out[:, 6] == 0).any() and (out[:, 7] == 1).any() and (out[:, 7] == 0).any()
    # two anchors computed by hand from launch_score_k / set_balanced_tail as they were: 256 CUs, 10^6 and 10^6 + 3 candidates
    a = _call(lib.plan_batch, [(10 ** 6, 256, 3, 10 ** 6, 0, 0), (1000003, 256, 3, 1000003, 0, 0)], len(PLAN_OUT))
    assert dict(zip(PLAN_OUT, a[0])) == dict(grid=2048, strip=64, rr_end=524288, tail_nhi=5156, tail_hi=4, tail_lo=3, pf_mloc=0, spread=0)
    assert a[1, 3] == 5160 and tuple(a[1, :3]) == (2048, 64, 524288)
    sh = (ctypes.c_int * 8)()
    code = lib.shapes(sh)
    assert list(sh) == [64, 3, 50, 3, 50, 3, 64, 4]
    assert code == 100 * 4 + 10 * 2 + 1      # exactly the four shipped shapes; two column tiles per pass; K = 3 counts the fine histogram


def test_pf_mloc_rule(lib):
    head = [-1, 0, 1, 100, 5000, 7496, 7497, 7498, 16384]
    per_wg = [1, 256, 489, 1000, 59999, 60000, 60001]
    total = [-1, 0, 1, 1000, 10 ** 6, 10 ** 8]
    cases = np.array(list(itertools.product(head, per_wg, total)), dtype=np.int64)
    out = _call(lib.mloc_batch, cases, 1)[:, 0]
    want = np.array([_mloc_restated(*[int(v) for v in c]) for c in cases])
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, (cases[bad[0]], out[bad[0]], want[bad[0]])
    by = {tuple(int(v) for v in c): int(o) for c, o in zip(cases, out)}
    assert by[(5000, 59999, 10 ** 6)] > 0 and by[(5000, 60000, 10 ** 6)] == 0      # a table counter could overflow: no fine histogram
    assert (by[(7496, 1000, 1000)], by[(7497, 1000, 1000)], by[(7498, 1000, 1000)]) == (59992, 60000, 60000)      # m across 60000
    assert by[(16384, 59999, 1000)] == 60000 and by[(0, 256, 1000)] == 0 and by[(1, 1, 10 ** 8)] == 24 and by[(100, 256, 1000)] == 229


# ---- the form of a scoring call ------------------------------------------------------------------------------------------------
# per class 2..5: (n, network set, shipped shape, pre-activations bounded)
EMPTY, SHIPPED = (0, 1, 1, 1), (1000, 1, 1, 1)
CLASS_PATTERNS = {
    "none": (EMPTY, EMPTY, EMPTY, EMPTY),
    "one": (EMPTY, SHIPPED, EMPTY, EMPTY),
    "three, one unshaped": ((10, 1, 0, 1), SHIPPED, SHIPPED, EMPTY),
    "three, one clamped": ((10, 1, 1, 1), (1000, 1, 1, 0), (2000, 1, 1, 1), EMPTY),
    "three, one without a network": ((10, 1, 1, 1), SHIPPED, (5, 0, 0, 0), EMPTY),
    "three shipped": ((10, 1, 1, 1), (70000, 1, 1, 1), EMPTY, (70000, 1, 1, 1)),
}


def _parent_decision(c):
    """launch_score as it was, with launch_classes_one and launch_score_k under it, followed launch by launch: the first refusal a
    launch would have met (whichever classes had been launched before it), else the form."""
    ks = [k for k in (2, 3, 4, 5) if c["n%d" % k] > 0]
    nn, eig = bool(c["flags"] & NN), bool(c["flags"] & EIG)

    def shape_ok(k):      # net_shape_ok
        return (not nn) or bool(c["set%d" % k] and c["shape%d" % k])

    fuse = bool(c["fuse"])
    if fuse:
        ok = c["variant"] == MFMA and all(shape_ok(k) for k in ks)
        fuse = ok and bool(ks)
    r = dict(err=0, msg=MSG_NONE, fused=int(fuse), calibrate=0, form=FORM_SEQ)
    mode = c["fuse_mode"] if fuse else 0
    if c["flags"] == EIG and c["variant"] == MFMA and c["eig_kernel"]:
        if fuse and mode != FEAS:
            return dict(r, err=EINVAL, msg=MSG_MEASURE)
        return dict(r, form=FORM_EIG, timed=int(c["timing"] != 0 and c["n_total"] > 0))
    first, last = (ks[0], ks[-1]) if ks else (0, 0)
    kbig = 0
    for k in ks:
        if not kbig or c["n%d" % k] > c["n%d" % kbig]:
            kbig = k
    r.update(first=first, last=last, kbig=kbig, nclasses=len(ks), timed=int(c["timing"] != 0 and first != 0))

    def class_launch(k, f):      # launch_score_k of a non-empty class: the refusal it returns, or None
        if nn and not c["set%d" % k]:
            return (ESTATE, MSG_NO_NETWORK)
        if c["variant"] == MFMA and shape_ok(k):
            if f not in (0, FEAS, OPT, STRONG):
                return (EINVAL, MSG_NO_VARIANT)
            if (not eig) if f == FEAS else (f != 0 and not nn):
                return (EINVAL, MSG_MEASURE)
        return None

    def launches(order, f):
        for k in order:
            e = class_launch(k, f)
            if e:
                return e
        return None

    if len(ks) > 1 and c["one_launch"]:      # launch_classes_one: 1 launched, 0 not applicable
        applicable = (c["variant"] == MFMA and nn and mode in (0, FEAS, OPT, STRONG) and not (mode == FEAS and not eig)
                      and all(c["set%d" % k] and shape_ok(k) and c["unc%d" % k] for k in ks))
        if applicable:
            return dict(r, form=FORM_ONE)
    side_order = [kbig] + [k for k in ks if k != kbig]
    if len(ks) > 1 and not r["timed"] and c["side_streams"]:
        if c["side_streams"] == 2 and c["side_choice"] < 0:
            r["calibrate"] = 1
            e = launches(ks, 0) or launches(side_order, 0)      # calibrate_side_streams: both forms, no fuse
            if e:
                return dict(r, err=e[0], msg=e[1])
            # (what the measurement finds is not the decision's: the real launches are followed for both outcomes)
            e = launches(side_order, mode) or launches(ks, mode)
            return dict(r, err=e[0], msg=e[1]) if e else r
        if c["side_streams"] == 1 or c["side_choice"] == 1:
            e = launches(side_order, mode)
            return dict(r, err=e[0], msg=e[1]) if e else dict(r, form=FORM_SIDE)
    e = launches(ks, mode)
    return dict(r, err=e[0], msg=e[1]) if e else r


def test_form_table(lib):
    rows, names = [], []
    for name, pat in CLASS_PATTERNS.items():
        per_class = [[p[j] for p in pat] for j in range(4)]      # n, set, shape, unclamped by class
        n_total = sum(per_class[0])
        for variant, flags, mode, eig_kernel, one_launch, side, choice, timing in itertools.product(
                (MFMA, SIMPLE, VALU), (EIG, NN, EIG | NN), (None, FEAS, OPT, STRONG, COMBAUTO), (0, 1), (0, 1), (0, 1, 2), (-1, 0, 1), (0, 1)):
            rows.append([variant, flags, int(mode is not None), mode or 0, eig_kernel, one_launch, side, choice, timing, n_total]
                        + per_class[0] + per_class[1] + per_class[2] + per_class[3])
            names.append(name)
    cases = np.array(rows, dtype=np.int64)
    assert cases.shape == (6 * 3 * 3 * 5 * 2 * 2 * 3 * 3 * 2, len(FORM_IN))
    out = _call(lib.form_batch, cases, len(FORM_OUT))
    forms_seen, refusals_seen, calibrations = set(), set(), 0
    for name, c, o in zip(names, cases, out):
        cd = dict(zip(FORM_IN, (int(v) for v in c)))
        got = dict(zip(FORM_OUT, (int(v) for v in o)))
        want = _parent_decision(cd)
        keys = ("err", "msg", "fused") if want["err"] else tuple(want)      # a refused call has no form
        assert {k: got[k] for k in keys} == {k: want[k] for k in keys}, (name, cd, got, want)
        if want["err"]:
            refusals_seen.add((want["err"], want["msg"], "eig" if cd["flags"] == EIG and cd["variant"] == MFMA and cd["eig_kernel"] else "mlp"))
        else:
            forms_seen.add(want["form"])
            calibrations += want["calibrate"]
    assert forms_seen == {FORM_EIG, FORM_ONE, FORM_SIDE, FORM_SEQ} and calibrations > 0
    assert refusals_seen == {(EINVAL, MSG_MEASURE, "eig"), (ESTATE, MSG_NO_NETWORK, "mlp"), (EINVAL, MSG_NO_VARIANT, "mlp"),
                             (EINVAL, MSG_MEASURE, "mlp")}
    for msg, text in MESSAGES.items():
        assert lib.message_is(msg, text.encode())
