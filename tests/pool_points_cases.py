"""Test pools for the pool at tree nodes (pool_separate_points / pool_drop; tests/test_pool_points_cpu.py, tests/test_gpu_pool_points.py).

Keys under direct control.  A row with ONE entry (column c, value 1.0), sense +1 and right-hand side r has norm 1, and at a point
with v[c] = 0 its activity is 0.0, d = -r and its key (-d) / norm is exactly r: any chosen bit pattern of a positive finite double
can be a key.  A single entry of value 0.0 gives a zero-norm row, whose key is +inf where r > 0.  The families:

    byte_family(b, m)     m keys that differ in exactly byte b (0 = lowest, 7 = the top byte with the exponent) of one pattern: what
                          the radix select of the kernel (eight 8-bit digits from the top) has to tell apart in digit 7 - b alone.
                          More rows than byte values: every key has copies, so ties are there as well
    identical(m)          m equal keys: the K lowest serials must come back
    tie_runs()            runs of equal keys interleaved in serial order; the cap falls inside a run
    inf_keys()            zero-norm rows with r > 0 (+inf), r = 0 and r < 0 (not violated) among ordinary rows
    threshold(vt)         keys one ulp above vt, vt itself and one ulp below: only the first kind is violated at viol_tol = vt
                          (vt = 0.0 is the smallest viol_tol check_pool_params accepts: the smallest subnormal is violated, 0.0 not)

Pools of real shapes: mixed_block has rows of 3, 4, 6, 9, 14 and 20 entries (the lengths of McCormick rows, triangle rows and
eigen-cuts of 3, 4 and 5 variables), both senses, right-hand sides placed around the activity at a base point; park_some parks part
of a pool with one step, so that both states are there.  real_rows (needs a device) takes the rows themselves from round_csr and
tri_round_csr on spar020-100-1 and the model's McCormick rows."""
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances", "spar020-100-1.in")
N = 20
NCOLS = N * (N + 1) // 2 + N
BASE_BITS = 0x3F55555555555555      # about 1.3e-3; every byte 0x55 below the top one: any top byte 0x00 .. 0x7f gives a finite positive double
OUT = ("serial", "key", "indptr", "indices", "values", "rhs", "sense")
STATE = ("serial", "state", "age", "nnz", "sense", "rhs", "norm", "cols", "vals")
LIST = 4096                        # entries of the kernel's list in LDS: more violated rows than this force the radix select


def bits_to_double(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def single_rows(keys, col=0, value=1.0):
    """one-entry rows (col, value) >= keys[i] as a pool_add block"""
    m = len(keys)
    return (np.arange(m + 1, dtype=np.int32), np.full(m, col, np.int32), np.full(m, float(value)), np.asarray(keys, dtype=np.float64), None)


def byte_family(b, m):
    """m keys, BASE_BITS with byte b replaced by a value that walks through all its values in a scrambled order"""
    span = 128 if b == 7 else 256
    keys = []
    for i in range(m):
        v = (i * 37 + 11) % span
        keys.append(bits_to_double((BASE_BITS & ~(0xFF << (8 * b))) | (v << (8 * b))))
    assert all(np.isfinite(k) and k > 0 for k in keys)
    return keys


def identical(m):
    return [0.75] * m


def tie_runs():
    """18 keys: three runs (3.0 x 3, 2.0 x 10, 1.0 x 5) interleaved; a cap of 4 .. 12 falls inside the run of 2.0"""
    return [2.0, 1.0, 3.0, 2.0, 2.0, 1.0, 2.0, 3.0, 2.0, 2.0, 1.0, 2.0, 2.0, 3.0, 1.0, 2.0, 2.0, 1.0]


def inf_keys():
    """-> (block, number of violated rows at the zero point with viol_tol 0): zero-norm rows (value 0.0) with r = 2, 0, -1, 0.5 and
    three ordinary rows; the zero-norm rows with r > 0 have the key +inf and stand first, by serial"""
    ptr = np.arange(8, dtype=np.int32)
    val = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0])
    rhs = np.array([5.0, 2.0, 0.0, 1e300, -1.0, 0.5, -3.0])
    return (ptr, np.zeros(7, np.int32), val, rhs, None), 4


def threshold(vt):
    """keys one ulp above vt, vt, one ulp below, three of each, interleaved; only the first kind is violated at viol_tol = vt"""
    up, down = np.nextafter(vt, np.inf), np.nextafter(vt, -np.inf)
    return [up, vt, down] * 3


def zero_point():
    return np.zeros(NCOLS)


LENGTHS = (3, 4, 6, 9, 14, 20)


def mixed_block(rng, m, base):
    """m rows of the lengths LENGTHS in turn, both senses; the right-hand side of row i sits at the activity at ``base`` shifted by
    (0, +-0.1, +-0.001) ||row||: violated, slack and exactly tight rows, some of which change sides at a perturbed point"""
    from sdpcutsel_via_nn_amd.cutpool import row_norm
    ptr, ind, val, rhs, sense = [0], [], [], [], []
    for i in range(m):
        ln = LENGTHS[i % len(LENGTHS)]
        cols = rng.choice(NCOLS, size=ln, replace=False)
        vals = rng.standard_normal(ln)
        sg = 1 if rng.random() < 0.5 else -1
        act = 0.0
        for c, v in zip(cols, vals):
            act = act + float(v) * float(base[c])
        shift = (0.0, 0.1, -0.1, 0.001, -0.001)[i % 5] * row_norm(vals, ln)
        ind.extend(cols)
        val.extend(vals)
        ptr.append(len(ind))
        rhs.append(act - sg * shift if shift else act)
        sense.append(sg)
    return (np.array(ptr, np.int32), np.array(ind, np.int32), np.array(val), np.array(rhs), np.array(sense, np.int32))


def mixed_pool(pools, n, seed=5):
    """n mixed rows into every pool of ``pools`` (a Scorer and / or twins), then one step that parks the rows slack at the base point
    -> (base point, P perturbed points generator)"""
    rng = np.random.default_rng(seed + n)
    base = rng.random(NCOLS)
    blk = mixed_block(rng, n, base)
    for pl in pools:
        assert pl.pool_add(*blk) == 0
    park_some(pools, base)
    return base, rng


def park_some(pools, point):
    """one step with max_age 1: the rows slack at ``point`` are parked, the others stay in the LP"""
    outs = [pl.pool_step(point, tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=1000, max_return=0) for pl in pools]
    return outs[0]


def points_near(rng, base, P, scale=0.01):
    return np.ascontiguousarray(base[None, :] + scale * rng.standard_normal((P, NCOLS)))


def same_separation(a, b):
    """device result ``a`` (list of dicts) equals the twin's ``b`` byte for byte; -> the select_passes of the points"""
    assert len(a) == len(b)
    for p, (x, y) in enumerate(zip(a, b)):
        for f in OUT:
            assert x[f].dtype == y[f].dtype and x[f].shape == y[f].shape and x[f].tobytes() == y[f].tobytes(), (p, f, x[f][:8], y[f][:8])
        assert x["n_violated"] == y["n_violated"], p
    return [x["select_passes"] for x in a]


def same_state(a, b):
    assert a["n"] == b["n"] and a["next_serial"] == b["next_serial"]
    for f in STATE:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f
    return a


def real_rows(sc, inst):
    """Rows of real shapes from the device's own separations on spar020-100-1 at a random McCormick point -> pool_add block with
    rows of 3 (McCormick), 4 and 6 (triangle), 9, 14 and 20 (eigen-cuts of 3, 4, 5 variables) entries; every other row is
    negated and given sense -1 (the same half-space)."""
    from sdpcutsel_via_nn_amd import harness
    pt = harness.random_mccormick_point(N, np.random.default_rng(7))
    blocks = []
    ptr, ind, val, rhs = harness.mccormick_csr(N, inst["adj"])
    ptr = np.asarray(ptr, dtype=np.int64)
    three = np.flatnonzero(np.diff(ptr) == 3)[:40]
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in three])
    # (the model states these as <= rows: as >= rows of the pool they are negated)
    blocks.append((np.arange(three.size + 1) * 3, np.asarray(ind)[take], -np.asarray(val, dtype=np.float64)[take],
                   -np.asarray(rhs, dtype=np.float64)[three]))
    sc.tri_preprocess(inst["adj"])
    t = sc.tri_round_csr(60, point=pt, copy=True)
    blocks.append((t["indptr"], t["indices"], t["values"], t["rhs"]))
    for dim in (3, 4, 5):
        sc.set_candidates_cover(inst["adj"], dim)
        r = sc.round_csr(1, 40, point=pt, copy=True)
        blocks.append((r["indptr"], r["indices"], r["values"], r["rhs"]))
    lens = np.concatenate([np.diff(np.asarray(b[0], dtype=np.int64)) for b in blocks])
    ind = np.concatenate([np.asarray(b[1], dtype=np.int64)[int(b[0][0]):int(b[0][-1])] for b in blocks]).astype(np.int32)
    val = np.concatenate([np.asarray(b[2], dtype=np.float64)[int(b[0][0]):int(b[0][-1])] for b in blocks])
    rhs = np.concatenate([np.asarray(b[3], dtype=np.float64) for b in blocks])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    sense = np.where(np.arange(rhs.shape[0]) % 2 == 0, 1, -1).astype(np.int32)
    flip = np.repeat(sense, lens).astype(np.float64)
    return (ptr, ind, val * flip, rhs * sense, sense), pt
