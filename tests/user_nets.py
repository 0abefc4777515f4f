"""User networks for the scoring tests (test_user_networks_cpu.py, test_gpu_user_networks.py): networks of any accepted shape with
a chosen net_pack bound, the inputs of a candidate list as the device's gather defines them, the references obj = negSM + y max_elem
in long double / float64 / float64 with the fast tansig's stated error, the two tolerance rules, the instances and points of the
GPU tests and the compiled score_plan.  A plain module: no fixtures, no GPU.

The two tolerance rules (both from reference-side quantities only, computed per case):
  library-exp kernels (nn_batch, the simple kernel, the exact head):  device error <= LIB_FACTOR x the float64 twin's error
  fast-tansig kernels (MFMA with and without the clamps, VALU):       device error <= FAST_FACTOR x max(float64 twin's error,
                                                                       noisy twin's error)
errors being normwise against the long double reference.  LIB_FACTOR = 16 is the factor test_gpu_train.py uses for the same
arithmetic.  The noisy twin adds +-TAU = 1e-15 -- the absolute error csrc/tansig.h states for the fast tansig -- with random signs
to every hidden activation; aligned errors over a dot product of H <= 64 terms can exceed random ones by up to sqrt(64) = 8, and
FAST_FACTOR is that bound.  (It began at 4 -- a CPU emulation of tansig4 / exp_y8_scaled lands at 0.16-0.46 of the noisy twin's
error on 512 inputs -- with leave to go up to 16 for a kernel that exceeds 4 while agreeing with the other kernels at that level.
Measured on an MI355X: every case lies below 1.9 except ONE list of one candidate, where the twins' errors, 2.1e-17, happen to lie
below the unit roundoff 1.1e-16 of the result itself: the VALU kernel's score is 9.2e-17 off, ratio 4.3, the MFMA kernel's the
neighbouring double, ratio 5.3 between the two.  The tests assert that agreement between the kernels under the same allowance.)
DESIGN.md section 5 records the ratios measured on the device."""
import ctypes
import os
import subprocess

import numpy as np

from sdpcutsel_via_nn_amd import networks, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
LD = np.longdouble

LIB_FACTOR = 16.0
FAST_FACTOR = 8.0
TAU = 1e-15

BOUNDS = (12.0, 38.5, 41.5, 90.0, 700.0)      # clamp-free, clamp-free near the limit, just clamped, saturating, saturating
SHAPES = {2: (64, 3), 3: (50, 3), 4: (50, 3), 5: (64, 4)}      # NetShape<K> of csrc/score_plan.h: (H, hidden layers)
NARROW_GAIN = 8.0       # mapminmax of x in [0.375, 0.625]: [0, 1] -> [-4, 4]

N_VARS = 24
BASE = 512              # base candidates per size
LIST_LENGTHS = (1, 17, 48, 257, 1000)      # section c; 48 = three 16-tiles: a two-tile and a one-tile pass
STRIP64_LENGTH = 70001
ROUND_LENGTHS = (9001, 40000)
MIXED_COUNTS = {3: 3000, 5: 40, 4: 7, 2: 1}


# ---- networks ------------------------------------------------------------------------------------------------------------------
def net_bound(k, widths, params):
    """the bound of csrc/net_pack.h on every hidden pre-activation: |b_j| + sum_i |W_ji| max|in_i|, max|in| = 3 for the mapped inputs
    and 1 behind a tansig"""
    _, _, _, Ws, Bs, _ = networks.split_params(k, widths, np.asarray(params, dtype=np.float64))
    return max(float((np.abs(B) + np.abs(W).sum(axis=1) * (networks.INPUT_CLAMP if l == 0 else 1.0)).max())
               for l, (W, B) in enumerate(zip(Ws[:-1], Bs[:-1])))


def domain_image(k, widths, params):
    """the mapped endpoints of the input domain (x_i in [0, 1], q_m in [-1/k, 1/k]) -> float64 [2, d_in]"""
    xoffset, gain, ymin, _, _, _ = networks.split_params(k, widths, np.asarray(params, dtype=np.float64))
    d_in = xoffset.shape[0]
    lo = np.array([0.0] * k + [-1.0 / k] * (d_in - k))
    hi = np.array([1.0] * k + [1.0 / k] * (d_in - k))
    return np.stack([(lo - xoffset) * gain + ymin, (hi - xoffset) * gain + ymin])


def make_network(k, H, nh, bound, seed, x_gain=2.0):
    """A tansig MLP of nh hidden layers of width H for k-variable candidates -> (widths int32, params float64) in the packing of
    sdpcut_set_network.  Weights and biases uniform in +-1, the hidden part then rescaled so that net_bound is `bound` (the
    construction of _random_network in test_net_pack.py).  The mapping is near the shipped one: x in [0, 1] and q in [-1/k, 1/k] go
    to [-1, 1] up to a per-cent (xoffset ~ 0 | -1/k, gain ~ 2 | k, ymin -1).  x_gain changes the mapping of the x inputs only: it is
    mapminmax of x in [1/2 - 1/x_gain, 1/2 + 1/x_gain], so x_gain = 8 sends [0, 1] onto [-4, 4]."""
    rng = np.random.default_rng(seed)
    d_in = k * (k + 3) // 2
    widths = np.array([H] * nh + [1], dtype=np.int32)
    jit = rng.uniform(-0.01, 0.01, (2, d_in))
    xoffset = np.concatenate([np.full(k, 0.5 - 1.0 / x_gain), np.full(d_in - k, -1.0 / k)]) + jit[0] * np.concatenate([np.full(k, 1.0), np.full(d_in - k, 1.0 / k)])
    gain = np.concatenate([np.full(k, float(x_gain)), np.full(d_in - k, float(k))]) * (1.0 + jit[1])
    parts, fan = [xoffset, gain, np.array([-1.0])], d_in
    for w in widths:
        parts += [rng.uniform(-1, 1, int(w) * fan), rng.uniform(-1, 1, int(w))]
        fan = int(w)
    parts.append(np.array([-1.0, 0.31, -3.4]) * (1.0 + rng.uniform(-0.01, 0.01, 3)))      # y_ymin, y_gain, y_xoffset near the shipped ones
    params = np.concatenate(parts).astype(np.float64)
    hidden = slice(2 * d_in + 1, params.shape[0] - 3 - (H + 1))
    params[hidden] *= bound / net_bound(k, widths, params)
    networks.check_network(k, widths, params)
    return widths, params


def shaped_network(k, bound, seed=None, x_gain=2.0):
    """a user network of the shape the MFMA / VALU kernels of size class k are compiled for"""
    H, nh = SHAPES[k]
    return make_network(k, H, nh, bound, 1000 * k + int(bound) if seed is None else seed, x_gain=x_gain)


def narrow_network(k):
    """shipped shape, small weights (bound 12), trained on a narrower x range: fails the domain condition of unclamped_ok only"""
    return shaped_network(k, 12.0, seed=7000 + k, x_gain=NARROW_GAIN)


def unshaped_network(k, bound=12.0, H=49, nh=2, seed=None):
    return make_network(k, H, nh, bound, 2000 * k + H + nh if seed is None else seed)


#  k, H, hidden layers, bound: every k in 2..5, every H of the issue's list, every depth 1..4 and every bound at least twice;
#  H = 64 with 4 layers and H = 1 with 1 layer included; none of them is a shipped shape except where said
NN_BATCH_GRID = [
    (2, 1, 1, 12.0), (3, 1, 2, 700.0), (4, 3, 1, 38.5), (5, 3, 3, 41.5), (2, 16, 2, 90.0), (3, 16, 4, 12.0),
    (4, 47, 1, 700.0), (5, 47, 3, 38.5), (2, 48, 2, 41.5), (3, 48, 4, 90.0), (4, 49, 1, 12.0), (5, 49, 2, 700.0),
    (2, 52, 3, 38.5), (3, 52, 4, 41.5), (4, 53, 1, 90.0), (5, 53, 2, 12.0), (2, 63, 3, 700.0), (3, 63, 4, 38.5),
    (4, 64, 4, 41.5), (5, 64, 4, 90.0), (2, 64, 3, 700.0), (3, 50, 3, 90.0), (4, 50, 2, 12.0), (5, 64, 1, 41.5),
]


# ---- instances, points, lists ---------------------------------------------------------------------------------------------------
def instance(seed, n=N_VARS):
    """Q integer in +-20 (rounded N(0, 20^2), a few beyond) with 30 % zeros, as test_gpu_fuzz._instance draws it -> Q_arr [n(n+1)/2]"""
    rng = np.random.default_rng(seed)
    L = n * (n + 1) // 2
    return np.round(rng.normal(size=L) * 20) * (rng.uniform(size=L) < 0.7)


def generic_point(seed, n=N_VARS):
    """a McCormick-feasible point [X packed | x]"""
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(n)
    x = rng.uniform(0, 1, n)
    lo = np.maximum(0.0, x[iu[0]] + x[iu[1]] - 1.0)
    hi = np.minimum(x[iu[0]], x[iu[1]])
    return np.concatenate([lo + rng.uniform(size=lo.shape[0]) * (hi - lo), x])


def corner_point(seed, n=N_VARS):
    """every x in {0, 1}, X = min(x_i, x_j): the ends of the x domain"""
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(n)
    x = rng.integers(0, 2, n).astype(np.float64)
    x[:2] = (0.0, 1.0)
    return np.concatenate([np.minimum(x[iu[0]], x[iu[1]]), x])


def base_sets(k, seed, n=N_VARS, count=BASE):
    return synthetic.random_index_sets(n, k, count, np.random.default_rng(seed))


def padded(sets):
    """[N, k] -> the [N, 5] layout of set_candidates (padded with -1) and ks"""
    out = np.full((sets.shape[0], 5), -1, dtype=np.int32)
    out[:, :sets.shape[1]] = sets
    return out, np.full(sets.shape[0], sets.shape[1], dtype=np.int32)


def nn_batch_inputs(k, seed, count=257, corners=32):
    """rows [x | q] of sdpcut_nn_batch: x uniform in [0, 1], q uniform in [-1/k, 1/k]; the last `corners` rows are all-corner rows
    (every x in {0, 1}, every q = +-1/k)"""
    rng = np.random.default_rng(seed)
    m = k * (k + 1) // 2
    X = np.concatenate([rng.uniform(0, 1, (count, k)), rng.uniform(-1.0 / k, 1.0 / k, (count, m))], axis=1)
    X[-corners:, :k] = rng.integers(0, 2, (corners, k))
    X[-corners:, k:] = np.where(rng.integers(0, 2, (corners, m)) == 1, 1.0 / k, -1.0 / k)
    X[-1, :k], X[-2, :k] = 1.0, 0.0
    return X


def tiled(sets, N):
    """the base list repeated to length N: candidate i is base candidate i % len(base)"""
    return sets[np.arange(N) % sets.shape[0]]


# ---- inputs and references -------------------------------------------------------------------------------------------------------
def inputs_of(oracle, sets, k, n, vv, Q):
    """-> (x [N, k], q [N, k(k+1)/2], max_elem [N], negSM [N]) in float64, built as oracle.candidate_record / opt_score_entry build
    them (cut_select_qp.py:529-540, :573-582): max_elem = k max|Q_slice| (1 if that is 0), q = np.divide(Q_slice, max_elem),
    S = ((0 + q_0 X_0) + q_1 X_1) + ... summed left to right, negSM = (-S) max_elem.  The device's gather (csrc/gather.h) is defined
    to give these bits."""
    sets = np.asarray(sets, dtype=np.int64)
    vv = np.asarray(vv, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    L = n * (n + 1) // 2
    pos = oracle.triu_positions(sets, n)
    qraw = Q[pos]
    max_elem = float(k) * np.abs(qraw).max(axis=1)
    max_elem = np.where(max_elem == 0.0, max_elem + 1.0, max_elem)
    q = np.divide(qraw, max_elem[:, None])
    X = vv[:L][pos]
    S = np.zeros(sets.shape[0])
    for m in range(pos.shape[1]):
        S = S + q[:, m] * X[:, m]
    return vv[L:][sets], q, max_elem, (-S) * max_elem


def forward_noisy(k, widths, params, inputs, tau, seed):
    """networks.forward_twin in float64 with +-tau (random signs) added to every hidden activation"""
    rng = np.random.default_rng(seed)
    params = np.asarray(params, dtype=np.float64)
    xoffset, gain, ymin, Ws, Bs, (y_ymin, y_gain, y_xoffset) = networks.split_params(k, widths, params)
    a = (np.asarray(inputs, dtype=np.float64) - xoffset) * gain + ymin
    for W, b in zip(Ws[:-1], Bs[:-1]):
        a = networks._tansig(a @ W.T + b)
        a = a + tau * rng.choice([-1.0, 1.0], size=a.shape)
    y = a @ Ws[-1][0] + Bs[-1][0]
    return (y - y_ymin) / y_gain + y_xoffset


def obj_reference(k, widths, params, x, q, max_elem, negSM, dtype=LD, noise=None):
    """obj_improve = negSM + y max_elem with y the network's output on [x | q]:
    dtype = np.longdouble: networks.forward_twin and the composition in long double (THE reference);
    dtype = np.float64: the float64 twin;
    noise = (tau, seed), dtype float64: the noisy twin (forward_noisy)."""
    inputs = np.concatenate([x, q], axis=1)
    with np.errstate(over="ignore"):      # exp(-2n) of a saturating network overflows to inf, tansig goes to -1: as intended
        if noise is not None:
            y = forward_noisy(k, widths, params, inputs, noise[0], noise[1])
        else:
            y = networks.forward_twin(k, widths, params, inputs, dtype=dtype)
    return np.asarray(negSM).astype(y.dtype) + y * np.asarray(max_elem).astype(y.dtype)


def normwise(a, ref):
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.sqrt(((a - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))


def ratio(err, allowance_base):
    return err / allowance_base if allowance_base > 0 else (0.0 if err == 0 else float("inf"))


class Reference(object):
    """the three references of one (network, inputs) case and the allowances of the two rules"""

    def __init__(self, k, widths, params, x, q, max_elem, negSM, seed=0):
        self.ld = obj_reference(k, widths, params, x, q, max_elem, negSM, dtype=LD)
        self.f64 = obj_reference(k, widths, params, x, q, max_elem, negSM, dtype=np.float64)
        self.noisy = obj_reference(k, widths, params, x, q, max_elem, negSM, dtype=np.float64, noise=(TAU, seed))

    def part(self, idx):
        """the same case restricted to the candidates idx (errors are normwise over those)"""
        r = Reference.__new__(Reference)
        r.ld, r.f64, r.noisy = self.ld[idx], self.f64[idx], self.noisy[idx]
        return r

    @property
    def twin_err(self):
        return normwise(self.f64, self.ld)

    @property
    def noisy_err(self):
        return normwise(self.noisy, self.ld)

    @property
    def lib_allowance(self):
        return LIB_FACTOR * self.twin_err

    @property
    def fast_allowance(self):
        return FAST_FACTOR * max(self.twin_err, self.noisy_err)

    def check_lib(self, dev, what):
        e = normwise(dev, self.ld)
        print("%s: device %.3e, float64 twin %.3e, ratio %.2f (library-exp rule, limit %g)" % (what, e, self.twin_err, ratio(e, self.twin_err), LIB_FACTOR))
        assert np.all(np.isfinite(dev)) and e <= self.lib_allowance, (what, e, self.twin_err)
        return ratio(e, self.twin_err)

    def check_agree(self, dev_a, dev_b, what):
        """two fast-tansig kernels agree with each other at the level either may be off the reference"""
        e, base = normwise(dev_a, np.asarray(dev_b, dtype=LD)), max(self.twin_err, self.noisy_err)
        print("%s: difference %.3e, ratio %.2f (fast-tansig rule, limit %g)" % (what, e, ratio(e, base), FAST_FACTOR))
        assert e <= self.fast_allowance, (what, e, self.twin_err, self.noisy_err)
        return ratio(e, base)

    def check_fast(self, dev, what):
        e, base = normwise(dev, self.ld), max(self.twin_err, self.noisy_err)
        print("%s: device %.3e, float64 twin %.3e, noisy twin %.3e, ratio %.2f (fast-tansig rule, limit %g)"
              % (what, e, self.twin_err, self.noisy_err, ratio(e, base), FAST_FACTOR))
        assert np.all(np.isfinite(dev)) and e <= self.fast_allowance, (what, e, self.twin_err, self.noisy_err)
        return ratio(e, base)


def fuzz_tolerance(ref):
    """the elementwise rule of test_gpu_fuzz.py for shipped networks: 1e-9 max(|ref|, 1e-3 max|ref|) + 1e-9"""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return 1e-9 * np.maximum(ref, 1e-3 * ref.max() + 1e-12) + 1e-9


# ---- the compiled score_plan (as tests/test_score_plan.py compiles it) -----------------------------------------------------------------
PLAN_OUT = ("grid", "strip", "rr_end", "tail_nhi", "tail_hi", "tail_lo", "pf_mloc", "spread")
PLAN_WRAPPER = r"""
#include "score_plan.h"
extern "C" void plan_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + 6 * i;
        int64_t *o = out + 8 * i;
        const ScorePlan p = score_plan(a[0], (int)a[1], (int)a[2], a[3], a[4], a[5] != 0);
        o[0] = p.grid; o[1] = p.strip; o[2] = p.rr_end; o[3] = p.tail_nhi; o[4] = p.tail_hi; o[5] = p.tail_lo; o[6] = p.pf_mloc; o[7] = p.spread;
    }
}
/* the smallest n in [1, n_max] whose plan has a balanced tail on n_cu CUs, 0 if none */
extern "C" int64_t first_balanced(int n_cu, int K, int64_t n_max)
{
    for (int64_t n = 1; n <= n_max; ++n)
        if (score_plan(n, n_cu, K, n, 0, false).tail_hi > 0) return n;
    return 0;
}
"""


def compile_plan(directory):
    """csrc/score_plan.h alone behind a C wrapper -> ctypes library"""
    src = os.path.join(str(directory), "user_plan.cpp")
    so = os.path.join(str(directory), "user_plan.so")
    with open(src, "w") as f:
        f.write(PLAN_WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.first_balanced.restype = ctypes.c_int64
    lib.first_balanced.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    return lib


def plan(lib, n, n_cu, K=3):
    """score_plan of a single-class list of n candidates, not fused -> dict"""
    a = np.array([[n, n_cu, K, n, 0, 0]], dtype=np.int64)
    out = np.full((1, 8), -99, dtype=np.int64)
    P64 = ctypes.POINTER(ctypes.c_int64)
    lib.plan_batch(ctypes.c_long(1), a.ctypes.data_as(P64), out.ctypes.data_as(P64))
    return dict(zip(PLAN_OUT, (int(v) for v in out[0])))


def balanced_length(n_cu):
    """The smallest list length whose plan has a balanced tail, from the rule of score_plan: strips of 64 need n > 256 n_cu; below a
    full grid (n < 2048 n_cu) one round-robin round holds the whole list (R = 0, or rem = 0 at a multiple of 256); from there on a
    round is 2048 n_cu candidates and the tail is balanced once the rest fills 90 % of one: n = round + ceil(0.9 round)."""
    rnd = n_cu * 8 * 256
    return rnd + -(-90 * rnd // 100)


def check_plan_branches(lib, n_cu):
    """the list lengths of the GPU tests hit the branches they are chosen for on a device of n_cu CUs"""
    def last_tiles(n, p):      # 16-tiles of the last strip of a plan without a balanced tail
        return -(-(n - (n - 1) // p["strip"] * p["strip"]) // 16)
    for n in LIST_LENGTHS + ROUND_LENGTHS:
        p = plan(lib, n, n_cu)
        assert p["strip"] == 32 and p["rr_end"] == n and p["tail_hi"] == 0, (n, n_cu, p)      # strip 32: one pass per wave
    assert [n % 16 != 0 for n in LIST_LENGTHS] == [True, True, False, True, True]      # partial tiles: 1, 17, 257, 1000
    # 48 in strips of 32: a two-tile pass, then a strip of ONE tile (the single-tile pass); 17: two tiles, the second partial;
    # 257 and 1000: a last strip of one partial tile
    assert [last_tiles(n, plan(lib, n, n_cu)) for n in LIST_LENGTHS] == [1, 2, 1, 1, 1]
    p = plan(lib, STRIP64_LENGTH, n_cu)
    assert p["strip"] == 64 and p["rr_end"] == STRIP64_LENGTH and p["tail_hi"] == 0, (n_cu, p)      # strips of 64, no balanced tail
    assert STRIP64_LENGTH % 64 == 49      # its last strip: four tiles, the last with one candidate
    nb = balanced_length(n_cu)
    p, before = plan(lib, nb, n_cu), plan(lib, nb - 1, n_cu)
    assert p["strip"] == 64 and p["tail_hi"] > 0 and p["rr_end"] < nb and before["tail_hi"] == 0, (n_cu, nb, p, before)
    assert lib.first_balanced(n_cu, 3, nb) == nb, (n_cu, nb)      # ... and no shorter list has one
    assert p["tail_lo"] % 2 == 1 or p["tail_hi"] % 2 == 1      # three-tile tail strips: an odd number of tiles on strips of 64
    return nb
