"""Networks that make ONE premise of a written derivation decisive, for test_probe_nets_cpu.py and test_gpu_probe_nets.py.  Two things
in the library are correct only because a derivation says so: the margin of the fp32 filter (csrc/net_pack.h: net_filter_layers,
net_filter_margin, net_filter_slope_terms; networks.filter_margin*) and the accuracy constants of the fp64 fast tansig
(csrc/tansig.h).  On dense networks the observed error is a random walk far below the worst-case sum, so a single premise could be
off by a large factor unseen.  Here every network has exactly one live path -- or one live accumulation chain -- and the library's
own bound becomes tight.  A plain module: no fixtures, no GPU.

The instance: Q = 0, so max_elem = 1, every q input is 0 and obj_improve is the unmapped network output; candidate i is the set
(i, .., i + k - 1) and reads x_i as its input 0.  The output mapping is the identity, the input mapping sends x in [0, 1] onto
[-x_gain / 2, x_gain / 2] (xoffset 1/2, gain x_gain, ymin 0) and q in [-1/k, 1/k] onto [-1, 1].

Family A  one fp32 activation at a time (k = 3, H = 50, three hidden layers: the shape that filters).  Links 2 and 3 are 2^-12, the
          third neuron has the bias b3: the error of the first two layers arrives divided by 2^12 and |y32 - y64| is the error of
          ONE v_exp_f32 / v_rcp_f32 activation at z = fl32(c b3) and its neighbours (the 13 u charge), plus the conversion and the
          rounding count of b3 times the slope there (a further set with link 2 = 1 spreads z over hundreds of neighbouring floats
          per network).  A second set probes layer 1 (links 2 and 3 = 1): the one-term chain
          z1 = fl32(fl32(c w1) v32) with w1 no power of two and v32 a full 24-bit significand.
Family B  the fp32 accumulation chain.  Layer 1 is saturated by biases of +-39 with zero weights (activations exactly +-1: Family A
          pins that at b3 = +-39), one neuron of layer 2 has 50 live weights and the bias that cancels their sum (z ~ 0, slope 1),
          the links behind it are 1.  Patterns: "coherent" (every term of one sign against the bias and the low bits of every
          term chosen so that a sequential fp32 chain rounds the same way at every step), "random" (random signs), "ascending" and
          "descending" (magnitudes sorted along the order the terms are consumed in).
Family C  one fp64 activation at a time, k = 2..5 at the shapes the MFMA / VALU kernels are compiled for (user_nets.SHAPES):
          clamp-free sweeps of the first pre-activation over [-39.9, 39.9] and of the last one around a bias, clamped networks
          whose first bias (up to +-700) carries the argument across y8max = 22 of tansig4 (n = -88) and 88 of tansig (n = -352),
          and "companions": the three other neurons that share the probe's reciprocal in tansig4 -- rows of the same C/D fragment
          with the same row % 4 (csrc/tansig.h: tansig_tile) -- saturated all negative, all positive or mixed with zero outgoing
          weights, which puts the product of the four half-denominators at the extremes tansig.h argues about.

The reference is networks.forward_twin(..., dtype=np.longdouble); for a one-path network that is the closed form
T(w_L T(.. T(w_1 v + b_1) ..) + b_L) (closed_form below; test_probe_nets_cpu.py holds the two equal)."""
import numpy as np

import user_nets
from sdpcutsel_via_nn_amd import networks

LD = np.longdouble
U = 2.0 ** -24                       # unit roundoff of fp32
EPS = 2.0 ** -53                     # ... of fp64
C = networks.FILTER_EXP_SCALE        # -2 log2(e)
CHARGE = 13.0                        # u per fp32 activation (net_pack.h)
L2 = 4.0 / (3.0 * np.sqrt(3.0))      # max |tansig''|
FILTER_SHAPE = (3, 50, 3)            # k, H, hidden layers

# rows of a hidden layer of 50: first and last row of every 16-row tile on the matrix core, a row of each register slot of a C/D
# fragment (fp32: register i of lane (q, c) is row 4 q + i, so rows 0..3 are the four slots of q = 0), and the two tail rows
ROWS_MFMA = (0, 1, 2, 3, 15, 16, 31, 32, 47)
ROWS_TAIL = (48, 49)
W1 = 0.7390851332151607              # the first link: no power of two, its scaled fp32 form has a full significand
LINK = 2.0 ** -12

# per-activation bounds of the fp64 kernels (csrc/tansig.h).  tansig / tansig_y8: "absolute error vs the exact formula <= 1e-15".
# tansig4: the same formula through a shared reciprocal whose extra roundings "stay below 5e-16 relative" of 1 / h <= 2, so 1e-15
# more.  The library route 2 / (exp(-2n) + 1) - 1 with exp to 1 ulp: the sensitivity of the formula to exp is 2E / (1 + E)^2 <= 1/2
# (2^-52 / 2), the add and the division each move 2 / (1 + E) <= 2 by 2^-53 relative, the subtraction rounds a value <= 1: 6 x 2^-53.
ACT_BOUND = {"tansig": 1e-15, "tansig4": 2e-15, "lib": 6.0 * EPS}
KERNEL_ACT = {"mfma": "tansig4", "valu": "tansig", "simple": "lib", "nn_batch": "lib"}


class Net(object):
    """one probe network: widths / params in set_network's layout and what the tests need to know about it"""

    def __init__(self, name, k, widths, params, **meta):
        self.name, self.k, self.widths, self.params = name, k, widths, params
        self.path = None                 # (rows, links, biases) of a one-path network
        self.x_gain = None
        self.__dict__.update(meta)

    @property
    def net(self):
        return self.widths, self.params


# ---- construction -------------------------------------------------------------------------------------------------------------
def blank(k, H, nh, x_gain):
    """every weight and bias zero, the mappings as the module docstring gives them -> (widths, params, Ws, Bs): views of params"""
    if not 0.0 < x_gain <= 6.0:
        raise ValueError("x_gain must be in (0, 6]: the domain condition of unclamped_ok")
    d_in = k * (k + 3) // 2
    widths = np.array([H] * nh + [1], dtype=np.int32)
    n_w = sum(int(w) * f + int(w) for w, f in zip(widths, [d_in] + [H] * nh))
    params = np.zeros(2 * d_in + 1 + n_w + 3)
    params[:k] = 0.5
    params[d_in:d_in + k] = float(x_gain)
    params[d_in + k:2 * d_in] = float(k)
    params[-3:] = (0.0, 1.0, 0.0)      # y_ymin, y_gain, y_xoffset: the identity
    _, _, _, Ws, Bs, _ = networks.split_params(k, widths, params)
    return widths, params, Ws, Bs


def companion_rows(H, row):
    """the rows whose tansig shares a reciprocal with `row` in the MFMA kernel: register r of a C/D fragment of
    v_mfma_f64_16x16x4_f64 is row 16 t + 4 r + q (csrc/tansig.h: tansig_tile), so the four registers of a lane are the rows of tile
    t with the same row % 4.  None where the row's tile is a tail tile (<= 4 live rows: one tansig_y8 per neuron on the VALU)."""
    t = row // 16
    live = min(H - 16 * t, 16)
    if live <= 4:
        return None
    return [r for r in range(16 * t + row % 4, 16 * t + 16, 4) if r != row and r < H]


COMPANIONS = {"negative": (-1.0, -1.0, -1.0), "positive": (1.0, 1.0, 1.0), "mixed": (1.0, -1.0, 1.0)}


def one_path(k, H, nh, rows, links, biases, x_gain, companions=None, companion_bias=39.9):
    """-> (widths, params): every weight and bias zero except the link input 0 -> neuron rows[0] of layer 1 -> .. -> neuron
    rows[nh - 1] (links[l] into layer l + 1), the biases on that path and output weight 1 on the last neuron.  companions (a key
    of COMPANIONS): the rows that share a reciprocal with each path neuron get biases of +-companion_bias, no weights in or out."""
    if not (len(rows) == len(links) == len(biases) == nh):
        raise ValueError("one row, link and bias per hidden layer")
    widths, params, Ws, Bs = blank(k, H, nh, x_gain)
    prev = 0
    for l in range(nh):
        Ws[l][rows[l], prev] = links[l]
        Bs[l][rows[l]] = biases[l]
        if companions is not None:
            comp = companion_rows(H, rows[l])
            for r, s in zip(comp or [], COMPANIONS[companions]):
                Bs[l][r] = s * companion_bias
        prev = rows[l]
    Ws[nh][0, prev] = 1.0
    networks.check_network(k, widths, params)
    return widths, params


def tansig_ld(n):
    n = np.asarray(n, dtype=LD)
    with np.errstate(over="ignore"):
        return LD(2) / (LD(1) + np.exp(LD(-2) * n)) - LD(1)


def closed_form(p, x):
    """the long double output of the one-path network p (a Net with .path) on first inputs x: T(w_L T(.. T(w_1 v + b_1)) + b_L)"""
    rows, links, biases = p.path
    a = (np.asarray(x, dtype=LD) - LD(0.5)) * LD(p.x_gain)
    for w, b in zip(links, biases):
        a = tansig_ld(a * LD(w) + LD(b))
    return a


def path_activations(p, x):
    """the long double pre-activations and activations along the path -> [(n_l, a_l)]"""
    rows, links, biases = p.path
    a = (np.asarray(x, dtype=LD) - LD(0.5)) * LD(p.x_gain)
    out = []
    for w, b in zip(links, biases):
        n = a * LD(w) + LD(b)
        a = tansig_ld(n)
        out.append((n, a))
    return out


# ---- the probe instance -----------------------------------------------------------------------------------------------------------
def instance(k, count):
    """-> (n_vars, Q_arr = 0, sets [count, k]: candidate i = (i, .., i + k - 1))"""
    n = count + k - 1
    sets = (np.arange(count)[:, None] + np.arange(k)[None, :]).astype(np.int32)
    return n, np.zeros(n * (n + 1) // 2), sets


def point(n, x_first):
    """the LP point [X packed | x] with x_i = x_first[i] (1/2 behind them) and X = x x^T with 0.05 taken off the diagonal: every
    candidate is violated (lambda_min <= -0.05 + ..), and with Q = 0 no score reads X"""
    x = np.full(n, 0.5)
    x[:len(x_first)] = x_first
    X = np.outer(x, x)
    d = np.arange(n)
    X[d, d] -= 0.05
    return np.concatenate([X[np.triu_indices(n)], x])


def inputs_of(k, sets, vv, n):
    """the network's inputs [count, d_in] of every candidate: [x | q = 0]"""
    L = n * (n + 1) // 2
    return np.concatenate([vv[L:][sets], np.zeros((sets.shape[0], k * (k + 1) // 2))], axis=1)


def grid_f32(count, gain, seed, emin=-6):
    """x in [0, 1] whose mapped value v = (x - 1/2) gain is exact in fp32 with a full 24-bit significand (lowest bit set):
    v = +-(1 + m 2^-23) 2^e, m odd, e in emin .. log2(gain) - 2 -> (x float64 [count], v float64 [count])"""
    if gain not in (1.0, 2.0, 4.0):
        raise ValueError("a power-of-two gain")
    rng = np.random.default_rng(seed)
    emax = int(np.log2(gain)) - 2
    e = rng.integers(emin, emax + 1, count)
    m = 2 * rng.integers(0, 2 ** 22, count) + 1
    v = rng.choice([-1.0, 1.0], count) * (1.0 + m * 2.0 ** -23) * 2.0 ** e
    x = v / gain + 0.5
    assert np.all((x - 0.5) * gain == v) and np.all(v.astype(np.float32).astype(np.float64) == v) and np.all((x >= 0) & (x <= 1))
    return x, v


def grid_dyadic(count):
    """x = i / (count - 1), count - 1 a power of two: both ends of the domain, and (x - 1/2) x_gain is exact in fp64"""
    assert (count - 1) & (count - 2) == 0
    return np.arange(count) / float(count - 1)


def predict_z1(w1, v):
    """what the fp32 pass holds in front of the first activation of a one-term path: z1 = fl32(fl32(c w1) v32).  The accumulator
    starts as the bias, an exact 0, and every other term adds an exact 0: ONE rounding, that of the product."""
    wt = np.float32(C * w1)
    return (wt * np.asarray(v, dtype=np.float32)).astype(np.float32)


# ---- the derivation of net_pack.h (lines 45 - 79), restated premise by premise ---------------------------------------------------------
def gamma(m):
    return m * U / (1.0 - m * U)


def rounding_counts(l, fan, H=50):
    """-> (m [H, fan], mb [H]): the roundings term j and the bias see in row i of hidden layer l (0 = the input layer) of a network
    of the filtering shape.  Rows 0..47: the chain of v_mfma_f32_16x16x4_f32, the bias enters as C and sees one rounding per
    (counted) term, `fan`; a term sees fan - (the terms in front of the FIRST of its k-step).  The k-steps: inputs 4 s .. 4 s + 3 in
    the input layer; neurons {16 t + 4 q + i, q = 0..3} for (t, i) in order, then ONE k-step with neurons 48, 49, behind it.
    Tail rows 48, 49: lane q chains [bias on q = 0], the tail neuron 48 + q of the layer in front, then its twelve terms
    j = 16 tk + 4 q + i in the order of 4 tk + i, and the four lanes are summed by a two-level tree: term j < 48 sees
    12 - (4 tk + i) + 2, terms 48, 49 and the bias 1 + 12 + 2.  Input layer: lane q chains inputs q, 4 + q, ..: live - j / 4 + 2,
    the bias ceil(fan / 4) + 2."""
    j = np.arange(fan)
    if l == 0:
        before = 4 * (j // 4)
        m_tail = (fan - j % 4 + 3) // 4 - j // 4 + 2
        mb_tail = (fan + 3) // 4 + 2
    else:
        before = np.zeros(fan, dtype=np.int64)
        cnt = 0
        for t in range(3):
            for i in range(4):
                before[[16 * t + 4 * q + i for q in range(4)]] = cnt
                cnt += 4
        before[48:] = 48
        m_tail = np.where(j < 48, 12 - (4 * (j // 16) + j % 4) + 2, 15)
        mb_tail = 15
    m = np.tile(fan - before, (H, 1))
    mb = np.full(H, fan)
    m[48:] = m_tail
    mb[48:] = mb_tail
    return m, mb


def premise_layers(p, charge=CHARGE, saturated_exact=False):
    """The bound of net_filter_layers on a network of the filtering shape, from its premises -> [(delta [H], e [H])] per hidden layer:
    delta the bound on |z / c - n|, e = delta + charge u that on the activation.
      delta_i = ( sum_j |w~_ij| A_j gamma(m_ij) + |b~_i| gamma(mb_i) + sum_j |w~_ij - c W_ij| A_j + |b~_i - c b_i|
                  + |c| sum_j |W_ij| e_j ) / |c|
    with w~ = fl32(c W), b~ = fl32(c b); inputs e_j = u B_j, A_j = (1 + u) B_j, B_j the larger endpoint of filter_box; behind a
    tansig A_j = 1 + 8 u.  saturated_exact: a neuron without weights whose |bias| is >= 39 counts as exactly +-1 (e = 0, A = 1),
    the premise Family B builds on."""
    k, H, nh = FILTER_SHAPE
    assert p.k == k and [int(w) for w in p.widths] == [H] * nh + [1]
    params = np.asarray(p.params, dtype=np.float64)
    _, _, _, Ws, Bs, _ = networks.split_params(k, p.widths, params)
    Bx = np.abs(networks.filter_box(k, p.widths, params)).max(axis=1)
    e, A = U * Bx, (1.0 + U) * Bx
    out = []
    for l in range(nh):
        W, b = Ws[l], Bs[l]
        m, mb = rounding_counts(l, W.shape[1])
        wt = (C * W).astype(np.float32).astype(np.float64)
        bt = (C * b).astype(np.float32).astype(np.float64)
        acc = np.abs(bt) * gamma(mb) + np.abs(bt - C * b)
        acc = acc + (np.abs(wt) * A * gamma(m) + np.abs(wt - C * W) * A + np.abs(C * W) * e).sum(axis=1)
        delta = acc / abs(C)
        e = delta + charge * U
        A = np.full(H, 1.0 + 8.0 * U)
        if saturated_exact:
            sat = (np.abs(W).sum(axis=1) == 0.0) & (np.abs(b) >= 39.0)
            e = np.where(sat, 0.0, e)
            A = np.where(sat, 1.0, A)
        out.append((delta, e))
    return out


def premise_bound(p, charge=CHARGE, saturated_exact=True):
    """the bound on |y32 - y64| the premises give for p: sum_j |Wout_j| e_j of the last hidden layer, times the 1 + 2^-10 of the
    a-priori margin (the fp64 roundings of the derivation and of the epilogue, terms of second order in u); y_gain is 1"""
    _, _, _, Ws, _, _ = networks.split_params(p.k, p.widths, np.asarray(p.params, dtype=np.float64))
    e = premise_layers(p, charge, saturated_exact)[-1][1]
    return float((np.abs(Ws[-1][0]) * e).sum() * (1.0 + 2.0 ** -10))


# ---- Family A ---------------------------------------------------------------------------------------------------------------------
A_COUNT = 1024
A_GAIN = 4.0
LN2H = 0.5 * np.log(2.0)
# b3: 0, +-m ln2 / 2 (2^z = 2^-+m: the powers of two), moderate values, saturation, and just inside the limit of unclamped_ok
# (|b3| + 2^-12 < 40): |z| up to 115.1
B3_GRID = tuple(sorted(set([0.0] + [s * v for s in (-1.0, 1.0) for v in
                                   [m * LN2H for m in range(1, 11)] + [0.1, 0.5, 2.0, 3.0, 5.0, 7.0, 10.0, 15.0, 20.0, 25.0, 30.0,
                                                                       35.0, 39.0, 39.9]])))
Z_BUCKETS = (0.0, 1.0, 8.0, 32.0, 64.0, 116.0)      # |z| of the probed activation: the buckets the device's error is recorded in


def bucket(z):
    """index into Z_BUCKETS of |z|: 0 for z = 0, i for Z_BUCKETS[i - 1] < |z| <= Z_BUCKETS[i]"""
    return int(np.searchsorted(Z_BUCKETS, abs(z), side="left"))


def mfma_row_admits(b3):
    """On rows 0..47 the bias sees fan = 50 roundings, on a tail row 15: the margin of a candidate is about
    (13 + m |b3| (1 - tansig(b3)^2)) u.  The cap of the tests, 26 u, admits a bias on a matrix-core row where 50 |b3| slope stays
    below 11 (two u of room for the conversion of b3 and the factors of the margin); a tail row admits every b3."""
    t = np.tanh(b3)
    return 50.0 * abs(b3) * (1.0 - t * t) <= 11.0


def _path_net(name, family, k, H, nh, rows, links, biases, x_gain, **kw):
    companions = kw.pop("companions", None)
    companion_bias = kw.pop("companion_bias", 39.9)
    widths, params = one_path(k, H, nh, rows, links, biases, x_gain, companions, companion_bias)
    return Net(name, k, widths, params, family=family, path=(tuple(rows), tuple(links), tuple(biases)), x_gain=x_gain,
               companions=companions, **kw)


def family_a3():
    """the probe on layer 3: every b3 of B3_GRID on a tail row (48 and 49 in turn), and on every row of ROWS_MFMA those b3 the
    cap admits there; the rows of layers 1 and 2 walk through all the rows as well"""
    k, H, nh = FILTER_SHAPE
    rows_all = ROWS_MFMA + ROWS_TAIL
    nets = []
    for i, b3 in enumerate(B3_GRID):
        rows = (rows_all[i % len(rows_all)], rows_all[(3 * i + 1) % len(rows_all)], ROWS_TAIL[i % 2])
        nets.append(_path_net("A3 b3 %+.4g rows %s" % (b3, rows), "A3", k, H, nh, rows, (W1, LINK, LINK), (0.0, 0.0, b3), A_GAIN, b3=b3))
    admitted = [b for b in B3_GRID if mfma_row_admits(b)]
    for i, r in enumerate(ROWS_MFMA):
        for s in range(4):
            b3 = admitted[(4 * i + s) * 5 % len(admitted)]
            rows = (rows_all[(i + s + 5) % len(rows_all)], rows_all[(2 * i + s) % len(rows_all)], r)
            nets.append(_path_net("A3 b3 %+.4g rows %s" % (b3, rows), "A3", k, H, nh, rows, (W1, LINK, LINK), (0.0, 0.0, b3), A_GAIN, b3=b3))
    return nets


def family_a3_wide():
    """Beside the set above, not in its place: the same probe with link 2 = 1, every b3 of B3_GRID on a tail row.  The third
    pre-activation is then b3 + 2^-12 tansig(tansig(w1 v)) and z3 runs over hundreds of neighbouring floats on both sides of
    fl32(c b3) across the list, where links of 2^-12 twice move it by an ulp or two at most.  What layers 1 and 2 contribute
    still arrives divided by 2^12: the margin per candidate stays what it is above."""
    k, H, nh = FILTER_SHAPE
    rows_all = ROWS_MFMA + ROWS_TAIL
    nets = []
    for i, b3 in enumerate(B3_GRID):
        rows = (rows_all[(i + 3) % len(rows_all)], rows_all[(5 * i + 2) % len(rows_all)], ROWS_TAIL[(i + 1) % 2])
        nets.append(_path_net("A3w b3 %+.4g rows %s" % (b3, rows), "A3w", k, H, nh, rows, (W1, 1.0, LINK), (0.0, 0.0, b3), A_GAIN, b3=b3))
    return nets


A1_LINKS = (13.0, -7.3, 3.1, -1.37, 0.61, W1)


def family_a1():
    """the probe on layer 1: link 1 of magnitude up to 13 (|w1| 3 < 40), links 2 and 3 = 1, no biases; rows[0] on every row"""
    k, H, nh = FILTER_SHAPE
    rows_all = ROWS_MFMA + ROWS_TAIL
    nets = []
    for i, r in enumerate(rows_all):
        w1 = A1_LINKS[i % len(A1_LINKS)]
        rows = (r, rows_all[(i + 4) % len(rows_all)], rows_all[(i + 7) % len(rows_all)])
        nets.append(_path_net("A1 w1 %+.4g rows %s" % (w1, rows), "A1", k, H, nh, rows, (w1, 1.0, 1.0), (0.0, 0.0, 0.0), A_GAIN, b3=0.0))
    return nets


def a_points():
    """-> (n, Q, sets, vv, inputs, x, v) of the Family A list: 1024 candidates, x on grid_f32"""
    n, Q, sets = instance(3, A_COUNT)
    x, v = grid_f32(A_COUNT, A_GAIN, seed=11)
    vv = point(n, x)
    return n, Q, sets, vv, inputs_of(3, sets, vv, n), x, v


def round_net():
    """the network of the round check: Family A's path with b3 = 0 and link 2 raised to 2^-6, so that the measure
    y = tansig(2^-12 tansig(2^-6 tansig(w1 v))) ~ 2^-18 a1 runs over +-64 u across the list -- both sides of 0, and both sides of
    one and of two margins of about 13 u below it.  (With link 2 = 2^-12 every measure would lie within 1 u of 0 and nothing could drop; the
    layers in front still arrive divided by 2^12.)"""
    k, H, nh = FILTER_SHAPE
    return _path_net("round check", "A3", k, H, nh, (5, 48, 49), (W1, 2.0 ** -6, LINK), (0.0, 0.0, 0.0), A_GAIN, b3=0.0)


def round_points():
    """as a_points with |v| >= 1/16: no measure within 1e-9 of zero (the tie allowance of the round helper)"""
    n, Q, sets = instance(3, A_COUNT)
    x, v = grid_f32(A_COUNT, A_GAIN, seed=12, emin=-4)
    vv = point(n, x)
    return n, Q, sets, vv, inputs_of(3, sets, vv, n), x, v


# ---- Family B ---------------------------------------------------------------------------------------------------------------------
B_COUNT = 32
B_PATTERNS = ("coherent", "random", "ascending", "descending")
B_ROWS = (5, 37, 48, 49)      # the probed row of layer 2: two on the matrix core, the two tail rows
B_SEEDS = (0, 1, 2)


def consumption_order(row):
    """the order in which the 50 terms of hidden row `row` are consumed.  Matrix-core rows: k-step by k-step, (t, i) in order with
    q = 0..3 inside, the tail k-step (48, 49) last.  Tail rows: link by link of the lane chains (the head links 48, 49 first, then
    4 tk + i = 0..11 with q = 0..3 inside)."""
    body = [16 * t + 4 * q + i for t in range(3) for i in range(4) for q in range(4)]
    return body + [48, 49] if row < 48 else [48, 49] + body


def emulate_chain(row, wt, a, bt, pick=None):
    """A float32 emulation of hidden row `row` of the fp32 pass in the order net_pack.h documents, one rounding per term (a chain of
    correctly rounded fmas; inside a k-step q = 0..3 in turn) -> z float32.  wt [50] float32 scaled weights, a [50] float32
    activations of the layer in front, bt the scaled bias.  pick(acc, j) -> float32, where given, chooses wt[j] on the way."""
    wt = np.array(wt, dtype=np.float32)
    a = np.asarray(a, dtype=np.float32)

    def link(acc, j):
        if pick is not None:
            wt[j] = pick(acc, j)
        # fma: the product of two floats is exact in float64, the sum of it and a float is rounded once (to float64 first, which
        # is exact here: the terms of these probes lie within 2^29 of each other)
        return np.float32(np.float64(wt[j]) * np.float64(a[j]) + np.float64(acc))

    if row < 48:
        acc = np.float32(bt)
        for j in consumption_order(row):
            acc = link(acc, j)
        return acc, wt
    lanes = []
    for q in range(4):
        p = np.float32(bt) if q == 0 else np.float32(0.0)
        if q < 2:
            p = link(p, 48 + q)
        for tk in range(3):
            for i in range(4):
                p = link(p, 16 * tk + 4 * q + i)
        lanes.append(p)
    return np.float32(np.float32(lanes[0] + lanes[1]) + np.float32(lanes[2] + lanes[3])), wt


def family_b_net(pattern, row, seed):
    """-> Net with .chain = (row, W2 row [50] float64, s [50] the saturated activations +-1, b2)"""
    k, H, nh = FILTER_SHAPE
    rng = np.random.default_rng(1000 * B_PATTERNS.index(pattern) + 10 * row + seed)
    widths, params, Ws, Bs = blank(k, H, nh, A_GAIN)
    s = rng.choice([-1.0, 1.0], H)
    Bs[0][:] = 39.0 * s
    order = consumption_order(row)
    if pattern == "coherent":
        # the scaled bias first, then every scaled weight a float32 chosen on the way down the emulated chain: among the 64
        # float32 neighbours above a base near 1.07 the one whose addition loses the most in ONE direction (computed below exact).  W = w~ / c is then
        # converted back to exactly w~, and the terms sum to about -b~.
        base = np.float32(rng.uniform(1.04, 1.09))
        bt = np.float32(-50.0 * base)
        cand = (base + np.arange(64, dtype=np.float32) * np.float32(2.0 ** -23)).astype(np.float32)

        def pick(acc, j):
            exact = np.float64(acc) + cand.astype(np.float64)
            lost = exact - (np.float32(acc) + cand).astype(np.float32).astype(np.float64)
            return np.float32(s[j]) * cand[int(np.argmax(lost))]      # times a_j = s_j: the term itself is +cand

        _, wt = emulate_chain(row, np.zeros(H, dtype=np.float32), s, bt, pick)
        w = wt.astype(np.float64) / C
        b2 = float(bt) / C
    else:
        mag = rng.uniform(0.15, 0.6, H)      # sum ~ 19
        if pattern in ("ascending", "descending"):
            mag = np.sort(mag)[::-1 if pattern == "descending" else 1]
            mag = mag[np.argsort(order)]      # position of term j in the order -> its magnitude
            sign = np.ones(H)
        else:
            sign = rng.choice([-1.0, 1.0], H)
        w = sign * mag * s                    # the term w_j a_j = sign_j mag_j
        b2 = -float((w * s).sum())
    assert abs(b2) + np.abs(w).sum() < 40.0
    Ws[1][row, :] = w
    Bs[1][row] = b2
    r3 = (row + 11) % 48
    Ws[2][r3, row] = 1.0
    Ws[3][0, r3] = 1.0
    networks.check_network(k, widths, params)
    return Net("B %s row %d seed %d" % (pattern, row, seed), k, widths, params, family="B", pattern=pattern,
               chain=(row, w.copy(), s.copy(), b2), x_gain=A_GAIN)


def family_b():
    return [family_b_net(p, r, s) for p in B_PATTERNS for r in B_ROWS for s in B_SEEDS]


def chain_error(p):
    """-> (|z / c - n| of the emulated chain of p, the chain's own share of the premise-level bound: delta of that neuron with
    e_j = 0, A_j = 1) in units of u"""
    row, w, s, b2 = p.chain
    wt = (C * w).astype(np.float32)
    bt = np.float32(C * b2)
    z, _ = emulate_chain(row, wt, s, bt)
    n = (w.astype(LD) * s.astype(LD)).sum() + LD(b2)
    delta = premise_layers(p, saturated_exact=True)[1][0][row]
    return float(abs(LD(z) / LD(C) - n)) / U, float(delta) / U


def b_points():
    n, Q, sets = instance(3, B_COUNT)
    x, v = grid_f32(B_COUNT, A_GAIN, seed=13)
    vv = point(n, x)
    return n, Q, sets, vv, inputs_of(3, sets, vv, n)


# ---- Family C ---------------------------------------------------------------------------------------------------------------------
C_COUNT = 1025
C_GAIN = 6.0
C_W1 = 13.3                           # 13.3 x 3 = 39.9
C_LAST_BIASES = (0.0, 1.0, -5.0, 10.0, -20.0, 30.0, -38.9)
C_CLAMPED_BIASES = (-88.0, 88.0, -352.0, 352.0, -700.0, 700.0)
N_BUCKETS = (0.0, 1.0, 5.0, 20.0, 40.0, 100.0, 1000.0)      # |n| of the probed activation


def c_rows(H, nh, which):
    """three placements of the path: rows on the matrix core, tile borders, and the last rows below H (the tail rows at H = 50)"""
    base = {0: (0, 17, 34, 7), 1: (15, 32, 47, 16), 2: (H - 1, H - 2, H - 1, H - 2)}[which]
    return base[:nh]


def family_c(k):
    """-> (clamp-free nets, clamped nets) of size class k"""
    H, nh = user_nets.SHAPES[k]
    ones, zeros = (1.0,) * (nh - 1), (0.0,) * (nh - 1)
    free, clamped = [], []
    for which in range(3):
        rows = c_rows(H, nh, which)
        for comp in (None,) + tuple(COMPANIONS):
            free.append(_path_net("C k %d rows %s sweep of layer 1, companions %s" % (k, rows, comp), "C", k, H, nh, rows,
                                  (C_W1,) + ones, (0.0,) * nh, C_GAIN, companions=comp, probe=0))
        free.append(_path_net("C k %d rows %s fine sweep of layer 1" % (k, rows), "C", k, H, nh, rows, (2.7,) + ones, (0.0,) * nh,
                              C_GAIN, probe=0))
        for i, b in enumerate(C_LAST_BIASES):
            comp = (None,) + tuple(COMPANIONS)
            free.append(_path_net("C k %d rows %s last layer at %+g, companions %s" % (k, rows, b, comp[i % 4]), "C", k, H, nh, rows,
                                  (1.0,) * nh, zeros + (b,), C_GAIN, companions=comp[i % 4], probe=nh - 1))
    for which in (0, 2):
        rows = c_rows(H, nh, which)
        for i, b in enumerate(C_CLAMPED_BIASES):
            for comp in COMPANIONS:
                clamped.append(_path_net("C k %d rows %s clamped, b1 %+g, companions %s" % (k, rows, b, comp), "C", k, H, nh, rows,
                                         (C_W1,) + ones, (b,) + zeros, C_GAIN, companions=comp, companion_bias=700.0, probe=0))
    return free, clamped


def c_points(k):
    n, Q, sets = instance(k, C_COUNT)
    x = grid_dyadic(C_COUNT)
    vv = point(n, x)
    return n, Q, sets, vv, inputs_of(k, sets, vv, n), x


def c_allowance(p, x, kernel):
    """The allowance on |obj - reference| of one-path network p for every first input x under `kernel` (a key of KERNEL_ACT): the
    sum over the path's activations of the documented per-activation bound times the Lipschitz product behind it, plus a few fp64
    eps for the affine steps.  Along the path, with E_0 = 0 (the mapped input (x - 1/2) x_gain is exact: x is dyadic):
        dn_l = |w_l| E_(l-1) + 2 eps (|w_l a_(l-1)| + |b_l|)      what reaches pre-activation l: the error behind it through the
                                                                   link, the rounding of the product and that of the sum
        E_l  = (1 - a_l^2 + L2 dn_l) dn_l + ACT                    tansig' = 1 - tansig^2 at the reference's a_l, the mean value
                                                                   theorem with L2 = max |tansig''| for the segment, and the
                                                                   kernel's documented bound ACT_BOUND on one activation
    and the allowance is E_L + 2 eps |y| (output weight 1, no output bias, the identity mapping; obj = -0 + y 1).  Every other term
    of every dot product is an exact zero.  The MFMA kernel is charged the tansig4 bound on every row (its tail rows run tansig_y8,
    whose bound is smaller)."""
    act = ACT_BOUND[KERNEL_ACT[kernel]]
    rows, links, biases = p.path
    E = np.zeros(len(x))
    a_prev = np.abs(((np.asarray(x, dtype=LD) - LD(0.5)) * LD(p.x_gain)).astype(np.float64))
    for (n, a), w, b in zip(path_activations(p, x), links, biases):
        a = np.abs(a.astype(np.float64))
        dn = abs(w) * E + 2.0 * EPS * (abs(w) * a_prev + abs(b))
        E = (1.0 - a * a + L2 * dn) * dn + act
        a_prev = a
    return E + 2.0 * EPS * a_prev
