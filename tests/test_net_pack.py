"""The host packing of a network into its device blob (csrc/net_pack.h: net_pack) against a numpy restatement written from
the comments of NetDev in csrc/common.h, not generated from the header.  Every operation is a copy or a multiplication by
-1/4, so the comparison is bit for bit.  CPU only: the header is plain C++."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from sdpcutsel_via_nn_amd import networks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

OK, EINVAL = 0, -1      # include/sdpcut.h
INPUT_CLAMP = 3.0       # the clamp-free kernel cuts the mapped inputs of the first layer to [-3, 3]; behind a tansig they lie in [-1, 1]
WIDTHS = (1, 7, 16, 47, 48, 49, 50, 52, 63, 64)
OFFS = ("inmap", "bias", "bias_q", "wout", "frag", "wtail", "wvalu")

WRAPPER = r"""
#include "net_pack.h"
extern "C" int pack(int k, int n_layers, const int32_t *widths, const double *params, int64_t n_params, double *blob, int64_t cap,
                    int64_t *n_blob, int64_t *offs, int32_t *ints, double *dbl, const char **why)
{
    NetPack p;
    *why = "";
    const int rc = net_pack(k, n_layers, widths, params, n_params, &p, why);
    if (rc != SDPCUT_OK) return rc;
    *n_blob = (int64_t)p.blob.size();
    if ((int64_t)p.blob.size() > cap) return -99;
    std::memcpy(blob, p.blob.data(), p.blob.size() * sizeof(double));
    const size_t o[7] = { p.o_inmap, p.o_bias, p.o_bias_q, p.o_wout, p.o_frag, p.o_wtail, p.o_wvalu };
    for (int i = 0; i < 7; ++i) offs[i] = (int64_t)o[i];
    for (int l = 0; l < n_layers; ++l) { offs[7 + l] = (int64_t)p.o_rw[l]; offs[7 + MAX_LAYERS + l] = (int64_t)p.o_rb[l]; }
    ints[0] = p.d_in; ints[1] = p.n_hidden; ints[2] = p.width; ints[3] = p.s0; ints[4] = p.sh; ints[5] = p.unclamped_ok;
    dbl[0] = p.ymin; dbl[1] = p.b_out; dbl[2] = p.y_ymin; dbl[3] = p.y_gain; dbl[4] = p.y_xoffset;
    return rc;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("net_pack")
    src = d / "pack.cpp"
    src.write_text(WRAPPER)
    so = d / "pack.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _pack(lib, k, widths, params, n_layers=None, n_params=None):
    widths = None if widths is None else np.ascontiguousarray(widths, dtype=np.int32)
    params = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    blob = np.full(1 << 16, np.nan)
    n_blob = ctypes.c_int64(-1)
    offs = np.full(17, -1, dtype=np.int64)
    ints = np.full(6, -1, dtype=np.int32)
    dbl = np.full(5, np.nan)
    why = ctypes.c_char_p()
    rc = lib.pack(int(k), int(len(widths) if n_layers is None else n_layers),
                  None if widths is None else widths.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                  None if params is None else params.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                  ctypes.c_int64(params.shape[0] if n_params is None else n_params),
                  blob.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int64(blob.shape[0]), ctypes.byref(n_blob),
                  offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                  dbl.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(why))
    assert rc != -99, "the test's blob buffer is too small"
    return rc, why.value.decode(), blob[:max(n_blob.value, 0)], offs, ints, dbl


def _split(k, widths, params):
    """params = xoffset | gain | ymin | (W row-major [out][in], b) per layer | y_ymin, y_gain, y_xoffset"""
    d_in = k * (k + 3) // 2
    o = 2 * d_in + 1
    Ws, Bs, fan = [], [], d_in
    for w in widths:
        Ws.append(params[o:o + w * fan].reshape(w, fan)); o += w * fan
        Bs.append(params[o:o + w]); o += w
        fan = w
    assert o + 3 == params.shape[0]
    return d_in, params[:d_in], params[d_in:2 * d_in], params[2 * d_in], Ws, Bs, params[o:o + 3]


def _bound(k, widths, params):
    """largest |pre-activation| a hidden unit can see: |b_j| + sum_i |W_ji| max|in_i|"""
    _, _, _, _, Ws, Bs, _ = _split(k, widths, params)
    return max(float((np.abs(B) + np.abs(W).sum(axis=1) * (INPUT_CLAMP if l == 0 else 1.0)).max())
               for l, (W, B) in enumerate(zip(Ws[:-1], Bs[:-1])))


def _domain_ok(k, widths, params):
    """does the network's own mapping v -> (v - xoffset_i) gain_i + ymin send the input domain -- x_i in [0, 1] for the first k
    inputs, q_m in [-1/k, 1/k] for the others -- into [-INPUT_CLAMP, INPUT_CLAMP]?  (Affine: the two endpoints decide.)  Only
    then is the input clamp of the clamp-free kernel inactive on the domain."""
    d_in, xoffset, gain, ymin, _, _, _ = _split(k, widths, params)
    lo = np.array([0.0] * k + [-1.0 / k] * (d_in - k))
    hi = np.array([1.0] * k + [1.0 / k] * (d_in - k))
    ends = np.concatenate([(lo - xoffset) * gain + ymin, (hi - xoffset) * gain + ymin])
    return bool(np.all(np.abs(ends) <= INPUT_CLAMP))


def _domain_margin(k, widths, params):
    """smallest distance of a mapped endpoint of the domain from +-INPUT_CLAMP (the rule is not this test's business at a tie)"""
    d_in, xoffset, gain, ymin, _, _, _ = _split(k, widths, params)
    lo = np.array([0.0] * k + [-1.0 / k] * (d_in - k))
    hi = np.array([1.0] * k + [1.0 / k] * (d_in - k))
    ends = np.concatenate([(lo - xoffset) * gain + ymin, (hi - xoffset) * gain + ymin])
    return float(np.abs(np.abs(ends) - INPUT_CLAMP).min())


def _expected(k, widths, params):
    """the blob, section by section, as the comments of NetDev describe the arrays behind its pointers"""
    d_in, xoffset, gain, ymin, Ws, Bs, tail = _split(k, widths, params)
    nh, H = len(widths) - 1, int(widths[0])
    s0, sh = -(-d_in // 4), -(-H // 4)
    parts, offs = [], {}

    def put(name, a):
        offs[name] = sum(p.shape[0] for p in parts)
        parts.append(np.ascontiguousarray(a, dtype=np.float64).ravel())

    put("inmap", np.concatenate([xoffset, gain]))                    # xoffset[d_in] | gain[d_in]
    bias = np.zeros((nh, 64))
    bias_q = np.zeros((nh, 64))
    for l in range(nh):
        bias[l, :H] = Bs[l]
        bias_q[l, :H] = -0.25 * Bs[l]
    put("bias", bias)                                                # [n_hidden][64] zero padded
    put("bias_q", bias_q)                                            # (x -1/4)
    wout = np.zeros(64)
    wout[:H] = Ws[nh][0]
    put("wout", wout)                                                # [64] zero padded output weights
    for l in range(nh + 1):                                          # row-major [out][in], then the biases, per layer
        put("rw%d" % l, Ws[l])
        put("rb%d" % l, Bs[l])
    lane = np.arange(64)
    frags = []
    for l in range(nh):                                              # layer-major, then [t][s][lane], x -1/4
        S = s0 if l == 0 else sh
        P = np.zeros((64, 4 * S))
        P[:H, :Ws[l].shape[1]] = -0.25 * Ws[l]
        t, s = np.meshgrid(np.arange(4), np.arange(S), indexing="ij")
        # lane l of an A-fragment holds A[row = l & 15][k = l >> 4] of the 16 x 4 tile (t, s)
        frags.append(P[16 * t[:, :, None] + (lane & 15), 4 * s[:, :, None] + (lane >> 4)])
    put("frag", np.concatenate([f.ravel() for f in frags]))
    wtail = np.zeros((nh, 4, 64))                                    # rows 48..51 of each hidden layer, x -1/4
    for l in range(nh):
        rows = Ws[l][48:52]
        wtail[l, :rows.shape[0], :rows.shape[1]] = -0.25 * rows
    put("wtail", wtail)
    nb = -(-H // 8)
    valu = []
    for l in range(nh):                                              # layer-major, then [j/8][i][j%8], zero padded
        P = np.zeros((nb * 8, Ws[l].shape[1]))
        P[:H] = Ws[l]
        valu.append(P.reshape(nb, 8, -1).transpose(0, 2, 1))
    put("wvalu", np.concatenate([v.ravel() for v in valu] + [np.zeros(16)]))      # + the slack of the 16-double batches
    scal = dict(d_in=d_in, n_hidden=nh, width=H, s0=s0, sh=sh, ymin=ymin, b_out=Bs[nh][0], y_ymin=tail[0], y_gain=tail[1],
                y_xoffset=tail[2])
    return np.concatenate(parts), offs, scal


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _compare(lib, k, widths, params):
    rc, why, blob, offs, ints, dbl = _pack(lib, k, widths, params)
    assert rc == OK, why
    want, woffs, scal = _expected(k, widths, params)
    tag = (k, list(widths))
    assert blob.shape == want.shape, tag
    bad = np.nonzero(_bits(blob) != _bits(want))[0]
    assert bad.size == 0, (tag, int(bad[0]), blob[bad[0]], want[bad[0]])
    assert [int(v) for v in offs[:7]] == [woffs[n] for n in OFFS], tag
    n = len(widths)
    assert [int(v) for v in offs[7:7 + n]] == [woffs["rw%d" % l] for l in range(n)], tag
    assert [int(v) for v in offs[12:12 + n]] == [woffs["rb%d" % l] for l in range(n)], tag
    assert [int(v) for v in ints[:5]] == [scal[n] for n in ("d_in", "n_hidden", "width", "s0", "sh")], tag
    assert np.array_equal(_bits(dbl), _bits([scal[n] for n in ("ymin", "b_out", "y_ymin", "y_gain", "y_xoffset")])), tag
    return int(ints[5])


def _random_network(rng, k, n_layers, H, target):
    """weights scaled so that the bound of the hidden pre-activations is `target` (up to rounding)"""
    d_in = k * (k + 3) // 2
    widths = np.array([H] * (n_layers - 1) + [1], dtype=np.int32)
    n = 2 * d_in + 1 + 3 + sum(int(w) * f + int(w) for w, f in zip(widths, [d_in] + [int(w) for w in widths[:-1]]))
    params = rng.standard_normal(n)
    params[rng.integers(0, n, size=max(n // 50, 1))] = 0.0      # exact zeros: -1/4 of them is -0.0
    hidden = slice(2 * d_in + 1, n - 3 - (H + 1))
    params[hidden] *= target / _bound(k, widths, params)
    return widths, params


def test_shipped_networks_pack_bit_for_bit(lib):
    for k in (2, 3, 4, 5):
        widths, params = networks.load_network(k)
        ok = _compare(lib, k, widths, params)
        b = _bound(k, widths, params)
        assert _domain_ok(k, widths, params) and _domain_margin(k, widths, params) > 1.0, k      # gain ~ 2, ymin -1: [0, 1] -> [-1, 1]
        if not 39.0 <= b <= 41.0:      # (at the threshold the order of the sum decides: not this test's business)
            assert ok == (1 if b < 40.0 else 0), (k, b)
        assert b < 39.0 and ok == 1, (k, b)      # the shipped networks stay on the clamp-free kernels


def test_random_networks_pack_bit_for_bit(lib):
    rng = np.random.default_rng(20261016)
    targets = itertools.cycle((0.5, 12.0, 38.5, 41.5, 90.0, 700.0))
    seen, seen_rule = set(), set()
    for k, n_layers, H in itertools.product((2, 3, 4, 5), (2, 3, 4, 5), WIDTHS):
        widths, params = _random_network(rng, k, n_layers, H, next(targets))
        b = _bound(k, widths, params)
        assert not 39.0 <= b <= 41.0, ("test set-up: a generated network lies at the threshold", k, n_layers, H, b)
        assert _domain_margin(k, widths, params) > 1e-9, ("test set-up: a mapped endpoint lies at the clamp", k, n_layers, H)
        dom = _domain_ok(k, widths, params)
        ok = _compare(lib, k, widths, params)
        assert ok == (1 if (b < 40.0 and dom) else 0), (k, n_layers, H, b, dom)
        assert bool(ok) == networks.unclamped_ok(k, widths, params), (k, n_layers, H)      # the Python twin of the rule
        seen.add(ok)
        seen_rule.add((b < 40.0, dom))
    assert seen == {0, 1}      # both outcomes occur ...
    # ... and both outcomes of EACH condition, in every combination (xoffset / gain are drawn from N(0, 1))
    assert seen_rule == {(True, True), (True, False), (False, True), (False, False)}


def test_domain_condition_alone_decides_a_bounded_network(lib):
    """a shipped network (bounded, mapping near gain 2 / ymin -1) stays clamp-free; the same weights behind a mapping trained on a
    narrower range -- the middle fifth of an input's interval, x in [0.4, 0.6]: mapminmax gives xoffset 0.4, gain 10 -- send x = 0, 1 to -5, +5 and lose the status, input
    by input and endpoint by endpoint"""
    for k in (2, 3, 4, 5):
        widths, params = networks.load_network(k)
        d_in = k * (k + 3) // 2
        assert _compare(lib, k, widths, params) == 1
        for i in (0, k - 1, k, d_in - 1):
            lo, hi = (0.0, 1.0) if i < k else (-1.0 / k, 1.0 / k)
            for gain, xoff in ((10.0 / (hi - lo), lo + 0.4 * (hi - lo)), (2.0 / (hi - lo), lo + 1.01 * (hi - lo)), (2.0 / (hi - lo), lo - 1.01 * (hi - lo))):
                p = params.copy()
                p[i], p[d_in + i] = xoff, gain
                assert _bound(k, widths, p) == _bound(k, widths, params) and not _domain_ok(k, widths, p)
                assert _compare(lib, k, widths, p) == 0, (k, i, gain, xoff)
                assert not networks.unclamped_ok(k, widths, p)
            p = params.copy()      # just inside: [lo, hi] -> [-3, 3] shrunk by 1 %
            p[i], p[d_in + i] = lo, (2.0 * INPUT_CLAMP * 0.99) / (hi - lo)
            p[2 * d_in] = -INPUT_CLAMP * 0.99
            assert _domain_ok(k, widths, p), (k, i)      # (the other inputs keep their shipped mapping: [-1, 1] - 1.97)
            assert _compare(lib, k, widths, p) == 1 and networks.unclamped_ok(k, widths, p), (k, i)


def test_refusals_keep_their_texts(lib):
    widths, params = networks.load_network(3)
    n = len(widths)

    def refused(text, k=3, w=widths, p=params, **kw):
        rc, why = _pack(lib, k, w, p, **kw)[:2]
        assert (rc, why) == (EINVAL, text), (rc, why, text)

    for k in (-1, 0, 1, 6):
        refused("k must be 2..5", k=k)
    for nl in (-1, 0, 1, 6):
        refused("bad layer description", n_layers=nl)
    refused("bad layer description", w=None, n_layers=n)
    refused("bad layer description", p=None, n_params=params.shape[0])
    last = widths.copy()
    last[-1] = 2
    refused("last layer must have one output", w=last)
    uneven = np.array([16, 15, 1], dtype=np.int32)
    refused("hidden layers must share one width <= 64", w=uneven, p=np.zeros(4096))
    for H in (0, -3, 65):
        refused("hidden layers must share one width <= 64", w=np.array([H, H, 1], dtype=np.int32), p=np.zeros(8192))
    for d in (-1, 1):
        refused("n_params does not match the layer description", n_params=params.shape[0] + d)
    assert _pack(lib, 3, widths, params)[0] == OK
