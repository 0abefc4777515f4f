"""The margin of the fp32 filter (csrc/net_pack.h: net_filter_margin, restated in sdpcutsel_via_nn_amd/networks.py).  CPU only:
the header is plain C++ and is compiled with the host compiler, as tests/test_net_pack.py does.

What is checked here: the numpy restatement against the C side, which networks filter, the packed fp32 weights, and an ORDER OF
MAGNITUDE check of the bound with a float32 numpy emulation.  numpy accumulates a dot product in another order than the matrix
cores do and its exp is not v_exp_f32: this is a sanity check, not the proof.  The bound on the real instructions and the real
accumulation order is checked on the device, through sdpcut_filter_audit (tests/test_gpu_fp32_filter.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sdpcutsel_via_nn_amd import networks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

WRAPPER = r"""
#include "net_pack.h"
extern "C" int filter(int k, int n_layers, const int32_t *widths, const double *params, int64_t n_params, double *margin, int32_t *ok,
                      double *box, float *f32, int64_t cap, int64_t *n_f32, int64_t *offs)
{
    NetPack p;
    const char *why = "";
    const int rc = net_pack(k, n_layers, widths, params, n_params, &p, &why);
    if (rc != SDPCUT_OK) return rc;
    *margin = p.filter_margin;
    *ok = p.filter_ok;
    for (int i = 0; i < p.d_in; ++i) { box[2 * i] = p.filter_box[i][0]; box[2 * i + 1] = p.filter_box[i][1]; }
    *n_f32 = (int64_t)p.f32.size();
    if ((int64_t)p.f32.size() > cap) return -99;
    for (size_t i = 0; i < p.f32.size(); ++i) f32[i] = p.f32[i];
    offs[0] = (int64_t)p.o32_in; offs[1] = (int64_t)p.o32_hid; offs[2] = (int64_t)p.o32_bias;
    return rc;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_margin")
    src = d / "filter.cpp"
    src.write_text(WRAPPER)
    so = d / "filter.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _c_side(lib, k, widths, params):
    widths = np.ascontiguousarray(widths, dtype=np.int32)
    params = np.ascontiguousarray(params, dtype=np.float64)
    margin, ok, n_f32 = ctypes.c_double(-1.0), ctypes.c_int32(-1), ctypes.c_int64(-1)
    box = np.full(40, np.nan)
    f32 = np.full(1 << 14, np.nan, dtype=np.float32)
    offs = np.full(3, -1, dtype=np.int64)
    rc = lib.filter(int(k), int(widths.shape[0]), widths.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                    params.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int64(params.shape[0]), ctypes.byref(margin),
                    ctypes.byref(ok), box.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                    f32.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_int64(f32.shape[0]), ctypes.byref(n_f32),
                    offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    assert rc == 0, rc
    d_in = k * (k + 3) // 2
    return margin.value, bool(ok.value), box[:2 * d_in].reshape(d_in, 2), f32[:n_f32.value], offs


def test_margins_of_the_shipped_networks(lib):
    for k in (2, 3, 4, 5):
        widths, params = networks.load_network(k)
        m = networks.filter_margin(k, widths, params)
        assert np.isfinite(m) and m > 0.0, (k, m)
        cm, ok, box, f32, _ = _c_side(lib, k, widths, params)
        # the same formula in the same order of operations up to numpy's sums: far inside the 2 % asked for
        assert abs(cm - m) <= 1e-9 * m, (k, cm, m)
        assert np.array_equal(box, networks.filter_box(k, widths, params)), k
        assert ok == networks.filter_ok(k, widths, params) == (k == 3), (k, ok, m)
        assert (f32.shape[0] > 0) == ok
    # the 3-variable network filters with a margin of a few hundredths of y; the 5-variable one (four hidden layers of 64) would
    # need about 1: useless, it must not filter
    assert 0.01 < networks.filter_margin(3, *networks.load_network(3)) < networks.FILTER_MARGIN_CUTOFF
    assert networks.filter_margin(5, *networks.load_network(5)) > 0.5


def test_what_does_not_filter(lib):
    widths, params = networks.load_network(3)
    _, offs, _ = networks.check_network(3, widths, params)
    # output weights twice as large: twice the margin, above the cut-off; still clamp-free
    p = params.copy()
    p[offs[3][0]:offs[3][1]] *= 2.0
    assert networks.unclamped_ok(3, widths, p) and not networks.filter_ok(3, widths, p)
    cm, ok, _, f32, _ = _c_side(lib, 3, widths, p)
    assert not ok and f32.shape[0] == 0 and cm >= networks.FILTER_MARGIN_CUTOFF
    # not clamp-free (a mapping trained on a narrower range): the margin may be small, the network still does not filter
    p = params.copy()
    p[0], p[9] = 0.4, 10.0
    assert not networks.unclamped_ok(3, widths, p) and not networks.filter_ok(3, widths, p)
    assert not _c_side(lib, 3, widths, p)[1]
    # another shape
    w2 = np.array([50, 50, 1], dtype=np.int32)
    p2 = np.concatenate([params[:offs[1][1] + 50], params[offs[3][0]:]])
    networks.check_network(3, w2, p2)
    assert not networks.filter_ok(3, w2, p2) and not _c_side(lib, 3, w2, p2)[1]


def test_packed_fp32_weights(lib):
    """the A-fragments in the k-order the C/D fragment of the layer in front imposes, scaled by -2 log2(e), rounded once"""
    widths, params = networks.load_network(3)
    _, _, _, Ws, Bs, _ = networks.split_params(3, widths, params)
    _, ok, _, f32, offs = _c_side(lib, 3, widths, params)
    assert ok and list(offs) == [0, 4 * 64 * 4, 4 * 64 * 4 + 2 * 4 * 4 * 64 * 4] and f32.shape[0] == offs[2] + 3 * 64
    c = networks.FILTER_EXP_SCALE
    lane = np.arange(64)
    W0 = np.zeros((64, 16))
    W0[:50, :9] = Ws[0]
    t, s = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    want = (c * W0[16 * t[:, None, :] + (lane & 15)[None, :, None], 4 * s[:, None, :] + (lane >> 4)[None, :, None]]).astype(np.float32)
    assert np.array_equal(f32[:offs[1]].reshape(4, 64, 4), want)
    for l in (1, 2):
        W = np.zeros((64, 64))
        W[:50, :50] = Ws[l]
        got = f32[offs[1]:offs[2]].reshape(2, 4, 4, 64, 4)[l - 1]
        for t in range(4):
            for tk in range(4):
                rows = 16 * t + (lane & 15)
                cols = 16 * tk + 4 * (lane >> 4)[:, None] + np.arange(4)[None, :]
                assert np.array_equal(got[t, tk], (c * W[rows[:, None], cols]).astype(np.float32)), (l, t, tk)
    bias = np.zeros((3, 64))
    for l in range(3):
        bias[l, :50] = c * Bs[l]
    assert np.array_equal(f32[offs[2]:].reshape(3, 64), bias.astype(np.float32))


def test_float32_emulation_stays_inside_the_margin():
    """ORDER OF MAGNITUDE ONLY: numpy's float32 matmul and exp are not the kernel's fmaf chain and v_exp_f32.  20 000 inputs from
    the domain box, its corners and faces included."""
    k = 3
    widths, params = networks.load_network(k)
    m = networks.filter_margin(k, widths, params)
    rng = np.random.default_rng(11)
    lo = np.array([0.0] * 3 + [-1.0 / 3] * 6)
    hi = np.array([1.0] * 3 + [1.0 / 3] * 6)
    u = rng.uniform(size=(20000, 9))
    u[:4000] = rng.integers(0, 2, size=(4000, 9))                          # corners
    face = rng.uniform(size=(4000, 9)) < 0.5
    u[4000:8000] = np.where(face, rng.integers(0, 2, size=(4000, 9)), u[4000:8000])      # faces of every dimension
    x = lo + (hi - lo) * u
    y64 = networks.forward_twin(k, widths, params, x)
    y32 = networks.forward_twin(k, widths, params, x, dtype=np.float32).astype(np.float64)
    err = np.abs(y32 - y64).max()
    print("float32 emulation: max |y32 - y64| = %.3g, margin %.4g" % (err, m))
    assert err <= m, (err, m)
