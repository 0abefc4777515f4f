"""The margin PER CANDIDATE of the fp32 filter (csrc/net_pack.h: net_filter_slope_terms, restated in networks.filter_margin_terms):
M = min(filter_margin, (S (1 + 2^-9) + C0) (1 + 2^-10)), S = sum_j G_j (1 - a_j^2) over the last hidden layer.  CPU only: the header
is compiled with the host compiler, as tests/test_filter_margin_cpu.py does.

What is checked here: the C side against the numpy twin, the rounding direction and the padding of G, that the a-priori margin
kept its bits, and a replay of the filter's rule on 4096 synthetic sets.  That the bound holds on the real instructions is checked
on the device (tests/test_gpu_filter_slope_margin.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_tail_nets
from sdpcutsel_via_nn_amd import networks, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

WRAPPER = r"""
#include "net_pack.h"
extern "C" int terms(int k, int n_layers, const int32_t *widths, const double *params, int64_t n_params, double *margin, int32_t *ok,
                     double *g64, float *g32, double *c0)
{
    NetPack p;
    const char *why = "";
    const int rc = net_pack(k, n_layers, widths, params, n_params, &p, &why);
    if (rc != SDPCUT_OK) return rc;
    *margin = p.filter_margin;
    *ok = p.filter_ok;
    for (int j = 0; j < MAX_HIDDEN; ++j) { g64[j] = p.filter_g64[j]; g32[j] = p.filter_g[j]; }
    *c0 = p.filter_c0;
    return rc;
}
"""

# net_filter_margin of the commit before the margin per candidate, C side (g++ -O2), as hex floats
MARGIN_BEFORE = {
    2: "0x1.2e588795f9b40p-6", 3: "0x1.d96661246464fp-6", 4: "0x1.e8fd33a8e2d88p-5", 5: "0x1.268c4b093650fp+0",
    "speaks": "0x1.9e9cc22cb8f3ap-10", "heard": "0x1.cc2bf63ece836p-11", "both": "0x1.c1f4cffb66c0ep-15",
}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_slope_margin")
    src = d / "terms.cpp"
    src.write_text(WRAPPER)
    so = d / "terms.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _c_side(lib, k, widths, params):
    widths = np.ascontiguousarray(widths, dtype=np.int32)
    params = np.ascontiguousarray(params, dtype=np.float64)
    margin, ok, c0 = ctypes.c_double(-1.0), ctypes.c_int32(-1), ctypes.c_double(-1.0)
    g64 = np.full(64, np.nan)
    g32 = np.full(64, np.nan, dtype=np.float32)
    rc = lib.terms(int(k), int(widths.shape[0]), widths.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                   params.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int64(params.shape[0]), ctypes.byref(margin),
                   ctypes.byref(ok), g64.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                   g32.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(c0))
    assert rc == 0, rc
    return margin.value, bool(ok.value), g64, g32, c0.value


def _nets():
    yield "shipped", 3, networks.load_network(3)
    for name in filter_tail_nets.NAMES:
        yield name, 3, filter_tail_nets.tail_network(name)


def test_terms_against_the_twin(lib):
    for name, k, (widths, params) in _nets():
        m, ok, g64, g32, c0 = _c_side(lib, k, widths, params)
        G, Gf, C0, e = networks.filter_margin_terms(k, widths, params)
        assert ok, name
        assert np.all(np.abs(g64 - G) <= 1e-9 * G), name
        assert abs(c0 - C0) <= 1e-9 * C0, (name, c0, C0)
        # rounded UP, entry by entry, and by no more than one float spacing; what the twin rounds is what the C side rounds
        assert np.all(g32.astype(np.float64) >= g64), name
        assert np.all(g32.astype(np.float64) <= g64 * (1.0 + 2.0 ** -22)), name
        assert np.array_equal(g32, Gf) or np.all(np.abs(g32.astype(np.float64) - Gf.astype(np.float64)) <= 2.0 ** -22 * G), name
        assert np.all(g64[50:] == 0.0) and np.all(g32[50:] == 0.0) and np.all(G[50:] == 0.0) and np.all(Gf[50:] == 0.0), name
        assert np.all(g64[:50] >= 0.0) and c0 > 0.0 and e.shape == (50,)
        # S <= sum G (every slope is at most 1): the bound with every slope at 1 is the a-priori one and a little more
        assert (g64.sum() + c0) * (1.0 + 2.0 ** -10) >= m, name
        print("%s: margin %.6g, sum G %.6g, C0 %.3g" % (name, m, g64.sum(), c0))


def test_the_a_priori_margin_kept_its_bits(lib):
    for k in (2, 3, 4, 5):
        assert _c_side(lib, k, *networks.load_network(k))[0] == float.fromhex(MARGIN_BEFORE[k]), k
    for name in filter_tail_nets.NAMES:
        assert _c_side(lib, 3, *filter_tail_nets.tail_network(name))[0] == float.fromhex(MARGIN_BEFORE[name]), name
    # ... and the twin still restates it
    for k in (2, 3, 4, 5):
        m = networks.filter_margin(k, *networks.load_network(k))
        assert abs(m - float.fromhex(MARGIN_BEFORE[k])) <= 1e-9 * m, k


def synthetic_replay(oracle, net=None):
    """The 4096 synthetic sets (n = 100, seed 7) -> (lambda_min, obj64 / max_elem, the twin's margin per candidate, the a-priori margin)"""
    net = networks.load_network(3) if net is None else net
    wl = synthetic.make_workload(nb_vars=100, k=3, count=4096, seed=7)
    n, vv, Q = 100, wl["vars_values"], wl["Q_arr"]
    sets = wl["set_inds"][:, :3].astype(np.int32)
    L = n * (n + 1) // 2
    eig = oracle.eigmin_batch(3, vv[L:][sets], vv[:L][oracle.triu_positions(sets, n)])
    pos = oracle.triu_positions(sets, n)
    q = Q[pos]
    me = 3.0 * np.abs(q).max(axis=1)
    me[me == 0.0] = 1.0
    q = q / me[:, None]
    _, _, obj = filter_tail_nets.measure(oracle, net, sets, n, vv, Q)
    m = networks.filter_margin_at(3, net[0], net[1], np.concatenate([vv[L:][sets], q], axis=1))
    return eig, obj / me, m, networks.filter_margin(3, *net)


def test_replay_on_the_synthetic_sets(oracle):
    eig, r, m, m0 = synthetic_replay(oracle)
    viol = eig < oracle.THRES_NEG_EIGVAL
    assert np.all(m > 0.0) and np.all(m <= m0)
    positives = int((viol & (r > 0)).sum())
    survivors = int((viol & (r > -m)).sum())
    a_priori = int((viol & (r > -m0)).sum())
    print("synthetic sets: %d violated, %d positive, %d survive the margin per candidate (%.4g .. %.4g), %d the a-priori margin %.4g"
          % (viol.sum(), positives, survivors, m.min(), m.max(), a_priori, m0))
    assert positives <= survivors < a_priori
