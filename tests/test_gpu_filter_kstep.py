"""The fp32 filter's pass with neurons 48 and 49 in ONE k-step (csrc/score_mfma.hip: filter_pass_f32 -- neuron 48 on the q = 0 slot
of the hidden layers' last k-step, 49 on q = 1, the A operand merged in the kernel from the packed fragment (t, 3); the VALU tail
takes the tail activation lane q holds at the head of its chain), on the device:
  1. the shipped network's audit on the 4 096 synthetic sets (n = 100, seed 7) and the pattern list (n = 40, 9 880 sets): every
     |y32 - y64| inside the margin, and the largest within four times the 1.00e-5 of the pass before the tail left the matrix core
     (profiles/fp32_filter_ab.txt; the yardstick of tests/test_gpu_filter_tail.py, not a figure of this build);
  2. the three tail networks of tests/filter_tail_nets.py -- all their weight on neurons 48 and 49, so a wrong lane moves the output
     by more than ten margins (tests/test_filter_tail_cpu.py): the audit, and one combined round each on the "fills" and "runs"
     lists under SDPCUT_OPT_SKIP_NONVIOLATED = 2 whose head is the one of a round with SDPCUT_OPT_FP32_FILTER = 0;
  3. (CPU) the C margin and networks.filter_margin agree to 1e-9 relative for the shipped network and the three tail networks: both
     count terms 48 and 49 from the first term of their shared k-step.
Lists and helpers are those of tests/test_gpu_filter_tail.py, tests/test_gpu_fp32_filter.py and tests/test_gpu_skip_nonviolated.py."""
import numpy as np
import pytest

import filter_tail_nets as ftn
import test_filter_margin_cpu as fm
import test_gpu_filter_tail as tail
import test_gpu_fp32_filter as fp
import test_gpu_skip_nonviolated as base

lib = fm.lib      # the compiled wrapper around net_pack.h (module-scoped fixture)

PARENT_AUDIT_MAX = tail.PARENT_AUDIT_MAX


@pytest.fixture(scope="module")
def world(oracle):
    return base._World(oracle)


@pytest.fixture(scope="module")
def synth():
    from sdpcutsel_via_nn_amd import synthetic
    return synthetic.make_workload(nb_vars=100, k=3, count=4096, seed=7)


@pytest.mark.gpu
def test_shipped_network_audit(world, synth, oracle):
    from sdpcutsel_via_nn_amd import networks
    want = networks.filter_margin(3, *networks.load_network(3))
    worst = 0.0
    for what, n_vars, Q, sets, vv in tail._lists(world, synth):
        y32, y64, m = tail._audit(oracle, None, n_vars, Q, sets, vv)
        assert abs(m - want) <= 1e-9 * want, (m, want)
        err = float(np.abs(y32 - y64).max())
        print("shipped network, %s: %d candidates, max |y32 - y64| = %.3g = %.3g of the margin %.6f" % (what, sets.shape[0], err, err / m, m))
        assert np.isfinite(y32).all() and err < m, (what, err, m)
        worst = max(worst, err)
    print("shipped network: largest |y32 - y64| %.3g (yardstick %.3g)" % (worst, PARENT_AUDIT_MAX))
    assert worst <= 4.0 * PARENT_AUDIT_MAX, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ftn.NAMES)
def test_tail_network_audit_and_round(world, synth, oracle, name):
    from sdpcutsel_via_nn_amd import networks
    net = ftn.tail_network(name)
    want = networks.filter_margin(3, *net)
    vv = world.points[3]
    for kind in ("fills", "runs"):
        which, flags = base._layout(world, kind)
        sets = base.ALL_SETS[which]
        y32, y64, m = tail._audit(oracle, net, base.N_VARS, world.Q, sets, vv)
        assert abs(m - want) <= 1e-9 * want, (name, m, want)
        err = float(np.abs(y32 - y64).max())
        print("%s, %s: %d candidates, max |y32 - y64| = %.3g = %.3g of the margin %.4g" % (name, kind, sets.shape[0], err, err / m, m))
        assert np.isfinite(y32).all() and err < m, (name, kind, err, m)
        handles = fp._handles(world, which, ((2, 1), (2, 0)), net=net)      # filtering | skipping only
        try:
            outs = fp._round(handles, "round_csr", 4, 20, vv)
            fp._all_same(outs, base.CSR_FIELDS, (name, kind))
            assert outs[0]["idx"].shape[0] == 20
        finally:
            for sc in handles:
                sc.close()


@pytest.mark.parametrize("name", ("shipped",) + ftn.NAMES)
def test_margins_agree(lib, name):
    from sdpcutsel_via_nn_amd import networks
    widths, params = networks.load_network(3) if name == "shipped" else ftn.tail_network(name)
    m = networks.filter_margin(3, widths, params)
    cm, ok, _, _, _ = fm._c_side(lib, 3, widths, params)
    print("%s: margin %.9g (C side %.9g)" % (name, m, cm))
    assert ok and abs(cm - m) <= 1e-9 * m, (name, cm, m)
