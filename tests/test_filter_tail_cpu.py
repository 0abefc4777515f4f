"""The three tail networks of tests/filter_tail_nets.py, on the CPU: they filter, the C margin (csrc/net_pack.h, whose count for
rows 48 and 49 follows the VALU tail of the fp32 pass) agrees with the numpy restatement, and a tail neuron that is dropped or
swapped moves the float64 twin's output by more than ten margins on nearly every input -- which is what makes the device audit of
tests/test_gpu_filter_tail.py unable to miss one."""
import numpy as np
import pytest

import filter_tail_nets as ftn
import test_filter_margin_cpu as fm
import user_nets
from sdpcutsel_via_nn_amd import networks

lib = fm.lib      # the compiled wrapper around net_pack.h (module-scoped fixture)

INPUTS = user_nets.nn_batch_inputs(3, 5, 4096, 64)


@pytest.mark.parametrize("name", ftn.NAMES)
def test_tail_network_filters_and_margins_agree(lib, name):
    widths, params = ftn.tail_network(name)
    networks.check_network(3, widths, params)
    assert networks.filter_ok(3, widths, params)
    m = networks.filter_margin(3, widths, params)
    cm, ok, _, f32, _ = fm._c_side(lib, 3, widths, params)
    print("%s: margin %.4g (C side %.4g)" % (name, m, cm))
    assert ok and f32.shape[0] > 0
    assert abs(cm - m) <= 1e-9 * m, (name, cm, m)


def test_margin_counts_the_tail_rows_chain(lib):
    """the shipped network: rows 48 and 49 see at most 16 roundings per term where a matrix-core row sees up to 50, so the margin
    lies a little below the any-row count, and the C side follows"""
    widths, params = networks.load_network(3)
    m = networks.filter_margin(3, widths, params)
    cm = fm._c_side(lib, 3, widths, params)[0]
    print("shipped 3-variable network: margin %.6f" % m)
    assert abs(cm - m) <= 1e-9 * m
    assert 0.01 < m < 0.029588 + 1e-6      # the figure before the tail rows had a count of their own


@pytest.mark.parametrize("name", ftn.NAMES)
def test_a_broken_tail_moves_the_output_by_many_margins(name):
    widths, params = ftn.tail_network(name)
    m = networks.filter_margin(3, widths, params)
    y = networks.forward_twin(3, widths, params, INPUTS)
    for what, p in ftn.broken_tails(widths, params).items():
        moved = np.abs(networks.forward_twin(3, widths, p, INPUTS) - y)
        share = float((moved > 10.0 * m).mean())
        print("%s, %s: %.4f of %d rows moved by more than 10 margins (margin %.3g, median move %.3g)"
              % (name, what, share, INPUTS.shape[0], m, np.median(moved)))
        assert share >= 0.9, (name, what, share)
