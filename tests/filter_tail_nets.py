"""User networks that make the two tail neurons (48 and 49) of the fp32 filter's pass decisive, for test_filter_tail_cpu.py and
test_gpu_filter_tail.py.  The filter's pass runs neurons 0..47 of every hidden layer on the matrix core and neurons 48, 49 on the
VALU (csrc/score_mfma.hip: filter_pass_f32); in these networks a dropped, swapped or misplaced tail neuron moves the output by many
margins.  A plain module: no fixtures, no GPU.

All three start from user_nets.shaped_network(3, 12.0, seed=SEED) -- three hidden layers of 50, clamp-free -- with Ws[l] as
networks.split_params returns them (l = 1, 2 hidden -> hidden, l = 3 the output layer):
  speaks  Ws[3][0, :48] = 0, Ws[3][0, 48:] = (0.9, -0.7): only the tail of the last hidden layer reaches the output
  heard   for l in (1, 2): Ws[l][:, :48] = 0, Ws[l][:, 48] *= 4, Ws[l][:, 49] *= -4: the next layer hears only the tail
  both    both edits"""
import numpy as np

import user_nets
from sdpcutsel_via_nn_amd import networks

SEED = 32
NAMES = ("speaks", "heard", "both")


def tail_network(name):
    if name not in NAMES:
        raise ValueError(name)
    widths, params = user_nets.shaped_network(3, 12.0, seed=SEED)
    params = params.copy()
    Ws = networks.split_params(3, widths, params)[3]      # views of params
    if name in ("speaks", "both"):
        Ws[3][0, :48] = 0.0
        Ws[3][0, 48:] = (0.9, -0.7)
    if name in ("heard", "both"):
        for l in (1, 2):
            Ws[l][:, :48] = 0.0
            Ws[l][:, 48] *= 4.0
            Ws[l][:, 49] *= -4.0
    return widths, params


def broken_tails(widths, params):
    """the network with a tail neuron dropped, or the two swapped, in what the layers behind read: column 48 of every Ws[1..3]
    zeroed, column 49 zeroed, the two columns exchanged -> {what: params}"""
    out = {}
    for what in ("no 48", "no 49", "swapped"):
        p = params.copy()
        Ws = networks.split_params(3, widths, p)[3]
        for l in (1, 2, 3):
            if what == "no 48":
                Ws[l][:, 48] = 0.0
            elif what == "no 49":
                Ws[l][:, 49] = 0.0
            else:
                Ws[l][:, [48, 49]] = Ws[l][:, [49, 48]]
        out[what] = p
    return out


def measure(oracle, net, sets, n_vars, vv, Q):
    """float64 twin of `net` on every 3-variable set -> (y64 unmapped output, max_elem, obj = -S max_elem + y max_elem): _measure of
    test_gpu_fp32_filter.py for a network of one's own"""
    L = n_vars * (n_vars + 1) // 2
    pos = oracle.triu_positions(sets, n_vars)
    q = Q[pos]
    me = 3.0 * np.abs(q).max(axis=1)
    me[me == 0.0] = 1.0
    q = q / me[:, None]
    S = (q * vv[:L][pos]).sum(axis=1)
    y = networks.forward_twin(3, net[0], net[1], np.concatenate([vv[L:][sets], q], axis=1))
    return y, me, (-S) * me + y * me
