"""Training on the CPU (sdpcutsel_via_nn_amd/networks.py): the numpy twin of the device's loss / gradient, the Table-1 sampler and
the scaled-conjugate-gradient trainer on the twin.  No GPU: the device kernel is compared with the same twin in test_gpu_train.py."""
import ctypes
import subprocess

import numpy as np
import pytest

from sdpcutsel_via_nn_amd import exact_sdp, networks
from test_net_pack import CSRC, EINVAL, OK, WRAPPER, _pack

LD = np.longdouble


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    """csrc/net_pack.h behind a C wrapper, compiled as tests/test_net_pack.py compiles it"""
    d = tmp_path_factory.mktemp("net_pack_train")
    src = d / "pack.cpp"
    src.write_text(WRAPPER)
    so = d / "pack.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def random_network(k, hidden, seed):
    """weights and biases in +-1, non-trivial mapping constants"""
    rng = np.random.default_rng(seed)
    d_in = k * (k + 3) // 2
    widths = np.array(list(hidden) + [1], dtype=np.int32)
    parts, fan = [rng.uniform(-0.5, 0.5, d_in), rng.uniform(0.5, 2.5, d_in), np.array([-0.9])], d_in
    for w in widths:
        parts += [rng.uniform(-1, 1, int(w) * fan), rng.uniform(-1, 1, int(w))]
        fan = int(w)
    parts.append(np.array([-0.8, 1.7, 0.3]))
    return widths, np.concatenate(parts)


def test_twin_gradient_against_central_differences():
    """k = 2, H = 3, one hidden layer, 7 samples, everything in long double: central differences with step h have a truncation
    error ~ h^2 |f'''| / 6 and a rounding error ~ eps_ld |f| / h; h = 1e-6 balances them near 1e-12 relative."""
    k, rng = 2, np.random.default_rng(5)
    widths, params = random_network(k, (3,), 11)
    X, t = rng.uniform(-1, 1, (7, 5)), rng.uniform(-1, 1, 7)
    loss, grad = networks.loss_grad_twin(k, widths, params, X, t, dtype=LD)
    assert grad.dtype == LD and grad.shape == (params.shape[0] - 2 * 5 - 4,) == (3 * 5 + 3 + 3 + 1,)
    h = LD(1e-6)
    fd = np.zeros(grad.shape[0], dtype=LD)
    for i in range(grad.shape[0]):
        p1, p2 = params.astype(LD), params.astype(LD)
        p1[11 + i] += h
        p2[11 + i] -= h
        fd[i] = (networks.loss_grad_twin(k, widths, p1, X, t, dtype=LD)[0] - networks.loss_grad_twin(k, widths, p2, X, t, dtype=LD)[0]) / (2 * h)
    err = float(np.abs(fd - grad).max() / np.abs(grad).max())
    print("central differences vs backprop, long double: %.2e relative" % err)
    assert err < 1e-9
    # the float64 twin agrees with the long double one to rounding
    l64, g64 = networks.loss_grad_twin(k, widths, params, X, t)
    assert g64.dtype == np.float64 and abs(l64 - float(loss)) <= 1e-15 * abs(l64) * 8
    assert np.linalg.norm(g64 - grad.astype(np.float64)) <= 1e-14 * np.linalg.norm(g64)


CASES = [  # (k, widths, delta n_params, accepted)
    (2, [3, 1], 0, True), (5, [64, 64, 64, 64, 1], 0, True), (3, [50, 50, 50, 1], 0, True), (4, [1, 1], 0, True),
    (1, [3, 1], 0, False), (6, [3, 1], 0, False), (2, [1], 0, False), (2, [3, 3, 3, 3, 3, 1], 0, False),
    (2, [3, 2], 0, False), (2, [3, 4, 1], 0, False), (2, [65, 1], 0, False), (2, [0, 1], 0, False),
    (2, [3, 1], 1, False), (2, [3, 1], -1, False),
]


@pytest.mark.parametrize("k,widths,dn,accepted", CASES)
def test_twin_refuses_where_net_pack_refuses(lib, k, widths, dn, accepted):
    d_in = max(k, 1) * (max(k, 1) + 3) // 2
    n, fan = 2 * d_in + 4, d_in
    for w in widths:
        n += w * fan + w
        fan = w
    params = np.linspace(-0.5, 0.5, n + dn)
    rc, why = _pack(lib, k, widths, params)[:2]
    assert rc == (OK if accepted else EINVAL)
    X, t = np.zeros((2, k * (k + 3) // 2)), np.zeros(2)
    if accepted:
        loss, grad = networks.loss_grad_twin(k, np.array(widths), params, X, t)
        assert np.isfinite(loss) and grad.shape == (n - 2 * d_in - 4,)
    else:
        with pytest.raises(ValueError) as ei:
            networks.loss_grad_twin(k, np.array(widths), params, X, t)
        assert str(ei.value) == why      # the same message


def test_sample_table1():
    for k in (2, 3, 4, 5):
        S = networks.sample_table1(k, 300, seed=5)
        assert S.shape == (300, k * (k + 3) // 2) and S.dtype == np.float64
        x, q = S[:, :k], S[:, k:]
        assert x.min() >= 0.0 and x.max() <= 1.0
        ia, ib = np.triu_indices(k)
        Q = np.zeros((300, k, k))
        Q[:, ia, ib] = np.where(ia == ib, q, 0.5 * q)      # off-diagonals come doubled
        Q[:, ib, ia] = Q[:, ia, ib]
        ev = np.linalg.eigvalsh(Q)
        assert ev.min() >= -1.0 - 1e-12 and ev.max() <= 1.0 + 1e-12
        assert ev.min() < -0.8 and ev.max() > 0.8            # ... and fill the interval
        # the convention is the one the exact solver reads: C = unpack(...) is the same matrix
        assert np.array_equal(exact_sdp.unpack(k, S)[1], Q)
        # read WITHOUT halving the spectrum leaves [-1, 1] (k >= 2: some off-diagonal weight is always there)
        Q2 = Q.copy()
        Q2[:, ia, ib] = q
        Q2[:, ib, ia] = Q2[:, ia, ib]
        assert np.abs(np.linalg.eigvalsh(Q2)).max() > 1.0
        assert np.array_equal(S, networks.sample_table1(k, 300, seed=5))
        assert not np.array_equal(S, networks.sample_table1(k, 300, seed=6))
        assert np.array_equal(S[:100], networks.sample_table1(k, 300, seed=5)[:100])


@pytest.fixture(scope="module")
def trained():
    k = 2
    X = networks.sample_table1(k, 512, seed=3)
    t = exact_sdp.solve(k, X)["value"]
    widths, params, rep = networks.train(k, X, t, hidden=(8,), epochs=100, seed=7)
    return k, X, t, widths, params, rep


def affine_val_mse(X, t, rep, y_gain):
    """validation MSE, in the network's normalised units, of the least-squares affine fit on the training part of the same split"""
    perm, (f0, ntr), (v0, nva) = rep["perm"], rep["split"]["train"], rep["split"]["val"]
    Xp, tp = X[perm], t[perm]
    coef = np.linalg.lstsq(np.c_[Xp[f0:f0 + ntr], np.ones(ntr)], tp[f0:f0 + ntr], rcond=None)[0]
    pred = np.c_[Xp[v0:v0 + nva], np.ones(nva)] @ coef
    return float(np.mean(((pred - tp[v0:v0 + nva]) * y_gain) ** 2))


def test_train_on_the_twin(trained):
    """k = 2, H = 8, one hidden layer, 512 Table-1 samples labelled by exact_sdp.solve, 100 SCG iterations (seed 7).
    Measured on the CPU: validation MSE 2.05e-3 against 3.00e-2 of the affine least-squares fit (1.47e-3 after 200 iterations,
    3.4e-3 after 50): a factor of 14 of room."""
    k, X, t, widths, params, rep = trained
    tl, vl = np.array(rep["train_loss"]), np.array(rep["val_loss"])
    assert tl.shape == vl.shape == (rep["iterations"] + 1,) and rep["stop"] == "epochs" and rep["iterations"] == 100
    assert np.all(tl[1:] <= tl[:-1])                         # SCG accepts only decreases
    assert tl[-1] < 0.1 * tl[0]
    # the weights returned are those of the best validation loss
    assert rep["best_val_loss"] == vl.min() == vl[rep["best_iteration"]]
    perm, (v0, nva) = rep["perm"], rep["split"]["val"]
    val = networks.loss_grad_twin(k, widths, params, X[perm][v0:v0 + nva], t[perm][v0:v0 + nva])[0]
    assert val == rep["best_val_loss"]
    aff = affine_val_mse(X, t, rep, params[-2])
    print("validation MSE %.3e, affine fit %.3e" % (val, aff))
    assert val < aff
    # the three parts partition the samples
    assert sorted(perm.tolist()) == list(range(512))
    assert sum(c for _, c in rep["split"].values()) == 512 and rep["split"]["train"] == (0, 384)
    assert rep["grad_evals"] <= 2 * rep["iterations"] + 1


def test_train_stops_on_validation_failures_and_min_grad():
    k = 2
    X = networks.sample_table1(k, 64, seed=4)
    t = exact_sdp.solve(k, X)["value"]
    _, _, rep = networks.train(k, X, t, hidden=(8,), epochs=400, max_fail=3, seed=7)
    assert rep["stop"] == "max_fail" and rep["iterations"] < 400
    vl = rep["val_loss"]
    assert rep["best_iteration"] == int(np.argmin(vl)) and all(v > rep["best_val_loss"] for v in vl[-3:])
    _, _, rep = networks.train(k, X, t, hidden=(8,), epochs=50, min_grad=1e3, seed=7)
    assert rep["stop"] == "min_grad" and rep["iterations"] == 0


def test_trained_network_round_trips_through_net_pack(lib, trained):
    k, X, t, widths, params, rep = trained
    rc, why, blob, offs, ints, dbl = _pack(lib, k, widths, params)
    assert rc == OK, why
    assert tuple(ints[:3]) == (5, 1, 8) and bool(ints[5]) == rep["unclamped_ok"] == networks.unclamped_ok(k, widths, params)
    # mapminmax of the data: the mapped inputs and targets of the samples fill [-1, 1]
    assert np.array_equal(blob[offs[0]:offs[0] + 5], X.min(axis=0)) and np.allclose(blob[offs[0] + 5:offs[0] + 10], 2.0 / (X.max(axis=0) - X.min(axis=0)))
    assert (dbl[0], dbl[2]) == (-1.0, -1.0) and dbl[4] == t.min() and np.isclose(dbl[3], 2.0 / (t.max() - t.min()))
    # the raw weights in the blob are the trained ones
    _, _, _, Ws, Bs, _ = networks.split_params(k, widths, params)
    for l in range(2):
        assert np.array_equal(blob[offs[7 + l]:offs[7 + l] + Ws[l].size], Ws[l].ravel())
        assert np.array_equal(blob[offs[7 + 5 + l]:offs[7 + 5 + l] + Bs[l].size], Bs[l])
    # and the forward twin undoes the output mapping: on the training data it is closer to the labels than their mean
    y = networks.forward_twin(k, widths, params, X)
    assert np.mean((y - t) ** 2) < 0.2 * np.var(t)
