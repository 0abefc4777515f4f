"""Loss and gradient of a user's MLP on the device (sdpcut_train_set_data / sdpcut_train_loss_grad, csrc/train.hip) against the
numpy twin (networks.loss_grad_twin), and training end to end with the device as back end.

Tolerance of the comparisons with the twin: not a constant.  Every case computes the twin in float64 and in long double; the
device's normwise error against the long double result may be at most FACTOR = 16 times the float64 twin's own error against it
(the device evaluates tansig with the library exp, like the twin, but multiplies in MFMA order and sums the samples in another
order: per strip, per workgroup, then over the workgroups).  The same rule holds for the loss, one number, without a floor.

Every comparison prints its ratio (device error / twin error; run with -s).  DESIGN.md section 5, "Training", records what has been
measured."""
import numpy as np
import pytest

from sdpcutsel_via_nn_amd import _capi, networks
from test_train_cpu import affine_val_mse, random_network

pytestmark = pytest.mark.gpu
LD = np.longdouble
FACTOR = 16.0

#        k, H, hidden layers, count, first
# The last case has 1025 strips of 16 samples, more than the 2 x CUs workgroups of a launch: every workgroup takes two or three
# strips, so the accumulators carried from strip to strip and the reuse of the strip's LDS are exercised
# (test_multi_strip_case_is_multi_strip checks the premise against the device).
MULTI_STRIP = (2, 3, 1, 16 * 1024 + 5, 0)
CASES = [(2, 3, 1, 1, 0), (3, 50, 3, 17, 0), (4, 64, 3, 1029, 5), (5, 64, 4, 16 * 64 * 3 + 5, 0), MULTI_STRIP]


def normwise(a, ref):
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.sqrt(((a - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))


def ratio(err, twin):
    return err / twin if twin > 0 else (0.0 if err == 0 else float("inf"))


@pytest.fixture(scope="module")
def scorer():
    import sdpcutsel_via_nn_amd as pkg
    sc = pkg.Scorer(0)
    yield sc
    sc.close()


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "k%d_H%d_L%d_n%d_f%d" % c)
def case(request, scorer):
    """one device evaluation and the two twins of a case, shared by the tests below"""
    k, H, nh, count, first = request.param
    widths, params = random_network(k, (H,) * nh, seed=100 + k)
    rng = np.random.default_rng(200 + k)
    n_data = first + count + 3                        # the range ends inside the set
    X = np.concatenate([rng.uniform(0, 1, (n_data, k)), rng.uniform(-1, 1, (n_data, k * (k + 1) // 2))], axis=1)
    t = rng.uniform(-1, 1, n_data)
    scorer.train_set_data(k, X, t)
    loss, grad = scorer.train_loss_grad(k, widths, params, first, count)
    sl = slice(first, first + count)
    l64, g64 = networks.loss_grad_twin(k, widths, params, X[sl], t[sl])
    lld, gld = networks.loss_grad_twin(k, widths, params, X[sl], t[sl], dtype=LD)
    return dict(k=k, widths=widths, params=params, X=X, t=t, first=first, count=count, loss=loss, grad=grad, l64=l64, g64=g64,
                lld=lld, gld=gld, sc=scorer)


def test_loss_and_gradient_against_the_twin(case):
    c = case
    assert c["grad"].shape == c["g64"].shape and np.all(np.isfinite(c["grad"]))
    e_dev, e_twin = normwise(c["grad"], c["gld"]), normwise(c["g64"], c["gld"])
    l_dev = abs(float(LD(c["loss"]) - c["lld"])) / float(c["lld"])
    l_twin = abs(float(LD(c["l64"]) - c["lld"])) / float(c["lld"])
    print("k %d H %d layers %d count %d: gradient error device %.3e twin %.3e ratio %.2f; loss error device %.3e twin %.3e ratio %.2f"
          % (c["k"], c["widths"][0], len(c["widths"]) - 1, c["count"], e_dev, e_twin, ratio(e_dev, e_twin), l_dev, l_twin, ratio(l_dev, l_twin)))
    assert e_dev <= FACTOR * e_twin
    assert l_dev <= FACTOR * l_twin


def test_multi_strip_case_is_multi_strip(scorer):
    """a launch has at most 2 x CUs workgroups (csrc/train.hip); the last case must give every one of them more than one strip"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert (MULTI_STRIP[3] + 15) // 16 >= 2 * (2 * n_cu)


def test_forward_only_loss_against_the_twin(case):
    """grad = NULL takes another way through the strip loop (no backward part): its loss under the same rule"""
    c = case
    loss = c["sc"].train_loss_grad(c["k"], c["widths"], c["params"], c["first"], c["count"], want_grad=False)[0]
    l_dev = abs(float(LD(loss) - c["lld"])) / float(c["lld"])
    l_twin = abs(float(LD(c["l64"]) - c["lld"])) / float(c["lld"])
    print("forward only, count %d: loss error device %.3e twin %.3e ratio %.2f" % (c["count"], l_dev, l_twin, ratio(l_dev, l_twin)))
    assert l_dev <= FACTOR * l_twin


def test_same_bits_twice_and_without_gradient(case):
    c = case
    loss2, grad2 = c["sc"].train_loss_grad(c["k"], c["widths"], c["params"], c["first"], c["count"])
    loss3, none = c["sc"].train_loss_grad(c["k"], c["widths"], c["params"], c["first"], c["count"], want_grad=False)
    assert none is None
    assert np.float64(loss2).tobytes() == np.float64(c["loss"]).tobytes() == np.float64(loss3).tobytes()
    assert grad2.tobytes() == c["grad"].tobytes()


@pytest.mark.parametrize("cut", [1, 7, 16, 500])
def test_split_range_sums_to_the_whole(case, cut):
    """two calls over [first, first + cut) and [first + cut, first + count), weighted by their counts"""
    c = case
    if cut >= c["count"]:
        cut = c["count"] // 2
    if cut < 1:
        cut, rest = c["count"], 0                     # a one-sample range has no second part
    else:
        rest = c["count"] - cut
    l1, g1 = c["sc"].train_loss_grad(c["k"], c["widths"], c["params"], c["first"], cut)
    l2, g2 = (0.0, np.zeros_like(g1)) if rest == 0 else c["sc"].train_loss_grad(c["k"], c["widths"], c["params"], c["first"] + cut, rest)
    g = (cut * g1.astype(LD) + rest * g2.astype(LD)) / c["count"]
    loss = (cut * LD(l1) + rest * LD(l2)) / c["count"]
    e_split, e_twin = normwise(g, c["gld"]), normwise(c["g64"], c["gld"])
    l_split = abs(float(loss - c["lld"])) / float(c["lld"])
    l_twin = abs(float(LD(c["l64"]) - c["lld"])) / float(c["lld"])
    print("split at %d of %d: gradient ratio %.2f, loss ratio %.2f" % (cut, c["count"], ratio(e_split, e_twin), ratio(l_split, l_twin)))
    assert e_split <= FACTOR * e_twin
    assert l_split <= FACTOR * l_twin


def test_training_forward_is_the_inference_forward(scorer):
    """for a network that is also loaded with set_network, the loss of a range is the mean of (nn_batch -> normalised - t_n)^2"""
    k, first, count = 4, 5, 1029
    widths, params = random_network(k, (64, 64, 64), seed=31)
    _, _, _, Ws, Bs, _ = networks.split_params(k, widths, params)
    for a in Ws + Bs:
        a *= 0.5                                      # (views of params) keeps every pre-activation below net_pack's bound
    assert networks.unclamped_ok(k, widths, params)
    rng = np.random.default_rng(32)
    X = np.concatenate([rng.uniform(0, 1, (1100, k)), rng.uniform(-1, 1, (1100, 10))], axis=1)
    t = rng.uniform(-1, 1, 1100)
    scorer.train_set_data(k, X, t)
    scorer.set_network(k, widths, params)
    loss = scorer.train_loss_grad(k, widths, params, first, count, want_grad=False)[0]
    y = scorer.nn_batch(k, X[first:first + count])
    y_ymin, y_gain, y_xoffset = params[-3:]
    host = np.mean(((y - y_xoffset) * y_gain + y_ymin - ((t[first:first + count] - y_xoffset) * y_gain + y_ymin)) ** 2)
    print("loss %.17g, from nn_batch %.17g, relative difference %.2e" % (loss, host, abs(loss - host) / host))
    assert abs(loss - host) <= 1e-12 * host


def test_refusals(scorer):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import synthetic
    k = 3
    widths, params = random_network(k, (8,), seed=1)
    X, t = np.random.default_rng(1).uniform(0, 1, (40, 9)), np.zeros(40)
    sc = pkg.Scorer(0)
    try:
        with pytest.raises(_capi.SdpCutError, match="sdpcut_train_set_data"):           # before train_set_data
            sc.train_loss_grad(k, widths, params, 0, 10)
        sc.train_set_data(k, X, t)
        assert np.isfinite(sc.train_loss_grad(k, widths, params, 0, 40)[0])
        with pytest.raises(_capi.SdpCutError, match="sdpcut_train_set_data"):           # another size has no set
            sc.train_loss_grad(2, *random_network(2, (8,), seed=1), first=0, count=10)
        with pytest.raises(ValueError, match="k must be 2..5"):                         # an unknown k
            sc.train_loss_grad(6, widths, params, 0, 10)
        with pytest.raises(ValueError, match="k must be 2..5"):
            sc._check(sc._lib.sdpcut_train_set_data(sc._h, 6, 1, _capi._ptr(X, _capi._dp), _capi._ptr(t, _capi._dp)))
        for first, count in ((0, 41), (40, 1), (-1, 5), (10, 0), (39, 2)):              # a range outside the data
            with pytest.raises(ValueError, match="range"):
                sc.train_loss_grad(k, widths, params, first, count)
        with pytest.raises(ValueError, match="n_params does not match"):                # a mismatched n_params
            sc.train_loss_grad(k, widths, params[:-1], 0, 10)
        with pytest.raises(ValueError, match="share one width"):
            sc.train_loss_grad(k, np.array([8, 9, 1]), params, 0, 10)
        # between round_csr_begin and _end
        wl = synthetic.make_workload(nb_vars=30, k=k, count=500, seed=7)
        sc.set_network(k, *networks.load_network(k))
        sc.set_instance(30, wl["Q_arr"])
        sc.set_candidates(wl["set_inds"], wl["ks"])
        sc.set_point(wl["vars_values"])
        before = sc.train_loss_grad(k, widths, params, 3, 30)
        sc.round_csr_begin(1, 100)
        with pytest.raises(_capi.SdpCutError, match="pending"):
            sc.train_loss_grad(k, widths, params, 3, 30)
        with pytest.raises(_capi.SdpCutError, match="pending"):
            sc.train_set_data(k, X, t)
        sc.round_csr_end()
        after = sc.train_loss_grad(k, widths, params, 3, 30)      # the set survived instance, candidates, point and the round
        assert before[0] == after[0] and before[1].tobytes() == after[1].tobytes()
        sc.train_set_data(k, X[:0], t[:0])                        # dropped
        with pytest.raises(_capi.SdpCutError, match="sdpcut_train_set_data"):
            sc.train_loss_grad(k, widths, params, 0, 10)
    finally:
        sc.close()


def test_train_end_to_end_on_the_device(scorer):
    """k = 2, H = 8, 2048 Table-1 samples labelled by sdp_batch, 100 SCG iterations with the device as back end: the criterion of
    tests/test_train_cpu.py (validation MSE below the affine least-squares fit's), then the network goes into set_network and
    nn_batch reproduces the twin's forward pass."""
    k = 2
    X = networks.sample_table1(k, 2048, seed=3)
    t = scorer.sdp_batch(k, X)[0]
    widths, params, rep = networks.train(k, X, t, hidden=(8,), scorer=scorer, epochs=100, seed=7)
    tl = np.array(rep["train_loss"])
    assert np.all(tl[1:] <= tl[:-1]) and rep["best_val_loss"] == min(rep["val_loss"])
    aff = affine_val_mse(X, t, rep, params[-2])
    print("device-trained: validation MSE %.3e, affine fit %.3e, stop %s after %d iterations, %d gradient evaluations"
          % (rep["best_val_loss"], aff, rep["stop"], rep["iterations"], rep["grad_evals"]))
    assert rep["best_val_loss"] < aff
    scorer.set_network(k, widths, params)
    y = scorer.nn_batch(k, X)
    ref = networks.forward_twin(k, widths, params, X)
    assert np.abs(y - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # the same start trained on the twin: the start and the first step agree (the curvature estimate divides gradient differences
    # by sigma = 5e-5 / |p|, which magnifies rounding differences of 1e-16 to ~1e-12 per step)
    _, _, rep_cpu = networks.train(k, X, t, hidden=(8,), epochs=1, seed=7)
    assert np.allclose(rep_cpu["train_loss"], rep["train_loss"][:2], rtol=1e-9)
