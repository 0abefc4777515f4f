"""The premises of tests/test_gpu_user_networks.py, checked without a GPU: the long double reference restates the right operation
(against the oracle on the shipped networks), every generated network lies on the intended side of both conditions of
unclamped_ok, the allowances of the two tolerance rules (user_nets.py) stay below what the suite demands of shipped networks
today, the list lengths hit the score_plan branches they are chosen for, and the divergence the narrow-domain network exposes on
a library without the domain condition, stated on the CPU."""
import numpy as np
import pytest

import user_nets as un
from sdpcutsel_via_nn_amd import networks

LD = np.longdouble


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    return un.compile_plan(tmp_path_factory.mktemp("user_plan"))


def _lists(oracle, k, seed=0):
    """the base list of size k at the two points of the GPU tests -> [(name, x, q, max_elem, negSM)]"""
    Q = un.instance(100 + seed)
    sets = un.base_sets(k, 200 + k)
    return Q, sets, [(name, vv) + un.inputs_of(oracle, sets, k, un.N_VARS, vv, Q)
                     for name, vv in (("generic", un.generic_point(300 + seed)), ("corner", un.corner_point(400 + seed)))]


def test_long_double_reference_is_the_oracles_operation(oracle):
    """on the shipped networks the reference agrees with oracle.opt_score_batch (bit-exact against the real reference) to the
    library-exp rule, and inputs_of gives the inputs the oracle's records hold, bit for bit"""
    for k in (2, 3, 4, 5):
        widths, params = networks.load_network(k)
        Q, sets, lists = _lists(oracle, k)
        for name, vv, x, q, max_elem, negSM in lists:
            ref = un.Reference(k, widths, params, x, q, max_elem, negSM)
            got = oracle.opt_score_batch(k, sets, un.N_VARS, vv, Q)
            r = ref.check_lib(got, "oracle, shipped k = %d, %s point" % (k, name))
            assert r <= un.LIB_FACTOR
            assert np.all(np.abs(got - ref.f64) <= un.fuzz_tolerance(got))
        # the records, entry by entry (the literal reference loop), on a few candidates
        L = un.N_VARS * (un.N_VARS + 1) // 2
        name, vv, x, q, max_elem, negSM = lists[0]
        for i in (0, 1, 17, un.BASE - 1):
            rec = oracle.candidate_record([int(v) for v in sets[i]], un.N_VARS, list(Q))
            assert np.array_equal(np.asarray(rec[2], dtype=np.float64), q[i]) and float(rec[3]) == max_elem[i]
            obj, curr_pt, X_slice = oracle.opt_score_entry(rec, vv[:L], vv[L:])
            assert np.array_equal(np.asarray(curr_pt), x[i])
            y = oracle.nn_scalar(k, list(curr_pt) + list(rec[2]))
            assert obj == negSM[i] + y * max_elem[i]      # the composition in the reference's order


def test_generated_networks_lie_where_they_are_meant_to():
    nets = [(k, H, nh, b, un.make_network(k, H, nh, b, 10 * i + 1)) for i, (k, H, nh, b) in enumerate(un.NN_BATCH_GRID)]
    nets += [(k,) + un.SHAPES[k] + (b, un.shaped_network(k, b)) for k in (2, 3, 4, 5) for b in un.BOUNDS]
    nets += [(k, 49, 2, 12.0, un.unshaped_network(k)) for k in (2, 3, 4, 5)]
    for k, H, nh, b, (widths, params) in nets:
        got = un.net_bound(k, widths, params)
        assert abs(got - b) <= 1e-9 * b and not 39.0 <= got <= 41.0, (k, H, nh, b, got)
        assert list(widths) == [H] * nh + [1]
        img = un.domain_image(k, widths, params)
        assert np.abs(img).max() <= 1.05, (k, H, nh, img)      # the domain condition holds with a wide margin
        assert networks.unclamped_ok(k, widths, params) == (b < 40.0), (k, H, nh, b)
    # the grid of the nn_batch test covers what the issue lists, every value of every axis at least twice
    ks, Hs, nhs, bs = (list(c) for c in zip(*un.NN_BATCH_GRID))
    assert 22 <= len(un.NN_BATCH_GRID) <= 26
    assert set(ks) == {2, 3, 4, 5} and set(Hs) >= {1, 3, 16, 47, 48, 49, 52, 53, 63, 64} and set(nhs) == {1, 2, 3, 4} and set(bs) == set(un.BOUNDS)
    for axis in (ks, Hs, nhs, bs):
        assert min(axis.count(v) for v in set(axis) if v != 50) >= 2
    assert (4, 64, 4, 41.5) in un.NN_BATCH_GRID or any(g[1:3] == (64, 4) for g in un.NN_BATCH_GRID)
    assert any(g[1:3] == (1, 1) for g in un.NN_BATCH_GRID)
    # the shipped networks stay clamp-free
    for k in (2, 3, 4, 5):
        widths, params = networks.load_network(k)
        assert networks.unclamped_ok(k, widths, params) and un.net_bound(k, widths, params) < 32.0
        assert tuple(int(w) for w in widths) == (un.SHAPES[k][0],) * un.SHAPES[k][1] + (1,)


def test_narrow_domain_network_fails_the_domain_condition_only(oracle):
    """small weights (bound 12 < 40) behind a mapping of x in [0.375, 0.625]: [0, 1] goes to [-4, 4].  unclamped_ok is false by the
    domain condition alone.  The divergence of a library WITHOUT that condition, stated on the CPU: the twin with its mapped inputs
    cut at +-3 (what the clamp-free kernel computes) and the true twin differ by orders of magnitude more than the allowance of
    the fast-tansig rule, at the corner point and at the generic one."""
    for k in (2, 3, 4, 5):
        widths, params = un.narrow_network(k)
        assert abs(un.net_bound(k, widths, params) - 12.0) <= 1e-8
        img = un.domain_image(k, widths, params)
        assert np.abs(img[:, :k]).min() > 3.9 and np.abs(img[:, k:]).max() < 1.05      # the x inputs leave [-3, 3], the q inputs do not
        assert not networks.unclamped_ok(k, widths, params)
        wide = params.copy()      # the same weights behind the ordinary mapping: clamp-free
        wide[:2 * (k * (k + 3) // 2)] = un.shaped_network(k, 12.0)[1][:2 * (k * (k + 3) // 2)]
        assert networks.unclamped_ok(k, widths, wide)
        Q, sets, lists = _lists(oracle, k)
        xoffset, gain, ymin, _, _, _ = networks.split_params(k, widths, params)
        for name, vv, x, q, max_elem, negSM in lists:
            ref = un.Reference(k, widths, params, x, q, max_elem, negSM)
            # inputs whose MAPPED value is cut at +-3, mapped back: what the clamp-free kernel would feed the network
            raw = np.concatenate([x, q], axis=1)
            cut = np.clip((raw - xoffset) * gain + ymin, -3.0, 3.0)
            back = (cut - ymin) / gain + xoffset
            clamped = un.obj_reference(k, widths, params, back[:, :k], back[:, k:], max_elem, negSM, dtype=LD)
            d = un.normwise(clamped, ref.ld)
            print("k = %d, %s point: clamped-input twin vs true twin %.3e, allowance %.3e" % (k, name, d, ref.fast_allowance))
            assert d > 1e6 * ref.fast_allowance and d > 1e-6, (k, name, d, ref.fast_allowance)


def test_allowances_stay_below_the_fuzz_rule(oracle):
    """The new rules are normwise, the rule test_gpu_fuzz.py applies to shipped networks today is elementwise:
    |dev_i - ref_i| <= t_i = 1e-9 max(|ref_i|, 1e-3 max|ref|) + 1e-9.  Compared like with like: an error vector at the fuzz rule's
    limits has the norm ||t||_2, so the fuzz rule's normwise allowance is ||t||_2 / ||ref||_2 >= 1e-9, and every allowance of the
    new rules must lie below it -- for every network, list length and point of section c.  They do by more than two orders of
    magnitude (printed with -s), which also covers an error that is not spread evenly: the largest share of the error norm a
    single candidate could take before the elementwise rule noticed is printed beside it."""
    worst, worst_single = 0.0, 0.0
    for k in (2, 3, 4, 5):
        Q, sets, lists = _lists(oracle, k)
        nets = [un.shaped_network(k, b) for b in (12.0, 41.5, 700.0)] + [un.narrow_network(k), un.unshaped_network(k)]
        for widths, params in nets:
            for name, vv, x, q, max_elem, negSM in lists:
                full = un.Reference(k, widths, params, x, q, max_elem, negSM)
                for N in un.LIST_LENGTHS:
                    ref = full.part(np.arange(N) % un.BASE)
                    norm = float(np.sqrt((ref.ld ** 2).sum()))
                    tol = un.fuzz_tolerance(ref.f64)
                    fuzz_normwise = float(np.sqrt((tol ** 2).sum())) / norm
                    assert fuzz_normwise >= 1e-9
                    for a in (ref.fast_allowance, ref.lib_allowance):
                        worst = max(worst, a / fuzz_normwise)
                        worst_single = max(worst_single, a * norm / tol.min())
                        assert a <= 1e-2 * fuzz_normwise, (k, name, N, a, fuzz_normwise)
                    assert 0.0 < ref.twin_err < 1e-11 and 0.0 < ref.noisy_err < 1e-11      # (sanity: a few ulps amplified by the network)
    print("largest allowance / fuzz rule's normwise allowance: %.3g; allowance x ||ref|| / smallest elementwise tolerance: %.3g"
          % (worst, worst_single))


def test_nn_batch_allowances(oracle):
    """the same for the nn_batch grid: 257 inputs, all-corner rows included; the twin's error is what float64 gives (a few ulps)"""
    for i, (k, H, nh, b) in enumerate(un.NN_BATCH_GRID):
        widths, params = un.make_network(k, H, nh, b, 10 * i + 1)
        X = un.nn_batch_inputs(k, 500 + i)
        assert X.shape == (257, k * (k + 3) // 2)
        corner = X[-32:]
        assert set(np.unique(corner[:, :k])) <= {0.0, 1.0} and np.all(np.abs(corner[:, k:]) == 1.0 / k)
        with np.errstate(over="ignore"):
            ref = networks.forward_twin(k, widths, params, X, dtype=LD)
            f64 = networks.forward_twin(k, widths, params, X)
        e = un.normwise(f64, ref)
        assert np.all(np.isfinite(f64)) and 0.0 < e < 1e-11, (k, H, nh, b, e)
        tol = 1e-9 * np.maximum(np.abs(f64), 1e-3 * np.abs(f64).max()) + 1e-9
        assert un.LIB_FACTOR * e <= 1e-2 * float(np.sqrt((tol ** 2).sum()) / np.sqrt((ref ** 2).sum())), (k, H, nh, b, e)


def test_list_lengths_hit_their_plan_branches(plan_lib):
    """against the compiled header, as tests/test_score_plan.py reads it; the GPU test repeats the check with the CU count it reads
    from the device"""
    nb = un.check_plan_branches(plan_lib, 256)
    assert nb == 524288 + 471860 == un.balanced_length(256)      # about 1.0e6 at 256 CUs
    # the mixed list of the launch-form test: four classes, every one in strips of 32
    for k, n in un.MIXED_COUNTS.items():
        assert un.plan(plan_lib, n, 256, K=k)["strip"] == 32
    assert sorted(un.MIXED_COUNTS.values()) == [1, 7, 40, 3000]
