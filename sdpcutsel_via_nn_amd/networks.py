"""Trained MLPs (2D..5D) of the optimality estimator.

The reference bakes the weights into NNs.so (source of truth neural_nets/neural_net_kD.m,
constants section).  Here they live in the data fixture ``data/nn_weights.npz`` (extracted
by tools/extract_weights.py; numbers only, provenance recorded there) and are handed to
the GPU library through ``sdpcut_set_network``.
"""
import os

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "nn_weights.npz")


def load_network(k, path=None):
    """-> (widths int32[n_layers], params float64[...]) in the packing sdpcut_set_network expects:
    xoffset, gain, ymin, (W row-major, b) per layer, y_ymin, y_gain, y_xoffset."""
    z = np.load(path or DATA)
    p = "k%d_" % k
    if p + "W1" not in z:
        raise ValueError("no trained network for %d-variable candidates" % k)
    parts = [z[p + "xoffset"].ravel(), z[p + "gain"].ravel(), np.array([z[p + "ymin"]], dtype=np.float64)]
    widths = []
    layer = 1
    while p + "W%d" % layer in z:
        W = z[p + "W%d" % layer]
        widths.append(W.shape[0])
        parts += [W.ravel(), z[p + "b%d" % layer].ravel()]
        layer += 1
    parts.append(np.array([z[p + "y_ymin"], z[p + "y_gain"], z[p + "y_xoffset"]], dtype=np.float64))
    return np.array(widths, dtype=np.int32), np.concatenate(parts).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# Training a network of one's own: sample -> Scorer.sdp_batch (labels) -> train -> Scorer.set_network.
# The reference trains with MATLAB (neural_nets/train_NNs.m: feedforwardnet + trainscg + dividerand 75/15/10, mapminmax on inputs
# and targets, mse); here the loss and its gradient come from the device (Scorer.train_loss_grad, csrc/train.hip) or from the numpy
# twin below, and Moller's scaled conjugate gradient runs on the host over the flat parameter vector.

MAX_HIDDEN, MAX_LAYERS, INPUT_CLAMP = 64, 5, 3.0      # csrc/net_pack.h
SCG_SIGMA, SCG_LAMBDA = 5e-5, 5e-7                      # trainscg's defaults


def check_network(k, widths, params):
    """The refusals of csrc/net_pack.h (net_check), with its messages: raises ValueError where sdpcut_set_network and
    sdpcut_train_loss_grad return SDPCUT_EINVAL.  -> (d_in, offsets of (W, b) per layer in params, offset of the output mapping)"""
    if k < 2 or k > 5:
        raise ValueError("k must be 2..5")
    n_layers = 0 if widths is None else len(widths)
    if n_layers < 2 or n_layers > MAX_LAYERS or params is None:
        raise ValueError("bad layer description")
    d_in = k * (k + 3) // 2
    H = int(widths[0])
    if int(widths[-1]) != 1:
        raise ValueError("last layer must have one output")
    for w in widths[:-1]:
        if int(w) != H or H < 1 or H > MAX_HIDDEN:
            raise ValueError("hidden layers must share one width <= 64")
    offs, o, fan = [], 2 * d_in + 1, d_in
    for w in widths:
        offs.append((o, o + int(w) * fan))
        o += int(w) * fan + int(w)
        fan = int(w)
    if o + 3 != len(params):
        raise ValueError("n_params does not match the layer description")
    return d_in, offs, o


def split_params(k, widths, params):
    """-> (xoffset, gain, ymin, [W_l [out, in]], [b_l], (y_ymin, y_gain, y_xoffset)): views of params"""
    d_in, offs, tail = check_network(k, widths, params)
    Ws, Bs, fan = [], [], d_in
    for w, (ow, ob) in zip(widths, offs):
        Ws.append(params[ow:ob].reshape(int(w), fan))
        Bs.append(params[ob:ob + int(w)])
        fan = int(w)
    return params[:d_in], params[d_in:2 * d_in], params[2 * d_in], Ws, Bs, params[tail:tail + 3]


def unclamped_ok(k, widths, params):
    """NetPack::unclamped_ok of csrc/net_pack.h: every hidden pre-activation is provably below 40 in magnitude for mapped inputs
    in [-3, 3], AND the mapping sends the documented input domain (x_i in [0, 1], q_m in [-1/k, 1/k]) into [-3, 3], so that the
    input clamp of the clamp-free variant changes no score on the domain.  Then the score kernels run that variant (and the
    one-launch form over all size classes); otherwise the variant with the tansig clamps, which clamps no input."""
    xoffset, gain, ymin, Ws, Bs, _ = split_params(k, widths, np.asarray(params, dtype=np.float64))
    worst = 0.0
    for l, (W, b) in enumerate(zip(Ws[:-1], Bs[:-1])):
        worst = max(worst, float((np.abs(b) + np.abs(W).sum(axis=1) * (INPUT_CLAMP if l == 0 else 1.0)).max()))
    lo = np.where(np.arange(xoffset.shape[0]) < k, 0.0, -1.0 / k)
    hi = np.where(np.arange(xoffset.shape[0]) < k, 1.0, 1.0 / k)
    with np.errstate(invalid="ignore", over="ignore"):
        ends = np.abs(np.stack([(lo - xoffset) * gain + ymin, (hi - xoffset) * gain + ymin]))
    return bool(worst < 40.0 and np.all(ends <= INPUT_CLAMP))


FILTER_EXP_SCALE = -2.8853900817779268147      # -2 log2(e), csrc/net_pack.h
FILTER_MARGIN_CUTOFF = 0.05


def filter_box(k, widths, params):
    """NetPack::filter_box of csrc/net_pack.h: [d_in, 2], the mapped image of the input domain, 1e-9 wider at both ends"""
    xoffset, gain, ymin, _, _, _ = split_params(k, widths, np.asarray(params, dtype=np.float64))
    idx = np.arange(xoffset.shape[0])
    lo, hi = np.where(idx < k, 0.0, -1.0 / k), np.where(idx < k, 1.0, 1.0 / k)
    a, b = (lo - xoffset) * gain + ymin, (hi - xoffset) * gain + ymin
    return np.stack([np.minimum(a, b) - 1e-9, np.maximum(a, b) + 1e-9], axis=1)


def filter_margin(k, widths, params):
    """net_filter_margin of csrc/net_pack.h, restated: the a-priori bound on |y32 - y64| of the unmapped network output for mapped
    inputs inside filter_box, y32 as the fp32 filter of the skipping kernel computes it (the derivation is the comment there):
    per layer  e' = (|w~| A gamma(m) + |b~| gamma(n) + |w~ - c W| A + |b~ - c b| + |c| |W| e) / |c| + 13 u,  the output layer in
    fp64, the output mapping's gain, and 1 + 2^-10."""
    p = np.asarray(params, dtype=np.float64)
    _, _, _, Ws, _, (_, y_gain, _) = split_params(k, widths, p)
    e = _filter_layers(k, widths, p)
    return float((np.abs(Ws[-1][0]) * e).sum() / abs(y_gain) * (1.0 + 2.0 ** -10))


def filter_margin_terms(k, widths, params):
    """net_filter_slope_terms of csrc/net_pack.h, restated: the terms of the margin PER CANDIDATE,
    M = min(filter_margin, (S (1 + 2^-9) + C0) (1 + 2^-10)),  S = sum_j G_j (1 - a_j^2) over the last hidden layer's activations.
    -> (G float64 [64], G rounded up to float32 [64] -- what the kernel multiplies --, C0, e [H]: the a-priori bound on the error of
    those activations).  With delta = e - 13 u the bound on the pre-activations:  G_j = |Wout_j| delta_j / |y_gain|,
    C0 = sum_j |Wout_j| ((27 u + L2 delta_j) delta_j + 13 u) / |y_gain| + (gamma(15) + u) sum_j Gf_j,  L2 = 4 / (3 sqrt 3)."""
    p = np.asarray(params, dtype=np.float64)
    _, _, _, Ws, _, (_, y_gain, _) = split_params(k, widths, p)
    u, L2 = 2.0 ** -24, 4.0 / (3.0 * np.sqrt(3.0))
    e = _filter_layers(k, widths, p)
    delta = e - 13.0 * u
    w = np.abs(Ws[-1][0])
    H = w.shape[0]
    G = np.zeros(64)
    G[:H] = w * delta / abs(y_gain)
    Gf = G.astype(np.float32)
    Gf = np.where(Gf.astype(np.float64) < G, np.nextafter(Gf, np.float32(np.inf)), Gf).astype(np.float32)
    C0 = (w * ((27.0 * u + L2 * delta) * delta + 13.0 * u)).sum() / abs(y_gain)
    C0 += (15.0 * u / (1.0 - 15.0 * u) + u) * float(Gf.astype(np.float64).sum())
    return G, Gf, float(C0), e


def filter_margin_at(k, widths, params, inputs):
    """M of filter_margin_terms for every row of inputs [count, d_in] (the network's own, unmapped inputs), with the last hidden
    layer's activations taken in float64 and G unrounded -> float64 [count].  The device's value (sdpcut_filter_audit_margins)
    differs by what its fp32 activations differ: at most 2 sum_j G_j e_j, and the fp32 sum's 2^-9."""
    p = np.asarray(params, dtype=np.float64)
    xoffset, gain, ymin, Ws, Bs, _ = split_params(k, widths, p)
    G, _, C0, _ = filter_margin_terms(k, widths, p)
    a = (np.asarray(inputs, dtype=np.float64) - xoffset) * gain + ymin
    for W, b in zip(Ws[:-1], Bs[:-1]):
        a = _tansig(a @ W.T + b)
    S = (1.0 - a * a) @ G[:a.shape[1]]
    return np.minimum(filter_margin(k, widths, p), (S * (1.0 + 2.0 ** -9) + C0) * (1.0 + 2.0 ** -10))


def _filter_layers(k, widths, params):
    """net_filter_layers of csrc/net_pack.h: the a-priori bound e [H] on the error of the last hidden layer's fp32 activations"""
    p = np.asarray(params, dtype=np.float64)
    xoffset, gain, ymin, Ws, Bs, (y_ymin, y_gain, y_xoffset) = split_params(k, widths, p)
    u, c = 2.0 ** -24, FILTER_EXP_SCALE

    def gamma(m):
        return m * u / (1.0 - m * u)

    Bx = np.abs(filter_box(k, widths, p)).max(axis=1)
    e, A = u * Bx, (1.0 + u) * Bx
    for l, (W, b) in enumerate(zip(Ws[:-1], Bs[:-1])):
        fan = W.shape[1]
        j = np.arange(fan)
        if l == 0:
            before = 4 * (j // 4)      # k-step s holds inputs 4 s .. 4 s + 3
        else:                          # k-step (t, i) holds neurons 16 t + 4 q + i, q = 0..3: the live terms in front of it
            before = np.zeros(fan, dtype=np.int64)
            cnt = 0
            for t in range(4):
                for i in range(4):
                    live = [16 * t + 4 * q + i for q in range(4) if 16 * t + 4 * q + i < fan]
                    before[live] = cnt
                    cnt += len(live)
        wt = (c * W).astype(np.float32).astype(np.float64)
        bt = (c * b).astype(np.float32).astype(np.float64)
        H = W.shape[0]
        tail = 48 < H <= 52                    # tail rows 48 .. H - 1: a lane chain and a two-level tree on the VALU
        if tail and l > 0:                     # the tail neurons of the layer in front share ONE k-step, neuron 48 + v on q = v
            before[48:] = 48
        m = np.tile(fan - before, (H, 1))      # roundings term j sees in row i
        mb = np.full(H, fan)                   # ... and the bias
        if tail:
            if l == 0:                         # lane q chains inputs q, 4 + q, ..: `live` of them
                mt = (fan - j % 4 + 3) // 4 - j // 4 + 2
                mbt = (fan + 3) // 4 + 2
            else:                              # b on q = 0, tail neuron 48 + v of the layer in front on q = v, then links 4 tk + i of twelve
                mt = np.where(j < 48, 12 - (4 * (j // 16) + j % 4) + 2, 1 + 12 + 2)
                mbt = 1 + 12 + 2
            m[48:] = mt
            mb[48:] = mbt
        acc = np.abs(bt) * gamma(mb) + np.abs(bt - c * b)
        acc = acc + (np.abs(wt) * (A * gamma(m)) + np.abs(wt - c * W) * A + np.abs(c * W) * e).sum(axis=1)
        e = acc / abs(c) + 13.0 * u
        A = np.full(W.shape[0], 1.0 + 8.0 * u)
    return e


def filter_ok(k, widths, params):
    """NetPack::filter_ok: clamp-free, the shipped 3-variable shape (three hidden layers of 50), margin below the cut-off"""
    return bool(unclamped_ok(k, widths, params) and k == 3 and [int(w) for w in widths] == [50, 50, 50, 1]
                and filter_margin(k, widths, params) < FILTER_MARGIN_CUTOFF)


def _tansig(n):
    return 2.0 / (1.0 + np.exp(-2.0 * n)) - 1.0


def forward_twin(k, widths, params, inputs, dtype=np.float64, normalised=False):
    """The network's output on inputs [count, d_in] in `dtype` arithmetic, without the input clamp: what sdpcut_nn_batch returns,
    or with normalised=True the y_n of the training loss (before the output mapping is undone)."""
    params = np.asarray(params).astype(dtype)
    xoffset, gain, ymin, Ws, Bs, (y_ymin, y_gain, y_xoffset) = split_params(k, widths, params)
    a = (np.asarray(inputs).astype(dtype) - xoffset) * gain + ymin
    for W, b in zip(Ws[:-1], Bs[:-1]):
        a = _tansig(a @ W.T + b)
    y = a @ Ws[-1][0] + Bs[-1][0]
    return y if normalised else (y - y_ymin) / y_gain + y_xoffset


def loss_grad_twin(k, widths, params, inputs, targets, dtype=np.float64):
    """Plain numpy backprop of the loss sdpcut_train_loss_grad defines (include/sdpcut.h): the mean over the samples of
    (y_n - t_n)^2 in normalised units, tansig(n) = 2 / (1 + exp(-2n)) - 1, no input clamp -> (loss, grad) with grad = d loss / d(W, b)
    of every layer in the order of params.  All arithmetic in `dtype` (np.longdouble for a reference).  The checker of the device
    kernel and the CPU back end of train()."""
    params = np.asarray(params).astype(dtype)
    xoffset, gain, ymin, Ws, Bs, (y_ymin, y_gain, y_xoffset) = split_params(k, widths, params)
    x = np.asarray(inputs).astype(dtype)
    t = np.asarray(targets).astype(dtype)
    count = x.shape[0]
    if x.ndim != 2 or x.shape[1] != k * (k + 3) // 2 or t.shape != (count,) or count < 1:
        raise ValueError("inputs must be [count, k(k+3)/2] and targets [count], count >= 1")
    acts = [(x - xoffset) * gain + ymin]
    for W, b in zip(Ws[:-1], Bs[:-1]):
        acts.append(_tansig(acts[-1] @ W.T + b))
    y = acts[-1] @ Ws[-1][0] + Bs[-1][0]
    e = y - ((t - y_xoffset) * y_gain + y_ymin)
    loss = (e * e).sum() / dtype(count)
    delta = (dtype(2) * e / dtype(count))[:, None]            # d loss / d y_n
    grads = []
    for l in range(len(Ws) - 1, -1, -1):
        grads.append(delta.sum(axis=0))                       # db_l
        grads.append((delta.T @ acts[l]).ravel())             # dW_l
        if l > 0:
            delta = (delta @ Ws[l]) * (dtype(1) - acts[l] * acts[l])
    return loss, np.concatenate(grads[::-1])


def sample_table1(k, count, seed=7):
    """The sampling of the paper's Table 1 (utilities.py: gen_data_ndim) -> rows [x | Q_slice], float64 [count, k(k+3)/2], the
    layout Scorer.sdp_batch and Scorer.nn_batch take.  Q = V diag(lam) V^T with V Haar-distributed orthogonal (QR of a Gaussian
    matrix, columns multiplied by the signs of R's diagonal) and lam uniform in [-1, 1]; x uniform in [0, 1]; Q_slice is the upper
    triangle row-major with the off-diagonal entries DOUBLED (Q = triu(Q, 1) + triu(Q, 0), utilities.py:48).
    Same distribution as the reference's scipy.stats.ortho_group + numpy.random.seed stream, NOT the same numbers: the draws
    come from numpy's Generator(PCG64(seed)) in one batch."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((count, k, k))
    lam = rng.uniform(-1.0, 1.0, (count, k))
    x = rng.uniform(0.0, 1.0, (count, k))
    V, R = np.linalg.qr(G)
    V = V * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]
    Q = np.einsum("nij,nj,nkj->nik", V, lam, V)
    Q = 0.5 * (Q + np.transpose(Q, (0, 2, 1)))
    ia, ib = np.triu_indices(k)
    return np.concatenate([x, np.where(ia == ib, 1.0, 2.0) * Q[:, ia, ib]], axis=1)


def _mapminmax(a):
    """MATLAB's mapminmax onto [-1, 1] per column -> (xoffset, gain); a constant column keeps gain 1"""
    lo, hi = a.min(axis=0), a.max(axis=0)
    rng = hi - lo
    return lo, np.where(rng > 0, 2.0 / np.where(rng > 0, rng, 1.0), 1.0)


def init_network(k, hidden, inputs, targets, seed=7):
    """Seeded start of train(): mapping constants from the data (mapminmax), weights and biases uniform in +-sqrt(6 / (fan_in +
    fan_out)) (not MATLAB's initnw) -> (widths int32, params float64) in the packing of sdpcut_set_network."""
    rng = np.random.default_rng(seed)
    d_in = k * (k + 3) // 2
    widths = np.array(list(hidden) + [1], dtype=np.int32)
    xoffset, gain = _mapminmax(np.asarray(inputs, dtype=np.float64))
    y_xoffset, y_gain = _mapminmax(np.asarray(targets, dtype=np.float64)[:, None])
    parts, fan = [xoffset, gain, np.array([-1.0])], d_in
    for w in widths:
        a = np.sqrt(6.0 / (fan + int(w)))
        parts += [rng.uniform(-a, a, int(w) * fan), rng.uniform(-a, a, int(w))]
        fan = int(w)
    parts.append(np.array([-1.0, float(y_gain[0]), float(y_xoffset[0])]))
    params = np.concatenate(parts).astype(np.float64)
    check_network(k, widths, params)
    return widths, params


def train(k, inputs, targets, hidden=(50, 50, 50), scorer=None, epochs=1000, max_fail=100, min_grad=1e-6,
          split=(0.75, 0.15, 0.10), seed=7):
    """Train a tansig MLP on (inputs [count, k(k+3)/2], targets [count]) -> (widths, params, report); (widths, params) go straight
    into Scorer.set_network.

    What train_NNs.m does with MATLAB's toolbox: mapminmax on inputs and targets (the mapping constants are part of params and
    stay fixed), a random train / validation / test split, mse in normalised units, Moller's scaled conjugate gradient with
    trainscg's defaults (sigma 5e-5, lambda 5e-7): two gradient evaluations per iteration, a step is accepted only if the train
    loss does not increase.  Stops after `epochs` iterations, after `max_fail` iterations in a row whose validation loss is above
    the best one seen, or when the gradient's norm falls below `min_grad`; the weights of the best validation loss are returned.
    The start is seeded (init_network), not MATLAB's initnw; trajectories are not MATLAB's.

    scorer=None: loss and gradient from loss_grad_twin on the CPU.  With a Scorer the samples become its resident training set of
    size k (train_set_data, permuted so that the three parts are ranges) and every evaluation runs on the device.  That REPLACES
    whatever training set of size k the Scorer held, and the permuted samples stay resident after the call (train_set_data with
    an empty set drops them).

    report: train_loss / val_loss per iteration (entry 0 = the start), stop ('epochs' | 'max_fail' | 'min_grad'), iterations,
    best_iteration, best_val_loss, test_loss, grad_evals, unclamped_ok (net_pack's status of the returned network: whether the
    score kernels run their clamp-free variant on it), perm (the permutation of the samples: sample perm[i] is row i of the
    permuted -- and, with a Scorer, resident -- set) and split ({'train' | 'val' | 'test': (first, count)}, ranges of that set)."""
    inputs = np.ascontiguousarray(inputs, dtype=np.float64)
    targets = np.ascontiguousarray(targets, dtype=np.float64)
    count = targets.shape[0]
    widths, w0 = init_network(k, hidden, inputs, targets, seed)
    d_in = k * (k + 3) // 2
    lo, hi = 2 * d_in + 1, w0.shape[0] - 3              # the trainable slice of params
    perm = np.random.default_rng(seed + 1).permutation(count)
    n_tr = int(round(split[0] * count))
    n_va = int(round(split[1] * count))
    if n_tr < 1 or n_va < 1 or n_tr + n_va > count:
        raise ValueError("the split leaves the training or the validation part empty")
    X, T = inputs[perm], targets[perm]
    parts = {"train": (0, n_tr), "val": (n_tr, n_va), "test": (n_tr + n_va, count - n_tr - n_va)}
    if scorer is not None:
        scorer.train_set_data(k, X, T)
    evals = [0]

    def full(w):
        p = w0.copy()
        p[lo:hi] = w
        return p

    def fg(w, part, want_grad=True):
        first, cnt = parts[part]
        evals[0] += 1 if want_grad else 0
        if scorer is not None:
            return scorer.train_loss_grad(k, widths, full(w), first, cnt, want_grad=want_grad)
        f, g = loss_grad_twin(k, widths, full(w), X[first:first + cnt], T[first:first + cnt])
        return float(f), g

    w = w0[lo:hi].copy()
    f, g = fg(w, "train")
    r, p = -g, -g
    lam, lam_bar, success, delta, stop = SCG_LAMBDA, 0.0, True, 0.0, "epochs"
    fv = fg(w, "val", False)[0]
    best = (fv, w.copy(), 0)
    fails = 0
    train_loss, val_loss = [f], [fv]
    n = w.shape[0]
    it = 0
    for it in range(1, int(epochs) + 1):
        pp = float(p @ p)
        if pp == 0.0 or np.sqrt(float(r @ r)) < min_grad:
            stop, it = "min_grad", it - 1
            break
        if success:                                    # second-order information along p
            sig = SCG_SIGMA / np.sqrt(pp)
            s = (fg(w + sig * p, "train")[1] - g) / sig
            delta = float(p @ s)
        delta += (lam - lam_bar) * pp
        if delta <= 0.0:                               # make the Hessian estimate positive definite
            lam_bar = 2.0 * (lam - delta / pp)
            delta = -delta + lam * pp
            lam = lam_bar
        mu = float(p @ r)
        alpha = mu / delta
        w_new = w + alpha * p
        f_new, g_new = fg(w_new, "train")
        Delta = 2.0 * delta * (f - f_new) / (mu * mu)
        if Delta >= 0.0 and np.isfinite(f_new):       # accepted: the train loss did not increase
            r_new = -g_new
            lam_bar, success = 0.0, True
            if it % n == 0:
                p = r_new
            else:
                p = r_new + (float(r_new @ r_new) - float(r_new @ r)) / mu * p
            w, f, g, r = w_new, f_new, g_new, r_new
            if Delta >= 0.75:
                lam *= 0.25
        else:
            lam_bar, success = lam, False
        if not (Delta >= 0.25):                        # poor agreement with the quadratic model: raise the scale
            lam = lam + delta * (1.0 - Delta) / pp if np.isfinite(Delta) else 2.0 * lam
        fv = fg(w, "val", False)[0] if success else val_loss[-1]
        train_loss.append(f)
        val_loss.append(fv)
        if fv < best[0]:
            best, fails = (fv, w.copy(), it), 0
        elif fv > best[0]:
            fails += 1
            if fails >= max_fail:
                stop = "max_fail"
                break
    params = full(best[1])
    report = dict(train_loss=train_loss, val_loss=val_loss, stop=stop, iterations=it, best_iteration=best[2],
                  best_val_loss=best[0], test_loss=fg(best[1], "test", False)[0] if parts["test"][1] > 0 else float("nan"),
                  grad_evals=evals[0], unclamped_ok=bool(unclamped_ok(k, widths, params)), split=dict(parts), perm=perm)
    return widths, params, report
