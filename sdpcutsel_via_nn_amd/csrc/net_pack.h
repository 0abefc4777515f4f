// Host packing of one trained MLP into the device blob behind NetDev (common.h).  Plain C++, pure arithmetic:
// tests/test_net_pack.py compiles this header with the host compiler and compares the blob bit for bit.
#pragma once
#include <cmath>
#include <cstring>
#include <stdint.h>
#include <vector>

#include "../../include/sdpcut.h"

#define MAX_HIDDEN 64
#define MAX_LAYERS 5
#define SDPCUT_INPUT_CLAMP 3.0

// blob = inmap | bias | bias_q | wout | raw W,b per layer | A-fragments | tail rows | VALU packing; o_* = offsets in doubles
struct NetPack {
    std::vector<double> blob;
    size_t o_inmap, o_bias, o_bias_q, o_wout, o_frag, o_wtail, o_wvalu, o_rw[MAX_LAYERS], o_rb[MAX_LAYERS];
    int d_in, n_hidden, width, s0, sh, unclamped_ok;
    double ymin, b_out, y_ymin, y_gain, y_xoffset;
};

// What the library accepts as a network description (sdpcut_set_network, and sdpcut_train_loss_grad through the same lines):
// -> SDPCUT_OK, or SDPCUT_EINVAL with *why set.
static inline int net_check(int k, int n_layers, const int32_t *widths, const double *params, int64_t n_params, const char **why)
{
    auto refuse = [&](const char *msg) { *why = msg; return SDPCUT_EINVAL; };
    if (k < 2 || k > SDPCUT_MAX_K) return refuse("k must be 2..5");
    if (n_layers < 2 || n_layers > MAX_LAYERS || !widths || !params) return refuse("bad layer description");
    const int d_in = k * (k + 3) / 2;
    const int nh = n_layers - 1;
    const int H = widths[0];
    if (widths[n_layers - 1] != 1) return refuse("last layer must have one output");
    for (int l = 0; l < nh; ++l)
        if (widths[l] != H || H < 1 || H > MAX_HIDDEN) return refuse("hidden layers must share one width <= 64");
    int64_t need = 2 * d_in + 1 + 3;
    {
        int fan = d_in;
        for (int l = 0; l < n_layers; ++l) { need += (int64_t)widths[l] * fan + widths[l]; fan = widths[l]; }
    }
    if (need != n_params) return refuse("n_params does not match the layer description");
    return SDPCUT_OK;
}

// params = xoffset[d_in] | gain[d_in] | ymin | (W, b) per layer | y_ymin, y_gain, y_xoffset  (sdpcut_set_network).
// -> SDPCUT_OK, or SDPCUT_EINVAL with *why set.
static inline int net_pack(int k, int n_layers, const int32_t *widths, const double *params, int64_t n_params, NetPack *out,
                           const char **why)
{
    if (net_check(k, n_layers, widths, params, n_params, why) != SDPCUT_OK) return SDPCUT_EINVAL;
    const int d_in = k * (k + 3) / 2;
    const int nh = n_layers - 1;
    const int H = widths[0];

    // ---- unpack
    const double *p = params;
    const double *xoffset = p; p += d_in;
    const double *gain = p; p += d_in;
    out->ymin = *p++;
    const double *W[MAX_LAYERS], *B[MAX_LAYERS];
    {
        int fan = d_in;
        for (int l = 0; l < n_layers; ++l) {
            W[l] = p; p += (int64_t)widths[l] * fan;
            B[l] = p; p += widths[l];
            fan = widths[l];
        }
    }
    out->y_ymin = p[0]; out->y_gain = p[1]; out->y_xoffset = p[2];
    out->b_out = B[nh][0];

    // ---- pack the device blob: inmap | bias | wout | raw W,b | A-fragments
    const int T = 4;
    const int s0 = (d_in + 3) / 4, sh = (H + 3) / 4;
    out->d_in = d_in; out->n_hidden = nh; out->width = H; out->s0 = s0; out->sh = sh;
    std::vector<double> &blob = out->blob;
    blob.clear();
    auto reserve = [&](size_t n) { size_t o = blob.size(); blob.resize(o + n, 0.0); return o; };
    const size_t o_inmap = out->o_inmap = reserve(2 * d_in);
    for (int i = 0; i < d_in; ++i) { blob[o_inmap + i] = xoffset[i]; blob[o_inmap + d_in + i] = gain[i]; }
    const size_t o_bias = out->o_bias = reserve((size_t)nh * 64);
    for (int l = 0; l < nh; ++l)
        for (int j = 0; j < H; ++j) blob[o_bias + l * 64 + j] = B[l][j];
    const size_t o_bias_q = out->o_bias_q = reserve((size_t)nh * 64);
    for (int l = 0; l < nh; ++l)
        for (int j = 0; j < H; ++j) blob[o_bias_q + l * 64 + j] = -0.25 * B[l][j];
    const size_t o_wout = out->o_wout = reserve(64);
    for (int j = 0; j < H; ++j) blob[o_wout + j] = W[nh][j];
    {
        int fan = d_in;
        for (int l = 0; l < n_layers; ++l) {
            out->o_rw[l] = reserve((size_t)widths[l] * fan);
            std::memcpy(&blob[out->o_rw[l]], W[l], sizeof(double) * widths[l] * fan);
            out->o_rb[l] = reserve(widths[l]);
            std::memcpy(&blob[out->o_rb[l]], B[l], sizeof(double) * widths[l]);
            fan = widths[l];
        }
    }
    // A-fragment of v_mfma_f64_16x16x4_f64: lane l holds A[row = l & 15][k = l >> 4]
    // => frag[t][s][l] = W[16 t + (l & 15)][4 s + (l >> 4)], zero outside the matrix
    out->o_frag = reserve((size_t)T * (s0 + (size_t)(nh - 1) * sh) * 64);
    {
        size_t o = out->o_frag;
        int fan = d_in;
        for (int l = 0; l < nh; ++l) {
            const int S = (l == 0) ? s0 : sh;
            for (int t = 0; t < T; ++t)
                for (int s = 0; s < S; ++s)
                    for (int ln = 0; ln < 64; ++ln) {
                        const int row = 16 * t + (ln & 15), col = 4 * s + (ln >> 4);
                        // pre-scaled by -1/4 (exact: a power of two), see NetDev::bias_q
                        blob[o++] = (row < H && col < fan) ? -0.25 * W[l][(size_t)row * fan + col] : 0.0;
                    }
            fan = H;
        }
    }
    // rows 48..51 of every hidden layer, for the VALU tail of the MFMA kernel: [layer][4][64]
    const size_t o_wtail = out->o_wtail = reserve((size_t)nh * 4 * 64);
    {
        int fan = d_in;
        for (int l = 0; l < nh; ++l) {
            for (int u = 0; u < 4; ++u)
                for (int i = 0; i < fan; ++i)
                    if (48 + u < H) blob[o_wtail + ((size_t)l * 4 + u) * 64 + i] = -0.25 * W[l][(size_t)(48 + u) * fan + i];
            fan = H;
        }
    }
    // scalar-operand packing of the VALU kernel: [layer][j/8][i][j%8]
    const int NBv = (H + 7) / 8;
    // (+16: the kernel streams the weights in 16-double batches and may read past an odd fan-in)
    out->o_wvalu = reserve((size_t)NBv * 8 * ((size_t)d_in + (size_t)(nh - 1) * H) + 16);
    {
        size_t o = out->o_wvalu;
        int fan = d_in;
        for (int l = 0; l < nh; ++l) {
            for (int jb = 0; jb < NBv; ++jb)
                for (int i = 0; i < fan; ++i)
                    for (int jj = 0; jj < 8; ++jj) {
                        const int j = jb * 8 + jj;
                        blob[o++] = (j < H) ? W[l][(size_t)j * fan + i] : 0.0;
                    }
            fan = H;
        }
    }
    {
        // bound of every hidden pre-activation: |n_j| <= sum_i |W_ji| max|in_i| + |b_j| with |in| <= SDPCUT_INPUT_CLAMP
        // for the mapped inputs (the clamp-free kernel cuts them there; the shipped mappings send x in [0,1], |q| <= 1/k into
        // [-1,1]) and <= 1 behind a tansig.  The tansig4 path
        // needs -2n <= 176, the tail rows -2n <= 704; 80 leaves a factor of two.
        double worst = 0.0;
        int fan = d_in;
        for (int l = 0; l < nh; ++l) {
            const double in_max = l == 0 ? SDPCUT_INPUT_CLAMP : 1.0;
            for (int j = 0; j < H; ++j) {
                double acc = std::fabs(B[l][j]);
                for (int i = 0; i < fan; ++i) acc += std::fabs(W[l][(size_t)j * fan + i]) * in_max;
                worst = acc > worst ? acc : worst;
            }
            fan = H;
        }
        // ... and the clamp-free variant clamps the mapped inputs to +-SDPCUT_INPUT_CLAMP, which is what makes the bound a proof.
        // It may only run where that clamp cannot change a score: the image of the documented input domain -- x_i in [0, 1] for
        // i < k, q_m in [-1/k, 1/k] behind them (Q_slice / max_elem, max_elem = k max|Q_slice|) -- under
        // v -> (v - xoffset_i) gain_i + ymin must lie in [-3, 3] for every input (an affine map: its two endpoints decide).
        // True of the shipped mappings (gain ~ 2, ymin -1); a network trained on a narrower range (x in [0.4, 0.6]: gain 10) maps
        // [0, 1] onto [-5, 5] and takes the CLAMP = true instantiation, which clamps no input and needs no bound.
        bool domain_ok = true;
        for (int i = 0; i < d_in; ++i) {
            const double lo = i < k ? 0.0 : -1.0 / (double)k, hi = i < k ? 1.0 : 1.0 / (double)k;
            const double a = (lo - xoffset[i]) * gain[i] + out->ymin, b = (hi - xoffset[i]) * gain[i] + out->ymin;
            // (written so that a NaN fails)
            if (!(std::fabs(a) <= SDPCUT_INPUT_CLAMP && std::fabs(b) <= SDPCUT_INPUT_CLAMP)) domain_ok = false;
        }
        out->unclamped_ok = (worst < 40.0 && domain_ok) ? 1 : 0;      // |n| < 40  <=>  -2n < 80
    }
    return SDPCUT_OK;
}
