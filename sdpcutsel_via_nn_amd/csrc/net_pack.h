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

#define MAX_DIN 20                          /* k (k + 3) / 2 at k = 5 */
// The fp32 filter of the skipping kernel (score_mfma.hip, stage F) evaluates tansig as 2 / (1 + 2^z) - 1 with z = FILTER_EXP_SCALE n:
// the scale -2 log2(e) is folded into its copies of the hidden layers' weights and biases.
#define FILTER_EXP_SCALE (-2.8853900817779268147)
// a network filters only if the proven bound on |y32 - y64| is below this (see net_filter_margin)
#define FILTER_MARGIN_CUTOFF 0.05

// blob = inmap | bias | bias_q | wout | raw W,b per layer | A-fragments | tail rows | VALU packing; o_* = offsets in doubles
// f32 (only where filter_ok) = input-layer A-fragments | hidden-layer A-fragments | biases; o32_* = offsets in floats
struct NetPack {
    std::vector<double> blob;
    size_t o_inmap, o_bias, o_bias_q, o_wout, o_frag, o_wtail, o_wvalu, o_rw[MAX_LAYERS], o_rb[MAX_LAYERS];
    int d_in, n_hidden, width, s0, sh, unclamped_ok;
    double ymin, b_out, y_ymin, y_gain, y_xoffset;
    std::vector<float> f32;
    size_t o32_in, o32_hid, o32_bias;
    int filter_ok;
    double filter_margin;                 // bound on |y32 - y64| of the unmapped output for mapped inputs inside filter_box
    double filter_box[MAX_DIN][2];        // [lo, hi] of every mapped input the bound was derived on
    float filter_g[MAX_HIDDEN];           // the per-candidate margin (net_filter_slope_terms): the last hidden layer's slope weights ..
    double filter_g64[MAX_HIDDEN];        // .. before they were rounded up to float (tests) ..
    double filter_c0;                     // .. and its constant term
};

// the networks the fp32 filter is instantiated for: the shipped 3-variable class (NetShape<3> of score_plan.h)
static inline bool filter_shape(int k, int H, int nh) { return k == 3 && H == 50 && nh == 3; }

// ---- The margin of the fp32 filter: an a-priori bound on |y32 - y64|, y the unmapped network output, y32 what stage F of the
// skipping kernel computes and y64 the network itself (the fp64 kernels are within 1e-11 of it, far inside the last factor).
//
// Stage F, per hidden layer: z_i = fl-chain(b~_i + sum_j w~_ij a^_j) on v_mfma_f32_16x16x4_f32 with b~ = fl32(c b), w~ = fl32(c W),
// c = FILTER_EXP_SCALE, then a^_i = fma(2, rcp(exp2(z_i) + 1), -1).  With e_j >= |a^_j - a_j| of the layer's inputs and
// A_j >= |a^_j|, u = 2^-24, gamma(m) = m u / (1 - m u):
//   |z_i - c n_i| <=   sum_j |w~_ij| A_j gamma(m_j) + |b~_i| gamma(n)     the fmaf chain: the bias enters as C and sees all n
//                                                                         roundings of the n live terms; a term sees its own and
//                                                                         every later one.  The matrix core consumes the terms
//                                                                         four at a time (one k-step); m_j counts from the FIRST
//                                                                         term of j's k-step, so the order inside a k-step does
//                                                                         not matter.  Zero-padded terms add 0 exactly: no rounding.
//                    + sum_j |w~_ij - c W_ij| A_j + |b~_i - c b_i|        fp32 conversion of the scaled weights (the host knows
//                                                                         both sides, no u-bound needed)
//                    + |c| sum_j |W_ij| e_j                               the inputs' own error
// The k-steps of a hidden layer hold neurons {16 t + 4 q + i, q = 0..3} for (t, i) in order -- the C/D fragment of one layer is the
// B fragment of the next -- and those of the input layer inputs 4 s .. 4 s + 3.  That is the chain of rows 0 .. 47, the three
// row tiles on the matrix core; ONE k-step, their last, holds the tail neurons of the layer in front: neuron 48 + v on its slot
// q = v (the kernel merges components 0 and 1 of the q = 0 lanes of fragment (t, 3) into that A operand; the packed blob keeps
// them apart), exact zeros on q >= NT.  Terms 48 and 49 both count from the first term of that shared k-step: 2 roundings each.
// TAIL ROWS.  A last row tile with NT = H - 48 <= 4 live rows (two at H = 50) does not run on the matrix core: each of its rows
// is summed on the VALU, by the four lanes q = 0..3 of the candidate's column (score_mfma.hip: filter_pass_f32).  Lane q chains
//   p_q = fma-chain( [q = 0: b~_i, else 0], then ONE head link w~_i,48+q a^_(48+q) (the tail neuron of the layer in front that
//                    lane q holds; on q >= NT the activation is an exact zero and the link adds it to an exact zero),
//                    then its twelve terms j = 16 tk + 4 q + i' in the order of 4 tk + i' = 0 .. 11 ),
// one rounding per fma, and the lanes are summed as
//   z_i = (p_q + p_(q^1)) + (p_(q^2) + p_(q^3)):  two more roundings for every term.
// So in a tail row term j < 48 sees m_j = 12 - (4 tk + i') + 2 roundings (its own fma, the later ones of its lane, the tree),
// every tail term 48 + v sees 1 + 12 + 2 (its head link, the twelve behind it, the tree) and so does the bias, which enters
// that head link as its addend; these replace gamma(fan - before[j]) and gamma(fan) above.
// In the input layer lane q chains the inputs q, 4 + q, 8 + q .. below the fan-in (`live` of them; a padded term adds an exact
// zero) behind the bias on q = 0:  m_j = live - j / 4 + 2, and the bias sees the ceil(fan / 4) links of lane 0 and the tree.
// Every other term of the bound -- conversion, inputs' error, tansig -- is that of the other rows.  (Widths whose last tile
// holds more than four rows, or none, have no tail rows: NT = 0.)
// tansig is 1-Lipschitz in n = z / c, which covers the error of exp2's ARGUMENT; what the hardware adds on top of the exact
// 2 / (1 + 2^z) - 1:  v_exp_f32 and v_rcp_f32 are documented to 1 ulp, counted as 2 ulp = 4 u each, the add and the fma u each.
// With E = 2^z, r = 1 / (1 + E) <= 1:  |2 r^ - 2 r| <= 2 r (4 u + u) + 2 (4 u) E / (1 + E)^2 <= 10 u + 2 u, and the fma's own
// rounding of a value <= 1 adds u:  13 u.  (unclamped_ok bounds |z| by 116: exp2 neither overflows nor reaches the denormals.)
//   e'_i = |z_i - c n_i| / |c| + 13 u,   A'_i = 1 + 8 u
// Inputs: the staged fp64 feature is converted once, e_j = u B_j, A_j = (1 + u) B_j with B_j the larger endpoint of filter_box.
// The output layer runs in fp64 on the fp32 activations: |acc32 - acc64| <= sum_j |Wout_j| e_j, and the output mapping divides by
// its gain.  The factor 1 + 2^-10 covers the fp64 roundings of this derivation and of the kernels' epilogues and the terms of
// second order in u; there is no other safety factor -- the margin decides how many candidates the filter passes on.
// filter_box: the image of the input domain (x in [0, 1], |q| <= 1/k) under the network's mapping, 1e-9 wider at both ends so
// that a contracted (v - xoffset) gain + ymin on the device and a quotient one ulp above 1/k stay inside.
// networks.filter_margin restates this in numpy (tests/test_filter_margin_cpu.py).
// The layers of that derivation: -> e[j] of the LAST hidden layer's activations, and in delta[j] (if asked for) their
// pre-activations' share of it, |z_j / c - n_j| <= delta_j = e_j - 13 u, which net_filter_slope_terms below starts from.
static inline void net_filter_layers(int k, int nh, int H, int d_in, const double *const *W, const double *const *B,
                                     const double *xoffset, const double *gain, double ymin, double (*box)[2], double *e, double *delta)
{
    const double u = 0x1p-24, c = FILTER_EXP_SCALE;
    auto gamma = [&](int m) { return m * u / (1.0 - m * u); };
    const int NT = (H > 48 && H <= 52) ? H - 48 : 0;      // tail rows 48 .. H - 1 (two at the width that filters, 50)
    double A[MAX_HIDDEN], en[MAX_HIDDEN];
    for (int i = 0; i < d_in; ++i) {
        const double lo = i < k ? 0.0 : -1.0 / (double)k, hi = i < k ? 1.0 : 1.0 / (double)k;
        const double a = (lo - xoffset[i]) * gain[i] + ymin, b = (hi - xoffset[i]) * gain[i] + ymin;
        box[i][0] = (a < b ? a : b) - 1e-9;
        box[i][1] = (a < b ? b : a) + 1e-9;
        const double Bi = std::fabs(box[i][0]) > std::fabs(box[i][1]) ? std::fabs(box[i][0]) : std::fabs(box[i][1]);
        e[i] = u * Bi;
        A[i] = (1.0 + u) * Bi;
    }
    int fan = d_in;
    for (int l = 0; l < nh; ++l) {
        int before[MAX_HIDDEN];      // live terms in front of the k-step of input j
        if (l == 0) {
            for (int j = 0; j < fan; ++j) before[j] = 4 * (j / 4);
        } else {
            int cnt = 0;
            for (int t = 0; t < 4; ++t)
                for (int i = 0; i < 4; ++i) {
                    int live = 0;
                    for (int q = 0; q < 4; ++q) {
                        const int j = 16 * t + 4 * q + i;
                        if (j < fan) { before[j] = cnt; ++live; }
                    }
                    cnt += live;
                }
            if (NT > 0)
                for (int j = 48; j < fan; ++j) before[j] = 48;      // the tail neurons share one k-step: 48 + v on q = v
        }
        // the tail rows' own count: roundings seen by term j, and by the bias
        int mtail[MAX_HIDDEN], mtail_bias = 0;
        if (NT > 0) {
            if (l == 0) {
                for (int j = 0; j < fan; ++j) {
                    const int q = j % 4, s = j / 4, live = (fan - q + 3) / 4;      // lane q chains inputs q, 4 + q, ...: `live` of them
                    mtail[j] = live - s + 2;
                }
                mtail_bias = (fan + 3) / 4 + 2;
            } else {
                for (int j = 0; j < 48; ++j) mtail[j] = 12 - (4 * (j / 16) + j % 4) + 2;      // j = 16 tk + 4 q + i: link 4 tk + i of 12
                for (int j = 48; j < fan; ++j) mtail[j] = 1 + 12 + 2;      // lane q = j - 48: one head link, then its twelve
                mtail_bias = 1 + 12 + 2;
            }
        }
        for (int i = 0; i < H; ++i) {
            const bool tail = NT > 0 && i >= 48;
            const double bt = (double)(float)(c * B[l][i]);
            double acc = std::fabs(bt) * gamma(tail ? mtail_bias : fan) + std::fabs(bt - c * B[l][i]);
            for (int j = 0; j < fan; ++j) {
                const double w = W[l][(size_t)i * fan + j], wt = (double)(float)(c * w);
                acc += std::fabs(wt) * A[j] * gamma(tail ? mtail[j] : fan - before[j]) + std::fabs(wt - c * w) * A[j] + std::fabs(c * w) * e[j];
            }
            en[i] = acc / std::fabs(c) + 13.0 * u;
            if (delta) delta[i] = acc / std::fabs(c);
        }
        for (int i = 0; i < H; ++i) { e[i] = en[i]; A[i] = 1.0 + 8.0 * u; }
        fan = H;
    }
}

static inline double net_filter_margin(int k, int nh, int H, int d_in, const double *const *W, const double *const *B,
                                       const double *xoffset, const double *gain, double ymin, double y_gain, double (*box)[2])
{
    double e[MAX_HIDDEN];
    net_filter_layers(k, nh, H, d_in, W, B, xoffset, gain, ymin, box, e, nullptr);
    double out = 0.0;
    for (int j = 0; j < H; ++j) out += std::fabs(W[nh][j]) * e[j];
    return out / std::fabs(y_gain) * (1.0 + 0x1p-10);
}

// ---- The margin PER CANDIDATE: the same bound with the last hidden layer's tansig taken at its slope instead of as 1-Lipschitz.
// Neuron j of the LAST hidden layer: n_j its exact pre-activation, n^_j = z_j / c what the fp32 pass holds, |n^_j - n_j| <= delta_j
// (the a-priori bound of the derivation above, e'_j without its 13 u: net_filter_layers), a_j = tansig(n_j), t_j = tansig(n^_j)
// exactly and a^_j the hardware's value, |a^_j - t_j| <= 13 u (above).  The mean value theorem on the segment between n_j and n^_j:
//   |t_j - a_j| = tansig'(xi) |n^_j - n_j|,   tansig'(xi) <= tansig'(n^_j) + L2 |xi - n^_j| <= 1 - t_j^2 + L2 delta_j
// with tansig' = 1 - tansig^2 and L2 = max |tansig''| = max |2 t (1 - t^2)| = 4 / (3 sqrt 3) (at t^2 = 1/3).  The pass holds a^_j,
// not t_j:  |t_j^2 - a^_j^2| = |t_j - a^_j| |t_j + a^_j| <= 13 u (2 + 8 u) <= 27 u.  So
//   |a^_j - a_j| <= (1 - a^_j^2 + 27 u + L2 delta_j) delta_j + 13 u
// The output layer is fp64 on the fp32 activations and the mapping divides by its gain, as above:
//   |y32 - y64| <= S + C,   S = sum_j G_j (1 - a^_j^2),   G_j = |Wout_j| delta_j / |y_gain|,
//                           C = sum_j |Wout_j| ((27 u + L2 delta_j) delta_j + 13 u) / |y_gain|
// S is evaluated by the fp32 pass itself (score_mfma.hip: filter_pass_f32), with G_j rounded UP to float (Gf_j >= G_j):
//   s_j = fma(-a^_j, a^_j, 1)                       one rounding of a value in [-17 u, 1] (|a^_j| <= 1 + 8 u):  |s_j - (1 - a^_j^2)| <= u
//   lane q:  p = fma(Gf_j, s_j, p) over its 13 terms    13 links (the tail term is its last; forced to 0 on q >= 2, where the lane
//                                                   holds an exact 0 whose slope would count as 1)
//   S~ = (p_q + p_(q^1)) + (p_(q^2) + p_(q^3))      2 more roundings for every term
// A term sees at most 13 + 2 = 15 roundings of the sum and |s_j| <= 1:  |S~ - sum_j Gf_j (1 - a^_j^2)| <= (gamma(15) + u) sum_j Gf_j,
// 16 roundings counted in all, charged in ABSOLUTE terms:
//   C0 = C + (gamma(15) + u) sum_j Gf_j
// (An s_j below zero, >= -17 u, makes Gf_j s_j smaller than G_j s_j by at most 17 u (Gf_j - G_j) <= 17 u^2 G_j: second order.)
//   M(cand) = min( filter_margin, (S~ (1 + 2^-9) + C0) (1 + 2^-10) )
// Both arguments of the min are bounds on |y32 - y64|.  1 + 2^-10 is the factor of the a-priori margin, for the same fp64 roundings
// and second-order terms; 1 + 2^-9 on S~ is slack on top of the counted terms (gamma(15) is 9e-7), none of which depends on it.
// -> Gd[64] = G_j, Gf[64] = the floats the kernel multiplies (zeros from H on in both), *C0.  networks.filter_margin_terms restates it.
static inline void net_filter_slope_terms(int k, int nh, int H, int d_in, const double *const *W, const double *const *B,
                                          const double *xoffset, const double *gain, double ymin, double y_gain, double *Gd, float *Gf,
                                          double *C0)
{
    const double u = 0x1p-24, L2 = 4.0 / (3.0 * std::sqrt(3.0)), g15 = 15.0 * u / (1.0 - 15.0 * u);
    double e[MAX_HIDDEN], delta[MAX_HIDDEN], box[MAX_DIN][2];
    net_filter_layers(k, nh, H, d_in, W, B, xoffset, gain, ymin, box, e, delta);
    double c = 0.0, gsum = 0.0;
    for (int j = 0; j < MAX_HIDDEN; ++j) { Gd[j] = 0.0; Gf[j] = 0.0f; }
    for (int j = 0; j < H; ++j) {
        const double w = std::fabs(W[nh][j]);
        Gd[j] = w * delta[j] / std::fabs(y_gain);
        float g = (float)Gd[j];
        if ((double)g < Gd[j]) g = std::nextafterf(g, INFINITY);
        Gf[j] = g;
        gsum += (double)g;
        c += w * ((27.0 * u + L2 * delta[j]) * delta[j] + 13.0 * u);
    }
    *C0 = c / std::fabs(y_gain) + (g15 + u) * gsum;
}

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
    // ---- the fp32 filter (stage F of the skipping kernel): its margin, and -- where the network qualifies -- its weights
    out->filter_margin = net_filter_margin(k, nh, H, d_in, W, B, xoffset, gain, out->ymin, out->y_gain, out->filter_box);
    net_filter_slope_terms(k, nh, H, d_in, W, B, xoffset, gain, out->ymin, out->y_gain, out->filter_g64, out->filter_g, &out->filter_c0);
    // (written so that a NaN margin fails)
    out->filter_ok = (out->unclamped_ok && filter_shape(k, H, nh) && out->filter_margin < FILTER_MARGIN_CUTOFF) ? 1 : 0;
    out->f32.clear();
    out->o32_in = out->o32_hid = out->o32_bias = 0;
    if (out->filter_ok) {
        const double c = FILTER_EXP_SCALE;
        std::vector<float> &f = out->f32;
        // A-fragment of v_mfma_f32_16x16x4_f32: lane l holds A[row = l & 15][k = l >> 4].  Input layer: one float4 per lane and row
        // tile, component s = k-step s:  in[t][l][s] = c W0[16 t + (l & 15)][4 s + (l >> 4)]  (s0 <= 4 for this shape)
        out->o32_in = f.size();
        f.resize(f.size() + (size_t)T * 64 * 4, 0.f);
        for (int t = 0; t < T; ++t)
            for (int ln = 0; ln < 64; ++ln)
                for (int s = 0; s < s0; ++s) {
                    const int row = 16 * t + (ln & 15), col = 4 * s + (ln >> 4);
                    if (row < H && col < d_in) f[out->o32_in + ((size_t)t * 64 + ln) * 4 + s] = (float)(c * W[0][(size_t)row * d_in + col]);
                }
        // Hidden layers: the C/D fragment of the layer in front holds rows 16 tk + 4 (l >> 4) + i in register i of row tile tk,
        // so k-step (tk, i) multiplies neurons {16 tk + 4 q + i}:  hid[layer][t][tk][l][i] = c W[16 t + (l & 15)][16 tk + 4 (l >> 4) + i]
        out->o32_hid = f.size();
        f.resize(f.size() + (size_t)(nh - 1) * T * 4 * 64 * 4, 0.f);
        for (int l = 1; l < nh; ++l)
            for (int t = 0; t < T; ++t)
                for (int tk = 0; tk < 4; ++tk)
                    for (int ln = 0; ln < 64; ++ln)
                        for (int i = 0; i < 4; ++i) {
                            const int row = 16 * t + (ln & 15), col = 16 * tk + 4 * (ln >> 4) + i;
                            if (row < H && col < H)
                                f[out->o32_hid + ((((size_t)(l - 1) * T + t) * 4 + tk) * 64 + ln) * 4 + i] = (float)(c * W[l][(size_t)row * H + col]);
                        }
        out->o32_bias = f.size();
        f.resize(f.size() + (size_t)nh * 64, 0.f);
        for (int l = 0; l < nh; ++l)
            for (int j = 0; j < H; ++j) f[out->o32_bias + (size_t)l * 64 + j] = (float)(c * B[l][j]);
    }
    return SDPCUT_OK;
}
