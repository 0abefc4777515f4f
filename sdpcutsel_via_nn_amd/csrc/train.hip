// Training support of libsdpcut_hip.so (gfx950): loss and gradient of a tansig MLP over a data set resident on the device
// (sdpcut_train_set_data / sdpcut_train_loss_grad, include/sdpcut.h).  The optimiser itself -- scaled conjugate gradient over
// the flat parameter vector -- runs on the host (networks.py: train) and calls this twice per iteration.
//
// One workgroup (four waves) works through STRIPS of 16 samples = one column tile of v_mfma_f64_16x16x4_f64; wave t owns the
// neurons 16 t .. 16 t + 15 of every layer (hidden width <= 64 = four row tiles).  Per strip, with the samples on the N axis:
//   forward    Z_l = W_l A_{l-1} + b_l, A_l = tansig(Z_l): the score kernel's product (A-fragment = W_l[row][k], B-fragment = the
//              previous layer's activations), but EVERY layer's activations stay in LDS for the way back;
//   backward   D_l = (W_{l+1}^T D_{l+1}) .* (1 - A_l^2): the same product with the TRANSPOSED weight fragment W[k][row];
//   gradient   dW_l += D_l A_{l-1}^T, contracted over the strip's 16 SAMPLES (four k-steps): A-fragment = D_l[row][sample],
//              B-fragment = A_{l-1}[col][sample].  The accumulators of wave t's rows of every layer's dW (<= 14 tiles, 112 VGPRs)
//              live in registers across all strips of the workgroup; db_l is the lane's sum of the A-fragments it fed.
// A workgroup writes its partial sums once, at its end; train_reduce_kernel adds the workgroups' partials in workgroup order and
// scales them.  No atomics anywhere, and the work split depends only on (count, number of CUs): two calls with the same
// arguments return the same bits, with or without a gradient (the forward instructions are the same code either way).
#include "common.h"
#include "tansig.h"

// Row pitch of the strip's arrays in LDS: 16 samples and one pad.  The gradient product reads them with the SAMPLE index across
// the k-steps and the row across the lanes (x[16 u + c16][4 s + q]); at a pitch of 16 doubles = 128 B eight of every sixteen
// lanes meet in one bank, at 17 the rows spread over the banks.  The forward and W^T D fragments (row across q, sample across c16) are unaffected.
constexpr int LDN = 17;

template <int NH>
struct TrainLds {
    double a0[32][LDN];       // mapped inputs of the strip, feature-major; rows >= d_in stay zero
    double act[NH][64][LDN];  // activations of every hidden layer; rows >= H stay zero
    double dl[2][64][LDN];    // D_l of the layer being processed and of the one in front of it
    double e[16];             // y_n - t_n per sample (0 behind the end of the range)
    double tn[16];            // mapped targets
};

struct TrainArgs {
    const double *in, *tg, *params;
    double *part;                                     // [workgroups][pstride]: gradient in the order of params, then the loss
    int64_t first, count, pstride;
    int64_t off_w[MAX_LAYERS], off_b[MAX_LAYERS];     // offsets of W_l / b_l in params
    int64_t off_tail;                                 // y_ymin, y_gain, y_xoffset
    int H, want_grad;
};

template <int K, int NH>
__global__ __launch_bounds__(256, 2) void train_kernel(const TrainArgs A)
{
#pragma clang fp contract(off)
    constexpr int DIN = K * (K + 3) / 2;
    constexpr int S0 = (DIN + 3) / 4;       // k-steps of the input layer
    constexpr int U0 = (DIN + 15) / 16;     // column tiles of the input layer's dW
    __shared__ TrainLds<NH> S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = __builtin_amdgcn_readfirstlane(tid >> 6);      // row tile of this wave
    const int q = lane >> 4, c16 = lane & 15;
    const int H = A.H, T = (H + 15) >> 4, SH = (H + 3) >> 2;
    const bool active = t < T;      // uniform per wave; barriers stay outside of it
    const double *P = A.params;

    {
        double *raw = reinterpret_cast<double *>(&S);
        for (int i = tid; i < (int)(sizeof(S) / sizeof(double)); i += 256) raw[i] = 0.0;
    }
    __syncthreads();

    const double ymin = P[2 * DIN];
    const double y_ymin = P[A.off_tail], y_gain = P[A.off_tail + 1], y_xoffset = P[A.off_tail + 2];
    const double b_out = P[A.off_b[NH]];
    const double *Wo = P + A.off_w[NH];

    const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
    d4 acc0[U0], acc[NH > 1 ? NH - 1 : 1][4];
#pragma unroll
    for (int u = 0; u < U0; ++u) acc0[u] = zero4;
#pragma unroll
    for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[l][u] = zero4;
    double db[NH];
#pragma unroll
    for (int l = 0; l < NH; ++l) db[l] = 0.0;
    double dwo = 0.0, dbo = 0.0, loss = 0.0;

    const int64_t nstrips = (A.count + 15) >> 4;
    const int64_t last = A.first + A.count - 1;
    for (int64_t st = blockIdx.x; st < nstrips; st += gridDim.x) {
        const int64_t s0 = A.first + 16 * st;
        // ---- stage: x_n = (x - xoffset) gain + ymin, t_n = (t - y_xoffset) y_gain + y_ymin.  No input clamp: training sees the
        // network as it is.  Columns behind the end of the range repeat the last sample; their error is set to zero below.
        for (int idx = tid; idx < 16 * DIN; idx += 256) {
            const int n = idx / DIN, i = idx - n * DIN;
            const int64_t smp = s0 + n < last ? s0 + n : last;
            S.a0[i][n] = (A.in[smp * DIN + i] - P[i]) * P[DIN + i] + ymin;
        }
        if (tid < 16) {
            const int64_t smp = s0 + tid < last ? s0 + tid : last;
            S.tn[tid] = (A.tg[smp] - y_xoffset) * y_gain + y_ymin;
        }
        __syncthreads();

        // ---- forward
#pragma unroll
        for (int l = 0; l < NH; ++l) {
            if (active) {
                const double *W = P + A.off_w[l], *B = P + A.off_b[l];
                const int fan = l == 0 ? DIN : H;
                const int steps = l == 0 ? S0 : SH;
                const double *prev = l == 0 ? &S.a0[0][0] : &S.act[l > 0 ? l - 1 : 0][0][0];
                d4 c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * t + q + 4 * r;
                    c[r] = j < H ? B[j] : 0.0;
                }
                const int row = 16 * t + c16;
                for (int s = 0; s < steps; ++s) {
                    const int col = 4 * s + q;
                    const double a = (row < H && col < fan) ? W[(int64_t)row * fan + col] : 0.0;
                    c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, prev[col * LDN + c16], c, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * t + q + 4 * r;
                    // the library exp, not the score kernels' branch-free one (1e-15 absolute): the optimiser's accept / reject
                    // decisions hang on low-order bits, and 4 activations per lane and layer are nothing next to the products
                    S.act[l][j][c16] = j < H ? tansig_lib(c[r]) : 0.0;
                }
            }
            __syncthreads();
        }

        // ---- linear output, error, loss
        if (t == 0) {
            double part = 0.0;
            for (int j = q; j < H; j += 4) part = fma(S.act[NH - 1][j][c16], Wo[j], part);
            part = part + __shfl_xor(part, 16);
            part = part + __shfl_xor(part, 32);
            const double y = part + b_out;
            const double e = s0 + c16 <= last ? y - S.tn[c16] : 0.0;
            if (q == 0) {
                S.e[c16] = e;
                loss = fma(e, e, loss);
                dbo = dbo + e;
            }
        }
        __syncthreads();
        if (!A.want_grad) continue;      // uniform

        // ---- output layer: dW_out += sum_n e_n a_n, D of the last hidden layer
        if (tid < H) {
            double s = dwo;
#pragma unroll
            for (int n = 0; n < 16; ++n) s = fma(S.e[n], S.act[NH - 1][tid][n], s);
            dwo = s;
        }
        if (active) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * t + q + 4 * r;
                const double a = S.act[NH - 1][j][c16];
                S.dl[0][j][c16] = j < H ? (Wo[j] * S.e[c16]) * fma(-a, a, 1.0) : 0.0;
            }
        }
        __syncthreads();

        // ---- hidden layers, last to first: dW_l, db_l, then D of the layer in front
#pragma unroll
        for (int l = NH - 1; l >= 0; --l) {
            const int cur = (NH - 1 - l) & 1;
            if (active) {
                double af[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) af[s] = S.dl[cur][16 * t + c16][4 * s + q];
                db[l] = db[l] + ((af[0] + af[1]) + (af[2] + af[3]));
                if (l == 0) {
#pragma unroll
                    for (int u = 0; u < U0; ++u)
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            acc0[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[s], S.a0[16 * u + c16][4 * s + q], acc0[u], 0, 0, 0);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (u < T) {
#pragma unroll
                            for (int s = 0; s < 4; ++s)
                                acc[l > 0 ? l - 1 : 0][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                                    af[s], S.act[l > 0 ? l - 1 : 0][16 * u + c16][4 * s + q], acc[l > 0 ? l - 1 : 0][u], 0, 0, 0);
                        }
                    // D_{l-1}[i][n] = (sum_j W_l[j][i] D_l[j][n]) (1 - a_{l-1}[i][n]^2): A-fragment = W_l[k = j][row = i]
                    const double *W = P + A.off_w[l];
                    const int i = 16 * t + c16;
                    d4 g = zero4;
                    for (int s = 0; s < SH; ++s) {
                        const int j = 4 * s + q;
                        const double a = (j < H && i < H) ? W[(int64_t)j * H + i] : 0.0;
                        g = __builtin_amdgcn_mfma_f64_16x16x4f64(a, S.dl[cur][j][c16], g, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i2 = 16 * t + q + 4 * r;
                        const double a = S.act[l > 0 ? l - 1 : 0][i2][c16];
                        S.dl[cur ^ 1][i2][c16] = i2 < H ? g[r] * fma(-a, a, 1.0) : 0.0;
                    }
                }
            }
            __syncthreads();      // (behind l = 0 too: the next strip's staging overwrites a0, tn and e)
        }
    }

    // ---- this workgroup's partial sums: every entry of its row is written by exactly one lane
    double *out = A.part + (int64_t)blockIdx.x * A.pstride;
    const int64_t g0 = 2 * DIN + 1;      // the gradient leaves out the input mapping in front of the first W
    if (A.want_grad) {
        if (active) {
#pragma unroll
            for (int u = 0; u < U0; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * t + q + 4 * r, i = 16 * u + c16;
                    if (j < H && i < DIN) out[A.off_w[0] - g0 + (int64_t)j * DIN + i] = acc0[u][r];
                }
#pragma unroll
            for (int l = 1; l < NH; ++l)
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = 16 * t + q + 4 * r, i = 16 * u + c16;
                        if (j < H && i < H) out[A.off_w[l] - g0 + (int64_t)j * H + i] = acc[l - 1][u][r];
                    }
#pragma unroll
            for (int l = 0; l < NH; ++l) {
                double v = db[l];
                v = v + __shfl_xor(v, 16);
                v = v + __shfl_xor(v, 32);
                if (q == 0 && 16 * t + c16 < H) out[A.off_b[l] - g0 + 16 * t + c16] = v;
            }
        }
        if (tid < H) out[A.off_w[NH] - g0 + tid] = dwo;
    }
    if (t == 0) {
        double v = loss, w = dbo;      // (lanes q = 0 hold the sums of their column, the others zero)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            v = v + __shfl_xor(v, off);
            w = w + __shfl_xor(w, off);
        }
        if (lane == 0) {
            out[A.pstride - 1] = v;
            if (A.want_grad) out[A.off_b[NH] - g0] = w;
        }
    }
}

// out[p] = (2 / count) (part[0][p] + part[1][p] + ...), the workgroups in ascending order; the last entry is the loss: sum / count
__global__ __launch_bounds__(256) void train_reduce_kernel(const double *part, int nblk, int64_t pstride, int64_t p_first,
                                                           double gscale, double cnt, double *out)
{
#pragma clang fp contract(off)
    const int64_t p = p_first + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pstride) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s = s + part[(int64_t)b * pstride + p];
    out[p] = p == pstride - 1 ? s / cnt : s * gscale;
}

template <int K>
static void train_launch_k(int nh, const TrainArgs &A, int grid, hipStream_t st)
{
    switch (nh) {
    case 1: hipLaunchKernelGGL((train_kernel<K, 1>), dim3(grid), dim3(256), 0, st, A); break;
    case 2: hipLaunchKernelGGL((train_kernel<K, 2>), dim3(grid), dim3(256), 0, st, A); break;
    case 3: hipLaunchKernelGGL((train_kernel<K, 3>), dim3(grid), dim3(256), 0, st, A); break;
    default: hipLaunchKernelGGL((train_kernel<K, 4>), dim3(grid), dim3(256), 0, st, A); break;
    }
}

extern "C" {

int sdpcut_train_set_data(sdpcut_handle h, int k, int64_t count, const double *inputs, const double *targets)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (k < 2 || k > SDPCUT_MAX_K) return sdpcut_fail(h, SDPCUT_EINVAL, "k must be 2..5");
    if (count < 0 || (count > 0 && (!inputs || !targets))) return sdpcut_fail(h, SDPCUT_EINVAL, "bad train_set_data arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    TrainData &td = h->train[k];
    td = TrainData();
    if (count == 0) return SDPCUT_OK;      // the set of this size is dropped
    const size_t d = (size_t)k * (k + 3) / 2;
    HIP_TRY(h, td.d_in.reset((size_t)count * d));
    HIP_TRY(h, td.d_t.reset((size_t)count));
    HIP_TRY(h, hipMemcpy(td.d_in.get(), inputs, (size_t)count * d * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(td.d_t.get(), targets, (size_t)count * sizeof(double), hipMemcpyHostToDevice));
    td.count = count;
    return SDPCUT_OK;
}

int sdpcut_train_loss_grad(sdpcut_handle h, int k, int n_layers, const int32_t *widths, const double *params, int64_t n_params,
                           int64_t first, int64_t count, double *loss, double *grad)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    const char *why = nullptr;
    if (net_check(k, n_layers, widths, params, n_params, &why) != SDPCUT_OK) return sdpcut_fail(h, SDPCUT_EINVAL, why);
    const TrainData &td = h->train[k];
    if (td.count == 0) return sdpcut_fail(h, SDPCUT_ESTATE, "sdpcut_train_set_data for this candidate size first");
    if (first < 0 || count < 1 || first > td.count || count > td.count - first)
        return sdpcut_fail(h, SDPCUT_EINVAL, "sample range outside the resident training set");
    if (!loss) return sdpcut_fail(h, SDPCUT_EINVAL, "loss is NULL");
    HIP_TRY(h, hipSetDevice(h->device));

    const int d_in = k * (k + 3) / 2, nh = n_layers - 1;
    TrainArgs A{};
    {
        int64_t o = 2 * d_in + 1;
        int fan = d_in;
        for (int l = 0; l < n_layers; ++l) {
            A.off_w[l] = o; o += (int64_t)widths[l] * fan;
            A.off_b[l] = o; o += widths[l];
            fan = widths[l];
        }
        A.off_tail = o;
    }
    const int64_t n_grad = n_params - (2 * d_in + 1 + 3);
    const int64_t nstrips = (count + 15) / 16;
    const int grid = (int)(nstrips < 2 * (int64_t)h->n_cu ? nstrips : 2 * (int64_t)h->n_cu);
    A.pstride = n_grad + 1;
    // workspace: params | reduced gradient and loss | partial sums
    const size_t need = (size_t)n_params + (size_t)A.pstride * ((size_t)grid + 1);
    int rc_ws = grow(h, h->d_train_ws, need);
    if (rc_ws) return rc_ws;
    double *d_params = h->d_train_ws.get(), *d_out = d_params + n_params, *d_part = d_out + A.pstride;
    HIP_TRY(h, hipMemcpyAsync(d_params, params, (size_t)n_params * sizeof(double), hipMemcpyHostToDevice, h->stream));
    A.in = td.d_in.get(); A.tg = td.d_t.get(); A.params = d_params; A.part = d_part;
    A.first = first; A.count = count;
    A.H = widths[0]; A.want_grad = grad ? 1 : 0;
    switch (k) {
    case 2: train_launch_k<2>(nh, A, grid, h->stream); break;
    case 3: train_launch_k<3>(nh, A, grid, h->stream); break;
    case 4: train_launch_k<4>(nh, A, grid, h->stream); break;
    default: train_launch_k<5>(nh, A, grid, h->stream); break;
    }
    HIP_TRY(h, hipGetLastError());
    const int64_t p_first = grad ? 0 : n_grad;      // forward only: the loss entry alone
    const int rgrid = (int)((A.pstride - p_first + 255) / 256);
    hipLaunchKernelGGL(train_reduce_kernel, dim3(rgrid), dim3(256), 0, h->stream, d_part, grid, A.pstride, p_first,
                       2.0 / (double)count, (double)count, d_out);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(loss, d_out + n_grad, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad) HIP_TRY(h, hipMemcpyAsync(grad, d_out, (size_t)n_grad * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

} // extern "C"
