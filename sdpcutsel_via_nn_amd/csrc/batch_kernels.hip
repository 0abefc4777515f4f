// Batch kernels of libsdpcut_hip.so (gfx950) that score no candidate list: the NNs.so call and _get_eigendecomp on explicit
// inputs, and the probe of the MFMA fragment maps the scoring kernel assumes; each with its launcher (declared in common.h).
#include "common.h"
#include "jacobi.h"
#include "gather.h"
#include "libm_exp.h"
#include "tansig.h"      // d4

// ------------------------------------------------------------------------------------------
// Raw batched MLP forward on explicit inputs (the NNs.so call, batched) -- simple order.
__global__ __launch_bounds__(64) void nn_batch_kernel(NetDev net, int64_t count, const double *in, double *out)
{
#pragma clang fp contract(off)
    __shared__ double act[2][MAX_HIDDEN][64];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    const int64_t cc = c < count ? c : count - 1;
    const int DIN = net.d_in;
    for (int i = 0; i < DIN; ++i)
        act[0][i][lane] = (in[cc * DIN + i] - net.inmap[i]) * net.inmap[DIN + i] + net.ymin;
    int cur = 0, fan_in = DIN;
    for (int l = 0; l < net.n_hidden; ++l) {
        const double *W = net.raw_w[l], *b = net.raw_b[l];
        for (int j = 0; j < net.width; ++j) {
            double acc = 0.0;
            for (int i = 0; i < fan_in; ++i) acc = acc + act[cur][i][lane] * W[j * fan_in + i];
            acc = acc + b[j];
            act[cur ^ 1][j][lane] = 2.0 / (libm_exp(acc * -2.0) + 1.0) + -1.0;      // the host libm's exp: NNs.so's bits (libm_exp.h)
        }
        cur ^= 1;
        fan_in = net.width;
    }
    const double *w = net.raw_w[net.n_hidden];
    double acc = 0.0;
    for (int j = 0; j < fan_in; ++j) acc = acc + act[cur][j][lane] * w[j];
    acc = acc + net.b_out;
    if (c < count) out[c] = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
}

// ------------------------------------------------------------------------------------------
// Batched full eigen-decomposition of explicit sub-matrices (twin of _get_eigendecomp).
template <int K>
__global__ __launch_bounds__(64) void eig_batch_kernel(int64_t count, const double *xr, const double *Xr,
                                                       double *vals, double *vecs)
{
    constexpr int M = K * (K + 1) / 2;
    constexpr int D = K + 1;
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double x[K], X[M];
#pragma unroll
    for (int a = 0; a < K; ++a) x[a] = xr[i * K + a];
#pragma unroll
    for (int m = 0; m < M; ++m) X[m] = Xr[i * M + m];
    double a[D][D], v[D][D];
    fill_lifted<K>(a, x, X);
    jacobi_eig<D, true>(a, v);
    double w[D];
#pragma unroll
    for (int j = 0; j < D; ++j) w[j] = a[j][j];
    // ascending sort of the eigenpairs (odd-even transposition network, static indices)
#pragma unroll
    for (int round = 0; round < D; ++round)
#pragma unroll
        for (int j = round & 1; j + 1 < D; j += 2) {
            const bool sw = w[j + 1] < w[j];
            const double lo = sw ? w[j + 1] : w[j], hi = sw ? w[j] : w[j + 1];
            w[j] = lo; w[j + 1] = hi;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                const double p = v[r][j], qv = v[r][j + 1];
                v[r][j] = sw ? qv : p;
                v[r][j + 1] = sw ? p : qv;
            }
        }
#pragma unroll
    for (int j = 0; j < D; ++j) vals[i * D + j] = w[j];
    if (vecs) {
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int j = 0; j < D; ++j) vecs[(i * D + r) * D + j] = v[r][j];
    }
}

// ------------------------------------------------------------------------------------------
// Fragment-map probe: C[16][16] = A[16][4] * B[4][16] with the maps the MLP kernel assumes.
__global__ __launch_bounds__(64) void mfma_probe_kernel(const double *Am, const double *Bm, double *Cm)
{
    const int lane = threadIdx.x;
    const double a = Am[(lane & 15) * 4 + (lane >> 4)];   // A[row = lane&15][k = lane>>4]
    const double b = Bm[(lane >> 4) * 16 + (lane & 15)];  // B[k = lane>>4][col = lane&15]
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Cm[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
}

int launch_eig_batch(sdpcut_ctx *h, int k, int64_t count, const double *d_x, const double *d_X,
                     double *d_vals, double *d_vecs)
{
    if (count == 0) return 0;
    const int grid = (int)((count + 63) / 64);
    switch (k) {
    case 2: hipLaunchKernelGGL((eig_batch_kernel<2>), dim3(grid), dim3(64), 0, h->stream, count, d_x, d_X, d_vals, d_vecs); break;
    case 3: hipLaunchKernelGGL((eig_batch_kernel<3>), dim3(grid), dim3(64), 0, h->stream, count, d_x, d_X, d_vals, d_vecs); break;
    case 4: hipLaunchKernelGGL((eig_batch_kernel<4>), dim3(grid), dim3(64), 0, h->stream, count, d_x, d_X, d_vals, d_vecs); break;
    case 5: hipLaunchKernelGGL((eig_batch_kernel<5>), dim3(grid), dim3(64), 0, h->stream, count, d_x, d_X, d_vals, d_vecs); break;
    default: return sdpcut_fail(h, SDPCUT_EINVAL, "k must be 2..5");
    }
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int launch_nn_batch(sdpcut_ctx *h, int k, int64_t count, const double *d_in, double *d_out)
{
    if (count == 0) return 0;
    const int grid = (int)((count + 63) / 64);
    hipLaunchKernelGGL(nn_batch_kernel, dim3(grid), dim3(64), 0, h->stream, h->net[k].dev, count, d_in, d_out);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int launch_mfma_probe(sdpcut_ctx *h, const double *d_A, const double *d_B, double *d_C)
{
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, h->stream, d_A, d_B, d_C);
    HIP_TRY(h, hipGetLastError());
    return 0;
}
