// The two cross-check scoring kernels of libsdpcut_hip.so (gfx950): the VALU kernel (SDPCUT_KERNEL_VALU: the fast tansig, no
// MFMA) and the deliberately simple one (SDPCUT_KERNEL_SIMPLE: lane = candidate, reference operation order), for cross-checking
// and A/B timing of score_mfma_kernel (score_mfma.hip), and the launcher that starts them (score_launch.h).
#include "score_launch.h"
#include "jacobi.h"
#include "gather.h"
#include "libm_exp.h"
#include "tansig.h"

// ------------------------------------------------------------------------------------------
// VALU kernel: lane = candidate, activations in registers, weights as SCALAR operands.
//
// On gfx950 v_mfma_f64_16x16x4_f64 and v_fma_f64 share the fp64 datapath: they do not overlap
// (profiles/r01_ubench_mfma_valu_overlap.txt: MFMA-only 0.85 ms, FMA-only 0.94 ms, both on one
// SIMD 1.81 ms) and peak at the same 78.6 TFLOP/s.  The MFMA form pads 50 neurons to 64 rows
// (26 % wasted FLOPs); here every fp64 FMA is a useful one.  Weights are wave-uniform, so they
// are read through the scalar cache (s_load_dwordx16 = 8 weights) and enter v_fma_f64 as SGPR
// operands: no LDS, no vector memory traffic in the MLP at all.  Eight output neurons are
// accumulated at once (8 independent FMA chains hide the fp64 latency); weights are packed
// host-side as [layer][j/8][i][j%8] so that each (block, i) is one 64-byte scalar load.
typedef const __attribute__((address_space(4))) double *cdouble_p;   // constant AS => SMEM loads

// Scalar loads return out of order, so the only usable wait is lgkmcnt(0): the weight stream is
// software-pipelined in batches of two input steps (2 x s_load_dwordx16 = 16 weights): batch
// g+1 is issued, then the 16 FMAs of batch g run while it is in flight.  The sched_barriers pin
// that order (left alone, hipcc issues each load right in front of its first use and eats the
// full scalar-cache latency every 8 FMAs).
template <int FAN, int H>
__device__ __forceinline__ void dense_tansig(cdouble_p wv, cdouble_p bias, const double (&in)[FAN], double (&out)[H])
{
    constexpr int JB = 8, NB = (H + JB - 1) / JB;
    constexpr int NBAT = (FAN + 1) / 2;          // batches of two input steps per output block
    double wa[2 * JB], wb[2 * JB];            // the two weight buffers (SGPRs)
#pragma unroll
    for (int t = 0; t < 2 * JB; ++t) wa[t] = wv[t];
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) {
        double acc[JB];
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) acc[jj] = bias[jb * JB + jj];
#pragma unroll
        for (int bt = 0; bt < NBAT; ++bt) {
            const int g = jb * NBAT + bt;             // global batch number: its parity picks the buffer
            const bool last = (jb == NB - 1) && (bt == NBAT - 1);
            const int jn = (bt + 1 < NBAT) ? jb : jb + 1, bn = (bt + 1 < NBAT) ? bt + 1 : 0;
            // lgkmcnt(0) BEFORE the next batch is issued: the current buffer is complete and the
            // new loads stay in flight during the FMAs below (0xc07f = vmcnt/expcnt untouched)
            __builtin_amdgcn_s_waitcnt(0xc07f);
            if (!last) {
#pragma unroll
                for (int t = 0; t < 2 * JB; ++t) {
                    const double v = wv[(jn * FAN + 2 * bn) * JB + t];
                    if (g & 1) wa[t] = v; else wb[t] = v;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = 2 * bt + u;
                if (i < FAN) {
#pragma unroll
                    for (int jj = 0; jj < JB; ++jj)
                        if (jb * JB + jj < H)
                            acc[jj] = fma(in[i < FAN ? i : 0], (g & 1) ? wb[u * JB + jj] : wa[u * JB + jj], acc[jj]);
                }
            }
            if (bt == NBAT - 1) {
#pragma unroll
                for (int jj = 0; jj < JB; ++jj)
                    if (jb * JB + jj < H) out[jb * JB + jj] = tansig(acc[jj]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int K, int H, int NH>
__global__ __launch_bounds__(256, (H > 56 ? 1 : 2)) void score_valu_kernel(ScoreArgs A)
{
    constexpr int M = K * (K + 1) / 2;
    constexpr int DIN = K + M;
    constexpr int NB = (H + 7) / 8;
    const NetDev &net = A.net;
    const int64_t ntiles = (A.n + 255) / 256;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t c = tile * 256 + threadIdx.x;
        const bool valid = c < A.n;
        const int64_t cc = valid ? c : A.n - 1;
        Cand<K> cd;
        gather_candidate<K>(cd, A.set, A.n, cc, A.vars, A.Q, A.nv, A.L, (A.flags & SDPCUT_NN) != 0);
        const int32_t out_idx = A.orig[cc];
        double lam = 0.0;
        if (A.flags & SDPCUT_EIG) lam = candidate_eigmin<K>(cd);
        double obj = 0.0;
        if (A.flags & SDPCUT_NN) {
            cdouble_p inmap = (cdouble_p)net.inmap;
            double in[DIN];
#pragma unroll
            for (int i = 0; i < DIN; ++i) {
                const double v = (i < K) ? cd.x[i < K ? i : 0] : cd.q[i >= K ? i - K : 0];
                in[i] = (v - inmap[i]) * inmap[DIN + i] + net.ymin;
            }
            double a[H];
            dense_tansig<DIN, H>((cdouble_p)net.wvalu, (cdouble_p)net.bias, in, a);
            cdouble_p wv = (cdouble_p)net.wvalu + NB * DIN * 8;
#pragma unroll 1
            for (int l = 1; l < NH; ++l) {
                double o[H];
                dense_tansig<H, H>(wv, (cdouble_p)net.bias + l * 64, a, o);
#pragma unroll
                for (int j = 0; j < H; ++j) a[j] = o[j];
                wv += NB * H * 8;
            }
            cdouble_p wout = (cdouble_p)net.wout;
            double p0 = 0.0, p1 = 0.0;
#pragma unroll
            for (int j = 0; j + 1 < H; j += 2) {
                p0 = fma(a[j], wout[j], p0);
                p1 = fma(a[j + 1], wout[j + 1], p1);
            }
            if (H & 1) p0 = fma(a[H - 1], wout[H - 1], p0);
            {
#pragma clang fp contract(off)
                double acc = p0 + p1;
                acc = acc + net.b_out;
                const double y = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
                obj = cd.negSM;
                obj = obj + y * cd.max_elem;
            }
        }
        if (valid) {
            if (A.flags & SDPCUT_EIG) A.eig_out[out_idx] = lam;
            if (A.flags & SDPCUT_NN) A.obj_out[out_idx] = obj;
        }
        if (A.strong_out) {
            const unsigned long long m = __ballot(valid && obj > 0.0 && lam < SDPCUT_NEG_EIGVAL);
            if ((threadIdx.x & 63) == 0 && m)
                __hip_atomic_fetch_add((unsigned long long *)&A.strong_out[blockIdx.x & 7], (unsigned long long)__popcll(m),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Simple kernel: lane = candidate, activations in LDS, reference operation order.
template <int K>
__global__ __launch_bounds__(64) void score_simple_kernel(ScoreArgs A)
{
    constexpr int M = K * (K + 1) / 2;
    constexpr int DIN = K + M;
    __shared__ double act[2][MAX_HIDDEN][64];
    const int lane = threadIdx.x;
    const NetDev &net = A.net;
    const int64_t ntiles = (A.n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t c = tile * 64 + lane;
        const bool valid = c < A.n;
        const int64_t cc = valid ? c : A.n - 1;
        Cand<K> cd;
        gather_candidate<K>(cd, A.set, A.n, cc, A.vars, A.Q, A.nv, A.L, (A.flags & SDPCUT_NN) != 0);
        const int32_t out_idx = A.orig[cc];
        double lam_c = 0.0;
        if (A.flags & SDPCUT_EIG) {
            const double lam = candidate_eigmin<K>(cd);
            lam_c = lam;
            if (valid) A.eig_out[out_idx] = lam;
        }
        if (!(A.flags & SDPCUT_NN)) continue;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int i = 0; i < DIN; ++i) {
                const double v = (i < K) ? cd.x[i < K ? i : 0] : cd.q[i >= K ? i - K : 0];
                act[0][i][lane] = (v - net.inmap[i]) * net.inmap[DIN + i] + net.ymin;
            }
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
            const double y = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
            double obj = cd.negSM;
            obj = obj + y * cd.max_elem;
            if (valid) A.obj_out[out_idx] = obj;
            if (A.strong_out) {
                const unsigned long long m = __ballot(valid && obj > 0.0 && lam_c < SDPCUT_NEG_EIGVAL);
                if (lane == 0 && m)
                    __hip_atomic_fetch_add((unsigned long long *)&A.strong_out[blockIdx.x & 7], (unsigned long long)__popcll(m),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

template <int K>
static void score_alt_launch_k(bool valu, const ScoreArgs &A, int n_cu, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    if (valu) {
        const int grid = grid_for(n_cu, (A.n + 255) / 256, 8);
        SCORE_LAUNCH((score_valu_kernel<K, NetShape<K>::H, NetShape<K>::NH>), grid, 256);
    } else {
        const int grid = grid_for(n_cu, (A.n + 63) / 64, 16);
        SCORE_LAUNCH((score_simple_kernel<K>), grid, 64);
    }
}

void score_alt_launch(int K, bool valu, const ScoreArgs &A, int n_cu, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    switch (K) {
    case 2: score_alt_launch_k<2>(valu, A, n_cu, st, ev_start, ev_stop); break;
    case 3: score_alt_launch_k<3>(valu, A, n_cu, st, ev_start, ev_stop); break;
    case 4: score_alt_launch_k<4>(valu, A, n_cu, st, ev_start, ev_stop); break;
    default: score_alt_launch_k<5>(valu, A, n_cu, st, ev_start, ev_stop); break;
    }
}
