// The scoring kernel of libsdpcut_hip.so on the matrix cores -- hand-written for gfx950 (CDNA4, wave64).
//
// One launch per candidate size k scores every k-variable candidate at the current LP
// point (reference: the loop bodies of _sel_eigcut_by_ordering_on_measure,
// cut_select_qp.py:570-582 and :642-648, plus NNs.so and numpy.linalg.eigvalsh under them):
//
//   phase A  lane = candidate: read the index set (SoA, coalesced), gather x_rho / X_rho /
//            Q_rho from the HBM-resident, cache-hot tables, derive max_elem / Q_slice / S,
//            Jacobi lambda_min of the lifted matrix in registers, stage the mapminmax'ed MLP
//            inputs in LDS (feature-major, one 64-candidate strip per wave);
//   phase B  the MLP on the matrix cores: H^T = tansig(W * X^T + b) with
//            v_mfma_f64_16x16x4_f64, neurons on the M axis and candidates on the N axis, so
//            that the C/D fragment of one layer IS the B fragment of the next (row =
//            (lane>>4) + 4*reg is exactly k-step reg of row tile t) -- activations never leave
//            registers; weights are pre-packed host-side into A-fragment order and streamed
//            from L2 as coalesced 512-B wave loads; tansig runs on the VALU between MFMAs.
//
// This unit holds the kernel for one class (score_mfma_kernel), its variant that runs the MLP for violated candidates only
// (score_mfma_skip_kernel: the same body with SKIP; score_mfma_filter_kernel: with an fp32 pass in front of the fp64 one, FILTER, and
// filter_audit_kernel, which runs that fp32 pass for every candidate), the one over all classes of a list (score_mfma_all_kernel: the same body per
// class) and the launchers that start them (score_launch.h).  Which wave scores which candidate is
// decided on the host (score_plan.h); the cross-check kernels are in score_alt.hip.
#include <type_traits>

#include "score_launch.h"
#include "jacobi.h"
#include "gather.h"
#include "tansig.h"

// The LDS strips of the MFMA kernel (feat, ynn) are private to one wave.  A wave's LDS
// instructions are issued and serviced in program order, so a write followed by a read of
// another lane's slot needs no workgroup barrier -- only that the compiler keeps the order and
// that the data has returned (lgkmcnt) before use.  Dropping __syncthreads() decouples the four
// waves of a workgroup: none waits for the slowest (PMC: SQ_WAIT_ANY 45 % of wave cycles).
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v + v(lane ^ 32) and v + v(lane ^ 16) through v_permlane{32,16}_swap_b32 (gfx950) instead of ds_bpermute_b32: the swap of
// a register pair holding the same value leaves one register with the lower / even rows' values everywhere and the other with the
// upper / odd rows', and their sum is the butterfly sum on every lane -- bit for bit what v + __shfl_xor(v, 32 | 16) gives
// (addition commutes).  No LDS crossbar round trip (two dependent ones per reduction, ~250 cycles, at every layer boundary of a pass).
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#ifndef SDPCUT_PERMLANE_SWAP
#define SDPCUT_PERMLANE_SWAP 1
#endif
__device__ __forceinline__ double xor_add32(double v)
{
#if SDPCUT_PERMLANE_SWAP
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const u32x2 a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const u32x2 b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
#else
    return v + __shfl_xor(v, 32);
#endif
}
__device__ __forceinline__ double xor_add16(double v)
{
#if SDPCUT_PERMLANE_SWAP
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const u32x2 a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const u32x2 b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
#else
    return v + __shfl_xor(v, 16);
#endif
}
// v(lane ^ 32)
__device__ __forceinline__ double xor_get32(double v, int lane)
{
#if SDPCUT_PERMLANE_SWAP
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const u32x2 a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);      // [0]: lower half everywhere, [1]: upper half everywhere
    const u32x2 b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    const double lower = __hiloint2double((int)b[0], (int)a[0]), upper = __hiloint2double((int)b[1], (int)a[1]);
    return (lane & 32) ? lower : upper;
#else
    return __shfl_xor(v, 32);
#endif
}

// Tail rows of a hidden layer on the VALU: ts[u] holds this lane's partial dot product of tail
// neuron u over the k-slots it owns (n = 4 s + q); the four k-slot lanes of a candidate column
// (lane, lane^16, lane^32, lane^48) are summed, and lane q keeps neuron u = q in register 0 of
// the last row tile -- exactly where the MFMA C/D layout would have put it.
// Both column tiles of a pass share ONE tansig evaluation: after the two xor-adds every lane of a
// column holds the full sums, so lanes q = 0, 1 take tile j = 0 and lanes q = 2, 3 tile j = 1
// (neuron u = q & 1); a final xor-32 shuffle hands the j = 1 values to lanes q = 0, 1.
template <int NT, bool CLAMP = true>
__device__ __forceinline__ void tail_rows2(const double (&ts)[2][NT ? NT : 1], const double *bias, int q, d4 &out0,
                                           d4 &out1)
{
    static_assert(NT <= 2, "at most two tail neurons");
    double pre = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            double v = ts[j][u];
            v = xor_add16(v);
            v = xor_add32(v);
            pre = (q == 2 * j + u) ? v + bias[u] : pre;
        }
    const double t = tansig_y8<CLAMP>(pre);
    const double t1 = xor_get32(t, 16 * q);
    out0 = d4{0.0, 0.0, 0.0, 0.0};
    out1 = d4{0.0, 0.0, 0.0, 0.0};
    out0[0] = (q < NT) ? t : 0.0;
    out1[0] = (q < NT) ? t1 : 0.0;
}

// The same for a pass of ONE column tile (the three-waves-per-SIMD variant of the kernel): lanes q < NT evaluate the tansig
// of neuron u = q, the other k-slot lanes idle through it.
template <int NT, bool CLAMP = true>
__device__ __forceinline__ void tail_rows1(const double (&ts)[1][NT ? NT : 1], const double *bias, int q, d4 &out0)
{
    static_assert(NT <= 2, "at most two tail neurons");
    double pre = 0.0;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        double v = ts[0][u];
        v = xor_add16(v);
        v = xor_add32(v);
        pre = (q == u) ? v + bias[u] : pre;
    }
    const double t = tansig_y8<CLAMP>(pre);
    out0 = d4{0.0, 0.0, 0.0, 0.0};
    out0[0] = (q < NT) ? t : 0.0;
}

// Timing experiments (tools/build_ablation.sh; results are wrong by design): drop the bias or
// weight-fragment loads to see what their latency costs.
// Biases, tail-row weights and output weights (<= 8.5 KB) are copied to LDS once per workgroup:
// they are read at every tile / layer boundary, exactly where a wave has nothing else in flight
// to cover an L2 round trip (ds_read ~100 cycles instead of ~700).
#ifndef SDPCUT_SMALL_IN_LDS
#define SDPCUT_SMALL_IN_LDS 1
#endif
// (The A-fragments themselves were tried in LDS too -- 44.5 KB for the 3-variable net, two
// workgroups per CU still fit: no gain, the register ring already hides their L2 latency.)
#ifdef SDPCUT_ABL_NOBIAS
#define BIAS_AT(i) (0.125 + 0.0 * (double)(i))
#elif SDPCUT_SMALL_IN_LDS
#define BIAS_AT(i) s_bias[i]
#else
#define BIAS_AT(i) net.bias_q[i]
#endif
#if SDPCUT_SMALL_IN_LDS
#define WTAIL_AT(i) s_wtail[i]
#define WOUT_AT(i) s_wout[i]
#define BIAS_PTR s_bias
#else
#define WTAIL_AT(i) net.wtail[i]
#define WOUT_AT(i) net.wout[i]
#define BIAS_PTR net.bias_q
#endif
#ifdef SDPCUT_ABL_NOWLOAD
#define WFRAG_AT(i) (0.01 * (double)((i) & 7))
#else
#define WFRAG_AT(i) wf[i]
#endif

// Timing experiment (tools/build_ablation.sh ...:PHASETIME): cycles a wave spends between the phase
// boundaries of a tile, printed by a few waves.  [0-1] gather wait, [1-2] Jacobi, [2-3] staging,
// [3-4] the MLP passes.
#ifdef SDPCUT_ABL_PHASETIME
#define PHASE_DECL unsigned long long ph_t[5] = {0, 0, 0, 0, 0}, ph_acc[4] = {0, 0, 0, 0}; int ph_n = 0
#define PHASE_MARK(i)                                                      \
    do {                                                                   \
        ph_t[i] = __builtin_readcyclecounter();                            \
        if ((i) > 0) ph_acc[(i) - 1] += ph_t[i] - ph_t[(i) - 1];           \
        if ((i) == 4) ++ph_n;                                              \
    } while (0)
#define PHASE_WAITMEM asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define PHASE_REPORT                                                                                        \
    if ((threadIdx.x & 63) == 0 && (blockIdx.x % 509) == 3)                                                 \
    printf("blk %d wave %d tiles %d: gather %llu jacobi %llu stage %llu mlp %llu cycles/tile\n", (int)blockIdx.x, \
           (int)(threadIdx.x >> 6), ph_n, ph_acc[0] / (ph_n ? ph_n : 1), ph_acc[1] / (ph_n ? ph_n : 1),      \
           ph_acc[2] / (ph_n ? ph_n : 1), ph_acc[3] / (ph_n ? ph_n : 1))
#elif defined(SDPCUT_ABL_CLOCKS)
// shader clock actually sustained while the kernel runs: core-clock counter against the 100 MHz one
#define PHASE_DECL const unsigned long long ph_c0 = clock64(), ph_w0 = wall_clock64()
#define PHASE_MARK(i)
#define PHASE_WAITMEM
#define PHASE_REPORT                                                                                         \
    if (threadIdx.x == 0 && (blockIdx.x % 509) == 3) {                                                       \
        const unsigned long long dc = clock64() - ph_c0, dw = wall_clock64() - ph_w0;                        \
        printf("blk %d: %llu core cycles in %llu ticks of 10 ns -> %.0f MHz\n", (int)blockIdx.x, dc, dw,     \
               dw ? 100.0 * (double)dc / (double)dw : 0.0);                                                  \
    }
#else
#define PHASE_DECL
#define PHASE_MARK(i)
#define PHASE_WAITMEM
#define PHASE_REPORT
#endif

// ------------------------------------------------------------------------------------------
// MFMA kernel.  K candidate size, H hidden width, NH hidden layers; FUSE = TK_MODE_FEAS / OPT / STRONG:
// also count the class members by the leading radix digit of that mode's selection keys (ScoreArgs::tk).
// CLAMP = false (NetDev::unclamped_ok): the tansig clamps are dropped and the staged (mapped) inputs are
// clamped to [-3, 3] instead.  net_pack grants unclamped_ok only to a network whose own mapping sends the input
// domain -- x in [0, 1], |q| <= 1/k -- into [-3, 3], so on the domain the clamp is inactive and the kernel computes
// the network itself; outside it (an LP point a solver tolerance beyond the box) it cuts the mapped input at +-3,
// which keeps the bound on the pre-activations a proof.  CLAMP = true clamps no input (see sdpcut_set_network).
// JK = 16-candidate column tiles per pass (mfma_cols, score_plan.h).

// LDS of one workgroup of the MFMA kernel for size class K (a union of these serves the launch over all classes)
template <int K, int H, int NH>
struct MfmaLds {
    static constexpr int S0 = (K + K * (K + 1) / 2 + 3) / 4;
    static constexpr int T = (H + 15) / 16;
    static constexpr int NT = (H - 16 * (T - 1) <= 4) ? H - 16 * (T - 1) : 0;
    double feat[4][S0 * 4][64];  // per wave: feature-major strip of 64 candidates
    double ynn[4][64];           // per wave: raw network outputs
    double s_bias[NH * 64];
    double s_wtail[NT ? NH * 4 * 64 : 1];
    double s_wout[64];
    uint32_t tk_hist[256];       // leading-digit histogram of the selection that follows (A.tk != nullptr)
    uint32_t tk_cnt[2];
    uint32_t s_strong;
    uint32_t pf_tab[pf_score_k(K) ? PF_BINS / 2 : 1];    // (r5) the class members by window code, 16-bit counters, two per word (topk_dev.h)
};

// LDS of one workgroup of the skipping kernel (SKIP, see score_mfma_body): instead of a strip, a wave keeps a QUEUE of the violated
// candidates it has met -- their mapped features (feat, column = queue slot) and what the epilogue needs of them (negSM, max_elem,
// output slot).  A ring of QCAP = 96 slots: a pass takes the oldest 32, so at most 31 are pending when a strip appends at most 64.
template <int K, int H, int NH>
struct MfmaLdsSkip {
    static constexpr int S0 = (K + K * (K + 1) / 2 + 3) / 4;
    static constexpr int T = (H + 15) / 16;
    static constexpr int NT = (H - 16 * (T - 1) <= 4) ? H - 16 * (T - 1) : 0;
    static constexpr int DIN = K + K * (K + 1) / 2;
    static constexpr int QCAP = 96;
    double feat[4][S0 * 4][QCAP];
    double ynn[4][QCAP];
    double q_negsm[4][QCAP];
    double q_maxel[4][QCAP];
    int32_t q_out[4][QCAP];
    double s_bias[NH * 64];
    double s_wtail[NT ? NH * 4 * 64 : 1];
    double s_wout[64];
    alignas(16) double s_stage[DIN][2];      // launch constants of the staging loop, per feature: xoffset, gain (stage_lds_fill)
    uint32_t tk_hist[256];
    uint32_t tk_cnt[2];
    uint32_t s_strong;
    uint32_t pf_tab[pf_score_k(K) ? PF_BINS / 2 : 1];
};

// The small fp32 constants of the filter's pass in LDS: [NH][64] biases, then the weights of the two tail neurons 48 and 49 as
// the lanes of the VALU tail read them, [layer][u][q][16]: for a hidden layer entries 4 tk + i = c W[48 + u][16 tk + 4 q + i]
// (tk < 3: the twelve activations lane (q, c) holds), entries 12, 13 = c W[48 + u][48], c W[48 + u][49]; for the input layer
// entries s = c W0[48 + u][4 s + q].  All of them are read out of the packed A-fragments of row tile 3 (net_pack.h: lane
// u + 16 q of fragment (3, tk)), the same fl32(c W) values the matrix core used to multiply (filter_lds_fill below).  Then the
// slope weights G of the margin per candidate, 64 floats in neuron order (NetDev::f32_g).
template <int NH>
struct FilterLds {
    static constexpr int BIAS = NH * 64, TAIL = NH * 2 * 4 * 16, SLOPE = 64;
    alignas(16) float v[BIAS + TAIL + SLOPE];
};

// LDS of one workgroup of the skipping kernel with the fp32 filter (FILTER, see score_mfma_body): TWO rings per wave.  Ring 1 (f_*,
// FCAP = 96 slots: <= 31 pending + <= 64 appended by a strip) holds the violated candidates, ring 2 (the names of MfmaLdsSkip,
// QCAP = 64: <= 31 pending + <= 32 survivors of one filter pass) those of them the fp32 pass could not rule out.  Only the DIN live
// feature rows are kept; the fp64 pass reads the padding rows of its B fragments as literal zeros.
template <int K, int H, int NH>
struct MfmaLdsFilter {
    static constexpr int DIN = K + K * (K + 1) / 2;
    static constexpr int T = (H + 15) / 16;
    static constexpr int NT = (H - 16 * (T - 1) <= 4) ? H - 16 * (T - 1) : 0;
    static constexpr int QCAP = 64, FCAP = 96;
    double feat[4][DIN][QCAP];
    double ynn[4][QCAP];
    double q_negsm[4][QCAP];
    double q_maxel[4][QCAP];
    int32_t q_out[4][QCAP];
    double f_feat[4][DIN][FCAP];
    double f_negsm[4][FCAP];
    double f_maxel[4][FCAP];
    int32_t f_out[4][FCAP];
    uint8_t f_byp[4][FCAP];      // the candidate has a mapped input outside NetDev::filter_box: it survives unconditionally
    double f_y[4][32];           // raw fp32-pass outputs of the 32 entries of a filter pass
    FilterLds<NH> s_f32;         // biases and tail-neuron weights of the fp32 pass
    double s_bias[NH * 64];
    double s_wtail[NT ? NH * 4 * 64 : 1];
    double s_wout[64];
    alignas(16) double s_stage[DIN][4];      // launch constants of the staging loop, per feature: xoffset, gain, box lo, box hi
    uint32_t tk_hist[256];
    uint32_t tk_cnt[3];
    uint32_t s_strong;
    uint32_t pf_tab[pf_score_k(K) ? PF_BINS / 2 : 1];
};

// ------------------------------------------------------------------------------------------
// v + v(lane ^ 32) and v + v(lane ^ 16) of a float, as xor_add32 / xor_add16 above: both lanes of a pair add the same two values
__device__ __forceinline__ float xor_add32f(float v)
{
    const unsigned x = __float_as_uint(v);
    const u32x2 a = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
__device__ __forceinline__ float xor_add16f(float v)
{
    const unsigned x = __float_as_uint(v);
    const u32x2 a = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}

// Fills FilterLds (above) from the packed fp32 weights.  Call before a __syncthreads().
template <int NH>
__device__ __forceinline__ void filter_lds_fill(const NetDev &net, FilterLds<NH> &F)
{
    for (int i = threadIdx.x; i < FilterLds<NH>::BIAS; i += blockDim.x) F.v[i] = net.f32_bias[i];
    for (int i = threadIdx.x; i < FilterLds<NH>::TAIL; i += blockDim.x) {
        const int l = i >> 7, u = (i >> 6) & 1, q = (i >> 4) & 3, e = i & 15;
        float w = 0.0f;
        if (l == 0) {
            if (e < 4) w = net.f32_in[((size_t)(3 * 64 + u + 16 * q)) * 4 + e];
        } else if (e < 12) {
            w = net.f32_hid[((((size_t)(l - 1) * 4 + 3) * 4 + (e >> 2)) * 64 + u + 16 * q) * 4 + (e & 3)];
        } else if (e < 14) {
            w = net.f32_hid[((((size_t)(l - 1) * 4 + 3) * 4 + 3) * 64 + u) * 4 + (e - 12)];
        }
        F.v[FilterLds<NH>::BIAS + i] = w;
    }
    for (int i = threadIdx.x; i < FilterLds<NH>::SLOPE; i += blockDim.x) F.v[FilterLds<NH>::BIAS + FilterLds<NH>::TAIL + i] = net.f32_g[i];
}

// The launch constants the strip loop's staging reads per feature, copied next to each other into LDS (s_stage of MfmaLdsSkip /
// MfmaLdsFilter): the input mapping's xoffset and gain, and with BOX the feature's interval of NetDev::filter_box.  Read through
// the NetDev pointers inside the strip loop they are vector loads from a uniform address, one L2 round trip each and -- behind
// the short-circuit of the box test -- one after the other.  Call before a __syncthreads().
template <int DIN, bool BOX, int W>
__device__ __forceinline__ void stage_lds_fill(const NetDev &net, double (&C)[DIN][W])
{
    static_assert(W == (BOX ? 4 : 2), "xoffset, gain (, lo, hi) per feature");
    if (threadIdx.x < 2 * DIN) {
        C[threadIdx.x % DIN][threadIdx.x / DIN] = net.inmap[threadIdx.x];
        if constexpr (BOX) C[threadIdx.x >> 1][2 + (threadIdx.x & 1)] = net.filter_box[threadIdx.x];
    }
}

// The margin of ONE candidate from the slope sum S its fp32 pass returned (net_pack.h: net_filter_slope_terms has the derivation):
// never above the a-priori margin, and the a-priori margin itself where S is a NaN.
__device__ __forceinline__ double filter_cand_margin(const NetDev &net, const float S)
{
    const double m = ((double)S * (1.0 + 0x1p-9) + net.filter_c0) * (1.0 + 0x1p-10);
    return m < net.filter_margin ? m : net.filter_margin;
}

// The fp32 pass of the filter (stage F of the skipping kernel, and all of filter_audit_kernel): the MLP of 32 candidates on
// v_mfma_f32_16x16x4_f32, two column tiles of 16 = two independent accumulator chains.  feat_at(row, col) is the staged (mapped,
// fp64) input `row` of column col = 0..31.  Returns in yraw[j], on every lane of column c16 of tile j, the output layer's sum
// (without b_out) as a double, and in slope[j] the sum S = sum_i G_i (1 - a_i^2) over the last hidden layer's activations in fp32.
//  * Layouts: A lane l = A[row l & 15][k l >> 4], B lane l = B[k l >> 4][col l & 15], C/D register i of lane l = row
//    4 (l >> 4) + i.  So register i of row tile tk IS the B operand of a k-step that multiplies neurons {16 tk + 4 q + i}: the
//    host packs the A-fragments in that k-order (net_pack.h) and the activations never leave registers.
//  * Row tiles 0..2 (neurons 0..47) run on the matrix core.  Their accumulator starts as the (scaled) bias and the k-steps follow
//    in order -- (0, 0) .. (2, 3), then ONE k-step for the tail neurons: its B operand holds neuron 48 on the q = 0 lanes, 49 on
//    q = 1 and an exact 0.0f on q >= 2; its A operand is c W[row][48] on q = 0 and c W[row][49] on q = 1, merged here from
//    components 0 and 1 of the q = 0 lanes of the packed fragment (t, 3) by one v_permlane16_swap (rows q >= 1 of that fragment
//    are packed zeros, which is what lands on q = 2, 3).  The chain the margin's derivation counts.
//  * Neurons 48 and 49 (a fourth row tile would be 14 rows of padding) run on the VALU.  Lane (q, c) chains
//        p = (q == 0 ? bias : 0);  p = fma(w[48 + q], a_(48 + q), p);  p = fma(w[16 tk + 4 q + i], a, p), (tk, i) in order
//    over the tail activation of the layer in front that it holds (neuron 48 + q on q = 0, 1; an exact 0 on q >= 2), at the HEAD
//    of its chain, and the twelve activations it holds; the four q-lanes of the column are then summed as
//    (p_q + p_(q^1)) + (the same of q^2) -- every lane then holds both neurons' sums, takes the one of neuron q & 1 and ONE
//    tansig of it.  The input layer's tail chains the lane's S0 inputs 4 s + q the same way.  This order, too, is what
//    net_filter_margin counts.
//  * The output layer is a fp64 dot product of the fp32 activations with the fp64 output weights (13 fma per lane and tile) and the
//    cross-lane sum of the fp64 pass: no fp32 rounding behind the last tansig.
//  * The slope sum, beside it (the layer in front is dead there): per lane and tile thirteen links s = fma(G_i, fma(-a_i, a_i, 1), s)
//    in the order of the lane's activations, the tail neuron's last -- forced to zero on q >= 2, whose exact 0 is no neuron --
//    then the two-level lane sum of the tail rows.  This order is what net_filter_slope_terms counts.
// Columns are independent: the tail's sums go across the q-lanes of ONE column, so a stale or padding column (NaN included)
// changes no other column's result, and the select behind the tansig puts a finite zero on q >= 1 whatever the sum was.
template <int K, int H, int NH, class FeatAt>
__device__ __forceinline__ void filter_pass_f32(const NetDev &net, const FilterLds<NH> &F, const double *s_wout, FeatAt feat_at,
                                                const int lane, double (&yraw)[2], float (&slope)[2])
{
    constexpr int DIN = K + K * (K + 1) / 2;
    constexpr int S0 = (DIN + 3) / 4;
    static_assert(S0 <= 4 && H == 50, "one float4 of input k-steps per lane; three row tiles and the tail neurons 48, 49");
    const float *s_bias32 = F.v, *s_tail32 = F.v + FilterLds<NH>::BIAS;
    const int q = lane >> 4, c16 = lane & 15;
    float bin[S0][2];
#pragma unroll
    for (int s = 0; s < S0; ++s)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = 4 * s + q;
            const double v = feat_at(row < DIN ? row : 0, 16 * j + c16);
            bin[s][j] = row < DIN ? (float)v : 0.0f;
        }
    // tansig of a C/D fragment of a row tile below 48: every row is a neuron
    auto act = [&](const f4 z) __attribute__((always_inline)) {
        f4 a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = tansig_f32_z(z[i]);
        return a;
    };
    // the two tail neurons from their lane chains: the column's four q-lanes summed, then neuron 48 + u kept on lane q = u
    auto tail_act = [&](float p48, float p49) __attribute__((always_inline)) {
        p48 = xor_add32f(xor_add16f(p48));
        p49 = xor_add32f(xor_add16f(p49));
        const float a = tansig_f32_z(q == 0 ? p48 : p49);
        return q < 2 ? a : 0.0f;
    };
    f4 cur[3][2], prev[3][2];
    float ctl[2], ptl[2];            // [column tile]: neuron 48 + q on the lanes q = 0, 1
    // ---------------- input layer
    {
        const f4 *w_in = (const f4 *)net.f32_in;
        f4 w[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) w[t] = w_in[t * 64 + lane];
        float pt[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f4 wt = *(const f4 *)&s_tail32[(u * 4 + q) * 16];
            const float b = q == 0 ? s_bias32[48 + u] : 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float p = b;
#pragma unroll
                for (int s = 0; s < S0; ++s) p = __builtin_fmaf(wt[s], bin[s][j], p);
                pt[j][u] = p;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) ctl[j] = tail_act(pt[j][0], pt[j][1]);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const f4 bias = *(const f4 *)&s_bias32[16 * t + 4 * q];
            f4 acc0 = bias, acc1 = bias;
#pragma unroll
            for (int s = 0; s < S0; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][s], bin[s][0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][s], bin[s][1], acc1, 0, 0, 0);
            }
            cur[t][0] = act(acc0);
            cur[t][1] = act(acc1);
        }
    }
    // ---------------- hidden -> hidden layers (rolled); the fragments of row tile t + 1 are requested while tile t computes
#pragma unroll 1
    for (int l = 1; l < NH; ++l) {
#pragma unroll
        for (int t = 0; t < 3; ++t) { prev[t][0] = cur[t][0]; prev[t][1] = cur[t][1]; }
#pragma unroll
        for (int j = 0; j < 2; ++j) ptl[j] = ctl[j];
        const f4 *wh = (const f4 *)net.f32_hid + (size_t)(l - 1) * 4 * 4 * 64 + lane;
        f4 wnx[4];
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) wnx[tk] = wh[tk * 64];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            f4 w[4];
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) w[tk] = wnx[tk];
            if (t + 1 < 3) {
#pragma unroll
                for (int tk = 0; tk < 4; ++tk) wnx[tk] = wh[((t + 1) * 4 + tk) * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
            const f4 bias = *(const f4 *)&s_bias32[l * 64 + 16 * t + 4 * q];
            f4 acc0 = bias, acc1 = bias;
#pragma unroll
            for (int tk = 0; tk < 3; ++tk)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tk][i], prev[tk][0][i], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tk][i], prev[tk][1][i], acc1, 0, 0, 0);
                }
            {      // the tail k-step: neuron 48 + q on q = 0, 1, zeros elsewhere.  Odd rows of w[3][0] <- even rows of w[3][1]
                const float w3 = __uint_as_float(
                    __builtin_amdgcn_permlane16_swap(__float_as_uint(w[3][0]), __float_as_uint(w[3][1]), false, false)[0]);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3, ptl[0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3, ptl[1], acc1, 0, 0, 0);
            }
            if (t == 0) {
                // the layer's two tail neurons, in the region of tile 0: everything they read is the layer in front
                const float *tw = &s_tail32[((l * 2) * 4 + q) * 16];
                float pt[2][2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    f4 wk[3];
#pragma unroll
                    for (int tk = 0; tk < 3; ++tk) wk[tk] = *(const f4 *)&tw[u * 64 + 4 * tk];
                    const float wq = tw[u * 64 + 12 + (q & 1)];      // the weight of the tail neuron this lane holds (a 0 on q >= 2)
                    const float b = q == 0 ? s_bias32[l * 64 + 48 + u] : 0.0f;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        float p = __builtin_fmaf(wq, ptl[j], b);
#pragma unroll
                        for (int tk = 0; tk < 3; ++tk)
#pragma unroll
                            for (int i = 0; i < 4; ++i) p = __builtin_fmaf(wk[tk][i], prev[tk][j][i], p);
                        pt[j][u] = p;
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) ctl[j] = tail_act(pt[j][0], pt[j][1]);
            }
            cur[t][0] = act(acc0);
            cur[t][1] = act(acc1);
        }
    }
    // ---------------- linear output layer in fp64; the tail neurons' terms last, as rows 48 and 49 of the fourth tile were
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double part = 0.0;
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) part = fma((double)cur[t][j][i], s_wout[16 * t + 4 * q + i], part);
        part = fma((double)ctl[j], s_wout[48 + (q & 1)], part);      // neuron 48 + q on q = 0, 1; an exact zero on q >= 2
        part = xor_add16(part);
        part = xor_add32(part);
        yraw[j] = part;
    }
    // ---------------- the slope sum of the margin per candidate (behind the output layer: its weights are dead, G takes their place)
    {
        const float *s_g32 = F.v + FilterLds<NH>::BIAS + FilterLds<NH>::TAIL;
        f4 g[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) g[t] = *(const f4 *)&s_g32[16 * t + 4 * q];
        const float gq = s_g32[48 + (q & 1)];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) s = __builtin_fmaf(g[t][i], __builtin_fmaf(-cur[t][j][i], cur[t][j][i], 1.0f), s);
            const float st = __builtin_fmaf(-ctl[j], ctl[j], 1.0f);
            s = __builtin_fmaf(gq, q < 2 ? st : 0.0f, s);
            slope[j] = xor_add32f(xor_add16f(s));
        }
    }
}

// bid / nblk: this workgroup's index among the nblk workgroups that serve the class (blockIdx.x / gridDim.x of a launch over
// one class; the launch over all classes of a list hands every class its own range of workgroups, score_mfma_all_kernel)
// SKIP (FUSE = TK_MODE_STRONG, both flags, JK = 2 only; LDS = MfmaLdsSkip): the MLP runs for VIOLATED candidates only -- the strong
// class the launch counts for holds no other, and nothing else of a combined round in its strong regime reads obj_improve.  Phase A
// is unchanged (every valid lane stores lambda_min and is counted); the violated lanes then append to the wave's queue, and phase
// B runs a two-tile pass over the oldest 32 entries while there are 32; the wave's last strip flushes the rest (one tile if <= 16).
// A queue entry's score does not depend on its slot or its neighbours (tansig.h), and mlp_pass<1> equals mlp_pass<2> bit for bit:
// a violated candidate gets the bits the plain kernel gives it.  Non-violated candidates get NO obj_out store.
// FILTER (SKIP with LDS = MfmaLdsFilter; NetDev::filter_ok): a stage F between the two.  The violated lanes append to ring 1; while
// it holds 32 entries an fp32 pass (filter_pass_f32) evaluates the network for them, and an entry moves on to ring 2 -- the queue of
// the fp64 pass, which is unchanged -- iff  obj32 = negSM + y32 max_elem > -M max_elem,  or it carries the bypass bit
// (a mapped input outside filter_box, where the margin was not derived).  M <= filter_margin is the margin of THIS candidate, from
// the slopes of its last hidden layer (filter_cand_margin);  |y32 - y64| <= M is proven (net_pack.h), so
// every violated candidate with a positive measure survives and gets the bits the plain kernel gives it; the others are not strong
// whatever their measure, and store their (non-positive) fp32 measure so that the selection, which reads obj_out of every violated
// candidate, sees them as what they are.  The strong count, the histograms and the head are the plain kernel's.
template <int K, int H, int NH, int FUSE, bool CLAMP, int JK, bool SKIP = false, class LDS = MfmaLds<K, H, NH>, bool FILTER = false>
__device__ __forceinline__ void score_mfma_body(const ScoreArgs A, LDS &S, const int bid, const int nblk)
{
    static_assert(!SKIP || (FUSE == TK_MODE_STRONG && JK == 2), "the skipping variant serves the fused launch of a combined round");
    static_assert(!FILTER || (SKIP && !CLAMP), "the fp32 filter is a stage of the clamp-free skipping variant");
    constexpr int M = K * (K + 1) / 2;
    constexpr int DIN = K + M;
    constexpr int S0 = (DIN + 3) / 4;      // k-steps of the input layer
    constexpr int SH = (H + 3) / 4;        // k-steps of a hidden->hidden layer
    constexpr int T = (H + 15) / 16;       // 16-neuron row tiles
    // A last tile with <= 4 live rows (H = 50: neurons 48, 49) would cost a full 16-row MFMA
    // per k-step for 1/8 of the work: those rows run on the VALU instead (tail_rows below).
    constexpr int NT = (H - 16 * (T - 1) <= 4) ? H - 16 * (T - 1) : 0;
    constexpr int TM = NT ? T - 1 : T;     // row tiles computed with MFMA
    static_assert(JK == 1 || JK == 2, "one or two column tiles per pass");
    static_assert(T == 4, "hidden width must be in 49..64");

    auto &feat = S.feat;
    auto &ynn = S.ynn;

    const int lane = threadIdx.x & 63;
    // (wave-uniform by construction; said so to the compiler: the wave's range, its strip loop and pass counts are then scalar)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int q = lane >> 4;      // MFMA k-slot / output row group
    const int c16 = lane & 15;    // MFMA column (candidate within a 16-tile)
    const NetDev &net = A.net;
    // Work split (r3).  The list is cut into STRIPS of A.strip candidates, and wave g of the launch takes strips g, g + W, g + 2W ...
    // (W waves in the launch: the four waves of a workgroup take four consecutive strips, the workgroups move through the list
    // together -- at 10^8 candidates that keeps the 3 GB of index sets and scores the resident waves touch close together).
    //  * Long lists: strips of 64 candidates = two passes of the MLP over two 16-candidate column tiles each, eight workgroups per
    //    CU (short-lived: the dispatcher balances them).
    //  * Lists that leave the device part-empty (<= 32 candidates per resident wave, i.e. <= 65 536 -- most real covers): strips
    //    of 32, ONE pass per wave.  A launch over such a list takes as long as its slowest wave -- phase A plus its passes, 45-95 us
    //    of dependent stages -- and twice as many waves with one pass each finish sooner than half as many with two.  (Finer does
    //    not pay: a single-tile pass of a lone wave takes as long as a two-tile pass, profiles/r03_k3_kernel_time_vs_list_length.txt.)
    // The last strip of a list may hold fewer candidates: it runs the passes its column tiles need, the last one over a single
    // tile if their number is odd (mlp_pass<1>: the same arithmetic per candidate, bit-equal scores).
    // (r5) A.spread (lists of ONE strip per wave -- most real covers): wave w of workgroup b is wave w * nblk + b of the launch, the
    // four waves of a workgroup work on four DISTANT quarters of the list.  Real covers are enumerated index set by index set,
    // neighbours share variables and scores: 256 consecutive candidates rich in members of the head would otherwise be one
    // workgroup's whole share, which then reports fewer of them than it holds and sends the selection through its radix passes
    // (pf_retire_table, topk_dev.h; 13 of 191 recorded rounds).  Longer lists keep the consecutive strips (a workgroup's share
    // already comes from several rounds of the list; spreading its waves cost the 10^6-candidate launch 3 us).  Scores do not
    // depend on who computes them.
    const int64_t gw = A.spread ? (int64_t)wave * nblk + bid : (int64_t)bid * 4 + wave;
    const int64_t wstride = (int64_t)nblk * 4 * A.strip;      // candidates between two strips of one wave
    const int64_t c_first = gw * A.strip;
    // ... and the LAST round of a list of a few rounds, when it is nearly full (r4): 10^6 candidates are 7.63 strips per resident
    // wave slot, every slot ran 8 -- 4.6 % of the kernel idle at its end.  Now the round-robin part ends at the last FULL round
    // (rr_end) and what is left is split evenly in column tiles of 16: three or four per wave (a three-tile strip = one two-tile
    // pass + one single-tile pass), every workgroup the same for its four waves.
    const int64_t t_tiles = gw < A.tail_nhi ? A.tail_hi : A.tail_lo;
    const int64_t t_start0 = A.rr_end + 16 * (gw < A.tail_nhi ? gw * A.tail_hi : A.tail_nhi * A.tail_hi + (gw - A.tail_nhi) * A.tail_lo);
    const int64_t t_start = t_start0 < A.n ? t_start0 : A.n;
    const int64_t t_end = t_start + 16 * t_tiles < A.n ? t_start + 16 * t_tiles : A.n;      // (empty when t_start == t_end)
    bool tail = c_first >= A.rr_end;                  // this wave's current strip is its tail strip
    int64_t s0 = tail ? t_start : c_first;
    bool more = tail ? t_start < t_end : true;

    // The index set (and the output slot) of the NEXT strip are requested before phase B of the
    // current one: the first of the two dependent memory round trips of phase A (HBM: indices, then
    // L2: the gathers they address) is off the critical path.
    // (The first strip's request goes out before the LDS preload below so that the two latencies of a
    // workgroup's start overlap.)
    int32_t s_nxt[K];
    int32_t orig_nxt = 0;
    if (more) {
        const int64_t lim0 = tail ? t_end : (s0 + A.strip < A.rr_end ? s0 + A.strip : A.rr_end);
        const int64_t c0 = s0 + lane;
        const int64_t cc0 = c0 < lim0 ? c0 : s0;
        load_index_set<K>(s_nxt, A.set, A.n, cc0);
        orig_nxt = A.orig[cc0];
    }

#if SDPCUT_SMALL_IN_LDS
    auto &s_bias = S.s_bias;
    auto &s_wtail = S.s_wtail;
    auto &s_wout = S.s_wout;
    if (A.flags & SDPCUT_NN) {     // uniform; an eigenvalue-only launch may come without a network
        for (int i = threadIdx.x; i < NH * 64; i += 256) s_bias[i] = net.bias_q[i];
        if constexpr (NT > 0)
            for (int i = threadIdx.x; i < NH * 4 * 64; i += 256) s_wtail[i] = net.wtail[i];
        if (threadIdx.x < 64) s_wout[threadIdx.x] = net.wout[threadIdx.x];
        if constexpr (FILTER) filter_lds_fill<NH>(net, S.s_f32);
        if constexpr (SKIP) stage_lds_fill<DIN, FILTER>(net, S.s_stage);
        __syncthreads();
    }
#endif

    // leading-digit histograms of the selection that follows (A.tk != nullptr)
    auto &tk_hist = S.tk_hist;
    auto &tk_cnt = S.tk_cnt;
    uint32_t c_viol = 0, c_pos = 0, c_strong = 0;     // per lane (vector registers: the scalar file is full)
    [[maybe_unused]] uint32_t c_eval = 0;             // (FILTER) entries the fp64 pass evaluated
    // (r5) the fine histogram of the selection's class (topk_dev.h) is compiled into the kernel of 3-variable candidates only:
    // merely present -- not executed -- it costs the 4-variable kernel 11 us on the 1.7e6-candidate cover of spar125-075-1 (240
    // registers, 112 bytes of scratch: the allocation of its hot loop moves), executed 22, against the 12 us the selection saves
    // (profiles/r05_fine_histogram_score_kernel_variants.txt); the 2-variable kernel loses 7 us on 10^6 candidates the same way
    // (profiles/r05_vs_r4_same_box.txt); on 10^6 three-variable candidates it costs 5-6 and saves 10.  Feasibility rounds -- three
    // quarters of a BoxQP run -- count in the eigenvalue kernel (eig.hip) for every size.
    constexpr bool PF = FUSE != 0 && pf_score_k(K);
    auto &pf_tab = S.pf_tab;
    if constexpr (FUSE != 0) {
        tk_hist[threadIdx.x] = 0;
        if (threadIdx.x < sizeof(tk_cnt) / sizeof(tk_cnt[0])) tk_cnt[threadIdx.x] = 0;
        if constexpr (PF) {
#pragma unroll
            for (int j = 0; j < PF_BINS / 2 / 256; ++j) pf_tab[threadIdx.x + 256 * j] = 0;
        }
        __syncthreads();
    }

    [[maybe_unused]] int q_head = 0, q_fill = 0;      // (SKIP) the wave's queue: first pending slot (0, 32 or 64) and pending entries; scalar
    [[maybe_unused]] int f_head = 0, f_fill = 0;      // (FILTER) the same for ring 1; q_* is ring 2 then
    PHASE_DECL;
    while (more) {
        PHASE_MARK(0);
        const int64_t lim = tail ? t_end : (s0 + A.strip < A.rr_end ? s0 + A.strip : A.rr_end);      // one past this strip's last candidate
        // the strip after this one: the next round-robin strip, or the tail strip behind the last of them
        const bool nx_rr = !tail && s0 + wstride < A.rr_end;
        const bool nx_tail = !tail && !nx_rr;
        const int64_t nx_s0 = nx_rr ? s0 + wstride : t_start;
        const int64_t nx_lim = nx_rr ? (nx_s0 + A.strip < A.rr_end ? nx_s0 + A.strip : A.rr_end) : t_end;
        const bool nx_more = nx_rr || (nx_tail && t_start < t_end);
        const int64_t c = s0 + lane;
        const bool valid = c < lim;
        int32_t s_cur[K];
#pragma unroll
        for (int a = 0; a < K; ++a) s_cur[a] = s_nxt[a];
        const int32_t out_idx = orig_nxt;
        Cand<K> cd;
        gather_candidate<K>(cd, s_cur, A.vars, A.Q, A.nv, A.L, (A.flags & SDPCUT_NN) != 0);
        if (nx_more) {                       // uniform per wave
            const int64_t c1 = nx_s0 + lane;
            const int64_t cc1 = c1 < nx_lim ? c1 : nx_s0;
            load_index_set<K>(s_nxt, A.set, A.n, cc1);
            orig_nxt = A.orig[cc1];
        }

        double lam = 0.0;
        PHASE_WAITMEM;
        PHASE_MARK(1);
        if (A.flags & SDPCUT_EIG) {
            lam = candidate_eigmin<K>(cd, s_cur, A.vars, A.nv, A.L);
            if (valid) A.eig_out[out_idx] = lam;
        }
        PHASE_MARK(2);
        if (!(A.flags & SDPCUT_NN)) {           // uniform branch
            if constexpr (FUSE != 0) {
                const bool viol = valid && lam < SDPCUT_NEG_EIGVAL;      // (only TK_MODE_FEAS ranks without the network)
                const uint64_t key = key_of(-lam);
                hist_add_few(tk_hist, (uint32_t)(key >> 56), viol);
                if (PF && viol) { const int f = pf_code(key, true); atomicAdd(&pf_tab[f >> 1], (f & 1) ? 0x10000u : 1u); }
                c_viol += viol;
            }
            tail = tail || nx_tail; s0 = nx_s0; more = nx_more;
            continue;
        }

        // (SKIP) the violated lanes append to the queue: slot = its end + the lane's rank among them
        [[maybe_unused]] bool q_viol = true;
        [[maybe_unused]] int q_slot = lane;
        if constexpr (SKIP) {
            q_viol = valid && lam < SDPCUT_NEG_EIGVAL;
            c_viol += q_viol;
            const unsigned long long vm = __ballot(q_viol);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(vm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)vm, 0u));
            if constexpr (FILTER) {
                const int tail_slot = f_head + f_fill >= LDS::FCAP ? f_head + f_fill - LDS::FCAP : f_head + f_fill;      // (scalar)
                q_slot = tail_slot + rank >= LDS::FCAP ? tail_slot + rank - LDS::FCAP : tail_slot + rank;
                f_fill += __popcll(vm);
                if (q_viol) {
                    S.f_negsm[wave][q_slot] = cd.negSM;
                    S.f_maxel[wave][q_slot] = cd.max_elem;
                    S.f_out[wave][q_slot] = out_idx;
                }
            } else {
                const int tail_slot = q_head + q_fill >= LDS::QCAP ? q_head + q_fill - LDS::QCAP : q_head + q_fill;      // (scalar)
                q_slot = tail_slot + rank >= LDS::QCAP ? tail_slot + rank - LDS::QCAP : tail_slot + rank;
                q_fill += __popcll(vm);
                if (q_viol) {
                    S.q_negsm[wave][q_slot] = cd.negSM;
                    S.q_maxel[wave][q_slot] = cd.max_elem;
                    S.q_out[wave][q_slot] = out_idx;
                }
            }
        }
        [[maybe_unused]] bool f_outside = false;      // (FILTER) a mapped input lies outside the box the margin was derived on
        // ---- stage mapminmax'ed inputs (neural_net_3D.m:69-73): xp = (v - xoffset)*gain + ymin
#pragma unroll
        for (int i = 0; i < S0 * 4; ++i) {
            double xp = 0.0;
            [[maybe_unused]] const int ic = i < DIN ? i : 0;
            if (i < DIN) {
                const double v = (i < K) ? cd.x[i < K ? i : 0] : cd.q[i >= K ? i - K : 0];
                if constexpr (SKIP) xp = (v - S.s_stage[ic][0]) * S.s_stage[ic][1] + net.ymin;
                else xp = (v - net.inmap[i]) * net.inmap[DIN + i] + net.ymin;
                if constexpr (!CLAMP) xp = min_f64_raw(max_f64_raw(xp, -SDPCUT_INPUT_CLAMP), SDPCUT_INPUT_CLAMP);
            }
            if constexpr (FILTER) {
                if (i < DIN) {
                    // (a NaN is outside, the bounds are inclusive; no short-circuit: the constants of a strip are requested together)
                    f_outside = f_outside | !((xp >= S.s_stage[ic][2]) & (xp <= S.s_stage[ic][3]));
                    if (q_viol) S.f_feat[wave][i][q_slot] = xp;
                }
            } else if constexpr (SKIP) {
                if (q_viol) feat[wave][i][q_slot] = xp;
            } else {
                feat[wave][i][lane] = xp;
            }
        }
        if constexpr (FILTER) {
            if (q_viol) S.f_byp[wave][q_slot] = f_outside ? 1 : 0;
        }
        wave_lds_sync();
        PHASE_MARK(3);

        // Weight fragments requested one stage ahead of their use (SDPCUT_XPREFETCH): the input layer's
        // tile t+1 while tile t computes, the first fragments of a hidden layer before the last tansig of
        // the layer in front of it, the first input tile of the next pass before the output layer.
        // Measured: the 2-variable kernel gains 1.5 % (0.399 -> 0.393 ms), the 3-variable one loses 0.6 %
        // (its other wave already covers the L2 round trips at the stage boundaries; 5 more live
        // registers cost more), the 4/5-variable ones have no registers left (spills): on for K = 2 only.
#ifndef SDPCUT_XPREFETCH
#define SDPCUT_XPREFETCH 1
#endif
#ifndef SDPCUT_XPREFETCH_MAXK
#define SDPCUT_XPREFETCH_MAXK 2
#endif
// (r4) ... and for K = 5 again: with lambda_min by lmin.h instead of the 6x6 Jacobi the 5-variable kernel has the registers the
// prefetch needs -- 584 -> 566 us on 1e6 candidates (-3 %); K = 3 still loses 0.6 %, K = 4 is indifferent.
#ifndef SDPCUT_XPREFETCH_MINK
#define SDPCUT_XPREFETCH_MINK 5
#endif
#ifndef SDPCUT_RING_DEPTH
#define SDPCUT_RING_DEPTH 4
#endif
        constexpr int RD = SDPCUT_RING_DEPTH;
        constexpr bool XP = SDPCUT_XPREFETCH && (K <= SDPCUT_XPREFETCH_MAXK || K >= SDPCUT_XPREFETCH_MINK);
        double a_in[S0];              // input-layer fragments of the tile about to run
        double pre[RD];               // head of the next hidden layer's fragment stream
        if constexpr (XP) {
#pragma unroll
            for (int s = 0; s < S0; ++s) a_in[s] = net.wfrag[s * 64 + lane];
        }
        // one pass of the MLP over JJ column tiles (16 JJ candidates from column col0 of the wave's strip)
        auto mlp_pass = [&](auto jj_tag, const int col0) __attribute__((always_inline)) {
            constexpr int J = decltype(jj_tag)::value;
            // B fragments of the input layer: B[k = 4s + q][col = candidate]
            double bin[S0][J];
#pragma unroll
            for (int s = 0; s < S0; ++s)
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    if constexpr (FILTER) {      // (ring 2 keeps the DIN live rows; the padding rows of the strip hold 0.0)
                        const int row = 4 * s + q;
                        const double v = feat[wave][row < DIN ? row : 0][col0 + 16 * j + c16];
                        bin[s][j] = row < DIN ? v : 0.0;
                    } else {
                        bin[s][j] = feat[wave][4 * s + q][col0 + 16 * j + c16];
                    }
                }

            d4 prev[T][J], cur[T][J];
            const double *wf = net.wfrag;
            // ---------------- input layer
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                d4 bias;
#pragma unroll
                for (int r = 0; r < 4; ++r) bias[r] = BIAS_AT(16 * t + 4 * r + q);
#pragma unroll
                for (int j = 0; j < J; ++j) cur[t][j] = bias;
                double a_nx[S0];
                if constexpr (XP) {
                    if (t + 1 < TM) {
#pragma unroll
                        for (int s = 0; s < S0; ++s) a_nx[s] = WFRAG_AT(((t + 1) * S0 + s) * 64 + lane);
                    } else if (NH > 1) {      // the first hidden layer's stream starts behind the T input tiles
#pragma unroll
                        for (int g = 0; g < RD - 1; ++g) pre[g] = WFRAG_AT((T * S0 + g) * 64 + lane);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int s = 0; s < S0; ++s) {
                    const double a = XP ? a_in[s] : WFRAG_AT((t * S0 + s) * 64 + lane);
#pragma unroll
                    for (int j = 0; j < J; ++j)
                        cur[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bin[s][j], cur[t][j], 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < J; ++j) cur[t][j] = tansig_tile<H, CLAMP>(cur[t][j], t);
                __builtin_amdgcn_sched_barrier(0);
                if (XP && t + 1 < TM) {
#pragma unroll
                    for (int s = 0; s < S0; ++s) a_in[s] = a_nx[s];
                }
            }
            if constexpr (NT > 0) {
                double ts[J][NT ? NT : 1];
#pragma unroll
                for (int j = 0; j < J; ++j)
#pragma unroll
                    for (int u = 0; u < NT; ++u) ts[j][u] = 0.0;
#pragma unroll
                for (int s = 0; s < S0; ++s)
#pragma unroll
                    for (int u = 0; u < NT; ++u) {
                        const double w = WTAIL_AT(u * 64 + 4 * s + q);
#pragma unroll
                        for (int j = 0; j < J; ++j) ts[j][u] = fma(bin[s][j], w, ts[j][u]);
                    }
                if constexpr (J == 2) tail_rows2<NT, CLAMP>(ts, BIAS_PTR + 16 * (T - 1), q, cur[T - 1][0], cur[T - 1][J - 1]);
                else tail_rows1<NT, CLAMP>(ts, BIAS_PTR + 16 * (T - 1), q, cur[T - 1][0]);
            }
            wf += T * S0 * 64;
            // ---------------- hidden -> hidden layers (rolled: bounds code size and live ranges)
#pragma unroll 1
            for (int l = 1; l < NH; ++l) {
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int j = 0; j < J; ++j) prev[t][j] = cur[t][j];
                // The A-fragment stream of the layer is one contiguous sequence g = t*SH + s.  Left
                // alone hipcc loads each fragment right before its two MFMAs and waits vmcnt(0)
                // (an L2 round trip per 128 MFMA cycles, the dominant stall in the first PMC run):
                // a ring of RD fragments keeps RD-1 loads in flight; the sched_barriers pin the order.
                constexpr int NG = TM * SH;
                static_assert(NG >= RD - 1, "fragment stream shorter than the ring");
                double ring[RD];
#pragma unroll
                for (int g = 0; g < RD - 1 && g < NG; ++g) ring[g] = XP ? pre[g] : WFRAG_AT(g * 64 + lane);
#pragma unroll
                for (int t = 0; t < TM; ++t) {
                    d4 bias;
#pragma unroll
                    for (int r = 0; r < 4; ++r) bias[r] = BIAS_AT(l * 64 + 16 * t + 4 * r + q);
#pragma unroll
                    for (int j = 0; j < J; ++j) cur[t][j] = bias;
#pragma unroll
                    for (int s = 0; s < SH; ++s) {
                        const int g = t * SH + s;
                        if (g + RD - 1 < NG) ring[(g + RD - 1) % RD] = WFRAG_AT((g + RD - 1) * 64 + lane);
                        if (XP && g == NG - 1) {
                            // the stage behind this layer: the next hidden layer's head, or -- behind the last
                            // one -- the first input tile of the next pass
                            if (l + 1 < NH) {
#pragma unroll
                                for (int gg = 0; gg < RD - 1; ++gg) pre[gg] = WFRAG_AT((T * SH + gg) * 64 + lane);
                            } else {
#pragma unroll
                                for (int ss = 0; ss < S0; ++ss) a_in[ss] = net.wfrag[ss * 64 + lane];
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int j = 0; j < J; ++j)
                            cur[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ring[g % RD], prev[s / 4][j][s % 4],
                                                                             cur[t][j], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int j = 0; j < J; ++j) cur[t][j] = tansig_tile<H, CLAMP>(cur[t][j], t);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (NT > 0) {
                    double ts[J][NT ? NT : 1];
#pragma unroll
                    for (int j = 0; j < J; ++j)
#pragma unroll
                        for (int u = 0; u < NT; ++u) ts[j][u] = 0.0;
#pragma unroll
                    for (int s = 0; s < SH; ++s)
#pragma unroll
                        for (int u = 0; u < NT; ++u) {
                            const double w = WTAIL_AT((l * 4 + u) * 64 + 4 * s + q);
#pragma unroll
                            for (int j = 0; j < J; ++j) ts[j][u] = fma(prev[s / 4][j][s % 4], w, ts[j][u]);
                        }
                    if constexpr (J == 2) tail_rows2<NT, CLAMP>(ts, BIAS_PTR + l * 64 + 16 * (T - 1), q, cur[T - 1][0], cur[T - 1][J - 1]);
                    else tail_rows1<NT, CLAMP>(ts, BIAS_PTR + l * 64 + 16 * (T - 1), q, cur[T - 1][0]);
                }
                wf += T * SH * 64;
            }
            // ---------------- linear output layer: dot over this lane's 16 neurons, then the
            // four k-slot lanes (q = 0..3) of each candidate column are summed by shuffles
#pragma unroll
            for (int j = 0; j < J; ++j) {
                double part = 0.0;
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (16 * t + 4 * r < H) part = fma(cur[t][j][r], WOUT_AT(16 * t + 4 * r + q), part);
                part = xor_add16(part);
                part = xor_add32(part);
                if (q == 0) ynn[wave][col0 + 16 * j + c16] = part;
            }
        };
        if constexpr (SKIP) {
            // the epilogue of a pass over the cnt <= 32 entries from slot q_head on: the arithmetic of the plain epilogue below on
            // what the queue kept of the candidate; every entry is violated, so it is strong exactly when its measure is positive
            auto skip_epilogue = [&](const int cnt) __attribute__((always_inline)) {
#pragma clang fp contract(off)
                const int s = q_head + (lane & 31);
                const bool live = lane < cnt;
                double acc = ynn[wave][s];
                acc = acc + net.b_out;
                const double y = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
                double obj = S.q_negsm[wave][s];
                obj = obj + y * S.q_maxel[wave][s];
                if (live) A.obj_out[S.q_out[wave][s]] = obj;
                const bool pos = live && obj > 0.0;
                if constexpr (FILTER) c_eval += live;
                c_strong += pos;
                c_pos += pos;
                const uint64_t key = key_of(obj);
                hist_add_few(tk_hist, (uint32_t)(key >> 56), pos);
                if (PF && pos) { const int f = pf_code(key, false); atomicAdd(&pf_tab[f >> 1], (f & 1) ? 0x10000u : 1u); }
                // the strong members of the pass go to the emitted list (ScoreArgs::emit): ONE returning atomic reserves their
                // slots; the selection of a round in its strong regime reads (key, index) from there (TK_ROUTE_EMITTED)
                if (A.emit) {      // uniform
                    const unsigned long long pm = __ballot(pos);
                    if (pm) {      // uniform per wave
                        const int leader = __ffsll((long long)pm) - 1;
                        uint32_t base = 0;
                        if (lane == leader)
                            base = __hip_atomic_fetch_add(&A.tk->emit_n, (uint32_t)__popcll(pm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
                        const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((unsigned)(pm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)pm, 0u));
                        if (pos) {
                            if (slot < A.emit_cap) {
                                A.emit[2 * (size_t)slot] = key;
                                A.emit[2 * (size_t)slot + 1] = (uint64_t)(uint32_t)S.q_out[wave][s];
                            } else {
                                __hip_atomic_store(&A.tk->emit_over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                        }
                    }
                }
            };
            if constexpr (FILTER) {
                // one fp32 pass over the cnt <= 32 oldest entries of ring 1 (always two column tiles: padding columns compute on
                // stale slots and are not live); the survivors are appended to ring 2 in ring-1 order
                auto filter_round = [&](const int cnt) __attribute__((always_inline)) {
                    double yr[2];
                    float sl[2];
                    filter_pass_f32<K, H, NH>(net, S.s_f32, s_wout,
                                              [&](const int row, const int col) { return S.f_feat[wave][row][f_head + col]; }, lane, yr, sl);
                    if (q == 0) { S.f_y[wave][c16] = yr[0]; S.f_y[wave][16 + c16] = yr[1]; }
                    // (no staging for the slope sums: every lane of a column holds them, and lane s < 32 decides entry s = 16 q + c16,
                    // which is column c16 of tile q)
                    const float sv = q & 1 ? sl[1] : sl[0];
                    wave_lds_sync();
                    {
#pragma clang fp contract(off)
                        const int s = f_head + (lane & 31);
                        const bool live = lane < cnt;
                        // the exact epilogue's arithmetic on the fp32 pass's output
                        double acc = S.f_y[wave][lane & 31];
                        acc = acc + net.b_out;
                        const double y = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
                        const double me = S.f_maxel[wave][s];
                        double obj = S.f_negsm[wave][s];
                        obj = obj + y * me;
                        // (written so that a NaN survives)
                        const double mc = filter_cand_margin(net, sv);
                        const bool surv = live && (S.f_byp[wave][s] != 0 || !(obj <= -(mc * me)));
                        // The selection that follows reads obj_out of every violated candidate to tell the strong ones: an entry that
                        // stops here stores its fp32 measure, which is <= -margin max_elem <= 0 -- not strong, as proven.  (The
                        // array counts as not scored after such a launch; a completion overwrites the value.)
                        if (live && !surv) A.obj_out[S.f_out[wave][s]] = obj;
                        const unsigned long long sm = __ballot(surv);
                        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(sm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)sm, 0u));
                        const int tail_slot = q_head + q_fill >= LDS::QCAP ? q_head + q_fill - LDS::QCAP : q_head + q_fill;      // (scalar)
                        const int s2 = tail_slot + rank >= LDS::QCAP ? tail_slot + rank - LDS::QCAP : tail_slot + rank;
                        if (surv) {
#pragma unroll
                            for (int i = 0; i < DIN; ++i) feat[wave][i][s2] = S.f_feat[wave][i][s];
                            S.q_negsm[wave][s2] = S.f_negsm[wave][s];
                            S.q_maxel[wave][s2] = me;
                            S.q_out[wave][s2] = S.f_out[wave][s];
                        }
                        q_fill += __popcll(sm);
                    }
                    wave_lds_sync();      // ring 2 is complete for the fp64 pass, the ring-1 slots are free
                    f_head = f_head + 32 >= LDS::FCAP ? 0 : f_head + 32;
                    f_fill -= cnt;
                };
                // ring 2 first (an fp32 pass needs room for 32 survivors behind <= 31 pending), then ring 1; behind the wave's last
                // strip both are drained
                for (;;) {
                    if (q_fill >= 32 || (!nx_more && f_fill == 0 && q_fill > 16)) {
                        const int cnt = q_fill < 32 ? q_fill : 32;
                        mlp_pass(std::integral_constant<int, 2>{}, q_head);
                        wave_lds_sync();
                        skip_epilogue(cnt);
                        wave_lds_sync();
                        q_head = q_head + 32 >= LDS::QCAP ? 0 : q_head + 32;
                        q_fill -= cnt;
                        continue;
                    }
                    if (f_fill >= 32 || (!nx_more && f_fill > 0)) {
                        filter_round(f_fill < 32 ? f_fill : 32);
                        continue;
                    }
                    break;
                }
                if (!nx_more && q_fill > 0) {
                    mlp_pass(std::integral_constant<int, 1>{}, q_head);
                    wave_lds_sync();
                    skip_epilogue(q_fill);
                    wave_lds_sync();
                    q_fill = 0;
                }
                PHASE_MARK(4);
                tail = tail || nx_tail; s0 = nx_s0; more = nx_more;
                continue;
            }
            // passes while 32 entries are pending; behind the wave's last strip the rest (padding columns compute on stale slots, their
            // results are not stored)
            while (q_fill > 16 && (q_fill >= 32 || !nx_more)) {
                const int cnt = q_fill < 32 ? q_fill : 32;
                mlp_pass(std::integral_constant<int, 2>{}, q_head);
                wave_lds_sync();
                skip_epilogue(cnt);
                wave_lds_sync();      // the slots are free for the next strip's entries
                q_head = q_head + 32 >= LDS::QCAP ? 0 : q_head + 32;
                q_fill -= cnt;
            }
            if (!nx_more && q_fill > 0) {
                mlp_pass(std::integral_constant<int, 1>{}, q_head);
                wave_lds_sync();
                skip_epilogue(q_fill);
                wave_lds_sync();
                q_fill = 0;
            }
            PHASE_MARK(4);
            tail = tail || nx_tail; s0 = nx_s0; more = nx_more;
            continue;
        }
        {
            const int units = (int)((lim - s0 + 15) >> 4);      // column tiles of this strip that hold candidates
            // (a whole strip has its own loop with a constant trip count, and the rare paths are marked so: with one generic loop
            // the 5-variable kernel ran 1.5 % slower than before the split, this way 0.8 %, the 3- and 4-variable ones 1 % faster)
            if (__builtin_expect(units == 4, 1)) {
#pragma unroll 1
                for (int pass = 0; pass < 4 / JK; ++pass) mlp_pass(std::integral_constant<int, JK>{}, 16 * JK * pass);
            } else {
#pragma unroll 1
                for (int pass = 0; pass < units / JK; ++pass) mlp_pass(std::integral_constant<int, JK>{}, 16 * JK * pass);
                if constexpr (JK == 2) {
                    if (units & 1) mlp_pass(std::integral_constant<int, 1>{}, 16 * (units - 1));
                }
            }
        }
        wave_lds_sync();
        {
            // neural_net_3D.m:60-62, 81-85: y = (a + b - ymin)/gain + xoffset;  then :582
#pragma clang fp contract(off)
            double acc = ynn[wave][lane];
            acc = acc + net.b_out;
            const double y = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
            double obj = cd.negSM;
            obj = obj + y * cd.max_elem;
            if (valid) A.obj_out[out_idx] = obj;
            const bool viol = valid && (A.flags & SDPCUT_EIG) && lam < SDPCUT_NEG_EIGVAL, pos = valid && obj > 0.0;
            c_strong += viol && pos;
            if constexpr (FUSE != 0) {
                c_viol += viol;
                c_pos += pos;
                const bool member = FUSE == TK_MODE_OPT ? valid : FUSE == TK_MODE_FEAS ? viol : (viol && pos);
                const uint64_t key = key_of(FUSE == TK_MODE_FEAS ? -lam : obj);
                hist_add_few(tk_hist, (uint32_t)(key >> 56), member);
                if (PF && member) { const int f = pf_code(key, FUSE == TK_MODE_FEAS); atomicAdd(&pf_tab[f >> 1], (f & 1) ? 0x10000u : 1u); }      // (LDS, no return value: one ds_add per candidate)
            }
        }
        wave_lds_sync();   // feat / ynn are rewritten by the next tile
        PHASE_MARK(4);
        tail = tail || nx_tail; s0 = nx_s0; more = nx_more;
    }
    PHASE_REPORT;
    if (A.strong_out) {      // uniform: one no-return atomic per workgroup, into one of eight replicas
        uint32_t &s_strong = S.s_strong;
        if (threadIdx.x == 0) s_strong = 0;
        __syncthreads();
        for (int off = 32; off > 0; off >>= 1) c_strong += __shfl_xor((int)c_strong, off);
        if (lane == 0 && c_strong) atomicAdd(&s_strong, c_strong);
        __syncthreads();
        if (threadIdx.x == 0 && s_strong)
            __hip_atomic_fetch_add((unsigned long long *)&A.strong_out[blockIdx.x & 7], (unsigned long long)s_strong,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (FUSE != 0) {
        // No ticket, nobody waits: the kernel boundary orders the atomics before the selection.  (A ticket per
        // workgroup -- the last one resolving the digit, as the selection's own passes do -- costs a drain
        // of the workgroup's stores plus an atomic round trip before each of the 2048 workgroups may
        // retire: +14 us on this kernel.)
        for (int off = 32; off > 0; off >>= 1) {
            c_viol += __shfl_xor((int)c_viol, off);
            c_pos += __shfl_xor((int)c_pos, off);
        }
        if constexpr (FILTER) {
            for (int off = 32; off > 0; off >>= 1) c_eval += __shfl_xor((int)c_eval, off);
        }
        if (lane == 0) {
            if (c_viol) atomicAdd(&tk_cnt[0], c_viol);
            if (c_pos) atomicAdd(&tk_cnt[1], c_pos);
            if constexpr (FILTER) {
                if (c_eval) atomicAdd(&tk_cnt[2], c_eval);
            }
        }
        __syncthreads();
        if constexpr (FILTER) {
            if (threadIdx.x == 2 && tk_cnt[2])
                __hip_atomic_fetch_add((unsigned long long *)&A.tk->eval_rep[blockIdx.x % TK_SHREP], (unsigned long long)tk_cnt[2],
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (threadIdx.x < 2 && tk_cnt[threadIdx.x])
            __hip_atomic_fetch_add((unsigned long long *)(threadIdx.x ? &A.tk->pos_rep[blockIdx.x % TK_SHREP] : &A.tk->viol_rep[blockIdx.x % TK_SHREP]),
                                   (unsigned long long)tk_cnt[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tk_hist[threadIdx.x])
            __hip_atomic_fetch_add(&A.tk->hist_score[blockIdx.x % TK_SHREP][threadIdx.x], tk_hist[threadIdx.x], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (PF) {
            if (A.pf_mloc > 0) pf_retire_table(A.tk, pf_tab, A.pf_mloc);
        }      // (behind the barrier above: the table is complete)
    }
}

template <int K, int H, int NH, int FUSE = 0, bool CLAMP = true, int JK = 2>
__global__ __launch_bounds__(256, (JK == 1 ? SDPCUT_MFMA_J1_WAVES : 2)) void score_mfma_kernel(ScoreArgs A)
{
    __shared__ MfmaLds<K, H, NH> S;
    score_mfma_body<K, H, NH, FUSE, CLAMP, JK>(A, S, (int)blockIdx.x, (int)gridDim.x);
}

// The skipping variant (SKIP of score_mfma_body; score_plan_skip decides its work split): the fused scoring launch of a combined
// round over a class whose size is in SDPCUT_SKIP_KMASK.  Two workgroups per CU must stay resident: 80 KB of LDS at the most.
template <int K, int H, int NH, bool CLAMP>
__global__ __launch_bounds__(256, 2) void score_mfma_skip_kernel(ScoreArgs A)
{
    static_assert(sizeof(MfmaLdsSkip<K, H, NH>) <= 80 * 1024, "two workgroups of the skipping kernel must fit a CU's LDS");
    static_assert(SDPCUT_SMALL_IN_LDS, "the staging constants (s_stage) are filled with the small weights");
    __shared__ MfmaLdsSkip<K, H, NH> S;
    score_mfma_body<K, H, NH, TK_MODE_STRONG, CLAMP, 2, true>(A, S, (int)blockIdx.x, (int)gridDim.x);
}

// The skipping variant with the fp32 filter (FILTER of score_mfma_body): launched instead of it for a network with
// NetDev::filter_ok under SDPCUT_OPT_FP32_FILTER.  Clamp-free by construction (filter_ok implies unclamped_ok).
template <int K, int H, int NH>
__global__ __launch_bounds__(256, 2) void score_mfma_filter_kernel(ScoreArgs A)
{
    static_assert(sizeof(MfmaLdsFilter<K, H, NH>) <= 80 * 1024, "two workgroups of the filtering kernel must fit a CU's LDS");
    static_assert(SDPCUT_SMALL_IN_LDS, "the staging constants (s_stage) are filled with the small weights");
    __shared__ MfmaLdsFilter<K, H, NH> S;
    score_mfma_body<K, H, NH, TK_MODE_STRONG, false, 2, true, MfmaLdsFilter<K, H, NH>, true>(A, S, (int)blockIdx.x, (int)gridDim.x);
}

static_assert(2 * sizeof(MfmaLdsFilter<3, 50, 3>) <= 160 * 1024, "two workgroups of the shipped K = 3 filtering kernel per CU (160 KiB of LDS)");

// sdpcut_filter_audit: the fp32 pass of the filter -- the same device function as stage F -- for EVERY candidate of the class, its
// output unmapped into y32_out and, where asked for, its margin (filter_cand_margin) into m_out (caller order).  Not on the hot path: a wave takes 32 candidates at a time, stages their mapped
// inputs exactly as the scoring kernel does (clamp-free form) and runs one pass.
template <int K, int H, int NH>
__global__ __launch_bounds__(256) void filter_audit_kernel(ScoreArgs A, double *y32_out, double *m_out)
{
    constexpr int DIN = K + K * (K + 1) / 2;
    __shared__ double s_feat[4][DIN][32];
    __shared__ FilterLds<NH> s_f32;
    __shared__ double s_wout[64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int q = lane >> 4, c16 = lane & 15;
    const NetDev &net = A.net;
    filter_lds_fill<NH>(net, s_f32);
    if (threadIdx.x < 64) s_wout[threadIdx.x] = net.wout[threadIdx.x];
    __syncthreads();
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 32; base < A.n; base += (int64_t)gridDim.x * 4 * 32) {
        const int64_t c = base + (lane & 31);
        Cand<K> cd;
        gather_candidate<K>(cd, A.set, A.n, c < A.n ? c : base, A.vars, A.Q, A.nv, A.L, true);
        if (lane < 32) {
#pragma unroll
            for (int i = 0; i < DIN; ++i) {
                const double v = (i < K) ? cd.x[i < K ? i : 0] : cd.q[i >= K ? i - K : 0];
                double xp = (v - net.inmap[i]) * net.inmap[DIN + i] + net.ymin;
                xp = min_f64_raw(max_f64_raw(xp, -SDPCUT_INPUT_CLAMP), SDPCUT_INPUT_CLAMP);
                s_feat[wave][i][lane] = xp;
            }
        }
        wave_lds_sync();
        double yr[2];
        float sl[2];
        filter_pass_f32<K, H, NH>(net, s_f32, s_wout, [&](const int row, const int col) { return s_feat[wave][row][col]; }, lane, yr, sl);
        if (q == 0) {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t cj = base + 16 * j + c16;
                double acc = yr[j];
                acc = acc + net.b_out;
                const double y = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
                if (cj < A.n) {
                    y32_out[A.orig[cj]] = y;
                    if (m_out) m_out[A.orig[cj]] = filter_cand_margin(net, sl[j]);
                }
            }
        }
        wave_lds_sync();      // s_feat is rewritten by the next round
    }
}

// The same kernel at the P = gridDim.y LP points of a batch (sdpcut_score_points / sdpcut_round_csr_points, points.hip): workgroup
// row y reads point y (and, in a boxed batch, the Q' of point y: ps.Q = L, else 0) and writes row y of the batch's score arrays (and
// adds to point y's strong counter).  The offsets are applied
// to the kernel ARGUMENT -- blockIdx.y and the strides are scalars, the sums stay in scalar registers -- and the unchanged body runs
// on the copy: the same code per candidate, the same scores.  No histogram variants (FUSE = 0): the batched selection builds its
// own keys.
template <int K, int H, int NH, bool CLAMP, int JK>
__global__ __launch_bounds__(256, (JK == 1 ? SDPCUT_MFMA_J1_WAVES : 2)) void score_mfma_points_kernel(ScoreArgs A, ScorePointStrides ps)
{
    __shared__ MfmaLds<K, H, NH> S;
    const int64_t p = (int64_t)blockIdx.y;
    A.vars += p * ps.vars;
    A.Q += p * ps.Q;
    A.eig_out += p * ps.scores;
    A.obj_out += p * ps.scores;
    if (A.strong_out) A.strong_out += p * ps.strong;
    score_mfma_body<K, H, NH, 0, CLAMP, JK>(A, S, (int)blockIdx.x, (int)gridDim.x);
}

// ONE launch for every size class of a list (r3).  Real covers hold one large class and a few sets of the smaller sizes
// (spar100-050-1, dim 5: 72 673 five-variable sets, 103 of four, 1 of three); a launch per class costs what one pass costs however
// few candidates it holds, and side streams run side by side only if the process's streams were handed different hardware queues.
// Here every class gets its own range of workgroups of one launch, the largest class first; a workgroup serves exactly one
// class (its code is the single-class kernel's, its LDS a union of the classes').
template <int K> using MfmaLdsOf = MfmaLds<K, NetShape<K>::H, NetShape<K>::NH>;

// one class of the launch over all classes: the single-class kernel's body, two column tiles per pass
#define SCORE_MFMA_CLASS(K, lds) score_mfma_body<K, NetShape<K>::H, NetShape<K>::NH, FUSE, CLAMP, 2>(AA.a[c], lds, bid, nblk)

template <int FUSE, bool CLAMP>
__global__ __launch_bounds__(256, 2) void score_mfma_all_kernel(ScoreArgsAll AA)
{
    __shared__ union LdsAll {
        MfmaLdsOf<2> l2;
        MfmaLdsOf<3> l3;
        MfmaLdsOf<4> l4;
        MfmaLdsOf<5> l5;
        __device__ LdsAll() {}
    } S;
    int c = 0;
    while (c + 1 < AA.nclasses && (int)blockIdx.x >= AA.bend[c]) ++c;      // uniform
    const int b0 = c ? AA.bend[c - 1] : 0;
    const int bid = (int)blockIdx.x - b0, nblk = AA.bend[c] - b0;
    switch (AA.k[c]) {
    case 2: SCORE_MFMA_CLASS(2, S.l2); break;
    case 3: SCORE_MFMA_CLASS(3, S.l3); break;
    case 4: SCORE_MFMA_CLASS(4, S.l4); break;
    default: SCORE_MFMA_CLASS(5, S.l5); break;
    }
}
#undef SCORE_MFMA_CLASS

// ------------------------------------------------------------------------------------------
// host launchers
// The FUSE argument of the kernels as a compile-time tag: f(std::integral_constant<int, FUSE>) for the mode's FUSE ...
template <class F>
static void with_fuse_tag(int mode, F &&f)
{
    switch (mode) {
    case TK_MODE_STRONG: f(std::integral_constant<int, TK_MODE_STRONG>{}); break;
    case TK_MODE_OPT: f(std::integral_constant<int, TK_MODE_OPT>{}); break;
    case TK_MODE_FEAS: f(std::integral_constant<int, TK_MODE_FEAS>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
    }
}
// ... and FUSE x CLAMP: f(fuse tag, std::bool_constant<CLAMP>)
template <class F>
static void with_fuse_clamp_tags(int mode, bool clamp, F &&f)
{
    with_fuse_tag(mode, [&](auto fuse_tag) {
        if (clamp) f(fuse_tag, std::true_type{});
        else f(fuse_tag, std::false_type{});
    });
}

template <int K>
static void score_mfma_launch_k(const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    // (same arithmetic in every variant of one network: bit-equal scores)
    with_fuse_clamp_tags(A.tk ? A.tk_mode : 0, !A.net.unclamped_ok, [&](auto fuse_tag, auto clamp_tag) {
        constexpr int F = decltype(fuse_tag)::value;
        constexpr bool C = decltype(clamp_tag)::value;
        SCORE_LAUNCH((score_mfma_kernel<K, NetShape<K>::H, NetShape<K>::NH, F, C, mfma_cols(K)>), grid, 256);
    });
}

void score_mfma_launch(int K, const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    switch (K) {
    case 2: score_mfma_launch_k<2>(A, grid, st, ev_start, ev_stop); break;
    case 3: score_mfma_launch_k<3>(A, grid, st, ev_start, ev_stop); break;
    case 4: score_mfma_launch_k<4>(A, grid, st, ev_start, ev_stop); break;
    default: score_mfma_launch_k<5>(A, grid, st, ev_start, ev_stop); break;
    }
}

template <int K>
static void score_mfma_skip_launch_k(const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    if constexpr (skip_k(K) && mfma_cols(K) == 2) {
        if (A.net.unclamped_ok) SCORE_LAUNCH((score_mfma_skip_kernel<K, NetShape<K>::H, NetShape<K>::NH, false>), grid, 256);
        else SCORE_LAUNCH((score_mfma_skip_kernel<K, NetShape<K>::H, NetShape<K>::NH, true>), grid, 256);
    }
}

// has size class K a skipping instantiation?  (score_skip_applies asks skip_k alone; the one-tile-per-pass experiment has none)
bool score_mfma_skip_built(int K) { return skip_k(K) && mfma_cols(K) == 2; }

void score_mfma_skip_launch(int K, const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    switch (K) {
    case 2: score_mfma_skip_launch_k<2>(A, grid, st, ev_start, ev_stop); break;
    case 3: score_mfma_skip_launch_k<3>(A, grid, st, ev_start, ev_stop); break;
    case 4: score_mfma_skip_launch_k<4>(A, grid, st, ev_start, ev_stop); break;
    default: score_mfma_skip_launch_k<5>(A, grid, st, ev_start, ev_stop); break;
    }
}

// The fp32 filter is instantiated for the shipped 3-variable class alone (net_pack.h: filter_shape grants filter_ok to no other)
static_assert(NetShape<3>::H == 50 && NetShape<3>::NH == 3 && skip_k(3) && mfma_cols(3) == 2, "filter_shape of net_pack.h names NetShape<3>");
bool score_mfma_filter_built(int K) { return K == 3; }

void score_mfma_filter_launch(int K, const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    if (K == 3) SCORE_LAUNCH((score_mfma_filter_kernel<3, NetShape<3>::H, NetShape<3>::NH>), grid, 256);
}

void score_filter_audit_launch(int K, const ScoreArgs &A, int grid, double *d_y32, double *d_m, hipStream_t st)
{
    if (K == 3) hipLaunchKernelGGL((filter_audit_kernel<3, NetShape<3>::H, NetShape<3>::NH>), dim3(grid), dim3(256), 0, st, A, d_y32, d_m);
}

template <int K>
static void score_mfma_points_launch_k(const ScoreArgs &A, const ScorePointStrides &ps, int grid, int n_points, hipStream_t st)
{
    if (A.net.unclamped_ok)
        hipLaunchKernelGGL((score_mfma_points_kernel<K, NetShape<K>::H, NetShape<K>::NH, false, mfma_cols(K)>), dim3(grid, n_points), dim3(256), 0, st, A, ps);
    else
        hipLaunchKernelGGL((score_mfma_points_kernel<K, NetShape<K>::H, NetShape<K>::NH, true, mfma_cols(K)>), dim3(grid, n_points), dim3(256), 0, st, A, ps);
}

void score_mfma_points_launch(int K, const ScoreArgs &A, const ScorePointStrides &ps, int grid, int n_points, hipStream_t st)
{
    switch (K) {
    case 2: score_mfma_points_launch_k<2>(A, ps, grid, n_points, st); break;
    case 3: score_mfma_points_launch_k<3>(A, ps, grid, n_points, st); break;
    case 4: score_mfma_points_launch_k<4>(A, ps, grid, n_points, st); break;
    default: score_mfma_points_launch_k<5>(A, ps, grid, n_points, st); break;
    }
}

// every class runs the clamp-free instantiation (score_form: the one-launch form needs unclamped_ok of every class)
void score_mfma_all_launch(const ScoreArgsAll &A, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    const int grid = A.bend[A.nclasses - 1];
    with_fuse_tag(A.a[0].tk ? A.a[0].tk_mode : 0, [&](auto fuse_tag) {
        SCORE_LAUNCH((score_mfma_all_kernel<decltype(fuse_tag)::value, false>), grid, 256);
    });
}
