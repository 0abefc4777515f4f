// tansig, the activation of the trained MLPs, as the scoring kernels evaluate it (score_mfma.hip: tansig_tile / tansig_y8 on the
// MFMA accumulators; score_alt.hip: tansig in the VALU kernel).  Device code only; the accuracy derivations below are the
// documentation of every constant.
#pragma once
#include <hip/hip_runtime.h>

typedef double d4 __attribute__((ext_vector_type(4)));

// tansig as MATLAB defines it (neural_net_3D.m:77-79): a = 2 / (1 + exp(-2 n)) - 1
__device__ __forceinline__ double tansig_lib(double n)
{
    return 2.0 / (exp(-2.0 * n) + 1.0) - 1.0;
}

// The same formula with a branch-free exp and reciprocal: 23 VALU instructions instead of the
// ~36 of the library route (every VALU instruction costs ~2-2.5 ns per wave on gfx950 whatever
// its type, v_rcp_f64 ~7 ns: profiles/r01_ubench_fp64_instruction_costs.txt -- the COUNT is
// what matters).
//
// exp(-2n): with y = -2n,  exp(y) = 2^k * exp(r/8)^8,  k = rint(y log2 e),  r/8 = y/8 - k ln2/8
// (|r/8| <= ln2/16 = 0.0433), three squarings.
//  * one-constant reduction: fl(ln2/8) is off by <= 7e-18, so r/8 is off by <= |k| 7e-18; where
//    tansig is sensitive to exp (|k| <= 40, sensitivity 2e/(1+e)^2 <= 1/2) that is <= 3e-16 in
//    the result, in saturation the sensitivity kills it;
//  * degree-7 near-minimax polynomial (truncated Chebyshev series of exp on |r| <= ln2/16;
//    coefficients computed in 60-digit arithmetic): max relative error 5e-18, the accuracy of the
//    degree-8 Taylor polynomial with one FMA less;
//  * only the upper clamp is needed (y8max = 88 keeps exp finite; towards -inf ldexp underflows
//    to 0 and tansig saturates at +1 by itself).
//  * k is rounded with the 1.5 * 2^52 trick: the low dword of t IS k as an int32 (|k| < 2^31, i.e.
//    |y| < 1.4e9 -- pre-activations of these networks stay below 1e3), which saves the
//    double->int conversion; with the constant lowered by SHIFT the dword holds k - SHIFT, so
//    exp(y) / 2 (SHIFT = 1, what tansig4/tansig8 want) costs nothing extra and is exact.
// fmin() goes through the IEEE quieting rule (v_max_f64 x, x in front of the v_min_f64): the operand
// here is an accumulator that cannot be a signalling NaN, so take the bare instruction (one issue
// slot per activation, 150 activations per candidate)
__device__ __forceinline__ double min_f64_raw(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ double max_f64_raw(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// CLAMP = false: the caller guarantees y8_in <= y8max (NetDev::unclamped_ok: the network's
// pre-activations are bounded, see sdpcut_set_network) -- one instruction less per activation.
// Degree of the exp polynomial.  7 (default): tansig to 8e-16, obj_improve to <= 1e-11 of the CPU path on the
// synthetic workload.  6 saves one FMA per activation (-4.5 us of 333 on 1e6 three-variable candidates) but
// raises the score error to 2-5e-10 relative (tools/accuracy.py) -- inside BASELINE's 1e-6, too close to the
// 1e-9 this repository tests to; measured and left off.
#ifndef SDPCUT_EXP_DEGREE
#define SDPCUT_EXP_DEGREE 7
#endif
template <int SHIFT, bool CLAMP = true>
__device__ __forceinline__ double exp_y8_scaled(double y8_in, double y8max)     // exp(8 y8_in) / 2^SHIFT
{
    constexpr double MAGIC = 0x1.8p52 - (double)SHIFT;
    const double y8 = CLAMP ? min_f64_raw(y8_in, y8max) : y8_in;
    const double t = fma(y8, 11.541560327111707259, MAGIC);         // 8 log2 e
    const double k = t - MAGIC;
    const double r = fma(k, -0x1.62e42fefa39efp-4, y8);              // fl(ln2 / 8)
#if SDPCUT_EXP_DEGREE == 7
    double p = 0x1.a02041015378fp-13;
    p = fma(p, r, 0x1.6c1d00cea5bf1p-10);
    p = fma(p, r, 0x1.111111080fc42p-7);
    p = fma(p, r, 0x1.5555554653263p-5);
    p = fma(p, r, 0x1.5555555555689p-3);
    p = fma(p, r, 0x1.0000000000171p-1);
#else   // degree 6, weighted minimax of (exp(r) - 1 - r) / r^2 (tools/exp_poly.py): relative error 1.5e-15
    double p = 0x1.6c0ed7b92eac2p-10;
    p = fma(p, r, 0x1.1115b77b92f70p-7);
    p = fma(p, r, 0x1.5555558fc88efp-5);
    p = fma(p, r, 0x1.55555548f8ee9p-3);
    p = fma(p, r, 0x1.fffffffffee2fp-2);
#endif
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    p = p * p;
    p = p * p;
    p = p * p;
    return ldexp(p, __double2loint(t));
}

// exp(8 y8) / 2^SHIFT + addend for BOUNDED arguments (|8 y8| <= 80, NetDev::unclamped_ok): the power of two goes
// into the exponent field of p^4 with one integer add -- p^4 lies in [0.65, 1.47] and |k| <= 117, so the field
// neither overflows nor reaches the denormals -- and the last squaring, the scaling and the addend become ONE
// fma: 14 instead of 16 issue slots per activation, one rounding less.
#ifndef SDPCUT_EXP_SCALE_LDEXP
#define SDPCUT_EXP_SCALE_LDEXP 1
#endif
template <int SHIFT>
__device__ __forceinline__ double exp_y8_plus_bounded(double y8, double addend)
{
    constexpr double MAGIC = 0x1.8p52 - (double)SHIFT;
    const double t = fma(y8, 11.541560327111707259, MAGIC);         // 8 log2 e; low dword = k - SHIFT
    const double k = t - MAGIC;
    const double r = fma(k, -0x1.62e42fefa39efp-4, y8);              // fl(ln2 / 8)
    double p = 0x1.a02041015378fp-13;
    p = fma(p, r, 0x1.6c1d00cea5bf1p-10);
    p = fma(p, r, 0x1.111111080fc42p-7);
    p = fma(p, r, 0x1.5555554653263p-5);
    p = fma(p, r, 0x1.5555555555689p-3);
    p = fma(p, r, 0x1.0000000000171p-1);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    p = p * p;
    p = p * p;                                                       // exp(r)^4
#if SDPCUT_EXP_SCALE_LDEXP
    // (r4) v_ldexp_f64 with the low dword of t as its integer operand: ONE instruction for the scaled copy where the integer add
    // into the exponent field needs two (v_lshl_add_u32 on the high dword + a v_mov_b32 of the low one to complete the register
    // pair -- the unscaled p is still needed).  Same bits: both are exact scalings by 2^(k - SHIFT) in this range.
    const double ps = ldexp(p, __double2loint(t));
#else
    const double ps = __hiloint2double(__double2hiint(p) + (__double2loint(t) << 20), __double2loint(p));
#endif
    return fma(ps, p, addend);
}
__device__ __forceinline__ double exp_y8(double y8_in, double y8max)     // exp(8 y8_in), y8_in = -n / 4
{
    return exp_y8_scaled<0>(y8_in, y8max);
}
__device__ __forceinline__ double exp_m2n(double n, double y8max) { return exp_y8(n * -0.25, y8max); }

// The reciprocal is v_rcp_f64 (4.5e-8) + one cubically convergent step.  Absolute error of
// tansig vs the exact formula <= 1e-15.
__device__ __forceinline__ double tansig(double n)
{
    const double d = exp_m2n(n, 88.0) + 1.0;
    double q = __builtin_amdgcn_rcp(d);
    const double e = fma(-d, q, 1.0);
    q = fma(q, fma(e, e, e), q);                        // q (1 + e + e^2)
    return fma(2.0, q, -1.0);
}

template <bool CLAMP = true>
__device__ __forceinline__ double tansig_y8(double y8)  // the accumulators of the MFMA kernel hold y/8 = -n/4 (NetDev::bias_q)
{
    const double d = CLAMP ? exp_y8_scaled<0, true>(y8, 88.0) + 1.0 : exp_y8_plus_bounded<0>(y8, 1.0);
    double q = __builtin_amdgcn_rcp(d);
    const double e = fma(-d, q, 1.0);
    q = fma(q, fma(e, e, e), q);
    return fma(2.0, q, -1.0);
}

// HALF the denominator of tansig, h = (exp(-2n) + 1) / 2, so that tansig = 1/h - 1 (the factor 2
// of the formula is absorbed exactly by the exponent shift of exp_y8_scaled<1>).
template <bool CLAMP = true>
__device__ __forceinline__ double tansig_hden_y8(double y8, double y8max)
{
    if constexpr (CLAMP) return exp_y8_scaled<1, true>(y8, y8max) + 0.5;
    else return exp_y8_plus_bounded<1>(y8, 0.5);
}

// Four tansig values with ONE reciprocal: 1/h_i = (1 / (h0 h1 h2 h3)) * prod_{j != i} h_j.
// v_rcp_f64 plus its refinement is 6 issue slots (the kernel is bound by the VALU/MFMA
// instruction count): shared by four values the reciprocal part costs 3.5 slots per value
// instead of 7, and the halved denominators drop the doubling.  Every h_i is >= 1/2 and
// <= (1 + e^176) / 2 (y = -2n clamped to 176: tansig(-88) is -1 to 2e-76 either way), so the
// product neither underflows nor overflows; the extra roundings stay below 5e-16 relative.
// The four values are four neurons of ONE candidate (the rows of a C/D fragment), so a
// candidate's score does not depend on its neighbours in the wave.  (Sharing over the eight
// values of the two column tiles saved another 0.7 % but made duplicates of a candidate differ
// in the last bit depending on their position -- ties would no longer break by index.)
template <bool CLAMP = true>
__device__ __forceinline__ void tansig4(double &v0, double &v1, double &v2, double &v3)
{
    const double d0 = tansig_hden_y8<CLAMP>(v0, 22.0), d1 = tansig_hden_y8<CLAMP>(v1, 22.0);
    const double d2 = tansig_hden_y8<CLAMP>(v2, 22.0), d3 = tansig_hden_y8<CLAMP>(v3, 22.0);
    const double d01 = d0 * d1, d23 = d2 * d3;
    const double dd = d01 * d23;
    double q = __builtin_amdgcn_rcp(dd);
    const double e = fma(-dd, q, 1.0);
    q = fma(q, fma(e, e, e), q);
    const double q01 = q * d23, q23 = q * d01;          // 1/(h0 h1), 1/(h2 h3)
    v0 = fma(q01, d1, -1.0);
    v1 = fma(q01, d0, -1.0);
    v2 = fma(q23, d3, -1.0);
    v3 = fma(q23, d2, -1.0);
}

// tansig of one MFMA C/D fragment (rows 16 t + 4 r + q, r = 0..3); rows >= H are padding -> 0
template <int H, bool CLAMP = true>
__device__ __forceinline__ d4 tansig_tile(d4 c, int t)
{
    double v0 = c[0], v1 = c[1], v2 = c[2], v3 = c[3];
#ifndef SDPCUT_ABL_NOTANSIG     // tools/build_ablation.sh: timing experiments only
    tansig4<CLAMP>(v0, v1, v2, v3);
#endif
    d4 out;
    out[0] = (16 * t + 0 < H) ? v0 : 0.0;
    out[1] = (16 * t + 4 < H) ? v1 : 0.0;
    out[2] = (16 * t + 8 < H) ? v2 : 0.0;
    out[3] = (16 * t + 12 < H) ? v3 : 0.0;
    return out;
}

// ---- fp32, for the filter stage of the skipping kernel (score_mfma.hip, stage F).  Its accumulators hold z = -2 log2(e) n (the
// scale is folded into the packed weights and biases, net_pack.h), so tansig(n) = 2 / (1 + 2^z) - 1 is v_exp_f32, v_add_f32,
// v_rcp_f32, v_fma_f32 -- no range reduction, no refinement.  Accuracy: both transcendentals are documented to 1 ulp; the
// derivation of the filter's margin (net_pack.h: net_filter_margin) charges 13 * 2^-24 per activation for this function on top of
// the exact formula and spells out where each part comes from.  |z| <= 116 for a network with unclamped_ok, the only kind that
// filters: 2^z stays a normal number.  A NaN or an infinity (a stale queue slot) passes through as NaN or saturates; the filter
// lets a NaN survive.
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float tansig_f32_z(float z)
{
    const float d = __builtin_amdgcn_exp2f(z) + 1.0f;
    return __builtin_fmaf(2.0f, __builtin_amdgcn_rcpf(d), -1.0f);
}
