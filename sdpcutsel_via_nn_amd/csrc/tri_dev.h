// Triangle inequalities, the device functions the kernels of tri.hip and tri_points.hip share: the four violations of a triple, the
// selection key of an entry, the row of an entry in the original variables, a block scan.  The numpy twin is
// sdpcutsel_via_nn_amd/triangles.py: every expression below is written there in the same order, fp64, no contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TRI_VIOL_THRES 1e-7     /* _THRES_TRI_VIOL, cut_select_qp.py:33 */

// the four violations of triple a < b < c at the point table `vars` ([X packed | x]; at a node: the box table x', X'), cut_select_qp.py
// :836-839, left to right
__device__ __forceinline__ void tri_viol4(const double *vars, int32_t nv, int64_t L, int32_t a, int32_t b, int32_t c, double v[4])
{
#pragma clang fp contract(off)
    const int32_t ra = nv * a - (a * (a + 1)) / 2, rb = nv * b - (b * (b + 1)) / 2;
    const double X1 = vars[ra + b], X2 = vars[ra + c], X4 = vars[rb + c];      // X_slice[1], [2], [4]
    const double x0 = vars[L + a], x1 = vars[L + b], x2 = vars[L + c];
    v[0] = X1 + X2 - X4 - x0;
    v[1] = X1 - X2 + X4 - x1;
    v[2] = -X1 + X2 + X4 - x2;
    v[3] = -X1 - X2 - X4 + (((0.0 + x0) + x1) + x2) - 1.0;
}

// key: bit 63 = density 3, low bits = the positive violation's IEEE image (positive doubles order like integers); 0 = not violated
// (a NaN compares false: not violated).  Violations are <= 2 in every box's own units, so bit 63 is free.
__device__ __forceinline__ uint64_t tri_key(double v, uint64_t hi)
{
    return v >= TRI_VIOL_THRES ? (hi | (uint64_t)__double_as_longlong(v)) : 0ull;
}
__device__ __forceinline__ double tri_key_viol(uint64_t key) { return __longlong_as_double((long long)(key & 0x7fffffffffffffffull)); }

// The row of entry 4 t + type of triple a < b < c, sense >=, in the columns of vars_values.  The facet in the box's variables is
//     s1 X'_ab + s2 X'_ac + s4 X'_bc + ta x'_a + tb x'_b + tc x'_c >= r      (type 0 .. 2: r = 0, one t is 1; type 3: r = -1, t = -1)
// and X'_ij = (X_ij - l_i x_j - l_j x_i + l_i l_j) / (d_i d_j), x'_i = (x_i - l_i) / d_i put into it give three X columns, up to three
// x columns and a right-hand side.  ld: the (l | d) table of the box, [2 nv], or NULL (the unit box: l = 0, d = 1).  A coefficient
// that is exactly zero is dropped: on the unit box the 4 / 6 pattern with coefficients +-1 and rhs 0 / -1 comes back.
// cols / vals: X_ab, X_ac, X_bc, then the x columns in ascending variable order -> the number of non-zeros.
__device__ __forceinline__ int tri_row(int type, int32_t a, int32_t b, int32_t c, const double *ld, int32_t nv, int64_t L, int32_t cols[6],
                                       double vals[6], double &rhs)
{
#pragma clang fp contract(off)
    const double la = ld ? ld[a] : 0.0, lb = ld ? ld[b] : 0.0, lc = ld ? ld[c] : 0.0;
    const double da = ld ? ld[nv + a] : 1.0, db = ld ? ld[nv + b] : 1.0, dc = ld ? ld[nv + c] : 1.0;
    const double s1 = type >= 2 ? 1.0 : -1.0, s2 = (type & 1) ? 1.0 : -1.0, s4 = (type == 0 || type == 3) ? 1.0 : -1.0;
    const double ta = type == 0 ? 1.0 : (type == 3 ? -1.0 : 0.0), tb = type == 1 ? 1.0 : (type == 3 ? -1.0 : 0.0),
                 tc = type == 2 ? 1.0 : (type == 3 ? -1.0 : 0.0);
    const double r = type == 3 ? -1.0 : 0.0;
    const double w1 = s1 / (da * db), w2 = s2 / (da * dc), w4 = s4 / (db * dc);
    const double ca = (ta / da - w1 * lb) - w2 * lc;
    const double cb = (tb / db - w1 * la) - w4 * lc;
    const double cc = (tc / dc - w2 * la) - w4 * lb;
    rhs = (r - ((w1 * (la * lb) + w2 * (la * lc)) + w4 * (lb * lc))) + ((ta * (la / da) + tb * (lb / db)) + tc * (lc / dc));
    const int32_t ra = nv * a - (a * (a + 1)) / 2, rb = nv * b - (b * (b + 1)) / 2;
    cols[0] = ra + b; cols[1] = ra + c; cols[2] = rb + c;
    vals[0] = w1; vals[1] = w2; vals[2] = w4;
    int m = 3;
    if (ca != 0.0) { cols[m] = (int32_t)L + a; vals[m] = ca; ++m; }
    if (cb != 0.0) { cols[m] = (int32_t)L + b; vals[m] = cb; ++m; }
    if (cc != 0.0) { cols[m] = (int32_t)L + c; vals[m] = cc; ++m; }
    return m;
}

// exclusive scan of v over a workgroup of NW waves (every thread calls it); s_wave: NW words of LDS, free again on return
template <int NW>
__device__ __forceinline__ uint32_t tri_block_scan(uint32_t v, uint32_t *s_wave, uint32_t &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(incl, off);
        if (lane >= off) incl += u;
    }
    if (lane == 63) s_wave[w] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint32_t x = s_wave[i];
        before += i < w ? x : 0u;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return before + incl - v;
}

// The rows of `count` head entries into the block at `block` (tri_layout.h: tri_layout(cap)), by a whole workgroup of NW waves:
// entry i = ent(i), its violation vio(i); a scan over the row lengths places the rows.  Writes the header last (word 3: void_flag).
struct TriBlockPtrs { int64_t *hdr, *entry; double *viol, *rhs, *values; int32_t *indptr, *indices; };
template <int NW, typename EntF, typename VioF>
__device__ __forceinline__ void tri_emit_rows(int64_t count, EntF ent, VioF vio, const int32_t *tri, int64_t T, const double *ld, int32_t nv, int64_t L,
                                              const TriBlockPtrs &B, int64_t n_violated, int64_t void_flag, uint32_t *s_wave)
{
    uint32_t run = 0;
    for (int64_t base = 0; base < count; base += NW * 64) {      // (uniform trip count: the scan holds barriers)
        const int64_t i = base + threadIdx.x;
        int32_t cols[6];
        double vals[6], rhs = 0.0;
        int m = 0;
        int64_t e = 0;
        if (i < count) {
            e = ent(i);
            const int64_t t = (e >= 0 && e < 4 * T) ? e >> 2 : 0;      // (a selected entry is one of the 4 T; never an address from a stray id)
            m = tri_row((int)(e & 3), tri[3 * t], tri[3 * t + 1], tri[3 * t + 2], ld, nv, L, cols, vals, rhs);
        }
        uint32_t total;
        const uint32_t at = run + tri_block_scan<NW>((uint32_t)m, s_wave, total);
        if (i < count) {
            B.entry[i] = e;
            B.viol[i] = vio(i);
            B.rhs[i] = rhs;
            B.indptr[i] = (int32_t)at;
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (j < m) { B.values[at + j] = vals[j]; B.indices[at + j] = cols[j]; }
        }
        run += total;
    }
    if (threadIdx.x == 0) {
        B.indptr[count] = (int32_t)run;
        B.hdr[0] = count; B.hdr[1] = n_violated; B.hdr[2] = (int64_t)run; B.hdr[3] = void_flag;
    }
}
