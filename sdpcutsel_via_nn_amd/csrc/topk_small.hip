// Top-k selection, the one-workgroup routes for short lists (TK_ROUTE_SMALLSORT / TK_ROUTE_SMALLSEL / TK_ROUTE_SMALL,
// topk_route.h): no key array, no radix passes over memory.

#include "topk_launch.h"
#include "topk_small_dev.h"

// Lists that fit the sort buffers whole (n <= 8192 -- most of the reference's BoxQP / QCQP instances)
// need no radix passes: ONE workgroup builds the keys, counts the class and compacts its members;
// the sort that follows orders all of them and emits the first k_eff.  Three launches instead of
// seven on the latency-bound end of the problem sizes.
#ifndef TK_SMALL_THREADS
#define TK_SMALL_THREADS 1024     // (one workgroup: a row of the list per 1024 candidates instead of 256)
#endif
__global__ __launch_bounds__(TK_SMALL_THREADS) void tk_small_kernel(int mode, int64_t sel, int64_t n, int64_t k, const double *eig,
                                                              const double *obj, TopkWs *ws, uint64_t *sel_key,
                                                              uint32_t *sel_idx)
{
    __shared__ uint32_t cnt[4];      // class members, violated, positive, next slot
    mode = resolve_mode(mode, ws, sel);
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // (r4) eight rows of loads in flight: ONE workgroup has nobody to hide a memory round trip behind, and a 7899-candidate cover
    // is 31 rows -- 23 us of dependent trips on the critical path of a QCQP round before, ~5 now
    const double *pe = eig ? eig : obj, *po = obj ? obj : eig;      // (a measure the mode does not use is never looked at)
    double pre_e[8], pre_o[8];
    for (int64_t i0 = 0; i0 < n; i0 += TK_SMALL_THREADS) {
        const int u = (int)((i0 / TK_SMALL_THREADS) & 7);
        if (u == 0) {
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int64_t j = i0 + (int64_t)v * TK_SMALL_THREADS + threadIdx.x;
                const int64_t jc = j < n ? j : n - 1;
                pre_e[v] = pe[jc];
                pre_o[v] = po[jc];
            }
        }
        double e_u = pre_e[0], o_u = pre_o[0];
#pragma unroll
        for (int v = 1; v < 8; ++v) { e_u = (u == v) ? pre_e[v] : e_u; o_u = (u == v) ? pre_o[v] : o_u; }
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < n;
        const double e = (in && eig) ? e_u : 0.0, o = (in && obj) ? o_u : 0.0;
        const uint64_t key = in ? masked_key(mode, e, o) : 0ull;
        const bool member = in && ((mode == TK_MODE_OPT || mode == TK_MODE_COMBALL) ? true : key != 0ull);
        const unsigned long long mm = __ballot(member);
        const unsigned long long mv = __ballot(in && eig != nullptr && e < SDPCUT_NEG_EIGVAL);
        const unsigned long long mp = __ballot(in && obj != nullptr && o > 0.0);
        uint32_t base = 0;
        if (lane == 0) {
            if (mm) base = atomicAdd(&cnt[3], (uint32_t)__popcll(mm));
            if (mv) atomicAdd(&cnt[1], (uint32_t)__popcll(mv));
            if (mp) atomicAdd(&cnt[2], (uint32_t)__popcll(mp));
        }
        base = (uint32_t)__shfl((int)base, 0);
        if (member) {
            const uint32_t slot = base + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
            sel_key[slot] = key;
            sel_idx[slot] = (uint32_t)i;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t cls = cnt[3];
        ws->counters[0] = cls;
        ws->counters[1] = cnt[1];
        ws->counters[2] = cnt[2];
        ws->counters[3] = k < cls ? k : cls;
        ws->n_sel = cls;
        ws->mode = mode;
        ws->counters[6] = mode;
        ws->counters[5] = strong_total(ws);
    }
}

// Short lists WITH a selection: ONE workgroup keeps the keys of n <= TK_SMALLSEL_N candidates in LDS, selects, and (SORT) sorts and
// emits the head itself.  The algorithm is smallsel_body (topk_small_dev.h).
template <bool SORT>
__global__ __launch_bounds__(TK_SMALLSEL_THREADS) void tk_smallsel_kernel(int mode, int64_t sel, int n, int k, const double *eig,
                                                                          const double *obj, TopkWs *ws, uint64_t *sel_key,
                                                                          uint32_t *sel_idx, int64_t base, double score_add,
                                                                          int64_t *idx_out, double *score_out)
{
    smallsel_body<SORT, TK_SMALLSEL_N>(mode, sel, n, k, eig, obj, ws, sel_key, sel_idx, base, score_add, idx_out, score_out);
}

void tk_small_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    if (p.route == TK_ROUTE_SMALLSORT)      // a short list with a head of one tile at most: selection, sort and emission in ONE launch
        hipLaunchKernelGGL(tk_smallsel_kernel<true>, dim3(1), dim3(TK_SMALLSEL_THREADS), 0, h->stream, j.mode, j.sel, (int)j.n, (int)j.k, j.eig,
                           j.obj, j.ws, h->d_sel_key.get(), h->d_sel_idx.get(), j.base, j.score_add, j.d_idx_out, j.d_score_out);
    else if (p.route == TK_ROUTE_SMALLSEL)
        hipLaunchKernelGGL(tk_smallsel_kernel<false>, dim3(1), dim3(TK_SMALLSEL_THREADS), 0, h->stream, j.mode, j.sel, (int)j.n, (int)j.k, j.eig,
                           j.obj, j.ws, h->d_sel_key.get(), h->d_sel_idx.get(), j.base, j.score_add, j.d_idx_out, j.d_score_out);
    else
        hipLaunchKernelGGL(tk_small_kernel, dim3(1), dim3(TK_SMALL_THREADS), 0, h->stream, j.mode, j.sel, j.n, j.k, j.eig, j.obj, j.ws,
                           h->d_sel_key.get(), h->d_sel_idx.get());
}
