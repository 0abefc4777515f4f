// Top-k selection, the compaction of the launch-per-digit route (TK_ROUTE_DIGITS, topk_route.h) behind the seven launches of
// tk_hist_kernel (topk_passes.hip): the threshold is known, two launches without atomics on memory.

#include "topk_launch.h"

// threshold known: per block (contiguous chunk of the index space) count the keys above it and
// the keys equal to it -- no global atomics, the write pass derives its offsets from these
__global__ __launch_bounds__(TK_THREADS) void tk_count_kernel(int64_t n, int64_t chunk, const uint64_t *keys, TopkWs *ws)
{
    __shared__ uint32_t c_gt, c_eq;
    if (threadIdx.x == 0) { c_gt = 0; c_eq = 0; }
    __syncthreads();
    const TkState st = ws->state[8];
    if (st.need < 1) return;
    const uint64_t T = st.prefix;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    uint32_t my_gt = 0, my_eq = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += TK_THREADS) {
        const uint64_t key = keys[i];
        my_gt += (key > T);
        my_eq += (key == T);
    }
    if (my_gt) atomicAdd(&c_gt, my_gt);
    if (my_eq) atomicAdd(&c_eq, my_eq);
    __syncthreads();
    if (threadIdx.x == 0) { ws->blk_gt[blockIdx.x] = c_gt; ws->blk_eq[blockIdx.x] = c_eq; }
}

// write pass: keys above the threshold go to slots [0, greater) (order inside a block is free,
// the final sort fixes it); of the keys equal to it the `need` lowest indices follow
__global__ __launch_bounds__(TK_THREADS) void tk_write_kernel(int64_t n, int64_t chunk, const uint64_t *keys, TopkWs *ws,
                                                              uint64_t *sel_key, uint32_t *sel_idx)
{
    __shared__ uint32_t red_gt[TK_THREADS], red_eq[TK_THREADS], all_gt[TK_THREADS], all_eq[TK_THREADS];
    __shared__ uint32_t wave_cnt[TK_THREADS / 64];
    __shared__ uint32_t gt_local;
    const TkState st = ws->state[8];
    if (st.need < 1) return;
    const uint64_t T = st.prefix;
    uint32_t pg = 0, pe = 0, tg = 0, te = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += TK_THREADS) {
        const uint32_t g = ws->blk_gt[b], e = ws->blk_eq[b];
        tg += g; te += e;
        if (b < (int)blockIdx.x) { pg += g; pe += e; }
    }
    red_gt[threadIdx.x] = pg;
    red_eq[threadIdx.x] = pe;
    all_gt[threadIdx.x] = tg;
    all_eq[threadIdx.x] = te;
    if (threadIdx.x == 0) gt_local = 0;
    __syncthreads();
    for (int off = TK_THREADS / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            red_gt[threadIdx.x] += red_gt[threadIdx.x + off]; red_eq[threadIdx.x] += red_eq[threadIdx.x + off];
            all_gt[threadIdx.x] += all_gt[threadIdx.x + off]; all_eq[threadIdx.x] += all_eq[threadIdx.x + off];
        }
        __syncthreads();
    }
    const int64_t base_gt = red_gt[0];
    int64_t base_eq = red_eq[0];
    const int64_t greater = all_gt[0];                 // keys above the threshold, over all blocks
    if (blockIdx.x == 0 && threadIdx.x == 0) ws->n_sel = greater + (st.need < (int64_t)all_eq[0] ? st.need : (int64_t)all_eq[0]);
    const bool want_gt = ws->blk_gt[blockIdx.x] != 0;
    const bool want_eq = ws->blk_eq[blockIdx.x] != 0 && base_eq < st.need;
    if (!want_gt && !want_eq) return;     // uniform
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = lo; row < hi; row += TK_THREADS) {
        const int64_t i = row + threadIdx.x;
        const uint64_t key = (i < hi) ? keys[i] : 0ull;
        if (i < hi && key > T) {
            const int64_t slot = base_gt + atomicAdd(&gt_local, 1u);
            sel_key[slot] = key;
            sel_idx[slot] = (uint32_t)i;
        }
        if (want_eq) {     // uniform
            const bool is_eq = (i < hi) && (key == T);
            const unsigned long long m = __ballot(is_eq);
            if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            uint32_t row_total = 0;
            for (int w = 0; w < TK_THREADS / 64; ++w) {
                if (w < wave) before += wave_cnt[w];
                row_total += wave_cnt[w];
            }
            const int64_t rank = base_eq + before;
            if (is_eq && rank < st.need) {
                sel_key[greater + rank] = T;
                sel_idx[greater + rank] = (uint32_t)i;
            }
            base_eq += row_total;
            __syncthreads();
        }
    }
}

void tk_compact_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    const dim3 grid(p.grid_pass), blk(TK_THREADS);
    hipLaunchKernelGGL(tk_count_kernel, grid, blk, 0, h->stream, j.n, p.chunk, h->d_key_a.get(), j.ws);
    hipLaunchKernelGGL(tk_write_kernel, grid, blk, 0, h->stream, j.n, p.chunk, h->d_key_a.get(), j.ws, h->d_sel_key.get(), h->d_sel_idx.get());
}
