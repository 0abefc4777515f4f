// Top-k selection, the histogram passes: every kernel that resolves a radix digit through finish_pass / resolve_digit
// (topk_dev.h).  tk_keys_kernel builds the keys and counts the leading digit, tk_prekeys_kernel does the same over keys that exist
// already; then either ONE launch of tk_refine_kernel does everything up to the sort (TK_ROUTE_ONFLY / COOP / FUSED, topk_route.h)
// or tk_hist_kernel runs once per remaining digit (TK_ROUTE_DIGITS: no wait inside any kernel, the route that always answers;
// its compaction is topk_compact.hip).

#include "topk_launch.h"

// pass 0: build the keys, histogram of digit 7, class / violated / positive counts
__global__ __launch_bounds__(TK_THREADS) void tk_keys_kernel(int mode, int64_t sel, int64_t n, int64_t k, const double *eig,
                                                             const double *obj, uint64_t *keys, TopkWs *ws)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t cnt[3];
    mode = resolve_mode(mode, ws, sel);      // uniform over the grid: counters[5] is final before this launch
    hist[threadIdx.x] = 0;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t c_class = 0, c_viol = 0, c_pos = 0;
    const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
    const int64_t rounds = (n + stride - 1) / stride;
    // TK_UNROLL rounds at a time with all loads issued first: a thread only has ~8 rounds, and one
    // dependent HBM round trip per round (~2 us) was the whole cost of the pass
    for (int64_t r0 = 0; r0 < rounds; r0 += TK_UNROLL) {
        double e[TK_UNROLL], o[TK_UNROLL];
        int64_t idx[TK_UNROLL];
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            idx[u] = (r0 + u) * stride + (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
            const bool in = idx[u] < n;
            e[u] = (in && eig) ? eig[idx[u]] : 0.0;
            o[u] = (in && obj) ? obj[idx[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            const bool in = idx[u] < n;
            uint64_t key = 0;
            if (in) {
                key = masked_key(mode, e[u], o[u]);
                keys[idx[u]] = key;
                c_class += (mode == TK_MODE_OPT || mode == TK_MODE_COMBALL) ? 1u : (key != 0ull);
                c_viol += (eig != nullptr) && (e[u] < SDPCUT_NEG_EIGVAL);
                c_pos += (obj != nullptr) && (o[u] > 0.0);
            }
            hist_add(hist, (uint32_t)(key >> 56), in);
        }
    }
    if (c_class) atomicAdd(&cnt[0], c_class);
    if (c_viol) atomicAdd(&cnt[1], c_viol);
    if (c_pos) atomicAdd(&cnt[2], c_pos);
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x])
        atomicAdd((unsigned long long *)&ws->counters[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st_i64(&ws->mode, mode);
        st_i64(&ws->counters[6], mode);
        st_i64(&ws->counters[5], strong_total(ws));      // for the host (round header)
    }
    finish_pass(ws, 0, k, hist, gridDim.x);
}

// pass p = 1..7: histogram of digit 7-p among the keys that match the prefix resolved so far
__global__ __launch_bounds__(TK_THREADS) void tk_hist_kernel(int p, int64_t n, int64_t k, const uint64_t *keys, TopkWs *ws)
{
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const TkState st = ws->state[p];
    if (st.stop) return;                              // uniform: selection already closed
    if (st.need >= 1) {                               // uniform
        const int shift = 8 * (7 - p);
        const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
        const int64_t rounds = (n + stride - 1) / stride;
        for (int64_t r0 = 0; r0 < rounds; r0 += TK_UNROLL) {
            uint64_t key[TK_UNROLL];
            bool in[TK_UNROLL];
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u) {
                const int64_t i = (r0 + u) * stride + (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
                in[u] = i < n;
                key[u] = in[u] ? keys[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u) {
                const bool match = in[u] && (((key[u] ^ st.prefix) >> (shift + 8)) == 0);
                hist_add(hist, (uint32_t)((key[u] >> shift) & 255), match);
            }
        }
        __syncthreads();
    }
    finish_pass(ws, p, k, hist, gridDim.x);
}

// bounded waits of the fused selection kernel (tk_refine_kernel): x s_sleep, a few milliseconds; a legitimate wait is
// tens of microseconds.  When a flag does not come (the GPU shared with a kernel that keeps workgroups of the grid from
// starting) counters[4] is raised, every workgroup leaves, and the host answers through a path without waits.
#define TK_SPIN_LIMIT (1 << 16)

// One-shot grid barrier `b` of a selection (its arrival counter starts at zero with the workspace).
// Every thread's device-scope atomics are drained before the workgroup arrives.  Bounded like the
// wait for a published state: if the other workgroups do not show up (the GPU shared with a kernel
// that keeps them from starting) counters[4] marks the selection void and everybody leaves.
static __device__ bool grid_barrier(TopkWs *ws, int b, uint32_t nblocks)
{
    __shared__ int bar_ok;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(&ws->bar[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int ok = 1;
        uint32_t it = 0;
        while (ld_u32(&ws->bar[b]) < nblocks) {
            __builtin_amdgcn_s_sleep(4);
            const int64_t gone = ld_i64(&ws->counters[4]);      // 2: the selection has declared itself void (tie group): leave, keep the 2
            if (++it > TK_SPIN_LIMIT || gone) {
                if (!gone) st_i64(&ws->counters[4], 1);
                ok = 0;
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        bar_ok = ok;
    }
    __syncthreads();
    return bar_ok != 0;
}

// Passes 1..7, the count and the compaction in ONE launch (the fast path's replacement of
// tk_hist_kernel (x7) + tk_count_kernel + tk_write_kernel: launch hand-offs
// of ~5 us each become one or two grid barriers).  After pass 1 the selection is normally closed
// (early stop: every key >= T, at most TK_MAXK of them, in any order -- the sort that follows orders
// them): each workgroup counts its keys >= T, reserves its slice of the output with ONE fetch-add and
// writes.  Masses of equal keys run the remaining digits behind grid barriers and cut the last group by
// index, which needs the per-workgroup counts of all workgroups: one more barrier.
//
// ONFLY: the score kernels have already counted the leading digit (ScoreArgs::tk -> TopkWs::hist_score) and
// there is no key array: every workgroup resolves pass 0 for itself (same inputs, same result), and the
// keys are built from the scores as they are read -- once, into the LDS cache, when the chunk fits.
// Mode COMBAUTO resolved to COMBALL (fewer strong candidates than asked for -- the score kernels
// counted the STRONG keys): this launch runs its own pass 0 first, histogram in TopkWs::hist_alt.
// (r5) DIRECT: the score / eigenvalue kernels also left the FINE histogram of the class (TopkWs::pf_tab, topk_dev.h).  Every
// workgroup resolves from it the window bin e* that holds the k-th largest key; if e* lies at or above the floor the producers
// published and the members at or above e* fit the sort buffers -- the usual case: 5000 .. 5100 of 10^6 -- they are compacted in
// ONE pass over the scores and handed to the sort exactly like an early stop of the digit passes: no histogram pass, no grid
// barrier, no wait.  pf_k = 0, a workgroup rich in head members, a fat bin, or the every-entry-visited regime: the passes below
// run as before.
// EMIT (with ONFLY; TK_ROUTE_EMITTED): the skipping score launch of this round appended every strong candidate -- selection key and
// index -- to a list of at most emit_cap pairs of 64-bit words in `keys`; TopkWs::emit_n counts them, emit_over says that
// some did not fit.  What only the device knows decides first: mode COMBAUTO resolved to STRONG, no overflow, the count equal to
// the strong count.  Then the strong class IS the list: workgroup b takes entries 1024 b .. 1024 b + 1023 (and every gridDim.x-th
// block of 1024 behind), the others leave (at once if the class fits the sort buffers, else once the table says that its threshold serves), and nobody
// reads a score.  The threshold is the direct one of the fine
// histogram; without one (pf_k = 0, e* below the floor, a fat bin) a class that fits the sort buffers is taken whole, which is what
// resolve_digit would close digit 0 with.  The list's order is not deterministic and nothing depends on it: the compacted superset is
// handed to the sort in whatever order the slices are reserved, as on the direct path.  In every other case -- the other regime, an
// overflow, a class beyond the sort buffers without a direct threshold -- the scores of the first batch are requested late, once
// that is known, and the launch is TK_ROUTE_ONFLY's from there on.
#define TK_EMIT_PER (4 * TK_THREADS)
template <bool ONFLY, bool EMIT = false>
__global__ __launch_bounds__(TK_THREADS) void tk_refine_kernel(int64_t n, int64_t k, int64_t chunk, const uint64_t *keys,
                                                               TopkWs *ws, uint64_t *sel_key, uint32_t *sel_idx, int mode,
                                                               int64_t sel, const double *eig, const double *obj, int64_t pf_k,
                                                               unsigned long long *d_stats, int64_t emit_cap)
{
    static_assert(!EMIT || ONFLY, "the emitted list belongs to a selection that starts from the score launch's histograms");
    __shared__ uint32_t hist[256];
    __shared__ int go;
    __shared__ uint32_t red_gt[TK_THREADS], red_eq[TK_THREADS], all_gt[TK_THREADS], all_eq[TK_THREADS];
    __shared__ uint32_t wave_cnt[TK_THREADS / 64];
    __shared__ uint32_t c_gt, c_eq, gt_local, c_above;
    __shared__ unsigned long long slice;
    __shared__ uint64_t cache[TK_CACHE];
    __shared__ TkState st1;                         // ONFLY: state after pass 0, resolved by this workgroup
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    const bool use_cache = chunk <= TK_CACHE;      // uniform: the chunk is read from memory once
    bool cached = false;
    int last_pass = -1;                             // last digit pass this launch ran (its histogram is still in LDS)
    int p_first = 1;
    bool direct = false;                            // (r5) resolved from the fine table: uniform over the grid
    __shared__ int pf_e, pf_floor_f;
    __shared__ int64_t pf_count;
    if (threadIdx.x == 0) c_above = 0;
    auto key_at = [&](int64_t i) -> uint64_t {
        if constexpr (ONFLY) return masked_key(mode, eig[i], obj[i]);     // (both valid: see the launch)
        else return keys[i];
    };
    // ONFLY: the scores of the first batch are requested before digit 0 is resolved (they do not depend on it)
    double pre_e[TK_UNROLL], pre_o[TK_UNROLL], pre_e2[TK_UNROLL], pre_o2[TK_UNROLL];
    uint32_t pf_q[2 * (PF_BINS / 1024)][4];      // (r5) this thread's words of the fine table, both replicas, and of the floor
    uint32_t pf_fl = 0;
    [[maybe_unused]] int list_mode = 0;             // (EMIT) 1: the list's entries at or above the direct threshold; 2: all of them
    [[maybe_unused]] uint32_t emit_n = 0;
    if constexpr (ONFLY) {
        if (pf_k > 0) {      // uniform; coalesced 16-byte loads, independent of everything else the kernel reads
            static_assert(PF_REP == 2 && PF_BINS % 1024 == 0, "two replicas of 1024-word blocks");
#pragma unroll
            for (int r = 0; r < PF_REP; ++r)
#pragma unroll
                for (int i = 0; i < PF_BINS / 1024; ++i) {
                    const uint4 q = *(const uint4 *)&ws->pf_tab[r][1024 * i + 4 * threadIdx.x];
                    pf_q[r * (PF_BINS / 1024) + i][0] = q.x; pf_q[r * (PF_BINS / 1024) + i][1] = q.y;
                    pf_q[r * (PF_BINS / 1024) + i][2] = q.z; pf_q[r * (PF_BINS / 1024) + i][3] = q.w;
                }
            if ((threadIdx.x & 63) < PF_FLOOR_REP) pf_fl = ws->pf_floor[threadIdx.x & 63][0];
        }
        auto issue_pre = [&]() __attribute__((always_inline)) {
        if (lo < hi) {
            // (r5) only the measure the mode ranks by: a feasibility / optimality selection reads 8 bytes per candidate, not 16 -- the
            // scan of the scores is what this kernel waits for longest (phase stamps: table 3.2 us, scores 3.5-4.3 more)
            const double *m0 = mode == TK_MODE_OPT ? obj : eig;
            const bool two = mode != TK_MODE_OPT && mode != TK_MODE_FEAS;      // uniform
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u) {
                const int64_t i = lo + (int64_t)u * TK_THREADS + threadIdx.x;
                const int64_t ic = i < hi ? i : hi - 1;
                pre_e[u] = m0[ic];
            }
            if (two) {
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) {
                    const int64_t i = lo + (int64_t)u * TK_THREADS + threadIdx.x;
                    const int64_t ic = i < hi ? i : hi - 1;
                    pre_o[u] = obj[ic];
                }
            } else {
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) pre_o[u] = pre_e[u];      // (masked_key looks at one of the two)
            }
            if (pf_k > 0 && use_cache) {      // uniform: the direct path reads its whole chunk (<= 4096 scores) without a second round trip
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) {
                    const int64_t i = lo + (int64_t)(TK_UNROLL + u) * TK_THREADS + threadIdx.x;
                    const int64_t ic = i < hi ? i : hi - 1;
                    pre_e2[u] = m0[ic];
                }
                if (two) {
#pragma unroll
                    for (int u = 0; u < TK_UNROLL; ++u) {
                        const int64_t i = lo + (int64_t)(TK_UNROLL + u) * TK_THREADS + threadIdx.x;
                        const int64_t ic = i < hi ? i : hi - 1;
                        pre_o2[u] = obj[ic];
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < TK_UNROLL; ++u) pre_o2[u] = pre_e2[u];
                }
            }
        }
        };
        if constexpr (!EMIT) issue_pre();
        const bool both = mode == TK_MODE_COMBAUTO;
        // (everything read here was written by earlier launches: plain loads)
        int64_t strong = 0;
#pragma unroll
        for (int r = 0; r < TK_SREP; ++r) strong += ws->strong_rep[r];
        if (both) mode = strong >= sel ? TK_MODE_STRONG : TK_MODE_COMBALL;      // uniform over the grid
        [[maybe_unused]] bool use_list = false;     // uniform over the grid
        if constexpr (EMIT) {
            emit_n = ws->emit_n;
            // a class that fits the sort buffers is served from the list whatever the fine histogram says; a larger one needs the
            // direct threshold, which exists only where the table was counted (pf_k > 0) and is known only once it is resolved
            const bool fits = (int64_t)emit_n <= (k <= TK_LDSK ? TK_LDSK : TK_MAXK);
            use_list = both && mode == TK_MODE_STRONG && ws->emit_over == 0u && (int64_t)emit_n == strong && (int64_t)emit_n <= emit_cap &&
                       (fits || pf_k > 0);
            if (!use_list) issue_pre();
            // no entry of the list is this workgroup's, and the list is certain to serve: leave.  (A larger class keeps every
            // workgroup until the table is resolved: without a direct threshold all of them scan their chunks of the scores.)
            else if (fits && blockIdx.x != 0 && (int64_t)blockIdx.x * TK_EMIT_PER >= (int64_t)emit_n) return;
        }
        int64_t nviol = 0, npos = 0;      // counted by the score / eigenvalue kernels, replicated by workgroup
#pragma unroll 4
        for (int r = 0; r < TK_SHREP; ++r) { nviol += ws->viol_rep[r]; npos += ws->pos_rep[r]; }
        const int64_t cls = (mode == TK_MODE_OPT || mode == TK_MODE_COMBALL) ? n
                            : (mode == TK_MODE_FEAS) ? nviol : strong;
        if (threadIdx.x == 0 && blockIdx.x == 0) {
            st_i64(&ws->counters[1], nviol);
            st_i64(&ws->counters[2], npos);
            st_i64(&ws->mode, mode);
            st_i64(&ws->counters[6], mode);
            st_i64(&ws->counters[5], strong);      // for the host (round header)
            st_i64(&ws->counters[0], cls);
            if (d_stats) {      // SDPCUT_STAT_NN_EVALUATED of a filtering launch: what its waves passed on to the fp64 pass
                int64_t neval = 0;
                for (int r = 0; r < TK_SHREP; ++r) neval += ws->eval_rep[r];
                d_stats[5] = (unsigned long long)neval;
            }
        }
        if (both && mode == TK_MODE_COMBALL) {      // uniform over the grid
            p_first = 0;
            if (threadIdx.x == 0) { st1.prefix = 0; st1.need = k < cls ? k : cls; st1.stop = 0; }
        } else {
            if (pf_k > 0 && mode != TK_MODE_COMBALL) {
                // ---- the fine table (requested at the top of the kernel, in memory order: two replicas x 2048 words, consecutive
                // bins in consecutive lines) goes through LDS into bin order -- the key cache is not in use yet --; thread t then owns
                // bins 8 t .. 8 t + 7, suffix sums from the top.
                __shared__ uint32_t pf_wtot[TK_THREADS / 64];
                uint32_t *nat = (uint32_t *)cache;
                const int t = threadIdx.x, ln = t & 63, wv = t >> 6;
#pragma unroll
                for (int i = 0; i < PF_BINS / 1024; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int w = 1024 * i + 4 * t + j;      // word of a replica: bin (w % 32) * 64 + w / 32
                        nat[(w & 31) * 64 + (w >> 5)] = pf_q[i][j] + pf_q[PF_BINS / 1024 + i][j];
                    }
                uint32_t fl = pf_fl;
                for (int off = 8; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)fl, off); fl = o > fl ? o : fl; }
                if (t == 0) { pf_e = -1; pf_count = 0; pf_floor_f = (int)fl; }
                __syncthreads();
                constexpr int PER = PF_BINS / TK_THREADS;      // 8
                uint32_t hf[PER], mine8 = 0;
#pragma unroll
                for (int j = 0; j < PER; ++j) { hf[j] = nat[PER * t + j]; mine8 += hf[j]; }
                uint32_t v = mine8;
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_down((int)v, off);
                    if (ln + off < 64) v += o;
                }
                if (ln == 0) pf_wtot[wv] = v;
                __syncthreads();
                for (int w = wv + 1; w < TK_THREADS / 64; ++w) v += pf_wtot[w];
                const int64_t need = k < cls ? k : cls;
                int64_t above = (int64_t)(v - mine8);
#pragma unroll
                for (int j = PER - 1; j >= 0; --j) {
                    const int64_t here = above + (int64_t)hf[j];
                    if (need >= 1 && here >= need && above < need) { pf_e = PER * t + j; pf_count = here; }      // one bin of one thread
                    above = here;
                }
                __syncthreads();
                const int64_t maxk = k <= TK_LDSK ? TK_LDSK : TK_MAXK;
                // e* at or above the floor: every workgroup reported every bin from e* up, the counts there are exact and the members
                // there are all of the class's members with such keys.  (Below the floor some workgroup kept members to itself: the
                // table undercounts, e* would lie too low -- never trusted.)
                direct = pf_e >= 0 && pf_e >= pf_floor_f && pf_count <= maxk;
                if (d_stats && blockIdx.x == 0 && threadIdx.x == 0) {      // what the last selection saw (sdpcut_get_stat, diagnostics)
                    d_stats[1] = (unsigned long long)(long long)pf_e;
                    d_stats[2] = (unsigned long long)(long long)pf_floor_f;
                    d_stats[3] = (unsigned long long)pf_count;
                }
                if (direct) {
                    const bool all_members = mode == TK_MODE_OPT;
                    const uint64_t edge = pf_edge(pf_e, mode == TK_MODE_FEAS);
                    if (threadIdx.x == 0) {
                        st1.prefix = edge > 0ull || all_members ? edge : 1ull;      // (key 0 = not in the class)
                        st1.need = 1;
                        st1.stop = 1;
                        if (blockIdx.x == 0) {
                            st_i64(&ws->counters[3], need);      // k_eff for the sort
                            if (d_stats) atomicAdd(&d_stats[0], 1ull);
                        }
                    }
                }
            }
            if (!direct) resolve_digit(ws, 0, k, ws->hist_score, cls, &st1, blockIdx.x == 0, mode, true, TK_SHREP);
            if constexpr (EMIT) {
                if (use_list) {
                    if (direct) list_mode = 1;
                    else if ((int64_t)emit_n <= (k <= TK_LDSK ? TK_LDSK : TK_MAXK)) list_mode = 2;
                    else issue_pre();      // a class beyond the sort buffers and no direct threshold: the passes below scan the scores
                }
            }
        }
        __syncthreads();
    }
    if constexpr (EMIT) {
        if (list_mode) {      // uniform over the workgroups that are still here
            const uint64_t T0 = list_mode == 1 ? st1.prefix : 1ull;      // (key 0 = not in the class; the list holds members only)
            const ulonglong2 *elist = (const ulonglong2 *)keys;
            const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
            for (int64_t base = (int64_t)blockIdx.x * TK_EMIT_PER; base < (int64_t)emit_n; base += (int64_t)gridDim.x * TK_EMIT_PER) {
                uint64_t ek[TK_EMIT_PER / TK_THREADS];
                uint32_t ei[TK_EMIT_PER / TK_THREADS], mask = 0;
#pragma unroll
                for (int u = 0; u < TK_EMIT_PER / TK_THREADS; ++u) {
                    const int64_t i = base + (int64_t)u * TK_THREADS + threadIdx.x;
                    const int64_t ic = i < (int64_t)emit_n ? i : (int64_t)emit_n - 1;
                    const ulonglong2 e = elist[ic];
                    ek[u] = e.x;
                    ei[u] = (uint32_t)e.y;
                }
#pragma unroll
                for (int u = 0; u < TK_EMIT_PER / TK_THREADS; ++u)
                    mask |= (uint32_t)(base + (int64_t)u * TK_THREADS + threadIdx.x < (int64_t)emit_n && ek[u] >= T0) << u;
                const uint32_t cnt = (uint32_t)__popc(mask);
                uint32_t incl = cnt;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
                    if (ln >= off) incl += o;
                }
                if (ln == 63) wave_cnt[wv] = incl;
                __syncthreads();
                uint32_t wbase = 0, total = 0;
#pragma unroll
                for (int w = 0; w < TK_THREADS / 64; ++w) {
                    if (w < wv) wbase += wave_cnt[w];
                    total += wave_cnt[w];
                }
                if (threadIdx.x == 0 && total)
                    slice = __hip_atomic_fetch_add((unsigned long long *)&ws->n_sel, (unsigned long long)total, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                __syncthreads();
                int64_t slot = (int64_t)slice + wbase + incl - cnt;
#pragma unroll
                for (int u = 0; u < TK_EMIT_PER / TK_THREADS; ++u) {
                    if ((mask >> u) & 1u) {
                        if (slot < (int64_t)TK_MAXK) {
                            sel_key[slot] = ek[u];
                            sel_idx[slot] = ei[u];
                        } else {
                            st_i64(&ws->counters[4], 1);      // cannot happen (see the direct path below): the selection is void
                        }
                        ++slot;
                    }
                }
                __syncthreads();      // wave_cnt and slice are rewritten by the next round
            }
            if (d_stats && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&d_stats[6], 1ull);
            return;
        }
    }
    TkState st;
    if constexpr (ONFLY) {
        if (direct && use_cache) {      // uniform over the grid
            // ---- (r5) the whole chunk is the two batches requested at the top of the kernel: keys and membership stay in registers,
            // ONE scan over the workgroup gives every thread its offset and the workgroup its count, one returning atomic reserves the
            // slice, the members are written.  (The general path below counts, reserves, then re-reads its keys row by row with an
            // LDS atomic per row: 16 dependent LDS round trips, 2.5 us of this kernel's 15 by its phase stamps.)
            const uint64_t T0 = st1.prefix;
            const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
            uint64_t dk[2 * TK_UNROLL];
            uint32_t mask = 0;
#pragma unroll
            for (int u = 0; u < 2 * TK_UNROLL; ++u) {
                const int64_t i = lo + (int64_t)u * TK_THREADS + threadIdx.x;
                const bool in = i < hi;
                dk[u] = in ? masked_key(mode, u < TK_UNROLL ? pre_e[u % TK_UNROLL] : pre_e2[u % TK_UNROLL],
                                        u < TK_UNROLL ? pre_o[u % TK_UNROLL] : pre_o2[u % TK_UNROLL]) : 0ull;
                mask |= (uint32_t)(in && dk[u] >= T0) << u;
            }
            const uint32_t cnt = (uint32_t)__popc(mask);
            uint32_t incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
                if (ln >= off) incl += o;
            }
            if (ln == 63) wave_cnt[wv] = incl;
            __syncthreads();
            uint32_t wbase = 0, total = 0;
#pragma unroll
            for (int w = 0; w < TK_THREADS / 64; ++w) {
                if (w < wv) wbase += wave_cnt[w];
                total += wave_cnt[w];
            }
            if (total == 0) return;      // uniform per workgroup
            if (threadIdx.x == 0)
                slice = __hip_atomic_fetch_add((unsigned long long *)&ws->n_sel, (unsigned long long)total, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            int64_t slot = (int64_t)slice + wbase + incl - cnt;
#pragma unroll
            for (int u = 0; u < 2 * TK_UNROLL; ++u) {
                if ((mask >> u) & 1u) {
                    if (slot < (int64_t)TK_MAXK) {
                        sel_key[slot] = dk[u];
                        sel_idx[slot] = (uint32_t)(lo + (int64_t)u * TK_THREADS + threadIdx.x);
                    } else {
                        st_i64(&ws->counters[4], 1);      // cannot happen (the table is exact from e* up): the selection is void, the host's general path answers
                    }
                    ++slot;
                }
            }
            return;
        }
    }
    if (direct) {
        // ---- one pass: the keys of this chunk (into the LDS cache when they fit), how many of them lie at or above the edge
        st = st1;
        const uint64_t T0 = st.prefix;
        uint32_t my = 0;
        if (threadIdx.x == 0) c_gt = 0;
        __syncthreads();
        if constexpr (ONFLY) {
            for (int64_t r0 = lo; r0 < hi; r0 += (int64_t)TK_UNROLL * TK_THREADS) {
                double e[TK_UNROLL], o[TK_UNROLL];
                bool in[TK_UNROLL];
                if (r0 == lo) {      // uniform: the batch requested at the top of the kernel
#pragma unroll
                    for (int u = 0; u < TK_UNROLL; ++u) {
                        in[u] = lo + (int64_t)u * TK_THREADS + threadIdx.x < hi;
                        e[u] = pre_e[u];
                        o[u] = pre_o[u];
                    }
                } else if (use_cache && r0 == lo + (int64_t)TK_UNROLL * TK_THREADS) {      // uniform: the second batch, requested there as well
#pragma unroll
                    for (int u = 0; u < TK_UNROLL; ++u) {
                        in[u] = r0 + (int64_t)u * TK_THREADS + threadIdx.x < hi;
                        e[u] = pre_e2[u];
                        o[u] = pre_o2[u];
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < TK_UNROLL; ++u) {
                        const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                        in[u] = i < hi;
                        const int64_t ic = in[u] ? i : hi - 1;
                        e[u] = eig[ic];
                        o[u] = obj[ic];
                    }
                }
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) {
                    const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                    const uint64_t key = in[u] ? masked_key(mode, e[u], o[u]) : 0ull;
                    if (use_cache && in[u]) cache[i - lo] = key;
                    my += in[u] && key >= T0;
                }
            }
        }
        cached = use_cache;
        for (int off = 32; off > 0; off >>= 1) my += __shfl_xor((int)my, off);
        if ((threadIdx.x & 63) == 0 && my) atomicAdd(&c_gt, my);
        __syncthreads();
    }
    for (int p = p_first; !direct; ++p) {
        if (p > p_first) {        // state[p] is published inside this launch
            if (threadIdx.x == 0) {
                int ok = 1;
                uint32_t it = 0;
                while (ld_u32(&ws->ready[p]) == 0u) {
                    __builtin_amdgcn_s_sleep(4);
                    const int64_t gone = ld_i64(&ws->counters[4]);
                    if (++it > TK_SPIN_LIMIT || gone) {
                        if (!gone) st_i64(&ws->counters[4], 1);
                        ok = 0;
                        break;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // pairs with the release in front of the flag (finish_pass)
                go = ok;
            }
            __syncthreads();
            if (!go) return;
        }
        if (ONFLY && p == p_first) {
            st = st1;
        } else {
            st.prefix = (uint64_t)ld_i64((const int64_t *)&ws->state[p].prefix);
            st.need = ld_i64(&ws->state[p].need);
            st.stop = ld_i64(&ws->state[p].stop);
        }
        if (st.stop || st.need < 1 || p == 8) break;      // uniform over the grid
        hist[threadIdx.x] = 0;
        if (threadIdx.x == 0) c_above = 0;
        __syncthreads();
        const int shift = 8 * (7 - p);
        uint32_t above = 0;                               // keys of this chunk beyond the prefix' range
        for (int64_t r0 = lo; r0 < hi; r0 += (int64_t)TK_UNROLL * TK_THREADS) {
            uint64_t key[TK_UNROLL];
            bool in[TK_UNROLL];
            if (ONFLY && !cached) {      // uniform
                // all 2 x TK_UNROLL score loads are issued before the first key is built (unconditional,
                // from a clamped position: a load inside a branch is waited for on the spot)
                double e[TK_UNROLL], o[TK_UNROLL];
                if (r0 == lo) {      // uniform: the batch requested at the top of the kernel
#pragma unroll
                    for (int u = 0; u < TK_UNROLL; ++u) {
                        in[u] = lo + (int64_t)u * TK_THREADS + threadIdx.x < hi;
                        e[u] = pre_e[u];
                        o[u] = pre_o[u];
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < TK_UNROLL; ++u) {
                        const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                        in[u] = i < hi;
                        const int64_t ic = in[u] ? i : hi - 1;
                        e[u] = eig[ic];
                        o[u] = obj[ic];
                    }
                }
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) key[u] = in[u] ? masked_key(mode, e[u], o[u]) : 0ull;
            } else {
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) {
                    const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                    in[u] = i < hi;
                    key[u] = !in[u] ? 0ull : (cached ? cache[i - lo] : keys[i]);
                }
            }
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u) {
                const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                if (use_cache && !cached && in[u]) cache[i - lo] = key[u];
                const uint64_t hi_part = p ? key[u] >> (shift + 8) : 0ull, pre_part = p ? st.prefix >> (shift + 8) : 0ull;
                const bool match = in[u] && hi_part == pre_part;
                above += in[u] && hi_part > pre_part;
                hist_add(hist, (uint32_t)((key[u] >> shift) & 255), match);
            }
        }
        cached = use_cache;
        for (int off = 32; off > 0; off >>= 1) above += __shfl_xor((int)above, off);
        if ((threadIdx.x & 63) == 0 && above) atomicAdd(&c_above, above);
        __syncthreads();
        last_pass = p;
        finish_pass(ws, p, k, hist, gridDim.x, true, p ? nullptr : ws->hist_alt);
        __syncthreads();
    }
    if (st.need < 1) return;                               // empty class: n_sel stays 0
    const uint64_t T = st.prefix;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (st.stop) {
        // early stop: every key >= T is wanted, in any order (the sort that follows orders them)
        uint32_t mine;
        if (last_pass >= 0) {
            // closed by the pass just run: this chunk's count is in its own histogram -- the keys beyond
            // the prefix' range plus the bins from the threshold bin up -- no counting pass over the keys
            const int shift = 8 * (7 - last_pass);
            const uint32_t tbin = (uint32_t)((T >> shift) & 255);
            uint32_t part = (threadIdx.x >= tbin) ? hist[threadIdx.x] : 0u;
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor((int)part, off);
            if (threadIdx.x == 0) c_gt = 0;
            __syncthreads();
            if (lane == 0 && part) atomicAdd(&c_gt, part);
            __syncthreads();
            mine = c_gt + c_above;
        } else if (direct) {
            mine = c_gt;                                   // counted by the direct pass above
        } else {
            if (threadIdx.x == 0) c_gt = 0;
            __syncthreads();
            uint32_t my = 0;
            for (int64_t i = lo + threadIdx.x; i < hi; i += TK_THREADS) my += key_at(i) >= T;
            for (int off = 32; off > 0; off >>= 1) my += __shfl_xor((int)my, off);
            if (lane == 0 && my) atomicAdd(&c_gt, my);
            __syncthreads();
            mine = c_gt;
        }
        if (mine == 0) return;                             // uniform per workgroup
        if (threadIdx.x == 0) {
            gt_local = 0;
            slice = __hip_atomic_fetch_add((unsigned long long *)&ws->n_sel, (unsigned long long)mine, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int64_t base = (int64_t)slice;
        // (rows in batches of TK_UNROLL with all their loads issued first: a chunk that does not fit the LDS cache
        // -- 4.9e4 keys per workgroup on a 1.25e7-candidate shard -- would otherwise pay a trip to HBM per row)
        for (int64_t r0 = lo; r0 < hi; r0 += (int64_t)TK_UNROLL * TK_THREADS) {
            uint64_t kk[TK_UNROLL];
            if (ONFLY && !cached) {      // uniform
                double e[TK_UNROLL], o[TK_UNROLL];
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) {
                    const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                    const int64_t ic = i < hi ? i : hi - 1;
                    e[u] = eig[ic];
                    o[u] = obj[ic];
                }
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) kk[u] = masked_key(mode, e[u], o[u]);
            } else {
#pragma unroll
                for (int u = 0; u < TK_UNROLL; ++u) {
                    const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                    kk[u] = (i < hi) ? (cached ? cache[i - lo] : keys[i]) : 0ull;
                }
            }
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u) {
                const int64_t i = r0 + (int64_t)u * TK_THREADS + threadIdx.x;
                if (r0 + (int64_t)u * TK_THREADS >= hi) break;      // uniform
                const uint64_t key = kk[u];
                const bool take = (i < hi) && key >= T;
                const unsigned long long m = __ballot(take);
                uint32_t wbase = 0;
                if (lane == 0 && m) wbase = atomicAdd(&gt_local, (uint32_t)__popcll(m));
                wbase = (uint32_t)__shfl((int)wbase, 0);
                if (take) {
                    const int64_t slot = base + wbase + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    sel_key[slot] = key;
                    sel_idx[slot] = (uint32_t)i;
                }
            }
        }
        return;
    }
    // ---- counts of this workgroup's chunk
    if (threadIdx.x == 0) { c_gt = 0; c_eq = 0; gt_local = 0; }
    __syncthreads();
    {
        uint32_t my_gt = 0, my_eq = 0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += TK_THREADS) {
            const uint64_t key = cached ? cache[i - lo] : key_at(i);
            my_gt += (key > T);
            my_eq += (key == T);
        }
        for (int off = 32; off > 0; off >>= 1) {
            my_gt += __shfl_xor((int)my_gt, off);
            my_eq += __shfl_xor((int)my_eq, off);
        }
        if ((threadIdx.x & 63) == 0) {
            if (my_gt) atomicAdd(&c_gt, my_gt);
            if (my_eq) atomicAdd(&c_eq, my_eq);
        }
    }
    __syncthreads();
    // ---- exact cut at the last digit: offsets from the counts of ALL workgroups (tk_write_kernel's scheme)
    if (threadIdx.x == 0) {
        __hip_atomic_store(&ws->blk_gt[blockIdx.x], c_gt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ws->blk_eq[blockIdx.x], c_eq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!grid_barrier(ws, 0, gridDim.x)) return;
    uint32_t pg = 0, pe = 0, tg = 0, te = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += TK_THREADS) {
        const uint32_t g = ld_u32(&ws->blk_gt[b]), e = ld_u32(&ws->blk_eq[b]);
        tg += g; te += e;
        if (b < (int)blockIdx.x) { pg += g; pe += e; }
    }
    red_gt[threadIdx.x] = pg;
    red_eq[threadIdx.x] = pe;
    all_gt[threadIdx.x] = tg;
    all_eq[threadIdx.x] = te;
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
    const int64_t greater = all_gt[0];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        st_i64(&ws->n_sel, greater + (st.need < (int64_t)all_eq[0] ? st.need : (int64_t)all_eq[0]));
    const bool want_gt = c_gt != 0;
    const bool want_eq = c_eq != 0 && base_eq < st.need;
    if (!want_gt && !want_eq) return;     // uniform
    for (int64_t row = lo; row < hi; row += TK_THREADS) {
        const int64_t i = row + threadIdx.x;
        const uint64_t key = (i < hi) ? (cached ? cache[i - lo] : key_at(i)) : 0ull;
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

// pass 0 over keys that already exist (key 0 = not in the class): leading-digit histogram and class size
__global__ __launch_bounds__(TK_THREADS) void tk_prekeys_kernel(int64_t n, int64_t k, const uint64_t *keys, TopkWs *ws)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t cnt;
    hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    uint32_t c_class = 0;
    const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
    const int64_t rounds = (n + stride - 1) / stride;
    for (int64_t r = 0; r < rounds; ++r) {          // every lane runs every round: hist_add is wave-cooperative
        const int64_t i = r * stride + (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
        const bool in = i < n;
        const uint64_t key = in ? keys[i] : 0ull;
        c_class += in && key != 0ull;
        hist_add(hist, (uint32_t)(key >> 56), in);
    }
    if (c_class) atomicAdd(&cnt, c_class);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd((unsigned long long *)&ws->counters[0], (unsigned long long)cnt);
    if (blockIdx.x == 0 && threadIdx.x == 0) { st_i64(&ws->mode, TK_MODE_FEAS); st_i64(&ws->counters[6], TK_MODE_FEAS); }
    finish_pass(ws, 0, k, hist, gridDim.x);
}

void tk_keys_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    hipLaunchKernelGGL(tk_keys_kernel, dim3(p.grid_keys), dim3(TK_THREADS), 0, h->stream, j.mode, j.sel, j.n, j.k, j.eig, j.obj, h->d_key_a.get(), j.ws);
}

void tk_prekeys_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    hipLaunchKernelGGL(tk_prekeys_kernel, dim3(p.grid_keys), dim3(TK_THREADS), 0, h->stream, j.n, j.k, h->d_key_a.get(), j.ws);
}

// one launch per digit (each returns at once when the selection has been closed by an earlier digit)
void tk_hist_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    for (int d = 1; d < 8; ++d)
        hipLaunchKernelGGL(tk_hist_kernel, dim3(p.grid_pass), dim3(TK_THREADS), 0, h->stream, d, j.n, j.k, h->d_key_a.get(), j.ws);
}

// workgroups of the fused selection kernel the device holds at once (its grid barriers rely on it)
int tk_refine_coresident(sdpcut_ctx *h, int64_t *coresident)
{
    int b_on = 0, b_off = 0;
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&b_on, tk_refine_kernel<true>, TK_THREADS, 0));
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&b_off, tk_refine_kernel<false>, TK_THREADS, 0));
    int b_emit = 0;
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&b_emit, tk_refine_kernel<true, true>, TK_THREADS, 0));
    b_on = b_emit < b_on ? b_emit : b_on;
    *coresident = (int64_t)(b_on < b_off ? b_on : b_off) * h->n_cu;
    return 0;
}

int tk_refine_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    const dim3 grid(p.grid_pass), blk(TK_THREADS);
    if (p.route == TK_ROUTE_EMITTED) {      // the list the score launch emitted lies in the key array (launch_score_k)
        hipLaunchKernelGGL((tk_refine_kernel<true, true>), grid, blk, 0, h->stream, j.n, j.k, p.chunk, h->d_key_a.get(), j.ws, h->d_sel_key.get(),
                           h->d_sel_idx.get(), j.mode, j.sel, j.eig ? j.eig : j.obj, j.obj ? j.obj : j.eig, p.pf_k, h->d_stats.get(), h->emit_cap);
    } else if (p.route == TK_ROUTE_ONFLY) {      // (a measure the mode does not use is never looked at: any readable array of n doubles will do)
        hipLaunchKernelGGL(tk_refine_kernel<true>, grid, blk, 0, h->stream, j.n, j.k, p.chunk, nullptr, j.ws, h->d_sel_key.get(), h->d_sel_idx.get(),
                           j.mode, j.sel, j.eig ? j.eig : j.obj, j.obj ? j.obj : j.eig, p.pf_k, h->d_stats.get(), (int64_t)0);
    } else if (p.route == TK_ROUTE_COOP) {      // the runtime guarantees the co-residency (+20 us per launch)
        const uint64_t *keys_arg = h->d_key_a.get();
        TopkWs *ws_arg = j.ws;
        uint64_t *sk_arg = h->d_sel_key.get();
        uint32_t *si_arg = h->d_sel_idx.get();
        int64_t n_arg = j.n, k_arg = j.k, chunk_arg = p.chunk, sel_arg = j.sel, pf_arg = 0;
        int mode_arg = j.mode;
        const double *eig_arg = j.eig, *obj_arg = j.obj;
        unsigned long long *stats_arg = nullptr;
        int64_t ecap_arg = 0;
        void *args[] = {&n_arg, &k_arg, &chunk_arg, &keys_arg, &ws_arg, &sk_arg, &si_arg, &mode_arg, &sel_arg, &eig_arg, &obj_arg, &pf_arg, &stats_arg,
                        &ecap_arg};
        HIP_TRY(h, hipLaunchCooperativeKernel((const void *)tk_refine_kernel<false>, grid, blk, args, 0, h->stream));
    } else {
        hipLaunchKernelGGL(tk_refine_kernel<false>, grid, blk, 0, h->stream, j.n, j.k, p.chunk, h->d_key_a.get(), j.ws, h->d_sel_key.get(), h->d_sel_idx.get(),
                           j.mode, j.sel, j.eig, j.obj, (int64_t)0, (unsigned long long *)nullptr, (int64_t)0);
    }
    return 0;
}
