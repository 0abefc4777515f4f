// Top-k selection, the sort tail of every route but TK_ROUTE_SMALLSORT (topk_route.h): the compacted superset of the head in
// h->d_sel_key / h->d_sel_idx is ordered and the first k_eff entries are emitted.

#include "topk_launch.h"

// Final order of the selected pairs, (key desc, idx asc) = ascending composite (~key, idx):
//   1. tk_tilesort_kernel: bitonic sort of 512-entry tiles in LDS (one workgroup per tile);
//   2. tk_mergerank_kernel: every entry's final rank = its position in its own tile + the number
//      of entries preceding it in every other tile (binary searches over tiles staged in LDS;
//      composites are unique, so ranks are a permutation).
// ~k log k work instead of the k^2 of a counting sort, two short launches.  They serve the big heads, the raw key output and
// the shard records.  Everything else (TkPlan::count_rank) is ranked by tk_countrank_kernel below: on a chain of short
// dependent launches a launch costs more than k^2 comparisons spread over an otherwise idle device.

template <bool TIE>
__device__ __forceinline__ void tilesort_body(const TopkWs *ws, const uint64_t *sel_key, const uint32_t *sel_idx,
                                              uint64_t *tile_key, uint32_t *tile_idx, const double *obj, uint64_t *sk,
                                              uint32_t *si)
{
    const int k_eff = (int)ws->n_sel;              // compacted entries (a superset of the head after an early stop)
    const int lo = blockIdx.x * TK_TILE;
    if (lo >= k_eff) return;                       // uniform
    for (int t = threadIdx.x; t < TK_TILE; t += TK_THREADS) {
        const int j = lo + t;
        sk[t] = (j < k_eff) ? ~sel_key[j] : ~0ull;       // padding sorts last
        si[t] = (j < k_eff) ? sel_idx[j] : 0xffffffffu;
    }
    __syncthreads();
    for (int size = 2; size <= TK_TILE; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int t = threadIdx.x;
            const int pos = 2 * t - (t & (stride - 1));
            const int par = pos + stride;
            const bool up = (pos & size) == 0;
            const uint64_t ka = sk[pos], kb = sk[par];
            const uint32_t ia = si[pos], ib = si[par];
            if (comp_less<TIE>(kb, ib, ka, ia, obj) == up) {
                sk[pos] = kb; sk[par] = ka;
                si[pos] = ib; si[par] = ia;
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < TK_TILE; t += TK_THREADS) {
        tile_key[lo + t] = sk[t];
        tile_idx[lo + t] = si[t];
    }
}

// TIE: 0 plain composite compare, 1 obj_improve as tie key (mode COMBALL), 2 decided by the mode the
// selection resolved on the device (TK_MODE_COMBAUTO): one uniform branch at entry picks the
// specialised body, the comparators stay branch-free
template <int TIE>
__global__ __launch_bounds__(TK_THREADS) void tk_tilesort_kernel(const TopkWs *ws, const uint64_t *sel_key,
                                                                 const uint32_t *sel_idx, uint64_t *tile_key,
                                                                 uint32_t *tile_idx, const double *obj)
{
    __shared__ uint64_t sk[TK_TILE];
    __shared__ uint32_t si[TK_TILE];
    if (TIE == 1 || (TIE == 2 && ws->mode == TK_MODE_COMBALL))
        tilesort_body<true>(ws, sel_key, sel_idx, tile_key, tile_idx, obj, sk, si);
    else
        tilesort_body<false>(ws, sel_key, sel_idx, tile_key, tile_idx, obj, sk, si);
}

template <bool TIE>
__device__ __forceinline__ void mergerank_body(int64_t base, double score_add, const TopkWs *ws, const uint64_t *tile_key,
                                               const uint32_t *tile_idx, int64_t *idx_out, double *score_out,
                                               const double *obj, uint64_t *sk, uint32_t *si)
{
    const int n_sel = (int)ws->n_sel, k_eff = (int)ws->counters[3];
    if (blockIdx.x * TK_THREADS >= n_sel) return;   // uniform
    const int ntiles = (n_sel + TK_TILE - 1) / TK_TILE;
    // (a head of 5000: 11 tiles, 22 entries per thread; each batch is a round trip to L2)
    for (int j0 = 0; j0 < ntiles * TK_TILE; j0 += 24 * TK_THREADS) {      // 24 pairs in flight per thread: 12 tiles in ONE trip to L2
        uint64_t kk[24];
        uint32_t ii[24];
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            const int j = j0 + u * TK_THREADS + threadIdx.x;
            const bool in = j < ntiles * TK_TILE;
            kk[u] = in ? tile_key[j] : 0ull;
            ii[u] = in ? tile_idx[j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            const int j = j0 + u * TK_THREADS + threadIdx.x;
            if (j < ntiles * TK_TILE) { sk[j] = kk[u]; si[j] = ii[u]; }
        }
    }
    __syncthreads();
    const int e = blockIdx.x * TK_THREADS + threadIdx.x;      // position in the tiled array
    if (e >= ntiles * TK_TILE) return;
    const uint64_t ke = sk[e];
    const uint32_t ie = si[e];
    if (ie == 0xffffffffu && ke == ~0ull) return;             // padding
    const int te = e / TK_TILE;
    int rank = e - te * TK_TILE;
    // lower bound of e's composite inside every other tile (all composites are distinct).  (r5) The searches of FOUR tiles run
    // side by side, branch-free: a search is a chain of ten dependent LDS reads, and one after the other the up-to-15 chains were
    // a third of this kernel's time (11.6 -> 8.8 us).  Steps 256, 128 .. 1 count the entries below e among the first 511 of a
    // tile, one more comparison settles the 512-th.
    constexpr int MR_T = 4;
    // (the searches are bound by the LDS's throughput for scattered reads -- 8 or 16 at a time are no faster than 4, and they take
    // as long as the number of tiles searched says -- so e's own tile and tiles that do not exist are not searched: the other
    // ntiles - 1 tiles in batches of four, the last batch with its own trip count; branch-free inside a batch)
    auto search = [&](auto live_tag, const int t0) __attribute__((always_inline)) {
        constexpr int LIVE = decltype(live_tag)::value;
        int tb[LIVE], pos[LIVE];
#pragma unroll
        for (int u = 0; u < LIVE; ++u) {
            const int o = t0 + u;                    // the o-th OTHER tile
            tb[u] = (o < te ? o : o + 1) * TK_TILE;
            pos[u] = 0;
        }
#pragma unroll
        for (int step = TK_TILE / 2; step >= 1; step >>= 1) {
            uint64_t km[LIVE];
            uint32_t im[LIVE];
#pragma unroll
            for (int u = 0; u < LIVE; ++u) { km[u] = sk[tb[u] + pos[u] + step - 1]; im[u] = si[tb[u] + pos[u] + step - 1]; }
#pragma unroll
            for (int u = 0; u < LIVE; ++u) pos[u] += comp_less<TIE>(km[u], im[u], ke, ie, obj) ? step : 0;
        }
#pragma unroll
        for (int u = 0; u < LIVE; ++u) {
            const bool last = pos[u] == TK_TILE - 1 && comp_less<TIE>(sk[tb[u] + TK_TILE - 1], si[tb[u] + TK_TILE - 1], ke, ie, obj);
            rank += pos[u] + (last ? 1 : 0);
        }
    };
    const int others = ntiles - 1;      // uniform per workgroup
    int t0 = 0;
    for (; t0 + MR_T <= others; t0 += MR_T) search(std::integral_constant<int, MR_T>{}, t0);
    switch (others - t0) {
    case 3: search(std::integral_constant<int, 3>{}, t0); break;
    case 2: search(std::integral_constant<int, 2>{}, t0); break;
    case 1: search(std::integral_constant<int, 1>{}, t0); break;
    default: break;
    }
    if (rank >= k_eff) return;                                // superset entries beyond the head
    idx_out[rank] = base + (int64_t)ie;
    score_out[rank] = score_of(~ke) + score_add;
}

template <int TIE>
__global__ __launch_bounds__(TK_THREADS) void tk_mergerank_kernel(int64_t base, double score_add, const TopkWs *ws,
                                                                  const uint64_t *tile_key, const uint32_t *tile_idx,
                                                                  int64_t *idx_out, double *score_out, const double *obj,
                                                                  int64_t *rec_hdr, int64_t rec_count, int64_t rec_len)
{
    __shared__ uint64_t sk[TK_LDSK];
    __shared__ uint32_t si[TK_LDSK];
    if (rec_hdr) {
        // shard record (shard.hip): this launch also writes the 8-word header in front of the head
        // and pads the slots behind the entries it emits with (-inf, INT64_MAX); rec_len >= 0 is the
        // length of the shard's list when that is not the class size (optimality ranking)
        const int64_t g = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
        const int64_t written = ws->counters[4] ? 0 : ws->counters[3];
        if (g < rec_count && g >= written) {
            score_out[g] = -__builtin_huge_val();
            idx_out[g] = 0x7fffffffffffffffLL;
        }
        if (g < 8)
            rec_hdr[g] = g == 0 ? (rec_len >= 0 ? rec_len : ws->counters[0]) : g <= 4 ? ws->counters[g] : 0;
    }
    if (TIE == 1 || (TIE == 2 && ws->mode == TK_MODE_COMBALL)) {
        // (device-resolved regime: BIG_M belongs to the strong class only, not to COMBALL's own scores)
        mergerank_body<true>(base, TIE == 2 ? 0.0 : score_add, ws, tile_key, tile_idx, idx_out, score_out, obj, sk, si);
    } else {
        mergerank_body<false>(base, score_add, ws, tile_key, tile_idx, idx_out, score_out, obj, sk, si);
    }
}

// Heads of 8193 .. 16384 entries: the composite (key, index) pairs of all tiles no longer fit LDS, the
// keys alone do (128 KB); an index is fetched from the tile array only where two keys are equal.
// raw: score_out receives the key's low 63 bits as a double (keys that are not score images: the
// triangle inequalities' (density, violation) composite).
template <bool TIE>
__global__ __launch_bounds__(TK_THREADS) void tk_mergerank_big_kernel(int64_t base, double score_add, const TopkWs *ws,
                                                                      const uint64_t *tile_key, const uint32_t *tile_idx,
                                                                      int64_t *idx_out, double *score_out, const double *obj,
                                                                      int raw, int64_t emit_limit, int64_t *rec_hdr,
                                                                      int64_t rec_count, int64_t rec_len)
{
    __shared__ uint64_t sk[TK_MAXK];
    if (rec_hdr) {      // shard record: header and padding, as in tk_mergerank_kernel
        const int64_t g = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
        const int64_t written = ws->counters[4] ? 0 : ws->counters[3];
        if (g < rec_count && g >= written) {
            score_out[g] = -__builtin_huge_val();
            idx_out[g] = 0x7fffffffffffffffLL;
        }
        if (g < 8)
            rec_hdr[g] = g == 0 ? (rec_len >= 0 ? rec_len : ws->counters[0]) : g <= 4 ? ws->counters[g] : 0;
    }
    const int n_sel = (int)ws->n_sel, k_eff = (int)ws->counters[3];
    if (blockIdx.x * TK_THREADS >= n_sel) return;   // uniform
    const int ntiles = (n_sel + TK_TILE - 1) / TK_TILE;
    for (int j = threadIdx.x; j < ntiles * TK_TILE; j += TK_THREADS) sk[j] = tile_key[j];
    __syncthreads();
    const int e = blockIdx.x * TK_THREADS + threadIdx.x;
    if (e >= ntiles * TK_TILE) return;
    const uint64_t ke = sk[e];
    const uint32_t ie = tile_idx[e];
    if (ie == 0xffffffffu && ke == ~0ull) return;             // padding
    const int te = e / TK_TILE;
    int rank = e - te * TK_TILE;
    for (int t = 0; t < ntiles; ++t) {
        if (t == te) continue;
        int lo = 0, hi = TK_TILE;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const uint64_t km = sk[t * TK_TILE + mid];
            bool less = km < ke;
            if (km == ke) less = comp_less<TIE>(km, tile_idx[t * TK_TILE + mid], ke, ie, obj);
            lo = less ? mid + 1 : lo;
            hi = less ? hi : mid;
        }
        rank += lo;
    }
    if (rank >= k_eff || rank >= emit_limit) return;
    idx_out[rank] = base + (int64_t)ie;
    score_out[rank] = raw ? __longlong_as_double((long long)(~ke & 0x7fffffffffffffffull)) : score_of(~ke) + score_add;
}

// ---- ranks by counting, ONE launch (TkPlan::count_rank) ----------------------------------------------------------------------
// The rank of an entry among the n_sel <= TK_LDSK unique composites is the number of composites in front of it.  A wave is
// (group g of 64 compacted entries, slice s of the TK_CR_SLICES slices of the scanned entries); lane = entry.  The slice bounds
// depend on n_sel alone, so the scanned keys and indices are wave-uniform and arrive through scalar loads, eight pairs at a time;
// per scanned key a 64-bit compare with an add, and a compare for equality whose vcc decides ONE scalar branch: only where some
// lane holds an equal key does the tie rule of comp_less<TIE> run (by index; TIE: obj_improve of the scanned entry first -- a
// scalar load; the lane's own side is fetched once, in front of the loop).
// The TK_CR_SLICES partial ranks of an entry meet in acc[entry] = arrivals << 32 | rank sum through one returning device-scope
// add each.  The wave that sees the last arrival holds the final rank, emits the entry exactly as mergerank_body does and leaves
// the word zero for the next launch (the words are zeroed once, when the workspace is made: ensure_topk_ws).  No workgroup waits
// for another.  Groups beyond n_sel return at once, as idle tiles do.
template <bool TIE>
__device__ __forceinline__ void countrank_body(int64_t base, double score_add, const TopkWs *ws, const uint64_t *__restrict__ sel_key,
                                               const uint32_t *__restrict__ sel_idx, unsigned long long *acc, int64_t *idx_out,
                                               double *score_out, const double *__restrict__ obj)
{
    constexpr int WPG = TK_THREADS / 64;              // slices (waves) per workgroup
    constexpr int BPG = TK_CR_SLICES / WPG;           // workgroups per entry group
    static_assert(TK_CR_SLICES % WPG == 0 && BPG >= 1, "a workgroup holds whole slices");
    int n_sel = (int)ws->n_sel;
    if (n_sel > TK_LDSK) n_sel = TK_LDSK;             // (never: this path is planned for heads whose superset fits TK_LDSK)
    const int k_eff = (int)ws->counters[3];
    const int g = blockIdx.x / BPG;
    if (g * 64 >= n_sel) return;                      // uniform
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % BPG) * WPG + (int)(threadIdx.x >> 6));
    const int e = g * 64 + (int)(threadIdx.x & 63);
    const bool live = e < n_sel;
    const uint64_t ke = live ? ~sel_key[e] : 0ull;
    const uint32_t ie = live ? sel_idx[e] : 0u;
    uint64_t oe = 0ull;
    if constexpr (TIE) oe = live ? key_of(obj[ie]) : 0ull;
    const int len = ((n_sel + TK_CR_SLICES - 1) / TK_CR_SLICES + 7) & ~7;
    const int lo = s * len;
    const int hi = lo + len < n_sel ? lo + len : n_sel;      // (lo >= n_sel: an empty slice still reports its zero)
    uint32_t rank = 0;
    auto scan = [&](const uint64_t key, const uint32_t si) __attribute__((always_inline)) {
        const uint64_t sk = ~key;
        rank += sk < ke ? 1u : 0u;
        if (__ballot(sk == ke)) {                     // some lane ties with the scanned key (its own entry included): scalar branch
            asm volatile("" ::: "memory");            // (keeps the branch: flattened, every key pays the tie rule's compares)
            bool first = si < ie;
            if constexpr (TIE) {
                const uint64_t os = key_of(obj[si]);
                first = os != oe ? os > oe : first;
            }
            rank += (sk == ke && first) ? 1u : 0u;
        }
    };
    int j = lo;
    for (; j + 8 <= hi; j += 8) {
        uint64_t kk[8];
        uint32_t ii[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { kk[u] = sel_key[j + u]; ii[u] = sel_idx[j + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) scan(kk[u], ii[u]);
    }
    for (; j < hi; ++j) scan(sel_key[j], sel_idx[j]);
    if (!live) return;
    const unsigned long long old = __hip_atomic_fetch_add(&acc[e], (1ull << 32) | (unsigned long long)rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)(old >> 32) != (uint32_t)(TK_CR_SLICES - 1)) return;
    __hip_atomic_store(&acc[e], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int final_rank = (int)((uint32_t)old + rank);
    if (final_rank >= k_eff) return;                  // superset entries beyond the head
    idx_out[final_rank] = base + (int64_t)ie;
    score_out[final_rank] = score_of(~ke) + score_add;
}

// TIE as in tk_tilesort_kernel
template <int TIE>
__global__ __launch_bounds__(TK_THREADS) void tk_countrank_kernel(int64_t base, double score_add, const TopkWs *ws,
                                                                  const uint64_t *sel_key, const uint32_t *sel_idx,
                                                                  unsigned long long *acc, int64_t *idx_out, double *score_out,
                                                                  const double *obj)
{
    if (TIE == 1 || (TIE == 2 && ws->mode == TK_MODE_COMBALL)) {
        // (device-resolved regime: BIG_M belongs to the strong class only, not to COMBALL's own scores)
        countrank_body<true>(base, TIE == 2 ? 0.0 : score_add, ws, sel_key, sel_idx, acc, idx_out, score_out, obj);
    } else {
        countrank_body<false>(base, score_add, ws, sel_key, sel_idx, acc, idx_out, score_out, obj);
    }
}

// T: the plan's sort_tie.  Big heads (8193 .. 16384) go through the keys-only merge, the only one with the raw key output;
// the device-resolved regime (T = 2) never asks for them (tk_route refuses).
template <int T>
static void sort_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    uint64_t *tile_key = h->d_sel_key.get() + TK_MAXK;      // first half: compacted selection, second half: the sorted tiles
    uint32_t *tile_idx = h->d_sel_idx.get() + TK_MAXK;
    const double *tie_obj = T ? (j.tie_obj ? j.tie_obj : h->d_obj) : nullptr;
    if (p.count_rank) {      // one launch: 64-entry groups x slices, four slices per workgroup; idle groups exit at once
        const dim3 g_count(p.ntiles * (TK_TILE / 64) * (TK_CR_SLICES / (TK_THREADS / 64)));
        hipLaunchKernelGGL(tk_countrank_kernel<T>, g_count, dim3(TK_THREADS), 0, h->stream, j.base, j.score_add, j.ws, h->d_sel_key.get(),
                           h->d_sel_idx.get(), h->d_rank_acc.get(), j.d_idx_out, j.d_score_out, tie_obj);
        return;
    }
    const dim3 g_sort(p.ntiles), g_merge(p.ntiles * TK_TILE / TK_THREADS), blk(TK_THREADS);      // idle tiles exit at once
    hipLaunchKernelGGL(tk_tilesort_kernel<T>, g_sort, blk, 0, h->stream, j.ws, h->d_sel_key.get(), h->d_sel_idx.get(), tile_key, tile_idx, tie_obj);
    if constexpr (T < 2) {
        if (p.big_merge) {
            hipLaunchKernelGGL(tk_mergerank_big_kernel<(T != 0)>, g_merge, blk, 0, h->stream, j.base, j.score_add, j.ws, tile_key, tile_idx,
                               j.d_idx_out, j.d_score_out, tie_obj, j.raw, j.emit_limit, h->shard_rec, h->shard_rec_count, h->shard_rec_len);
            return;
        }
    }
    hipLaunchKernelGGL(tk_mergerank_kernel<T>, g_merge, blk, 0, h->stream, j.base, j.score_add, j.ws, tile_key, tile_idx, j.d_idx_out,
                       j.d_score_out, tie_obj, h->shard_rec, h->shard_rec_count, h->shard_rec_len);
}

void tk_sort_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j)
{
    if (p.sort_tie == 2) sort_launch<2>(h, p, j);
    else if (p.sort_tie == 1) sort_launch<1>(h, p, j);
    else sort_launch<0>(h, p, j);
}
