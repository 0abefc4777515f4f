// Triangle rounds over a batch of LP points (include/sdpcut.h: sdpcut_tri_round_csr_points): the open nodes of a tree search, each
// with the variable bounds of its node.  The single-point call costs a launch chain and a host hand-off per point; here
//   point copy           the P points from pinned staging to the device (boxed batches: a second copy, their (l | d) rows)
//   box_points_kernel    (box.hip; boxed batches) the transformed point x', X' of every point, Q' not computed
//   tri_points_kernel    one workgroup per point: counts, selects, sorts and emits
// and ONE host wait.  tri_points_kernel never stores a key array: the key of an entry is recomputed from the six table entries of
// its triple wherever it is needed (the tables of a point are a few KB to 64 KB and stay in cache).  Its steps, all inside the
// workgroup, barriers only:
//   count     n_violated; K = min(max_out, n_violated)
//   select    where n_violated > K: the K-th largest key by radix select, eight 8-bit digits from the top, a 256-bin histogram in
//             LDS per digit and one walk over the 4 T entries per digit
//   collect   the entries above the threshold key in any order, the threshold key's ties in entry order until K are held
//   sort      bitonic, (key descending, entry ascending), in LDS
//   emit      the rows (tri_dev.h: tri_emit_rows) into the point's slice of the pinned batch block, then the header
// There is no grid barrier and no wait on another workgroup: no give-up path.  Which batches go this way: tri_route.h; the others
// run sdpcut_tri_round_csr once per point inside the call.
#include <cstring>

#include "common.h"
#include "tri_dev.h"
#include "tri_layout.h"
#include "tri_route.h"

#define TRI_POINTS_WAVES 16
#define TRI_POINTS_THREADS (TRI_POINTS_WAVES * 64)

struct TriPointsArgs {
    int64_t T;
    const int32_t *tri;
    const uint8_t *dense3;
    const double *vars;      // [P][vars_stride]: the tables the violations are read from (boxed: the transformed points)
    int64_t vars_stride;
    const double *ld;        // [P][2 nv] (l | d) or NULL
    int32_t nv;
    int64_t L;
    int64_t max_out;         // <= TRI_POINTS_MAX_HEAD
    int64_t cap;             // min(max_out, 4 T): the entries a slice has room for
    char *block;
    int64_t slice;
};

// the four keys of triple t
__device__ __forceinline__ void tri_keys4(const TriPointsArgs &A, const double *vars, int64_t t, uint64_t k[4])
{
    double v[4];
    tri_viol4(vars, A.nv, A.L, A.tri[3 * t], A.tri[3 * t + 1], A.tri[3 * t + 2], v);
    const uint64_t hi = A.dense3[t] ? 0x8000000000000000ull : 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = tri_key(v[j], hi);
}

// the sort state of a head entry is what tri_route.h sizes TRI_POINTS_MAX_HEAD by: s_key + s_ent of tri_points_kernel
static_assert(sizeof(uint64_t) + sizeof(uint32_t) == TRI_POINTS_ENTRY_BYTES, "tri_route.h: TRI_POINTS_ENTRY_BYTES is the kernel's key + entry id");
static_assert(TRI_POINTS_MAX_HEAD * TRI_POINTS_ENTRY_BYTES + 2048 <= 64 * 1024, "the sort state, the histogram and the scan words fit 64 KB of LDS");

// before(a, b): a stands in front of b in the head
__device__ __forceinline__ bool tri_before(uint64_t ka, uint32_t ea, uint64_t kb, uint32_t eb) { return ka > kb || (ka == kb && ea < eb); }

// LDS: 32 KB keys + 16 KB entry ids + 1 KB histogram + scan words = 50 256 bytes (TRI_POINTS_MAX_HEAD of tri_route.h)
__global__ __launch_bounds__(TRI_POINTS_THREADS) void tri_points_kernel(TriPointsArgs A)
{
    __shared__ uint64_t s_key[TRI_POINTS_MAX_HEAD];
    __shared__ uint32_t s_ent[TRI_POINTS_MAX_HEAD];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[TRI_POINTS_WAVES];
    __shared__ uint32_t s_word[4];      // 0 n_violated, 1 the digit's bin, 2 still wanted from that bin, 3 entries collected above the threshold
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t p = blockIdx.x, T = A.T;
    const double *vars = A.vars + p * A.vars_stride;
    const double *ld = A.ld ? A.ld + p * 2 * (int64_t)A.nv : nullptr;
    char *block = A.block + p * A.slice;

    // count
    if (tid < 4) s_word[tid] = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int64_t t = tid; t < T; t += TRI_POINTS_THREADS) {
        uint64_t k[4];
        tri_keys4(A, vars, t, k);
#pragma unroll
        for (int j = 0; j < 4; ++j) mine += k[j] != 0;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0 && mine) atomicAdd(&s_word[0], mine);
    __syncthreads();
    const uint32_t nviol = s_word[0];
    const uint32_t K = nviol < (uint64_t)A.max_out ? nviol : (uint32_t)A.max_out;      // (<= TRI_POINTS_MAX_HEAD, <= cap)

    // select: thr = the K-th largest key, `need` of its ties wanted; thr = 0: every violated entry is wanted
    uint64_t thr = 0;
    uint32_t need = 0;
    if (nviol > K && K > 0) {      // (uniform)
        uint64_t prefix = 0, mask = 0;
        need = K;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            for (int64_t t = tid; t < T; t += TRI_POINTS_THREADS) {
                uint64_t k[4];
                tri_keys4(A, vars, t, k);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k[j] != 0 && (k[j] & mask) == prefix) atomicAdd(&s_hist[(k[j] >> shift) & 255], 1u);
            }
            __syncthreads();
            if (tid < 64) {      // wave 0: lane l owns the bins 255 - 4 l .. 252 - 4 l; the bin where the count from the top reaches `need`
                uint32_t c[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = s_hist[255 - 4 * lane - j]; sum += c[j]; }
                uint32_t incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t u = __shfl_up(incl, off);
                    if (lane >= off) incl += u;
                }
                uint32_t above = incl - sum;
                if (above < need && need <= incl) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (above < need && need <= above + c[j]) { s_word[1] = 255 - 4 * lane - j; s_word[2] = need - above; }
                        above += c[j];
                    }
                }
            }
            __syncthreads();
            prefix |= (uint64_t)s_word[1] << shift;
            mask |= 255ull << shift;
            need = s_word[2];
        }
        thr = prefix;
    }
    const uint32_t n_above = K - need;

    // collect
    uint32_t tie_run = 0;
    for (int64_t base = 0; base < T && K > 0; base += TRI_POINTS_THREADS) {      // (uniform trip count: the scan holds barriers)
        const int64_t t = base + tid;
        uint64_t k[4] = {0, 0, 0, 0};
        if (t < T) tri_keys4(A, vars, t, k);
        uint32_t ties = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k[j] > thr) {
                const uint32_t at = atomicAdd(&s_word[3], 1u);
                if (at < n_above) { s_key[at] = k[j]; s_ent[at] = (uint32_t)(4 * t + j); }
            }
            ties += thr != 0 && k[j] == thr;
        }
        if (tie_run < need) {      // (uniform)
            uint32_t total;
            uint32_t r = tie_run + tri_block_scan<TRI_POINTS_WAVES>(ties, s_wave, total);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k[j] == thr && thr != 0) {
                    if (r < need) { s_key[n_above + r] = thr; s_ent[n_above + r] = (uint32_t)(4 * t + j); }
                    ++r;
                }
            tie_run += total;
        }
    }
    // sort: the K held entries padded to a power of two with keys that stand last
    uint32_t n2 = 2;
    while (n2 < K) n2 <<= 1;
    __syncthreads();
    for (uint32_t i = K + tid; i < n2; i += TRI_POINTS_THREADS) { s_key[i] = 0; s_ent[i] = 0xffffffffu; }
    __syncthreads();
    if (K > 1) {
        for (uint32_t k2 = 2; k2 <= n2; k2 <<= 1)
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < n2; i += TRI_POINTS_THREADS) {
                    const uint32_t o = i ^ j;
                    if (o > i) {
                        const uint64_t ka = s_key[i], kb = s_key[o];
                        const uint32_t ea = s_ent[i], eb = s_ent[o];
                        const bool swap = (i & k2) == 0 ? tri_before(kb, eb, ka, ea) : tri_before(ka, ea, kb, eb);
                        if (swap) { s_key[i] = kb; s_key[o] = ka; s_ent[i] = eb; s_ent[o] = ea; }
                    }
                }
                __syncthreads();
            }
    }

    // emit
    const TriLayout y = tri_layout(A.cap);
    const TriBlockPtrs B = {(int64_t *)block, (int64_t *)(block + y.entry), (double *)(block + y.viol), (double *)(block + y.rhs),
                            (double *)(block + y.values), (int32_t *)(block + y.indptr), (int32_t *)(block + y.indices)};
    tri_emit_rows<TRI_POINTS_WAVES>((int64_t)K, [&](int64_t i) { return (int64_t)s_ent[i]; }, [&](int64_t i) { return tri_key_viol(s_key[i]); }, A.tri, T,
                                    ld, A.nv, A.L, B, (int64_t)nviol, 0, s_wave);
}

// ------------------------------------------------------------------------------------------
// buffers (grown on demand through grow, common.h)

struct TriPointsBufs {
    HostBuf stage{false};           // pinned staging (default memory: the source of a hipMemcpyAsync): the points [P][L + n], then the (l | d) rows [P][2 n]
    DevBuf<double> d_pts, d_vb, d_ld;
    HostBuf pinned{true};           // the batch block (tri_layout.h: tri_batch_layout)
};

void free_tri_points_ws(sdpcut_ctx *h)
{
    delete (TriPointsBufs *)h->tri_pts;
    h->tri_pts = nullptr;
}

static int ensure_tri_points(sdpcut_ctx *h, int P, bool boxed, bool tables, size_t block_bytes)
{
    if (!h->tri_pts) h->tri_pts = new TriPointsBufs();
    TriPointsBufs &b = *(TriPointsBufs *)h->tri_pts;
    int rc;
    if ((rc = grow(h, b.pinned, block_bytes))) return rc;
    if (!tables) return 0;
    const size_t m = (size_t)(h->L + h->nb_vars), pts = (size_t)P * m, lds = boxed ? (size_t)P * 2 * (size_t)h->nb_vars : 0;
    if ((rc = grow(h, b.stage, (pts + lds) * 8))) return rc;
    if ((rc = grow(h, b.d_pts, pts))) return rc;
    if (boxed && (rc = grow(h, b.d_vb, pts))) return rc;
    if (boxed && (rc = grow(h, b.d_ld, lds))) return rc;
    return 0;
}

extern "C" {

int sdpcut_tri_round_csr_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                                int64_t max_out, sdpcut_tri_csr_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    const char *what = "sdpcut_tri_round_csr_points";
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    int rc;
    if ((rc = check_point_batch(h, "", n_points, points, point_ld, h->L + h->nb_vars))) return rc;
    if (!h->d_vars.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if ((rc = check_box_pair(h, "sdpcut_tri_round_csr_points: ", lb, ub))) return rc;
    if (max_out < 0 || max_out > 16384) return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": max_out must be 0 .. 16384");
    if (!h->tri_ready) return sdpcut_fail(h, SDPCUT_ESTATE, std::string(what) + ": sdpcut_tri_preprocess first");
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, what);      // (the call brings its boxes; the handle's own would be lost)
    const int P = n_points;
    const int32_t nv = h->nb_vars;
    const bool boxed = lb != nullptr;
    if (boxed) {
        if (h->exact_head) return sdpcut_fail(h, SDPCUT_ESTATE, std::string(what) + ": SDPCUT_OPT_EXACT_HEAD is on (reference-exact heads have no node box)");
        for (int p = 0; p < P; ++p)
            if ((rc = box_check(h, what, p, lb + (size_t)p * nv, ub + (size_t)p * nv))) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    NoPointAfter leave(h);
    NoBoxAfter unboxed(h);
    std::memset(out, 0, (size_t)P * sizeof(*out));
    const int64_t T = h->n_tri, E = 4 * T, m = h->L + nv;
    const int64_t cap = max_out < E ? max_out : E;
    const int route = E == 0 ? TRI_LOOP : tri_route(max_out, nv, P, boxed, TRI_POINTS_BUDGET_BYTES);
    const TriBatchLayout y = tri_batch_layout(cap, P);
    if ((rc = ensure_tri_points(h, P, boxed, route == TRI_FAST, y.bytes))) return rc;
    TriPointsBufs &b = *(TriPointsBufs *)h->tri_pts;
    char *block = (char *)b.pinned.get();
    if (route == TRI_LOOP) {
        for (int p = 0; p < P; ++p) {
            if (boxed && (rc = sdpcut_set_box(h, lb + (size_t)p * nv, ub + (size_t)p * nv))) return rc;
            if ((rc = sdpcut_tri_round_csr(h, points + (size_t)p * point_ld, max_out, out + p))) return rc;
            std::memcpy(block + y.slice * (size_t)p, h->pinned.get(), tri_layout(cap).bytes);
            tri_out_from_block(block + y.slice * (size_t)p, out + p);
        }
        return SDPCUT_OK;
    }

    double *st = (double *)b.stage.get();
    pack_points(st, P, points, point_ld, m);
    HIP_TRY(h, hipMemcpyAsync(b.d_pts.get(), st, (size_t)P * m * 8, hipMemcpyHostToDevice, h->stream));
    if (boxed) {
        double *ld = st + (size_t)P * m;      // the (l | d) rows as sdpcut_set_box forms them
        pack_box_ld(ld, P, nv, lb, nv, ub, nv);
        HIP_TRY(h, hipMemcpyAsync(b.d_ld.get(), ld, (size_t)P * 2 * nv * 8, hipMemcpyHostToDevice, h->stream));
        if ((rc = launch_box_points(h, P, b.d_pts.get(), m, b.d_ld.get(), nullptr, b.d_vb.get()))) return rc;
    }
    TriPointsArgs A;
    A.T = T;
    A.tri = h->d_tri.get();
    A.dense3 = h->d_tri_dense3.get();
    A.vars = boxed ? b.d_vb.get() : b.d_pts.get();
    A.vars_stride = m;
    A.ld = boxed ? b.d_ld.get() : nullptr;
    A.nv = nv;
    A.L = h->L;
    A.max_out = max_out;
    A.cap = cap;
    A.block = (char *)b.pinned.dev();
    A.slice = (int64_t)y.slice;
    hipLaunchKernelGGL(tri_points_kernel, dim3((unsigned)P), dim3(TRI_POINTS_THREADS), 0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sdpcut_sync(h));      // the one wait of the batch
    for (int p = 0; p < P; ++p) {
        out[p].cap = cap;
        tri_out_from_block(block + y.slice * (size_t)p, out + p);
    }
    h->stat_tri_points_fast += P;
    return SDPCUT_OK;
}

} // extern "C"
