// Triangle-inequality separation (SURVEY.md section 8 f, row 3; reference
// cut_select_qp.py:799-863).  Per round every retained triple i1<i2<i3 yields four
// violations; the violated ones (>= 1e-7) are ranked by (density desc, violation desc), ties
// in entry order 4*triple + type (Python's stable sort), and the head is returned.  The caller
// consumes at most 10 000 of the ~1e6 entries (_TRI_CUTS_PER_ROUND_MAX): the head comes from the
// radix select of topk.hip over the composite keys, not from a sort of all of them.
#include <cstring>

#include "common.h"
#include "tri_dev.h"        // TRI_VIOL_THRES, the row of an entry, the block scan
#include "tri_layout.h"

// key: bit 63 = density 3, low bits = the positive violation's IEEE image (positive doubles
// order like integers); 0 = not violated.  Violations are <= 2, so bit 63 is free.
__global__ __launch_bounds__(256) void tri_viol_kernel(int64_t T, const int32_t *tri, const uint8_t *dense3,
                                                       const double *vars, int32_t nv, int64_t L, uint64_t *key,
                                                       uint32_t *val, int64_t *counters)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int nviol = 0;
    if (t < T) {
#pragma clang fp contract(off)
        const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        const int32_t ra = nv * a - (a * (a + 1)) / 2, rb = nv * b - (b * (b + 1)) / 2;
        const double X1 = vars[ra + b], X2 = vars[ra + c], X4 = vars[rb + c];      // X_slice[1], [2], [4]
        const double x0 = vars[L + a], x1 = vars[L + b], x2 = vars[L + c];
        double v[4];
        v[0] = X1 + X2 - X4 - x0;                                                  // :836-839, left to right
        v[1] = X1 - X2 + X4 - x1;
        v[2] = -X1 + X2 + X4 - x2;
        v[3] = -X1 - X2 - X4 + (((0.0 + x0) + x1) + x2) - 1.0;
        const uint64_t hi = dense3[t] ? 0x8000000000000000ull : 0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool viol = v[k] >= TRI_VIOL_THRES;                              // :841
            key[4 * t + k] = viol ? (hi | (uint64_t)__double_as_longlong(v[k])) : 0ull;
            val[4 * t + k] = (uint32_t)(4 * t + k);
            nviol += viol;
        }
    }
    for (int off = 32; off > 0; off >>= 1) nviol += __shfl_xor(nviol, off);
    if ((threadIdx.x & 63) == 0 && nviol) atomicAdd((unsigned long long *)&counters[0], (unsigned long long)nviol);
}

int tri_preprocess(sdpcut_ctx *h, const uint8_t *adjacency, int64_t *n_triples)
{
    const int n = h->nb_vars;
    std::vector<int32_t> tri;
    std::vector<uint8_t> d3;
    auto adj = [&](int i, int j) { return adjacency[(size_t)i * n + j] != 0; };
    for (int i1 = 0; i1 < n; ++i1)
        for (int i2 = i1 + 1; i2 < n; ++i2)
            for (int i3 = i2 + 1; i3 < n; ++i3) {
                const int dens = (int)adj(i1, i2) + (int)adj(i1, i3) + (int)adj(i2, i3);   // :812
                if (dens >= 2) {                                                          // _THRES_TRI_DENSE
                    tri.push_back(i1); tri.push_back(i2); tri.push_back(i3);
                    d3.push_back(dens == 3);
                }
            }
    const int64_t T = (int64_t)d3.size();
    if (4 * T > 0x7fffffffLL) return sdpcut_fail(h, SDPCUT_EINVAL, "too many triangle inequalities");
    h->d_tri.release(); h->d_tri_dense3.release();
    h->n_tri = 0;
    if (T > 0) {
        HIP_TRY(h, h->d_tri.reset((size_t)T * 3));
        HIP_TRY(h, h->d_tri_dense3.reset((size_t)T));
        HIP_TRY(h, hipMemcpy(h->d_tri.get(), tri.data(), (size_t)T * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_tri_dense3.get(), d3.data(), (size_t)T, hipMemcpyHostToDevice));
    }
    h->n_tri = T;
    h->tri_ready = true;
    h->tri_host = tri;
    h->tri_dense_host = d3;
    if (n_triples) *n_triples = T;
    return 0;
}

int tri_separate(sdpcut_ctx *h, int64_t max_out, int64_t *d_entry_out, double *d_viol_out, int64_t *n_violated,
                 int64_t *n_written)
{
    const int64_t T = h->n_tri, E = 4 * T;
    int64_t cnt[5] = {0, 0, 0, 0, 0};
    if (max_out > 16384) return sdpcut_fail(h, SDPCUT_EINVAL, "tri_separate: at most 16384 entries (the reference takes <= 10000)");
    if (E > 0) {
        int rc = ensure_rank_ws(h, E > h->N ? E : h->N);      // (the selection below sizes the key array for the candidate list as well: it must not move)
        if (rc) return rc;
        h->last_total = -1;
        HIP_TRY(h, hipMemsetAsync(h->d_counters.get(), 0, 8 * sizeof(int64_t), h->stream));
        hipLaunchKernelGGL(tri_viol_kernel, dim3((int)((T + 255) / 256)), dim3(256), 0, h->stream, T, h->d_tri.get(),
                           h->d_tri_dense3.get(), h->d_vars.get(), h->nb_vars, h->L, h->d_key_a.get(), h->d_val_a.get(), h->d_counters.get());
        HIP_TRY(h, hipGetLastError());
        if (max_out > 0) {
            rc = topk_select_keys_on_device(h, E, max_out, d_entry_out, d_viol_out, cnt);
            if (rc) return rc;
            if (cnt[4]) {
                // a bounded wait of the fused selection expired (the GPU shared with a kernel that kept its workgroups
                // from starting): the same selection with one launch per digit has no waits and always answers
                const bool fused = h->fused_tail;
                h->fused_tail = false;
                rc = topk_select_keys_on_device(h, E, max_out, d_entry_out, d_viol_out, cnt);
                h->fused_tail = fused;
                ++h->stat_fallbacks;
                if (rc) return rc;
                if (cnt[4]) return sdpcut_fail(h, SDPCUT_EHIP, "tri_separate: selection void");
            }
        } else {
            HIP_TRY(h, hipMemcpyAsync(cnt, h->d_counters.get(), sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, sdpcut_sync(h));
        }
    }
    const int64_t w = cnt[0] < max_out ? cnt[0] : max_out;
    if (n_violated) *n_violated = cnt[0];
    if (n_written) *n_written = w;
    return 0;
}

// ------------------------------------------------------------------------------------------
// The round with its rows (include/sdpcut.h: sdpcut_tri_round_csr): violation launch, the selection of tri_separate -- enqueued, not
// waited for --, then ONE workgroup writes the rows of the selected entries into the handle's pinned block, a block scan over
// the row lengths placing them (no look-back, no wait on another workgroup); one host wait.  With a node box the violation
// launch reads the box table of the point (box.hip: box_point_kernel, in front of it in stream order) and the rows are the
// box's facets in the original variables (tri_dev.h: tri_row).

#define TRI_EMIT_WAVES 4
// nviol: the violation launch's count; sel_cnt: the selection's counters (word 4: void) or NULL where nothing was selected
__global__ __launch_bounds__(TRI_EMIT_WAVES * 64) void tri_emit_kernel(int64_t cap, const int64_t *nviol, const int64_t *sel_cnt, const int64_t *ent,
                                                                        const double *vio, int64_t T, const int32_t *tri, const double *ld, int32_t nv,
                                                                        int64_t L, char *block)
{
    __shared__ uint32_t s_wave[TRI_EMIT_WAVES];
    const TriLayout y = tri_layout(cap);
    const TriBlockPtrs B = {(int64_t *)block, (int64_t *)(block + y.entry), (double *)(block + y.viol), (double *)(block + y.rhs),
                            (double *)(block + y.values), (int32_t *)(block + y.indptr), (int32_t *)(block + y.indices)};
    const int64_t nvl = nviol[0], vflag = sel_cnt ? sel_cnt[4] : 0;
    const int64_t w = vflag ? 0 : (nvl < cap ? nvl : cap);
    tri_emit_rows<TRI_EMIT_WAVES>(w, [&](int64_t i) { return ent[i]; }, [&](int64_t i) { return vio[i]; }, tri, T, ld, nv, L, B, nvl, vflag, s_wave);
}

void tri_out_from_block(const void *block, sdpcut_tri_csr_t *out)
{
    const TriLayout y = tri_layout(out->cap);
    const char *b = (const char *)block;
    const int64_t *hdr = (const int64_t *)b;
    out->n_rows = hdr[0];
    out->n_violated = hdr[1];
    out->nnz = hdr[2];
    out->entry = (const int64_t *)(b + y.entry);
    out->viol = (const double *)(b + y.viol);
    out->rhs = (const double *)(b + y.rhs);
    out->values = (const double *)(b + y.values);
    out->indptr = (const int32_t *)(b + y.indptr);
    out->indices = (const int32_t *)(b + y.indices);
}

// one pass: violations, selection (where cap > 0), rows; waited for.  -> the block's void word
static int tri_round_pass(sdpcut_ctx *h, int64_t cap, int64_t *d_e, double *d_v, int64_t *void_flag)
{
    const int64_t T = h->n_tri, E = 4 * T;
    HIP_TRY(h, hipMemsetAsync(h->d_counters.get(), 0, 8 * sizeof(int64_t), h->stream));
    hipLaunchKernelGGL(tri_viol_kernel, dim3((int)((T + 255) / 256)), dim3(256), 0, h->stream, T, h->d_tri.get(), h->d_tri_dense3.get(),
                       (const double *)(h->box_set ? h->d_vars_box.get() : h->d_vars.get()), h->nb_vars, h->L, h->d_key_a.get(), h->d_val_a.get(), h->d_counters.get());
    HIP_TRY(h, hipGetLastError());
    const int64_t *d_cnt = nullptr;
    if (cap > 0) {
        const int rc = topk_select_keys_enqueue(h, E, cap, d_e, d_v, &d_cnt);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(tri_emit_kernel, dim3(1), dim3(TRI_EMIT_WAVES * 64), 0, h->stream, cap, (const int64_t *)h->d_counters.get(), d_cnt, (const int64_t *)d_e,
                       (const double *)d_v, T, (const int32_t *)h->d_tri.get(), (const double *)(h->box_set ? h->d_box_ld.get() : nullptr), h->nb_vars, h->L,
                       (char *)h->pinned.dev());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sdpcut_sync(h));      // the one wait of the call
    *void_flag = ((const int64_t *)h->pinned.get())[3];
    return 0;
}

extern "C" {

int sdpcut_tri_round_csr(sdpcut_handle h, const double *vars_values, int64_t max_out, sdpcut_tri_csr_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    if (max_out < 0 || max_out > 16384) return sdpcut_fail(h, SDPCUT_EINVAL, "tri_round_csr: max_out must be 0 .. 16384 (the reference takes <= 10000)");
    if (!h->tri_ready) return sdpcut_fail(h, SDPCUT_ESTATE, "tri_round_csr: sdpcut_tri_preprocess first");
    if (!vars_values && !h->have_point) return sdpcut_fail(h, SDPCUT_ESTATE, "set_point first");
    int rc;
    if (vars_values && (rc = sdpcut_set_point(h, vars_values))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t T = h->n_tri, E = 4 * T;
    const int64_t cap = max_out < E ? max_out : E;
    std::memset(out, 0, sizeof(*out));
    out->cap = cap;
    if ((rc = ensure_pinned(h, tri_layout(cap).bytes))) return rc;
    if (E == 0) {      // an empty list: an empty block, nothing launched
        std::memset(h->pinned.get(), 0, tri_layout(0).bytes);
        tri_out_from_block(h->pinned.get(), out);
        return SDPCUT_OK;
    }
    if ((rc = ensure_stage(h, (size_t)(cap < 1 ? 1 : cap) * 16))) return rc;
    int64_t *d_e = (int64_t *)h->d_stage.get();
    double *d_v = (double *)((char *)h->d_stage.get() + (size_t)(cap < 1 ? 1 : cap) * 8);
    if ((rc = ensure_rank_ws(h, E > h->N ? E : h->N))) return rc;      // (as tri_separate: the key array serves the candidate list as well)
    h->last_total = -1;
    int64_t vflag = 0;
    if ((rc = tri_round_pass(h, cap, d_e, d_v, &vflag))) return rc;
    if (vflag) {
        // a bounded wait of the fused selection expired: the same selection with one launch per digit has no waits (tri_separate)
        const bool fused = h->fused_tail;
        h->fused_tail = false;
        rc = tri_round_pass(h, cap, d_e, d_v, &vflag);
        h->fused_tail = fused;
        ++h->stat_fallbacks;
        if (rc) return rc;
        if (vflag) return sdpcut_fail(h, SDPCUT_EHIP, "tri_round_csr: selection void");
    }
    tri_out_from_block(h->pinned.get(), out);
    return SDPCUT_OK;
}

} // extern "C"
