// What a handle is given before it can score (include/sdpcut.h): the networks, the instance, the candidate list, the LP point.
#include <cstring>

#include "common.h"

// Device arrays of a candidate list of N entries, cnt[k] of them with k variables (the callers
// fill them: sdpcut_set_candidates from host arrays, the Philox generator and the cover
// enumeration on the device).  Frees the previous list; sizes the ranking workspace.
int alloc_candidates(sdpcut_ctx *h, int64_t N, const int64_t cnt[SDPCUT_MAX_K + 1], int64_t global_base)
{
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    free_candidates(h);
    h->base = global_base;
    const size_t nn = (size_t)(N < 1 ? 1 : N);
    HIP_TRY(h, h->d_set_orig.reset(nn * 5));
    HIP_TRY(h, h->d_k.reset(nn));
    HIP_TRY(h, h->d_eig.reset(nn));
    HIP_TRY(h, h->obj_own.reset(nn));
    h->d_obj = h->obj_own.get();
    h->row_len_max = 5;
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) {
        Bucket &b = h->bucket[k];
        b.n = cnt[k];
        if (!cnt[k]) continue;
        h->row_len_max = k * (k + 3) / 2;
        HIP_TRY(h, b.d_set.reset((size_t)cnt[k] * k));
        HIP_TRY(h, b.d_orig.reset((size_t)cnt[k]));
    }
    h->N = N;
    return 0;      // (the ranking workspaces are allocated by whoever first needs them: ensure_key_ws / ensure_rank_ws)
}

void free_candidates(sdpcut_ctx *h)
{
    for (int k = 0; k <= SDPCUT_MAX_K; ++k) h->bucket[k] = Bucket();
    h->d_set_orig.release(); h->d_k.release(); h->d_eig.release(); h->obj_own.release();
    h->d_obj = nullptr;
    free_sdp_ws(h);
    free_eff_ws(h);
    h->N = 0; h->scored = 0; h->obj_partial = false; h->last_total = -1;
    h->stat_nn_skipped = 0; h->nn_skipped_on_device = false;
    h->nn_eval_mode = 0; h->nn_eval_n = 0;
    h->topk_alt_clean = false;      // (how much of the selection workspace a round's epilogue zeroes depends on the list's length)
    h->side_choice = -1;      // (a new list measures for itself whether its small size classes go to side streams)
}

extern "C" {

int sdpcut_set_network(sdpcut_handle h, int k, int n_layers, const int32_t *widths, const double *params,
                       int64_t n_params)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    NetPack pk;
    const char *why = nullptr;
    if (net_pack(k, n_layers, widths, params, n_params, &pk, &why) != SDPCUT_OK) return sdpcut_fail(h, SDPCUT_EINVAL, why);
    HIP_TRY(h, hipSetDevice(h->device));
    NetHost &nh_ = h->net[k];
    HIP_TRY(h, sdpcut_sync(h));
    nh_.d_blob.release();
    nh_.set = false;
    h->scored &= ~(uint32_t)SDPCUT_NN; h->obj_partial = false;      // the list's optimality scores were the old network's: a round scores again
    // one allocation: the blob | filter_box [d_in][2] | the fp32 forms of the filter (floats; empty unless filter_ok) | filter_g [64]
    const size_t n_box = 2 * (size_t)pk.d_in;
    const size_t n_pre = (pk.blob.size() + n_box + 1) & ~(size_t)1;      // (an even number of doubles: the float4 loads stay aligned)
    HIP_TRY(h, nh_.d_blob.reset(n_pre * sizeof(double) + (pk.f32.size() + MAX_HIDDEN) * sizeof(float)));
    double *const blob = (double *)nh_.d_blob.get();
    HIP_TRY(h, hipMemcpy(blob, pk.blob.data(), pk.blob.size() * sizeof(double), hipMemcpyHostToDevice));
    double *d_box = blob + pk.blob.size();
    float *d_f32 = (float *)(blob + n_pre);
    HIP_TRY(h, hipMemcpy(d_box, &pk.filter_box[0][0], n_box * sizeof(double), hipMemcpyHostToDevice));
    if (!pk.f32.empty()) HIP_TRY(h, hipMemcpy(d_f32, pk.f32.data(), pk.f32.size() * sizeof(float), hipMemcpyHostToDevice));
    float *d_g = d_f32 + pk.f32.size();      // (a multiple of four floats behind d_f32: the float4 loads stay aligned)
    HIP_TRY(h, hipMemcpy(d_g, pk.filter_g, MAX_HIDDEN * sizeof(float), hipMemcpyHostToDevice));
    NetDev &d = nh_.dev;
    d = NetDev{};
    d.d_in = pk.d_in; d.n_hidden = pk.n_hidden; d.width = pk.width; d.s0 = pk.s0; d.sh = pk.sh;
    d.inmap = blob + pk.o_inmap;
    d.bias = blob + pk.o_bias;
    d.bias_q = blob + pk.o_bias_q;
    d.wout = blob + pk.o_wout;
    d.wfrag = blob + pk.o_frag;
    d.wvalu = blob + pk.o_wvalu;
    d.wtail = blob + pk.o_wtail;
    for (int l = 0; l < n_layers; ++l) { d.raw_w[l] = blob + pk.o_rw[l]; d.raw_b[l] = blob + pk.o_rb[l]; }
    d.ymin = pk.ymin; d.b_out = pk.b_out; d.y_ymin = pk.y_ymin; d.y_gain = pk.y_gain; d.y_xoffset = pk.y_xoffset;
    d.unclamped_ok = pk.unclamped_ok;
    d.filter_ok = pk.filter_ok; d.filter_margin = pk.filter_margin; d.filter_box = d_box;
    if (pk.filter_ok) { d.f32_in = d_f32 + pk.o32_in; d.f32_hid = d_f32 + pk.o32_hid; d.f32_bias = d_f32 + pk.o32_bias; d.f32_g = d_g; }
    d.filter_c0 = pk.filter_c0;
    nh_.set = true;
    return SDPCUT_OK;
}
int sdpcut_set_instance(sdpcut_handle h, int32_t nb_vars, const double *Q_arr)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    // (one variable: no candidate set fits, but sdpcut_node_eval_points serves it)
    if (nb_vars < 1 || nb_vars > 40000 || !Q_arr) return sdpcut_fail(h, SDPCUT_EINVAL, "bad instance");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    const int64_t L = (int64_t)nb_vars * (nb_vars + 1) / 2;
    h->d_Q.release(); h->d_vars.release();
    box_clear(h);      // (a box belongs to the instance it was set for)
    free_lpobj(h);     // (so does an LP objective vector: its length is the instance's)
    h->have_point = false; h->scored = 0; h->obj_partial = false;
    HIP_TRY(h, h->d_Q.reset((size_t)L));
    HIP_TRY(h, h->d_vars.reset((size_t)(L + nb_vars)));
    HIP_TRY(h, hipMemcpy(h->d_Q.get(), Q_arr, L * sizeof(double), hipMemcpyHostToDevice));
    h->nb_vars = nb_vars;
    h->L = L;
    h->q_absmax = 0.0;
    for (int64_t i = 0; i < L; ++i) {
        const double a = Q_arr[i] < 0.0 ? -Q_arr[i] : Q_arr[i];
        if (a > h->q_absmax) h->q_absmax = a;
    }
    return SDPCUT_OK;
}

int sdpcut_set_candidates(sdpcut_handle h, int64_t N, const int32_t *set_inds, int32_t ld, const int32_t *ks,
                          int64_t global_base)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (h->nb_vars == 0) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if (N < 0 || N > 0x7fffffffLL || (N > 0 && (!set_inds || !ks)) || ld < 2)
        return sdpcut_fail(h, SDPCUT_EINVAL, "bad candidate list");
    HIP_TRY(h, hipSetDevice(h->device));
    // validate + bucket by size on the host (once per instance)
    int64_t cnt[SDPCUT_MAX_K + 1] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < N; ++i) {
        const int k = ks[i];
        if (k < 2 || k > SDPCUT_MAX_K || k > ld) return sdpcut_fail(h, SDPCUT_EINVAL, "candidate size must be 2..5");
        for (int a = 0; a < k; ++a) {
            const int32_t v = set_inds[i * ld + a];
            if (v < 0 || v >= h->nb_vars) return sdpcut_fail(h, SDPCUT_EINVAL, "variable index out of range");
        }
        ++cnt[k];
    }
    std::vector<int32_t> pad((size_t)N * 5, -1), kk((size_t)N);
    std::vector<int32_t> soa[SDPCUT_MAX_K + 1], orig[SDPCUT_MAX_K + 1];
    int64_t fill[SDPCUT_MAX_K + 1] = {0, 0, 0, 0, 0, 0};
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) { soa[k].resize((size_t)cnt[k] * k); orig[k].resize((size_t)cnt[k]); }
    for (int64_t i = 0; i < N; ++i) {
        const int k = ks[i];
        kk[i] = k;
        const int64_t p = fill[k]++;
        orig[k][p] = (int32_t)i;
        for (int a = 0; a < k; ++a) {
            const int32_t v = set_inds[i * ld + a];
            pad[i * 5 + a] = v;
            soa[k][(size_t)a * cnt[k] + p] = v;
        }
    }
    int rc = alloc_candidates(h, N, cnt, global_base);
    if (rc) return rc;
    if (N > 0) {
        HIP_TRY(h, hipMemcpy(h->d_set_orig.get(), pad.data(), (size_t)N * 5 * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_k.get(), kk.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) {
        Bucket &b = h->bucket[k];
        if (!cnt[k]) continue;
        HIP_TRY(h, hipMemcpy(b.d_set.get(), soa[k].data(), soa[k].size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(b.d_orig.get(), orig[k].data(), orig[k].size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return SDPCUT_OK;
}

static int ensure_point_stage(sdpcut_ctx *h)
{
    return grow(h, h->point_stage, (size_t)(h->L + h->nb_vars) * sizeof(double));
}

int sdpcut_point_buffer(sdpcut_handle h, double **buf)
{
    if (!h) return SDPCUT_EINVAL;
    if (!buf) return sdpcut_fail(h, SDPCUT_EINVAL, "buf is NULL");
    if (!h->d_vars.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_point_stage(h);
    if (rc) return rc;
    *buf = (double *)h->point_stage.get();
    return SDPCUT_OK;
}

int sdpcut_set_point(sdpcut_handle h, const double *vars_values)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!h->d_vars.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if (!vars_values) return sdpcut_fail(h, SDPCUT_EINVAL, "vars_values is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    // The caller's (pageable) buffer is copied into a pinned staging block and sent from there: the
    // call returns as soon as the host copy is done -- the caller may reuse its buffer at once -- and
    // the DMA runs behind it on the stream, in front of the score kernels (no blocking round trip
    // per round).  The staging block is reused once the previous transfer out of it has completed.
    // A caller that wrote the point straight into the staging block (sdpcut_point_buffer) skips the copy.
    const size_t bytes = (size_t)(h->L + h->nb_vars) * sizeof(double);
    int rc = ensure_point_stage(h);
    if (rc) return rc;
    if (vars_values != (const double *)h->point_stage.get()) {
        // (every round ends in a host wait on the device, so this one is normally skipped; an event per
        // transfer would put a barrier packet -- ~10 us -- in front of every score launch)
        if (h->point_inflight) HIP_TRY(h, sdpcut_sync(h));
        std::memcpy(h->point_stage.get(), vars_values, bytes);
    }
    // a kernel of the compute queue pulls the block over PCIe (mapped host memory): the score launch
    // follows it in queue order, whereas a copy-engine transfer costs a cross-queue hand-off (~10 us)
    // in front of every round
    rc = launch_point_copy(h, (const double *)h->point_stage.dev(), h->L + h->nb_vars);
    if (rc) return rc;
    if ((rc = box_after_point(h))) return rc;
    h->point_inflight = true;
    h->have_point = true;
    h->scored = 0; h->obj_partial = false;
    h->last_total = -1;
    return SDPCUT_OK;
}

int sdpcut_set_point_device(sdpcut_handle h, const void *d_vars_values)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!h->d_vars.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if (!d_vars_values) return sdpcut_fail(h, SDPCUT_EINVAL, "d_vars_values is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->d_vars.get(), d_vars_values, (h->L + h->nb_vars) * sizeof(double),
                              hipMemcpyDeviceToDevice, h->stream));
    int rc = box_after_point(h);
    if (rc) return rc;
    h->have_point = true;
    h->scored = 0; h->obj_partial = false;
    h->last_total = -1;
    return SDPCUT_OK;
}

} // extern "C"
