// api.cpp — the extern "C" surface of libdsdiff.so (see include/dsdiff.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "net.h"

using namespace dsd;

static thread_local std::string g_err;

#define DSD_TRY try {
#define DSD_CATCH                          \
    }                                      \
    catch (const std::exception& e) {      \
        g_err = e.what();                  \
        return -1;                         \
    }                                      \
    catch (...) {                          \
        g_err = "unknown error";           \
        return -1;                         \
    }                                      \
    return 0;

namespace {

void ensure_buf(float** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return;
    if (*p) {
        DSD_HIP(hipDeviceSynchronize());
        DSD_HIP(hipFree(*p));
        *p = nullptr;
        *cap = 0;
    }
    DSD_HIP(hipMalloc((void**)p, bytes));
    *cap = bytes;
}

// temp device buffer for the dsd_op_* test entry points
struct Tmp {
    void* p = nullptr;
    explicit Tmp(size_t bytes) { DSD_HIP(hipMalloc(&p, bytes ? bytes : 256)); }
    ~Tmp() {
        if (p) {
            (void)hipDeviceSynchronize();
            (void)hipFree(p);
        }
    }
    template <class T> T* as() { return reinterpret_cast<T*>(p); }
};

void set_device(int device) {
    if (device >= 0) DSD_HIP(hipSetDevice(device));
}

// y of a dsd_conditioning against the handle's label_emb (kind lk, width lw) and the call's batch; int labels are read back
// and checked against the table, whose rows the lookup kernel indexes unchecked
void check_y(dsd_handle* h, const dsd_conditioning& c, int lk, int lw, int B) {
    const int want = lk == 1 ? 0 : lw;
    DSD_CHECK(c.y_width == want, "y_width %d does not match the handle's label_emb (kind %d wants %d: 0 = int64 labels)", c.y_width, lk, want);
    DSD_CHECK(c.B == B, "the conditioning was set for a batch of %d but the call has %d", c.B, B);
    if (lk == 1) {
        std::vector<long long> lab((size_t)B);
        for (const void* p : {c.y, c.y_uncond}) {
            if (!p) continue;
            DSD_HIP(hipDeviceSynchronize());
            DSD_HIP(hipMemcpy(lab.data(), p, (size_t)B * sizeof(long long), hipMemcpyDeviceToHost));
            for (int i = 0; i < B; ++i)
                DSD_CHECK(lab[i] >= 0 && lab[i] < lw, "label %d is %lld but the model has %d classes", i, lab[i], lw);
        }
    }
}

void bind_planes(dsd_handle* h, const float* x, int C, int H, int W, hipStream_t s) {
    const int64_t hw = (int64_t)H * W;
    DSD_CHECK(C == 2 || C == 4, "x must have 2 or 4 channels (noise + 1 or 3 conditions), got %d", C);
    h->io.plane[0] = x;
    h->io.plane[1] = x + hw;
    h->io.plane_bs[0] = h->io.plane_bs[1] = (int64_t)C * hw;
    if (C == 2) {  // model.py:654-658: al = l = zeros_like(n)
        ensure_buf(&h->zplane, &h->zplane_cap, (size_t)hw * sizeof(float));
        DSD_HIP(hipMemsetAsync(h->zplane, 0, (size_t)hw * sizeof(float), s));
        h->io.plane[2] = h->io.plane[3] = h->zplane;
        h->io.plane_bs[2] = h->io.plane_bs[3] = 0;
    } else {       // model.py:660-663
        h->io.plane[2] = x + 2 * hw;
        h->io.plane[3] = x + 3 * hw;
        h->io.plane_bs[2] = h->io.plane_bs[3] = (int64_t)C * hw;
    }
}

}  // namespace

extern "C" {

const char* dsd_last_error(void) { return g_err.c_str(); }

int dsd_device_info(int device, char* name, int name_len, int* n_cu, int64_t* hbm_bytes) {
    DSD_TRY
    int cnt = 0;
    DSD_HIP(hipGetDeviceCount(&cnt));
    DSD_CHECK(device >= 0 && device < cnt, "device %d not present (%d visible)", device, cnt);
    hipDeviceProp_t prop;
    DSD_HIP(hipGetDeviceProperties(&prop, device));
    DSD_CHECK(std::strncmp(prop.gcnArchName, "gfx950", 6) == 0, "device %d is %s; libdsdiff is built for gfx950 only", device,
              prop.gcnArchName);
    if (name && name_len > 0) {
        std::strncpy(name, prop.name, name_len - 1);
        name[name_len - 1] = 0;
    }
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    DSD_CATCH
}

int dsd_create(const dsd_config* cfg, int device, dsd_handle** out) {
    DSD_TRY
    DSD_CHECK(cfg && out, "null argument");
    set_device(device);
    auto* h = new dsd_handle();
    h->device = device;
    h->cfg = *cfg;
    try {
        net_declare_params(h);
    } catch (...) {
        net_free(h);
        delete h;
        throw;
    }
    *out = h;
    DSD_CATCH
}

int dsd_create_disc(const dsd_config* cfg, int device, dsd_handle** out) {
    DSD_TRY
    DSD_CHECK(cfg && out, "null argument");
    set_device(device);
    auto* h = new dsd_handle();
    h->device = device;
    h->is_disc = true;
    h->cfg = *cfg;
    // UNet_disc_Model has only the openai-style AttentionBlock(num_heads, num_head_channels): the head rule the spec builder
    // applies under `legacy` (heads = the argument, or channels / num_head_channels), decoder heads from num_heads_upsample
    h->cfg.legacy = 1;
    try {
        net_declare_params(h);
    } catch (...) {
        net_free(h);
        delete h;
        throw;
    }
    *out = h;
    DSD_CATCH
}

int dsd_block_create(int kind, const int32_t* iargs, int n_iargs, int device, dsd_handle** out) {
    DSD_TRY
    DSD_CHECK(out && (iargs || n_iargs == 0), "null argument");
    set_device(device);
    auto* h = new dsd_handle();
    h->device = device;
    h->is_block = true;
    h->block_kind = kind;
    h->iargs.assign(iargs, iargs + n_iargs);
    h->cfg.use_new_attention_order = 1;
    try {
        net_declare_params(h);
    } catch (...) {
        net_free(h);
        delete h;
        throw;
    }
    *out = h;
    DSD_CATCH
}

void dsd_destroy(dsd_handle* h) {
    if (!h) return;
    if (h->device >= 0) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
    }
    net_free(h);
    delete h;
}

int dsd_param_count(dsd_handle* h) { return h ? (int)h->params.size() : -1; }

int dsd_param_info(dsd_handle* h, int idx, const char** name, int64_t shape[4], int* ndim) {
    DSD_TRY
    DSD_CHECK(h && idx >= 0 && idx < (int)h->params.size(), "parameter index out of range");
    const Param& p = h->params[idx];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = (int)p.shape.size();
    if (shape)
        for (size_t i = 0; i < 4; ++i) shape[i] = i < p.shape.size() ? p.shape[i] : 1;
    DSD_CATCH
}

int dsd_set_param(dsd_handle* h, const char* name, const float* src, const int64_t* shape, int ndim, int src_is_device,
                  void* stream) {
    DSD_TRY
    DSD_CHECK(h && name && src && shape, "null argument");
    set_device(h->device);
    net_set_param(h, name, src, shape, ndim, src_is_device, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_set_timestep_freqs(dsd_handle* h, const float* freqs_host, int n) {
    DSD_TRY
    DSD_CHECK(h && freqs_host && (!h->is_block || h->block_kind == DSD_BLOCK_DIT || h->block_kind == DSD_BLOCK_UNET),
              "null argument / handle without a timestep embedding");
    const int want = h->block_kind == DSD_BLOCK_DIT ? 128 : h->cfg.model_channels / 2;   // DiT: frequency_embedding_size 256 (DiT_models.py:31)
    DSD_CHECK(n == want, "expected %d frequencies, got %d", want, n);
    set_device(h->device);
    if (!h->freqs) DSD_HIP(hipMalloc((void**)&h->freqs, (size_t)n * sizeof(float)));
    DSD_HIP(hipMemcpy(h->freqs, freqs_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    DSD_CATCH
}

int dsd_set_precision(dsd_handle* h, int precision) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    DSD_CHECK(precision >= PREC_F32 && precision <= PREC_BF16, "unknown precision %d", precision);
    DSD_CHECK(precision <= PREC_F16X3 || (h->is_block && h->block_kind == DSD_BLOCK_DIT),
              "DSD_PREC_F16 / DSD_PREC_BF16 (single-product autocast arithmetic) exist for DSD_BLOCK_DIT handles only: the other "
              "networks are checked against the fp32 CPU path at 1e-4 and keep fp32-grade products");
    if (h->precision != precision) {
        set_device(h->device);
        h->precision = precision;
        h->plan.valid = false;   // the plan bakes the kernel choice in
        net_drop_graph(h);
        net_drop_other_pieces(h, precision);   // bf16 and fp16 pieces (6 B per weight each) are never both resident
    }
    DSD_CATCH
}

int dsd_get_precision(dsd_handle* h) { return h ? h->precision : -1; }

int dsd_set_share_zero_streams(dsd_handle* h, int on) {
    DSD_TRY
    DSD_CHECK(h && !h->is_block, "needs a model handle");
    DSD_CHECK(!(h->is_disc && on), "UNet_disc_Model has no zero streams to share: all four encoder streams (x, T1, T2, DWI) are live");
    h->share_zero_streams = on != 0;
    DSD_CATCH
}

int dsd_params_ready(dsd_handle* h) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    for (const auto& p : h->params) DSD_CHECK(p.set, "parameter '%s' has not been set", p.name.c_str());
    DSD_CATCH
}

int dsd_plan(dsd_handle* h, int B, int C, int H, int W) {
    DSD_TRY
    DSD_CHECK(h && !h->is_block, "dsd_plan needs a model handle");
    set_device(h->device);
    DSD_CHECK(C == 2 || C == 4, "x must have 2 or 4 channels, got %d", C);
    DSD_CHECK(!h->is_disc || C == 4, "UNet_disc_Model takes 4 channels (x, T1, T2, DWI), got %d", C);
    net_plan(h, B, C, H, W, C == 2, 0, 0, 0);
    DSD_CATCH
}

int64_t dsd_workspace_bytes(dsd_handle* h) { return h && h->plan.valid ? (int64_t)h->plan.arena_bytes : -1; }

int64_t dsd_device_bytes(dsd_handle* h) {
    if (!h) return -1;
    return (int64_t)(h->slab_bytes + h->staging_bytes + h->arena_cap + net_piece_bytes(h) + h->tbuf_cap + h->mout_cap +
                     h->zplane_cap + h->dpm_m_cap + h->lat_in_cap + h->ctx_cap + h->y_cap + h->cfg_io_cap + h->plms_hist_cap + h->dpm_prog_cap + h->dpm_adapt_cap + h->bpd_cap + h->loss_cap);
}

int dsd_set_graph(dsd_handle* h, int on) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    h->use_graph = on != 0;
    if (!on) {
        set_device(h->device);
        net_drop_graph(h);
    }
    DSD_CATCH
}

int dsd_set_fuse_gn_stats(dsd_handle* h, int on) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (h->fuse_gn_stats != (on != 0)) {
        h->fuse_gn_stats = on != 0;
        h->plan.valid = false;
    }
    DSD_CATCH
}

int dsd_set_fuse_gn_apply(dsd_handle* h, int on) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (h->fuse_gn_apply != (on != 0)) {
        h->fuse_gn_apply = on != 0;
        h->plan.valid = false;
    }
    DSD_CATCH
}

int dsd_set_stream_lanes(dsd_handle* h, int on, int max_pixels) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    const int px = max_pixels > 0 ? max_pixels : h->lane_pixels;
    const int mode = on == 2 ? 2 : (on != 0);   // 2: the plan of the lanes (tile choices included), launched on ONE stream (tests)
    if (h->use_lanes != mode || h->lane_pixels != px) {
        h->use_lanes = mode;
        h->lane_pixels = px;
        h->plan.valid = false;   // the emission order of the plan (and what the arena may recycle) depends on it
        net_drop_graph(h);
    }
    DSD_CATCH
}

int dsd_set_winograd(dsd_handle* h, int on) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (h->use_winograd != (on != 0)) {
        h->use_winograd = on != 0;
        h->plan.valid = false;
    }
    DSD_CATCH
}

int dsd_set_vae_fused_attention(dsd_handle* h, int on) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (h->vae_fused_attention != (on != 0)) {
        h->vae_fused_attention = on != 0;
        h->plan.valid = false;
    }
    DSD_CATCH
}

int dsd_graph_stats(dsd_handle* h, int* captures, int* launches) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (captures) *captures = h->graph_captures;
    if (launches) *launches = h->graph_launches;
    DSD_CATCH
}

int dsd_set_slice_ids(dsd_handle* h, const int64_t* ids_host, int n) {
    DSD_TRY
    DSD_CHECK(h && (!h->is_block || h->block_kind == DSD_BLOCK_UNET || h->block_kind == DSD_BLOCK_DIT) && n >= 0 &&
                  (ids_host || n == 0), "bad argument");
    set_device(h->device);
    if (h->slice_ids) {
        DSD_HIP(hipDeviceSynchronize());
        DSD_HIP(hipFree(h->slice_ids));
        h->slice_ids = nullptr;
    }
    h->n_slice_ids = 0;
    if (n > 0) {
        for (int i = 0; i < n; ++i) DSD_CHECK(ids_host[i] >= 0, "slice id %d is negative", i);
        DSD_HIP(hipMalloc((void**)&h->slice_ids, (size_t)n * sizeof(int64_t)));
        DSD_HIP(hipMemcpy(h->slice_ids, ids_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
        h->n_slice_ids = n;
    }
    DSD_CATCH
}
int dsd_plan_launches(dsd_handle* h) { return h && h->plan.valid ? h->plan.launches : -1; }
double dsd_plan_flops(dsd_handle* h) { return h && h->plan.valid ? h->plan.flops : -1.0; }

int dsd_forward(dsd_handle* h, const float* x, const void* t, int t_is_float, int B, int C, int H, int W, float* out,
                float* const* feats, void* stream) {
    DSD_TRY
    DSD_CHECK(h && !h->is_block && x && t && out, "null argument");
    DSD_CHECK(!h->is_disc || C == 4, "UNet_disc_Model takes 4 channels (x, T1, T2, DWI), got %d", C);
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    net_plan(h, B, C, H, W, C == 2, feats != nullptr, 0, 0, 0, s);
    bind_planes(h, x, C, H, W, s);
    h->io.t = t;
    h->io.t_is_float = t_is_float;
    h->io.out = out;
    h->io.feats = feats;
    net_run(h, s);
    net_check_overflow(h, s);
    DSD_CATCH
}

int dsd_profile_enable(dsd_handle* h, int on) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    h->profiling = on != 0;
    if (on) {
        h->prof_names.clear();
        h->prof_runs = 0;
        h->prof_x_names.clear(); h->prof_x_ms.clear(); h->prof_x_bytes.clear(); h->prof_x_calls.clear();
    }
    DSD_CATCH
}

int dsd_profile_count(dsd_handle* h) { return h ? (int)(h->prof_names.size() + h->prof_x_names.size()) : -1; }

int dsd_profile_get(dsd_handle* h, int idx, const char** kind, double* total_ms, double* flops, double* bytes,
                    int64_t* calls, int* runs) {
    DSD_TRY
    DSD_CHECK(h && idx >= 0 && idx < dsd_profile_count(h), "profile index out of range");
    if (idx >= (int)h->prof_names.size()) {   // the records behind the plan's kinds (dsd_eval_loss)
        const size_t j = (size_t)idx - h->prof_names.size();
        if (kind) *kind = h->prof_x_names[j].c_str();
        if (total_ms) *total_ms = h->prof_x_ms[j];
        if (flops) *flops = 0.0;
        if (bytes) *bytes = h->prof_x_bytes[j];
        if (calls) *calls = h->prof_x_calls[j];
        if (runs) *runs = h->prof_runs;
        return 0;
    }
    if (kind) *kind = h->prof_names[idx].c_str();
    if (total_ms) *total_ms = h->prof_ms[idx];
    if (flops) *flops = h->prof_flops[idx];
    if (bytes) *bytes = h->prof_bytes[idx];
    if (calls) *calls = h->prof_calls[idx];
    if (runs) *runs = h->prof_runs;
    DSD_CATCH
}

int dsd_profile_op_count(dsd_handle* h) { return h ? (int)h->prof_op_ms.size() : -1; }

int dsd_profile_op_get(dsd_handle* h, int idx, const char** kind, double* ms, double* flops, double* bytes) {
    DSD_TRY
    DSD_CHECK(h && idx >= 0 && idx < (int)h->prof_op_ms.size() && h->prof_op_ms.size() == h->plan.ops.size(),
              "op index out of range (or the plan changed since the profiled forward)");
    if (kind) *kind = h->plan.kind_names[h->plan.op_kind[idx]].c_str();
    if (ms) *ms = h->prof_op_ms[idx];
    if (flops) *flops = h->plan.op_flops[idx];
    if (bytes) *bytes = h->plan.op_bytes[idx];
    DSD_CATCH
}

int dsd_profile_op_name(dsd_handle* h, int idx, const char** name) {
    DSD_TRY
    DSD_CHECK(h && name && idx >= 0 && idx < (int)h->plan.op_name.size(), "op index out of range");
    *name = h->plan.op_name[idx].c_str();
    DSD_CATCH
}

int dsd_set_conditioning(dsd_handle* h, const dsd_conditioning* c) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (!c) {
        h->cond = dsd_conditioning{};
        h->has_cond = false;
    } else {
        DSD_CHECK(h->is_block, "the four-stream model takes 'concat' conditioning only: no context or y reaches DSUnetModel.forward");
        DSD_CHECK(h->block_kind != DSD_BLOCK_DIT,
                  "the DiT takes 'concat' conditioning only in the device loops: no context or y reaches it through DiffusionWrapper");
        DSD_CHECK(h->block_kind == DSD_BLOCK_UNET, "dsd_set_conditioning takes a DSD_BLOCK_UNET handle, got block kind %d", h->block_kind);
        DSD_CHECK(c->B >= 1 && c->tokens >= 0 && c->y_width >= 0, "bad conditioning: B %d tokens %d y_width %d", c->B, c->tokens, c->y_width);
        DSD_CHECK(!c->context || c->tokens >= 1, "a context needs tokens >= 1, got %d", c->tokens);
        DSD_CHECK(c->context || !c->context_uncond, "context_uncond without a context");
        DSD_CHECK(c->y || !c->y_uncond, "y_uncond without y");
        h->cond = *c;
        h->has_cond = true;
    }
    DSD_CATCH
}

int dsd_set_trace(dsd_handle* h, const dsd_trace* t) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (t) {   // checked whole before the handle changes: a rejected trace leaves the installed one in place
        DSD_CHECK(t->n_keep >= 1, "trace: n_keep is %d; a trace keeps at least one iteration (NULL clears it)", t->n_keep);
        DSD_CHECK(t->keep, "trace: keep is null");
        DSD_CHECK(t->x || t->pred_x0, "trace: both buffers are NULL (x and pred_x0); nothing would be written");
        DSD_CHECK(t->keep[0] >= 0, "trace: keep[0] = %d is out of range; iterations start at 0", t->keep[0]);
        for (int j = 1; j < t->n_keep; ++j)
            DSD_CHECK(t->keep[j] > t->keep[j - 1], "trace: keep is not strictly ascending (unsorted or repeated): keep[%d] = %d after keep[%d] = %d",
                      j, t->keep[j], j - 1, t->keep[j - 1]);
        h->trace_keep.assign(t->keep, t->keep + t->n_keep);
        h->trace_x = t->x;
        h->trace_x0 = t->pred_x0;
    } else {
        h->trace_keep.clear();
        h->trace_x = h->trace_x0 = nullptr;
    }
    h->has_trace = t != nullptr;
    DSD_CATCH
}

int dsd_set_disentangle(dsd_handle* h, const dsd_disentangle* d) {
    DSD_TRY
    DSD_CHECK(h, "null handle");
    if (d) {   // checked whole before the handle changes, as a trace is
        DSD_CHECK(d->mode >= DSD_CONTRAST_CL && d->mode <= DSD_CONTRAST_EU_CL,
                  "disentangle: unknown mode %d (DSD_CONTRAST_CL / _EU / _EU_CL; training_losses has no L1 form)", d->mode);
        DSD_CHECK(d->mode == DSD_CONTRAST_EU || (d->temperature_cs > 0.f && d->temperature_sal > 0.f),
                  "disentangle: the cosine modes divide by the temperatures, got %g and %g", (double)d->temperature_cs, (double)d->temperature_sal);
        DSD_CHECK(d->labels_cs && d->labels_sal && d->loss && d->logits_cs && d->logits_sal,
                  "disentangle: null argument (labels_cs %p labels_sal %p loss %p logits_cs %p logits_sal %p)", (void*)d->labels_cs,
                  (void*)d->labels_sal, (void*)d->loss, (void*)d->logits_cs, (void*)d->logits_sal);
        DSD_CHECK(d->n_labels_cs >= 1 && d->n_labels_sal >= 1, "disentangle: %d and %d labels", d->n_labels_cs, d->n_labels_sal);
        h->disen = *d;
    } else {
        h->disen = dsd_disentangle{};
    }
    h->has_disen = d != nullptr;
    DSD_CATCH
}

int dsd_block_forward(dsd_handle* h, const float* x, int B, int C, int H, int W, const float* aux, int aux_len,
                      const float* aux2, int aux_len2, float* out, void* stream) {
    DSD_TRY
    DSD_CHECK(h && h->is_block && x && out, "null argument / not a block handle");
    set_device(h->device);
    const void* y = nullptr;
    if (h->block_kind == DSD_BLOCK_UNET) {   // label_emb: y comes through dsd_set_conditioning
        int lk = 0, lw = 0;
        net_unet_label_emb(h, &lk, &lw);
        const bool has_y = h->has_cond && h->cond.y;
        DSD_CHECK(has_y == (lk != 0), lk ? "UNetModel with label_emb: y is missing (dsd_set_conditioning)"
                                         : "UNetModel without label_emb takes no y");
        if (lk) {
            check_y(h, h->cond, lk, lw, B);
            y = h->cond.y;
        }
    }
    net_plan(h, B, C, H, W, 0, 0, aux ? aux_len : 0, aux2 ? aux_len2 : 0, 0, (hipStream_t)stream);
    h->io.x_nchw = x;
    h->io.aux = aux;
    h->io.aux2 = aux2;
    h->io.aux3 = y;
    h->io.out = out;
    net_run(h, (hipStream_t)stream);
    net_check_overflow(h, (hipStream_t)stream);
    DSD_CATCH
}

}  // extern "C"

namespace {

// ------------------------------------------------------------------------------------------- device sampling loops
// Every loop is: the checks of the call (all of them before any device work, so a rejected call leaves the state untouched), a
// LoopBinding (where the state lives), a step_range, run_loop with the sampler's step body, finish.
struct LoopBinding {
    float* xs = nullptr;            // the state the loop works on: row b at xs + b*x_bs, rows [0,B) (+ [B,2B) when guided)
    int64_t x_bs = 0;
    int B = 0, rows = 0, Cz = 1;    // rows = B, or 2B under classifier-free guidance (uncond half first)
    int64_t hw = 0;
    const float* out_u = nullptr;   // the halves of mout: uncond rows (null when unguided), cond rows
    const float* out_c = nullptr;
    const int64_t* ids = nullptr;   // slice ids keying the Philox noise, or null
    float* x = nullptr;             // the caller's state: receives rows [0,B) in finish unless the loop ran on it (xs == x)
    bool latent = false;            // xs is lat_in (strided rows) rather than x / cfg_io
    int64_t n() const { return Cz * hw; }
};

struct Range { int k0, k1; };
Range step_range(int first_step, int n_steps, int steps) {
    const int k0 = first_step < 0 ? 0 : first_step;
    return {k0, n_steps <= 0 ? steps : std::min(steps, k0 + n_steps)};
}

void check_slice_ids(const dsd_handle* h, int B) {
    DSD_CHECK(h->n_slice_ids == 0 || h->n_slice_ids == B, "dsd_set_slice_ids gave %d ids but the batch has %d slices", h->n_slice_ids, B);
}

// the four-stream denoiser (DSUnetModel): a one-channel state beside 1 or 3 condition planes
void check_four_stream(dsd_handle* h, const float* cond, int Cc, const float* x, int Cz, int B, int H, int W) {
    DSD_CHECK(cond && x, "null argument");
    DSD_CHECK(Cz == 1, "the four-stream model denoises a state of %d channel (the denoised image has one channel), got Cz = %d", 1, Cz);
    DSD_CHECK(!h->is_disc || Cc == 3, "UNet_disc_Model takes 3 condition planes (t1, t2, dwi) behind the state, got Cc = %d (%d input channels, 4 needed)",
              Cc, Cc + 1);
    DSD_CHECK(Cc == 1 || Cc == 3, "cond must have 1 or 3 channels, got %d", Cc);
    DSD_CHECK(B >= 1 && H >= 1 && W >= 1, "bad shape: B %d H %d W %d", B, H, W);
    check_slice_ids(h, B);
}

// the state-in-input denoisers on a Cz-channel latent state with a 'concat' conditioning of Cc channels: the plain UNetModel
// (DSD_BLOCK_UNET) or the DiT (DSD_BLOCK_DIT: square input of input_size, no labels — through DiffusionWrapper none reaches it,
// DiT_models.py:245-249 — and Cc = 0 for an unconditional one).  want_ch: the output channels the sampler reads, Cz or (learned
// range) 2*Cz.  Returns the handle's output channel count, the row stride of mout in planes: the UNetModel's equals want_ch; the
// DiT's (in_channels // 3 * 2 with learn_sigma, sic) is Cz or 2*Cz, and a sampler without learned variance ignores the second
// half (gaussian_diffusion.py:484-485).
bool is_dit(const dsd_handle* h) { return h->is_block && h->block_kind == DSD_BLOCK_DIT; }

int check_latent(dsd_handle* h, const dsd_guidance* g, const float* cond, int Cc, const float* x, int Cz, int B, int H, int W,
                 int want_ch) {
    if (is_dit(h)) {
        DSD_CHECK(x && (cond || Cc == 0), "null argument");
        const std::vector<int32_t>& a = h->iargs;   // input_size, patch_size, in_channels, ..., learn_sigma at [8] (net.cpp DitCfg)
        const int out_ch = a[8] ? a[2] / 3 * 2 : a[2];
        DSD_CHECK(Cz >= 1 && Cc >= 0 && B >= 1 && H >= 1 && W >= 1, "bad shape: Cz %d Cc %d B %d H %d W %d", Cz, Cc, B, H, W);
        DSD_CHECK(!g || Cc >= 1, "guidance needs a 'concat' conditioning to replace (Cc = %d)", Cc);
        DSD_CHECK(a[2] == Cz + Cc, "the DiT takes %d input channels but state + conditioning have %d + %d", a[2], Cz, Cc);
        DSD_CHECK(H == a[0] && W == a[0], "the DiT takes %dx%d inputs (input_size) but the state is %dx%d", a[0], a[0], H, W);
        DSD_CHECK(out_ch == Cz || out_ch == 2 * Cz,
                  "the DiT has %d output channels but a state of %d channels needs %d, or %d with a learned variance", out_ch, Cz, Cz,
                  2 * Cz);
        DSD_CHECK(want_ch <= out_ch, "a learned-range variance needs %d output channels (2 per state channel) but the DiT has %d",
                  want_ch, out_ch);
        check_slice_ids(h, B);
        return out_ch;
    }
    DSD_CHECK(x, "null argument");
    DSD_CHECK(h->block_kind == DSD_BLOCK_UNET, "the latent loops take a DSD_BLOCK_UNET handle (the plain UNetModel)");
    const std::vector<int32_t>& a = h->iargs;
    DSD_CHECK(Cz >= 1 && Cc >= 0 && B >= 1 && H >= 1 && W >= 1, "bad shape: Cz %d Cc %d B %d H %d W %d", Cz, Cc, B, H, W);
    // the bundle of dsd_set_conditioning against the handle (context <-> spatial transformer, y <-> label_emb)
    const dsd_conditioning none{};
    const dsd_conditioning& c = h->has_cond ? h->cond : none;
    const int ctx_dim = net_unet_context_dim(h);
    int lk = 0, lw = 0;
    net_unet_label_emb(h, &lk, &lw);
    DSD_CHECK(!ctx_dim || c.context, "the UNetModel has a spatial transformer (context_dim %d) but no context is set (dsd_set_conditioning)",
              ctx_dim);
    DSD_CHECK(ctx_dim || !c.context, "a context of %d tokens is set but the UNetModel has no spatial transformer", c.tokens);
    DSD_CHECK(!lk || c.y, "the UNetModel has a label_emb (kind %d, width %d) but no y is set (dsd_set_conditioning)", lk, lw);
    DSD_CHECK(lk || !c.y, "a y of width %d is set but the UNetModel has no label_emb", c.y_width);
    DSD_CHECK(!h->has_cond || c.B == B, "the conditioning was set for a batch of %d but the call has %d", c.B, B);
    if (lk) check_y(h, c, lk, lw, B);
    DSD_CHECK(cond || Cc == 0, "null argument: cond with Cc = %d", Cc);
    if (g) {
        DSD_CHECK(Cc >= 1 || c.context || c.y, "guidance needs a 'concat' conditioning to replace (Cc = %d)", Cc);
        DSD_CHECK(Cc == 0 || g->uncond, "guidance needs the unconditional conditioning (uncond is null)");
        DSD_CHECK(!c.context || c.context_uncond, "guidance needs the unconditional twin of the context (context_uncond is null, %d tokens)",
                  c.tokens);
        DSD_CHECK(!c.y || c.y_uncond, "guidance needs the unconditional twin of y (y_uncond is null, y_width %d)", c.y_width);
    }
    DSD_CHECK(a[0] == Cz + Cc, "the UNetModel takes %d input channels but state + conditioning have %d + %d", a[0], Cz, Cc);
    DSD_CHECK(a[2] == want_ch, "the UNetModel has %d output channels but the sampler expects %d", a[2], want_ch);
    check_slice_ids(h, B);
    return want_ch;
}

LoopBinding make_binding(dsd_handle* h, const dsd_guidance* g, float* xs, int64_t x_bs, float* x, int Cz, int B, int64_t hw,
                         int out_ch) {
    LoopBinding b;
    b.xs = xs; b.x_bs = x_bs; b.x = x;
    b.B = B; b.rows = g ? 2 * B : B; b.Cz = Cz; b.hw = hw;
    b.out_u = g ? h->mout : nullptr;
    b.out_c = g ? h->mout + (size_t)B * out_ch * hw : h->mout;
    b.ids = h->n_slice_ids == B ? h->slice_ids : nullptr;
    return b;
}

// The four-stream model reads planes in place (DiffusionWrapper 'concat', ddpm.py:1331-1333, without materialising the cat):
// unguided the caller's x and cond; guided (ddim.py:197-218) the 2B-row planes of cfg_io — state [2B,1,H,W] then conditions
// [2B,Cc,H,W] = cat([uncond, cond]) — whose step-invariant halves are copied once per call.
LoopBinding bind_four_stream(dsd_handle* h, const dsd_guidance* g, const float* cond, int Cc, float* x, int B, int H, int W,
                             int out_ch, hipStream_t s, int want_feats = 0) {
    const int64_t hw = (int64_t)H * W;
    const int rows = g ? 2 * B : B;
    // (kept head tensors, dsd_set_disentangle: build_unet refuses zero-stream sharing beside features)
    net_plan(h, rows, Cc + 1, H, W, Cc == 1, want_feats, 0, 0, (Cc == 1 && (g || B > 1) && !want_feats) ? h->share_zero_streams : 0, s);
    ensure_buf(&h->tbuf, &h->tbuf_cap, (size_t)rows * sizeof(float));
    ensure_buf(&h->mout, &h->mout_cap, (size_t)rows * out_ch * hw * sizeof(float));
    float* xs = x;
    if (g) {
        ensure_buf(&h->cfg_io, &h->cfg_io_cap, (size_t)2 * B * (1 + Cc) * hw * sizeof(float));
        xs = h->cfg_io;
        float* cs = xs + (size_t)2 * B * hw;
        const size_t xb = (size_t)B * hw * sizeof(float), cb = xb * Cc;
        DSD_HIP(hipMemcpyAsync(xs, x, xb, hipMemcpyDeviceToDevice, s));
        DSD_HIP(hipMemcpyAsync(xs + (size_t)B * hw, x, xb, hipMemcpyDeviceToDevice, s));
        DSD_HIP(hipMemcpyAsync(cs, g->uncond, cb, hipMemcpyDeviceToDevice, s));
        DSD_HIP(hipMemcpyAsync(cs + (size_t)B * Cc * hw, cond, cb, hipMemcpyDeviceToDevice, s));
        cond = cs;
    }
    h->io.plane[0] = xs;
    h->io.plane_bs[0] = hw;
    h->io.plane[1] = cond;
    h->io.plane_bs[1] = (int64_t)Cc * hw;
    if (Cc == 1) {
        ensure_buf(&h->zplane, &h->zplane_cap, (size_t)hw * sizeof(float));
        DSD_HIP(hipMemsetAsync(h->zplane, 0, (size_t)hw * sizeof(float), s));
        h->io.plane[2] = h->io.plane[3] = h->zplane;
        h->io.plane_bs[2] = h->io.plane_bs[3] = 0;
    } else {
        h->io.plane[2] = cond + hw;
        h->io.plane[3] = cond + 2 * hw;
        h->io.plane_bs[2] = h->io.plane_bs[3] = (int64_t)Cc * hw;
    }
    h->io.t = h->tbuf;
    h->io.t_is_float = 1;
    h->io.out = h->mout;
    h->io.feats = nullptr;
    return make_binding(h, g, xs, hw, x, 1, B, hw, out_ch);
}

// The state x [B,Cz,h,w] is copied once into channels [0,Cz) of the UNetModel's persistent NCHW input lat_in [rows,Cz+Cc,h,w]
// and the conditioning into channels [Cz,Cz+Cc) (guided: x_in = cat([x]*2), c_in = cat([uncond, cond])); every update then reads
// and writes the state in place there, so the next network evaluation reads x_{t-1} with no concatenation and no copy.
LoopBinding bind_latent(dsd_handle* h, const dsd_guidance* g, const float* cond, int Cc, float* x, int Cz, int B, int H, int W,
                        int out_ch, hipStream_t s) {
    const int64_t hw = (int64_t)H * W, Cin = Cz + Cc;
    const int rows = g ? 2 * B : B;
    const dsd_conditioning none{};
    const dsd_conditioning& c = h->has_cond ? h->cond : none;
    const int tokens = c.context ? c.tokens : 0;
    net_plan(h, rows, (int)Cin, H, W, 0, 0, 1, tokens, 0, s);
    ensure_buf(&h->tbuf, &h->tbuf_cap, (size_t)rows * sizeof(float));
    ensure_buf(&h->mout, &h->mout_cap, (size_t)rows * out_ch * hw * sizeof(float));
    ensure_buf(&h->lat_in, &h->lat_in_cap, (size_t)rows * Cin * hw * sizeof(float));
    const size_t row = (size_t)Cin * hw * sizeof(float);
    for (int half = 0; half * B < rows; ++half) {
        float* dst = h->lat_in + (size_t)half * B * Cin * hw;
        DSD_HIP(hipMemcpy2DAsync(dst, row, x, (size_t)Cz * hw * sizeof(float), (size_t)Cz * hw * sizeof(float), B,
                                 hipMemcpyDeviceToDevice, s));
        if (Cc)
            DSD_HIP(hipMemcpy2DAsync(dst + Cz * hw, row, (g && half == 0) ? g->uncond : cond, (size_t)Cc * hw * sizeof(float),
                                     (size_t)Cc * hw * sizeof(float), B, hipMemcpyDeviceToDevice, s));
    }
    h->io = IO();
    h->io.x_nchw = h->lat_in;
    h->io.aux = h->tbuf;
    h->io.out = h->mout;
    // context and y: copied once into `rows` rows of the handle's own (c_in = cat([uncond, cond]) part by part, ddim.py:199-217)
    if (c.context) {
        const size_t half_bytes = (size_t)B * tokens * net_unet_context_dim(h) * sizeof(float);
        ensure_buf(&h->ctx_buf, &h->ctx_cap, rows / B * half_bytes);
        for (int half = 0; half * B < rows; ++half)
            DSD_HIP(hipMemcpyAsync(reinterpret_cast<char*>(h->ctx_buf) + half * half_bytes, (g && half == 0) ? c.context_uncond : c.context,
                                   half_bytes, hipMemcpyDeviceToDevice, s));
        h->io.aux2 = h->ctx_buf;
    }
    if (c.y) {
        const size_t half_bytes = (size_t)B * (c.y_width ? c.y_width * sizeof(float) : sizeof(long long));
        ensure_buf(&h->y_buf, &h->y_cap, rows / B * half_bytes);
        for (int half = 0; half * B < rows; ++half)
            DSD_HIP(hipMemcpyAsync(reinterpret_cast<char*>(h->y_buf) + half * half_bytes, (g && half == 0) ? c.y_uncond : c.y, half_bytes,
                                   hipMemcpyDeviceToDevice, s));
        h->io.aux3 = h->y_buf;
    }
    LoopBinding b = make_binding(h, g, h->lat_in, Cin * hw, x, Cz, B, hw, out_ch);
    b.latent = true;
    return b;
}

// The handle picks the denoiser: a block handle reads the state from its own input (UNetModel / DiT, a Cz-channel state), a model
// handle is the four-stream model (Cz = 1).  Every loop rejects a null handle with this before anything else.
bool state_in_input(const dsd_handle* h) {
    DSD_CHECK(h, "null argument");
    return h->is_block;
}

// want_ch: the output channels the sampler reads; returns the channels one output row holds (the four-stream callers check theirs).
int check_denoiser(dsd_handle* h, const dsd_guidance* g, const float* cond, int Cc, const float* x, int Cz, int B, int H, int W,
                   int want_ch) {
    if (state_in_input(h)) return check_latent(h, g, cond, Cc, x, Cz, B, H, W, want_ch);
    check_four_stream(h, cond, Cc, x, Cz, B, H, W);
    return want_ch;
}

// want_feats (four-stream handles): net_plan's — 2 keeps UNet_disc_Model's bottleneck tensors, or DSUnetModel's ten head tensors,
// in the workspace (dsd_eval_loss)
LoopBinding bind_denoiser(dsd_handle* h, const dsd_guidance* g, const float* cond, int Cc, float* x, int Cz, int B, int H, int W,
                          int out_ch, hipStream_t s, int want_feats = 0) {
    return state_in_input(h) ? bind_latent(h, g, cond, Cc, x, Cz, B, H, W, out_ch, s)
                             : bind_four_stream(h, g, cond, Cc, x, B, H, W, out_ch, s, want_feats);
}

// iterations [r.k0, r.k1): pre(k) in front of the network evaluation at time t[k] (through the cached graph), step(k) after it
template <class Pre, class Step>
void run_loop(dsd_handle* h, const LoopBinding& b, const float* t, Range r, hipStream_t s, Pre&& pre, Step&& step) {
    for (int k = r.k0; k < r.k1; ++k) {
        pre(k);
        fill_t(h->tbuf, b.rows, t[k], s);
        net_run_cached(h, s);
        step(k);
    }
}

void finish(dsd_handle* h, const LoopBinding& b, hipStream_t s) {
    const size_t sample = (size_t)b.n() * sizeof(float);
    if (b.latent)
        DSD_HIP(hipMemcpy2DAsync(b.x, sample, b.xs, (size_t)b.x_bs * sizeof(float), sample, b.B, hipMemcpyDeviceToDevice, s));
    else if (b.xs != b.x)
        DSD_HIP(hipMemcpyAsync(b.x, b.xs, b.B * sample, hipMemcpyDeviceToDevice, s));
    net_check_overflow(h, s);
}

// dsd_set_trace as one loop call sees it.  The loop asks for iteration k's slots in ascending k, so `j` only moves forward; with
// no trace installed every slot is null and the loop launches what it launches without one.
struct Trace {
    const dsd_handle* h;
    size_t plane;                   // B*Cz*H*W: one entry of either buffer
    size_t j = 0;
    Trace(const dsd_handle* h_, const LoopBinding& b) : h(h_), plane((size_t)b.B * b.n()) {}
    bool kept(int k) {
        if (!h->has_trace) return false;
        while (j < h->trace_keep.size() && h->trace_keep[j] < k) ++j;
        return j < h->trace_keep.size() && h->trace_keep[j] == k;
    }
    // where the update kernel of iteration k writes its pred_x0 (it forms the value anyway), or null
    float* x0_slot(int k) { return h->trace_x0 && kept(k) ? h->trace_x0 + j * plane : nullptr; }
    // the B logical rows of the state after iteration k, dense, whatever row stride the binding keeps them at (under guidance the
    // first half of the 2B rows; the update wrote both)
    void state(int k, const LoopBinding& b, hipStream_t s) {
        if (!h->trace_x || !kept(k)) return;
        const size_t sample = (size_t)b.n() * sizeof(float);
        DSD_HIP(hipMemcpy2DAsync(h->trace_x + j * plane, sample, b.xs, (size_t)b.x_bs * sizeof(float), sample, b.B,
                                 hipMemcpyDeviceToDevice, s));
    }
};

void check_trace(const dsd_handle* h, int steps) {
    if (!h->has_trace) return;
    DSD_CHECK(h->trace_keep.back() < steps, "trace: keep[%d] = %d is out of range; the schedule executes iterations 0..%d",
              (int)h->trace_keep.size() - 1, h->trace_keep.back(), steps - 1);
}

// the loops that hand out no intermediates through a trace say so instead of ignoring one
void refuse_trace(const dsd_handle* h, const char* loop) {
    DSD_CHECK(!h->has_trace, "%s does not honour a trace (dsd_set_trace): dsd_sample and dsd_sample_plms do; clear it with "
              "dsd_set_trace(h, NULL) before this call", loop);
}

StepCoef step_coef(const dsd_schedule* sc, int k) {
    StepCoef c{};
    for (int j = 0; j < DSD_NCOEF; ++j) c.c[j] = sc->coef[(size_t)k * DSD_NCOEF + j];
    c.mode = sc->mode; c.pred = sc->pred; c.learned_range = sc->learned_range; c.clip = sc->clip_denoised;
    c.nonzero = sc->nonzero ? sc->nonzero[k] : 1;
    c.eta = sc->eta;
    return c;
}

void check_schedule(const dsd_schedule* sc) {
    DSD_CHECK(sc && sc->coef && sc->t_model && sc->steps >= 1, "bad schedule");
    DSD_CHECK(sc->mode != DSD_MODE_B_PLMS,
              "DSD_MODE_B_PLMS carries a history of noise predictions across iterations: it runs in dsd_sample_plms only");
    DSD_CHECK(sc->mode >= DSD_MODE_A_DDPM && sc->mode <= DSD_MODE_B_DDIM, "unknown sampler mode %d", sc->mode);
    DSD_CHECK(sc->pred >= DSD_PRED_EPS && sc->pred <= DSD_PRED_V, "unknown prediction type %d", sc->pred);
    DSD_CHECK(!(sc->learned_range && sc->mode >= DSD_MODE_B_DDPM), "learned-range variance exists only in the guided-diffusion family");
}

// Classifier-free guidance (ddim.py:194-219 / dpm_solver_pytorch.py:324-332): both halves in ONE network pass over 2B rows (uncond
// half first), combined by the update kernels (sampler.hip), which write x_{t-1} to both state rows.  Noise and slice ids stay per
// logical sample.
// need_uncond: false where a latent call has no 'concat' part (Cc = 0) and a dsd_set_conditioning bundle carries what is replaced
void check_guidance(const dsd_guidance* g, int steps, bool need_uncond = true) {
    DSD_CHECK(g->uncond || !need_uncond, "guidance needs the unconditional conditioning (uncond is null)");
    DSD_CHECK(g->scale && g->n_scale == steps, "guidance carries %d scales but the schedule executes %d steps (one scale per step)",
              g->scale ? g->n_scale : 0, steps);
}

void check_guided_schedule(const dsd_schedule* sc) {   // after check_schedule
    DSD_CHECK(!sc->learned_range, "classifier-free guidance does not take a learned-range variance (learned_range is set)");
    DSD_CHECK(sc->mode == DSD_MODE_B_DDIM,
              "classifier-free guidance exists only in the DDIM loop of the LDM family (DSD_MODE_B_DDIM); the reference has none in "
              "mode %d", sc->mode);
}

void check_mask(const dsd_inpaint* inp, int Cz) {
    DSD_CHECK(inp && inp->mask, "masked sampling needs a mask (mask is null)");
    DSD_CHECK(inp->x0, "a mask needs the image it keeps (x0 is null)");
    DSD_CHECK(inp->mask_channels == 1 || inp->mask_channels == Cz, "the mask has %d channels; 1 or the state's %d are taken",
              inp->mask_channels, Cz);
}

void blend_step(const dsd_schedule* sc, int k, const dsd_inpaint* inp, const LoopBinding& b, uint64_t seed, hipStream_t s) {
    const float* c = sc->coef + (size_t)k * DSD_NCOEF;
    q_sample_blend(c[0], c[1], nullptr, nullptr, inp->x0, inp->mask, inp->mask_channels, b.xs,
                   inp->noise ? inp->noise + (size_t)k * b.B * b.n() : nullptr, seed, (uint64_t)k, b.B, b.Cz, (int)b.hw, s, b.x_bs,
                   b.out_u != nullptr, b.ids);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------- DDPM / DDIM
// dsd_sample: the fused update after every evaluation; guided (g) in DSD_MODE_B_DDIM; masked (inp): ddim.py:160-163 blends in front
// of every network evaluation, ddpm.py:1085-1087 after every update.
int dsd_sample(dsd_handle* h, const dsd_schedule* sc, const dsd_guidance* g, const dsd_inpaint* inp, const float* cond, int Cc,
               float* x, int Cz, const float* noise, uint64_t seed, int B, int H, int W, int first_step, int n_steps, void* stream) {
    DSD_TRY
    const bool latent = state_in_input(h);
    if (inp) check_mask(inp, Cz);
    check_schedule(sc);
    if (inp) {
        DSD_CHECK(sc->mode == DSD_MODE_B_DDPM || sc->mode == DSD_MODE_B_DDIM,
                  "masked sampling exists only in the loops of the LDM family (DSD_MODE_B_DDPM / DSD_MODE_B_DDIM); the reference has no "
                  "mask in mode %d", sc->mode);
        DSD_CHECK(!(g && sc->mode == DSD_MODE_B_DDPM), "the masked DDPM loop (DSD_MODE_B_DDPM) has no guidance in the reference");
    }
    if (g) {
        check_guided_schedule(sc);
        check_guidance(g, sc->steps, !(latent && Cc == 0 && h->has_cond));
    }
    DSD_CHECK(!(sc->learned_range && Cz > 1) || is_dit(h),
              "learned-range variance needs one state channel (the model output interleaves mean and variance per sample); Cz = %d", Cz);
    const int want_ch = (sc->learned_range ? 2 : 1) * Cz;
    const int out_ch = check_denoiser(h, g, cond, Cc, x, Cz, B, H, W, want_ch);
    DSD_CHECK(latent || h->cfg.out_channels == out_ch, "model has %d output channels but the schedule expects %d", h->cfg.out_channels,
              out_ch);
    check_trace(h, sc->steps);
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    const LoopBinding b = bind_denoiser(h, g, cond, Cc, x, Cz, B, H, W, out_ch, s);
    const bool blend_first = inp && sc->mode == DSD_MODE_B_DDIM, blend_last = inp && !blend_first;
    Trace tr(h, b);   // x after the update and (B_DDPM, ddpm.py:1085-1090) its blend; pred_x0 straight from the update kernel
    run_loop(h, b, sc->t_model, step_range(first_step, n_steps, sc->steps), s,
             [&](int k) {
                 if (blend_first) blend_step(sc, k, inp, b, seed, s);
             },
             [&](int k) {
                 sampler_update(step_coef(sc, k), b.out_u, b.out_c, g ? g->scale[k] : 1.f, b.xs,
                                noise ? noise + (size_t)k * B * b.n() : nullptr, seed, (uint64_t)k, B, (int)b.hw, s, tr.x0_slot(k), b.ids,
                                Cz, b.x_bs, out_ch * b.hw);
                 if (blend_last) blend_step(sc, k, inp, b, seed, s);
                 tr.state(k, b, s);
             });
    finish(h, b, s);
    DSD_CATCH
}

int dsd_op_sampler_update(const dsd_schedule* sc, int k, const float* model_out, float* x, const float* noise,
                          uint64_t philox_seed, int B, int H, int W, float* pred_xstart, void* stream) {
    DSD_TRY
    check_schedule(sc);
    DSD_CHECK(k >= 0 && k < sc->steps && model_out && x, "bad argument");
    sampler_update(step_coef(sc, k), nullptr, model_out, 1.f, x, noise, philox_seed, (uint64_t)k, B, H * W, (hipStream_t)stream,
                   pred_xstart);
    DSD_CATCH
}

static void check_op_state(int B, int Cz, int H, int W, int64_t x_row_stride) {
    DSD_CHECK(B >= 1 && Cz >= 1 && H >= 1 && W >= 1, "bad shape: B %d Cz %d H %d W %d", B, Cz, H, W);
    DSD_CHECK(x_row_stride == 0 || x_row_stride >= (int64_t)Cz * H * W, "x_row_stride %lld is smaller than one sample (%lld)",
              (long long)x_row_stride, (long long)Cz * H * W);
}

int dsd_op_sampler_update_guided(const dsd_schedule* sc, int k, const float* out_uncond, const float* out_cond, float scale,
                                 float* x, int64_t x_row_stride, const float* noise, uint64_t philox_seed, int B, int Cz, int H,
                                 int W, float* pred_xstart, void* stream) {
    DSD_TRY
    check_schedule(sc);
    check_guided_schedule(sc);
    DSD_CHECK(k >= 0 && k < sc->steps && out_uncond && out_cond && x, "bad argument");
    check_op_state(B, Cz, H, W, x_row_stride);
    sampler_update(step_coef(sc, k), out_uncond, out_cond, scale, x, noise, philox_seed, (uint64_t)k, B, H * W, (hipStream_t)stream,
                   pred_xstart, nullptr, Cz, x_row_stride);
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- DPM-Solver(++)
static void check_dpm_schedule(const dsd_dpm_schedule* sc) {
    DSD_CHECK(sc && sc->steps > 0 && sc->coef && sc->t_input && sc->order, "bad DPM schedule");
    DSD_CHECK(sc->pred >= DSD_PRED_EPS && sc->pred <= DSD_PRED_V, "bad pred %d", sc->pred);
    for (int k = 0; k < sc->steps; ++k) {
        DSD_CHECK(sc->order[k] >= 0 && sc->order[k] <= 2, "order[%d] = %d: the multistep solver is built for order <= 2", k,
                  sc->order[k]);
        DSD_CHECK(!(k == 0 && sc->order[k] == 2), "the first update cannot be second order");
    }
    DSD_CHECK(!sc->thresholding || (sc->threshold_ratio >= 0.f && sc->threshold_ratio <= 1.f), "threshold_ratio outside [0,1]");
}

static DpmCoef dpm_coef(const dsd_dpm_schedule* sc, int k) {
    const float* c = sc->coef + (size_t)k * DSD_NCOEF;
    DpmCoef d;
    d.alpha = c[0]; d.sigma = c[1]; d.cx = c[2]; d.cm = c[3]; d.cd = c[4]; d.ir0 = c[5];
    d.order = sc->order[k];
    d.pred = sc->pred;
    d.data_pred = sc->data_pred || d.order == 0;
    d.thresh = sc->thresholding;
    return d;
}

// One sample = all Cz*h*w elements: the dynamic-thresholding quantile is per sample over C*h*w (sampler.py:379-388).  The
// four-stream model and the DiT may carry a learned sigma in a second half of the output channels, which the solver ignores.
int dsd_sample_dpm(dsd_handle* h, const dsd_dpm_schedule* sc, const dsd_guidance* g, const float* cond, int Cc, float* x, int Cz,
                   int B, int H, int W, void* stream) {
    DSD_TRY
    const bool latent = state_in_input(h);
    refuse_trace(h, "dsd_sample_dpm");
    check_dpm_schedule(sc);
    if (g) check_guidance(g, sc->steps, !(latent && Cc == 0 && h->has_cond));
    const int out_ch = check_denoiser(h, g, cond, Cc, x, Cz, B, H, W, Cz);
    const int Cm = latent ? out_ch / Cz : h->cfg.out_channels;   // an output row is Cm samples long; the solver reads the first
    DSD_CHECK(Cm == 1 || Cm == 2, "model has %d output channels; the solver takes 1 (or 2 with a learned sigma)", Cm);
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    const LoopBinding b = bind_denoiser(h, g, cond, Cc, x, Cz, B, H, W, Cm * Cz, s);
    const size_t plane = (size_t)B * b.n();
    ensure_buf(&h->dpm_m, &h->dpm_m_cap, (2 * plane + B) * sizeof(float));
    float *m_cur = h->dpm_m, *m_prev = h->dpm_m + plane, *s_buf = h->dpm_m + 2 * plane;
    run_loop(h, b, sc->t_input, Range{0, sc->steps}, s, [](int) {}, [&](int k) {
        dpm_step(dpm_coef(sc, k), b.out_u, b.out_c, Cm, g ? g->scale[k] : 1.f, b.xs, m_cur, m_prev, s_buf, sc->threshold_ratio,
                 sc->threshold_max, B, (int)b.n(), s, b.x_bs);
        std::swap(m_cur, m_prev);
    });
    finish(h, b, s);
    DSD_CATCH
}

int dsd_op_dpm_step(const dsd_dpm_schedule* sc, int k, const float* model_out, int Cm, float* x, float* m_cur,
                    const float* m_prev, int B, int H, int W, void* stream) {
    DSD_TRY
    check_dpm_schedule(sc);
    DSD_CHECK(k >= 0 && k < sc->steps && model_out && x && m_cur && (Cm == 1 || Cm == 2), "bad argument");
    DSD_CHECK(sc->order[k] < 2 || m_prev, "a second-order update needs m_prev");
    Tmp sb((size_t)B * sizeof(float));
    dpm_step(dpm_coef(sc, k), nullptr, model_out, Cm, 1.f, x, m_cur, m_prev, sb.as<float>(), sc->threshold_ratio, sc->threshold_max, B,
             H * W, (hipStream_t)stream);
    DSD_HIP(hipStreamSynchronize((hipStream_t)stream));
    DSD_CATCH
}

int dsd_op_dpm_step_guided(const dsd_dpm_schedule* sc, int k, const float* out_uncond, const float* out_cond, int Cm, float scale,
                           float* x, int64_t x_row_stride, float* m_cur, const float* m_prev, int B, int Cz, int H, int W,
                           void* stream) {
    DSD_TRY
    check_dpm_schedule(sc);
    DSD_CHECK(k >= 0 && k < sc->steps && out_uncond && out_cond && x && m_cur && (Cm == 1 || Cm == 2), "bad argument");
    check_op_state(B, Cz, H, W, x_row_stride);
    DSD_CHECK(sc->order[k] < 2 || m_prev, "a second-order update needs m_prev");
    Tmp sb((size_t)B * sizeof(float));
    dpm_step(dpm_coef(sc, k), out_uncond, out_cond, Cm, scale, x, m_cur, m_prev, sb.as<float>(), sc->threshold_ratio,
             sc->threshold_max, B, Cz * H * W, (hipStream_t)stream, x_row_stride);
    DSD_HIP(hipStreamSynchronize((hipStream_t)stream));
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- DPM-Solver programs
static const int kDpmReads[] = {1, 1, 2, 3, 1, 2, 2, 2, 3};   // history planes a kind reads (ma, mb, mc), by DSD_DPM_*

// Walks the program once: kinds, slots, the history a multistep update reads, the order of singlestep stages.
static void check_dpm_program(const dsd_dpm_program* p) {
    DSD_CHECK(p, "null DPM program");
    DSD_CHECK(p->n_eval >= 1, "a DPM program of %d evaluations", p->n_eval);
    DSD_CHECK(p->kind && p->t_input && p->alpha && p->sigma && p->coef && p->slot,
              "DPM program: null array (kind %p t_input %p alpha %p sigma %p coef %p slot %p)", (const void*)p->kind,
              (const void*)p->t_input, (const void*)p->alpha, (const void*)p->sigma, (const void*)p->coef, (const void*)p->slot);
    DSD_CHECK(p->pred >= DSD_PRED_EPS && p->pred <= DSD_PRED_V, "DPM program: unknown prediction type %d", p->pred);
    DSD_CHECK(!p->thresholding || (p->threshold_ratio >= 0.f && p->threshold_ratio <= 1.f),
              "DPM program: threshold_ratio %g outside [0,1]", (double)p->threshold_ratio);
    unsigned written = 0;
    int stage = 0;                                             // 0 between steps, 1 after SS_S1, 2 after SS_S2
    for (int k = 0; k < p->n_eval; ++k) {
        const int kind = p->kind[k];
        const int32_t* sl = p->slot + (size_t)k * 4;
        DSD_CHECK(kind >= DSD_DPM_MS0 && kind <= DSD_DPM_SS_T3_TAYLOR, "DPM program: evaluation %d has kind %d; the table ends at %d",
                  k, kind, (int)DSD_DPM_SS_T3_TAYLOR);
        const int want = kind == DSD_DPM_SS_S2 || kind == DSD_DPM_SS_T2 ? 1 : (kind == DSD_DPM_SS_T3 || kind == DSD_DPM_SS_T3_TAYLOR ? 2 : 0);
        DSD_CHECK(stage == want,
                  "DPM program: evaluation %d (kind %d) comes after %d stage(s) of a singlestep step; it needs %d (SS_S2 / SS_T2 follow "
                  "SS_S1, which saves the base state; SS_T3 / SS_T3_TAYLOR follow SS_S2; every other kind stands between steps)",
                  k, kind, stage, want);
        stage = kind == DSD_DPM_SS_S1 ? 1 : (kind == DSD_DPM_SS_S2 ? 2 : 0);
        for (int j = 0; j < 4; ++j)
            DSD_CHECK(sl[j] >= 0 && sl[j] <= 2, "DPM program: evaluation %d names history plane %d (slot[%d]); there are planes 0..2", k,
                      sl[j], j);
        written |= 1u << sl[0];
        for (int j = 1; j <= kDpmReads[kind]; ++j)
            DSD_CHECK(written >> sl[j] & 1u,
                      "DPM program: evaluation %d (kind %d) reads history plane %d as model value %d, which no evaluation up to it wrote "
                      "(a higher-order update before its history exists)", k, kind, sl[j], j);
        DSD_CHECK(sl[1] != sl[2] || kDpmReads[kind] < 2, "DPM program: evaluation %d (kind %d) reads plane %d twice", k, kind, sl[1]);
        DSD_CHECK(kDpmReads[kind] < 3 || (sl[3] != sl[1] && sl[3] != sl[2]), "DPM program: evaluation %d (kind %d) reads plane %d twice", k,
                  kind, sl[3]);
    }
    DSD_CHECK(stage == 0, "DPM program: it ends after %d stage(s) of a singlestep step, before the step's x_t", stage);
}

static int dpm_program_kept(const dsd_dpm_program* p) {
    int n = 0;
    for (int k = 0; p->keep && k < p->n_eval; ++k) n += p->keep[k] != 0;
    return n;
}

static void dpm_program_eval(const dsd_dpm_program* p, int k, const float* out_u, const float* out_c, int Cm, float scale, float* x,
                             int64_t x_bs, float* hist, float* base, float* s_buf, int B, int64_t n, hipStream_t s) {
    const int32_t* sl = p->slot + (size_t)k * 4;
    const size_t plane = (size_t)B * n;
    DpmCoef c{};
    c.alpha = p->alpha[k]; c.sigma = p->sigma[k];
    c.order = 0;
    c.pred = p->pred;
    c.data_pred = p->data_pred || p->kind[k] == DSD_DPM_MS0;
    c.thresh = p->thresholding;
    DpmEval e;
    for (int j = 0; j < DSD_DPM_NCOEF; ++j) e.c[j] = p->coef[(size_t)k * DSD_DPM_NCOEF + j];
    e.kind = p->kind[k];
    e.mw = hist + sl[0] * plane;
    e.ma = hist + sl[1] * plane;
    e.mb = kDpmReads[e.kind] >= 2 ? hist + sl[2] * plane : nullptr;
    e.mc = kDpmReads[e.kind] >= 3 ? hist + sl[3] * plane : nullptr;
    e.x = x; e.x_bs = x_bs; e.base = base;
    dpm_eval(c, e, out_u, out_c, Cm, scale, s_buf, p->threshold_ratio, p->threshold_max, B, (int)n, s);
}

// One driver for the four-stream model and the state-in-input denoisers, guided or not.  The history planes, the base plane and
// the thresholds share one handle buffer, sized before the loop and left alone inside it.  dpm_program_checks is everything the
// call is checked for (before any device work) and returns Cm; dpm_program_loop binds, runs every evaluation, calls
// after(binding, hist, base) on the planes the program left, and finishes.
static int dpm_program_checks(dsd_handle* h, const dsd_dpm_program* p, const dsd_guidance* g, const float* cond, int Cc, const float* x,
                              int Cz, int B, int H, int W, const float* inter, bool inter_loop) {
    const bool latent = state_in_input(h);
    refuse_trace(h, inter_loop ? "dsd_sample_dpm_program (its intermediates come through `intermediates`)" : "dsd_sample_dpm_adaptive_trial");
    check_dpm_program(p);
    if (g) check_guidance(g, p->n_eval, !(latent && Cc == 0 && h->has_cond));                          // one scale per evaluation
    const int kept = dpm_program_kept(p);
    DSD_CHECK(kept == 0 || inter, "the program keeps %d intermediate states but the output for them is null", kept);
    const int out_ch = check_denoiser(h, g, cond, Cc, x, Cz, B, H, W, Cz);
    const int Cm = latent ? out_ch / Cz : h->cfg.out_channels;
    DSD_CHECK(Cm == 1 || Cm == 2, "model has %d output channels; the solver takes 1 (or 2 with a learned sigma)", Cm);
    return Cm;
}

static void dpm_program_loop(dsd_handle* h, const dsd_dpm_program* p, const dsd_guidance* g, const float* cond, int Cc, float* x,
                             int Cz, int B, int H, int W, int Cm, float* inter, hipStream_t s,
                             const std::function<void(const LoopBinding&, float*, float*)>& after) {
    const LoopBinding b = bind_denoiser(h, g, cond, Cc, x, Cz, B, H, W, Cm * Cz, s);
    const size_t plane = (size_t)B * b.n();
    ensure_buf(&h->dpm_prog, &h->dpm_prog_cap, (4 * plane + B) * sizeof(float));
    float *hist = h->dpm_prog, *base = hist + 3 * plane, *s_buf = hist + 4 * plane;
    const size_t sample = (size_t)b.n() * sizeof(float);
    int n_kept = 0;
    run_loop(h, b, p->t_input, Range{0, p->n_eval}, s, [](int) {}, [&](int k) {
        dpm_program_eval(p, k, b.out_u, b.out_c, Cm, g ? g->scale[k] : 1.f, b.xs, b.x_bs, hist, base, s_buf, B, b.n(), s);
        if (p->keep && p->keep[k])
            DSD_HIP(hipMemcpy2DAsync(inter + (size_t)n_kept++ * plane, sample, b.xs, (size_t)b.x_bs * sizeof(float), sample, B,
                                     hipMemcpyDeviceToDevice, s));
    });
    after(b, hist, base);
    finish(h, b, s);
}

int dsd_sample_dpm_program(dsd_handle* h, const dsd_dpm_program* p, const dsd_guidance* g, const float* cond, int Cc, float* x, int Cz,
                           int B, int H, int W, float* inter, void* stream) {
    DSD_TRY
    const int Cm = dpm_program_checks(h, p, g, cond, Cc, x, Cz, B, H, W, inter, true);
    set_device(h->device);
    dpm_program_loop(h, p, g, cond, Cc, x, Cz, B, H, W, Cm, inter, (hipStream_t)stream, [](const LoopBinding&, float*, float*) {});
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- adaptive DPM-Solver
// The lower-order row of a trial against the step it belongs to: both results start from the same c0*x_s - c1*model_s
// (sampler.py:509-553, 592-631, 692-753 share sigma_t/sigma_s | exp(log_alpha_t - log_alpha_s) and the phi_1 term).
static void check_adaptive_lower(int lower_order, const float* lower, const float* step_row, float atol, float rtol) {
    DSD_CHECK(lower, "adaptive trial: the lower-order coefficients are null");
    DSD_CHECK(lower[0] == step_row[0] && lower[1] == step_row[1],
              "adaptive trial: the lower-order row (c0 %.9g, c1 %.9g) does not belong to the step (c0 %.9g, c1 %.9g): both updates "
              "go from the same s to the same t", (double)lower[0], (double)lower[1], (double)step_row[0], (double)step_row[1]);
    DSD_CHECK(lower_order == 2 ? std::isfinite(lower[2]) : lower[2] == 0.f,
              "adaptive trial: c2 of the lower-order row is %g; the first-order update has none (0) and the second-order one a finite "
              "value", (double)lower[2]);
    DSD_CHECK(atol > 0.f, "adaptive trial: atol %g; it must be positive (it bounds delta from below, and the error is divided by delta)",
              (double)atol);
    DSD_CHECK(rtol >= 0.f, "adaptive trial: rtol %g; it must not be negative", (double)rtol);
}

int dsd_sample_dpm_adaptive_trial(dsd_handle* h, const dsd_dpm_program* p, const dsd_guidance* g, const float* cond, int Cc,
                                  const float* lower_coef, float atol, float rtol, float* x, const float* x_prev, float* x_lower, int Cz,
                                  int B, int H, int W, float* err_host, void* stream) {
    DSD_TRY
    const int Cm = dpm_program_checks(h, p, g, cond, Cc, x, Cz, B, H, W, nullptr, false);
    const int n_eval = p->n_eval, last = p->kind[n_eval - 1];
    const bool one_step = (n_eval == 2 && p->kind[0] == DSD_DPM_SS_S1 && last == DSD_DPM_SS_T2) ||
                          (n_eval == 3 && p->kind[0] == DSD_DPM_SS_S1 && p->kind[1] == DSD_DPM_SS_S2 &&
                           (last == DSD_DPM_SS_T3 || last == DSD_DPM_SS_T3_TAYLOR));
    DSD_CHECK(one_step,
              "adaptive trial: the program has %d evaluation(s) (first kind %d, last kind %d); a trial is exactly one singlestep step of "
              "order 2 (SS_S1, SS_T2) or 3 (SS_S1, SS_S2, SS_T3 / SS_T3_TAYLOR)", n_eval, p->kind[0], last);
    check_adaptive_lower(n_eval - 1, lower_coef, p->coef + (size_t)(n_eval - 1) * DSD_DPM_NCOEF, atol, rtol);
    DSD_CHECK(x_prev && x_lower && err_host, "adaptive trial: null array (x_prev %p x_lower %p err %p)", (const void*)x_prev,
              (const void*)x_lower, (const void*)err_host);
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    // the partial sums first (hipMalloc aligns them), the B results behind; the pinned mirror of the results
    const size_t part_bytes = dpm_adaptive_part_doubles(B) * sizeof(double);
    ensure_buf(&h->dpm_adapt, &h->dpm_adapt_cap, part_bytes + (size_t)B * sizeof(float));
    if (h->dpm_adapt_host_n < B) {
        if (h->dpm_adapt_host) DSD_HIP(hipHostFree(h->dpm_adapt_host));
        h->dpm_adapt_host = nullptr;
        h->dpm_adapt_host_n = 0;
        DSD_HIP(hipHostMalloc((void**)&h->dpm_adapt_host, (size_t)B * sizeof(float), hipHostMallocDefault));
        h->dpm_adapt_host_n = B;
    }
    float* err_dev = reinterpret_cast<float*>(reinterpret_cast<char*>(h->dpm_adapt) + part_bytes);
    dpm_program_loop(h, p, g, cond, Cc, x, Cz, B, H, W, Cm, nullptr, s, [&](const LoopBinding& b, float* hist, float* base) {
        const size_t plane = (size_t)B * b.n();
        DpmAdaptiveErr a;
        for (int j = 0; j < 3; ++j) a.c[j] = lower_coef[j];
        a.lower_order = n_eval - 1;
        a.atol = atol; a.rtol = rtol;
        a.base = base;
        a.ma = hist + p->slot[0] * plane;                                       // model_s, model_s1: the planes evaluations 0, 1 wrote
        a.mb = hist + p->slot[4] * plane;
        a.xh = b.xs; a.x_bs = b.x_bs;
        a.x_prev = x_prev; a.x_lower = x_lower;
        a.part = reinterpret_cast<double*>(h->dpm_adapt);
        a.err = err_dev;
        dpm_adaptive_error(a, B, b.n(), s);
    });
    // the trial's one synchronisation, outside any capture (the network's graph was replayed, not recorded, on s)
    DSD_HIP(hipMemcpyAsync(h->dpm_adapt_host, err_dev, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
    DSD_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) err_host[b] = h->dpm_adapt_host[b];
    DSD_CATCH
}

int dsd_op_dpm_adaptive_error(int lower_order, const float* lower_coef, float atol, float rtol, const float* base, const float* ma,
                              const float* mb, const float* x_higher, int64_t x_row_stride, const float* x_prev, float* x_lower,
                              float* err, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    DSD_CHECK(lower_order == 1 || lower_order == 2, "adaptive error estimate: lower order %d; it is 1 or 2", lower_order);
    DSD_CHECK(lower_coef, "adaptive error estimate: the lower-order coefficients are null");
    check_adaptive_lower(lower_order, lower_coef, lower_coef, atol, rtol);
    DSD_CHECK(base && ma && (mb || lower_order == 1) && x_higher && x_prev && x_lower && err,
              "adaptive error estimate: null array (base %p ma %p mb %p x_higher %p x_prev %p x_lower %p err %p)", (const void*)base,
              (const void*)ma, (const void*)mb, (const void*)x_higher, (const void*)x_prev, (const void*)x_lower, (const void*)err);
    check_op_state(B, Cz, H, W, x_row_stride);
    Tmp part(dpm_adaptive_part_doubles(B) * sizeof(double));
    DpmAdaptiveErr a;
    for (int j = 0; j < 3; ++j) a.c[j] = lower_coef[j];
    a.lower_order = lower_order;
    a.atol = atol; a.rtol = rtol;
    a.base = base; a.ma = ma; a.mb = mb;
    a.xh = x_higher; a.x_bs = x_row_stride;
    a.x_prev = x_prev; a.x_lower = x_lower;
    a.part = part.as<double>();
    a.err = err;
    dpm_adaptive_error(a, B, (int64_t)Cz * H * W, (hipStream_t)stream);
    DSD_HIP(hipStreamSynchronize((hipStream_t)stream));
    DSD_CATCH
}

int dsd_op_dpm_eval(const dsd_dpm_program* prog, int k, const float* out_uncond, const float* out_cond, int Cm, float scale, float* x,
                    int64_t x_row_stride, float* hist, float* base, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    check_dpm_program(prog);
    DSD_CHECK(k >= 0 && k < prog->n_eval, "evaluation %d of a program of %d", k, prog->n_eval);
    DSD_CHECK(out_cond && x && hist, "null argument (out_cond %p x %p hist %p)", (const void*)out_cond, (const void*)x, (const void*)hist);
    DSD_CHECK(base || prog->kind[k] < DSD_DPM_SS_S1, "evaluation %d (kind %d) is a singlestep stage: it needs the base plane", k,
              prog->kind[k]);
    DSD_CHECK(Cm == 1 || Cm == 2, "Cm %d: an output row holds 1 or (with a learned sigma) 2 samples' worth of channels", Cm);
    check_op_state(B, Cz, H, W, x_row_stride);
    Tmp sb((size_t)B * sizeof(float));
    dpm_program_eval(prog, k, out_uncond, out_cond, Cm, scale, x, x_row_stride, hist, base, sb.as<float>(), B, (int64_t)Cz * H * W,
                     (hipStream_t)stream);
    DSD_HIP(hipStreamSynchronize((hipStream_t)stream));
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- PLMS
// plms.py:119-245: the blend in front of the (first) network evaluation of an iteration, the PLMS kernels after it.  The history
// of noise predictions stays on the handle: iterations from first_step > 0 need it resident, first_step = 0 starts it.
static void check_plms_schedule(const dsd_schedule* sc) {
    DSD_CHECK(sc && sc->coef && sc->t_model && sc->steps >= 1, "bad schedule");
    DSD_CHECK(sc->mode == DSD_MODE_B_PLMS, "the PLMS loops take a DSD_MODE_B_PLMS schedule; mode %d belongs to dsd_sample",
              sc->mode);
    DSD_CHECK(!sc->learned_range, "PLMS does not take a learned-range variance (learned_range is set)");
    DSD_CHECK(sc->pred == DSD_PRED_EPS,
              "PLMS feeds the network output to its update as a noise prediction (plms.py:227-243); prediction type %d is not one",
              sc->pred);
    for (int k = 0; k < sc->steps; ++k)
        DSD_CHECK(sc->coef[(size_t)k * DSD_NCOEF + 6] == 0.f, "PLMS takes eta = 0 only: sigma of iteration %d is %g, not 0", k,
                  (double)sc->coef[(size_t)k * DSD_NCOEF + 6]);
}

int dsd_sample_plms(dsd_handle* h, const dsd_schedule* sc, const dsd_guidance* g, const dsd_inpaint* inp, float thr, const float* cond,
                    int Cc, float* x, int Cz, uint64_t seed, int B, int H, int W, int first_step, int n_steps, void* stream) {
    DSD_TRY
    const bool latent = state_in_input(h);
    check_plms_schedule(sc);
    if (g) check_guidance(g, sc->steps, !(latent && Cc == 0 && h->has_cond));
    if (inp) check_mask(inp, Cz);
    const int out_ch = check_denoiser(h, g, cond, Cc, x, Cz, B, H, W, Cz);
    DSD_CHECK(latent || h->cfg.out_channels == 1, "model has %d output channels but the schedule expects 1", h->cfg.out_channels);
    const int64_t n = (int64_t)Cz * H * W, plane = (int64_t)B * n;
    check_trace(h, sc->steps);
    const Range r = step_range(first_step, n_steps, sc->steps);
    if (r.k0 > 0 && r.k0 < r.k1)
        DSD_CHECK(h->plms_next == r.k0 && h->plms_B == B && h->plms_n == n && h->plms_steps == sc->steps,
                  "PLMS history for iteration %d is not resident on this handle (it holds %s iteration %d of %d, %d samples of %lld "
                  "elements): run the iterations before it first, with the same batch and schedule",
                  r.k0, h->plms_next < 0 ? "nothing;" : "the history for", h->plms_next, h->plms_steps, h->plms_B,
                  (long long)h->plms_n);
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t planes = ((size_t)3 * plane * sizeof(float) + 15) / 16 * 16;   // nothing is allocated once the planes have their size
    ensure_buf(&h->plms_hist, &h->plms_hist_cap, planes + plms_norm_doubles(B, n) * sizeof(double));
    const LoopBinding b = bind_denoiser(h, g, cond, Cc, x, Cz, B, H, W, out_ch, s);
    PlmsStep a;
    a.thr = thr > 0.f ? thr : 0.f;
    a.out_u = b.out_u;
    a.out_c = b.out_c;
    a.o_bs = out_ch * b.hw;
    a.x = b.xs;
    a.x_bs = b.x_bs;
    a.part = reinterpret_cast<double*>(reinterpret_cast<char*>(h->plms_hist) + planes);
    float* hist[3] = {h->plms_hist, h->plms_hist + plane, h->plms_hist + 2 * plane};
    Trace tr(h, b);   // pred_x0 of the step's final get_x_prev_and_pred_x0: iteration 0's from its corrector, not its predictor
    run_loop(h, b, sc->t_model, r, s,
             [&](int k) {
                 h->plms_next = -1;                                           // until this iteration's e_t is in its plane
                 if (inp) blend_step(sc, k, inp, b, seed, s);
             },
             [&](int k) {
                 const float* c = sc->coef + (size_t)k * DSD_NCOEF;
                 a.a_t = c[4]; a.a_prev = c[5]; a.sigma = c[6]; a.s1m = c[7];
                 a.scale = g ? g->scale[k] : 1.f;
                 if (k == 0) {                                                // plms.py:228-232: Euler, second evaluation at t_next
                     a.order = DSD_PLMS_PREDICT;
                     a.h_new = hist[0]; a.x_saved = hist[1]; a.o1 = a.o2 = nullptr;
                     plms_step(a, B, Cz, (int)b.hw, s);
                     fill_t(h->tbuf, b.rows, sc->t_model[std::min(1, sc->steps - 1)], s);
                     net_run_cached(h, s);
                     a.order = DSD_PLMS_CORRECT;
                     a.x0_out = tr.x0_slot(k);
                     plms_step(a, B, Cz, (int)b.hw, s);
                 } else {                                                     // newest prediction in plane (k-1) % 3; plane k % 3 retires
                     a.order = std::min(k, 3) + 1;
                     a.h_new = hist[k % 3]; a.o1 = hist[(k + 2) % 3]; a.o2 = hist[(k + 1) % 3]; a.x_saved = nullptr;
                     a.x0_out = tr.x0_slot(k);
                     plms_step(a, B, Cz, (int)b.hw, s);
                 }
                 tr.state(k, b, s);
                 h->plms_next = k + 1;
                 h->plms_B = B; h->plms_n = n; h->plms_steps = sc->steps;
             });
    finish(h, b, s);
    DSD_CATCH
}

int dsd_op_plms_step(int order, float a_t, float a_prev, float sqrt_1m_at, const float* out_uncond, const float* out_cond, float scale,
                     float* h_new, const float* o1, const float* o2, float* x_saved, float* x, int64_t x_row_stride,
                     float dynamic_threshold, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    DSD_CHECK(order >= DSD_PLMS_PREDICT && order <= DSD_PLMS_AB4, "unknown PLMS order %d", order);
    DSD_CHECK(out_cond && h_new && x, "null argument");
    DSD_CHECK(order > DSD_PLMS_CORRECT || x_saved, "the first PLMS step needs x_saved (null)");
    DSD_CHECK(order < DSD_PLMS_AB2 || o1, "PLMS order %d needs o1 (null)", order);
    DSD_CHECK(order < DSD_PLMS_AB3 || o2, "PLMS order %d needs o2 (null)", order);
    check_op_state(B, Cz, H, W, x_row_stride);
    PlmsStep a;
    a.a_t = a_t; a.a_prev = a_prev; a.sigma = 0.f; a.s1m = sqrt_1m_at;
    a.order = order;
    a.thr = dynamic_threshold > 0.f ? dynamic_threshold : 0.f;
    a.scale = scale;
    a.out_u = out_uncond; a.out_c = out_cond;
    a.h_new = h_new; a.o1 = o1; a.o2 = o2; a.x_saved = x_saved;
    a.x = x; a.x_bs = x_row_stride;
    Tmp part(a.thr > 0.f ? plms_norm_doubles(B, (int64_t)Cz * H * W) * sizeof(double) : 0);
    a.part = part.as<double>();
    plms_step(a, B, Cz, H * W, (hipStream_t)stream);
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- DDIM inversion
// ddim.py:263-308: the sampling loops' bindings, the inversion step in place of the update
int dsd_invert(dsd_handle* h, const dsd_invert_schedule* sc, const dsd_guidance* g, const float* cond, int Cc, float* x, int Cz, int B,
               int H, int W, int first_step, int n_steps, void* stream) {
    DSD_TRY
    const bool latent = state_in_input(h);
    refuse_trace(h, "dsd_invert");
    DSD_CHECK(sc && sc->coef && sc->t_model && sc->steps >= 1, "bad inversion schedule");
    if (g) check_guidance(g, sc->steps, !(latent && Cc == 0 && h->has_cond));
    const int out_ch = check_denoiser(h, g, cond, Cc, x, Cz, B, H, W, Cz);
    DSD_CHECK(latent || h->cfg.out_channels == 1, "model has %d output channels but the inversion takes 1", h->cfg.out_channels);
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    const LoopBinding b = bind_denoiser(h, g, cond, Cc, x, Cz, B, H, W, out_ch, s);
    run_loop(h, b, sc->t_model, step_range(first_step, n_steps, sc->steps), s, [](int) {}, [&](int k) {
        ddim_invert_step(sc->coef[2 * k], sc->coef[2 * k + 1], b.out_u, b.out_c, g ? g->scale[k] : 1.f, b.xs, B, Cz, (int)b.hw, s, b.x_bs,
                         out_ch * b.hw);
    });
    finish(h, b, s);
    DSD_CATCH
}

int dsd_op_mask_blend(float a, float s, const float* x0, const float* mask, int mask_channels, float* x, int64_t x_row_stride,
                      int guided, const float* noise, uint64_t philox_seed, uint64_t step, int B, int Cz, int H, int W,
                      void* stream) {
    DSD_TRY
    DSD_CHECK(x0 && mask && x, "null argument");
    check_op_state(B, Cz, H, W, x_row_stride);
    DSD_CHECK(mask_channels == 1 || mask_channels == Cz, "the mask has %d channels; 1 or the state's %d are taken", mask_channels, Cz);
    q_sample_blend(a, s, nullptr, nullptr, x0, mask, mask_channels, x, noise, philox_seed, step, B, Cz, H * W, (hipStream_t)stream,
                   x_row_stride, guided != 0);
    DSD_CATCH
}

int dsd_op_q_sample(const float* a, const float* s, const float* x0, const float* noise, uint64_t philox_seed, uint64_t step,
                    float* out, int64_t out_row_stride, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    DSD_CHECK(a && s && x0 && out, "null argument");
    check_op_state(B, Cz, H, W, out_row_stride);
    q_sample_blend(0.f, 0.f, a, s, x0, nullptr, 0, out, noise, philox_seed, step, B, Cz, H * W, (hipStream_t)stream, out_row_stride);
    DSD_CATCH
}

int dsd_op_ddim_invert_step(float cx, float ce, const float* out_uncond, const float* out_cond, float scale, float* x,
                            int64_t x_row_stride, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    DSD_CHECK(out_cond && x, "null argument");
    check_op_state(B, Cz, H, W, x_row_stride);
    ddim_invert_step(cx, ce, out_uncond, out_cond, scale, x, B, Cz, H * W, (hipStream_t)stream, x_row_stride);
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- variational bound
// calc_bpd_loop (gaussian_diffusion.py:938-991): the sampling loops' bindings with a state of the loop's own — pre(k) is the
// q_sample of x_start into it, step(k) the read-only terms pass — so the caller's x_start is never written and finish() never runs.
static void check_bpd_schedule(const dsd_schedule* sc) {
    check_schedule(sc);
    DSD_CHECK(sc->mode == DSD_MODE_A_DDPM,
              "the variational bound is defined on the guided-diffusion posterior (DSD_MODE_A_DDPM: coef 4-7 hold its mean "
              "coefficients and log-variances); the schedule has mode %d", sc->mode);
}

static VlbStep vlb_step(const dsd_schedule* sc, int k, float post_log_var) {
    VlbStep a;
    a.sc = step_coef(sc, k);
    a.post_log_var = post_log_var;
    a.step = (uint64_t)k;
    return a;
}

int dsd_calc_bpd(dsd_handle* h, const dsd_schedule* sc, const dsd_bpd* bpd, const float* cond, int Cc, const float* x_start, int Cz,
                 const float* noise, uint64_t seed, int B, int H, int W, int first_step, int n_steps, void* stream) {
    DSD_TRY
    const bool latent = state_in_input(h);
    refuse_trace(h, "dsd_calc_bpd");
    check_bpd_schedule(sc);
    DSD_CHECK(bpd, "null dsd_bpd");
    DSD_CHECK(bpd->post_log_var, "the bound needs the true posterior's log-variances (post_log_var is null; %d steps)", sc->steps);
    DSD_CHECK(bpd->vb && bpd->xstart_mse && bpd->mse, "null output: vb %p xstart_mse %p mse %p", (void*)bpd->vb, (void*)bpd->xstart_mse,
              (void*)bpd->mse);
    DSD_CHECK(!(sc->learned_range && Cz > 1) || is_dit(h),
              "learned-range variance needs one state channel (the model output interleaves mean and variance per sample); Cz = %d", Cz);
    const int want_ch = (sc->learned_range ? 2 : 1) * Cz;
    const int out_ch = check_denoiser(h, nullptr, cond, Cc, x_start, Cz, B, H, W, want_ch);
    DSD_CHECK(latent || h->cfg.out_channels == out_ch, "model has %d output channels but the schedule expects %d%s", h->cfg.out_channels,
              out_ch, sc->learned_range ? " (learned_range needs a variance half)" : "");
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W, n = Cz * hw;
    const size_t part_bytes = (vlb_part_doubles(B, n) * sizeof(double) + 15) / 16 * 16;
    ensure_buf(&h->bpd_buf, &h->bpd_cap, part_bytes + (latent ? 0 : (size_t)B * n * sizeof(float)));
    double* part = reinterpret_cast<double*>(h->bpd_buf);
    // the four-stream model reads its state plane in place: it gets the loop's own; the latent binding copies into lat_in and
    // only finish() would write back
    float* state = latent ? const_cast<float*>(x_start) : h->bpd_buf + part_bytes / sizeof(float);
    const LoopBinding b = bind_denoiser(h, nullptr, cond, Cc, state, Cz, B, H, W, out_ch, s);
    const float* c_first = sc->coef;
    if (bpd->prior) prior_bpd(c_first[0], bpd->prior_log_var, x_start, part, bpd->prior, B, n, s);
    run_loop(h, b, sc->t_model, step_range(first_step, n_steps, sc->steps), s,
             [&](int k) {
                 const float* c = sc->coef + (size_t)k * DSD_NCOEF;
                 q_sample_blend(c[0], c[1], nullptr, nullptr, x_start, nullptr, 0, b.xs, noise ? noise + (size_t)k * B * n : nullptr,
                                seed, (uint64_t)k, B, Cz, (int)hw, s, b.x_bs, false, b.ids);
             },
             [&](int k) {
                 VlbStep a = vlb_step(sc, k, bpd->post_log_var[k]);
                 a.x_start = x_start;
                 a.xt = b.xs; a.x_bs = b.x_bs;
                 a.out = b.out_c; a.o_bs = out_ch * hw;
                 a.noise = noise ? noise + (size_t)k * B * n : nullptr;
                 a.seed = seed;
                 a.slice_ids = b.ids;
                 a.part = part;
                 vlb_terms(a, k == sc->steps - 1, bpd->vb + k, bpd->xstart_mse + k, bpd->mse + k, sc->steps, B, Cz, (int)hw, s);
             });
    net_check_overflow(h, s);
    DSD_CATCH
}

int dsd_op_vlb_terms(const dsd_schedule* sc, int k, float post_log_var, const float* model_out, int64_t out_row_stride,
                     const float* x_t, int64_t x_row_stride, const float* x_start, const float* noise, uint64_t philox_seed,
                     float* vb, float* xstart_mse, float* mse, int64_t term_stride, float* mean, float* log_variance,
                     float* pred_xstart, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    check_bpd_schedule(sc);
    DSD_CHECK(k >= 0 && k < sc->steps && model_out && x_t && x_start, "bad argument");
    check_op_state(B, Cz, H, W, x_row_stride);
    const int64_t need = (int64_t)(sc->learned_range ? 2 : 1) * Cz * H * W;
    DSD_CHECK(out_row_stride == 0 || out_row_stride >= need, "out_row_stride %lld is smaller than one output row (%lld)",
              (long long)out_row_stride, (long long)need);
    DSD_CHECK(term_stride >= 0, "term_stride %lld", (long long)term_stride);
    Tmp part(vlb_part_doubles(B, (int64_t)Cz * H * W) * sizeof(double));
    VlbStep a = vlb_step(sc, k, post_log_var);
    a.x_start = x_start;
    a.xt = x_t; a.x_bs = x_row_stride;
    a.out = model_out; a.o_bs = out_row_stride;
    a.noise = noise;
    a.seed = philox_seed;
    a.part = part.as<double>();
    a.mean = mean; a.log_variance = log_variance; a.pred_xstart = pred_xstart;
    vlb_terms(a, k == sc->steps - 1, vb, xstart_mse, mse, term_stride, B, Cz, H * W, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_prior_bpd(float sqrt_acp, float log_1m_acp, const float* x_start, float* prior, int B, int Cz, int H, int W,
                     void* stream) {
    DSD_TRY
    DSD_CHECK(x_start && prior, "null argument");
    check_op_state(B, Cz, H, W, 0);
    Tmp part(vlb_part_doubles(B, (int64_t)Cz * H * W) * sizeof(double));
    prior_bpd(sqrt_acp, log_1m_acp, x_start, part.as<double>(), prior, B, (int64_t)Cz * H * W, (hipStream_t)stream);
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- denoising loss
// training_losses / p_losses, forward only (include/dsdiff.h): q_sample with per-row coefficients into a state of the call's own
// (as dsd_calc_bpd keeps one), the per-sample t copied into the handle's timestep rows, one evaluation through the cached
// graph, then the reductions of loss.hip into the caller's [B,DSD_LOSS_NTERMS] rows.
static void check_loss_codes(int pred, int kind) {
    DSD_CHECK(pred >= DSD_PRED_EPS && pred <= DSD_PRED_V, "unknown prediction type %d", pred);
    DSD_CHECK(kind >= DSD_LOSS_L2 && kind <= DSD_LOSS_CHARBONNIER, "unknown loss kind %d (DSD_LOSS_L2 / _L1 / _CHARBONNIER)", kind);
}

// fn() on s; while the handle profiles, between two events whose distance is added to the record of `kind` (algorithmic bytes)
static void profiled_launch(dsd_handle* h, const char* kind, double bytes, hipStream_t s, const std::function<void()>& fn) {
    if (!h->profiling) {
        fn();
        return;
    }
    hipEvent_t e0, e1;
    DSD_HIP(hipEventCreate(&e0));
    DSD_HIP(hipEventCreate(&e1));
    DSD_HIP(hipEventRecord(e0, s));
    fn();
    DSD_HIP(hipEventRecord(e1, s));
    DSD_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    DSD_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    size_t j = 0;
    while (j < h->prof_x_names.size() && h->prof_x_names[j] != kind) ++j;
    if (j == h->prof_x_names.size()) {
        h->prof_x_names.push_back(kind);
        h->prof_x_ms.push_back(0.0); h->prof_x_bytes.push_back(0.0); h->prof_x_calls.push_back(0);
    }
    h->prof_x_ms[j] += ms; h->prof_x_bytes[j] += bytes; h->prof_x_calls[j] += 1;
}

static VlbStep vlb_rows_step(int pred, int learned_range, int clip, uint64_t step) {
    VlbStep a;
    a.sc = StepCoef{};
    a.sc.mode = DSD_MODE_A_DDPM; a.sc.pred = pred; a.sc.learned_range = learned_range; a.sc.clip = clip; a.sc.nonzero = 1;
    a.step = step;
    return a;
}

int dsd_eval_loss(dsd_handle* h, const dsd_loss* spec, const float* cond, int Cc, const float* x_start, int Cz, const float* noise,
                  uint64_t seed, uint64_t step, int B, int H, int W, void* stream) {
    DSD_TRY
    const bool latent = state_in_input(h);
    refuse_trace(h, "dsd_eval_loss");
    DSD_CHECK(spec, "null dsd_loss");
    check_loss_codes(spec->pred, spec->kind);
    check_loss_codes(spec->target, spec->kind);
    DSD_CHECK(spec->t_model && spec->a && spec->s && spec->terms, "null rows: t_model %p a %p s %p terms %p", (void*)spec->t_model,
              (void*)spec->a, (void*)spec->s, (void*)spec->terms);
    DSD_CHECK(!spec->vlb_coef || (spec->post_log_var && spec->decoder),
              "the vb term needs post_log_var and decoder beside vlb_coef (post_log_var %p decoder %p)", (void*)spec->post_log_var,
              (void*)spec->decoder);
    DSD_CHECK(!spec->learned_range || spec->vlb_coef, "learned_range is read by the vb term only, which needs vlb_coef (null)");
    DSD_CHECK(!(spec->learned_range && Cz > 1) || is_dit(h),
              "learned-range variance needs one state channel (the model output interleaves mean and variance per sample); Cz = %d", Cz);
    const int want_ch = (spec->learned_range ? 2 : 1) * Cz;
    const int out_ch = check_denoiser(h, nullptr, cond, Cc, x_start, Cz, B, H, W, want_ch);
    DSD_CHECK(latent || h->cfg.out_channels == out_ch, "model has %d output channels but the loss expects %d%s", h->cfg.out_channels,
              out_ch, spec->learned_range ? " (learned_range needs a variance half)" : "");
    const dsd_disentangle* dz = h->has_disen ? &h->disen : nullptr;
    if (dz) {
        DSD_CHECK(!latent && !h->is_disc, "a disentangle rider (dsd_set_disentangle) is installed: only the DSUnetModel of dsd_create has "
                  "the content / style / anatomy / lesion heads; this handle is %s", h->is_disc ? "a UNet_disc_Model" : "a block handle (UNetModel / DiT)");
        DSD_CHECK(dz->n_labels_cs == 6 * B && dz->n_labels_sal == 7 * B, "disentangle: %d and %d labels, but a batch of %d has %d "
                  "content + style rows and %d style + anatomy + lesion rows", dz->n_labels_cs, dz->n_labels_sal, B, 6 * B, 7 * B);
        DSD_CHECK(7 * B <= DSD_CONTRAST_MAX_ROWS, "disentangle: a batch of %d has %d style + anatomy + lesion rows; up to %d are taken",
                  B, 7 * B, DSD_CONTRAST_MAX_ROWS);
    }
    set_device(h->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W, n = Cz * hw;
    const bool disc = !latent && h->is_disc;
    // UNet_disc_Model: planned first (bind_four_stream asks for the same plan again), since the size of its bottleneck tensors,
    // which the com / dist reduction's partials follow, comes from the plan
    if (disc) net_plan(h, B, Cc + 1, H, W, 0, 2, 0, 0, 0, s);
    // the head tensors likewise (the binding below asks for the same plan again)
    if (dz) net_plan(h, B, Cc + 1, H, W, Cc == 1, 2, 0, 0, 0, s);
    const size_t part_doubles = std::max({vlb_part_doubles(B, n), loss_part_doubles(B, n), disc ? pair_part_doubles(B, h->plan.feat_n) : (size_t)0,
                                          dz ? contrast_part_doubles(7 * B, h->plan.feat_n) : (size_t)0});
    const size_t part_bytes = (part_doubles * sizeof(double) + 15) / 16 * 16;
    ensure_buf(&h->loss_buf, &h->loss_cap, part_bytes + (latent ? 0 : (size_t)B * n * sizeof(float)));
    // the four-stream model reads its state plane in place: it gets the call's own; the latent binding copies into lat_in
    float* state = latent ? const_cast<float*>(x_start) : h->loss_buf + part_bytes / sizeof(float);
    const LoopBinding b = bind_denoiser(h, nullptr, cond, Cc, state, Cz, B, H, W, out_ch, s, disc || dz ? 2 : 0);
    double* part = reinterpret_cast<double*>(h->loss_buf);
    q_sample_blend(0.f, 0.f, spec->a, spec->s, x_start, nullptr, 0, b.xs, noise, seed, step, B, Cz, (int)hw, s, b.x_bs, false, b.ids);
    DSD_HIP(hipMemcpyAsync(h->tbuf, spec->t_model, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
    net_run_cached(h, s);
    LossRows l;
    l.out = b.out_c; l.o_bs = out_ch * hw;
    l.x_start = x_start; l.noise = noise;
    l.a_row = spec->a; l.s_row = spec->s;
    l.target = spec->target; l.kind = spec->kind;
    l.seed = seed; l.step = step; l.slice_ids = b.ids;
    l.part = part;
    l.loss = spec->terms + DSD_LOSS_TERM_MSE; l.stride = DSD_LOSS_NTERMS;
    const double plane = (double)B * n * sizeof(float);   // one [B,Cz,H,W] tensor
    profiled_launch(h, "loss_rows", plane * (spec->target == DSD_PRED_V ? 3 : 2), s, [&] { loss_rows(l, B, Cz, (int)hw, s); });
    if (spec->vlb_coef) {
        VlbStep a = vlb_rows_step(spec->pred, spec->learned_range, 0, step);   // clip_denoised=False (:847, :872)
        a.x_start = x_start;
        a.xt = b.xs; a.x_bs = b.x_bs;
        a.out = b.out_c; a.o_bs = out_ch * hw;
        a.noise = noise;
        a.seed = seed;
        a.slice_ids = b.ids;
        a.part = part;
        VlbRows r;
        r.coef = spec->vlb_coef; r.post_log_var = spec->post_log_var; r.decoder = spec->decoder;
        profiled_launch(h, "vlb_terms_rows", plane * (spec->learned_range ? 5 : 4), s, [&] {
            vlb_terms_rows(a, r, spec->terms + DSD_LOSS_TERM_VB, nullptr, nullptr, DSD_LOSS_NTERMS, B, Cz, (int)hw, s);
        });
    }
    if (disc) {
        for (int half = 0; half < 2; ++half) {
            PairMse pm;
            pm.nf = 4;
            for (int i = 0; i < 4; ++i) pm.f[i] = h->at<float>(h->plan.feat_off[4 * half + i]);
            pm.part = part;
            pm.out = spec->terms + (half ? DSD_LOSS_TERM_DIST : DSD_LOSS_TERM_COM);
            pm.stride = DSD_LOSS_NTERMS;
            profiled_launch(h, "pair_mse_rows", 4.0 * B * h->plan.feat_n * sizeof(float), s,
                            [&] { pair_mse_rows(pm, B, h->plan.feat_n, s); });
        }
    }
    if (dz) {   // c_s = content + style, s_a_l = style + anatomy + lesion (:917-918, :940); feat_off: style, content, anatomy, lesion
        static const int cs[6] = {3, 4, 5, 0, 1, 2}, sal[7] = {0, 1, 2, 6, 7, 8, 9};
        for (int half = 0; half < 2; ++half) {
            const int nv = half ? 7 : 6;
            ContrastRows c;
            for (int i = 0; i < nv; ++i) c.v[i] = h->at<float>(h->plan.feat_off[half ? sal[i] : cs[i]]);
            c.labels = half ? dz->labels_sal : dz->labels_cs;
            c.part = part;
            c.loss = dz->loss + half;
            c.logits = half ? dz->logits_sal : dz->logits_cs;
            const float temp = half ? dz->temperature_sal : dz->temperature_cs;
            profiled_launch(h, "contrast_rows", (double)nv * B * h->plan.feat_n * sizeof(float), s,
                            [&] { contrast_rows(c, nv, B, h->plan.feat_n, dz->mode, temp, s); });
        }
    }
    net_check_overflow(h, s);
    DSD_CATCH
}

int dsd_op_contrast_rows(const float* const* views, int n_views, int B, int64_t n, int64_t row_stride, const int32_t* labels,
                         int mode, float temperature, float* loss, float* logits, void* stream) {
    DSD_TRY
    DSD_CHECK(views && labels && loss && logits, "null argument");
    contrast_check(n_views, B, n, mode, temperature);
    for (int i = 0; i < n_views; ++i) DSD_CHECK(views[i], "view %d is null", i);
    DSD_CHECK(row_stride == 0 || row_stride >= n, "row_stride %lld is smaller than one row (%lld)", (long long)row_stride, (long long)n);
    Tmp part(contrast_part_doubles(n_views * B, n) * sizeof(double));
    ContrastRows c;
    for (int i = 0; i < n_views; ++i) c.v[i] = views[i];
    c.bs = row_stride;
    c.labels = labels;
    c.part = part.as<double>();
    c.loss = loss;
    c.logits = logits;
    contrast_rows(c, n_views, B, n, mode, temperature, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_image_metrics(const dsd_image_metrics* spec, void* stream) {
    DSD_TRY
    DSD_CHECK(spec, "image_metrics: spec is null");
    DSD_CHECK(spec->pred, "image_metrics: pred is null");
    DSD_CHECK(spec->target, "image_metrics: target is null");
    DSD_CHECK(spec->scale_out, "image_metrics: scale_out is null");
    DSD_CHECK(spec->elem_out, "image_metrics: elem_out is null");
    image_metrics_check(spec->B, spec->C, spec->H, spec->W, spec->scales, spec->data_range, spec->pre);
    Tmp scratch(image_metrics_scratch_doubles(spec->B, spec->C, spec->H, spec->W, spec->scales) * sizeof(double));
    ImageMetrics m;
    m.pred = spec->pred; m.target = spec->target;
    m.B = spec->B; m.C = spec->C; m.H = spec->H; m.W = spec->W;
    m.scales = spec->scales;
    m.data_range = spec->data_range;
    m.pre = spec->pre;
    m.scratch = scratch.as<double>();
    m.scale_out = spec->scale_out;
    m.elem_out = spec->elem_out;
    image_metrics(m, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_volume_metrics(const dsd_volume_metrics* spec, void* stream) {
    DSD_TRY
    DSD_CHECK(spec, "volume_metrics: spec is null");
    DSD_CHECK(spec->target, "volume_metrics: target is null");
    DSD_CHECK(spec->pred, "volume_metrics: pred is null");
    DSD_CHECK(spec->out, "volume_metrics: out is null");
    volume_metrics_check(spec->D, spec->H, spec->W, spec->win, spec->elem_is_double);
    Tmp scratch(volume_metrics_scratch_bytes(spec->D, spec->H, spec->W, spec->win));
    VolumeMetrics m;
    m.target = spec->target; m.pred = spec->pred;
    m.elem_is_double = spec->elem_is_double;
    m.mask = spec->mask;
    m.D = spec->D; m.H = spec->H; m.W = spec->W;
    m.win = spec->win;
    m.scratch = scratch.p;
    m.out = spec->out;
    volume_metrics(m, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_kth_double(const double* x, int64_t n, int64_t k, double* out, void* stream) {
    DSD_TRY
    DSD_CHECK(x && out, "kth_double: null argument");
    kth_double_check(n, k);
    Tmp scratch(kth_double_scratch_bytes());
    kth_double(x, n, k, scratch.p, out, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_loss_rows(int pred, int kind, const float* model_out, int64_t out_row_stride, const float* x_start, const float* noise,
                     uint64_t philox_seed, uint64_t step, const float* a, const float* s, float* loss, int64_t loss_stride, int B,
                     int Cz, int H, int W, void* stream) {
    DSD_TRY
    check_loss_codes(pred, kind);
    DSD_CHECK(model_out && loss, "null argument");
    check_op_state(B, Cz, H, W, out_row_stride);
    DSD_CHECK(loss_stride >= 0, "loss_stride %lld", (long long)loss_stride);
    Tmp part(loss_part_doubles(B, (int64_t)Cz * H * W) * sizeof(double));
    LossRows l;
    l.out = model_out; l.o_bs = out_row_stride;
    l.x_start = x_start; l.noise = noise;
    l.a_row = a; l.s_row = s;
    l.target = pred; l.kind = kind;
    l.seed = philox_seed; l.step = step;
    l.part = part.as<double>();
    l.loss = loss; l.stride = loss_stride;
    loss_rows(l, B, Cz, H * W, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_pair_mse_rows(const float* const* feats, int n_feats, int B, int64_t n, float* out, void* stream) {
    DSD_TRY
    DSD_CHECK(feats && out, "null argument");
    DSD_CHECK(n_feats >= 2 && n_feats <= 4, "pair_mse_rows takes 2, 3 or 4 feature tensors, got %d", n_feats);
    DSD_CHECK(B >= 1 && n >= 1, "bad shape: B %d n %lld", B, (long long)n);
    Tmp part(pair_part_doubles(B, n) * sizeof(double));
    PairMse pm;
    pm.nf = n_feats;
    for (int i = 0; i < n_feats; ++i) pm.f[i] = feats[i];
    pm.part = part.as<double>();
    pm.out = out;
    pair_mse_rows(pm, B, n, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_vlb_terms_rows(int pred, int learned_range, int clip_denoised, const float* coef, const float* post_log_var,
                          const int32_t* decoder, const float* model_out, int64_t out_row_stride, const float* x_t,
                          int64_t x_row_stride, const float* x_start, const float* noise, uint64_t philox_seed, uint64_t step,
                          float* vb, float* xstart_mse, float* mse, int64_t term_stride, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    DSD_CHECK(pred >= DSD_PRED_EPS && pred <= DSD_PRED_V, "unknown prediction type %d", pred);
    DSD_CHECK(coef && post_log_var && decoder && model_out && x_t && x_start, "null argument");
    check_op_state(B, Cz, H, W, x_row_stride);
    const int64_t need = (int64_t)(learned_range ? 2 : 1) * Cz * H * W;
    DSD_CHECK(out_row_stride == 0 || out_row_stride >= need, "out_row_stride %lld is smaller than one output row (%lld)",
              (long long)out_row_stride, (long long)need);
    DSD_CHECK(term_stride >= 0, "term_stride %lld", (long long)term_stride);
    Tmp part(vlb_part_doubles(B, (int64_t)Cz * H * W) * sizeof(double));
    VlbStep a = vlb_rows_step(pred, learned_range != 0, clip_denoised != 0, step);
    a.x_start = x_start;
    a.xt = x_t; a.x_bs = x_row_stride;
    a.out = model_out; a.o_bs = out_row_stride;
    a.noise = noise;
    a.seed = philox_seed;
    a.part = part.as<double>();
    VlbRows r;
    r.coef = coef; r.post_log_var = post_log_var; r.decoder = decoder;
    vlb_terms_rows(a, r, vb, xstart_mse, mse, term_stride, B, Cz, H * W, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_ddim_reverse_step(const dsd_schedule* sc, int k, float alpha_bar_next, const float* model_out, int64_t out_row_stride,
                             float* x, int64_t x_row_stride, float* pred_xstart, int B, int Cz, int H, int W, void* stream) {
    DSD_TRY
    check_schedule(sc);
    DSD_CHECK(sc->mode == DSD_MODE_A_DDPM || sc->mode == DSD_MODE_A_DDIM,
              "ddim_reverse_sample belongs to the guided-diffusion family (DSD_MODE_A_*: coef 0-3); the schedule has mode %d", sc->mode);
    DSD_CHECK(k >= 0 && k < sc->steps && model_out && x, "bad argument");
    check_op_state(B, Cz, H, W, x_row_stride);
    DSD_CHECK(out_row_stride == 0 || out_row_stride >= (int64_t)Cz * H * W, "out_row_stride %lld is smaller than one sample (%lld)",
              (long long)out_row_stride, (long long)Cz * H * W);
    ddim_reverse_step(step_coef(sc, k), alpha_bar_next, model_out, x, pred_xstart, B, Cz, H * W, (hipStream_t)stream, x_row_stride,
                      out_row_stride);
    DSD_CATCH
}

int dsd_op_dpm_threshold(const float* x0, int B, int n, float ratio, float max_val, float* y, float* s_out, void* stream) {
    DSD_TRY
    DSD_CHECK(x0 && y && s_out && B >= 0 && n >= 1 && ratio >= 0.f && ratio <= 1.f, "bad argument");
    dpm_threshold(x0, y, s_out, ratio, max_val, B, n, (hipStream_t)stream);
    DSD_CATCH
}

// ------------------------------------------------------------------------------------------- kernel-level ops
// The `precision` argument of the convolution entry points -> ConvArgs: arithmetic in bits 0-1; 16 / 32 / 64 force the
// A-direct / staged / 256-row A-direct structure of the split kernels; 256 plans as inside a stream-lane region (three launches
// of the same shape run beside this one).  Bit 128 (the F(2,3) kernel) needs packed weights: conv2d_op.
static void conv_option_bits(int bits, ConvArgs* a) {
    a->precision = bits & 3;
    if (a->precision != PREC_F32) a->variant = (bits & 64) ? 32 : (bits & 32) ? 31 : (bits & 16) ? 30 : -1;
    if (bits & 256) a->lanes = 4;
}

static dsd_conv_ex conv_ex_defaults() {
    dsd_conv_ex ex{};
    ex.x_batch_stride = ex.pad_lo = ex.pad_total = -1;
    return ex;
}

// The one body of the convolution entry points.  gn == nullptr: no GroupNorm arguments, always launched.  `launch` replaces the
// single conv2d() call (dsd_bench_conv2d times its own).
static void conv2d_op(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout, int ks,
                      int stride, int upsample, const float* emb, const float* res, int bits, dsd_conv_ex* ex, dsd_conv_gn* gn,
                      float* y, hipStream_t s, const std::function<void(ConvArgs&)>& launch = {}) {
    // every argument is checked before the first launch (the rules of the planner's destination views, net.cpp conv())
    DSD_CHECK(x && w_oihw && y && ex, "conv2d_ex: null argument");
    DSD_CHECK(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && (ks == 1 || ks == 3) && (stride == 1 || stride == 2),
              "conv2d_ex: bad problem size");
    const int64_t plane = (int64_t)H * W * Cin;
    DSD_CHECK(ex->x_batch_stride == -1 || ex->x_batch_stride == 0 || ex->x_batch_stride >= plane,
              "conv2d_ex: x_batch_stride %lld is neither -1, 0 nor at least one plane (%lld)", (long long)ex->x_batch_stride, (long long)plane);
    DSD_CHECK((ex->pad_lo < 0) == (ex->pad_total < 0) && ex->pad_lo < ks && ex->pad_total < 2 * ks && ex->pad_lo <= std::max(ex->pad_total, 0),
              "conv2d_ex: pad_lo %d / pad_total %d", ex->pad_lo, ex->pad_total);
    const int y_ld = ex->y_ld > 0 ? ex->y_ld : Cout, emb_stride = ex->emb_stride > 0 ? ex->emb_stride : Cout;
    DSD_CHECK(ex->y_ld >= 0 && y_ld >= Cout, "conv2d_ex: y_ld %d is smaller than Cout %d", ex->y_ld, Cout);
    DSD_CHECK(y_ld == Cout || y_ld % 4 == 0, "conv2d_ex: y_ld %d of a channel slice is not a multiple of 4", y_ld);
    DSD_CHECK(reinterpret_cast<uintptr_t>(y) % 16 == 0, "conv2d_ex: y is not 16-byte aligned");
    DSD_CHECK(!ex->out_nchw || y_ld == Cout, "conv2d_ex: an NCHW output has no row stride");
    DSD_CHECK(ex->emb_stride >= 0 && emb_stride >= Cout, "conv2d_ex: emb_stride %d is smaller than Cout %d", ex->emb_stride, Cout);
    DSD_CHECK(emb_stride == Cout || emb_stride % 4 == 0, "conv2d_ex: emb_stride %d of a column range is not a multiple of 4", emb_stride);
    DSD_CHECK(reinterpret_cast<uintptr_t>(emb) % 16 == 0, "conv2d_ex: emb is not 16-byte aligned");
    // the whole ConvArgs first, with a placeholder where a buffer will be: the queries below only look at which pointers are
    // present, so every refusal — and all of query mode — comes before anything touches a device
    const void* const present = ex;
    const size_t nw = (size_t)Cout * Cin * ks * ks;
    ConvArgs a;
    a.x = x; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.w = w_oihw; a.bias = bias; a.Cout = Cout; a.ks = ks;
    a.stride = stride; a.ups = upsample; a.emb = emb; a.emb_stride = emb_stride; a.res = res; a.y = y;
    a.x_bs = ex->x_batch_stride; a.pad_lo = ex->pad_lo; a.pad_total = ex->pad_total; a.y_ld = ex->y_ld;
    conv_option_bits(bits, &a);
    const bool split = a.precision != PREC_F32, f16 = a.precision == PREC_F16X3;
    if (split) a.w_split = present;
    if (bits & 128) {   // packed as the planner does, before the output layout is known: an NCHW launch then diverts
        DSD_CHECK(conv2d_wino_shape_ok(a), "conv2d: this problem cannot run on the F(2,3) kernel (3x3, stride 1, even width, "
                                           "Cin %% 16 == 0, Cout %% 32 == 0, >= 4096 output pixels, bf16x6)");
        a.w_wino = present;
    }
    a.out_nchw = ex->out_nchw ? 1 : 0;
    if (gn) {
        a.gn_scale = gn->gn_scale;
        a.gn_shift = gn->gn_shift;
    }
    const bool sub = conv2d_subpixel_ok(a);
    if (sub) a.w_subpixel = present;
    // what runs: the route of the launch these very arguments get, with / without scratch
    const ConvRoute route = conv2d_route(a, !ex->no_scratch);
    snprintf(ex->kernel, sizeof(ex->kernel), "%s", conv2d_route_name(route, a.gn_scale != nullptr));
    ex->ksplit = route.ksplit;
    if (gn) {
        gn->stats_chunks = route.stats_chunks;
        DSD_CHECK((gn->gn_scale == nullptr) == (gn->gn_shift == nullptr), "conv2d_gn: gn_scale and gn_shift come together");
        DSD_CHECK(gn->gn_scale == nullptr || route.fuses_gn, "conv2d_gn: GroupNorm coefficients given, but %s does not apply them "
                                                                  "(ConvRoute.fuses_gn)", ex->kernel);
        DSD_CHECK(gn->gn_scale == nullptr || (reinterpret_cast<uintptr_t>(gn->gn_scale) % 16 == 0 && reinterpret_cast<uintptr_t>(gn->gn_shift) % 16 == 0),
                  "conv2d_gn: gn_scale / gn_shift are not 16-byte aligned");
        if (gn->stats) {
            DSD_CHECK(gn->stats_chunks > 0, "conv2d_gn: output statistics requested, but %s cannot emit them for these arguments "
                                            "(ConvRoute.stats_chunks = 0)", ex->kernel);
            DSD_CHECK(gn->stats_doubles >= (int64_t)N * gn->stats_chunks * Cout * 2, "conv2d_gn: the statistics buffer holds %lld doubles, "
                      "%d chunks need %lld", (long long)gn->stats_doubles, gn->stats_chunks, (long long)N * gn->stats_chunks * Cout * 2);
            DSD_CHECK(reinterpret_cast<uintptr_t>(gn->stats) % 8 == 0, "conv2d_gn: stats is not 8-byte aligned");
            a.stats = gn->stats;
            a.stats_chunks = gn->stats_chunks;
        }
        if (gn->query) return;
    }
    // the derived weights of this call, then the launch
    Tmp wp(nw * sizeof(float)), planes(split ? nw * 2 * 3 : 0), ovf(sizeof(int));
    Tmp wpk(a.w_wino ? wino_packed_bytes(Cout, Cin) + 256 : 0), wsub(sub ? subpixel_weight_bytes(Cout, Cin) : 0), scratch(route.scratch_bytes);
    a.w = wp.as<float>();
    pack_ohwi(w_oihw, wp.as<float>(), Cout, Cin, ks, s);
    DSD_HIP(hipMemsetAsync(ovf.p, 0, sizeof(int), s));
    if (split) {
        split_weights(wp.as<float>(), (int64_t)nw, 3, planes.p, s, f16, f16 ? ovf.as<int>() : nullptr);
        a.w_split = planes.p;
        a.ovf = f16 ? ovf.as<int>() : nullptr;
    }
    if (a.w_wino) {
        wino_pack_weights(wp.as<float>(), Cout, Cin, wpk.p, s);
        a.w_wino = wpk.p;
    }
    if (sub) {
        subpixel_weights(wp.as<float>(), Cout, Cin, wsub.p, s);
        a.w_subpixel = wsub.p;
    }
    if (!ex->no_scratch) {
        a.scratch = scratch.as<float>();
        a.scratch_bytes = route.scratch_bytes;
    }
    if (launch)
        launch(a);
    else
        conv2d(a, s);
    int flag = 0;
    DSD_HIP(hipMemcpyAsync(&flag, ovf.p, sizeof(int), hipMemcpyDeviceToHost, s));
    DSD_HIP(hipStreamSynchronize(s));
    DSD_CHECK(!flag, "f16x3: a convolution operand exceeded the fp16 range (|x| > 65504); the result is invalid - use bf16x6 or f32");
}

int dsd_op_conv2d(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout, int ks,
                  int stride, int upsample, const float* emb, const float* res, float* y, void* stream) {
    return dsd_op_conv2d_prec(x, N, H, W, Cin, w_oihw, bias, Cout, ks, stride, upsample, emb, res, PREC_F32, y, stream);
}

int dsd_subpixel_weights_host(const float* w_oihw, int Cout, int Cin, double* out) {
    DSD_TRY
    DSD_CHECK(w_oihw && out && Cout > 0 && Cin > 0, "bad argument");
    for (int ph = 0; ph < 4; ++ph)
        for (int co = 0; co < Cout; ++co)
            for (int t = 0; t < 4; ++t)
                for (int ci = 0; ci < Cin; ++ci) {
                    double acc = 0.0;
                    for (int kh = 0; kh < 3; ++kh)
                        for (int kw = 0; kw < 3; ++kw)
                            if (subpixel_tap(ph >> 1, kh) == (t >> 1) && subpixel_tap(ph & 1, kw) == (t & 1))
                                acc += (double)w_oihw[(((size_t)co * Cin + ci) * 3 + kh) * 3 + kw];
                    out[(((size_t)ph * Cout + co) * 4 + t) * Cin + ci] = acc;
                }
    DSD_CATCH
}

int dsd_set_conv_mfma16(int on) {
    const int prev = conv2d_get_mfma16();
    conv2d_set_mfma16(on);
    return prev;
}

int dsd_conv_plan(int N, int H, int W, int Cin, int Cout, int ks, int stride, int precision, int* structure, int* nt,
                  int* ksplit, uint64_t* scratch_bytes) {
    DSD_TRY
    DSD_CHECK(structure && nt && ksplit && scratch_bytes, "null argument");
    ConvArgs a;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.ks = ks; a.stride = stride;
    conv_option_bits(precision, &a);
    a.w_split = a.precision != PREC_F32 ? &a : nullptr;   // only its presence matters to the route
    const ConvRoute r = conv2d_route(a, true);
    *structure = r.structure;
    *nt = r.nt;
    *ksplit = r.ksplit;
    *scratch_bytes = r.scratch_bytes;
    DSD_CATCH
}

int dsd_bench_conv2d(int N, int H, int W, int Cin, int Cout, int ks, int stride, int variant, int iters, float* avg_ms,
                     double* flops) {
    DSD_TRY
    DSD_CHECK(iters >= 1 && avg_ms, "bad argument");
    // variant numbers (tools/bench_conv.py): 0 / 1 = fp32 with buffer / flat loads; 10 + p = split arithmetic p (0 bf16x3, 1 bf16x6,
    // 2 f16x3); 20 + p / 30 + p / 40 + p = the same forced onto the staged / 128-row / 256-row A-direct structure; 50 = F(2,3), bf16x6
    DSD_CHECK(variant == 0 || variant == 1 || variant == 50 || (variant >= 10 && variant < 50 && variant % 10 <= 2), "bad variant %d", variant);
    static const int structure_bit[5] = {0, 0, 32, 16, 64};
    const int bits = variant < 10 ? PREC_F32 : variant == 50 ? (PREC_BF16X6 | 128) : ((variant % 10 + 1) | structure_bit[variant / 10]);
    hipStream_t s = nullptr;
    const int pad = ks / 2;
    const int OH = (H + 2 * pad - ks) / stride + 1, OW = (W + 2 * pad - ks) / stride + 1;
    const size_t nx = (size_t)N * H * W * Cin, nw = (size_t)Cout * Cin * ks * ks, ny = (size_t)N * OH * OW * Cout;
    Tmp x(nx * 4), w(nw * 4), b((size_t)Cout * 4), y(ny * 4);
    philox_normal(x.as<float>(), (int64_t)nx, 1, 0, s);
    philox_normal(w.as<float>(), (int64_t)nw, 2, 0, s);   // (random weights: their layout does not matter to the timing)
    philox_normal(b.as<float>(), Cout, 3, 0, s);
    dsd_conv_ex ex = conv_ex_defaults();
    conv2d_op(x.as<float>(), N, H, W, Cin, w.as<float>(), b.as<float>(), Cout, ks, stride, 0, nullptr, nullptr, bits, &ex, nullptr,
              y.as<float>(), s, [&](ConvArgs& a) {
        if (variant == 1) a.variant = 1;
        a.ovf = nullptr;   // (the f16x3 kernels are timed without their range check, as they always were here)
        conv2d(a, s);  // warm-up
        hipEvent_t e0, e1;
        DSD_HIP(hipEventCreate(&e0));
        DSD_HIP(hipEventCreate(&e1));
        DSD_HIP(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) conv2d(a, s);
        DSD_HIP(hipEventRecord(e1, s));
        DSD_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        DSD_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / iters;
        if (flops) *flops = conv2d_flops(a);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    });
    DSD_CATCH
}

int dsd_bench_conv2d_stamps(int N, int H, int W, int Cin, int Cout, int warm, int whatif, long long* out, int max_wgs,
                            int* n_wgs) {
    DSD_TRY
    DSD_CHECK(out && n_wgs && max_wgs > 0, "bad argument");
    hipStream_t s = nullptr;
    const size_t nx = (size_t)N * H * W * Cin, nw = (size_t)Cout * Cin * 9, ny = (size_t)N * H * W * Cout;
    Tmp x(nx * 4), w(nw * 4), b((size_t)Cout * 4), y(ny * 4), planes(nw * 2 * 3);
    philox_normal(x.as<float>(), (int64_t)nx, 1, 0, s);
    philox_normal(w.as<float>(), (int64_t)nw, 2, 0, s);
    philox_normal(b.as<float>(), Cout, 3, 0, s);
    ConvArgs a;
    a.x = x.as<float>(); a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.w = w.as<float>(); a.bias = b.as<float>();
    a.Cout = Cout; a.ks = 3; a.stride = 1; a.y = y.as<float>(); a.variant = 32; a.precision = PREC_BF16X6;
    split_weights(w.as<float>(), (int64_t)nw, 3, planes.p, s, false);
    a.w_split = planes.p;
    const int wgs = (int)(((int64_t)N * H * W + 255) / 256) * ((Cout + 159) / 160);
    DSD_CHECK(wgs <= max_wgs, "room for %d workgroups needed", wgs);
    for (int i = 0; i < warm; ++i) conv2d(a, s);
    Tmp st((size_t)wgs * 8 * sizeof(long long));
    DSD_HIP(hipMemsetAsync(st.p, 0, (size_t)wgs * 8 * sizeof(long long), s));
    a.stamps = st.as<long long>();
    a.diag = whatif;
    for (int i = 0; i < (whatif ? 20 : 0); ++i) conv2d(a, s);   // the what-if build's own steady state
    conv2d(a, s);
    DSD_HIP(hipMemcpyAsync(out, st.p, (size_t)wgs * 8 * sizeof(long long), hipMemcpyDeviceToHost, s));
    DSD_HIP(hipStreamSynchronize(s));
    *n_wgs = wgs;
    DSD_CATCH
}

int dsd_bench_mfma_peak(int variant, int workgroups_per_cu, float ms_target, int iters, float* avg_ms, double* tflops) {
    DSD_TRY
    DSD_CHECK(variant >= 0 && variant <= 7 && iters >= 1 && avg_ms && tflops, "bad argument");
    hipStream_t s = nullptr;
    const int wgs = 256 * (workgroups_per_cu > 0 ? std::min(workgroups_per_cu, 64) : 8);
    Tmp src((size_t)mfma_peak_src_bytes()), sink((size_t)wgs * 256 * sizeof(float));
    mfma_peak_fill(src.p, (variant & 2) != 0, s);
    hipEvent_t e0, e1;
    DSD_HIP(hipEventCreate(&e0));
    DSD_HIP(hipEventCreate(&e1));
    auto timed = [&](int loops, int n, double* fl) {
        DSD_HIP(hipEventRecord(e0, s));
        for (int i = 0; i < n; ++i) *fl = mfma_peak_launch(variant, src.p, sink.as<float>(), wgs, loops, s);
        DSD_HIP(hipEventRecord(e1, s));
        DSD_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        DSD_HIP(hipEventElapsedTime(&ms, e0, e1));
        return ms / n;
    };
    double fl = 0.0;
    int loops = 64;
    const float probe = timed(loops, 1, &fl);   // also the warm-up; then size the loop for ms_target per launch
    const float want = ms_target > 0.f ? std::min(ms_target, 200.f) : 5.f;
    loops = (int)std::max(16.0, std::min(1.0e6, loops * (double)want / std::max(probe, 1e-3f)));
    (void)timed(loops, 1, &fl);
    const float ms = timed(loops, iters, &fl);
    *avg_ms = ms;
    *tflops = fl / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    DSD_CATCH
}

int dsd_op_conv2d_prec(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout, int ks,
                       int stride, int upsample, const float* emb, const float* res, int precision, float* y, void* stream) {
    DSD_TRY
    dsd_conv_ex ex = conv_ex_defaults();
    conv2d_op(x, N, H, W, Cin, w_oihw, bias, Cout, ks, stride, upsample, emb, res, precision, &ex, nullptr, y, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_conv2d_ex(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout, int ks,
                     int stride, int upsample, const float* emb, const float* res, int precision, dsd_conv_ex* ex, float* y,
                     void* stream) {
    DSD_TRY
    conv2d_op(x, N, H, W, Cin, w_oihw, bias, Cout, ks, stride, upsample, emb, res, precision, ex, nullptr, y, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_conv2d_gn(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout, int ks,
                     int stride, int upsample, const float* emb, const float* res, int precision, dsd_conv_ex* ex, dsd_conv_gn* gn,
                     float* y, void* stream) {
    DSD_TRY
    DSD_CHECK(gn, "conv2d_gn: null argument");
    conv2d_op(x, N, H, W, Cin, w_oihw, bias, Cout, ks, stride, upsample, emb, res, precision, ex, gn, y, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_gn_finalize(const double* p0, int chunks0, int c0, const double* p1, int chunks1, int c1, int N, int HW, int C,
                       const float* gamma, const float* beta, float eps, const float* film, int film_stride, float* scale,
                       float* shift, void* stream) {
    DSD_TRY
    hipStream_t s = (hipStream_t)stream;
    DSD_CHECK(p0 && gamma && beta && scale && shift, "gn_finalize: null argument");
    DSD_CHECK(N >= 1 && HW >= 1 && C >= 32 && C % 32 == 0, "gn_finalize: bad problem size (GroupNorm32: C %% 32 == 0)");
    DSD_CHECK(chunks0 >= 1 && c0 >= 1 && (!p1 || (chunks1 >= 1 && c1 >= 1)), "gn_finalize: a source needs chunks >= 1 and channels >= 1");
    DSD_CHECK(c0 + (p1 ? c1 : 0) == C, "gn_finalize: the statistic sources (%d + %d channels) do not cover the %d channels", c0,
              p1 ? c1 : 0, C);
    DSD_CHECK(!film || film_stride >= 2 * C, "gn_finalize: film_stride %d is smaller than 2 C = %d", film_stride, 2 * C);
    GnSrc s0, s1;
    s0.p = p0; s0.chunks = chunks0; s0.c0 = 0; s0.c = c0;
    if (p1) {
        s1.p = p1; s1.chunks = chunks1; s1.c0 = c0; s1.c = c1;
    }
    gn_finalize(s0, s1, N, HW, C, gamma, beta, eps, film, film_stride, scale, shift, s);
    DSD_HIP(hipStreamSynchronize(s));
    DSD_CATCH
}

int dsd_op_avg_into_stats(const float* a, const float* b, const float* c, const float* d, float div, int N, int HW, int C, float* dst,
                          int dstC, int coff, int act, int bmask, double* partial, int64_t partial_doubles, int* nchunk,
                          void* stream) {
    DSD_TRY
    hipStream_t s = (hipStream_t)stream;
    DSD_CHECK(a && dst && partial && nchunk, "avg_into_stats: null argument");
    DSD_CHECK((b || !c) && (c || !d), "avg_into_stats: sources are given in order (a, b, c, d)");
    DSD_CHECK(N >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && dstC % 4 == 0 && coff % 4 == 0 && coff >= 0 && coff + C <= dstC,
              "avg_into_stats: channels [%d, %d) of %d: counts must be multiples of 4 and the slice inside the row", coff, coff + C, dstC);
    DSD_CHECK(div > 0.f && (act == ACT_NONE || act == ACT_SILU) && bmask >= 0 && bmask < 16, "avg_into_stats: bad div / act / bmask");
    for (const void* q : {(const void*)a, (const void*)b, (const void*)c, (const void*)d, (const void*)dst})
        DSD_CHECK(reinterpret_cast<uintptr_t>(q) % 16 == 0, "avg_into_stats: pointers must be 16-byte aligned");
    *nchunk = gn_nchunks(HW, C);
    DSD_CHECK(partial_doubles >= (int64_t)N * *nchunk * C * 2, "avg_into_stats: the statistics buffer holds %lld doubles, %d chunks need %lld",
              (long long)partial_doubles, *nchunk, (long long)N * *nchunk * C * 2);
    avg_into_stats(a, b, c, d, div, N, HW, C, dst, dstC, coff, act, bmask, partial, *nchunk, s);
    DSD_HIP(hipStreamSynchronize(s));
    DSD_CATCH
}

int dsd_op_disc_bottleneck(const float* const* com, const float* const* dist, const float* const* w1, const float* const* w2,
                           int B, int HW, int half, int Cr, float* cat, float* const* feats, int unfused, void* stream) {
    DSD_TRY
    hipStream_t s = (hipStream_t)stream;
    DSD_CHECK(com && dist && w1 && w2 && cat, "disc_bottleneck: null argument");
    DSD_CHECK(B >= 1 && HW >= 1 && half >= 4 && Cr >= 1, "disc_bottleneck: bad shape (B %d, HW %d, half %d, Cr %d)", B, HW, half, Cr);
    DSD_CHECK(half % 4 == 0, "disc_bottleneck: half = %d is not a multiple of 4 (the kernels move 16 bytes per access)", half);
    DiscArgs a;
    a.B = B; a.HW = HW; a.half = half; a.Cr = Cr; a.cat = cat;
    for (int i = 0; i < 4; ++i) { a.com[i] = com[i]; a.dist[i] = dist[i]; }
    for (int i = 0; i < 5; ++i) { a.w1[i] = w1[i]; a.w2[i] = w2[i]; }
    if (feats)
        for (int i = 0; i < 8; ++i) a.feat[i] = feats[i];
    for (int i = 0; i < 4; ++i)
        DSD_CHECK(a.com[i] && a.dist[i] && reinterpret_cast<uintptr_t>(a.com[i]) % 16 == 0 && reinterpret_cast<uintptr_t>(a.dist[i]) % 16 == 0,
                  "disc_bottleneck: inputs must be non-null and 16-byte aligned");
    DSD_CHECK(reinterpret_cast<uintptr_t>(cat) % 16 == 0, "disc_bottleneck: cat must be 16-byte aligned");
    for (int i = 0; i < 8; ++i)
        DSD_CHECK(!feats || (a.feat[i] && reinterpret_cast<uintptr_t>(a.feat[i]) % 16 == 0), "disc_bottleneck: feature outputs must be non-null and 16-byte aligned");
    const bool uf = unfused < 0 ? disc_unfused_env() : unfused != 0;
    Tmp scratch(disc_scratch_bytes(B, HW, half, uf));
    a.scratch = scratch.p;
    if (uf) disc_bottleneck_unfused(a, s); else disc_bottleneck(a, s);
    DSD_HIP(hipStreamSynchronize(s));
    DSD_CATCH
}

int dsd_op_gn_small(const float* x, int N, int HW, int C, const float* gamma, const float* beta, float eps, const float* film,
                    int film_stride, int act, float* y, void* stream) {
    DSD_TRY
    hipStream_t s = (hipStream_t)stream;
    DSD_CHECK(x && gamma && beta && y, "gn_small: null argument");
    DSD_CHECK(N >= 1 && HW >= 1 && C >= 32 && C % 32 == 0, "gn_small: bad problem size (GroupNorm32: C %% 32 == 0)");
    DSD_CHECK((int64_t)HW * (C / 32) <= 32768, "gn_small: a group of %d x %d values is beyond the kernel's reach (32768)", HW, C / 32);
    DSD_CHECK(act == ACT_NONE || act == ACT_SILU, "gn_small: bad activation %d", act);
    DSD_CHECK(!film || film_stride >= 2 * C, "gn_small: film_stride %d is smaller than 2 C = %d", film_stride, 2 * C);
    DSD_CHECK(reinterpret_cast<uintptr_t>(x) % 8 == 0 && reinterpret_cast<uintptr_t>(y) % 8 == 0, "gn_small: x / y must be 8-byte aligned");
    gn_small(x, N, HW, C, gamma, beta, eps, film, film_stride, act, y, s);
    DSD_HIP(hipStreamSynchronize(s));
    DSD_CATCH
}

int dsd_op_group_norm(const float* x, int N, int HW, int C, const float* gamma, const float* beta, float eps, int silu,
                      float* y, void* stream) {
    DSD_TRY
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = gn_nchunks(HW, C);
    Tmp part((size_t)N * nchunk * C * 2 * sizeof(double)), sc((size_t)N * C * sizeof(float)), sh((size_t)N * C * sizeof(float));
    gn_stats(x, N, HW, C, part.as<double>(), nchunk, s);
    GnSrc s0;
    s0.p = part.as<double>(); s0.chunks = nchunk; s0.c0 = 0; s0.c = C;
    gn_finalize(s0, GnSrc{}, N, HW, C, gamma, beta, eps, nullptr, 0, sc.as<float>(), sh.as<float>(), s);
    affine_act(x, N, HW, C, sc.as<float>(), sh.as<float>(), silu ? ACT_SILU : ACT_NONE, y, s);
    DSD_HIP(hipStreamSynchronize(s));
    DSD_CATCH
}

int dsd_op_gn_silu_conv_out1(const float* x, int N, int H, int W, int C, const float* gamma, const float* beta, float eps,
                             const float* w_oihw, const float* bias, float* y, void* stream) {
    DSD_TRY
    hipStream_t s = (hipStream_t)stream;
    DSD_CHECK(conv_out1_ok(C, 1, 3, 1), "gn_silu_conv_out1: %d input channels unsupported (a multiple of 64 up to 320)", C);
    const int HW = H * W, nchunk = gn_nchunks(HW, C);
    Tmp part((size_t)N * nchunk * C * 2 * sizeof(double)), sc((size_t)N * C * sizeof(float)), sh((size_t)N * C * sizeof(float));
    Tmp wp((size_t)C * 9 * sizeof(float));
    pack_ohwi(w_oihw, wp.as<float>(), 1, C, 3, s);
    gn_stats(x, N, HW, C, part.as<double>(), nchunk, s);
    GnSrc s0;
    s0.p = part.as<double>(); s0.chunks = nchunk; s0.c0 = 0; s0.c = C;
    gn_finalize(s0, GnSrc{}, N, HW, C, gamma, beta, eps, nullptr, 0, sc.as<float>(), sh.as<float>(), s);
    ConvOut1Args a;
    a.x = x; a.N = N; a.H = H; a.W = W; a.C = C; a.scale = sc.as<float>(); a.shift = sh.as<float>(); a.w = wp.as<float>();
    a.bias = bias; a.y = y;
    conv_out1(a, s);
    DSD_HIP(hipStreamSynchronize(s));
    DSD_CATCH
}

int dsd_op_qkv_attention(const float* qkv, int N, int T, int C, int heads, int new_order, int split, float* out, void* stream) {
    DSD_TRY
    DSD_CHECK(heads > 0 && C % heads == 0, "C=%d not divisible by heads=%d", C, heads);
    const int d = C / heads;
    AttnArgs a;
    a.N = N; a.Tq = a.Tk = T; a.heads = heads; a.d = d;
    a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C;
    a.scale_q = a.scale_k = 1.f / std::sqrt(std::sqrt((float)d));
    if (new_order) {
        a.q = qkv; a.k = qkv + C; a.v = qkv + 2 * C;
        a.q_hs = a.k_hs = a.v_hs = d;
    } else {
        a.q = qkv; a.k = qkv + d; a.v = qkv + 2 * d;
        a.q_hs = a.k_hs = a.v_hs = 3 * d;
    }
    a.out = out;
    a.split = split != 0;
    attention(a, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_attention(const float* q, const float* k, const float* v, int N, int Tq, int Tk, int heads, int d, int ldq, int ldk,
                     int ldv, int ldo, int q_hs, int k_hs, int v_hs, float scale_q, float scale_k, float scale_s, int split,
                     float* out, void* stream) {
    DSD_TRY
    DSD_CHECK(q && k && v && out, "attention: null argument");
    DSD_CHECK(N >= 1 && heads >= 1 && d >= 1 && q_hs >= 0 && k_hs >= 0 && v_hs >= 0, "attention: bad problem size");
    DSD_CHECK(ldq >= d && ldk >= d && ldv >= d && ldo >= heads * d && ldo % 4 == 0, "attention: row strides do not hold the heads");
    DSD_CHECK(reinterpret_cast<uintptr_t>(q) % 16 == 0 && reinterpret_cast<uintptr_t>(k) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(v) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0, "attention: pointers must be 16-byte aligned");
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.N = N; a.Tq = Tq; a.Tk = Tk; a.heads = heads; a.d = d;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.q_hs = q_hs; a.k_hs = k_hs; a.v_hs = v_hs;
    a.scale_q = scale_q; a.scale_k = scale_k; a.scale_s = scale_s;
    a.split = split != 0;
    attention_any(a, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_gemm_half(const float* x, const float* w, const float* bias, int M, int N, int K, int bf16, int epi, const float* gate,
                     int T, float* y, void* stream) {
    DSD_TRY
    DSD_CHECK(x && w && y && epi >= 0 && epi <= 2 && (epi != 2 || (gate && T >= 1)), "bad argument");
    hipStream_t s = (hipStream_t)stream;
    Tmp x16((size_t)M * K * 2), w16((size_t)N * K * 2), y16((size_t)M * N * 2);
    cast16(x, (int64_t)M * K, x16.p, bf16, s);
    cast16(w, (int64_t)N * K, w16.p, bf16, s);
    Gemm16Args a;
    a.x = x16.p; a.ldx = K; a.w = w16.p; a.bias = bias; a.M = M; a.N = N; a.K = K; a.bf16 = bf16; a.epi = epi;
    a.y16 = y16.p; a.ldy = N;
    if (epi == EPI16_GATED) {
        a.x32 = y; a.ldx32 = N; a.gate = gate; a.gate_stride = N; a.T = T;
    }
    gemm16(a, s);
    if (epi != EPI16_GATED) uncast16(y16.p, (int64_t)M * N, y, bf16, s);
    DSD_CATCH
}

int dsd_bench_gemm_half(int M, int N, int K, int bf16, int epi, int whatif, int iters, float* avg_ms) {
    DSD_TRY
    DSD_CHECK(iters >= 1 && avg_ms && M > 0 && N > 0 && K > 0, "bad argument");
    hipStream_t s = nullptr;
    Tmp xf((size_t)M * K * 4), wf((size_t)N * K * 4), x16((size_t)M * K * 2), w16((size_t)N * K * 2), y16((size_t)M * N * 2), b((size_t)N * 4);
    Tmp x32(epi == EPI16_GATED ? (size_t)M * N * 4 : 256), gate(epi == EPI16_GATED ? (size_t)N * 4 : 256);
    philox_normal(xf.as<float>(), (int64_t)M * K, 1, 0, s);
    philox_normal(wf.as<float>(), (int64_t)N * K, 2, 0, s);
    philox_normal(b.as<float>(), N, 3, 0, s);
    cast16(xf.as<float>(), (int64_t)M * K, x16.p, bf16, s);
    cast16(wf.as<float>(), (int64_t)N * K, w16.p, bf16, s);
    if (epi == EPI16_GATED) {
        DSD_HIP(hipMemsetAsync(x32.p, 0, (size_t)M * N * 4, s));
        philox_normal(gate.as<float>(), N, 4, 0, s);
    }
    Gemm16Args a;
    a.x = x16.p; a.ldx = K; a.w = w16.p; a.bias = b.as<float>(); a.M = M; a.N = N; a.K = K; a.bf16 = bf16; a.epi = epi;
    a.y16 = y16.p; a.ldy = N; a.x32 = x32.as<float>(); a.ldx32 = N; a.gate = gate.as<float>(); a.gate_stride = 0; a.T = M;
    gemm16_whatif(a, whatif, s);
    hipEvent_t e0, e1;
    DSD_HIP(hipEventCreate(&e0));
    DSD_HIP(hipEventCreate(&e1));
    DSD_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) gemm16_whatif(a, whatif, s);
    DSD_HIP(hipEventRecord(e1, s));
    DSD_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    DSD_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    DSD_CATCH
}

int dsd_bench_attention_half(int N, int T, int C, int heads, int bf16, int whatif, int iters, float* avg_ms) {
    DSD_TRY
    DSD_CHECK(iters >= 1 && avg_ms && heads > 0 && C % heads == 0, "bad argument");
    hipStream_t s = nullptr;
    const int d = C / heads;
    Tmp qf((size_t)N * T * 3 * C * 4), q16((size_t)N * T * 3 * C * 2), o16((size_t)N * T * C * 2);
    philox_normal(qf.as<float>(), (int64_t)N * T * 3 * C, 5, 0, s);
    cast16(qf.as<float>(), (int64_t)N * T * 3 * C, q16.p, bf16, s);
    Attn16Args a;
    a.N = N; a.Tq = a.Tk = T; a.heads = heads; a.d = d;
    a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C;
    a.q_hs = a.k_hs = a.v_hs = d;
    a.q = q16.p;
    a.k = (const char*)q16.p + (size_t)C * 2;
    a.v = (const char*)q16.p + (size_t)2 * C * 2;
    a.bf16 = bf16;
    a.out = o16.p;
    a.scale_q = 1.4426950408889634f / std::sqrt((float)d);   // scores of unit variance in base 2, as the qkv GEMM's epilogue leaves them
    attention16_whatif(a, whatif, s);
    hipEvent_t e0, e1;
    DSD_HIP(hipEventCreate(&e0));
    DSD_HIP(hipEventCreate(&e1));
    DSD_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) attention16_whatif(a, whatif, s);
    DSD_HIP(hipEventRecord(e1, s));
    DSD_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    DSD_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    DSD_CATCH
}

int dsd_op_attention_half(const float* qkv, int N, int T, int C, int heads, int bf16, float thr, float* out, void* stream) {
    DSD_TRY
    DSD_CHECK(qkv && out && heads > 0 && C % heads == 0, "C=%d not divisible by heads=%d", C, heads);
    hipStream_t s = (hipStream_t)stream;
    const int d = C / heads;
    Tmp q16((size_t)N * T * 3 * C * 2), o16((size_t)N * T * C * 2);
    cast16(qkv, (int64_t)N * T * 3 * C, q16.p, bf16, s);
    Attn16Args a;
    a.N = N; a.Tq = a.Tk = T; a.heads = heads; a.d = d;
    a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C;
    a.q_hs = a.k_hs = a.v_hs = d;
    a.q = q16.p;
    a.k = (const char*)q16.p + (size_t)C * 2;
    a.v = (const char*)q16.p + (size_t)2 * C * 2;
    a.scale_q = 1.4426950408889634f / std::sqrt((float)d);   // scores as base-2 logits
    a.thr = thr;
    a.bf16 = bf16;
    a.out = o16.p;
    attention16(a, s);
    uncast16(o16.p, (int64_t)N * T * C, out, bf16, s);
    DSD_CATCH
}

int dsd_op_timestep_embedding(const void* t, int t_is_float, int N, int dim, const float* freqs, float* y, void* stream) {
    DSD_TRY
    timestep_embedding(t, t_is_float, N, dim, y, (hipStream_t)stream, freqs);
    DSD_CATCH
}

int dsd_op_linear(const float* x, int N, int K, const float* w, const float* bias, int O, int act_in, float* y, void* stream) {
    DSD_TRY
    linear(x, N, K, K, w, bias, O, act_in, y, O, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_gaussian_sample(const float* moments, const float* noise, uint64_t philox_seed, int B, int E, int H, int W, float* z,
                           void* stream) {
    DSD_TRY
    DSD_CHECK(moments && z && B >= 0 && E >= 1 && H >= 1 && W >= 1, "bad argument");
    gaussian_sample(moments, noise, philox_seed, B, E, H * W, z, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_posterior_sample_scaled(const float* moments, const float* noise, uint64_t philox_seed, int B, int E, int H, int W,
                                   float scale, float* z, void* stream) {
    DSD_TRY
    DSD_CHECK(moments && z && B >= 0 && E >= 1 && H >= 1 && W >= 1, "bad argument");
    gaussian_sample(moments, noise, philox_seed, B, E, H * W, z, (hipStream_t)stream, scale);
    DSD_CATCH
}

int dsd_op_philox_normal(float* y, int64_t n, uint64_t seed, uint64_t step, void* stream) {
    DSD_TRY
    philox_normal(y, n, seed, step, (hipStream_t)stream);
    DSD_CATCH
}

int dsd_op_tail(int kind, void* const* ptrs, const int64_t* ints, const float* floats, void* stream) {
    DSD_TRY
    DSD_CHECK(kind >= 0 && kind < DSD_TAIL_NKINDS && ptrs && ints, "dsd_op_tail: bad argument (kind %d)", kind);
    hipStream_t s = (hipStream_t)stream;
    auto P = [&](int k) { return (float*)ptrs[k]; };
    auto I = [&](int k) { return (int)ints[k]; };
    const float f0 = floats ? floats[0] : 0.f;
    switch (kind) {
        case DSD_TAIL_SE_SCALE: se_scale(P(0), I(0), I(1), I(2), P(1), P(2), I(3), P(3), s); break;
        case DSD_TAIL_AVG_INTO: avg_into(P(0), P(1), P(2), P(3), f0, ints[0], I(1), P(4), I(2), I(3), I(4), s, ints[5], I(6)); break;
        case DSD_TAIL_NCHW_TO_NHWC: nchw_to_nhwc(P(0), I(0), I(1), I(2), P(1), s); break;
        case DSD_TAIL_NHWC_TO_NCHW: nhwc_to_nchw(P(0), I(0), I(1), I(2), P(1), s); break;
        case DSD_TAIL_AVGPOOL2: avgpool2(P(0), I(0), I(1), I(2), I(3), P(1), s); break;
        case DSD_TAIL_UPSAMPLE2: upsample2(P(0), I(0), I(1), I(2), I(3), P(1), s); break;
        case DSD_TAIL_GEGLU: geglu(P(0), ints[0], I(1), P(1), s); break;
        case DSD_TAIL_SOFTMAX_ROWS: softmax_rows(P(0), ints[0], I(1), f0, s); break;
        case DSD_TAIL_LN_MODULATE: ln_modulate(P(0), I(0), I(1), I(2), P(1), I(3), I(4), I(5), f0, P(2), s); break;
        case DSD_TAIL_LN_MODULATE16: ln_modulate16(P(0), I(0), I(1), I(2), P(1), I(3), I(4), I(5), f0, ptrs[2], I(6), s); break;
        case DSD_TAIL_LAYER_NORM: layer_norm(P(0), ints[0], I(1), P(1), P(2), f0, P(3), s); break;
        case DSD_TAIL_GATED_RESIDUAL: gated_residual(P(0), P(1), I(0), I(1), I(2), P(2), I(3), I(4), s); break;
        case DSD_TAIL_GELU_TANH: gelu_tanh(P(0), ints[0], s); break;
        case DSD_TAIL_PATCHIFY: patchify(P(0), I(0), I(1), I(2), I(3), I(4), P(1), s); break;
        case DSD_TAIL_UNPATCHIFY: unpatchify(P(0), I(0), I(1), I(2), I(3), I(4), P(1), s); break;
        case DSD_TAIL_ADD_ROWS_BROADCAST: add_rows_broadcast(P(0), P(1), I(0), ints[1], s); break;
        case DSD_TAIL_EMBED_ADD: embed_add(P(0), P(1), (const long long*)ptrs[2], I(0), I(1), P(3), s); break;
        case DSD_TAIL_ADD2: add2(P(0), P(1), ints[0], P(2), s); break;
        case DSD_TAIL_CAST16: cast16(P(0), ints[0], ptrs[1], I(1), s); break;
        default: uncast16(ptrs[0], ints[0], P(1), I(1), s); break;
    }
    DSD_CATCH
}

}  // extern "C"
