// net.h — parameter store, workspace planner and launch-plan builder of libdsdiff.
#pragma once
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dsdiff.h"
#include "kernels.h"

namespace dsd {

struct Param {
    std::string name;
    std::vector<int64_t> shape;
    int64_t numel = 0;
    size_t off = 0;      // byte offset into the parameter slab
    bool pack3x3 = false;  // stored OHWI on device
    bool set = false;
    int region = 0;      // 0 general, 1 emb_layers weights (contiguous), 2 emb_layers biases (contiguous)
};

// GroupNorm statistics that travel with a tensor: per-column partial sums (kernels.h GnSrc) of its channels [c0, c0+c),
// written by the op that produced those channels.
struct StatRef {
    size_t off = (size_t)-1;   // arena offset of [n][chunks][c][2] doubles
    int chunks = 0, c0 = 0, c = 0;
    bool valid() const { return off != (size_t)-1; }
    size_t bytes(int n) const { return (size_t)n * chunks * c * 2 * sizeof(double); }
};

// Activation living in the workspace arena (NHWC).
struct Tn {
    size_t off = (size_t)-1;
    int n = 0, h = 0, w = 0, c = 0;
    int esz = 4;     // bytes per element: 4 (fp32) everywhere but the 16-bit activations of DSD_PREC_F16 / DSD_PREC_BF16
    StatRef st[2];   // st[0] covers channels [0, st[0].c); st[1] (concatenated tensors) the rest
    bool valid() const { return off != (size_t)-1; }
    int64_t numel() const { return (int64_t)n * h * w * c; }
    size_t bytes() const { return (size_t)numel() * esz; }
    int hw() const { return h * w; }
};

// A GroupNorm whose statistics are finalised (per-(sample, channel) scale / shift in the arena) but not yet applied: either
// the apply pass makes a tensor of it, or the consuming convolution applies it while staging its input (ConvRoute::fuses_gn).
struct GnRef {
    Tn x;
    size_t scoff = 0, shoff = 0, sbytes = 0;
    int act = 0;
};

struct ArenaPlanner {
    struct Blk { size_t off, size; };
    std::vector<Blk> free_list;  // sorted by offset
    size_t top = 0, peak = 0;
    size_t alloc(size_t bytes);
    void release(size_t off, size_t bytes);
};

// Per-call bindings read by the plan's closures.
struct IO {
    const float* plane[4] = {nullptr, nullptr, nullptr, nullptr};  // noise, a, al, l input planes ([B,1,H,W] each)
    int64_t plane_bs[4] = {0, 0, 0, 0};
    const void* t = nullptr;
    int t_is_float = 0;
    float* out = nullptr;
    float* const* feats = nullptr;
    const float* x_nchw = nullptr;  // block handles
    const float* aux = nullptr;
    const float* aux2 = nullptr;
    const void* aux3 = nullptr;     // DSD_BLOCK_UNET with label_emb: y, int64 [B] (class table) or fp32 [B, width]
};

struct Plan {
    int B = 0, H = 0, W = 0, C = 0;
    int zero_al_l = 0, want_feats = 0, share = 0;
    int disc_unfused = 0;   // UNet_disc_Model: the bottleneck head composed from the older ops (DSD_DISC_UNFUSED) instead of disc.hip
    int aux_len = 0, aux_len2 = 0;
    // want_feats == 2: arena offsets of the tensors the forward keeps, NHWC, feat_n elements per sample.  UNet_disc_Model:
    // com_h1..4 / dist_h1..4; DSUnetModel: style[3], content[3], anatomy[2], lesion[2] (dsd_set_disentangle)
    size_t feat_off[10] = {};
    int64_t feat_n = 0;
    bool valid = false;
    std::vector<std::function<void(hipStream_t)>> ops;
    std::vector<signed char> op_lane;   // -1: the caller's stream after joining every lane; 0..3: encoder stream lanes (run concurrently)
    std::vector<std::string> op_name;   // the last parameter looked up before the op was emitted = the layer it belongs to (dsd_profile_op_name)
    std::vector<int> op_kind;        // index into kind_names
    std::vector<double> op_flops;    // algorithmic FLOPs of the op (0 for memory-bound ops)
    std::vector<double> op_bytes;    // algorithmic bytes (read+write) of the op (0 if not tracked)
    std::vector<std::string> kind_names;
    size_t arena_bytes = 0;
    double flops = 0.0;
    int launches = 0;
    int gen = 0;          // bumped every time the plan is rebuilt (a captured graph of an older plan is stale)
    int eager_runs = 0;   // forwards launched from the host since the plan was built (capture waits for the first one)
};

// What a captured forward bakes in besides the plan: every pointer the closures read from dsd_handle::io.
struct GraphKey {
    int plan_gen = -1;
    const void* ptr[13] = {};
    int64_t bs[4] = {};
    int t_is_float = 0;
    bool operator==(const GraphKey& o) const {
        if (plan_gen != o.plan_gen || t_is_float != o.t_is_float) return false;
        for (int i = 0; i < 13; ++i) if (ptr[i] != o.ptr[i]) return false;
        for (int i = 0; i < 4; ++i) if (bs[i] != o.bs[i]) return false;
        return true;
    }
};

// Device-resident forms made from a parameter at plan time.  The family says which arithmetic modes read an entry
// (net_drop_other_pieces keeps or frees by it); the source says which upload makes it stale (net_set_param).
enum WeightFamily {
    WF_BF16_PIECES,   // three bf16 pieces: bf16x3 / bf16x6, the fp32-grade layers of the half modes, sub-pixel and Winograd forms
    WF_F16_PIECES,    // three fp16 pieces (f16x3)
    WF_F16_COPY,      // one fp16 copy of a Linear weight (f16)
    WF_BF16_COPY,     // one bf16 copy of a Linear weight (bf16)
};
struct DerivedWeight {
    void* ptr = nullptr;
    size_t bytes = 0;
    std::string source;   // name of the parameter it was made from
    WeightFamily family = WF_BF16_PIECES;
};

struct dsd_net;
using Net = dsd_net;

}  // namespace dsd

struct dsd_handle {
    int device = 0;
    bool is_block = false;
    bool is_disc = false;   // dsd_create_disc: UNet_disc_Model (four live streams, shared bottleneck head) instead of DSUnetModel
    int block_kind = -1;
    std::vector<int32_t> iargs;
    dsd_config cfg{};
    // parameters
    std::vector<dsd::Param> params;
    std::unordered_map<std::string, int> pidx;
    char* slab = nullptr;
    size_t slab_bytes = 0;
    float* staging = nullptr;
    size_t staging_bytes = 0;
    size_t emb_w_off = 0, emb_b_off = 0;  // start of the contiguous emb_layers regions
    int64_t emb_total = 0;                 // sum of emb_layers output widths
    // workspace + plan
    char* arena = nullptr;
    size_t arena_cap = 0;
    dsd::Plan plan;
    dsd::IO io;
    // sampling scratch, sized by the loop's binding (api.cpp LoopBinding: rows = B, or 2B under classifier-free guidance)
    float* tbuf = nullptr;     // [rows] timesteps (fp32)
    float* mout = nullptr;     // [rows,out_ch,H,W]: the binding's out_u (rows [0,B), guided only) and out_c halves
    float* zplane = nullptr;   // [H*W] zeros
    float* dpm_m = nullptr;    // DPM-Solver step body: m_k, m_{k-1} [B,Cz*H*W] each + thresholds [B]
    float* lat_in = nullptr;   // latent binding (UNET block): the denoiser's NCHW input [rows,Cz+Cc,h,w]; channels [0,Cz) are the state
    // dsd_set_conditioning: the caller's bundle (device pointers, read when a latent loop binds) and the loop's persistent
    // copies of `rows` rows each (uncond half first under guidance), which io.aux2 / io.aux3 point at
    dsd_conditioning cond{};
    bool has_cond = false;
    // dsd_set_trace: the kept iterations (copied) and the caller's two output buffers, read by dsd_sample / dsd_sample_plms
    std::vector<int32_t> trace_keep;
    float* trace_x = nullptr;
    float* trace_x0 = nullptr;
    bool has_trace = false;
    // dsd_set_disentangle: the rider dsd_eval_loss reads on a DSUnetModel handle
    dsd_disentangle disen{};
    bool has_disen = false;
    float* ctx_buf = nullptr;  // [rows, tokens, context_dim]
    float* y_buf = nullptr;    // [rows] int64 or [rows, y_width] fp32
    float* cfg_io = nullptr;   // guided four-stream binding: state [2B,1,H,W] then conditions [2B,Cc,H,W] (uncond half first)
    float* dpm_prog = nullptr; // DPM-Solver program: three history planes + the base-state plane [B,Cz*H*W] each + thresholds [B]
    // one adaptive trial (dsd_sample_dpm_adaptive_trial): the error kernel's partial sums and its B results on the device, and the
    // pinned host buffer they are read back through
    float* dpm_adapt = nullptr;
    float* dpm_adapt_host = nullptr;
    int dpm_adapt_host_n = 0;
    // PLMS loops: three history planes [B,Cz,h,w] (a ring: iteration k >= 1 reads its newest prediction from plane (k-1) % 3 and
    // retires plane k % 3) followed by the threshold's per-block partial sums.  The history outlives a call, so a later call
    // with first_step > 0 continues it: plms_next is the iteration it is valid for (-1: none), for plms_B samples of plms_n
    // elements under a schedule of plms_steps iterations.
    float* plms_hist = nullptr;
    float* bpd_buf = nullptr;  // variational-bound loops: the per-block partial sums (doubles), then the four-stream loop's x_t state [B,H*W]
    float* loss_buf = nullptr; // dsd_eval_loss: the reductions' partial sums (doubles), then the four-stream call's x_t state [B,H*W]
    size_t loss_cap = 0;
    int plms_next = -1, plms_B = 0, plms_steps = 0;
    int64_t plms_n = 0;
    float* freqs = nullptr;    // [model_channels/2] optional timestep-embedding frequency table (host-supplied)
    int64_t* slice_ids = nullptr;  // [n_slice_ids] global slice index of every batch row (Philox counter base), optional
    int n_slice_ids = 0;
    // whole-forward hipGraph (sampling loops): captured on cap_stream after the first host-launched forward of a plan,
    // replayed on the caller's stream while plan + bound pointers stay the same
    // one event per stream dsd_set_param has been called on, re-recorded after every upload on that stream: plan-time
    // consumers of the slab (weight splitting, on the planning call's stream) wait on ALL of them, so uploads spread over
    // several non-blocking streams need no synchronisation by the caller
    std::unordered_map<hipStream_t, hipEvent_t> param_evs;
    hipStream_t last_param_stream = nullptr;
    bool any_param_upload = false;
    int use_graph = 0;
    int vae_fused_attention = 0;   // opt-in: the KL-VAE's AttnBlock as one fused attention() launch (no T x T score buffer)
    int use_winograd = 0;    // bf16x6 only, opt-in: 3x3 stride-1 convolutions as F(2,3) along the width (conv_wino.hip)
    int fuse_gn_stats = 1;   // GroupNorm statistics from the producing kernel's epilogue (0: always the standalone pass)
    int fuse_gn_apply = 1;   // GroupNorm + SiLU applied by the consuming 3x3 convolution while it stages its input (0: apply pass)
    // The four encoder streams are independent chains (UNet_DS_Diff/model.py:674-686).  Where their layers are too small to fill
    // 256 CUs (pixels per layer <= lane_pixels), the plan tags them with a lane and the executor runs lanes 1..3 on streams of
    // its own between a fork and a join event: four under-filled grids share the chip instead of queueing.  Same kernels,
    // same arithmetic: bit-identical to the sequential order.  dsd_set_stream_lanes.
    int use_lanes = 1;
    int lane_pixels = 16384;
    hipStream_t lane_stream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t lane_fork = nullptr, lane_join[3] = {nullptr, nullptr, nullptr};
    hipStream_t cap_stream = nullptr;
    hipGraphExec_t gexec = nullptr;
    dsd::GraphKey gkey;
    int graph_launches = 0, graph_captures = 0;
    // arithmetic mode of the convolutions (PREC_*): bf16 pieces of each conv weight are made lazily at plan time
    int precision = dsd::PREC_BF16X6;
    // dsd_sample only: evaluate the two all-zero-input streams of the C_in = 2 branch ONCE per step instead of once per
    // slice (same input, same timestep for every slice of the batch -> same result).  Off by default.
    int share_zero_streams = 0;
    // every derived form of a weight, made lazily at plan time (Builder::derived), keyed by layer name + form:
    // "<conv>" [3][numel] bf16 pieces, "<conv>#f16" the fp16 ones, "<conv>#sub" sub-pixel phase weights, "<conv>#wino" packed
    // Winograd weights, "<linear>.weight#h16" / "#b16" the 16-bit copy of the half-precision modes
    std::unordered_map<std::string, dsd::DerivedWeight> derived;
    int* ovf = nullptr;                              // device flag: fp16 range exceeded in f16x3 mode (ensure_ovf)
    // per-kernel profiling (dsd_profile_*): hipEvents around every op of the plan on the caller's stream
    bool profiling = false;
    std::vector<hipEvent_t> ev;
    std::vector<double> prof_ms, prof_flops, prof_bytes;   // per kind
    std::vector<int64_t> prof_calls;
    std::vector<float> prof_op_ms;                         // per op of the plan, last profiled forward
    std::vector<std::string> prof_names;
    int prof_runs = 0;
    // records of kernels a driver launches behind the plan's ops while profiling (dsd_eval_loss: loss_rows, vlb_terms_rows,
    // pair_mse_rows), served by dsd_profile_count / dsd_profile_get after the plan's kinds
    std::vector<std::string> prof_x_names;
    std::vector<double> prof_x_ms, prof_x_bytes;
    std::vector<int64_t> prof_x_calls;
    size_t tbuf_cap = 0, mout_cap = 0, zplane_cap = 0, dpm_m_cap = 0, lat_in_cap = 0, cfg_io_cap = 0, plms_hist_cap = 0, dpm_prog_cap = 0, dpm_adapt_cap = 0, bpd_cap = 0, ctx_cap = 0, y_cap = 0;

    float* P(const std::string& name) const;
    float* slab_at(size_t off) const { return reinterpret_cast<float*>(slab + off); }
    // typed view of the workspace arena at a planned offset (read when a closure runs: the arena may have been regrown since)
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(arena + off); }
    int* ensure_ovf();
    const dsd::Param& PP(const std::string& name) const;
};

namespace dsd {
void net_declare_params(dsd_handle* h);
void net_set_param(dsd_handle* h, const char* name, const float* src, const int64_t* shape, int ndim, int src_is_device,
                   hipStream_t s);
// s: the caller's stream — plan-time device work (splitting the weights into bf16 / fp16 pieces) is ordered after the
// parameter uploads the caller enqueued on it
void net_plan(dsd_handle* h, int B, int C, int H, int W, int zero_al_l, int want_feats, int aux_len, int aux_len2,
              int share = 0, hipStream_t s = nullptr);
void net_run(dsd_handle* h, hipStream_t s);
// every op of the plan in order; lane-tagged ops on the lane streams (fork / join through events) unless lanes are off
void net_launch_ops(dsd_handle* h, hipStream_t s);
// the same forward through the captured hipGraph when one is valid for the current plan and bindings (sampling loops)
void net_run_cached(dsd_handle* h, hipStream_t s);
void net_drop_graph(dsd_handle* h);
// DSD_BLOCK_UNET handles: built with use_spatial_transformer (a SpatialTransformer on `context` in every attention slot)
bool net_unet_has_spatial_transformer(const dsd_handle* h);
int net_unet_context_dim(const dsd_handle* h);   // 0 without spatial transformer
// label_emb of a DSD_BLOCK_UNET handle: kind 0 none, 1 int classes (width = num_classes), 2 continuous (width 1), 3 sequential
// (width = adm_in_channels)
void net_unet_label_emb(const dsd_handle* h, int* kind, int* width);
// frees the derived weights whose family (WeightFamily) `precision` does not read
void net_drop_other_pieces(dsd_handle* h, int precision);
size_t net_piece_bytes(const dsd_handle* h);
// f16x3 only: synchronises the stream and throws if an operand left the fp16 range during the work enqueued so far
void net_check_overflow(dsd_handle* h, hipStream_t s);
void net_free(dsd_handle* h);
}  // namespace dsd
