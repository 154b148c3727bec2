// Host-side engine: weight arena, execution plan, batched UNet forward and the rich-text step driver.
//
// One engine = one GPU = one HIP stream.  The reference (pure Python, one process, batch 1) runs the
// R+1 / R+3 UNet forwards of a rich-text step sequentially and rewires nn.Module hooks between them
// (models/region_diffusion.py:99-173, models/region_diffusion_sdxl.py:779-872).  Here all forwards of
// a step are ONE batched forward ("streams"); the hook families become per-stream mode words:
//   font-size hooks (rd.py:465-494)        -> fontsize[b]  : multiplier set used by cross-attention
//   selfattn capture + replacement hooks   -> qk_src[b]    : stream whose Q,K drive self-attention
//   resnet feature capture/injection       -> res_src[b]   : stream whose up_blocks.1.resnets.1 residual
//                                                            branch replaces this stream's (resnet.py:639-643)
// The text_ref stream is in the same batch, so its Q/K and resnet feature are available to the region
// streams at every layer without storing 5.9 GB of probabilities per step.
#include "common.h"
#include "../../include/rtdiff.h"
#include <map>
#include <mutex>
#include <vector>
#include <string>
#include <cmath>
#include <cstring>
#include <functional>
#include <algorithm>

static thread_local std::string g_create_error;
static thread_local std::string g_op_error;

// ------------------------------------------------------------------------------------------------
// memory helpers
struct Arena {           // bump allocator over one device allocation; base == nullptr => measuring pass
    char* base = nullptr;
    size_t off = 0, cap = 0;
    void* alloc(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        void* p = base ? base + off : (void*)(uintptr_t)(off + 256);   // fake non-null pointer when measuring
        off += bytes;
        if (base && off > cap) throw rt_error(RT_E_STATE, "arena overflow");
        return p;
    }
};

struct Workspace {       // stack allocator with mark/release; dry == true measures the peak only
    char* base = nullptr;
    size_t off = 0, cap = 0, peak = 0;
    bool dry = false;
    void* alloc(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        void* p = base ? base + off : (void*)(uintptr_t)(off + 256);
        off += bytes;
        if (off > peak) peak = off;
        if (!dry && off > cap) throw rt_error(RT_E_STATE, "workspace overflow");
        return p;
    }
    float* f32(size_t n) { return (float*)alloc(n * 4); }
    bf16_t* b16(size_t n) { return (bf16_t*)alloc(n * 2); }
    f16_t* f16(size_t n) { return (f16_t*)alloc(n * 2); }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
};
struct Scope {
    Workspace& w; size_t m;
    explicit Scope(Workspace& ws) : w(ws), m(ws.mark()) {}
    ~Scope() { w.release(m); }
};

// ------------------------------------------------------------------------------------------------
// plan
struct NormW { float* g = nullptr; float* b = nullptr; int C = 0; };
struct MatW { bf16_t* w = nullptr; float* b = nullptr; int N = 0, K = 0;      // packed [N, K] bf16 (+ f32 bias)
              bf16_t* w_up2 = nullptr; };                                      // up-sampler convolutions: the phase pack [4][N][4 Cin] (launch_pack_up2)

struct ResnetP {
    std::string name;
    int cin = 0, cout = 0;
    int temb_first = 0;          // prefix sum of cout over the resnets before this one (index into the per-forward temb buffer)
    NormW n1, n2;
    MatW c1, c2, temb, sc;
    bool has_sc = false;
};
struct LoraW { bf16_t* down = nullptr; bf16_t* up = nullptr; float* aor = nullptr; int K = 0, N = 0; };      // down [R, K], up [N, R], alpha / rank [R]
struct TBlockP {
    NormW ln1, ln2, ln3;
    MatW qk1, v1, out1, q2, k2, v2, out2, ff1, ff2;
    // LayerNorm folded into its consumers (gemm16.hip, "LNF"): W' = bf16(gamma W) in the place of w (no .b), and per weight row the pair
    // (s, c) = (row sum of W', b + W beta).  Derived from the packed arena by ensure_fold(); null when the block's width has no folded form.
    MatW qk1f, v1f, q2f, ff1f;
    float* qk1s = nullptr; float* v1s = nullptr; float* q2s = nullptr; float* ff1s = nullptr;
    bf16_t* kcache = nullptr;    // [maxP*KP, H*DP]   KP = 96 rows per 77-key chunk of rt_config.max_keys; a prompt's valid keys come first
    bf16_t* vtcache = nullptr;   // [H*DP, maxP*KP]
    // image prompts (rt_config.ip_tokens > 0; ipattn.hip): to_k_ip / to_v_ip packed like k2 / v2, and their caches, 16 rows per prompt slot
    MatW kip, vip;
    bf16_t* kipcache = nullptr;  // [maxP*16, H*DP]   a slot's valid image tokens come first, the rest of its 16 rows are zero
    bf16_t* vtipcache = nullptr; // [H*DP, maxP*16]
    // regional LoRA (rt_config.lora_rank > 0, main UNet only; lora.hip): the factors of the eight attention projections, packed like the
    // base weight they sit beside - index 4 a + {0 to_q, 1 to_k, 2 to_v, 3 to_out.0} of attn(a + 1)
    LoraW lora[8];
    LoraW lora_ff1, lora_ff2;    // rt_config.lora_targets = 1: ff.net.0.proj (`up` rows in ff1's GEGLU order) and ff.net.2; null otherwise
    // token-map attention store: index 0 = attn1, 1 = attn2
    std::string mod_name[2];
    float* store[2] = {nullptr, nullptr};
    int store_mode[2] = {0, 0};            // 0 off, 1 accumulate after the 10th call, 2 overwrite after the 10th call
    int store_calls[2] = {0, 0};
    int store_rows[2] = {0, 0}, store_cols[2] = {0, 0};
    size_t store_cap[2] = {0, 0};
    bool pag = false;                      // attn1 of this block is an applied module of rt_set_pag_layers
};
struct TransformerP {
    std::string name;
    int C = 0, heads = 0, d = 0, DP = 0, level = 0;
    NormW gn;
    MatW pin, pout;
    LoraW lora_pin, lora_pout;   // rt_config.lora_targets = 1: proj_in / proj_out, plain; null otherwise
    std::vector<TBlockP> blocks;
};
struct DownP { std::vector<ResnetP> res; std::vector<TransformerP> attn; bool has_attn = false, has_down = false; MatW down; int C = 0; };
struct UpP { std::vector<ResnetP> res; std::vector<TransformerP> attn; bool has_attn = false, has_up = false; MatW up; int C = 0; };

// One network: the time-embedding head, conv_in, the down blocks and the mid block, with its own time_emb_proj table and addition embeddings.
// The engine owns two, built (build_encoder) and walked (time_embed, encode) by the same code: the UNet - which alone has up blocks, their
// resnets in the same table - and, with rt_config.controlnet, the ControlNet's copy of the encoder under the prefix "controlnet.".
struct NetP {
    std::string prefix;
    bool adapters = true;        // its transformer blocks carry the image-prompt and LoRA slots (the UNet's do, the ControlNet's never)
    MatW conv_in, t1, t2, a1, a2;
    std::vector<DownP> down;
    ResnetP mid_r0, mid_r1;
    TransformerP mid_t;
    std::vector<UpP> up;
    // every resnet's time_emb_proj(silu(emb)) is computed by ONE launch at the start of a forward (launch_temb_all)
    std::vector<TembEntry> temb_tab;
    int temb_total = 0;
    TembEntry* temb_tab_dev = nullptr;
    float* aug_emb = nullptr;    // [maxP, temb_dim] (zeros when no addition embedding)
    template <typename F> void for_each_tblock(F f) {
        for (auto& d : down) for (auto& t : d.attn) for (auto& k : t.blocks) f(t, k);
        for (auto& k : mid_t.blocks) f(mid_t, k);
        for (auto& u : up) for (auto& t : u.attn) for (auto& k : t.blocks) f(t, k);
    }
};

// ControlNet (rt_config.controlnet): what it has beyond its NetP - the hint embedder in front and one 1x1 zero convolution per skip / for the
// mid block behind.  An engine without an active hint computes nothing for it.
struct ControlP {
    std::vector<MatW> zero;      // controlnet_down_blocks.{k}: one per skip, in the order unet_forward pushes them
    MatW zero_mid;               // controlnet_mid_block
    struct ConvF { float* w = nullptr; float* b = nullptr; int N = 0, CinP = 0; };      // fp32 [N][tap][CinP] + bias
    ConvF ce_in, ce_blocks[6], ce_out;     // controlnet_cond_embedding: kept in fp32 (control_conv3_kernel)
    int ce_ch[4] = {0, 0, 0, 0}, hint_ch = 3;
    // per image: the cached hint embedding [h w, C0] (fp32 as rt_control_embedding_read returns it; fp16 = the same accumulators rounded once,
    // the residual operand of controlnet.conv_in's epilogue) and the scale of every prompt slot
    float* emb_f32 = nullptr; f16_t* emb_f16 = nullptr;
    bool has_hint = false;
    int hint_h = 0, hint_w = 0;
    std::vector<float> scale;
};

struct WeightSlot {
    std::string name;
    std::vector<int64_t> shape;
    PackArgs pack;     // everything except src/src_dtype
    bf16_t* up2 = nullptr; int up2_cout = 0, up2_cin = 0;   // second pack of the same source tensor: the phase form of an up-sampler convolution
    bool bound = false;
};

static int pad_head_dim(int d) {
    if (d <= 32) return 32;
    if (d <= 64) return 64;
    if (d <= 96) return 96;
    if (d <= 160) return 160;
    throw rt_error(RT_E_UNSUPPORTED, "head dim > 160 not supported");
}

struct Tensor { f16_t* p; int C; };   // trunk tensor [B, HW, C]: fp16 in HBM (what the reference's fp16 pipelines carry), fp32 in every epilogue's arithmetic

struct FwdIn {
    int B = 0, h = 0, w = 0;
    const float* x[RT_MAXB];
    float scale[RT_MAXB];
    float t = 0;
    int prompt[RT_MAXB], fontsize[RT_MAXB], qk_src[RT_MAXB], res_src[RT_MAXB];
    float* eps_out = nullptr;    // [B, HW, 4] fp32
    int store_stream = -1;       // stream whose head-averaged attention maps are recorded (plain pass: the conditional one)
    bool control = false;        // the forward of the ControlNet's encoder copy (control_pass): no image-prompt term, no adapters
    int perturb[RT_MAXB] = {};   // perturbed-attention guidance: 1 = a twin, whose attention output at the applied attn1 modules (rt_set_pag_layers)
                                 // is its V (pag.hip); the twins trail the list.  Never set on the control copy.
};

extern int g_store_own_stats;
// The statistics hand-over of a recorded self-attention layer (attn_store.hip, stats_ready; cross-attention: cross_route): the launch leaves (m, 1 / (H l))
// of the recorded stream when the store would run its statistics + apply pair and the stream attends with its own Q / K, not an injected stream's.
static inline bool store_handover_self(int tokens, int DP, const int* qk_src, int stream) {
    return attn_store_takes_stats(tokens, tokens, DP) && qk_src[stream] == stream;
}
// step epilogue (defined in step.hip)
struct StepArgs;
struct SolverArgs;
void launch_step_epilogue(const StepArgs& a, const SolverArgs& d, hipStream_t st);
void launch_step_noise(unsigned long long seed, int step, int HW, float* out, unsigned* words, hipStream_t st);
// the SDE kinds share the DPM kinds' tables, x0 history and family rule; Euler ancestral shares Euler's tables, input scaling and family rule
static inline bool rt_sched_is_dpm(int kind) {
    return kind == RT_SCHED_DPMPP_1 || kind == RT_SCHED_DPMPP_2 || kind == RT_SCHED_DPMPP_SDE_1 || kind == RT_SCHED_DPMPP_SDE_2;
}
static inline bool rt_sched_is_euler(int kind) { return kind == RT_SCHED_EULER || kind == RT_SCHED_EULER_A; }
static inline bool rt_sched_is_stoch(int kind) { return kind == RT_SCHED_EULER_A || kind == RT_SCHED_DPMPP_SDE_1 || kind == RT_SCHED_DPMPP_SDE_2; }
void launch_gather_add_rows(const float* base, const float* table, const int* /*host*/ idx, float* out, int B, int C, hipStream_t st);
void launch_inject_add(f16_t* out, const f16_t* sc, const float* hres, const int* /*host*/ src, int B, size_t per_batch, hipStream_t st);
void launch_nhwc4_to_nchw(const float* in, float* out, int B, int HW, hipStream_t st);
void launch_trace_f16_nhwc_to_nchw(const f16_t* in, float* out, int B, int C, int HW, hipStream_t st);
void launch_pad_ctx(const float* ctx, bf16_t* out, int rows_valid, int rows_out, int D, hipStream_t st);
void launch_background_blend(float* lat, const float* lat_ref, const float* mask_last, int n, hipStream_t st);
void launch_noise_latents(float* lat, float* lat_ref, const float* x0, const float* noise, float a, float b, int n, hipStream_t st);
void launch_source_blend(float* lat, const float* x0, const float* noise, const float* keep, float a, float b, int HW, hipStream_t st);

#include "step.h"
#include "guided.h"
#include "vae.h"

// ------------------------------------------------------------------------------------------------
// The route of an attn2 (cross-attention) launch: the ONE place that decides which kernel runs it and whether the launch may leave its
// softmax statistics for the token-map store - asked by the UNet forward, every rt_op_* entry that launches cross-attention and the host-only
// rt_op_cross_route.  A function of the layer's shape and the streams' key counts (77 per chunk), never of the capacity: prompt_rows (96 per
// chunk the caches hold) is only the stride between prompts, so a launch of 77-key streams takes the kernels - and gives the bits - of an
// engine built for one chunk.  (Except the one-launch forms: their kernels hold the 96-row stride.)
struct CrossRoute {
    enum Kind {
        GENERIC,        // attn_kernel
        CROSS77,        // head dim 64, every stream with 77 keys: cross77_kernel behind the plain to_q GEMM (debug bit 19 clear)
        RUNS,           // that shape with DIFFERENT key counts: every run of streams on the kernel of its own count (cross_run)
        XATTN_FUSED,    // RT_PROBES builds: to_q + attention as one launch (gemm16.hip, EPI_XATTN: the Q tile stays in LDS; debug bit 4 clear)
        XBLOCK,         // RT_PROBES builds: to_q, attention AND to_out + residual as one launch (xblock.hip; debug bit 16 set)
    } kind;
    bool handover;      // the launch may leave the recorded stream's statistics (cross77_kernel only; debug bit 17 clear)
};
// d: the head dim (a caller that only knows the padded DP passes that: every kernel but attn_kernel needs DP = 64).  The two-launch forms
// stay with a LayerNorm folded into to_q, a recorded token map (the store reads Q from HBM) and an entry that is handed Q (with_to_q = false).
static CrossRoute cross_route(int C, int heads, int d, int DP, int tokens, int prompt_rows, const int* nkeys, int B, bool folded, bool recorded,
                              bool with_to_q = true) {
    const bool all77 = std::all_of(nkeys, nkeys + B, [](int c) { return c == 77; });
    const bool c77ok = gemm_cross77_enabled() && cross77_supported(heads, DP, tokens, prompt_rows, 77) && d == 64;
    const bool one_launch = with_to_q && all77 && prompt_rows == 96 && !folded && !recorded;
    CrossRoute r{CrossRoute::GENERIC, false};
    if (one_launch && gemm_xblock_enabled() && xblock_supported(C, heads, DP, tokens) && d == 64) r.kind = CrossRoute::XBLOCK;
    else if (one_launch && !c77ok && gemm_xattn_enabled() && xattn_fused_supported(C, heads, DP, tokens)) r.kind = CrossRoute::XATTN_FUSED;
    else if (c77ok) r.kind = all77 ? CrossRoute::CROSS77 : CrossRoute::RUNS;
    r.handover = recorded && r.kind == CrossRoute::CROSS77 && !g_store_own_stats;
    return r;
}
// RUNS (prompts of one to three 77-token windows in one launch): the kernel of a stream is a function of its OWN key count - maximal runs
// of 77-key streams go to cross77_kernel (*kernel = 1), the runs of longer ones to crossmw_kernel (2; cross77.hip: all 154 / 231 keys of the
// head in LDS; 0 = attn_kernel) - so a one-window stream computes the bits it computes alone, whatever its neighbours are.  Returns the run's end.
static int cross_run(const int* nkeys, int B, int b0, int heads, int DP, int tokens, int prompt_rows, int* kernel) {
    const bool one = nkeys[b0] == 77;
    *kernel = one ? 1 : crossmw_supported(heads, DP, tokens, prompt_rows) ? 2 : 0;
    while (b0 < B && (nkeys[b0] == 77) == one) ++b0;
    return b0;
}
// The attention launch of the two-launch routes.  A run is the same launch on offset Q / O pointers; no statistics hand-over on RUNS.
static void launch_cross(const AttnArgs& a, const CrossRoute& route, hipStream_t st) {
    if (route.kind == CrossRoute::CROSS77) return launch_cross77(a, st);
    if (route.kind == CrossRoute::GENERIC) return launch_attention(a, st);
    RT_REQUIRE(route.kind == CrossRoute::RUNS, "launch_cross: the one-launch forms include to_q and are launched by their callers");
    for (int b0 = 0, b1, kernel; b0 < a.B; b0 = b1) {
        b1 = cross_run(a.nkeys, a.B, b0, a.H, a.DP, a.N, a.NK, &kernel);
        AttnArgs r = a;
        r.B = b1 - b0; r.stats = nullptr;
        r.Q = a.Q + (size_t)b0 * a.N * a.ldq; r.O = a.O + (size_t)b0 * a.N * a.ldo;
        for (int i = 0; i < RT_MAXB; ++i) {
            const int b = b0 + i < a.B ? b0 + i : b0;
            r.q_src[i] = i; r.k_src[i] = a.k_src[b]; r.v_src[i] = a.v_src[b]; r.wset[i] = a.wset[b]; r.nkeys[i] = i < r.B ? a.nkeys[b] : 0;
        }
        if (kernel == 1) launch_cross77(r, st); else if (kernel == 2) launch_crossmw(r, st); else launch_attention(r, st);
    }
}

// ------------------------------------------------------------------------------------------------
// Launch arguments of the UNet's kernels, built HERE for rt_engine and for the stateless rt_op_* entries alike (as vae.h does for rt_vae), so
// that an entry launches what the forward launches.  zero: the caller's zero page.  hw: the tokens ONE stream contributes (0: not known): the
// split-K rule and the tile classes are keyed on it, so that results are batch invariant.  (temb_ld is only read with temb set.)
static GemmArgs unet_dense_args(const bf16_t* zero, int hw, const bf16_t* A, int lda, const MatW& W, int M, void* out, int ldo, int epi,
                                const void* res = nullptr, int ldres = 0, const float* temb = nullptr, int rows_per_batch = 0) {
    GemmArgs g{}; g.A = A; g.W = W.w; g.bias = W.b; g.out = out; g.res = res; g.temb = temb; g.zero = zero;
    g.mode = A_DENSE; g.epi = epi; g.M = M; g.N = W.N; g.K = W.K; g.lda = lda; g.ldw = W.K; g.ldo = ldo; g.ldres = ldres; g.temb_ld = W.N;
    g.rows_per_batch = rows_per_batch;
    if (hw > 0) { g.split_tiles = cdiv(hw, 128) * cdiv(W.N, 128); g.rows_per_stream = hw; }
    return g;
}
// V^T = Wv [HD, K] x X[M, K]^T -> [HD, M]
static GemmArgs unet_vt_args(const bf16_t* zero, int hw, const MatW& Wv, const bf16_t* X, int ldx, int M, bf16_t* out, int ldo) {
    GemmArgs g{}; g.A = Wv.w; g.W = X; g.bias = Wv.b; g.out = out; g.zero = zero;
    g.mode = A_DENSE; g.epi = EPI_BF16; g.M = Wv.N; g.N = M; g.K = Wv.K; g.lda = Wv.K; g.ldw = ldx; g.ldo = ldo; g.weights_on_rows = 1;
    if (hw > 0) { g.split_tiles = cdiv(Wv.N, 128) * cdiv(hw, 128); g.rows_per_stream = hw; }
    return g;
}
// 3x3 convolution (A_CONV3 / A_CONV3_S2: k3 s2 p1 / A_CONV3_UP2) of B maps [Hin, Win, CinP] to W.N channels
static GemmArgs unet_conv3_args(const bf16_t* zero, const bf16_t* in, int mode, const MatW& W, int B, int Hin, int Win, int CinP, void* out, int epi,
                                const void* res = nullptr, const float* temb = nullptr) {
    const int Hout = mode == A_CONV3_S2 ? (Hin + 1) / 2 : mode == A_CONV3_UP2 ? Hin * 2 : Hin;
    const int Wout = mode == A_CONV3_S2 ? (Win + 1) / 2 : mode == A_CONV3_UP2 ? Win * 2 : Win;
    GemmArgs g{}; g.A = in; g.W = W.w; g.W_up2 = mode == A_CONV3_UP2 ? W.w_up2 : nullptr; g.bias = W.b; g.out = out; g.res = res; g.temb = temb; g.zero = zero;
    g.mode = mode; g.epi = epi; g.M = B * Hout * Wout; g.N = W.N; g.K = W.K; g.lda = 0; g.ldw = W.K; g.ldo = W.N; g.ldres = W.N; g.temb_ld = W.N;
    g.rows_per_batch = Hout * Wout; g.Hin = Hin; g.Win = Win; g.Cin = CinP; g.Hout = Hout; g.Wout = Wout; g.split_tiles = cdiv(Hout * Wout, 128) * cdiv(W.N, 128);
    return g;
}
// LayerNorm fold of a launch (gemm16.hip, "LNF"): `part` set = consumer (A / X is xb, the un-normalised trunk as bf16; W the folded
// copy, `s` its (row sum, c) pairs); `emit` set = producer: leaves xb in `copy` and the partials of its output rows in `emit`
struct LnFold { const float* part = nullptr; int npair = 0; int ld = 0; const float* s = nullptr; float* emit = nullptr; bf16_t* copy = nullptr; };
static void ln_apply(GemmArgs& g, const LnFold* ln, int C) {
    if (!ln) return;
    g.ln_part = ln->part; g.ln_npair = ln->npair; g.ln_ld = ln->ld; g.ln_s = ln->s; g.ln_emit = ln->emit; g.ln_copy = ln->copy;
    g.ln_inv_c = 1.f / (float)C; g.ln_eps = 1e-5f;
}
// GroupNorm of the UNet: its chunk rule, the per-chunk partials [B, nchunk, G, 2] reduced by the apply kernel's own blocks
static GroupNormArgs unet_gn_args(const void* x1, const void* x2, int in_type /* 0 fp32, 1 bf16, 2 fp16 */, int C1, int C2, int G, int B, int HW,
                                  const float* gamma, const float* beta, float eps, int silu, bf16_t* out, bf16_t* raw, float* partial) {
    GroupNormArgs a{}; a.x1 = x1; a.x2 = x2; a.in_bf16 = in_type; a.C1 = C1; a.C2 = C2; a.G = G; a.B = B; a.HW = HW;
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.silu = silu; a.out = out; a.raw_out = raw; a.partial = partial;
    a.nchunk = groupnorm_nchunk(HW); a.rows_per_chunk = groupnorm_rows_per_chunk(HW); a.fuse_finalize = 1;
    return a;
}
// Attention: Q, K, V^T and O of a launch as AttnArgs lays them out
struct AttnIO { const bf16_t* Q; int ldq; const bf16_t* K; int ldk; const bf16_t* VT; int ldvt; bf16_t* O; int ldo; };
static AttnArgs attn_io_args(const AttnIO& io, int B, int H, int N, int NK, int nk_valid, int DP, int cross, float* stats, int stats_b) {
    AttnArgs a{}; a.Q = io.Q; a.ldq = io.ldq; a.K = io.K; a.ldk = io.ldk; a.VT = io.VT; a.ldvt = io.ldvt; a.O = io.O; a.ldo = io.ldo;
    a.B = B; a.H = H; a.N = N; a.NK = NK; a.nk_valid = nk_valid; a.DP = DP; a.cross = cross;
    if (stats) { a.stats = stats; a.stats_b = stats_b; }
    return a;
}
// attn1: stream b attends with Q / K of stream qk_src[b] and its own V.  stats non-null: the launch leaves the softmax statistics of
// stream stats_b there (store_handover_self).  (wabs / wsgn stay null: attn_kernel reads them for cross launches only.)
static AttnArgs unet_self_attn_args(const AttnIO& io, const int* qk_src, int B, int H, int N, int DP, float* stats, int stats_b) {
    AttnArgs a = attn_io_args(io, B, H, N, N, N, DP, 0, stats, stats_b);
    for (int b = 0; b < B; ++b) { a.q_src[b] = a.k_src[b] = qk_src[b]; a.v_src[b] = b; a.wset[b] = 0; }
    return a;
}
// attn2 behind the to_q GEMM: stream b reads K / V^T of prompt[b] (prompt_rows cached rows each, nkeys[b] = 77 c of them valid) with multiplier
// set wset[b] (-1: plain softmax, no tables).  (cross77_kernel masks by nk_valid and does not read nkeys, attn_kernel takes 0 as nk_valid.)
static AttnArgs unet_cross_attn_args(const AttnIO& io, const int* prompt, const int* wset, const int* nkeys, const float* wabs, const float* wsgn, int B,
                                     int H, int N, int prompt_rows, int DP, float* stats = nullptr /* CrossRoute.handover */, int stats_b = 0) {
    AttnArgs a = attn_io_args(io, B, H, N, prompt_rows, 77, DP, 1, stats, stats_b);
    a.wabs = wabs; a.wsgn = wsgn;
    for (int b = 0; b < B; ++b) { a.q_src[b] = b; a.k_src[b] = a.v_src[b] = prompt[b]; a.wset[b] = wset[b]; a.nkeys[b] = nkeys[b]; }
    return a;
}
// The token-map store of stream `stream` behind the launch `a`: its Q rows against its own K rows (attn1: [N, N]; NKpad is the caller's - the
// forward passes N, which launch_attn_store refuses unless N % 32 == 0, rt_op_attention_store_handover N padded to the store's 32-key step)
// or against the recorded prompt's own keys (attn2: [N, 77 c] out of its 96 c cached rows).  a.stats set: the launch left the statistics, the
// store runs its apply kernel only; attn1 passes its scratch either way.
static AttnStoreArgs unet_store_args(const AttnArgs& a, int stream, float* out, bool overwrite, float* self_scratch = nullptr, int self_NKpad = 0) {
    const int rows = a.cross ? 96 * (a.nkeys[stream] / 77) : a.N;
    AttnStoreArgs sa{}; sa.Q = a.Q; sa.ldq = a.ldq; sa.q_row0 = (long)stream * a.N; sa.K = a.K; sa.ldk = a.ldk;
    sa.k_row0 = a.cross ? (long)a.k_src[stream] * a.NK : (long)stream * a.N;
    sa.out = out; sa.H = a.H; sa.N = a.N; sa.NK = a.cross ? a.nkeys[stream] : a.N; sa.NKpad = a.cross ? rows : self_NKpad; sa.NKrows = rows; sa.DP = a.DP;
    sa.overwrite = overwrite; sa.stats = a.cross ? a.stats : self_scratch; sa.stats_ready = a.stats ? 1 : 0;
    return sa;
}
// The one-launch forms of attn2 (head dim 64, 77 of 96 cached keys; CrossRoute::XBLOCK / XATTN_FUSED): x = the LayerNorm'd tokens
static XBlockArgs unet_xblock_args(const bf16_t* x, const bf16_t* wq, const bf16_t* wo, const float* bo, const bf16_t* kc, const bf16_t* vt, int ldvt,
                                   const f16_t* res, f16_t* out, const float* wabs, const float* wsgn, const int* prompt, const int* wset, int B,
                                   int tokens, int C, int H) {
    XBlockArgs xa{}; xa.x = x; xa.wq = wq; xa.wo = wo; xa.bo = bo; xa.kc = kc; xa.vt = vt; xa.res = res; xa.out = out; xa.wabs = wabs; xa.wsgn = wsgn;
    xa.ldk = H * 64; xa.ldvt = ldvt; xa.ldres = C; xa.ldo = C; xa.M = B * tokens; xa.tokens = tokens; xa.nk_valid = 77; xa.C = C; xa.H = H;
    for (int b = 0; b < B; ++b) { xa.prompt[b] = prompt[b]; xa.wset[b] = wset[b]; }
    return xa;
}
static GemmArgs unet_xattn_args(const bf16_t* zero, const bf16_t* x, const bf16_t* wq, bf16_t* o, const bf16_t* kc, const bf16_t* vt, int ldvt,
                                const float* wabs, const float* wsgn, const int* prompt, const int* wset, int B, int tokens, int C, int H) {
    GemmArgs g{}; g.A = x; g.W = wq; g.out = o; g.zero = zero; g.mode = A_DENSE; g.epi = EPI_XATTN;
    g.M = B * tokens; g.N = H * 64; g.K = C; g.lda = C; g.ldw = C; g.ldo = H * 64; g.rows_per_stream = tokens;
    g.xa_k = kc; g.xa_vt = vt; g.xa_ldk = H * 64; g.xa_ldvt = ldvt; g.xa_tokens = tokens; g.xa_nk_valid = 77; g.xa_wabs = wabs; g.xa_wsgn = wsgn;
    for (int b = 0; b < B; ++b) { g.xa_prompt[b] = prompt[b]; g.xa_wset[b] = wset[b]; }
    return g;
}

// multistep state of the running schedule
struct SolverState {
    int pndm_counter = 0, pndm_nets = 0, pndm_head = 0;
    int dpm_lower_order_nums = 0, dpm_head = 0;     // DPM-Solver++: steps taken (capped at 2), history slot this step writes
    int steps_done = 0;
    void reset() { *this = SolverState{}; }
};

struct rt_engine {
    rt_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;       // the stream every launch of this engine goes to
    hipStream_t own_stream = nullptr;   // created by rt_create; rt_set_stream(NULL) returns to it
    std::string err;

    Arena arena;                 // packed weights only (this is what a multi-GPU launch broadcasts)
    Arena sarena;                // K/V caches + per-image sampler state
    Arena farena;                // LayerNorm-folded copies of the projections that consume a LayerNorm (derived on every rank from the
                                 // packed arena: not part of what a multi-GPU launch broadcasts)
    char* farena_base = nullptr;
    size_t farena_bytes = 0;
    bool fold_dirty = true;      // a weight was bound / the arena was filled since the last derivation
    char* arena_base = nullptr;
    char* sarena_base = nullptr;
    size_t arena_bytes = 0, sarena_bytes = 0;
    Workspace ws;
    bf16_t* zero = nullptr;

    std::vector<WeightSlot> slots;
    std::map<std::string, int> slot_index;

    // plan
    NetP unet, cnet;             // cnet: rt_config.controlnet
    std::vector<NetP*> nets;     // the networks this engine has, the UNet first: what is done "for both" loops over this
    MatW conv_out;
    NormW norm_out;
    ControlP ctl;                // rt_config.controlnet
    int temb_dim = 0;
    template <typename F> void for_each_tblock(F f) { unet.for_each_tblock(f); }      // the token-map store, the image prompts and the adapters are the UNet's alone

    // per-image state
    int n_prompts = 0;
    std::vector<int> prompt_keys;    // [max_prompts] valid keys of every resident prompt (77 per chunk); rt_create fills 77
    // rt_set_image_prompts: per prompt slot the valid image tokens and the scale of the image term (0 = the prompt has no image); rt_create
    // sizes both to max_prompts, rt_set_prompts zeroes the scales
    std::vector<int> ip_count;
    std::vector<float> ip_scale;
    // rt_set_lora_scales (rt_config.lora_rank > 0): [max_prompts][4] adapter scales per prompt slot, zeroed by rt_set_prompts; the padded bf16
    // prompt embeddings rt_set_prompts builds (kept, so that the attn2 caches can be rebuilt and adapted: [max_prompts * KP, D]); the adapter
    // of every rank column (device: the kernel reads it; all 0 until rt_set_lora_columns); whether the attn2 caches carry a LoRA term
    std::vector<float> lora_scale;
    bf16_t* lora_ctx = nullptr;
    int* lora_col = nullptr;
    bool lora_cache_dirty = false;
    bool lora_on(int slot) const {
        if (cfg.lora_rank <= 0) return false;
        for (int l = 0; l < 4; ++l) if (lora_scale[(size_t)slot * 4 + l] != 0.f) return true;
        return false;
    }
    int KP() const { return 96 * (cfg.max_keys / 77); }      // rows per prompt in the K / V^T caches and the multiplier tables
    float* wabs = nullptr;           // [2, KP]
    float* wsgn = nullptr;
    float* masks = nullptr;          // [R, 4, HW]
    int n_regions = 0, mask_hw = 0;
    float* lat = nullptr;            // [4, HW]
    float* lat_ref = nullptr;
    float* noise_pred = nullptr;     // [4, HW] CFG-combined prediction of the last step (guidance input)
    float* eps = nullptr;            // [maxB, HW, 4]
    float* ets = nullptr;            // PNDM history [4][2][4*HW]; DPM-Solver++ uses slots 0 / 1 as the x0 history of the two streams
    float* cur_sample = nullptr;     // PNDM [2][4*HW]
    int lat_h = 0, lat_w = 0;
    // schedule (host)
    int sched_kind = 0, num_inference_steps = 0;
    std::vector<float> timesteps, table;
    SolverState solver;              // reset by rt_set_schedule / rt_set_latents / rt_noise_latents
    // rt_set_prediction: what the UNet predicts (0 epsilon, 1 v) and the CFG rescale phi; (0, 0) launches nothing new.  Survive rt_set_schedule / rt_set_latents.
    int prediction_type = 0;
    float guidance_rescale = 0.f;
    float* gpred = nullptr;          // [2][HW][4] guided prediction of the main stream / the reference pair
    double* gpartials = nullptr;     // [cdiv(HW, 256)][8]
    float* gfactors = nullptr;       // [2]
    void guided_prepass(int i, StepArgs& a);
    // rt_set_freeu: (s1, s2, b1, b2) of the first two up blocks; all 1 = off, under which a forward launches nothing new.  Survives everything but rt_set_freeu.
    float fu_s[2] = {1.f, 1.f}, fu_b[2] = {1.f, 1.f};
    bool freeu_on() const { return fu_s[0] != 1.f || fu_s[1] != 1.f || fu_b[0] != 1.f || fu_b[1] != 1.f; }
    // Perturbed-attention guidance (rt_set_pag_layers / rt_set_pag_scales; pag.hip): sigma per prompt slot (all 0 = off: no twin stream, no
    // new launch) and the number of applied attn1 modules (their blocks carry TBlockP::pag).  The scales are reset by rt_set_prompts, the
    // layers survive everything but rt_set_pag_layers.  No weight, no persistent buffer.
    std::vector<float> pag_scale;
    int pag_layers = 0;
    bool pag_on() const { for (float v : pag_scale) if (v != 0.f) return true; return false; }
    unsigned long long noise_seed = 0;              // stochastic samplers: key of the per-step noise field (rt_set_noise_seed); survives rt_set_schedule / rt_set_latents

    // optional per-launch HIP-event profiling of the MFMA kernels (bench.py roofline leg)
    struct ProfRec { int cls; double flops, bytes; hipEvent_t a, b; };
    bool profiling = false;
    std::vector<ProfRec> prof;
    void prof_begin(int cls, double flops, double bytes = 0.0) {
        if (!profiling) return;
        ProfRec r; r.cls = cls; r.flops = flops; r.bytes = bytes;
        HIP_CHECK(hipEventCreate(&r.a)); HIP_CHECK(hipEventCreate(&r.b));
        HIP_CHECK(hipEventRecord(r.a, stream));
        prof.push_back(r);
    }
    void prof_end() { if (profiling) HIP_CHECK(hipEventRecord(prof.back().b, stream)); }

    // trace seam (rt_unet_forward_trace): the modules whose trunk tensor can be read, in execution order (build_plan), and the request of
    // the running forward (empty name: none).  trace_point is a no-op unless the forward was asked for exactly that module.
    struct TraceMod { std::string name; int C; int shift; };      // grid of the module's output = the latent grid >> shift
    std::vector<TraceMod> trace_mods;
    std::string trace_name;
    float* trace_out = nullptr;
    bool tracing() const { return !trace_name.empty() && !dry(); }      // (callers that have to BUILD a module's name ask first: an untraced forward allocates nothing)
    void trace_point(const std::string& name, const Tensor& x, int B, int HW) {
        if (!tracing() || trace_name != name) return;
        launch_trace_f16_nhwc_to_nchw(x.p, trace_out, B, x.C, HW, stream);
    }

    // ---------------------------------------------------------------------------- plan building
    void add_slot(const std::string& name, std::vector<int64_t> shape, const PackArgs& pk) {
        WeightSlot s; s.name = name; s.shape = std::move(shape); s.pack = pk;
        slot_index[name] = (int)slots.size();
        slots.push_back(s);
    }
    static PackArgs pk_matrix(void* dst, int rows, int cols, int ld, long s_r) {
        PackArgs p{}; p.dst = dst; p.dst_f32 = 0; p.rows = rows; p.cols = cols; p.ld_dst = ld;
        p.row_map = PACK_ROWS_ID; p.c_inner = cols; p.ci_valid = cols; p.s_r = s_r; p.s_co = 0; p.s_ci = 1; p.scale = 1.f;
        return p;
    }
    static PackArgs pk_vec(void* dst, int n) {
        PackArgs p{}; p.dst = dst; p.dst_f32 = 1; p.rows = n; p.cols = 1; p.ld_dst = 1;
        p.row_map = PACK_ROWS_ID; p.c_inner = 1; p.ci_valid = 1; p.s_r = 1; p.s_co = 0; p.s_ci = 0; p.scale = 1.f;
        return p;
    }
    NormW mk_norm(const std::string& name, int C) {
        NormW n; n.C = C;
        n.g = (float*)arena.alloc((size_t)C * 4); n.b = (float*)arena.alloc((size_t)C * 4);
        add_slot(name + ".weight", {C}, pk_vec(n.g, C));
        add_slot(name + ".bias", {C}, pk_vec(n.b, C));
        return n;
    }
    // nn.Linear [N, K] (optionally a 1x1 conv [N, K, 1, 1])
    MatW mk_linear(const std::string& name, int K, int N, bool bias, bool as_conv1x1 = false) {
        MatW m; m.N = N; m.K = K;
        m.w = (bf16_t*)arena.alloc((size_t)N * K * 2);
        std::vector<int64_t> shp = as_conv1x1 ? std::vector<int64_t>{N, K, 1, 1} : std::vector<int64_t>{N, K};
        add_slot(name + ".weight", shp, pk_matrix(m.w, N, K, K, K));
        if (bias) { m.b = (float*)arena.alloc((size_t)N * 4); add_slot(name + ".bias", {N}, pk_vec(m.b, N)); }
        return m;
    }
    // nn.Conv2d 3x3 [Cout, Cin, 3, 3] -> [Cout, 9*CinP], K index = tap*CinP + c
    // up2 (Upsample2D's convolution, Cin % 64 == 0): the SAME slot also fills the phase pack [4][Cout][4 Cin] next to the 3x3 pack - in
    // the weight arena (32 Cin Cout bytes), so that the one broadcast of a multi-GPU launch carries it; both are re-derived by every bind
    MatW mk_conv3(const std::string& name, int Cin, int Cout, bool up2 = false) {
        const int CinP = (Cin + 7) & ~7;
        MatW m; m.N = Cout; m.K = 9 * CinP;
        m.w = (bf16_t*)arena.alloc((size_t)Cout * m.K * 2);
        PackArgs p{}; p.dst = m.w; p.rows = Cout; p.cols = m.K; p.ld_dst = m.K; p.row_map = PACK_ROWS_ID;
        p.c_inner = CinP; p.ci_valid = Cin; p.s_r = (long)Cin * 9; p.s_co = 1; p.s_ci = 9; p.scale = 1.f;
        add_slot(name + ".weight", {Cout, Cin, 3, 3}, p);
        if (up2 && Cin % 64 == 0) {
            m.w_up2 = (bf16_t*)arena.alloc((size_t)16 * Cout * Cin * 2);
            WeightSlot& sl = slots.back(); sl.up2 = m.w_up2; sl.up2_cout = Cout; sl.up2_cin = Cin;
        }
        m.b = (float*)arena.alloc((size_t)Cout * 4);
        add_slot(name + ".bias", {Cout}, pk_vec(m.b, Cout));
        return m;
    }
    // the hint embedder's convolutions: the same slot layout as mk_conv3, packed as fp32
    ControlP::ConvF mk_conv3_f32(const std::string& name, int Cin, int Cout) {
        const int CinP = (Cin + 7) & ~7;
        ControlP::ConvF m; m.N = Cout; m.CinP = CinP;
        m.w = (float*)arena.alloc((size_t)Cout * 9 * CinP * 4);
        PackArgs p{}; p.dst = m.w; p.dst_f32 = 1; p.rows = Cout; p.cols = 9 * CinP; p.ld_dst = 9 * CinP; p.row_map = PACK_ROWS_ID;
        p.c_inner = CinP; p.ci_valid = Cin; p.s_r = (long)Cin * 9; p.s_co = 1; p.s_ci = 9; p.scale = 1.f;
        add_slot(name + ".weight", {Cout, Cin, 3, 3}, p);
        m.b = (float*)arena.alloc((size_t)Cout * 4);
        add_slot(name + ".bias", {Cout}, pk_vec(m.b, Cout));
        return m;
    }
    ResnetP mk_resnet(NetP& net, const std::string& name, int cin, int cout) {      // net: whose time_emb_proj table it joins
        RT_REQUIRE(cin % 8 == 0 && cout % 8 == 0, "resnet: channel counts must be multiples of 8");
        ResnetP r; r.name = name; r.cin = cin; r.cout = cout;
        r.n1 = mk_norm(name + ".norm1", cin);
        r.c1 = mk_conv3(name + ".conv1", cin, cout);
        r.temb = mk_linear(name + ".time_emb_proj", temb_dim, cout, true);
        r.n2 = mk_norm(name + ".norm2", cout);
        r.c2 = mk_conv3(name + ".conv2", cout, cout);
        r.has_sc = cin != cout;
        if (r.has_sc) r.sc = mk_linear(name + ".conv_shortcut", cin, cout, true, true);
        r.temb_first = net.temb_total; net.temb_total += cout;
        net.temb_tab.push_back(TembEntry{r.temb.w, r.temb.b, cout, r.temb_first});
        return r;
    }
    // q/k/v projection with head padding d -> DP on the output rows
    MatW mk_headproj(const std::string& wname, int K, int H, int d, int DP, float scale, bf16_t* dst_rows, int ld) {
        MatW m; m.N = H * DP; m.K = K; m.w = dst_rows;
        PackArgs p = pk_matrix(dst_rows, H * DP, K, ld, K);
        p.row_map = PACK_ROWS_HEADPAD; p.rm_a = DP; p.rm_b = d; p.scale = scale;
        add_slot(wname + ".weight", {H * d, K}, p);
        return m;
    }
    MatW mk_outproj(const std::string& name, int C, int H, int d, int DP) {
        MatW m; m.N = C; m.K = H * DP;
        m.w = (bf16_t*)arena.alloc((size_t)C * m.K * 2);
        PackArgs p{}; p.dst = m.w; p.rows = C; p.cols = m.K; p.ld_dst = m.K; p.row_map = PACK_ROWS_ID;
        p.c_inner = DP; p.ci_valid = d; p.s_r = (long)H * d; p.s_co = d; p.s_ci = 1; p.scale = 1.f;
        add_slot(name + ".weight", {C, H * d}, p);
        m.b = (float*)arena.alloc((size_t)C * 4);
        add_slot(name + ".bias", {C}, pk_vec(m.b, C));
        return m;
    }
    // widths whose LayerNorms can be folded: C / 80 = 8 or 16 partial sums per token (SDXL's 640 / 1280; SD-v1.5's 320 / 960-free levels
    // have K = 320, outside the 16x16x32 family)
    static bool ln_fold_width(int C) { return C == 640 || C == 1280; }
    // W' / s / c of every folded projection from the packed arena (idempotent; a few ms, once per checkpoint)
    void ensure_fold() {
        if (!fold_dirty || !farena_base) { fold_dirty = false; return; }
        for (auto& sl : slots) if (!sl.bound) return;                   // not all weights are there yet
        for (NetP* net : nets) net->for_each_tblock([&](TransformerP& t, TBlockP& k) {
            if (!k.qk1f.w) return;
            launch_ln_fold_derive(k.qk1.w, k.qk1.K, k.qk1.b, k.ln1.g, k.ln1.b, k.qk1.N, k.qk1.K, k.qk1f.w, k.qk1s, stream);
            launch_ln_fold_derive(k.v1.w, k.v1.K, k.v1.b, k.ln1.g, k.ln1.b, k.v1.N, k.v1.K, k.v1f.w, k.v1s, stream);
            launch_ln_fold_derive(k.q2.w, k.q2.K, k.q2.b, k.ln2.g, k.ln2.b, k.q2.N, k.q2.K, k.q2f.w, k.q2s, stream);
            launch_ln_fold_derive(k.ff1.w, k.ff1.K, k.ff1.b, k.ln3.g, k.ln3.b, k.ff1.N, k.ff1.K, k.ff1f.w, k.ff1s, stream);
        });
        fold_dirty = false;
    }
    // adapters: the blocks get the image-prompt (rt_config.ip_tokens) and LoRA (rt_config.lora_rank) slots - NetP.adapters of their network
    TransformerP mk_transformer(const std::string& name, int C, int heads, int nlayers, int level, bool adapters) {
        TransformerP t; t.name = name; t.C = C; t.heads = heads; t.d = C / heads; t.DP = pad_head_dim(t.d); t.level = level;
        RT_REQUIRE(C % heads == 0, "channels not divisible by heads");
        const int HD = heads * t.DP, D = cfg.cross_attention_dim;
        const float qscale = (float)(std::pow((double)t.d, -0.5) * 1.4426950408889634);   // d^-1/2 * log2(e)
        t.gn = mk_norm(name + ".norm", C);
        t.pin = mk_linear(name + ".proj_in", C, C, true, !cfg.use_linear_projection);
        // rt_config.lora_targets = 1: the factors of a further module [N, K], packed like the base weight (up_rows: the row order of `up`)
        const bool lora_wide = cfg.lora_rank > 0 && cfg.lora_targets == 1 && adapters;
        auto mk_lora = [&](const std::string& module, int K, int N, int up_rows) {
            const int R = cfg.lora_rank;
            LoraW w; w.K = K; w.N = N;
            w.down = (bf16_t*)arena.alloc((size_t)R * K * 2);
            w.up = (bf16_t*)arena.alloc((size_t)N * R * 2);
            w.aor = (float*)arena.alloc((size_t)R * 4);
            add_slot("lora." + module + ".down.weight", {R, K}, pk_matrix(w.down, R, K, K, K));
            PackArgs p = pk_matrix(w.up, N, R, R, R); p.row_map = up_rows;
            add_slot("lora." + module + ".up.weight", {N, R}, p);
            add_slot("lora." + module + ".alpha_over_rank", {R}, pk_vec(w.aor, R));
            return w;
        };
        if (lora_wide) t.lora_pin = mk_lora(name + ".proj_in", C, C, PACK_ROWS_ID);
        for (int li = 0; li < nlayers; ++li) {
            const std::string b = name + ".transformer_blocks." + std::to_string(li);
            TBlockP k;
            k.mod_name[0] = b + ".attn1"; k.mod_name[1] = b + ".attn2";
            k.ln1 = mk_norm(b + ".norm1", C);
            bf16_t* qk = (bf16_t*)arena.alloc((size_t)2 * HD * C * 2);
            k.qk1 = mk_headproj(b + ".attn1.to_q", C, heads, t.d, t.DP, qscale, qk, C);
            mk_headproj(b + ".attn1.to_k", C, heads, t.d, t.DP, 1.f, qk + (size_t)HD * C, C);
            k.qk1.N = 2 * HD;
            bf16_t* v = (bf16_t*)arena.alloc((size_t)HD * C * 2);
            k.v1 = mk_headproj(b + ".attn1.to_v", C, heads, t.d, t.DP, 1.f, v, C);
            k.out1 = mk_outproj(b + ".attn1.to_out.0", C, heads, t.d, t.DP);
            k.ln2 = mk_norm(b + ".norm2", C);
            bf16_t* q2 = (bf16_t*)arena.alloc((size_t)HD * C * 2);
            k.q2 = mk_headproj(b + ".attn2.to_q", C, heads, t.d, t.DP, qscale, q2, C);
            bf16_t* k2 = (bf16_t*)arena.alloc((size_t)HD * D * 2);
            k.k2 = mk_headproj(b + ".attn2.to_k", D, heads, t.d, t.DP, 1.f, k2, D);
            bf16_t* v2 = (bf16_t*)arena.alloc((size_t)HD * D * 2);
            k.v2 = mk_headproj(b + ".attn2.to_v", D, heads, t.d, t.DP, 1.f, v2, D);
            if (cfg.ip_tokens > 0 && adapters) {
                bf16_t* kip = (bf16_t*)arena.alloc((size_t)HD * D * 2);
                k.kip = mk_headproj(b + ".attn2.to_k_ip", D, heads, t.d, t.DP, 1.f, kip, D);
                bf16_t* vip = (bf16_t*)arena.alloc((size_t)HD * D * 2);
                k.vip = mk_headproj(b + ".attn2.to_v_ip", D, heads, t.d, t.DP, 1.f, vip, D);
            }
            k.out2 = mk_outproj(b + ".attn2.to_out.0", C, heads, t.d, t.DP);
            k.ln3 = mk_norm(b + ".norm3", C);
            // GEGLU: nn.Linear(C, 8C); rows interleaved per 64-block [32 value | 32 gate]
            k.ff1.N = 8 * C; k.ff1.K = C;
            k.ff1.w = (bf16_t*)arena.alloc((size_t)8 * C * C * 2);
            k.ff1.b = (float*)arena.alloc((size_t)8 * C * 4);
            RT_REQUIRE((4 * C) % 32 == 0, "GEGLU width must be a multiple of 32");
            { PackArgs p = pk_matrix(k.ff1.w, 8 * C, C, C, C); p.row_map = PACK_ROWS_GEGLU; add_slot(b + ".ff.net.0.proj.weight", {8 * C, C}, p); }
            { PackArgs p = pk_vec(k.ff1.b, 8 * C); p.row_map = PACK_ROWS_GEGLU; add_slot(b + ".ff.net.0.proj.bias", {8 * C}, p); }
            k.ff2 = mk_linear(b + ".ff.net.2", 4 * C, C, true);
            k.kcache = (bf16_t*)sarena.alloc((size_t)cfg.max_prompts * KP() * HD * 2);
            k.vtcache = (bf16_t*)sarena.alloc((size_t)cfg.max_prompts * KP() * HD * 2);
            if (cfg.ip_tokens > 0 && adapters) {
                k.kipcache = (bf16_t*)sarena.alloc((size_t)cfg.max_prompts * 16 * HD * 2);
                k.vtipcache = (bf16_t*)sarena.alloc((size_t)cfg.max_prompts * 16 * HD * 2);
            }
            if (ln_fold_width(C)) {
                auto mkf = [&](const MatW& w, MatW& f, float*& sv) {
                    f.N = w.N; f.K = w.K;
                    f.w = (bf16_t*)farena.alloc((size_t)w.N * w.K * 2);
                    sv = (float*)farena.alloc((size_t)w.N * 8);
                };
                mkf(k.qk1, k.qk1f, k.qk1s); mkf(k.v1, k.v1f, k.v1s); mkf(k.q2, k.q2f, k.q2s); mkf(k.ff1, k.ff1f, k.ff1s);
            }
            if (cfg.lora_rank > 0 && adapters) {
                const int R = cfg.lora_rank;
                static const char* leaf[4] = {"to_q", "to_k", "to_v", "to_out.0"};
                for (int a = 0; a < 2; ++a)
                    for (int j = 0; j < 4; ++j) {
                        const std::string m = "lora." + b + ".attn" + std::to_string(a + 1) + "." + leaf[j];
                        LoraW& w = k.lora[4 * a + j];
                        const int Kin = a == 1 && (j == 1 || j == 2) ? D : C;      // attn2's to_k / to_v read the prompt embeddings
                        w.K = j == 3 ? HD : Kin; w.N = j == 3 ? C : HD;
                        w.down = (bf16_t*)arena.alloc((size_t)R * w.K * 2);
                        w.up = (bf16_t*)arena.alloc((size_t)w.N * R * 2);
                        w.aor = (float*)arena.alloc((size_t)R * 4);
                        if (j == 3) {      // to_out.0: `down` reads the head-padded attention output (mk_outproj's columns), `up` is plain
                            PackArgs p{}; p.dst = w.down; p.rows = R; p.cols = HD; p.ld_dst = HD; p.row_map = PACK_ROWS_ID;
                            p.c_inner = t.DP; p.ci_valid = t.d; p.s_r = (long)heads * t.d; p.s_co = t.d; p.s_ci = 1; p.scale = 1.f;
                            add_slot(m + ".down.weight", {R, heads * t.d}, p);
                            add_slot(m + ".up.weight", {C, R}, pk_matrix(w.up, C, R, R, R));
                        } else {           // to_q / to_k / to_v: `up` rows head-padded like mk_headproj's, to_q's with the same qscale
                            add_slot(m + ".down.weight", {R, Kin}, pk_matrix(w.down, R, Kin, Kin, Kin));
                            PackArgs p = pk_matrix(w.up, HD, R, R, R);
                            p.row_map = PACK_ROWS_HEADPAD; p.rm_a = t.DP; p.rm_b = t.d; p.scale = j == 0 ? qscale : 1.f;
                            add_slot(m + ".up.weight", {heads * t.d, R}, p);
                        }
                        add_slot(m + ".alpha_over_rank", {R}, pk_vec(w.aor, R));
                    }
            }
            if (lora_wide) {
                k.lora_ff1 = mk_lora(b + ".ff.net.0.proj", C, 8 * C, PACK_ROWS_GEGLU);
                k.lora_ff2 = mk_lora(b + ".ff.net.2", 4 * C, C, PACK_ROWS_ID);
            }
            t.blocks.push_back(k);
        }
        t.pout = mk_linear(name + ".proj_out", C, C, true, !cfg.use_linear_projection);
        if (lora_wide) t.lora_pout = mk_lora(name + ".proj_out", C, C, PACK_ROWS_ID);
        return t;
    }

    // The encoder of `net` under net.prefix, its slots in the order of the checkpoint; tm: its traceable modules in execution order
    void build_encoder(NetP& net, std::vector<TraceMod>& tm) {
        const int L = cfg.n_levels;
        const int* boc = cfg.block_out_channels;
        const std::string& P = net.prefix;
        net.conv_in = mk_conv3(P + "conv_in", cfg.in_channels, boc[0]);
        tm.push_back({P + "conv_in", boc[0], 0});
        net.t1 = mk_linear(P + "time_embedding.linear_1", boc[0], temb_dim, true);
        net.t2 = mk_linear(P + "time_embedding.linear_2", temb_dim, temb_dim, true);
        if (cfg.addition_text_time) {
            net.a1 = mk_linear(P + "add_embedding.linear_1", cfg.projection_class_embeddings_input_dim, temb_dim, true);
            net.a2 = mk_linear(P + "add_embedding.linear_2", temb_dim, temb_dim, true);
        }
        int out_c = boc[0];
        for (int i = 0; i < L; ++i) {
            DownP d; const int in_c = out_c; out_c = boc[i]; d.C = out_c;
            d.has_attn = cfg.down_has_attn[i]; d.has_down = i != L - 1;
            const std::string pre = P + "down_blocks." + std::to_string(i);
            for (int j = 0; j < cfg.layers_per_block[i]; ++j) {
                d.res.push_back(mk_resnet(net, pre + ".resnets." + std::to_string(j), j == 0 ? in_c : out_c, out_c));
                tm.push_back({d.res.back().name, out_c, i});
                if (d.has_attn) {
                    d.attn.push_back(mk_transformer(pre + ".attentions." + std::to_string(j), out_c, cfg.heads[i], cfg.transformer_layers[i], i, net.adapters));
                    tm.push_back({d.attn.back().name, out_c, i});
                }
            }
            if (d.has_down) { d.down = mk_conv3(pre + ".downsamplers.0.conv", out_c, out_c); tm.push_back({pre + ".downsamplers.0.conv", out_c, i + 1}); }
            net.down.push_back(d);
        }
        net.mid_r0 = mk_resnet(net, P + "mid_block.resnets.0", boc[L - 1], boc[L - 1]);
        net.mid_t = mk_transformer(P + "mid_block.attentions.0", boc[L - 1], cfg.heads[L - 1], cfg.transformer_layers[L - 1], L - 1, net.adapters);
        net.mid_r1 = mk_resnet(net, P + "mid_block.resnets.1", boc[L - 1], boc[L - 1]);
        for (const char* m : {"mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"}) tm.push_back({P + m, boc[L - 1], L - 1});
    }
    // The ControlNet behind the UNet's own weights (diffusers' ControlNetModel layout under "controlnet."): slots, arena offsets and caches of
    // the UNet are what they are without it.  Its traceable modules go where they run: behind the main mid block.
    void build_control_plan() {
        ctl = ControlP{};
        const int L = cfg.n_levels;
        const int* boc = cfg.block_out_channels;
        const std::string& P = cnet.prefix;
        static const int def_ch[4] = {16, 32, 96, 256};
        bool all0 = true;
        for (int i = 0; i < 4; ++i) all0 = all0 && cfg.control_embed_channels[i] == 0;
        for (int i = 0; i < 4; ++i) {
            ctl.ce_ch[i] = all0 ? def_ch[i] : cfg.control_embed_channels[i];
            RT_REQUIRE(ctl.ce_ch[i] >= 8 && ctl.ce_ch[i] % 8 == 0, "rt_create: control_embed_channels must be multiples of 8");
        }
        ctl.hint_ch = cfg.control_hint_channels ? cfg.control_hint_channels : 3;
        RT_REQUIRE(ctl.hint_ch >= 1 && ctl.hint_ch <= 64, "rt_create: control_hint_channels");
        std::vector<TraceMod> em, tm;      // em: the encoder's modules as build_encoder lists them; tm: all of the ControlNet's, the skips between them
        build_encoder(cnet, em);
        tm.push_back({P + "hint_embedding", boc[0], 0});
        tm.push_back(em[0]);
        ctl.ce_in = mk_conv3_f32(P + "controlnet_cond_embedding.conv_in", ctl.hint_ch, ctl.ce_ch[0]);
        for (int i = 0; i < 3; ++i) {
            ctl.ce_blocks[2 * i] = mk_conv3_f32(P + "controlnet_cond_embedding.blocks." + std::to_string(2 * i), ctl.ce_ch[i], ctl.ce_ch[i]);
            ctl.ce_blocks[2 * i + 1] = mk_conv3_f32(P + "controlnet_cond_embedding.blocks." + std::to_string(2 * i + 1), ctl.ce_ch[i], ctl.ce_ch[i + 1]);
        }
        ctl.ce_out = mk_conv3_f32(P + "controlnet_cond_embedding.conv_out", ctl.ce_ch[3], boc[0]);
        // one zero convolution per skip, in push order: conv_in, then every resnet (/ attention) and down-sampler; skip k's trace point
        // follows the module that produces the control copy's k-th skip
        int k = 0;
        auto zc = [&](int C, int shift) {
            ctl.zero.push_back(mk_linear(P + "controlnet_down_blocks." + std::to_string(k), C, C, true, true));
            tm.push_back({P + "skip." + std::to_string(k), C, shift});
            ++k;
        };
        zc(boc[0], 0);
        size_t di = 1;
        for (int i = 0; i < L; ++i) {
            for (int j = 0; j < cfg.layers_per_block[i]; ++j) {
                tm.push_back(em[di++]);
                if (cfg.down_has_attn[i]) tm.push_back(em[di++]);
                zc(boc[i], i);
            }
            if (i != L - 1) { tm.push_back(em[di++]); zc(boc[i], i + 1); }
        }
        ctl.zero_mid = mk_linear(P + "controlnet_mid_block", boc[L - 1], boc[L - 1], true, true);
        tm.insert(tm.end(), em.begin() + di, em.end());      // the mid block's three
        tm.push_back({P + "mid", boc[L - 1], L - 1});
        cnet.aug_emb = (float*)sarena.alloc((size_t)cfg.max_prompts * temb_dim * 4);
        ctl.scale.assign((size_t)std::max(1, cfg.max_prompts), 0.f);
        size_t at = 0;
        while (at < trace_mods.size() && trace_mods[at].name != "mid_block.resnets.1") ++at;
        trace_mods.insert(trace_mods.begin() + (at < trace_mods.size() ? at + 1 : at), tm.begin(), tm.end());
    }

    void build_plan() {
        slots.clear(); slot_index.clear(); trace_mods.clear();
        unet = NetP{}; cnet = NetP{}; cnet.prefix = "controlnet."; cnet.adapters = false;
        nets.assign(1, &unet);
        if (cfg.controlnet) nets.push_back(&cnet);
        const int L = cfg.n_levels;
        const int* boc = cfg.block_out_channels;
        temb_dim = boc[0] * 4;
        zero = (bf16_t*)sarena.alloc(256);
        build_encoder(unet, trace_mods);
        int out_c = boc[L - 1];
        for (int i = 0; i < L; ++i) {
            UpP u; const int prev = out_c; out_c = boc[L - 1 - i];
            const int in_c = boc[L - 1 - std::min(i + 1, L - 1)];
            u.C = out_c; u.has_attn = cfg.up_has_attn[i]; u.has_up = i != L - 1;
            const int nl = cfg.layers_per_block[L - 1 - i] + 1;
            const std::string pre = "up_blocks." + std::to_string(i);
            for (int j = 0; j < nl; ++j) {
                const int skip_c = j == nl - 1 ? in_c : out_c;
                const int res_in = j == 0 ? prev : out_c;
                u.res.push_back(mk_resnet(unet, pre + ".resnets." + std::to_string(j), res_in + skip_c, out_c));
                trace_mods.push_back({u.res.back().name, out_c, L - 1 - i});
                if (u.has_attn) {
                    u.attn.push_back(mk_transformer(pre + ".attentions." + std::to_string(j), out_c, cfg.heads[L - 1 - i], cfg.transformer_layers[L - 1 - i], L - 1 - i, true));
                    trace_mods.push_back({u.attn.back().name, out_c, L - 1 - i});
                }
            }
            if (u.has_up) { u.up = mk_conv3(pre + ".upsamplers.0.conv", out_c, out_c, true); trace_mods.push_back({pre + ".upsamplers.0.conv", out_c, L - 2 - i}); }
            unet.up.push_back(u);
        }
        norm_out = mk_norm("conv_norm_out", boc[0]);
        conv_out = mk_conv3("conv_out", boc[0], cfg.out_channels);
        trace_mods.push_back({"conv_out", cfg.out_channels, 0});
        // per-image sampler state
        const size_t HW = (size_t)cfg.latent_h * cfg.latent_w;
        unet.aug_emb = (float*)sarena.alloc((size_t)cfg.max_prompts * temb_dim * 4);
        wabs = (float*)sarena.alloc((size_t)2 * KP() * 4); wsgn = (float*)sarena.alloc((size_t)2 * KP() * 4);
        masks = (float*)sarena.alloc((size_t)RT_MAXB * 4 * HW * 4);
        lat = (float*)sarena.alloc(4 * HW * 4); lat_ref = (float*)sarena.alloc(4 * HW * 4); noise_pred = (float*)sarena.alloc(4 * HW * 4);
        eps = (float*)sarena.alloc((size_t)cfg.max_streams * HW * 4 * 4);
        ets = (float*)sarena.alloc((size_t)4 * 2 * 4 * HW * 4);
        cur_sample = (float*)sarena.alloc((size_t)2 * 4 * HW * 4);
        // guided-prediction pre-pass (guided.hip): behind everything else, so the buffers above keep their offsets
        gpred = (float*)sarena.alloc((size_t)2 * HW * 4 * 4);
        gpartials = (double*)sarena.alloc((size_t)cdiv((int)HW, 256) * RT_GUIDED_SERIES * 8);
        gfactors = (float*)sarena.alloc(2 * 4);
        if (cfg.lora_rank > 0) {         // regional LoRA: behind everything else as well
            lora_ctx = (bf16_t*)sarena.alloc((size_t)cfg.max_prompts * KP() * cfg.cross_attention_dim * 2);
            lora_col = (int*)sarena.alloc((size_t)cfg.lora_rank * 4);
        }
        if (cfg.controlnet) build_control_plan();
    }

    // ---------------------------------------------------------------------------- launch helpers
    bool dry() const { return ws.dry; }
    int cur_hw = 0;              // tokens per stream of the block being executed (0 outside the UNet forward): the split-K rule of
                                 // launch_gemm is keyed on ONE stream's share of a GEMM so that results are batch invariant
    // split-K partial sums live in one engine-owned buffer sized by the dry pass of the plan (the former thread_local
    // buffer inside gemm.hip was shared by every stream / device of the thread and grew with a hipMalloc in the middle of a forward)
    float* splitk_buf = nullptr;
    size_t splitk_floats = 0, splitk_need = 0;
    bool run_gemm(GemmArgs& g) {        // false in the dry pass (only records the scratch the launch would need)
        if (dry()) { splitk_need = std::max(splitk_need, gemm_splitk_scratch_floats(g)); return false; }
        g.splitk_ws = splitk_buf; g.splitk_ws_floats = splitk_floats;
        return true;
    }
    GemmArgs dense_args(const bf16_t* A, int lda, const MatW& W, int M, void* out, int ldo, int epi, const void* res = nullptr, int ldres = 0) const {
        return unet_dense_args(zero, cur_hw, A, lda, W, M, out, ldo, epi, res, ldres);
    }
    GemmArgs vt_args(const MatW& Wv, const bf16_t* X, int ldx, int M, bf16_t* out, int ldo) const { return unet_vt_args(zero, cur_hw, Wv, X, ldx, M, out, ldo); }
    void run(GemmArgs& g, int prof_class, double flops) {      // one launch_gemm, with the engine's split-K scratch and its profiling record
        if (!run_gemm(g)) return;
        prof_begin(prof_class, flops);
        launch_gemm(g, stream);
        prof_end();
    }
    void gemm(const bf16_t* A, int lda, const MatW& W, int M, void* out, int ldo, int epi, const void* res = nullptr, int ldres = 0, const LnFold* ln = nullptr) {
        GemmArgs g = dense_args(A, lda, W, M, out, ldo, epi, res, ldres);
        ln_apply(g, ln, ln && ln->part ? W.K : W.N);
        run(g, RT_PROF_GEMM_DENSE, 2.0 * M * W.N * W.K);
    }
    void gemm_vt(const MatW& Wv, const bf16_t* X, int ldx, int M, bf16_t* out, int ldo) {
        GemmArgs g = vt_args(Wv, X, ldx, M, out, ldo);
        run(g, RT_PROF_GEMM_DENSE, 2.0 * M * Wv.N * Wv.K);
    }
    // attn1: the stacked Q|K projection of the first Mqk rows and V^T of all M rows read the same LayerNorm output: ONE grouped launch
    // where gemm16.hip has the pair of tiles (launch_gemm_pair), otherwise one launch each - the same tile bodies either way
    void gemm_qk_vt(const bf16_t* X, int ldx, const MatW& Wqk, int Mqk, bf16_t* qk, int ldqk, const MatW& Wv, int M, bf16_t* vt, int ldvt,
                    const LnFold* lnqk = nullptr, const LnFold* lnv = nullptr) {
        GemmArgs a = dense_args(X, ldx, Wqk, Mqk, qk, ldqk, EPI_BF16);
        GemmArgs b = vt_args(Wv, X, ldx, M, vt, ldvt);
        ln_apply(a, lnqk, Wqk.K); ln_apply(b, lnv, Wv.K);
        const bool ra = run_gemm(a), rb = run_gemm(b);
        if (!ra || !rb) return;
        prof_begin(RT_PROF_GEMM_DENSE, 2.0 * Mqk * Wqk.N * Wqk.K + 2.0 * M * Wv.N * Wv.K);
        launch_gemm_pair(a, b, stream);
        prof_end();
    }
    void conv3(const bf16_t* in, int mode, const MatW& W, int B, int Hin, int Win, int CinP, void* out, int epi,
               const void* res = nullptr, const float* temb = nullptr) {
        GemmArgs g = unet_conv3_args(zero, in, mode, W, B, Hin, Win, CinP, out, epi, res, temb);
        RT_REQUIRE(W.K == 9 * CinP, "conv: weight/input channel mismatch");
        // executed FLOPs: the phase form of an up-sampler convolution multiplies 4 taps per output pixel, not 9
        const bool phase = profiling && !dry() && gemm_route(g).kind == GemmRoute::G16_UP2;
        run(g, RT_PROF_GEMM_CONV, 2.0 * g.M * W.N * (phase ? 4 * CinP : W.K));
    }
    void groupnorm(const void* x1, const void* x2, int in_type /* 0 fp32, 1 bf16, 2 fp16 */, int C1, int C2, int B, int HW, const NormW& n, float eps_,
                   bool silu, bf16_t* out, bf16_t* raw) {
        Scope sc(ws);
        float* partial = ws.f32((size_t)B * groupnorm_nchunk(HW) * cfg.norm_groups * 2);
        if (dry()) return;
        launch_groupnorm(unet_gn_args(x1, x2, in_type, C1, C2, cfg.norm_groups, B, HW, n.g, n.b, eps_, silu, out, raw, partial), stream);
    }
    void layernorm(const f16_t* x, const NormW& n, bf16_t* out, int rows) {
        if (dry()) return;
        launch_layernorm(x, 1, n.g, n.b, out, rows, n.C, 1e-5f, stream);
    }

    // ---------------------------------------------------------------------------- blocks
    // ResnetBlock2D.forward (models/resnet.py:591-645); x2 = skip tensor of the up path (virtual concat)
    // temb: the time_emb_proj table of the running forward (time_embed)
    Tensor resnet(const ResnetP& r, const FwdIn& in, int HW, int Hh, int Ww, Tensor x1, const Tensor* x2, const float* temb,
                  bool inject_here) {
        const int B = in.B, M = B * HW;
        const int c1 = x1.C, c2 = x2 ? x2->C : 0;
        cur_hw = HW;
        RT_REQUIRE(c1 + c2 == r.cin, "resnet: input channel mismatch");
        f16_t* out = ws.f16((size_t)M * r.cout);
        {
            Scope sc(ws);
            bf16_t* h1 = ws.b16((size_t)M * r.cin);
            bf16_t* raw = r.has_sc ? ws.b16((size_t)M * r.cin) : nullptr;
            groupnorm(x1.p, x2 ? x2->p : nullptr, 2, c1, c2, B, HW, r.n1, cfg.norm_eps, true, h1, raw);
            const float* tp = temb + (size_t)B * r.temb_first;            // computed for all resnets at the start of the forward
            // rich-text feature injection (resnet.py:639-643): out[b] = shortcut(x[b]) + hidden[res_src[b]].  The residual branch
            // (conv1 / norm2 / conv2) of an injected stream is never used, so the trailing run of injected streams is not computed
            // at all (the region streams of a rich-text step are the last ones): Bk streams keep their branch.
            int Bk = B;
            bool any_inject = false;
            if (inject_here) {
                for (int b = 0; b < B; ++b) any_inject |= in.res_src[b] >= 0;
                while (Bk > 1 && in.res_src[Bk - 1] >= 0) --Bk;
                for (int b = 0; b < B; ++b)
                    if (in.res_src[b] >= 0) RT_REQUIRE(in.res_src[b] < Bk && in.res_src[in.res_src[b]] < 0, "resnet: a feature source stream must compute its own residual branch");
            }
            if (dry()) Bk = B;                       // the workspace is sized for the case without injection
            const int Mk = Bk * HW;
            bf16_t* h2 = ws.b16((size_t)Mk * r.cout);
            conv3(h1, A_CONV3, r.c1, Bk, Hh, Ww, r.cin, h2, EPI_BF16_TEMB, nullptr, tp);
            bf16_t* h3 = ws.b16((size_t)Mk * r.cout);
            groupnorm(h2, nullptr, 1, r.cout, 0, Bk, HW, r.n2, cfg.norm_eps, true, h3, nullptr);
            const f16_t* resid = x1.p;
            if (r.has_sc) { gemm(raw, r.cin, r.sc, M, out, r.cout, EPI_F16); resid = out; }
            else RT_REQUIRE(!x2, "resnet without shortcut cannot take a concat input");
            if (!any_inject) {
                conv3(h3, A_CONV3, r.c2, B, Hh, Ww, r.cout, out, EPI_F16, resid);
            } else {
                float* hres = ws.f32((size_t)Mk * r.cout);        // fp32: rounded once, together with the shortcut (launch_inject_add)
                conv3(h3, A_CONV3, r.c2, Bk, Hh, Ww, r.cout, hres, EPI_F32, nullptr);
                int src[RT_MAXB];
                for (int b = 0; b < B; ++b) src[b] = in.res_src[b] >= 0 ? in.res_src[b] : b;
                if (!dry()) launch_inject_add(out, resid, hres, src, B, (size_t)HW * r.cout, stream);
            }
        }
        return Tensor{out, r.cout};
    }

    // ---------------------------------------------------------------------------- transformer
    // Regional LoRA (rt_set_lora_scales): the adapted streams of a forward - those whose prompt slot has a non-zero scale - get the low-rank
    // term added behind each of the eight attention projections - with rt_config.lora_targets = 1 behind proj_in, ff.net.2 and proj_out as
    // well, and their ff.net.0.proj runs unfused (feed_forward) -; every other stream is in none of these launches
    struct LoraRows {
        rt_engine& e;
        int B, HW;
        int rows[RT_MAXB]; float sc[RT_MAXB * 4];
        bool any = false;
        LoraRows(rt_engine& e_, const FwdIn& in, int HW_) : e(e_), B(in.B), HW(HW_) {
            for (int b = 0; b < B; ++b) {
                const bool on = !e.dry() && !in.control && e.lora_on(in.prompt[b]);
                rows[b] = b * HW;
                for (int l = 0; l < 4; ++l) sc[4 * b + l] = on ? e.lora_scale[(size_t)in.prompt[b] * 4 + l] : 0.f;
                any = any || on;
            }
        }
        bool on(int b) const { return sc[4 * b] != 0.f || sc[4 * b + 1] != 0.f || sc[4 * b + 2] != 0.f || sc[4 * b + 3] != 0.f; }
        // run f(first stream, streams) over the maximal runs of adapted streams (the row-wise kernels take a run as one launch) - or,
        // adapted = false, of the streams the adapters leave alone
        template <typename F> void runs(F f, bool adapted = true) const {
            for (int b = 0; b < B;) {
                if (on(b) != adapted) { ++b; continue; }
                int e_ = b; while (e_ < B && on(e_) == adapted) ++e_;
                f(b, e_ - b); b = e_;
            }
        }
        // the term of one projection for the first nb streams (a module without factors - rt_config.lora_targets = 0 - has none)
        void add(const LoraW& w, const bf16_t* X, int ldx, void* Y, int ldy, int form, int nb) const {
            if (any && w.down) e.lora_add(w, X, ldx, Y, ldy, form, rows, sc, nb, HW);
        }
        // a folded LayerNorm is never materialised: the adapters' input is computed for the adapted rows only, into `n`
        void norm(const NormW& ln, const f16_t* h, bf16_t* n) const {
            runs([&](int b, int nb) { launch_layernorm(h + (size_t)b * HW * ln.C, 1, ln.g, ln.b, n + (size_t)b * HW * ln.C, nb * HW, ln.C, 1e-5f, e.stream); });
        }
    };
    // The LayerNorms of one transformer() call, folded into their consumers (gemm16.hip, "LNF"; attention.py:150,168,181) wherever every
    // consumer of the LayerNorm has the folded instantiation - a pure function of the layer's shape (width, tokens per stream), never of the
    // batch.  The trunk's producers (proj_in, to_out, ff.net.2: fp16-trunk epilogues) then leave the per-row partial sums next to it; a
    // producer without that form is followed by the stand-alone partials kernel.  Debug bit 22 restores the LayerNorm launches.
    struct LnTrunk {
        rt_engine& e;
        const LoraRows& lora;
        int M, C;
        f16_t* hcur;                 // the trunk
        float* part;                 // [M, 16]: up to 4 tile pairs x float4 per token
        bf16_t* xb;                  // the trunk as bf16, written next to it by its producer
        bool fold[3] = {false, false, false};                            // norm1 / norm2 / norm3
        bool emit_pin = false, emit_out = false, emit_ff2 = false;       // the producers that leave the partials themselves
        int ln_bn = 160, npair;      // column-tile width of the partials (a function of the class of the producers: of (C, tokens per stream))
        LnFold em;
        LnTrunk(rt_engine& e_, const LoraRows& l, const TransformerP& t, int M_, f16_t* h, float* p, bf16_t* x)
            : e(e_), lora(l), M(M_), C(t.C), hcur(h), part(p), xb(x) {
            const int HD = t.heads * t.DP;
            if (gemm_lnfold_enabled() && ln_fold_width(C) && !t.blocks.empty() && t.blocks[0].qk1f.w) {
                const TBlockP& k0 = t.blocks[0];
                const int bn_pin = gemm_ln_emit_bn(e.dense_args(nullptr, C, t.pin, M, nullptr, C, EPI_F16));
                const int bn_out = gemm_ln_emit_bn(e.dense_args(nullptr, HD, k0.out1, M, nullptr, C, EPI_F16));
                const int bn_ff2 = gemm_ln_emit_bn(e.dense_args(nullptr, 4 * C, k0.ff2, M, nullptr, C, EPI_F16));
                ln_bn = bn_out ? bn_out : (bn_ff2 ? bn_ff2 : (bn_pin ? bn_pin : 160));
                emit_pin = bn_pin == ln_bn; emit_out = bn_out == ln_bn; emit_ff2 = bn_ff2 == ln_bn;     // (one class for all three: same N, same tokens per stream)
                const int np = C / ln_bn / 2;
                GemmArgs cq = e.dense_args(nullptr, C, k0.qk1f, M, nullptr, 2 * HD, EPI_BF16); cq.ln_npair = np;
                GemmArgs cv = e.vt_args(k0.v1f, nullptr, C, M, nullptr, M); cv.ln_npair = np;
                GemmArgs c2 = e.dense_args(nullptr, C, k0.q2f, M, nullptr, HD, EPI_BF16); c2.ln_npair = np;
                GemmArgs c3 = e.dense_args(nullptr, C, k0.ff1f, M, nullptr, 4 * C, EPI_GEGLU); c3.ln_npair = np;
                fold[0] = gemm_ln_fold_ok(cq) && gemm_ln_fold_ok(cv);
                fold[1] = gemm_ln_fold_ok(c2);
                fold[2] = gemm_ln_fold_ok(c3);
            }
            npair = C / ln_bn / 2;
            em.emit = part; em.copy = xb;
        }
        // the consumer side of a folded launch: A / X is xb, W the folded copy, s its (row sum, c) pairs
        LnFold reads(const float* s) const { LnFold l; l.part = part; l.npair = npair; l.ld = M; l.s = s; return l; }
        // partials of the trunk as it stands, for the LayerNorm that follows
        void partials() { if (!e.dry()) launch_ln_partials(hcur, xb, part, M, C, ln_bn, e.stream); }
        // consume: out = epi(LayerNorm i of the trunk x W^T) - the folded GEMM on xb, or the LayerNorm into `n` and the plain GEMM
        void consume(int i, const NormW& ln, bf16_t* n, const MatW& W, const MatW& Wf, const float* s, bf16_t* out, int ldo, int epi) {
            consume_rows(i, ln, n, W, Wf, s, out, ldo, epi, 0, M);
        }
        // ... of `rows` rows from row0 on (a run of streams): the same launches over fewer rows, whose bits do not depend on the run
        void consume_rows(int i, const NormW& ln, bf16_t* n, const MatW& W, const MatW& Wf, const float* s, bf16_t* out, int ldo, int epi, int row0, int rows) {
            const size_t r0 = (size_t)row0;
            if (fold[i]) { LnFold l = reads(s); l.part = part + r0 * 4; e.gemm(xb + r0 * C, C, Wf, rows, out + r0 * ldo, ldo, epi, nullptr, 0, &l); }
            else { e.layernorm(hcur + r0 * C, ln, n + r0 * C, rows); e.gemm(n + r0 * C, C, W, rows, out + r0 * ldo, ldo, epi); }
        }
        // produce into the trunk: hcur = A W^T (+ hcur with `residual`), then the adapters' term `lw` (the adapted rows are rounded to fp16 a
        // second time: control_add_kernel's precedent).  folds: the LayerNorm that reads the trunk next is folded, so it needs the partials
        // and xb - from the GEMM's epilogue where the producer `emits`, otherwise (if the trunk is `read_again` by a LayerNorm at all) from
        // the stand-alone kernel; rows the adapters changed behind an emitting GEMM get theirs recomputed.
        void produce(const bf16_t* A, int lda, const MatW& W, bool residual, bool folds, bool emits, bool read_again = true, const LoraW* lw = nullptr) {
            e.gemm(A, lda, W, M, hcur, C, EPI_F16, residual ? hcur : nullptr, residual ? C : 0, folds && emits ? &em : nullptr);
            if (lw && !lw->down) lw = nullptr;
            if (lw) lora.add(*lw, A, lda, hcur, C, 2, lora.B);
            if (folds && !emits && read_again) partials();
            if (folds && emits && lw)
                lora.runs([&](int b, int nb) { launch_ln_partials(hcur + (size_t)b * lora.HW * C, xb + (size_t)b * lora.HW * C, part + (size_t)b * lora.HW * 4, nb * lora.HW, C, ln_bn, e.stream, M); });
        }
    };
    // What the blocks of one transformer() call share.  The per-stream tables depend on the forward, not on the block.
    struct TCall {
        TransformerP& t; const FwdIn& in;
        int B, HW, M, C, HD;
        LoraRows lora;
        LnTrunk ln;
        int nkeys[RT_MAXB], wset2[RT_MAXB];                                  // attn2: valid keys; multiplier set (-1: plain softmax, no tables)
        int ip_slot[RT_MAXB], ip_cnt[RT_MAXB]; float ip_sc[RT_MAXB];         // image prompts (rt_set_image_prompts): slot -1 = no image
        bool any_ip = false;
        double keysum = 0, ip_keys = 0, nip = 0;
        bf16_t *n = nullptr, *qk = nullptr, *vt = nullptr, *o = nullptr;     // scratch of the running block
        float* store_stats = nullptr;                                        // softmax statistics of the token-map accumulation (attn_store.hip)
        TCall(rt_engine& e, TransformerP& t_, const FwdIn& in_, int HW_, f16_t* hcur, float* part, bf16_t* xb)
            : t(t_), in(in_), B(in_.B), HW(HW_), M(in_.B * HW_), C(t_.C), HD(t_.heads * t_.DP), lora(e, in_, HW_), ln(e, lora, t_, M, hcur, part, xb) {
            for (int b = 0; b < B; ++b) {
                const int p = in.prompt[b];
                const bool on = e.cfg.ip_tokens > 0 && !in.control && e.ip_scale[p] != 0.f;
                nkeys[b] = e.prompt_keys[p]; wset2[b] = in.fontsize[b] ? 1 : -1; keysum += nkeys[b];
                ip_slot[b] = on ? p : -1; ip_cnt[b] = on ? e.ip_count[p] : 0; ip_sc[b] = on ? e.ip_scale[p] : 0.f;
                if (on) { any_ip = true; ip_keys += ip_cnt[b]; nip += 1; }
            }
        }
    };

    // attn1 (self; attention_processor.py:476-545)
    void attn1(TCall& c, TBlockP& k) {
        TransformerP& t = c.t; const FwdIn& in = c.in; LnTrunk& ln = c.ln;
        const int B = c.B, HW = c.HW, M = c.M, C = c.C, HD = c.HD;
        // Q,K are only needed for streams that some stream attends with (injected region streams use the
        // text_ref stream's Q,K: attention_processor.py:522-524 discards their own scores)
        // Perturbed-attention guidance: at an applied module the trailing twins do not attend - their attention output is their V (below) -,
        // so the launch covers the leading natt entries and a twin's Q / K rows are projected only where an attending stream reads them
        int natt = B;
        if (k.pag) { natt = 0; while (natt < B && !in.perturb[natt]) ++natt; }
        int nqk = natt ? 0 : 1;                 // (a launch of twins alone keeps one stream's rows: the projection pair has no V-only form)
        for (int b = 0; b < natt; ++b) nqk = std::max(nqk, in.qk_src[b] + 1);
        if (ln.fold[0]) {
            const LnFold lq = ln.reads(k.qk1s), lv = ln.reads(k.v1s);
            gemm_qk_vt(ln.xb, C, k.qk1f, nqk * HW, c.qk, 2 * HD, k.v1f, M, c.vt, M, &lq, &lv);
            c.lora.norm(k.ln1, ln.hcur, c.n);
        } else {
            layernorm(ln.hcur, k.ln1, c.n, M);
            gemm_qk_vt(c.n, C, k.qk1, nqk * HW, c.qk, 2 * HD, k.v1, M, c.vt, M);
        }
        // (an injected region stream attends with text_ref's Q and K - rows >= nqk are not even computed -, so its own to_q /
        // to_k adapters are moot; its to_v and to_out adapters act)
        c.lora.add(k.lora[0], c.n, C, c.qk, 2 * HD, 0, nqk);
        c.lora.add(k.lora[1], c.n, C, c.qk + HD, 2 * HD, 0, nqk);
        c.lora.add(k.lora[2], c.n, C, c.vt, M, 1, B);
        if (!dry()) {
            // a layer whose map is recorded in this call: the attention launch leaves the softmax statistics of the recorded stream,
            // so the store runs its apply kernel only (debug bit 17: the store computes them itself, round 4's two launches)
            const bool will_store = in.store_stream >= 0 && k.store_mode[0] && k.store_calls[0] + 1 > 10;      // n_maps[name] > 10 (rd.py:422, xl.py:988)
            const bool stats_from_attn = will_store && store_handover_self(HW, t.DP, in.qk_src, in.store_stream);
            const AttnArgs a = unet_self_attn_args(AttnIO{c.qk, 2 * HD, c.qk + HD, 2 * HD, c.vt, M, c.o, HD}, in.qk_src, natt, t.heads, HW, t.DP,
                                                   stats_from_attn ? c.store_stats : nullptr, in.store_stream);
            if (natt) {
                prof_begin(RT_PROF_ATTN_SELF, 4.0 * natt * t.heads * (double)HW * HW * t.d);
                launch_attention(a, stream);
                prof_end();
            }
            if (natt < B) {                     // the twins' rows of o: O = V, head for head (pag.hip)
                int twins[RT_MAXB];
                for (int b = natt; b < B; ++b) twins[b - natt] = b;
                prof_begin(RT_PROF_PAG, 0.0, 2.0 * 2.0 * (B - natt) * (double)HW * HD);      // priced in bytes: V^T read once, O written once
                launch_identity_attention(c.vt, M, c.o, HD, twins, B - natt, B, t.heads, HW, t.DP, stream);
                prof_end();
            }
            if (in.store_stream >= 0 && k.store_mode[0] && ++k.store_calls[0] > 10) {
                RT_REQUIRE((size_t)HW * HW <= k.store_cap[0], "attention store: map larger than the enabled buffer");
                prof_begin(RT_PROF_ATTN_STORE, 2.0 * 2.0 * t.heads * (double)HW * HW * t.d, 8.0 * HW * HW + 2.0 * 2.0 * HW * HD);
                launch_attn_store(unet_store_args(a, in.store_stream, k.store[0], k.store_mode[0] == 2, c.store_stats, HW), stream);
                prof_end();
                k.store_rows[0] = HW; k.store_cols[0] = HW;
            }
        }
        ln.produce(c.o, HD, k.out1, true, ln.fold[1], ln.emit_out, true, &k.lora[3]);
    }

    // attn2 (cross, K/V from the per-prompt cache; font-size softmax on flagged streams)
    void attn2(TCall& c, TBlockP& k) {
        TransformerP& t = c.t; const FwdIn& in = c.in; LnTrunk& ln = c.ln;
        const int B = c.B, HW = c.HW, M = c.M, C = c.C, HD = c.HD;
        // the route (cross_route): a layer with its map enabled counts as recorded whether or not this call is past the tenth
        const bool capture2 = in.store_stream >= 0 && k.store_mode[1];
        const int KPr = KP(), ldvt2 = cfg.max_prompts * KPr;
        CrossRoute route = cross_route(C, t.heads, t.d, t.DP, HW, KPr, c.nkeys, B, ln.fold[1], capture2);
        // Image prompts: the image term is added into o behind the text attention, which the one-launch forms never write - a launch with an
        // image takes the two-launch route of the same shape.  Regional LoRA likewise: to_q's term is added to a materialised Q, to_out's
        // behind the GEMM.  (Only RT_PROBES builds with their debug switches on ever reach the one-launch kinds.  The dry planning forward
        // of an engine that can hold images or adapters takes the two-launch route as well, so that the to_q GEMM such a launch runs has
        // been planned: its split-K scratch is recorded like every other GEMM's.)
        if ((c.any_ip || c.lora.any || (dry() && (cfg.ip_tokens > 0 || cfg.lora_rank > 0) && !in.control)) && (route.kind == CrossRoute::XBLOCK || route.kind == CrossRoute::XATTN_FUSED))
            route = cross_route(C, t.heads, t.d, t.DP, HW, KPr, c.nkeys, B, ln.fold[1], capture2, false);
        if (route.kind == CrossRoute::XBLOCK || route.kind == CrossRoute::XATTN_FUSED) {
            layernorm(ln.hcur, k.ln2, c.n, M);      // (a folded norm2 never takes the one-launch forms)
            if (route.kind == CrossRoute::XBLOCK) {
                if (!dry()) {
                    RT_REQUIRE(k.q2.K == C && k.out2.K == HD && HD == C, "xblock: packed projection widths");
                    prof_begin(RT_PROF_XBLOCK, 4.0 * M * HD * C + 4.0 * B * t.heads * (double)HW * 77 * t.d);
                    launch_xblock(unet_xblock_args(c.n, k.q2.w, k.out2.w, k.out2.b, k.kcache, k.vtcache, ldvt2, ln.hcur, ln.hcur, wabs, wsgn, in.prompt, c.wset2, B, HW, C, t.heads), stream);
                    prof_end();
                }
                if (ln.fold[2]) ln.partials();
                return;                              // to_out + residual were part of that launch
            }
            if (!dry()) {
                prof_begin(RT_PROF_XATTN_FUSED, 2.0 * M * HD * C + 4.0 * B * t.heads * (double)HW * 77 * t.d);
                launch_xattn_fused(unet_xattn_args(zero, c.n, k.q2.w, c.o, k.kcache, k.vtcache, ldvt2, wabs, wsgn, in.prompt, c.wset2, B, HW, C, t.heads), stream);
                prof_end();
            }
        } else {
            ln.consume(1, k.ln2, c.n, k.q2, k.q2f, k.q2s, c.qk, HD, EPI_BF16);
            if (ln.fold[1]) c.lora.norm(k.ln2, ln.hcur, c.n);
            c.lora.add(k.lora[4], c.n, C, c.qk, HD, 0, B);
            if (!dry()) {
                // (a recorded layer on cross77_kernel hands its statistics over as attn1 does, from the eleventh recorded call on)
                const AttnArgs a = unet_cross_attn_args(AttnIO{c.qk, HD, k.kcache, HD, k.vtcache, ldvt2, c.o, HD}, in.prompt, c.wset2, c.nkeys, wabs, wsgn, B, t.heads, HW,
                                                        KPr, t.DP, route.handover && k.store_calls[1] + 1 > 10 ? c.store_stats : nullptr, in.store_stream);
                prof_begin(RT_PROF_ATTN_CROSS, 4.0 * t.heads * (double)HW * c.keysum * t.d);
                launch_cross(a, route, stream);
                prof_end();
                if (capture2 && ++k.store_calls[1] > 10) {
                    const int snk = c.nkeys[in.store_stream], srows = 96 * (snk / 77);
                    RT_REQUIRE((size_t)HW * snk <= k.store_cap[1], "attention store: map larger than the enabled buffer");
                    prof_begin(RT_PROF_ATTN_STORE, 2.0 * 2.0 * t.heads * (double)HW * snk * t.d, 8.0 * HW * snk + 2.0 * (HW + (double)srows) * HD);
                    launch_attn_store(unet_store_args(a, in.store_stream, k.store[1], k.store_mode[1] == 2), stream);
                    prof_end();
                    k.store_rows[1] = HW; k.store_cols[1] = snk;
                }
                if (c.any_ip) {                                   // (the token-map store above recorded the text probabilities only)
                    prof_begin(RT_PROF_IP_ATTN, 4.0 * t.heads * (double)HW * c.ip_keys * t.d, 3.0 * 2.0 * c.nip * HW * HD);
                    launch_ip_attention(c.qk, HD, k.kipcache, HD, k.vtipcache, cfg.max_prompts * 16, c.o, HD, c.ip_slot, c.ip_cnt, c.ip_sc, B, t.heads, HW, t.DP, stream);
                    prof_end();
                }
            }
        }
        ln.produce(c.o, HD, k.out2, true, ln.fold[2], ln.emit_out, true, &k.lora[7]);
    }

    // GEGLU feed-forward (attention.py:209-304)
    void feed_forward(TCall& c, TBlockP& k, bool last) {
        const int HW = c.HW, C = c.C;
        bf16_t* gg = ws.b16((size_t)c.M * 4 * C);
        // ff.net.0.proj's adapter (rt_config.lora_targets = 1): the GEGLU epilogue cannot take an add behind the GEMM, so an adapted stream
        // runs unfused and once - LayerNorm 3 of its rows, the plain weight into fp32 scratch z (ONE stream's at a time), lora_geglu_kernel
        // into its rows of gg - while the maximal runs of the other streams keep the fused launch and its bits.  The dry planning forward
        // plans both: the whole fused launch and one stream's fp32 GEMM with its scratch.
        const bool wide = k.lora_ff1.down && (c.lora.any || dry());
        if (!wide) {
            c.ln.consume(2, k.ln3, c.n, k.ff1, k.ff1f, k.ff1s, gg, 4 * C, EPI_GEGLU);
        } else {
            float* z = ws.f32((size_t)HW * 8 * C);
            if (dry()) {
                c.ln.consume(2, k.ln3, c.n, k.ff1, k.ff1f, k.ff1s, gg, 4 * C, EPI_GEGLU);
                gemm(c.n, C, k.ff1, HW, z, 8 * C, EPI_F32);
            } else {
                c.lora.runs([&](int b, int nb) { c.ln.consume_rows(2, k.ln3, c.n, k.ff1, k.ff1f, k.ff1s, gg, 4 * C, EPI_GEGLU, b * HW, nb * HW); }, false);
                for (int b = 0; b < c.B; ++b) {
                    if (!c.lora.on(b)) continue;
                    bf16_t* nb_ = c.n + (size_t)b * HW * C;
                    layernorm(c.ln.hcur + (size_t)b * HW * C, k.ln3, nb_, HW);
                    gemm(nb_, C, k.ff1, HW, z, 8 * C, EPI_F32);
                    lora_geglu(k.lora_ff1, nb_, z, gg + (size_t)b * HW * 4 * C, c.lora.sc + 4 * b, HW);
                }
            }
        }
        // the next block's norm1 reads what ff.net.2 leaves; behind the LAST block proj_out reads the trunk as bf16 - which is
        // exactly the xb an emitting ff.net.2 writes (the cast launch in transformer() is then not needed; the rows ff.net.2's adapter
        // changed are refreshed in xb by produce, together with their partials)
        c.ln.produce(gg, 4 * C, k.ff2, true, c.ln.fold[0], c.ln.emit_ff2, !last, &k.lora_ff2);
    }

    // Transformer2DModel.forward (models/transformer_2d.py:270-310) + BasicTransformerBlock (attention.py:131-206)
    Tensor transformer(TransformerP& t, const FwdIn& in, int HW, Tensor x) {
        const int B = in.B, M = B * HW, C = t.C, HD = t.heads * t.DP;
        cur_hw = HW;
        RT_REQUIRE(x.C == C, "transformer: channel mismatch");
        RT_REQUIRE(HW % 8 == 0, "transformer: token count (h*w of the attention level) must be a multiple of 8");
        f16_t* out = ws.f16((size_t)M * C);
        {
            Scope sc(ws);
            f16_t* hcur = ws.f16((size_t)M * C);
            float* part = ws.f32((size_t)M * 16);
            bf16_t* xb = ws.b16((size_t)M * C);
            TCall c(*this, t, in, HW, hcur, part, xb);
            {
                Scope s2(ws);
                bf16_t* g = ws.b16((size_t)M * C);
                groupnorm(x.p, nullptr, 2, C, 0, B, HW, t.gn, 1e-6f, false, g, nullptr);
                c.ln.produce(g, C, t.pin, false, c.ln.fold[0], c.ln.emit_pin, true, &t.lora_pin);
            }
            for (size_t bi = 0; bi < t.blocks.size(); ++bi) {
                Scope s2(ws);
                c.n = ws.b16((size_t)M * C);
                c.qk = ws.b16((size_t)M * 2 * HD);
                c.vt = ws.b16((size_t)HD * M);
                c.o = ws.b16((size_t)M * HD);
                c.store_stats = ws.f32((size_t)t.heads * HW * 2);
                attn1(c, t.blocks[bi]);
                attn2(c, t.blocks[bi]);
                feed_forward(c, t.blocks[bi], bi + 1 == t.blocks.size());
            }
            const bool have_xb = c.ln.fold[0] && c.ln.emit_ff2 && !t.blocks.empty();
            bf16_t* hb = ws.b16((size_t)M * C);
            if (!dry() && !have_xb) launch_cast_f16_bf16(hcur, hb, (size_t)M * C, stream);
            gemm(have_xb ? xb : hb, C, t.pout, M, out, C, EPI_F16, x.p, C);
            c.lora.add(t.lora_pout, have_xb ? xb : hb, C, out, C, 2, B);
        }
        return Tensor{out, C};
    }

    // ---------------------------------------------------------------------------- ControlNet
    // the controlled streams of a forward, in stream order: those whose prompt slot has a scale != 0 while a hint is set
    int control_streams(const FwdIn& in, int* cs, float* csc) const {
        int n = 0;
        for (int b = 0; b < in.B; ++b) {
            const float s = dry() ? 1.f : (ctl.has_hint ? ctl.scale[in.prompt[b]] : 0.f);      // the dry pass sizes the workspace for every stream controlled
            if (s != 0.f) { cs[n] = b; csc[n] = s; ++n; }
        }
        return n;
    }
    // refusals of a forward, before anything is launched
    void control_check(const FwdIn& in) {
        int cs[RT_MAXB]; float csc[RT_MAXB];
        const int Bc = control_streams(in, cs, csc);
        if (Bc && (in.h != ctl.hint_h || in.w != ctl.hint_w))
            throw rt_error(RT_E_INVALID, "forward: the control hint was set for a " + std::to_string(ctl.hint_h) + " x " + std::to_string(ctl.hint_w) +
                                             " latent grid, the forward runs " + std::to_string(in.h) + " x " + std::to_string(in.w) + " (rt_set_control_hint again: a hint is never resized)");
        if (tracing() && trace_name.compare(0, 11, "controlnet.") == 0) {
            const bool main_side = trace_name.compare(0, 16, "controlnet.skip.") == 0 || trace_name == "controlnet.mid";
            if (trace_name == "controlnet.hint_embedding") { if (!ctl.has_hint) throw rt_error(RT_E_INVALID, "rt_unet_forward_trace: no control hint is set"); }
            else if (!main_side && !Bc) throw rt_error(RT_E_INVALID, "rt_unet_forward_trace: " + trace_name + " does not run: the call controls no stream");
        }
    }
    // one residual: r = zero_conv(xc) of the controlled streams as ONE GEMM into fp32 scratch, then the add into the main UNet's tensor
    void control_residual(const MatW& z, const Tensor& xc, Tensor& dst, const int* cs, const float* csc, int Bc, int B, int HW) {
        RT_REQUIRE(xc.C == dst.C && z.K == xc.C && z.N == xc.C, "controlnet: zero convolution / skip channel mismatch");
        Scope sc(ws);
        const int C = xc.C;
        bf16_t* xb = ws.b16((size_t)Bc * HW * C);
        float* r = ws.f32((size_t)Bc * HW * C);
        if (!dry()) launch_cast_f16_bf16(xc.p, xb, (size_t)Bc * HW * C, stream);
        cur_hw = HW;
        gemm(xb, C, z, Bc * HW, r, C, EPI_F32);
        if (dry()) return;
        prof_begin(RT_PROF_CONTROL_ADD, 0.0, 8.0 * Bc * HW * C);      // r read (4 B), skip read + written (2 + 2 B) per element
        launch_control_add(dst.p, (size_t)HW * C, C, r, (size_t)HW * C, C, cs, csc, Bc, B, HW, C, stream);
        prof_end();
    }
    // ---------------------------------------------------------------------------- the forward
    // The time / addition embeddings of a forward of `net` (unet_2d_condition.py:784-877) and from them time_emb_proj(silu(emb)) of every
    // resnet of its table (resnet.py:611-613) in one launch: [resnet][B][cout], allocated in the caller's scope - it lives as long as the
    // forward - and handed to resnet() by the caller
    const float* time_embed(const NetP& net, const FwdIn& in) {
        const int B = in.B, C0 = cfg.block_out_channels[0];
        float* emb = ws.f32((size_t)B * temb_dim);
        {
            Scope sc(ws);
            float* tsin = ws.f32(C0);
            float* e1 = ws.f32(temb_dim); float* e2 = ws.f32(temb_dim);
            if (!dry()) {
                launch_timestep_embed_scalar(in.t, C0, tsin, stream);
                launch_small_linear(tsin, C0, net.t1.w, net.t1.K, net.t1.b, e1, temb_dim, 1, temb_dim, net.t1.K, 0, 0, stream);
                launch_small_linear(e1, temb_dim, net.t2.w, net.t2.K, net.t2.b, e2, temb_dim, 1, temb_dim, temb_dim, 1, 0, stream);
                launch_gather_add_rows(e2, net.aug_emb, in.prompt, emb, B, temb_dim, stream);
            }
        }
        float* temb = ws.f32((size_t)B * net.temb_total);
        {
            Scope sc(ws);
            float* semb = ws.f32((size_t)B * temb_dim);
            if (!dry()) launch_temb_all(emb, temb_dim, semb, net.temb_tab_dev, (int)net.temb_tab.size(), net.temb_total, B, temb_dim, temb, stream);
        }
        return temb;
    }
    // The encoder of `net` on the streams of `in`: stem, down blocks, mid block; returns the mid block's output on the grid (ch, cw).
    // stem(x8, x0): conv_in of the prepared latents x8 [B, HW0, 8] into x0.  skip(x, HW): every tensor the up path takes as a skip, in order.
    template <typename Stem, typename Skip>
    Tensor encode(NetP& net, const FwdIn& in, const float* temb, int& ch, int& cw, Stem stem, Skip skip) {
        const int B = in.B, HW0 = in.h * in.w, C0 = cfg.block_out_channels[0];
        Tensor x;
        {
            f16_t* x0 = ws.f16((size_t)B * HW0 * C0);
            Scope sc(ws);
            bf16_t* x8 = ws.b16((size_t)B * HW0 * 8);
            if (!dry()) {
                PrepArgs p{}; p.B = B; p.HW = HW0; p.dst = x8;
                for (int b = 0; b < B; ++b) { p.src[b] = in.x[b]; p.scale[b] = in.scale[b]; }
                launch_prep_latents(p, stream);
            }
            stem(x8, x0);
            x = Tensor{x0, C0};
        }
        if (tracing()) trace_point(net.prefix + "conv_in", x, B, HW0);
        skip(x, HW0);
        ch = in.h; cw = in.w;
        for (size_t i = 0; i < net.down.size(); ++i) {
            DownP& d = net.down[i];
            for (size_t j = 0; j < d.res.size(); ++j) {
                x = resnet(d.res[j], in, ch * cw, ch, cw, x, nullptr, temb, false);
                trace_point(d.res[j].name, x, B, ch * cw);
                if (d.has_attn) { x = transformer(d.attn[j], in, ch * cw, x); trace_point(d.attn[j].name, x, B, ch * cw); }
                skip(x, ch * cw);
            }
            if (d.has_down) {
                const int nh = (ch + 1) / 2, nw = (cw + 1) / 2;
                f16_t* y = ws.f16((size_t)B * nh * nw * d.C);
                {
                    Scope sc(ws);
                    bf16_t* xb = ws.b16((size_t)B * ch * cw * d.C);
                    if (!dry()) launch_cast_f16_bf16(x.p, xb, (size_t)B * ch * cw * d.C, stream);
                    conv3(xb, A_CONV3_S2, d.down, B, ch, cw, d.C, y, EPI_F16);
                }
                ch = nh; cw = nw;
                x = Tensor{y, d.C};
                if (tracing()) trace_point(net.prefix + "down_blocks." + std::to_string(i) + ".downsamplers.0.conv", x, B, ch * cw);
                skip(x, ch * cw);
            }
        }
        x = resnet(net.mid_r0, in, ch * cw, ch, cw, x, nullptr, temb, false);
        trace_point(net.mid_r0.name, x, B, ch * cw);
        x = transformer(net.mid_t, in, ch * cw, x);
        trace_point(net.mid_t.name, x, B, ch * cw);
        x = resnet(net.mid_r1, in, ch * cw, ch, cw, x, nullptr, temb, false);
        trace_point(net.mid_r1.name, x, B, ch * cw);
        return x;
    }

    // ControlNetModel.forward for the controlled streams of `in`, behind the main UNet's mid block: adds scale x zero_conv(skip_k) into
    // skips[k] and scale x zero_conv(mid) into xmid, in place.  Everything it allocates is released when it returns.
    void control_pass(const FwdIn& in, std::vector<Tensor>& skips, Tensor& xmid) {
        int cs[RT_MAXB]; float csc[RT_MAXB];
        const int Bc = control_streams(in, cs, csc), B = in.B, Hh = in.h, Ww = in.w, HW0 = Hh * Ww, C0 = cfg.block_out_channels[0];
        auto trace_main = [&](const std::string& n, const Tensor& t, int HW) { trace_point(cnet.prefix + n, t, B, HW); };      // (asked under tracing() only)
        if (tracing() && trace_name == "controlnet.hint_embedding") launch_trace_f16_nhwc_to_nchw(ctl.emb_f16, trace_out, 1, C0, HW0, stream);
        if (!Bc) {                        // nothing runs; the main-side trace points read the tensors as the up path will
            if (tracing()) {
                int ch = Hh, cw = Ww; size_t k = 0;
                trace_main("skip.0", skips[k++], ch * cw);
                for (const DownP& d : unet.down) {
                    for (size_t j = 0; j < d.res.size(); ++j, ++k) trace_main("skip." + std::to_string(k), skips[k], ch * cw);
                    if (d.has_down) { ch = (ch + 1) / 2; cw = (cw + 1) / 2; trace_main("skip." + std::to_string(k), skips[k], ch * cw); ++k; }
                }
                trace_main("mid", xmid, ch * cw);
            }
            return;
        }
        FwdIn c{}; c.B = Bc; c.h = Hh; c.w = Ww; c.t = in.t; c.control = true;
        for (int i = 0; i < Bc; ++i) {
            c.x[i] = in.x[cs[i]]; c.scale[i] = in.scale[cs[i]]; c.prompt[i] = in.prompt[cs[i]];
            c.fontsize[i] = 0; c.qk_src[i] = i; c.res_src[i] = -1;
        }
        Scope sc(ws);
        const float* temb = time_embed(cnet, c);
        size_t k = 0;
        int ch, cw;
        Tensor x = encode(cnet, c, temb, ch, cw,
            // conv_in(x) + hint embedding: the embedding [HW0, C0] is the residual operand of the convolution's epilogue (fp32 sum, one
            // rounding to fp16) - one launch per controlled stream, each the launch of a stream that runs alone
            [&](const bf16_t* x8, f16_t* x0) {
                for (int i = 0; i < Bc; ++i) conv3(x8 + (size_t)i * HW0 * 8, A_CONV3, cnet.conv_in, 1, Hh, Ww, 8, x0 + (size_t)i * HW0 * C0, EPI_F16, ctl.emb_f16);
            },
            // one residual per skip of the control copy, and its main-side trace point
            [&](const Tensor& xc, int HW) {
                RT_REQUIRE(k < skips.size() && k < ctl.zero.size(), "controlnet: more control skips than skips");
                control_residual(ctl.zero[k], xc, skips[k], cs, csc, Bc, B, HW);
                if (tracing()) trace_main("skip." + std::to_string(k), skips[k], HW);
                ++k;
            });
        RT_REQUIRE(k == skips.size(), "controlnet: skip count");
        control_residual(ctl.zero_mid, x, xmid, cs, csc, Bc, B, ch * cw);
        if (tracing()) trace_main("mid", xmid, ch * cw);
    }

    // Perturbed-attention guidance: what a forward with twins needs, refused before anything is launched - the twins trail the list, the
    // recorded stream is none of them, and every applied module's grid holds a multiple of 8 tokens (the identity kernel's 16-byte accesses)
    void pag_check(const FwdIn& in) {
        bool any = false;
        for (int b = 0; b < in.B; ++b) {
            if (in.perturb[b]) any = true;
            else RT_REQUIRE(!any, "forward: the perturbed streams must trail the stream list");
        }
        if (!any) return;
        RT_REQUIRE(!in.control, "forward: the ControlNet copy is never perturbed");
        RT_REQUIRE(in.store_stream < 0 || !in.perturb[in.store_stream], "forward: the token-map store never records a perturbed stream");
        if (pag_layers == 0) throw rt_error(RT_E_INVALID, "forward: a perturbed stream but no applied layer (rt_set_pag_layers: the applied set is empty)");
        for_each_tblock([&](TransformerP& t, TBlockP& k) {
            if (!k.pag) return;
            const int tokens = (in.h >> t.level) * (in.w >> t.level);
            if (tokens % 8 != 0)
                throw rt_error(RT_E_UNSUPPORTED, "forward: perturbed attention at " + k.mod_name[0] + " needs a multiple of 8 tokens, the grid has " + std::to_string(tokens));
        });
    }

    // UNet2DConditionModel.forward (models/unet_2d_condition.py:703-983), batched over streams
    void unet_forward(const FwdIn& in) {
        const int B = in.B, Hh = in.h, Ww = in.w, HW0 = Hh * Ww;
        RT_REQUIRE(B >= 1 && B <= cfg.max_streams && B <= RT_MAXB, "forward: too many streams");
        RT_REQUIRE(Hh <= cfg.latent_h && Ww <= cfg.latent_w, "forward: latent larger than configured");
        RT_REQUIRE((Hh % (1 << (cfg.n_levels - 1))) == 0 && (Ww % (1 << (cfg.n_levels - 1))) == 0, "forward: latent size not divisible");
        // FreeU (rt_set_freeu): the skip filter scales the bins {-1, 0} of both axes, which a side of 1 does not have - refused before any launch
        if (!dry() && freeu_on() && ((Hh >> (cfg.n_levels - 1)) < 2 || (Ww >> (cfg.n_levels - 1)) < 2))
            throw rt_error(RT_E_UNSUPPORTED, "forward: FreeU needs a deepest grid of at least 2 x 2 (latents of " + std::to_string(2 << (cfg.n_levels - 1)) + " or more per side)");
        if (!dry()) pag_check(in);
        if (cfg.controlnet && !dry()) control_check(in);
        if (!dry()) ensure_fold();       // (normally a no-op: rt_set_prompts derived the folded projections already)
        const size_t m0 = ws.mark();
        const float* temb = time_embed(unet, in);
        std::vector<Tensor> skips;
        int ch, cw;
        Tensor x = encode(unet, in, temb, ch, cw,
            [&](const bf16_t* x8, f16_t* x0) { conv3(x8, A_CONV3, unet.conv_in, B, Hh, Ww, 8, x0, EPI_F16); },
            [&](const Tensor& s, int) { skips.push_back(s); });
        if (cfg.controlnet) control_pass(in, skips, x);
        for (size_t i = 0; i < unet.up.size(); ++i) {
            UpP& u = unet.up[i];
            for (size_t j = 0; j < u.res.size(); ++j) {
                Tensor sk = skips.back(); skips.pop_back();
                const bool inject_here = (i == 1 && j == 1);        // 'up_blocks.1.resnets.1' (rd.py:350, xl.py:1101)
                // FreeU, in place in front of EVERY resnet of up blocks 0 and 1: the hidden tensor is consumed by this resnet only and the
                // skip was popped for it (its other reader, the down path, is behind us in stream order).  All streams, injected ones included.
                if (i < 2 && !dry() && (fu_b[i] != 1.f || fu_s[i] != 1.f)) {
                    const double by = (fu_b[i] != 1.f ? 2.0 * (x.C / 2) : 0.0) + (fu_s[i] != 1.f ? 3.0 * sk.C : 0.0);
                    prof_begin(RT_PROF_ATTN_STORE, 0.0, 2.0 * B * ch * cw * by);      // priced in bytes like the token-map store: skip read twice + written, half the hidden read + written
                    launch_freeu(x.p, x.C, sk.p, sk.C, B, ch, cw, fu_b[i], fu_s[i], stream);
                    prof_end();
                }
                x = resnet(u.res[j], in, ch * cw, ch, cw, x, &sk, temb, inject_here);
                trace_point(u.res[j].name, x, B, ch * cw);
                if (u.has_attn) { x = transformer(u.attn[j], in, ch * cw, x); trace_point(u.attn[j].name, x, B, ch * cw); }
            }
            if (u.has_up) {
                f16_t* y = ws.f16((size_t)B * ch * cw * 4 * u.C);
                {
                    Scope sc(ws);
                    bf16_t* xb = ws.b16((size_t)B * ch * cw * u.C);
                    if (!dry()) launch_cast_f16_bf16(x.p, xb, (size_t)B * ch * cw * u.C, stream);
                    conv3(xb, A_CONV3_UP2, u.up, B, ch, cw, u.C, y, EPI_F16);
                }
                ch *= 2; cw *= 2;
                x = Tensor{y, u.C};
                if (tracing()) trace_point("up_blocks." + std::to_string(i) + ".upsamplers.0.conv", x, B, ch * cw);
            }
        }
        {
            Scope sc(ws);
            bf16_t* hn = ws.b16((size_t)B * HW0 * x.C);
            groupnorm(x.p, nullptr, 2, x.C, 0, B, HW0, norm_out, cfg.norm_eps, true, hn, nullptr);
            conv3(hn, A_CONV3, conv_out, B, Hh, Ww, x.C, in.eps_out, EPI_F32);
        }
        ws.release(m0);
        cur_hw = 0;
    }

    // ---------------------------------------------------------------------------- per-image setup
    // pe [P, L, D]: prompt p's first counts[p] rows are its keys (77 per chunk; counts == nullptr: all L); the rest of its L rows is not read
    void set_prompts(const float* pe, const int* counts, int L, const float* pooled, const float* time_ids, int P, int pooled_dim) {
        RT_REQUIRE(P >= 1 && P <= cfg.max_prompts, "set_prompts: too many prompts");
        RT_REQUIRE(L >= 77 && L % 77 == 0, "set_prompts: the embeddings must hold whole 77-token windows");
        for (int p_ = 0; p_ < P; ++p_) {
            const int c = counts ? counts[p_] : L;
            RT_REQUIRE(c >= 77 && c % 77 == 0 && c <= L, "set_prompts: a prompt's key count must be a multiple of 77, at most the embeddings' length");
            if (c > cfg.max_keys)
                throw rt_error(RT_E_INVALID, "set_prompts: a prompt of " + std::to_string(c) + " keys on an engine built for at most " +
                                                 std::to_string(cfg.max_keys) + " (rt_config.max_keys)");
        }
        require_bound();
        const int D = cfg.cross_attention_dim, KPr = KP();
        Scope sc(ws);
        bf16_t* ctx = ws.b16((size_t)cfg.max_prompts * KPr * D);
        if (cfg.lora_rank > 0) ctx = lora_ctx;                        // kept for rt_set_lora_scales (the scratch above stays reserved: same workspace plan)
        // rows past a prompt's own keys are zeros: their K / V^T rows are finite, and masked by every attention kernel
        for (int p_ = 0; p_ < P; ++p_)
            launch_pad_ctx(pe + (size_t)p_ * L * D, ctx + (size_t)p_ * KPr * D, counts ? counts[p_] : L, KPr, D, stream);
        // one prompt = one "stream" of 96 rows: the tile class / split-K rule of these GEMMs is keyed on that, so a prompt's cached
        // K / V bits do not depend on how many other prompts share the set
        cur_hw = 96;
        for (NetP* net : nets) net->for_each_tblock([&](TransformerP& t, TBlockP& k) {
            gemm(ctx, D, k.k2, P * KPr, k.kcache, t.heads * t.DP, EPI_BF16);
            gemm_vt(k.v2, ctx, D, P * KPr, k.vtcache, cfg.max_prompts * KPr);
        });
        cur_hw = 0;
        for (NetP* net : nets) HIP_CHECK(hipMemsetAsync(net->aug_emb, 0, (size_t)cfg.max_prompts * temb_dim * 4, stream));
        if (cfg.addition_text_time) {
            RT_REQUIRE(pooled && time_ids, "set_prompts: SDXL needs pooled embeds and time_ids");
            const int td = cfg.addition_time_embed_dim, Kin = cfg.projection_class_embeddings_input_dim;
            RT_REQUIRE(pooled_dim + 6 * td == Kin, "set_prompts: pooled_dim + 6*time_embed_dim != projection input dim");
            float* tid = ws.f32(8); float* tsin = ws.f32((size_t)6 * td);
            float* add = ws.f32((size_t)P * Kin); float* hmid = ws.f32((size_t)P * temb_dim);
            HIP_CHECK(hipMemcpyAsync(tid, time_ids, 24, hipMemcpyHostToDevice, stream));
            launch_timestep_embed(tid, 6, td, tsin, td, stream);
            for (int p_ = 0; p_ < P; ++p_) {
                HIP_CHECK(hipMemcpyAsync(add + (size_t)p_ * Kin, pooled + (size_t)p_ * pooled_dim, (size_t)pooled_dim * 4, hipMemcpyDeviceToDevice, stream));
                HIP_CHECK(hipMemcpyAsync(add + (size_t)p_ * Kin + pooled_dim, tsin, (size_t)6 * td * 4, hipMemcpyDeviceToDevice, stream));
            }
            for (NetP* net : nets) {      // every network's own add_embedding of the same (pooled | time ids) rows
                launch_small_linear(add, Kin, net->a1.w, net->a1.K, net->a1.b, hmid, temb_dim, P, temb_dim, Kin, 0, 0, stream);
                launch_small_linear(hmid, temb_dim, net->a2.w, net->a2.K, net->a2.b, net->aug_emb, temb_dim, P, temb_dim, temb_dim, 1, 0, stream);
            }
        }
        n_prompts = P;
        for (int p_ = 0; p_ < P; ++p_) prompt_keys[p_] = counts ? counts[p_] : L;
        std::fill(ip_scale.begin(), ip_scale.end(), 0.f);              // the slots change meaning: no prompt has an image until rt_set_image_prompts
        std::fill(ctl.scale.begin(), ctl.scale.end(), 0.f);            // ... and none is controlled until rt_set_control_scales (the hint stays)
        std::fill(lora_scale.begin(), lora_scale.end(), 0.f);          // ... and none is adapted until rt_set_lora_scales (the caches above carry no term)
        std::fill(pag_scale.begin(), pag_scale.end(), 0.f);            // ... and none has a perturbed twin until rt_set_pag_scales (the applied layers stay)
        lora_cache_dirty = false;
        HIP_CHECK(hipStreamSynchronize(stream));   // host buffers (time_ids) may go away
    }

    // The regional LoRA term of one projection for up to RT_MAXB streams (rows_at / sc4 host arrays): profiled as RT_PROF_LORA
    void lora_add(const LoraW& w, const bf16_t* X, int ldx, void* Y, int ldy, int form, const int* rows_at, const float* sc4, int B, int rows) {
        double nact = 0;
        for (int b = 0; b < B; ++b) nact += sc4[4 * b] != 0.f || sc4[4 * b + 1] != 0.f || sc4[4 * b + 2] != 0.f || sc4[4 * b + 3] != 0.f;
        if (nact == 0) return;
        const int R = cfg.lora_rank;
        prof_begin(RT_PROF_LORA, 2.0 * nact * rows * R * ((double)w.K + w.N), 2.0 * nact * rows * ((double)w.K + 2.0 * w.N));
        launch_lora_add(X, ldx, w.down, w.K, w.up, R, w.aor, lora_col, Y, ldy, form, rows_at, sc4, B, rows, w.K, w.N, R, stream);
        prof_end();
    }
    // ff.net.0.proj of ONE adapted stream from its fp32 pre-activations (lora_geglu_kernel): Z read, X read, out written once
    void lora_geglu(const LoraW& w, const bf16_t* X, const float* Z, bf16_t* out, const float* sc4, int rows) {
        const int R = cfg.lora_rank, row0 = 0;
        prof_begin(RT_PROF_LORA, 2.0 * rows * R * ((double)w.K + w.N), (double)rows * (4.0 * w.N + 2.0 * w.K + w.N));
        launch_lora_geglu(X, w.K, w.down, w.K, w.up, R, w.aor, lora_col, Z, w.N, out, w.N / 2, &row0, sc4, 1, rows, w.K, w.N, R, stream);
        prof_end();
    }
    void set_lora_columns(const int* col, int R) {
        RT_REQUIRE(cfg.lora_rank > 0, "set_lora_columns: the engine was built without regional LoRA (rt_config.lora_rank == 0)");
        RT_REQUIRE(col && R == cfg.lora_rank, "set_lora_columns: one adapter index per rank column (rt_config.lora_rank of them)");
        for (int j = 0; j < R; ++j) RT_REQUIRE(col[j] >= 0 && col[j] < 4, "set_lora_columns: an adapter index must be 0 .. 3");
        for (float s : lora_scale) RT_REQUIRE(s == 0.f, "set_lora_columns: scales are set (rt_set_lora_scales with zeros, or rt_set_prompts, first)");
        HIP_CHECK(hipMemcpyAsync(lora_col, col, (size_t)R * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    // scales [P][4].  Validates everything before it touches the state.  The attn2 K / V^T caches of the main UNet: rebuilt with the GEMMs
    // of set_prompts (same arguments, same bits) when they carry a term, then the term of every slot with a non-zero scale is added to
    // that slot's KP rows - row-major into kcache, transposed into vtcache.
    void set_lora_scales(const float* scales, int P) {
        RT_REQUIRE(cfg.lora_rank > 0, "set_lora_scales: the engine was built without regional LoRA (rt_config.lora_rank == 0)");
        RT_REQUIRE(scales, "set_lora_scales: scales");
        RT_REQUIRE(P >= 1 && P <= n_prompts, "set_lora_scales: more slots than prompts set (rt_set_prompts first)");
        bool any = false;
        for (int i = 0; i < 4 * P; ++i) { RT_REQUIRE(std::isfinite(scales[i]), "set_lora_scales: a scale must be finite"); any = any || scales[i] != 0.f; }
        require_bound();
        const int D = cfg.cross_attention_dim, KPr = KP();
        if (lora_cache_dirty) {
            cur_hw = 96;
            for_each_tblock([&](TransformerP& t, TBlockP& k) {
                gemm(lora_ctx, D, k.k2, n_prompts * KPr, k.kcache, t.heads * t.DP, EPI_BF16);
                gemm_vt(k.v2, lora_ctx, D, n_prompts * KPr, k.vtcache, cfg.max_prompts * KPr);
            });
            cur_hw = 0;
            lora_cache_dirty = false;
        }
        for (int p_ = 0; p_ < cfg.max_prompts; ++p_)
            for (int l = 0; l < 4; ++l) lora_scale[(size_t)p_ * 4 + l] = p_ < P ? scales[4 * p_ + l] : 0.f;
        if (any) {
            for (int p0 = 0; p0 < P; p0 += RT_MAXB) {
                const int nb = std::min(RT_MAXB, P - p0);
                int rows_at[RT_MAXB];
                for (int b = 0; b < nb; ++b) rows_at[b] = (p0 + b) * KPr;
                for_each_tblock([&](TransformerP& t, TBlockP& k) {
                    lora_add(k.lora[5], lora_ctx, D, k.kcache, t.heads * t.DP, 0, rows_at, scales + 4 * p0, nb, KPr);
                    lora_add(k.lora[6], lora_ctx, D, k.vtcache, cfg.max_prompts * KPr, 1, rows_at, scales + 4 * p0, nb, KPr);
                });
            }
            lora_cache_dirty = true;
        }
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // tokens [P, ip_tokens, D] fp32 (device): slot p's first counts[p] rows are its image tokens.  Validates everything before it touches the state.
    void set_image_prompts(const float* tokens, const int* counts, const float* scales, int P) {
        RT_REQUIRE(cfg.ip_tokens > 0, "set_image_prompts: the engine was built without image prompts (rt_config.ip_tokens == 0)");
        RT_REQUIRE(scales, "set_image_prompts: scales");
        RT_REQUIRE(P >= 1 && P <= n_prompts, "set_image_prompts: more slots than prompts set (rt_set_prompts first)");
        bool any = false;
        for (int p_ = 0; p_ < P; ++p_) {
            RT_REQUIRE(std::isfinite(scales[p_]), "set_image_prompts: a scale must be finite");
            RT_REQUIRE(!counts || (counts[p_] >= 1 && counts[p_] <= cfg.ip_tokens), "set_image_prompts: a count must be in 1 .. ip_tokens");
            any = any || scales[p_] != 0.f;
        }
        RT_REQUIRE(tokens || !any, "set_image_prompts: tokens may be NULL only when every scale is 0");
        require_bound();
        if (tokens) {
            const int D = cfg.cross_attention_dim, T = cfg.ip_tokens;
            Scope sc(ws);
            bf16_t* ctx = ws.b16((size_t)cfg.max_prompts * 16 * D);
            for (int p_ = 0; p_ < P; ++p_)                            // rows past a slot's count are zeros, in the caches too
                launch_pad_ctx(tokens + (size_t)p_ * T * D, ctx + (size_t)p_ * 16 * D, counts ? counts[p_] : T, 16, D, stream);
            // one slot = one "stream" of 16 rows (set_prompts: a slot's cached bits do not depend on how many other slots are set)
            cur_hw = 16;
            for_each_tblock([&](TransformerP& t, TBlockP& k) {
                const int HD = t.heads * t.DP;
                gemm(ctx, D, k.kip, P * 16, k.kipcache, HD, EPI_BF16);
                gemm_vt(k.vip, ctx, D, P * 16, k.vtipcache, cfg.max_prompts * 16);
            });
            cur_hw = 0;
        }
        for (int p_ = 0; p_ < cfg.max_prompts; ++p_) {
            ip_scale[p_] = p_ < P ? scales[p_] : 0.f;
            if (p_ < P) ip_count[p_] = counts ? counts[p_] : cfg.ip_tokens;
        }
        HIP_CHECK(hipStreamSynchronize(stream));   // the launches read the caller's tokens
    }

    // controlnet_cond_embedding on the hint [Ch, 8 h, 8 w] (device, fp32): eight 3x3 convolutions in fp32 with the SiLU in their epilogue
    // (control_conv3_kernel).  The arguments are validated before the state is touched; scratch lives for this call only.
    void set_control_hint(const float* hint, int h, int w) {
        RT_REQUIRE(cfg.controlnet, "set_control_hint: the engine was built without a ControlNet (rt_config.controlnet == 0)");
        if (!hint) { ctl.has_hint = false; ctl.hint_h = ctl.hint_w = 0; return; }
        RT_REQUIRE(h >= 1 && w >= 1 && h <= cfg.latent_h && w <= cfg.latent_w, "set_control_hint: latent grid outside the plan");
        require_bound();
        const int C0 = cfg.block_out_channels[0], CP = (ctl.hint_ch + 7) & ~7;
        const size_t HWi = (size_t)64 * h * w;
        // the largest activation of the chain: the input, conv_in / blocks.0 at full size, then a quarter of the pixels per stride-2 block
        size_t need = HWi * std::max(CP, ctl.ce_ch[0]);
        for (int i = 1; i < 4; ++i) need = std::max(need, (HWi >> (2 * i)) * (size_t)ctl.ce_ch[i]);
        if (!ctl.emb_f32) {
            HIP_CHECK(hipMalloc((void**)&ctl.emb_f32, (size_t)cfg.latent_h * cfg.latent_w * C0 * 4));
            HIP_CHECK(hipMalloc((void**)&ctl.emb_f16, (size_t)cfg.latent_h * cfg.latent_w * C0 * 2));
        }
        struct Tmp { void* p = nullptr; ~Tmp() { (void)hipFree(p); } } a_, b_;
        HIP_CHECK(hipMalloc(&a_.p, need * 4)); HIP_CHECK(hipMalloc(&b_.p, need * 4));
        float* cur = (float*)a_.p; float* nxt = (float*)b_.p;
        ctl.has_hint = false;                 // (an error below leaves the engine without a hint, never with half of one)
        int Hc = 8 * h, Wc = 8 * w;
        auto conv_silu = [&](const ControlP::ConvF& W, int stride, int CinP) {
            RT_REQUIRE(W.CinP == CinP, "set_control_hint: weight / input channel mismatch");
            const int Ho = stride == 2 ? (Hc + 1) / 2 : Hc, Wo = stride == 2 ? (Wc + 1) / 2 : Wc;
            RT_REQUIRE((size_t)Hc * Wc * CinP <= need && (size_t)Ho * Wo * W.N <= need, "set_control_hint: scratch");
            launch_control_conv3(cur, W.w, W.b, nxt, nullptr, Hc, Wc, CinP, W.N, stride, 1, stream);
            Hc = Ho; Wc = Wo;
            std::swap(cur, nxt);
        };
        launch_control_hint(hint, cur, ctl.hint_ch, CP, HWi, stream);
        conv_silu(ctl.ce_in, 1, CP);
        for (int i = 0; i < 3; ++i) {
            conv_silu(ctl.ce_blocks[2 * i], 1, ctl.ce_ch[i]);
            conv_silu(ctl.ce_blocks[2 * i + 1], 2, ctl.ce_ch[i]);
        }
        RT_REQUIRE(Hc == h && Wc == w && ctl.ce_out.CinP == ctl.ce_ch[3], "set_control_hint: embedder grid");
        // conv_out: the fp32 embedding and the same values rounded once to the trunk's fp16 (the residual operand of controlnet.conv_in)
        launch_control_conv3(cur, ctl.ce_out.w, ctl.ce_out.b, ctl.emb_f32, ctl.emb_f16, h, w, ctl.ce_ch[3], C0, 1, 0, stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        ctl.has_hint = true; ctl.hint_h = h; ctl.hint_w = w;
    }
    void set_control_scales(const float* scales, int P) {
        RT_REQUIRE(cfg.controlnet, "set_control_scales: the engine was built without a ControlNet (rt_config.controlnet == 0)");
        RT_REQUIRE(scales, "set_control_scales: scales");
        RT_REQUIRE(P >= 1 && P <= n_prompts, "set_control_scales: more slots than prompts set (rt_set_prompts first)");
        for (int p_ = 0; p_ < P; ++p_) RT_REQUIRE(std::isfinite(scales[p_]), "set_control_scales: a scale must be finite");
        for (int p_ = 0; p_ < cfg.max_prompts; ++p_) ctl.scale[p_] = p_ < P ? scales[p_] : 0.f;
    }

    // Perturbed-attention guidance.  names: ';'-joined attn1 module names as rt_attn_module_info lists them (empty / NULL: none applied).
    // Everything is checked before the state changes.
    void set_pag_layers(const char* names) {
        std::vector<std::string> want;
        const std::string all = names ? names : "";
        for (size_t at = 0; at <= all.size();) {
            const size_t end = std::min(all.find(';', at), all.size());
            if (end > at) want.push_back(all.substr(at, end - at));
            at = end + 1;
        }
        for (const std::string& w : want) {
            int found = 0;      // 1: an attn1 module, 2: an attn2 module
            for_each_tblock([&](TransformerP&, TBlockP& k) { if (k.mod_name[0] == w) found = 1; else if (k.mod_name[1] == w) found = 2; });
            if (found == 2) throw rt_error(RT_E_INVALID, "set_pag_layers: " + w + " is a cross-attention module; perturbed attention applies to attn1 modules only");
            if (found == 0) throw rt_error(RT_E_INVALID, "set_pag_layers: unknown attention module " + w);
        }
        if (want.empty() && pag_on()) throw rt_error(RT_E_INVALID, "set_pag_layers: an empty applied set while a slot has a non-zero scale (rt_set_pag_scales)");
        pag_layers = 0;
        for_each_tblock([&](TransformerP&, TBlockP& k) {
            k.pag = std::find(want.begin(), want.end(), k.mod_name[0]) != want.end();
            if (k.pag) ++pag_layers;
        });
    }
    // One finite scale per prompt slot of rt_set_prompts, the calling pattern of rt_set_control_scales: slot 0 is the negative prompt, which
    // has no twin; the rich pass runs region r on slot r + 1 and the base prompt on the last slot, the plain pass its text on slot 1.
    void set_pag_scales(const float* scales, int P) {
        RT_REQUIRE(scales, "set_pag_scales: scales");
        RT_REQUIRE(P >= 1 && P <= n_prompts, "set_pag_scales: more slots than prompts set (rt_set_prompts first)");
        bool any = false;
        for (int p_ = 0; p_ < P; ++p_) {
            if (!std::isfinite(scales[p_])) throw rt_error(RT_E_INVALID, "set_pag_scales: the scale of slot " + std::to_string(p_) + " is not finite");
            any |= scales[p_] != 0.f;
        }
        if (scales[0] != 0.f) throw rt_error(RT_E_INVALID, "set_pag_scales: slot 0 is the negative prompt, which has no perturbed twin: its scale must be 0");
        if (any && pag_layers == 0) throw rt_error(RT_E_INVALID, "set_pag_scales: a non-zero scale but the applied set is empty (rt_set_pag_layers first)");
        for (int p_ = 0; p_ < cfg.max_prompts; ++p_) pag_scale[p_] = p_ < P ? scales[p_] : 0.f;
    }
    // Before any launch of a step with PAG on: the two combinations that are out of scope
    void pag_step_check(float g) const {
        if (!pag_on()) return;
        if (g == 0.f) throw rt_error(RT_E_INVALID, "perturbed-attention guidance needs classifier-free guidance: guidance_scale is 0 (the fold divides by it)");
        if (guidance_rescale > 0.f)
            throw rt_error(RT_E_INVALID, "perturbed-attention guidance together with guidance_rescale > 0 is not supported (the rescale needs the unfolded text prediction)");
    }
    // The twin of stream s, behind all streams planned so far
    int pag_twin(FwdIn& in, int& F, int s, const char* who) {
        if (F >= cfg.max_streams)
            throw rt_error(RT_E_INVALID, std::string(who) + ": perturbed-attention guidance needs more streams (" + std::to_string(F + 1) +
                                             " or more) than the engine was built for (max_streams " + std::to_string(cfg.max_streams) + ")");
        in.x[F] = in.x[s]; in.scale[F] = in.scale[s]; in.prompt[F] = in.prompt[s]; in.fontsize[F] = in.fontsize[s];
        in.qk_src[F] = in.qk_src[s] == s ? F : in.qk_src[s]; in.res_src[F] = in.res_src[s]; in.perturb[F] = 1;
        return F++;
    }
    // The fold of a step (pag.hip), ahead of everything in finish_step: eps[s] <- fmaf(sigma / g, eps[s] - eps[twin], eps[s])
    struct PagPairs { int n = 0, F = 0; int s[RT_MAXB], twin[RT_MAXB]; float rho[RT_MAXB]; };
    PagPairs pag_pairs;          // of the step being planned: region_plan / plain_finish set it, finish_step consumes it
    void pag_fold() {
        if (!pag_pairs.n) return;
        const PagPairs& p = pag_pairs;
        const int F = p.F;
        prof_begin(RT_PROF_PAG, 0.0, 3.0 * p.n * 16.0 * lat_h * lat_w);      // partner read + written, twin read
        launch_pag_fold(eps, F, lat_h * lat_w, p.s, p.twin, p.rho, p.n, stream);
        prof_end();
    }

    void set_fontsize(const int64_t* word_pos, const float* font_size, int n) {
        // set 0: plain softmax; set 1: font-size softmax (attention_processor.py:386-396).  wabs = 0 on padded keys.
        // One table row per key POSITION of the longest prompt the engine holds (KP = 96 rows per chunk, keys first): chunk c of a prompt
        // sits at keys 77 c + [0, 77), so every position < max_keys is a key of some prompt length.  The kernels mask by the stream's own
        // key count, not by these tables: an entry beyond a stream's keys has no effect on it.
        const int KPr = KP();
        float ha[2 * 288], hs[2 * 288];
        for (int s = 0; s < 2; ++s) for (int k = 0; k < KPr; ++k) { ha[s * KPr + k] = k < cfg.max_keys ? 1.f : 0.f; hs[s * KPr + k] = 1.f; }
        for (int i = 0; i < n; ++i) {
            RT_REQUIRE(word_pos[i] >= 0 && word_pos[i] < cfg.max_keys, "set_fontsize: word_pos out of range");
        }
        // torch index_put semantics with repeated indices: the last write wins for '=' and every '*=' on the
        // gathered copy also resolves to a single write per index (attention_processor.py:393,396)
        for (int i = 0; i < n; ++i) {
            const int k = (int)word_pos[i];
            ha[KPr + k] = std::fabs(font_size[i]);
            hs[KPr + k] = font_size[i] > 0 ? 1.f : (font_size[i] < 0 ? -1.f : 0.f);
        }
        HIP_CHECK(hipMemcpyAsync(wabs, ha, (size_t)2 * KPr * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(wsgn, hs, (size_t)2 * KPr * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    bool any_store() { bool any = false; for_each_tblock([&](TransformerP&, TBlockP& k) { any |= k.store_mode[0] || k.store_mode[1]; }); return any; }
    void attn_store_enable(const std::string& name, int mode) {
        bool found = false;
        for_each_tblock([&](TransformerP& t, TBlockP& k) {
            for (int w = 0; w < 2; ++w) {
                if (k.mod_name[w] != name) continue;
                found = true;
                const size_t N = (size_t)(cfg.latent_h >> t.level) * (cfg.latent_w >> t.level);
                const size_t cols = w == 0 ? N : (size_t)cfg.max_keys;
                if (mode != 0 && w == 0 && N > 1024)
                    throw rt_error(RT_E_UNSUPPORTED, "attention store: self-attention maps above 32x32 are not recorded (never consumed: attention_utils.py:243-248)");
                if (mode != 0 && k.store_cap[w] < N * cols) {
                    if (k.store[w]) HIP_CHECK(hipFree(k.store[w]));
                    HIP_CHECK(hipMalloc((void**)&k.store[w], N * cols * 4));
                    k.store_cap[w] = N * cols;
                }
                k.store_mode[w] = mode; k.store_calls[w] = 0; k.store_rows[w] = k.store_cols[w] = 0;
                if (mode != 0) HIP_CHECK(hipMemsetAsync(k.store[w], 0, k.store_cap[w] * 4, stream));
            }
        });
        if (!found) throw rt_error(RT_E_INVALID, "attention store: unknown attention module " + name);
    }
    void attn_store_reset() {
        for_each_tblock([&](TransformerP&, TBlockP& k) {
            for (int w = 0; w < 2; ++w) {
                k.store_calls[w] = 0; k.store_rows[w] = k.store_cols[w] = 0;
                if (k.store[w]) HIP_CHECK(hipMemsetAsync(k.store[w], 0, k.store_cap[w] * 4, stream));
            }
        });
    }

    void require_bound() {
        for (auto& s : slots) if (!s.bound) throw rt_error(RT_E_MISSING_WEIGHT, "weight not bound: " + s.name);
    }

    // ---------------------------------------------------------------------------- step drivers
    void region_step(int i, float g, double inject_selfattn, double inject_background, bool xl, bool elide, bool defer_blend);
    void region_plan(int i, float g, double isa, double ibg, bool xl, bool elide, bool defer_blend, FwdIn& in, StepArgs& a, bool& blend_out, bool& inject_out);
    void region_finish(int i, StepArgs& a, bool blend_deferred);
    void finish_step(int i, StepArgs& a);
    // intra-image split (step_driver.inl): the forwards of this rank's contiguous stream range, then - after the ranks exchanged their
    // slices of `eps` - the epilogue on all of them
    void region_step_part(int i, float g, double isa, double ibg, bool xl, bool elide, bool defer_blend, int part, int nparts, int* first, int* count, int* plan_info);
    void region_step_finish(int i, float g, double isa, double ibg, bool xl, bool elide, bool defer_blend);
    bool pending_blend = false;
    // the source image of an image start (rt_set_source): device copies owned by the engine, one allocation at the plan's latent size
    float* src_buf = nullptr;                    // x0 [4, HW] | noise [4, HW] | keep [HW]
    float *src_x0 = nullptr, *src_noise = nullptr, *src_keep = nullptr;
    bool has_source = false, has_keep = false;
    int src_h = 0, src_w = 0;
    void plain_step(int i, float g);
    void plain_forward(int i, int first, int count);
    int plain_streams();
    void plain_finish(int i, float g);
    void plain_step_part(int i, int part, int nparts, int* first, int* count);
};

#include "step_driver.inl"

// ================================================================================================
// C ABI
#define RT_TRY(e, ...)                                                             \
    try { __VA_ARGS__; return RT_OK; }                                                    \
    catch (const rt_error& ex) { (e)->err = ex.what(); return ex.code; }           \
    catch (const std::exception& ex) { (e)->err = ex.what(); return RT_E_INVALID; }

extern "C" {

int rt_create(const rt_config* cfg, int device, rt_engine** out) {
    rt_engine* e = nullptr;
    try {
        RT_REQUIRE(cfg && out, "rt_create: null argument");
        RT_REQUIRE(cfg->n_levels >= 2 && cfg->n_levels <= RT_MAX_LEVELS, "rt_create: n_levels");
        RT_REQUIRE(cfg->max_streams >= 1 && cfg->max_streams <= RT_MAXB, "rt_create: max_streams must be in [1,16]");
        RT_REQUIRE(cfg->in_channels == 4 && cfg->out_channels == 4, "rt_create: latent channels must be 4");
        RT_REQUIRE(cfg->cross_attention_dim % 8 == 0, "rt_create: cross_attention_dim % 8");
        RT_REQUIRE(cfg->max_keys == 0 || cfg->max_keys == 77 || cfg->max_keys == 154 || cfg->max_keys == 231, "rt_create: max_keys must be 77, 154 or 231 (0 = 77)");
        RT_REQUIRE(cfg->ip_tokens >= 0 && cfg->ip_tokens <= 16, "rt_create: ip_tokens must be 0 (no image prompts) or 1 .. 16");
        RT_REQUIRE(cfg->controlnet == 0 || cfg->controlnet == 1, "rt_create: controlnet must be 0 or 1");
        RT_REQUIRE(cfg->lora_rank >= 0 && cfg->lora_rank <= 128 && cfg->lora_rank % 16 == 0, "rt_create: lora_rank must be 0 (no regional LoRA) or a multiple of 16 up to 128");
        RT_REQUIRE(cfg->lora_targets == 0 || (cfg->lora_targets == 1 && cfg->lora_rank > 0), "rt_create: lora_targets must be 0 (the attention projections) or, with lora_rank > 0, 1 (feed-forward, proj_in and proj_out as well)");
        e = new rt_engine();
        e->cfg = *cfg; e->device = device;
        e->lora_scale.assign((size_t)std::max(1, cfg->max_prompts) * 4, 0.f);
        e->pag_scale.assign((size_t)std::max(1, cfg->max_prompts), 0.f);
        e->ip_count.assign((size_t)std::max(1, cfg->max_prompts), 0); e->ip_scale.assign((size_t)std::max(1, cfg->max_prompts), 0.f);
        if (e->cfg.max_keys == 0) e->cfg.max_keys = 77;
        e->prompt_keys.assign((size_t)std::max(1, e->cfg.max_prompts), 77);
        // pass 1: measure the arena (no device needed: lets CPU-only hosts enumerate the weight table)
        e->arena = Arena(); e->sarena = Arena(); e->farena = Arena(); e->ws.dry = true;
        e->build_plan();
        e->arena_bytes = e->arena.off + 256; e->sarena_bytes = e->sarena.off + 256; e->farena_bytes = e->farena.off + 256;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device < 0) {
            // weight-table-only engine (CPU box): every device call will fail with RT_E_STATE
            e->arena_base = nullptr;
            *out = e;
            return RT_OK;
        }
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipStreamCreate(&e->stream));
        e->own_stream = e->stream;
        HIP_CHECK(hipMalloc((void**)&e->arena_base, e->arena_bytes));
        HIP_CHECK(hipMemset(e->arena_base, 0, e->arena_bytes));
        HIP_CHECK(hipMalloc((void**)&e->sarena_base, e->sarena_bytes));
        HIP_CHECK(hipMemset(e->sarena_base, 0, e->sarena_bytes));
        HIP_CHECK(hipMalloc((void**)&e->farena_base, e->farena_bytes));
        HIP_CHECK(hipMemset(e->farena_base, 0, e->farena_bytes));
        e->arena = Arena(); e->arena.base = e->arena_base; e->arena.cap = e->arena_bytes;
        e->sarena = Arena(); e->sarena.base = e->sarena_base; e->sarena.cap = e->sarena_bytes;
        e->farena = Arena(); e->farena.base = e->farena_base; e->farena.cap = e->farena_bytes;
        e->build_plan();
        // pass 2: measure the workspace with a dry forward at the largest shape
        {
            FwdIn in{}; in.B = cfg->max_streams; in.h = cfg->latent_h; in.w = cfg->latent_w;
            for (int b = 0; b < in.B; ++b) { in.qk_src[b] = b; in.res_src[b] = b ? 0 : -1; in.prompt[b] = 0; }
            e->ws = Workspace(); e->ws.dry = true;
            e->splitk_need = 0;
            e->unet_forward(in);
            {   // the K / V^T cache GEMMs of rt_set_prompts (one prompt = one 96-row stream) at the largest prompt count
                const int D = cfg->cross_attention_dim, P96 = cfg->max_prompts * e->KP();
                e->cur_hw = 96;
                for (NetP* net : e->nets) net->for_each_tblock([&](TransformerP& t, TBlockP& k) {
                    e->gemm(nullptr, D, k.k2, P96, nullptr, t.heads * t.DP, EPI_BF16);
                    e->gemm_vt(k.v2, nullptr, D, P96, nullptr, P96);
                    if (cfg->ip_tokens > 0 && k.kip.w) {      // ... and those of rt_set_image_prompts (one slot = one 16-row stream)
                        e->cur_hw = 16;
                        e->gemm(nullptr, D, k.kip, cfg->max_prompts * 16, nullptr, t.heads * t.DP, EPI_BF16);
                        e->gemm_vt(k.vip, nullptr, D, cfg->max_prompts * 16, nullptr, cfg->max_prompts * 16);
                        e->cur_hw = 96;
                    }
                });
                e->cur_hw = 0;
            }
            size_t peak = e->ws.peak;
            {   // split-K slices GROW as the maps shrink (the rule keys on ONE stream's tile count): an engine built for 128 x 128
                // latents and stepped at 64 x 64 needs more partial-sum scratch than the largest shape measures.  Dry passes at every
                // halved latent size the architecture admits record it, so no forward ever allocates.
                const int align = 1 << (cfg->n_levels - 1);
                for (int s = 2; s <= 16; s *= 2) {
                    FwdIn in2 = in; in2.h = cfg->latent_h / s; in2.w = cfg->latent_w / s;
                    if (in2.h * s != cfg->latent_h || in2.w * s != cfg->latent_w || in2.h % align || in2.w % align || in2.h < 8 || in2.w < 8) break;
                    const int deep = (in2.h / align) * (in2.w / align);
                    if (deep % 8) break;                               // attention levels need h*w % 8 == 0
                    e->unet_forward(in2);
                }
            }
            // set_prompts scratch
            size_t sp = (size_t)cfg->max_prompts * e->KP() * cfg->cross_attention_dim * 2 + (size_t)cfg->max_prompts * (cfg->projection_class_embeddings_input_dim + e->temb_dim) * 4 + (1 << 16);
            if (sp > peak) peak = sp;
            peak += 1 << 20;
            e->ws = Workspace();
            HIP_CHECK(hipMalloc((void**)&e->ws.base, peak));
            e->ws.cap = peak;
            if (e->splitk_need) {
                HIP_CHECK(hipMalloc((void**)&e->splitk_buf, e->splitk_need * 4));
                e->splitk_floats = e->splitk_need;
            }
            for (NetP* net : e->nets) {      // the time_emb_proj table of temb_all_kernel: batch-independent, uploaded once
                if (net->temb_tab.empty()) continue;
                HIP_CHECK(hipMalloc((void**)&net->temb_tab_dev, net->temb_tab.size() * sizeof(TembEntry)));
                HIP_CHECK(hipMemcpy(net->temb_tab_dev, net->temb_tab.data(), net->temb_tab.size() * sizeof(TembEntry), hipMemcpyHostToDevice));
            }
        }
        e->set_fontsize(nullptr, nullptr, 0);      // multiplier set 0/1 = plain softmax until rt_set_fontsize is called
        *out = e;
        return RT_OK;
    } catch (const std::exception& ex) {
        g_create_error = ex.what();
        delete e;
        return RT_E_INVALID;
    }
}

int rt_destroy(rt_engine* e) {
    if (!e) return RT_OK;
    if (e->arena_base) {
        (void)hipSetDevice(e->device); (void)hipStreamSynchronize(e->stream);
        for (auto& r : e->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        (void)hipFree(e->arena_base); (void)hipFree(e->sarena_base); (void)hipFree(e->farena_base); (void)hipFree(e->ws.base); (void)hipFree(e->splitk_buf); (void)hipFree(e->src_buf);
        for (NetP* net : e->nets) (void)hipFree(net->temb_tab_dev);
        (void)hipFree(e->ctl.emb_f32); (void)hipFree(e->ctl.emb_f16);
        (void)hipStreamDestroy(e->own_stream);
    }
    delete e;
    return RT_OK;
}

const char* rt_last_error(rt_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

static void need_device(rt_engine* e) { if (!e->arena_base) throw rt_error(RT_E_STATE, "engine has no device (weight-table-only)"); }

int rt_set_stream(rt_engine* e, void* s) { RT_TRY(e, { need_device(e); e->stream = s ? (hipStream_t)s : e->own_stream; }) }
int rt_synchronize(rt_engine* e) { RT_TRY(e, { need_device(e); HIP_CHECK(hipStreamSynchronize(e->stream)); }) }

int rt_weight_count(rt_engine* e) { return (int)e->slots.size(); }
int rt_weight_info(rt_engine* e, int idx, char* name, int cap, int64_t* shape4, int* ndim) {
    RT_TRY(e, {
        RT_REQUIRE(idx >= 0 && idx < (int)e->slots.size(), "rt_weight_info: index");
        const WeightSlot& s = e->slots[idx];
        RT_REQUIRE((int)s.name.size() < cap, "rt_weight_info: name buffer too small");
        std::strcpy(name, s.name.c_str());
        *ndim = (int)s.shape.size();
        for (size_t i = 0; i < s.shape.size(); ++i) shape4[i] = s.shape[i];
    })
}
int rt_bind_weight(rt_engine* e, const char* name, const void* ptr, int dtype, const int64_t* shape, int ndim) {
    RT_TRY(e, {
        need_device(e);
        auto it = e->slot_index.find(name);
        if (it == e->slot_index.end()) throw rt_error(RT_E_INVALID, std::string("unknown weight: ") + name);
        WeightSlot& s = e->slots[it->second];
        RT_REQUIRE(ndim == (int)s.shape.size(), "rt_bind_weight: rank mismatch");
        for (int i = 0; i < ndim; ++i)
            if (shape[i] != s.shape[i]) throw rt_error(RT_E_INVALID, std::string("shape mismatch for ") + name);
        RT_REQUIRE(dtype >= 0 && dtype <= 2, "rt_bind_weight: dtype");
        PackArgs p = s.pack; p.src = ptr; p.src_dtype = dtype;
        launch_pack(p, e->stream);
        if (s.up2) launch_pack_up2(ptr, dtype, s.up2, s.up2_cout, s.up2_cin, e->stream);
        s.bound = true;
        // Derived data follows a re-bind: the up-sampler phase pack above, the folded projections at the next forward (fold_dirty) and the
        // time_emb_proj table, which every forward reads from the arena.  What rt_set_prompts derived from the OLD weight - the K / V^T caches
        // (attn2.to_k / to_v, to_k_ip / to_v_ip) and the addition embeddings (add_embedding.*) - cannot be rebuilt here (the engine does
        // not keep the prompt embeddings): the prompts are discarded, and a forward or step before the next rt_set_prompts is an error.
        e->fold_dirty = true;
        if (s.name.find("controlnet_cond_embedding.") != std::string::npos) e->ctl.has_hint = false;      // the cached embedding came from the old weight
        if (s.name.compare(0, 14, "add_embedding.") == 0 || s.name.compare(0, 25, "controlnet.add_embedding.") == 0 || s.name.find(".attn2.to_k") != std::string::npos || s.name.find(".attn2.to_v") != std::string::npos)
            e->n_prompts = 0;
    })
}
int rt_weights_missing(rt_engine* e, char* buf, int cap) {
    int n = 0; std::string acc;
    for (auto& s : e->slots) if (!s.bound) { ++n; if (acc.size() + s.name.size() + 2 < (size_t)cap) { acc += s.name; acc += ';'; } }
    if (buf && cap > 0) { std::strncpy(buf, acc.c_str(), cap - 1); buf[cap - 1] = 0; }
    return n;
}
int rt_arena_info(rt_engine* e, void** p, uint64_t* bytes) { RT_TRY(e, { need_device(e); *p = e->arena_base; *bytes = e->arena_bytes; }) }
int rt_arena_mark_bound(rt_engine* e) { for (auto& s : e->slots) s.bound = true; e->fold_dirty = true; e->n_prompts = 0; e->ctl.has_hint = false; return RT_OK; }

int rt_set_prompts(rt_engine* e, const float* pe, const float* pooled, const float* tids, int P, int pooled_dim) {
    RT_TRY(e, { need_device(e); e->ensure_fold(); e->set_prompts(pe, nullptr, 77, pooled, tids, P, pooled_dim); })
}
int rt_set_prompts_keys(rt_engine* e, const float* pe, const int* key_counts, int L, const float* pooled, const float* tids, int P, int pooled_dim) {
    RT_TRY(e, { need_device(e); RT_REQUIRE(key_counts, "rt_set_prompts_keys: key counts"); e->ensure_fold(); e->set_prompts(pe, key_counts, L, pooled, tids, P, pooled_dim); })
}
int rt_set_image_prompts(rt_engine* e, const float* tokens, const int* counts, const float* scales, int P) {
    RT_TRY(e, { need_device(e); e->set_image_prompts(tokens, counts, scales, P); })
}
int rt_set_control_hint(rt_engine* e, const float* hint, int h, int w) { RT_TRY(e, { need_device(e); e->set_control_hint(hint, h, w); }) }
int rt_set_control_scales(rt_engine* e, const float* scales, int P) { RT_TRY(e, { need_device(e); e->set_control_scales(scales, P); }) }
int rt_set_pag_layers(rt_engine* e, const char* names) { RT_TRY(e, { e->set_pag_layers(names); }) }
int rt_set_pag_scales(rt_engine* e, const float* scales, int P) { RT_TRY(e, { need_device(e); e->set_pag_scales(scales, P); }) }
int rt_attn_cache_info(rt_engine* e, int idx, void** kcache, void** vtcache, long long* bytes_each) {
    RT_TRY(e, {
        need_device(e);
        RT_REQUIRE(kcache && vtcache && bytes_each, "rt_attn_cache_info: null outputs");
        int i = 0; bool found = false;
        e->for_each_tblock([&](TransformerP& t, TBlockP& k) {
            if (i++ != idx) return;
            *kcache = k.kcache; *vtcache = k.vtcache;
            *bytes_each = (long long)e->cfg.max_prompts * e->KP() * t.heads * t.DP * 2;
            found = true;
        });
        RT_REQUIRE(found, "rt_attn_cache_info: block index out of range (rt_attn_module_count / 2 blocks)");
    })
}
int rt_set_lora_columns(rt_engine* e, const int* col, int R) { RT_TRY(e, { need_device(e); e->set_lora_columns(col, R); }) }
int rt_set_lora_scales(rt_engine* e, const float* scales, int P) { RT_TRY(e, { need_device(e); e->set_lora_scales(scales, P); }) }
int rt_control_embedding_read(rt_engine* e, float* dst, int* rows, int* cols) {
    RT_TRY(e, {
        need_device(e);
        RT_REQUIRE(e->cfg.controlnet, "rt_control_embedding_read: the engine was built without a ControlNet (rt_config.controlnet == 0)");
        const int n = e->ctl.has_hint ? e->ctl.hint_h * e->ctl.hint_w : 0, C0 = e->cfg.block_out_channels[0];
        if (rows) *rows = n;
        if (cols) *cols = C0;
        if (dst && n) {
            HIP_CHECK(hipMemcpyAsync(dst, e->ctl.emb_f32, (size_t)n * C0 * 4, hipMemcpyDeviceToDevice, e->stream));
            HIP_CHECK(hipStreamSynchronize(e->stream));
        }
    })
}
int rt_set_masks(rt_engine* e, const float* m, int R, int h, int w) {
    RT_TRY(e, {
        need_device(e);
        RT_REQUIRE(R >= 1 && R <= RT_MAXB && h <= e->cfg.latent_h && w <= e->cfg.latent_w, "rt_set_masks: bad shape");
        HIP_CHECK(hipMemcpyAsync(e->masks, m, (size_t)R * 4 * h * w * 4, hipMemcpyDeviceToDevice, e->stream));
        e->n_regions = R; e->mask_hw = h * w;
    })
}
int rt_set_fontsize(rt_engine* e, const int64_t* wp, const float* fs, int n) { RT_TRY(e, { need_device(e); e->set_fontsize(wp, fs, n); }) }
int rt_set_schedule(rt_engine* e, int kind, const float* ts, int nts, const float* table, int ntab, int nsteps) {
    RT_TRY(e, {
        RT_REQUIRE(rt_sched_is_euler(kind) || kind == RT_SCHED_PNDM || rt_sched_is_dpm(kind), "rt_set_schedule: kind");
        if (rt_sched_is_euler(kind)) RT_REQUIRE(ntab == nts + 1, "euler: need n+1 sigmas");
        if (rt_sched_is_dpm(kind)) {
            RT_REQUIRE(ntab == 1000 && nts >= 1, "dpm-solver++: need alphas_cumprod[1000] and at least one timestep");
            for (int k = 0; k < nts; ++k)
                RT_REQUIRE(ts[k] >= 0.f && ts[k] < 1000.f && ts[k] == (float)(int)ts[k] && (k == 0 || ts[k] < ts[k - 1]),
                           "dpm-solver++: timesteps must be distinct integers in [0, 1000), descending");
        }
        e->sched_kind = kind; e->num_inference_steps = nsteps;
        e->timesteps.assign(ts, ts + nts); e->table.assign(table, table + ntab);
        e->solver.reset();
    })
}
int rt_set_latents(rt_engine* e, const float* l, int h, int w) {
    RT_TRY(e, {
        need_device(e);
        RT_REQUIRE(h <= e->cfg.latent_h && w <= e->cfg.latent_w, "rt_set_latents: too large");
        const size_t n = (size_t)4 * h * w * 4;
        HIP_CHECK(hipMemcpyAsync(e->lat, l, n, hipMemcpyDeviceToDevice, e->stream));
        HIP_CHECK(hipMemcpyAsync(e->lat_ref, l, n, hipMemcpyDeviceToDevice, e->stream));
        e->lat_h = h; e->lat_w = w;
        e->solver.reset();
    })
}
int rt_set_noise_seed(rt_engine* e, unsigned long long seed) { RT_TRY(e, { e->noise_seed = seed; }) }
int rt_set_prediction(rt_engine* e, int prediction_type, float guidance_rescale) {
    RT_TRY(e, {
        RT_REQUIRE(prediction_type == RT_PRED_EPSILON || prediction_type == RT_PRED_V, "rt_set_prediction: prediction_type must be 0 (epsilon) or 1 (v)");
        RT_REQUIRE(guidance_rescale >= 0.f && guidance_rescale <= 1.f, "rt_set_prediction: guidance_rescale must be in [0, 1]");
        e->prediction_type = prediction_type; e->guidance_rescale = guidance_rescale;
    })
}
int rt_set_freeu(rt_engine* e, float s1, float s2, float b1, float b2) {
    RT_TRY(e, {
        for (float v : {s1, s2, b1, b2}) RT_REQUIRE(std::isfinite(v) && v > 0.f, "rt_set_freeu: s1, s2, b1, b2 must be finite and > 0");
        e->fu_s[0] = s1; e->fu_s[1] = s2; e->fu_b[0] = b1; e->fu_b[1] = b2;
    })
}
int rt_set_source(rt_engine* e, const float* x0, const float* noise, const float* keep, int h, int w) {
    RT_TRY(e, {
        need_device(e);
        if (!x0) { e->has_source = e->has_keep = false; return RT_OK; }
        RT_REQUIRE(noise, "rt_set_source: noise is NULL");
        RT_REQUIRE(h >= 1 && w >= 1 && h <= e->cfg.latent_h && w <= e->cfg.latent_w, "rt_set_source: bad shape");
        const size_t cap = (size_t)e->cfg.latent_h * e->cfg.latent_w, hw = (size_t)h * w;
        if (!e->src_buf) {
            HIP_CHECK(hipSetDevice(e->device));
            HIP_CHECK(hipMalloc((void**)&e->src_buf, 9 * cap * 4));
            e->src_x0 = e->src_buf; e->src_noise = e->src_buf + 4 * cap; e->src_keep = e->src_buf + 8 * cap;
        }
        HIP_CHECK(hipMemcpyAsync(e->src_x0, x0, 4 * hw * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_CHECK(hipMemcpyAsync(e->src_noise, noise, 4 * hw * 4, hipMemcpyDeviceToDevice, e->stream));
        if (keep) HIP_CHECK(hipMemcpyAsync(e->src_keep, keep, hw * 4, hipMemcpyDeviceToDevice, e->stream));
        e->has_source = true; e->has_keep = keep != nullptr; e->src_h = h; e->src_w = w;
    })
}
int rt_noise_latents(rt_engine* e, float a, float b) {
    RT_TRY(e, {
        need_device(e);
        if (!e->has_source) throw rt_error(RT_E_STATE, "rt_noise_latents: no source (rt_set_source)");
        launch_noise_latents(e->lat, e->lat_ref, e->src_x0, e->src_noise, a, b, 4 * e->src_h * e->src_w, e->stream);
        e->lat_h = e->src_h; e->lat_w = e->src_w;
        e->solver.reset();
    })
}
int rt_source_blend(rt_engine* e, float a, float b) {
    RT_TRY(e, {
        need_device(e);
        if (!e->has_source) throw rt_error(RT_E_STATE, "rt_source_blend: no source (rt_set_source)");
        if (e->src_h != e->lat_h || e->src_w != e->lat_w) throw rt_error(RT_E_STATE, "rt_source_blend: source and latents differ in shape");
        if (e->has_keep) launch_source_blend(e->lat, e->src_x0, e->src_noise, e->src_keep, a, b, e->lat_h * e->lat_w, e->stream);
    })
}
int rt_get_latents(rt_engine* e, float* out, float* out_ref) {
    RT_TRY(e, {
        need_device(e);
        const size_t n = (size_t)4 * e->lat_h * e->lat_w * 4;
        HIP_CHECK(hipMemcpyAsync(out, e->lat, n, hipMemcpyDeviceToDevice, e->stream));
        if (out_ref) HIP_CHECK(hipMemcpyAsync(out_ref, e->lat_ref, n, hipMemcpyDeviceToDevice, e->stream));
    })
}
int rt_get_state_ptrs(rt_engine* e, float** latents, float** noise_pred) {
    RT_TRY(e, { need_device(e); HIP_CHECK(hipStreamSynchronize(e->stream)); *latents = e->lat; *noise_pred = e->noise_pred; })
}
int rt_region_step(rt_engine* e, int i, float g, double isa, double ibg, int xl, int elide) {
    RT_TRY(e, { need_device(e); e->region_step(i, g, isa, ibg, xl != 0, (elide & 1) != 0, (elide & 2) != 0); })
}
int rt_region_step_part(rt_engine* e, int i, float g, double isa, double ibg, int xl, int flags, int part, int nparts, int* first, int* count,
                        int* plan_info) {
    RT_TRY(e, { need_device(e); RT_REQUIRE(first && count, "rt_region_step_part: null outputs");
                e->region_step_part(i, g, isa, ibg, xl != 0, (flags & 1) != 0, (flags & 2) != 0, part, nparts, first, count, plan_info); })
}
int rt_region_step_finish(rt_engine* e, int i, float g, double isa, double ibg, int xl, int flags) {
    RT_TRY(e, { need_device(e); e->region_step_finish(i, g, isa, ibg, xl != 0, (flags & 1) != 0, (flags & 2) != 0); })
}
int rt_eps_info(rt_engine* e, void** dev_ptr, unsigned long long* bytes_per_stream, int* max_streams) {
    RT_TRY(e, { need_device(e); RT_REQUIRE(dev_ptr && bytes_per_stream && max_streams, "rt_eps_info: null outputs");
                RT_REQUIRE(e->lat_h > 0, "rt_eps_info: call rt_set_latents first");
                *dev_ptr = e->eps; *bytes_per_stream = (unsigned long long)e->lat_h * e->lat_w * 4 * 4; *max_streams = e->cfg.max_streams; })
}
int rt_background_blend(rt_engine* e) {
    RT_TRY(e, {
        need_device(e);
        if (e->pending_blend) { launch_background_blend(e->lat, e->lat_ref, e->masks + (size_t)(e->n_regions - 1) * 4 * e->mask_hw, 4 * e->mask_hw, e->stream); e->pending_blend = false; }
    })
}
int rt_plain_step(rt_engine* e, int i, float g) { RT_TRY(e, { need_device(e); e->plain_step(i, g); }) }
int rt_plain_step_part(rt_engine* e, int i, int part, int nparts, int* first, int* count) {
    RT_TRY(e, { need_device(e); RT_REQUIRE(first && count, "rt_plain_step_part: null outputs"); e->plain_step_part(i, part, nparts, first, count); })
}
int rt_plain_streams(rt_engine* e, int* n_streams) { RT_TRY(e, { RT_REQUIRE(n_streams, "rt_plain_streams: null argument"); *n_streams = e->plain_streams(); }) }
int rt_plain_step_finish(rt_engine* e, int i, float g) { RT_TRY(e, { need_device(e); e->plain_finish(i, g); }) }

// rt_unet_forward and rt_unet_forward_trace: one body.  module == nullptr: no trace.  The request is validated before anything is launched.
static void unet_forward_entry(rt_engine* e, const float* x, int B, int h, int w, float t, const float* in_scale, const int* prompt, const int* fontsize,
                               const int* qk_src, const int* res_src, float* out, const char* module, float* trace_out, long long trace_cap,
                               const int* perturb = nullptr) {
    {
        need_device(e); e->require_bound();
        RT_REQUIRE(B >= 1 && B <= e->cfg.max_streams, "rt_unet_forward: batch");
        if (e->n_prompts <= 0)
            throw rt_error(RT_E_INVALID, "rt_unet_forward: call rt_set_prompts first (rt_bind_weight of a weight that rt_set_prompts reads - attn2.to_k / to_v, add_embedding.* - "
                                       "discards the prompts: their cached K / V and addition embeddings were derived from the old weight)");
        bool final_out = false;
        if (module) {
            RT_REQUIRE(trace_out, "rt_unet_forward_trace: trace_out is NULL");
            const rt_engine::TraceMod* tm = nullptr;
            for (const auto& m : e->trace_mods) if (m.name == module) tm = &m;
            if (!tm) throw rt_error(RT_E_INVALID, std::string("rt_unet_forward_trace: not a traceable module: ") + module);
            const long long need = (long long)B * tm->C * (h >> tm->shift) * (w >> tm->shift);
            if (trace_cap < need)
                throw rt_error(RT_E_INVALID, "rt_unet_forward_trace: trace_cap_floats " + std::to_string(trace_cap) + " < " + std::to_string(need) + " for " + module);
            final_out = tm->name == "conv_out";
        }
        struct TraceScope {      // the request lives for this forward only, also when it throws
            rt_engine* e;
            TraceScope(rt_engine* e_, const char* name, float* dst) : e(e_) { e->trace_name = name ? name : ""; e->trace_out = dst; }
            ~TraceScope() { e->trace_name.clear(); e->trace_out = nullptr; }
        } scope(e, module && !final_out ? module : nullptr, trace_out);
        FwdIn in{}; in.B = B; in.h = h; in.w = w; in.t = t; in.eps_out = e->eps;
        for (int b = 0; b < B; ++b) {
            in.x[b] = x + (size_t)b * 4 * h * w; in.scale[b] = in_scale ? in_scale[b] : 1.f;
            in.prompt[b] = prompt ? prompt[b] : 0; in.fontsize[b] = fontsize ? fontsize[b] : 0;
            in.qk_src[b] = qk_src ? qk_src[b] : b; in.res_src[b] = res_src ? res_src[b] : -1;
            in.perturb[b] = perturb && perturb[b] ? 1 : 0;
            RT_REQUIRE(in.prompt[b] >= 0 && in.prompt[b] < e->n_prompts, "rt_unet_forward: prompt index");
            RT_REQUIRE(in.qk_src[b] >= 0 && in.qk_src[b] < B && in.res_src[b] < B, "rt_unet_forward: source stream index");
        }
        e->unet_forward(in);
        launch_nhwc4_to_nchw(e->eps, out, B, h * w, e->stream);
        if (final_out) launch_nhwc4_to_nchw(e->eps, trace_out, B, h * w, e->stream);      // conv_out's tensor is `out` itself
    }
}
int rt_unet_forward(rt_engine* e, const float* x, int B, int h, int w, float t, const float* in_scale, const int* prompt,
                    const int* fontsize, const int* qk_src, const int* res_src, float* out) {
    RT_TRY(e, { unet_forward_entry(e, x, B, h, w, t, in_scale, prompt, fontsize, qk_src, res_src, out, nullptr, nullptr, 0); })
}
int rt_unet_forward_trace(rt_engine* e, const float* x, int B, int h, int w, float t, const float* in_scale, const int* prompt, const int* fontsize,
                          const int* qk_src, const int* res_src, float* out, const char* module_name, float* trace_out_dev, long long trace_cap_floats) {
    RT_TRY(e, {
        RT_REQUIRE(module_name, "rt_unet_forward_trace: module_name is NULL");
        unet_forward_entry(e, x, B, h, w, t, in_scale, prompt, fontsize, qk_src, res_src, out, module_name, trace_out_dev, trace_cap_floats);
    })
}
int rt_unet_forward_perturbed(rt_engine* e, const float* x, int B, int h, int w, float t, const float* in_scale, const int* prompt, const int* fontsize,
                              const int* qk_src, const int* res_src, float* out, const char* module_name, float* trace_out_dev, long long trace_cap_floats,
                              const int* perturb_host) {
    RT_TRY(e, { unet_forward_entry(e, x, B, h, w, t, in_scale, prompt, fontsize, qk_src, res_src, out, module_name, trace_out_dev, trace_cap_floats, perturb_host); })
}
int rt_trace_module_count(rt_engine* e) { return (int)e->trace_mods.size(); }
int rt_trace_module_info(rt_engine* e, int idx, char* name, int cap, int* channels, int* downshift) {
    RT_TRY(e, {
        RT_REQUIRE(idx >= 0 && idx < (int)e->trace_mods.size(), "rt_trace_module_info: index");
        const auto& m = e->trace_mods[idx];
        RT_REQUIRE(name && (int)m.name.size() < cap, "rt_trace_module_info: name buffer too small");
        std::strcpy(name, m.name.c_str());
        if (channels) *channels = m.C;
        if (downshift) *downshift = m.shift;
    })
}

int rt_attn_store_enable(rt_engine* e, const char* name, int mode) {
    RT_TRY(e, { need_device(e); RT_REQUIRE(mode >= 0 && mode <= 2, "rt_attn_store_enable: mode"); e->attn_store_enable(name, mode); })
}
int rt_attn_store_reset(rt_engine* e) { RT_TRY(e, { need_device(e); e->attn_store_reset(); }) }
int rt_attn_store_read(rt_engine* e, const char* name, float* dst, int* n_calls, int* rows, int* cols) {
    RT_TRY(e, {
        need_device(e);
        bool found = false;
        e->for_each_tblock([&](TransformerP&, TBlockP& k) {
            for (int w = 0; w < 2; ++w) {
                if (k.mod_name[w] != name) continue;
                found = true;
                *n_calls = k.store_calls[w]; *rows = k.store_rows[w]; *cols = k.store_cols[w];
                if (dst && k.store[w] && k.store_rows[w] > 0)
                    HIP_CHECK(hipMemcpyAsync(dst, k.store[w], (size_t)k.store_rows[w] * k.store_cols[w] * 4, hipMemcpyDeviceToDevice, e->stream));
            }
        });
        if (!found) throw rt_error(RT_E_INVALID, std::string("attention store: unknown attention module ") + name);
        HIP_CHECK(hipStreamSynchronize(e->stream));
    })
}
int rt_attn_module_count(rt_engine* e) { int n = 0; e->for_each_tblock([&](TransformerP&, TBlockP&) { n += 2; }); return n; }
int rt_attn_module_info(rt_engine* e, int idx, char* name, int cap, int* max_tokens, int* heads) {
    RT_TRY(e, {
        int i = 0; bool found = false;
        e->for_each_tblock([&](TransformerP& t, TBlockP& k) {
            for (int w = 0; w < 2; ++w, ++i) {
                if (i != idx) continue;
                found = true;
                RT_REQUIRE((int)k.mod_name[w].size() < cap, "rt_attn_module_info: name buffer too small");
                std::strcpy(name, k.mod_name[w].c_str());
                *max_tokens = (e->cfg.latent_h >> t.level) * (e->cfg.latent_w >> t.level);
                *heads = t.heads;
            }
        });
        RT_REQUIRE(found, "rt_attn_module_info: index");
    })
}

int rt_profile_enable(rt_engine* e, int on) {
    RT_TRY(e, {
        need_device(e);
        for (auto& r : e->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        e->prof.clear();
        e->profiling = on != 0;
    })
}
int rt_profile_read(rt_engine* e, int cls, int* count, double* total_ms, double* total_flops) {
    RT_TRY(e, {
        need_device(e);
        HIP_CHECK(hipStreamSynchronize(e->stream));
        int n = 0; double ms = 0, fl = 0;
        for (auto& r : e->prof) if (r.cls == cls) {
            float t = 0; HIP_CHECK(hipEventElapsedTime(&t, r.a, r.b));
            ++n; ms += t; fl += r.flops;
        }
        *count = n; *total_ms = ms; *total_flops = fl;
    })
}
int rt_profile_read2(rt_engine* e, int cls, int* count, double* total_ms, double* total_flops, double* total_bytes) {
    const int rc = rt_profile_read(e, cls, count, total_ms, total_flops);
    if (rc != RT_OK) return rc;
    double by = 0;
    for (auto& r : e->prof) if (r.cls == cls) by += r.bytes;
    *total_bytes = by;
    return RT_OK;
}

// ---- operator-level entry points (stateless; share one lazily allocated zero page per device) ----
static bf16_t* op_zero_page() {       // one page per DEVICE (a thread that drives two GPUs must not hand device-0 memory to device-1 kernels)
    static std::mutex mu;
    static std::map<int, bf16_t*> pages;
    int dev = 0; HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    bf16_t*& z = pages[dev];
    if (!z) { HIP_CHECK(hipMalloc((void**)&z, 256)); HIP_CHECK(hipMemset(z, 0, 256)); }
    return z;
}
// a caller's packed [N, K] weight (+ bias) as the plan's MatW, for the builders above (read only)
static MatW op_mat(const void* w, const float* b, int N, int K) { MatW m; m.w = (bf16_t*)w; m.b = (float*)b; m.N = N; m.K = K; return m; }
static bool op_key_count_ok(int c, int NK) { return c >= 77 && c % 77 == 0 && c / 77 * 96 <= NK; }
// statistics scratch of rt_op_attention_probs_avg: one buffer per (device, stream), grown on demand (never under capture: null then,
// which selects the one-pass kernel)
static float* op_store_stats(size_t floats, hipStream_t st) {
    struct Buf { float* p = nullptr; size_t n = 0; };
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, Buf> bufs;
    int dev = 0; HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    Buf& b = bufs[std::make_pair(dev, st)];
    if (floats > b.n) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cap);
        if (cap != hipStreamCaptureStatusNone) return nullptr;
        HIP_CHECK(hipStreamSynchronize(st));
        if (b.p) (void)hipFree(b.p);
        b.p = nullptr; b.n = 0;
        HIP_CHECK(hipMalloc((void**)&b.p, floats * 4));
        b.n = floats;
    }
    return b.p;
}
#define OP_TRY(...)                                                          \
    try { __VA_ARGS__; return RT_OK; }                                              \
    catch (const rt_error& ex) { g_op_error = ex.what(); return ex.code; }   \
    catch (const std::exception& ex) { g_op_error = ex.what(); return RT_E_INVALID; }

const char* rt_op_last_error(void) { return g_op_error.c_str(); }
// the stream ranges of the intra-image split (step_driver.inl) as a host-only query
int rt_op_split_range(int n_streams, int text_ref_stream, int inject, int part, int nparts, int* first, int* count) {
    OP_TRY({ RT_REQUIRE(first && count, "rt_op_split_range: null outputs"); region_split_range(n_streams, text_ref_stream, inject != 0, part, nparts, first, count); })
}
extern int g_store_legacy;
extern int g_store_apply_v1;
extern int g_c77_t1;
// host-only (no GPU): which streams of a self-attention launch share one softmax (csrc/attention.hip, launch_attention_units)
int rt_op_attention_units_plan(const int* q_src, const int* k_src, int B, int tokens, int DP, int mode, int* launch_of, int* unit_of, int* members_of) {
    if (!q_src || !k_src || !launch_of || !unit_of || !members_of || B < 1 || B > RT_MAXB) return -1;
    return attention_units_plan_host(q_src, k_src, B, tokens, DP, mode, launch_of, unit_of, members_of);
}
int rt_op_gemm_debug(int d) {
    auto on = [d](int bit) { return debug_bit(d, bit); };
    gemm_set_debug(d);
    g_store_legacy = on(DBG_STORE_TWO_PASS) | on(DBG_STORE_ONE_PASS) << 1; g_store_own_stats = on(DBG_STORE_OWN_STATS); g_store_apply_v1 = on(DBG_STORE_APPLY_V1);
    g_c77_t1 = on(DBG_C77_ONE_TILE) | on(DBG_C77_TWO_HEADS) << 1;
    attention_set_prio(!on(DBG_ATTN_NO_PRIO)); attention_set_units((d >> DBG_ATTN_UNITS) & 7);
    gemm16_set_tall(on(DBG_G16_TALL)); gemm16_set_deep(!on(DBG_G16_NO_DEEP));
    groupnorm_set_fused(!on(DBG_GN_TWO_LAUNCH)); groupnorm_set_chunk_div(on(DBG_GN_CHUNK_128) ? 128 : 64);
    return RT_OK;
}
int rt_op_gemm_debug2(int d) { gemm_set_debug2(d); return RT_OK; }
int rt_op_probes_built(void) {
#ifdef RT_PROBES
    return 1;
#else
    return 0;
#endif
}
int rt_op_gemm_force_config(int cfg) {
    if (cfg < -1 || cfg > 8) return RT_E_INVALID;
    gemm_force_config(cfg);
    return RT_OK;
}

// The GemmArgs of an rt_op_gemm call: what the launch and the host-only route query (rt_op_gemm_route) both build, so that they cannot drift.
// `zero` is the zero page of the launch (the query, which touches no device, leaves it null: no routing rule reads a pointer's value here).
static GemmArgs op_gemm_args(const void* A, const void* W, const float* bias, void* out, const void* res, const float* temb, const bf16_t* zero, int mode,
                             int epi, int M, int N, int K, int lda, int ldw, int ldo, int ldres, int temb_ld, int rows_per_batch, int Hin,
                             int Win, int Cin, int Hout, int Wout) {
    GemmArgs g{}; g.A = (const bf16_t*)A; g.W = (const bf16_t*)W; g.bias = bias; g.out = out; g.res = res; g.temb = temb;
    g.zero = zero; g.mode = mode; g.epi = epi; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldo = ldo;
    g.ldres = ldres; g.temb_ld = temb_ld; g.rows_per_batch = rows_per_batch; g.Hin = Hin; g.Win = Win; g.Cin = Cin;
    g.Hout = Hout; g.Wout = Wout;
    return g;
}
int rt_op_gemm(const void* A, const void* W, const float* bias, void* out, const void* res, const float* temb, int mode,
               int epi, int M, int N, int K, int lda, int ldw, int ldo, int ldres, int temb_ld, int rows_per_batch, int Hin,
               int Win, int Cin, int Hout, int Wout, void* stream) {
    OP_TRY({
        const GemmArgs g = op_gemm_args(A, W, bias, out, res, temb, op_zero_page(), mode, epi, M, N, K, lda, ldw, ldo, ldres, temb_ld, rows_per_batch,
                                        Hin, Win, Cin, Hout, Wout);
        launch_gemm(g, (hipStream_t)stream);
    })
}
// GemmRoute -> RT_ROUTE_* (+ the tile variant / configuration of the kinds that have one)
static int op_route_kind(const GemmRoute& r, int* v) {
    *v = -1;
    switch (r.kind) {
        case GemmRoute::TILE: *v = r.cfg; return RT_ROUTE_TILE;
        case GemmRoute::G16: *v = r.variant; return RT_ROUTE_G16;
        case GemmRoute::G16_UP2: *v = r.variant; return RT_ROUTE_G16_UP2;
        case GemmRoute::PATCH: return RT_ROUTE_PATCH;
        case GemmRoute::PATCH_SPLIT: return RT_ROUTE_PATCH_SPLIT;
        case GemmRoute::KSPLIT: return RT_ROUTE_KSPLIT;
        case GemmRoute::TRIPLE: return RT_ROUTE_TRIPLE;
    }
    return RT_ROUTE_TILE;
}
// The route of that call as a host-only query (no device needed): gemm_route of the same GemmArgs, under the same switches.
int rt_op_gemm_route(int mode, int epi, int M, int N, int K, int lda, int ldw, int ldo, int rows_per_batch, int Hin, int Win, int Cin, int Hout,
                     int Wout, int* kind, int* variant_or_cfg, int* slices) {
    try {
        if (mode < A_DENSE || mode > A_CONV3_S2P0 || epi < EPI_BF16 || epi > EPI_F16 || M <= 0 || N <= 0 || K <= 0) return RT_E_INVALID;
        if (mode != A_DENSE && (rows_per_batch <= 0 || Cin <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0)) return RT_E_INVALID;
        const GemmArgs g = op_gemm_args(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, mode, epi, M, N, K, lda, ldw, ldo, 0, 0,
                                        rows_per_batch, Hin, Win, Cin, Hout, Wout);
        const GemmRoute r = gemm_route(g);
        int v = -1;
        const int k = op_route_kind(r, &v);
        if (kind) *kind = k;
        if (variant_or_cfg) *variant_or_cfg = v;
        if (slices) *slices = r.slices;
        return RT_OK;
    } catch (...) { return RT_E_INVALID; }
}
// ---- the VAE's contraction call (vae.hip gemm1 / conv1) behind the operator ABI: the GemmArgs come from the VAE's own builders (vae.h), so
// the entry takes exactly the routes rt_vae takes (prefer_patch_conv by conv1's rule, one image, fp32 output).  The launch and the
// host-only query build them through this one function.
static GemmArgs op_hilo_args(const void* A, const void* A_lo, const void* W, const void* W_lo, const float* bias, void* out, void* pair_lo, const float* res,
                             const bf16_t* zero, int mode, int M, int N, int K, int lda, int ldw, int ldo, int ldres, int rows_per_batch, int Hin, int Win,
                             int Cin, int Hout, int Wout) {
    RT_REQUIRE(mode == A_DENSE || mode == A_CONV3 || mode == A_CONV3_UP2 || mode == A_CONV3_S2P0, "rt_op_gemm_hilo: mode 0 dense / 1 conv / 3 up-2 conv / 4 stride-2-pad-0 conv");
    RT_REQUIRE(M > 0 && N > 0 && K > 0, "rt_op_gemm_hilo: empty problem");
    RT_REQUIRE((A_lo == nullptr) == (W_lo == nullptr), "rt_op_gemm_hilo: both low planes or neither");
    if (mode == A_DENSE) {
        RT_REQUIRE(!pair_lo, "rt_op_gemm_hilo: the pair output exists for convolutions only");
        return vae_gemm_args((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K, out, ldo, EPI_F32, res, ldres, (const bf16_t*)A_lo, (const bf16_t*)W_lo, zero);
    }
    RT_REQUIRE(Hin > 0 && Win > 0 && Cin > 0, "rt_op_gemm_hilo: empty image");
    const GemmArgs g = vae_conv_args((const bf16_t*)A, mode, (const bf16_t*)W, ldw, bias, N, K, Hin, Win, Cin, out, ldo, EPI_F32, res, ldres, (const bf16_t*)A_lo,
                                     (const bf16_t*)W_lo, (bf16_t*)pair_lo, zero);
    RT_REQUIRE(g.M == M && g.rows_per_batch == rows_per_batch && g.Hout == Hout && g.Wout == Wout, "rt_op_gemm_hilo: M, rows_per_batch, Hout, Wout must be those of ONE image in this mode");
    return g;
}
int rt_op_gemm_hilo(const void* A, const void* A_lo, const void* W, const void* W_lo, const float* bias, float* out_f32, void* pair_lo, const float* res,
                    int mode, int M, int N, int K, int lda, int ldw, int ldo, int ldres, int rows_per_batch, int Hin, int Win, int Cin, int Hout, int Wout,
                    void* stream) {
    OP_TRY({
        const GemmArgs g = op_hilo_args(A, A_lo, W, W_lo, bias, out_f32, pair_lo, res, op_zero_page(), mode, M, N, K, lda, ldw, ldo, ldres, rows_per_batch, Hin,
                                        Win, Cin, Hout, Wout);
        if (pair_lo && !gemm_pair_output_ok(g)) throw rt_error(RT_E_UNSUPPORTED, "rt_op_gemm_hilo: this problem's route cannot write the pair (rt_op_gemm_hilo_route)");
        launch_gemm(g, (hipStream_t)stream);
    })
}
int rt_op_gemm_hilo_route(int hilo, int pair, int mode, int M, int N, int K, int lda, int ldw, int ldo, int rows_per_batch, int Hin, int Win, int Cin, int Hout,
                          int Wout, int* kind, int* variant_or_cfg, int* slices, int* pass_kind, int* pair_ok) {
    try {
        const void* some = (const void*)(uintptr_t)256;              // (any non-null value: no routing rule reads a pointer's value)
        const GemmArgs g = op_hilo_args(nullptr, hilo ? some : nullptr, nullptr, hilo ? some : nullptr, nullptr, nullptr, pair ? (void*)some : nullptr, nullptr, nullptr,
                                        mode, M, N, K, lda, ldw, ldo, 0, rows_per_batch, Hin, Win, Cin, Hout, Wout);
        const GemmRoute r = gemm_route(g);
        // TRIPLE = three launches of the single-pass problem (launch_routed): the route each of them takes
        GemmRoute rp = r;
        if (r.kind == GemmRoute::TRIPLE) { GemmArgs b = g; b.A_lo = nullptr; b.W_lo = nullptr; rp = gemm_route(b); }
        int v = -1;
        const int k = op_route_kind(r, &v), pk = op_route_kind(rp, &v);
        if (kind) *kind = k;
        if (variant_or_cfg) *variant_or_cfg = v;
        if (slices) *slices = rp.slices;
        if (pass_kind) *pass_kind = pk;
        if (pair_ok) *pair_ok = gemm_pair_output_ok(g) ? 1 : 0;
        return RT_OK;
    } catch (...) { return RT_E_INVALID; }
}
int rt_op_split_bf16(const float* x, void* hi_bf16, void* lo_bf16, long long n, void* stream) {
    OP_TRY({ RT_REQUIRE(x && hi_bf16 && lo_bf16 && n > 0, "rt_op_split_bf16: null argument or empty"); launch_cast_f32_bf16(x, (bf16_t*)hi_bf16, (size_t)n, (hipStream_t)stream, (bf16_t*)lo_bf16); })
}
int rt_op_pack_upconv(const void* w, int dtype, int Cout, int Cin, void* out_bf16, void* stream) {
    OP_TRY({ launch_pack_up2(w, dtype, (bf16_t*)out_bf16, Cout, Cin, (hipStream_t)stream); })
}
int rt_op_upconv(const void* x, const void* w9, const void* w_phase, const float* bias, void* out_f16, int B, int Hin, int Win, int Cin, int N,
                 int* phase_route, void* stream) {
    OP_TRY({
        MatW W = op_mat(w9, bias, N, 9 * Cin); W.w_up2 = (bf16_t*)w_phase;
        GemmArgs g = unet_conv3_args(op_zero_page(), (const bf16_t*)x, A_CONV3_UP2, W, B, Hin, Win, Cin, out_f16, EPI_F16);
        g.split_tiles = 0;      // this entry has never passed one stream's tile count: the split rule sees the B images' actual tiles
        if (phase_route) *phase_route = gemm_route(g).kind == GemmRoute::G16_UP2 ? 1 : 0;
        launch_gemm(g, (hipStream_t)stream);
    })
}
int rt_op_ln_partials(const void* x_f16, void* xb_bf16, float* partials, int rows, int C, int tile_cols, void* stream) {
    OP_TRY({ launch_ln_partials((const f16_t*)x_f16, (bf16_t*)xb_bf16, partials, rows, C, tile_cols, (hipStream_t)stream); })
}
int rt_op_gemm_emit_partials(const void* A, const void* W, const float* bias, void* out_f16, const void* res_f16, int M, int N, int K,
                             int rows_per_stream, void* xb_bf16, float* partials, int* tile_cols, void* stream) {
    OP_TRY({
        GemmArgs g = unet_dense_args(op_zero_page(), rows_per_stream, (const bf16_t*)A, K, op_mat(W, bias, N, K), M, out_f16, N, EPI_F16, res_f16, N);
        const int bn = gemm_ln_emit_bn(g);
        if (!bn) throw rt_error(RT_E_UNSUPPORTED, "rt_op_gemm_emit_partials: this shape's route has no partial-emitting epilogue");
        if (tile_cols) *tile_cols = bn;
        g.ln_emit = partials; g.ln_copy = (bf16_t*)xb_bf16;
        launch_gemm(g, (hipStream_t)stream);
    })
}
int rt_op_ln_gemm(const void* x_f16, const float* gamma, const float* beta, const void* W_bf16, const float* bias, void* out, int tokens,
                  int N, int C, int epi, int weights_on_rows, int rows_per_stream, const void* xb_bf16, const float* partials, int tile_cols, void* stream) {
    OP_TRY({
        RT_REQUIRE((C == 640 || C == 1280) && tokens > 0 && N > 0 && (epi == EPI_BF16 || epi == EPI_GEGLU) && !(weights_on_rows && epi != EPI_BF16), "rt_op_ln_gemm: shape");
        RT_REQUIRE((xb_bf16 != nullptr) == (partials != nullptr) && (xb_bf16 || x_f16), "rt_op_ln_gemm: a producer's (xb, partials) pair, or the fp16 trunk");
        RT_REQUIRE((tile_cols == 160 || tile_cols == 320) && C % (2 * tile_cols) == 0, "rt_op_ln_gemm: column tiles of 160 / 320, an even number per row");
        hipStream_t st = (hipStream_t)stream;
        const MatW Wn = op_mat(nullptr, nullptr, N, C);
        GemmArgs g = weights_on_rows ? unet_vt_args(op_zero_page(), rows_per_stream, Wn, nullptr, C, tokens, (bf16_t*)out, tokens)
                                     : unet_dense_args(op_zero_page(), rows_per_stream, nullptr, C, Wn, tokens, out, epi == EPI_GEGLU ? N / 2 : N, epi);
        LnFold ln; ln.npair = C / tile_cols / 2; ln.ld = tokens;
        ln_apply(g, &ln, C);
        if (!gemm_ln_fold_ok(g)) throw rt_error(RT_E_UNSUPPORTED, "rt_op_ln_gemm: this shape's route has no folded instantiation");
        // scratch of the op (the engine keeps these in its own arenas): W', (s, c), xb, partials
        bf16_t* Wf = nullptr; float* sc = nullptr; float* part = nullptr; bf16_t* xb = nullptr;
        HIP_CHECK(hipMalloc((void**)&Wf, (size_t)N * C * 2));
        HIP_CHECK(hipMalloc((void**)&sc, (size_t)N * 8));
        try {
            launch_ln_fold_derive((const bf16_t*)W_bf16, C, bias, gamma, beta, N, C, Wf, sc, st);
            if (!partials) {
                HIP_CHECK(hipMalloc((void**)&part, (size_t)tokens * 16 * 4));
                HIP_CHECK(hipMalloc((void**)&xb, (size_t)tokens * C * 2));
                launch_ln_partials((const f16_t*)x_f16, xb, part, tokens, C, tile_cols, st);
            }
            const bf16_t* xop = partials ? (const bf16_t*)xb_bf16 : xb;
            g.ln_part = partials ? partials : part; g.ln_s = sc; g.bias = nullptr;
            if (weights_on_rows) { g.A = Wf; g.W = xop; } else { g.A = xop; g.W = Wf; }
            launch_gemm(g, st);
            HIP_CHECK(hipStreamSynchronize(st));
        } catch (...) { (void)hipFree(Wf); (void)hipFree(sc); (void)hipFree(part); (void)hipFree(xb); throw; }
        (void)hipFree(Wf); (void)hipFree(sc); (void)hipFree(part); (void)hipFree(xb);
    })
}
int rt_op_attention(const void* Q, int ldq, const void* K, int ldk, const void* VT, int ldvt, void* O, int ldo, const int* q_src,
                    const int* k_src, const int* v_src, const int* wset, const float* wabs, const float* wsgn, int B, int H,
                    int N, int NK, int nk_valid, int DP, int cross, void* stream) {
    OP_TRY({
        RT_REQUIRE(B >= 1 && B <= RT_MAXB, "rt_op_attention: batch");
        AttnArgs a{}; a.Q = (const bf16_t*)Q; a.ldq = ldq; a.K = (const bf16_t*)K; a.ldk = ldk; a.VT = (const bf16_t*)VT; a.ldvt = ldvt;
        a.O = (bf16_t*)O; a.ldo = ldo; a.wabs = wabs; a.wsgn = wsgn;
        for (int b = 0; b < B; ++b) { a.q_src[b] = q_src ? q_src[b] : b; a.k_src[b] = k_src ? k_src[b] : b; a.v_src[b] = v_src ? v_src[b] : b; a.wset[b] = wset ? wset[b] : 0; }
        a.B = B; a.H = H; a.N = N; a.NK = NK; a.nk_valid = nk_valid; a.DP = DP; a.cross = cross;
        // the engine's route where the launch is one of its 77-key ones (K and V of one prompt, at most the 80 keys cross77_kernel reads; this
        // entry is handed Q and knows DP only), attn_kernel for everything else
        bool as77 = cross && nk_valid >= 1 && nk_valid <= 80;
        int k77[RT_MAXB];
        for (int b = 0; b < B; ++b) { as77 = as77 && a.k_src[b] == a.v_src[b]; k77[b] = 77; }
        launch_cross(a, as77 ? cross_route(H * DP, H, DP, DP, N, NK, k77, B, false, false, false) : CrossRoute{CrossRoute::GENERIC, false}, (hipStream_t)stream);
    })
}
int rt_op_ip_attention(const void* Q, int ldq, const void* Kip, int ldk, const void* VTip, int ldvt, void* O, int ldo, const int* slot_host,
                       const int* count_host, const float* scale_host, int B, int H, int N, int DP, void* stream) {
    OP_TRY({
        RT_REQUIRE(Q && Kip && VTip && O && slot_host && count_host && scale_host, "rt_op_ip_attention: null argument");
        launch_ip_attention((const bf16_t*)Q, ldq, (const bf16_t*)Kip, ldk, (const bf16_t*)VTip, ldvt, (bf16_t*)O, ldo, slot_host, count_host, scale_host,
                            B, H, N, DP, (hipStream_t)stream);
    })
}
int rt_op_attention_keys(const void* Q, int ldq, const void* K, int ldk, const void* VT, int ldvt, void* O, int ldo, const int* q_src,
                         const int* prompt, const int* wset, const float* wabs, const float* wsgn, const int* key_counts, int B, int H,
                         int N, int NK, int DP, void* stream) {
    OP_TRY({
        RT_REQUIRE(B >= 1 && B <= RT_MAXB && key_counts, "rt_op_attention_keys: batch / key counts");
        RT_REQUIRE(NK == 96 || NK == 192 || NK == 288, "rt_op_attention_keys: NK must be 96, 192 or 288 rows per prompt");
        int p[RT_MAXB], ws[RT_MAXB];
        for (int b = 0; b < B; ++b) {
            RT_REQUIRE(op_key_count_ok(key_counts[b], NK), "rt_op_attention_keys: a key count must be 77 per 96-row chunk of NK");
            p[b] = prompt ? prompt[b] : b; ws[b] = wset ? wset[b] : -1;
        }
        RT_REQUIRE(!q_src, "rt_op_attention_keys: cross launches read Q of their own batch entry (q_src must be NULL)");
        // the engine's launch and route (this entry is handed Q and knows DP only)
        launch_cross(unet_cross_attn_args(AttnIO{(const bf16_t*)Q, ldq, (const bf16_t*)K, ldk, (const bf16_t*)VT, ldvt, (bf16_t*)O, ldo}, p, ws, key_counts, wabs, wsgn,
                                          B, H, N, NK, DP),
                     cross_route(H * DP, H, DP, DP, N, NK, key_counts, B, false, false, false), (hipStream_t)stream);
    })
}
// The arguments of a host-only shape query as the engine launches them: `streams` streams / images of rows_per_stream rows each
// (3x3 convolution modes: a square map of rows_per_stream OUTPUT pixels - of even side for the 2x up-sampler - and K_or_Cin input channels,
// else false); N = the weight rows.  No pointer is set: no routing rule reads a pointer's value.
static bool query_args(GemmArgs& g, int mode, int epi, int streams, int rows_per_stream, int N, int K_or_Cin, int weights_on_rows) {
    const int M = streams * rows_per_stream;
    if (mode != A_DENSE) {
        int side = 1; while (side * side < rows_per_stream) ++side;
        if (side * side != rows_per_stream || (mode == A_CONV3_UP2 && side % 2)) return false;
        const int in = mode == A_CONV3_UP2 ? side / 2 : side;
        g = unet_conv3_args(nullptr, nullptr, mode, op_mat(nullptr, nullptr, N, 9 * K_or_Cin), streams, in, in, K_or_Cin, nullptr, epi);
        g.weights_on_rows = weights_on_rows;
    } else if (weights_on_rows) {
        g = unet_vt_args(nullptr, rows_per_stream, op_mat(nullptr, nullptr, N, K_or_Cin), nullptr, K_or_Cin, M, nullptr, M);
        g.epi = epi;
    } else g = unet_dense_args(nullptr, rows_per_stream, nullptr, K_or_Cin, op_mat(nullptr, nullptr, N, K_or_Cin), M, nullptr, N, epi);
    return true;
}
// The route launch_gemm takes for problems that cannot fill the chip (gemm_route) as a host-only query (no device needed).
int rt_op_split_plan(int conv3x3, int epi, int streams, int rows_per_stream, int N, int K_or_Cin, int* route, int* slices) {
    try {
        GemmArgs g;
        if (!query_args(g, conv3x3 == 3 ? A_CONV3_UP2 : conv3x3 ? A_CONV3 : A_DENSE, epi, streams, rows_per_stream, N, K_or_Cin, 0)) return RT_E_INVALID;
        const GemmRoute r = gemm_route(g);
        const int kind = r.kind == GemmRoute::KSPLIT ? 1 : r.kind == GemmRoute::PATCH_SPLIT ? 2 : 0;
        if (route) *route = kind;
        if (slices) *slices = kind ? r.slices : 1;
        return RT_OK;
    } catch (...) { return RT_E_INVALID; }
}
// The shape rule of csrc/gemm16.hip as a host-only query (no device needed): which tile variant a problem takes (-1: stays on gemm.hip /
// the patch convolution) and whether it uses the W-stationary tile -> XCD order.  `streams` images / streams of rows_per_stream rows each.
int rt_op_gemm16_pick(int conv3x3, int epi, int streams, int rows_per_stream, int N, int K_or_Cin, int weights_on_rows, int* w_stationary) {
    try {
        GemmArgs g;
        if (!query_args(g, conv3x3 ? A_CONV3 : A_DENSE, epi, streams, rows_per_stream, N, K_or_Cin, weights_on_rows)) return -2;     // square maps only
        int ws = 0;
        const int v = gemm16_pick(g, weights_on_rows, &ws);
        if (w_stationary) *w_stationary = ws;
        return v;
    } catch (...) { return -3; }
}
// One tile variant of the 16x16x32 family (csrc/gemm16.hip) on a dense problem - tests and micro-benchmarks; rt_op_gemm picks by shape.
int rt_op_gemm16_variant(const void* A, const void* W, const float* bias, void* out, const void* res, int epi, int M, int N, int K, int lda,
                         int ldw, int ldo, int ldres, int weights_on_rows, int variant, int wstat, void* stream) {
    OP_TRY({
        GemmArgs g = unet_dense_args(op_zero_page(), 0, (const bf16_t*)A, lda, op_mat(W, bias, N, K), M, out, ldo, epi, res, ldres);
        g.ldw = ldw; g.weights_on_rows = weights_on_rows;       // the caller's operands as they are (V^T form: A = the weight rows)
        if (variant < 0) { int ws = 0; variant = gemm16_pick(g, weights_on_rows, &ws); wstat = ws; RT_REQUIRE(variant >= 0, "rt_op_gemm16_variant: the family has no tile for this shape"); }
        launch_gemm16_variant(g, variant, wstat, (hipStream_t)stream);
    })
}
// Host-only query of the grouped-launch rule (tests): which grouped instantiation attn1's two projections take for `streams_qk` / `streams`
// streams of `rows_per_stream` tokens - 0: 224x320 + 160x224, 1: 224x256 + 160x224, 2: 128x256 + 160x64, 3: 224x256 + 160x128 (Q|K tile +
// V^T tile) - or -1: two launches.
int rt_op_gemm_pair_pick(int streams_qk, int streams, int rows_per_stream, int Nqk, int Nv, int K) {
    try {
        GemmArgs a, b;
        query_args(a, A_DENSE, EPI_BF16, streams_qk, rows_per_stream, Nqk, K, 0);
        query_args(b, A_DENSE, EPI_BF16, streams, rows_per_stream, Nv, K, 1);
        return gemm_pair_grouped(a, b);
    } catch (...) { return -3; }
}
// attn1's two projections of one LayerNorm output X [M, K] as the engine launches them (launch_gemm_pair): qk[Mqk, Nqk] = X[:Mqk] Wqk^T + bqk
// and vt[Nv, M] = Wv X^T.  *grouped = 1 when they went out as ONE grouped launch (gemm16_dual_kernel), 0 when as two launches.
int rt_op_gemm_qk_vt(const void* X, int ldx, int K, int rows_per_stream, const void* Wqk, const float* bqk, int Mqk, int Nqk, void* qk, int ldqk,
                     const void* Wv, int Nv, int M, void* vt, int ldvt, int* grouped, void* stream) {
    OP_TRY({
        const GemmArgs a = unet_dense_args(op_zero_page(), rows_per_stream, (const bf16_t*)X, ldx, op_mat(Wqk, bqk, Nqk, K), Mqk, qk, ldqk, EPI_BF16);
        const GemmArgs b = unet_vt_args(a.zero, rows_per_stream, op_mat(Wv, nullptr, Nv, K), (const bf16_t*)X, ldx, M, (bf16_t*)vt, ldvt);     // (no V bias in this entry)
        if (grouped) *grouped = gemm_pair_grouped(a, b) >= 0 ? 1 : 0;
        launch_gemm_pair(a, b, (hipStream_t)stream);
    })
}
// The block BASELINE.json's north star names: attn2 of a BasicTransformerBlock (models/attention.py:169-189) with the reference
// processor's arithmetic (models/attention_processor.py:476-545; font-size softmax :386-401) as ONE call:
//   trunk_out = trunk_in + to_out( softmax_fs( to_q(x) K[prompt]^T ) V[prompt] ) + b_out
// K / V^T come from the per-prompt cache (77 keys padded to 96; step invariant), Q and O live in caller-provided scratch.  Three
// launches (to_q GEMM, 96-key attention, to_out GEMM + fp16 residual): why the fused form is not faster is measured in LABNOTES.md R4.1 / 4.8.
int rt_op_cross_attn_block(const void* x, const void* wq, const void* wo, const float* bo, const void* kcache, const void* vtcache, int ldvt,
                           const int* prompt_host, const int* wset_host, const float* wabs, const float* wsgn, const void* trunk_in,
                           void* trunk_out, void* q_scratch, void* o_scratch, int B, int N, int C, int H, int DP, void* stream) {
    OP_TRY({
        RT_REQUIRE(B >= 1 && B <= RT_MAXB && N > 0 && C % 8 == 0 && H > 0 && DP % 32 == 0, "rt_op_cross_attn_block: shape");
        hipStream_t st = (hipStream_t)stream;
        const int M = B * N, HD = H * DP;
        const bf16_t* zero = op_zero_page();
        int prompt[RT_MAXB], wset[RT_MAXB], k77[RT_MAXB];
        for (int b = 0; b < B; ++b) { prompt[b] = prompt_host ? prompt_host[b] : 0; wset[b] = wset_host ? wset_host[b] : 0; k77[b] = 77; }
        // the engine's route for a layer of this shape with 77-key prompts in a 96-row cache, LayerNorm not folded, map not recorded
        const CrossRoute route = cross_route(C, H, DP, DP, N, 96, k77, B, false, false);
        if (route.kind == CrossRoute::XBLOCK) {                // the whole block in one launch (neither scratch buffer is written)
            launch_xblock(unet_xblock_args((const bf16_t*)x, (const bf16_t*)wq, (const bf16_t*)wo, bo, (const bf16_t*)kcache, (const bf16_t*)vtcache, ldvt,
                                           (const f16_t*)trunk_in, (f16_t*)trunk_out, wabs, wsgn, prompt, wset, B, N, C, H), st);
        } else if (route.kind == CrossRoute::XATTN_FUSED) {    // to_q + attention in one launch (Q stays in LDS; q_scratch is not written)
            launch_xattn_fused(unet_xattn_args(zero, (const bf16_t*)x, (const bf16_t*)wq, (bf16_t*)o_scratch, (const bf16_t*)kcache, (const bf16_t*)vtcache, ldvt,
                                               wabs, wsgn, prompt, wset, B, N, C, H), st);
        } else {
            launch_gemm(unet_dense_args(zero, N, (const bf16_t*)x, C, op_mat(wq, nullptr, HD, C), M, q_scratch, HD, EPI_BF16), st);
            launch_cross(unet_cross_attn_args(AttnIO{(const bf16_t*)q_scratch, HD, (const bf16_t*)kcache, HD, (const bf16_t*)vtcache, ldvt, (bf16_t*)o_scratch, HD},
                                              prompt, wset, k77, wabs, wsgn, B, H, N, 96, DP), route, st);
        }
        if (route.kind != CrossRoute::XBLOCK) launch_gemm(unet_dense_args(zero, N, (const bf16_t*)o_scratch, HD, op_mat(wo, bo, C, HD), M, trunk_out, C, EPI_F16, trunk_in, C), st);
    })
}
int rt_op_groupnorm(const void* x1, const void* x2, int in_bf16, int C1, int C2, int G, int B, int HW, const float* gamma,
                    const float* beta, float eps, int silu, void* out, void* raw, void* stream) {
    OP_TRY({
        float* partial = nullptr;
        HIP_CHECK(hipMalloc((void**)&partial, (size_t)B * groupnorm_nchunk(HW) * G * 2 * 4));
        launch_groupnorm(unet_gn_args(x1, x2, in_bf16, C1, C2, G, B, HW, gamma, beta, eps, silu, (bf16_t*)out, (bf16_t*)raw, partial), (hipStream_t)stream);
        HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        HIP_CHECK(hipFree(partial));
    })
}
// Host-only: the form launch_groupnorm takes for that call (the predicate of the launcher itself; rt_op_gemm_debug bit 23 counts).
int rt_op_groupnorm_form(int in_type, int C1, int C2, int G, int B, int HW) {
    if (in_type < 0 || in_type > 2 || C1 <= 0 || C2 < 0 || G < 1 || (C1 + C2) % G || B < 1 || HW < 1) return RT_E_INVALID;
    return groupnorm_form(unet_gn_args(nullptr, nullptr, in_type, C1, C2, G, B, HW, nullptr, nullptr, 0.f, 0, nullptr, nullptr, nullptr));
}
// ---- the VAE's kernels beyond the contractions (vae_kernels.hip; GroupNorm forward with the low planes: norm.hip), one call each, with the
// launch arguments of vae.h
int rt_op_vae_groupnorm_nchunk(int HW) { return HW < 1 ? RT_E_INVALID : vae_gn_nchunk(HW); }
int rt_op_vae_groupnorm(const void* x, int x_bf16, int C, int G, int B, int HW, const float* gamma, const float* beta, float eps, int silu, void* out,
                        void* out_lo, void* raw, void* raw_lo, float* stats, void* stream) {
    OP_TRY({
        RT_REQUIRE(x && out && stats && gamma && beta && (x_bf16 == 0 || x_bf16 == 1) && C > 0 && B >= 1 && HW >= 1, "rt_op_vae_groupnorm: bad argument");
        RT_REQUIRE(!raw_lo || raw, "rt_op_vae_groupnorm: raw_lo without raw");
        launch_groupnorm(vae_gn_fwd_args(x, x_bf16 != 0, C, G, B, HW, gamma, beta, eps, silu != 0, (bf16_t*)out, (bf16_t*)out_lo, (bf16_t*)raw, (bf16_t*)raw_lo, stats),
                         (hipStream_t)stream);
    })
}
int rt_op_vae_groupnorm_bwd(const void* x, int x_bf16, const void* dA, const void* dA_lo, const float* stats, const float* gamma, const float* beta, float eps,
                            int silu, int C, int G, int B, int HW, const float* add, float* out, void* out_bf16, void* out_bf16_lo, void* stream) {
    OP_TRY({
        RT_REQUIRE(x && dA && stats && gamma && beta && (x_bf16 == 0 || x_bf16 == 1) && C > 0 && G >= 1 && B >= 1 && HW >= 1, "rt_op_vae_groupnorm_bwd: bad argument");
        RT_REQUIRE(!out_bf16_lo || out_bf16, "rt_op_vae_groupnorm_bwd: out_bf16_lo without out_bf16");
        float* bp = nullptr;
        HIP_CHECK(hipMalloc((void**)&bp, (size_t)B * vae_gn_nchunk(HW) * G * 2 * 4));
        try {
            launch_groupnorm_bwd(vae_gn_bwd_args(x, x_bf16 != 0, (const bf16_t*)dA, (const bf16_t*)dA_lo, stats, bp, C, G, B, HW, gamma, beta, eps, silu != 0, add, out,
                                                 (bf16_t*)out_bf16, (bf16_t*)out_bf16_lo), (hipStream_t)stream);
            HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        } catch (...) { (void)hipFree(bp); throw; }
        HIP_CHECK(hipFree(bp));
    })
}
int rt_op_softmax_rows(const float* s, void* p, void* p_lo, int rows, int cols, float scale, void* stream) {
    OP_TRY({ RT_REQUIRE(s && p && rows >= 1 && cols >= 1, "rt_op_softmax_rows: bad argument"); launch_softmax_rows(s, (bf16_t*)p, rows, cols, scale, (hipStream_t)stream, (bf16_t*)p_lo); })
}
int rt_op_softmax_bwd(const void* p, const void* p_lo, const float* dp, void* ds, void* ds_lo, int rows, int cols, float scale, void* stream) {
    OP_TRY({
        RT_REQUIRE(p && dp && ds && rows >= 1 && cols >= 1, "rt_op_softmax_bwd: bad argument");
        launch_softmax_bwd((const bf16_t*)p, dp, (bf16_t*)ds, rows, cols, scale, (hipStream_t)stream, (const bf16_t*)p_lo, (bf16_t*)ds_lo);
    })
}
int rt_op_transpose_bf16(const void* in, void* out, int R, int C, void* stream) {
    OP_TRY({ RT_REQUIRE(in && out && R >= 1 && C >= 1, "rt_op_transpose_bf16: bad argument"); launch_transpose_bf16((const bf16_t*)in, (bf16_t*)out, R, C, (hipStream_t)stream); })
}
int rt_op_sumpool2x2(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    OP_TRY({ RT_REQUIRE(in && out && B >= 1 && H >= 1 && W >= 1 && C >= 4, "rt_op_sumpool2x2: bad argument"); launch_sumpool2x2(in, out, B, H, W, C, (hipStream_t)stream); })
}
int rt_op_pq_conv_fwd(const float* lat, const float* eps, float c_lat, float c_eps, const float* W, const float* b, void* out, void* out_lo, int HW, void* stream) {
    OP_TRY({
        RT_REQUIRE(lat && W && b && out && HW >= 1, "rt_op_pq_conv_fwd: bad argument");
        launch_pq_conv_fwd(lat, eps, c_lat, c_eps, W, b, (bf16_t*)out, HW, (hipStream_t)stream, (bf16_t*)out_lo);
    })
}
int rt_op_pq_conv_bwd_update(const float* dz, int ldz, const float* W, float gscale, float weight, const float* mask_all, float* lat, float* grad_out, int HW,
                             void* stream) {
    OP_TRY({
        RT_REQUIRE(dz && W && mask_all && lat && ldz >= 4 && HW >= 1, "rt_op_pq_conv_bwd_update: bad argument");
        launch_pq_conv_bwd_update(dz, ldz, W, gscale, weight, mask_all, lat, grad_out, HW, (hipStream_t)stream);
    })
}
int rt_op_color_loss_grad(const float* img, int ldi, const float* masks, const float* target_dev, int n, int HWi, void* dimg, void* dimg_lo, float* loss_dev,
                          void* stream) {
    OP_TRY({
        RT_REQUIRE(img && masks && target_dev && dimg && ldi >= 3 && HWi >= 1 && n >= 1 && n <= RT_MAXB, "rt_op_color_loss_grad: bad argument");
        float* part = nullptr;
        HIP_CHECK(hipMalloc((void**)&part, vae_color_partial_floats(n) * 4));
        try {
            launch_color_loss_grad(vae_color_args(img, ldi, masks, target_dev, n, HWi, part, (bf16_t*)dimg, (bf16_t*)dimg_lo, loss_dev), (hipStream_t)stream);
            HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        } catch (...) { (void)hipFree(part); throw; }
        HIP_CHECK(hipFree(part));
    })
}
int rt_op_layernorm(const float* x, const float* gamma, const float* beta, void* out, int rows, int C, float eps, void* stream) {
    OP_TRY({ launch_layernorm(x, 0, gamma, beta, (bf16_t*)out, rows, C, eps, (hipStream_t)stream); })
}
int rt_op_layernorm_f16(const void* x_f16, const float* gamma, const float* beta, void* out, int rows, int C, float eps, void* stream) {
    OP_TRY({ launch_layernorm(x_f16, 1, gamma, beta, (bf16_t*)out, rows, C, eps, (hipStream_t)stream); })
}
int rt_op_small_linear(const float* a, int lda, const void* W, int ldw, const float* bias, float* out, int ldo, int B, int N,
                       int K, int silu_in, int accumulate, void* stream) {
    OP_TRY({ launch_small_linear(a, lda, (const bf16_t*)W, ldw, bias, out, ldo, B, N, K, silu_in, accumulate, (hipStream_t)stream); })
}
int rt_op_timestep_embed(const float* t, int n, int dim, float* out, int ldo, void* stream) {
    OP_TRY({ launch_timestep_embed(t, n, dim, out, ldo, (hipStream_t)stream); })
}
int rt_op_embed(const int* ids, const float* tok, const float* pos, float* out, int rows, int N, int C, int vocab, void* stream) {
    OP_TRY({ launch_embed(ids, tok, pos, out, rows, N, C, vocab, (hipStream_t)stream); })
}
int rt_op_activation(const void* x_bf16, void* out_bf16, long long n, int kind, void* stream) {
    OP_TRY({ launch_activation((const bf16_t*)x_bf16, (bf16_t*)out_bf16, (size_t)n, kind, (hipStream_t)stream); })
}
int rt_op_causal_attention(const void* q, const void* k, const void* v, int ld, void* out, int ldo, int B, int H, int N, int d, float scale,
                           void* stream) {
    OP_TRY({ launch_causal_attention((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, (bf16_t*)out, ldo, B, H, N, d, scale, (hipStream_t)stream); })
}
int rt_op_patchify(const void* img_u8, void* out_bf16, int B, int S, int p, int Kp, const float* mean_host, const float* std_host, void* stream) {
    OP_TRY({ launch_patchify((const uint8_t*)img_u8, (bf16_t*)out_bf16, B, S, p, Kp, mean_host, std_host, (hipStream_t)stream); })
}
int rt_op_vit_embed(const float* patch, int ldp, const float* cls, const float* pos, const float* gamma, const float* beta, float* out,
                    int B, int N, int C, float eps, void* stream) {
    OP_TRY({ launch_vit_embed(patch, ldp, cls, pos, gamma, beta, out, B, N, C, eps, (hipStream_t)stream); })
}
int rt_op_bidir_attention(const void* q, const void* k, const void* v, int ld, void* out, int ldo, int B, int H, int N, int d, float scale,
                          void* stream) {
    OP_TRY({ launch_bidir_attention((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, (bf16_t*)out, ldo, B, H, N, d, scale, (hipStream_t)stream); })
}
int rt_op_latent_attention(const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, int ldo, int B, int H, int Nq, int Nk, int d,
                           float scale, void* stream) {
    OP_TRY({ launch_latent_attention((const bf16_t*)q, ldq, (const bf16_t*)k, (const bf16_t*)v, ldkv, (bf16_t*)out, ldo, B, H, Nq, Nk, d, scale, (hipStream_t)stream); })
}
int rt_op_step_noise(unsigned long long seed, int step, int h, int w, float* out_dev, unsigned int* words_dev, void* stream) {
    OP_TRY({
        RT_REQUIRE(out_dev && step >= 0 && h >= 1 && w >= 1 && (long long)h * w <= (1ll << 30), "rt_op_step_noise: bad arguments");
        launch_step_noise(seed, step, h * w, out_dev, words_dev, (hipStream_t)stream);
    })
}
int rt_op_guided_prediction(const float* eps, const float* masks, const float* lat, const float* lat_ref, int h, int w, int R, int s_uncond,
                            int s_base, int s_uref, int s_tref, const int* s_region_host, float g, int plain, int step_ref, float phi,
                            int prediction_type, float cv, float cx, float* gpred_dev, double* partials_dev, float* factors_dev, void* stream) {
    OP_TRY({
        RT_REQUIRE(eps && lat && gpred_dev && factors_dev && h >= 1 && w >= 1 && (long long)h * w <= (1ll << 26), "rt_op_guided_prediction: bad arguments");
        RT_REQUIRE(prediction_type == RT_PRED_EPSILON || prediction_type == RT_PRED_V, "rt_op_guided_prediction: prediction_type must be 0 or 1");
        RT_REQUIRE(phi >= 0.f && phi <= 1.f && (phi == 0.f || partials_dev), "rt_op_guided_prediction: phi in [0, 1], with the partials scratch when > 0");
        RT_REQUIRE(plain || (masks && R >= 1 && R <= RT_MAXB && (R == 1 || s_region_host)), "rt_op_guided_prediction: rich mode needs masks and the region streams");
        RT_REQUIRE(s_uncond >= 0 && s_base >= 0 && (s_uref < 0 || (s_tref >= 0 && lat_ref)), "rt_op_guided_prediction: stream indices");
        GuidedArgs q{};
        q.s.eps = eps; q.s.masks = masks; q.s.lat = const_cast<float*>(lat); q.s.lat_ref = const_cast<float*>(lat_ref); q.s.HW = h * w; q.s.R = plain ? 0 : R;
        q.s.s_uncond = s_uncond; q.s.s_base = s_base; q.s.s_uref = s_uref; q.s.s_tref = s_tref; q.s.g = g; q.s.plain = plain ? 1 : 0; q.s.step_ref = step_ref ? 1 : 0;
        if (!plain) for (int r = 0; r < R - 1; ++r) { RT_REQUIRE(s_region_host[r] >= 0, "rt_op_guided_prediction: region stream"); q.s.s_region[r] = s_region_host[r]; }
        q.gpred = gpred_dev; q.partials = partials_dev; q.factors = factors_dev; q.phi = phi; q.vpred = prediction_type == RT_PRED_V; q.cv = cv; q.cx = cx;
        launch_guided_prediction(q, (hipStream_t)stream);
    })
}
int rt_op_freeu(void* hidden_f16, int C1, void* skip_f16, int C2, int B, int H, int W, float b, float s, void* stream) {
    OP_TRY({
        RT_REQUIRE(std::isfinite(b) && b > 0.f && std::isfinite(s) && s > 0.f, "rt_op_freeu: b and s must be finite and > 0");
        launch_freeu((f16_t*)hidden_f16, C1, (f16_t*)skip_f16, C2, B, H, W, b, s, (hipStream_t)stream);
    })
}
int rt_op_identity_attention(const void* VT, int ldvt, void* O, int ldo, const int* entry_host, int n, int B, int H, int N, int DP, void* stream) {
    OP_TRY({ launch_identity_attention((const bf16_t*)VT, ldvt, (bf16_t*)O, ldo, entry_host, n, B, H, N, DP, (hipStream_t)stream); })
}
int rt_op_pag_fold(float* eps, int n_streams, int h, int w, const int* stream_host, const int* twin_host, const float* ratio_host, int n, void* stream) {
    OP_TRY({
        RT_REQUIRE(h >= 1 && w >= 1, "rt_op_pag_fold: grid");
        launch_pag_fold(eps, n_streams, h * w, stream_host, twin_host, ratio_host, n, (hipStream_t)stream);
    })
}
int rt_op_control_add(void* skip_f16, long long skip_stride, int lds, const float* r, long long r_stride, int ldr, const int* stream_host,
                      const float* scale_host, int n, int B, int HW, int C, void* stream) {
    OP_TRY({
        RT_REQUIRE(skip_f16 && r && stream_host && scale_host && skip_stride >= 0 && r_stride >= 0, "rt_op_control_add: null argument / negative stride");
        launch_control_add((f16_t*)skip_f16, (size_t)skip_stride, lds, r, (size_t)r_stride, ldr, stream_host, scale_host, n, B, HW, C, (hipStream_t)stream);
    })
}
int rt_op_lora_add(const void* X, int ldx, const void* down, int ldd, const void* up, int ldu, const float* alpha_over_rank, const int* col_adapter,
                   void* Y, int ldy, int form, const int* row_host, const float* scale_host, int B, int rows, int K, int N, int R, int* launched,
                   void* stream) {
    OP_TRY({
        RT_REQUIRE(X && down && up && alpha_over_rank && col_adapter && Y && row_host && scale_host, "rt_op_lora_add: null argument");
        const int n = launch_lora_add((const bf16_t*)X, ldx, (const bf16_t*)down, ldd, (const bf16_t*)up, ldu, alpha_over_rank, col_adapter, Y, ldy, form,
                                      row_host, scale_host, B, rows, K, N, R, (hipStream_t)stream);
        if (launched) *launched = n;
    })
}
int rt_op_lora_geglu(const void* X, int ldx, const void* down, int ldd, const void* up, int ldu, const float* alpha_over_rank, const int* col_adapter,
                     const float* Z, int ldz, void* out, int ldo, const int* row_host, const float* scale_host, int B, int rows, int K, int N, int R,
                     int* launched, void* stream) {
    OP_TRY({
        RT_REQUIRE(X && down && up && alpha_over_rank && col_adapter && Z && out && row_host && scale_host, "rt_op_lora_geglu: null argument");
        const int n = launch_lora_geglu((const bf16_t*)X, ldx, (const bf16_t*)down, ldd, (const bf16_t*)up, ldu, alpha_over_rank, col_adapter, Z, ldz,
                                        (bf16_t*)out, ldo, row_host, scale_host, B, rows, K, N, R, (hipStream_t)stream);
        if (launched) *launched = n;
    })
}
int rt_op_cast_bf16(const float* x, void* out_bf16, long long n, void* stream) {
    OP_TRY({ RT_REQUIRE(n > 0, "cast: empty"); launch_cast_f32_bf16(x, (bf16_t*)out_bf16, (size_t)n, (hipStream_t)stream); })
}
int rt_op_attention_probs_avg(const void* Q, int ldq, long long q_row0, const void* K, int ldk, long long k_row0, float* out,
                              int H, int N, int NK, int NKpad, int NKrows, int DP, int accumulate, void* stream) {
    OP_TRY({
        AttnStoreArgs a{}; a.Q = (const bf16_t*)Q; a.ldq = ldq; a.q_row0 = (long)q_row0; a.K = (const bf16_t*)K; a.ldk = ldk; a.k_row0 = (long)k_row0;
        a.out = out; a.H = H; a.N = N; a.NK = NK; a.NKpad = NKpad; a.NKrows = NKrows; a.DP = DP; a.overwrite = accumulate ? 0 : 1;
        a.stats = op_store_stats((size_t)H * N * 2, (hipStream_t)stream);
        launch_attn_store(a, (hipStream_t)stream);
    })
}
// A recorded layer as the UNet forward runs it: the attention launch, then the store of stream `store_stream`.
int rt_op_attention_store_handover(const void* Q, int ldq, const void* K, int ldk, const void* VT, int ldvt, void* O, int ldo,
                                   const int* qk_src_host, const int* prompt_host, const int* key_counts_host, const float* wabs,
                                   const float* wsgn, int B, int H, int N, int NK, int d, int DP, int cross, int store_stream,
                                   float* map_out, int accumulate, int* handover, void* stream) {
    OP_TRY({
        hipStream_t st = (hipStream_t)stream;
        RT_REQUIRE(B >= 1 && B <= RT_MAXB && store_stream >= 0 && store_stream < B && map_out && handover, "rt_op_attention_store_handover: batch / recorded stream / outputs");
        RT_REQUIRE(H >= 1 && H <= 32 && N >= 1, "rt_op_attention_store_handover: at most 32 heads");
        const AttnIO io{(const bf16_t*)Q, ldq, (const bf16_t*)K, ldk, (const bf16_t*)VT, ldvt, (bf16_t*)O, ldo};
        float* scratch = op_store_stats((size_t)H * N * 2, st);
        bool taken = false;
        if (!cross) {
            RT_REQUIRE(NK == N, "rt_op_attention_store_handover: self-attention has as many keys as queries");
            int src[RT_MAXB];
            for (int b = 0; b < B; ++b) src[b] = qk_src_host ? qk_src_host[b] : b;
            for (int b = 0; b < B; ++b) RT_REQUIRE(src[b] >= 0 && src[b] < B, "rt_op_attention_store_handover: Q / K source");
            taken = scratch && store_handover_self(N, DP, src, store_stream);
            const AttnArgs a = unet_self_attn_args(io, src, B, H, N, DP, taken ? scratch : nullptr, store_stream);
            launch_attention(a, st);
            // the key COUNT is padded to the store's 32-key step, the key rows are not (a map of N % 32 == 0 tokens: NKpad = N as in the forward)
            launch_attn_store(unet_store_args(a, store_stream, map_out, !accumulate, scratch, (N + 31) / 32 * 32), st);
        } else {
            RT_REQUIRE(prompt_host && key_counts_host && (NK == 96 || NK == 192 || NK == 288), "rt_op_attention_store_handover: prompts of 96, 192 or 288 rows");
            int wset[RT_MAXB];
            std::fill_n(wset, RT_MAXB, -1);
            for (int b = 0; b < B; ++b)
                RT_REQUIRE(op_key_count_ok(key_counts_host[b], NK) && prompt_host[b] >= 0, "rt_op_attention_store_handover: a key count must be 77 per 96-row chunk of NK");
            // a recorded layer whose Q is in HBM: the two-launch routes; the statistics where the route hands them over
            const CrossRoute route = cross_route(H * DP, H, d, DP, N, NK, key_counts_host, B, false, true, false);
            taken = scratch && route.handover;
            const AttnArgs a = unet_cross_attn_args(io, prompt_host, wset, key_counts_host, wabs, wsgn, B, H, N, NK, DP, taken ? scratch : nullptr, store_stream);
            launch_cross(a, route, st);
            launch_attn_store(unet_store_args(a, store_stream, map_out, !accumulate), st);
        }
        *handover = taken ? 1 : 0;
    })
}
// The forward's route of an attn2 launch as a host-only query (no device needed): cross_route and cross_run, under the same switches.
int rt_op_cross_route(int C, int heads, int d, int DP, int tokens, int prompt_rows, const int* key_counts_host, int B, int folded, int recorded,
                      int* kind, int* handover, int* stream_kernel) {
    static_assert(CrossRoute::GENERIC == RT_CROSS_GENERIC && CrossRoute::CROSS77 == RT_CROSS_CROSS77 && CrossRoute::RUNS == RT_CROSS_RUNS &&
                  CrossRoute::XATTN_FUSED == RT_CROSS_XATTN_FUSED && CrossRoute::XBLOCK == RT_CROSS_XBLOCK, "RT_CROSS_* mirror CrossRoute::Kind");
    if (!key_counts_host || B < 1 || B > RT_MAXB || !(prompt_rows == 96 || prompt_rows == 192 || prompt_rows == 288)) return RT_E_INVALID;
    for (int b = 0; b < B; ++b) if (!op_key_count_ok(key_counts_host[b], prompt_rows)) return RT_E_INVALID;
    const CrossRoute r = cross_route(C, heads, d, DP, tokens, prompt_rows, key_counts_host, B, folded != 0, recorded != 0);
    if (kind) *kind = r.kind;
    if (handover) *handover = r.handover ? 1 : 0;
    if (stream_kernel) {
        for (int b = 0; b < B; ++b) stream_kernel[b] = r.kind == CrossRoute::GENERIC ? 0 : r.kind == CrossRoute::CROSS77 ? 1 : -1;
        for (int b0 = 0, b1, kernel; r.kind == CrossRoute::RUNS && b0 < B; b0 = b1) {
            b1 = cross_run(key_counts_host, B, b0, heads, DP, tokens, prompt_rows, &kernel);
            std::fill(stream_kernel + b0, stream_kernel + b1, kernel);
        }
    }
    return RT_OK;
}

}  // extern "C"
