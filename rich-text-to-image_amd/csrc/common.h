// Shared device/host helpers for the region-diffusion engine (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <stdexcept>

typedef uint16_t bf16_t;   // raw bf16 bits in memory
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define RT_OK 0
#define RT_E_INVALID (-1)
#define RT_E_HIP (-2)
#define RT_E_STATE (-3)
#define RT_E_MISSING_WEIGHT (-4)
#define RT_E_UNSUPPORTED (-5)

struct rt_error : std::runtime_error {
    int code;
    rt_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIP_CHECK(expr)                                                                        \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            throw rt_error(RT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

#define RT_REQUIRE(cond, msg)                                                                  \
    do {                                                                                       \
        if (!(cond)) throw rt_error(RT_E_INVALID, std::string(msg) + " [" #cond "]");          \
    } while (0)

__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// fp32 -> bf16, round-to-nearest-even, NaN stays NaN: gfx950's v_cvt_pk_bf16_f32 (one instruction per PAIR; rounds 1-2 carried a
// 12-instruction integer sequence with an exec-mask branch for the NaN case per VALUE, which made the bf16 epilogues VALU bound)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 hw_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, hw_bf16x2));
}
__device__ __forceinline__ bf16_t f32_to_bf16(float f) { return (bf16_t)(pack_bf16x2(f, f) & 0xffffu); }
// "low part" of a value whose high part is its bf16 rounding: v ~= bf16(v) + bf16(v - bf16(v)) to 2^-17 relative.  The precise mode
// of the VAE engine (vae.hip) multiplies such pairs with three bf16 MFMA passes (hi*hi + lo*hi + hi*lo, fp32 accumulation).
__device__ __forceinline__ float bf16_residual(float v) { return v - bf16_to_f32(f32_to_bf16(v)); }
__device__ __forceinline__ uint32_t pack_bf16x2_lo(float a, float b) { return pack_bf16x2(bf16_residual(a), bf16_residual(b)); }

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// gelu(x) = 0.5 x (1 + erf(x / sqrt 2)), erf(x / sqrt 2) as an odd degree-17 polynomial P of clamp(x, +-4.25) with P(4.25) == 1
// (weighted least-squares minimax fit, tools/fit_gelu.py): |gelu error| <= 6.4e-5 absolute everywhere (below half an ulp of the bf16
// output for |gelu| > 0.03, exact saturation 0 / x outside the clamp), no transcendental instruction.  The GEGLU epilogues evaluate
// it on 56 gate values per lane and tile; round 3 measured them VALU bound on the previous rcp + exp2 form (2 quarter-rate
// instructions + 13 scalar FMAs per value).  The x2 form maps to v_pk_mul_f32 / v_pk_fma_f32, two gates per issue slot; both forms
// run the same IEEE fma sequence and are bit-identical.
#define RT_GELU_CLAMP 4.25f
#define RT_GELU_C8 1.203002836e-10f
#define RT_GELU_COEFS(K)                                                                                                                  \
    K(-1.137335648e-08f) K(4.748426363e-07f) K(-1.167462415e-05f) K(1.911683503e-04f) K(-2.242938848e-03f)           \
    K(1.971663348e-02f) K(-1.328222901e-01f) K(7.978754640e-01f)
__device__ __forceinline__ f32x2 gelu_erf_x2(f32x2 x) {
    f32x2 xc;
    xc.x = __builtin_amdgcn_fmed3f(x.x, -RT_GELU_CLAMP, RT_GELU_CLAMP);
    xc.y = __builtin_amdgcn_fmed3f(x.y, -RT_GELU_CLAMP, RT_GELU_CLAMP);
    const f32x2 s = xc * xc;
    f32x2 q = {RT_GELU_C8, RT_GELU_C8};
#define RT_K(c) q = __builtin_elementwise_fma(q, s, (f32x2){c, c});
    RT_GELU_COEFS(RT_K)
#undef RT_K
    const f32x2 pe = xc * q;                                        // erf(x / sqrt 2)
    const f32x2 h = x * 0.5f;
    return __builtin_elementwise_fma(h, pe, h);
}
__device__ __forceinline__ float gelu_erf(float x) {
    const float xc = __builtin_amdgcn_fmed3f(x, -RT_GELU_CLAMP, RT_GELU_CLAMP);
    const float s = xc * xc;
    float q = RT_GELU_C8;
#define RT_K(c) q = __builtin_fmaf(q, s, c);
    RT_GELU_COEFS(RT_K)
#undef RT_K
    const float pe = xc * q;
    const float h = x * 0.5f;
    return __builtin_fmaf(h, pe, h);
}

// async global -> LDS copy of 16 B per lane (LDS destination = wave-uniform base + lane*16)
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// LDS-DMA through a buffer descriptor: buffer_load_dwordx4 v(voff), s[rsrc], s(soff) offen lds.  `base` must be wave-uniform; the
// descriptor is rebuilt from it at every call site (4 SALU moves, hoisted by the compiler).  Kept in a non-template __device__
// function: the descriptor type exists in device compilation only and a kernel TEMPLATE that names it loses its host-side stub.
static __device__ __forceinline__ void glds16_buf(const void* base, int voff_bytes, int soff_bytes, void* lds_wave_base, unsigned range_bytes = 0x7fffffffu) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, range_bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff_bytes, soff_bytes, 0, 0);
}
// ---------------------------------------------------------------- GEMM / implicit-GEMM conv
// A_CONV3_S2P0: 3x3 stride-2 convolution with zero padding on the bottom / right only (diffusers Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1))
// then stride 2, pad 0), the VAE encoder's downsamplers; Hin, Win even, Hout = Hin / 2, Wout = Win / 2
enum { A_DENSE = 0, A_CONV3 = 1, A_CONV3_S2 = 2, A_CONV3_UP2 = 3, A_CONV3_S2P0 = 4 };
enum { EPI_BF16 = 0, EPI_F32 = 1, EPI_BF16_TEMB = 2, EPI_GEGLU = 3, EPI_F16 = 4,   // EPI_F16: fp16 output (+ fp16 residual): the UNet trunk
       EPI_XATTN = 5 };   // gemm16.hip only: the to_q projection whose tile never leaves the CU - 77-key cross-attention on it, O written (launch_xattn_fused)
typedef _Float16 f16_t;
#define RT_MAXB 16

struct GemmArgs {
    const bf16_t* A;   // dense: [M, lda]; conv: NHWC input [B, Hin, Win, Cin]
    const bf16_t* W;   // [N, ldw] (K contiguous)
    const float* bias; // [N] or null
    void* out;         // bf16 or f32, [M, ldo]
    const void* res;   // optional residual [M, ldres]: fp32 for EPI_F32, fp16 for EPI_F16
    const float* temb; // EPI_BF16_TEMB: [B, temb_ld]
    const bf16_t* zero; // >= 16 B of zeros
    int mode, epi;
    int M, N, K;
    int lda, ldw, ldo, ldres, temb_ld;
    int rows_per_batch;              // Hout*Wout (conv and temb)
    int Hin, Win, Cin, Hout, Wout;   // conv geometry (Cin padded to a multiple of 8; K = 9*Cin)
    int debug;                       // unused by the product kernels (kept so probe builds can pass flags without changing the ABI of the struct)
    int rows_per_stream;             // tokens ONE stream contributes to the batched dimension (0: unknown): keys the tile-class choice of
                                     // gemm16.hip so that a stream's result does not depend on the other streams of the launch
    float* splitk_ws;                // optional split-K partial-sum scratch owned by the caller (engine workspace); null: per-(device, stream) fallback
    size_t splitk_ws_floats;
    int prefer_patch_conv;           // 1: stride-1 3x3 convolution that should stay on the patch kernel (single-image VAE layers whose 224-row GEMM
                                     // tiles would leave most of the chip idle: the caller decides on its own, batch-free, shape)
    int weights_on_rows;             // 1: the V^T product (A = weight rows, W = token rows): tile-class choices key on M instead of N
    int split_tiles;                 // 128x128 output tiles of ONE batch entry's share of the problem (0: unknown).  The split-K rule
                                     // uses it instead of the actual tile count, so a stream's result does not depend on how many
                                     // other streams share the launch (batch invariance); see splitk_slices in gemm.hip
    // Triple-pass contraction of the VAE's precise mode (vae.hip): out = A W^T + A_lo W^T + A W_lo^T accumulated in ONE fp32 accumulator
    // (operands as bf16 pairs v = hi + lo).  Null: single pass.  The 3x3 convolution kernels run it as one launch with a three times
    // longer K loop (no fp32 read-modify-write of the output between passes); launch_gemm falls back to three launches elsewhere.
    const bf16_t* A_lo; const bf16_t* W_lo;
    // EPI_F32 with pair_lo != null (precise VAE, 3x3 convolutions on the patch kernel only: gemm_pair_output_ok): the fp32 result leaves
    // as the bf16 pair the NEXT contraction consumes - `out` = hi plane, `pair_lo` = lo plane, both bf16 [M, ldo] - instead of fp32
    // that a cast kernel would read back and split (8 B of traffic per element saved; same bits: pack_bf16x2 / pack_bf16x2_lo)
    bf16_t* pair_lo;
    // EPI_XATTN (launch_xattn_fused): A = LayerNorm'd tokens [B * xa_tokens, K], W = packed to_q [H * 64, K] (pre-scaled by
    // d^-1/2 log2 e), out = attention output O [M, ldo] bf16.  K / V^T: the per-prompt cross-attention cache (AttnArgs layout).
    const bf16_t* xa_k; const bf16_t* xa_vt;
    int xa_ldk, xa_ldvt;
    int xa_tokens;                   // query tokens per stream (multiple of 128: a 128-row tile never straddles two streams)
    int xa_nk_valid;                 // keys >= xa_nk_valid of the 96 cached rows are masked (77)
    const float* xa_wabs; const float* xa_wsgn;      // [nsets, 96] font-size multipliers (attention_processor.py:386-401)
    int xa_prompt[RT_MAXB], xa_wset[RT_MAXB];        // per stream: prompt index into the cache, multiplier set (-1: plain softmax)
    // LayerNorm folded into the projections (gemm16.hip, "LNF"; models/attention.py:150,168,181).
    //  consumer (ln_part != null; EPI_BF16 / EPI_GEGLU on the 16x16x32 family only): the token operand (A, or W when weights_on_rows) is
    //    xb = the UN-normalised trunk as bf16, the weight operand is W' = bf16(gamma W) (ln_fold_derive), ln_s = [weight rows] (s, c)
    //    pairs: s = row sums of W', c = b + W beta (`bias` is unused); out = rstd (xb W'^T - mu s) + c with (mu, rstd) of every token
    //    from ln_part: one (sum, sum of squares) of xb per token and column tile of the producer, pair-major [ln_npair][ln_ld] float4
    //    = two tiles each (ln_npair = 1, 2 or 4)
    //  producer (ln_emit != null; EPI_F16 on the 16x16x32 family's 80-column wave tiles): besides the fp16 trunk leaves xb in ln_copy
    //    [M, ldo] and that array for its OUTPUT rows in ln_emit (ln_ld = M)
    const float* ln_part; int ln_npair;
    int ln_ld;
    const float* ln_s;
    float ln_inv_c, ln_eps;
    bf16_t* ln_copy;
    float* ln_emit;
    // A_CONV3_UP2 only: the sub-pixel ("phase") pack of the same 3x3 weight, [phase 4][N][tap 4][Cin] bf16 (launch_pack_up2); null: the
    // layer has none and stays on the patch kernel.  With it the layer may run as four 2x2 convolutions of the low-resolution map
    // (gemm16.hip, MODE = A_CONV3_UP2; gemm_route: G16_UP2)
    const bf16_t* W_up2;
};
// LayerNorm fold plumbing (host-only predicates are pure functions of the shape, like every routing decision)
int gemm_ln_emit_bn(const GemmArgs& a);                 // column-tile width (160 / 320) of the partials launch_gemm(a) with a.ln_emit set would leave; 0: this route has no such epilogue
bool gemm_ln_fold_ok(const GemmArgs& a);                // launch_gemm(a) with a.ln_part set has a folded instantiation
bool gemm16_ln_variant_ok(const GemmArgs& a, int v);    // gemm16.hip: variant v has the LayerNorm-fold instantiation a.ln_part / a.ln_emit ask for
void launch_ln_partials(const f16_t* x, bf16_t* xb, float* part, int rows, int C, int bn, hipStream_t st, int part_ld = 0);      // (part_ld: the rows are a run inside a partials array of that many rows) stand-alone producer of xb + partials (column tiles of bn = 160 / 320) from an fp16 trunk (norm.hip)
void launch_ln_fold_derive(const bf16_t* W, int ldw, const float* bias, const float* gamma, const float* beta, int N, int K,
                           bf16_t* Wf, float* sc, hipStream_t st);                         // W' = bf16(gamma W), sc[n] = (row sum of W', bias + W beta)
int gemm16_variant_bn(int v);                           // column-tile width of a gemm16 variant
// Fused to_q -> 77-key cross-attention (one launch instead of two; Q never reaches HBM).  Eligible: head dim 64, H * 64 % 320 == 0,
// tokens % 128 == 0, C % 64 == 0, C >= 192.
bool xattn_fused_supported(int C, int H, int DP, int tokens);
void launch_xattn_fused(const GemmArgs& a, hipStream_t st);
// xblock.hip: the whole cross-attention block of the 640-channel level (to_q -> 77-key attention -> to_out + bias + fp16 residual) as ONE
// launch with Q, P and O in registers.  x = LayerNorm'd tokens (bf16), wq = packed to_q [H * 64, C] pre-scaled by d^-1/2 log2 e,
// wo = packed to_out [C, H * 64], K / V^T = the per-prompt cache (AttnArgs layout), res / out = the fp16 trunk.
struct XBlockArgs {
    const bf16_t* x; const bf16_t* wq; const bf16_t* wo; const float* bo;
    const bf16_t* kc; const bf16_t* vt;
    const f16_t* res; f16_t* out;
    const float* wabs; const float* wsgn;            // [nsets, 96] font-size multipliers (attention_processor.py:386-401)
    int ldk, ldvt, ldres, ldo;
    int M, tokens, nk_valid, C, H;                   // M = streams * tokens; keys >= nk_valid of the 96 cached rows are masked
    int prompt[RT_MAXB], wset[RT_MAXB];              // per stream: prompt index into the cache, multiplier set (-1: plain softmax)
};
bool xblock_supported(int C, int H, int DP, int tokens);
void launch_xblock(const XBlockArgs& a, hipStream_t st);
void launch_gemm(const GemmArgs& a, hipStream_t st);
// What launch_gemm does with a problem, host-only: a pure function of the arguments and the switches (gemm_set_debug, gemm_force_config).
// It reads the shape and also A_lo / W_lo / pair_lo / ln_part / ln_emit / prefer_patch_conv / weights_on_rows / split_tiles /
// rows_per_stream, so this and every query below must be asked with the arguments as they will be launched.
struct GemmRoute {
    enum Kind { G16, PATCH, PATCH_SPLIT, KSPLIT, TILE, TRIPLE, G16_UP2 };
    Kind kind = TILE;  // G16: gemm16.hip | G16_UP2: gemm16.hip, the 2x-upsample convolution as four 2x2 phase convolutions | PATCH: conv3p_kernel | PATCH_SPLIT: conv3p_kernel over input-channel chunks + reduction |
                       // KSPLIT: K slices of the 128x128 kernel + reduction | TILE: a gemm.hip tile configuration |
                       // TRIPLE: hi / lo contraction as three launches of the single-pass problem
    int variant = -1, wstat = 0;   // G16: tile variant, W-stationary tile order
    int slices = 1;                // PATCH_SPLIT / KSPLIT
    int cfg = -1;                  // TILE
};
GemmRoute gemm_route(const GemmArgs& a);
bool gemm_pair_output_ok(const GemmArgs& a);            // launch_gemm would run this problem on a kernel that can write GemmArgs.pair_lo
size_t gemm_splitk_scratch_floats(const GemmArgs& a);   // fp32 partial sums launch_gemm needs for this problem (0: not split)
void gemm_force_config(int cfg);   // -1: shape-based choice; 0..8: force a gemm.hip tile configuration (also keeps gemm16.hip out)
// rt_op_gemm_debug's A/B switches (benchmarks, tests, RTDIFF_DEBUG_FLAGS): bit positions, part of the interface - callers pass raw numbers
enum DebugBit {
    DBG_CONV_IMPLICIT = 0,        // patch-eligible 3x3 convolutions through the implicit-GEMM kernels
    DBG_NO_GEMM16 = 1,            // keep gemm16.hip out
    DBG_NO_SPLIT = 2,             // no split-K (neither K slices nor input-channel chunks)
    DBG_CONV_NO_GEMM16 = 3,       // stride-1 3x3 convolutions stay on the patch kernel instead of gemm16.hip's implicit GEMM
    DBG_NO_XATTN_FUSED = 4,       // cross-attention as to_q GEMM + attention launch instead of the fused kernel (probe builds)
    DBG_STORE_TWO_PASS = 5,       // token-map accumulation on the round-1 two-pass single-wave kernel for every shape (attn_store.hip)
    DBG_STORE_ONE_PASS = 6,       // large token maps on the one-pass kernel instead of the statistics + key-split apply pair
    DBG_TRIPLE = 7,               // the precise VAE's hi / lo contractions as three launches (round 3) instead of one
    DBG_TRIPLE_GEMM16 = 8,        // ... only those on the gemm16 convolution route
    DBG_TRIPLE_PATCH = 9,         // ... only those on the patch kernel
    DBG_CONV3P_NO_TN4 = 10,       // chunk-split patch convolutions keep 160-channel column tiles where N % 160 == 0
    DBG_GN_CHUNK_128 = 11,        // GroupNorm chunks of 128 rows (norm.hip) instead of 64
    DBG_G16_NO_DEEP = 12,         // no 5-slot ring for gemm16.hip's 64 x 160 tiles
    DBG_NO_PAIR = 13,             // attn1's Q|K and V^T projections as two launches instead of one grouped launch
    DBG_ATTN_NO_PRIO = 14,        // no raised wave priority in the MFMA phases of the attention kernel
    DBG_TRIPLE_DENSE = 15,        // the precise VAE's DENSE hi / lo contractions as three launches
    DBG_XBLOCK = 16,              // the 640-channel cross-attention block as xblock.hip's one launch (opt-in, probe builds)
    DBG_STORE_OWN_STATS = 17,     // the token-map store computes the softmax statistics itself although the attention launch could leave them
    DBG_STORE_APPLY_V1 = 18,      // round 4's apply kernel of the token-map store for every head dim
    DBG_NO_CROSS77 = 19,          // cross-attention on the round-4 kernels instead of cross77_kernel
    DBG_C77_ONE_TILE = 20,        // cross77_kernel / crossmw_kernel: one 16-query tile per wave for every shape
    DBG_C77_TWO_HEADS = 21,       // cross77_kernel: two heads per workgroup
    DBG_NO_LNFOLD = 22,           // LayerNorm launches + bf16 projections (rounds 1 - 5) instead of the folded form
    DBG_GN_TWO_LAUNCH = 23,       // GroupNorm always in its two-launch form
    DBG_ATTN_UNITS = 24,          // bits 24 - 26: shared-probability units mode of the self-attention launches (0: the shape rule)
    DBG_G16_TALL = 27,            // GEGLU launches that cannot take the W-stationary order run groups of 8 tile rows
    DBG_NO_CHUNK_SPLIT = 28,      // under-filled 3x3 convolutions on the split-K implicit GEMM instead of the chunk-split patch kernel
    DBG_NO_CHUNK_HALVES = 29,     // no two-halves chunk split for the 32x32 maps
    DBG_SPLIT_NO_SMALL_ROWS = 30, // the split rule counts streams of < 128 rows as whole 128-row tiles
};
// rt_op_gemm_debug2's switches: the second word (bits 0 - 30 of the first are taken, bit 31 stays unused)
enum DebugBit2 {
    DBG2_NO_UP2_PHASE = 0,        // the 2x-upsample convolutions stay on the patch kernel (nine taps on the up-sampled map) instead of four 2x2 phase convolutions
};
static inline int debug_bit(int flags, int bit) { return (flags >> bit) & 1; }
void gemm_set_debug(int flags);    // decodes the routing bits above
void gemm_set_debug2(int flags);   // ... and those of the second word
bool gemm_lnfold_enabled();       // LayerNorm folded into its consumers (debug bit 22 clear, gemm16 on, no forced configuration)
bool gemm_xblock_enabled();       // the one-launch cross-attention block (xblock.hip) is switched on (debug bit 16 SET - opt-in; gemm16 on, no forced configuration)
bool gemm_xattn_enabled();         // the fused to_q + cross-attention kernel is allowed (debug bit 4 clear, gemm16 on, no forced configuration)
// gemm16.hip: 16x16x32-MFMA family (224-row tiles, intra-tile K split); dense problems with K % 64 == 0 only
#define RT_G16_NVAR 14
bool gemm16_supported(const GemmArgs& a);
int gemm16_pick(const GemmArgs& a, int weights_on_rows, int* wstat);      // variant id or -1; pure function of the shape
void launch_gemm16_variant(const GemmArgs& a, int variant, int wstat, hipStream_t st);
int gemm16_pick_up2(const GemmArgs& a);         // A_CONV3_UP2 with a phase pack: tile variant (0 / 4) of the four-phase launch, -1: none; pure function of ONE image's shape
void launch_gemm16_up2(const GemmArgs& a, int variant, hipStream_t st);
int gemm16_pair_variant(const GemmArgs& a, int va, int wa, const GemmArgs& b, int vb, int wb);     // id of the grouped instantiation of tiles
                                                                                                  // va / vb (gemm16_pick) (0..3), -1: none
void launch_gemm16_pair(const GemmArgs& a, const GemmArgs& b, int pair, hipStream_t st);          // grouped launch of instantiation `pair` (gemm16.hip)
int gemm_pair_grouped(const GemmArgs& a, const GemmArgs& b);    // host-only: grouped instantiation launch_gemm_pair takes, -1: two launches
void launch_gemm_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t st);     // gemm.hip: the grouped launch where it exists (debug bit 13 clear), else two launch_gemm calls

// ---------------------------------------------------------------- attention
struct AttnArgs {
    const bf16_t* Q;  int ldq;   // [*, ldq]  row (q_src[b]*N + n), head h at column h*DP; pre-scaled by d^-1/2 * log2(e)
    const bf16_t* K;  int ldk;   // [*, ldk]  row (k_src[b]*NK + key), head h at column h*DP
    const bf16_t* VT; int ldvt;  // [H*DP, ldvt] row (h*DP + d), column (v_src[b]*NK + key)
    bf16_t* O;        int ldo;   // [B*N, ldo] row (b*N + n), head h at column h*DP
    int q_src[RT_MAXB], k_src[RT_MAXB], v_src[RT_MAXB], wset[RT_MAXB];
    // filled by launch_attention (attn_kernel only): a launch runs B UNITS; unit b attends with (q_src[b], k_src[b]) and has ng[b] members
    // that share its probabilities - member g reads V^T of batch entry gvs[b][g] and writes the output rows of batch entry gob[b][g]
    // (one-stream launches: ng = 1, gvs = v_src[b], gob = b)
    unsigned char ng[RT_MAXB], gvs[RT_MAXB][4], gob[RT_MAXB][4];
    const float* wabs;           // cross: [nsets, NK] |font size| multiplier per key; null => plain softmax
    const float* wsgn;           // cross: [nsets, NK] sign multiplier per key
    int B, H, N;                 // queries per batch entry
    int NK;                      // keys per batch entry in K / V^T (multiple of the key tile)
    int nk_valid;                // cross: keys >= nk_valid are masked out
    int nkeys[RT_MAXB];          // cross (attn_kernel only): the valid keys of batch entry b - its prompt's own count, 77 per chunk - when they
                                 // differ between the entries of a launch; 0 = nk_valid.  NK is then the prompt STRIDE (96 rows per chunk of
                                 // the longest prompt the caches are sized for): entry b runs ceil(nkeys[b] / 96) key tiles, never more
    int DP;                      // padded head dim (multiple of 32)
    int cross;
    int nqb;                     // set by launch_attention: 128-query blocks per (batch entry, head)
    // self-attention only: when non-null, the kernel also leaves the softmax statistics of batch entry stats_b - (running reference m,
    // 1 / (H * sum)) per (head, query), [H][N][2] fp32 - which is exactly what attn_store_apply_kernel needs to rebuild the
    // head-averaged probabilities of that stream: the token-map capture of the plain pass then skips its own statistics pass
    float* stats; int stats_b;
};
void launch_attention(const AttnArgs& a, hipStream_t st);
// xblock.hip: the 77-key cross-attention as its own kernel (d = 64, cached K / V^T): 64 queries x 2 heads per workgroup, K / V^T in LDS
bool cross77_supported(int H, int DP, int tokens, int NK, int nk_valid);
void launch_cross77(const AttnArgs& a, hipStream_t st);
bool crossmw_supported(int H, int DP, int tokens, int NK);    // crossmw_kernel (cross77.hip): streams of 154 / 231 keys, head dim 64
void launch_crossmw(const AttnArgs& a, hipStream_t st);
// ipattn.hip: the image-prompt term of decoupled cross-attention, O += scale[b] softmax(Q Kip[slot[b]]^T) Vip[slot[b]] in place over count[b] <= 16
// keys (Kip [*, ldk] 16 rows per slot, VTip [H*DP, ldvt] 16 columns per slot); host arrays; slot < 0 or scale == 0: the stream is not launched
void launch_ip_attention(const bf16_t* Q, int ldq, const bf16_t* Kip, int ldk, const bf16_t* VTip, int ldvt, bf16_t* O, int ldo, const int* slot,
                         const int* count, const float* scale, int B, int H, int N, int DP, hipStream_t st);
// lora.hip: the unmerged low-rank term Y += bf16(f_b (X down^T)) up^T in place, per stream (form 0 bf16 row-major, 1 bf16 transposed [N, ldy],
// 2 fp16 row-major); row / scale [B][4] are host arrays; a stream whose scales are all 0 is not launched; returns the streams in the grid
int launch_lora_add(const bf16_t* X, int ldx, const bf16_t* down, int ldd, const bf16_t* up, int ldu, const float* aor, const int* adapter, void* Y,
                    int ldy, int form, const int* row, const float* scale, int B, int rows, int K, int N, int R, hipStream_t st);
// ... and ff.net.0.proj of the adapted streams from the base GEMM's fp32 pre-activations Z [*, ldz] (bias in; N packed columns, per 64-block
// [32 value | 32 gate], `up` [N, ldu] in the same row order): out[*, ldo] (N / 2 columns) = bf16((Zv + Dv) gelu(Zg + Dg)), D = bf16(f_b (X down^T)) up^T
int launch_lora_geglu(const bf16_t* X, int ldx, const bf16_t* down, int ldd, const bf16_t* up, int ldu, const float* aor, const int* adapter, const float* Z,
                      int ldz, bf16_t* out, int ldo, const int* row, const float* scale, int B, int rows, int K, int N, int R, hipStream_t st);
bool gemm_cross77_enabled();      // debug bit 19 clear
int attention_units_plan_host(const int* q_src, const int* k_src, int B, int N, int DP, int mode, int* launch_of, int* unit_of, int* members_of);   // host-only: the partition launch_attention would take
void gemm16_set_tall(int on);        // (A/B) rt_op_gemm_debug bit 27
void gemm16_set_deep(int on);        // (A/B) rt_op_gemm_debug bit 12 clears the 5-slot ring of the 64 x 160 tiles
void attention_set_units(int mode);  // shared-probability units of the self-attention launches (attention.hip, launch_attention_units; rt_op_gemm_debug bits 24 - 26)
void attention_set_prio(int on);   // s_setprio around the MFMA phases of attn_kernel (default on; rt_op_gemm_debug bit 14 clears it)

// head-averaged probabilities of one stream, accumulated over calls (token-map producer)
struct AttnStoreArgs {
    const bf16_t* Q; int ldq; long q_row0;     // query rows q_row0 + [0, N), head h at column h*DP (pre-scaled like AttnArgs.Q)
    const bf16_t* K; int ldk; long k_row0;     // key rows k_row0 + [0, NKrows)
    float* out;                                // [N, NK] fp32 accumulator
    int H, N, NK, NKpad, NKrows, DP;
    int overwrite;                             // 1: out = avg(P); 0: out += avg(P)
    float* stats;                              // optional scratch [H][N][2] fp32 (softmax max, 1 / (H sum) per (head, query)): enables the
                                               // statistics + key-split apply pair for maps of >= 256 keys; null: one-pass kernel
    int stats_ready;                           // 1: `stats` already holds the statistics of this stream (written by the attention
                                               // launch itself, AttnArgs.stats): only the apply kernel runs
};
void launch_attn_store(const AttnStoreArgs& a, hipStream_t st);
bool attn_store_takes_stats(int N, int NK, int DP);   // the statistics + apply pair would run for this map: the self-attention launch may leave the statistics

// ---------------------------------------------------------------- norms / elementwise
struct GroupNormArgs {
    const void* x1; const void* x2;   // x2 may be null; virtual concat along channels [C1 | C2]
    int in_bf16;                       // input element type: 0 fp32, 1 bf16 (x2 must be null), 2 fp16 (UNet trunk)
    int C1, C2, G, B, HW;
    const float* gamma; const float* beta; float eps;
    int silu;
    bf16_t* out;                       // [B, HW, C1+C2] normalised (+SiLU)
    bf16_t* raw_out;                   // optional: un-normalised bf16 copy of the (concatenated) input
    bf16_t* out_lo;                    // optional low parts of out / raw_out (precise VAE mode: operand = hi + lo)
    bf16_t* raw_lo;
    float* partial;                    // workspace [B, nchunk, G, 2]
    int nchunk, rows_per_chunk;        // from groupnorm_nchunk / groupnorm_rows_per_chunk
    int fuse_finalize;                 // 1 (UNet forward, nchunk <= 128): every block of the apply kernel reduces the per-chunk partials
                                       // itself (one launch fewer; `partial` keeps the RAW sums).  0: gn_finalize_kernel leaves
                                       // (mean, rstd) in chunk 0's slot, which the VAE backward reads.
    double fin_n;                      // set by launch_groupnorm: elements per group
    int apply_rows;                    // set by launch_groupnorm: rows per workgroup of the apply kernel
    float* stats; int stats_ld;        // set by launch_groupnorm: where the apply kernel finds (mean, rstd) per (batch entry, group) in the non-fused form
};
int groupnorm_rows_per_chunk(int HW);
int groupnorm_bwd_rows_per_chunk(int HW);              // chunking of launch_groupnorm_bwd (its own partial-sum layout; one image: the forward's (mean, rstd) sit at offset 0 either way)
void launch_groupnorm(const GroupNormArgs& a, hipStream_t st);
int groupnorm_form(const GroupNormArgs& a);            // host-only: 1 = launch_groupnorm runs the one-launch form, 2 = the two-launch form (reads the shape, in_bf16 and out_lo / raw_lo)
void groupnorm_set_chunk_div(int d);                    // A/B
void groupnorm_set_fused(int on);                       // A/B: 0 = always the two-launch form (rt_op_gemm_debug bit 23)
int groupnorm_nchunk(int HW);

void launch_layernorm(const void* x, int x_f16 /* 0: fp32 rows, 1: fp16 rows (UNet trunk) */, const float* gamma, const float* beta,
                      bf16_t* out, int rows, int C, float eps, hipStream_t st);
void launch_cast_f16_bf16(const f16_t* x, bf16_t* out, size_t n, hipStream_t st);
// FreeU (freeu.hip), in place on fp16 token-major tensors of B streams on an H x W grid: hidden [B, HW, C1] - channels < C1 / 2 times b -
// and skip [B, HW, C2] - the four lowest frequency bins {-1, 0}^2 of every (stream, channel) map scaled by s.  A null pointer, b == 1
// or s == 1 launches nothing for that half; C1, C2 % 8 == 0, 16-byte aligned; the filter needs H, W >= 2 (RT_E_UNSUPPORTED below)
void launch_freeu(f16_t* hidden, int C1, f16_t* skip, int C2, int B, int H, int W, float b, float s, hipStream_t st);
// control.hip (ControlNet): the residual add of a step, the hint embedder's fp32 convolution and the hint's layout change
void launch_control_add(f16_t* skip, size_t skip_stride, int lds, const float* r, size_t r_stride, int ldr, const int* /*host*/ stream,
                        const float* /*host*/ scale, int n, int B, int HW, int C, hipStream_t st);
// pag.hip (perturbed-attention guidance): O[b N + n, c] = VT[c, b N + n] for the n named batch entries (a bf16 transpose in rt_op_attention's
// layouts; N % 8 == 0, leading dimensions multiples of 8), and the fold of a step: eps[s[i]] <- fmaf(rho[i], eps[s[i]] - eps[twin[i]], eps[s[i]])
void launch_identity_attention(const bf16_t* VT, int ldvt, bf16_t* O, int ldo, const int* /*host*/ entry, int n, int B, int H, int N, int DP, hipStream_t st);
void launch_pag_fold(float* eps, int F, int HW, const int* /*host*/ s, const int* /*host*/ twin, const float* /*host*/ rho, int n, hipStream_t st);
void launch_control_conv3(const float* in, const float* w, const float* bias, float* out, f16_t* out16, int Hin, int Win, int CinP, int Cout,
                          int stride, int silu, hipStream_t st);      // fp32 3x3 convolution (pad 1) of one NHWC image, optional SiLU, optional fp16 copy
void launch_control_hint(const float* hint, float* out, int Ch, int CP, size_t HW, hipStream_t st);            // [Ch, HW] f32 -> [HW, CP] f32, pad channels zero
void launch_cast_f32_bf16(const float* x, bf16_t* out, size_t n, hipStream_t st, bf16_t* out_lo = nullptr);
// out[b][n] (+)= sum_k act(a[b][k]) * W[n][k] + bias[n];  B <= 8
void launch_small_linear(const float* a, int lda, const bf16_t* W, int ldw, const float* bias, float* out, int ldo,
                         int B, int N, int K, int silu_in, int accumulate, hipStream_t st);
// one entry per ResnetBlock2D: out[B*first + b*N + n] = bias[n] + sum_k silu(emb[b][k]) * W[n][k]; `first` = prefix sum of N
struct TembEntry { const bf16_t* W; const float* bias; int N; int first; };       // output block of an entry: [B, N] at B * first (batch-independent table)
void launch_temb_all(const float* emb, int lde, float* silu_scratch, const TembEntry* tab, int ntab, int total, int B, int K, float* out,
                     hipStream_t st);
void launch_timestep_embed(const float* t, int n, int dim, float* out, int ldo, hipStream_t st);
void launch_timestep_embed_scalar(float t, int dim, float* out, hipStream_t st);
// CLIP text encoder pieces (text.hip)
void launch_embed(const int* ids, const float* tok, const float* pos, float* out, int rows, int N, int C, int vocab, hipStream_t st);
void launch_activation(const bf16_t* x, bf16_t* out, size_t n, int kind, hipStream_t st);      // 0 quick_gelu, 1 gelu(erf)
void launch_causal_attention(const bf16_t* q, const bf16_t* k, const bf16_t* v, int ld, bf16_t* out, int ldo, int B, int H, int N, int d,
                             float scale, hipStream_t st);
// CLIP vision encoder pieces (vision.hip)
// uint8 RGB [B, S, S, 3] -> bf16 patch rows [B (S/p)^2, Kp], column (c p + ky) p + kx = (u / 255 - mean_c) / std_c, columns 3 p^2 .. Kp zero
void launch_patchify(const uint8_t* img, bf16_t* out, int B, int S, int p, int Kp, const float* mean, const float* stdv, hipStream_t st);
// fp32 trunk [B N, C] = LayerNorm(row 0: cls + pos[0]; row 1 + i: patch[b (N - 1) + i] + pos[1 + i]); C <= 2048
void launch_vit_embed(const float* patch, int ldp, const float* cls, const float* pos, const float* gamma, const float* beta, float* out,
                      int B, int N, int C, float eps, hipStream_t st);
// unmasked self-attention, operands as launch_causal_attention; 1 <= N <= 640, d % 8 == 0, d <= 128
void launch_bidir_attention(const bf16_t* q, const bf16_t* k, const bf16_t* v, int ld, bf16_t* out, int ldo, int B, int H, int N, int d,
                            float scale, hipStream_t st);
// the Resampler's latent attention (resampler.hip): 1 <= Nq <= 16 queries [B Nq, ldq] over 1 <= Nk <= 656 keys / values [B Nk, ldkv]
void launch_latent_attention(const bf16_t* q, int ldq, const bf16_t* k, const bf16_t* v, int ldkv, bf16_t* out, int ldo, int B, int H, int Nq,
                             int Nk, int d, float scale, hipStream_t st);

// weight packing (device side): strided gather fp32/fp16/bf16 -> bf16 (or f32) with scale.
//   dst (r, c) <- scale * src[ srow(r)*s_r + (c / c_inner)*s_co + (c % c_inner)*s_ci ]   (0 where invalid)
//   row_map 0: srow = r
//           1: GEGLU interleave: per 64-row block [32 value rows | 32 gate rows]; gate rows start at rows/2
//           2: head padding: srow = (r / rm_a) * rm_b + r % rm_a, valid iff r % rm_a < rm_b   (rm_a = DP, rm_b = d)
//   column validity: (c % c_inner) < ci_valid
enum { PACK_ROWS_ID = 0, PACK_ROWS_GEGLU = 1, PACK_ROWS_HEADPAD = 2 };
struct PackArgs {
    const void* src; int src_dtype;   // 0 f32, 1 f16, 2 bf16
    void* dst; int dst_f32;
    int rows, cols, ld_dst;
    int row_map, rm_a, rm_b;
    int c_inner, ci_valid;
    long s_r, s_co, s_ci;
    float scale;
    long s_base;                      // constant source offset (flipped conv taps for the backward-data weights)
    int lo_part;                      // 1: store the low part bf16(v - bf16(v)) instead of bf16(v) (precise VAE mode)
};
void launch_pack(const PackArgs& a, hipStream_t st);
// Phase pack of a 3x3 weight behind a nearest-2x up-sample: src [Cout, Cin, 3, 3] (src_dtype as PackArgs) -> dst [phase 2a+b][Cout][tap 2r+c][Cin]
// bf16, W_ab[r][c] = sum of w[ky][kx] over ky in S_a(r), kx in S_b(c) with S_0 = {0}, {1, 2} and S_1 = {0, 1}, {2}: summed in fp32 from
// the SOURCE values in a fixed order, rounded once
void launch_pack_up2(const void* src, int src_dtype, bf16_t* dst, int Cout, int Cin, hipStream_t st);

// NCHW fp32 latents -> NHWC bf16 [B, HW, 8] (channels 4..7 zero), scaled per batch entry
struct PrepArgs {
    const float* src[RT_MAXB];   // each [4, HW]
    float scale[RT_MAXB];
    bf16_t* dst; int B, HW;
};
void launch_prep_latents(const PrepArgs& a, hipStream_t st);

// ---------------------------------------------------------------- VAE decoder forward / backward-data helpers (a13)
// GroupNorm(+SiLU) backward wrt the input: dx = rstd * (dxh - mean_g(dxh) - xh * mean_g(dxh * xh)),
// dxh = dA * silu'(y) * gamma, y = xh*gamma + beta, xh = (x - mean) * rstd; statistics are recomputed from the
// forward pass' partial sums.  `add` (fp32, may be null) is accumulated into the result (residual gradients).
struct GroupNormBwdArgs {
    const void* x; int x_bf16;         // forward input [B, HW, C]
    const bf16_t* dA;                  // gradient wrt the (activated) output [B, HW, C]
    const bf16_t* dA_lo;               // optional low part of dA (precise mode)
    bf16_t* out_bf16_lo;               // optional low part of out_bf16
    const float* fwd_partial;          // forward statistics partials [B, nchunk, G, 2]
    float* bwd_partial;                // workspace [B, nchunk, G, 2]
    const float* gamma; const float* beta; float eps;
    int silu, C, G, B, HW, nchunk, rows_per_chunk;
    const float* add;                  // optional fp32 [B, HW, C]
    float* out;                        // fp32 [B, HW, C] (may be null)
    bf16_t* out_bf16;                  // optional bf16 copy (operand of the next backward conv)
};
void launch_groupnorm_bwd(const GroupNormBwdArgs& a, hipStream_t st);
void launch_gn_finalize(float* partial, int B, int nchunk, int G, double n, float eps, int mode, hipStream_t st);
void launch_transpose_bf16(const bf16_t* in, bf16_t* out, int R, int C, hipStream_t st);        // [R,C] -> [C,R]
void launch_softmax_rows(const float* s, bf16_t* p, int rows, int cols, float scale, hipStream_t st, bf16_t* p_lo = nullptr);
// dS = scale * P o (dP - rowsum(dP o P))   (bf16 out)
void launch_softmax_bwd(const bf16_t* p, const float* dp, bf16_t* ds, int rows, int cols, float scale, hipStream_t st, const bf16_t* p_lo = nullptr,
                        bf16_t* ds_lo = nullptr);
void launch_sumpool2x2(const float* in, float* out, int B, int H, int W, int C, hipStream_t st);   // [B,2H,2W,C] -> [B,H,W,C]
// per pixel: out[pix][0..7] = bf16(W[4x4] * (in[c][pix] * scale) + b), channels 4..7 zero  (post_quant_conv 1x1)
void launch_pq_conv_fwd(const float* lat_nchw, const float* eps_nchw, float c_lat, float c_eps, const float* W, const float* b,
                        bf16_t* out, int HW, hipStream_t st, bf16_t* out_lo = nullptr);
// dlat[c][pix] = sum_o W[o][c] * dz[pix][o] * gscale ;  lat -= dlat * weight * mask_all
void launch_pq_conv_bwd_update(const float* dz, int ldz, const float* W, float gscale, float weight, const float* mask_all,
                               float* lat_nchw, float* grad_out /* optional [4,HW] */, int HW, hipStream_t st);
struct ColorLossArgs {
    const float* img; int ldi;         // decoder output [HWi, ldi] fp32 (3 valid channels), range [-1, 1]
    const float* masks;                // [n, HWi]
    const float* target;               // [n, 3] device
    int n, HWi;
    float* partial;                    // [nblk, n, 4] workspace
    int nblk;
    bf16_t* dimg;                      // [HWi, 8] bf16 gradient wrt the decoder output
    bf16_t* dimg_lo;                   // optional low part (precise mode)
    float* loss_out;                   // [1] optional
};
void launch_color_loss_grad(const ColorLossArgs& a, hipStream_t st);
