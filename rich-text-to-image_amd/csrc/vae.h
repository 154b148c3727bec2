#pragma once
#include "common.h"
void launch_nhwc4_to_nchw3(const float* in, float* out, int HW, hipStream_t st);   // [HW,4] -> [3,HW]
// VAE encoder (vae_kernels.hip)
void launch_image_in(const float* img, float a, float b, bf16_t* out, bf16_t* out_lo, int HW, hipStream_t st);   // [3,HW] f32 -> a x + b, [HW,8] bf16 (+ lo)
void launch_quant_moments(const float* x, const float* W, const float* b, float* mom, int HW, hipStream_t st);    // [HW,8] -> quant_conv -> [8,HW], logvar clamped
void launch_posterior_sample(const float* mom, const float* noise, float scale, float* lat, int HW, hipStream_t st);   // [8,HW], [4,HW] -> [4,HW]

// ---------------------------------------------------------------- launch arguments of the VAE's kernels
// Built HERE for rt_vae (vae.hip) and for the per-kernel operator entries (rt_op_gemm_hilo, rt_op_vae_groupnorm[_bwd], rt_op_color_loss_grad:
// engine.hip) alike, so that an entry cannot take a route, a chunking or a block count the VAE does not take - and the two cannot drift.
// Dense contraction out = A W^T (+bias) (+res); A_lo / W_lo non-null: the hi / lo contraction (EPI_F32 only)
static inline GemmArgs vae_gemm_args(const bf16_t* A, int lda, const bf16_t* W, int ldw, const float* bias, int M, int N, int K, void* out, int ldo, int epi,
                                     const float* res, int ldres, const bf16_t* A_lo, const bf16_t* W_lo, const bf16_t* zero) {
    GemmArgs g{}; g.A = A; g.W = W; g.bias = bias; g.out = out; g.res = res; g.zero = zero; g.mode = A_DENSE; g.epi = epi;
    g.A_lo = A_lo; g.W_lo = W_lo;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldo = ldo; g.ldres = ldres;
    return g;
}
// 3x3 convolution of ONE image [H, Wd, CinP] (mode A_CONV3 / A_CONV3_UP2 / A_CONV3_S2P0) to N channels; pair_lo as GemmArgs.pair_lo (ask
// gemm_pair_output_ok of the result before launching)
static inline GemmArgs vae_conv_args(const bf16_t* in, int mode, const bf16_t* W, int ldw, const float* bias, int N, int K, int H, int Wd, int CinP, void* out,
                                     int ldo, int epi, const float* res, int ldres, const bf16_t* in_lo, const bf16_t* W_lo, bf16_t* pair_lo,
                                     const bf16_t* zero) {
    int Ho = H, Wo = Wd;
    if (mode == A_CONV3_UP2) { Ho = 2 * H; Wo = 2 * Wd; }
    if (mode == A_CONV3_S2P0) { Ho = H / 2; Wo = Wd / 2; }
    GemmArgs g{}; g.A = in; g.W = W; g.bias = bias; g.out = out; g.res = res; g.zero = zero; g.mode = mode; g.epi = epi;
    g.A_lo = in_lo; g.W_lo = W_lo; g.pair_lo = pair_lo;
    g.M = Ho * Wo; g.N = N; g.K = K; g.ldw = ldw; g.ldo = ldo; g.ldres = ldres; g.rows_per_batch = Ho * Wo; g.Hin = H; g.Win = Wd; g.Cin = CinP;
    g.Hout = Ho; g.Wout = Wo;
    RT_REQUIRE(K == 9 * CinP, "vae conv: weight/input channel mismatch");
    // one image: the 224 x 256 tiles of the GEMM-loop convolution fill the chip only from 256^2 x 256 channels upwards (SD 64^2
    // latent: 13.1 ms per guidance call with every layer on it, 11.3 ms on the patch kernel; SDXL 128^2: 39.7 vs 41.0 the other way)
    // ... and every hi / lo (precise) contraction: as ONE launch of three passes the patch kernel runs the 128-channel layers at 1.6 PF
    // where the GEMM-loop form of the 256-channel layers reaches 0.86 (profiles/r4_vae_precise_kernel_stats.csv)
    g.prefer_patch_conv = in_lo != nullptr || (long)g.M * N < 192L * 224 * 256;
    return g;
}
// GroupNorm forward and backward of the VAE: its own chunk rule (norm.hip), statistics left as (mean, rstd) in stats[b][0][g]
static inline int vae_gn_rows_per_chunk(int HW) { return groupnorm_bwd_rows_per_chunk(HW); }
static inline int vae_gn_nchunk(int HW) { const int rpc = vae_gn_rows_per_chunk(HW); return (HW + rpc - 1) / rpc; }
static inline GroupNormArgs vae_gn_fwd_args(const void* x, bool x_bf16, int C, int G, int B, int HW, const float* gamma, const float* beta, float eps, bool silu,
                                            bf16_t* out, bf16_t* out_lo, bf16_t* raw, bf16_t* raw_lo, float* stats) {
    GroupNormArgs a{}; a.x1 = x; a.in_bf16 = x_bf16; a.C1 = C; a.C2 = 0; a.G = G; a.B = B; a.HW = HW; a.gamma = gamma; a.beta = beta; a.eps = eps;
    a.silu = silu; a.out = out; a.out_lo = out_lo; a.raw_out = raw; a.raw_lo = raw_lo; a.partial = stats; a.nchunk = vae_gn_nchunk(HW);
    a.rows_per_chunk = vae_gn_rows_per_chunk(HW);
    return a;
}
// (the forward's statistics sit at fwd_stats[b][0][g] in ITS chunking, which is the same rule: [B, nchunk, G, 2])
static inline GroupNormBwdArgs vae_gn_bwd_args(const void* x, bool x_bf16, const bf16_t* dA, const bf16_t* dA_lo, const float* fwd_stats, float* bwd_partial,
                                               int C, int G, int B, int HW, const float* gamma, const float* beta, float eps, bool silu, const float* add,
                                               float* out, bf16_t* out_bf16, bf16_t* out_bf16_lo) {
    GroupNormBwdArgs a{}; a.x = x; a.x_bf16 = x_bf16; a.dA = dA; a.dA_lo = dA_lo; a.fwd_partial = fwd_stats; a.bwd_partial = bwd_partial; a.gamma = gamma; a.beta = beta;
    a.eps = eps; a.silu = silu; a.C = C; a.G = G; a.B = B; a.HW = HW; a.nchunk = vae_gn_nchunk(HW); a.rows_per_chunk = vae_gn_rows_per_chunk(HW); a.add = add;
    a.out = out; a.out_bf16 = out_bf16; a.out_bf16_lo = out_bf16_lo;
    return a;
}
// Colour loss + gradient: `partial` holds vae_color_partial_floats(n) floats
#define VAE_COLOR_NBLK 1024
static inline size_t vae_color_partial_floats(int n) { return (size_t)VAE_COLOR_NBLK * n * 4; }
static inline ColorLossArgs vae_color_args(const float* img, int ldi, const float* masks, const float* target, int n, int HWi, float* partial, bf16_t* dimg,
                                           bf16_t* dimg_lo, float* loss_out) {
    ColorLossArgs c{}; c.img = img; c.ldi = ldi; c.masks = masks; c.target = target; c.n = n; c.HWi = HWi;
    c.nblk = VAE_COLOR_NBLK; c.partial = partial; c.dimg = dimg; c.dimg_lo = dimg_lo; c.loss_out = loss_out;
    return c;
}
