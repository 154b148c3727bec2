// Latent attention of IP-Adapter's Resampler (the image projection of the "plus" checkpoints): at most 16 latent queries per image
// attend over up to 656 keys (the image encoder's tokens and the latents themselves), queries and keys / values in different row sets.
// Every K and V row is read exactly once per (image, head) and there is no second query tile to reuse it for, so
//   one workgroup = one (image, head); its four waves split the KEYS: wave w takes the key tiles w, w + 4, ... of 64 keys and keeps its
//   own running maximum m, sum l and accumulator O for all 16 queries; the four partial results are merged through LDS at the end.
// Per key tile, in a wave (the fragment layouts are bidir_attn_kernel's, vision.hip):
//   S^T = K Q^T   16x16x32 bf16 MFMA; the A fragments (K rows) come straight from global memory - a lane's 8 consecutive head-dim values
//                 of one key row are one 16-byte load -; accumulator tile t of a 32-key block takes its A rows in the order
//                 row 4 a + e <- key 8 a + 4 t + e, so that the two tiles of a block, rounded to bf16, are the lane's B fragment of
//   O^T = V^T P^T A = V^T rows: V goes through a per-wave LDS tile [DP][32 + 8] for the transpose, 32 keys at a time.  The tile belongs
//                 to one wave (LDS operations of a wave complete in program order), so the key loop has no workgroup barrier.
// Arithmetic class of bidir_attn_kernel: fp32 scores times scale log2 e, online softmax in the exp2 domain with fp32 maximum and sum (over
// the fp32 probabilities), P rounded to bf16 for the PV product, fp32 accumulation, one division and ONE bf16 rounding of the result.
// Merge, in wave order 0, 1, 2, 3 and without atomics (two launches give the same bits):
//   M = max_w m_w,  f_w = exp2(m_w - M),  L = sum_w l_w f_w,  O = sum_w O_w f_w
// A wave without a key tile (the normal case below 193 keys) carries m = -inf, l = 0, O = 0 and its factor is set to 0, not computed as
// exp2(-inf - (-inf)).  Wave 0 always holds key 0, so M is finite.  Keys >= Nk score -inf and their K / V fragments are zeros, not memory;
// query rows >= Nq are neither read nor stored (their lanes compute on zeros).
#include "xb_common.h"
#include <math.h>

#define LA_KT 64                                                           // keys per tile
#define LA_VH 32                                                           // keys per V^T staging
#define LA_VLD (LA_VH + 8)
static __device__ __forceinline__ void la_wave_sync() {                    // orders this wave's LDS writes and reads (compiler only: the
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                 // hardware keeps a wave's LDS operations in order)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int KS>
__global__ __launch_bounds__(256) void latent_attn_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ k,
                                                          const bf16_t* __restrict__ v, int ldkv, bf16_t* __restrict__ out, int ldo,
                                                          int Nq, int Nk, int d, float scale_log2e) {
    constexpr int DP = 32 * KS, CH = DP / 8;
    constexpr int VT_BYTES = 4 * DP * LA_VLD * 2, MG_BYTES = 4 * (16 * DP + 32) * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[VT_BYTES > MG_BYTES ? VT_BYTES : MG_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, q4 = lane >> 4;
    const int h = blockIdx.x, b = blockIdx.y;
    bf16_t* vt = (bf16_t*)smem + wave * (DP * LA_VLD);                     // this wave's V^T tile [DP][LA_VLD]
    const bool valid = l15 < Nq;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 qf[KS];
    {
        const bf16_t* qp = q + ((size_t)b * Nq + (valid ? l15 : 0)) * ldq + (size_t)h * d + 8 * q4;
#pragma unroll
        for (int s = 0; s < KS; ++s) qf[s] = (valid && 32 * s + 8 * q4 < d) ? *(const bf16x8*)(qp + 32 * s) : zero8;
    }
    f32x4 o[2 * KS];
#pragma unroll
    for (int dt = 0; dt < 2 * KS; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const int krow = 8 * (l15 >> 2) + (l15 & 3);                           // A row l15 = 4 a + e  <-  key 8 a + 4 t + e of the 32-key block
    const bf16_t* kb = k + (size_t)b * Nk * ldkv + (size_t)h * d;
    const bf16_t* vb = v + (size_t)b * Nk * ldkv + (size_t)h * d;
    for (int k0 = wave * LA_KT; k0 < Nk; k0 += 4 * LA_KT) {                // wave-uniform: no workgroup barrier inside
        f32x4 s[LA_KT / 16];
#pragma unroll
        for (int sb = 0; sb < LA_KT / 32; ++sb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const int key = k0 + 32 * sb + krow + 4 * t;
                const bool in = key < Nk;
                const bf16_t* kp = kb + (size_t)(in ? key : 0) * ldkv + 8 * q4;
#pragma unroll
                for (int c = 0; c < KS; ++c) {
                    const bf16x8 kf = (in && 32 * c + 8 * q4 < d) ? *(const bf16x8*)(kp + 32 * c) : zero8;
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[c], acc, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = k0 + 32 * sb + 8 * q4 + 4 * t + e < Nk ? acc[e] * scale_log2e : -INFINITY;
                s[2 * sb + t] = acc;
            }
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < LA_KT / 16; ++j) mx = xb_max(mx, xb_max(xb_max(s[j][0], s[j][1]), xb_max(s[j][2], s[j][3])));
        const float mn = xb_max(m, xb_rowmax(mx));                         // finite: key k0 is valid
        const float alpha = __builtin_amdgcn_exp2f(m - mn);                // first tile: exp2(-inf) = 0
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < LA_KT / 16; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[j][e] = __builtin_amdgcn_exp2f(s[j][e] - mn); ps += s[j][e]; }
        l = l * alpha + xb_rowsum(ps);
        m = mn;
#pragma unroll
        for (int dt = 0; dt < 2 * KS; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int sb = 0; sb < LA_KT / 32; ++sb) {
            la_wave_sync();                                                // the previous staging's fragments have been read
#pragma unroll
            for (int i = lane; i < LA_VH * CH; i += 64) {
                const int r = i / CH, c8 = (i - r * CH) * 8;
                const int key = k0 + 32 * sb + r;
                const bool in = key < Nk && c8 < d;
                union { bf16x8 v; bf16_t e[8]; } vv;
                vv.v = in ? *(const bf16x8*)(vb + (size_t)key * ldkv + c8) : zero8;
#pragma unroll
                for (int e = 0; e < 8; ++e) vt[(c8 + e) * LA_VLD + r] = vv.e[e];
            }
            la_wave_sync();
            const bf16x8 pf = xb_pack8(s[2 * sb], s[2 * sb + 1]);
#pragma unroll
            for (int dt = 0; dt < 2 * KS; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(vt + (16 * dt + l15) * LA_VLD + 8 * q4), pf, o[dt], 0, 0, 0);
        }
    }
    // ---- merge of the four partial results (the V^T tiles are dead: the same LDS)
    __syncthreads();
    float* mo = (float*)smem;                                              // [4][DP][16] partial O, head-dim major
    float* mm = mo + 4 * DP * 16;                                          // [4][16] maxima
    float* ml = mm + 4 * 16;                                               // [4][16] sums
#pragma unroll
    for (int dt = 0; dt < 2 * KS; ++dt)
#pragma unroll
        for (int e = 0; e < 4; ++e) mo[(wave * DP + 16 * dt + 4 * q4 + e) * 16 + l15] = o[dt][e];
    if (q4 == 0) { mm[wave * 16 + l15] = m; ml[wave * 16 + l15] = l; }
    __syncthreads();
    for (int i = tid; i < 16 * (DP / 4); i += 256) {
        const int qy = i & 15, c4 = (i >> 4) * 4;
        if (qy >= Nq || c4 >= d) continue;                                 // d % 8 == 0: four values are all inside or all outside
        const float M = xb_max(xb_max(mm[qy], mm[16 + qy]), xb_max(mm[32 + qy], mm[48 + qy]));       // finite: wave 0 holds key 0
        float L = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = mm[w * 16 + qy];
            const float f = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - M);
            L += ml[w * 16 + qy] * f;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += mo[(w * DP + c4 + e) * 16 + qy] * f;
        }
        const float inv = 1.f / L;
        uint2 pk;
        pk.x = pack_bf16x2(acc[0] * inv, acc[1] * inv); pk.y = pack_bf16x2(acc[2] * inv, acc[3] * inv);
        *(uint2*)(out + ((size_t)b * Nq + qy) * ldo + (size_t)h * d + c4) = pk;
    }
}
void launch_latent_attention(const bf16_t* q, int ldq, const bf16_t* k, const bf16_t* v, int ldkv, bf16_t* out, int ldo, int B, int H, int Nq,
                             int Nk, int d, float scale, hipStream_t st) {
    RT_REQUIRE(q && k && v && out, "latent attention: null pointer");
    RT_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535, "latent attention: batch / heads");
    RT_REQUIRE(Nq >= 1 && Nq <= 16, "latent attention: 1 <= Nq <= 16 queries");
    RT_REQUIRE(Nk >= 1 && Nk <= 656, "latent attention: 1 <= Nk <= 656 keys");
    RT_REQUIRE(d >= 8 && d <= 128 && d % 8 == 0, "latent attention: head dim must be a multiple of 8 and <= 128");
    RT_REQUIRE(ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 4 == 0 && ldq >= H * d && ldkv >= H * d && ldo >= H * d,
               "latent attention: leading dimensions (ldq % 8, ldkv % 8, ldo % 4, a row holds every head)");
    RT_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0 && (uintptr_t)out % 8 == 0, "latent attention: q / k / v 16-byte, out 8-byte aligned");
    RT_REQUIRE(std::isfinite(scale), "latent attention: scale");
    const dim3 grid(H, B), block(256);
    const float sl = scale * 1.44269504088896340736f;
    switch (cdiv(d, 32)) {
        case 1: hipLaunchKernelGGL((latent_attn_kernel<1>), grid, block, 0, st, q, ldq, k, v, ldkv, out, ldo, Nq, Nk, d, sl); break;
        case 2: hipLaunchKernelGGL((latent_attn_kernel<2>), grid, block, 0, st, q, ldq, k, v, ldkv, out, ldo, Nq, Nk, d, sl); break;
        case 3: hipLaunchKernelGGL((latent_attn_kernel<3>), grid, block, 0, st, q, ldq, k, v, ldkv, out, ldo, Nq, Nk, d, sl); break;
        default: hipLaunchKernelGGL((latent_attn_kernel<4>), grid, block, 0, st, q, ldq, k, v, ldkv, out, ldo, Nq, Nk, d, sl); break;
    }
    HIP_CHECK(hipGetLastError());
}
