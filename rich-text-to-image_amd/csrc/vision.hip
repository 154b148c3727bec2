// CLIP vision-encoder pieces that the text encoder's kernels do not cover (transformers' CLIPVisionModelWithProjection, the image
// encoder of IP-Adapter): the patch rows of the patch convolution (which is then one GEMM), the class-token / position / pre-LayerNorm
// front end that leaves the fp32 trunk, and bidirectional self-attention over up to 640 tokens at head dims up to 128 (ViT-H/14: 257
// tokens, d = 80; ViT-bigG/14: 257 tokens, d = 104).  Every contraction with weights still goes through the MFMA GEMM.
#include "xb_common.h"
#include <math.h>

// ---------------------------------------------------------------- patchify
// rows[(b G + gy) G + gx][(c p + ky) p + kx] = bf16((u8[b][gy p + ky][gx p + kx][c] / 255 - mean_c) / std_c), columns 3 p^2 .. Kp zero:
// the flatten order of the conv weight [C, 3, p, p], so that the patch convolution is rows x W^T.
struct PatchifyArgs {
    const uint8_t* img; bf16_t* out;
    int S, p, G, Kp, K;
    float mean[3], inv_std[3];
};
__global__ __launch_bounds__(256) void patchify_kernel(PatchifyArgs a) {
    const int r = blockIdx.x;                                          // (b G + gy) G + gx
    const int gx = r % a.G, gy = (r / a.G) % a.G, b = r / (a.G * a.G);
    const uint8_t* base = a.img + ((size_t)b * a.S + (size_t)gy * a.p) * a.S * 3 + (size_t)gx * a.p * 3;
    const int pp = a.p * a.p;
    for (int col = threadIdx.x; col < a.Kp; col += 256) {
        float v = 0.f;
        if (col < a.K) {
            const int c = col / pp, rem = col - c * pp, ky = rem / a.p, kx = rem - ky * a.p;
            const float u = (float)base[((size_t)ky * a.S + kx) * 3 + c];
            v = (u / 255.f - a.mean[c]) * a.inv_std[c];
        }
        a.out[(size_t)r * a.Kp + col] = f32_to_bf16(v);
    }
}
void launch_patchify(const uint8_t* img, bf16_t* out, int B, int S, int p, int Kp, const float* mean, const float* stdv, hipStream_t st) {
    RT_REQUIRE(B > 0 && S > 0 && p > 0 && S % p == 0, "patchify: the image side must be a positive multiple of the patch side");
    RT_REQUIRE(Kp >= 3 * p * p && Kp % 8 == 0, "patchify: Kp must be a multiple of 8 and >= 3 p^2");
    RT_REQUIRE((long)B * (S / p) * (S / p) < (1l << 24), "patchify: too many patch rows");
    PatchifyArgs a{}; a.img = img; a.out = out; a.S = S; a.p = p; a.G = S / p; a.Kp = Kp; a.K = 3 * p * p;
    for (int c = 0; c < 3; ++c) {
        RT_REQUIRE(std::isfinite(mean[c]) && std::isfinite(stdv[c]) && stdv[c] > 0.f, "patchify: mean / std");
        a.mean[c] = mean[c]; a.inv_std[c] = 1.f / stdv[c];
    }
    hipLaunchKernelGGL(patchify_kernel, dim3(B * a.G * a.G), dim3(256), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------- class token + positions + pre-LayerNorm -> fp32 trunk
// One workgroup per output row (b N + t): e = t == 0 ? cls + pos[0] : patch[b (N - 1) + t - 1] + pos[t]; out = LN(e) in fp32 with
// two-pass statistics (mean, then the centred second moment), like layernorm_kernel.  C <= 2048: 8 values per thread.
#define VE_MAXV 8
__device__ __forceinline__ float ve_block_sum(float v, float* red) {         // sum over the 256 threads, result in every thread
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();                                                           // `red` may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void vit_embed_kernel(const float* __restrict__ patch, int ldp, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ out, int N, int C, float eps) {
    __shared__ float red[4];
    const int r = blockIdx.x, b = r / N, t = r - b * N;
    const float* src = t == 0 ? cls : patch + ((size_t)b * (N - 1) + (t - 1)) * ldp;
    const float* pr = pos + (size_t)t * C;
    float v[VE_MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VE_MAXV; ++i) {
        const int c = threadIdx.x + 256 * i;
        v[i] = c < C ? src[c] + pr[c] : 0.f;
        s += v[i];
    }
    const float mu = ve_block_sum(s, red) / C;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VE_MAXV; ++i) {
        const int c = threadIdx.x + 256 * i;
        const float dlt = v[i] - mu;
        ss += c < C ? dlt * dlt : 0.f;
    }
    const float rs = rsqrtf(ve_block_sum(ss, red) / C + eps);
#pragma unroll
    for (int i = 0; i < VE_MAXV; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < C) out[(size_t)r * C + c] = (v[i] - mu) * rs * gamma[c] + beta[c];
    }
}
void launch_vit_embed(const float* patch, int ldp, const float* cls, const float* pos, const float* gamma, const float* beta, float* out,
                      int B, int N, int C, float eps, hipStream_t st) {
    RT_REQUIRE(B > 0 && N >= 2 && C > 0 && C <= 256 * VE_MAXV, "vit_embed: N >= 2 tokens (class token + patches), C <= 2048");
    RT_REQUIRE(ldp >= C, "vit_embed: a patch row holds C values");
    RT_REQUIRE((long)B * N < (1l << 24), "vit_embed: too many rows");
    hipLaunchKernelGGL(vit_embed_kernel, dim3(B * N), dim3(256), 0, st, patch, ldp, cls, pos, gamma, beta, out, N, C, eps);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------- bidirectional attention
// One workgroup = 64 queries of one (head, image): four waves of one 16-query tile each.  Keys are walked in tiles of 64 staged in LDS:
// K row-major [64][DP + 8] and V transposed [DP][64 + 8] (bf16; the pads keep 16-byte fragment reads of neighbouring rows off the same
// banks), head dim zero-padded to DP = 32 KS in the staging.  25 KB at DP = 128.
//   S^T = K Q^T   (16x16x32 bf16 MFMA, A = K rows, B = Q rows): accumulator tile t of a 32-key block takes its A rows in the order
//                 row 4 a + e <- key 8 a + 4 t + e, so that lane (l15, q4) ends with keys 8 q4 + 4 t + e (e < 4) of query l15: the two
//                 tiles, rounded to bf16, ARE the lane's B fragment (contraction slots 8 q4 .. 8 q4 + 7 = 8 consecutive keys) of
//   O^T = V^T P^T (A = V^T rows = 16 head-dim values, 8 consecutive keys per lane: one 16-byte LDS read).
// Scores are fp32 (q . k accumulated in fp32, then times scale log2 e), the softmax is online in the exp2 domain with fp32 maximum and
// sum (the sum runs over the fp32 probabilities), P is rounded to bf16 for the PV product, O accumulates in fp32 and is divided by the sum
// once at the end: one bf16 rounding of the result.  Keys >= N score -inf (every key tile holds at least one valid key, so the running
// maximum is finite from the first tile on) and their K / V staging is zeros, not memory; query rows >= N are neither read nor stored.
#define BA_KT 64
template <int KS>
__global__ __launch_bounds__(256) void bidir_attn_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                         int ld, bf16_t* __restrict__ out, int ldo, int N, int d, float scale_log2e) {
    constexpr int DP = 32 * KS, KLD = DP + 8, VLD = BA_KT + 8, CH = DP / 8;
    __shared__ __attribute__((aligned(16))) bf16_t ks_[BA_KT * KLD];
    __shared__ __attribute__((aligned(16))) bf16_t vt_[DP * VLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, q4 = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const int n = blockIdx.x * 64 + wave * 16 + l15;
    const bool valid = n < N;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 qf[KS];
    {
        const bf16_t* qp = q + ((size_t)b * N + (valid ? n : 0)) * ld + (size_t)h * d + 8 * q4;
#pragma unroll
        for (int s = 0; s < KS; ++s) qf[s] = (valid && 32 * s + 8 * q4 < d) ? *(const bf16x8*)(qp + 32 * s) : zero8;
    }
    f32x4 o[2 * KS];
#pragma unroll
    for (int dt = 0; dt < 2 * KS; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const int krow = 8 * (l15 >> 2) + (l15 & 3);                       // A row l15 = 4 a + e  <-  key 8 a + 4 t + e of the 32-key block
    for (int k0 = 0; k0 < N; k0 += BA_KT) {
        __syncthreads();                                               // the previous tile's fragments have been read
        for (int i = tid; i < BA_KT * CH; i += 256) {
            const int r = i / CH, c8 = (i - r * CH) * 8;
            const bool in = k0 + r < N && c8 < d;
            const size_t off = ((size_t)b * N + (in ? k0 + r : 0)) * ld + (size_t)h * d + (in ? c8 : 0);
            const bf16x8 kv = in ? *(const bf16x8*)(k + off) : zero8;
            union { bf16x8 v; bf16_t e[8]; } vv;
            vv.v = in ? *(const bf16x8*)(v + off) : zero8;
            *(bf16x8*)(ks_ + r * KLD + c8) = kv;
#pragma unroll
            for (int e = 0; e < 8; ++e) vt_[(c8 + e) * VLD + r] = vv.e[e];
        }
        __syncthreads();
        f32x4 s[BA_KT / 16];
#pragma unroll
        for (int sb = 0; sb < BA_KT / 32; ++sb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const bf16_t* kp = ks_ + (32 * sb + krow + 4 * t) * KLD + 8 * q4;
#pragma unroll
                for (int c = 0; c < KS; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(kp + 32 * c), qf[c], acc, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = k0 + 32 * sb + 8 * q4 + 4 * t + e < N ? acc[e] * scale_log2e : -INFINITY;
                s[2 * sb + t] = acc;
            }
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < BA_KT / 16; ++j) mx = xb_max(mx, xb_max(xb_max(s[j][0], s[j][1]), xb_max(s[j][2], s[j][3])));
        const float mn = xb_max(m, xb_rowmax(mx));                     // finite: key k0 is valid
        const float alpha = __builtin_amdgcn_exp2f(m - mn);            // first tile: exp2(-inf) = 0
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < BA_KT / 16; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[j][e] = __builtin_amdgcn_exp2f(s[j][e] - mn); ps += s[j][e]; }
        l = l * alpha + xb_rowsum(ps);
        m = mn;
#pragma unroll
        for (int dt = 0; dt < 2 * KS; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int sb = 0; sb < BA_KT / 32; ++sb) {
            const bf16x8 pf = xb_pack8(s[2 * sb], s[2 * sb + 1]);
#pragma unroll
            for (int dt = 0; dt < 2 * KS; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(vt_ + (16 * dt + l15) * VLD + 32 * sb + 8 * q4), pf, o[dt], 0, 0, 0);
        }
    }
    if (!valid) return;
    const float inv = 1.f / l;
    bf16_t* op = out + ((size_t)b * N + n) * ldo + (size_t)h * d + 4 * q4;
#pragma unroll
    for (int dt = 0; dt < 2 * KS; ++dt)
        if (16 * dt + 4 * q4 < d) {                                    // d % 8 == 0: a lane's four values are all inside or all outside
            uint2 pk;
            pk.x = pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv); pk.y = pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
            *(uint2*)(op + 16 * dt) = pk;
        }
}
void launch_bidir_attention(const bf16_t* q, const bf16_t* k, const bf16_t* v, int ld, bf16_t* out, int ldo, int B, int H, int N, int d,
                            float scale, hipStream_t st) {
    RT_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535, "bidir attention: batch / heads");
    RT_REQUIRE(N >= 1 && N <= 640, "bidir attention: 1 <= N <= 640 tokens");
    RT_REQUIRE(d >= 8 && d <= 128 && d % 8 == 0, "bidir attention: head dim must be a multiple of 8 and <= 128");
    RT_REQUIRE(ld % 8 == 0 && ldo % 4 == 0 && ld >= H * d && ldo >= H * d, "bidir attention: leading dimensions (ld % 8, ldo % 4, a row holds every head)");
    RT_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0 && (uintptr_t)out % 8 == 0, "bidir attention: q / k / v 16-byte, out 8-byte aligned");
    RT_REQUIRE(std::isfinite(scale), "bidir attention: scale");
    const dim3 grid(cdiv(N, 64), H, B), block(256);
    const float sl = scale * 1.44269504088896340736f;
    switch (cdiv(d, 32)) {
        case 1: hipLaunchKernelGGL((bidir_attn_kernel<1>), grid, block, 0, st, q, k, v, ld, out, ldo, N, d, sl); break;
        case 2: hipLaunchKernelGGL((bidir_attn_kernel<2>), grid, block, 0, st, q, k, v, ld, out, ldo, N, d, sl); break;
        case 3: hipLaunchKernelGGL((bidir_attn_kernel<3>), grid, block, 0, st, q, k, v, ld, out, ldo, N, d, sl); break;
        default: hipLaunchKernelGGL((bidir_attn_kernel<4>), grid, block, 0, st, q, k, v, ld, out, ldo, N, d, sl); break;
    }
    HIP_CHECK(hipGetLastError());
}
