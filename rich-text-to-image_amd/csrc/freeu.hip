// FreeU on the fp16 token-major trunk [B, HW, C] of the up path (the operator of diffusers' apply_freeu / fourier_filter with its fixed
// threshold = 1, restated in closed form; parity with diffusers is unpinned, tests/freeu_ref.py pins the fp64 restatement):
//
//   backbone   x[:, :, c] <- fp16(fp32(x[:, :, c]) * b)                for c < C1 / 2                    (freeu_scale_kernel)
//   skip       out[y, x]  =  sk[y, x] + (s - 1) / HW * Re( sum over (ky, kx) in {-1, 0}^2 of X[ky, kx] e(ky y / H + kx x / W) )
//              X = fftn(sk) over (H, W) per (stream, channel),  e(t) = exp(2 pi i t)                      (freeu_skip_kernel)
//
// The box of the shifted spectrum that fourier_filter scales is exactly those four bins, so no FFT is needed: per (stream, channel) seven
// real sums over the map (sk is real: X[0, 0] is real, the other three bins are complex) and a rank-4 update.  With u = e(y / H),
// v = e(x / W) (bin -1 multiplies by the conjugate of what it reconstructs with):
//   S0 = sum sk            A = sum sk u            Bx = sum sk v            D = sum sk u v
//   corr = S0 + Re(A conj u) + Re(Bx conj v) + Re(D conj(u v))
// evaluated as written - then H = 2 or W = 2 (bin -1 is the Nyquist bin, sin = 0 exactly from sincospif) and odd sides need no special case.
//
// One workgroup owns (stream, slab of FU_CS channels) and walks ALL tokens of it twice: pass 1 accumulates the seven sums, pass 2 re-reads
// the slab (the same thread reads the same tokens: L2 hits for every slab the engine meets) and writes in place.  A slab of 32 channels is
// 64 B per token: 4 lanes of 8 channels, 128 token groups per workgroup (eight waves, four tokens in flight per lane: the walk is bound
// by memory latency, not by arithmetic).  Everything is fp32 with ONE rounding to fp16 at the end; the
// sums run in a fixed order that is a function of (H, W) alone - lane-sequential over tokens tg, tg + 128, ..; a butterfly over the 16
// token groups of a wave; the eight waves left to right - so a stream's result does not depend on the batch, and no atomics are needed.
#include "common.h"

#define FU_THREADS 512
#define FU_CS 32                          // channels per slab
#define FU_LANES (FU_CS / 8)              // lanes per token (16 B each)
#define FU_TG (FU_THREADS / FU_LANES)     // token groups per workgroup
#define FU_UNROLL 4                       // tokens a lane has in flight per trip
#define FU_MAX_SIDE 2048                  // twiddle tables of both axes in LDS: (H + W) float2

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

__global__ __launch_bounds__(FU_THREADS) void freeu_skip_kernel(f16_t* __restrict__ sk, int C, int H, int W, float g /* (s - 1) / HW */) {
    extern __shared__ float2 fu_tw[];                 // [H] e(y / H), then [W] e(x / W): (cos, sin)
    __shared__ float fu_part[FU_THREADS / 64][7][FU_CS];
    const int tid = threadIdx.x, lane = tid % FU_LANES, tg = tid / FU_LANES;
    const int c0 = blockIdx.x * FU_CS + lane * 8;
    const bool live = c0 < C;                         // C % 8 == 0: a lane's 8 channels are all inside or all outside
    const int HW = H * W;
    f16_t* base = sk + (size_t)blockIdx.y * HW * C + c0;
    for (int i = tid; i < H + W; i += FU_THREADS) {
        const float t = i < H ? 2.f * (float)i / (float)H : 2.f * (float)(i - H) / (float)W;
        float sn, cs;
        sincospif(t, &sn, &cs);
        fu_tw[i] = make_float2(cs, sn);
    }
    __syncthreads();
    float acc[7][8];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    if (live) {
        for (int t0 = tg; t0 < HW; t0 += FU_UNROLL * FU_TG) {          // FU_UNROLL loads in flight per lane, accumulated in token order
            f16x8 q[FU_UNROLL];
#pragma unroll
            for (int r = 0; r < FU_UNROLL; ++r) {
                const int t = t0 + r * FU_TG;
                if (t < HW) q[r] = *(const f16x8*)(base + (size_t)t * C);
            }
#pragma unroll
            for (int r = 0; r < FU_UNROLL; ++r) {
                const int t = t0 + r * FU_TG;
                if (t >= HW) break;
                const int y = t / W, x = t - y * W;
                const float2 u = fu_tw[y], v = fu_tw[H + x];
                const float cuv = u.x * v.x - u.y * v.y, suv = u.y * v.x + u.x * v.y;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float a = (float)q[r][j];
                    acc[0][j] += a;
                    acc[1][j] = __builtin_fmaf(a, u.x, acc[1][j]); acc[2][j] = __builtin_fmaf(a, u.y, acc[2][j]);
                    acc[3][j] = __builtin_fmaf(a, v.x, acc[3][j]); acc[4][j] = __builtin_fmaf(a, v.y, acc[4][j]);
                    acc[5][j] = __builtin_fmaf(a, cuv, acc[5][j]); acc[6][j] = __builtin_fmaf(a, suv, acc[6][j]);
                }
            }
        }
    }
    // the 16 token groups of a wave (lanes l, l + 4, ..): butterfly, every lane ends with the same sum
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = acc[k][j];
#pragma unroll
            for (int m = FU_LANES; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
            acc[k][j] = a;
        }
    const int wave = tid / 64;
    if (tid % 64 < FU_LANES) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) fu_part[wave][k][lane * 8 + j] = acc[k][j];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = fu_part[0][k][lane * 8 + j];
#pragma unroll
            for (int w = 1; w < FU_THREADS / 64; ++w) a += fu_part[w][k][lane * 8 + j];
            acc[k][j] = a;
        }
    for (int t0 = tg; t0 < HW; t0 += FU_UNROLL * FU_TG) {
        f16x8 q[FU_UNROLL];
#pragma unroll
        for (int r = 0; r < FU_UNROLL; ++r) {
            const int t = t0 + r * FU_TG;
            if (t < HW) q[r] = *(const f16x8*)(base + (size_t)t * C);
        }
#pragma unroll
        for (int r = 0; r < FU_UNROLL; ++r) {
            const int t = t0 + r * FU_TG;
            if (t >= HW) break;
            const int y = t / W, x = t - y * W;
            const float2 u = fu_tw[y], v = fu_tw[H + x];
            const float cuv = u.x * v.x - u.y * v.y, suv = u.y * v.x + u.x * v.y;
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float corr = acc[0][j];
                corr = __builtin_fmaf(acc[1][j], u.x, corr); corr = __builtin_fmaf(acc[2][j], u.y, corr);
                corr = __builtin_fmaf(acc[3][j], v.x, corr); corr = __builtin_fmaf(acc[4][j], v.y, corr);
                corr = __builtin_fmaf(acc[5][j], cuv, corr); corr = __builtin_fmaf(acc[6][j], suv, corr);
                o[j] = (f16_t)__builtin_fmaf(g, corr, (float)q[r][j]);
            }
            *(f16x8*)(base + (size_t)t * C) = o;
        }
    }
}

// x[row][c] <- fp16(fp32(x[row][c]) * b) for c < half; one thread per 8 channels of a row (the vector that straddles `half` keeps its tail)
__global__ __launch_bounds__(256) void freeu_scale_kernel(f16_t* __restrict__ x, int C, int half, int nvec, size_t total, float b) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / nvec;
    const int c0 = (int)(i - row * nvec) * 8;
    f16_t* p = x + row * C + c0;
    f16x8 q = *(const f16x8*)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        // the contract is (x.float() * b).half(): the product rounded to fp32, then to fp16.  Left to itself the compiler fuses the three
        // steps into v_fma_mix*_f16, which rounds the exact product once and differs in the last bit now and then; the empty asm keeps
        // the fp32 product a value of its own
        float v = (float)q[j] * b;
        asm volatile("" : "+v"(v));
        if (c0 + j < half) q[j] = (f16_t)v;
    }
    *(f16x8*)p = q;
}

void launch_freeu(f16_t* hidden, int C1, f16_t* skip, int C2, int B, int H, int W, float b, float s, hipStream_t st) {
    RT_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "freeu: batch / grid");
    if (hidden && b != 1.f) {
        RT_REQUIRE(C1 >= 8 && C1 % 8 == 0 && ((uintptr_t)hidden & 15) == 0, "freeu: hidden channels must be a multiple of 8, 16-byte aligned");
        const int half = C1 / 2, nvec = cdiv(half, 8);
        const size_t total = (size_t)B * H * W * nvec;
        RT_REQUIRE(total <= ((size_t)1 << 38), "freeu: tensor too large");
        freeu_scale_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(hidden, C1, half, nvec, total, b);
        HIP_CHECK(hipGetLastError());
    }
    if (skip && s != 1.f) {
        if (H < 2 || W < 2) throw rt_error(RT_E_UNSUPPORTED, "freeu: the skip filter needs a grid of at least 2 x 2");
        if (H > FU_MAX_SIDE || W > FU_MAX_SIDE) throw rt_error(RT_E_UNSUPPORTED, "freeu: grid side above 2048");
        RT_REQUIRE(C2 >= 8 && C2 % 8 == 0 && ((uintptr_t)skip & 15) == 0, "freeu: skip channels must be a multiple of 8, 16-byte aligned");
        const float g = (s - 1.f) / (float)(H * W);
        freeu_skip_kernel<<<dim3(cdiv(C2, FU_CS), B), FU_THREADS, (size_t)(H + W) * sizeof(float2), st>>>(skip, C2, H, W, g);
        HIP_CHECK(hipGetLastError());
    }
}
