// ControlNet's elementwise kernels (the control copy of the encoder itself runs on the UNet's own GEMM / attention / norm kernels):
//
//   control_add_kernel     skip[b] <- f16(fmaf(scale, r[i], float(skip[b])))    the residual add of a step: entry i of the launch names the
//                          main UNet stream b = stream[i] it adds into and its scale; r [n, HW, ldr] fp32 is the zero convolution's output
//                          of the controlled streams in launch order, skip [B, HW, lds] the main UNet's fp16 skip (or mid output), in place.
//                          One fp32 rounding (the fma), then one to fp16.  A thread owns 8 channels of one token: one 16-byte load and store
//                          of the skip, two 16-byte loads of r.  Streams that are not named are never addressed; no atomics - every
//                          element has one writer, and an entry is a function of itself alone (deterministic, batch invariant).
//   control_conv3_kernel   the hint embedder's 3x3 convolutions in fp32 with the SiLU fused into the epilogue (below)
//   control_hint_kernel    hint [Ch, H W] fp32 planar -> [H W, 8 ceil(Ch / 8)] fp32 token-major, pad channels zero (as the latents are)
#include "common.h"
#include <cmath>

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

struct ControlAddArgs { int stream[RT_MAXB]; float scale[RT_MAXB]; };

__global__ __launch_bounds__(256) void control_add_kernel(f16_t* __restrict__ skip, size_t skip_stride, int lds, const float* __restrict__ r,
                                                          size_t r_stride, int ldr, int HW, int nvec, ControlAddArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)HW * nvec) return;
    const size_t row = i / nvec;
    const int c0 = (int)(i - row * nvec) * 8;
    const float s = a.scale[blockIdx.y];
    f16_t* p = skip + (size_t)a.stream[blockIdx.y] * skip_stride + row * lds + c0;
    const float* q = r + (size_t)blockIdx.y * r_stride + row * ldr + c0;
    const f16x8 v = *(const f16x8*)p;
    const float4 r0 = *(const float4*)q, r1 = *(const float4*)(q + 4);
    const float rr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        // the contract rounds the fma to fp32 and THEN to fp16; the empty asm keeps the fp32 value a value of its own (left alone the
        // compiler folds both into v_fma_mix*_f16, which rounds once - freeu.hip has the same line for the same reason)
        float f = __builtin_fmaf(s, rr[j], (float)v[j]);
        asm volatile("" : "+v"(f));
        o[j] = (f16_t)f;
    }
    *(f16x8*)p = o;
}

void launch_control_add(f16_t* skip, size_t skip_stride, int lds, const float* r, size_t r_stride, int ldr, const int* stream, const float* scale,
                        int n, int B, int HW, int C, hipStream_t st) {
    RT_REQUIRE(n >= 1 && n <= RT_MAXB && B >= 1 && HW >= 1, "control add: stream count / tokens");
    RT_REQUIRE(C >= 8 && C % 8 == 0 && lds >= C && lds % 8 == 0 && ldr >= C && ldr % 4 == 0, "control add: channels must be a multiple of 8, leading dimensions at least C and 16-byte multiples");
    RT_REQUIRE(((uintptr_t)skip & 15) == 0 && ((uintptr_t)r & 15) == 0 && skip_stride % 8 == 0 && r_stride % 4 == 0, "control add: 16-byte alignment");
    RT_REQUIRE(skip_stride >= (size_t)(HW - 1) * lds + C && r_stride >= (size_t)(HW - 1) * ldr + C, "control add: stream stride smaller than a stream");
    ControlAddArgs a{};
    for (int i = 0; i < n; ++i) {
        RT_REQUIRE(stream[i] >= 0 && stream[i] < B, "control add: stream index");
        for (int j = 0; j < i; ++j) RT_REQUIRE(stream[j] != stream[i], "control add: a stream is named twice");
        RT_REQUIRE(std::isfinite(scale[i]), "control add: a scale must be finite");
        a.stream[i] = stream[i]; a.scale[i] = scale[i];
    }
    const int nvec = C / 8;
    const size_t per = (size_t)HW * nvec;
    RT_REQUIRE(per <= ((size_t)1 << 38), "control add: tensor too large");
    control_add_kernel<<<dim3((unsigned)((per + 255) / 256), n), 256, 0, st>>>(skip, skip_stride, lds, r, r_stride, ldr, HW, nvec, a);
    HIP_CHECK(hipGetLastError());
}

// 3x3 convolution, pad 1, stride 1 or 2, of ONE fp32 NHWC image [Hin, Win, CinP] (CinP % 4 == 0, pad channels zero) with fp32 weights
// [Cout][tap][CinP] and bias, optional SiLU: out fp32 NHWC [Hout, Wout, Cout] (+ the same values rounded once to fp16 in out16).  A thread
// owns one output pixel and CV_CO output channels; the taps and channels are summed in one fixed order (tap-major, channels ascending, fmaf),
// so the result is a function of the image alone.  The workgroup's threads share their CV_CO weight rows (uniform addresses) and read
// neighbouring pixels.  Plain fp32 FMAs: the embedder runs once per image and its result feeds every controlled forward at the root of the
// control copy's trunk, where a bf16 rounding per layer was the largest single share of that trunk's distance to the fp32 reference.
#define CV_CO 8
__global__ __launch_bounds__(256) void control_conv3_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ out, f16_t* __restrict__ out16, int Hin, int Win, int CinP, int Hout,
                                                            int Wout, int Cout, int stride, int silu) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hout * Wout) return;
    const int co0 = blockIdx.y * CV_CO;
    const int oy = pix / Wout, ox = pix - oy * Wout;
    const int K = 9 * CinP;
    float acc[CV_CO];
#pragma unroll
    for (int j = 0; j < CV_CO; ++j) acc[j] = bias[co0 + j];
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = oy * stride + tap / 3 - 1, ix = ox * stride + tap % 3 - 1;
        if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;
        const float* xp = in + ((size_t)iy * Win + ix) * CinP;
        const float* wp = w + (size_t)co0 * K + (size_t)tap * CinP;
        for (int ci = 0; ci < CinP; ci += 4) {
            const float4 xv = *(const float4*)(xp + ci);
#pragma unroll
            for (int j = 0; j < CV_CO; ++j) {
                const float4 wv = *(const float4*)(wp + (size_t)j * K + ci);
                acc[j] = __builtin_fmaf(xv.x, wv.x, acc[j]); acc[j] = __builtin_fmaf(xv.y, wv.y, acc[j]);
                acc[j] = __builtin_fmaf(xv.z, wv.z, acc[j]); acc[j] = __builtin_fmaf(xv.w, wv.w, acc[j]);
            }
        }
    }
    float* op = out + (size_t)pix * Cout + co0;
#pragma unroll
    for (int j = 0; j < CV_CO; ++j) {
        if (silu) acc[j] = acc[j] / (1.f + __expf(-acc[j]));
        op[j] = acc[j];
        if (out16) out16[(size_t)pix * Cout + co0 + j] = (f16_t)acc[j];
    }
}

void launch_control_conv3(const float* in, const float* w, const float* bias, float* out, f16_t* out16, int Hin, int Win, int CinP, int Cout,
                          int stride, int silu, hipStream_t st) {
    RT_REQUIRE(Hin >= 1 && Win >= 1 && CinP >= 4 && CinP % 4 == 0 && Cout >= CV_CO && Cout % CV_CO == 0 && (stride == 1 || stride == 2), "control conv: shape");
    RT_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)w & 15) == 0, "control conv: 16-byte alignment");
    const int Hout = stride == 2 ? (Hin + 1) / 2 : Hin, Wout = stride == 2 ? (Win + 1) / 2 : Win;
    RT_REQUIRE((size_t)Hout * Wout <= ((size_t)1 << 30) && Cout / CV_CO <= 65535, "control conv: image too large");
    control_conv3_kernel<<<dim3((unsigned)(((size_t)Hout * Wout + 255) / 256), Cout / CV_CO), 256, 0, st>>>(in, w, bias, out, out16, Hin, Win, CinP, Hout, Wout,
                                                                                                           Cout, stride, silu);
    HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void control_hint_kernel(const float* __restrict__ hint, float* __restrict__ out, int Ch, int CP, size_t HW) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW * CP) return;
    const size_t pix = i / CP;
    const int c = (int)(i - pix * CP);
    out[i] = c < Ch ? hint[(size_t)c * HW + pix] : 0.f;
}

void launch_control_hint(const float* hint, float* out, int Ch, int CP, size_t HW, hipStream_t st) {
    RT_REQUIRE(Ch >= 1 && CP >= Ch && CP % 4 == 0 && HW >= 1, "control hint: channels");
    control_hint_kernel<<<(unsigned)((HW * CP + 255) / 256), 256, 0, st>>>(hint, out, Ch, CP, HW);
    HIP_CHECK(hipGetLastError());
}
