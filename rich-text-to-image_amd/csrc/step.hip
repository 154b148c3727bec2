// a11 + a12 + a14 of SURVEY.md section 8a: mask-weighted region combine (models/region_diffusion.py:119-132,
// models/region_diffusion_sdxl.py:810-825), classifier-free guidance, scheduler update (third-party
// diffusers 0.18.2 PNDM/PLMS, Euler, DPM-Solver++, Euler ancestral and SDE-DPM-Solver++ restated, see oracle/schedulers.py,
// tests/dpm_solver_ref.py and tests/sde_ref.py) and background blend
// (rd.py:171-173, xl.py:870-872) fused into one elementwise launch over 4*h*w elements.
// The arithmetic follows the reference's fp32 operation order so that the epilogue itself is exact.
// One kernel body, instantiated per solver: the guard that kept the PLMS / Euler kernel's ISA byte-identical (and with it three copies
// of the head and tail) was lifted here; what holds is the latents' bits and the step's time (profiles/step_epilogue_unified.txt).
#include "step.h"
#include "philox.h"
#include "../../include/rtdiff.h"

// mask combine + CFG of the main stream into e and, while the reference pair is stepped, of the pair into er; returns has_ref
__device__ __forceinline__ bool step_combine(const StepArgs& p, int pix, float (&e)[4], float (&er)[4]) {
    auto ld4 = [&](int s) { return *(const float4*)(p.eps + ((size_t)s * p.HW + pix) * 4); };
    const float4 eu = ld4(p.s_uncond), eb = ld4(p.s_base);
    const float euv[4] = {eu.x, eu.y, eu.z, eu.w}, ebv[4] = {eb.x, eb.y, eb.z, eb.w};
    if (p.plain) {
#pragma unroll
        for (int c = 0; c < 4; ++c) e[c] = euv[c] + p.g * (ebv[c] - euv[c]);
    } else {
        float nu[4], nt[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ml = p.masks[((size_t)(p.R - 1) * 4 + c) * p.HW + pix];
            nu[c] = euv[c] * ml; nt[c] = ebv[c] * ml;
        }
        for (int r = 0; r < p.R - 1; ++r) {
            const float4 q = ld4(p.s_region[r]);
            const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float m = p.masks[((size_t)r * 4 + c) * p.HW + pix];
                nu[c] = nu[c] + euv[c] * m; nt[c] = nt[c] + qv[c] * m;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) e[c] = nu[c] + p.g * (nt[c] - nu[c]);
    }
    if (p.noise_pred) {
#pragma unroll
        for (int c = 0; c < 4; ++c) p.noise_pred[(size_t)c * p.HW + pix] = e[c];
    }
    const bool has_ref = p.s_uref >= 0 && p.step_ref;
    if (has_ref) {
        const float4 a = ld4(p.s_uref), b = ld4(p.s_tref);
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) er[c] = av[c] + p.g * (bv[c] - av[c]);
    }
    return has_ref;
}
// background blend + store of the stepped streams
__device__ __forceinline__ void step_store(const StepArgs& p, int pix, const float (&newv)[2][4], bool has_ref) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const size_t li = (size_t)c * p.HW + pix;
        float l = newv[0][c];
        const float lr = has_ref ? newv[1][c] : p.lat_ref[li];
        if (p.blend) {
            const float ml = p.masks[((size_t)(p.R - 1) * 4 + c) * p.HW + pix];
            l = lr * ml + l * (1.f - ml);
        }
        p.lat[li] = l;
        if (has_ref) p.lat_ref[li] = lr;
    }
}
// One element of one stream through solver S, in diffusers' fp32 operation order.  hi = the element's index in the stream's half of a
// history slot.  PLMS keeps its eps history in ets[0..3] and the warm-up sample in cur_sample; DPM / SDE write this step's x0 to ets[0]
// and read m1 (the stream's x0 of the previous step) from ets[1] in the same pass.
template <int S>
__device__ __forceinline__ float step_update(const SolverArgs& d, float sample, float ep, float z, size_t hi) {
    if constexpr (S == STEP_PLMS) {
        if (d.push) d.ets[0][hi] = ep;
        if (d.pndm_mode == 0) { d.cur_sample[hi] = sample; }
        else if (d.pndm_mode == 1) { ep = (ep + d.ets[1][hi]) / 2.f; sample = d.cur_sample[hi]; }
        else if (d.pndm_mode == 2) { ep = (3.f * ep - d.ets[1][hi]) / 2.f; }
        else if (d.pndm_mode == 3) { ep = (23.f * ep - 16.f * d.ets[1][hi] + 5.f * d.ets[2][hi]) / 12.f; }
        else { ep = (1.f / 24.f) * (55.f * ep - 59.f * d.ets[1][hi] + 37.f * d.ets[2][hi] - 9.f * d.ets[3][hi]); }
        {
            // pinned to three roundings (two products, a subtraction) in every element: the bits the separate PLMS / Euler kernel gave,
            // whose compiler happened not to fuse this line.  Left to the compiler, this body fuses some elements and not others; the
            // fp64 tests tolerate either form, the pin keeps the latents' bits
#pragma clang fp contract(off)
            return d.ca * sample - d.cb * ep;
        }
    } else if constexpr (S == STEP_EULER) {
        // pred_x0 = x - sigma*eps; derivative = (x - pred_x0)/sigma; x += derivative * dsigma  (gamma = 0)
        return sample + ep * d.dsigma;
    } else if constexpr (S == STEP_EULER_A) {
        return sample + ep * d.dsigma + z * d.cn;
    } else {
        const float x0 = (sample - d.sigma_s0 * ep) / d.alpha_s0;
        float v;
        if constexpr (S == STEP_DPM) {
            v = d.ratio * sample - d.c1 * x0;
            if (d.order == 2) v = v - d.c2 * (d.inv_r0 * (x0 - d.ets[1][hi]));
        } else {
            v = d.ratio * sample + d.c1 * x0;
            if (d.order == 2) v = v + d.c2 * (d.inv_r0 * (x0 - d.ets[1][hi]));
        }
        d.ets[0][hi] = x0;
        if constexpr (S == STEP_SDE) v = v + d.cn * z;
        return v;
    }
}
// The stochastic solvers draw one Philox call per pixel for the four channels' normals of this step; the SAME values go to the main and
// the reference latents, so streams that are equal before the step are equal after it and the reference stream of a rich pass sees the
// noise the plain pass saw.
template <int S>
__global__ void step_epilogue_kernel(StepArgs p, SolverArgs d) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= p.HW) return;
    float e[4], er[4];
    const bool has_ref = step_combine(p, pix, e, er);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (S == STEP_EULER_A || S == STEP_SDE) step_noise4(d.seed_lo, d.seed_hi, (unsigned)d.step, (unsigned)pix, z);
    float newv[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (s == 1 && !has_ref) break;
        const float* x = s == 0 ? p.lat : p.lat_ref;
        const float* ee = s == 0 ? e : er;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const size_t li = (size_t)c * p.HW + pix;
            newv[s][c] = step_update<S>(d, x[li], ee[c], z[c], (size_t)s * 4 * p.HW + li);
        }
    }
    step_store(p, pix, newv, has_ref);
}
// The field alone (rt_op_step_noise): out [4, HW] fp32, words [HW, 4] or null
__global__ void step_noise_kernel(unsigned seed_lo, unsigned seed_hi, int step, int HW, float* out, unsigned* words) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= HW) return;
    float z[4];
    step_noise4(seed_lo, seed_hi, (unsigned)step, (unsigned)pix, z, words ? words + (size_t)pix * 4 : nullptr);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[(size_t)c * HW + pix] = z[c];
}
template <int S>
static void launch_step_solver(const StepArgs& a, const SolverArgs& d, hipStream_t st) {
    hipLaunchKernelGGL(step_epilogue_kernel<S>, dim3(cdiv(a.HW, 256)), dim3(256), 0, st, a, d);
    HIP_CHECK(hipGetLastError());
}
void launch_step_epilogue(const StepArgs& a, const SolverArgs& d, hipStream_t st) {
    switch (d.solver) {
    case STEP_PLMS: return launch_step_solver<STEP_PLMS>(a, d, st);
    case STEP_EULER: return launch_step_solver<STEP_EULER>(a, d, st);
    case STEP_DPM: return launch_step_solver<STEP_DPM>(a, d, st);
    case STEP_EULER_A: return launch_step_solver<STEP_EULER_A>(a, d, st);
    case STEP_SDE: return launch_step_solver<STEP_SDE>(a, d, st);
    }
    RT_REQUIRE(false, "step epilogue: no such solver");
}
void launch_step_noise(unsigned long long seed, int step, int HW, float* out, unsigned* words, hipStream_t st) {
    hipLaunchKernelGGL(step_noise_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, st, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), step, HW, out,
                       words);
    HIP_CHECK(hipGetLastError());
}

// emb[b][c] = base[c] + table[idx[b]][c]
__global__ void gather_add_rows_kernel(const float* base, const float* table, IdxList idx, float* out, int B, int C) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * C; i += gridDim.x * blockDim.x) {
        const int b = i / C, c = i % C;
        out[i] = base[c] + table[(size_t)idx.v[b] * C + c];
    }
}
void launch_gather_add_rows(const float* base, const float* table, const int* idx, float* out, int B, int C, hipStream_t st) {
    IdxList l{}; for (int b = 0; b < B; ++b) l.v[b] = idx[b];
    hipLaunchKernelGGL(gather_add_rows_kernel, dim3(cdiv(B * C, 256)), dim3(256), 0, st, base, table, l, out, B, C);
    HIP_CHECK(hipGetLastError());
}

// out[b] = sc[b] + hres[src[b]]   (out may alias sc).  sc / out are fp16 trunk tensors, hres is the fp32 residual branch: the sum is
// rounded once, exactly like the fused epilogue of a resnet without injection (a stream keeps its bits whether or not another
// stream of the batch injects).
__global__ void inject_add_kernel(f16_t* out, const f16_t* sc, const float* hres, IdxList src, size_t per_batch4) {
    const int b = blockIdx.y;
    const uint2* s4 = (const uint2*)sc + (size_t)b * per_batch4;
    const float4* h4 = (const float4*)hres + (size_t)src.v[b] * per_batch4;
    uint2* o4 = (uint2*)out + (size_t)b * per_batch4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per_batch4; i += (size_t)gridDim.x * blockDim.x) {
        const uint2 a = s4[i]; const float4 h = h4[i];
        const f16_t* ah = (const f16_t*)&a;
        uint2 o; f16_t* oh = (f16_t*)&o;
        oh[0] = (f16_t)(h.x + (float)ah[0]); oh[1] = (f16_t)(h.y + (float)ah[1]); oh[2] = (f16_t)(h.z + (float)ah[2]); oh[3] = (f16_t)(h.w + (float)ah[3]);
        o4[i] = o;
    }
}
void launch_inject_add(f16_t* out, const f16_t* sc, const float* hres, const int* src, int B, size_t per_batch, hipStream_t st) {
    IdxList l{}; for (int b = 0; b < B; ++b) l.v[b] = src[b];
    const size_t n4 = per_batch / 4;
    int gx = (int)((n4 + 255) / 256); if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(inject_add_kernel, dim3(gx, B), dim3(256), 0, st, out, sc, hres, l, n4);
    HIP_CHECK(hipGetLastError());
}

// [B, HW, 4] -> [B, 4, HW]
__global__ void nhwc4_to_nchw_kernel(const float* in, float* out, int B, int HW) {
    const size_t n = (size_t)B * HW;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / HW, pix = i % HW;
        const float4 v = ((const float4*)in)[i];
        float* o = out + b * 4 * HW + pix;
        o[0] = v.x; o[HW] = v.y; o[2 * (size_t)HW] = v.z; o[3 * (size_t)HW] = v.w;
    }
}
void launch_nhwc4_to_nchw(const float* in, float* out, int B, int HW, hipStream_t st) {
    hipLaunchKernelGGL(nhwc4_to_nchw_kernel, dim3(cdiv(B * HW, 256)), dim3(256), 0, st, in, out, B, HW);
    HIP_CHECK(hipGetLastError());
}

// trace seam (rt_unet_forward_trace): the fp16 trunk [B, HW, C] as fp32 [B, C, HW]; one output element per thread, stores coalesced along HW
__global__ void trace_f16_nhwc_to_nchw_kernel(const f16_t* in, float* out, size_t n, int C, int HW) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i % HW, bc = i / HW, c = bc % C, b = bc / C;
        out[i] = (float)in[(b * HW + pix) * C + c];
    }
}
void launch_trace_f16_nhwc_to_nchw(const f16_t* in, float* out, int B, int C, int HW, hipStream_t st) {
    const size_t n = (size_t)B * C * HW;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(trace_f16_nhwc_to_nchw_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, in, out, n, C, HW);
    HIP_CHECK(hipGetLastError());
}

// one prompt: its rows_valid embedding rows as bf16, zeros behind them up to the rows_out rows the prompt owns in the K / V^T caches
__global__ void pad_ctx_kernel(const float* ctx, bf16_t* out, int rows_valid, int rows_out, int D) {
    const size_t n = (size_t)rows_out * D;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = i < (size_t)rows_valid * D ? f32_to_bf16(ctx[i]) : (bf16_t)0;
}
void launch_pad_ctx(const float* ctx, bf16_t* out, int rows_valid, int rows_out, int D, hipStream_t st) {
    hipLaunchKernelGGL(pad_ctx_kernel, dim3(cdiv(rows_out * D, 256)), dim3(256), 0, st, ctx, out, rows_valid, rows_out, D);
    HIP_CHECK(hipGetLastError());
}

// lat = lat_ref * M + lat * (1 - M)   (rd.py:171-173, xl.py:870-872) as a separate launch when colour guidance has to run
// between the scheduler step and the blend
__global__ void background_blend_kernel(float* lat, const float* lat_ref, const float* m, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) lat[i] = lat_ref[i] * m[i] + lat[i] * (1.f - m[i]);
}
void launch_background_blend(float* lat, const float* lat_ref, const float* mask_last, int n, hipStream_t st) {
    hipLaunchKernelGGL(background_blend_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, lat, lat_ref, mask_last, n);
    HIP_CHECK(hipGetLastError());
}

// Image start and source pinning (rt_noise_latents / rt_source_blend): kernels of their own, nothing of the step epilogues changes.
// x0, noise [4, HW]; keep [HW], one value per pixel for all four channels.  fp32 operation order, every line one rounding:
//   p = a * x0
//   s = fma(b, noise, p)                        the source at level (a, b)
// noise_latents:  lat = lat_ref = s
// source_blend:
//   q = 1 - keep
//   r = q * lat
//   lat = fma(keep, s, r)
// keep == 0 leaves lat's bits alone (fma(0, s, 1 * lat)); keep == 1 at the level (1, 0) gives x0's bits (fma(1, fma(0, noise, x0), 0 * lat)).
__global__ void noise_latents_kernel(float* lat, float* lat_ref, const float* x0, const float* noise, float a, float b, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = __fmaf_rn(b, noise[i], __fmul_rn(a, x0[i]));
    lat[i] = s; lat_ref[i] = s;
}
__global__ void source_blend_kernel(float* lat, const float* x0, const float* noise, const float* keep, float a, float b, int HW) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * HW) return;
    const float k = keep[i % HW];
    const float s = __fmaf_rn(b, noise[i], __fmul_rn(a, x0[i]));
    const float r = __fmul_rn(__fsub_rn(1.f, k), lat[i]);
    lat[i] = __fmaf_rn(k, s, r);
}
void launch_noise_latents(float* lat, float* lat_ref, const float* x0, const float* noise, float a, float b, int n, hipStream_t st) {
    hipLaunchKernelGGL(noise_latents_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, lat, lat_ref, x0, noise, a, b, n);
    HIP_CHECK(hipGetLastError());
}
void launch_source_blend(float* lat, const float* x0, const float* noise, const float* keep, float a, float b, int HW, hipStream_t st) {
    hipLaunchKernelGGL(source_blend_kernel, dim3(cdiv(4 * HW, 256)), dim3(256), 0, st, lat, x0, noise, keep, a, b, HW);
    HIP_CHECK(hipGetLastError());
}
