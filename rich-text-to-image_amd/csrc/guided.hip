// Guided-prediction pre-pass: CFG rescale (rescale_noise_cfg, models/region_diffusion_sdxl.py:42-53) and v-prediction for every sampler.
// Runs only when the engine's prediction type is v or its rescale phi > 0 (rt_set_prediction); the step epilogue of step.hip (whichever solver) is
// untouched and afterwards reads `gpred` as a plain two-stream eps buffer whose "unconditional" and "text" slots coincide
// (E + g (E - E) = E), so it reproduces the value made here.
//
//   compose:  per pixel the mask combine + CFG of step_combine (step.hip) in its fp32 operation order, every product-sum one fma:
//               text = nt, cfg = nu + g (nt - nu);  while the reference pair is stepped: text_r = eps[s_tref], cfg_r = a + g (b - a)
//             cfg -> gpred[0], cfg_r -> gpred[1]; with phi > 0 each workgroup also leaves (sum x, sum x^2) of the four series as fp64
//             partial sums: lanes (shuffle tree), then the four waves in wave order.  No atomics.
//   finish:   every workgroup adds the partials of all workgroups in block order (fp64; staged through LDS 32 workgroups at a time), std = sqrt((sum x^2 - (sum x)^2 / n) / (n - 1)),
//             n = 4 HW (torch's unbiased default), f = phi std_text / std_cfg + (1 - phi) per stream in fp64, rounded to fp32 once; then
//               m = cfg * f                      (phi > 0)
//               e = fma(cv, m, cx * x)           (v-prediction; x = the stream's own unscaled latent)
//             written to gpred in place.  A zero std_cfg gives inf / NaN as torch does.
// No workgroup waits on another; nothing is allocated; both launches are graph-capturable.
#include "guided.h"

__device__ __forceinline__ float cfg1(float u, float t, float g) { return __fmaf_rn(g, __fsub_rn(t, u), u); }

// (text, cfg) of the main stream and, when the pair is stepped, of the pair; returns has_ref
__device__ __forceinline__ bool guided_combine(const StepArgs& p, int pix, float (&text)[4], float (&cfg)[4], float (&text_r)[4], float (&cfg_r)[4]) {
    auto ld4 = [&](int s) { return *(const float4*)(p.eps + ((size_t)s * p.HW + pix) * 4); };
    const float4 eu = ld4(p.s_uncond), eb = ld4(p.s_base);
    const float euv[4] = {eu.x, eu.y, eu.z, eu.w}, ebv[4] = {eb.x, eb.y, eb.z, eb.w};
    if (p.plain) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { text[c] = ebv[c]; cfg[c] = cfg1(euv[c], ebv[c], p.g); }
    } else {
        float nu[4], nt[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ml = p.masks[((size_t)(p.R - 1) * 4 + c) * p.HW + pix];
            nu[c] = __fmul_rn(euv[c], ml); nt[c] = __fmul_rn(ebv[c], ml);
        }
        for (int r = 0; r < p.R - 1; ++r) {
            const float4 q = ld4(p.s_region[r]);
            const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float m = p.masks[((size_t)r * 4 + c) * p.HW + pix];
                nu[c] = __fmaf_rn(euv[c], m, nu[c]); nt[c] = __fmaf_rn(qv[c], m, nt[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) { text[c] = nt[c]; cfg[c] = cfg1(nu[c], nt[c], p.g); }
    }
    const bool has_ref = p.s_uref >= 0 && p.step_ref;
    if (has_ref) {
        const float4 a = ld4(p.s_uref), b = ld4(p.s_tref);
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) { text_r[c] = bv[c]; cfg_r[c] = cfg1(av[c], bv[c], p.g); }
    }
    return has_ref;
}

__global__ void __launch_bounds__(256) guided_compose_kernel(GuidedArgs q) {
    const StepArgs& p = q.s;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const bool live = pix < p.HW;
    float text[4] = {0.f, 0.f, 0.f, 0.f}, cfg[4] = {0.f, 0.f, 0.f, 0.f}, text_r[4] = {0.f, 0.f, 0.f, 0.f}, cfg_r[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const bool has_ref = guided_combine(p, pix, text, cfg, text_r, cfg_r);
        *(float4*)(q.gpred + (size_t)pix * 4) = make_float4(cfg[0], cfg[1], cfg[2], cfg[3]);
        if (has_ref) *(float4*)(q.gpred + ((size_t)p.HW + pix) * 4) = make_float4(cfg_r[0], cfg_r[1], cfg_r[2], cfg_r[3]);
    }
    if (!(q.phi > 0.f)) return;                                     // uniform over the grid
    // a pixel past the end (and an unstepped pair) contributes zeros
    double s[RT_GUIDED_SERIES];
    const float* series[4] = {text, cfg, text_r, cfg_r};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) { const double x = (double)series[k][c]; a += x; b += x * x; }
        s[2 * k] = a; s[2 * k + 1] = b;
    }
    // lanes: a fixed shuffle tree over the 64 lanes of the wave
#pragma unroll
    for (int k = 0; k < RT_GUIDED_SERIES; ++k)
        for (int off = 32; off >= 1; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    __shared__ double red[4][RT_GUIDED_SERIES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < RT_GUIDED_SERIES; ++k) red[wave][k] = s[k];
    }
    __syncthreads();
    // waves, in wave order
    if (threadIdx.x < RT_GUIDED_SERIES) {
        const int k = threadIdx.x;
        q.partials[(size_t)blockIdx.x * RT_GUIDED_SERIES + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

__global__ void __launch_bounds__(256) guided_finish_kernel(GuidedArgs q) {
    const StepArgs& p = q.s;
    const bool has_ref = p.s_uref >= 0 && p.step_ref;
    __shared__ double tot[RT_GUIDED_SERIES];
    __shared__ float fac[2];
    if (q.phi > 0.f) {
        // the partials of 32 workgroups at a time: one coalesced load of 256 doubles into LDS by the whole workgroup, then eight threads
        // add their series' 32 values in block order - the order (and the bits) of a serial walk over global memory, without its latency
        __shared__ double stage[256];
        const int total = (int)gridDim.x * RT_GUIDED_SERIES;
        double a = 0.0;
        for (int base = 0; base < total; base += 256) {
            const int idx = base + threadIdx.x;
            stage[threadIdx.x] = idx < total ? q.partials[idx] : 0.0;
            __syncthreads();
            if (threadIdx.x < RT_GUIDED_SERIES) {
                const int nb = min(32, (total - base) / RT_GUIDED_SERIES);
                for (int b = 0; b < nb; ++b) a += stage[b * RT_GUIDED_SERIES + threadIdx.x];
            }
            __syncthreads();
        }
        if (threadIdx.x < RT_GUIDED_SERIES) tot[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x < 2) {
            const int st = threadIdx.x;
            float f = st == 0 ? 1.f : 0.f;
            if (st == 0 || has_ref) {
                const double n = 4.0 * (double)p.HW;
                auto sd = [&](int k) { return sqrt((tot[2 * k + 1] - tot[2 * k] * tot[2 * k] / n) / (n - 1.0)); };
                const double phi = (double)q.phi;
                f = (float)(phi * sd(2 * st) / sd(2 * st + 1) + (1.0 - phi));
            }
            fac[st] = f;
            if (blockIdx.x == 0 && q.factors) q.factors[st] = f;
        }
        __syncthreads();
    } else if (blockIdx.x == 0 && threadIdx.x < 2 && q.factors) {
        q.factors[threadIdx.x] = threadIdx.x == 0 || has_ref ? 1.f : 0.f;
    }
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= p.HW) return;
    for (int st = 0; st < (has_ref ? 2 : 1); ++st) {
        float* gp = q.gpred + ((size_t)st * p.HW + pix) * 4;
        const float* x = st == 0 ? p.lat : p.lat_ref;
        const float4 v4 = *(const float4*)gp;
        float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float m = v[c];
            if (q.phi > 0.f) m = __fmul_rn(m, fac[st]);
            if (q.vpred) m = __fmaf_rn(q.cv, m, __fmul_rn(q.cx, x[(size_t)c * p.HW + pix]));
            v[c] = m;
        }
        *(float4*)gp = make_float4(v[0], v[1], v[2], v[3]);
    }
}

void launch_guided_prediction(const GuidedArgs& a, hipStream_t st) {
    const int blocks = cdiv(a.s.HW, 256);
    hipLaunchKernelGGL(guided_compose_kernel, dim3(blocks), dim3(256), 0, st, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(guided_finish_kernel, dim3(blocks), dim3(256), 0, st, a);
    HIP_CHECK(hipGetLastError());
}
