// Step epilogue: region-mask noise composition + CFG + scheduler update + background blend in one launch.
#pragma once
#include "common.h"

struct StepArgs {
    const float* eps;      // [F, HW, 4] (NHWC, 4 channels) UNet outputs of all streams
    const float* masks;    // [R, 4, HW]
    float* lat;            // [4, HW] in/out
    float* lat_ref;        // [4, HW] in/out (may be untouched)
    int HW, R;
    int s_uncond, s_base, s_uref, s_tref;   // stream indices; s_uref < 0 => no reference pair
    int s_region[RT_MAXB];                  // stream of region r (r < R-1); plain mode: R == 0
    float g;
    int plain;             // 1: eps = eps[s_uncond] + g (eps[s_base] - eps[s_uncond]) without masks
    int sched;             // RT_SCHED_EULER / RT_SCHED_PNDM / RT_SCHED_DPMPP_* (the DPM kernel takes its scalars in DpmArgs, the stochastic one in StochArgs)
    int step_ref;          // advance lat_ref too
    float dsigma;          // Euler: sigma_{i+1} - sigma_i
    int pndm_mode;         // 0 first call, 1 second call (counter == 1), 2/3/4 = 2/3/4 stored eps
    float ca, cb;          // PNDM: x_prev = ca * sample - cb * eps'
    float* ets[4];         // PNDM history, ets[0] = slot to write the current eps (if push), ets[1..3] = older;
                           // DPM-Solver++: ets[0] = slot to write this step's x0, ets[1] = the x0 of the previous step (m1)
    float* cur_sample;     // PNDM: [2][4*HW]
    int push;
    int blend;             // lat = lat_ref * M[R-1] + lat * (1 - M[R-1]) after the update
    float* noise_pred;     // optional [4, HW]: CFG-combined prediction of the main stream (input of the guidance step)
};

struct IdxList { int v[RT_MAXB]; };

// DPM-Solver++ (order 1 / 2, midpoint) scalars of one step, computed on the host in fp32 (step_driver.inl: dpm_coeffs):
//   x0 = (x - sigma_s0 eps) / alpha_s0;  x' = ratio x - c1 x0 [- c2 inv_r0 (x0 - m1)]   (order 2)
struct DpmArgs {
    float alpha_s0, sigma_s0;
    float ratio;           // sigma_p / sigma_s0
    float c1;              // alpha_p (exp(-h) - 1)
    float c2;              // 0.5 c1
    float inv_r0;          // 1 / r0, r0 = (lambda_s0 - lambda_s1) / h
    int order;             // 1 or 2
};

// Stochastic samplers (Euler ancestral, SDE-DPM-Solver++ of order 1 / 2): scalars of one step, computed on the host in fp32
// (step_driver.inl: stoch_coeffs), and the coordinates of the step's noise field z (csrc/philox.h).
//   Euler ancestral:   x' = x + eps dsig + z cn                                    dsig = sigma_down - sigma, cn = sigma_up
//   SDE-DPM-Solver++:  x0 = (x - sigma_s0 eps) / alpha_s0;  x' = ratio x + c1 x0 [+ c2 inv_r0 (x0 - m1)] + cn z
struct StochArgs {
    int euler;             // 1: Euler ancestral, 0: SDE-DPM-Solver++
    float dsig;            // Euler ancestral: sigma_down - sigma_i
    float alpha_s0, sigma_s0;
    float ratio;           // sigma_p / sigma_s0 exp(-h)
    float c1;              // alpha_p (1 - exp(-2h))
    float c2;              // 0.5 c1
    float inv_r0;
    int order;             // 1 or 2
    float cn;              // noise scale: sigma_up / sigma_p sqrt(1 - exp(-2h))
    unsigned seed_lo, seed_hi;
    int step;              // index into the executed schedule
};
