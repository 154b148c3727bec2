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
    int step_ref;          // advance lat_ref too
    int blend;             // lat = lat_ref * M[R-1] + lat * (1 - M[R-1]) after the update
    float* noise_pred;     // optional [4, HW]: CFG-combined prediction of the main stream (input of the guidance step)
};

struct IdxList { int v[RT_MAXB]; };

// Everything of one step that depends on the scheduler: which update the epilogue runs and its scalars, computed on the host in fp32
// (step_driver.inl), the history pointers, and the coordinates of the step's noise field z (csrc/philox.h).
//   PLMS:              x' = ca x - cb eps',  eps' the linear multistep combination of mode pndm_mode
//   Euler:             x' = x + eps dsigma                                          dsigma = sigma_{i+1} - sigma_i
//   DPM-Solver++:      x0 = (x - sigma_s0 eps) / alpha_s0;  x' = ratio x - c1 x0 [- c2 inv_r0 (x0 - m1)]          (order 2)
//   Euler ancestral:   x' = x + eps dsigma + z cn                                   dsigma = sigma_down - sigma_i, cn = sigma_up
//   SDE-DPM-Solver++:  x0 as above;  x' = ratio x + c1 x0 [+ c2 inv_r0 (x0 - m1)] + cn z
enum StepSolver { STEP_PLMS, STEP_EULER, STEP_DPM, STEP_EULER_A, STEP_SDE };
struct SolverArgs {
    int solver;            // StepSolver: the instantiation launch_step_epilogue picks
    float dsigma;          // Euler, Euler ancestral
    int pndm_mode;         // PLMS: 0 first call, 1 second call (counter == 1), 2/3/4 = 2/3/4 stored eps
    float ca, cb;
    int push;
    float* cur_sample;     // PLMS: [2][4*HW]
    float* ets[4];         // PLMS history, ets[0] = slot to write the current eps (if push), ets[1..3] = older;
                           // DPM / SDE: ets[0] = slot to write this step's x0, ets[1] = the x0 of the previous step (m1)
    float alpha_s0, sigma_s0;
    float ratio;           // DPM: sigma_p / sigma_s0;            SDE: sigma_p / sigma_s0 exp(-h)
    float c1;              // DPM: alpha_p (exp(-h) - 1);         SDE: alpha_p (1 - exp(-2h))
    float c2;              // 0.5 c1
    float inv_r0;          // 1 / r0, r0 = (lambda_s0 - lambda_s1) / h
    int order;             // 1 or 2
    float cn;              // noise scale: Euler ancestral sigma_up, SDE sigma_p sqrt(1 - exp(-2h))
    unsigned seed_lo, seed_hi;
    int step;              // index into the executed schedule
};
