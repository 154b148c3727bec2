// Guided-prediction pre-pass (guided.hip): the composed, guided prediction of a step made explicit BEFORE the step epilogue, for the two
// things the fused epilogues cannot do on the fly - a CFG rescale factor (a standard deviation over all 4*HW values of two tensors) and
// the v -> epsilon conversion of a v-prediction model.  Two launches; the epilogue of the schedule's kind then runs unchanged on `gpred`.
#pragma once
#include "step.h"

#define RT_GUIDED_SERIES 8     // per stream (sum, sum of squares) of (text, cfg): main text, main cfg, pair text, pair cfg

struct GuidedArgs {
    StepArgs s;            // eps / masks / lat / lat_ref / HW / R / stream indices / g / plain / step_ref as the epilogue reads them
    float* gpred;          // [2][HW][4] (layout of the eps buffer): slot 0 the main stream's prediction, slot 1 the reference pair's
    double* partials;      // [cdiv(HW, 256)][8] per-workgroup sums (only touched when phi > 0)
    float* factors;        // [2] the rescale factors of the main stream and of the pair (written by workgroup 0; 1 / 0 when unused)
    float phi;             // guidance_rescale; 0: no rescale
    int vpred;             // 1: the model predicts v; eps = cv * m + cx * x
    float cv, cx;
};

void launch_guided_prediction(const GuidedArgs& a, hipStream_t st);
