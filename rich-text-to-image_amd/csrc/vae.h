#pragma once
#include "common.h"
void launch_nhwc4_to_nchw3(const float* in, float* out, int HW, hipStream_t st);   // [HW,4] -> [3,HW]
// VAE encoder (vae_kernels.hip)
void launch_image_in(const float* img, float a, float b, bf16_t* out, bf16_t* out_lo, int HW, hipStream_t st);   // [3,HW] f32 -> a x + b, [HW,8] bf16 (+ lo)
void launch_quant_moments(const float* x, const float* W, const float* b, float* mom, int HW, hipStream_t st);    // [HW,8] -> quant_conv -> [8,HW], logvar clamped
void launch_posterior_sample(const float* mom, const float* noise, float scale, float* lat, int HW, hipStream_t st);   // [8,HW], [4,HW] -> [4,HW]
