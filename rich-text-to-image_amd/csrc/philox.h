// Counter-based N(0, 1) field of the stochastic samplers: Philox4x32-10 (Random123 definition) + Box-Muller, plain C++.
// A value is a pure function of (seed, step, pixel): it does not depend on rank, launch shape or call order, so every rank of a split
// step, the plain pass and the reference stream of the rich pass see the same field without any exchange.
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (pix, step, 0, 0), pix = y * w + x of the latent grid, step = index into the executed schedule
//   the four output words r0..r3 give the four channels of the pixel:
//     u1 = ((r0 >> 8) + 1) 2^-24 in (0, 1], u2 = (r1 >> 8) 2^-24 (both exact in fp32); rad = sqrt(-2 ln u1)
//     channel 0 = rad cos(2 pi u2), channel 1 = rad sin(2 pi u2); channels 2 / 3 the same way from (r2, r3)
// Precise logf / sqrtf / sincospif (no fast-math flag in the Makefile); tests/sde_ref.py restates it in uint64 / fp64.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
    const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ void box_muller(unsigned ra, unsigned rb, float& z0, float& z1) {
    const float u1 = (float)((ra >> 8) + 1u) * 5.9604644775390625e-8f;      // 2^-24
    const float u2 = (float)(rb >> 8) * 5.9604644775390625e-8f;
    const float rad = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(2.f * u2, &s, &c);
    z0 = rad * c; z1 = rad * s;
}

// the four normals of pixel `pix` at step `step`; words (may be null) receives r0..r3
__device__ __forceinline__ void step_noise4(unsigned seed_lo, unsigned seed_hi, unsigned step, unsigned pix, float (&z)[4], unsigned* words = nullptr) {
    unsigned r[4];
    philox4x32_10(pix, step, 0u, 0u, seed_lo, seed_hi, r);
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
    if (words) { words[0] = r[0]; words[1] = r[1]; words[2] = r[2]; words[3] = r[3]; }
}
