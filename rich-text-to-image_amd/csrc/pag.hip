// Perturbed-attention guidance (rt_set_pag_layers / rt_set_pag_scales): the two kernels the feature adds.
//
//   pag_identity_kernel    O[b N + n, c] <- VT[c, b N + n] for c < H DP, for the batch entries b the launch names: the attention output of a
//                          perturbed stream at an applied attn1 module is its V, head for head (no Q, no K, no softmax).  A batched bf16
//                          transpose in rt_op_attention's layouts (VT [H DP, ldvt], row h DP + d, column = token; O [B N, ldo], head h at
//                          column h DP; the pad rows d .. DP of V^T are copied like the rest).  A workgroup moves a tile of 64 rows of V^T by
//                          64 tokens through LDS: 16-byte loads along the tokens, 16-byte stores along the channels.  The LDS image is
//                          [64 rows][8 slots of 16 bytes] with slot' = slot ^ (row / 8):
//                            row writes (16 bytes per lane; eight contiguous lanes are served together and hold the eight slots of one
//                              row): a permutation of the row's 128 bytes - all 32 banks once;
//                            column reads (2 bytes per lane; a 32-lane half holds 8 channel groups x 4 neighbouring tokens of one slot):
//                              channel group g reads row 8 g + j, whose slot is (n / 8) ^ g - eight different slots -, and the four tokens
//                              are two dwords of it (a pair shares its dword: a broadcast): 16 banks, each once.
//                          Entries that are not named are never addressed; one writer per element, no atomics: bit-exact by construction.
//   pag_fold_kernel        eps[s] <- fmaf(rho, eps[s] - eps[s'], eps[s]) over the 4 h w fp32 values of a stream, for every (partner s, twin
//                          s', rho = sigma_slot / g) of the launch: after it the two-term guidance u + g (T' - u) is the three-term
//                          u + g (T - u) + sigma (T - P).  Two roundings (the subtraction, the fma).  The twin's slot is read only;
//                          streams that are not named keep their bytes.
#include "common.h"
#include <cmath>

struct PagEntries { int e[RT_MAXB]; };

__global__ __launch_bounds__(256) void pag_identity_kernel(const bf16_t* __restrict__ VT, int ldvt, bf16_t* __restrict__ O, int ldo, PagEntries ent,
                                                           int N, int HD) {
    __shared__ uint4 tile[64 * 8];
    const int b = ent.e[blockIdx.z];
    const int n0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const size_t col0 = (size_t)b * N;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = threadIdx.x + 256 * i, r = q >> 3, s = q & 7;
        const int c = c0 + r, n = n0 + s * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c < HD && n < N) v = *(const uint4*)(VT + (size_t)c * ldvt + col0 + n);      // N % 8 == 0: a chunk is inside the entry or outside
        tile[r * 8 + (s ^ (r >> 3))] = v;
    }
    __syncthreads();
    const unsigned short* th = (const unsigned short*)tile;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = threadIdx.x + 256 * i, g = q & 7, nn = q >> 3;
        const int c = c0 + g * 8, n = n0 + nn;
        if (c >= HD || n >= N) continue;                                                 // H DP % 8 == 0: a channel group likewise
        const int at = ((nn >> 3) ^ g) * 8 + (nn & 7);
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned lo = th[(g * 8 + 2 * j) * 64 + at], hi = th[(g * 8 + 2 * j + 1) * 64 + at];
            w[j] = lo | (hi << 16);
        }
        *(uint4*)(O + (col0 + n) * (size_t)ldo + c) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

void launch_identity_attention(const bf16_t* VT, int ldvt, bf16_t* O, int ldo, const int* entry, int n, int B, int H, int N, int DP, hipStream_t st) {
    RT_REQUIRE(VT && O && entry, "identity attention: null argument");
    RT_REQUIRE(B >= 1 && B <= RT_MAXB && n >= 1 && n <= B && H >= 1 && N >= 8 && N % 8 == 0, "identity attention: batch / entries / heads / tokens (N % 8 == 0)");
    RT_REQUIRE(DP % 32 == 0 && DP >= 32 && DP <= 160, "identity attention: padded head dim must be 32, 64, 96, 128 or 160");
    RT_REQUIRE(ldvt % 8 == 0 && ldo % 8 == 0, "identity attention: leading dimensions must be multiples of 8");
    RT_REQUIRE((long long)ldvt >= (long long)B * N && ldo >= H * DP, "identity attention: a row of V^T holds every entry's tokens, a row of O every head");
    RT_REQUIRE(((uintptr_t)VT & 15) == 0 && ((uintptr_t)O & 15) == 0, "identity attention: 16-byte alignment");
    RT_REQUIRE((long long)H * DP <= 65535LL * 64, "identity attention: too many channels");
    PagEntries ent{};
    for (int i = 0; i < n; ++i) {
        RT_REQUIRE(entry[i] >= 0 && entry[i] < B, "identity attention: entry index");
        for (int j = 0; j < i; ++j) RT_REQUIRE(entry[j] != entry[i], "identity attention: an entry is named twice");
        ent.e[i] = entry[i];
    }
    pag_identity_kernel<<<dim3(cdiv(N, 64), cdiv(H * DP, 64), n), 256, 0, st>>>(VT, ldvt, O, ldo, ent, N, H * DP);
    HIP_CHECK(hipGetLastError());
}

struct PagFoldArgs { int s[RT_MAXB], twin[RT_MAXB]; float rho[RT_MAXB]; };

__global__ __launch_bounds__(256) void pag_fold_kernel(float* __restrict__ eps, size_t per4, PagFoldArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per4) return;
    const float rho = a.rho[blockIdx.y];
    float4* t = (float4*)eps + (size_t)a.s[blockIdx.y] * per4 + i;
    const float4 p = *((const float4*)eps + (size_t)a.twin[blockIdx.y] * per4 + i);
    float4 v = *t;
    v.x = __builtin_fmaf(rho, v.x - p.x, v.x);
    v.y = __builtin_fmaf(rho, v.y - p.y, v.y);
    v.z = __builtin_fmaf(rho, v.z - p.z, v.z);
    v.w = __builtin_fmaf(rho, v.w - p.w, v.w);
    *t = v;
}

// eps [F][HW][4] fp32 (the engine's eps buffer); pair i folds the twin twin[i] into the partner s[i].  A partner is named once and is no
// pair's twin (a twin's slot is read only, so the launch has no order); a twin may serve one partner only.
void launch_pag_fold(float* eps, int F, int HW, const int* s, const int* twin, const float* rho, int n, hipStream_t st) {
    RT_REQUIRE(eps && s && twin && rho, "pag fold: null argument");
    RT_REQUIRE(F >= 2 && F <= RT_MAXB && HW >= 1 && n >= 1 && n <= RT_MAXB, "pag fold: streams / pixels / pairs");
    RT_REQUIRE(((uintptr_t)eps & 15) == 0, "pag fold: 16-byte alignment");
    PagFoldArgs a{};
    for (int i = 0; i < n; ++i) {
        RT_REQUIRE(s[i] >= 0 && s[i] < F && twin[i] >= 0 && twin[i] < F && s[i] != twin[i], "pag fold: stream index");
        RT_REQUIRE(std::isfinite(rho[i]), "pag fold: a ratio must be finite");
        for (int j = 0; j < n; ++j) {
            RT_REQUIRE(j == i || (s[j] != s[i] && twin[j] != twin[i]), "pag fold: a stream is named twice");
            RT_REQUIRE(s[i] != twin[j], "pag fold: a partner is another pair's twin");
        }
        a.s[i] = s[i]; a.twin[i] = twin[i]; a.rho[i] = rho[i];
    }
    const size_t per4 = (size_t)HW;
    RT_REQUIRE(per4 <= ((size_t)1 << 38), "pag fold: tensor too large");
    pag_fold_kernel<<<dim3((unsigned)((per4 + 255) / 256), n), 256, 0, st>>>(eps, per4, a);
    HIP_CHECK(hipGetLastError());
}
