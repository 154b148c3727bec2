// lora_add_kernel: the unmerged low-rank term of a projection, added into that projection's output in place, per stream:
//   T[m, j]  = sum_k X[m, k] A[j, k]                                  bf16 operands, fp32 accumulation (16x16x32 bf16 MFMA)
//   Ts[m, j] = bf16( f_b[j] T[m, j] ),  f_b[j] = scale[b][adapter(j)] aor[j]     the factor is fp32 and meets T BEFORE the one bf16 rounding
//   Y[m, n]  = round_out( float(Y[m, n]) + sum_j Ts[m, j] B[n, j] )   ONE rounding to Y's type
// A = the adapters' down projections stacked along the rank [R, K], B = their up projections side by side [N, R], aor = alpha / rank of
// every rank column (0 on the zero pad columns that bring an adapter's block to a multiple of 16), adapter(j) < 4 the adapter a column
// belongs to.  The per-stream scales travel by value; nothing about a stream is read from the device but its own rows.
//
// The launch is bound by bytes: X is read once, Y read and written once, A and B are small and stay in L2.  So nothing goes through
// LDS and no barrier exists: a wave owns 32 rows of ONE stream and chains both products in registers.  The first product is
// T^T = A X^T (the operand roles of ipattn_kernel): lane (l15, q4) ends with T of row l15 for four rank columns, and the rows of A are
// taken in cross77_kernel's pi order (tile 2 ks + h, row i <- rank column 32 ks + 8 (i >> 2) + 4 h + (i & 3)), so the two tiles of a
// 32-column rank step leave the lane with the 8 CONSECUTIVE columns 32 ks + 8 q4 .. + 7 - which, scaled and rounded, IS the operand
// fragment of the second product's contraction step ks, with no lane movement.  The second product takes the rows of B in the same
// order for the row-major forms (a lane ends with 8 consecutive n of its row: one 16-byte piece of Y), and for the transposed form
// swaps the operand roles (Y^T[n, m]: the lane is n) and takes the 32 ROWS of the wave in that order instead (a lane ends with 8
// consecutive m of its n).  Every global access is 16 bytes.  No atomics, no workgroup waits on another, a row's arithmetic depends on
// neither the grid nor the other streams.  An element whose term is exactly 0 - the head-pad columns, whose rows of B are zero -
// keeps its bits.
//
// lora_geglu_kernel (further down) is the same wave structure for ff.net.0.proj, whose GEGLU epilogue an add behind the GEMM cannot
// reach: the first product and its rounding are shared (lora_ts), the second meets the base GEMM's fp32 pre-activations.
#include "xb_common.h"
#include <cmath>

enum { LORA_BF16 = 0, LORA_BF16_T = 1, LORA_F16 = 2 };
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct LoraArgs {
    const bf16_t* X; int ldx;      // [*, ldx]  row (row[i] + m), K columns
    const bf16_t* A; int lda;      // [R, lda]  down projections, K contiguous
    const bf16_t* B; int ldb;      // [N, ldb]  up projections, R contiguous
    const float* aor;              // [R] alpha / rank per rank column
    const int* adapter;            // [R] adapter (0 .. 3) per rank column
    void* Y; int ldy;              // row-major forms: [*, ldy] row (row[i] + m), N columns; transposed: [N, ldy] column (row[i] + m)
    const float* Z; int ldz;       // lora_geglu_kernel only: [*, ldz] row (row[i] + m), the N packed pre-activations; Y then has N / 2 columns
    int nact, rows, K, N, R, ntile;      // streams in the grid, rows per stream, 64-row tiles per stream
    int row[RT_MAXB];
    float scale[RT_MAXB][4];
};

// The first product and its one rounding, shared by both kernels: T^T = A X^T of the wave's rows mrow[2] of stream i, then Ts = bf16(f T).
// Tile (mt, 2 ks + h): lane (l15, q4) reg e <- row mrow[mt] (of lane l15), rank column 32 ks + 8 q4 + 4 h + e; the fragment ts[mt][ks] of
// contraction step ks holds rank columns 32 ks + 8 q4 .. + 7 of the lane's row.
template <int NKS>                                                    // R <= 32 NKS
static __device__ __forceinline__ void lora_ts(const LoraArgs& p, int i, size_t row0, const int (&mrow)[2], int pi, int q4, bf16x8 (&ts)[2][NKS]) {
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const bf16_t* xp[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) xp[mt] = p.X + (row0 + (mrow[mt] < p.rows ? mrow[mt] : 0)) * p.ldx + 8 * q4;
    const bf16_t* ap[2 * NKS];
    bool aok[2 * NKS];
#pragma unroll
    for (int t = 0; t < 2 * NKS; ++t) {
        const int j = 32 * (t >> 1) + pi + 4 * (t & 1);
        aok[t] = j < p.R;
        ap[t] = p.A + (size_t)(aok[t] ? j : 0) * p.lda + 8 * q4;
    }
    f32x4 acc[2][2 * NKS];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int t = 0; t < 2 * NKS; ++t) acc[mt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += 32) {
        const bool kok = k0 + 8 * q4 < p.K;                           // K % 8 == 0
        bf16x8 xf[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) xf[mt] = kok && mrow[mt] < p.rows ? *(const bf16x8*)(xp[mt] + k0) : zero8;
#pragma unroll
        for (int t = 0; t < 2 * NKS; ++t) {
            const bf16x8 af = kok && aok[t] ? *(const bf16x8*)(ap[t] + k0) : zero8;
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[0], acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[1], acc[1][t], 0, 0, 0);
        }
    }
    const float s0 = p.scale[i][0], s1 = p.scale[i][1], s2 = p.scale[i][2], s3 = p.scale[i][3];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        f32x4 f[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = 32 * ks + 8 * q4 + 4 * h;
            const bool ok = j < p.R;                                  // R % 4 == 0
            const f32x4 ar = ok ? *(const f32x4*)(p.aor + j) : (f32x4){0.f, 0.f, 0.f, 0.f};
            const int4 ad = ok ? *(const int4*)(p.adapter + j) : make_int4(0, 0, 0, 0);
            const int adv[4] = {ad.x, ad.y, ad.z, ad.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) f[h][e] = ar[e] * (adv[e] == 0 ? s0 : adv[e] == 1 ? s1 : adv[e] == 2 ? s2 : s3);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) ts[mt][ks] = xb_pack8(acc[mt][2 * ks] * f[0], acc[mt][2 * ks + 1] * f[1]);
    }
}

template <int NKS, int FORM>                                          // R <= 32 NKS
__global__ __launch_bounds__(128) void lora_add_kernel(LoraArgs p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, q4 = lane >> 4;
    const int i = blockIdx.x / p.ntile, tile = blockIdx.x % p.ntile;
    const int m0 = tile * 64 + wave * 32;
    if (m0 >= p.rows) return;                                         // wave-uniform; the kernel has no barrier
    const size_t row0 = (size_t)p.row[i];
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int pi = 8 * (l15 >> 2) + (l15 & 3);                        // + 4 h: the pi order of a pair of 16-row tiles
    int mrow[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) mrow[mt] = m0 + (FORM == LORA_BF16_T ? pi + 4 * mt : 16 * mt + l15);
    bf16x8 ts[2][NKS];
    lora_ts<NKS>(p, i, row0, mrow, pi, q4, ts);
    // ---- Y += Ts B^T
    if (FORM != LORA_BF16_T) {
        // 32 columns per step: tile h, row i <- n = n0 + pi + 4 h; lane (l15, q4) reg e of tile h = row mrow[mt], n = n0 + 8 q4 + 4 h + e
        for (int n0 = 0; n0 < p.N; n0 += 32) {
            f32x4 d[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) { d[mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; d[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = n0 + pi + 4 * h;
                const bf16_t* bp = p.B + (size_t)(n < p.N ? n : 0) * p.ldb + 8 * q4;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bf16x8 bf = n < p.N && 32 * ks + 8 * q4 < p.R ? *(const bf16x8*)(bp + 32 * ks) : zero8;      // R % 8 == 0
                    d[0][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, ts[0][ks], d[0][h], 0, 0, 0);
                    d[1][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, ts[1][ks], d[1][h], 0, 0, 0);
                }
            }
            const int nc = n0 + 8 * q4;                               // N % 8 == 0
            if (nc >= p.N) continue;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if (mrow[mt] >= p.rows) continue;
                const size_t off = (row0 + mrow[mt]) * p.ldy + nc;
                if (FORM == LORA_BF16) {
                    bf16_t* yp = (bf16_t*)p.Y + off;
                    union { bf16x8 v; uint32_t u[4]; } yi; yi.v = *(const bf16x8*)yp;
                    f32x4 r[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const float y0 = __uint_as_float(yi.u[2 * h + e] << 16), y1 = __uint_as_float(yi.u[2 * h + e] & 0xffff0000u);
                            r[h][2 * e] = d[mt][h][2 * e] == 0.f ? y0 : y0 + d[mt][h][2 * e];
                            r[h][2 * e + 1] = d[mt][h][2 * e + 1] == 0.f ? y1 : y1 + d[mt][h][2 * e + 1];
                        }
                    *(bf16x8*)yp = xb_pack8(r[0], r[1]);
                } else {
                    f16_t* yp = (f16_t*)p.Y + off;
                    f16x8 y = *(const f16x8*)yp;
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (d[mt][h][e] != 0.f) y[4 * h + e] = (f16_t)((float)y[4 * h + e] + d[mt][h][e]);
                    *(f16x8*)yp = y;
                }
            }
        }
    } else {
        // 16 columns per step, the lane is n = n0 + l15: reg e of tile mt = row m0 + 8 q4 + 4 mt + e - 8 consecutive columns of Y^T row n
        const int mc = m0 + 8 * q4;                                   // rows % 8 == 0
        for (int n0 = 0; n0 < p.N; n0 += 16) {
            const int n = n0 + l15;
            const bf16_t* bp = p.B + (size_t)(n < p.N ? n : 0) * p.ldb + 8 * q4;
            f32x4 d[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const bf16x8 bf = n < p.N && 32 * ks + 8 * q4 < p.R ? *(const bf16x8*)(bp + 32 * ks) : zero8;
                d[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ts[0][ks], bf, d[0], 0, 0, 0);
                d[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ts[1][ks], bf, d[1], 0, 0, 0);
            }
            if (n >= p.N || mc >= p.rows) continue;
            bf16_t* yp = (bf16_t*)p.Y + (size_t)n * p.ldy + row0 + mc;
            union { bf16x8 v; uint32_t u[4]; } yi; yi.v = *(const bf16x8*)yp;
            f32x4 r[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float y0 = __uint_as_float(yi.u[2 * mt + e] << 16), y1 = __uint_as_float(yi.u[2 * mt + e] & 0xffff0000u);
                    r[mt][2 * e] = d[mt][2 * e] == 0.f ? y0 : y0 + d[mt][2 * e];
                    r[mt][2 * e + 1] = d[mt][2 * e + 1] == 0.f ? y1 : y1 + d[mt][2 * e + 1];
                }
            *(bf16x8*)yp = xb_pack8(r[0], r[1]);
        }
    }
}

// lora_geglu_kernel: ff.net.0.proj of an adapted stream.  The GEGLU epilogue of the base GEMM is not reachable by an add behind it, so
// the base GEMM of such a stream leaves its fp32 pre-activations Z (bias in; packed column order, per 64-block [32 value | 32 gate]) and
// this kernel finishes the projection:
//   out[m, c] = bf16( (Zv + Dv) * gelu(Zg + Dg) ),   D = Ts B^T                     ONE rounding; gelu = gelu_erf_x2 (common.h), EPI_GEGLU's
// with Ts as above and B [N, R] in the packed row order of the base weight.  One step takes a packed 64-block: the value tiles and the
// gate tiles are the h tiles of two row-major steps 32 columns apart, so lane (l15, q4) ends with the value AND the gate of output
// columns 32 blk + 8 q4 .. + 7 of its row: four float4 of Z in, one 16-byte piece of out.
template <int NKS>
__global__ __launch_bounds__(128) void lora_geglu_kernel(LoraArgs p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, q4 = lane >> 4;
    const int i = blockIdx.x / p.ntile, tile = blockIdx.x % p.ntile;
    const int m0 = tile * 64 + wave * 32;
    if (m0 >= p.rows) return;                                         // wave-uniform; the kernel has no barrier
    const size_t row0 = (size_t)p.row[i];
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int pi = 8 * (l15 >> 2) + (l15 & 3);
    const int mrow[2] = {m0 + l15, m0 + 16 + l15};
    bf16x8 ts[2][NKS];
    lora_ts<NKS>(p, i, row0, mrow, pi, q4, ts);
    // tile (g, h), g = 0 value / 1 gate: row i <- n = n0 + 32 g + pi + 4 h; lane (l15, q4) reg e = row mrow[mt], n = n0 + 32 g + 8 q4 + 4 h + e
    for (int n0 = 0; n0 < p.N; n0 += 64) {                            // N % 64 == 0
        f32x4 d[2][2][2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                d[0][g][h] = (f32x4){0.f, 0.f, 0.f, 0.f}; d[1][g][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
                const bf16_t* bp = p.B + (size_t)(n0 + 32 * g + pi + 4 * h) * p.ldb + 8 * q4;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bf16x8 bf = 32 * ks + 8 * q4 < p.R ? *(const bf16x8*)(bp + 32 * ks) : zero8;      // R % 8 == 0
                    d[0][g][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, ts[0][ks], d[0][g][h], 0, 0, 0);
                    d[1][g][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, ts[1][ks], d[1][g][h], 0, 0, 0);
                }
            }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (mrow[mt] >= p.rows) continue;
            const float* zp = p.Z + (row0 + mrow[mt]) * p.ldz + n0 + 8 * q4;
            f32x4 o[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 v = *(const f32x4*)(zp + 4 * h) + d[mt][0][h], gt = *(const f32x4*)(zp + 32 + 4 * h) + d[mt][1][h];
                const f32x2 a0 = gelu_erf_x2((f32x2){gt[0], gt[1]}), a1 = gelu_erf_x2((f32x2){gt[2], gt[3]});
                o[h] = v * (f32x4){a0.x, a0.y, a1.x, a1.y};
            }
            *(bf16x8*)((bf16_t*)p.Y + (row0 + mrow[mt]) * p.ldy + (n0 >> 1) + 8 * q4) = xb_pack8(o[0], o[1]);
        }
    }
}

template <int NKS>
static void lora_launch_form(const LoraArgs& a, int form, dim3 grid, hipStream_t st) {
    switch (form) {
        case LORA_BF16: hipLaunchKernelGGL((lora_add_kernel<NKS, LORA_BF16>), grid, dim3(128), 0, st, a); break;
        case LORA_BF16_T: hipLaunchKernelGGL((lora_add_kernel<NKS, LORA_BF16_T>), grid, dim3(128), 0, st, a); break;
        default: hipLaunchKernelGGL((lora_add_kernel<NKS, LORA_F16>), grid, dim3(128), 0, st, a); break;
    }
}

// The streams of a launch: one whose four scales are all 0 is not in the grid
static void lora_streams(LoraArgs& a, const int* row, const float* scale /* [B][4] */, int B) {
    for (int b = 0; b < B; ++b) {
        bool on = false;
        for (int l = 0; l < 4; ++l) { RT_REQUIRE(std::isfinite(scale[4 * b + l]), "lora: scale"); on |= scale[4 * b + l] != 0.f; }
        if (!on) continue;
        RT_REQUIRE(row[b] >= 0 && row[b] % 8 == 0, "lora: a stream's row offset (a multiple of 8)");
        a.row[a.nact] = row[b];
        for (int l = 0; l < 4; ++l) a.scale[a.nact][l] = scale[4 * b + l];
        ++a.nact;
    }
}

// A stream whose four scales are all 0 is not in the grid and keeps its bytes; a launch without an adapted stream is not issued.
// Returns the number of streams launched.
int launch_lora_add(const bf16_t* X, int ldx, const bf16_t* down, int ldd, const bf16_t* up, int ldu, const float* aor, const int* adapter, void* Y,
                    int ldy, int form, const int* row, const float* scale /* [B][4] */, int B, int rows, int K, int N, int R, hipStream_t st) {
    RT_REQUIRE(form == LORA_BF16 || form == LORA_BF16_T || form == LORA_F16, "lora_add: output form (0 bf16, 1 bf16 transposed, 2 fp16)");
    RT_REQUIRE(B >= 1 && B <= RT_MAXB && rows >= 8 && rows % 8 == 0, "lora_add: batch / rows per stream (rows % 8 == 0)");
    RT_REQUIRE(K >= 8 && K % 8 == 0 && N >= 8 && N % 8 == 0, "lora_add: K and N must be multiples of 8");
    RT_REQUIRE(R >= 16 && R <= 128 && R % 16 == 0, "lora_add: 16 <= R <= 128 rank columns, a multiple of 16");
    RT_REQUIRE(ldx % 8 == 0 && ldd % 8 == 0 && ldu % 8 == 0 && ldy % 8 == 0, "lora_add: leading dimensions");
    RT_REQUIRE(ldx >= K && ldd >= K && ldu >= R && (form == LORA_BF16_T || ldy >= N), "lora_add: a row holds its columns");
    RT_REQUIRE(((uintptr_t)X | (uintptr_t)down | (uintptr_t)up | (uintptr_t)Y | (uintptr_t)aor | (uintptr_t)adapter) % 16 == 0, "lora_add: 16-byte alignment");
    LoraArgs a{}; a.X = X; a.ldx = ldx; a.A = down; a.lda = ldd; a.B = up; a.ldb = ldu; a.aor = aor; a.adapter = adapter; a.Y = Y; a.ldy = ldy;
    a.rows = rows; a.K = K; a.N = N; a.R = R; a.ntile = cdiv(rows, 64);
    lora_streams(a, row, scale, B);
    for (int i = 0; i < a.nact; ++i) RT_REQUIRE(form != LORA_BF16_T || (long)a.row[i] + rows <= ldy, "lora_add: stream beyond the transposed row");
    if (a.nact == 0) return 0;
    const dim3 grid(a.ntile * a.nact);
    switch (cdiv(R, 32)) {
        case 1: lora_launch_form<1>(a, form, grid, st); break;
        case 2: lora_launch_form<2>(a, form, grid, st); break;
        case 3: lora_launch_form<3>(a, form, grid, st); break;
        default: lora_launch_form<4>(a, form, grid, st); break;
    }
    HIP_CHECK(hipGetLastError());
    return a.nact;
}

// ff.net.0.proj of the adapted streams from the base GEMM's fp32 pre-activations (lora_geglu_kernel): N packed columns in, N / 2 out.
// The same streams rule as launch_lora_add; returns the number of streams launched.
int launch_lora_geglu(const bf16_t* X, int ldx, const bf16_t* down, int ldd, const bf16_t* up, int ldu, const float* aor, const int* adapter, const float* Z,
                      int ldz, bf16_t* out, int ldo, const int* row, const float* scale /* [B][4] */, int B, int rows, int K, int N, int R, hipStream_t st) {
    RT_REQUIRE(B >= 1 && B <= RT_MAXB && rows >= 8 && rows % 8 == 0, "lora_geglu: batch / rows per stream (rows % 8 == 0)");
    RT_REQUIRE(K >= 8 && K % 8 == 0 && N >= 64 && N % 64 == 0, "lora_geglu: K must be a multiple of 8, N (packed value | gate columns) of 64");
    RT_REQUIRE(R >= 16 && R <= 128 && R % 16 == 0, "lora_geglu: 16 <= R <= 128 rank columns, a multiple of 16");
    RT_REQUIRE(ldx % 8 == 0 && ldd % 8 == 0 && ldu % 8 == 0 && ldo % 8 == 0 && ldz % 4 == 0, "lora_geglu: leading dimensions");
    RT_REQUIRE(ldx >= K && ldd >= K && ldu >= R && ldz >= N && ldo >= N / 2, "lora_geglu: a row holds its columns");
    RT_REQUIRE(((uintptr_t)X | (uintptr_t)down | (uintptr_t)up | (uintptr_t)Z | (uintptr_t)out | (uintptr_t)aor | (uintptr_t)adapter) % 16 == 0, "lora_geglu: 16-byte alignment");
    LoraArgs a{}; a.X = X; a.ldx = ldx; a.A = down; a.lda = ldd; a.B = up; a.ldb = ldu; a.aor = aor; a.adapter = adapter; a.Y = out; a.ldy = ldo;
    a.Z = Z; a.ldz = ldz; a.rows = rows; a.K = K; a.N = N; a.R = R; a.ntile = cdiv(rows, 64);
    lora_streams(a, row, scale, B);
    if (a.nact == 0) return 0;
    const dim3 grid(a.ntile * a.nact);
    switch (cdiv(R, 32)) {
        case 1: hipLaunchKernelGGL(lora_geglu_kernel<1>, grid, dim3(128), 0, st, a); break;
        case 2: hipLaunchKernelGGL(lora_geglu_kernel<2>, grid, dim3(128), 0, st, a); break;
        case 3: hipLaunchKernelGGL(lora_geglu_kernel<3>, grid, dim3(128), 0, st, a); break;
        default: hipLaunchKernelGGL(lora_geglu_kernel<4>, grid, dim3(128), 0, st, a); break;
    }
    HIP_CHECK(hipGetLastError());
    return a.nact;
}
