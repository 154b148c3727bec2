// ipattn_kernel: the image-prompt term of decoupled cross-attention (IP-Adapter), added into the attention output in place:
//   O[b, n, h, :] <- bf16( fp32(O[b, n, h, :]) + sigma_b * sum_j softmax_j(Q[b, n, h, :] . Kip[s_b, j, h, :]) Vip[s_b, j, h, :] ),   j < T_b <= 16
// behind the text attention of attn2 and in front of to_out.  A softmax of its own (two separate softmaxes: the layer is
// attn(Q, K_text, V_text) + sigma attn(Q, K_ip, V_ip)), ONE rounding of the sum.
//
// The launch is bound by bytes: Q is read once, O read and written once, and the 16 keys of a head are 2 * 16 * DP * 2 bytes.  So the keys
// never touch LDS: a wave owns one head and a run of 16-query tiles and keeps K (the A operand of S^T = Kip Q^T, the operand roles of
// cross77_kernel) and V^T (the A operand of O^T = V^T P^T) of that head in registers for all of its tiles - no LDS, no barrier, no wait
// rule to keep.  S^T is ONE 16-key accumulator tile: lane (l15, q4) holds the scores of keys 4 q4 .. 4 q4 + 3 for query l15, which - as
// bf16 behind four zero slots - is the B operand of the 16x16x32 MFMA whose contraction slots 8 q4 + e carry key 4 q4 + e (e < 4) and
// nothing (e >= 4): the V^T fragment of a lane is 8 bytes of a V^T row and four zeros.  The V^T rows of a pair of accumulator tiles are
// taken in cross77_kernel's pi order, so a lane ends with 8 CONSECUTIVE d of its query = the 16-byte column block it loaded Q from: O is
// read and written in 16-byte pieces.  Keys >= T carry score -inf and a zero V^T column (their cached rows are zero in the engine, but
// the kernel does not rely on it).  A d whose image term is exactly 0 - the pad columns d .. DP, whose V^T rows are zero - keeps its bits.
// No atomics, no workgroup depends on another, a query's arithmetic does not depend on the grid: every stream is a function of itself.
#include "xb_common.h"
#include <cmath>

struct IpAttnArgs {
    const bf16_t* Q;  int ldq;   // [*, ldq]   row (row[i] * N + n), head h at column h * DP; pre-scaled by d^-1/2 * log2(e)
    const bf16_t* K;  int ldk;   // [*, ldk]   row (slot[i] * 16 + key), head h at column h * DP
    const bf16_t* VT; int ldvt;  // [H * DP, ldvt]  row (h * DP + d), column (slot[i] * 16 + key)
    bf16_t* O;        int ldo;   // [*, ldo]   row (row[i] * N + n), head h at column h * DP: updated in place
    int nact, H, N, tpw;         // streams in the grid, heads, queries per stream, 16-query tiles per wave
    int row[RT_MAXB], slot[RT_MAXB], count[RT_MAXB];
    float scale[RT_MAXB];
};

template <int KS>                                                     // DP = 32 KS
__global__ __launch_bounds__(256) void ipattn_kernel(IpAttnArgs p) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, q4 = lane >> 4;
    constexpr int DP = 32 * KS;
    const int ntile = (p.N + 15) >> 4, nqb = (ntile + 4 * p.tpw - 1) / (4 * p.tpw);
    int bid = blockIdx.x;
    const int qb = bid % nqb; bid /= nqb;
    const int i = bid % p.nact, h = bid / p.nact;
    const int b = p.row[i], slot = p.slot[i], T = p.count[i];
    const float sigma = p.scale[i];
    // ---- K fragments: key l15, d = 32 ks + 8 q4 .. + 7
    const bf16_t* kp = p.K + (size_t)(slot * 16 + l15) * p.ldk + h * DP + 8 * q4;
    bf16x8 kf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kf[ks] = *(const bf16x8*)(kp + 32 * ks);
    // ---- V^T fragments: accumulator tile dt = 2 s2 + half, row l15 <- d = 32 s2 + 8 (l15 >> 2) + 4 half + (l15 & 3); keys 4 q4 .. + 3
    bf16x8 vf[2 * KS];
    {
        const bf16_t* vp = p.VT + (size_t)(h * DP + 8 * (l15 >> 2) + (l15 & 3)) * p.ldvt + slot * 16 + 4 * q4;
#pragma unroll
        for (int dt = 0; dt < 2 * KS; ++dt) {
            union { uint2 u; bf16_t e[4]; } ld;
            ld.u = *(const uint2*)(vp + (size_t)(32 * (dt >> 1) + 4 * (dt & 1)) * p.ldvt);
            union { bf16_t e[8]; bf16x8 v; } pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) { pk.e[e] = 4 * q4 + e < T ? ld.e[e] : (bf16_t)0; pk.e[4 + e] = 0; }
            vf[dt] = pk.v;
        }
    }
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int tile0 = (qb * 4 + wave) * p.tpw;
    for (int t = 0; t < p.tpw; ++t) {
        const int tile = tile0 + t;
        if (tile >= ntile) break;                                     // wave-uniform
        const int n = tile * 16 + l15;
        const bool valid = n < p.N;                                   // N % 8 == 0: the last tile may hold 8 queries
        const size_t qrow = (size_t)b * p.N + (valid ? n : 0);
        const bf16_t* qp = p.Q + qrow * p.ldq + h * DP + 8 * q4;
        bf16_t* op = p.O + qrow * p.ldo + h * DP + 8 * q4;
        bf16x8 qf[KS], of[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { qf[ks] = valid ? *(const bf16x8*)(qp + 32 * ks) : zero8; of[ks] = valid ? *(const bf16x8*)(op + 32 * ks) : zero8; }
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[ks], s, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = 4 * q4 + e < T ? s[e] : -INFINITY;
        const float mx = xb_rowmax(xb_max(xb_max(s[0], s[1]), xb_max(s[2], s[3])));      // key 0 is always valid: finite
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = __builtin_amdgcn_exp2f(s[e] - mx);             // Q carries d^-1/2 log2 e
        const float c = sigma / xb_rowsum((s[0] + s[1]) + (s[2] + s[3]));
        union { uint32_t u[4]; bf16x8 v; } pf;
        pf.u[0] = pack_bf16x2(s[0], s[1]); pf.u[1] = pack_bf16x2(s[2], s[3]); pf.u[2] = 0; pf.u[3] = 0;
#pragma unroll
        for (int s2 = 0; s2 < KS; ++s2) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[2 * s2], pf.v, z, 0, 0, 0);
            const f32x4 a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[2 * s2 + 1], pf.v, z, 0, 0, 0);
            // (a0, a1) of lane (l15, q4): d = 32 s2 + 8 q4 + [0, 8) of query l15
            union { bf16x8 v; uint32_t u[4]; } oi; oi.v = of[s2];
            f32x4 r0, r1;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float o0 = __uint_as_float(oi.u[e] << 16), o1 = __uint_as_float(oi.u[e] & 0xffff0000u);
                const float o2 = __uint_as_float(oi.u[2 + e] << 16), o3 = __uint_as_float(oi.u[2 + e] & 0xffff0000u);
                r0[2 * e] = a0[2 * e] == 0.f ? o0 : __builtin_fmaf(c, a0[2 * e], o0);
                r0[2 * e + 1] = a0[2 * e + 1] == 0.f ? o1 : __builtin_fmaf(c, a0[2 * e + 1], o1);
                r1[2 * e] = a1[2 * e] == 0.f ? o2 : __builtin_fmaf(c, a1[2 * e], o2);
                r1[2 * e + 1] = a1[2 * e + 1] == 0.f ? o3 : __builtin_fmaf(c, a1[2 * e + 1], o3);
            }
            if (valid) *(bf16x8*)(op + 32 * s2) = xb_pack8(r0, r1);
        }
    }
}

// slot < 0 or scale == 0: that stream is not in the grid and keeps its bytes
void launch_ip_attention(const bf16_t* Q, int ldq, const bf16_t* Kip, int ldk, const bf16_t* VTip, int ldvt, bf16_t* O, int ldo, const int* slot,
                         const int* count, const float* scale, int B, int H, int N, int DP, hipStream_t st) {
    RT_REQUIRE(B >= 1 && B <= RT_MAXB && H >= 1 && N >= 8 && N % 8 == 0, "ip_attention: batch / heads / tokens (N % 8 == 0)");
    RT_REQUIRE(DP % 32 == 0 && DP >= 32 && DP <= 160, "ip_attention: padded head dim must be 32, 64, 96, 128 or 160");
    RT_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 8 == 0, "ip_attention: leading dimensions");
    RT_REQUIRE(ldq >= H * DP && ldk >= H * DP && ldo >= H * DP, "ip_attention: a row holds every head");
    IpAttnArgs a{}; a.Q = Q; a.ldq = ldq; a.K = Kip; a.ldk = ldk; a.VT = VTip; a.ldvt = ldvt; a.O = O; a.ldo = ldo; a.H = H; a.N = N;
    for (int b = 0; b < B; ++b) {
        RT_REQUIRE(std::isfinite(scale[b]), "ip_attention: scale");
        if (slot[b] < 0 || scale[b] == 0.f) continue;
        RT_REQUIRE(count[b] >= 1 && count[b] <= 16, "ip_attention: a slot holds 1 to 16 image tokens");
        RT_REQUIRE((long)(slot[b] + 1) * 16 <= ldvt, "ip_attention: slot beyond the V^T row");
        a.row[a.nact] = b; a.slot[a.nact] = slot[b]; a.count[a.nact] = count[b]; a.scale[a.nact] = scale[b];
        ++a.nact;
    }
    if (a.nact == 0) return;
    const int ntile = cdiv(N, 16);
    a.tpw = ntile >= 64 ? 4 : 1;                                      // keys stay in registers over four tiles where a stream has 1024 tokens or more
    const dim3 grid(cdiv(ntile, 4 * a.tpw) * a.nact * H);
    switch (DP / 32) {
        case 1: hipLaunchKernelGGL((ipattn_kernel<1>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((ipattn_kernel<2>), grid, dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((ipattn_kernel<3>), grid, dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((ipattn_kernel<4>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((ipattn_kernel<5>), grid, dim3(256), 0, st, a); break;
    }
    HIP_CHECK(hipGetLastError());
}
