// bb_policy_wide.hip -- fused policy inference on gfx950 for the observation
// rows of the 2v2 to 5v5 games: IN = 184, 264, 344 or 424 floats -> RunningMeanStd
// -> Linear(IN, 32) + LayerNorm + ReLU -> Linear(32, 32) + LayerNorm + ReLU ->
// heads -> per-bucket argmax or sample, log-prob, value (bb_policy.h has the row
// math, bb_policy_wide.h the layer-1 order and the host executor).
//
// k_policy (bb_policy.hip) keeps W1 in registers: 64 per lane at 128 inputs, 212
// at 424.  Here the weights live in LDS, once per workgroup:
//   w1[32][S], S = 32 NC + 4 floats, NC = ceil(IN / 32); columns IN.. are zero.
//       Lane (c, q) reads W1[16t + c][32v + 8q ..+7] as two ds_read_b128; S / 4 is
//       odd (49, 73, 89, 113), so the 16 lanes of a quarter cover the 64 banks once.
//   norm[2][32 NC]   obs_mean, obs_inv (broadcast reads)
//   w2, wh, cst      PolicyLdsWeights' images of layer 2, the heads, the constants
//   tile[16][33], BucketLds<16> per wave
// 25 to 58 KB of W1 beside 35 KB of per-wave tiles: one workgroup of 12 waves per
// CU (3 per SIMD), 16-row tiles per wave in a grid-stride loop.
//
// Layer 1 on v_mfma_f32_16x16x4_f32, the row streamed in chunks of 32 floats:
// chunk v gives lane (c, q) floats 32v + 8q ..+7 of row row0 + c -- two aligned
// 16-byte global loads, 128 contiguous bytes per row and chunk over the four
// quarters.  IN is a multiple of 8, so in the last chunk (24 or 8 floats) a
// quarter is wholly inside the row or wholly outside; outside it loads nothing of
// its own (it re-reads the row's first floats) and feeds x = 0 against W1 = 0.
// A lane holds three chunks of 8 floats: chunk v under its normalisation and
// MFMAs, v + 1 and v + 2 in flight; under the last two chunks of a tile the
// loads in flight are the wave's next tile's first two.  A row past the end
// reads the tensor's last row instead (never written out).
// Per chunk 8 k-steps for each output half (columns c and c + 16): 8 NC = 48,
// 72, 88, 112 steps.  Chains: A = even chunks, B = odd chunks, per half, all from
// zero, four independent accumulators; h1 = (A + B) + b1 (bb_policy_wide.h).
// After layer 1: ln_relu_to_tile, policy_tail_lds and bucket_pass_spread of
// bb_policy_dev.h, as k_policy_wg / k_step_ppo run them.
#include <hip/hip_runtime.h>
#include "bb_launch.h"
#include "bb_policy_dev.h"
#include "bb_policy_wide.h"

namespace bb {

#ifndef BB_PWIDE_WAVES
#define BB_PWIDE_WAVES 12  // 3 per SIMD
#endif
constexpr int PWIDE_WAVES = BB_PWIDE_WAVES;

template <int IN>
struct PolicyWideLds {
    static constexpr int NC = pol_wide_chunks(IN), S = 32 * NC + 4;
    float w1[32][S];
    float norm[2][32 * NC];
    float w2[4][32][PWG_P2];  // W2[n][8q + j]
    float wh[4][32][PWG_P2];  // head_w[n][8q + j]
    float cst[7][32];         // b1, ln1_w, ln1_b, b2, ln2_w, ln2_b, head_b
    float tile[PWIDE_WAVES][16][33];
    BucketLds<16> bl[PWIDE_WAVES];
};
static_assert(sizeof(PolicyWideLds<424>) <= 160 * 1024, "one workgroup's LDS");

// A lane's 8 floats of one chunk.
struct WideChunk {
    float4 lo, hi;
};

template <int IN, int STOCH>
__global__ __launch_bounds__(64 * PWIDE_WAVES) void k_policy_wide(const PolicyArgs a)
{
    using Lds = PolicyWideLds<IN>;
    constexpr int NC = Lds::NC;
    static_assert(pol_wide_width(IN) && NC >= 3, "observation width");
    __shared__ __attribute__((aligned(16))) Lds L;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int nw = (int)(blockDim.x >> 6);
    const int64_t tiles = (a.rows + 15) / 16;
    const int64_t tw0 = (int64_t)blockIdx.x * nw + wave, tstride = (int64_t)gridDim.x * nw;
    // the last chunk's quarters inside the row
    const bool tail_in = 32 * (NC - 1) + 8 * q < IN;
    // chunk v of the tile at row0: always a read inside the tensor (the last
    // row for rows past the end, float 0.. for a quarter past the row's end)
    auto load_chunk = [&](int64_t row0, int v) {
        int64_t r = row0 + c;
        r = r < a.rows ? r : a.rows - 1;
        const int off = (v < NC - 1 || tail_in) ? 32 * v + 8 * q : 0;
        const float4 *src = (const float4 *)(a.obs + r * a.obs_stride + off);
        WideChunk x;
        x.lo = src[0];
        x.hi = src[1];
        return x;
    };
    // the first tile's first two chunks in flight under the weight copy
    WideChunk n0{}, n1{};
    if (tw0 < tiles) {
        n0 = load_chunk(tw0 * 16, 0);
        n1 = load_chunk(tw0 * 16, 1);
    }
    policy_wide_weights_to_lds<IN>(L, a.w, tid, (int)blockDim.x);
    __syncthreads();
    float (*tile)[33] = L.tile[wave];

    for (int64_t tl = tw0; tl < tiles; tl += tstride) {
        const int64_t row0 = tl * 16;
        // the next tile of this wave (its own again after the last: the loads
        // stay inside the tensor and are dropped)
        const int64_t next0 = (tl + tstride < tiles ? tl + tstride : tl) * 16;
        // an offset the compiler cannot see through: the LDS operand reads stay
        // inside the loop instead of being hoisted into hundreds of live registers
        int z = 0;
        __asm__ volatile("" : "+v"(z));
        const Lds &Lz = *(const Lds *)((const char *)&L + z);
        WideChunk ring[3];
        ring[0] = n0;
        ring[1] = n1;
        f32x4 acc[2][2];  // [chain][output half]
#pragma unroll
        for (int i = 0; i < 2; i++) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int v = 0; v < NC; v++) {
            // chunk v + 2's loads, or the next tile's chunk 0 / 1
            if (v + 2 < NC) ring[(v + 2) % 3] = load_chunk(row0, v + 2);
            else if (v + 2 == NC) n0 = load_chunk(next0, 0);
            else n1 = load_chunk(next0, 1);
            const WideChunk xc = ring[v % 3];
            const float o[8] = {xc.lo.x, xc.lo.y, xc.lo.z, xc.lo.w, xc.hi.x, xc.hi.y, xc.hi.z, xc.hi.w};
            const int k0 = 32 * v + 8 * q;
            float x[8], w0[8], w1[8];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const float4 m4 = *(const float4 *)&Lz.norm[0][k0 + 4 * h];
                const float4 i4 = *(const float4 *)&Lz.norm[1][k0 + 4 * h];
                const float4 u0 = *(const float4 *)&Lz.w1[c][k0 + 4 * h];
                const float4 u1 = *(const float4 *)&Lz.w1[16 + c][k0 + 4 * h];
                x[4 * h] = pol_clamp((o[4 * h] - m4.x) * i4.x);
                x[4 * h + 1] = pol_clamp((o[4 * h + 1] - m4.y) * i4.y);
                x[4 * h + 2] = pol_clamp((o[4 * h + 2] - m4.z) * i4.z);
                x[4 * h + 3] = pol_clamp((o[4 * h + 3] - m4.w) * i4.w);
                w0[4 * h] = u0.x; w0[4 * h + 1] = u0.y; w0[4 * h + 2] = u0.z; w0[4 * h + 3] = u0.w;
                w1[4 * h] = u1.x; w1[4 * h + 1] = u1.y; w1[4 * h + 2] = u1.z; w1[4 * h + 3] = u1.w;
            }
            if (v == NC - 1) {
#pragma unroll
                for (int j = 0; j < 8; j++) x[j] = tail_in ? x[j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                acc[v & 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], w0[j], acc[v & 1][0], 0, 0, 0);
                acc[v & 1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], w1[j], acc[v & 1][1], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const f32x4 a0 = acc[0][0] + acc[1][0], a1 = acc[0][1] + acc[1][1];
        ln_relu_to_tile<false>(a0, a1, Lz.cst[0][c], Lz.cst[0][c + 16], Lz.cst[1][c], Lz.cst[1][c + 16], Lz.cst[2][c],
                               Lz.cst[2][c + 16], tile, c, q);
        pol_wave_sync();
        policy_tail_lds(Lz, tile, c, q);
        bucket_pass_spread<16, false, STOCH>(a, tile, row0, lane, L.bl[wave]);
        pol_wave_sync();
    }
}

// Waves per workgroup and workgroups: one workgroup per CU (256) once there
// are PWIDE_WAVES tiles per CU, fewer waves per workgroup below that so that
// every CU gets work (k_policy_wg's rule).
template <int IN>
static hipError_t launch_policy_wide_t(const PolicyArgs &a, hipStream_t s)
{
    constexpr int64_t CUS = 256;
    const int64_t tiles = (a.rows + 15) / 16;
    int64_t w = (tiles + CUS - 1) / CUS;
    w = w > PWIDE_WAVES ? PWIDE_WAVES : w;
    int64_t g = (tiles + w - 1) / w;
    g = g > CUS ? CUS : g;
    const dim3 grid((unsigned)g), block((unsigned)(64 * w));
    if (a.stochastic) hipLaunchKernelGGL((k_policy_wide<IN, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_policy_wide<IN, 0>), grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_policy_wide(const PolicyArgs &a, int in_dim, hipStream_t s)
{
    if (a.rows <= 0) return hipSuccess;
    switch (in_dim) {
    case 184: return launch_policy_wide_t<184>(a, s);
    case 264: return launch_policy_wide_t<264>(a, s);
    case 344: return launch_policy_wide_t<344>(a, s);
    case 424: return launch_policy_wide_t<424>(a, s);
    default: return hipErrorInvalidValue;
    }
}

void host_policy_wide(const PolicyArgs &a, int in_dim)
{
    for (int64_t r = 0; r < a.rows; r++) policy_row_host_wide(a, in_dim, r);
}

}  // namespace bb
