// bb_policy_wide.h -- the policy network (bb_policy.h) at the observation widths
// of the 2v2 to 5v5 games: bb_obs_width(N) = 184, 264, 344, 424 floats for N =
// 4, 6, 8, 10 (bb_sim.h), the first layer Agent(envs.get_input_dim(), ...) builds
// for them (scripts/agent.py:108-124).  Everything after layer 1 is bb_policy.h's.
//
// Layer-1 arithmetic order (fixed; the gfx950 kernel bb_policy_wide.hip and the
// host executor below give the same bits).  The row is cut into chunks of 32
// floats, chunk v = floats [32v, 32v + 32); NC = ceil(IN / 32) chunks (6, 9, 11,
// 14), the last one 24 or 8 floats wide and padded with zeros (x = 0, W1 = 0).
// Inside a chunk k = 32v + 8q + j: lane quarter q holds the 8 contiguous floats
// j = 0..7 (two aligned 16-byte loads; IN is a multiple of 8, so a quarter's 8
// floats lie wholly inside or wholly outside the row and nothing past the row is
// read).  One v_mfma_f32_16x16x4_f32 per j adds the four products q = 0..3 in q
// order, one rounding each: chunk v is the fmaf chain (j outer, q inner).
// Two independent accumulator chains per output: chain A runs the even chunks
// v = 0, 2, 4, ... in rising order, chain B the odd ones; both start at 0, and
//     h1[n] = (A[n] + B[n]) + b1[n].
#pragma once
#include "bb_policy.h"

namespace bb {

BB_HD constexpr bool pol_wide_width(int in_dim) { return in_dim == 184 || in_dim == 264 || in_dim == 344 || in_dim == 424; }
BB_HD constexpr int pol_wide_chunks(int in_dim) { return (in_dim + 31) / 32; }

// One row on the host, in the wide kernel's arithmetic order.  a.w.obs_mean,
// obs_inv [in_dim] and w1 [32][in_dim]; the rollout-record fields are not read.
inline void policy_row_host_wide(const PolicyArgs &a, int in_dim, int64_t r)
{
    const PolicyWeights &W = a.w;
    const float *o = a.obs + r * a.obs_stride;
    const int nc = pol_wide_chunks(in_dim);
    float x[32 * 14];
    for (int k = 0; k < 32 * nc; k++) x[k] = k < in_dim ? pol_clamp((o[k] - W.obs_mean[k]) * W.obs_inv[k]) : 0.f;
    float h1[POL_HID];
    for (int n = 0; n < POL_HID; n++) {
        const float *wn = W.w1 + (int64_t)n * in_dim;
        float chain[2] = {0.f, 0.f};
        for (int v = 0; v < nc; v++)
            for (int j = 0; j < 8; j++)
                for (int q = 0; q < 4; q++) {
                    const int k = 32 * v + 8 * q + j;
                    chain[v & 1] = __builtin_fmaf(x[k], k < in_dim ? wn[k] : 0.f, chain[v & 1]);
                }
        h1[n] = (chain[0] + chain[1]) + W.b1[n];
    }
    policy_row_host_rest(a, r, h1);
}

#if defined(__HIPCC__)
// Thread tid of nt copies its share of the weights into a workgroup's LDS
// image L (k_policy_wide's PolicyWideLds<IN>, k_ppo_grad_wide's): w1[32][32 NC
// + 4] with zero columns from IN on, norm[2][32 NC], and PolicyLdsWeights' w2,
// wh and cst.  The caller orders the writes before their first read.
template <int IN, class LW>
__device__ __forceinline__ void policy_wide_weights_to_lds(LW &L, const PolicyWeights &W, int tid, int nt)
{
    constexpr int NC = pol_wide_chunks(IN), G = IN / 4, GP = 8 * NC + 1;  // float4 groups per row: read, written
    for (int i = tid; i < 32 * GP; i += nt) {
        const int n = i / GP, g = i % GP;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g < G) w = ((const float4 *)W.w1)[n * G + g];
        *(float4 *)&L.w1[n][4 * g] = w;
    }
    for (int k = tid; k < 32 * NC; k += nt) {
        L.norm[0][k] = k < IN ? W.obs_mean[k] : 0.f;
        L.norm[1][k] = k < IN ? W.obs_inv[k] : 0.f;
    }
    for (int i = tid; i < 32 * 8; i += nt) {  // W2, head_w [32][32] as float4
        const int n = i >> 3, k = 4 * (i & 7);
        *(float4 *)&L.w2[k >> 3][n][k & 7] = ((const float4 *)W.w2)[i];
        *(float4 *)&L.wh[k >> 3][n][k & 7] = ((const float4 *)W.head_w)[i];
    }
    for (int k = tid; k < 7 * 32; k += nt) {
        const float *src[7] = {W.b1, W.ln1_w, W.ln1_b, W.b2, W.ln2_w, W.ln2_b, W.head_b};
        L.cst[k >> 5][k & 31] = src[k >> 5][k & 31];
    }
}
#endif

}  // namespace bb
