// bb_policy_grad_dev.h -- device building blocks of the PPO gradient on gfx950
// from the first LayerNorm on (bb_policy_grad.h has the row math): one 16-row
// tile of a wave, the MFMA C/D layout of bb_policy_dev.h (lane (c = l & 15,
// q = l >> 4): rows 4q + i, columns c and c + 16), the tiles [16][33] in the
// wave's own LDS.  Shared by k_ppo_grad (bb_policy_grad.hip, 128 inputs) and
// k_ppo_grad_wide (bb_policy_grad_wide.hip, 184 to 424 inputs): the same
// operations in the same order in both.
#pragma once
#include <hip/hip_runtime.h>
#include "bb_policy_dev.h"
#include "bb_policy_grad.h"

namespace bb {

__device__ __forceinline__ float quad_sum(float t)
{
    t = t + dpp_f<0xB1>(t);  // quad_perm [1,0,3,2]
    t = t + dpp_f<0x4E>(t);  // quad_perm [2,3,0,1]
    return t;
}

__device__ __forceinline__ double quad_sum(double t)
{
    const auto other = [](double v, auto ctrl) {
        const uint64_t u = __builtin_bit_cast(uint64_t, v);
        const uint64_t o = ((uint64_t)dpp_u<decltype(ctrl)::value>((uint32_t)(u >> 32)) << 32) |
                           dpp_u<decltype(ctrl)::value>((uint32_t)u);
        return __builtin_bit_cast(double, o);
    };
    t = t + other(t, std::integral_constant<int, 0xB1>());
    t = t + other(t, std::integral_constant<int, 0x4E>());
    return t;
}

// LayerNorm + ReLU of the 4 rows a lane holds (ln_relu_to_tile's operations),
// keeping xhat and rstd for the backward pass.
__device__ __forceinline__ void pg_ln_forward(f32x4 a0, f32x4 a1, const float *bias, const float *lw, const float *lb,
                                              float (*tile)[33], int c, int q, float (&xh0)[4], float (&xh1)[4],
                                              float (&rstd)[4])
{
    const float bias0 = bias[c], bias1 = bias[c + 16], w0 = lw[c], w1 = lw[c + 16], lb0 = lb[c], lb1 = lb[c + 16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float h0 = a0[i] + bias0, h1 = a1[i] + bias1;
        const float mean = quarter_sum(h0 + h1) * (1.0f / 32.0f);
        const float d0 = h0 - mean, d1 = h1 - mean;
        const float var = quarter_sum((d0 * d0) + (d1 * d1)) * (1.0f / 32.0f);
        rstd[i] = 1.0f / bbm::sqrtf_(var + 1e-5f);
        xh0[i] = d0 * rstd[i];
        xh1[i] = d1 * rstd[i];
        tile[4 * q + i][c] = pol_relu((xh0[i] * w0) + lb0);
        tile[4 * q + i][c + 16] = pol_relu((xh1[i] * w1) + lb1);
    }
}

// ReLU and LayerNorm backwards of the 4 rows a lane holds: d0 / d1 = dloss/dh
// of columns c / c + 16 (the MFMA's C/D layout), hact the block's output tile
// (the ReLU gate).  dz into out[row][col]; the column partials of the
// LayerNorm weight (dg), LayerNorm bias (dbt) and Linear bias (db) gradients
// are added to.
__device__ __forceinline__ void pg_ln_backward(f32x4 d0, f32x4 d1, const float (*hact)[33], const float (&xh0)[4],
                                               const float (&xh1)[4], const float (&rstd)[4], const float *lw,
                                               float (*out)[33], int c, int q, float (&dg)[2], float (&dbt)[2],
                                               float (&db)[2])
{
    const float w0 = lw[c], w1 = lw[c + 16];
    float z0[4], z1[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float dy0 = hact[4 * q + i][c] > 0.f ? d0[i] : 0.f;
        const float dy1 = hact[4 * q + i][c + 16] > 0.f ? d1[i] : 0.f;
        dg[0] += dy0 * xh0[i];
        dg[1] += dy1 * xh1[i];
        dbt[0] += dy0;
        dbt[1] += dy1;
        const float g0 = dy0 * w0, g1 = dy1 * w1;
        const float m1 = quarter_sum(g0 + g1) * (1.0f / 32.0f);
        const float m2 = quarter_sum((g0 * xh0[i]) + (g1 * xh1[i])) * (1.0f / 32.0f);
        z0[i] = rstd[i] * ((g0 - m1) - (xh0[i] * m2));
        z1[i] = rstd[i] * ((g1 - m1) - (xh1[i] * m2));
        db[0] += z0[i];
        db[1] += z1[i];
    }
    pol_wave_sync();  // every lane's reads of `out`'s earlier contents are done
#pragma unroll
    for (int i = 0; i < 4; i++) {
        out[4 * q + i][c] = z0[i];
        out[4 * q + i][c + 16] = z1[i];
    }
    pol_wave_sync();
}

// acc[m][n] += dz^T . in over the tile's 16 rows: output block (m, n) holds
// dW[16m + 4q + i][16n + c].  colsum[m] (optional): the lane's partial of dz's
// column sums (rows 4s + q of column 16m + c).
template <int NB, int STRIDE>
__device__ __forceinline__ void pg_weight_grad(f32x4 (&acc)[2][NB], const float (*dz)[33], const float (*in)[STRIDE],
                                               int c, int q, float *colsum)
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const float a0 = dz[4 * s + q][c], a1 = dz[4 * s + q][16 + c];
        float b[NB];
#pragma unroll
        for (int n = 0; n < NB; n++) b[n] = in[4 * s + q][16 * n + c];
        if (colsum) {
            colsum[0] += a0;
            colsum[1] += a1;
        }
#pragma unroll
        for (int n = 0; n < NB; n++) {
            acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[n], acc[0][n], 0, 0, 0);
            acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[n], acc[1][n], 0, 0, 0);
        }
    }
}

// d0 / d1 = dz . W (columns c / c + 16 of rows 4q + i) over KS k-steps:
// A = dz[c][4s + q], B = W[4s + q][16t + c], W row-major in LDS.
template <int KS>
__device__ __forceinline__ void pg_data_grad(const float (*dz)[33], const float (*w)[33], int c, int q, f32x4 &d0,
                                             f32x4 &d1)
{
    d0 = f32x4{0.f, 0.f, 0.f, 0.f};
    d1 = f32x4{0.f, 0.f, 0.f, 0.f};
    float a[KS], b0[KS], b1[KS];
#pragma unroll
    for (int s = 0; s < KS; s++) {
        a[s] = dz[c][4 * s + q];
        b0[s] = w[4 * s + q][c];
        b1[s] = w[4 * s + q][16 + c];
    }
#pragma unroll
    for (int s = 0; s < KS; s++) {
        d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b0[s], d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b1[s], d1, 0, 0, 0);
    }
}

// The bucket pass of one tile: logits + value in lg[row][0..19] become
// dloss/dlogit and dloss/dv (zero for a row that is not live); the lane's loss
// sums (part 0 of each live row) are added to.
__device__ __forceinline__ void pg_bucket_pass(const PpoGradArgs &a, float (*lg)[33], int lane, int64_t src,
                                               float inv_m, float (&loss)[4])
{
    const int r = lane >> 2, part = lane & 3;
    const bool live = src >= 0;
    const int64_t sr = live ? src : 0;
    // round 0: bucket `part` (2, 8, 3, 2 logits); round 1: bucket 4 + (part & 1), used by parts 0 and 1
    const int b1 = 4 + (part & 1);
    const int act0 = live ? a.actions[sr * POL_BUCKETS + part] : 0;
    const int act1 = live ? a.actions[sr * POL_BUCKETS + b1] : 0;
    const float lp_old = live ? a.log_prob[sr] : 0.f, v_old = live ? a.value[sr] : 0.f;
    const float adv = live ? a.adv[sr] : 0.f, ret = live ? a.ret[sr] : 0.f;
    const int o0 = pol_bucket_off(part), nb0 = pol_bucket(part), o1 = pol_bucket_off(b1);
    float l0[8], l1[2], p0[8], q0[8], p1[2], q1[2], H0, H1;
    double t0, t1;
#pragma unroll
    for (int i = 0; i < 8; i++) l0[i] = lg[r][o0 + i];  // (in the row: o0 + 8 <= 21 of its 33 floats)
    l1[0] = lg[r][o1];
    l1[1] = lg[r][o1 + 1];
    const float v = lg[r][POL_LOGITS];
    ppo_bucket_stats<8>(l0, nb0, act0, p0, q0, &H0, &t0);
    ppo_bucket_stats<2>(l1, 2, act1, p1, q1, &H1, &t1);
    const bool second = part < 2;
    const double lp = quad_sum(t0 + (second ? t1 : 0.0));
    const float ent = quad_sum(H0 + (second ? H1 : 0.f));
    float dlp, dv;
    const float pg = ppo_pg((float)(lp - (double)lp_old), adv, a.clip, &dlp);
    const float cl = ppo_vloss(v, v_old, ret, a.clip, &dv);
    if (part == 0 && live) {
        loss[0] += ((pg + a.vf_coef * cl) - a.ent_coef * ent) * inv_m;
        loss[1] += pg * inv_m;
        loss[2] += cl * inv_m;
        loss[3] += ent * inv_m;
    }
    pol_wave_sync();  // the quad's reads of the value column are done
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (i < nb0) lg[r][o0 + i] = live ? ppo_dlogit(dlp, a.ent_coef, inv_m, p0[i], q0[i], H0, act0 == i) : 0.f;
    if (second) {
#pragma unroll
        for (int i = 0; i < 2; i++)
            lg[r][o1 + i] = live ? ppo_dlogit(dlp, a.ent_coef, inv_m, p1[i], q1[i], H1, act1 == i) : 0.f;
    }
    if (part == 0) lg[r][POL_LOGITS] = live ? (a.vf_coef * dv) * inv_m : 0.f;
    pol_wave_sync();
}

// Element e >= PG_B1 of a gradient set (bb_policy_grad.h's order at 128 inputs)
// into its tensor or loss4; the PG_HEAD_PAD elements behind the set are the
// head's rows 20..31, written as zero.
constexpr int PG_HEAD_PAD = (POL_HEAD - PG_HEAD_LIVE) * (POL_HID + 1);  // 12 zero rows of head_w and head_b
__device__ __forceinline__ void pg_store_small(int e, float v, const PolicyGrads &g, float *loss4)
{
    if (e >= PG_FLOATS) {
        const int k = e - PG_FLOATS;
        if (k < (POL_HEAD - PG_HEAD_LIVE) * POL_HID) g.head_w[PG_HEAD_LIVE * POL_HID + k] = 0.f;
        else if (k < PG_HEAD_PAD) g.head_b[PG_HEAD_LIVE + (k - (POL_HEAD - PG_HEAD_LIVE) * POL_HID)] = 0.f;
        return;
    }
    if (e < PG_LN1W) g.b1[e - PG_B1] = v;
    else if (e < PG_LN1B) g.ln1_w[e - PG_LN1W] = v;
    else if (e < PG_W2) g.ln1_b[e - PG_LN1B] = v;
    else if (e < PG_B2) g.w2[e - PG_W2] = v;
    else if (e < PG_LN2W) g.b2[e - PG_B2] = v;
    else if (e < PG_LN2B) g.ln2_w[e - PG_LN2W] = v;
    else if (e < PG_HW) g.ln2_b[e - PG_LN2B] = v;
    else if (e < PG_HB) g.head_w[e - PG_HW] = v;
    else if (e < PG_LOSS) g.head_b[e - PG_HB] = v;
    else loss4[e - PG_LOSS] = v;
}

// Layer 2, then the heads, of one tile: h1 (relu(LN1)) in LDS -> h2 with its
// xhat / rstd kept, the logits and the value into lg.  w2l / whl: the [q][n][j]
// images of PolicyLdsWeights, cs its constants (k = 8q + j).
__device__ __forceinline__ void pg_tail_forward(const float (*w2l)[32][PWG_P2], const float (*whl)[32][PWG_P2],
                                                const float (*cs)[32], float (*h1)[33], float (*h2)[33],
                                                float (*lg)[33], int c, int q, float (&xh0)[4], float (&xh1)[4],
                                                float (&rstd)[4])
{
#pragma unroll
    for (int layer = 0; layer < 2; layer++) {
        const float (*wl)[32][PWG_P2] = layer == 0 ? w2l : whl;
        const float (*in)[33] = layer == 0 ? h1 : h2;
        float h[8], w0[8], w1[8];
#pragma unroll
        for (int j = 0; j < 8; j++) h[j] = in[c][8 * q + j];
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const float4 u0 = *(const float4 *)&wl[q][c][4 * v];
            const float4 u1 = *(const float4 *)&wl[q][16 + c][4 * v];
            w0[4 * v] = u0.x; w0[4 * v + 1] = u0.y; w0[4 * v + 2] = u0.z; w0[4 * v + 3] = u0.w;
            w1[4 * v] = u1.x; w1[4 * v + 1] = u1.y; w1[4 * v + 2] = u1.z; w1[4 * v + 3] = u1.w;
        }
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(h[j], w0[j], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(h[j], w1[j], a1, 0, 0, 0);
        }
        if (layer == 0) {
            pg_ln_forward(a0, a1, cs[3], cs[4], cs[5], h2, c, q, xh0, xh1, rstd);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                lg[4 * q + i][c] = a0[i] + cs[6][c];
                lg[4 * q + i][c + 16] = a1[i] + cs[6][c + 16];
            }
        }
        pol_wave_sync();
    }
}

}  // namespace bb
