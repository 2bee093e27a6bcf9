// bb_policy_grad.h -- PPO's loss and its gradient for one minibatch row of the
// policy network (scripts/ppo.py:192-210 update_policy with clip_vloss, over
// scripts/agent.py:172-178 get_stats and scripts/action.py:35-44 action_stats),
// shared by the host executor and the gfx950 kernel (bb_policy_grad.hip).
// Forward as bb_policy.h (clamped normaliser, pol_expf / pol_logf, bucket
// offsets); the normaliser's statistics are not parameters, so nothing flows
// back past xn.
//
//   lp = sum_b log p_b[a_b],  ent = sum_b H_b,  ratio = exp(lp - lp_old)
//   pg = max(-adv ratio, -adv clamp(ratio, 1 - c, 1 + c))                ppo.py:195-199
//   cl = 1/2 max((v - ret)^2, (v_old + clamp(v - v_old, +-c) - ret)^2)   ppo.py:201-204
//   loss = mean(pg) + vf_coef mean(cl) - ent_coef mean(ent)              ppo.py:206-210
//   dloss/dlogit_j = [dpg/dlp (1[j = a_b] - p_j) + ent_coef p_j (log p_j + H_b)] / M
//   dloss/dv       = vf_coef dcl/dv / M
// LayerNorm backward: dz = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma;
// ReLU gates on y > 0.  Unlike the rollout's forward, host and device are not
// bit-matched here (the sums over rows run in different orders); both are held
// to a float64 reference.
#pragma once
#include "bb_policy.h"

namespace bb {

// Floats of one gradient set, in bb_policy_grads' order with the head's 20 live
// rows only, then the four loss sums (total, pg, cl, ent).
constexpr int PG_W1 = 0, PG_B1 = 4096, PG_LN1W = 4128, PG_LN1B = 4160;
constexpr int PG_W2 = 4192, PG_B2 = 5216, PG_LN2W = 5248, PG_LN2B = 5280;
constexpr int PG_HW = 5312, PG_HB = 5952, PG_LOSS = 5972, PG_FLOATS = 5976;
constexpr int PG_HEAD_LIVE = POL_LOGITS + 1;  // 19 actor rows + the critic row

struct PolicyGrads {
    float *w1, *b1, *ln1_w, *ln1_b;  // [32][128], [32] x3
    float *w2, *b2, *ln2_w, *ln2_b;  // [32][32], [32] x3
    float *head_w, *head_b;          // [32][32], [32]: rows 20..31 zero
};

struct PpoGradArgs {
    PolicyWeights w;
    const float *obs;        // [rows][128] (the wide gradient: [rows][in_dim])
    const int32_t *actions;  // [rows][6]
    const float *log_prob, *value, *adv, *ret;  // [rows]
    const int64_t *idx;      // [m] rows of the minibatch, or nullptr: row i
    int64_t rows, m;
    float clip, vf_coef, ent_coef;
    PolicyGrads g;
    float *loss4;            // total, pg, cl before vf_coef, mean entropy
    float *partial;          // device: [groups][PG_FLOATS]
};

// Buffer row of minibatch row i, or -1 where there is none (past m, or an
// index outside the buffer: such a row contributes nothing).
BB_HD int64_t ppo_src_row(const int64_t *idx, int64_t rows, int64_t m, int64_t i)
{
    if (i >= m) return -1;
    const int64_t s = idx ? idx[i] : i;
    return (s >= 0 && s < rows) ? s : -1;
}

// The clipped surrogate of one row from dl = lp - lp_old, and dpg/dlp: -adv
// ratio, or 0 where the ratio is outside [1 - c, 1 + c] and the clamped term is
// the strictly larger.  (The callers sum the six log-probabilities and take the
// difference in double: lp is O(10) and its f32 rounding would be the largest
// error of the whole gradient, exp() turning it into a relative one.)
BB_HD float ppo_pg(float dl, float adv, float c, float *dlp)
{
    const float ratio = pol_expf(dl);
    const float rc = __builtin_fminf(__builtin_fmaxf(ratio, 1.0f - c), 1.0f + c);
    const float s1 = -adv * ratio, s2 = -adv * rc;
    const bool cut = rc != ratio && s2 > s1;
    *dlp = cut ? 0.f : s1;
    return s2 > s1 ? s2 : s1;
}

// The clipped value loss of one row and dcl/dv: v - ret, or 0 where
// |v - v_old| > c and the clipped term is the strictly larger.
BB_HD float ppo_vloss(float v, float v_old, float ret, float c, float *dv)
{
    const float d = v - v_old;
    const float dc = __builtin_fminf(__builtin_fmaxf(d, -c), c);
    const float e1 = v - ret, e2 = (v_old + dc) - ret;
    const float q1 = e1 * e1, q2 = e2 * e2;
    const bool cut = dc != d && q2 > q1;
    *dv = cut ? 0.f : e1;
    return 0.5f * (q2 > q1 ? q2 : q1);
}

// One bucket of nb <= NBM logits l[]: probabilities p[], log-probabilities
// lq[] (entries from nb on: 0), the entropy and log p[a] (the f32 terms
// combined in double).
template <int NBM>
BB_HD void ppo_bucket_stats(const float (&l)[NBM], int nb, int a, float (&p)[NBM], float (&lq)[NBM], float *ent,
                            double *la)
{
    float mx = l[0];
#pragma unroll
    for (int i = 1; i < NBM; i++) mx = (i < nb && l[i] > mx) ? l[i] : mx;
    float e[NBM], s = 0.f;
#pragma unroll
    for (int i = 0; i < NBM; i++) {
        e[i] = pol_expf((i < nb ? l[i] : mx) - mx);
        s = i < nb ? s + e[i] : s;
    }
    const float ls = pol_logf(s);
    float h = 0.f, t = mx;
#pragma unroll
    for (int i = 0; i < NBM; i++) {
        const bool in = i < nb;
        p[i] = in ? e[i] / s : 0.f;
        lq[i] = in ? (l[i] - mx) - ls : 0.f;
        h = h - p[i] * lq[i];
        t = (in && a == i) ? l[i] : t;
    }
    *ent = h;
    *la = ((double)t - (double)mx) - (double)ls;
}

// dloss/dlogit_j of a bucket with entropy H (the 1 / M included).
BB_HD float ppo_dlogit(float dlp, float ent_coef, float inv_m, float p, float lq, float H, bool taken)
{
    return (dlp * ((taken ? 1.0f : 0.0f) - p) + ent_coef * (p * (lq + H))) * inv_m;
}

// The widest first layer served (bb_policy_wide.h: 184, 264, 344, 424 inputs).
// At in_dim inputs W1's gradient is [32][in_dim] and every later element of a
// gradient set sits 32 (in_dim - 128) floats further on.
constexpr int PG_IN_MAX = 424;
BB_HD constexpr int pg_floats(int in_dim) { return PG_FLOATS + POL_HID * (in_dim - POL_IN); }

// Host executor: one row's forward, loss and backward in plain loops, its
// gradient added into acc[pg_floats(in_dim)] (double: the cross-row sums).
// obs rows and W1's rows are in_dim floats.
inline void ppo_grad_row_host(const PpoGradArgs &a, int64_t i, double *acc, int in_dim)
{
    const int64_t src = ppo_src_row(a.idx, a.rows, a.m, i);
    if (src < 0) return;
    const PolicyWeights &W = a.w;
    const float inv_m = 1.0f / (float)a.m;
    const float *o = a.obs + src * in_dim;
    const int sh = POL_HID * (in_dim - POL_IN);  // the elements behind W1
    float x[PG_IN_MAX], xh1[POL_HID], h1[POL_HID], xh2[POL_HID], h2[POL_HID], out[PG_HEAD_LIVE];
    float rstd1 = 0.f, rstd2 = 0.f;
    for (int k = 0; k < in_dim; k++) x[k] = pol_clamp((o[k] - W.obs_mean[k]) * W.obs_inv[k]);
    const auto layer = [](const float *in, int n_in, const float *w, const float *b, const float *lw, const float *lb,
                          float *xh, float *h, float *rstd) {
        float z[POL_HID], mean = 0.f, var = 0.f;
        for (int n = 0; n < POL_HID; n++) {
            float s = b[n];
            for (int k = 0; k < n_in; k++) s = __builtin_fmaf(in[k], w[n * n_in + k], s);
            z[n] = s;
            mean += s;
        }
        mean *= 1.0f / POL_HID;
        for (int n = 0; n < POL_HID; n++) var += (z[n] - mean) * (z[n] - mean);
        *rstd = 1.0f / bbm::sqrtf_(var * (1.0f / POL_HID) + 1e-5f);
        for (int n = 0; n < POL_HID; n++) {
            xh[n] = (z[n] - mean) * *rstd;
            h[n] = pol_relu(xh[n] * lw[n] + lb[n]);
        }
    };
    layer(x, in_dim, W.w1, W.b1, W.ln1_w, W.ln1_b, xh1, h1, &rstd1);
    layer(h1, POL_HID, W.w2, W.b2, W.ln2_w, W.ln2_b, xh2, h2, &rstd2);
    for (int n = 0; n < PG_HEAD_LIVE; n++) {
        float s = W.head_b[n];
        for (int k = 0; k < POL_HID; k++) s = __builtin_fmaf(h2[k], W.head_w[n * POL_HID + k], s);
        out[n] = s;
    }
    // buckets: log-prob of the taken actions and entropy, then the head gradient
    float p[POL_BUCKETS][8], lq[POL_BUCKETS][8], H[POL_BUCKETS], ent = 0.f;
    double lp = 0.0;
    const int32_t *act = a.actions + src * POL_BUCKETS;
    for (int b = 0; b < POL_BUCKETS; b++) {
        float l[8];
        double la;
        for (int j = 0; j < 8; j++) l[j] = j < pol_bucket(b) ? out[pol_bucket_off(b) + j] : 0.f;
        ppo_bucket_stats<8>(l, pol_bucket(b), act[b], p[b], lq[b], &H[b], &la);
        lp += la;
        ent += H[b];
    }
    float dlp, dv, dout[PG_HEAD_LIVE];
    const float pg = ppo_pg((float)(lp - (double)a.log_prob[src]), a.adv[src], a.clip, &dlp);
    const float cl = ppo_vloss(out[POL_LOGITS], a.value[src], a.ret[src], a.clip, &dv);
    for (int b = 0; b < POL_BUCKETS; b++)
        for (int j = 0; j < pol_bucket(b); j++)
            dout[pol_bucket_off(b) + j] = ppo_dlogit(dlp, a.ent_coef, inv_m, p[b][j], lq[b][j], H[b], act[b] == j);
    dout[POL_LOGITS] = (a.vf_coef * dv) * inv_m;
    acc[sh + PG_LOSS + 0] += (double)((pg + a.vf_coef * cl) - a.ent_coef * ent) * inv_m;
    acc[sh + PG_LOSS + 1] += (double)pg * inv_m;
    acc[sh + PG_LOSS + 2] += (double)cl * inv_m;
    acc[sh + PG_LOSS + 3] += (double)ent * inv_m;
    // heads, then the two Linear + LayerNorm + ReLU blocks backwards
    float d2[POL_HID], d1[POL_HID];
    for (int k = 0; k < POL_HID; k++) d2[k] = 0.f;
    for (int n = 0; n < PG_HEAD_LIVE; n++) {
        acc[sh + PG_HB + n] += dout[n];
        for (int k = 0; k < POL_HID; k++) {
            acc[sh + PG_HW + n * POL_HID + k] += dout[n] * h2[k];
            d2[k] += dout[n] * W.head_w[n * POL_HID + k];
        }
    }
    const auto back = [&](float *dh, const float *h, const float *xh, float rstd, const float *lw, const float *in,
                          int n_in, const float *w, int o_w, int o_b, int o_lw, int o_lb, float *din) {
        float g[POL_HID], m1 = 0.f, m2 = 0.f;
        for (int n = 0; n < POL_HID; n++) {
            const float dy = h[n] > 0.f ? dh[n] : 0.f;
            acc[o_lw + n] += dy * xh[n];
            acc[o_lb + n] += dy;
            g[n] = dy * lw[n];
            m1 += g[n];
            m2 += g[n] * xh[n];
        }
        m1 *= 1.0f / POL_HID;
        m2 *= 1.0f / POL_HID;
        for (int k = 0; din && k < n_in; k++) din[k] = 0.f;
        for (int n = 0; n < POL_HID; n++) {
            const float dz = rstd * ((g[n] - m1) - xh[n] * m2);
            acc[o_b + n] += dz;
            for (int k = 0; k < n_in; k++) {
                acc[o_w + n * n_in + k] += dz * in[k];
                if (din) din[k] += dz * w[n * n_in + k];
            }
        }
    };
    back(d2, h2, xh2, rstd2, W.ln2_w, h1, POL_HID, W.w2, sh + PG_W2, sh + PG_B2, sh + PG_LN2W, sh + PG_LN2B, d1);
    back(d1, h1, xh1, rstd1, W.ln1_w, x, in_dim, W.w1, PG_W1, sh + PG_B1, sh + PG_LN1W, sh + PG_LN1B, nullptr);
}

#if defined(__HIPCC__)
// Element e's sum over the workgroups' partials in a fixed tree, for a
// workgroup of 64 elements x 4 thread rows: row t adds the partials of
// workgroups t, t + 4, ... in order, then (c0 + c1) + (c2 + c3) through
// chain[4][64] in LDS (one barrier).  k_ppo_grad_reduce and k_ppo_step share
// it: the same gradient bits from either.  floats: the elements of one partial
// (k_ppo_grad_wide_reduce has two sets of partials of its own sizes).
__device__ __forceinline__ float pg_tree_sum(const float *partial, int groups, int e, float (*chain)[64],
                                             int floats = PG_FLOATS)
{
    const int x = (int)threadIdx.x, t = (int)threadIdx.y;
    float s = 0.f;
    if (e < floats) {
#pragma unroll 8
        for (int w = t; w < groups; w += 4) s = s + partial[(int64_t)w * floats + e];
    }
    chain[t][x] = s;
    __syncthreads();
    return (chain[0][x] + chain[1][x]) + (chain[2][x] + chain[3][x]);
}
#endif

}  // namespace bb
