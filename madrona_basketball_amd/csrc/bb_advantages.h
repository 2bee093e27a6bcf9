// bb_advantages.h -- PPO's phase between the rollout and the minibatch
// gradients: compute_advantages (scripts/ppo.py:144-177) over RunningMeanStd
// (scripts/agent.py:28-50), shared by the host executor and the gfx950 kernels
// (bb_advantages.hip).  With m = (float)vn.mean, s = (float)vn.var + 1e-5f,
// nd[t] = 1 - done[t]:
//
//   v[t]  = m + sqrt(s) clamp(value[t], +-5),  nv likewise from next_value   agent.py:31-34
//   t = K-1 .. 0:  nnt = nd[K-1] at t = K-1 (ppo.py:157 reads not_dones[t]), else nd[t+1]
//                  nxt = nv at t = K-1, else v[t+1]
//                  delta = reward[t] + gamma nxt nnt - v[t]                  ppo.py:162
//                  A[t] = last = delta + gamma lambda nnt last               ppo.py:163-164
//                  Rt[t] = A[t] + v[t]                                       ppo.py:166
//   obs_norm.update(obs rows); value_norm.update(v); value_norm.update(Rt)   ppo.py:168-170
//   advantages = (A - mu) / (sigma + 1e-8)                                   ppo.py:173-174
//   returns = clamp((Rt - m') rsqrt(s'), +-5), m', s' of the updated value_norm
//
// Every batch statistic is a sum of x - shift and of its square (shift: the
// normaliser's current mean, 0 for A), turned into (n, mean, M2) once per
// workgroup; partials merge with Chan's formula in double.  Host and device
// are not bit-matched (the sums run in different orders); both are held to a
// float64 reference.
#pragma once
#include "bb_math.h"

namespace bb {

constexpr int ADV_OBS = 128;        // observation columns
constexpr int ADV_OBS_MAX = 424;    // the widest rows served (bb_advantages_wide.hip: 184, 264, 344, 424)
constexpr int ADV_THREADS = 256;    // k_adv_scan: 4 waves
constexpr int ADV_GAE_GROUPS = 64;  // GAE role: at most 64 workgroups of 256 worlds, grid-stride
constexpr int ADV_OBS_LOADS = 8;    // observation role: 16-byte loads in flight per lane (2 rows per wave load)
constexpr int ADV_OBS_ROWS = 4 * 2 * ADV_OBS_LOADS;  // rows of one workgroup pass: 64
constexpr int ADV_OBS_GROUPS = 512;                  // at most two workgroups per CU, grid-stride
// k_adv_finish: a workgroup takes 16 statistics, 64 chains of up to 8 partials each, then a tree
constexpr int ADV_FIN_COLS = 16, ADV_FIN_CHAINS = 64, ADV_FIN_BATCH = 8;
static_assert(ADV_FIN_CHAINS * ADV_FIN_BATCH >= ADV_OBS_GROUPS && ADV_FIN_CHAINS >= ADV_GAE_GROUPS, "one batch per chain");
// workspace, in doubles: 8 of scalars (the four floats of the elementwise
// pass, then obs_norm's count before the update), the GAE partials (3 x (n, mean, M2), stride 12), the observation
// partials (mean[128], M2[128], n; stride 264)
constexpr int64_t ADV_MAX_STEPS = 1 << 20, ADV_MAX_WORLDS = (int64_t)1 << 31;  // the entry's argument check
constexpr int ADV_WS_HEAD = 8, ADV_WS_GAE = 12, ADV_WS_OBS = 264;

struct RunStats {
    double *mean, *var, *count;  // RunningMeanStd's buffers (agent.py:24-26)
};

struct AdvArgs {
    const float *obs;                          // [steps][worlds][128]
    const float *value, *reward, *done;        // [steps][worlds]
    const float *next_value;                   // [worlds]
    float *adv, *ret;                          // [steps][worlds]
    RunStats vn, on;                           // value normaliser (dim 1), observation normaliser (dim 128)
    float gamma, gl;                           // (float)gamma, (float)(gamma * lambda): ppo.py:162-164's scalars
    int32_t steps;
    int64_t worlds;
    float *out4;                               // mu, sigma of A; the value normaliser's new mean, var
    double *ws;                                // device only
};

struct AdvGrid {
    int gae, obs;
};
BB_HD AdvGrid adv_grid(int32_t steps, int64_t worlds)
{
    const int64_t g = (worlds + ADV_THREADS - 1) / ADV_THREADS;
    const int64_t o = (worlds * steps + ADV_OBS_ROWS - 1) / ADV_OBS_ROWS;
    return {(int)(g < ADV_GAE_GROUPS ? g : ADV_GAE_GROUPS), (int)(o < ADV_OBS_GROUPS ? o : ADV_OBS_GROUPS)};
}

// The observation role at 184, 264, 344, 424 columns (bb_advantages_wide.hip):
// a workgroup pass is RP whole rows, thread t the 16 bytes at 16 t of it (RP
// IN / 4 threads: 506, 990, 946, 954, rounded up to whole waves), ADV_OBS_LOADS
// passes per batch.  Wide grid rule: the GAE role as adv_grid has it; the
// observation role min(512, ceil(K W / (8 RP))) workgroups, grid-stride over
// batches of 8 RP = 88, 120, 88, 72 rows.  Partial stride: mean[IN], M2[IN], n.
BB_HD constexpr int adv_wide_rp(int in_dim) { return in_dim == 184 ? 11 : in_dim == 264 ? 15 : in_dim == 344 ? 11 : 9; }
BB_HD constexpr int adv_wide_threads(int in_dim) { return (adv_wide_rp(in_dim) * (in_dim / 4) + 63) / 64 * 64; }
BB_HD constexpr int adv_wide_ws_obs(int in_dim) { return 2 * in_dim + 8; }
BB_HD AdvGrid adv_wide_grid(int in_dim, int32_t steps, int64_t worlds)
{
    const int64_t batch = ADV_OBS_LOADS * adv_wide_rp(in_dim);
    const int64_t o = (worlds * steps + batch - 1) / batch;
    return {adv_grid(steps, worlds).gae, (int)(o < ADV_OBS_GROUPS ? o : ADV_OBS_GROUPS)};
}

// agent.py:31-34, unnorm with clamp 5: mean + sqrt(var) * clamp(x)
BB_HD float adv_unnorm(float m, float sq, float x)
{
    return m + sq * __builtin_fminf(__builtin_fmaxf(x, -5.f), 5.f);
}

// One step of the backward recursion; *last is last_gae_lam.  Returns A[t].
BB_HD float adv_gae_step(float reward, float v, float nxt, float nnt, float gamma, float gl, float *last)
{
    const float delta = (reward + (gamma * nxt) * nnt) - v;
    *last = delta + (gl * nnt) * *last;
    return *last;
}

// (n, mean, M2) of a batch.
struct Moments {
    double n, mean, m2;
};
// From the sums of x - shift and (x - shift)^2 over n values.
BB_HD Moments adv_moments(double n, double shift, double s, double q)
{
    if (!(n > 0.0)) return {0.0, 0.0, 0.0};
    const double d = s / n, m2 = q - s * d;
    return {n, shift + d, m2 > 0.0 ? m2 : 0.0};
}
// Chan's merge of b into a.
BB_HD void adv_merge(Moments &a, const Moments &b)
{
    if (!(b.n > 0.0)) return;
    const double n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
    a.mean = a.mean + d * f;
    a.m2 = (a.m2 + b.m2) + (d * d) * (a.n * f);
    a.n = n;
}
// RunningMeanStd.update (agent.py:43-50) with the batch's unbiased variance.
BB_HD void adv_update(double &mean, double &var, double &count, const Moments &b)
{
    const double var_b = b.m2 / (b.n - 1.0), count_ = b.n + count, delta = b.mean - mean;
    const double m = (var * count + var_b * b.n) + ((delta * delta) * count) * b.n / count_;
    mean = mean + delta * b.n / count_;
    var = m / count_;
    count = count_;
}

// The two value-normaliser updates, the [4] result and the elementwise pass's
// scalars {mu, sigma + 1e-8, m', rsqrt(s')} from the final moments of v, Rt, A.
BB_HD void adv_finish_scalars(const RunStats &vn, const Moments &mv, const Moments &mr, const Moments &ma, float *out4,
                              float *sc)
{
    double mean = vn.mean[0], var = vn.var[0], count = vn.count[0];
    adv_update(mean, var, count, mv);
    adv_update(mean, var, count, mr);
    vn.mean[0] = mean; vn.var[0] = var; vn.count[0] = count;
    const float mu = (float)ma.mean, sigma = (float)__builtin_sqrt(ma.m2 / (ma.n - 1.0));
    out4[0] = mu; out4[1] = sigma; out4[2] = (float)mean; out4[3] = (float)var;
    sc[0] = mu; sc[1] = sigma + 1e-8f; sc[2] = (float)mean;
    sc[3] = 1.0f / __builtin_sqrtf((float)var + 1e-5f);
}

BB_HD float adv_norm_a(float a, const float *sc) { return (a - sc[0]) / sc[1]; }
BB_HD float adv_norm_r(float r, const float *sc)
{
    return __builtin_fminf(__builtin_fmaxf((r - sc[2]) * sc[3], -5.f), 5.f);
}

}  // namespace bb
