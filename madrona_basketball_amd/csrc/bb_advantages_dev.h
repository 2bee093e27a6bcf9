// bb_advantages_dev.h -- device functions the advantage kernels of every
// observation width share (bb_advantages.hip, bb_advantages_wide.hip): the
// wave sum and the GAE role of the scan, which does not depend on the width.
#pragma once
#include <hip/hip_runtime.h>
#include "bb_advantages.h"

namespace bb {

constexpr int ADV_GAE_BLOCK = 8;  // steps whose loads are issued together

__device__ __forceinline__ double adv_wave_sum(double x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + __shfl_xor(x, m);
    return x;
}

// The GAE role, run by ADV_THREADS threads (a wider workgroup's other waves
// leave the kernel first).  red: [4 waves][7] doubles
__device__ inline void adv_gae_role(const AdvArgs &a, int group, int groups, double *red)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.steps;
    const int64_t W = a.worlds;
    const float m = (float)a.vn.mean[0], sq = __builtin_sqrtf((float)a.vn.var[0] + 1e-5f);
    const double shift = (double)m;
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // v, Rt, A: sum, sum of squares
    int worlds = 0;
    for (int64_t w = (int64_t)group * ADV_THREADS + tid; w < W; w += (int64_t)groups * ADV_THREADS) {
        float nxt = adv_unnorm(m, sq, a.next_value[w]);
        float nnt = 1.f - a.done[(int64_t)(K - 1) * W + w];
        float last = 0.f;
        for (int t1 = K; t1 > 0; t1 -= ADV_GAE_BLOCK) {
            float val[ADV_GAE_BLOCK], rew[ADV_GAE_BLOCK], dn[ADV_GAE_BLOCK];
#pragma unroll
            for (int i = 0; i < ADV_GAE_BLOCK; i++) {  // steps below 0 re-read row 0 and are not used
                const int t = t1 - 1 - i;
                const int64_t at = (int64_t)(t < 0 ? 0 : t) * W + w;
                val[i] = a.value[at]; rew[i] = a.reward[at]; dn[i] = a.done[at];
            }
#pragma unroll
            for (int i = 0; i < ADV_GAE_BLOCK; i++) {
                const int t = t1 - 1 - i;
                if (t >= 0) {
                    const float v = adv_unnorm(m, sq, val[i]);
                    const float adv = adv_gae_step(rew[i], v, nxt, nnt, a.gamma, a.gl, &last);
                    const float rt = adv + v;
                    const int64_t at = (int64_t)t * W + w;
                    a.adv[at] = adv;
                    a.ret[at] = rt;
                    const double dv = (double)v - shift, dr = (double)rt - shift, da = (double)adv;
                    sum[0] = sum[0] + dv; sum[1] = sum[1] + dv * dv;
                    sum[2] = sum[2] + dr; sum[3] = sum[3] + dr * dr;
                    sum[4] = sum[4] + da; sum[5] = sum[5] + da * da;
                    nxt = v;
                    nnt = 1.f - dn[i];
                }
            }
        }
        worlds++;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double s = adv_wave_sum(sum[k]);
        if (lane == 0) red[wave * 7 + k] = s;
    }
    const double n = adv_wave_sum((double)worlds * (double)K);
    if (lane == 0) red[wave * 7 + 6] = n;
    __syncthreads();
    if (tid < 3) {
        double s = 0.0, q = 0.0, cnt = 0.0;
        for (int w = 0; w < ADV_THREADS / 64; w++) {
            s = s + red[w * 7 + 2 * tid]; q = q + red[w * 7 + 2 * tid + 1]; cnt = cnt + red[w * 7 + 6];
        }
        const Moments mo = adv_moments(cnt, tid < 2 ? shift : 0.0, s, q);
        double *dst = a.ws + ADV_WS_HEAD + group * ADV_WS_GAE + 3 * tid;
        dst[0] = mo.n; dst[1] = mo.mean; dst[2] = mo.m2;
    }
}

}  // namespace bb
