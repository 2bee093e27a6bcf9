// bb_advantages_wide.hip -- compute_advantages (bb_advantages.h) on gfx950 for
// the observation rows of the 2v2 to 5v5 games: IN = 184, 264, 344 or 424
// floats (736 to 1 696 bytes).  The GAE role (bb_advantages_dev.h), k_adv_norm
// and every formula are bb_advantages.hip's; the observation role and the
// finish are written for these widths.
//
// k_adv_scan_wide<IN>, two roles by workgroup index as k_adv_scan has them:
//   [0, gae): the GAE role on the workgroup's first 256 threads (the other
//     waves leave at once: a wave that has ended is not waited for at a barrier).
//   [gae, gae + obs): the observation role.  A 128-float row is half a wave
//     load; these rows do not divide into waves.  With C4 = IN / 4 = 46, 66, 86,
//     106 16-byte columns a workgroup is RP C4 threads rounded up to whole
//     waves, RP = 11, 15, 11, 9 rows per pass (506 of 512, 990 of 1 024, 946 of
//     960, 954 of 960 threads; the tail lanes idle).  Thread t owns column
//     t mod C4 of row slot t / C4 for the whole call, its four shifts
//     (float)mean_old in registers.  A pass is RP whole contiguous rows and
//     thread t's load the 16 bytes at 16 t of it: fully coalesced, no LDS in
//     the loop.  ADV_OBS_LOADS = 8 passes are in flight per thread before their
//     arithmetic; x - shift and its square are summed over the batch in f32
//     and the batch added to the thread's double sums.  A row past the end
//     re-reads the last row and counts nothing.  At the end the RP slots of a
//     column are added in LDS in slot order and one (n, mean, M2) partial per
//     column and workgroup goes to the workspace through adv_moments.
// k_adv_finish_wide, ceil(IN / 16) + 1 = 12, 17, 22, 27 + 1 workgroups of 1 024
//   threads: k_adv_finish's scheme (64 chains of up to 8 partials loaded in one
//   batch, Chan's merge in double, a six-level tree in LDS), the last column
//   workgroup half empty behind a column guard; the last workgroup takes v, Rt,
//   A and writes obs_norm's count from the copy the scan left in the workspace.
// No atomics, no MFMA: a reduction over rows bound by memory.  The order of
// every sum is fixed by the shape: two calls give the same bits.
#include <hip/hip_runtime.h>
#include "bb_advantages_dev.h"
#include "bb_launch.h"
#include "bb_policy_wide.h"

namespace bb {

constexpr int ADVW_FIN_THREADS = ADV_FIN_COLS * ADV_FIN_CHAINS;

// red: [RP slots][2][IN] sums, then [RP] row counts
template <int IN>
__device__ __forceinline__ void adv_obs_role_wide(const AdvArgs &a, int group, int groups, double *red)
{
    constexpr int C4 = IN / 4, RP = adv_wide_rp(IN), BATCH = ADV_OBS_LOADS * RP;
    const int tid = (int)threadIdx.x, slot = tid / C4, c4 = tid - slot * C4;
    const int64_t rows = a.worlds * a.steps;
    if (slot < RP) {
        float sh[4];
#pragma unroll
        for (int j = 0; j < 4; j++) sh[j] = (float)a.on.mean[4 * c4 + j];
        double S[4] = {0.0, 0.0, 0.0, 0.0}, Q[4] = {0.0, 0.0, 0.0, 0.0};
        int cnt = 0;
        for (int64_t r0 = (int64_t)group * BATCH; r0 < rows; r0 += (int64_t)groups * BATCH) {
            const int64_t rw = r0 + slot;
            float4 x[ADV_OBS_LOADS];
#pragma unroll
            for (int u = 0; u < ADV_OBS_LOADS; u++) {  // a row past the end re-reads the last row and is not used
                const int64_t r = rw + u * RP;
                x[u] = *(const float4 *)(a.obs + (r < rows ? r : rows - 1) * IN + 4 * c4);
            }
            float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < ADV_OBS_LOADS; u++) {
                const bool ok = rw + u * RP < rows;
                const float xv[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float d = ok ? xv[j] - sh[j] : 0.f;
                    s[j] = s[j] + d;
                    q[j] = q[j] + d * d;
                }
                cnt += ok ? 1 : 0;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                S[j] = S[j] + (double)s[j];
                Q[j] = Q[j] + (double)q[j];
            }
        }
        double *rs = red + slot * 2 * IN;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            rs[4 * c4 + j] = S[j];
            rs[IN + 4 * c4 + j] = Q[j];
        }
        if (c4 == 0) red[RP * 2 * IN + slot] = (double)cnt;
    }
    __syncthreads();
    if (tid < IN) {
        double s = 0.0, q = 0.0, n = 0.0;
        for (int k = 0; k < RP; k++) {
            s = s + red[k * 2 * IN + tid]; q = q + red[k * 2 * IN + IN + tid]; n = n + red[RP * 2 * IN + k];
        }
        const Moments mo = adv_moments(n, (double)(float)a.on.mean[tid], s, q);
        double *dst = a.ws + ADV_WS_HEAD + ADV_GAE_GROUPS * ADV_WS_GAE + (int64_t)group * adv_wide_ws_obs(IN);
        dst[tid] = mo.mean;
        dst[IN + tid] = mo.m2;
        if (tid == 0) dst[2 * IN] = mo.n;
    }
}

template <int IN>
__global__ __launch_bounds__(adv_wide_threads(IN)) void k_adv_scan_wide(AdvArgs a, int gae_groups, int obs_groups)
{
    static_assert(pol_wide_width(IN) && adv_wide_threads(IN) >= IN && adv_wide_threads(IN) <= 1024, "observation width");
    __shared__ double red[adv_wide_rp(IN) * (2 * IN + 1)];
    static_assert(sizeof(red) >= sizeof(double) * 4 * 7 && sizeof(red) <= 64 * 1024, "both roles' LDS");
    const int g = (int)blockIdx.x;
    if (g == 0 && threadIdx.x == 0) a.ws[2] = a.on.count[0];  // k_adv_finish_wide's workgroups read this copy
    if (g < gae_groups) {
        if ((int)threadIdx.x >= ADV_THREADS) return;
        adv_gae_role(a, g, gae_groups, red);
    } else {
        adv_obs_role_wide<IN>(a, g - gae_groups, obs_groups, red);
    }
}

__global__ __launch_bounds__(ADVW_FIN_THREADS) void k_adv_finish_wide(AdvArgs a, int in_dim, int gae_groups, int obs_groups)
{
    __shared__ Moments sm[ADV_FIN_CHAINS][ADV_FIN_COLS];
    const int tid = (int)threadIdx.x, c = tid & (ADV_FIN_COLS - 1), j = tid / ADV_FIN_COLS;
    const bool obs = (int)blockIdx.x < (in_dim + ADV_FIN_COLS - 1) / ADV_FIN_COLS;
    const int col = (int)blockIdx.x * ADV_FIN_COLS + c;
    const bool live = obs && col < in_dim;  // the last column workgroup: 8 of 16 columns
    const int stride = adv_wide_ws_obs(in_dim);
    const double *gp = a.ws + ADV_WS_HEAD, *op = gp + ADV_GAE_GROUPS * ADV_WS_GAE;
    Moments mo{0.0, 0.0, 0.0};
    if (live) {
        Moments part[ADV_FIN_BATCH];
#pragma unroll
        for (int u = 0; u < ADV_FIN_BATCH; u++) {  // a partial past the last re-reads partial 0 with n = 0
            const int p = j + ADV_FIN_CHAINS * u;
            const double *src = op + (int64_t)(p < obs_groups ? p : 0) * stride;
            part[u] = Moments{p < obs_groups ? src[2 * in_dim] : 0.0, src[col], src[in_dim + col]};
        }
#pragma unroll
        for (int u = 0; u < ADV_FIN_BATCH; u++) adv_merge(mo, part[u]);
    } else if (!obs && c < 3 && j < gae_groups) {  // v, Rt, A
        const double *src = gp + j * ADV_WS_GAE + 3 * c;
        mo = Moments{src[0], src[1], src[2]};
    }
    sm[j][c] = mo;
    __syncthreads();
    for (int s = ADV_FIN_CHAINS / 2; s > 0; s >>= 1) {
        if (j < s) {
            adv_merge(mo, sm[j + s][c]);
            sm[j][c] = mo;
        }
        __syncthreads();
    }
    if (live && j == 0) {
        double mean = a.on.mean[col], var = a.on.var[col], count = a.ws[2];
        adv_update(mean, var, count, mo);
        a.on.mean[col] = mean;
        a.on.var[col] = var;
    }
    if (!obs && tid == 0) {
        a.on.count[0] = (double)(a.worlds * a.steps) + a.ws[2];
        adv_finish_scalars(a.vn, sm[0][0], sm[0][1], sm[0][2], a.out4, (float *)a.ws);
    }
}

int64_t advantages_wide_workspace_bytes(int in_dim, int32_t steps, int64_t worlds)
{
    if (!pol_wide_width(in_dim)) return 0;
    const AdvGrid g = adv_wide_grid(in_dim, steps, worlds);
    return (int64_t)sizeof(double) * (ADV_WS_HEAD + ADV_GAE_GROUPS * ADV_WS_GAE + (int64_t)g.obs * adv_wide_ws_obs(in_dim));
}

template <int IN>
static hipError_t launch_adv_scan_wide(const AdvArgs &a, const AdvGrid &g, hipStream_t s)
{
    hipLaunchKernelGGL(k_adv_scan_wide<IN>, dim3(g.gae + g.obs), dim3(adv_wide_threads(IN)), 0, s, a, g.gae, g.obs);
    return hipGetLastError();
}

hipError_t launch_advantages_wide(const AdvArgs &a, int in_dim, hipStream_t s)
{
    if (!pol_wide_width(in_dim)) return hipErrorInvalidValue;
    const AdvGrid g = adv_wide_grid(in_dim, a.steps, a.worlds);
    hipError_t e;
    switch (in_dim) {
    case 184: e = launch_adv_scan_wide<184>(a, g, s); break;
    case 264: e = launch_adv_scan_wide<264>(a, g, s); break;
    case 344: e = launch_adv_scan_wide<344>(a, g, s); break;
    default: e = launch_adv_scan_wide<424>(a, g, s); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_adv_finish_wide, dim3((in_dim + ADV_FIN_COLS - 1) / ADV_FIN_COLS + 1), dim3(ADVW_FIN_THREADS), 0, s,
                       a, in_dim, g.gae, g.obs);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_adv_norm(a, s);
}

}  // namespace bb
