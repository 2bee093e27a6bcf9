// bb_advantages.hip -- compute_advantages (scripts/ppo.py:144-177) on gfx950:
// GAE, the three normaliser updates and the normalisation of advantages and
// returns in three launches (row math and the formulas: bb_advantages.h).
//
// k_adv_scan, 256 threads, two roles by workgroup index:
//   [0, gae): the GAE role.  One lane per world, a workgroup takes 256 worlds
//     per grid-stride pass.  The value / reward / done rows of ADV_GAE_BLOCK
//     steps are loaded (one coalesced 256-byte load per wave and row) before
//     the block's dependent chain runs, so the chain waits on memory once per
//     block.  Raw A and Rt go to advantages / returns; each lane keeps the
//     sums of v - m, Rt - m, A and of their squares in double.
//   [gae, gae + obs): the observation role, K W rows of 512 B read once.  A
//     wave load covers two rows: lane l takes the 16 bytes of columns
//     4 (l & 31).. of row l >> 5.  A lane has ADV_OBS_LOADS loads in flight
//     (16 rows per wave, 64 per workgroup pass), sums x - mean_old and its
//     square over those 8 rows in f32 and adds the chunk to its double sums.
//   Either role then adds its lanes' sums (the half-waves / the wave by
//   cross-lane moves, the four waves in wave order in LDS) and stores one
//   (n, mean, M2) partial per statistic.  No atomics, no MFMA: a reduction over
//   rows bound by memory.
// k_adv_finish, nine workgroups of 1 024 threads, 16 statistics each (eight
//   take 16 observation columns, the ninth v, Rt, A): per statistic 64 chains
//   load up to 8 partials each in one batch and merge them with Chan's formula,
//   then the 64 chain results merge in a six-level tree in LDS.  The
//   normalisers are updated in place (obs_norm's count by the ninth, from the
//   copy of the old count k_adv_scan left in the workspace, which the other
//   eight read); out4 and the four scalars of the elementwise pass are written.
// k_adv_norm: advantages = (A - mu) / (sigma + 1e-8), returns =
//   clamp((Rt - m') rsqrt(s'), +-5), four elements per thread.
// The order of every sum is fixed by the shape alone: two calls on the same
// inputs give the same bits.
#include <hip/hip_runtime.h>
#include "bb_advantages_dev.h"
#include "bb_launch.h"

namespace bb {

constexpr int ADV_FIN_THREADS = ADV_FIN_COLS * ADV_FIN_CHAINS;

// red: [4 waves][2][128] sums, then [4] row counts
__device__ void adv_obs_role(const AdvArgs &a, int group, int groups, double *red)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c4 = lane & 31;
    const int64_t rows = a.worlds * a.steps;
    float sh[4];
#pragma unroll
    for (int j = 0; j < 4; j++) sh[j] = (float)a.on.mean[4 * c4 + j];
    double S[4] = {0.0, 0.0, 0.0, 0.0}, Q[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int64_t r0 = (int64_t)group * ADV_OBS_ROWS; r0 < rows; r0 += (int64_t)groups * ADV_OBS_ROWS) {
        const int64_t rw = r0 + wave * (2 * ADV_OBS_LOADS) + half;
        float4 x[ADV_OBS_LOADS];
#pragma unroll
        for (int u = 0; u < ADV_OBS_LOADS; u++) {  // a row past the end re-reads the last row and is not used
            const int64_t r = rw + 2 * u;
            x[u] = *(const float4 *)(a.obs + (r < rows ? r : rows - 1) * ADV_OBS + 4 * c4);
        }
        float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < ADV_OBS_LOADS; u++) {
            const bool ok = rw + 2 * u < rows;
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
    double *rs = red + wave * 2 * ADV_OBS, *rn = red + 4 * 2 * ADV_OBS;
#pragma unroll
    for (int j = 0; j < 4; j++) {  // the wave's two rows per load: lanes l and l + 32 hold the same columns
        const double s = S[j] + __shfl_xor(S[j], 32), q = Q[j] + __shfl_xor(Q[j], 32);
        if (half == 0) {
            rs[4 * c4 + j] = s;
            rs[ADV_OBS + 4 * c4 + j] = q;
        }
    }
    cnt += __shfl_xor(cnt, 32);
    if (lane == 0) rn[wave] = (double)cnt;
    __syncthreads();
    if (tid < ADV_OBS) {
        double s = 0.0, q = 0.0, n = 0.0;
        for (int w = 0; w < ADV_THREADS / 64; w++) {
            s = s + red[w * 2 * ADV_OBS + tid]; q = q + red[w * 2 * ADV_OBS + ADV_OBS + tid]; n = n + rn[w];
        }
        const Moments mo = adv_moments(n, (double)(float)a.on.mean[tid], s, q);
        double *dst = a.ws + ADV_WS_HEAD + ADV_GAE_GROUPS * ADV_WS_GAE + (int64_t)group * ADV_WS_OBS;
        dst[tid] = mo.mean;
        dst[ADV_OBS + tid] = mo.m2;
        if (tid == 0) dst[2 * ADV_OBS] = mo.n;
    }
}

__global__ __launch_bounds__(ADV_THREADS) void k_adv_scan(AdvArgs a, int gae_groups, int obs_groups)
{
    __shared__ double red[4 * 2 * ADV_OBS + 4];
    const int g = (int)blockIdx.x;
    if (g == 0 && threadIdx.x == 0) a.ws[2] = a.on.count[0];  // k_adv_finish's workgroups read this copy
    if (g < gae_groups) adv_gae_role(a, g, gae_groups, red);
    else adv_obs_role(a, g - gae_groups, obs_groups, red);
}

__global__ __launch_bounds__(ADV_FIN_THREADS) void k_adv_finish(AdvArgs a, int gae_groups, int obs_groups)
{
    __shared__ Moments sm[ADV_FIN_CHAINS][ADV_FIN_COLS];
    const int tid = (int)threadIdx.x, c = tid & (ADV_FIN_COLS - 1), j = tid / ADV_FIN_COLS;
    const bool obs = (int)blockIdx.x < ADV_OBS / ADV_FIN_COLS;
    const int col = (int)blockIdx.x * ADV_FIN_COLS + c;
    const double *gp = a.ws + ADV_WS_HEAD, *op = gp + ADV_GAE_GROUPS * ADV_WS_GAE;
    Moments mo{0.0, 0.0, 0.0};
    if (obs) {
        Moments part[ADV_FIN_BATCH];
#pragma unroll
        for (int u = 0; u < ADV_FIN_BATCH; u++) {  // a partial past the last re-reads partial 0 with n = 0
            const int p = j + ADV_FIN_CHAINS * u;
            const double *src = op + (int64_t)(p < obs_groups ? p : 0) * ADV_WS_OBS;
            part[u] = Moments{p < obs_groups ? src[2 * ADV_OBS] : 0.0, src[col], src[ADV_OBS + col]};
        }
#pragma unroll
        for (int u = 0; u < ADV_FIN_BATCH; u++) adv_merge(mo, part[u]);
    } else if (c < 3 && j < gae_groups) {  // v, Rt, A
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
    if (obs && j == 0) {
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

__global__ __launch_bounds__(256) void k_adv_norm(float *adv, float *ret, int64_t n, const float *scalars, int vec)
{
    const float sc[4] = {scalars[0], scalars[1], scalars[2], scalars[3]};
    const int64_t e = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (e >= n) return;
    if (vec && e + 4 <= n) {
        float4 x = *(const float4 *)(adv + e), r = *(const float4 *)(ret + e);
        x.x = adv_norm_a(x.x, sc); x.y = adv_norm_a(x.y, sc); x.z = adv_norm_a(x.z, sc); x.w = adv_norm_a(x.w, sc);
        r.x = adv_norm_r(r.x, sc); r.y = adv_norm_r(r.y, sc); r.z = adv_norm_r(r.z, sc); r.w = adv_norm_r(r.w, sc);
        *(float4 *)(adv + e) = x;
        *(float4 *)(ret + e) = r;
        return;
    }
    for (int64_t i = e; i < e + 4 && i < n; i++) {
        adv[i] = adv_norm_a(adv[i], sc);
        ret[i] = adv_norm_r(ret[i], sc);
    }
}

int64_t advantages_workspace_bytes(int32_t steps, int64_t worlds)
{
    const AdvGrid g = adv_grid(steps, worlds);
    return (int64_t)sizeof(double) * (ADV_WS_HEAD + ADV_GAE_GROUPS * ADV_WS_GAE + (int64_t)g.obs * ADV_WS_OBS);
}

hipError_t launch_advantages(const AdvArgs &a, hipStream_t s)
{
    const AdvGrid g = adv_grid(a.steps, a.worlds);
    hipLaunchKernelGGL(k_adv_scan, dim3(g.gae + g.obs), dim3(ADV_THREADS), 0, s, a, g.gae, g.obs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_adv_finish, dim3(ADV_OBS / ADV_FIN_COLS + 1), dim3(ADV_FIN_THREADS), 0, s, a, g.gae, g.obs);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_adv_norm(a, s);
}

hipError_t launch_adv_norm(const AdvArgs &a, hipStream_t s)
{
    const int64_t n = a.worlds * a.steps;
    const int vec = ((((uintptr_t)a.adv) | ((uintptr_t)a.ret)) & 15u) == 0;
    hipLaunchKernelGGL(k_adv_norm, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, s, a.adv, a.ret, n,
                       (const float *)a.ws, vec);
    return hipGetLastError();
}

// Host executor: scalar loops in the reference's order, every sum in double.
// in_dim: the observation width (128, or bb_advantages_wide.hip's).
void host_advantages(const AdvArgs &a, int in_dim)
{
    const int K = a.steps;
    const int64_t W = a.worlds, rows = W * K;
    const float m = (float)a.vn.mean[0], sq = __builtin_sqrtf((float)a.vn.var[0] + 1e-5f);
    const double shift = (double)m;
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t w = 0; w < W; w++) {
        float nxt = adv_unnorm(m, sq, a.next_value[w]), nnt = 1.f - a.done[(int64_t)(K - 1) * W + w], last = 0.f;
        for (int t = K - 1; t >= 0; t--) {
            const int64_t at = (int64_t)t * W + w;
            const float v = adv_unnorm(m, sq, a.value[at]);
            const float adv = adv_gae_step(a.reward[at], v, nxt, nnt, a.gamma, a.gl, &last);
            const float rt = adv + v;
            a.adv[at] = adv;
            a.ret[at] = rt;
            const double dv = (double)v - shift, dr = (double)rt - shift, da = (double)adv;
            sum[0] += dv; sum[1] += dv * dv; sum[2] += dr; sum[3] += dr * dr; sum[4] += da; sum[5] += da * da;
            nxt = v;
            nnt = 1.f - a.done[at];
        }
    }
    double S[ADV_OBS_MAX], Q[ADV_OBS_MAX], sh[ADV_OBS_MAX];
    for (int c = 0; c < in_dim; c++) { S[c] = 0.0; Q[c] = 0.0; sh[c] = (double)(float)a.on.mean[c]; }
    for (int64_t r = 0; r < rows; r++)
        for (int c = 0; c < in_dim; c++) {
            const double d = (double)a.obs[r * in_dim + c] - sh[c];
            S[c] += d; Q[c] += d * d;
        }
    double count = a.on.count[0];
    for (int c = 0; c < in_dim; c++) {
        count = a.on.count[0];
        adv_update(a.on.mean[c], a.on.var[c], count, adv_moments((double)rows, sh[c], S[c], Q[c]));
    }
    a.on.count[0] = count;
    float sc[4];
    adv_finish_scalars(a.vn, adv_moments((double)rows, shift, sum[0], sum[1]),
                       adv_moments((double)rows, shift, sum[2], sum[3]), adv_moments((double)rows, 0.0, sum[4], sum[5]),
                       a.out4, sc);
    for (int64_t i = 0; i < rows; i++) {
        a.adv[i] = adv_norm_a(a.adv[i], sc);
        a.ret[i] = adv_norm_r(a.ret[i], sc);
    }
}

}  // namespace bb
