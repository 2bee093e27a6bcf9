// bb_policy_step.hip -- what follows loss.backward() in one PPO minibatch
// (scripts/ppo.py:214-215), on gfx950: clip_grad_norm_, Adam's step and the
// repack of the new parameters into the packed weight image the next
// k_ppo_grad / bb_policy_forward reads (bb_policy_step.h has the element math).
//
// k_ppo_step takes k_ppo_grad_reduce's place behind k_ppo_grad, same grid idea
// (64 elements x 4 chains per workgroup, 94 workgroups).  Each workgroup:
//   sum     its 64 elements' partials in k_ppo_grad_reduce's tree (pg_tree_sum):
//           the unclipped gradient into the workspace, the 4 loss sums out;
//   square  the 64 squares in double, summed across the wave's lanes in a fixed
//           butterfly: one sum-of-squares partial per workgroup;
//   ticket  every storing lane fences at agent scope (the eight XCDs' L2s are
//           separate), then one acq_rel agent-scope integer atomic add on the
//           ticket.  The only atomic; nobody waits for anybody.
// The workgroup that drew the last ticket sees every other workgroup's stores
// and finishes the step for all 5 972 elements (step_finish): partials added in
// index order, norm and clip factor, step count + 1, bias corrections once (in
// double, through LDS), then per 4-element item (1 494 items over 256 threads,
// 16-byte accesses where all six pointers allow): load g, m, v, p; store the
// clipped g into param.grad, m, v, and p into the parameter tensor and the
// packed image (the two may be the same address: the same value is stored
// twice).  Then the ticket goes back to 0.
//
// k_adam_step<false> is the standalone step after any backward: one workgroup
// of 1 024 threads reads the 12 .grad tensors, sums their squares in the same
// 64-element chunks and the same butterfly (so it gives k_ppo_step's bits from
// the same gradient), then runs step_finish.  k_adam_step<true> runs
// step_finish from k_ppo_step's workspace: bb_policy_ppo_step launches
// k_ppo_step without the ticket and then this (faster than the ticket form,
// see launch_ppo_step; path override ppo_step_ticket = 1 takes the ticket).
// No MFMA: reductions and elementwise maps.  Deterministic: every order of
// summation is fixed by the shape.
#include <hip/hip_runtime.h>
#include "bb_launch.h"
#include "bb_policy_step.h"

namespace bb {

constexpr int PS_FIN_THREADS = 1024;  // k_adam_step

struct StepLds {
    StepSeg seg[PS_TENSORS];
    int q0[PS_TENSORS + 1];  // first 4-element item of each segment; [12]: items in all
    AdamScalars sc;
    double sqp[PS_CHUNKS];   // k_adam_step's sum-of-squares partials
    int last;
};

// The sum over the wave's 64 lanes, the same bits in every lane and on every call.
__device__ __forceinline__ double wave_sum_d(double s)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m);
    return s;
}

// The segment table into LDS, by static index (a per-lane index into the
// kernel's arguments would put a copy of them into scratch).  Barrier after it.
__device__ __forceinline__ void step_table(const PolicyStepArgs &a, StepLds &L, int tid)
{
#pragma unroll
    for (int s = 0; s < PS_TENSORS; s++)
        if (tid == s) L.seg[s] = step_seg(a, s);
    if (tid == 0) {
        int q = 0;
#pragma unroll
        for (int s = 0; s < PS_TENSORS; s++) {
            L.q0[s] = q;
            q += (step_seg(a, s).len + 3) / 4;
        }
        L.q0[PS_TENSORS] = q;
    }
    __syncthreads();
}

// The step for every element from the PS_CHUNKS sum-of-squares partials sq[]
// (index order).  WS: the raw gradient comes from the workspace (a.gsum) and
// norm / coef go behind the four losses; else from the .grad tensors.
template <bool WS>
__device__ __forceinline__ void step_finish(const PolicyStepArgs &a, StepLds &L, const double *sq, int tid, int nt)
{
    if (tid == 0) {
        double sum = 0.0;
#pragma unroll 8
        for (int c = 0; c < PS_CHUNKS; c++) sum = sum + sq[c];
        const int64_t t = *a.step + 1;
        *a.step = t;
        const AdamScalars sc = adam_scalars(a.h, sum, t);
        L.sc = sc;
        a.out[WS ? 4 : 0] = sc.norm;
        a.out[WS ? 5 : 1] = sc.coef;
    }
    __syncthreads();
    const AdamScalars sc = L.sc;
    const int items = L.q0[PS_TENSORS];
    for (int it = tid; it < items; it += nt) {
        int s = 0;
#pragma unroll
        for (int k = 1; k < PS_TENSORS; k++) s += it >= L.q0[k] ? 1 : 0;
        const StepSeg sg = L.seg[s];
        const int o = 4 * (it - L.q0[s]);
        const int n = sg.len - o < 4 ? sg.len - o : 4;
        const int e = sg.e0 + o;
        const float *gs = WS ? a.gsum + e : sg.grad + o;
        float *gd = sg.grad + o, *pp = sg.param + o, *pk = sg.packed + o;
        float *mm = a.exp_avg + e, *vv = a.exp_avg_sq + e;
        const uintptr_t al = (uintptr_t)gs | (uintptr_t)gd | (uintptr_t)pp | (uintptr_t)pk | (uintptr_t)mm | (uintptr_t)vv;
        if (n == 4 && (al & 15u) == 0) {
            float4 g = *(const float4 *)gs, m = *(const float4 *)mm, v = *(const float4 *)vv, p = *(const float4 *)pp;
            g.x = adam_element(sc, g.x, &m.x, &v.x, &p.x);
            g.y = adam_element(sc, g.y, &m.y, &v.y, &p.y);
            g.z = adam_element(sc, g.z, &m.z, &v.z, &p.z);
            g.w = adam_element(sc, g.w, &m.w, &v.w, &p.w);
            *(float4 *)gd = g;
            *(float4 *)mm = m;
            *(float4 *)vv = v;
            *(float4 *)pp = p;
            *(float4 *)pk = p;
        } else {
            for (int j = 0; j < n; j++) {
                float m = mm[j], v = vv[j], p = pp[j];
                gd[j] = adam_element(sc, gs[j], &m, &v, &p);
                mm[j] = m;
                vv[j] = v;
                pp[j] = p;
                pk[j] = p;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_ppo_step(const PolicyStepArgs a, int use_ticket)
{
    __shared__ float chain[4][64];
    __shared__ StepLds L;
    const int x = (int)threadIdx.x, t = (int)threadIdx.y, tid = 64 * t + x;
    const int e = (int)(blockIdx.x * 64) + x;
    const float v = pg_tree_sum(a.partial, a.groups, e, chain);
    if (t == 0) {  // wave 0 holds the 64 sums
        double q = 0.0;
        if (e < PG_FLOATS) {
            a.gsum[e] = v;
            if (e < PG_LOSS) q = (double)v * (double)v;
            else a.out[e - PG_LOSS] = v;
        }
        q = wave_sum_d(q);
        if (x == 0) a.sq[blockIdx.x] = q;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this lane's stores, before the ticket below
    }
    if (!use_ticket) return;
    __syncthreads();
    if (tid == 0) {
        const int got = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        L.last = got == (int)gridDim.x - 1 ? 1 : 0;
    }
    __syncthreads();
    if (!L.last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every lane that reads the others' stores
    step_table(a, L, tid);
    step_finish<true>(a, L, a.sq, tid, 256);
    if (tid == 0) *a.ticket = 0;
}

template <bool WS>
__global__ __launch_bounds__(PS_FIN_THREADS) void k_adam_step(const PolicyStepArgs a)
{
    __shared__ StepLds L;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
    step_table(a, L, tid);
    if (!WS) {
        // k_ppo_step's partials: chunk c = elements 64c .. 64c + 63 of the PG_* order
        for (int c = wave; c < PS_CHUNKS; c += nw) {
            const int e = 64 * c + lane;
            double q = 0.0;
            if (e < PS_ELEMS) {
                int s = 0;
#pragma unroll
                for (int k = 1; k < PS_TENSORS; k++) s += e >= L.seg[k].e0 ? 1 : 0;
                const float g = L.seg[s].grad[e - L.seg[s].e0];
                q = (double)g * (double)g;
            }
            q = wave_sum_d(q);
            if (lane == 0) L.sqp[c] = q;
        }
        __syncthreads();
    }
    step_finish<WS>(a, L, WS ? a.sq : L.sqp, tid, nt);
}

int64_t ppo_step_workspace_bytes(int64_t m) { return ppo_grad_workspace_bytes(m) + PS_WS_TAIL_BYTES; }

hipError_t launch_adam_step(const PolicyStepArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_adam_step<false>, dim3(1), dim3(PS_FIN_THREADS), 0, s, a);
    return hipGetLastError();
}

// The two-launch form (k_ppo_step without the ticket, then k_adam_step<true>)
// is the product's: measured 125.5 us per 65 536-row minibatch against 130.4
// for the ticket form, whose last workgroup walks the 1 494 items with 256
// threads (k_ppo_step 20.5 us) where k_adam_step has 1 024.
// DIAG_PPO_STEP_TICKET = 1 takes the ticket form (tests, A/B timing).
hipError_t launch_ppo_step(PpoGradArgs g, PolicyStepArgs a, void *workspace, hipStream_t s)
{
    g.partial = (float *)workspace;
    hipError_t e = launch_ppo_grad_partials(g, s, &a.groups);
    if (e != hipSuccess) return e;
    a.partial = g.partial;
    a.gsum = (float *)((char *)workspace + ppo_grad_workspace_bytes(g.m));
    a.sq = (double *)(a.gsum + PG_FLOATS);
    const int ticket = diag_or(DIAG_PPO_STEP_TICKET, 0) != 0 ? 1 : 0;
    hipLaunchKernelGGL(k_ppo_step, dim3(PS_CHUNKS), dim3(64, 4), 0, s, a, ticket);
    e = hipGetLastError();
    if (e != hipSuccess || ticket) return e;
    hipLaunchKernelGGL(k_adam_step<true>, dim3(1), dim3(PS_FIN_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace bb
