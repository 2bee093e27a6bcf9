// bb_policy_step_wide.hip -- clip_grad_norm_, Adam's step and the weight repack
// on gfx950 for the policies of 184, 264, 344 and 424 inputs
// (bb_policy_step_wide.h has the element order, bb_policy_step.h the math).
//
// k_ppo_step_wide takes k_ppo_grad_wide_reduce's place behind k_ppo_grad_wide
// and k_ppo_dw1: ceil((E + 4) / 64) = 122 .. 242 workgroups of 64 elements x 4
// chains.  32 IN is a multiple of 64, so a workgroup lies wholly in dW1 (pass
// 2's partials) or wholly in the rest (pass 1's); either way pg_tree_sum is
// called with the reduce's arguments and the gradient has ppo_grad_wide's
// bits.  The unclipped gradient goes to the workspace, the four loss sums to
// the result, and the workgroup's 64 squares are summed in double in a fixed
// cross-lane butterfly: one partial per workgroup.
//
// k_adam_step_wide<WS> is one workgroup of 1 024 threads: nothing waits across
// workgroups and no workgroup reads what another one of the same launch wrote.
//   norm   wave 0 takes the 122 .. 242 partials four per lane (lane l: 4l ..
//          4l + 3, in index order) and runs the butterfly: a fixed order, five
//          dependent double adds and six cross-lane steps instead of a chain of
//          242 on one thread.  <false> (standalone, behind any backward) first
//          sums the squares of the 12 .grad tensors in the same 64-element
//          chunks of the wide order with the same butterfly, so it gives the
//          fused path's bits from the same gradient.
//   walk   ceil(E / 4) or so 4-element items, at most 3 862: four per thread.
//          A thread issues the loads of all four items (g, m, v, p: sixteen
//          16-byte loads where the six pointers allow) before its first store.
//          The stores into the parameter tensor and the packed image may be
//          the same address, so a store between two rounds of loads keeps the
//          compiler from hoisting the second round over it and every round
//          waits out its own HBM latency (bb_policy_step.hip's loop: 1 494
//          items, 1.5 rounds; here it would be four).
// The segment table goes to LDS by static index (a per-lane index into the
// kernel's arguments would put a copy of them into scratch).  Head rows 20-31
// are not touched and have no Adam state.  No ticket form: DESIGN.md section 14
// measured it slower at 128.  No MFMA: reductions and elementwise maps.
// Deterministic: every order of summation is fixed by the shape.
#include <hip/hip_runtime.h>
#include "bb_launch.h"
#include "bb_policy_step_wide.h"

namespace bb {

constexpr int PSW_THREADS = 1024;                 // k_adam_step_wide
constexpr int PSW_ROUNDS = 4;                     // items per thread
constexpr int PSW_SMALL = PG_FLOATS - PG_B1;      // pass 1's partial: everything behind W1, and the loss sums
static_assert((POL_HID * PG_IN_MAX + PSW_SMALL - 4 + 3) / 4 + PS_TENSORS <= PSW_THREADS * PSW_ROUNDS, "four items per thread");
static_assert(PSW_CHUNKS_MAX <= 4 * 64, "four partials per lane of wave 0");

struct StepWideLds {
    StepSeg seg[PS_TENSORS];
    int q0[PS_TENSORS + 1];  // first 4-element item of each segment; [12]: items in all
    AdamScalars sc;
    double sqp[PSW_CHUNKS_MAX];  // <false>: the sum-of-squares partials
};

// The sum over the wave's 64 lanes, the same bits in every lane and on every call.
__device__ __forceinline__ double psw_wave_sum(double s)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m);
    return s;
}

// The segment table into LDS, by static index.  Barrier after it.
__device__ __forceinline__ void step_table_wide(const PolicyStepWideArgs &a, StepWideLds &L, int tid)
{
#pragma unroll
    for (int s = 0; s < PS_TENSORS; s++)
        if (tid == s) L.seg[s] = step_seg_wide(a, s);
    if (tid == 0) {
        int q = 0;
#pragma unroll
        for (int s = 0; s < PS_TENSORS; s++) {
            L.q0[s] = q;
            q += (step_seg_wide(a, s).len + 3) / 4;
        }
        L.q0[PS_TENSORS] = q;
    }
    __syncthreads();
}

// Item `it` of the walk: its six pointers, its elements n (0 past the last
// item) and whether they take 16-byte accesses.
struct StepItem {
    const float *gs;
    float *gd, *pp, *pk, *mm, *vv;
    int n;
    bool vec;
};
template <bool WS>
__device__ __forceinline__ StepItem step_item(const PolicyStepWideArgs &a, const StepWideLds &L, int it)
{
    const bool in = it < L.q0[PS_TENSORS];
    int s = 0;
#pragma unroll
    for (int k = 1; k < PS_TENSORS; k++) s += (in && it >= L.q0[k]) ? 1 : 0;
    const StepSeg sg = L.seg[s];
    const int o = in ? 4 * (it - L.q0[s]) : 0;
    const int e = sg.e0 + o;
    StepItem r;
    r.gs = WS ? a.s.gsum + e : sg.grad + o;
    r.gd = sg.grad + o;
    r.pp = sg.param + o;
    r.pk = sg.packed + o;
    r.mm = a.s.exp_avg + e;
    r.vv = a.s.exp_avg_sq + e;
    r.n = !in ? 0 : (sg.len - o < 4 ? sg.len - o : 4);
    const uintptr_t al = (uintptr_t)r.gs | (uintptr_t)r.gd | (uintptr_t)r.pp | (uintptr_t)r.pk | (uintptr_t)r.mm | (uintptr_t)r.vv;
    r.vec = r.n == 4 && (al & 15u) == 0;
    return r;
}
__device__ __forceinline__ float4 step_ld4(const float *p, int n, bool vec)
{
    if (vec) return *(const float4 *)p;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) r.x = p[0];
    if (n > 1) r.y = p[1];
    if (n > 2) r.z = p[2];
    if (n > 3) r.w = p[3];
    return r;
}
__device__ __forceinline__ void step_st4(float *p, const float4 &x, int n, bool vec)
{
    if (vec) {
        *(float4 *)p = x;
        return;
    }
    if (n > 0) p[0] = x.x;
    if (n > 1) p[1] = x.y;
    if (n > 2) p[2] = x.z;
    if (n > 3) p[3] = x.w;
}

__global__ __launch_bounds__(256) void k_ppo_step_wide(const PolicyStepWideArgs a)
{
    __shared__ float chain[4][64];
    const int x = (int)threadIdx.x, t = (int)threadIdx.y;
    const int e = (int)(blockIdx.x * 64) + x;
    const int w1_floats = POL_HID * a.in_dim, all = pg_floats(a.in_dim);
    const bool in_w1 = e < w1_floats;
    const float v = pg_tree_sum(in_w1 ? a.partial_w1 : a.s.partial, in_w1 ? a.groups_w1 : a.s.groups,
                                in_w1 ? e : e - w1_floats, chain, in_w1 ? w1_floats : PSW_SMALL);
    if (t != 0) return;  // wave 0 holds the 64 sums
    double q = 0.0;
    if (e < all) {
        a.s.gsum[e] = v;
        if (e < all - 4) q = (double)v * (double)v;
        else a.s.out[e - (all - 4)] = v;
    }
    q = psw_wave_sum(q);
    if (x == 0) a.s.sq[blockIdx.x] = q;
}

template <bool WS>
__global__ __launch_bounds__(PSW_THREADS) void k_adam_step_wide(const PolicyStepWideArgs a)
{
    __shared__ StepWideLds L;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int elems = psw_elems(a.in_dim), chunks = psw_chunks(a.in_dim);
    step_table_wide(a, L, tid);
    if (!WS) {
        // k_ppo_step_wide's partials: chunk c = elements 64c .. 64c + 63 of the wide order
        for (int c = wave; c < chunks; c += PSW_THREADS / 64) {
            const int e = 64 * c + lane;
            double q = 0.0;
            if (e < elems) {
                int s = 0;
#pragma unroll
                for (int k = 1; k < PS_TENSORS; k++) s += e >= L.seg[k].e0 ? 1 : 0;
                const float g = L.seg[s].grad[e - L.seg[s].e0];
                q = (double)g * (double)g;
            }
            q = psw_wave_sum(q);
            if (lane == 0) L.sqp[c] = q;
        }
        __syncthreads();
    }
    if (wave == 0) {
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = 4 * lane + k;
            double q = 0.0;
            if (c < chunks) q = WS ? a.s.sq[c] : L.sqp[c];
            sum = sum + q;
        }
        sum = psw_wave_sum(sum);
        if (lane == 0) {
            const int64_t t = *a.s.step + 1;
            *a.s.step = t;
            const AdamScalars sc = adam_scalars(a.s.h, sum, t);
            L.sc = sc;
            a.s.out[WS ? 4 : 0] = sc.norm;
            a.s.out[WS ? 5 : 1] = sc.coef;
        }
    }
    __syncthreads();
    const AdamScalars sc = L.sc;
    float4 g[PSW_ROUNDS], m[PSW_ROUNDS], v[PSW_ROUNDS], p[PSW_ROUNDS];
#pragma unroll
    for (int k = 0; k < PSW_ROUNDS; k++) {  // every load of the thread, before its first store
        const StepItem it = step_item<WS>(a, L, tid + PSW_THREADS * k);
        g[k] = step_ld4(it.gs, it.n, it.vec);
        m[k] = step_ld4(it.mm, it.n, it.vec);
        v[k] = step_ld4(it.vv, it.n, it.vec);
        p[k] = step_ld4(it.pp, it.n, it.vec);
    }
#pragma unroll
    for (int k = 0; k < PSW_ROUNDS; k++) {
        const StepItem it = step_item<WS>(a, L, tid + PSW_THREADS * k);
        g[k].x = adam_element(sc, g[k].x, &m[k].x, &v[k].x, &p[k].x);
        g[k].y = adam_element(sc, g[k].y, &m[k].y, &v[k].y, &p[k].y);
        g[k].z = adam_element(sc, g[k].z, &m[k].z, &v[k].z, &p[k].z);
        g[k].w = adam_element(sc, g[k].w, &m[k].w, &v[k].w, &p[k].w);
        step_st4(it.gd, g[k], it.n, it.vec);
        step_st4(it.mm, m[k], it.n, it.vec);
        step_st4(it.vv, v[k], it.n, it.vec);
        step_st4(it.pp, p[k], it.n, it.vec);
        step_st4(it.pk, p[k], it.n, it.vec);
    }
}

int64_t ppo_step_wide_workspace_bytes(int in_dim, int64_t m)
{
    if (!pol_wide_width(in_dim) || m <= 0) return 0;
    return ppo_grad_wide_workspace_bytes(in_dim, m) + psw_ws_tail_bytes(in_dim);
}

hipError_t launch_adam_step_wide(const PolicyStepWideArgs &a, hipStream_t s)
{
    if (!pol_wide_width(a.in_dim)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_adam_step_wide<false>, dim3(1), dim3(PSW_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ppo_step_wide(const PpoGradArgs &g, PolicyStepWideArgs a, void *workspace, hipStream_t s)
{
    if (!pol_wide_width(a.in_dim) || g.m <= 0) return hipErrorInvalidValue;
    PpoGradWidePartials pt;
    hipError_t e = launch_ppo_grad_wide_partials(g, a.in_dim, workspace, s, &pt);
    if (e != hipSuccess) return e;
    a.s.partial = pt.partial;
    a.s.groups = pt.groups;
    a.partial_w1 = pt.partial_w1;
    a.groups_w1 = pt.groups_w1;
    a.s.gsum = (float *)((char *)workspace + ppo_grad_wide_workspace_bytes(a.in_dim, g.m));
    a.s.sq = (double *)(a.s.gsum + pg_floats(a.in_dim));
    hipLaunchKernelGGL(k_ppo_step_wide, dim3(psw_chunks(a.in_dim)), dim3(64, 4), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_adam_step_wide<true>, dim3(1), dim3(PSW_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace bb
