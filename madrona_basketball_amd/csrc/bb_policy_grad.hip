// bb_policy_grad.hip -- PPO's minibatch update on gfx950 up to param.grad
// (scripts/ppo.py:190-213: get_minibatch, get_stats, the three losses,
// backward) as one pass over the minibatch rows: gather, forward, loss and
// backward of the 128 -> 32 -> 32 -> 20 network per 16-row tile, the weight
// gradients accumulated on the chip (bb_policy_grad.h has the row math).
//
// k_ppo_grad: workgroups of up to PG_WAVES waves, each wave taking 16-row tiles
// in a grid-stride loop over the M minibatch rows.  Per tile, lane (c = l & 15,
// q = l >> 4):
//   gather   lane (c, q) loads floats 32q..32q+31 of buffer row idx[row0 + c]
//            (no gathered copy of obs is made), normalises them (xn) and
//            leaves a copy in the wave's LDS tile xs[16][132];
//   forward  as k_policy_wg (v_mfma_f32_16x16x4_f32, B operands from the
//            workgroup's LDS images): h1, h2 and the logits into [16][33] LDS
//            tiles, xhat and rstd of both LayerNorms in the C/D layout
//            (rows 4q + i, columns c and c + 16) in registers;
//   buckets  4 lanes per row (a DPP quad), lane part p takes buckets p and
//            p + 4: p, log p, H; log-prob and entropy summed over the quad by
//            DPP; surrogate and value loss; dloss/dlogit and dloss/dv written
//            over the logits tile;
//   backward data gradients dh2 = dhead . head_w (5 k-steps: 20 live head rows)
//            and dh1 = dz2 . W2 (8 k-steps) as MFMA with the row-major weight
//            matrices read untransposed from LDS (B[k = 4s + q][n = 16t + c]),
//            their results in the C/D layout where the LayerNorm backward is
//            two quarter-wave DPP sums per row; dz2 / dz1 written over the dead
//            logits / h2 tiles;
//   weights  dW = dz^T . in with the reduction over the tile's 16 rows (four
//            k-steps, A = dz[4s + q][16m + c], B = in[4s + q][16n + c]) into
//            accumulators that live across the whole loop: 16 blocks of 16 x 16
//            for dW1, 4 each for dW2 and dhead_w (96 registers); bias and
//            LayerNorm-parameter gradients as per-lane column partials.
// After the loop the waves add their registers into one LDS image of the
// gradient in wave order (a barrier between waves), and the workgroup stores it
// as its partial.  k_ppo_grad_reduce sums the partials of each element in a
// fixed order and writes the gradient tensors and the losses.  No atomics: the
// same inputs give the same bits on every call.
#include <hip/hip_runtime.h>
#include <vector>
#include "bb_launch.h"
#include "bb_policy_grad_dev.h"

namespace bb {

constexpr int PG_WAVES = 8;   // 2 per SIMD: 256 registers each
constexpr int PG_CUS = 256;   // one workgroup per CU (LDS)
constexpr int PG_XS = 132;    // xs row stride: 16-byte rows, 4 banks of skew

struct PgWaveLds {
    float xs[16][PG_XS];  // xn
    float h1[16][33];     // relu(LN1)
    float h2[16][33];     // relu(LN2), then dz1
    float lg[16][33];     // logits + value, then dlogit + dvalue, then dz2
};
struct PgLds {
    union {
        PolicyLdsWeights wt;    // the forward's B operands and constants
        float red[PG_FLOATS];   // after the loop: the workgroup's gradient
    } u;
    float w2r[32][33];               // W2[n][k], row-major
    float whr[PG_HEAD_LIVE][33];     // head_w[n][k], the 20 live rows
    PgWaveLds wv[PG_WAVES];
};
static_assert(sizeof(PolicyLdsWeights) >= PG_FLOATS * sizeof(float), "the gradient image fits the weights' place");
static_assert(sizeof(PgLds) <= 160 * 1024, "LDS of a gfx950 workgroup");

__global__ __launch_bounds__(64 * PG_WAVES) void k_ppo_grad(const PpoGradArgs a)
{
    __shared__ __attribute__((aligned(16))) PgLds L;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int nt = (int)blockDim.x, nw = nt >> 6;
    const int64_t tiles = (a.m + 15) / 16;
    const int64_t tw0 = (int64_t)blockIdx.x * nw + wave, tstride = (int64_t)gridDim.x * nw;
    const float inv_m = 1.0f / (float)a.m;
    policy_weights_to_lds(L.u.wt, a.w, tid, nt);
    for (int i = tid; i < 32 * 32; i += nt) L.w2r[i >> 5][i & 31] = a.w.w2[i];
    for (int i = tid; i < PG_HEAD_LIVE * 32; i += nt) L.whr[i >> 5][i & 31] = a.w.head_w[i];
    __syncthreads();
    PgWaveLds &T = L.wv[wave];

    f32x4 gw1[2][8], gw2[2][2], gwh[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
#pragma unroll
        for (int n = 0; n < 8; n++) gw1[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < 2; n++) gw2[m][n] = gwh[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float db1[2] = {0.f, 0.f}, dg1[2] = {0.f, 0.f}, dbt1[2] = {0.f, 0.f};
    float db2[2] = {0.f, 0.f}, dg2[2] = {0.f, 0.f}, dbt2[2] = {0.f, 0.f};
    float dhb[2] = {0.f, 0.f}, loss[4] = {0.f, 0.f, 0.f, 0.f};

    for (int64_t tl = tw0; tl < tiles; tl += tstride) {
        const int64_t row0 = tl * 16;
        // gather: this lane's quarter of buffer row idx[row0 + c]
        const int64_t src = ppo_src_row(a.idx, a.rows, a.m, row0 + c);
        const int64_t src_b = ppo_src_row(a.idx, a.rows, a.m, row0 + (lane >> 2));  // the bucket pass's row
        float x[32];
        if (src >= 0) {
            const float4 *p = (const float4 *)(a.obs + src * POL_IN + 32 * q);
#pragma unroll
            for (int v = 0; v < 8; v++) {
                const float4 o = p[v];
                x[4 * v] = o.x; x[4 * v + 1] = o.y; x[4 * v + 2] = o.z; x[4 * v + 3] = o.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; j++) x[j] = 0.f;
        }
        // an offset the compiler cannot see through: the LDS operand reads stay
        // inside the loop instead of being hoisted into live registers
        int z = 0;
        __asm__ volatile("" : "+v"(z));
        const float (*nrm)[POL_IN] = (const float (*)[POL_IN])(&L.u.wt.norm[0][0] + z);
        const float (*w1l)[32][PWG_P1] = (const float (*)[32][PWG_P1])(&L.u.wt.w1[0][0][0] + z);
        const float (*w2l)[32][PWG_P2] = (const float (*)[32][PWG_P2])(&L.u.wt.w2[0][0][0] + z);
        const float (*whl)[32][PWG_P2] = (const float (*)[32][PWG_P2])(&L.u.wt.wh[0][0][0] + z);
        const float (*cs)[32] = (const float (*)[32])(&L.u.wt.cst[0][0] + z);
        const float (*w2r)[33] = (const float (*)[33])(&L.w2r[0][0] + z);
        const float (*whr)[33] = (const float (*)[33])(&L.whr[0][0] + z);
        // xn, and its copy for the transposed read of dW1's product
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const float4 m4 = *(const float4 *)&nrm[0][32 * q + 4 * v];
            const float4 i4 = *(const float4 *)&nrm[1][32 * q + 4 * v];
            x[4 * v] = pol_clamp((x[4 * v] - m4.x) * i4.x);
            x[4 * v + 1] = pol_clamp((x[4 * v + 1] - m4.y) * i4.y);
            x[4 * v + 2] = pol_clamp((x[4 * v + 2] - m4.z) * i4.z);
            x[4 * v + 3] = pol_clamp((x[4 * v + 3] - m4.w) * i4.w);
            *(float4 *)&T.xs[c][32 * q + 4 * v] = make_float4(x[4 * v], x[4 * v + 1], x[4 * v + 2], x[4 * v + 3]);
        }
        // layer 1 (k_policy_wg's operands, one 4-float group ahead), two chains
        // per output half: shorter sums and four independent MFMAs in flight
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a0, a3 = a0;
        float4 n0 = *(const float4 *)&w1l[q][c][0], n1 = *(const float4 *)&w1l[q][16 + c][0];
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const float w0[4] = {n0.x, n0.y, n0.z, n0.w}, w1[4] = {n1.x, n1.y, n1.z, n1.w};
            if (v + 1 < 8) {
                n0 = *(const float4 *)&w1l[q][c][4 * v + 4];
                n1 = *(const float4 *)&w1l[q][16 + c][4 * v + 4];
            }
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[4 * v + e], w0[e], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[4 * v + e], w1[e], a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[4 * v + e + 1], w0[e + 1], a2, 0, 0, 0);
                a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[4 * v + e + 1], w1[e + 1], a3, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        a0 = a0 + a2;
        a1 = a1 + a3;
        float xh1[2][4], rstd1[4], xh2[2][4], rstd2[4];
        pg_ln_forward(a0, a1, cs[0], cs[1], cs[2], T.h1, c, q, xh1[0], xh1[1], rstd1);
        pol_wave_sync();
        // layer 2, then the heads (k = 8q + j)
        pg_tail_forward(w2l, whl, cs, T.h1, T.h2, T.lg, c, q, xh2[0], xh2[1], rstd2);
        pg_bucket_pass(a, T.lg, lane, src_b, inv_m, loss);
        // heads backwards: dhead_w += dhead^T . h2, dh2 = dhead . head_w
        pg_weight_grad<2, 33>(gwh, T.lg, T.h2, c, q, dhb);
        f32x4 d0, d1;
        pg_data_grad<PG_HEAD_LIVE / 4>(T.lg, whr, c, q, d0, d1);
        pg_ln_backward(d0, d1, T.h2, xh2[0], xh2[1], rstd2, cs[4], T.lg, c, q, dg2, dbt2, db2);  // dz2 -> lg
        pg_weight_grad<2, 33>(gw2, T.lg, T.h1, c, q, nullptr);
        pg_data_grad<8>(T.lg, w2r, c, q, d0, d1);
        pg_ln_backward(d0, d1, T.h1, xh1[0], xh1[1], rstd1, cs[1], T.h2, c, q, dg1, dbt1, db1);  // dz1 -> h2
        pg_weight_grad<8, PG_XS>(gw1, T.h2, T.xs, c, q, nullptr);
        pol_wave_sync();
    }

    // the waves' sums into one image, in wave order
    __syncthreads();  // every wave is done with the weights
    float *red = L.u.red;
    const auto put = [&](int at, float v, bool first) { red[at] = first ? v : red[at] + v; };
    // a column partial summed over the 4 lane groups (fixed order), lane group 0 stores
    const auto col = [&](int at, float (&v)[2], bool first, int limit) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            float s = v[t];
            s = s + __shfl_xor(s, 16);
            s = s + __shfl_xor(s, 32);
            if (q == 0 && 16 * t + c < limit) put(at + 16 * t + c, s, first);
        }
    };
    for (int w = 0; w < nw; w++) {
        if (wave == w) {
            const bool first = w == 0;
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int n = 16 * m + 4 * q + i;
#pragma unroll
                    for (int k = 0; k < 8; k++) put(PG_W1 + n * POL_IN + 16 * k + c, gw1[m][k][i], first);
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        put(PG_W2 + n * POL_HID + 16 * k + c, gw2[m][k][i], first);
                        if (n < PG_HEAD_LIVE) put(PG_HW + n * POL_HID + 16 * k + c, gwh[m][k][i], first);
                    }
                }
            col(PG_B1, db1, first, 32); col(PG_LN1W, dg1, first, 32); col(PG_LN1B, dbt1, first, 32);
            col(PG_B2, db2, first, 32); col(PG_LN2W, dg2, first, 32); col(PG_LN2B, dbt2, first, 32);
            col(PG_HB, dhb, first, PG_HEAD_LIVE);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float s = loss[k];
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m);
                if (lane == 0) put(PG_LOSS + k, s, first);
            }
        }
        __syncthreads();
    }
    float *dst = a.partial + (int64_t)blockIdx.x * PG_FLOATS;
    for (int i = tid; i < PG_FLOATS; i += nt) dst[i] = red[i];
}

// Element e of the gradient: the sum of the workgroups' partials in a fixed
// tree -- four strided chains (thread row t: workgroups t, t + 4, ...), then
// their pairs -- stored into its tensor; the head's rows 20..31 are written as
// zero.  64 elements x 4 chains per workgroup: the chains' loads run side by
// side (one thread per element and all four chains in it: 65.7 us at 256
// partials, profiles/r08).
__global__ __launch_bounds__(256) void k_ppo_grad_reduce(const float *partial, int groups, PolicyGrads g, float *loss4)
{
    __shared__ float chain[4][64];
    const int e = (int)(blockIdx.x * 64 + threadIdx.x), t = (int)threadIdx.y;
    const float v = pg_tree_sum(partial, groups, e, chain);
    if (t != 0) return;
    if (e < PG_B1) g.w1[e] = v;
    else pg_store_small(e, v, g, loss4);
}

// Waves per workgroup and workgroups of a k_ppo_grad launch over `tiles` 16-row
// tiles: one workgroup per CU (256) once there are PG_WAVES tiles per CU,
// fewer waves per workgroup below that so that every CU gets work.
struct PpoGradGrid {
    int waves, groups;
};
static PpoGradGrid ppo_grad_grid(int64_t m)
{
    const int64_t tiles = (m + 15) / 16;
    int64_t w = (tiles + PG_CUS - 1) / PG_CUS;
    w = w < 1 ? 1 : (w > PG_WAVES ? PG_WAVES : w);
    int64_t g = (tiles + w - 1) / w;
    g = g < 1 ? 1 : (g > PG_CUS ? PG_CUS : g);
    return {(int)w, (int)g};
}

int64_t ppo_grad_workspace_bytes(int64_t m)
{
    return (int64_t)ppo_grad_grid(m).groups * PG_FLOATS * (int64_t)sizeof(float);
}

hipError_t launch_ppo_grad_partials(const PpoGradArgs &a, hipStream_t s, int *groups)
{
    const PpoGradGrid gr = ppo_grad_grid(a.m);
    *groups = gr.groups;
    hipLaunchKernelGGL(k_ppo_grad, dim3(gr.groups), dim3(64 * gr.waves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ppo_grad(const PpoGradArgs &a, hipStream_t s)
{
    PpoGradGrid gr;
    hipError_t e = launch_ppo_grad_partials(a, s, &gr.groups);
    if (e != hipSuccess) return e;
    const int items = PG_FLOATS + PG_HEAD_PAD;
    hipLaunchKernelGGL(k_ppo_grad_reduce, dim3((items + 63) / 64), dim3(64, 4), 0, s, a.partial, gr.groups, a.g, a.loss4);
    return hipGetLastError();
}

// The minibatch on the host at in_dim inputs: acc[pg_floats(in_dim)] scratch.
static void host_ppo_grad_rows(const PpoGradArgs &a, int in_dim, double *acc)
{
    const int sh = pg_floats(in_dim) - PG_FLOATS;  // the elements behind W1 sit this much further on
    for (int i = 0; i < PG_FLOATS + sh; i++) acc[i] = 0.0;
    for (int64_t i = 0; i < a.m; i++) ppo_grad_row_host(a, i, acc, in_dim);
    float *dst[10] = {a.g.w1, a.g.b1, a.g.ln1_w, a.g.ln1_b, a.g.w2, a.g.b2, a.g.ln2_w, a.g.ln2_b, a.g.head_w, a.g.head_b};
    const int at[11] = {PG_W1, PG_B1 + sh, PG_LN1W + sh, PG_LN1B + sh, PG_W2 + sh, PG_B2 + sh, PG_LN2W + sh,
                        PG_LN2B + sh, PG_HW + sh, PG_HB + sh, PG_LOSS + sh};
    for (int t = 0; t < 10; t++)
        for (int i = at[t]; i < at[t + 1]; i++) dst[t][i - at[t]] = (float)acc[i];
    for (int i = PG_HEAD_LIVE * POL_HID; i < POL_HEAD * POL_HID; i++) a.g.head_w[i] = 0.f;
    for (int i = PG_HEAD_LIVE; i < POL_HEAD; i++) a.g.head_b[i] = 0.f;
    for (int k = 0; k < 4; k++) a.loss4[k] = (float)acc[PG_LOSS + sh + k];
}

void host_ppo_grad(const PpoGradArgs &a)
{
    double acc[PG_FLOATS];
    host_ppo_grad_rows(a, POL_IN, acc);
}

void host_ppo_grad_wide(const PpoGradArgs &a, int in_dim)
{
    std::vector<double> acc((size_t)pg_floats(in_dim));
    host_ppo_grad_rows(a, in_dim, acc.data());
}

}  // namespace bb
