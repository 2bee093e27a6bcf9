// bb_policy_grad_wide.hip -- PPO's minibatch loss and gradient on gfx950 at the
// observation widths of the 2v2 to 5v5 games, IN = 184, 264, 344 or 424 floats
// (bb_policy_grad.h has the row math, bb_policy_grad_dev.h the tile's device
// functions from the first LayerNorm on, bb_policy_wide.h layer 1's order).
//
// k_ppo_grad (bb_policy_grad.hip) keeps dW1 in 16 accumulator blocks and the
// normalised tile xs[16][132] per wave in LDS; at 424 inputs that would be 54
// blocks (216 registers) and 27 KB per wave.  Here dW1 is a pass of its own:
//
// pass 1, k_ppo_grad_wide<IN>: everything except dW1.  Workgroups of up to
//   PGW_WAVES = 8 waves (2 per SIMD), 16-row tiles per wave in a grid-stride
//   loop.  LDS per workgroup: k_policy_wide's W1 image w1[32][32 NC + 4] and
//   norm[2][32 NC], PolicyLdsWeights' w2 / wh / cst, the row-major w2r / whr of
//   the data gradients, and h1, h2, lg [16][33] per wave (no copy of xn).
//   Layer 1 streams the gathered row idx[row0 + c] in NC chunks of 32 floats as
//   k_policy_wide does: lane (c, q) two aligned 16-byte loads per chunk, a ring
//   of three chunks, the wave's next tile's first two chunks in flight under
//   the last two.  Each chunk's 32 terms are summed from zero (even / odd
//   MFMA chains of 16 terms per output half) and the NC chunk sums added up in
//   chunk order: with up to 424 terms two running chains of 224 were the
//   gradient's largest rounding error (through the logits into exp(lp - lp_old),
//   a relative error of every element).  A quarter past the
//   row's end and a dead row (past m, or an index outside the buffer) feed
//   x = 0 (their loads stay inside the buffer: the row's first floats / row 0).
//   From the first LayerNorm on the tile runs k_ppo_grad's steps; dz1 is not
//   multiplied into dW1 but stored, dz1[16 tiles][32] in the workspace, 2 KB
//   per tile as 16-byte stores (a dead row's dz1 is zero: its dlogit is).
//   After the loop the waves add b1, both LayerNorms' parameters, W2, b2,
//   head_w, head_b and the four loss sums (PGW_SMALL = 1 880 floats) into one
//   LDS image in wave order; one partial per workgroup.
//
// pass 2, k_ppo_dw1<IN>: dW1[32][IN] = sum over rows of dz1^T . xn on
//   v_mfma_f32_16x16x4_f32.  IN = 8 mod 16: NB = ceil(IN / 16) = 12, 17, 22, 27
//   column blocks of 16, the last one half inside the row, cut into NS = 2, 3,
//   4, 4 slabs of SB = 6, 6, 6, 7 adjacent blocks (2 SB <= 14 accumulator
//   blocks, 56 registers).  A wave owns one slab and takes 16-row tiles in a
//   grid-stride loop, the accumulators living across it.  k-step s of a tile:
//   A = dz1[row0 + 4s + q][16m + c], B = xn of obs[idx[row0 + 4s + q]][col0 +
//   16n + c] read straight from the buffer (16 lanes: 64 contiguous bytes; the
//   second read of rows pass 1 pulled through L2) and normalised with the
//   lane's own per-column mean and inverse deviation (loop-invariant
//   registers).  Columns from IN on feed zero and are never stored.  A
//   workgroup is TW x NS waves, TW <= PD_WAVES / NS = 8, 5, 4, 4 waves per slab;
//   they add in LDS in wave order and the workgroup stores one [32][IN] partial.
//
// reduce, k_ppo_grad_wide_reduce: pg_tree_sum's fixed tree over either set of
//   partials, the 10 gradient tensors (head rows 20..31 zero) and loss4.
// No atomics: the same inputs give the same bits on every call.
//
// Grid rules (tiles = ceil(M / 16), at most one workgroup per CU, fewer waves
// per workgroup at small M so that every CU gets work):
//   pass 1  waves = clamp(ceil(tiles / 256), 1, 8), workgroups = min(256,
//           ceil(tiles / waves)): a wave runs its loop twice from tiles > 2 048;
//   pass 2  TW = clamp(ceil(tiles / 256), 1, PD_WAVES / NS), workgroups =
//           min(256, ceil(tiles / TW)), NS TW waves each: twice from tiles >
//           256 PD_WAVES / NS = 2 048, 1 280, 1 024, 1 024.
#include <hip/hip_runtime.h>
#include "bb_launch.h"
#include "bb_policy_grad_dev.h"
#include "bb_policy_wide.h"

namespace bb {

constexpr int PGW_WAVES = 8;   // pass 1: 2 per SIMD
constexpr int PD_WAVES = 16;   // pass 2: 4 per SIMD, 128 registers each
constexpr int PGW_CUS = 256;   // one workgroup per CU
constexpr int PGW_SMALL = PG_FLOATS - PG_B1;  // a gradient set without W1, and the loss sums: 1 880

struct PgWideWaveLds {
    float h1[16][33];  // relu(LN1)
    float h2[16][33];  // relu(LN2), then dz1
    float lg[16][33];  // logits + value, then dlogit + dvalue, then dz2
};
template <int IN>
struct PgWideWeights {
    static constexpr int NC = pol_wide_chunks(IN), S = 32 * NC + 4;
    float w1[32][S];
    float norm[2][32 * NC];
    float w2[4][32][PWG_P2];  // W2[n][8q + j]
    float wh[4][32][PWG_P2];  // head_w[n][8q + j]
    float cst[7][32];         // b1, ln1_w, ln1_b, b2, ln2_w, ln2_b, head_b
};
template <int IN>
struct PgWideLds {
    union {
        PgWideWeights<IN> wt;   // the forward's B operands and constants
        float red[PGW_SMALL];   // after the loop: the workgroup's small gradients
    } u;
    float w2r[32][33];              // W2[n][k], row-major
    float whr[PG_HEAD_LIVE][33];    // head_w[n][k], the 20 live rows
    PgWideWaveLds wv[PGW_WAVES];
};
static_assert(sizeof(PgWideWeights<184>) >= PGW_SMALL * sizeof(float), "the gradient image fits the weights' place");
static_assert(sizeof(PgWideLds<424>) <= 160 * 1024, "LDS of a gfx950 workgroup");

struct PpoGradWideArgs {
    PpoGradArgs g;     // obs [rows][IN], w.w1 / g.w1 [32][IN]; partial: [groups 1][PGW_SMALL]
    float *dz1;        // [16 tiles][32]
    float *partial_w1; // [groups 2][32][IN]
};

// A lane's 8 floats of one chunk.
struct PgChunk {
    float4 lo, hi;
};

template <int IN>
__global__ __launch_bounds__(64 * PGW_WAVES) void k_ppo_grad_wide(const PpoGradWideArgs aw)
{
    using Lds = PgWideLds<IN>;
    constexpr int NC = PgWideWeights<IN>::NC;
    static_assert(pol_wide_width(IN) && NC >= 3, "observation width");
    __shared__ __attribute__((aligned(16))) Lds L;
    const PpoGradArgs &a = aw.g;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int nt = (int)blockDim.x, nw = nt >> 6;
    const int64_t tiles = (a.m + 15) / 16;
    const int64_t tw0 = (int64_t)blockIdx.x * nw + wave, tstride = (int64_t)gridDim.x * nw;
    const float inv_m = 1.0f / (float)a.m;
    const bool tail_in = 32 * (NC - 1) + 8 * q < IN;  // the last chunk's quarters inside the row
    // chunk v of buffer row src: always a read inside the buffer (row 0 for a
    // dead row, float 0.. for a quarter past the row's end)
    const auto load_chunk = [&](int64_t src, int v) {
        const int64_t r = src >= 0 ? src : 0;
        const int off = (v < NC - 1 || tail_in) ? 32 * v + 8 * q : 0;
        const float4 *p = (const float4 *)(a.obs + r * IN + off);
        PgChunk x;
        x.lo = p[0];
        x.hi = p[1];
        return x;
    };
    // the first tile's first two chunks in flight under the weight copy
    int64_t src = tw0 < tiles ? ppo_src_row(a.idx, a.rows, a.m, tw0 * 16 + c) : -1;
    PgChunk n0 = load_chunk(src, 0), n1 = load_chunk(src, 1);
    policy_wide_weights_to_lds<IN>(L.u.wt, a.w, tid, nt);
    for (int i = tid; i < 32 * 32; i += nt) L.w2r[i >> 5][i & 31] = a.w.w2[i];
    for (int i = tid; i < PG_HEAD_LIVE * 32; i += nt) L.whr[i >> 5][i & 31] = a.w.head_w[i];
    __syncthreads();
    PgWideWaveLds &T = L.wv[wave];

    f32x4 gw2[2][2], gwh[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) gw2[m][n] = gwh[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float db1[2] = {0.f, 0.f}, dg1[2] = {0.f, 0.f}, dbt1[2] = {0.f, 0.f};
    float db2[2] = {0.f, 0.f}, dg2[2] = {0.f, 0.f}, dbt2[2] = {0.f, 0.f};
    float dhb[2] = {0.f, 0.f}, loss[4] = {0.f, 0.f, 0.f, 0.f};

    for (int64_t tl = tw0; tl < tiles; tl += tstride) {
        const int64_t row0 = tl * 16;
        // the wave's next tile (this one again after the last: the loads are dropped)
        const int64_t src_next = tl + tstride < tiles ? ppo_src_row(a.idx, a.rows, a.m, (tl + tstride) * 16 + c) : src;
        const int64_t src_b = ppo_src_row(a.idx, a.rows, a.m, row0 + (lane >> 2));  // the bucket pass's row
        const bool live = src >= 0;
        // an offset the compiler cannot see through: the LDS operand reads stay
        // inside the loop instead of being hoisted into live registers
        int z = 0;
        __asm__ volatile("" : "+v"(z));
        const Lds &Lz = *(const Lds *)((const char *)&L + z);
        const float (*cs)[32] = Lz.u.wt.cst;
        PgChunk ring[3];
        ring[0] = n0;
        ring[1] = n1;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;  // the chunk sums added up, per output half
#pragma unroll
        for (int v = 0; v < NC; v++) {
            // chunk v + 2's loads, or the next tile's chunk 0 / 1
            if (v + 2 < NC) ring[(v + 2) % 3] = load_chunk(src, v + 2);
            else if (v + 2 == NC) n0 = load_chunk(src_next, 0);
            else n1 = load_chunk(src_next, 1);
            const PgChunk xc = ring[v % 3];
            const float o[8] = {xc.lo.x, xc.lo.y, xc.lo.z, xc.lo.w, xc.hi.x, xc.hi.y, xc.hi.z, xc.hi.w};
            const int k0 = 32 * v + 8 * q;
            const bool keep = live && (v < NC - 1 || tail_in);
            float x[8], w0[8], w1[8];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const float4 m4 = *(const float4 *)&Lz.u.wt.norm[0][k0 + 4 * h];
                const float4 i4 = *(const float4 *)&Lz.u.wt.norm[1][k0 + 4 * h];
                const float4 u0 = *(const float4 *)&Lz.u.wt.w1[c][k0 + 4 * h];
                const float4 u1 = *(const float4 *)&Lz.u.wt.w1[16 + c][k0 + 4 * h];
                x[4 * h] = pol_clamp((o[4 * h] - m4.x) * i4.x);
                x[4 * h + 1] = pol_clamp((o[4 * h + 1] - m4.y) * i4.y);
                x[4 * h + 2] = pol_clamp((o[4 * h + 2] - m4.z) * i4.z);
                x[4 * h + 3] = pol_clamp((o[4 * h + 3] - m4.w) * i4.w);
                w0[4 * h] = u0.x; w0[4 * h + 1] = u0.y; w0[4 * h + 2] = u0.z; w0[4 * h + 3] = u0.w;
                w1[4 * h] = u1.x; w1[4 * h + 1] = u1.y; w1[4 * h + 2] = u1.z; w1[4 * h + 3] = u1.w;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = keep ? x[j] : 0.f;
            f32x4 acc[2][2];  // [chain: even / odd j][output half], from zero in every chunk
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                acc[j & 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], w0[j], acc[j & 1][0], 0, 0, 0);
                acc[j & 1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], w1[j], acc[j & 1][1], 0, 0, 0);
            }
            a0 = a0 + (acc[0][0] + acc[1][0]);
            a1 = a1 + (acc[0][1] + acc[1][1]);
            __asm__ volatile("" : "+v"(a0), "+v"(a1));  // added here, not after the last chunk with every chunk's sums live
            __builtin_amdgcn_sched_barrier(0);
        }
        float xh1[2][4], rstd1[4], xh2[2][4], rstd2[4];
        pg_ln_forward(a0, a1, cs[0], cs[1], cs[2], T.h1, c, q, xh1[0], xh1[1], rstd1);
        pol_wave_sync();
        pg_tail_forward(Lz.u.wt.w2, Lz.u.wt.wh, cs, T.h1, T.h2, T.lg, c, q, xh2[0], xh2[1], rstd2);
        pg_bucket_pass(a, T.lg, lane, src_b, inv_m, loss);
        // heads backwards: dhead_w += dhead^T . h2, dh2 = dhead . head_w
        pg_weight_grad<2, 33>(gwh, T.lg, T.h2, c, q, dhb);
        f32x4 d0, d1;
        pg_data_grad<PG_HEAD_LIVE / 4>(T.lg, Lz.whr, c, q, d0, d1);
        pg_ln_backward(d0, d1, T.h2, xh2[0], xh2[1], rstd2, cs[4], T.lg, c, q, dg2, dbt2, db2);  // dz2 -> lg
        pg_weight_grad<2, 33>(gw2, T.lg, T.h1, c, q, nullptr);
        pg_data_grad<8>(T.lg, Lz.w2r, c, q, d0, d1);
        pg_ln_backward(d0, d1, T.h1, xh1[0], xh1[1], rstd1, cs[1], T.h2, c, q, dg1, dbt1, db1);  // dz1 -> h2
        // the tile's dz1[16][32] to the workspace: 512 contiguous floats
        float4 *dz = (float4 *)(aw.dz1 + row0 * 32);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int f = 4 * (64 * k + lane), r = f >> 5, col = f & 31;
            dz[64 * k + lane] = make_float4(T.h2[r][col], T.h2[r][col + 1], T.h2[r][col + 2], T.h2[r][col + 3]);
        }
        pol_wave_sync();
        src = src_next;
    }

    // the waves' sums into one image, in wave order
    __syncthreads();  // every wave is done with the weights
    float *red = L.u.red;
    const auto put = [&](int at, float v, bool first) { red[at - PG_B1] = first ? v : red[at - PG_B1] + v; };
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
    float *dst = a.partial + (int64_t)blockIdx.x * PGW_SMALL;
    for (int i = tid; i < PGW_SMALL; i += nt) dst[i] = red[i];
}

// The column split of pass 2 at width IN.
template <int IN>
struct PgDw1Split {
    static constexpr int NB = (IN + 15) / 16;       // column blocks of 16
    static constexpr int NS = (NB + 6) / 7;         // slabs of at most 7 blocks
    static constexpr int SB = (NB + NS - 1) / NS;   // blocks per slab
    static constexpr int TW = PD_WAVES / NS;        // waves per slab in a workgroup, at most
};

template <int IN>
__global__ __launch_bounds__(64 * PD_WAVES) void k_ppo_dw1(const PpoGradWideArgs aw)
{
    using Sp = PgDw1Split<IN>;
    constexpr int NS = Sp::NS, SB = Sp::SB;
    static_assert(pol_wide_width(IN) && 2 * SB <= 14 && NS * SB * 16 >= IN, "column slabs");
    __shared__ __attribute__((aligned(16))) float red[32][IN];
    const PpoGradArgs &a = aw.g;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int nt = (int)blockDim.x, tw = (nt >> 6) / NS;  // the workgroup: tw waves per slab
    const int slab = wave % NS, tq = wave / NS;
    const int64_t tiles = (a.m + 15) / 16;
    const int64_t t0 = (int64_t)blockIdx.x * tw + tq, tstride = (int64_t)gridDim.x * tw;
    const int col0 = 16 * SB * slab + c;  // the lane's column of block 0
    // the lane's columns (block n: col0 + 16n; read at 0 where that is past the row): mean, inverse deviation
    float mean[SB], inv[SB];
#pragma unroll
    for (int n = 0; n < SB; n++) {
        const int col = col0 + 16 * n;
        mean[n] = col < IN ? a.w.obs_mean[col] : 0.f;
        inv[n] = col < IN ? a.w.obs_inv[col] : 0.f;
    }
    f32x4 acc[2][SB];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < SB; n++) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int64_t tl = t0; tl < tiles; tl += tstride) {
        const int64_t row0 = tl * 16;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int64_t src = ppo_src_row(a.idx, a.rows, a.m, row0 + 4 * s + q);
            const bool live = src >= 0;
            const float *orow = a.obs + (live ? src : 0) * IN;  // (a dead row: row 0, dropped)
            const float *dz = aw.dz1 + (row0 + 4 * s + q) * 32;
            const float a0 = dz[c], a1 = dz[16 + c];
            float b[SB];
#pragma unroll
            for (int n = 0; n < SB; n++) b[n] = orow[col0 + 16 * n < IN ? col0 + 16 * n : 0];
#pragma unroll
            for (int n = 0; n < SB; n++) {
                const float xn = pol_clamp((b[n] - mean[n]) * inv[n]);
                b[n] = (live && col0 + 16 * n < IN) ? xn : 0.f;
            }
#pragma unroll
            for (int n = 0; n < SB; n++) {
                acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[n], acc[0][n], 0, 0, 0);
                acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[n], acc[1][n], 0, 0, 0);
            }
        }
    }

    // the slab's waves add in wave order; block (m, n) holds dW1[16m + 4q + i][col0 + 16n]
    for (int t = 0; t < tw; t++) {
        if (tq == t) {
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int n = 0; n < SB; n++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int col = col0 + 16 * n;
                        if (col < IN) {
                            float &r = red[16 * m + 4 * q + i][col];
                            r = t == 0 ? acc[m][n][i] : r + acc[m][n][i];
                        }
                    }
        }
        __syncthreads();
    }
    float *dst = aw.partial_w1 + (int64_t)blockIdx.x * (32 * IN);
    for (int i = tid; i < 32 * IN; i += nt) dst[i] = (&red[0][0])[i];
}

// Element e of the wide gradient: elements [0, 32 IN) are dW1, summed over pass
// 2's partials, the PGW_SMALL behind them the rest and the losses, summed over
// pass 1's, both in pg_tree_sum's fixed tree; then the head's zero rows.  32 IN
// is a multiple of 64: a workgroup's 64 elements are on one side.
__global__ __launch_bounds__(256) void k_ppo_grad_wide_reduce(const float *partial_w1, int groups_w1,
                                                              const float *partial, int groups, int w1_floats,
                                                              PolicyGrads g, float *loss4)
{
    __shared__ float chain[4][64];
    const int e = (int)(blockIdx.x * 64 + threadIdx.x), t = (int)threadIdx.y;
    const bool in_w1 = e < w1_floats;
    const float v = pg_tree_sum(in_w1 ? partial_w1 : partial, in_w1 ? groups_w1 : groups, in_w1 ? e : e - w1_floats,
                                chain, in_w1 ? w1_floats : PGW_SMALL);
    if (t != 0) return;
    if (in_w1) g.w1[e] = v;
    else pg_store_small(e - w1_floats + PG_B1, v, g, loss4);
}

struct PpoGradWideGrid {
    int waves, groups;      // pass 1
    int tw, groups_w1;      // pass 2: waves per slab, workgroups
};
static PpoGradWideGrid ppo_grad_wide_grid(int in_dim, int64_t m)
{
    const int ns = ((in_dim + 15) / 16 + 6) / 7;
    const int64_t tiles = (m + 15) / 16;
    const auto rule = [&](int64_t wmax, int *waves, int *groups) {
        int64_t w = (tiles + PGW_CUS - 1) / PGW_CUS;
        w = w < 1 ? 1 : (w > wmax ? wmax : w);
        int64_t g = (tiles + w - 1) / w;
        g = g < 1 ? 1 : (g > PGW_CUS ? PGW_CUS : g);
        *waves = (int)w;
        *groups = (int)g;
    };
    PpoGradWideGrid gr;
    rule(PGW_WAVES, &gr.waves, &gr.groups);
    rule(PD_WAVES / ns, &gr.tw, &gr.groups_w1);
    return gr;
}

// dz1 [16 tiles][32], then pass 1's partials, then pass 2's (16-byte aligned each)
static int64_t wide_dz1_floats(int64_t m) { return (m + 15) / 16 * 512; }

int64_t ppo_grad_wide_workspace_bytes(int in_dim, int64_t m)
{
    if (!pol_wide_width(in_dim) || m <= 0) return 0;
    const PpoGradWideGrid gr = ppo_grad_wide_grid(in_dim, m);
    return (wide_dz1_floats(m) + (int64_t)gr.groups * PGW_SMALL + (int64_t)gr.groups_w1 * 32 * in_dim) *
           (int64_t)sizeof(float);
}

template <int IN>
static hipError_t launch_ppo_grad_wide_t(const PpoGradWideArgs &aw, const PpoGradWideGrid &gr, hipStream_t s)
{
    static_assert(PgDw1Split<IN>::TW * PgDw1Split<IN>::NS <= PD_WAVES, "pass 2's workgroup");
    hipLaunchKernelGGL(k_ppo_grad_wide<IN>, dim3(gr.groups), dim3(64 * gr.waves), 0, s, aw);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ppo_dw1<IN>, dim3(gr.groups_w1), dim3(64 * gr.tw * PgDw1Split<IN>::NS), 0, s, aw);
    return hipGetLastError();
}

// Passes 1 and 2 alone: where their partials lie in the workspace, and how many.
hipError_t launch_ppo_grad_wide_partials(const PpoGradArgs &a, int in_dim, void *workspace, hipStream_t s,
                                         PpoGradWidePartials *out)
{
    if (!pol_wide_width(in_dim) || a.m <= 0) return hipErrorInvalidValue;
    const PpoGradWideGrid gr = ppo_grad_wide_grid(in_dim, a.m);
    PpoGradWideArgs aw;
    aw.g = a;
    aw.dz1 = (float *)workspace;
    aw.g.partial = aw.dz1 + wide_dz1_floats(a.m);
    aw.partial_w1 = aw.g.partial + (int64_t)gr.groups * PGW_SMALL;
    *out = PpoGradWidePartials{aw.g.partial, gr.groups, aw.partial_w1, gr.groups_w1};
    switch (in_dim) {
    case 184: return launch_ppo_grad_wide_t<184>(aw, gr, s);
    case 264: return launch_ppo_grad_wide_t<264>(aw, gr, s);
    case 344: return launch_ppo_grad_wide_t<344>(aw, gr, s);
    default: return launch_ppo_grad_wide_t<424>(aw, gr, s);
    }
}

hipError_t launch_ppo_grad_wide(const PpoGradArgs &a, int in_dim, void *workspace, hipStream_t s)
{
    PpoGradWidePartials pt;
    const hipError_t e = launch_ppo_grad_wide_partials(a, in_dim, workspace, s, &pt);
    if (e != hipSuccess) return e;
    const int w1_floats = 32 * in_dim, items = w1_floats + PGW_SMALL + PG_HEAD_PAD;
    hipLaunchKernelGGL(k_ppo_grad_wide_reduce, dim3((items + 63) / 64), dim3(64, 4), 0, s, pt.partial_w1, pt.groups_w1,
                       pt.partial, pt.groups, w1_floats, a.g, a.loss4);
    return hipGetLastError();
}

}  // namespace bb
