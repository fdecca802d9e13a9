// The vertex-classification head: a linear layer fused with cross-entropy (and with the arg-max / top-k prediction).
//   z = h W^T + b          h (N,H), W (K,H), b (K) or null: a torch.nn.Linear; float32
//   loss_n = lse_n - sum_k q_nk z_nk,  lse_n = log sum_k exp z_nk,  q_nk = conf at the target, off elsewhere (conf + (K-1) off = 1)
// The N x K logits never exist in memory: every kernel recomputes the 64 x 64 tile it needs with ONE routine, logit_tile, on the
// fp32 matrix pipe (v_mfma_f32_16x16x4_f32), so a logit has the same bits in the loss, in the gradients and in fc_linear_topk
// (entry (n,k) is a sum over H in chunk order that depends on nothing but row n of h and row k of W).
//   fc_linear_ce_forward           lc_walk_kernel<0>: workgroup (row tile, part) walks its share of the class tiles and keeps per row
//                                  the running maximum m, s = sum exp(z - m), the target's logit and the plain sum of the logits
//                                  (label smoothing); lc_finish_kernel merges the parts of a row IN PART ORDER, writes lse and the
//                                  per-row loss and sums the rows in double in a fixed order (fc_loss.hip's scheme).
//   fc_linear_topk                 lc_walk_kernel<1|2|4|8>: the same walk with a sorted list of the best (z, class) per row (BestLogit,
//                                  fc_select.hpp: why the result cannot depend on parts); parts_merge_kernel merges the parts.
//   fc_linear_ce_backward_input    G = g_n (exp(z - lse_n) - q) recomputed tile by tile, g_h = G W accumulated in registers over ALL
//                                  class tiles by the workgroup that owns the row tile: no partial sums.
//   fc_linear_ce_backward_weight   the workgroup that owns a class tile accumulates g_W = G^T h and g_b = column sums of G over its
//                                  share of the row tiles; lc_sum_parts_kernel adds the parts in order.
// No atomics; every sum runs in a fixed order: two runs give the same bits.  Everything lives in caller-owned buffers.
#include "fc_common.hpp"
#include "fc_kernels.hpp"
#include "fc_select.hpp"
#include "fc_workspace.hpp"

namespace fc {

constexpr int kLcTile = 64;                  // rows and classes of a logit tile
constexpr int kLcChunk = 32;                 // entries of H per LDS chunk
constexpr int kLcThreads = 256;
constexpr int kLcStride = kLcTile + 16;      // operand chunks [k][row]: the four k rows of a fragment read fall into distinct bank groups
constexpr int kLcPitch = kLcTile + 4;        // the z / G tile
constexpr int kLcPer = kLcTile * kLcChunk / kLcThreads;
constexpr int kLcHBlock = 256;               // columns of g_h / g_W held in registers per walk (H beyond it: another walk)
constexpr int kLcMaxParts = 64;
constexpr int kLcMaxK = 8;
constexpr int kLcTargetGroups = 1024;        // parts = 0: about four workgroups per CU ...
constexpr int kLcMinTilesPerPart = 4;        // ... but no part shorter than four tiles
constexpr int kLcSumThreads = 1024;
constexpr int kLcSumWaves = kLcSumThreads / 64;

struct LcDims {
    int N, H, K;
};

__device__ __forceinline__ int lc_swz(int k) { return (k >> 2) & 7; }

// The logits of rows r0 .. r0 + 63 and classes c0 .. c0 + 63: acc[i][j][t] = z[r0 + wm + 16 i + 4 fq + t][c0 + wn + 16 j + fr] for
// wavefront quarter (wm, wn) and lane (fr, fq).  Rows, classes and entries of H outside the problem are staged as zeros (nothing
// outside the matrices is read).  Every thread of the workgroup must call it; it synchronises before it touches As / Bs.
__device__ __forceinline__ void logit_tile(const float* __restrict__ h, const float* __restrict__ W, const float* __restrict__ bias,
                                           const LcDims d, const int r0, const int c0, float (&As)[kLcChunk][kLcStride],
                                           float (&Bs)[kLcChunk][kLcStride], f32x4 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fq = lane >> 4;
    const int sk = tid & (kLcChunk - 1), sm = tid / kLcChunk;          // staged element j: row / class sm + 8 j, entry sk of the chunk
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < d.H; k0 += kLcChunk) {
        float ra[kLcPer], rb[kLcPer];
        const int k = k0 + sk;
#pragma unroll
        for (int j = 0; j < kLcPer; ++j) {
            const int row = r0 + sm + (kLcThreads / kLcChunk) * j, cls = c0 + sm + (kLcThreads / kLcChunk) * j;
            ra[j] = (row < d.N && k < d.H) ? h[(size_t)row * d.H + k] : 0.f;
            rb[j] = (cls < d.K && k < d.H) ? W[(size_t)cls * d.H + k] : 0.f;
        }
        __syncthreads();                     // the products of the chunk before (and the caller's use of the tile before) are done
#pragma unroll
        for (int j = 0; j < kLcPer; ++j) {
            const int m = sm + (kLcThreads / kLcChunk) * j;
            As[sk][m ^ lc_swz(sk)] = ra[j];
            Bs[sk][m ^ lc_swz(sk)] = rb[j];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kLcChunk; ks += 4) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = As[ks + fq][(wm + 16 * i + fr) ^ lc_swz(ks)];
                b[i] = Bs[ks + fq][(wn + 16 * i + fr) ^ lc_swz(ks)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cls = c0 + wn + 16 * j + fr;
        const float bv = (bias && cls < d.K) ? bias[cls] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[i][j][t] += bv;
    }
}

// (m, s) <- (m, s) merged with (m2, s2): the maximum and the sum of exponentials relative to it.  Order matters in the last bit:
// every caller merges in a documented order.
__device__ __forceinline__ void lse_merge(float& m, float& s, const float m2, const float s2) {
    const float mn = fmaxf(m, m2), mo = mn == -INFINITY ? 0.f : mn;
    s = s * expf(m - mo) + s2 * expf(m2 - mo);
    m = mn;
}

// Workgroup (row tile, part).  Thread (row, q) = (tid / 4, tid % 4) reads classes 16 q .. 16 q + 15 of every tile of its row from
// the tile in LDS, in class order; the four threads of a row are merged in q order, then (second launch) the parts in part order.
// KL = 0: the loss statistics, float4 (m, s, z_target, sum z) at stat[part N + n].  KL > 0: the KL best, at (part N + n) k + j.
template <int KL>
__global__ __launch_bounds__(kLcThreads) void lc_walk_kernel(const float* __restrict__ h, const float* __restrict__ W,
                                                             const float* __restrict__ bias, const int64_t* __restrict__ target,
                                                             const LcDims d, const int parts, float4* __restrict__ stat,
                                                             float* __restrict__ wsZ, int* __restrict__ wsC, const int k) {
    constexpr int KA = KL > 0 ? KL : 1;
    __shared__ float As[kLcChunk][kLcStride], Bs[kLcChunk][kLcStride];
    __shared__ float Zs[kLcTile][kLcPitch];
    __shared__ float Lz[kLcTile][4][KA];
    __shared__ int Lc[kLcTile][4][KA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fq = lane >> 4;
    const int r0 = blockIdx.x * kLcTile, part = blockIdx.y;
    const int tiles = (d.K + kLcTile - 1) / kLcTile, per = (tiles + parts - 1) / parts;
    const int t0 = min(part * per, tiles), t1 = min(t0 + per, tiles);
    const int row = tid >> 2, q = tid & 3, n = r0 + row;
    int tgt = -1;
    if (KL == 0 && n < d.N) {
        const int64_t tg = target[n];
        tgt = (tg >= 0 && tg < d.K) ? (int)tg : -1;
    }
    float m = -INFINITY, s = 0.f, zt = 0.f, sz = 0.f;
    float lz[KA];
    int lc[KA];
    list_clear<BestLogit>(lz, lc);
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * kLcTile;
        f32x4 acc[2][2];
        logit_tile(h, W, bias, d, r0, c0, As, Bs, acc);          // (its barriers also separate the reads of Zs below from these writes)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int u = 0; u < 4; ++u) Zs[wm + 16 * i + 4 * fq + u][wn + 16 * j + fr] = acc[i][j][u];
        __syncthreads();
        const int cbase = c0 + 16 * q, cnt = min(16, d.K - cbase);
        if (cnt <= 0) continue;
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = Zs[row][16 * q + u];
        if constexpr (KL == 0) {
            float tmax = -INFINITY;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (u < cnt) tmax = fmaxf(tmax, v[u]);
            const float mn = fmaxf(m, tmax), mo = mn == -INFINITY ? 0.f : mn;
            float e = 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (u < cnt) {
                    e += expf(v[u] - mo);
                    sz += v[u];
                    if (cbase + u == tgt) zt = v[u];
                }
            s = s * expf(m - mo) + e;
            m = mn;
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (u < cnt) list_insert<BestLogit>(lz, lc, v[u], cbase + u);
        }
    }
    if constexpr (KL == 0) {
        // the four threads of a row are neighbours in one wavefront: every one of them merges q = 0, 1, 2, 3 in that order
        float M = -INFINITY, S = 0.f, ZT = 0.f, SZ = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int src = (lane & ~3) + j;
            const float mj = __shfl(m, src, 64), sj = __shfl(s, src, 64);
            lse_merge(M, S, mj, sj);
            ZT += __shfl(zt, src, 64);          // (one of the four holds it, the others 0)
            SZ += __shfl(sz, src, 64);
        }
        if (q == 0 && n < d.N) stat[(size_t)part * d.N + n] = make_float4(M, S, ZT, SZ);
    } else {
#pragma unroll
        for (int j = 0; j < KA; ++j) {
            Lz[row][q][j] = lz[j];
            Lc[row][q][j] = lc[j];
        }
        __syncthreads();
        if (q == 0 && n < d.N) {
            for (int p = 1; p < 4; ++p)
#pragma unroll
                for (int j = 0; j < KA; ++j) list_insert<BestLogit>(lz, lc, Lz[row][p][j], Lc[row][p][j]);
#pragma unroll
            for (int j = 0; j < KA; ++j) {
                if (j >= k) break;
                const size_t e = ((size_t)part * d.N + n) * k + j;
                wsZ[e] = lz[j];
                wsC[e] = lc[j];
            }
        }
    }
}

// One workgroup.  Thread t takes rows t, t + 1024, ...: the parts of a row merged in part order, lse and the row's loss written,
// the losses and the number of counted rows summed in double (wavefront xor tree, then the wavefronts in index order).
// total[0] = sum, total[1] = sum / counted rows, total[2] = counted rows (rows whose target is not ignore_index).
__global__ __launch_bounds__(kLcSumThreads) void lc_finish_kernel(const float4* __restrict__ stat, const int64_t* __restrict__ target,
                                                                  const LcDims d, const int parts, const float conf, const float off,
                                                                  const int64_t ignore, float* __restrict__ lse, float* __restrict__ rows,
                                                                  float* __restrict__ total) {
    __shared__ double slots[kLcSumWaves];
    double sum = 0, cnt = 0;
    for (int n = threadIdx.x; n < d.N; n += kLcSumThreads) {
        float M = -INFINITY, S = 0.f, ZT = 0.f, SZ = 0.f;
        for (int p = 0; p < parts; ++p) {
            const float4 v = stat[(size_t)p * d.N + n];
            lse_merge(M, S, v.x, v.y);
            ZT += v.z;
            SZ += v.w;
        }
        const float l = M + logf(S);
        const int64_t tg = target[n];
        float loss = 0.f;
        if (tg != ignore) {
            cnt += 1;
            if (tg < 0 || tg >= d.K) loss = __builtin_nanf("");
            else loss = off != 0.f ? l - (conf * ZT + off * (SZ - ZT)) : l - conf * ZT;
        }
        lse[n] = l;
        rows[n] = loss;
        sum += (double)loss;
    }
    sum = block_sum<kLcSumWaves>(sum, slots);
    cnt = block_sum<kLcSumWaves>(cnt, slots);
    if (threadIdx.x == 0) {
        total[0] = (float)sum;
        total[1] = (float)(sum / cnt);
        total[2] = (float)cnt;
    }
}

// What the backward kernels know of a row: lse, the upstream scale (0 for an ignored row and for rows outside the matrix, NaN for a
// target outside [0,K) that is not ignore_index) and the target (-1: none).
__device__ __forceinline__ void lc_row_info(const int n, const LcDims d, const int64_t* __restrict__ target, const float* __restrict__ lse,
                                            const float* __restrict__ scale, const int64_t ignore, float& rl, float& rg, int& rt) {
    rl = 0.f, rg = 0.f, rt = -1;
    if (n >= d.N) return;
    const int64_t tg = target[n];
    rl = lse[n];
    if (tg == ignore) return;
    const bool in = tg >= 0 && tg < d.K;
    rg = in ? scale[n] : __builtin_nanf("");
    rt = in ? (int)tg : -1;
}

// G[n][k] = g_n (exp(z - lse_n) - q_nk); exactly 0 where g_n is 0 (ignored rows: their lse may be anything) and outside the matrix
__device__ __forceinline__ float lc_grad_logit(const float z, const float rl, const float rg, const int rt, const int cls, const int K,
                                               const float conf, const float off) {
    const float p = expf(z - rl) - (cls == rt ? conf : off);
    return (rg == 0.f || cls >= K) ? 0.f : rg * p;
}

// Workgroup = row tile.  g_h (64 x H) in registers: wavefront w owns columns hb + 64 w .. hb + 64 w + 63 of a 256-column block.
__global__ __launch_bounds__(kLcThreads) void lc_bwd_input_kernel(const float* __restrict__ h, const float* __restrict__ W,
                                                                  const float* __restrict__ bias, const int64_t* __restrict__ target,
                                                                  const float* __restrict__ lse, const float* __restrict__ scale,
                                                                  const LcDims d, const float conf, const float off, const int64_t ignore,
                                                                  float* __restrict__ g_h) {
    __shared__ float As[kLcChunk][kLcStride], Bs[kLcChunk][kLcStride];
    __shared__ float Gs[kLcTile][kLcPitch];          // [class][row]
    __shared__ float rl[kLcTile], rg[kLcTile];
    __shared__ int rt[kLcTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fq = lane >> 4;
    const int r0 = blockIdx.x * kLcTile;
    const int tiles = (d.K + kLcTile - 1) / kLcTile;
    if (tid < kLcTile) lc_row_info(r0 + tid, d, target, lse, scale, ignore, rl[tid], rg[tid], rt[tid]);
    for (int hb = 0; hb < d.H; hb += kLcHBlock) {
        const int col0 = hb + wave * 64;
        f32x4 o[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < tiles; ++t) {
            const int c0 = t * kLcTile;
            f32x4 acc[2][2];
            logit_tile(h, W, bias, d, r0, c0, As, Bs, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int r = wm + 16 * i + 4 * fq + u, c = wn + 16 * j + fr;
                        Gs[c][r] = lc_grad_logit(acc[i][j][u], rl[r], rg[r], rt[r], c0 + c, d.K, conf, off);
                    }
            __syncthreads();
            if (col0 < d.H) {          // (uniform over the wavefront)
#pragma unroll 4
                for (int ks = 0; ks < kLcTile; ks += 4) {
                    const int cls = c0 + ks + fq;
                    float a[4], b[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int col = col0 + 16 * i + fr;
                        a[i] = Gs[ks + fq][16 * i + fr];
                        b[i] = (cls < d.K && col < d.H) ? W[(size_t)cls * d.H + col] : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[i][j] = mfma16(a[i], b[j], o[i][j]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int n = r0 + 16 * i + 4 * fq + u, col = col0 + 16 * j + fr;
                    if (n < d.N && col < d.H) g_h[(size_t)n * d.H + col] = o[i][j][u];
                }
    }
}

// Workgroup (class tile, part): its share of the row tiles.  g_W (64 x H) in registers as above; g_b by threads 0 .. 63, one class
// each, the rows of a tile in row order.  gW / gb: the outputs (parts = 1) or the partials [part][K H] / [part][K]; either may be null.
__global__ __launch_bounds__(kLcThreads) void lc_bwd_weight_kernel(const float* __restrict__ h, const float* __restrict__ W,
                                                                   const float* __restrict__ bias, const int64_t* __restrict__ target,
                                                                   const float* __restrict__ lse, const float* __restrict__ scale,
                                                                   const LcDims d, const float conf, const float off, const int64_t ignore,
                                                                   const int parts, float* __restrict__ gW, float* __restrict__ gb) {
    __shared__ float As[kLcChunk][kLcStride], Bs[kLcChunk][kLcStride];
    __shared__ float Gs[kLcTile][kLcPitch];          // [row][class]
    __shared__ float rl[kLcTile], rg[kLcTile];
    __shared__ int rt[kLcTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fq = lane >> 4;
    const int c0 = blockIdx.x * kLcTile, part = blockIdx.y;
    const int tiles = (d.N + kLcTile - 1) / kLcTile, per = (tiles + parts - 1) / parts;
    const int t0 = min(part * per, tiles), t1 = min(t0 + per, tiles);
    const int hblocks = gW ? (d.H + kLcHBlock - 1) / kLcHBlock : 1;          // (bias gradient alone: one walk, no products)
    for (int hbi = 0; hbi < hblocks; ++hbi) {
        const int col0 = hbi * kLcHBlock + wave * 64;
        const bool product = gW && col0 < d.H;
        f32x4 o[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        float bsum = 0.f;
        for (int t = t0; t < t1; ++t) {
            const int r0 = t * kLcTile;
            // (the reads of rl / rg / rt for the tile before ended ahead of its barrier below)
            if (tid < kLcTile) lc_row_info(r0 + tid, d, target, lse, scale, ignore, rl[tid], rg[tid], rt[tid]);
            f32x4 acc[2][2];
            logit_tile(h, W, bias, d, r0, c0, As, Bs, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int r = wm + 16 * i + 4 * fq + u, c = wn + 16 * j + fr;
                        Gs[r][c] = lc_grad_logit(acc[i][j][u], rl[r], rg[r], rt[r], c0 + c, d.K, conf, off);
                    }
            __syncthreads();
            if (hbi == 0 && gb && tid < kLcTile)
                for (int r = 0; r < kLcTile; ++r) bsum += Gs[r][tid];
            if (product) {
#pragma unroll 4
                for (int ks = 0; ks < kLcTile; ks += 4) {
                    const int n = r0 + ks + fq;
                    float a[4], b[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int col = col0 + 16 * i + fr;
                        a[i] = Gs[ks + fq][16 * i + fr];
                        b[i] = (n < d.N && col < d.H) ? h[(size_t)n * d.H + col] : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[i][j] = mfma16(a[i], b[j], o[i][j]);
                }
            }
        }
        if (product) {
            float* const dst = gW + (size_t)part * d.K * d.H;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int cls = c0 + 16 * i + 4 * fq + u, col = col0 + 16 * j + fr;
                        if (cls < d.K && col < d.H) dst[(size_t)cls * d.H + col] = o[i][j][u];
                    }
        }
        if (hbi == 0 && gb && tid < kLcTile && c0 + tid < d.K) gb[(size_t)part * d.K + c0 + tid] = bsum;
    }
}

// out[i] = part[0][i] + part[1][i] + ... in part order
__global__ __launch_bounds__(256) void lc_sum_parts_kernel(const float* __restrict__ part, const size_t count, const int parts,
                                                           float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += part[(size_t)p * count + i];
    out[i] = s;
}

}  // namespace fc

namespace {

int lc_tiles(int n) { return (n + fc::kLcTile - 1) / fc::kLcTile; }

// parts = 0 when the tiles of `own` rows or classes each own a workgroup and walk the tiles of `walk` (fc_select.hpp)
int lc_choose_parts(int own, int walk) {
    return fc::parts_auto(lc_tiles(own), lc_tiles(walk), fc::kLcTargetGroups, fc::kLcMaxParts, fc::kLcMinTilesPerPart);
}

bool lc_dims_ok(int32_t N, int32_t H, int32_t K) {
    return N >= 1 && H >= 1 && K >= 1 && N < (1 << 30) && K < (1 << 30) && H <= (1 << 20) && (uint64_t)N * (uint64_t)H < ((uint64_t)1 << 40) &&
           (uint64_t)K * (uint64_t)H < ((uint64_t)1 << 40);
}

bool lc_parts_ok(int32_t parts) { return parts >= 0 && parts <= fc::kLcMaxParts; }

int lc_status() { return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH; }

// The workspaces, for `p` parts: the queries lay them out for the cap on the parts when parts == 0, the entry points for the parts chosen.
float4* lc_forward_ws(fc::Carver& c, int p, int N) { return c.take<float4>((size_t)p * N * sizeof(float4)); }       // a float4 per row and part

struct LcWeightWs { float *W, *b; };                    // partials of g_W and g_b: only when there is more than one part
LcWeightWs lc_weight_ws(fc::Carver& c, int p, int K, int H) {
    if (p <= 1) return {nullptr, nullptr};
    return {c.take<float>((size_t)p * K * H * sizeof(float)), c.take<float>((size_t)p * K * sizeof(float))};
}

struct LcTopkWs { float* z; int* cls; };                // k (logit, class) per row and part
LcTopkWs lc_topk_ws(fc::Carver& c, int p, int N, int k) {
    return {c.take<float>((size_t)p * N * k * sizeof(float)), c.take<int>((size_t)p * N * k * sizeof(int32_t))};
}

}  // namespace

extern "C" {

size_t fc_linear_ce_workspace_bytes(int32_t N, int32_t H, int32_t K, int32_t parts, int32_t pass, int32_t k) {
    if (!lc_dims_ok(N, H, K) || !lc_parts_ok(parts)) return 0;
    if (pass == 2 && (k < 1 || k > fc::kLcMaxK)) return 0;
    const int p = parts == 0 ? fc::parts_cap(lc_tiles(pass == 1 ? K : N), fc::kLcTargetGroups, fc::kLcMaxParts) : parts;
    if (pass == 0) return fc::carved_bytes(lc_forward_ws, p, N);
    if (pass == 1) return fc::carved_bytes(lc_weight_ws, p, K, H);            /* backward, weight side */
    return pass == 2 ? fc::carved_bytes(lc_topk_ws, p, N, k) : 0;
}

int fc_linear_ce_forward(const float* h, const float* weight, const float* bias, const int64_t* target, int32_t N, int32_t H, int32_t K,
                         double confidence, double off_value, int64_t ignore_index, int32_t parts, float* lse, float* loss_rows,
                         float* total, void* workspace, size_t workspace_bytes, void* stream) {
    if (!lc_dims_ok(N, H, K) || !lc_parts_ok(parts) || !h || !weight || !target || !lse || !loss_rows || !total) return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_linear_ce_workspace_bytes(N, H, K, parts, 0, 0)) return FC_ERR_WORKSPACE;
    if (parts == 0) parts = lc_choose_parts(N, K);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fc::LcDims d{N, H, K};
    fc::Carver ws(workspace);
    float4* stat = lc_forward_ws(ws, parts, N);
    hipLaunchKernelGGL(fc::lc_walk_kernel<0>, dim3((unsigned)lc_tiles(N), (unsigned)parts), dim3(fc::kLcThreads), 0, s, h, weight, bias, target,
                       d, parts, stat, (float*)nullptr, (int*)nullptr, 0);
    hipLaunchKernelGGL(fc::lc_finish_kernel, dim3(1), dim3(fc::kLcSumThreads), 0, s, stat, target, d, parts, (float)confidence, (float)off_value,
                       ignore_index, lse, loss_rows, total);
    return lc_status();
}

int fc_linear_topk(const float* h, const float* weight, const float* bias, int32_t N, int32_t H, int32_t K, int32_t k, int32_t parts,
                   int64_t* idx, float* z, void* workspace, size_t workspace_bytes, void* stream) {
    if (!lc_dims_ok(N, H, K) || !lc_parts_ok(parts) || !h || !weight || !idx || !z || k < 1 || k > fc::kLcMaxK) return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_linear_ce_workspace_bytes(N, H, K, parts, 2, k)) return FC_ERR_WORKSPACE;
    if (parts == 0) parts = lc_choose_parts(N, K);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fc::LcDims d{N, H, K};
    fc::Carver ws(workspace);
    const LcTopkWs w = lc_topk_ws(ws, parts, N, k);
    const dim3 grid((unsigned)lc_tiles(N), (unsigned)parts);
    fc::dispatch_k<1, 2, 4, 8>(k, [&](auto rung) {
        constexpr int KL = decltype(rung)::value;
        hipLaunchKernelGGL(fc::lc_walk_kernel<KL>, grid, dim3(fc::kLcThreads), 0, s, h, weight, bias, (const int64_t*)nullptr, d, parts,
                           (float4*)nullptr, w.z, w.cls, k);
        fc::launch_parts_merge<fc::BestLogit, KL>(w.z, w.cls, N, k, parts, idx, z, s);
    });
    return lc_status();
}

int fc_linear_ce_backward_input(const float* h, const float* weight, const float* bias, const int64_t* target, const float* lse,
                                const float* row_scale, int32_t N, int32_t H, int32_t K, double confidence, double off_value,
                                int64_t ignore_index, float* grad_h, void* stream) {
    if (!lc_dims_ok(N, H, K) || !h || !weight || !target || !lse || !row_scale || !grad_h) return FC_ERR_BAD_ARGUMENT;
    const fc::LcDims d{N, H, K};
    hipLaunchKernelGGL(fc::lc_bwd_input_kernel, dim3((unsigned)lc_tiles(N)), dim3(fc::kLcThreads), 0, static_cast<hipStream_t>(stream), h, weight,
                       bias, target, lse, row_scale, d, (float)confidence, (float)off_value, ignore_index, grad_h);
    return lc_status();
}

int fc_linear_ce_backward_weight(const float* h, const float* weight, const float* bias, const int64_t* target, const float* lse,
                                 const float* row_scale, int32_t N, int32_t H, int32_t K, double confidence, double off_value,
                                 int64_t ignore_index, int32_t parts, float* grad_weight, float* grad_bias, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!lc_dims_ok(N, H, K) || !lc_parts_ok(parts) || !h || !weight || !target || !lse || !row_scale || (!grad_weight && !grad_bias))
        return FC_ERR_BAD_ARGUMENT;
    const size_t need = fc_linear_ce_workspace_bytes(N, H, K, parts, 1, 0);
    if (need && (!workspace || workspace_bytes < need)) return FC_ERR_WORKSPACE;
    if (parts == 0) parts = lc_choose_parts(K, N);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fc::LcDims d{N, H, K};
    const size_t nW = (size_t)K * H;
    float* pW = grad_weight;
    float* pb = grad_bias;
    if (parts > 1) {
        fc::Carver ws(workspace);
        const LcWeightWs w = lc_weight_ws(ws, parts, K, H);
        pW = grad_weight ? w.W : nullptr;
        pb = grad_bias ? w.b : nullptr;
    }
    hipLaunchKernelGGL(fc::lc_bwd_weight_kernel, dim3((unsigned)lc_tiles(K), (unsigned)parts), dim3(fc::kLcThreads), 0, s, h, weight, bias, target,
                       lse, row_scale, d, (float)confidence, (float)off_value, ignore_index, parts, pW, pb);
    if (parts > 1) {
        if (grad_weight)
            hipLaunchKernelGGL(fc::lc_sum_parts_kernel, dim3((unsigned)((nW + 255) / 256)), dim3(256), 0, s, pW, nW, parts, grad_weight);
        if (grad_bias)
            hipLaunchKernelGGL(fc::lc_sum_parts_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, pb, (size_t)K, parts, grad_bias);
    }
    return lc_status();
}

}  // extern "C"
