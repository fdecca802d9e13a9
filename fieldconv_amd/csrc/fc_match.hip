// Descriptor matching: for every row a of xT the k rows b of xS with the smallest d2(a,b), ordered by (d2, b) ascending.
//   fc_match_topk     the dense 64 x 64 x 16-channel LDS tile of fc_twin_count_dense (fc_pair.hpp) with a selection on top of it;
//                     the N_T x N_S matrix never exists.
// d2 is fc_pair.hpp's distance, so a match agrees bit for bit with fc_pair_sqdist and with the counts of fc_twin_count_dense.
// Selection (fc_select.hpp: why no stage below can change a result): NearestRow lists, order (d2, b), so an exact tie goes to
// the lower row and a NaN distance is never kept.
//   lane      (ty, tx) of 16 x 16 owns rows 4 ty .. 4 ty + 3 of the xT tile and columns 4 tx .. 4 tx + 3 of every xS tile of its
//             workgroup's range; it keeps a sorted list of K = 1, 2, 4 or 8 (>= k) entries per row in registers.
//   row       the sixteen tx lanes of a row sit next to each other in one wavefront: four xor-butterfly steps (list_merge_xor).
//   parts     workgroup (tile, p) searches the p-th share of the tile's xS range; with parts > 1 it leaves its list in the
//             workspace and a second launch (parts_merge_kernel) merges the lists of a row.
// Empty slots are written out as d2 = +inf, idx = -1.
#include "../../include/fieldconv_hip.h"
#include "fc_pair.hpp"
#include "fc_select.hpp"
#include "fc_workspace.hpp"

namespace fc {

constexpr int kMatchMaxK = 8;
constexpr int kMatchMaxParts = 1024;
constexpr int kMatchTargetGroups = 1024;     // parts = 0: enough workgroups for 4 per CU on 256 CUs ...
constexpr int kMatchMinTilesPerPart = 4;     // ... but no part shorter than 4 tiles of xS (the row merge is paid once per part)

// ptr entry m clamped to [0, N]: a malformed table can give a meaningless result, never an access outside the features
__device__ __forceinline__ int segment_bound(const int64_t* __restrict__ ptr, int m, int N) {
    const int64_t v = ptr[m];
    return (int)(v < 0 ? 0 : (v > N ? N : v));
}

// Workgroup (g, part): 64 rows of xT against its share of their xS range.  Without tables g is the tile and the range all of xS.
// With them, segment m owns the tile slots base(m) .. base(m+1) - 1, base(m) = ptr_T[m] / 64 + m (integer division): base is
// strictly increasing and base(m+1) - base(m) >= ceil(n_m / 64), so N_T / 64 + B slots suffice whatever the table holds and a
// workgroup finds its segment by bisection (the arrangement of fc_support.hip's batched search); slots past a segment's last
// tile leave at once.  FINAL (parts == 1): the lists go to idx / d2; otherwise to the workspace, entry (part N_T + a) k + j.
template <typename T, int K, bool FINAL>
__global__ __launch_bounds__(kDenseThreads) void match_tile_kernel(const T* __restrict__ xS, int nS, const T* __restrict__ xT, int nT, int C,
                                                                   const int64_t* __restrict__ ptrS, const int64_t* __restrict__ ptrT,
                                                                   int B, const int64_t* __restrict__ exclude, int k, int parts,
                                                                   int64_t* __restrict__ idx, T* __restrict__ d2, T* __restrict__ wsD,
                                                                   int* __restrict__ wsI) {
    __shared__ __attribute__((aligned(16))) T sT[kDenseChunk][kDensePitch];
    __shared__ __attribute__((aligned(16))) T sS[kDenseChunk][kDensePitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, g = blockIdx.x, part = blockIdx.y;
    int a0 = g * kDenseTile, hiT = nT, s0 = 0, hiS = nS;          // xT rows [a0, min(a0 + 64, hiT)), xS rows [s0, hiS)
    if (ptrT) {
        int lo = 0, hi = B - 1;                                  // the largest m with base(m) <= g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segment_bound(ptrT, mid, nT) / kDenseTile + mid <= g) lo = mid;
            else hi = mid - 1;
        }
        const int p0 = segment_bound(ptrT, lo, nT);
        hiT = max(segment_bound(ptrT, lo + 1, nT), p0);
        const long long first = (long long)(g - (p0 / kDenseTile + lo)) * kDenseTile;
        if (first < 0 || first >= hiT - p0) return;
        a0 = p0 + (int)first;
        s0 = segment_bound(ptrS, lo, nS);
        hiS = max(segment_bound(ptrS, lo + 1, nS), s0);
    }
    const int tilesS = (hiS - s0 + kDenseTile - 1) / kDenseTile, per = (tilesS + parts - 1) / parts;
    const int t0 = min(part * per, tilesS), t1 = min(t0 + per, tilesS);

    using Row = NearestRow<T>;
    T bd[4][K];
    int bb[4][K], excl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        list_clear<Row>(bd[i], bb[i]);
        const int a = a0 + 4 * ty + i;
        const int64_t e = (exclude && a < hiT) ? exclude[a] : -1;
        excl[i] = (e >= 0 && e < nS) ? (int)e : -1;
    }
    const bool stage_T_once = C <= kDenseChunk;          // the xT tile is the same for every xS tile: one chunk stays in LDS
    for (int t = t0; t < t1; ++t) {
        const int b0 = s0 + t * kDenseTile;
        T acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0;
        for (int c0 = 0; c0 < C; c0 += kDenseChunk) {
            const int nc = min(kDenseChunk, C - c0);
            const bool stage_T = !stage_T_once || t == t0;
            __syncthreads();
#pragma unroll
            for (int e = tid; e < kDenseTile * kDenseChunk; e += kDenseThreads) {
                const int row = e / kDenseChunk, ch = e % kDenseChunk;
                const bool cin = ch < nc;
                if (stage_T) sT[ch][row] = (cin && a0 + row < hiT) ? xT[(size_t)(a0 + row) * C + c0 + ch] : static_cast<T>(0);
                sS[ch][row] = (cin && b0 + row < hiS) ? xS[(size_t)(b0 + row) * C + c0 + ch] : static_cast<T>(0);
            }
            __syncthreads();
            auto channel = [&](int c) {
                T a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[i] = sT[c][4 * ty + i];
                    b[i] = sS[c][4 * tx + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = d2_step(acc[i][j], a[i], b[j]);
            };
            if (nc == kDenseChunk) {
#pragma unroll
                for (int c = 0; c < kDenseChunk; ++c) channel(c);
            } else {
                for (int c = 0; c < nc; ++c) channel(c);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = b0 + 4 * tx + j;
                if (b < hiS && b != excl[i]) list_insert<Row>(bd[i], bb[i], acc[i][j], b);
            }
    }
    // the sixteen lanes of a row: lanes 16 q .. 16 q + 15 of the wavefront, so xor 1, 2, 4, 8 stays inside the row
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) list_merge_xor<Row>(bd[i], bb[i], m);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = a0 + 4 * ty + i;
        if (tx != i || a >= hiT) continue;          // lane tx = i writes row i: four lanes share the stores
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j >= k) break;
            if (FINAL) {
                idx[(size_t)a * k + j] = bb[i][j] == kSelNone ? -1 : bb[i][j];
                d2[(size_t)a * k + j] = bd[i][j];
            } else {
                const size_t e = ((size_t)part * nT + a) * k + j;
                wsD[e] = bd[i][j];
                wsI[e] = bb[i][j];
            }
        }
    }
}

}  // namespace fc

namespace {

int tiles_of(int n) { return (n + fc::kDenseTile - 1) / fc::kDenseTile; }

// parts = 0: as many parts as fill the card, none shorter than kMatchMinTilesPerPart tiles of xS; the workspace query sizes for the cap
int match_parts_cap(int32_t nT) { return fc::parts_cap(tiles_of(nT), fc::kMatchTargetGroups, fc::kMatchMaxParts); }

// [d2: parts N_T k entries of the dtype][idx: parts N_T k int32]; the query sizes it for 8-byte distances
template <typename T>
struct MatchWs { T* d2; int* idx; };
template <typename T>
MatchWs<T> match_ws(fc::Carver& c, int32_t nT, int32_t k, int parts) {
    const size_t entries = (size_t)parts * (size_t)nT * (size_t)k;
    if (parts <= 1) return {nullptr, nullptr};          // one part writes idx / d2 itself
    return {c.take<T>(entries * sizeof(T)), c.take<int>(entries * sizeof(int32_t))};
}

template <typename T>
int match_topk(const void* xS, int32_t nS, const void* xT, int32_t nT, int32_t C, const int64_t* ptrS, const int64_t* ptrT, int32_t B,
               const int64_t* exclude, int32_t k, int parts, int64_t* idx, void* d2, void* ws, hipStream_t s) {
    fc::Carver c(ws);
    const MatchWs<T> w = match_ws<T>(c, nT, k, parts);
    const dim3 grid((unsigned)(ptrT ? nT / fc::kDenseTile + B : tiles_of(nT)), (unsigned)parts);
    const T *pS = static_cast<const T*>(xS), *pT = static_cast<const T*>(xT);
    T* out = static_cast<T*>(d2);
    fc::dispatch_k<1, 2, 4, 8>(k, [&](auto rung) {
        constexpr int K = decltype(rung)::value;
        if (parts == 1) {
            hipLaunchKernelGGL((fc::match_tile_kernel<T, K, true>), grid, dim3(fc::kDenseThreads), 0, s, pS, nS, pT, nT, C, ptrS, ptrT, B, exclude,
                               k, parts, idx, out, w.d2, w.idx);
        } else {
            hipLaunchKernelGGL((fc::match_tile_kernel<T, K, false>), grid, dim3(fc::kDenseThreads), 0, s, pS, nS, pT, nT, C, ptrS, ptrT, B, exclude,
                               k, parts, idx, out, w.d2, w.idx);
            fc::launch_parts_merge<fc::NearestRow<T>, K>(w.d2, w.idx, nT, k, parts, idx, out, s);
        }
    });
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t fc_match_workspace_bytes(int32_t N_T, int32_t k, int32_t parts) {
    if (N_T < 1 || k < 1 || k > fc::kMatchMaxK || parts < 0 || parts > fc::kMatchMaxParts) return 0;
    return fc::carved_bytes(match_ws<double>, N_T, k, parts == 0 ? match_parts_cap(N_T) : parts);
}

int fc_match_topk(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* ptr_S,
                  const int64_t* ptr_T, int32_t B, const int64_t* exclude, int32_t k, int32_t parts, int64_t* idx, void* d2,
                  void* workspace, size_t workspace_bytes, void* stream) {
    if (!fc::features_ok(xS, N_S, xT, N_T, C, dtype) || !idx || !d2 || k < 1 || k > fc::kMatchMaxK || parts < 0 ||
        parts > fc::kMatchMaxParts || (ptr_S == nullptr) != (ptr_T == nullptr))
        return FC_ERR_BAD_ARGUMENT;
    if (ptr_T && (B < 1 || (int64_t)N_T + (int64_t)fc::kDenseTile * B >= ((int64_t)1 << 31))) return FC_ERR_BAD_ARGUMENT;
    const size_t need = fc_match_workspace_bytes(N_T, k, parts);
    if (need && (!workspace || workspace_bytes < need)) return FC_ERR_WORKSPACE;
    if (parts == 0) parts = fc::parts_auto(tiles_of(N_T), tiles_of(N_S), fc::kMatchTargetGroups, fc::kMatchMaxParts, fc::kMatchMinTilesPerPart);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == 0 ? match_topk<float>(xS, N_S, xT, N_T, C, ptr_S, ptr_T, B, exclude, k, parts, idx, d2, workspace, s)
                      : match_topk<double>(xS, N_S, xT, N_T, C, ptr_S, ptr_T, B, exclude, k, parts, idx, d2, workspace, s);
}

}  // extern "C"
