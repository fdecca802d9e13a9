// What the single-workgroup solvers over the edge graph share (fc_geodesic_fps.hip, fc_logmap.hip): the graph, the flagged
// pull-relaxation to the least fixpoint and the workgroup scan.  See the header of fc_geodesic_fps.hip for why the relaxation
// reaches the least fixpoint whatever the schedule.
#pragma once
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"

namespace fc {

constexpr int kGfThreads = 1024;
constexpr int kGfWaves = kGfThreads / 64;
// Vertices of a range solved in LDS.  Sampling keeps 7 B per vertex (distance, two dirty buffers, taken), a ball 6 B:
// 140 000 B of the CU's 163 840, beside the static scratch of the workgroup reductions.
constexpr int kGfLdsVertices = 20000;

struct gf_graph {
    const int32_t* rowptr;       // (V+1) CSR over the vertices of all meshes
    const int32_t* nbr;          // (E)
    const float* len;            // (E)
    int32_t V, E;
};

__device__ __forceinline__ int64_t gf_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the neighbours of local vertex i (inside the range) get flag[u] = 1; the whole workgroup shares the row
__device__ __forceinline__ void gf_flag_neighbours(const gf_graph& g, int v0, int n, int i, uint8_t* flag, int t) {
    const int e0 = max(g.rowptr[v0 + i], 0), e1 = min(g.rowptr[v0 + i + 1], g.E);
    for (int e = e0 + t; e < e1; e += kGfThreads) {
        const int u = g.nbr[e] - v0;
        if ((unsigned)u < (unsigned)n) flag[u] = 1;
    }
}

// Pull-relaxation of the flagged vertices to the fixpoint (see the header of fc_geodesic_fps.hip).  Called by the whole
// workgroup after a barrier; every sweep ends in one, the last included.  Candidates must be < bound (+inf: no bound).
// Returns the sweeps; the last changes nothing.
__device__ __forceinline__ int gf_relax(const gf_graph& g, int v0, int n, float* d, uint8_t*& cur, uint8_t*& nxt, float bound, int t) {
    int sw = 0;
    for (;;) {
        int changed = 0;
        for (int i = t; i < n; i += kGfThreads) {
            if (!cur[i]) continue;
            cur[i] = 0;
            const int e0 = max(g.rowptr[v0 + i], 0), e1 = min(g.rowptr[v0 + i + 1], g.E);
            const float old = d[i];
            float best = old;
            for (int e = e0; e < e1; ++e) {
                const int u = g.nbr[e] - v0;
                if ((unsigned)u < (unsigned)n) {
                    const float c = d[u] + g.len[e];
                    best = (c < best && c < bound) ? c : best;
                }
            }
            if (best < old) {
                d[i] = best;
                changed = 1;
                for (int e = e0; e < e1; ++e) {
                    const int u = g.nbr[e] - v0;
                    if ((unsigned)u < (unsigned)n) nxt[u] = 1;
                }
            }
        }
        ++sw;
        uint8_t* const s = cur;
        cur = nxt, nxt = s;
        if (!__syncthreads_or(changed) || sw > n) break;
    }
    return sw;
}

// exclusive prefix of pred over the workgroup (thread order) and the total; two barriers
__device__ __forceinline__ int gf_scan(bool pred, int t, int* s_wave, int& total) {
    const unsigned long long b = __ballot(pred);
    const int lane = t & 63, w = t >> 6;
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[w] = __popcll(b);
    __syncthreads();
    int below = 0;
    total = 0;
    for (int i = 0; i < kGfWaves; ++i) {
        const int c = s_wave[i];
        below += i < w ? c : 0;
        total += c;
    }
    __syncthreads();
    return below + before;
}

// ---- host side
inline bool gf_graph_ok(const int32_t* rowptr, const int32_t* nbr, const float* len, int32_t V, int32_t E) {
    return rowptr && V >= 1 && E >= 0 && (E == 0 || (nbr && len));
}

// dynamic LDS above 64 KiB has to be allowed once per device and kernel
inline int gf_allow_lds(const void* kernel, bool* done, size_t most) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return FC_ERR_LAUNCH;
    if (!done[dev]) {
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess) return FC_ERR_LAUNCH;
        done[dev] = true;
    }
    return FC_OK;
}

}  // namespace fc
