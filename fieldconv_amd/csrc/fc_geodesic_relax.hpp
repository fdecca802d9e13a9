// The shared core of the single-workgroup solvers over the edge graph (fc_geodesic.hip, fc_geodesic_fps.hip, fc_logmap.hip):
// the graph, the ranges of a mini-batch, the relaxation state of one problem and its flagged pull-relaxation, the workgroup
// scan, and on the host the argument rules and the LDS/global launch pair.  A solver supplies its argument struct (a gf_graph,
// an lds_vertices field), its kernel body in two instantiations <kLds>, and its LDS bytes per vertex.
//
// A workgroup of 1024 threads owns one problem: thread t owns the vertices t, t + 1024, ... of the problem's range, pulls
// d[v] = min(d[v], fl32(d[u] + len(u,v))) over their CSR rows and is the only writer of their distances.
// Why the result is the least fixpoint whatever the schedule.  Reads of neighbours may be stale: every value ever written is
// the rounded length of some path from a source, an upper bound of the least fixpoint, and fl32(a + l) is monotone in a, so the
// least fixpoint is the only state in which a whole sweep over every vertex changes nothing -- whatever the order of the
// relaxations.  A sweep sees at least everything the previous sweep wrote (the barrier), so at most n sweeps change something.
// That is the un-flagged loop of fc_geodesic.hip.  gf_relax pulls a vertex only while its dirty flag is set.  Flags are
// double-buffered: in a sweep the owner reads and clears cur[v]; a vertex whose distance drops sets nxt[u] = 1 on all its
// neighbours; the buffers swap at the barrier.  Take the LAST pull of v, in sweep s: it left d[v] <= fl32(d_read[u] + len) for
// every neighbour u.  If d[u] dropped at or after that read, in a sweep s' >= s, then u set nxt[v] in s' and v was pulled again
// in s' + 1 > s, so it was not the last pull: on every edge d[v] <= fl32(d[u] + len) holds at the end, and that state is the
// fixpoint.  Nothing in this needs an order between a thread's accesses inside a sweep; only the barrier orders.  A flag byte
// is written with the value it is meant to have by whoever writes it (cur: 0 by the owner; nxt: 1 by anyone), so concurrent
// stores agree.  An incremental start is legitimate for the same reason: after d[new] = 0 the state is pointwise an upper bound
// of the new fixpoint, and only the neighbours of `new` can violate their edge condition: they are the ones flagged.
// A bounded field accepts a candidate only if it is < bound; a prefix of a shortest path is never longer than the path (float32
// additions of non-negative lengths are monotone), so it equals the unbounded field wherever that is < bound.
// Loops are bounded by the problem: a relaxation runs at most n + 1 sweeps.  No atomics, nothing crosses a workgroup.
#pragma once
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"

namespace fc {

constexpr int kGfThreads = 1024;
constexpr int kGfWaves = kGfThreads / 64;
// Vertices of a range solved in LDS.  Distances with labels keep 8 B per vertex (160 000 B of the CU's 163 840), sampling 7 B
// (distance, two dirty buffers, taken), a ball 6 B, beside the static scratch of the workgroup reductions.
constexpr int kGfLdsVertices = 20000;

struct gf_graph {
    const int32_t* rowptr;       // (V+1) CSR over the vertices of all meshes
    const int32_t* nbr;          // (E)
    const float* len;            // (E)
    int32_t V, E;
};

__device__ __forceinline__ int64_t gf_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// mesh p spans [v0, v0 + n): [pos_ptr[p], pos_ptr[p+1]) clamped into [0,V], or [0,V) without a table (any (B+1) range table
// over V rows: the samples of a mesh as well)
__device__ __forceinline__ void gf_mesh_range(const int64_t* pos_ptr, int p, int V, int& v0, int& n) {
    int v1 = V;
    v0 = 0;
    if (pos_ptr) {
        v0 = (int)gf_clamp(pos_ptr[p], 0, V);
        v1 = (int)gf_clamp(pos_ptr[p + 1], v0, V);
    }
    n = v1 - v0;
}

// the last of the B meshes whose sample range begins at or before q
__device__ __forceinline__ int gf_mesh_of(const int64_t* smp_ptr, int B, int q) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (smp_ptr[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the CSR row of vertex v, inside [0,E) whatever the table holds
__device__ __forceinline__ void gf_row(const gf_graph& g, int v, int& e0, int& e1) {
    e0 = max(g.rowptr[v], 0), e1 = min(g.rowptr[v + 1], g.E);
}

// A single-source problem's relaxation state is one slot: cap distances, then two dirty buffers of cap bytes.
__host__ __device__ inline size_t gf_slot_bytes(size_t n) { return (6 * n + 15) / 16 * 16; }

__device__ __forceinline__ void gf_carve(uint8_t* slot, int cap, float*& d, uint8_t*& cur, uint8_t*& nxt) {
    d = reinterpret_cast<float*>(slot);
    cur = slot + 4 * (size_t)cap;
    nxt = cur + cap;
}

// the neighbours of local vertex i (inside the range) get flag[u] = 1; the whole workgroup shares the row
__device__ __forceinline__ void gf_flag_neighbours(const gf_graph& g, int v0, int n, int i, uint8_t* flag, int t) {
    int e0, e1;
    gf_row(g, v0 + i, e0, e1);
    for (int e = e0 + t; e < e1; e += kGfThreads) {
        const int u = g.nbr[e] - v0;
        if ((unsigned)u < (unsigned)n) flag[u] = 1;
    }
}

// Pull-relaxation of the flagged vertices to the fixpoint (see the header).  Called by the whole workgroup after a barrier;
// every sweep ends in one, the last included.  Candidates must be < bound (+inf: no bound).  Returns the sweeps; the last
// changes nothing.
__device__ __forceinline__ int gf_relax(const gf_graph& g, int v0, int n, float* d, uint8_t*& cur, uint8_t*& nxt, float bound, int t) {
    int sw = 0;
    for (;;) {
        int changed = 0;
        for (int i = t; i < n; i += kGfThreads) {
            if (!cur[i]) continue;
            cur[i] = 0;
            int e0, e1;
            gf_row(g, v0 + i, e0, e1);
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

// The field of the one source src (local; outside [0,n): d stays +inf everywhere) bounded by `bound`.  Called by the whole
// workgroup; src is uniform over it.
__device__ __forceinline__ void gf_single_source(const gf_graph& g, int v0, int n, int64_t src, float* d, uint8_t*& cur, uint8_t*& nxt,
                                                 float bound, int t) {
    for (int i = t; i < n; i += kGfThreads) {
        d[i] = __int_as_float(0x7f800000);
        cur[i] = 0, nxt[i] = 0;
    }
    __syncthreads();
    if (src < 0 || src >= n) return;
    if (t == 0) d[src] = 0.f;
    gf_flag_neighbours(g, v0, n, (int)src, cur, t);
    __syncthreads();
    gf_relax(g, v0, n, d, cur, nxt, bound, t);
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

// The shape of a mini-batch: B meshes of at most max_range vertices, both range tables or neither (then one mesh, all of
// [0,V)), S samples of which a launch takes the window [q0, q0 + nq).
inline bool gf_batch_ok(const int64_t* pos_ptr, const int64_t* sample_ptr, int32_t B, int32_t max_range, int32_t V, int32_t S, int32_t q0,
                        int32_t nq) {
    if (S < 1 || B < 1 || max_range < 0 || max_range > V || q0 < 0 || nq < 0 || (int64_t)q0 + nq > S) return false;
    return (pos_ptr == nullptr) == (sample_ptr == nullptr) && (pos_ptr || (B == 1 && max_range == V));
}

inline bool gf_workspace_ok(size_t need, const void* workspace, size_t workspace_bytes) {
    return !need || (workspace && workspace_bytes >= need);
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

// The two instantiations of a solver over one grid.  Ranges of at most a.lds_vertices vertices (set here: all of them up to
// the capacity; none when a single mesh without tables is larger) belong to in_lds, which gets lds_bytes(lds_vertices) of
// dynamic LDS, at most `most` ever; larger ranges belong to in_global, which gets global_lds.  lds_ok: one array of
// kMaxDevices per kernel.
template <class Args, class LdsBytes>
inline int gf_launch_pair(void (*in_lds)(Args), void (*in_global)(Args), Args a, unsigned grid, int32_t max_range, bool tables,
                          LdsBytes lds_bytes, size_t most, size_t global_lds, bool* lds_ok, hipStream_t s) {
    a.lds_vertices = max_range <= kGfLdsVertices ? max_range : (tables ? kGfLdsVertices : 0);
    if (a.lds_vertices > 0) {
        const size_t lds = lds_bytes((size_t)a.lds_vertices);
        if (lds > 64 * 1024) {
            const int st = gf_allow_lds(reinterpret_cast<const void*>(in_lds), lds_ok, most);
            if (st != FC_OK) return st;
        }
        hipLaunchKernelGGL(in_lds, dim3(grid), dim3(kGfThreads), lds, s, a);
    }
    if (max_range > kGfLdsVertices) hipLaunchKernelGGL(in_global, dim3(grid), dim3(kGfThreads), global_lds, s, a);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // namespace fc
