// Sampling and neighbourhoods by the edge-graph metric of fc_geodesic.hip (same CSR, same float32 lengths, same fixpoint):
//   fc_geodesic_fps              farthest-point sampling: per mesh, n_samples rounds of (argmax of the field over the vertices not
//                                yet taken, d[new] = 0, relaxation to the new fixpoint) inside ONE launch, one workgroup per mesh;
//   fc_geodesic_fps_among        the same with the argmax restricted to a mask of candidates: the vertices outside it start as
//                                taken, and still relax;
//   fc_geodesic_ball_count/fill  one workgroup per query sample: the single-source field bounded by epsilon, then the samples of
//                                the query's mesh with d < epsilon as rows [query, position], at most K nearest of them;
//   ..._count_at / ..._fill_at   the same for a list of queries: workgroup w solves the query its list slot names.
// Both rest on one relaxation loop, gf_relax of fc_geodesic_relax.hpp, whose header says why the flagged relaxation reaches the
// least fixpoint whatever the schedule, why a round may start from the previous field, and why the field bounded by epsilon
// equals the unbounded one below epsilon.  A mesh runs exactly n_samples rounds.  No atomics.
#include <limits.h>
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"
#include "fc_kernels.hpp"
#include "fc_geodesic_relax.hpp"

namespace fc {

// ------------------------------------------------------------------------------------------------ farthest-point sampling
struct gfps_args {
    gf_graph g;
    const int64_t* pos_ptr;      // null: one mesh spanning [0,V); else mesh p spans [pos_ptr[p], pos_ptr[p+1])
    const uint8_t* candidate;    // null: every vertex may be taken; else (V), nonzero where it may
    const int64_t* n_samples;    // (B) rounds of mesh p
    const int64_t* start;        // (B) first sample, local to the mesh
    const int64_t* out_ptr;      // (B) where mesh p's indices begin in idx
    int64_t total_out;
    int64_t* idx;                // (total_out) local indices in selection order
    float* dist;                 // (V) the final field of every mesh
    int64_t* sweeps;             // null, or (B) relaxation sweeps summed over the rounds
    uint8_t* ws;                 // (3 V) flags of the ranges that do not fit LDS
    int32_t lds_vertices;        // ranges of at most this many vertices belong to the LDS instantiation, larger ones to the other
};

template <bool kLds>
__global__ __launch_bounds__(kGfThreads) void geodesic_fps_kernel(const gfps_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned long long s_key[kGfWaves];
    const int p = blockIdx.x, t = threadIdx.x;
    // whatever the tables hold, a mesh reads and writes inside [0,V) and its own slots of idx only
    int v0, n;
    gf_mesh_range(a.pos_ptr, p, a.g.V, v0, n);
    if ((n <= a.lds_vertices) != kLds || n < 1) return;          // (uniform over the workgroup)
    const int64_t o0 = gf_clamp(a.out_ptr[p], 0, a.total_out);
    const int64_t rounds = gf_clamp(a.n_samples[p], 0, min((int64_t)n, a.total_out - o0));
    const int first = (int)gf_clamp(a.start[p], 0, n - 1);
    float* const row = a.dist + v0;
    float* const d = kLds ? reinterpret_cast<float*>(smem) : row;
    uint8_t* const flags = kLds ? reinterpret_cast<uint8_t*>(smem) + 4 * (size_t)a.lds_vertices : nullptr;
    uint8_t* cur = kLds ? flags : a.ws + v0;
    uint8_t* nxt = kLds ? flags + a.lds_vertices : a.ws + (size_t)a.g.V + v0;
    uint8_t* const taken = kLds ? flags + 2 * (size_t)a.lds_vertices : a.ws + 2 * (size_t)a.g.V + v0;
    const float inf = __int_as_float(0x7f800000);

    for (int i = t; i < n; i += kGfThreads) {
        d[i] = inf;
        cur[i] = 0, nxt[i] = 0, taken[i] = a.candidate ? !a.candidate[v0 + i] : 0;
    }
    __syncthreads();

    int64_t sweeps = 0;
    for (int64_t k = 0; k < rounds; ++k) {
        int pick = first;
        if (k > 0) {
            // largest d, then lowest vertex: d >= 0 or +inf, so its bits order as an unsigned integer
            unsigned long long key = 0;
            for (int i = t; i < n; i += kGfThreads) {
                if (taken[i]) continue;
                const unsigned long long c = ((unsigned long long)__float_as_uint(d[i]) << 32) | (0xffffffffu - (unsigned)i);
                key = c > key ? c : key;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long c = __shfl_xor(key, o);
                key = c > key ? c : key;
            }
            if ((t & 63) == 0) s_key[t >> 6] = key;
            __syncthreads();
            key = 0;
            for (int w = 0; w < kGfWaves; ++w) key = s_key[w] > key ? s_key[w] : key;
            __syncthreads();          // (s_key is written again in the next round)
            // Without a mask rounds <= n leaves a vertex free.  With one the candidates can run out: a real key is never 0 (its
            // low word is 0xffffffff - i), so key == 0 says nothing is free; the remaining slots hold -1 and dist the field of
            // what was taken.  (key is the same in every thread: the exit is uniform.)
            if (key == 0) {
                for (int64_t j = k + t; j < rounds; j += kGfThreads) a.idx[o0 + j] = -1;
                break;
            }
            pick = (int)gf_clamp((int64_t)(0xffffffffu - (unsigned)(key & 0xffffffffu)), 0, n - 1);
        }
        if (t == 0) {
            taken[pick] = 1;
            d[pick] = 0.f;
            a.idx[o0 + k] = pick;
        }
        gf_flag_neighbours(a.g, v0, n, pick, cur, t);
        __syncthreads();
        sweeps += gf_relax(a.g, v0, n, d, cur, nxt, inf, t);
    }
    if (kLds)
        for (int i = t; i < n; i += kGfThreads) row[i] = d[i];
    if (t == 0 && a.sweeps) a.sweeps[p] = sweeps;
}

// ------------------------------------------------------------------------------------------------ geodesic balls
struct gball_args {
    gf_graph g;
    const int64_t* pos_ptr;      // both null: one mesh, every sample; else (B+1) ranges of the vertices and of the sample positions
    const int64_t* smp_ptr;
    int32_t B;
    const int64_t* sample_idx;   // (S) vertex numbers
    int32_t S;
    const int64_t* query_pos;    // null: list slot s is query s; else (Q) positions in sample_idx, slot s is query query_pos[s]
    int32_t Q;                   // list slots: S without a list
    int32_t q0;                  // workgroup w solves list slot q0 + w
    float eps;
    int32_t K;
    int32_t* count;              // (Q) min(in-ball samples, K) of every list slot: written by the counting launch
    const int64_t* off;          // (Q+1) where every list slot's rows begin: read by the filling launch
    int64_t n_edges;
    int64_t* edges;              // (n_edges, 2)
    float* edge_dist;            // null, or (n_edges)
    uint8_t* ws;                 // slot w of the ranges that do not fit LDS: 4 n bytes of distances, then 2 n of flags
    size_t ws_stride;
    int32_t lds_vertices;
    int32_t max_range;           // what a workspace slot was sized for: a larger range is left unsolved
};

template <bool kLds, bool kFill>
__global__ __launch_bounds__(kGfThreads) void geodesic_ball_kernel(const gball_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_wave[kGfWaves];
    const int t = threadIdx.x;
    const int slot = a.q0 + (int)blockIdx.x;
    if (slot < 0 || slot >= a.Q) return;
    const int64_t listed = a.query_pos ? a.query_pos[slot] : slot;
    if (listed < 0 || listed >= a.S) {          // (a list may name anything: such a slot is skipped, with no rows)
        if (!kFill && t == 0) a.count[slot] = 0;
        return;
    }
    const int q = (int)listed;
    const int mesh = a.pos_ptr ? gf_mesh_of(a.smp_ptr, a.B, q) : 0;
    int v0, n, s0, ns;
    gf_mesh_range(a.pos_ptr, mesh, a.g.V, v0, n);
    gf_mesh_range(a.smp_ptr, mesh, a.S, s0, ns);          // the samples of the mesh: positions [s0, s1), by the same rule
    const int s1 = s0 + ns;
    if ((n <= a.lds_vertices) != kLds || n > a.max_range) return;          // (uniform over the workgroup)
    uint8_t* const state = kLds ? reinterpret_cast<uint8_t*>(smem) : a.ws + a.ws_stride * blockIdx.x;
    float* d;
    uint8_t *cur, *nxt;
    gf_carve(state, kLds ? a.lds_vertices : n, d, cur, nxt);
    gf_single_source(a.g, v0, n, a.sample_idx[q] - v0, d, cur, nxt, a.eps, t);          // (a source outside the range: an empty ball)

    // the samples of this mesh inside the ball: d < eps (the source holds 0, every other finite value passed the bound)
    auto key_of = [&](int j, unsigned long long& key) -> bool {
        if (j >= s1) return false;
        const int64_t v = a.sample_idx[j] - v0;
        if (v < 0 || v >= n) return false;
        const float dv = d[v];
        key = ((unsigned long long)__float_as_uint(dv) << 32) | (unsigned)j;          // (distance, position)
        return dv < a.eps;
    };
    int found = 0;
    for (int base = s0; base < s1; base += kGfThreads) {
        unsigned long long key = 0;
        found += __syncthreads_count(key_of(base + t, key));
    }
    const int keep = min(found, a.K);
    if (!kFill) {
        if (t == 0) a.count[slot] = keep;
        return;
    }
    // more than K: the K-th smallest key, bit by bit from the top (keys are distinct, so exactly K keys are <= it)
    unsigned long long limit = ~0ull;
    if (found > a.K) {
        limit = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const unsigned long long trial = limit | ((1ull << bit) - 1ull);          // this bit 0, every lower bit 1
            int below = 0;
            for (int base = s0; base < s1; base += kGfThreads) {
                unsigned long long key = 0;
                const bool in = key_of(base + t, key);
                below += __syncthreads_count(in && key <= trial);
            }
            if (below < a.K) limit |= 1ull << bit;
        }
    }
    const int64_t o0 = gf_clamp(a.off[slot], 0, a.n_edges), o1 = gf_clamp(a.off[slot + 1], o0, a.n_edges);
    int64_t at = o0;
    for (int base = s0; base < s1; base += kGfThreads) {
        unsigned long long key = 0;
        const bool in = key_of(base + t, key) && key <= limit;
        int total;
        const int64_t mine = at + gf_scan(in, t, s_wave, total);
        if (in && mine < o1) {
            a.edges[2 * mine] = q;
            a.edges[2 * mine + 1] = base + t;
            if (a.edge_dist) a.edge_dist[mine] = __uint_as_float((unsigned)(key >> 32));
        }
        at += total;
    }
}

}  // namespace fc

namespace {

using fc::gf_graph_ok;

template <bool kFill>
int gf_ball_launch(const fc::gball_args& a, int32_t nq, int32_t max_range, hipStream_t s) {
    static bool lds_ok[fc::kMaxDevices] = {};          // (per instantiation of this template: per kernel)
    return fc::gf_launch_pair(fc::geodesic_ball_kernel<true, kFill>, fc::geodesic_ball_kernel<false, kFill>, a, (unsigned)nq, max_range,
                              a.pos_ptr != nullptr, [](size_t n) { return 6 * n; }, 6 * (size_t)fc::kGfLdsVertices, 0, lds_ok, s);
}

// listed: the launch windows the list query_pos (Q slots) in place of the S samples
bool gf_ball_args(fc::gball_args& a, const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                  const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S, bool listed,
                  const int64_t* query_pos, int32_t Q, int32_t q0, int32_t nq, float epsilon, int32_t K, void* workspace, size_t workspace_bytes,
                  int* status) {
    *status = FC_ERR_BAD_ARGUMENT;
    if (!gf_graph_ok(rowptr, nbr, length, V, E) || !fc::gf_batch_ok(pos_ptr, sample_ptr, B, max_range, V, S, 0, 0) ||
        !fc::gf_batch_ok(pos_ptr, sample_ptr, B, max_range, V, listed ? Q : S, q0, nq) || (listed && !query_pos) || !sample_idx || K < 1 ||
        !(epsilon > 0.f))
        return false;
    if (!fc::gf_workspace_ok(fc_geodesic_ball_workspace_bytes(max_range, nq), workspace, workspace_bytes)) {
        *status = FC_ERR_WORKSPACE;
        return false;
    }
    a.g = {rowptr, nbr, length, V, E};
    a.pos_ptr = pos_ptr, a.smp_ptr = sample_ptr, a.B = B;
    a.sample_idx = sample_idx, a.S = S, a.query_pos = listed ? query_pos : nullptr, a.Q = listed ? Q : S, a.q0 = q0, a.eps = epsilon, a.K = K;
    a.ws = static_cast<uint8_t*>(workspace), a.ws_stride = fc::gf_slot_bytes(max_range), a.max_range = max_range;
    *status = FC_OK;
    return true;
}

int gf_ball_count(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                  const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S, bool listed,
                  const int64_t* query_pos, int32_t Q, int32_t q0, int32_t nq, float epsilon, int32_t K, int32_t* count, void* workspace,
                  size_t workspace_bytes, void* stream) {
    fc::gball_args a = {};
    int status;
    if (!gf_ball_args(a, rowptr, nbr, length, V, E, pos_ptr, sample_ptr, B, max_range, sample_idx, S, listed, query_pos, Q, q0, nq, epsilon, K,
                      workspace, workspace_bytes, &status))
        return status;
    if (!count) return FC_ERR_BAD_ARGUMENT;
    if (nq == 0) return FC_OK;
    a.count = count;
    return gf_ball_launch<false>(a, nq, max_range, static_cast<hipStream_t>(stream));
}

int gf_ball_fill(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                 const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S, bool listed,
                 const int64_t* query_pos, int32_t Q, int32_t q0, int32_t nq, float epsilon, int32_t K, const int64_t* offsets, int64_t n_edges,
                 int64_t* edges, float* edge_dist, void* workspace, size_t workspace_bytes, void* stream) {
    fc::gball_args a = {};
    int status;
    if (!gf_ball_args(a, rowptr, nbr, length, V, E, pos_ptr, sample_ptr, B, max_range, sample_idx, S, listed, query_pos, Q, q0, nq, epsilon, K,
                      workspace, workspace_bytes, &status))
        return status;
    if (!offsets || n_edges < 0 || (n_edges > 0 && !edges)) return FC_ERR_BAD_ARGUMENT;
    if (nq == 0 || n_edges == 0) return FC_OK;
    a.off = offsets, a.n_edges = n_edges, a.edges = edges, a.edge_dist = edge_dist;
    return gf_ball_launch<true>(a, nq, max_range, static_cast<hipStream_t>(stream));
}

// masked: the argmax runs over the candidates only
int gf_fps(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr, int32_t B,
           int32_t max_range, bool masked, const uint8_t* candidate, const int64_t* n_samples, const int64_t* start, const int64_t* out_ptr,
           int64_t total_out, int64_t* idx, float* dist, int64_t* sweeps, void* workspace, size_t workspace_bytes, void* stream) {
    if (!gf_graph_ok(rowptr, nbr, length, V, E) || B < 1 || max_range < 0 || max_range > V || !n_samples || !start || !out_ptr ||
        total_out < 1 || !idx || !dist || (masked && !candidate))
        return FC_ERR_BAD_ARGUMENT;
    if (!pos_ptr && (B != 1 || max_range != V)) return FC_ERR_BAD_ARGUMENT;
    if (!fc::gf_workspace_ok(fc_geodesic_fps_workspace_bytes(V, max_range), workspace, workspace_bytes)) return FC_ERR_WORKSPACE;
    static bool lds_ok[fc::kMaxDevices] = {};
    fc::gfps_args a = {};
    a.g = {rowptr, nbr, length, V, E};
    a.pos_ptr = pos_ptr, a.candidate = masked ? candidate : nullptr;
    a.n_samples = n_samples, a.start = start, a.out_ptr = out_ptr, a.total_out = total_out;
    a.idx = idx, a.dist = dist, a.sweeps = sweeps, a.ws = static_cast<uint8_t*>(workspace);
    return fc::gf_launch_pair(fc::geodesic_fps_kernel<true>, fc::geodesic_fps_kernel<false>, a, (unsigned)B, max_range, pos_ptr != nullptr,
                              [](size_t n) { return 7 * n; }, 7 * (size_t)fc::kGfLdsVertices, 0, lds_ok, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int32_t fc_geodesic_fps_lds_vertices(void) { return fc::kGfLdsVertices; }

size_t fc_geodesic_fps_workspace_bytes(int32_t V, int32_t max_range) {
    return V > 0 && max_range > fc::kGfLdsVertices ? 3 * (size_t)V : 0;
}

int fc_geodesic_fps(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr, int32_t B,
                    int32_t max_range, const int64_t* n_samples, const int64_t* start, const int64_t* out_ptr, int64_t total_out,
                    int64_t* idx, float* dist, int64_t* sweeps, void* workspace, size_t workspace_bytes, void* stream) {
    return gf_fps(rowptr, nbr, length, V, E, pos_ptr, B, max_range, false, nullptr, n_samples, start, out_ptr, total_out, idx, dist, sweeps,
                  workspace, workspace_bytes, stream);
}

int fc_geodesic_fps_among(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                          int32_t B, int32_t max_range, const uint8_t* candidate, const int64_t* n_samples, const int64_t* start,
                          const int64_t* out_ptr, int64_t total_out, int64_t* idx, float* dist, int64_t* sweeps, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return gf_fps(rowptr, nbr, length, V, E, pos_ptr, B, max_range, true, candidate, n_samples, start, out_ptr, total_out, idx, dist, sweeps,
                  workspace, workspace_bytes, stream);
}

size_t fc_geodesic_ball_workspace_bytes(int32_t max_range, int32_t queries) {
    return max_range > fc::kGfLdsVertices && queries > 0 ? fc::gf_slot_bytes(max_range) * (size_t)queries : 0;
}

int fc_geodesic_ball_count(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                           const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S, int32_t q0,
                           int32_t nq, float epsilon, int32_t K, int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    return gf_ball_count(rowptr, nbr, length, V, E, pos_ptr, sample_ptr, B, max_range, sample_idx, S, false, nullptr, 0, q0, nq, epsilon, K,
                         count, workspace, workspace_bytes, stream);
}

int fc_geodesic_ball_fill(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                          const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S, int32_t q0,
                          int32_t nq, float epsilon, int32_t K, const int64_t* offsets, int64_t n_edges, int64_t* edges, float* edge_dist,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return gf_ball_fill(rowptr, nbr, length, V, E, pos_ptr, sample_ptr, B, max_range, sample_idx, S, false, nullptr, 0, q0, nq, epsilon, K,
                        offsets, n_edges, edges, edge_dist, workspace, workspace_bytes, stream);
}

int fc_geodesic_ball_count_at(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                              const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S,
                              const int64_t* query_pos, int32_t Q, int32_t q0, int32_t nq, float epsilon, int32_t K, int32_t* count,
                              void* workspace, size_t workspace_bytes, void* stream) {
    return gf_ball_count(rowptr, nbr, length, V, E, pos_ptr, sample_ptr, B, max_range, sample_idx, S, true, query_pos, Q, q0, nq, epsilon, K,
                         count, workspace, workspace_bytes, stream);
}

int fc_geodesic_ball_fill_at(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                             const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S,
                             const int64_t* query_pos, int32_t Q, int32_t q0, int32_t nq, float epsilon, int32_t K, const int64_t* offsets,
                             int64_t n_edges, int64_t* edges, float* edge_dist, void* workspace, size_t workspace_bytes, void* stream) {
    return gf_ball_fill(rowptr, nbr, length, V, E, pos_ptr, sample_ptr, B, max_range, sample_idx, S, true, query_pos, Q, q0, nq, epsilon, K,
                        offsets, n_edges, edges, edge_dist, workspace, workspace_bytes, stream);
}

}  // extern "C"
