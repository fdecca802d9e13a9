// Per-edge log map and parallel transport by the discrete exponential map (Schmidt, Grimm, Wyvill 2006) over the edge-graph
// metric of fc_geodesic.hip -- not the Vector Heat Method of the reference's fcutils:
//   fc_vertex_frames     n_v = normalised sum of the incident faces' cross products (a fixed order over a vertex-to-face CSR),
//                        e1 = normalize(ref x n), e2 = n x e1: every operation a float32 operation rounded on its own;
//   fc_logmap            one workgroup per query sample s: (1) the distance field bounded by `bound` (gf_single_source, as
//                        in the ball kernel); (2) the reached vertices are compacted into a ball, hop counts h over the tight edges
//                        fl32(d[u] + len) == d[v] are swept to their least fixpoint and pred[v] = the lowest-numbered tight u with
//                        h[u] = h[v] - 1; (3) the tree is unfolded level by level into s's tangent plane, X[v] = rho X[u],
//                        L[v] = L[u] + conj(X[u]) c; (4) the query's rows [s, t] read L[t], X[t].
// Every discrete decision (reached, tight, h, pred) is a function of the bits of d, which do not depend on the schedule; h is a
// least fixpoint of integers (every value ever written is the hop count of some tight path, an upper bound; the sweeps end in a
// state where no vertex can drop), so pred cannot be cyclic even where zero-length edges make the tight edges so.  Level k of the
// unfolding reads level k - 1 only, across a barrier: a vertex's value has one writer and one definition, the same bits on every
// run.  No atomics.  Loops are bounded by the problem: n + 1 relaxation sweeps, m + 1 hop sweeps and m levels for a ball of m
// vertices; none waits on data.  The state of steps 2-4 (36 B per ball vertex) lives in LDS where the ball fits the launch's
// share, else in the workgroup's workspace slot.  After the compaction the distance array of the range holds each vertex's
// position in the ball (-1: not reached): one word per vertex serves both.  A workgroup writes its own query's rows, its own
// slot and, for the debug output, its own row of (S,V) only; what it reads from pred and the tables is range-checked.
#include <limits.h>
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"
#include "fc_kernels.hpp"
#include "fc_geodesic_relax.hpp"

namespace fc {

// Ball vertices whose tree state stays in LDS: 36 B each beside the 6 B per vertex of the range's relaxation state
// (120 000 + 36 864 of the CU's 163 840 B at both capacities, and the static scratch of the scan).
constexpr int kLmBallLds = 1024;
constexpr int kLmBallBytes = 36;

struct lm_args {
    gf_graph g;
    const int64_t* pos_ptr;      // both null: one mesh; else (B+1) ranges of the vertices and of the sample positions
    const int64_t* smp_ptr;
    int32_t B;
    const float* pos;            // (V,3), and the frames of fc_vertex_frames
    const float* nrm;
    const float* e1;
    const float* e2;
    const int64_t* sample_idx;   // (S) vertex numbers
    int32_t S;
    int32_t q0;                  // workgroup w solves query q0 + w
    float bound;
    const int64_t* row_ptr;      // (S+1): query q owns the rows row_ptr[q] .. row_ptr[q+1] - 1
    const int64_t* row_tgt;      // (R) positions in sample_idx
    int64_t R;
    float* log_mag;              // (R)
    float* log_ang;              // (R)
    float* xp;                   // (R,2) re, im
    uint8_t* reached;            // (R)
    int32_t* dbg_pred;           // both null, or (S,V): the predecessor (a vertex number) and the hop count, -1 where none
    int32_t* dbg_hops;
    uint8_t* ws;                 // slot w: the relaxation state of a range above the LDS capacity, then the ball state
    size_t ws_stride, ws_ball_off;
    int32_t lds_vertices;        // ranges of at most this many vertices relax in LDS (the other instantiation takes the rest)
    int32_t max_range;           // what a slot was sized for
    int32_t ball_lds;            // balls of at most this many vertices keep their tree state in LDS
};

struct lm_ball {
    int* vid;                    // vertex of the range, ascending
    float* d;
    int* h;
    int* pred;                   // a position in the ball
    float* plen;                 // the length of the edge to pred
    float2* L;
    float2* X;
};

// cap even and base 16-byte aligned: L and X are 8-byte aligned
__device__ __forceinline__ lm_ball lm_carve(uint8_t* base, int cap) {
    lm_ball b;
    b.vid = reinterpret_cast<int*>(base);
    b.d = reinterpret_cast<float*>(base + 4 * (size_t)cap);
    b.h = reinterpret_cast<int*>(base + 8 * (size_t)cap);
    b.pred = reinterpret_cast<int*>(base + 12 * (size_t)cap);
    b.plen = reinterpret_cast<float*>(base + 16 * (size_t)cap);
    b.L = reinterpret_cast<float2*>(base + 20 * (size_t)cap);
    b.X = reinterpret_cast<float2*>(base + 28 * (size_t)cap);
    return b;
}

struct lm_vec { float x, y, z; };

__device__ __forceinline__ lm_vec lm_load(const float* p, int v) { return {p[3 * (size_t)v], p[3 * (size_t)v + 1], p[3 * (size_t)v + 2]}; }

__device__ __forceinline__ float lm_dot(lm_vec a, lm_vec b) {
#pragma clang fp contract(off)
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}

__device__ __forceinline__ lm_vec lm_cross(lm_vec a, lm_vec b) {
#pragma clang fp contract(off)
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// One step of the unfolding, from u (value Lu, Xu) to its child v over an edge of length len; u, v vertex numbers in [0,V).
// Plain operators with contraction off, in the order of tests/_logmap_ref.py.
__device__ __forceinline__ void lm_child(const lm_args& a, int u, int v, float len, float2 Lu, float2 Xu, float2& Lv, float2& Xv) {
#pragma clang fp contract(off)
    const lm_vec pu = lm_load(a.pos, u), pv = lm_load(a.pos, v), nu = lm_load(a.nrm, u), nv = lm_load(a.nrm, v);
    const lm_vec e1u = lm_load(a.e1, u), e2u = lm_load(a.e2, u), e1v = lm_load(a.e1, v), e2v = lm_load(a.e2, v);
    // c: the edge without its normal component, in u's frame, rescaled to the edge's length
    const lm_vec w = {pv.x - pu.x, pv.y - pu.y, pv.z - pu.z};
    const float wn = lm_dot(w, nu);
    const lm_vec tg = {w.x - wn * nu.x, w.y - wn * nu.y, w.z - wn * nu.z};
    float c1 = lm_dot(tg, e1u), c2 = lm_dot(tg, e2u);
    const float r = sqrtf(c1 * c1 + c2 * c2);
    if (r > 0.f) {
        const float s = len / r;
        c1 = c1 * s, c2 = c2 * s;
    } else {
        c1 = 0.f, c2 = 0.f;
    }
    // rho: e1_u carried by the minimal rotation n_u -> n_v, in v's frame
    const float cth = lm_dot(nu, nv), opc = 1.f + cth;
    lm_vec g;
    if (opc > 1e-6f) {
        const lm_vec k = lm_cross(nu, nv), ke = lm_cross(k, e1u);
        const float f = lm_dot(k, e1u) / opc;
        g = {(e1u.x * cth + ke.x) + k.x * f, (e1u.y * cth + ke.y) + k.y * f, (e1u.z * cth + ke.z) + k.z * f};
    } else {
        const float dn = lm_dot(e1u, nv);
        g = {e1u.x - dn * nv.x, e1u.y - dn * nv.y, e1u.z - dn * nv.z};
    }
    float r1 = lm_dot(g, e1v), r2 = lm_dot(g, e2v);
    const float rn = sqrtf(r1 * r1 + r2 * r2);
    if (rn > 0.f) {
        r1 = r1 / rn, r2 = r2 / rn;
    } else {
        r1 = 1.f, r2 = 0.f;
    }
    Xv = make_float2(r1 * Xu.x - r2 * Xu.y, r1 * Xu.y + r2 * Xu.x);
    Lv = make_float2(Lu.x + (Xu.x * c1 + Xu.y * c2), Lu.y + (Xu.x * c2 - Xu.y * c1));
}

// Steps 2-4 for a ball of m vertices whose state is `ball` (cap entries).  mapf: the range's distances on entry, the ball
// positions (as bits) afterwards.  Called by the whole workgroup after a barrier.
__device__ __forceinline__ void lm_tree(const lm_args& a, const lm_ball ball, int cap, int m, float* mapf, int v0, int n, int src, int q,
                                        int t, int* s_wave) {
    const float inf = __int_as_float(0x7f800000);
    // compaction, in vertex order; a thread is the only reader and writer of its own vertices' words
    int at = 0;
    for (int base = 0; base < n; base += kGfThreads) {
        const int i = base + t;
        const float dv = i < n ? mapf[i] : inf;
        const bool in = dv < inf;
        int total;
        const int j = at + gf_scan(in, t, s_wave, total);
        const bool kept = in && j < cap;
        if (kept) {
            ball.vid[j] = i;
            ball.d[j] = dv;
            ball.h[j] = i == src ? 0 : INT_MAX;
            ball.pred[j] = -1;
            ball.plen[j] = 0.f;
            if (i == src) ball.L[j] = make_float2(0.f, 0.f), ball.X[j] = make_float2(1.f, 0.f);
        }
        if (i < n) mapf[i] = __int_as_float(kept ? j : -1);
        at += total;
    }
    __syncthreads();
    auto slot_of = [&](int u) -> int {          // the ball position of vertex u of the range, or -1
        if ((unsigned)u >= (unsigned)n) return -1;
        const int j = __float_as_int(mapf[u]);
        return (unsigned)j < (unsigned)m && j < cap ? j : -1;
    };

    // hop counts: the least fixpoint over the tight edges
    for (int sw = 0;;) {
        int changed = 0;
        for (int i = t; i < m; i += kGfThreads) {
            const int vi = ball.vid[i];
            if (vi == src) continue;
            int e0, e1;
            gf_row(a.g, v0 + vi, e0, e1);
            const float dv = ball.d[i];
            const int old = ball.h[i];
            int best = old;
            for (int e = e0; e < e1; ++e) {
                const int j = slot_of(a.g.nbr[e] - v0);
                if (j >= 0 && ball.d[j] + a.g.len[e] == dv) {
                    const int hj = ball.h[j];
                    best = (hj != INT_MAX && hj + 1 < best) ? hj + 1 : best;
                }
            }
            if (best < old) {
                ball.h[i] = best;
                changed = 1;
            }
        }
        ++sw;
        if (!__syncthreads_or(changed) || sw > m) break;
    }
    // predecessors: the CSR rows ascend, so the first hit is the lowest-numbered
    for (int i = t; i < m; i += kGfThreads) {
        const int vi = ball.vid[i], hi = ball.h[i];
        if (vi == src || hi == INT_MAX) continue;
        int e0, e1;
        gf_row(a.g, v0 + vi, e0, e1);
        const float dv = ball.d[i];
        for (int e = e0; e < e1; ++e) {
            const int j = slot_of(a.g.nbr[e] - v0);
            const float le = a.g.len[e];
            if (j >= 0 && ball.d[j] + le == dv && ball.h[j] == hi - 1) {
                ball.pred[i] = j;
                ball.plen[i] = le;
                break;
            }
        }
    }
    __syncthreads();
    // unfolding: level k takes its values from level k - 1, written before the previous barrier
    for (int k = 1; k <= m; ++k) {
        int any = 0;
        for (int i = t; i < m; i += kGfThreads) {
            if (ball.h[i] != k) continue;
            any = 1;
            const int p = ball.pred[i];
            float2 Lv = make_float2(0.f, 0.f), Xv = make_float2(1.f, 0.f);
            if ((unsigned)p < (unsigned)m && p < cap && ball.h[p] == k - 1)
                lm_child(a, v0 + ball.vid[p], v0 + ball.vid[i], ball.plen[i], ball.L[p], ball.X[p], Lv, Xv);
            ball.L[i] = Lv, ball.X[i] = Xv;
        }
        if (!__syncthreads_or(any)) break;
    }

    // the rows of this query
    const int64_t r0 = gf_clamp(a.row_ptr[q], 0, a.R), r1 = gf_clamp(a.row_ptr[q + 1], r0, a.R);
    for (int64_t r = r0 + t; r < r1; r += kGfThreads) {
        const float nan = __int_as_float(0x7fc00000);
        float2 Lt = make_float2(nan, nan), Xt = make_float2(nan, nan);
        uint8_t ok = 0;
        const int64_t b = a.row_tgt[r];
        const int64_t tv = b >= 0 && b < a.S ? a.sample_idx[b] : -1;
        if (tv >= 0 && tv < a.g.V) {
            const int64_t local = tv - v0;
            const int j = local >= 0 && local < n ? slot_of((int)local) : -1;
            if (j >= 0 && ball.h[j] != INT_MAX) {
                Lt = ball.L[j], Xt = ball.X[j], ok = 1;
            } else {
#pragma clang fp contract(off)
                // not reached below the bound: a child of the source over a virtual edge of the chord's length
                const int s = v0 + src;
                const float dx = a.pos[3 * (size_t)tv] - a.pos[3 * (size_t)s], dy = a.pos[3 * (size_t)tv + 1] - a.pos[3 * (size_t)s + 1],
                            dz = a.pos[3 * (size_t)tv + 2] - a.pos[3 * (size_t)s + 2];
                lm_child(a, s, (int)tv, sqrtf((dx * dx + dy * dy) + dz * dz), make_float2(0.f, 0.f), make_float2(1.f, 0.f), Lt, Xt);
            }
        }
        {
#pragma clang fp contract(off)
            a.log_mag[r] = sqrtf(Lt.x * Lt.x + Lt.y * Lt.y);
        }
        a.log_ang[r] = (Lt.x == 0.f && Lt.y == 0.f) ? 0.f : atan2f(Lt.y, Lt.x);
        a.xp[2 * r] = Xt.x, a.xp[2 * r + 1] = Xt.y;
        a.reached[r] = ok;
    }
    if (a.dbg_hops && a.dbg_pred) {
        int32_t* const hops = a.dbg_hops + (size_t)q * a.g.V + v0;
        int32_t* const pred = a.dbg_pred + (size_t)q * a.g.V + v0;
        for (int i = t; i < n; i += kGfThreads) {
            const int j = slot_of(i);
            const bool has = j >= 0 && ball.h[j] != INT_MAX;
            const int p = has ? ball.pred[j] : -1;
            hops[i] = has ? ball.h[j] : -1;
            pred[i] = ((unsigned)p < (unsigned)m && p < cap) ? v0 + ball.vid[p] : -1;
        }
    }
}

template <bool kLds>
__global__ __launch_bounds__(kGfThreads) void logmap_kernel(const lm_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_wave[kGfWaves];
    const int t = threadIdx.x;
    const int q = a.q0 + (int)blockIdx.x;
    if (q < 0 || q >= a.S) return;
    int v0, n;
    gf_mesh_range(a.pos_ptr, a.pos_ptr ? gf_mesh_of(a.smp_ptr, a.B, q) : 0, a.g.V, v0, n);
    if ((n <= a.lds_vertices) != kLds) return;          // (uniform over the workgroup) the other instantiation's query
    const int64_t src = a.sample_idx[q] - v0;
    if (n > a.max_range || src < 0 || src >= n) {
        // the caller checks the ranges and the samples; should it not, the query's rows say so: NaN, not reached
        const int64_t r0 = gf_clamp(a.row_ptr[q], 0, a.R), r1 = gf_clamp(a.row_ptr[q + 1], r0, a.R);
        const float nan = __int_as_float(0x7fc00000);
        for (int64_t r = r0 + t; r < r1; r += kGfThreads) {
            a.log_mag[r] = nan, a.log_ang[r] = nan, a.xp[2 * r] = nan, a.xp[2 * r + 1] = nan;
            a.reached[r] = 0;
        }
        return;
    }
    if (!a.dbg_hops && gf_clamp(a.row_ptr[q], 0, a.R) >= gf_clamp(a.row_ptr[q + 1], 0, a.R)) return;          // no rows: nothing to solve

    const size_t lds_mesh = kLds ? gf_slot_bytes(a.lds_vertices) : 0;
    uint8_t* const own = a.ws + a.ws_stride * blockIdx.x;
    uint8_t* const slot = kLds ? reinterpret_cast<uint8_t*>(smem) : own;
    float* d;
    uint8_t *cur, *nxt;
    gf_carve(slot, kLds ? a.lds_vertices : n, d, cur, nxt);
    gf_single_source(a.g, v0, n, src, d, cur, nxt, a.bound, t);
    const float inf = __int_as_float(0x7f800000);

    int m = 0;
    for (int base = 0; base < n; base += kGfThreads) m += __syncthreads_count(base + t < n && d[base + t] < inf);
    if (m <= a.ball_lds)
        lm_tree(a, lm_carve(reinterpret_cast<uint8_t*>(smem) + lds_mesh, (a.ball_lds + 1) & ~1), (a.ball_lds + 1) & ~1, m, d, v0, n, (int)src, q, t,
                s_wave);
    else
        lm_tree(a, lm_carve(own + a.ws_ball_off, (a.max_range + 1) & ~1), (a.max_range + 1) & ~1, m, d, v0, n, (int)src, q, t, s_wave);
}

// one thread per vertex: the incident faces in the order of the CSR (ascending face, then corner), corners as stored
__global__ void vertex_frames_kernel(const float* __restrict__ pos, const int64_t* __restrict__ face, const int32_t* __restrict__ fptr,
                                     const int32_t* __restrict__ fidx, int V, int F, float* __restrict__ nrm, float* __restrict__ e1,
                                     float* __restrict__ e2) {
#pragma clang fp contract(off)
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int64_t k0 = gf_clamp(fptr[v], 0, 3 * (int64_t)F), k1 = gf_clamp(fptr[v + 1], k0, 3 * (int64_t)F);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int64_t k = k0; k < k1; ++k) {
        const int f = fidx[k];
        if ((unsigned)f >= (unsigned)F) continue;
        const int64_t ia = face[f], ib = face[(size_t)F + f], ic = face[2 * (size_t)F + f];
        if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) continue;
        const lm_vec pa = lm_load(pos, (int)ia), pb = lm_load(pos, (int)ib), pc = lm_load(pos, (int)ic);
        const lm_vec c = lm_cross({pb.x - pa.x, pb.y - pa.y, pb.z - pa.z}, {pc.x - pa.x, pc.y - pa.y, pc.z - pa.z});
        sx = sx + c.x, sy = sy + c.y, sz = sz + c.z;
    }
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    lm_vec n = {0.f, 0.f, 1.f};
    if (len > 0.f) n = {sx / len, sy / len, sz / len};
    const lm_vec ref = fabsf(n.z) < 0.95f ? lm_vec{0.f, 0.f, 1.f} : lm_vec{1.f, 0.f, 0.f};
    const lm_vec c = lm_cross(ref, n);
    const float cl = sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z);
    const lm_vec a1 = {c.x / cl, c.y / cl, c.z / cl};
    const lm_vec a2 = lm_cross(n, a1);
    nrm[3 * (size_t)v] = n.x, nrm[3 * (size_t)v + 1] = n.y, nrm[3 * (size_t)v + 2] = n.z;
    e1[3 * (size_t)v] = a1.x, e1[3 * (size_t)v + 1] = a1.y, e1[3 * (size_t)v + 2] = a1.z;
    e2[3 * (size_t)v] = a2.x, e2[3 * (size_t)v + 1] = a2.y, e2[3 * (size_t)v + 2] = a2.z;
}

}  // namespace fc

namespace {

int32_t lm_even(int32_t x) { return (x + 1) & ~1; }

size_t lm_mesh_bytes(int32_t max_range) { return max_range > fc::kGfLdsVertices ? fc::gf_slot_bytes(max_range) : 0; }

size_t lm_ball_bytes(int32_t max_range, int32_t ball_lds) {
    return max_range > ball_lds ? ((size_t)fc::kLmBallBytes * lm_even(max_range) + 15) / 16 * 16 : 0;
}

}  // namespace

extern "C" {

int32_t fc_logmap_ball_lds_vertices(void) { return fc::kLmBallLds; }

int fc_vertex_frames(const float* pos, const int64_t* face, const int32_t* face_ptr, const int32_t* face_idx, int32_t V, int32_t F,
                     float* normal, float* e1, float* e2, void* stream) {
    if (V < 1 || F < 0 || !pos || !face_ptr || !normal || !e1 || !e2 || (F > 0 && (!face || !face_idx)) || (int64_t)F * 3 > INT_MAX)
        return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::vertex_frames_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, face,
                       face_ptr, face_idx, V, F, normal, e1, e2);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

size_t fc_logmap_workspace_bytes(int32_t max_range, int32_t queries, int32_t ball_lds) {
    if (max_range < 1 || queries < 1 || ball_lds < 0) return 0;
    return (lm_mesh_bytes(max_range) + lm_ball_bytes(max_range, ball_lds)) * (size_t)queries;
}

int fc_logmap(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
              const int64_t* sample_ptr, int32_t B, int32_t max_range, const float* pos, const float* normal, const float* e1, const float* e2,
              const int64_t* sample_idx, int32_t S, int32_t q0, int32_t nq, float bound, const int64_t* row_ptr, const int64_t* row_target,
              int64_t n_rows, float* log_mag, float* log_ang, float* xp, uint8_t* reached, int32_t* debug_pred, int32_t* debug_hops,
              int32_t ball_lds, void* workspace, size_t workspace_bytes, void* stream) {
    if (!fc::gf_graph_ok(rowptr, nbr, length, V, E) || !fc::gf_batch_ok(pos_ptr, sample_ptr, B, max_range, V, S, q0, nq) || max_range < 1 ||
        !sample_idx || !(bound > 0.f) || !pos || !normal || !e1 || !e2 || !row_ptr || n_rows < 0 || ball_lds < 0 || ball_lds > fc::kLmBallLds ||
        (debug_pred == nullptr) != (debug_hops == nullptr))
        return FC_ERR_BAD_ARGUMENT;
    if (n_rows > 0 && (!row_target || !log_mag || !log_ang || !xp || !reached)) return FC_ERR_BAD_ARGUMENT;
    if (nq == 0 || (n_rows == 0 && !debug_hops)) return FC_OK;
    if (!fc::gf_workspace_ok(fc_logmap_workspace_bytes(max_range, nq, ball_lds), workspace, workspace_bytes)) return FC_ERR_WORKSPACE;
    fc::lm_args a = {};
    a.g = {rowptr, nbr, length, V, E};
    a.pos_ptr = pos_ptr, a.smp_ptr = sample_ptr, a.B = B;
    a.pos = pos, a.nrm = normal, a.e1 = e1, a.e2 = e2;
    a.sample_idx = sample_idx, a.S = S, a.q0 = q0, a.bound = bound;
    a.row_ptr = row_ptr, a.row_tgt = row_target, a.R = n_rows;
    a.log_mag = log_mag, a.log_ang = log_ang, a.xp = xp, a.reached = reached;
    a.dbg_pred = debug_pred, a.dbg_hops = debug_hops;
    a.ws = static_cast<uint8_t*>(workspace);
    a.ws_ball_off = lm_mesh_bytes(max_range), a.ws_stride = a.ws_ball_off + lm_ball_bytes(max_range, ball_lds);
    a.max_range = max_range, a.ball_lds = ball_lds;
    static bool lds_ok[fc::kMaxDevices] = {};
    // the ball state follows the range's slot in LDS; the instantiation whose ranges relax in global memory keeps the balls there
    const size_t ball = (size_t)fc::kLmBallBytes * lm_even(ball_lds);
    return fc::gf_launch_pair(fc::logmap_kernel<true>, fc::logmap_kernel<false>, a, (unsigned)nq, max_range, pos_ptr != nullptr,
                              [=](size_t n) { return fc::gf_slot_bytes(n) + ball; },
                              fc::gf_slot_bytes(fc::kGfLdsVertices) + (size_t)fc::kLmBallBytes * fc::kLmBallLds, ball, lds_ok,
                              static_cast<hipStream_t>(stream));
}

}  // extern "C"
