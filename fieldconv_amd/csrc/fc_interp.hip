// Interpolation weights between two sample levels (fieldconv_amd/transfer.py: interpolation_plan): of all the coarse samples
// within a radius of a receiving sample, the k nearest and their normalised inverse-distance weights.
//
// The candidates arrive as a CSR by receiving row f: cand[e] the coarse position and dist[e] >= 0 its distance, for the slots e
// in [rowptr[f], rowptr[f+1]).  With m = min(k, row length) the row's m smallest slots by the key (dist as a float32 compare,
// cand, slot) go out in that order -- sel[f, i] the slot, weight[f, i] its weight -- and the ranks from m on hold -1 and 0.
// Weights, every operation a float32 operation rounded on its own (tests/_interp_ref.py restates them bit for bit):
//   dist of rank 0 == 0:  1, 0, ..., 0      (a coarse sample reproduces its own value exactly)
//   else  q_i = d_i (power 1) or d_i * d_i (power 2),  u_i = 1 / max(q_i, 1e-30),  s = ((u_0 + u_1) + u_2) + ...,  w_i = u_i / s.
//
// Work split: one lane per row.  A row is short (5 to 40 candidates of which k <= 16 stay) and there are as many rows as fine
// samples, thousands, so the rows alone fill the device; a wavefront per row would leave most of its 64 lanes without a
// candidate and pay a cross-lane sort for a list this small.  The lanes of a wavefront own neighbouring rows, whose slots are
// neighbours in cand / dist, so their loads share cache lines although one load instruction is not contiguous.  A lane keeps the
// best K entries (4, 8 or 16, the least that holds k) sorted in registers as a NearestCand list of fc_select.hpp, three planes
// (dist, cand, slot), and inserts with list_insert_carry.  Lanes of one wavefront run as long as the longest of their rows.
//
// Nothing outside the buffers is touched whatever rowptr holds: its entries are clamped to [0, n_slots] and to the row's own
// start, as fc_transfer clamps them.  No atomics, no workspace, one launch: two runs give the same bits.
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"
#include "fc_select.hpp"

namespace fc {

constexpr int kKnnThreads = 256;
constexpr int kKnnMax = 16;

template <int K>
__global__ __launch_bounds__(kKnnThreads) void knn_weights_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cand,
                                                                  const float* __restrict__ dist, int n_f, int n_slots, int k, int power,
                                                                  int32_t* __restrict__ sel, float* __restrict__ weight) {
    const long long g = (long long)blockIdx.x * kKnnThreads + threadIdx.x;
    if (g >= n_f) return;
    const int f = (int)g;
    const int e0 = min(max(rowptr[f], 0), n_slots), e1 = min(max(rowptr[f + 1], e0), n_slots);

    float bd[K];
    int bc[K], bs[K];
    list_clear<NearestCand>(bd, bc, bs);
    for (int e = e0; e < e1; ++e) list_insert_carry<NearestCand>(bd, bc, bs, dist[e], cand[e], e);

    const int m = min(k, e1 - e0);
    float u[K];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float q = power == 2 ? __fmul_rn(bd[j], bd[j]) : bd[j];
        u[j] = j < m ? __fdiv_rn(1.0f, fmaxf(q, 1e-30f)) : 0.0f;
        if (j == 0) sum = u[0];
        else if (j < m) sum = __fadd_rn(sum, u[j]);
    }
    const bool exact = m > 0 && bd[0] == 0.0f;
    int32_t* srow = sel + (size_t)f * k;
    float* wrow = weight + (size_t)f * k;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) {
            const bool in = j < m && bs[j] != kSelNone;
            const float w = exact ? (j == 0 ? 1.0f : 0.0f) : __fdiv_rn(u[j], sum);
            srow[j] = in ? bs[j] : -1;
            wrow[j] = in ? w : 0.0f;
        }
    }
}

}  // namespace fc

extern "C" {

int fc_knn_weights(const int32_t* rowptr, const int32_t* cand, const float* dist, int32_t n_f, int32_t n_slots, int32_t k, int32_t power,
                   int32_t* sel, float* weight, void* stream) {
    if (n_f < 0 || n_slots < 0 || k < 1 || k > fc::kKnnMax || (power != 1 && power != 2)) return FC_ERR_BAD_ARGUMENT;
    if (n_f == 0) return FC_OK;
    if (!rowptr || !sel || !weight || (n_slots > 0 && (!cand || !dist))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)(((long long)n_f + fc::kKnnThreads - 1) / fc::kKnnThreads);
    fc::dispatch_k<4, 8, 16>(k, [&](auto rung) {
        hipLaunchKernelGGL((fc::knn_weights_kernel<decltype(rung)::value>), dim3(blocks), dim3(fc::kKnnThreads), 0, s, rowptr, cand, dist,
                           (int)n_f, (int)n_slots, (int)k, (int)power, sel, weight);
    });
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // extern "C"
