// Selection: the best k candidates of a row, kept as a sorted list in registers and merged across lanes and workgroups.
// Users: fc_match.hip (nearest rows), fc_linear_ce.hip (best logits), fc_interp.hip (nearest coarse samples).
//
// Why a result depends on nothing but the candidates.  Every entry type below orders the candidates of a row by a TOTAL order
// (its last field is unique within the row), so "the k best" is one well-defined list whatever the order in which candidates are
// looked at.  Every stage keeps, of the candidates it has seen, the k best in that order, and the k best of a union are the k best
// of the parts' k best.  Hence neither the lane that owns a candidate, nor the split of the candidates over `parts` workgroups,
// nor the order of the merges can change a result, and an exact tie goes to the lower id.  An empty slot sorts after
// every candidate that can be kept and is never inserted itself.  No atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace fc {

constexpr int kSelNone = 0x7fffffff;          // the id of an entry nothing was put into

// An entry type says what a list holds and how it is ordered.  An entry is (key, id) or (key, id, tag): Key, Tag (NoTag where
// there is none), before(k1, i1, t1, k2, i2, t2) (the total order), none_key() (the key of the empty slot, whose id and tag are
// kSelNone).
struct NoTag {
    NoTag() = default;
    __device__ __forceinline__ NoTag(int) {}
};
__device__ __forceinline__ NoTag tag_of_lane_xor(NoTag, int) { return {}; }
__device__ __forceinline__ int tag_of_lane_xor(int t, int mask) { return __shfl_xor(t, mask, 64); }

// fc_match.hip: (d2, row), the smaller distance first.  A NaN distance compares false with everything and is never kept; an
// infinite distance of a real row still beats an empty slot (lower row).
template <typename T>
struct NearestRow {
    using Key = T;
    using Tag = NoTag;
    __device__ __forceinline__ static bool before(T d1, int b1, NoTag, T d2, int b2, NoTag) { return d1 < d2 || (d1 == d2 && b1 < b2); }
    __device__ __forceinline__ static T none_key() { return static_cast<T>(INFINITY); }
};

// fc_linear_ce.hip: (z, class): a real candidate before an empty slot, a number before a NaN, the larger logit first.
struct BestLogit {
    using Key = float;
    using Tag = NoTag;
    __device__ __forceinline__ static bool before(float z1, int c1, NoTag, float z2, int c2, NoTag) {
        if (c2 == kSelNone) return c1 != kSelNone;
        if (c1 == kSelNone) return false;
        const bool n1 = z1 != z1, n2 = z2 != z2;
        if (n1 || n2) return n1 == n2 ? c1 < c2 : n2;
        return z1 > z2 || (z1 == z2 && c1 < c2);
    }
    __device__ __forceinline__ static float none_key() { return -INFINITY; }
};

// fc_interp.hip: (dist, cand, slot) ascending; the slot is the tag.  A NaN distance is never kept.  The compare has no branch on
// purpose (| and & on bools): with || and && hipcc keeps control flow inside the carry insert and knn_weights_kernel<16> takes 101
// VGPRs (4 wavefronts per SIMD) where this form takes 63 (8).
struct NearestCand {
    using Key = float;
    using Tag = int;
    __device__ __forceinline__ static bool before(float d1, int c1, int s1, float d2, int c2, int s2) {
        return (d1 < d2) | ((d1 == d2) & ((c1 < c2) | ((c1 == c2) & (s1 < s2))));
    }
    __device__ __forceinline__ static float none_key() { return __builtin_inff(); }
};

// The sorted list: the K best entries seen, best first, one LOCAL ARRAY per field (key[K], id[K], tag[K]) handed to the functions
// below by reference.  K is a compile-time power of two, every loop is unrolled and every index static: the list lives in
// registers, nothing goes to scratch.  Separate arrays on purpose: with the planes as members of one struct, or as an array of
// entry structs, hipcc allocates the same lists worse (lc_walk_kernel<8>: 150 VGPRs against 134; matching 20 % slower at k = 8).
// The forms without a tag plane are for entries whose Tag is NoTag.
template <class E, int K>
__device__ __forceinline__ void list_clear(typename E::Key (&key)[K], int (&id)[K], typename E::Tag (&tag)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        key[j] = E::none_key();
        id[j] = kSelNone;
        tag[j] = kSelNone;
    }
}

// slots lo < hi: the better of the two entries to lo
template <class E, int K>
__device__ __forceinline__ void list_order(typename E::Key (&key)[K], int (&id)[K], typename E::Tag (&tag)[K], int lo, int hi) {
    const bool sw = E::before(key[hi], id[hi], tag[hi], key[lo], id[lo], tag[lo]);
    const typename E::Key kl = sw ? key[hi] : key[lo], kh = sw ? key[lo] : key[hi];
    const int il = sw ? id[hi] : id[lo], ih = sw ? id[lo] : id[hi];
    const typename E::Tag tl = sw ? tag[hi] : tag[lo], th = sw ? tag[lo] : tag[hi];
    key[lo] = kl, key[hi] = kh;
    id[lo] = il, id[hi] = ih;
    tag[lo] = tl, tag[hi] = th;
}

// Keep the K best of the list and (nk, ni, nt): a newcomer that beats the last entry (rare once the list has warmed up) replaces it
// and sinks to its place.
template <class E, int K>
__device__ __forceinline__ void list_insert(typename E::Key (&key)[K], int (&id)[K], typename E::Tag (&tag)[K], typename E::Key nk, int ni,
                                            typename E::Tag nt) {
    if (!E::before(nk, ni, nt, key[K - 1], id[K - 1], tag[K - 1])) return;
    key[K - 1] = nk;
    id[K - 1] = ni;
    tag[K - 1] = nt;
#pragma unroll
    for (int j = K - 1; j > 0; --j) list_order<E>(key, id, tag, j - 1, j);
}

// The same list without a branch: the newcomer goes in front of the first entry it beats and the displaced entry is carried down
// the list (the list is sorted, so it goes in front of every entry behind it): K compare-and-swaps.
template <class E, int K>
__device__ __forceinline__ void list_insert_carry(typename E::Key (&key)[K], int (&id)[K], typename E::Tag (&tag)[K], typename E::Key nk,
                                                  int ni, typename E::Tag nt) {
    bool carried = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool less = carried | E::before(nk, ni, nt, key[j], id[j], tag[j]);
        carried = less;
        const typename E::Key tk = key[j];
        const int ti = id[j];
        const typename E::Tag tt = tag[j];
        key[j] = less ? nk : tk;
        id[j] = less ? ni : ti;
        tag[j] = less ? nt : tt;
        nk = less ? tk : nk;
        ni = less ? ti : ni;
        nt = less ? tt : nt;
    }
}

// The K best of this lane's list and the list of lane ^ mask, sorted, the same in both lanes.  A bitonic merge: mine against the
// partner's reversed -- the better of each pair are the K best of the union and form a bitonic sequence, which log2 K
// compare-exchange stages sort.
template <class E, int K>
__device__ __forceinline__ void list_merge_xor(typename E::Key (&key)[K], int (&id)[K], typename E::Tag (&tag)[K], int mask) {
    typename E::Key ok[K];
    int oi[K];
    typename E::Tag ot[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        ok[j] = __shfl_xor(key[K - 1 - j], mask, 64);
        oi[j] = __shfl_xor(id[K - 1 - j], mask, 64);
        ot[j] = tag_of_lane_xor(tag[K - 1 - j], mask);
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (E::before(ok[j], oi[j], ot[j], key[j], id[j], tag[j])) {
            key[j] = ok[j];
            id[j] = oi[j];
            tag[j] = ot[j];
        }
#pragma unroll
    for (int s = K / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int j = 0; j < K; ++j)
            if ((j & s) == 0) list_order<E>(key, id, tag, j, j + s);
}

template <class E, int K>
__device__ __forceinline__ void list_clear(typename E::Key (&key)[K], int (&id)[K]) {
    NoTag tag[K];
    list_clear<E>(key, id, tag);
}
template <class E, int K>
__device__ __forceinline__ void list_insert(typename E::Key (&key)[K], int (&id)[K], typename E::Key nk, int ni) {
    NoTag tag[K];
    list_insert<E>(key, id, tag, nk, ni, NoTag{});
}
template <class E, int K>
__device__ __forceinline__ void list_merge_xor(typename E::Key (&key)[K], int (&id)[K], int mask) {
    NoTag tag[K];
    list_merge_xor<E>(key, id, tag, mask);
}

// One thread per row: the k best of the row's `parts` lists, which lie at entry (part n_rows + row) k + j of the two workspace planes.
// An empty slot goes out as id -1 with E::none_key().
constexpr int kPartsMergeThreads = 256;
template <class E, int K>
__global__ __launch_bounds__(kPartsMergeThreads) void parts_merge_kernel(const typename E::Key* __restrict__ keys, const int* __restrict__ ids,
                                                                         int n_rows, int k, int parts, int64_t* __restrict__ idx,
                                                                         typename E::Key* __restrict__ out) {
    const int row = blockIdx.x * kPartsMergeThreads + threadIdx.x;
    if (row >= n_rows) return;
    typename E::Key key[K];
    int id[K];
    list_clear<E>(key, id);
    for (int p = 0; p < parts; ++p)
        for (int j = 0; j < k; ++j) {
            const size_t at = ((size_t)p * n_rows + row) * k + j;
            list_insert<E>(key, id, keys[at], ids[at]);
        }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j >= k) break;
        idx[(size_t)row * k + j] = id[j] == kSelNone ? -1 : id[j];
        out[(size_t)row * k + j] = key[j];
    }
}

template <class E, int K>
void launch_parts_merge(const typename E::Key* keys, const int* ids, int n_rows, int k, int parts, int64_t* idx, typename E::Key* out,
                        hipStream_t s) {
    hipLaunchKernelGGL((parts_merge_kernel<E, K>), dim3((unsigned)((n_rows + kPartsMergeThreads - 1) / kPartsMergeThreads)),
                       dim3(kPartsMergeThreads), 0, s, keys, ids, n_rows, k, parts, idx, out);
}

// parts = 0.  Each of `own_tiles` tiles owns a workgroup per part and walks its share of `walk_tiles` tiles.  parts_cap: the most
// parts the library may choose, enough workgroups to reach target_groups (what a workspace query sizes for).  parts_auto: what it
// chooses, no part shorter than min_tiles_per_part (the merge of a part's lists is paid once per part).
inline int parts_cap(int own_tiles, int target_groups, int max_parts) {
    const int p = target_groups / own_tiles;
    return p < 1 ? 1 : (p > max_parts ? max_parts : p);
}
inline int parts_auto(int own_tiles, int walk_tiles, int target_groups, int max_parts, int min_tiles_per_part) {
    const int cap = parts_cap(own_tiles, target_groups, max_parts), by_range = (walk_tiles + min_tiles_per_part - 1) / min_tiles_per_part;
    return cap < by_range ? cap : by_range;
}

// fn(std::integral_constant<int, K>) for the least rung K of the ascending ladder that holds k (the last rung when none does: the
// callers have checked k against it).
template <int K0, int... Ks, class Fn>
auto dispatch_k(int k, Fn&& fn) {
    if constexpr (sizeof...(Ks) == 0) return fn(std::integral_constant<int, K0>{});
    else return k <= K0 ? fn(std::integral_constant<int, K0>{}) : dispatch_k<Ks...>(k, fn);
}

}  // namespace fc
