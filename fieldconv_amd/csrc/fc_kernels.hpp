// Internal declarations shared by the .hip translation units of libfieldconv_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/fieldconv_hip.h"

// (n_rings, band_limit) pairs with compiled kernels: every n_rings in 2..8 for band limits 1..3 (the
// reference's notebooks use (6,1), (6,2), (6,3)).  Anything else returns FC_ERR_UNSUPPORTED
// (fc_supported() == 0).
#define FC_FOR_EACH_SHAPE(X) \
    X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(6, 1) X(7, 1) X(8, 1) \
    X(2, 2) X(3, 2) X(4, 2) X(5, 2) X(6, 2) X(7, 2) X(8, 2) \
    X(2, 3) X(3, 3) X(4, 3) X(5, 3) X(6, 3) X(7, 3) X(8, 3)

namespace fc {

constexpr size_t kMaxLds = 160 * 1024;
constexpr int kDefaultCUs = 256;     // MI355X: 8 XCDs x 32 CUs (used when no device can be queried, e.g. size queries on a CPU-only box)
constexpr int kMaxDevices = 16;
// Compute units of the current device (hipDeviceAttributeMultiprocessorCount; a partitioned or partial-CU device reports
// fewer than 256): sizes the persistent grids, the edge split and the ring-major threshold.  Queried once per device.
inline int num_cus() {
    static int cached[kMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return kDefaultCUs;
    if (dev < kMaxDevices && cached[dev] > 0) return cached[dev];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = kDefaultCUs;
    if (dev < kMaxDevices) cached[dev] = n;
    return n;
}
constexpr int kMaxChannels = 64;     // one channel per lane in the gather phases

// kind: 0 dense stencil rows, 1 factored records, 2 geometric-phase records
// ws: optional scratch of forward_workspace_bytes(d, kind) bytes that lets several workgroups share a tile on small meshes; the callers
// hand over what they have: a missing or short one runs the unsplit launch (same result)
int forward_impl(const float* x, const float* sten, const fc_csr* g, const float* wpk, float* y,
                 const fc_dims* d, int kind, void* ws, size_t ws_bytes, const fc_epilogue* epi, hipStream_t stream);
size_t forward_workspace_bytes(const fc_dims* d, int kind);
size_t backward_workspace_bytes(const fc_dims* d);
// What a backward entry point is told about its pass; from these and the dims backward_route() (fc_backward_stream.hpp) picks the arrangement.
enum class Drive { kDenseRows, kRecords };      // the launch reads dense stencil rows / factored records (the C ABI's `records`)
inline Drive drive_of(int records) { return records ? Drive::kRecords : Drive::kDenseRows; }
// kDeferred: the partial gx arrays of shared tiles, or the gxt slices, stay in the workspace and the finishing launch forms gx (DeferredGx)
enum class GxSum { kInPass, kDeferred };
enum class StreamStages { kGather, kStream, kWholePass };      // the gather kernel | the streaming kernel + gx (fc_backward_gather / _stream time them apart)
int backward_data_impl(const float* x, const float* gy, const float* sten, const fc_csr* g, const float* wpk, float* gx,
                       void* ws, size_t ws_bytes, const fc_dims* d, Drive drive, hipStream_t stream, GxSum gx_sum);
int backward_filter_impl(const float* x, void* ws, size_t ws_bytes, const fc_dims* d, Drive drive, hipStream_t stream);
bool backward_streams(const fc_dims* d, Drive drive);
int backward_stream_impl(const float* x, const float* gy, const float* rec, const fc_csr* g, const float* wpk, float* gx, void* ws,
                         size_t ws_bytes, const fc_dims* d, hipStream_t stream, StreamStages stages);
int backward_finish_impl(float* gw_eff, void* ws, size_t ws_bytes, const fc_dims* d, Drive drive, hipStream_t stream);
// records != 0: images for the record-driven entry points (fc_forward_factored / _geometric, fc_backward_all and the staged backward calls)
int pack_filter_impl(const float* w_eff, float* wpk_fwd, float* wpk_bwd, const fc_dims* d, int records, hipStream_t stream);
int pack_filter_params_impl(const float* zonal, const float* sph, const float* phase, int ftype, float* wpk_fwd,
                            float* wpk_bwd, const fc_dims* d, int records, hipStream_t stream);
// the filter images of TWO layers from one launch (an FCResNetBlock's two convolutions)
int pack_filter_params_pair_impl(const fc_filter_params& f0, float* fwd0, float* bwd0, const fc_dims* d0, const fc_filter_params& f1,
                                 float* fwd1, float* bwd1, const fc_dims* d1, int records, hipStream_t stream);
size_t packed_filter_floats_fwd(const fc_dims* d, int records);
size_t packed_filter_floats_bwd(const fc_dims* d, int records);

int filter_param_grads_impl(const float* gw_eff, const float* zonal, const float* sph, const float* phase, int ftype,
                            float* g_zonal, float* g_sph, float* g_phase, const fc_dims* d, hipStream_t stream);

// reduction of the filter-gradient partials fused with the parameter-gradient chain (fc_pack.hip); backward_route() fills in the
// partial layout of its kernel family.  Partial (p, r, f, o, i) lies at gwp[p*sp + r*sr + f*sf + o*so + i]; with ring_pairs the
// (r, o) part is dump_k(r, o) * so instead.
struct PartialsLayout { const float* gwp; size_t sp, sr, sf, so; bool ring_pairs; int P; };
// the filter is the block [o0, o0 + O) x [i0, i0 + I) of parameter tensors with Ifull input channels; the default: the whole layer
struct FilterBlock { int o0 = 0, i0 = 0, Ifull = 0; };
// A rider of the finishing launch: extra workgroups complete gx, (N, I) complex numbers.  kSumParts: the sum of the data kernel's
// `nparts` partial arrays, `stride` apart (fc_sum_parts_kernel's arithmetic; one part or no gx: nothing to add).  kFromSlices: from the
// streaming kernel's gxt slices and x, band limit B, KS slices per frequency (fc_backward_gx_kernel's arithmetic).
struct GxRider {
    enum Kind { kNone, kSumParts, kFromSlices } kind = kNone;
    float* gx = nullptr;
    struct SumParts { const float* parts; size_t stride; int nparts; } sum = {};
    struct FromSlices { const float* gxt; const float* x; int B, KS; } slices = {};
};
// (fc_filter_params' rider, bias_partials: more workgroups sum the modReLU's bias-gradient partials, as tangent_nonlin_gb_reduce_kernel does)
int reduce_param_grads_impl(const PartialsLayout& partials, float* gw_eff, const fc_filter_params& fp, const FilterBlock& block,
                            const GxRider& gx_rider, const fc_dims* d, hipStream_t stream);
// the rider as a launch of its own (fc_pointwise.hip): g_bias[c] = fixed-order sum over p of partials[p][c]
int bias_partials_reduce_impl(const float* partials, int nparts, int C, float* g_bias, hipStream_t stream);

// k index of entry (ring r, channel o) in a row of the kept H slabs, hence of the filter-gradient partials.  The split modes keep the
// rings in PAIRS -- (2p, o) and (2p + 1, o) adjacent -- so that the data kernel stores two entries with one instruction; the last ring
// of an odd count, and every ring in fp32 mode, lie ring-major.
__host__ __device__ inline int dump_k(int r, int o, int R, int O, bool pairs) {
    return (pairs && (r | 1) < R) ? (r >> 1) * 2 * O + 2 * o + (r & 1) : r * O + o;
}
// what backward_data_impl left unfinished under GxSum::kDeferred: where gx goes, and x (the streaming arrangement's gx needs it)
struct DeferredGx { float* gx = nullptr; const float* x = nullptr; };
int backward_finish_params_impl(float* gw_eff, void* ws, size_t ws_bytes, const fc_dims* d, Drive drive, const fc_filter_params& fp,
                                const FilterBlock& block, const DeferredGx& deferred, hipStream_t stream);
int pack_filter_block_impl(const float* w_eff, float* wpk_fwd, float* wpk_bwd, const fc_dims* d, int records, int o0, int i0, int Ifull,
                           hipStream_t stream);
int pack_filter_params_block_impl(const float* zonal, const float* sph, const float* phase, int ftype, float* wpk_fwd, float* wpk_bwd,
                                  const fc_dims* d, int records, int o0, int i0, int Ifull, hipStream_t stream);

bool shape_compiled(int R, int B);
// the record-driven kernels form 32-bit row offsets with a 24-bit multiply: N < 2^24 and N * channels * 8 < 4 GiB
bool rows_fit_32bit(const fc_dims* d);
// one-line descriptions of the kernels a launch with these dims selects (fc_describe_kernels)
void describe_forward(const fc_dims* d, int kind, char* buf, size_t n);
void describe_backward(const fc_dims* d, int records, char* buf, size_t n);

// TangentLin's backward pass (fc_pointwise.hip) with an optional addend of the input gradient (may be gx itself): the block-level
// entry points (fc_blocks.hip) add the residual branch's input gradient to the convolution's inside this launch
int tangent_lin_backward_impl(const float* x, const float* gy, const float* re_w, const float* im_w, float* gx, const float* gx_addend,
                              float* g_re, float* g_im, void* workspace, size_t workspace_bytes, int N, int I, int O, hipStream_t s);

// FCPrecomp's area sums total[dst] += w[src] over the kept edges (csrc/fc_precomp.hip), shared with the fused build
int precomp_area_sums(const int64_t* edges, const int32_t* keep, const float* w, float* total, int N, int E, hipStream_t s);

// development: device buffer that receives in-kernel time stamps (fc_debug_stamp_buffer), or nullptr
unsigned long long* debug_stamp_buffer();

// Kernels with more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised -- once per
// function and device, not per launch (the call costs a few microseconds of host time).  `done`: a static flag array of
// the calling launcher (one per kernel instantiation).
inline bool allow_full_lds(const void* fn, size_t lds_bytes, bool (&done)[kMaxDevices]) {
    if (lds_bytes <= 64 * 1024) return true;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (dev >= 0 && dev < kMaxDevices && done[dev]) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds) != hipSuccess) return false;
    if (dev >= 0 && dev < kMaxDevices) done[dev] = true;
    return true;
}
template <typename K, typename... A>
int launch_full_lds(K kern, bool (&done)[kMaxDevices], dim3 grid, size_t lds_bytes, hipStream_t stream, A... args) {
    if (!allow_full_lds(reinterpret_cast<const void*>(kern), lds_bytes, done)) return FC_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, grid, dim3(1024), lds_bytes, stream, args...);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}
// LDS budget of the factored kernels in the current MFMA mode (the dense kernels need less)
bool forward_fits(const fc_dims* d);
bool backward_fits(const fc_dims* d);

}  // namespace fc
