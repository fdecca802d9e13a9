// FieldConv forward on per-edge records, ring-major kernels (fc_forward_ring.hpp): instantiation and launch.
#include "fc_forward_route.hpp"

namespace fc {

template <int R, int B, bool GEO, int LOGH>
static int launch_forward_ring(const float2* x, const float* rec, const fc_csr* g, const float* wpk, float2* y, const RingArgs& a,
                               size_t lds, int grid, hipStream_t stream) {
    auto kern = fc_forward_ring_kernel<R, B, GEO, LOGH>;
    static bool lds_ok[kMaxDevices] = {};
    if (!allow_full_lds(reinterpret_cast<const void*>(kern), lds, lds_ok)) return FC_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kDuoThreads), lds, stream, x, rec, g->rowptr, g->runs, wpk, y, a);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int forward_ring_launch(const float* x, const float* rec, const fc_csr* g, const float* wpk, float* out, const fc_dims* d, int kind,
                        const ForwardRoute& r, const FwdEpi& epi, hipStream_t stream) {
    const RingPlan& p = r.ring;
    RingArgs a;
    fill_shared_args(a, d, r, epi);
    a.spread_cus = r.sched.spread_cus;
    a.nr = p.nr;
    a.alias_part = p.alias;
    a.slab_bytes_w = (uint32_t)(2 * p.g.split * p.g.MP * p.g.KP * 2);
    static const bool meter = [] { const char* e = dev_env("FC_STAMP_KERNEL"); return e && e[0] == 'w'; }();
    a.stamps = meter ? nullptr : debug_stamp_buffer();
    a.meter = meter && debug_stamp_buffer() ? debug_stamp_buffer() + kMeterForward : nullptr;
    const int grid = r.sched.grid;
    int rc = FC_ERR_UNSUPPORTED;
    const float2* x2 = reinterpret_cast<const float2*>(x);
    float2* y2 = reinterpret_cast<float2*>(out);
#define FC_CASE(RR, BB)                                                                                            \
    if (d->R == RR && d->B == BB) {                                                                                \
        if constexpr (BB >= 2) {                                                                                   \
            if (p.logh)                                                                                            \
                rc = kind == 2 ? launch_forward_ring<RR, BB, true, 1>(x2, rec, g, wpk, y2, a, p.lds, grid, stream)  \
                               : launch_forward_ring<RR, BB, false, 1>(x2, rec, g, wpk, y2, a, p.lds, grid, stream); \
        }                                                                                                          \
        if (!p.logh)                                                                                               \
            rc = kind == 2 ? launch_forward_ring<RR, BB, true, 0>(x2, rec, g, wpk, y2, a, p.lds, grid, stream)      \
                           : launch_forward_ring<RR, BB, false, 0>(x2, rec, g, wpk, y2, a, p.lds, grid, stream);    \
    }
    FC_FOR_EACH_SHAPE(FC_CASE)
#undef FC_CASE
    return rc;
}

}  // namespace fc
