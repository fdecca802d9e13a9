// FieldConv forward, fp32-MFMA instantiation, the dispatch on the route and what is asked of the route (fc_forward_route.hpp).
#include <stdio.h>
#include "fc_forward_route.hpp"

namespace fc {

template int forward_launch_mode<false>(const float*, const float*, const fc_csr*, const float*, float*, const fc_dims*, int,
                                        const ForwardRoute&, const FwdEpi&, hipStream_t);
extern template int forward_launch_mode<true>(const float*, const float*, const fc_csr*, const float*, float*, const fc_dims*, int,
                                              const ForwardRoute&, const FwdEpi&, hipStream_t);

int forward_impl(const float* x, const float* sten, const fc_csr* g, const float* wpk, float* y, const fc_dims* d,
                 int kind, void* ws, size_t ws_bytes, const fc_epilogue* epi, hipStream_t stream) {
    ForwardRoute r = forward_route(d, kind, num_cus());
    // without a workspace (or with a short one) the tiles are not split: same result, fewer workgroups
    if (!ws || ws_bytes < r.ws_bytes) use_parts(r, 0);
    if (r.status != FC_OK) return r.status;
    const FwdEpi e = make_epi(epi);
    float* const out = r.parts_log2 ? static_cast<float*>(ws) : y;
    const int rc = r.arrangement == Arrangement::kRingMajor ? forward_ring_launch(x, sten, g, wpk, out, d, kind, r, e, stream)
                   : halves_of(d)                           ? forward_launch_mode<true>(x, sten, g, wpk, out, d, kind, r, e, stream)
                                                            : forward_launch_mode<false>(x, sten, g, wpk, out, d, kind, r, e, stream);
    if (rc != FC_OK || r.parts_log2 == 0) return rc;
    return sum_parts_epilogue(static_cast<const float*>(ws), y, (size_t)d->N * d->O, r.part_stride, 1 << r.parts_log2, d->O, e, stream);
}

size_t forward_workspace_bytes(const fc_dims* d, int kind) { return forward_route(d, kind, num_cus()).ws_bytes; }

bool forward_fits(const fc_dims* d) { return forward_route(d, 1, num_cus()).records_fit; }

// Which kernel a forward launch with these dims takes, given its workspace (fc_describe_kernels); kind as in forward_impl.
void describe_forward(const fc_dims* d, int kind, char* buf, size_t n) {
    const ForwardRoute r = forward_route(d, kind, num_cus());
    const char* mode = halves_of(d) == 2 ? "split-f16" : halves_of(d) == 1 ? "f16" : "f32";
    const char* rec = kind == 2 ? "geometric records" : kind == 1 ? "factored records" : "dense rows";
    char what[224], slabs[16] = "";
    if (r.arrangement == Arrangement::kRingMajor) {
        const RingPlan& p = r.ring;
        snprintf(what, sizeof(what), "fc_forward_ring_kernel<%s,%s> (ring-major, 2 workgroups x 8 wavefronts per CU, %zu B LDS, %d %s record chunks%s)",
                 rec, mode, p.lds, p.nr, p.logh ? "half-size" : "1 KiB", p.alias ? ", partials aliased onto the slab" : "");
    } else {
        snprintf(what, sizeof(what), "%s<%s,%s> (frequency-major, 16 wavefronts per CU, parts=%d)", kind ? "fc_forward_factored_kernel" : "fc_forward_kernel",
                 rec, mode, 1 << r.parts_log2);
        snprintf(slabs, sizeof(slabs), " slabs=%d", r.slabs);
    }
    snprintf(buf, n, "%s grid=%d whole=%d half=%d spread=%d lds=%zu cus=%d%s", what, r.sched.grid, r.sched.nv_full, r.sched.nv_total - r.sched.nv_full,
             r.sched.spread_cus ? 1 : 0, r.lds, r.cus, slabs);
}

}  // namespace fc
