// What a forward call runs, resolved ONCE per question: forward_impl, describe_forward, the size queries and the filter pack all read
// the answer of forward_route().
//
// Pack and launch each build a route and must be given the same dims and the same kind / records -- pack's `records & 1` is the launch's
// `kind != 0`.  The route fixes the LAYOUT of the packed forward image (ring_image), and nothing in an image says which layout it has: an
// image packed with records = 0 and launched as records on a mesh that runs ring-major (or packed for another vertex count, on the other
// side of the ring-major threshold) is read in the other layout -- wrong numbers, not an error.
#pragma once
#include "fc_forward_kernels.hpp"
#include "fc_forward_ring.hpp"

namespace fc {

struct ForwardRoute {
    int status;                 // FC_OK, or FC_ERR_UNSUPPORTED: the arrangement's LDS plan does not fit
    Arrangement arrangement;
    MmaGeom g;                  // the launch's contraction geometry (ring-major: ring.g)
    RingPlan ring;              // ring-major only
    bool records_fit;           // the frequency-major record kernels fit the LDS with one slab buffer: what fc_supported promises for any N
    int cus, ntiles;
    size_t record_ring_bytes;   // frequency-major records: the wavefronts' LDS record rings
    bool k_padded;              // frequency-major: slab rows end in k padding [R*KI, KP)
    // the edge split the route uses GIVEN a workspace of ws_bytes (use_parts: the caller's answer), and what follows from it
    int parts_log2;
    size_t part_stride, ws_bytes;
    TileSchedule sched;
    int slabs;                  // frequency-major: slab buffers in LDS (FwdArgs::slabs)
    size_t lds;
    size_t image_floats;        // the packed forward image
    bool ring_image;            // ... in the ring-major layout
};

// The schedule for a split of 2^parts_log2, and what depends on it: slabs (on grid and items) and the LDS bytes.
inline void use_parts(ForwardRoute& r, int parts_log2) {
    r.parts_log2 = parts_log2;
    r.ws_bytes = parts_log2 ? (r.part_stride << parts_log2) * sizeof(float2) : 0;
    r.sched = tile_schedule(r.ntiles, parts_log2, r.cus, r.arrangement);
    if (r.arrangement == Arrangement::kRingMajor) {
        r.slabs = 0;
        r.lds = r.ring.lds;
        return;
    }
    // With two slab buffers the epilogue parks its fp32 k-partials in the idle one.  A workgroup that walks several
    // tiles would then read those bits back as halves in the k padding [R*KI, KP) of the next tile's slab rows (the
    // padding is zeroed once, before the tile loop), and 0 x NaN poisons the accumulators: shapes with k padding
    // keep the partials in their own region whenever a workgroup sees more than one tile.
    const bool aliasing_hazard = r.k_padded && r.sched.grid < r.sched.nv_total;
    r.slabs = (r.g.split && !aliasing_hazard && partial_floats(r.g.NKP, r.g.MP) <= slab_floats(r.g) &&
               forward_lds_floats(r.g, 2) * sizeof(float) + r.record_ring_bytes <= kMaxLds) ? 2 : 1;
    r.lds = forward_lds_floats(r.g, r.slabs) * sizeof(float) + r.record_ring_bytes;
    r.status = r.lds > kMaxLds ? FC_ERR_UNSUPPORTED : FC_OK;
}

// kind as in forward_impl; cus: num_cus() (a parameter, so that the route of any part can be asked for).  A pure function of its
// arguments and the development switches.
//
// Meshes of up to one tile per CU (4096 vertices on 256 CUs) are one round of the frequency-major kernels (one 16-vertex tile per CU, with
// the edge split for the smallest ones), which they keep: 41 against 46 us at C = 48, k = 32.  From there on the frequency-major grid
// needs a second round while the ring-major one (two workgroups per CU) still takes one: 59 against 66 us between 4097 and 8192
// vertices, 91 against 94 up to 12288 (tools/ring_threshold.py); config 2 on MI355X: 138 us against 150 us.  The ring-major kernels exist
// for the default two-halves mode.  FC_RING=0 keeps the frequency-major kernels, FC_RING=2 forces the ring-major ones for any size (tests).
inline ForwardRoute forward_route(const fc_dims* d, int kind, int cus) {
    static const int ring_switch = [] { const char* e = dev_env("FC_RING"); return e ? atoi(e) : 1; }();       // read once per process
    const int F = 2 * d->B + 1, halves = halves_of(d);
    ForwardRoute r = {};
    r.cus = cus;
    r.ntiles = (d->N + kTile - 1) / kTile;
    r.g = make_mma_geom(d->O, d->R, d->I, halves);
    const size_t record_rings = (size_t)kWaves * kRingChunks * 1024;
    r.record_ring_bytes = kind ? record_rings : 0;
    r.records_fit = forward_lds_floats(r.g, 1) * sizeof(float) + record_rings <= kMaxLds;
    r.k_padded = r.g.KP > d->R * r.g.KI;
    r.arrangement = kind ? Arrangement::kFrequencyMajor : Arrangement::kDenseRows;
    if (kind && ring_switch != 0 && halves == 2 && (ring_switch == 2 || r.ntiles > cus)) {
        r.ring = plan_ring(d->O, F, d->I, halves);
        if (r.ring.ok) {
            r.arrangement = Arrangement::kRingMajor;
            r.g = r.ring.g;
        }
    }
    r.ring_image = r.arrangement == Arrangement::kRingMajor;
    r.image_floats = r.ring_image ? packed_ring_image_floats(d->O, F, d->I, d->R, halves) : packed_image_floats(d->O, d->R, d->I, F, halves);
    r.part_stride = part_stride((size_t)d->N * d->O);
    use_parts(r, kind ? edge_parts_log2(d, cus) : 0);
    return r;
}

// The fields FwdArgs and RingArgs share.
template <typename Args>
void fill_shared_args(Args& a, const fc_dims* d, const ForwardRoute& r, const FwdEpi& epi) {
    a.N = d->N; a.I = d->I; a.O = d->O;
    a.g = r.g;
    a.ntiles = r.ntiles;
    a.nv_full = r.sched.nv_full;
    a.nv_total = r.sched.nv_total;
    a.parts_log2 = r.parts_log2;
    a.part_stride = (uint32_t)r.part_stride;
    a.wpk_bytes = (uint32_t)(r.image_floats * sizeof(float));
    static const int dbg = [] { const char* e = dev_env("FC_DEBUG"); return e ? atoi(e) : 0; }();       // read once per process
    a.dbg = dbg;
    a.epi = epi;
}

// The arrangement-specific launches; `out`: y, or the workspace's partial outputs when the route splits the tiles (forward_impl).
int forward_ring_launch(const float* x, const float* rec, const fc_csr* g, const float* wpk, float* out, const fc_dims* d, int kind,
                        const ForwardRoute& r, const FwdEpi& epi, hipStream_t stream);

template <bool SPLIT>
int forward_launch_mode(const float* x, const float* sten, const fc_csr* g, const float* wpk, float* out, const fc_dims* d, int kind,
                        const ForwardRoute& r, const FwdEpi& epi, hipStream_t stream) {
    FwdArgs a;
    fill_shared_args(a, d, r, epi);
    a.ring_chunks = kind ? kRingChunks : 0;
    a.slabs = r.slabs;
    int rc = FC_ERR_UNSUPPORTED;
    const float2* x2 = reinterpret_cast<const float2*>(x);
    float2* y2 = reinterpret_cast<float2*>(out);
#define FC_CASE(RR, BB)                                                                                                   \
    if (d->R == RR && d->B == BB) {                                                                                       \
        if (kind == 2) rc = launch_forward<RR, BB, 2, SPLIT>(x2, sten, g, wpk, y2, a, r.lds, r.sched.grid, stream);       \
        else if (kind == 1) rc = launch_forward<RR, BB, 1, SPLIT>(x2, sten, g, wpk, y2, a, r.lds, r.sched.grid, stream);  \
        else rc = launch_forward<RR, BB, 0, SPLIT>(x2, sten, g, wpk, y2, a, r.lds, r.sched.grid, stream);                 \
    }
    FC_FOR_EACH_SHAPE(FC_CASE)
#undef FC_CASE
    return rc;
}

}  // namespace fc
