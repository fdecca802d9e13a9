// Whole network blocks from ONE foreign call per pass (include/fieldconv_hip.h, "whole blocks").
//
//   FCResNetBlock  reference nn/fc_resnet_block.py:65-88   out = modReLU_2(res(x) + conv2(modReLU_1(conv1(x))))
//   ECHOBlock      reference nn/echo_block.py:93-94        desc = ECHO(modReLU(conv(x)))   (the MLP behind it is the reference's nn.Linear)
//   LiftBlock      reference nn/lift_block.py:53-55        out = modReLU(TransField(x))
//
// Nothing here computes: every function lays the caller's `saved` / `workspace` buffers out and enqueues the kernels of the
// per-operator entry points in the order the reference applies the operators.  What it removes is the HOST side of a block --
// sixteen foreign calls, a dozen tensor allocations and five autograd nodes per FCResNetBlock pass pair -- which on the
// reference's ~1k-vertex meshes (a new one every step, so a captured HIP graph does not apply) cost more than the GPU work.
#include "fc_common.hpp"
#include "fc_kernels.hpp"
#include "fc_workspace.hpp"

namespace fc {


static bool mesh_valid(const fc_mesh* m, bool need_records) {
    if (!m || m->N <= 0 || m->E < 0 || m->R <= 0 || m->B < 0 || m->kind < 0 || m->kind > 2) return false;
    if (!m->by_target || !m->by_source || !m->by_target->rowptr || !m->by_source->rowptr) return false;
    if (need_records && m->E > 0 && (!m->fwd || !m->bwd)) return false;
    return true;
}

static fc_dims conv_dims(const fc_mesh* m, int I, int O) { return fc_dims{m->N, m->E, I, O, m->R, m->B, m->mode}; }

// ---- FCResNetBlock ----------------------------------------------------------------------------------------------------------
struct ResnetPlan {
    fc_dims d1, d2;
    int records, kind, C_in, C_mid, C_out;
    size_t N;
};

static bool resnet_plan(const fc_mesh* m, const fc_resnet_block_params* p, ResnetPlan& pl) {
    if (!mesh_valid(m, true) || !p || p->C_in <= 0 || p->C_mid <= 0 || p->C_out <= 0) return false;
    pl.d1 = conv_dims(m, p->C_in, p->C_mid);
    pl.d2 = conv_dims(m, p->C_mid, p->C_out);
    if (!fc_supported(&pl.d1) || !fc_supported(&pl.d2)) return false;
    pl.records = m->kind != 0 ? 1 : 0;
    pl.kind = m->kind;
    pl.C_in = p->C_in, pl.C_mid = p->C_mid, pl.C_out = p->C_out;
    pl.N = (size_t)m->N;
    return true;
}

struct ResnetSaved { float *pre1, *act1, *pre2, *wpk_b1, *wpk_b2; };
static ResnetSaved resnet_saved(Carver& c, const ResnetPlan& pl) {
    return {c.take<float>(pl.N * pl.C_mid * 8), c.take<float>(pl.N * pl.C_mid * 8), c.take<float>(pl.N * pl.C_out * 8),
            c.take<float>(packed_filter_floats_bwd(&pl.d1, pl.records) * sizeof(float)),
            c.take<float>(packed_filter_floats_bwd(&pl.d2, pl.records) * sizeof(float))};
}

struct ResnetFwdWs { float *wpk_f1, *wpk_f2, *res_out; void* conv; size_t conv_bytes; };
static ResnetFwdWs resnet_fwd_ws(Carver& c, const ResnetPlan& pl) {
    ResnetFwdWs w;
    w.wpk_f1 = c.take<float>(packed_filter_floats_fwd(&pl.d1, pl.records) * sizeof(float));
    w.wpk_f2 = c.take<float>(packed_filter_floats_fwd(&pl.d2, pl.records) * sizeof(float));
    w.res_out = c.take<float>(pl.N * pl.C_out * 8);
    const size_t f1 = pl.records ? forward_workspace_bytes(&pl.d1, pl.kind) : 0, f2 = pl.records ? forward_workspace_bytes(&pl.d2, pl.kind) : 0;
    w.conv = c.take(f1 > f2 ? f1 : f2, &w.conv_bytes);
    return w;
}

// (the convolutions' gW_eff tensors are not wanted, so they have no piece: fc_backward_all pulls the partial sums back to the parameters)
struct ResnetBwdWs { float *g_pre2, *g_h, *g_pre1, *part1, *part2; void *lin, *conv; size_t part1_bytes, part2_bytes, lin_bytes, conv_bytes; };
static ResnetBwdWs resnet_bwd_ws(Carver& c, const ResnetPlan& pl) {
    ResnetBwdWs w;
    const int N = (int)pl.N;
    w.g_pre2 = c.take<float>(pl.N * pl.C_out * 8);
    w.g_h = c.take<float>(pl.N * pl.C_mid * 8);
    w.g_pre1 = c.take<float>(pl.N * pl.C_mid * 8);
    w.part1 = c.take<float>(fc_tangent_nonlin_backward_workspace_bytes(N, pl.C_mid), &w.part1_bytes);
    w.part2 = c.take<float>(fc_tangent_nonlin_backward_workspace_bytes(N, pl.C_out), &w.part2_bytes);
    w.lin = c.take(fc_tangent_lin_backward_workspace_bytes(N, pl.C_in, pl.C_out), &w.lin_bytes);
    const size_t b1 = backward_workspace_bytes(&pl.d1), b2 = backward_workspace_bytes(&pl.d2);
    w.conv = c.take(b1 > b2 ? b1 : b2, &w.conv_bytes);
    return w;
}

static bool filter_params_ok(const fc_filter_params& f, bool backward) {
    if (!f.zonal || !f.spherical || f.ftype < 0 || f.ftype > 2 || (f.ftype == 1 && !f.phase)) return false;
    if (backward && (!f.g_zonal || !f.g_spherical || (f.ftype == 1 && !f.g_phase))) return false;
    return true;
}

// packed = true: the images were written by an earlier launch of this pass (pack_filter_params_pair_impl)
static int conv_forward(const float* x, const fc_mesh* m, const fc_dims* d, const fc_filter_params& f, float* wpk_f, float* wpk_b, float* y,
                        const fc_epilogue* epi, void* ws, size_t ws_bytes, int records, hipStream_t st, bool packed = false) {
    if (!packed) {
        const int rc = pack_filter_params_impl(f.zonal, f.spherical, f.phase, f.ftype, wpk_f, wpk_b, d, records, st);
        if (rc != FC_OK) return rc;
    }
    return forward_impl(x, m->fwd, m->by_target, wpk_f, y, d, m->kind, ws, ws_bytes, epi, st);
}

}  // namespace fc

extern "C" {

size_t fc_resnet_block_saved_bytes(const fc_mesh* mesh, const fc_resnet_block_params* p) {
    fc::ResnetPlan pl;
    return fc::resnet_plan(mesh, p, pl) ? fc::carved_bytes(fc::resnet_saved, pl) : 0;
}

size_t fc_resnet_block_workspace_bytes(const fc_mesh* mesh, const fc_resnet_block_params* p, int32_t backward) {
    fc::ResnetPlan pl;
    if (!fc::resnet_plan(mesh, p, pl)) return 0;
    return backward ? fc::carved_bytes(fc::resnet_bwd_ws, pl) : fc::carved_bytes(fc::resnet_fwd_ws, pl);
}

int fc_resnet_block_forward(const float* x, const fc_mesh* mesh, const fc_resnet_block_params* p, float* out, void* saved,
                            size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !out || !fc::mesh_valid(mesh, true) || !p) return FC_ERR_BAD_ARGUMENT;
    if (!fc::filter_params_ok(p->conv1, false) || !fc::filter_params_ok(p->conv2, false) || !p->bias1 || !p->bias2 || !p->res_re || !p->res_im)
        return FC_ERR_BAD_ARGUMENT;
    fc::ResnetPlan pl;
    if (!fc::resnet_plan(mesh, p, pl)) return FC_ERR_UNSUPPORTED;
    if (!saved || saved_bytes < fc::carved_bytes(fc::resnet_saved, pl) || !workspace || workspace_bytes < fc::carved_bytes(fc::resnet_fwd_ws, pl))
        return FC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    fc::Carver sv(saved), ws(workspace);
    const fc::ResnetSaved s = fc::resnet_saved(sv, pl);
    const fc::ResnetFwdWs w = fc::resnet_fwd_ws(ws, pl);
    // both convolutions' filter images (forward and backward) from one launch: the parameters are all known now
    int rc = fc::pack_filter_params_pair_impl(p->conv1, w.wpk_f1, s.wpk_b1, &pl.d1, p->conv2, w.wpk_f2, s.wpk_b2, &pl.d2, pl.records, st);
    if (rc != FC_OK) return rc;
    // h = modReLU_1(conv1(x)): the modReLU in the convolution's epilogue (pre1 = the pre-activation its VJP needs)
    fc_epilogue e1 = {nullptr, p->bias1, s.act1};
    rc = fc::conv_forward(x, mesh, &pl.d1, p->conv1, w.wpk_f1, s.wpk_b1, s.pre1, &e1, w.conv, w.conv_bytes, pl.records, st, true);
    if (rc != FC_OK) return rc;
    // res(x)
    rc = fc_tangent_lin_forward(x, p->res_re, p->res_im, w.res_out, mesh->N, p->C_in, p->C_out, stream);
    if (rc != FC_OK) return rc;
    // out = modReLU_2(res(x) + conv2(h)): residual add and modReLU in conv2's epilogue
    fc_epilogue e2 = {w.res_out, p->bias2, out};
    return fc::conv_forward(s.act1, mesh, &pl.d2, p->conv2, w.wpk_f2, s.wpk_b2, s.pre2, &e2, w.conv, w.conv_bytes, pl.records, st, true);
}

int fc_resnet_block_backward(const float* x, const float* g_out, const fc_mesh* mesh, const fc_resnet_block_params* p, const void* saved,
                             size_t saved_bytes, float* gx, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !g_out || !gx || !fc::mesh_valid(mesh, true) || !p) return FC_ERR_BAD_ARGUMENT;
    if (!fc::filter_params_ok(p->conv1, true) || !fc::filter_params_ok(p->conv2, true) || !p->bias1 || !p->bias2 || !p->res_re || !p->res_im ||
        !p->g_bias1 || !p->g_bias2 || !p->g_res_re || !p->g_res_im)
        return FC_ERR_BAD_ARGUMENT;
    fc::ResnetPlan pl;
    if (!fc::resnet_plan(mesh, p, pl)) return FC_ERR_UNSUPPORTED;
    if (!saved || saved_bytes < fc::carved_bytes(fc::resnet_saved, pl) || !workspace || workspace_bytes < fc::carved_bytes(fc::resnet_bwd_ws, pl))
        return FC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    fc::Carver sv(saved), ws(workspace);
    const fc::ResnetSaved s = fc::resnet_saved(sv, pl);
    const fc::ResnetBwdWs w = fc::resnet_bwd_ws(ws, pl);
    const int N = mesh->N;
    // modReLU_2: g_pre2 and the bias-gradient partials, which conv2's finishing launch sums (fc_filter_params' rider)
    int rc = fc_tangent_nonlin_backward_partial(s.pre2, p->bias2, g_out, w.g_pre2, w.part2, w.part2_bytes, N, p->C_out, stream);
    if (rc != FC_OK) return rc;
    fc_filter_params f2 = p->conv2;
    f2.bias_partials = w.part2;
    f2.bias_nparts = fc_tangent_nonlin_backward_groups(N);
    f2.g_bias = p->g_bias2;
    rc = fc_backward_all(s.act1, w.g_pre2, mesh->bwd, mesh->by_source, pl.records, s.wpk_b2, w.g_h, nullptr, &f2, w.conv, w.conv_bytes, &pl.d2,
                         stream);
    if (rc != FC_OK) return rc;
    // modReLU_1 and conv1: gx = conv1's input gradient ...
    rc = fc_tangent_nonlin_backward_partial(s.pre1, p->bias1, w.g_h, w.g_pre1, w.part1, w.part1_bytes, N, p->C_mid, stream);
    if (rc != FC_OK) return rc;
    fc_filter_params f1 = p->conv1;
    f1.bias_partials = w.part1;
    f1.bias_nparts = fc_tangent_nonlin_backward_groups(N);
    f1.g_bias = p->g_bias1;
    rc = fc_backward_all(x, w.g_pre1, mesh->bwd, mesh->by_source, pl.records, s.wpk_b1, gx, nullptr, &f1, w.conv, w.conv_bytes, &pl.d1, stream);
    if (rc != FC_OK) return rc;
    // ... plus the residual branch's (res sees the same cotangent as conv2: g_pre2), added by the TangentLin kernel itself
    return fc::tangent_lin_backward_impl(x, w.g_pre2, p->res_re, p->res_im, gx, gx, p->g_res_re, p->g_res_im, w.lin, w.lin_bytes, N, p->C_in,
                                         p->C_out, st);
}

}  // extern "C"

// ---- ECHOBlock (tangent-feature half) ---------------------------------------------------------------------------------------
namespace fc {

struct EchoPlan {
    fc_dims d;
    int records, kind, dS, n_des;
    size_t N;
};

static bool echo_plan(const fc_mesh* m, const fc_echo_block_params* p, EchoPlan& pl) {
    if (!mesh_valid(m, true) || !p || p->C_in <= 0 || p->n_des <= 0) return false;
    pl.dS = fc_echo_hist_dim(p->n_bins);
    if (pl.dS == 0) return false;
    pl.d = conv_dims(m, p->C_in, p->n_des);
    if (!fc_supported(&pl.d)) return false;
    pl.records = m->kind != 0 ? 1 : 0;
    pl.kind = m->kind;
    pl.n_des = p->n_des;
    pl.N = (size_t)m->N;
    return true;
}

struct EchoSaved { float *pre, *act, *hist, *wpk_b; };
static EchoSaved echo_saved(Carver& c, const EchoPlan& pl) {
    return {c.take<float>(pl.N * pl.n_des * 8), c.take<float>(pl.N * pl.n_des * 8), c.take<float>(pl.N * pl.n_des * pl.dS * 8),
            c.take<float>(packed_filter_floats_bwd(&pl.d, pl.records) * sizeof(float))};
}

struct EchoFwdWs { float* wpk_f; void* conv; size_t conv_bytes; };
static EchoFwdWs echo_fwd_ws(Carver& c, const EchoPlan& pl) {
    EchoFwdWs w;
    w.wpk_f = c.take<float>(packed_filter_floats_fwd(&pl.d, pl.records) * sizeof(float));
    w.conv = c.take(pl.records ? forward_workspace_bytes(&pl.d, pl.kind) : 0, &w.conv_bytes);
    return w;
}

struct EchoBwdWs { float *g_act, *g_pre, *part, *gh; void* conv; size_t part_bytes, conv_bytes; };
static EchoBwdWs echo_bwd_ws(Carver& c, const EchoPlan& pl) {
    EchoBwdWs w;
    w.g_act = c.take<float>(pl.N * pl.n_des * 8);
    w.g_pre = c.take<float>(pl.N * pl.n_des * 8);
    w.part = c.take<float>(fc_tangent_nonlin_backward_workspace_bytes((int)pl.N, pl.n_des), &w.part_bytes);
    w.gh = c.take<float>(pl.N * pl.n_des * pl.dS * 8);
    w.conv = c.take(backward_workspace_bytes(&pl.d), &w.conv_bytes);
    return w;
}

}  // namespace fc

extern "C" {

size_t fc_echo_block_saved_bytes(const fc_mesh* mesh, const fc_echo_block_params* p) {
    fc::EchoPlan pl;
    return fc::echo_plan(mesh, p, pl) ? fc::carved_bytes(fc::echo_saved, pl) : 0;
}

size_t fc_echo_block_workspace_bytes(const fc_mesh* mesh, const fc_echo_block_params* p, int32_t backward) {
    fc::EchoPlan pl;
    if (!fc::echo_plan(mesh, p, pl)) return 0;
    return backward ? fc::carved_bytes(fc::echo_bwd_ws, pl) : fc::carved_bytes(fc::echo_fwd_ws, pl);
}

int fc_echo_block_forward(const float* x, const fc_mesh* mesh, const float* ln_t, const float* wxp_t, const fc_echo_block_params* p,
                          float* desc, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !desc || !fc::mesh_valid(mesh, true) || !p || !fc::filter_params_ok(p->conv, false) || !p->bias) return FC_ERR_BAD_ARGUMENT;
    if (mesh->E > 0 && (!ln_t || !wxp_t || !mesh->by_target->nbr)) return FC_ERR_BAD_ARGUMENT;
    fc::EchoPlan pl;
    if (!fc::echo_plan(mesh, p, pl)) return FC_ERR_UNSUPPORTED;
    if (!saved || saved_bytes < fc::carved_bytes(fc::echo_saved, pl) || !workspace || workspace_bytes < fc::carved_bytes(fc::echo_fwd_ws, pl))
        return FC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    fc::Carver sv(saved), ws(workspace);
    const fc::EchoSaved s = fc::echo_saved(sv, pl);
    const fc::EchoFwdWs w = fc::echo_fwd_ws(ws, pl);
    fc_epilogue e = {nullptr, p->bias, s.act};
    int rc = fc::conv_forward(x, mesh, &pl.d, p->conv, w.wpk_f, s.wpk_b, s.pre, &e, w.conv, w.conv_bytes, pl.records, st);
    if (rc != FC_OK) return rc;
    return fc_echo_forward(s.act, ln_t, wxp_t, mesh->by_target, s.hist, desc, mesh->N, mesh->E, p->n_des, p->n_bins, stream);
}

int fc_echo_block_backward(const float* x, const float* g_desc, const fc_mesh* mesh, const float* ln_s, const float* wxp_s,
                           const fc_echo_block_params* p, const void* saved, size_t saved_bytes, float* gx, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!x || !g_desc || !gx || !fc::mesh_valid(mesh, true) || !p || !fc::filter_params_ok(p->conv, true) || !p->bias || !p->g_bias)
        return FC_ERR_BAD_ARGUMENT;
    if (mesh->E > 0 && (!ln_s || !wxp_s || !mesh->by_source->nbr)) return FC_ERR_BAD_ARGUMENT;
    fc::EchoPlan pl;
    if (!fc::echo_plan(mesh, p, pl)) return FC_ERR_UNSUPPORTED;
    if (!saved || saved_bytes < fc::carved_bytes(fc::echo_saved, pl) || !workspace || workspace_bytes < fc::carved_bytes(fc::echo_bwd_ws, pl))
        return FC_ERR_WORKSPACE;
    fc::Carver sv(saved), ws(workspace);
    const fc::EchoSaved s = fc::echo_saved(sv, pl);
    const fc::EchoBwdWs w = fc::echo_bwd_ws(ws, pl);
    const int N = mesh->N;
    int rc = fc_echo_backward(s.act, ln_s, wxp_s, mesh->by_source, s.hist, g_desc, w.g_act, w.gh, N, mesh->E, p->n_des, p->n_bins, stream);
    if (rc != FC_OK) return rc;
    rc = fc_tangent_nonlin_backward_partial(s.pre, p->bias, w.g_act, w.g_pre, w.part, w.part_bytes, N, p->n_des, stream);
    if (rc != FC_OK) return rc;
    fc_filter_params f = p->conv;
    f.bias_partials = w.part;
    f.bias_nparts = fc_tangent_nonlin_backward_groups(N);
    f.g_bias = p->g_bias;
    return fc_backward_all(x, w.g_pre, mesh->bwd, mesh->by_source, pl.records, s.wpk_b, gx, nullptr, &f, w.conv, w.conv_bytes, &pl.d, stream);
}

}  // extern "C"

// ---- LiftBlock --------------------------------------------------------------------------------------------------------------
namespace fc {

static bool lift_valid(const fc_mesh* m, const fc_lift_block_params* p) {
    return m && m->N > 0 && m->E >= 0 && m->R > 0 && m->by_target && m->by_source && p && p->C_in > 0 && p->C_out > 0;
}

struct LiftSaved { float *pre, *ang, *mag, *s1sum; };
static LiftSaved lift_saved(Carver& c, const fc_mesh* m, const fc_lift_block_params* p) {
    const size_t N = (size_t)m->N;
    return {c.take<float>(N * p->C_out * 8), c.take<float>(N * p->C_in * m->R * 8), c.take<float>(N * p->C_in * m->R * 4),
            c.take<float>(N * m->R * 8)};
}

struct LiftBwdWs { float* g_pre; void *nl, *tf; size_t nl_bytes, tf_bytes; };
static LiftBwdWs lift_bwd_ws(Carver& c, const fc_mesh* m, const fc_lift_block_params* p) {
    LiftBwdWs w;
    w.g_pre = c.take<float>((size_t)m->N * p->C_out * 8);
    w.nl = c.take(fc_tangent_nonlin_backward_workspace_bytes(m->N, p->C_out), &w.nl_bytes);
    w.tf = c.take(fc_trans_field_backward_workspace_bytes(m->N, p->C_in, p->C_out, m->R), &w.tf_bytes);
    return w;
}

}  // namespace fc

extern "C" {

size_t fc_lift_block_saved_bytes(const fc_mesh* mesh, const fc_lift_block_params* p) {
    return fc::lift_valid(mesh, p) ? fc::carved_bytes(fc::lift_saved, mesh, p) : 0;
}

size_t fc_lift_block_workspace_bytes(const fc_mesh* mesh, const fc_lift_block_params* p, int32_t backward) {
    return fc::lift_valid(mesh, p) && backward ? fc::carved_bytes(fc::lift_bwd_ws, mesh, p) : 0;
}

int fc_lift_block_forward(const float* x, const float* lift_sten, int32_t sten_stride, const fc_mesh* mesh, const int64_t* slot_to_edge_t,
                          const fc_lift_block_params* p, float* out, void* saved, size_t saved_bytes, void* stream) {
    if (!x || !out || !fc::lift_valid(mesh, p) || !p->zonal_ang || !p->zonal_mag || !p->phase || !p->bias) return FC_ERR_BAD_ARGUMENT;
    if (!saved || saved_bytes < fc::carved_bytes(fc::lift_saved, mesh, p)) return FC_ERR_WORKSPACE;
    fc::Carver sv(saved);
    const fc::LiftSaved s = fc::lift_saved(sv, mesh, p);
    int rc = fc_trans_field_forward(x, lift_sten, mesh->by_target, slot_to_edge_t, p->zonal_ang, p->zonal_mag, p->phase, s.pre, s.ang, s.mag,
                                    s.s1sum, mesh->N, mesh->E, p->C_in, p->C_out, mesh->R, sten_stride, stream);
    if (rc != FC_OK) return rc;
    return fc_tangent_nonlin_forward(s.pre, p->bias, out, mesh->N, p->C_out, stream);
}

int fc_lift_block_backward(const float* g_out, const float* lift_sten, int32_t sten_stride, const fc_mesh* mesh, const int64_t* slot_to_edge_s,
                           const fc_lift_block_params* p, const void* saved, size_t saved_bytes, float* gx, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!g_out || !gx || !fc::lift_valid(mesh, p) || !p->zonal_ang || !p->zonal_mag || !p->phase || !p->bias || !p->g_zonal_ang ||
        !p->g_zonal_mag || !p->g_bias || (p->ftype != 0 && !p->g_phase))
        return FC_ERR_BAD_ARGUMENT;
    if (!saved || saved_bytes < fc::carved_bytes(fc::lift_saved, mesh, p) || !workspace || workspace_bytes < fc::carved_bytes(fc::lift_bwd_ws, mesh, p))
        return FC_ERR_WORKSPACE;
    fc::Carver sv(saved), ws(workspace);
    const fc::LiftSaved s = fc::lift_saved(sv, mesh, p);
    const fc::LiftBwdWs w = fc::lift_bwd_ws(ws, mesh, p);
    int rc = fc_tangent_nonlin_backward(s.pre, p->bias, g_out, w.g_pre, p->g_bias, w.nl, w.nl_bytes, mesh->N, p->C_out, stream);
    if (rc != FC_OK) return rc;
    return fc_trans_field_backward(lift_sten, mesh->by_source, slot_to_edge_s, p->zonal_ang, p->zonal_mag, p->phase, s.ang, s.mag, s.s1sum,
                                   w.g_pre, gx, p->g_zonal_ang, p->g_zonal_mag, p->ftype != 0 ? p->g_phase : nullptr, w.tf, w.tf_bytes,
                                   mesh->N, mesh->E, p->C_in, p->C_out, mesh->R, sten_stride, p->ftype, stream);
}

}  // extern "C"
