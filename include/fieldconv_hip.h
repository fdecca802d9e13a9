/* fieldconv_hip.h -- C ABI of libfieldconv_hip.so (gfx950 / MI355X).
 *
 * The reference (twmitchel/FieldConv) has no native interface for this path: its hot loop is a
 * composite of stock torch ops plus torch_scatter.scatter_add inside Python modules.  Each entry
 * point below replaces the body of one reference Python method; a maintainer binds it with
 * ctypes / a torch custom op exactly as fieldconv_amd/_lib.py does.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch); nothing is allocated,
 *     freed or retained by the library; workspaces are caller-provided
 *   - complex tensors are interleaved (re, im) fp32 pairs == torch.complex64 storage
 *   - indices are int32; `stream` is a hipStream_t passed as void*
 *   - return value: 0 on success, a negative fc_status otherwise; no exceptions, no globals,
 *     re-entrant; work is enqueued on `stream` and NOT synchronised
 */
#ifndef FIELDCONV_HIP_H
#define FIELDCONV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fc_status {
    FC_OK = 0,
    FC_ERR_BAD_ARGUMENT = -1,   /* null pointer, non-positive size, inconsistent dims */
    FC_ERR_UNSUPPORTED = -2,    /* (n_rings, band_limit, channels) outside the compiled set */
    FC_ERR_LAUNCH = -3,         /* hipLaunchKernel reported an error */
    FC_ERR_WORKSPACE = -4       /* workspace pointer missing or too small */
} fc_status;

/* Problem dimensions of one FieldConv call (reference nn/field_conv.py:104-123). */
typedef struct fc_dims {
    int32_t N;   /* vertices                                   */
    int32_t E;   /* support edges                              */
    int32_t I;   /* in_channels                                */
    int32_t O;   /* out_channels                               */
    int32_t R;   /* n_rings                                    */
    int32_t B;   /* band_limit; F = 2B+1 angular frequencies   */
    int32_t mode; /* fc_mfma_mode: arithmetic of the contractions (0 = FC_MFMA_SPLIT_F16, the default) -- see below.  Part of the dims
                   * of EVERY call: size queries, packing calls and launches of one convolution carry the same value; two convolutions
                   * in one process may differ (the library keeps no arithmetic state) */
} fc_dims;

/* Edge list grouped by one endpoint (CSR).  Slot s in [rowptr[v], rowptr[v+1]) is one edge
 * incident to vertex v; nbr[s] is the OTHER endpoint.  Grouped by target (col 1 of supp_edges)
 * for the forward pass, by source (col 0) for the backward pass.  The stencil passed alongside a
 * CSR is stored in that CSR's SLOT order (the kernels stream it): see fc_forward / fc_backward. */
typedef struct fc_csr {
    const int32_t* rowptr;   /* N+1 */
    const int32_t* nbr;      /* E   (dense entry points; may be NULL for the factored ones) */
    const int32_t* runs;     /* factored entry points only, else NULL: N x 8 ints; runs[8v + q] = first slot of
                              * vertex v, relative to rowptr[v], whose ring index is >= q (so the slots of ring q
                              * are [runs[8v+q], runs[8v+q+1]) and runs[8v] = 0) */
} fc_csr;

int fc_abi_version(void);
/* Arithmetic of the three contractions (forward, input gradient, filter gradient), carried PER CALL in fc_dims::mode / fc_mesh::mode --
 * no process-wide setter, no environment variable: FC_MFMA_SPLIT_F16 (default) carries every operand as two f16 halves with
 * power-of-two row scales on v_mfma_f32_16x16x32_f16, fp32 accumulation (fp32-grade: 2^-22 of the row maximum); FC_MFMA_F32 runs
 * v_mfma_f32_16x16x4_f32 on fp32 operands throughout; FC_MFMA_F16 drops the low halves (reduced precision, ~3e-4).  Packed filter
 * images, workspaces and kernels all follow the mode: a packing call and the launches that use its images carry the same one. */
typedef enum fc_mfma_mode { FC_MFMA_SPLIT_F16 = 0, FC_MFMA_F32 = 1, FC_MFMA_F16 = 2 } fc_mfma_mode;
/* 1 when this library was compiled with -DFC_DEV_SWITCHES (libfieldconv_hip_dev.so: the FC_* development variables of
 * fieldconv_amd/_env.py select older kernel families, skip phases, write stamps); the product library returns 0 and reads no variable. */
int fc_dev_switches(void);
/* Development only (tools/stamps.py): a device buffer of 16 x 256 uint64 that the record-driven kernels fill with in-kernel
 * time stamps of workgroup 0 (label << 56 | s_memtime), or NULL to switch the stamps off (the default).  Process-wide. */
void fc_debug_stamp_buffer(void* device_buffer);
const char* fc_status_string(int status);

/* 1 if the compiled kernels cover these dims, 0 otherwise (then every call returns FC_ERR_UNSUPPORTED for them):
 * (n_rings, band_limit) among the compiled shapes, at most 64 channels, and slab + partial sums + record ring within
 * the CU's 160 KB of LDS in the current MFMA mode (8 rings with more than 56 channels are not, in the default mode).
 * The operator is linear in the input channels and independent across output channels: wider layers run as channel blocks
 * (fc_forward_wide / fc_backward_wide below). */
int fc_supported(const fc_dims* dims);
/* Which kernels a forward + backward pass with these dims launches in this process, as one line of text (kernel family,
 * record kind, MFMA mode, tile counts): the library picks them from the dims, the device's CU count, the MFMA mode and -- in the
 * development build only -- its switches, and a benchmark line should say what it timed.  kind: 0 dense rows, 1 factored
 * records, 2 geometric records in the forward pass (factored ones in the backward pass).  No GPU work.
 * The forward part ends with what the launch is, given its workspace: grid=G (workgroups) whole=W half=H (work items: 16-vertex tiles
 * and 8-vertex half tiles; with the edge split a tile counts once per part) spread=0|1 (ring-major: one item per workgroup, whole and
 * half tiles dealt so that every CU holds at most a whole and a half tile) lds=BYTES (dynamic LDS of a workgroup) cus=C (the CU count
 * the choices were made for; 256 without a device), and for the frequency-major kernels slabs=S (slab buffers in LDS, 1 or 2). */
int fc_describe_kernels(const fc_dims* dims, int32_t kind, char* buffer, size_t buffer_bytes);

/* ---- filter packing -------------------------------------------------------------------- *
 * W_eff (O,I,R,F) complex64 is what reference nn/field_conv.py:10-33 (weightContrib*) builds
 * from (zonal, spherical, phase); the 1/(2B+1) of :14,:25,:33 is folded in here.
 * The packed images are opaque to the caller: allocate fc_packed_filter_floats_{fwd,bwd}() floats
 * each and hand them to the convolution calls.  Default ("split") layout, one image per contraction:
 *   OP inverse row scales (floats), then F x {re_hi, re_lo, im_hi, im_lo} x KP/32 k blocks x OP x 32 halves,
 *   forward rows o, k = r*ceil8(I) + i;  backward rows i, k = r*ceil8(O) + o, conjugated;
 *   OP = ceil16(rows), KP = ceil32(R * ceil8(channels)).
 * In FC_MFMA_F32 mode (fc_dims::mode): F x {re,im} x OP x ceil16(R*channels) floats.
 * `records`: which family of convolution entry points the images are for -- 0: the dense-stencil ones (fc_forward,
 * fc_backward_data), 1: the record-driven ones (fc_forward_factored, fc_forward_geometric, fc_backward_data_factored).
 * In the default mode the record-driven forward image is RING-major: OP inverse row scales, then
 * R x {re_hi, re_lo, im_hi, im_lo} x KP/32 k blocks x OP x 32 halves with k = f*ceil8(I) + i, KP = ceil32(F * ceil8(I))
 * (csrc/fc_forward_ring.hpp) whenever the forward launch with these dims takes the ring-major kernel (meshes of more than
 * 256 tiles of 16 vertices): the layout follows dims->N, so an image is packed with the dims of the launch it is for
 * (a forward pass launched in two row ranges packs one image per range).  Sizes differ between the two families, ask with
 * the same `records`.  wpk_bwd may be NULL: only the forward image is written. */
/* `records` for every call below that takes one: 0 for the dense-stencil entry points, 1 for the record-driven ones
 * (fc_records_flags(dims, record_driven) returns exactly that; kept so that a binding never hard-codes the value).
 * Either image pointer of the packing calls may be NULL (not both): only the other image is written. */
int32_t fc_records_flags(const fc_dims* dims, int32_t record_driven);
size_t fc_packed_filter_floats_fwd(const fc_dims* dims, int32_t records);
size_t fc_packed_filter_floats_bwd(const fc_dims* dims, int32_t records);
int fc_pack_filter(const float* w_eff, float* wpk_fwd, float* wpk_bwd, const fc_dims* dims, int32_t records, void* stream);
/* Same, assembling W_eff on the fly from the module parameters exactly as reference
 * nn/field_conv.py:10-33 does (zonal (O,I,R[,2]), spherical (O,I,R,B|2B,2), phase (O,I,B+1), all fp32
 * contiguous; ftype 0/1/2 as in :53-59; phase is read for ftype 1 only). */
int fc_pack_filter_params(const float* zonal, const float* spherical, const float* phase, int32_t ftype,
                          float* wpk_fwd, float* wpk_bwd, const fc_dims* dims, int32_t records, void* stream);
/* Autograd twin of the assembly: dL/dW_eff (O,I,R,F) c64 -> gradients shaped like the parameters
 * (overwritten; g_phase written for ftype 1 only). */
int fc_filter_param_grads(const float* gw_eff, const float* zonal, const float* spherical, const float* phase,
                          int32_t ftype, float* g_zonal, float* g_spherical, float* g_phase,
                          const fc_dims* dims, void* stream);

/* Optional epilogue of the forward convolutions (reference nn/fc_resnet_block.py:84-88): what follows a
 * FieldConv inside an FCResNetBlock / ECHOBlock is applied to the output tile before it leaves the kernel.
 *   addend        (N,O) c64 or NULL   added to the convolution's output (the block's TangentLin residual)
 *   modrelu_bias  O floats or NULL    TangentNonLin (reference nn/tangent_nonlin.py:24-35) of (conv + addend)
 *   activated     (N,O) c64           receives the activated values; required with modrelu_bias
 * `y` always receives conv + addend (the pre-activation: the backward pass of the modReLU needs it).  NULL epilogue = none. */
typedef struct fc_epilogue {
    const float* addend;
    const float* modrelu_bias;
    float* activated;
} fc_epilogue;

/* ---- FieldConv.forward, reference nn/field_conv.py:128-137 ------------------------------- *
 * y[n,o] = 1/F sum_{e: dst_e=n} sum_{i,r,f} x[src_e,i] e^{-i(f-B)phi[src_e,i]} S[e,r,f] W_eff[o,i,r,f]
 * x (N,I) c64; by_target: CSR grouped by target; sten_t (E,R,F) c64 = supp_sten rows permuted into
 * by_target slot order; y (N,O) c64 (overwritten). */
int fc_forward(const float* x, const float* sten_t, const fc_csr* by_target, const float* wpk_fwd,
               float* y, const fc_dims* dims, const fc_epilogue* epilogue, void* stream);

/* ---- factored stencil fast path ---------------------------------------------------------- *
 * FCPrecomp's stencil (reference transforms/fc_precomp.py:24-25,95) is rank-1 and 2-sparse in the
 * ring index: supp_sten[e,r,f] = w[e,r] * ph[e,f] with w[e,q], w[e,q+1] the only non-zeros.  When
 * the caller has verified that structure it may pass, instead of the dense rows, one record of
 * fc_factored_record_floats(B) floats per edge (in by_target slot order and, inside every target's
 * slot range, sorted by q; followed by at least 1 KiB of readable padding):  [0] q as int32 bits, [1] w[q], [2] w[q+1],
 * [3] the slot's other endpoint (= by_target->nbr[slot]) as int32 bits, [4+2f], [5+2f] = Re, Im ph[f].  Same result as fc_forward up to fp32 rounding.
 * workspace (optional, may be NULL / 0): fc_forward_workspace_bytes(dims) bytes of scratch.  On meshes whose N/16 vertex
 * tiles cannot occupy the 256 CUs (the reference's segmentation meshes: ~1k vertices with ~128 neighbours) it lets up
 * to 8 workgroups share a tile, each taking a share of every target's edges; their partial outputs are added in a
 * fixed order.  fc_forward_workspace_bytes returns 0 when the split does not apply. */
int fc_factored_record_floats(int32_t band_limit);
size_t fc_forward_workspace_bytes(const fc_dims* dims);
int fc_forward_factored(const float* x, const float* rec_t, const fc_csr* by_target, const float* wpk_fwd,
                        float* y, void* workspace, size_t workspace_bytes, const fc_dims* dims, const fc_epilogue* epilogue,
                        void* stream);

/* ---- geometric-phase records (forward only) ---------------------------------------------- *
 * FCPrecomp's phases are geometric in the frequency: ph[e,f] = c[e] * g[e]^(f-B) with |g| = 1
 * (fSten = exp(i m theta) times the per-edge weight, reference transforms/fc_precomp.py:88-95).  When the
 * caller has verified that as well, the forward pass takes records of fc_geometric_record_floats() = 8
 * floats per edge, same order and padding as above:  [0] q bits, [1] w[q], [2] w[q+1], [3] other endpoint
 * bits, [4],[5] = Re, Im c, [6],[7] = Re, Im g.  Same result as fc_forward up to fp32 rounding. */
int fc_geometric_record_floats(void);
int fc_forward_geometric(const float* x, const float* geo_t, const fc_csr* by_target, const float* wpk_fwd,
                         float* y, void* workspace, size_t workspace_bytes, const fc_dims* dims, const fc_epilogue* epilogue,
                         void* stream);

/* ---- autograd of the above (the reference relies on torch autograd through :128-137) ----- *
 * Three calls on the same stream, sharing `workspace` (fc_backward_workspace_bytes(dims) bytes,
 * 256-byte aligned, untouched in between):
 *   fc_backward_data[_factored]  one kernel: source-centric gather of H = sum gy conj(S) over the
 *                                out-edges (by_source: CSR grouped by source; sten_s / rec_s in its
 *                                slot order, records sorted by ring inside a source and carrying the
 *                                target in [3]), MFMA contraction with the conjugated filter, writes
 *                                gx (N,I) c64 and leaves H in the workspace
 *   fc_backward_filter           one kernel: filter-gradient partials from the stored H and x
 *   fc_backward_finish           fixed-order sum of the partials into gw_eff (O,I,R,F) c64 */
size_t fc_backward_workspace_bytes(const fc_dims* dims, int32_t records);
int fc_backward_data(const float* x, const float* gy, const float* sten_s, const fc_csr* by_source,
                     const float* wpk_bwd, float* gx, void* workspace, size_t workspace_bytes,
                     const fc_dims* dims, void* stream);
int fc_backward_data_factored(const float* x, const float* gy, const float* rec_s, const fc_csr* by_source,
                              const float* wpk_bwd, float* gx, void* workspace, size_t workspace_bytes,
                              const fc_dims* dims, int32_t records, void* stream);
int fc_backward_filter(const float* x, void* workspace, size_t workspace_bytes, const fc_dims* dims, int32_t records, void* stream);
/* Large meshes on records in the default arithmetic mode (fc_backward_streams(dims, records) != 0) run the H-STREAMING arrangement
 * behind the same three calls: fc_backward_data_factored = a gather kernel (H of every source vertex to the workspace, nothing else) +
 * ONE kernel that streams H once for both products (gxt = H conj(W), gW = H^T conj(xt)) + a small kernel that forms gx; gx is complete
 * and the filter-gradient partials are in the workspace when its work is done, and fc_backward_filter has nothing left to launch.
 * fc_backward_gather / fc_backward_stream are the two halves of that fc_backward_data_factored call as entry points of their own
 * (per-kernel timing; FC_ERR_UNSUPPORTED where the arrangement does not apply).  The gather launch also leaves, in the workspace, a
 * copy of the packed filter in the order the streaming launch's wavefronts load their fragments: fc_backward_stream reads what the
 * fc_backward_gather call before it wrote for the same wpk_bwd.  Autograd of reference nn/field_conv.py:21,130,134. */
int32_t fc_backward_streams(const fc_dims* dims, int32_t records);
int fc_backward_gather(const float* gy, const float* rec_s, const fc_csr* by_source, const float* wpk_bwd, void* workspace,
                       size_t workspace_bytes, const fc_dims* dims, void* stream);
int fc_backward_stream(const float* x, const float* wpk_bwd, float* gx, void* workspace, size_t workspace_bytes, const fc_dims* dims,
                       void* stream);
int fc_backward_finish(float* gw_eff, void* workspace, size_t workspace_bytes, const fc_dims* dims, int32_t records, void* stream);

/* ---- one call per pass: the same kernels, enqueued by one entry point (a binding that pays microseconds per foreign call --
 * ctypes -- spends more time on six calls per convolution than the GPU needs for a small mesh) ---------------------------- *
 * fc_filter_params: the module parameters as fc_pack_filter_params takes them and, for the backward pass, where their
 * gradients go (g_* are ignored by fc_forward_params; g_phase / phase may be NULL unless ftype == 1).
 * fc_forward_params = fc_pack_filter_params (wpk_bwd may be NULL; `records` as above) + fc_forward (kind 0) / fc_forward_factored (1) /
 *                     fc_forward_geometric (2), same arguments;
 * fc_backward_all   = fc_backward_data (records 0) or fc_backward_data_factored (1) + fc_backward_filter +
 *                     fc_backward_finish into gw_eff + fc_filter_param_grads when params is not NULL (then the pass
 *                     ends in fc_backward_finish_params' single launch, which also adds the data kernel's partial gx arrays when
 *                     tiles were shared: gx is complete when the call's work is, not between its kernels).  gw_eff is required
 *                     without params and OPTIONAL with them: NULL = only the parameter gradients are wanted (a module's backward
 *                     pass; the (O,I,R,F) tensor is then never written). */
typedef struct fc_filter_params {
    const float* zonal;
    const float* spherical;
    const float* phase;
    int32_t ftype;
    float* g_zonal;
    float* g_spherical;
    float* g_phase;
    /* optional rider of the launch that finishes the backward pass (fc_backward_finish_params / fc_backward_all): the fixed-order sum of
     * the modReLU's bias-gradient partials -- bias_partials (bias_nparts, O) floats as fc_tangent_nonlin_backward_partial left them --
     * into g_bias (O), instead of a launch of its own.  NULL / 0: nothing. */
    const float* bias_partials;
    int32_t bias_nparts;
    float* g_bias;
} fc_filter_params;
int fc_forward_params(const float* x, const float* sten_or_records, const fc_csr* by_target, int32_t kind,
                      const fc_filter_params* params, float* wpk_fwd, float* wpk_bwd, float* y, void* workspace,
                      size_t workspace_bytes, const fc_dims* dims, int32_t records, const fc_epilogue* epilogue, void* stream);
int fc_backward_all(const float* x, const float* gy, const float* sten_or_rec_s, const fc_csr* by_source, int32_t records,
                    const float* wpk_bwd, float* gx, float* gw_eff, const fc_filter_params* params, void* workspace,
                    size_t workspace_bytes, const fc_dims* dims, void* stream);
/* fc_backward_finish + fc_filter_param_grads in ONE launch: every workgroup sums the partials of its
 * (output channel, 16 input channels) block in the fixed order, writes gw_eff (unless NULL) and pulls the block back to the parameters.
 * The partials are summed in four consecutive groups whose sums are then added in order: deterministic, but rounded
 * differently from fc_backward_finish's single chain.  fc_backward_all uses it when it is given params. */
int fc_backward_finish_params(float* gw_eff, void* workspace, size_t workspace_bytes, const fc_dims* dims, int32_t records,
                              const fc_filter_params* params, void* stream);

/* ---- layers wider than 64 channels, natively (reference nn/field_conv.py:62 takes any width) ----------------------------------- *
 * The kernels above take at most 64 input and 64 output channels (one channel per lane in their gather phases).  The operator is
 * linear in the input channels and independent across output channels, so a wider layer is nob x nib launches of the same
 * kernels on channel blocks of `block` channels (a multiple of 8, <= 64, with fc_supported(block x block) true); these two entry
 * points enqueue a whole pass from one call -- strided 2-D copies cut x / gy into contiguous blocks, the filter images are packed
 * straight from the (o0, i0) block of the full parameter tensors (or of an explicit W_eff), the sum over input blocks rides in the
 * convolution's residual epilogue, the input gradient's sum over output blocks is a fixed-order sum of partials, and a block's
 * parameter gradients land in their block of the full gradient tensors (params->g_*), or in gw_eff (O,I,R,F) for an explicit filter.
 * Exactly one of `params` / `w_eff` is given.  dims carries the FULL widths I, O; y (N,O), gx (N,I) complex64, overwritten.
 * workspace: fc_wide_workspace_bytes(dims, block, records, backward) bytes. */
size_t fc_wide_workspace_bytes(const fc_dims* dims, int32_t block, int32_t records, int32_t backward);
int fc_forward_wide(const float* x, const float* sten_or_records, const fc_csr* by_target, int32_t kind, const fc_filter_params* params,
                    const float* w_eff, float* y, void* workspace, size_t workspace_bytes, const fc_dims* dims, int32_t records,
                    int32_t block, void* stream);
int fc_backward_wide(const float* x, const float* gy, const float* sten_or_rec_s, const fc_csr* by_source, int32_t records,
                     const fc_filter_params* params, const float* w_eff, float* gw_eff, float* gx, void* workspace,
                     size_t workspace_bytes, const fc_dims* dims, int32_t block, void* stream);

/* ---- any (n_rings, band_limit): the run-time path for shapes outside the compiled set (reference nn/field_conv.py:62-98
 * takes any) ---- *
 * fc_shape_compiled: 1 for n_rings 2..8 x band_limit 1..3 (the specialised kernels above), else 0.  For the others -- and for
 * complex128 features of ANY shape (the reference's modules run under .double()) -- the operator is evaluated in the reference's
 * own two steps, with dense stencil rows in slot order, in the tensors' own precision (dtype):
 *   fc_generic_gather   contrib (n_targets, I, R, F) c64 = the per-target response of :128-134 (by_target CSR with nbr; sten_t
 *                       (E,R,F) complex in its slot order); the caller contracts it with W_eff and forms the two backward
 *                       products with fc_cgemm (below);
 *   fc_generic_scatter  gx (N, I) c64 from g_contrib (n_targets, I, R, F) over the out-edges (by_source CSR with nbr = targets,
 *                       sten_s in its slot order), including the chain rule through the rotation e^{-i m angle(x)}.
 * Any channel count: a workgroup takes as many input channels as its R * F accumulators per channel fit in the CU's 160 KB of LDS. */
typedef enum fc_dtype { FC_F32 = 0, FC_F64 = 1 } fc_dtype;       /* real scalar type of a complex tensor: complex64 / complex128 */
int fc_shape_compiled(int32_t n_rings, int32_t band_limit);
int fc_generic_gather(const void* x, const void* sten_t, const fc_csr* by_target, void* contrib, int32_t n_targets, int32_t I,
                      int32_t R, int32_t B, int32_t dtype, void* stream);
int fc_generic_scatter(const void* x, const void* g_contrib, const void* sten_s, const fc_csr* by_source, void* gx, int32_t N,
                       int32_t I, int32_t R, int32_t B, int32_t dtype, void* stream);
/* The contractions of the run-time path (and TangentLin in double precision): a complex GEMM on the matrix pipe,
 *   C[m, n] = alpha * sum_k A[m*sam + k*sak] * op(B[k*sbk + n*sbn]),   op = conj when conj_b != 0,
 * C (M, N) row-major and contiguous, A and B complex arrays addressed with element strides (in complex numbers), all three of
 * dtype FC_F32 (interleaved float pairs) or FC_F64 (double pairs).  With contrib viewed as (n, K = I*R*F) and W_eff as (O, K):
 *   y         = contrib . W_eff^T / F         fc_cgemm(contrib, W, y,  n, O, K,  K, 1,  1, K,  0, 1/F, ...)
 *   g_contrib = gy . conj(W_eff) / F          fc_cgemm(gy, W, gc,      n, K, O,  O, 1,  K, 1,  1, 1/F, ...)
 *   gW_eff    = gy^T . conj(contrib) / F      fc_cgemm(gy, contrib, gW, O, K, n,  1, O,  K, 1,  1, 1/F, ...)            */
/* workspace (optional): fc_cgemm_workspace_bytes(M, N, K, dtype) bytes -- non-zero for products with a small output and a long
 * contraction (the two weight-gradient products: K = the vertex count), which are then split along k over many workgroups with per-slice
 * partials summed in slice order; NULL / 0: one workgroup per 64 x 64 output tile walks all of K. */
size_t fc_cgemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t dtype);
int fc_cgemm(const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t sam, int64_t sak, int64_t sbk, int64_t sbn,
             int32_t conj_b, double alpha, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- TangentLin.forward, reference nn/tangent_lin.py:27-29 ------------------------------- *
 * y[n,o] = sum_i x[n,i] (Re + i Im)[o,i];  re_w, im_w are (O,I) fp32 row-major. */
int fc_tangent_lin_forward(const float* x, const float* re_w, const float* im_w, float* y,
                           int32_t N, int32_t I, int32_t O, void* stream);
/* gx (N,I) c64, g_re / g_im (O,I) fp32 (all overwritten); I, O <= 64.
 * workspace: fc_tangent_lin_backward_workspace_bytes() bytes of per-wavefront partial sums. */
size_t fc_tangent_lin_backward_workspace_bytes(int32_t N, int32_t I, int32_t O);
int fc_tangent_lin_backward(const float* x, const float* gy, const float* re_w, const float* im_w,
                            float* gx, float* g_re, float* g_im, void* workspace, size_t workspace_bytes,
                            int32_t N, int32_t I, int32_t O, void* stream);
/* Which kernel one launch of the (N, K, M) product takes in this process, as one line of text (fc_describe_kernels' idiom; no GPU
 * work, and without a device the CU count counts as 256).  The forward pass is the launch K = I, M = O, transposed = 0; the input
 * gradient K = O, M = I, transposed = 1.  aligned: 1 when the input rows (x, or gy when transposed) start on a 16-byte boundary and,
 * in the forward launch, re_w and im_w on 8-byte ones with an even row length; with 0 the staged kernel loads its rows element by
 * element.  The line reads
 *     direct grid=G blocks=B trips=T cus=C
 *     staged split=0|1 loads=vector|scalar tiles=MT kchunks=KC lds=BYTES grid=G blocks=B trips=T cus=C
 * (blocks: 16-vertex blocks; trips: the most blocks one wavefront walks; tiles: 16-channel output tiles; kchunks: sets of input
 * fragments a wavefront loads per block).  FC_ERR_BAD_ARGUMENT for sizes the launchers refuse, -2 when the buffer is too small. */
int fc_tangent_lin_describe(int32_t N, int32_t K, int32_t M, int32_t transposed, int32_t aligned, char* buffer, size_t buffer_bytes);

/* ---- TangentNonLin.forward (modReLU), reference nn/tangent_nonlin.py:24-35 --------------- *
 * y = relu(|x| + b_c) x/|x| outside the origin box, x inside it.  bias: C floats. */
int fc_tangent_nonlin_forward(const float* x, const float* bias, float* y, int32_t N, int32_t C, void* stream);
/* gx (N,C) c64 overwritten; gbias (C floats) overwritten.
 * workspace: fc_tangent_nonlin_backward_workspace_bytes() bytes of per-block bias partials. */
size_t fc_tangent_nonlin_backward_workspace_bytes(int32_t N, int32_t C);
int fc_tangent_nonlin_backward(const float* x, const float* bias, const float* gy, float* gx, float* gbias,
                               void* workspace, size_t workspace_bytes, int32_t N, int32_t C, void* stream);
/* The same VJP without the second launch: gx as above, the per-group partial sums of the bias gradient left in `workspace` as
 * (fc_tangent_nonlin_backward_groups(N), C) floats for fc_filter_params::bias_partials (a modReLU fused behind a convolution: its
 * backward pass ends in that convolution's finish launch anyway). */
int32_t fc_tangent_nonlin_backward_groups(int32_t N);
int fc_tangent_nonlin_backward_partial(const float* x, const float* bias, const float* gy, float* gx, void* workspace,
                                       size_t workspace_bytes, int32_t N, int32_t C, void* stream);

/* softAbs, reference utils/field.py:29-37 (what ECHOBlock feeds its linear residual, nn/echo_block.py:103): y = |x| outside the origin
 * box, 0 inside; its VJP gx = gy x/|x| (0 inside).  x: count complex64 values, y / gy: count floats. */
int fc_soft_abs_forward(const float* x, float* y, size_t count, void* stream);
int fc_soft_abs_backward(const float* x, const float* gy, float* gx, size_t count, void* stream);

/* The same in double precision (complex128 features, float64 bias): the reference's modules run under .double().
 * TangentLin in double precision is fc_cgemm with Wc = Re + i Im built by the caller. */
int fc_tangent_nonlin_forward_f64(const double* x, const double* bias, double* y, int32_t N, int32_t C, void* stream);
size_t fc_tangent_nonlin_backward_workspace_bytes_f64(int32_t N, int32_t C);
int fc_tangent_nonlin_backward_f64(const double* x, const double* bias, const double* gy, double* gx, double* gbias,
                                   void* workspace, size_t workspace_bytes, int32_t N, int32_t C, void* stream);

/* ---- ECHO descriptors, reference nn/echo.py:94-148 (ECHO.forward with rasterize :30-61, diskMap :11-27) ---- *
 * hist[n,c,b] = sum over in-edges e of n of the bilinear votes of the point ln[e] * exp(-i angle(x[src_e,c])) in the
 * rasterised disk of (2*n_bins+1)^2 cells, each vote carrying x[src_e,c] * wxp[e]; zero features do not vote; the
 * descriptor is |hist| (zero-safe).  x (N,C) c64, any C; ln_t / wxp_t (E) c64 in by_target slot order; hist
 * (N,C,dS) c64 and desc (N,C,dS) f32 are overwritten, dS = fc_echo_hist_dim(n_bins), 1 <= n_bins <= 8.  The channels are
 * independent: a call launches ceil(C / fc_echo_channel_block(n_bins)) channel blocks (64 up to n_bins = 4, then 57, 42, 30, 23: one
 * channel per lane, the histograms of a workgroup in LDS).  Any n_bins, and double precision: fc_echo_forward_generic below.
 * Backward: by_source groups the edges by source (nbr = targets), ln_s / wxp_s in that slot order; g_desc (N,C,dS) f32;
 * gx (N,C) c64 is overwritten; hist_grad_workspace: N*C*dS complex64 values of scratch. */
int fc_echo_hist_dim(int32_t n_bins);
int fc_echo_channel_block(int32_t n_bins);
int fc_echo_forward(const float* x, const float* ln_t, const float* wxp_t, const fc_csr* by_target, float* hist,
                    float* desc, int32_t N, int32_t E, int32_t C, int32_t n_bins, void* stream);
int fc_echo_backward(const float* x, const float* ln_s, const float* wxp_s, const fc_csr* by_source, const float* hist,
                     const float* g_desc, float* gx, float* hist_grad_workspace, int32_t N, int32_t E, int32_t C,
                     int32_t n_bins, void* stream);

/* ---- TransField (the learned 'gradient' of LiftBlock), reference nn/trans_field.py:78-113, weightContrib* :9-24 ---- *
 * x (N,Cin) f32 scalar features, Cin <= 4; lift_sten: the stencil columns m = 0, 1 (reference segmentation.ipynb:204)
 * in ORIGINAL edge order, element (e,r,j) at complex index (e*R + r)*sten_stride + j -- sten_stride = 2 for a packed
 * (E,R,2) array, 2B+1 for a pointer to column m = 0 of the full (E,R,2B+1) stencil, 0 when lift_sten is the (E,8) factor table of
 * fc_precomp_graph (the two columns are then formed on the fly: w_r c and w_r c e^{i theta}; no (E,R,2) array exists); by_target / by_source: the edges grouped by target / source with
 * slot_to_edge (E) int64 giving the original edge of every slot; zonal_ang, zonal_mag (O,Cin,R) f32, phase (O,Cin) f32
 * (zeros for ftype 0); y (N,O) c64, O <= 64.  The forward call also leaves ang (N,Cin,R) c64, mag (N,Cin,R) f32 and
 * s1sum (N,R) c64 for the backward call, which overwrites gx (N,Cin) f32 and the parameter gradients (g_phase for
 * ftype != 0 only) using a caller-provided workspace. */
int fc_trans_field_forward(const float* x, const float* lift_sten, const fc_csr* by_target, const int64_t* slot_to_edge,
                           const float* zonal_ang, const float* zonal_mag, const float* phase, float* y, float* ang,
                           float* mag, float* s1sum, int32_t N, int32_t E, int32_t Cin, int32_t O, int32_t R, int32_t sten_stride,
                           void* stream);
size_t fc_trans_field_backward_workspace_bytes(int32_t N, int32_t Cin, int32_t O, int32_t R);
int fc_trans_field_backward(const float* lift_sten, const fc_csr* by_source, const int64_t* slot_to_edge_s,
                            const float* zonal_ang, const float* zonal_mag, const float* phase, const float* ang,
                            const float* mag, const float* s1sum, const float* gy, float* gx, float* g_zonal_ang,
                            float* g_zonal_mag, float* g_phase, void* workspace, size_t workspace_bytes, int32_t N,
                            int32_t E, int32_t Cin, int32_t O, int32_t R, int32_t sten_stride, int32_t ftype, void* stream);

/* ---- whole blocks from ONE call per pass ---------------------------------------------------------------- *
 * The reference's networks are built from three blocks -- FCResNetBlock (nn/fc_resnet_block.py:65-88), ECHOBlock
 * (nn/echo_block.py:73-103) and LiftBlock (nn/lift_block.py:35-55) -- and train with batch size 1 on a different ~1k-vertex mesh every
 * step (segmentation.ipynb:120,137): a binding that crosses into the library once per KERNEL spends more host time per block than the
 * GPU needs to run it.  The entry points below enqueue a whole block pass -- filter assembly, convolutions with their fused
 * residual / modReLU epilogues, the TangentLin residual, the descriptor splat, and in the backward pass the complete VJP chain with
 * every parameter gradient -- from one foreign call, with caller-owned buffers only:
 *   saved      what the backward pass needs from the forward pass (pre-activations, activations, backward filter images, ...):
 *              fc_*_saved_bytes() bytes, 256-byte aligned, written by *_forward, read by *_backward, untouched in between
 *   workspace  scratch of one call: fc_*_workspace_bytes(..., backward) bytes, 256-byte aligned
 * Same kernels and the same results, bit for bit, as the per-operator calls above in the order the reference applies them. */
typedef struct fc_mesh {           /* one mesh's support graph as the convolutions consume it */
    int32_t N, E, R, B;            /* vertices, support edges, n_rings, band_limit of the stencil */
    int32_t kind;                  /* 0 dense stencil rows, 1 factored records, 2 geometric forward records (factored backward) */
    const fc_csr* by_target;       /* as for fc_forward* (nbr also read by the ECHO / lift blocks) */
    const fc_csr* by_source;       /* as for fc_backward_data* */
    const float* fwd;              /* sten_t / rec_t / geo_t, by kind, in by_target slot order */
    const float* bwd;              /* sten_s (kind 0) or rec_s, in by_source slot order */
    int32_t mode;                  /* fc_mfma_mode of the block's convolutions (0: the default) */
} fc_mesh;

/* FCResNetBlock: out = modReLU_2(res(x) + conv2(modReLU_1(conv1(x)))), reference nn/fc_resnet_block.py:84-88.
 * conv1: (C_mid, C_in) filter, conv2: (C_out, C_mid); bias1 (C_mid), bias2 (C_out): the TangentNonLin biases; res_re / res_im
 * (C_out, C_in): the TangentLin residual.  The g_* members receive the gradients in the backward call (conv*.g_*, g_bias*, g_res_*);
 * the bias riders of conv1 / conv2 (fc_filter_params::bias_partials ...) are set by the library and ignored on entry. */
typedef struct fc_resnet_block_params {
    int32_t C_in, C_mid, C_out;
    fc_filter_params conv1, conv2;
    const float* bias1;
    const float* bias2;
    const float* res_re;
    const float* res_im;
    float* g_bias1;
    float* g_bias2;
    float* g_res_re;
    float* g_res_im;
} fc_resnet_block_params;
size_t fc_resnet_block_saved_bytes(const fc_mesh* mesh, const fc_resnet_block_params* p);
size_t fc_resnet_block_workspace_bytes(const fc_mesh* mesh, const fc_resnet_block_params* p, int32_t backward);
/* x (N,C_in) c64 -> out (N,C_out) c64 */
int fc_resnet_block_forward(const float* x, const fc_mesh* mesh, const fc_resnet_block_params* p, float* out, void* saved,
                            size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* g_out (N,C_out) c64 -> gx (N,C_in) c64 and every parameter gradient of the block */
int fc_resnet_block_backward(const float* x, const float* g_out, const fc_mesh* mesh, const fc_resnet_block_params* p, const void* saved,
                             size_t saved_bytes, float* gx, void* workspace, size_t workspace_bytes, void* stream);

/* The tangent-feature half of ECHOBlock: desc = ECHO(modReLU(conv(x))), reference nn/echo_block.py:93-94 (the MLP on the descriptors
 * and the linear residual on |x|, :95-103, are the reference's own nn.Linear layers and stay with the caller).  conv: (n_des, C_in)
 * filter; bias: the first n_des entries of the module's TangentNonLin bias (:57,93); ln_* / wxp_* (E) c64 in by_target / by_source slot
 * order as for fc_echo_forward / fc_echo_backward; desc (N, n_des, fc_echo_hist_dim(n_bins)) f32. */
typedef struct fc_echo_block_params {
    int32_t C_in, n_des, n_bins;
    fc_filter_params conv;
    const float* bias;
    float* g_bias;
} fc_echo_block_params;
size_t fc_echo_block_saved_bytes(const fc_mesh* mesh, const fc_echo_block_params* p);
size_t fc_echo_block_workspace_bytes(const fc_mesh* mesh, const fc_echo_block_params* p, int32_t backward);
int fc_echo_block_forward(const float* x, const fc_mesh* mesh, const float* ln_t, const float* wxp_t, const fc_echo_block_params* p,
                          float* desc, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int fc_echo_block_backward(const float* x, const float* g_desc, const fc_mesh* mesh, const float* ln_s, const float* wxp_s,
                           const fc_echo_block_params* p, const void* saved, size_t saved_bytes, float* gx, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ECHOBlock behind its descriptors, reference nn/echo_block.py:95-103:  y = lin3(relu(lin2(relu(lin1(d))))) + res(softAbs(x)).
 * d (N, D) f32 the flattened descriptors (D = n_des * fc_echo_hist_dim(n_bins)), x (N, C_in) c64 the block's input, y (N, C_out) f32;
 * w1 (H1, D), w2 (H2, H1), w3 (C_out, H2), wr (C_out, C_in) and the biases as torch.nn.Linear holds them (the reference: H1 = 128,
 * H2 = 64); H1 <= 128, H2 <= 64, C_in <= 64, C_out <= 64, else FC_ERR_UNSUPPORTED (the host then composes the tail of dense layers).
 * forward: h1 (N, H1) and h2 (N, H2) receive the hidden activations (after their ReLUs) -- the caller keeps them, with d and x, for the
 * backward pass.  backward: g (N, C_out) the cotangent of y; g_d (N, D), gx (N, C_in) c64, every g_* of the struct (weights and biases)
 * and g_h1 (N, H1, scratch the caller provides) are written.  All products run on v_mfma_f32_16x16x4_f32 (fp32 operands and sums);
 * three launches per pass (csrc/fc_head.hip). */
typedef struct fc_echo_head_params {
    int32_t D, H1, H2, C_in, C_out;
    const float *w1, *b1, *w2, *b2, *w3, *b3, *wr, *br;
    float *g_w1, *g_b1, *g_w2, *g_b2, *g_w3, *g_b3, *g_wr, *g_br;       /* backward only */
} fc_echo_head_params;
size_t fc_echo_head_forward_workspace_bytes(int32_t N, const fc_echo_head_params* p);
int fc_echo_head_forward(const float* d, const float* x, const fc_echo_head_params* p, float* h1, float* h2, float* y, void* workspace,
                         size_t workspace_bytes, int32_t N, void* stream);
size_t fc_echo_head_backward_workspace_bytes(int32_t N, const fc_echo_head_params* p);
int fc_echo_head_backward(const float* d, const float* x, const float* h1, const float* h2, const float* g, const fc_echo_head_params* p,
                          float* g_d, float* gx, float* g_h1, void* workspace, size_t workspace_bytes, int32_t N, void* stream);

/* LiftBlock: out = modReLU(TransField(x)), reference nn/lift_block.py:53-55.  x (N,C_in) f32, C_in <= 4, C_out <= 64; lift_sten /
 * sten_stride / slot_to_edge_* as for fc_trans_field_forward / _backward (mesh: N, E, R and the two groupings with nbr; kind, fwd, bwd
 * are not read); phase / g_phase for ftype != 0 only (phase: zeros otherwise). */
typedef struct fc_lift_block_params {
    int32_t C_in, C_out, ftype;
    const float* zonal_ang;
    const float* zonal_mag;
    const float* phase;
    const float* bias;
    float* g_zonal_ang;
    float* g_zonal_mag;
    float* g_phase;
    float* g_bias;
} fc_lift_block_params;
size_t fc_lift_block_saved_bytes(const fc_mesh* mesh, const fc_lift_block_params* p);
size_t fc_lift_block_workspace_bytes(const fc_mesh* mesh, const fc_lift_block_params* p, int32_t backward);
int fc_lift_block_forward(const float* x, const float* lift_sten, int32_t sten_stride, const fc_mesh* mesh, const int64_t* slot_to_edge_t,
                          const fc_lift_block_params* p, float* out, void* saved, size_t saved_bytes, void* stream);
int fc_lift_block_backward(const float* g_out, const float* lift_sten, int32_t sten_stride, const fc_mesh* mesh, const int64_t* slot_to_edge_s,
                           const fc_lift_block_params* p, const void* saved, size_t saved_bytes, float* gx, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- TransField and ECHO outside the specialised kernels' range: any number of scalar inputs / output channels / rings / raster bins,
 * float32 or float64 (dtype: fc_dtype of every tensor; the reference's TransField / LiftBlock run under .double(), nn/trans_field.py:78-113;
 * its ECHO and FCPrecomp do not -- both raise a dtype error -- so the float64 ECHO here has no reference counterpart).  Run-time loops, one
 * thread per output entry, fixed summation order: a correctness path.  Same arguments as the specialised calls; lift_sten is a complex array
 * (float2 / double2 elements) with sten_stride >= 2 (no factor table); the backward workspace is
 * fc_trans_field_backward_generic_workspace_bytes(...) bytes; the ECHO calls take fc_echo_generic_workspace_bytes(n_bins) bytes of scratch
 * (the raster map) and dS = fc_echo_hist_dim_generic(n_bins). */
int fc_trans_field_forward_generic(const void* x, const void* lift_sten, const fc_csr* by_target, const int64_t* slot_to_edge,
                                   const void* zonal_ang, const void* zonal_mag, const void* phase, void* y, void* ang, void* mag,
                                   void* s1sum, int32_t N, int32_t E, int32_t Cin, int32_t O, int32_t R, int32_t sten_stride, int32_t dtype,
                                   void* stream);
size_t fc_trans_field_backward_generic_workspace_bytes(int32_t N, int32_t Cin, int32_t O, int32_t R, int32_t dtype);
int fc_trans_field_backward_generic(const void* lift_sten, const fc_csr* by_source, const int64_t* slot_to_edge_s, const void* zonal_ang,
                                    const void* zonal_mag, const void* phase, const void* ang, const void* mag, const void* s1sum,
                                    const void* gy, void* gx, void* g_zonal_ang, void* g_zonal_mag, void* g_phase, void* workspace,
                                    size_t workspace_bytes, int32_t N, int32_t E, int32_t Cin, int32_t O, int32_t R, int32_t sten_stride,
                                    int32_t ftype, int32_t dtype, void* stream);
int fc_echo_hist_dim_generic(int32_t n_bins);
size_t fc_echo_generic_workspace_bytes(int32_t n_bins);
int fc_echo_forward_generic(const void* x, const void* ln_t, const void* wxp_t, const fc_csr* by_target, void* hist, void* desc,
                            void* workspace, size_t workspace_bytes, int32_t N, int32_t E, int32_t C, int32_t n_bins, int32_t dtype,
                            void* stream);
int fc_echo_backward_generic(const void* x, const void* ln_s, const void* wxp_s, const fc_csr* by_source, const void* hist,
                             const void* g_desc, void* gx, void* hist_grad_workspace, void* workspace, size_t workspace_bytes, int32_t N,
                             int32_t E, int32_t C, int32_t n_bins, int32_t dtype, void* stream);

/* ---- support-graph build (what every FieldConv needs before its first launch on a mesh) ---------------------------- *
 * From the operator's own inputs (reference nn/field_conv.py:104-121): supp_edges (E,2) int64, col 0 = source, col 1 =
 * target; supp_sten (E,R,F) c64 contiguous, F = 2B+1 (NULL: edge grouping only, for the ECHO / TransField entry points)
 * to the two fc_csr groupings and the per-edge records of fc_forward_factored / fc_forward_geometric /
 * fc_backward_data_factored.  Slots are ordered by (vertex, lower ring q, original edge index); perm_* (E) int64 give the
 * original edge of every slot; runs_* are (N,8) int32; rec_* hold E rows of fc_factored_record_floats(B) floats, geo_t E
 * rows of 8 floats -- the caller allocates and zeroes the >= 1 KiB of padding behind them.  flags (one device int32):
 * bit 0 the stencil is NOT of the rank-1 / two-adjacent-rings form (every row is reconstructed and compared, relative
 * tolerance 2e-6): rec_* / geo_t must not be used, use the dense entry points with supp_sten[perm]; bit 1 the phases are
 * not geometric in the frequency: geo_t must not be used; bit 2 an edge refers to a vertex outside [0, N).
 * No host synchronisation inside; reading `flags` is the caller's one synchronisation per mesh. */
size_t fc_graph_workspace_bytes(int32_t N, int32_t E, int32_t R, int32_t F, int32_t with_stencil);
int fc_graph_build(const int64_t* supp_edges, const float* supp_sten, int32_t N, int32_t E, int32_t R, int32_t F,
                   int32_t* rowptr_t, int32_t* nbr_t, int32_t* runs_t, int64_t* perm_t, int32_t* rowptr_s,
                   int32_t* nbr_s, int32_t* runs_s, int64_t* perm_s, float* rec_t, float* rec_s, float* geo_t,
                   int32_t* flags, void* workspace, size_t workspace_bytes, void* stream);

/* ---- FCPrecomp (stencil assembly), reference transforms/fc_precomp.py:53-97 ------------------------------------------ *
 * Inputs as the reference's data object holds them: log_mag (E) f32, log_ang (E) f32, xp (E) c64, w (N) f32 (vertex
 * areas), supp_edges (E,2) int64, epsilon (support radius).  Two steps because the number of kept edges E' (those with
 * log_mag / epsilon <= 1) sizes the outputs: fc_precomp_mark enqueues the selection; the two int32 at
 * fc_precomp_kept_count_ptr() then hold E' and a flag that is non-zero when a kept edge refers to a vertex outside [0, N)
 * (device memory: the caller's one synchronisation; supp_edges may be NULL for fc_precomp_mark: no range check).  Then, with
 * the same workspace, EITHER
 *   fc_precomp_build   writes supp_edges_out (E',2) int64, supp_sten (E',R,F) c64, ln (E') c64 and wxp (E') c64 in the
 *                      original edge order (the reference's outputs as they are), OR
 *   fc_precomp_graph   goes straight to what the convolutions consume: supp_edges_out, ln, wxp as above,
 *                      `factors` (E',8) f32 = [q bits, w_q, w_{q+1}, 0, Re wxp, Im wxp, cos theta, sin theta] per kept edge
 *                      (the stencil row is w_r * wxp * e^{i m theta}: anything that wants dense rows builds them from this),
 *                      and every output of fc_graph_build (both groupings, ring-run offsets, permutations, factored and
 *                      geometric records) -- the (E',R,F) stencil is never written or read.  graph_workspace:
 *                      fc_graph_workspace_bytes(N, E', R, F, 1) bytes; flags as for fc_graph_build (bits 0/1 never set).
 *                      rec_t / rec_s hold E' + rec_pad_rows rows, geo_t E' + geo_pad_rows: the rows behind the E'-th are
 *                      zero-filled here (the convolution kernels stream a little past the end of the records). */
size_t fc_precomp_workspace_bytes(int32_t N, int32_t E);
int fc_precomp_mark(const float* log_mag, const int64_t* supp_edges, float epsilon, int32_t N, int32_t E, void* workspace,
                    size_t workspace_bytes, void* stream);
const int32_t* fc_precomp_kept_count_ptr(const void* workspace, int32_t E);
int fc_precomp_build(const float* log_mag, const float* log_ang, const float* xp, const float* w, const int64_t* supp_edges,
                     float epsilon, int32_t N, int32_t E, int32_t R, int32_t F, int64_t* supp_edges_out, float* supp_sten,
                     float* ln, float* wxp, void* workspace, size_t workspace_bytes, void* stream);
int fc_precomp_graph(const float* log_mag, const float* log_ang, const float* xp, const float* w, const int64_t* supp_edges,
                     float epsilon, int32_t N, int32_t E, int32_t E_kept, int32_t R, int32_t F, int32_t rec_pad_rows,
                     int32_t geo_pad_rows, int64_t* supp_edges_out, float* ln, float* wxp, float* factors, int32_t* rowptr_t, int32_t* nbr_t, int32_t* runs_t, int64_t* perm_t,
                     int32_t* rowptr_s, int32_t* nbr_s, int32_t* runs_s, int64_t* perm_s, float* rec_t, float* rec_s, float* geo_t,
                     int32_t* flags, void* precomp_workspace, size_t precomp_workspace_bytes, void* graph_workspace,
                     size_t graph_workspace_bytes, void* stream);

/* ---- fused Adam over a flat float32 parameter buffer (torch.optim.Adam arithmetic, L2 weight decay, no amsgrad) -------- *
 * params, grads, exp_avg, exp_avg_sq: n floats each, n a multiple of 4, 16-byte aligned; step: one device float holding
 * the number of steps taken so far (incremented on the device, so the call is capturable in a HIP graph). */
int fc_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step, size_t n, float lr,
                 float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- the same step with controls a captured step can steer from the device (csrc/fc_optim.hip) ------------------------- *
 * The buffers are those above; in addition
 *   lr      one DEVICE float: the learning rate, read by the update kernel (a replayed graph follows what is written there)
 *   stats   four DEVICE floats, written every call: {gradient norm before clipping, clip coefficient, 1 if this step was
 *           skipped else 0, number of steps skipped so far (stats[3] is read and incremented: zero it once)}
 *   ema     n floats, the moving average of the parameters; NULL unless ema_decay >= 0
 *   ctl     the struct below, read on the host at call time (so its values are constants of a captured graph)
 * Three launches (two when neither the norm nor the skip is wanted), no atomics, no host synchronisation:
 *  a. sum of squares, launched when max_norm > 0 or skip_nonfinite: workgroup b of 256 threads covers the float4
 *     [1024 b, 1024 (b+1)) of grads; thread t adds, to a running DOUBLE that starts at 0, ((x^2 + y^2) + z^2) + w^2 of the float4
 *     1024 b + 256 r + t for r = 0, 1, 2, 3 in that order (every square formed in double: exact); the 64 lanes of a wavefront
 *     are combined by an xor butterfly (lane distance 32, 16, 8, 4, 2, 1), then the workgroup's four wavefronts are added in
 *     index order starting from 0, and the result is partial[b].  There are ceil(n / 4096) partials.
 *  b. finalize and tick, one workgroup of 256 threads: thread t adds partial[t], partial[t + 256], ... in that order to a
 *     double that starts at 0, then butterfly and wavefront order as in a.: S.  The order of every addition is a function of n
 *     alone, so two runs give the same bits.  A NaN or an infinity anywhere in grads makes S non-finite; S cannot overflow
 *     otherwise.  Then, with norm_d = sqrt(S) in double:
 *         skip  = skip_nonfinite && !isfinite(S)
 *         coef  = max_norm > 0 ? (float)min(1, (double)max_norm / (norm_d + 1e-6)) : 1        (torch's clip_grad_norm_, in double,
 *                 rounded once; as in torch's clamp a NaN quotient stays a NaN)
 *         step[0] += 1 unless skip;  stats = {(float)norm_d, coef, skip, stats[3] + skip}
 *     (float)norm_d may be inf while S is finite: that is reported, not a skip.  When neither the norm nor the skip is wanted the
 *     launch only ticks and writes stats = {0, 1, 0, stats[3]}.
 *  c. update, one pass over the flat buffers.  If skip, nothing is written: params, the moments, ema and step keep their bits.
 *     Otherwise, with t = step[0] and lr = lr[0]:
 *         g  = coef * grads[i]                       (grads itself is NOT modified, unlike torch's clip_grad_norm_)
 *         decoupled == 0:  g' = g + wd p             (L2, as the step above)
 *         decoupled != 0:  p = p * (1 - lr * wd) first, then g' = g          (torch.optim.AdamW's order)
 *         m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *         ema_decay >= 0:  ema = d * ema + (1 - d) * p      (the new p; d = ema_decay < 1)
 *     every operation in float32.  With max_norm <= 0, skip_nonfinite == 0, decoupled == 0 and ema_decay < 0 the results are the
 *     bits of the step above for the same lr.
 * Errors as above (null pointers, n not a multiple of 4, ema missing or ema_decay >= 1: FC_ERR_BAD_ARGUMENT); n == 0 is FC_OK and
 * launches nothing.  Workspace: the query below, 256 + 8 ceil(n / 4096) bytes rounded up to 256; FC_ERR_WORKSPACE when it is missing
 * or smaller.  It carries coef and skip from b. to c. and need not be kept between calls. */
typedef struct fc_adam_ctl {
    float beta1, beta2, eps, weight_decay;
    int32_t decoupled;        /* 0: L2 weight decay, else decoupled (AdamW) */
    float max_norm;           /* <= 0: no clipping */
    int32_t skip_nonfinite;   /* != 0: a step whose gradient holds a NaN or an infinity changes nothing */
    float ema_decay;          /* < 0: no moving average */
} fc_adam_ctl;
size_t fc_adam_ctl_workspace_bytes(size_t n);
int fc_adam_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, float* step, const float* lr,
                     float* stats, void* workspace, size_t workspace_bytes, size_t n, const fc_adam_ctl* ctl, void* stream);

/* ---- support graph (the reference's SupportGraph transform: farthest-point sampling, then a radius search) ---------- *
 * Distances: d2 = (dx*dx + dy*dy) + dz*dz in fp32 with dx = p_n.x - p_q.x, every operation rounded on its own (no fused
 * multiply-add), in both searches.  pos: (N,3) float32, contiguous, device memory.
 * fc_fps             idx (n_samples) int64 in selection order, idx[0] = start; each round takes the unselected point with the
 *                    largest min over selected s of d2(i, s), ties to the lowest index; a point is never taken twice.
 *                    1 <= n_samples <= N, 0 <= start < N.  One workgroup; workspace: fc_fps_workspace_bytes(N).
 * fc_radius_count    enqueues the per-query counts of the points n with d2(q, n) < r2, r2 = epsilon * epsilon in fp32 (q itself
 *                    included), capped at max_num_neighbors = K, and their scan; afterwards fc_radius_edge_count_ptr() points
 *                    at the device int64 E, the number of rows (the caller's one synchronisation reads it).
 * fc_radius_fill     with the same workspace, writes supp_edges (E,2) int64 [q, n]: queries ascending, each query's
 *                    neighbours ascending; a query with more than K qualifying points keeps the K smallest (d2, n).
 * epsilon must be positive and finite, K >= 1.  No allocation or synchronisation inside. */
size_t fc_fps_workspace_bytes(int32_t N);
int fc_fps(const float* pos, int32_t N, int32_t n_samples, int32_t start, int64_t* idx, void* workspace, size_t workspace_bytes,
           void* stream);
size_t fc_radius_workspace_bytes(int32_t N);
int fc_radius_count(const float* pos, int32_t N, float epsilon, int32_t max_num_neighbors, void* workspace, size_t workspace_bytes,
                    void* stream);
const int64_t* fc_radius_edge_count_ptr(const void* workspace, int32_t N);
int fc_radius_fill(const float* pos, int32_t N, float epsilon, int32_t max_num_neighbors, int64_t E, int64_t* supp_edges,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The same over a mini-batch of point sets: pos (N,3) holds B sets one after the other, set b in the rows ptr[b] .. ptr[b+1] - 1
 * (ptr: B+1 int64 in DEVICE memory, ascending, ptr[0] = 0, ptr[B] = N).  The tables live on the device and the library cannot
 * look at them: the CALLER has checked them.  The kernels clamp what they read from them, so that a malformed table gives a
 * meaningless result but no access outside the buffers.
 * fps batched        one workgroup per set, fc_fps's rounds and selection rule inside it.  n_samples, start, out_ptr: B int64
 *                    each, device memory; set b writes n_samples[b] indices LOCAL to the set (0 <= index < n_b, the first one
 *                    start[b]) to idx[out_ptr[b] ..]; idx holds S_total int64.  A set with n_samples[b] outside [1, n_b], start[b]
 *                    outside [0, n_b) or an output range outside idx writes nothing.  Workspace: the query below.
 * radius batched     count / fill as above with neighbours searched inside the query's own set only; rows [q, n] are numbered in
 *                    the union (local index + ptr[b]), queries ascending, each query's neighbours ascending: the single-set rows
 *                    of every set plus its offset, one set after the other.  One epsilon and one K for the batch.  Workgroups
 *                    map to (set, tile of 256 queries) pairs.  Workspace and edge count: fc_radius_workspace_bytes(N) and
 *                    fc_radius_edge_count_ptr(workspace, N), as above.  N + 256 B < 2^31. */
size_t fc_fps_batched_workspace_bytes(int32_t N);
int fc_fps_batched(const float* pos, const int64_t* pos_ptr, int32_t N, int32_t B, const int64_t* n_samples, const int64_t* start,
                   const int64_t* out_ptr, int64_t S_total, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream);
int fc_radius_count_batched(const float* pos, const int64_t* ptr, int32_t N, int32_t B, float epsilon, int32_t max_num_neighbors,
                            void* workspace, size_t workspace_bytes, void* stream);
int fc_radius_fill_batched(const float* pos, const int64_t* ptr, int32_t N, int32_t B, float epsilon, int32_t max_num_neighbors, int64_t E,
                           int64_t* supp_edges, void* workspace, size_t workspace_bytes, void* stream);

/* ---- losses (the reference's TwinLoss, TwinEval, LabelSmoothingLoss) and the pair kernels under them ------------------ *
 * Features: xS (N_S,C) and xT (N_T,C), row-major, contiguous, device memory, real; dtype 0 = float32, 1 = float64 (every
 * device scalar and array of the call then has that type).  Pair lists: (K,2) int64 rows [row of xT, row of xS].
 * Distance: d2(a,b) = ((t0*t0 + t1*t1) + t2*t2) + ... with t_c = xT[a,c] - xS[b,c], c ascending, every operation rounded on
 * its own (no fused multiply-add); all four pair kernels produce the same bits for the same pair.  Sums that end in one
 * scalar run in double in a fixed order: two runs give the same bits.  Rows within N < 2^24 and N*C*8 < 4 GiB.
 * pair sqdist         d2 (K) for a pair list whose indices the CALLER has checked (the kernel does not).
 * twin loss forward   loss[0] = sum_k d2(p_k) / P + sum_k (yN_k d2(n_k) + (1 - yN_k) max(mu - d2(n_k), 0)) / M, and
 *                     d2 (P + M): the positives' distances, then the negatives', saved for the backward pass.  A pair with an
 *                     index outside [0,N_T) x [0,N_S) reads nothing and counts as NaN.  P, M >= 1.  yN (M) is float32 for either
 *                     dtype, and 1 - yN_k is rounded in float32 before it is widened (the reference draws float32 weights).
 * twin loss backward  grad_xT[a] = sum over the pairs k at row a of c_k t, grad_xS[b] = -sum c_k t, t = xT[a] - xS[b],
 *                     c_k = 2 g / P (positives), 2 g (yN_k - (1 - yN_k) [mu - d2_k > 0]) / M (negatives), g = grad_loss[0].
 *                     Pairs are numbered p_ first, then n_ (k in [0, P + M)).  order_T (P + M): the pair numbers sorted
 *                     stably by their xT row; rowptr_T (N_T + 1): row a owns order_T[rowptr_T[a] .. rowptr_T[a + 1]);
 *                     likewise order_S / rowptr_S by xS row.  Each row sums its pairs in that order (no atomics) and every
 *                     row of the dense (N,C) gradients is written, zeros where no pair touches it.
 * twin count dense    over ALL pairs (a,b) in [0,N_T) x [0,N_S): counts[t] = #{d2 < thr_t}, counts[T + t] = #{d2 > thr_t} for
 *                     T = n_thresholds in [1,16]; thresholds is a HOST array, each value rounded to dtype.  counts: 2T device int64.
 * label smoothing     pred (N,K), target (N) int64, weight (K) or null: loss[0] = mean_n sum_k -t_nk w_k log_softmax(pred_n)_k
 *                     with t_nk = confidence at k = target_n and off_value elsewhere; backward recomputes the softmax:
 *                     grad_pred[n,j] = (g / N) (softmax_nj sum_k t_nk w_k - t_nj w_j).  A target outside [0,K) selects no class.
 * Workspaces: the *_workspace_bytes queries (per-workgroup partial sums).  No allocation or synchronisation inside. */
int fc_pair_sqdist(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* pairs, int64_t K,
                   void* d2, void* stream);
size_t fc_twin_loss_workspace_bytes(int64_t P, int64_t M);
int fc_twin_loss_forward(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* p_, int64_t P,
                         const int64_t* n_, int64_t M, const void* yN, double mu, void* d2, void* loss, void* workspace,
                         size_t workspace_bytes, void* stream);
int fc_twin_loss_backward(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* p_, int64_t P,
                          const int64_t* n_, int64_t M, const void* yN, double mu, const void* d2, const void* grad_loss,
                          const int64_t* rowptr_T, const int64_t* order_T, const int64_t* rowptr_S, const int64_t* order_S, void* grad_xT,
                          void* grad_xS, void* stream);
int fc_twin_count_dense(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const double* thresholds,
                        int32_t n_thresholds, int64_t* counts, void* stream);
size_t fc_label_smoothing_workspace_bytes(int64_t N, int32_t K);
int fc_label_smoothing_forward(const void* pred, const int64_t* target, const void* weight, int64_t N, int32_t K, int32_t dtype,
                               double confidence, double off_value, void* loss, void* workspace, size_t workspace_bytes, void* stream);
int fc_label_smoothing_backward(const void* pred, const int64_t* target, const void* weight, const void* grad_loss, int64_t N, int32_t K,
                                int32_t dtype, double confidence, double off_value, void* grad_pred, void* stream);


/* ---- per-mesh pooling over a mini-batch of meshes (csrc/fc_segment.hip) ---------------------------------------------- *
 * x (N,C) row-major, contiguous, device memory; mesh b owns the rows ptr[b] .. ptr[b+1] - 1 (ptr: B+1 int64 in DEVICE memory,
 * ascending, ptr[0] = 0, ptr[B] = N, checked by the CALLER; the kernels clamp its entries to [0, N], so a malformed ptr
 * gives meaningless values but no access outside the buffers).  dtype 0 = float32, 1 = float64; reduce 0 = mean, 1 = sum.
 * soft abs forward   x: complex (interleaved re, im of that dtype); out[b,c] = reduce_{n in mesh b} softAbs(x[n,c]), out (B,C)
 *                    real: |x| outside the origin box, 0 inside (reference utils/field.py:29-37), never written out per vertex.
 * soft abs backward  grad_x[n,c] = grad_out[b,c] s_b x/|x| outside the origin box and 0 inside (fc_soft_abs_backward's rule),
 *                    s_b = 1 (sum) or 1 / n_b (mean); grad_out (B,C) real, grad_x complex like x.
 * forward, backward  the same for real x: out[b,c] = reduce x[n,c]; grad_x[n,c] = grad_out[b,c] s_b.
 * An empty mesh gives 0 (also as a mean) and no gradient.  Sums run in the input's precision in an order fixed by (ptr, C):
 * rows in chunks of 64 counted from the mesh's first row; in a chunk, four running sums over the rows w, w + 4, ... (w = 0..3,
 * ascending), combined as (a_0 + a_1) + (a_2 + a_3); the chunks of a mesh the same way (chunks w, w + 4, ...; then
 * (s_0 + s_1) + (s_2 + s_3)); a mean divides the sum by n_b.  No atomics: the same bits on every run.  Two launches forward,
 * one backward.  N >= 0, B >= 1, 1 <= C <= 64 * 65535, N + 64 B < 2^31.  Workspace (forward only): the query below.
 * No allocation or synchronisation inside. */
size_t fc_segment_pool_workspace_bytes(int32_t N, int32_t B, int32_t C, int32_t dtype);
int fc_segment_pool_soft_abs_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t reduce,
                                     void* out, void* workspace, size_t workspace_bytes, void* stream);
int fc_segment_pool_soft_abs_backward(const void* x, const void* grad_out, const int64_t* ptr, int32_t N, int32_t B, int32_t C,
                                      int32_t dtype, int32_t reduce, void* grad_x, void* stream);
int fc_segment_pool_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t reduce, void* out,
                            void* workspace, size_t workspace_bytes, void* stream);
int fc_segment_pool_backward(const void* grad_out, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t reduce,
                             void* grad_x, void* stream);

/* ---- descriptor matching: the k nearest rows of xS for every row of xT (csrc/fc_match.hip) ---------------------------- *
 * Features and distance as in the losses section above: xS (N_S,C), xT (N_T,C), dtype 0 = float32, 1 = float64, d2(a,b) the
 * SAME bits as fc_pair_sqdist and fc_twin_count_dense (one definition, csrc/fc_pair.hpp); the same limits on N and C.
 * match topk         for every row a of xT the k rows b of xS with the smallest d2(a,b), ordered by the pair (d2, b) ascending:
 *                    an exact tie goes to the lower row.  idx (N_T,k) int64 row numbers of xS, d2 (N_T,k) of the dtype;
 *                    1 <= k <= 8.  A NaN distance is never a match.  A slot without a candidate (fewer than k rows to search,
 *                    an excluded row, NaN distances) holds idx = -1, d2 = +inf.
 *                    ptr_S, ptr_T: both null, or (B+1) int64 tables in DEVICE memory of ascending ranges (ptr[0] = 0, ptr[B] = N),
 *                    checked by the CALLER: the rows ptr_T[m] .. ptr_T[m+1] - 1 of xT search the rows ptr_S[m] .. ptr_S[m+1] - 1
 *                    of xS only (the meshes of two mini-batches); idx stays a row number of the whole xS.  The kernels clamp
 *                    what they read from the tables: a malformed table gives a meaningless result but no access outside the
 *                    buffers.  B >= 1, N_T + 64 B < 2^31.
 *                    exclude: null, or (N_T) int64 in device memory: the one row of xS that row a skips; a value outside
 *                    [0, N_S) (-1 by convention) skips nothing.
 *                    parts: the xS range of every 64-row tile of xT is searched by `parts` workgroups (1 <= parts <= 1024), each
 *                    leaving its k best in the workspace, and a second launch merges them; parts = 1 is one launch and needs
 *                    no workspace; parts = 0 lets the library choose (enough workgroups to fill the card when N_T is small,
 *                    no part shorter than 4 tiles of xS).  The order (d2, b) is total, so the result does not depend on parts.
 * No atomics: two runs give the same bits.  Workspace: the query below, O(N_T k parts) bytes whatever N_S is (0 for parts = 1;
 * for parts = 0 sized for the most parts the library may choose for N_T rows); FC_ERR_WORKSPACE when it is missing or smaller.
 * No allocation or synchronisation inside. */
size_t fc_match_workspace_bytes(int32_t N_T, int32_t k, int32_t parts);
int fc_match_topk(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* ptr_S,
                  const int64_t* ptr_T, int32_t B, const int64_t* exclude, int32_t k, int32_t parts, int64_t* idx, void* d2,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- vertex-classification head: linear layer fused with cross-entropy / top-k prediction (csrc/fc_linear_ce.hip) ------ *
 * z = h W^T + b with h (N,H), weight (K,H), bias (K) or null (a torch.nn.Linear), float32 only.  The N x K logits are never
 * stored: every kernel recomputes the 64 x 64 tile it needs with one routine on the fp32 matrix pipe, so a logit has the same
 * bits in the loss, in the gradients and in the prediction.  target (N) int64 in DEVICE memory.
 * forward            lse[n] = log sum_k exp z[n,k]; loss_rows[n] = lse[n] - sum_k q[n,k] z[n,k] with q = confidence at the
 *                    target and off_value elsewhere (the caller keeps confidence + (K-1) off_value = 1); 0 where target[n] ==
 *                    ignore_index; NaN for any other target outside [0,K) (nothing is read for it).  total[0] = the sum of
 *                    loss_rows, total[1] = total[0] / total[2], total[2] = the number of rows whose target is not ignore_index
 *                    (three floats; the sums run in double in a fixed order).
 * topk               idx (N,k) int64, z (N,k): the k <= 8 classes with the largest logits per row ordered by (z descending,
 *                    class ascending): an exact tie goes to the lower class; a NaN logit sorts after every number; slots beyond
 *                    K hold idx = -1, z = -inf.
 * backward input     grad_h (N,H) = G weight,  G[n,k] = row_scale[n] (exp(z[n,k] - lse[n]) - q[n,k]); a row whose target is
 *                    ignore_index has G = 0 whatever row_scale holds, a row whose target is otherwise outside [0,K) has G = NaN.
 * backward weight    grad_weight (K,H) = G^T h and grad_bias (K) = the column sums of G; either may be null (not both).
 * parts              forward / topk: the classes of every 64-row tile are walked by `parts` workgroups whose per-row results a
 *                    second launch merges in part order; backward weight: the rows of every 64-class tile likewise, the
 *                    partial sums added in part order.  0 <= parts <= 64; 0 lets the library choose (enough workgroups to
 *                    fill the card, no part shorter than 4 tiles).  parts changes the order of the sums (the last bits), never
 *                    the top-k result (a total order).
 * No atomics: two runs give the same bits.  Workspace: the query below with pass 0 = forward, 1 = backward weight, 2 = topk
 * (k matters for pass 2 only): O(N parts), O(K H parts) (0 for parts = 1) and O(N k parts) bytes; for parts = 0 sized for the
 * most parts the library may choose; FC_ERR_WORKSPACE when it is missing or smaller.  No allocation or synchronisation inside. */
size_t fc_linear_ce_workspace_bytes(int32_t N, int32_t H, int32_t K, int32_t parts, int32_t pass, int32_t k);
int fc_linear_ce_forward(const float* h, const float* weight, const float* bias, const int64_t* target, int32_t N, int32_t H, int32_t K,
                         double confidence, double off_value, int64_t ignore_index, int32_t parts, float* lse, float* loss_rows,
                         float* total, void* workspace, size_t workspace_bytes, void* stream);
int fc_linear_topk(const float* h, const float* weight, const float* bias, int32_t N, int32_t H, int32_t K, int32_t k, int32_t parts,
                   int64_t* idx, float* z, void* workspace, size_t workspace_bytes, void* stream);
int fc_linear_ce_backward_input(const float* h, const float* weight, const float* bias, const int64_t* target, const float* lse,
                                const float* row_scale, int32_t N, int32_t H, int32_t K, double confidence, double off_value,
                                int64_t ignore_index, float* grad_h, void* stream);
int fc_linear_ce_backward_weight(const float* h, const float* weight, const float* bias, const int64_t* target, const float* lse,
                                 const float* row_scale, int32_t N, int32_t H, int32_t K, double confidence, double off_value,
                                 int64_t ignore_index, int32_t parts, float* grad_weight, float* grad_bias, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- mesh geodesics over the edge graph: distance rows, nearest source (csrc/fc_geodesic.hip) ---------------------------- *
 * The graph is a CSR over the vertices (rowptr (V+1), nbr (E) int32: the undirected triangle sides in both directions,
 * neighbours ascending; built by the caller) with one float32 length per slot.  This is the edge-graph metric, not the heat
 * method of the reference's fcutils: it overestimates the true geodesic by up to a few percent.
 * edge lengths       length[e] = sqrt((dx dx + dy dy) + dz dz) between pos[src[e]] and pos[nbr[e]] (src: the row of slot e), every
 *                    operation rounded on its own and a correctly rounded root: a numpy float32 restatement gives the same
 *                    bits.  An index outside [0,V) gives NaN and reads nothing.
 * distances          d is the least fixpoint of d[s] = 0 at the sources and d[v] = min_u fl32(d[u] + length(u,v)); unreachable
 *                    vertices hold +inf.  fl32(a + l) is monotone in a, so the fixpoint is unique and equals a heap Dijkstra
 *                    with float32 additions bit for bit, whatever the order of the relaxations.
 * labels             computed after d has converged, over the tight edges fl32(d[u] + length) == d[v] with d[v] finite:
 *                    label[v] = the smallest position in the source list among the sources that reach v along tight edges (a
 *                    source reaches itself; of a vertex listed twice the lower position counts); -1 where d = +inf.
 * One workgroup of 1024 threads solves one problem and writes only that problem's outputs: no atomics, no communication
 * between workgroups, the same bits on every run.  A range of at most fc_geodesic_lds_vertices vertices is solved in LDS (sized
 * to the range), a larger one in the output row in global memory by the same loop.
 * rows               S problems on one mesh, problem k with the single source sources[k]: dist (S,V).
 * nearest            B problems: mesh b owns the vertices pos_ptr[b] .. pos_ptr[b+1] - 1 and the sources (vertex numbers of
 *                    the union) at the positions src_ptr[b] .. src_ptr[b+1] - 1 of the list; both tables (B+1) int64 in DEVICE
 *                    memory, checked by the CALLER, or both null for one mesh (B = 1, max_range = V).  dist (V), label (V)
 *                    int64 positions in the whole list.  max_range: the largest range, at least every range's size (a larger
 *                    range would be left unsolved).  The kernels clamp what they read from the tables and skip sources and
 *                    neighbours outside the problem's range: malformed input gives a meaningless result, no access outside
 *                    the buffers.
 * sweeps             null, or int32 (problems,2): the sweeps of the distance loop and of the label loop (the last one of each
 *                    changes nothing).
 * Workspace (nearest only): the query below, 4 V bytes when max_range exceeds the LDS capacity, else 0; FC_ERR_WORKSPACE when
 * missing or smaller.  V, E < 2^31.  No allocation or synchronisation inside.
 * face areas         area[f] = 0.5 |(b - a) x (c - a)| for face (3,F) int64, float32, each operation rounded on its own; NaN for
 *                    an index outside [0,V).
 * segment sum        out[k] = (x[ptr[k]] + ... + x[ptr[k+1] - 1]) / divisor, added in float32 from left to right, one rounded
 *                    division (ptr (K+1) int64 in device memory, clamped to [0,N]): the fixed-order sum under the lumped
 *                    vertex masses (divisor 3) and the sample weights (divisor 1). */
int32_t fc_geodesic_lds_vertices(void);
int fc_mesh_edge_lengths(const float* pos, const int32_t* src, const int32_t* nbr, int32_t V, int32_t E, float* length, void* stream);
int fc_geodesic_rows(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* sources, int32_t S,
                     float* dist, int32_t* sweeps, void* stream);
size_t fc_geodesic_workspace_bytes(int32_t V, int32_t max_range);
int fc_geodesic_nearest(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                        const int64_t* sources, const int64_t* src_ptr, int32_t S, int32_t B, int32_t max_range, float* dist,
                        int64_t* label, int32_t* sweeps, void* workspace, size_t workspace_bytes, void* stream);
int fc_face_areas(const float* pos, const int64_t* face, int32_t V, int32_t F, float* area, void* stream);
int fc_segment_sum_f32(const float* x, const int64_t* ptr, int64_t N, int32_t K, float divisor, float* out, void* stream);

/* ---- sampling and neighbourhoods by the edge-graph metric (csrc/fc_geodesic_fps.hip) -------------------------------------- *
 * The graph, the lengths and the distance field d are those of the section above: every result is a function of least
 * fixpoints, the same bits whatever the schedule.  One workgroup of 1024 threads per problem, no atomics.  A relaxation pulls
 * only the vertices a neighbour's drop has flagged, runs at most n + 1 sweeps, and a mesh runs exactly n_samples rounds.
 * fps                B meshes in one launch: mesh b owns the vertices pos_ptr[b] .. pos_ptr[b+1] - 1 ((B+1) int64 in DEVICE
 *                    memory, checked by the CALLER; null: one mesh, B = 1, max_range = V).  n_samples, start, out_ptr: B
 *                    int64 each in device memory (also for one mesh).  idx[out_ptr[b] + k], k < n_samples[b], LOCAL to the
 *                    mesh: idx[.. + 0] = start[b]; sample k+1 is the vertex not yet taken with the largest d_k, the field of
 *                    the first k+1 samples (+inf is the largest value: other components and faceless vertices come first;
 *                    ties to the lowest vertex; no vertex twice, even where zero-length edges leave d = 0 on vertices not
 *                    taken).  1 <= n_samples[b] <= n_b, 0 <= start[b] < n_b, out_ptr[b] + n_samples[b] <= total_out.  dist
 *                    (V): every mesh's final field.  sweeps: null, or B int64, the relaxation sweeps summed over the rounds.
 *                    Each round starts from the previous field.  Workspace: 3 V bytes when max_range exceeds the LDS capacity.
 * ball count / fill  S queries: query q is the single-source problem from sample_idx[q] ((S) int64 vertex numbers, STRICTLY
 *                    ASCENDING, checked by the caller), relaxed only while candidates stay < epsilon (which leaves every
 *                    distance < epsilon as in the unbounded problem).  Its rows are [q, j] for the positions j with
 *                    d_q[sample_idx[j]] < epsilon (strict; j = q included), j ascending; with more than K of them the K
 *                    smallest by (distance, position).  pos_ptr / sample_ptr: both null, or the (B+1) int64 device tables of
 *                    the vertex ranges and the sample-position ranges: a query searches its own mesh.  count[q] = rows of
 *                    query q (int32) for q0 <= q < q0 + nq.  The caller forms offsets (S+1) int64 = exclusive prefix sums in
 *                    device memory and n_edges = offsets[S]; fill solves the queries again and writes edges (n_edges,2) int64
 *                    and, unless null, edge_dist (n_edges) float32: the bits of fc_geodesic_rows' row q.  Workspace: when
 *                    max_range exceeds the LDS capacity, one slot per query of the launch (the query below), else 0.
 * fps_among          fps with the choice restricted to candidates: candidate (V) uint8 in device memory, in the union's vertex
 *                    numbering, nonzero where the vertex may be taken.  idx[.. + 0] = start[b] (taken first even where it is no
 *                    candidate: the caller forbids that); sample k+1 is the CANDIDATE not yet taken with the largest d_k, and
 *                    d_k is still the field of the first k+1 samples over the whole mesh: every vertex relaxes, candidate or
 *                    not.  +inf first, ties to the lowest vertex, no vertex twice, as above; with every vertex a candidate the
 *                    result is fps's, index for index and bit for bit.  n_samples[b] may exceed the candidates of mesh b: once
 *                    none is free the remaining slots of the mesh hold -1 and dist is the field of what was taken.  Workspace
 *                    and errors as fps (fc_geodesic_fps_workspace_bytes); a null candidate is FC_ERR_BAD_ARGUMENT.
 * ball count_at /    ball count / fill for a LIST of queries: query_pos (Q) int64 in device memory, positions in sample_idx
 * fill_at            (ascending, checked by the caller, so that the rows come grouped as above); list slot s, for
 *                    q0 <= s < q0 + nq <= Q, solves query q = query_pos[s] and is skipped, with count 0, where q is outside
 *                    [0,S).  count (Q) and offsets (Q+1) are indexed by the list slot; the rows are [q, j], and bound, strict
 *                    threshold and truncation to K are those of the query q above: the rows of ball fill whose column 0 is in
 *                    the list.  Workspace: fc_geodesic_ball_workspace_bytes(max_range, nq), one slot per list slot of the
 *                    launch.  Q >= 1; a null query_pos is FC_ERR_BAD_ARGUMENT.
 * max_range as above: the largest range; the kernels clamp what they read from the tables.  V, E, S < 2^31.  FC_ERR_WORKSPACE
 * when a workspace is missing or smaller.  No allocation or synchronisation inside. */
int32_t fc_geodesic_fps_lds_vertices(void);
size_t fc_geodesic_fps_workspace_bytes(int32_t V, int32_t max_range);
int fc_geodesic_fps(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr, int32_t B,
                    int32_t max_range, const int64_t* n_samples, const int64_t* start, const int64_t* out_ptr, int64_t total_out,
                    int64_t* idx, float* dist, int64_t* sweeps, void* workspace, size_t workspace_bytes, void* stream);
size_t fc_geodesic_ball_workspace_bytes(int32_t max_range, int32_t queries);
int fc_geodesic_ball_count(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                           const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S, int32_t q0,
                           int32_t nq, float epsilon, int32_t K, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
int fc_geodesic_ball_fill(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                          const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S, int32_t q0,
                          int32_t nq, float epsilon, int32_t K, const int64_t* offsets, int64_t n_edges, int64_t* edges, float* edge_dist,
                          void* workspace, size_t workspace_bytes, void* stream);
int fc_geodesic_fps_among(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                          int32_t B, int32_t max_range, const uint8_t* candidate, const int64_t* n_samples, const int64_t* start,
                          const int64_t* out_ptr, int64_t total_out, int64_t* idx, float* dist, int64_t* sweeps, void* workspace,
                          size_t workspace_bytes, void* stream);
int fc_geodesic_ball_count_at(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                              const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S,
                              const int64_t* query_pos, int32_t Q, int32_t q0, int32_t nq, float epsilon, int32_t K, int32_t* count,
                              void* workspace, size_t workspace_bytes, void* stream);
int fc_geodesic_ball_fill_at(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                             const int64_t* sample_ptr, int32_t B, int32_t max_range, const int64_t* sample_idx, int32_t S,
                             const int64_t* query_pos, int32_t Q, int32_t q0, int32_t nq, float epsilon, int32_t K, const int64_t* offsets,
                             int64_t n_edges, int64_t* edges, float* edge_dist, void* workspace, size_t workspace_bytes, void* stream);

/* ---- log map and parallel transport by the discrete exponential map (csrc/fc_logmap.hip) ----------------------------------- *
 * Schmidt, Grimm, Wyvill 2006 over the edge-graph metric of the sections above; not the Vector Heat Method of the reference's
 * fcutils, and no parity with it.  The graph, the lengths and the bounded field d are those of the ball search.
 * frames             face_ptr (V+1) / face_idx (3F) int32: a CSR over the vertices of the faces that name them, one entry per
 *                    corner, ascending by (face, corner); built by the caller.  normal[v] = the sum of cross(p1 - p0, p2 - p0)
 *                    over that list (corners as stored), divided by its norm; (0,0,1) where the norm is 0.  ref = (0,0,1) where
 *                    |normal.z| < 0.95, else (1,0,0); e1 = normalize(cross(ref, normal)), e2 = cross(normal, e1).  Each (V,3)
 *                    float32, every operation rounded on its own: a numpy float32 restatement gives the same bits.
 * logmap             S queries as in the ball search (pos_ptr / sample_ptr / B / max_range / q0 / nq likewise; sample_idx need not
 *                    ascend).  Query q owns the rows row_ptr[q] .. row_ptr[q+1] - 1 ((S+1) int64 in device memory, clamped to
 *                    [0,n_rows]); row r names its target sample row_target[r], a position in sample_idx.  Per query: d bounded by
 *                    `bound` (candidates >= bound discarded); edge (u,v) is tight when both ends are reached and
 *                    fl32(d[u] + length) has the bits of d[v]; h = the least fixpoint of h[source] = 0, h[v] = 1 + min h[u] over
 *                    tight (u,v); pred[v] = the lowest-numbered tight u with h[u] = h[v] - 1.  Along pred, in float32:
 *                    X[source] = 1, L[source] = 0, X[v] = rho X[u], L[v] = L[u] + conj(X[u]) c, where c is p_v - p_u without its
 *                    normal[u] component, in u's frame, rescaled to the edge's length (0 where nothing is left), and rho is e1[u]
 *                    carried by the minimal rotation normal[u] -> normal[v], in v's frame, normalised (1 + n_u.n_v <= 1e-6: e1[u]
 *                    projected onto v's plane; 1 where that vanishes).  Row r: log_mag = |L[t]|, log_ang = atan2(im, re) (0 at
 *                    the origin), xp (n_rows,2) = X[t] (re, im), reached = 1.  A target not reached below the bound is unfolded
 *                    as a child of the source over a virtual edge of length |p_t - p_source|, with reached = 0.
 *                    debug_pred / debug_hops: both null, or (S,V) int32 set to -1 by the caller: the query's row gets pred (a
 *                    vertex number) and h of the vertices of its range, -1 where there is none.
 *                    ball_lds (at most fc_logmap_ball_lds_vertices): a ball of at most this many reached vertices keeps its tree
 *                    state in LDS, a larger one in the workgroup's workspace slot: the same bits either way.
 *                    A query whose source lies outside its range, or whose range exceeds max_range, gets NaN rows with
 *                    reached = 0.
 * One workgroup of 1024 threads per query writes that query's rows and slot only; no atomics, the same bits on every run;
 * every loop is bounded by the size of the range.  Workspace: the query below (0 when max_range fits both LDS capacities);
 * FC_ERR_WORKSPACE when missing or smaller.  No allocation or synchronisation inside. */
int32_t fc_logmap_ball_lds_vertices(void);
int fc_vertex_frames(const float* pos, const int64_t* face, const int32_t* face_ptr, const int32_t* face_idx, int32_t V, int32_t F,
                     float* normal, float* e1, float* e2, void* stream);
size_t fc_logmap_workspace_bytes(int32_t max_range, int32_t queries, int32_t ball_lds);
int fc_logmap(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
              const int64_t* sample_ptr, int32_t B, int32_t max_range, const float* pos, const float* normal, const float* e1, const float* e2,
              const int64_t* sample_idx, int32_t S, int32_t q0, int32_t nq, float bound, const int64_t* row_ptr, const int64_t* row_target,
              int64_t n_rows, float* log_mag, float* log_ang, float* xp, uint8_t* reached, int32_t* debug_pred, int32_t* debug_hops,
              int32_t ball_lds, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the edge graph enriched by unfolded diagonals (csrc/fc_mesh_graph.hip) -------------------------------------------------- *
 * Beside the triangle sides, the graph gets one edge across every interior side whose two faces unfold into a quadrilateral that
 * the straight segment between the opposite vertices stays inside.  Float32 throughout, every operation rounded on its own.
 * diagonals          face (3,F) int64; half-edge h = 3 f + k runs from corner k of face f to corner k + 1 and has corner k + 2
 *                    opposite.  key (N) int64, N <= 3 F: one entry per half-edge, equal exactly for the half-edges of one
 *                    undirected side, SORTED ascending with ties by ascending face; half (N) int64: the half-edge of each entry.
 *                    Half-edges of faces that name a vertex twice must not share a key with any other (the caller gives them a
 *                    key above every side's, or leaves them out).  Slot i is a candidate when it is the first of a run of exactly
 *                    two equal keys, both half-edges lie on the same side {u, v}, u < v, and the opposite vertices c (slot i) and
 *                    d (slot i + 1) differ.  Then e = p_v - p_u, L2 = (ex ex + ey ey) + ez ez (nothing when L2 == 0),
 *                    L = sqrt(L2); for w in (c, d): r = p_w - p_u, x_w = ((rx ex + ry ey) + rz ez) / L,
 *                    y_w = sqrt(max(((rx rx + ry ry) + rz rz) - x_w x_w, 0)); s = y_c + y_d (nothing when s <= 0);
 *                    t = x_c + (x_d - x_c) (y_c / s); the diagonal exists when 0 < t < L, both strict, and then
 *                    lo[i] = min(c, d), hi[i] = max(c, d), length[i] = sqrt((x_c - x_d) (x_c - x_d) + s s).  Every other slot
 *                    gets lo = hi = -1 and length NaN.  An index outside its range makes a slot no candidate and reads nothing.
 * merge              key (N) int64 SORTED ascending: the directed entries u V + v of sides and diagonals, both directions of
 *                    each; length (N) in the same order.  head[i] = 1 at the first entry of every run of equal keys inside
 *                    [0, V V), and there src[i] = u, nbr[i] = v, out_length[i] = the run's lengths folded from its first entry by
 *                    m = x < m ? x : m (the smallest; both directions of a pair hold the same lengths, so the same bits).  Every
 *                    other slot gets head 0, src = nbr = -1, NaN.  The heads, in order, are the CSR's slots by row with neighbours
 *                    ascending; the caller compacts them.
 * One thread per slot, each slot written by its own thread only: no atomics, the same bits on every run.  V, N < 2^31.  No
 * allocation or synchronisation inside. */
int fc_mesh_diagonals(const float* pos, const int64_t* face, int32_t V, int32_t F, const int64_t* key, const int64_t* half, int32_t N,
                      int32_t* lo, int32_t* hi, float* length, void* stream);
int fc_mesh_graph_merge(const int64_t* key, const float* length, int32_t N, int32_t V, uint8_t* head, int32_t* src, int32_t* nbr,
                        float* out_length, void* stream);

/* ---- sparse transfer between two sample levels: tangent-feature pooling and unpooling (csrc/fc_transfer.hip) ------------------- *
 *   y[o, c] = sum over the slots e in [rowptr[o], rowptr[o+1]) of coef[e] * x[col[e], c]
 * x (n_in, C) and y (n_out, C) row-major, dtype FC_F32 / FC_F64, is_complex 1 (interleaved pairs: complex64 / complex128) or 0
 * (float32 / float64).  rowptr (n_out+1) / col (n_slots) int32: a CSR by OUTPUT row.  weight (n_slots) real and phase (n_slots)
 * complex (interleaved), both of x's scalar type; phase may be NULL (1 everywhere).  Complex x: coef = weight * phase, or
 * weight * conj(phase) when conj_phase is 1.  Real x: coef = weight; phase and conj_phase are not read.
 * One lane owns one piece of 8 bytes or more of an output row and adds the row's terms to a zero in ascending slot order: no
 * atomics, the same bits on every run, a row without slots is written as zero.  The gradient to x is the same call on the
 * transposed CSR with conj_phase flipped.  rowptr entries are clamped to [0, n_slots]; a slot whose col lies outside [0, n_in)
 * contributes nothing and reads nothing.  C >= 1 is arbitrary.  No workspace, no allocation or synchronisation inside. */
int fc_transfer(const void* x, const int32_t* rowptr, const int32_t* col, const void* weight, const void* phase, int32_t conj_phase,
                int32_t n_out, int32_t n_in, int32_t n_slots, int32_t C, int32_t dtype, int32_t is_complex, void* y, void* stream);

/* ---- TangentNorm: per-mesh normalisation of tangent features (csrc/fc_norm.hip) ------------------------------------------------ *
 * x (N,C) complex (interleaved re, im of dtype: 0 = float32, 1 = float64), row-major, contiguous, device memory; mesh b owns the
 * rows ptr[b] .. ptr[b+1] - 1 (ptr as in the per-mesh pooling section: B+1 int64 in DEVICE memory, checked by the CALLER, clamped
 * to [0, N] by the kernels).  w (N) real of that dtype, non-negative, or NULL for 1; gain (C) real or NULL for 1; eps >= 0.
 *   W[b] = sum_n w[n]      m[b,c] = sum_n w[n] |x[n,c]|^2 / W[b]  (0 where W[b] == 0, and for an empty mesh)
 *   r[b,c] = 1 / sqrt(m[b,c] + eps)                     y[n,c] = gain[c] r[b,c] x[n,c]
 * forward   writes y (N,C) complex and r (B,C) real; r is what backward takes: the statistic is not recomputed.
 * backward  with t[b,c] = sum_n re(x) re(gy) + im(x) im(gy):
 *             gx[n,c]  = gain[c] r[b,c] gy[n,c] - gain[c] r[b,c]^3 t[b,c] (w[n] / W[b]) x[n,c]   (second term 0 where W[b] == 0)
 *             ggain[c] = sum_b r[b,c] t[b,c], b ascending
 *           gx (N,C) complex or NULL, ggain (C) real or NULL, not both NULL: what is NULL is not computed.
 * No mean is subtracted (a mean over samples would mix their frames), so only magnitudes are touched; magnitudes whose squares
 * leave the dtype's range are outside the contract.  Sums (W, m, t) run in the input's precision in the order of the per-mesh
 * pooling section -- 64-row chunks counted from the mesh's first row, four running sums per chunk and per mesh combined as
 * (a_0 + a_1) + (a_2 + a_3) -- which depends on the mesh's own row count and C only: no atomics, the same bits on every run and
 * for a mesh alone or inside a batch.  Three launches forward, at most four backward.  N >= 0, B >= 1, 1 <= C <= 64 * 65535,
 * N + 64 B < 2^31, else FC_ERR_BAD_ARGUMENT.  Workspace (both passes): the query below; FC_ERR_WORKSPACE when it is missing or
 * smaller.  No allocation or synchronisation inside. */
size_t fc_tangent_norm_workspace_bytes(int32_t N, int32_t B, int32_t C, int32_t dtype);
int fc_tangent_norm_forward(const void* x, const void* w, const int64_t* ptr, const void* gain, int32_t N, int32_t B, int32_t C, int32_t dtype,
                            double eps, void* y, void* r, void* workspace, size_t workspace_bytes, void* stream);
int fc_tangent_norm_backward(const void* x, const void* w, const int64_t* ptr, const void* gain, const void* r, const void* gy, int32_t N,
                             int32_t B, int32_t C, int32_t dtype, void* gx, void* ggain, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- interpolation weights: the k nearest candidates of every row and their inverse-distance weights (csrc/fc_interp.hip) ------ *
 * rowptr (n_f+1) / cand (n_slots) int32 / dist (n_slots) float32, >= 0 and finite: a CSR of candidates by receiving row, cand the
 * coarse position.  1 <= k <= 16, power 1 or 2, else FC_ERR_BAD_ARGUMENT.  With m = min(k, row length):
 *   sel (n_f, k) int32      the slots of the row's m smallest candidates by the key (dist as a float32 compare, cand, slot), in
 *                           that order; -1 from rank m on
 *   weight (n_f, k) float32 dist of rank 0 == 0: 1, 0, ..., 0.  Else q_i = d_i (power 1) or d_i * d_i (power 2),
 *                           u_i = 1 / max(q_i, 1e-30), s = ((u_0 + u_1) + u_2) + ... in rank order, w_i = u_i / s: every operation
 *                           a float32 operation rounded on its own.  0 from rank m on.
 * An empty row gives m = 0.  rowptr entries are clamped to [0, n_slots] and to the row's own start.  One lane per row, no atomics:
 * the same bits on every run.  No workspace, no allocation or synchronisation inside. */
int fc_knn_weights(const int32_t* rowptr, const int32_t* cand, const float* dist, int32_t n_f, int32_t n_slots, int32_t k, int32_t power,
                   int32_t* sel, float* weight, void* stream);

/* ---- max pooling by magnitude: over the rows of a transfer plan and over the meshes of a batch (csrc/fc_maxpool.hip) ----------- *
 * key     of a complex entry z: k = fl(fl(re * re) + fl(im * im)) in z's scalar type (float32 for complex64, float64 for
 *         complex128), every operation rounded on its own, no fused multiply-add: numpy gives the same bits.  |z| does not depend
 *         on the frame z is written in.  Of a real entry: k = x itself, a plain max and not a magnitude max.
 * winner  among candidates (k, s), s the slot (transfer) or the row number (meshes): the largest k wins, ties go to the smallest s.
 *         A candidate replaces the incumbent iff k_new > k_old, or k_new == k_old and s_new < s_old.  This is a total order: the
 *         result does not depend on how the candidates are split over lanes, wavefronts or launches.  NaN features are outside
 *         the contract: the winner is then meaningless, but nothing is read or written outside the buffers.
 * No atomics: every output element is owned by one lane, the same bits on every run.  No allocation or synchronisation inside.
 * Alignment: every feature and gradient buffer (x, y, grad_y, grad_x, out, grad_out, partial_key) starts on a multiple of the size of
 *         one of its entries -- 4 bytes for float32, 8 for float64 and complex64, 16 for complex128 -- and every int32 / int64 array
 *         on a multiple of its element's size; rows are dense, so every entry is then aligned.  This is not checked.  Only the
 *         float32 path of fc_transfer_max* asks for more when it can use it: with C even and x, y, arg (grad_y, grad_x, arg) on
 *         8-byte boundaries it moves two channels per lane, else one.
 *
 * fc_transfer_max            x (n_in, C), y (n_out, C), rowptr / col, phase, conj_phase, dtype, is_complex as in fc_transfer; there is
 *         NO weight: a max is not weighted and every slot of a row is a member.  For output row o and channel c the candidates are
 *         the slots e in [rowptr[o], rowptr[o+1]) with key(x[col[e], c]); with e* the winner, arg[o, c] = e* (arg: (n_out, C) int32)
 *         and y[o, c] = u[e*] * x[col[e*], c] for complex x, u = phase[e] (conj(phase[e]) when conj_phase is 1, 1 when phase is
 *         NULL): the winner's value parallel-transported into the receiver's frame; y[o, c] = x[col[e*], c], copied bit for bit, for
 *         real x (phase and conj_phase are not read).  rowptr entries are clamped to [0, n_slots]; a slot whose col lies outside
 *         [0, n_in) is no candidate and reads nothing.  A row without a usable slot gives y = 0 exactly and arg = -1.  A row may
 *         have any number of slots.  One launch.
 * fc_transfer_max_backward   on the TRANSPOSED CSR of the same plan: rowptr_t (n_in+1) / col_t (n_slots; the OUTPUT row of a slot) /
 *         phase_t (n_slots, or NULL) and slot_t (n_slots) int32, the slot number in the forward CSR of every transposed slot;
 *         conj_phase as given to the forward call.  grad_x[i, c] = the sum over the slots t of transposed row i, added to a zero in
 *         ascending order, with arg[col_t[t], c] == slot_t[t], of conj(u[t]) * grad_y[col_t[t], c] (real x: grad_y[col_t[t], c]
 *         alone).  An input that won nowhere gets exactly zero.  rowptr_t is clamped as above; a slot whose col_t lies outside
 *         [0, n_out) is skipped; arg and slot_t are only compared.  One launch.
 *
 * fc_segment_max_forward     x (N, C), ptr (B+1 int64, DEVICE memory, clamped to [0, N] by the kernels), dtype as in the per-mesh
 *         pooling section; is_complex 1 (interleaved pairs) or 0.  For mesh b and channel c the candidates are the rows
 *         n = ptr[b] .. ptr[b+1] - 1 with key(x[n, c]) and s = n; with n* the winner, index[b, c] = n* (index: (B, C) int32) and
 *         out[b, c] (real, (B, C)) = softAbs(x[n*, c]) for complex x -- sqrt(k) outside the origin box, 0 inside (reference
 *         utils/field.py:29-37, fc_soft_abs_forward's rule); |x| is never written per row -- or x[n*, c] bit for bit for real x.
 *         It is the softAbs of the entry of largest key, not the largest softAbs: softAbs is not monotone in |x| at the corner of the
 *         origin box.  An empty mesh gives out = 0 and index = -1.  Two launches: the partial winners (key, row) of every chunk of
 *         64 rows counted from a mesh's first row, then one combination per mesh over its chunks, both in the (k, s) order: the
 *         result equals a plain argmax whatever the chunking, and a mesh gets the same bits alone and inside a batch.  The partial
 *         buffers are caller-owned and need not be initialised: partial_key, N / 64 + B (integer division) rows of C scalars of
 *         dtype, and partial_row, as many rows of C int32 -- the chunk slots of the per-mesh pooling section, at least
 *         sum_b ceil(n_b / 64), known without reading ptr.
 * fc_segment_max_backward    one launch, every (n, c) written by its own thread: grad_x[n, c] = grad_out[b, c] * x / |x| outside the
 *         origin box and 0 inside (fc_soft_abs_backward's rule) where n == index[b, c], b the mesh of row n, and 0 everywhere else;
 *         for real x grad_x[n, c] = grad_out[b, c] there (x is not read and may be NULL).  grad_out (B, C) real, grad_x like x.
 * Limits of both: N >= 0, B >= 1, 1 <= C <= 64 * 65535, N + 64 B < 2^31, else FC_ERR_BAD_ARGUMENT. */
int fc_transfer_max(const void* x, const int32_t* rowptr, const int32_t* col, const void* phase, int32_t conj_phase, int32_t n_out,
                    int32_t n_in, int32_t n_slots, int32_t C, int32_t dtype, int32_t is_complex, void* y, int32_t* arg, void* stream);
int fc_transfer_max_backward(const void* grad_y, const int32_t* arg, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* slot_t,
                             const void* phase_t, int32_t conj_phase, int32_t n_out, int32_t n_in, int32_t n_slots, int32_t C, int32_t dtype,
                             int32_t is_complex, void* grad_x, void* stream);
int fc_segment_max_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t is_complex, void* out,
                           int32_t* index, void* partial_key, int32_t* partial_row, void* stream);
int fc_segment_max_backward(const void* x, const void* grad_out, const int32_t* index, const int64_t* ptr, int32_t N, int32_t B, int32_t C,
                            int32_t dtype, int32_t is_complex, void* grad_x, void* stream);

/* ---- a counter-based generator on the device, and dropout by a real mask (csrc/fc_philox.hpp, csrc/fc_dropout.hip) ------------- *
 * generator  Philox4x32-10 as published (Salmon et al., SC'11; Random123): multipliers 0xD2511F53 and 0xCD9E8D57, key increments
 *         0x9E3779B9 and 0xBB67AE85, ten rounds.  One round, from (c0, c1, c2, c3) and (k0, k1): p0 = M0 * c0 and p1 = M1 * c2 as
 *         64-bit products, c = (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)), then the key is bumped.
 * draws   key = (lo32(seed), hi32(seed)); counter = (lo32(q), hi32(q), lo32(step), stream): q the 64-bit block number, step the
 *         draw number (its low 32 bits), stream the user: 0 element dropout, 1 channel dropout, 2 augmentation.  Entry e of a draw
 *         uses word e & 3 of block e >> 2; a uniform is u = (word >> 8) * 2^-24, exact in float32, in [0, 1).
 * step    every entry point below that draws takes (step, step_ptr): with step_ptr NULL the draw number is step, else it is the
 *         int64 step_ptr points to in DEVICE memory, read by the kernel when it runs -- no synchronisation, and the replay of a
 *         captured launch sees the value of that time.
 *
 * fc_philox_words  the raw words, so that the generator itself can be pinned on the device: out (4 n_blocks) uint32, block i of it
 *         the words of counter (lo32(q), hi32(q), lo32(hi), hi32(hi)), q = first_block + i (wrapping at 2^64), under the key of
 *         seed.  n_blocks >= 0.
 * fc_dropout  x, y (N, C) row-major, contiguous, dtype FC_F32 / FC_F64, is_complex 1 (interleaved pairs: complex64 / complex128) or
 *         0; y must not be x.  threshold = floor(p * 2^24) for the drop probability p in [0, 1), computed by the CALLER in double;
 *         scale = 1 / (1 - p) in double, rounded here once to dtype.  Entry e is dropped iff (word >> 8) < threshold, an integer
 *         compare.  A kept entry is scale * x, one multiplication per scalar (re and im each) rounded on its own; a dropped entry
 *         is +0 (+0 +0j) exactly, whatever x holds.  The mask is real: the whole complex entry is kept or dropped, which commutes
 *         with any change of frames.
 *           mode 0 (element, stream 0)  e = n C + c in 64-bit arithmetic; ptr and B are not read (B >= 1 all the same)
 *           mode 1 (channel, stream 1)  e = b C + c, b the mesh of row n: mesh b owns the rows ptr[b] .. ptr[b+1] - 1 (ptr as in the
 *                                       per-mesh pooling section: B+1 int64 in DEVICE memory, checked by the CALLER, clamped to
 *                                       [0, N] by the kernel; NULL with B == 1: one mesh).  One decision per mesh and channel.
 *         The gradient is the same call on grad_y: the mask is never stored.  A decision is a function of (seed, step, stream, e)
 *         alone, so the result does not depend on the launch geometry.  x and y on 16-byte boundaries move 16 bytes per access in
 *         mode 0, anything else one scalar; entries are aligned as in the max-pooling section (not checked).  N >= 0, B >= 1,
 *         1 <= C <= 64 * 65535, N + 64 B < 2^31, threshold <= 2^24, scale > 0, else FC_ERR_BAD_ARGUMENT.
 * One launch each, every output element written by one thread: no atomics, the same bits on every run.  No workspace, no
 * allocation or synchronisation inside. */
int fc_philox_words(uint64_t seed, uint64_t hi, uint64_t first_block, int64_t n_blocks, uint32_t* out, void* stream);
int fc_dropout(const void* x, void* y, int32_t N, int32_t C, int32_t dtype, int32_t is_complex, int32_t mode, const int64_t* ptr, int32_t B,
               uint32_t threshold, double scale, uint64_t seed, int64_t step, const int64_t* step_ptr, void* stream);

/* ---- per-mesh augmentation: one random similarity per mesh of a batch (csrc/fc_augment.hip) ------------------------------------ *
 * fc_mesh_affine_draw   params (B, 4) and M (B, 3, 3) float32, row-major.  Mesh b uses block q = b of stream 2 of the draw
 *         (seed, step, step_ptr as above), u_k from word k:
 *           s = scale_lo + (scale_hi - scale_lo) * u_0  (has_scale 1; with has_scale 0, s = 1 and u_0 is unused)
 *           a_k = (2 * u_{k+1} - 1) * degrees_k, the angle about axis k in degrees;  params[b] = (s, a_0, a_1, a_2)
 *         every operation a float32 operation rounded on its own, no fused multiply-add: numpy gives the same bits.  With
 *         r_k = a_k * fl32(pi / 180), M[b] = s Rz(r_2) Ry(r_1) Rx(r_0), the right-handed rotations
 *           Rx = [1 0 0; 0 c -s; 0 s c]   Ry = [c 0 s; 0 1 0; -s 0 c]   Rz = [c -s 0; s c 0; 0 0 1]
 *         for column vectors: scale, then the rotation about axis 0, then 1, then 2.  sinf and cosf are the device library's, so M
 *         is accurate to a few units in the last place and NOT bit-exact.  B >= 1.
 * fc_mesh_affine_apply  pos (V, 3) float32; mesh b owns the vertices pos_ptr[b] .. pos_ptr[b+1] - 1 (B+1 int64, DEVICE memory,
 *         checked by the caller, clamped to [0, V] by the kernel); M (B, 3, 3); t (B, 3) float32 or NULL; index (R) int64 or NULL
 *         (then R output rows take the vertices 0 .. R - 1); out (R, 3).  Output row r takes vertex v = index[r] of the mesh b
 *         that owns v:  d = p_v - t_b (p_v without t),  out_i = (M_i0 d_0 + M_i1 d_1) + M_i2 d_2, every operation rounded on
 *         its own in float32.  A v outside [0, V) gives a row of NaN and reads nothing.  out must not overlap pos.
 *         B >= 1, 0 <= V < 2^31, R >= 0.
 * One launch each, one thread per mesh / per output row: no atomics, the same bits on every run.  No workspace, no allocation or
 * synchronisation inside. */
int fc_mesh_affine_draw(int32_t B, uint64_t seed, int64_t step, const int64_t* step_ptr, int32_t has_scale, float scale_lo, float scale_hi,
                        float degrees0, float degrees1, float degrees2, float* params, float* M, void* stream);
int fc_mesh_affine_apply(const float* pos, const int64_t* pos_ptr, int32_t B, int32_t V, const float* M, const float* t, const int64_t* index,
                         int64_t R, float* out, void* stream);

/* ---- intrinsic gradient of sample features and its adjoint, the divergence (csrc/fc_diffops.hip) --------------------------------- *
 * A weighted least-squares fit of a linear function over each sample's ball in its own tangent plane: the meshless gradient.  It
 * maps real features to complex ones (the gradient as a complex number in the sample's frame) with complex coefficients that depend
 * on the geometry alone, so it is a sparse operator built once per mesh.
 *
 * fc_gradient_coefficients   rowptr (n+1) / col (n_slots) int32: a CSR by QUERY sample; logMag, logAng (n_slots) float32 in slot
 *         order: slot e of row a holds the polar coordinates of log_a(col[e]) in a's frame; w (n) float32, the integration weights,
 *         or NULL for 1.  With p_e = fl(m_e * cosf(theta_e)), q_e = fl(m_e * sinf(theta_e)), omega_e = w[col[e]]:
 *           active   slot e iff m_e > 0 and finite, theta_e finite, col[e] in [0, n), omega_e > 0 and finite.  An inactive slot (a
 *                    row [a, a], a zero-weight neighbour) takes part in no sum, reads nothing out of range, and has coef = 0 exactly.
 *           moments  A11 = sum omega p p, A12 = sum omega p q, A22 = sum omega q q over the active slots, det = A11 A22 - A12 A12,
 *                    tr = A11 + A22.  valid[a] = 1 iff det > rcond tr tr (rcond rounded once to float32; det / tr^2 <= 1/4 bounds
 *                    the ratio of the two eigenvalues of the fit), else 0.
 *           coef[e]  = (omega_e / det) ((A22 p_e - A12 q_e) + i (A11 q_e - A12 p_e)) on a valid row, diag[a] = sum_e coef[e].  On an
 *                    invalid row (empty, one neighbour, collinear neighbours, a NaN among the sums) every coef and diag are 0.
 *         coef (n_slots) and diag (n) complex64 (interleaved), valid (n) uint8.  One wavefront owns one row.  Every sum runs in this
 *         order, fixed by the row's length alone: lane l adds the terms of slots e0 + l, e0 + l + 64, ... to a zero in ascending
 *         order, then the 64 partial sums are folded p[l] += p[l + 32], p[l] += p[l + 16], ..., p[0] += p[1].  Every operation is a
 *         float32 operation rounded on its own; cosf and sinf are the device library's, so the result is accurate to a few units in
 *         the last place of p and q and NOT bit-exact against another library.  0 <= rcond <= 1, else FC_ERR_BAD_ARGUMENT.
 * fc_gradient_apply          x (n, C) real, y (n, C) complex (interleaved), dtype FC_F32 (coef complex64) / FC_F64 (coef complex128:
 *         the CALLER casts the coefficients to x's scalar type):  y[a, c] = sum_e coef[e] * fl(x[col[e], c] - x[a, c]) over the slots
 *         of row a, added to a zero in ascending slot order.  A constant x gives exactly 0; a row without slots is written as zero.
 * fc_gradient_adjoint        on the TRANSPOSED CSR rowptr_t (n+1) / col_t (n_slots; the query row of a slot) / coef_t (n_slots), and
 *         diag (n): g (n, C) complex, gx (n, C) real,
 *           gx[i, c] = so[i] * ((sum_t Re(conj(coef_t[t]) si[col_t[t]] g[col_t[t], c])) - Re(conj(diag[i]) si[i] g[i, c]))
 *         the t sum added to a zero in ascending transposed-slot order.  scale_in = si and scale_out = so are (n) real of g's scalar
 *         type or NULL for 1: si multiplies g's rows as they are read, so the result's rows.  With si = w and so = -1 / w this is
 *         the divergence -W^-1 G^T W in one launch.
 * apply / adjoint: one launch each; one lane owns one piece of an output row (two channels in float32 when C is even and x, y (g, gx)
 * lie on 8-byte boundaries, else one), the lanes across one source row are contiguous.  rowptr entries are clamped to [0, n_slots]
 * and to the row's own start; a slot whose col lies outside [0, n) contributes nothing and reads nothing out of range.  C >= 1 is
 * arbitrary.  Entries are aligned as in the max-pooling section (not checked).  No atomics: the same bits on every run.  No workspace,
 * no allocation or synchronisation inside. */
int fc_gradient_coefficients(const int32_t* rowptr, const int32_t* col, const float* logMag, const float* logAng, const float* w, double rcond,
                             int32_t n, int32_t n_slots, void* coef, void* diag, uint8_t* valid, void* stream);
int fc_gradient_apply(const void* x, const int32_t* rowptr, const int32_t* col, const void* coef, int32_t n, int32_t n_slots, int32_t C,
                      int32_t dtype, void* y, void* stream);
int fc_gradient_adjoint(const void* g, const int32_t* rowptr_t, const int32_t* col_t, const void* coef_t, const void* diag,
                        const void* scale_in, const void* scale_out, int32_t n, int32_t n_slots, int32_t C, int32_t dtype, void* gx,
                        void* stream);

/* ---- heat diffusion of sample features: connection Laplacian and on-device CG (csrc/fc_diffusion.hip) ---------------------------- *
 * The stiffness matrix S = 1/2 D^H C D of the support graph, (D v)[e] = v[b] - u_e v[a] for a row e = [a, b] with transport u_e, as a
 * merged CSR of 2 E entries: row i holds one entry per row [i, b] (col b, the OUT entries, in ascending e), then one per row [a, i]
 * (col a, the IN entries, in ascending e).  The caller lays the pattern out; edge[k] is e for an in entry and -e - 1 for an out entry.
 *
 * fc_diffusion_coefficients   rowptr (n+1), col, edge (n_entries) int32; logMag (n_edges) float32; xp (n_edges) complex64; w (n) float32
 *         or NULL for 1; h > 0.  four_h = fl32(4 h) and norm = fl32(4 pi h^2) are rounded once from double.  A row e is ACTIVE iff
 *         a != b, m_e = logMag[e] is finite and > 0, xp[e] is finite, w_a and w_b are finite and > 0.  On an active row
 *           c_e = ((w_a * w_b) * expf(-((m_e * m_e) / four_h))) / norm,   g_e = -0.5 * c_e
 *           coef = (g_e Re u_e, -(g_e Im u_e)) for the out entry and (g_e Re u_e, g_e Im u_e) for the in entry;  coef_real = g_e
 *         and on an inactive one both are exactly 0 (its entries stay in the pattern).  Per row, over its active entries in entry order,
 *         added to a zero:  diag[i] = 0.5 * sum (c_e * (Re u_e Re u_e + Im u_e Im u_e) for an out entry, c_e for an in entry),
 *         diag_real[i] = 0.5 * sum c_e.  coef (n_entries) complex64, coef_real (n_entries), diag, diag_real (n) float32.  Every
 *         operation is a float32 operation rounded on its own; expf is the device library's: accurate to a few units in the last
 *         place, NOT bit-exact against another library.  The two entries of a row are exact conjugates: S is Hermitian to the bit.
 *         One thread per row of the matrix, one launch, no atomics.
 * fc_diffusion_apply          x, y (n, C) of dtype FC_F32 / FC_F64, is_complex 1 (interleaved pairs; coef complex) or 0 (coef real);
 *         coef, diag, scale_in, scale_out in x's scalar type (the CALLER casts):
 *           y[i, c] = so[i] * ((sum_k coef[k] * (si[col[k]] * x[col[k], c])) + diag[i] * (si[i] * x[i, c]))
 *         the k sum over the row's entries added to a zero in entry order; si, so (n) or NULL for 1.  so = -1 / w is the Laplacian
 *         -W^-1 S, si = -1 / w its adjoint.  One lane per (row, channel), one launch, no atomics.
 * fc_diffusion_solve          per mesh b (rows ptr[b] .. ptr[b+1] - 1; ptr (B+1) int64 DEVICE memory, or NULL: B = 1, all n rows) and
 *         channel c, exactly `iters` (1 .. 1024) steps of Jacobi-preconditioned conjugate gradients on (W + t_c S) y = rhs:
 *           mode 0   rhs = W x,  y0 = x,  out = y              mode 1   rhs = x,  y0 = x / w (0 where w <= 0),  out = W y,  lam = y
 *           P_i = w_i + t_c d_i                  (z = r / P where P > 0, else 0)
 *           r0 = rhs - (W + t S) y0      z0 = r0 / P      p0 = z0      rz = Re<r0, z0>
 *           repeat iters times:
 *               q = (W + t S) p                  pq = Re<p, q>
 *               alpha = rz / pq if pq > 0 else 0
 *               y += alpha p      r -= alpha q      (both skipped when alpha == 0)      z = r / P
 *               rz' = Re<r, z>    beta = rz' / rz if rz > 0 else 0
 *               p = z + beta p    rz = rz'
 *         with ((W + t S) v)[i] = w_i v_i + t_c ((sum_k coef[k] v[col[k]]) + d_i v_i), the k sum as in apply.  Vectors and every
 *         operation on them are in x's scalar type, each rounded on its own; alpha and beta are double quotients rounded once.  The
 *         inner products are double: thread l of 1024 adds the terms of the mesh's rows l, l + 1024, ... in ascending order to a
 *         zero, the 64 lanes of a wavefront are folded v[l] += v[l + 32], v[l + 16], ..., v[l + 1], and the 16 wavefronts' sums are
 *         added in index order.  t (C) in x's scalar type: t_c = 0 gives out = x bit for bit (mode 0); a negative or non-finite t_c
 *         gives NaN in column c of out, lam and resid and touches nothing else.  resid (B, C) in x's scalar type or NULL: sqrt(rz) at
 *         exit.  lam (n, C) or NULL.
 *         One launch: a workgroup of 1024 threads owns one mesh and 16 bytes of a row (4 float32, 2 float64 / complex64 or
 *         1 complex128 channel) through all iterations.  The search direction p lives in LDS when max_rows <= fc_diffusion_lds_rows()
 *         and where == 0, else (where == 1 forces it) in the workspace; the loop and the bits are the same.  max_rows: the largest
 *         mesh (n without ptr); a range that ptr makes longer is cut to it.  No atomics, no cooperative launch, nothing waits on another workgroup.  Entries whose col lies
 *         outside the row's mesh contribute nothing.  Workspace: the query below; FC_ERR_WORKSPACE when missing or smaller.
 * fc_diffusion_time_gradient  gt[c] = -sum_b (sum over the rows i of mesh b of Re(conj(lam[i, c]) sy[i, c])), in double and in a
 *         fixed order (thread (j, l) of 16 x 64 adds the rows j, j + 16, ... of a channel, the 16 sums are added in index order,
 *         then the meshes in index order), rounded once to x's scalar type.  Two launches.  Workspace: 8 B C bytes rounded up to 256.
 * No allocation or synchronisation inside. */
int32_t fc_diffusion_lds_rows(void);
int fc_diffusion_coefficients(const int32_t* rowptr, const int32_t* col, const int32_t* edge, const float* logMag, const void* xp,
                              const float* w, double h, int32_t n, int32_t n_edges, int32_t n_entries, void* coef, float* coef_real,
                              float* diag, float* diag_real, void* stream);
int fc_diffusion_apply(const void* x, const int32_t* rowptr, const int32_t* col, const void* coef, const void* diag, const void* scale_in,
                       const void* scale_out, int32_t n, int32_t n_entries, int32_t C, int32_t dtype, int32_t is_complex, void* y,
                       void* stream);
size_t fc_diffusion_workspace_bytes(int32_t n, int32_t B, int32_t C, int32_t dtype, int32_t is_complex, int32_t max_rows, int32_t where);
int fc_diffusion_solve(const void* x, const void* t, const void* w, const void* diag, const int32_t* rowptr, const int32_t* col,
                       const void* coef, const int64_t* ptr, int32_t n, int32_t n_entries, int32_t B, int32_t C, int32_t max_rows,
                       int32_t dtype, int32_t is_complex, int32_t iters, int32_t mode, int32_t where, void* y, void* lam, void* resid,
                       void* workspace, size_t workspace_bytes, void* stream);
int fc_diffusion_time_gradient(const void* lam, const void* sy, const int64_t* ptr, int32_t n, int32_t B, int32_t C, int32_t dtype,
                               int32_t is_complex, void* gt, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FIELDCONV_HIP_H */
