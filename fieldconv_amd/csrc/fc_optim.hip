// Fused Adam over one flat parameter buffer: the segmentation network has ~60 parameter tensors with
// ~1 M entries in total; torch's multi-tensor Adam is a dozen launches of list kernels (0.5 ms per step at config 3, a
// quarter of the whole forward + backward), this is two: a one-thread tick of the device-side step counter (so that the
// step is capturable in a HIP graph: nothing step-dependent comes from the host) and one elementwise update with the
// arithmetic of torch.optim.Adam (L2 weight decay, no amsgrad):
//   g' = g + wd p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//
// fc_adam_step_ctl is the same update with controls that a captured step can steer from the device: the learning rate in a device
// float, global-norm gradient clipping, a step that a non-finite gradient skips, decoupled weight decay (AdamW) and an exponential
// moving average of the parameters.  Three launches, no atomics, no host synchronisation (include/fieldconv_hip.h has the formulas
// and the order of every addition): partial sums of squares -> finalize and tick -> update.
#include "fc_common.hpp"
#include "fc_kernels.hpp"
#include "fc_workspace.hpp"

namespace fc {

__global__ void adam_tick_kernel(float* __restrict__ step) { step[0] += 1.f; }

__global__ __launch_bounds__(256) void adam_update_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                          float4* __restrict__ v, const float* __restrict__ step, size_t n4, float lr,
                                                          float b1, float b2, float eps, float wd) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    const float t = step[0];
    const float bc1 = 1.f - powf(b1, t), bc2_sqrt = sqrtf(1.f - powf(b2, t));
    const float step_size = lr / bc1;
    float4 pp = p[idx], mm = m[idx], vv = v[idx];
    const float4 gg = g[idx];
    float* pa = reinterpret_cast<float*>(&pp);
    float* ma = reinterpret_cast<float*>(&mm);
    float* va = reinterpret_cast<float*>(&vv);
    const float* ga = reinterpret_cast<const float*>(&gg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gk = ga[k] + wd * pa[k];
        ma[k] = b1 * ma[k] + (1.f - b1) * gk;
        va[k] = b2 * va[k] + (1.f - b2) * gk * gk;
        pa[k] -= step_size * (ma[k] / (sqrtf(va[k]) / bc2_sqrt + eps));
    }
    p[idx] = pp;
    m[idx] = mm;
    v[idx] = vv;
}

// ---- the step with controls --------------------------------------------------------------------------------------------------
constexpr int ADAM_THREADS = 256;                                   // every kernel below: 4 wavefronts
constexpr int ADAM_SQ_ROUNDS = 4;                                   // float4 per thread in the sum of squares
constexpr size_t ADAM_SQ_CHUNK = (size_t)ADAM_THREADS * ADAM_SQ_ROUNDS;     // float4 per workgroup there: 1024 (4096 floats)

inline size_t adam_partials(size_t n) { return (n / 4 + ADAM_SQ_CHUNK - 1) / ADAM_SQ_CHUNK; }

// workspace: gate {coef, skip (0 or 1)} as two floats | one double per workgroup of the sum of squares
struct AdamCtlWorkspace { float* gate; double* partial; };
inline AdamCtlWorkspace adam_ctl_workspace(Carver& c, size_t n) {
    return {c.take<float>(2 * sizeof(float)), c.take<double>(adam_partials(n) * sizeof(double))};
}

// Workgroup b sums the squares of the float4 [b CHUNK, (b+1) CHUNK) of g: thread t takes b CHUNK + r 256 + t for r = 0..3 in that
// order, ((x^2 + y^2) + z^2) + w^2 of each added to its running double; then block_sum (xor tree per wavefront, wavefronts in index
// order).  Every product of two floats is exact in double, whether or not the compiler fuses it into the addition.
__global__ __launch_bounds__(ADAM_THREADS) void adam_sumsq_kernel(const float4* __restrict__ g, size_t n4, double* __restrict__ partial) {
    __shared__ double slots[ADAM_THREADS / 64];
    const size_t base = (size_t)blockIdx.x * ADAM_SQ_CHUNK + threadIdx.x;
    double acc = 0;
#pragma unroll
    for (int r = 0; r < ADAM_SQ_ROUNDS; ++r) {
        const size_t idx = base + (size_t)r * ADAM_THREADS;
        if (idx < n4) {
            const float4 q = g[idx];
            const double x = q.x, y = q.y, z = q.z, w = q.w;
            acc += ((x * x + y * y) + z * z) + w * w;
        }
    }
    const double s = block_sum<ADAM_THREADS / 64>(acc, slots);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup: thread t adds partials t, t + 256, ... in that order, then block_sum; thread 0 decides and ticks.  nparts == 0:
// neither the norm nor the skip is wanted, the launch only ticks.
__global__ __launch_bounds__(ADAM_THREADS) void adam_finalize_kernel(const double* __restrict__ partial, size_t nparts, float* __restrict__ gate,
                                                                     float* __restrict__ step, float* __restrict__ stats, float max_norm,
                                                                     int skip_nonfinite) {
    __shared__ double slots[ADAM_THREADS / 64];
    double acc = 0;
    for (size_t i = threadIdx.x; i < nparts; i += ADAM_THREADS) acc += partial[i];
    const double S = block_sum<ADAM_THREADS / 64>(acc, slots);
    if (threadIdx.x != 0) return;
    const double norm_d = sqrt(S);
    const bool skip = skip_nonfinite && !isfinite(S);
    float coef = 1.f;
    if (max_norm > 0.f) {                      // torch's clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1), a NaN stays a NaN
        const double c = (double)max_norm / (norm_d + 1e-6);
        coef = (float)(c > 1.0 ? 1.0 : c);
    }
    if (!skip) step[0] += 1.f;
    gate[0] = coef;
    gate[1] = skip ? 1.f : 0.f;
    stats[0] = (float)norm_d;
    stats[1] = coef;
    stats[2] = skip ? 1.f : 0.f;
    stats[3] += skip ? 1.f : 0.f;
}

// A value the compiler may not fuse into the arithmetic around it: the scaled gradient and the decayed parameter enter the
// expressions of adam_update_kernel as its loaded g and p do, so that those expressions contract exactly as they do there.
__device__ __forceinline__ float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}

// adam_update_kernel's expressions in its order, with lr, coef and skip read from device memory.  DECOUPLED: p (1 - lr wd) first
// and no L2 term; EMA: e = d e + (1 - d) p_new.  <false, false> with coef == 1 gives adam_update_kernel's bits.
template <bool DECOUPLED, bool EMA>
__global__ __launch_bounds__(ADAM_THREADS) void adam_update_ctl_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                                       float4* __restrict__ v, float4* __restrict__ ema,
                                                                       const float* __restrict__ step, const float* __restrict__ lr_ptr,
                                                                       const float* __restrict__ gate, size_t n4, float b1, float b2, float eps,
                                                                       float wd, float ema_decay) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4 || gate[1] != 0.f) return;
    const float t = step[0], lr = lr_ptr[0], coef = gate[0];
    const float bc1 = 1.f - powf(b1, t), bc2_sqrt = sqrtf(1.f - powf(b2, t));
    const float step_size = lr / bc1;
    const float keep = 1.f - lr * wd;
    float4 pp = p[idx], mm = m[idx], vv = v[idx];
    const float4 gg = g[idx];
    float* pa = reinterpret_cast<float*>(&pp);
    float* ma = reinterpret_cast<float*>(&mm);
    float* va = reinterpret_cast<float*>(&vv);
    const float* ga = reinterpret_cast<const float*>(&gg);
    float4 ee;
    float* ea = reinterpret_cast<float*>(&ee);
    if constexpr (EMA) ee = ema[idx];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gs = rounded(coef * ga[k]);
        float gk;
        if constexpr (DECOUPLED) {
            pa[k] = rounded(pa[k] * keep);
            gk = gs;
        } else {
            gk = gs + wd * pa[k];
        }
        ma[k] = b1 * ma[k] + (1.f - b1) * gk;
        va[k] = b2 * va[k] + (1.f - b2) * gk * gk;
        pa[k] -= step_size * (ma[k] / (sqrtf(va[k]) / bc2_sqrt + eps));
        if constexpr (EMA) ea[k] = ema_decay * ea[k] + (1.f - ema_decay) * pa[k];
    }
    p[idx] = pp;
    m[idx] = mm;
    v[idx] = vv;
    if constexpr (EMA) ema[idx] = ee;
}

}  // namespace fc

extern "C" {

int fc_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step, size_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || (n & 3)) return FC_ERR_BAD_ARGUMENT;
    if (n == 0) return FC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(fc::adam_tick_kernel, dim3(1), dim3(1), 0, s, step);
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(fc::adam_update_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(params),
                       reinterpret_cast<const float4*>(grads), reinterpret_cast<float4*>(exp_avg), reinterpret_cast<float4*>(exp_avg_sq),
                       step, n4, lr, beta1, beta2, eps, weight_decay);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

size_t fc_adam_ctl_workspace_bytes(size_t n) { return fc::carved_bytes(fc::adam_ctl_workspace, n); }

int fc_adam_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, float* step, const float* lr,
                     float* stats, void* workspace, size_t workspace_bytes, size_t n, const fc_adam_ctl* ctl, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !lr || !stats || !ctl || (n & 3)) return FC_ERR_BAD_ARGUMENT;
    const bool with_ema = ctl->ema_decay >= 0.f;
    if (with_ema && (!ema || !(ctl->ema_decay < 1.f))) return FC_ERR_BAD_ARGUMENT;
    if (n == 0) return FC_OK;
    if (!workspace || workspace_bytes < fc_adam_ctl_workspace_bytes(n)) return FC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    fc::Carver c(workspace);
    const fc::AdamCtlWorkspace ws = fc::adam_ctl_workspace(c, n);
    const size_t n4 = n / 4;
    const bool norm_wanted = ctl->max_norm > 0.f || ctl->skip_nonfinite;
    const size_t nparts = norm_wanted ? fc::adam_partials(n) : 0;
    if (norm_wanted)
        hipLaunchKernelGGL(fc::adam_sumsq_kernel, dim3((unsigned)nparts), dim3(fc::ADAM_THREADS), 0, s, reinterpret_cast<const float4*>(grads), n4,
                           ws.partial);
    hipLaunchKernelGGL(fc::adam_finalize_kernel, dim3(1), dim3(fc::ADAM_THREADS), 0, s, ws.partial, nparts, ws.gate, step, stats, ctl->max_norm,
                       (int)(ctl->skip_nonfinite != 0));
    const dim3 grid((unsigned)((n4 + fc::ADAM_THREADS - 1) / fc::ADAM_THREADS)), block(fc::ADAM_THREADS);
    auto update = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, reinterpret_cast<float4*>(params), reinterpret_cast<const float4*>(grads),
                           reinterpret_cast<float4*>(exp_avg), reinterpret_cast<float4*>(exp_avg_sq), reinterpret_cast<float4*>(ema), step, lr,
                           ws.gate, n4, ctl->beta1, ctl->beta2, ctl->eps, ctl->weight_decay, ctl->ema_decay);
    };
    if (ctl->decoupled)
        with_ema ? update(fc::adam_update_ctl_kernel<true, true>) : update(fc::adam_update_ctl_kernel<true, false>);
    else
        with_ema ? update(fc::adam_update_ctl_kernel<false, true>) : update(fc::adam_update_ctl_kernel<false, false>);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // extern "C"
