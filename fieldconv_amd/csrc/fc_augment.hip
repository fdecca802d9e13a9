// Per-mesh augmentation of a mini-batch of meshes: one random similarity (scale and three rotations) per mesh, drawn on the device
// from the counter-based generator (fc_philox.hpp, stream 2), and its application to the vertices of every mesh in one launch.
//
// draw     mesh b uses block q = b of the draw (seed, step), u_k = (word k >> 8) * 2^-24:
//            s   = lo + (hi - lo) * u_0                       (1, and u_0 unused, without a scale range)
//            a_k = (2 * u_{k+1} - 1) * degrees[k]             k = 0, 1, 2: the angle about axis k, in degrees
//          params[b] = (s, a_0, a_1, a_2): float32 operations, each rounded on its own (contraction off), so numpy gives the same
//          bits.  r_k = a_k * fl32(pi / 180), and M[b] = s Rz(r_2) Ry(r_1) Rx(r_0), the right-handed rotations about the axes
//            Rx = [1 0 0; 0 c -s; 0 s c]    Ry = [c 0 s; 0 1 0; -s 0 c]    Rz = [c -s 0; s c 0; 0 0 1]
//          applied to column vectors: scale, then the rotation about axis 0, then 1, then 2.  sinf / cosf are the device library's,
//          so M is accurate to a few units in the last place, not bit-exact.
// apply    output row r takes vertex v = index[r] (v = r without index) of the mesh b that owns v by pos_ptr:
//            d = p_v - t_b (p_v without t),   out_i = (M_i0 d_0 + M_i1 d_1) + M_i2 d_2      (each operation rounded on its own)
//          An index outside [0, V) gives a row of NaN and reads nothing.
// One launch each, one thread per mesh / per output row, no atomics, no workspace.
#include "../../include/fieldconv_hip.h"
#include "fc_philox.hpp"
#include "fc_segment.hpp"

namespace fc {

constexpr int kAugThreads = 256;

__device__ __forceinline__ float aug_scale(float lo, float hi, float u) {
#pragma clang fp contract(off)          // (plain operators: __fmul_rn / __fadd_rn are header functions that hipcc contracts)
    const float d = hi - lo;
    const float m = d * u;
    return lo + m;
}

__device__ __forceinline__ float aug_angle(float u, float degrees) {
#pragma clang fp contract(off)
    const float t = 2.0f * u;
    const float c = t - 1.0f;
    return c * degrees;
}

__device__ __forceinline__ float aug_dot3(float m0, float m1, float m2, float d0, float d1, float d2) {
#pragma clang fp contract(off)
    const float a = m0 * d0, b = m1 * d1, c = m2 * d2;
    const float ab = a + b;
    return ab + c;
}

__global__ __launch_bounds__(kAugThreads) void mesh_affine_draw_kernel(int B, uint64_t seed, int64_t step, const int64_t* __restrict__ step_ptr,
                                                                       int has_scale, float lo, float hi, float deg0, float deg1, float deg2,
                                                                       float* __restrict__ params, float* __restrict__ M) {
    const int b = blockIdx.x * kAugThreads + threadIdx.x;
    if (b >= B) return;
    const PhiloxBlock w = philox_draw(seed, (uint64_t)b, philox_step(step, step_ptr), kStreamAugment);
    const float s = has_scale ? aug_scale(lo, hi, philox_uniform(w.w[0])) : 1.0f;
    const float a0 = aug_angle(philox_uniform(w.w[1]), deg0), a1 = aug_angle(philox_uniform(w.w[2]), deg1),
                a2 = aug_angle(philox_uniform(w.w[3]), deg2);
    float* p = params + 4 * (size_t)b;
    p[0] = s;
    p[1] = a0;
    p[2] = a1;
    p[3] = a2;
    const float rad = 0.017453292519943295f;          // fl32(pi / 180)
    const float r0 = a0 * rad, r1 = a1 * rad, r2 = a2 * rad;
    const float cx = cosf(r0), sx = sinf(r0), cy = cosf(r1), sy = sinf(r1), cz = cosf(r2), sz = sinf(r2);
    float* m = M + 9 * (size_t)b;
    m[0] = s * (cz * cy);
    m[1] = s * (cz * sy * sx - sz * cx);
    m[2] = s * (cz * sy * cx + sz * sx);
    m[3] = s * (sz * cy);
    m[4] = s * (sz * sy * sx + cz * cx);
    m[5] = s * (sz * sy * cx - cz * sx);
    m[6] = s * -sy;
    m[7] = s * (cy * sx);
    m[8] = s * (cy * cx);
}

__global__ __launch_bounds__(kAugThreads) void mesh_affine_apply_kernel(const float* __restrict__ pos, const int64_t* __restrict__ pos_ptr, int B,
                                                                        int V, const float* __restrict__ M, const float* __restrict__ t,
                                                                        const int64_t* __restrict__ index, int64_t R, float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kAugThreads + threadIdx.x;
    if (r >= R) return;
    const int64_t v = index != nullptr ? index[r] : r;
    float* o = out + 3 * (size_t)r;
    if (v < 0 || v >= (int64_t)V) {
        o[0] = o[1] = o[2] = __builtin_nanf("");
        return;
    }
    const int b = seg_mesh_of_row(pos_ptr, B, V, (int)v);
    const float* p = pos + 3 * (size_t)v;
    float d0 = p[0], d1 = p[1], d2 = p[2];
    if (t != nullptr) {
        d0 -= t[3 * (size_t)b];
        d1 -= t[3 * (size_t)b + 1];
        d2 -= t[3 * (size_t)b + 2];
    }
    const float* m = M + 9 * (size_t)b;
    o[0] = aug_dot3(m[0], m[1], m[2], d0, d1, d2);
    o[1] = aug_dot3(m[3], m[4], m[5], d0, d1, d2);
    o[2] = aug_dot3(m[6], m[7], m[8], d0, d1, d2);
}

}  // namespace fc

extern "C" {

int fc_mesh_affine_draw(int32_t B, uint64_t seed, int64_t step, const int64_t* step_ptr, int32_t has_scale, float scale_lo, float scale_hi,
                        float degrees0, float degrees1, float degrees2, float* params, float* M, void* stream) {
    if (B < 1 || !params || !M || (has_scale != 0 && has_scale != 1)) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::mesh_affine_draw_kernel, dim3((unsigned)((B + fc::kAugThreads - 1) / fc::kAugThreads)), dim3(fc::kAugThreads), 0,
                       static_cast<hipStream_t>(stream), B, seed, step, step_ptr, has_scale, scale_lo, scale_hi, degrees0, degrees1, degrees2,
                       params, M);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_mesh_affine_apply(const float* pos, const int64_t* pos_ptr, int32_t B, int32_t V, const float* M, const float* t, const int64_t* index,
                         int64_t R, float* out, void* stream) {
    if (B < 1 || V < 0 || R < 0 || !pos_ptr || !M || R > (int64_t)2147483647 * fc::kAugThreads) return FC_ERR_BAD_ARGUMENT;
    if (R == 0) return FC_OK;
    if (!out || (V > 0 && !pos)) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::mesh_affine_apply_kernel, dim3((unsigned)((R + fc::kAugThreads - 1) / fc::kAugThreads)), dim3(fc::kAugThreads), 0,
                       static_cast<hipStream_t>(stream), pos, pos_ptr, B, V, M, t, index, R, out);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // extern "C"
