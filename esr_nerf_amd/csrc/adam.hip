// Fused Adam step -- replaces the ~10 dense elementwise torch passes per parameter tensor of
// app/utils/optimizer.py:183-228 (`adam`), including the optional per-voxel learning rate
// (optimizer.py:98-100, 224-225).
//
// One streaming pass: reads p, g, m, v (+ per_lr), writes p, m, v -- 28 B per parameter, HBM-bound
// (C2: 54.6 M parameters -> 1.5 GB -> ~0.3 ms at HBM rate, where the reference's op chain moves ~10x
// that).  16-byte accesses when everything is 16-byte aligned.  Arithmetic order follows the
// reference line by line: m = m*b1 + g*(1-b1); v = v*b2 + (g*g)*(1-b2);
// denom = sqrt(v)/sqrt(bc2) + eps; p += (-lr/bc1) * (m [* per_lr] / denom), each op rounded separately.
//
// Live-brick form (esr_adam_step_live; DESIGN section 4 "Live-brick Adam").  With g == 0, m == 0, v == 0, no weight
// decay, eps > 0 and a finite per_lr the lines above give m' = 0, v' = 0 and p' = p + neg_step * (0 / eps) = p: the
// update is the identity.  The tensor is cut into the 512-B bricks of brick.hip; a brick is LIVE once a gradient of it
// was non-zero (or its loaded moments are) and stays live, since its moments keep decaying.  Dead bricks with an
// all-zero gradient are skipped after the gradient read: 4 B per parameter instead of 28, with the same bytes in
// p, m and v as the dense kernel.  The pass can also zero the gradient bricks it found non-zero, which replaces the
// trainer's memset of the whole buffer.
#include "esr_common.h"

namespace {

struct AdamParams {
    float *p, *m, *v;
    const float *g, *per_lr;
    int64_t n;
    float beta1, beta2, eps, weight_decay;
    float one_m_b1, one_m_b2, sqrt_bc2, neg_step;
};

__device__ __forceinline__ void adam1(const AdamParams &A, float &p, float g, float &m, float &v, float plr, bool has_plr)
{
#pragma clang fp contract(off)
    if (A.weight_decay != 0.f) g = g + p * A.weight_decay;
    m = m * A.beta1 + g * A.one_m_b1;
    v = v * A.beta2 + (g * g) * A.one_m_b2;
    const float denom = __fdiv_rn(sqrtf(v), A.sqrt_bc2) + A.eps;
    const float num = has_plr ? m * plr : m;
    p = p + A.neg_step * __fdiv_rn(num, denom);
}

template <bool VEC>
__global__ void __launch_bounds__(256) adam_kernel(AdamParams A)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool has = A.per_lr != nullptr;
    if (VEC) {
        const int64_t n4 = A.n >> 2;
        for (int64_t i = tid; i < n4; i += stride) {
            float4 p = reinterpret_cast<float4 *>(A.p)[i], m = reinterpret_cast<float4 *>(A.m)[i],
                   v = reinterpret_cast<float4 *>(A.v)[i];
            const float4 g = reinterpret_cast<const float4 *>(A.g)[i];
            float4 l = {1.f, 1.f, 1.f, 1.f};
            if (has) l = reinterpret_cast<const float4 *>(A.per_lr)[i];
            adam1(A, p.x, g.x, m.x, v.x, l.x, has);
            adam1(A, p.y, g.y, m.y, v.y, l.y, has);
            adam1(A, p.z, g.z, m.z, v.z, l.z, has);
            adam1(A, p.w, g.w, m.w, v.w, l.w, has);
            reinterpret_cast<float4 *>(A.p)[i] = p;
            reinterpret_cast<float4 *>(A.m)[i] = m;
            reinterpret_cast<float4 *>(A.v)[i] = v;
        }
        for (int64_t i = (n4 << 2) + tid; i < A.n; i += stride) {
            float p = A.p[i], m = A.m[i], v = A.v[i];
            adam1(A, p, A.g[i], m, v, has ? A.per_lr[i] : 1.f, has);
            A.p[i] = p; A.m[i] = m; A.v[i] = v;
        }
    } else {
        for (int64_t i = tid; i < A.n; i += stride) {
            float p = A.p[i], m = A.m[i], v = A.v[i];
            adam1(A, p, A.g[i], m, v, has ? A.per_lr[i] : 1.f, has);
            A.p[i] = p; A.m[i] = m; A.v[i] = v;
        }
    }
}

// ---- live bricks ----------------------------------------------------------------------------------------------------
constexpr int BRICK = 128;           // floats per brick (32 lanes x float4), as brick.hip
constexpr int QUAD = 4;              // consecutive bricks per 32-lane group and trip: 4 gradient loads in flight, 4 flags = one dword

__device__ __forceinline__ bool any_nz(const float4 &g)
{
    return (g.x != 0.f) | (g.y != 0.f) | (g.z != 0.f) | (g.w != 0.f);         // by value: -0.0 is zero
}

// true in every lane of the 32-lane group when `c` holds in one of them
__device__ __forceinline__ bool group_any(bool c)
{
    const unsigned long long m = __ballot(c);
    return ((threadIdx.x & 32) ? (unsigned)(m >> 32) : (unsigned)m) != 0u;
}

// One 32-lane group per quad of bricks.  The four gradient loads and the flag dword are issued before the first branch;
// a dead brick with a zero gradient costs nothing more.  The bricks that need the update then take it one after the
// other: one copy of the arithmetic, and the brick's gradient is read a second time there -- it reached this XCD's L2 a
// moment ago, so HBM sees it once -- instead of holding four bricks' gradients in registers across the update, which
// would not leave registers for 8 waves per SIMD.  What lies behind the last whole quad -- up to three whole bricks and
// a ragged one -- is taken value by value by the group whose turn it would be.
// No LDS, no communication between groups: every byte written depends on the inputs alone.
template <bool ZERO>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
adam_live_kernel(AdamParams A, float *__restrict__ gw, uint8_t *__restrict__ live, int64_t n_bricks,
                 unsigned long long *__restrict__ stats)
{
    const int sub = threadIdx.x & 31;
    const int64_t grp0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 5;
    const int64_t ngrp = ((int64_t)gridDim.x * blockDim.x) >> 5;
    const int64_t full_quads = A.n / (QUAD * BRICK);                 // quads whose four bricks are all whole
    const bool has = A.per_lr != nullptr;
    int n_live = 0, n_nz = 0;                                         // the same in every lane of the group
    for (int64_t q = grp0; q < full_quads; q += ngrp) {
        const int64_t b0 = q * QUAD, e = b0 * BRICK + sub * 4;
        const float4 g0 = *reinterpret_cast<const float4 *>(A.g + e), g1 = *reinterpret_cast<const float4 *>(A.g + e + BRICK),
                     g2 = *reinterpret_cast<const float4 *>(A.g + e + 2 * BRICK),
                     g3 = *reinterpret_cast<const float4 *>(A.g + e + 3 * BRICK);
        const unsigned fl = *reinterpret_cast<const unsigned *>(live + b0);          // live is 16-B aligned, b0 % 4 == 0
        unsigned nzm = 0, was = 0;                                    // bit k: brick b0 + k has a non-zero gradient / is live
        nzm |= (unsigned)group_any(any_nz(g0)) << 0;
        nzm |= (unsigned)group_any(any_nz(g1)) << 1;
        nzm |= (unsigned)group_any(any_nz(g2)) << 2;
        nzm |= (unsigned)group_any(any_nz(g3)) << 3;
#pragma unroll
        for (int k = 0; k < QUAD; ++k) was |= (unsigned)(((fl >> (8 * k)) & 0xffu) != 0u) << k;
        const unsigned todo = nzm | was;
        n_live += __popc(todo);
        n_nz += __popc(nzm);
#pragma unroll 1
        for (int k = 0; k < QUAD; ++k) {
            if (!((todo >> k) & 1u)) continue;
            const int64_t ek = e + (int64_t)k * BRICK;
            const float4 g = *reinterpret_cast<const float4 *>(A.g + ek);      // again, from the L2: see above
            float4 p = *reinterpret_cast<float4 *>(A.p + ek), m = *reinterpret_cast<float4 *>(A.m + ek),
                   v = *reinterpret_cast<float4 *>(A.v + ek);
            float4 l = {1.f, 1.f, 1.f, 1.f};
            if (has) l = *reinterpret_cast<const float4 *>(A.per_lr + ek);
            adam1(A, p.x, g.x, m.x, v.x, l.x, has);
            adam1(A, p.y, g.y, m.y, v.y, l.y, has);
            adam1(A, p.z, g.z, m.z, v.z, l.z, has);
            adam1(A, p.w, g.w, m.w, v.w, l.w, has);
            *reinterpret_cast<float4 *>(A.p + ek) = p;
            *reinterpret_cast<float4 *>(A.m + ek) = m;
            *reinterpret_cast<float4 *>(A.v + ek) = v;
            if (ZERO && ((nzm >> k) & 1u)) *reinterpret_cast<float4 *>(gw + ek) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!((was >> k) & 1u) && sub == 0) live[b0 + k] = 1;
        }
    }
    if (full_quads % ngrp == grp0) {                                  // the tail: bricks [4 * full_quads, n_bricks)
        for (int64_t b = full_quads * QUAD; b < n_bricks; ++b) {
            const int64_t e = b * BRICK + sub * 4;
            bool nz = false;
            for (int64_t i = e; i < min(e + 4, A.n); ++i) nz |= A.g[i] != 0.f;
            nz = group_any(nz);
            const bool was = live[b] != 0;
            if (!(was | nz)) continue;
#pragma unroll 1
            for (int64_t i = e; i < min(e + 4, A.n); ++i) {
                float p = A.p[i], m = A.m[i], v = A.v[i];
                adam1(A, p, A.g[i], m, v, has ? A.per_lr[i] : 1.f, has);
                A.p[i] = p; A.m[i] = m; A.v[i] = v;
                if (ZERO && nz) gw[i] = 0.f;
            }
            if (!was && sub == 0) live[b] = 1;
            n_live += 1;
            n_nz += nz;
        }
    }
    if (stats) {                                                       // one add per wave and counter
        n_live += __shfl_xor(n_live, 32);
        n_nz += __shfl_xor(n_nz, 32);
        if ((threadIdx.x & 63) == 0) {
            if (n_live) atomicAdd(stats + 0, (unsigned long long)n_live);
            if (n_nz) atomicAdd(stats + 1, (unsigned long long)n_nz);
        }
    }
}

__global__ void __launch_bounds__(256) live_from_moments_kernel(const float *__restrict__ m, const float *__restrict__ v,
                                                                int64_t n, int64_t n_bricks, uint8_t *__restrict__ live)
{
    const int sub = threadIdx.x & 31;
    const int64_t grp0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 5;
    const int64_t ngrp = ((int64_t)gridDim.x * blockDim.x) >> 5;
    for (int64_t b = grp0; b < n_bricks; b += ngrp) {
        const int64_t e = b * BRICK + sub * 4;
        bool nz = false;
        if (e + 4 <= n) {
            nz = any_nz(*reinterpret_cast<const float4 *>(m + e)) || any_nz(*reinterpret_cast<const float4 *>(v + e));
        } else {
            for (int64_t i = e; i < n; ++i) nz |= (m[i] != 0.f) | (v[i] != 0.f);
        }
        if (group_any(nz) && sub == 0) live[b] = 1;
    }
}

// host scalars exactly as the python reference forms them (double arithmetic, then one rounding)
int adam_params(AdamParams &A, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *per_lr,
                int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step)
{
    if (n < 0 || step < 1 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return ESR_EINVAL;
    if (n && (!param || !grad || !exp_avg || !exp_avg_sq)) return ESR_EINVAL;
    A = {};
    A.p = param; A.g = grad; A.m = exp_avg; A.v = exp_avg_sq; A.per_lr = per_lr; A.n = n;
    A.beta1 = beta1; A.beta2 = beta2; A.eps = eps; A.weight_decay = weight_decay;
    const double b1 = (double)beta1, b2 = (double)beta2;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    A.one_m_b1 = (float)(1.0 - b1);
    A.one_m_b2 = (float)(1.0 - b2);
    A.sqrt_bc2 = (float)sqrt(bc2);
    A.neg_step = (float)(-((double)lr / bc1));
    return 0;
}

}  // namespace

ESR_API int esr_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                          const float *per_lr, int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int32_t step, void *stream)
{
    AdamParams A;
    if (const int rc = adam_params(A, param, grad, exp_avg, exp_avg_sq, per_lr, n, lr, beta1, beta2, eps, weight_decay, step))
        return rc;
    if (n == 0) return 0;
    const bool vec = ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
                        (uintptr_t)per_lr) & 15u) == 0);
    const int grid = esr_grid_for(vec ? (n + 3) / 4 : n, 256, 256 * 16);
    if (vec) adam_kernel<true><<<grid, 256, 0, esr_stream(stream)>>>(A);
    else adam_kernel<false><<<grid, 256, 0, esr_stream(stream)>>>(A);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_adam_step_live(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const float *per_lr,
                               uint8_t *live, int64_t n, float lr, float beta1, float beta2, float eps, int32_t step,
                               int32_t zero_grad, int64_t *stats, void *stream)
{
    AdamParams A;
    if (const int rc = adam_params(A, param, grad, exp_avg, exp_avg_sq, per_lr, n, lr, beta1, beta2, eps, 0.f, step))
        return rc;
    if (!(eps > 0.f)) return ESR_EINVAL;               // the identity on dead bricks divides 0 by eps
    if (n == 0) return 0;
    if (!live) return ESR_EINVAL;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)per_lr |
         (uintptr_t)live | (uintptr_t)stats) & 15u)
        return ESR_EINVAL;
    const int64_t nb = (n + BRICK - 1) / BRICK;
    const int grid = esr_grid_for((nb + QUAD - 1) / QUAD * 32, 256, 256 * 16);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(stats);
    if (zero_grad) adam_live_kernel<true><<<grid, 256, 0, esr_stream(stream)>>>(A, grad, live, nb, st);
    else adam_live_kernel<false><<<grid, 256, 0, esr_stream(stream)>>>(A, grad, live, nb, st);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_brick_live_from_moments(const float *exp_avg, const float *exp_avg_sq, int64_t n, uint8_t *live,
                                        void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n == 0) return 0;
    if (!exp_avg || !exp_avg_sq || !live || (((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15u)) return ESR_EINVAL;
    const int64_t nb = (n + BRICK - 1) / BRICK;
    live_from_moments_kernel<<<esr_grid_for(nb * 32, 256, 256 * 16), 256, 0, esr_stream(stream)>>>(exp_avg, exp_avg_sq, n,
                                                                                                   nb, live);
    ESR_CHECK_LAUNCH();
    return 0;
}
