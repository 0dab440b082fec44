// Direct light from the emissive sources of the exported surface (esr_nerf_amd/sources.py: direct_light, lit_view).  Section U
// of include/esr_hip.h is the definition; tests/surflight_ref.py restates it.
//
// The reference has nothing of the kind: its `emo` component is learnt per sample of the volume
// (app/fine/model/esrnerf.py:565-572).  Here the same quantity -- light that left a source and is reflected once by the Disney
// BRDF -- is estimated on the surface from the sources' sample points.
//
// One kernel.  Kp adjacent lanes form the group of one (point, source): lane k holds slot k of the source.  A wave holds
// 64 / Kp points, a block of 256 lanes 256 / Kp; the blocks stride over the points.  A lane
//   loads its point once (position, normal, material, view direction: registers, kept over the loop over the sources),
//   per source forms the geometric term of its slot in binary64, and only where that is not zero
//   walks the shadow segment through bvh_walk.h's any-hit walk and evaluates the BRDF (disney.h, binary32);
//   the three channel terms of the group are then summed by log2(Kp) xor-shuffle steps on doubles -- a butterfly: after
//   the step with distance 2^j every lane holds the sum of its aligned block of 2^(j+1) slots, so the order is the balanced
//   pairwise one of the header whatever the lane (binary64 addition commutes) -- and lane 0 of the group stores.
// The lanes of a group share their origin and aim at one patch: the walk's divergence is that of neighbouring rays.
// Nothing of size P S Kp is written but the optional `seen` bytes; no LDS, no atomics, no scratch.
#include "bvh_walk.h"
#include "disney.h"

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_BLOCKS = 2048;
constexpr double kInv2Pi = 1.0 / (2.0 * 3.14159265358979323846);

struct LightArgs {
    esr_surface_light_t a;
    int lg;                               // log2(slots)
    double tmax;                          // 1 - eps
};

// The walk leaves no scalar register free: bvh.hip's two kernels stand at the hardware's 102 with nothing but the walk in
// them.  So whatever this kernel needs outside the walk -- the points' and lights' pointers, the outputs, the counts -- does
// not live through the walk in scalar registers (the compiler would spill them): it is read from the kernel-argument segment
// again where it is used, a scalar load per point or per source.  LightArgs is the kernel's only argument and so lies at the
// start of the segment; the empty asm only keeps the compiler from hoisting the loads back out of the loops.
typedef const __attribute__((address_space(4))) LightArgs *KernArgs;

__device__ __forceinline__ KernArgs kernargs()
{
    KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

template <int MODE> __device__ __forceinline__ void surface_light()
{
#pragma clang fp contract(off)
    const KernArgs k0 = kernargs();
    const BvhScene scene{k0->a.nodes, k0->a.n_faces, k0->a.vertices, k0->a.n_vertices, k0->a.triangles};
    const double eps = k0->a.eps, tmax = k0->tmax;
    const int lg = k0->lg, kp = 1 << lg, k = threadIdx.x & (kp - 1);
    const int64_t per_block = SL_THREADS >> lg;
    for (int64_t p = (int64_t)blockIdx.x * per_block + (threadIdx.x >> lg);; p += (int64_t)gridDim.x * per_block) {
        const KernArgs kpt = kernargs();
        if (p >= kpt->a.n_points) break;
        double x[3];
        float n[3], base[3] = {0.f, 0.f, 0.f}, wo[3] = {0.f, 0.f, 0.f}, rough = 0.f, metal = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) x[i] = kpt->a.p_point[3 * p + i], n[i] = kpt->a.p_normal[3 * p + i];
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) base[i] = kpt->a.p_base[3 * p + i], wo[i] = kpt->a.p_wo[3 * p + i];
            rough = kpt->a.p_rough[p], metal = kpt->a.p_metal[p];
        }
        for (int64_t s = 0;; ++s) {
            const KernArgs ks = kernargs();
            if (s >= ks->a.n_sources) break;
            const int64_t slot = s * kp + k;
            const double A = ks->a.l_weight[slot];
            double term[3] = {0.0, 0.0, 0.0};
            double d[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, cos_x = 0.0, G = 0.0;
            int32_t skip = -1;
            bool live = A != 0.0;
            uint8_t seen = 0;
            if (live) {
                double g[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) d[i] = ks->a.l_point[3 * slot + i] - x[i], g[i] = ks->a.l_normal[3 * slot + i];
                skip = ks->a.l_face[slot];
                const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                const double r = __dsqrt_rn(r2);
#pragma unroll
                for (int i = 0; i < 3; ++i) w[i] = d[i] / r;
                const double cos_l = -((g[0] * w[0] + g[1] * w[1]) + g[2] * w[2]);
                cos_x = ((double)n[0] * w[0] + (double)n[1] * w[1]) + (double)n[2] * w[2];
                live = r2 > 0.0 && cos_l > 0.0 && cos_x > 0.0;                // (false for a NaN)
                G = (cos_l * A) / fmax(r2, A);
            }
            if (live) {                                                       // (a silent lane walks nothing)
                // every component of x and d is finite here: one that is not makes r2, and so a cosine, inf or NaN
                Ray ray;
#pragma unroll
                for (int i = 0; i < 3; ++i) ray.o[i] = x[i], ray.d[i] = d[i], ray.inv[i] = 1.0 / d[i];
                ray.tmin = eps;
                Best best{tmax, 0.0, 0.0, -1};
                int n_box = 0, n_tri = 0;
                bvh_walk<true>(scene, ray, true, skip, tmax, best, n_box, n_tri);
                seen = best.face >= 0 ? 2 : 1;
            }
            const KernArgs ko = kernargs();
            if (seen == 1) {
                const float *E = ko->a.l_radiance + 3 * slot;
                if (MODE == 0) {
                    const float wi[3] = {(float)w[0], (float)w[1], (float)w[2]};
                    const Disney R = disney_eval(base, rough, metal, n, wi, wo);
#pragma unroll
                    for (int c = 0; c < 3; ++c) term[c] = (((double)R.R[c] * kInv2Pi) * G) * (double)E[c];
                } else {
                    const double cg = cos_x * G;
#pragma unroll
                    for (int c = 0; c < 3; ++c) term[c] = cg * (double)E[c];
                }
            }
            // the interleaved butterfly of the three channels: every lane of the group is here (its lanes share p and s)
            for (int off = 1; off < kp; off <<= 1) {
                const double t0 = __shfl_xor(term[0], off), t1 = __shfl_xor(term[1], off), t2 = __shfl_xor(term[2], off);
                term[0] = term[0] + t0, term[1] = term[1] + t1, term[2] = term[2] + t2;
            }
            const int64_t ps = p * ko->a.n_sources + s;
            if (k == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ko->a.out[ps * 3 + c] = (float)term[c];
            }
            if (ko->a.seen) ko->a.seen[(ps << lg) + k] = seen;
        }
    }
}

__global__ void __launch_bounds__(SL_THREADS) surflight_reflect_kernel(LightArgs) { surface_light<0>(); }
__global__ void __launch_bounds__(SL_THREADS) surflight_irradiance_kernel(LightArgs) { surface_light<1>(); }

bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
bool given(const void *p, size_t a) { return p && aligned(p, a); }

}  // namespace

ESR_API int esr_surface_light(const esr_surface_light_t *args, void *stream)
{
    if (!args) return ESR_EINVAL;
    const esr_surface_light_t &a = *args;
    if (a.n_faces < 0 || a.n_vertices < 0 || a.n_sources < 0 || a.n_points < 0 || (a.mode != 0 && a.mode != 1) || a.slots < 1 ||
        !(a.eps >= 0.0 && a.eps < 0.5))
        return ESR_EINVAL;
    const int64_t cap = (int64_t)1 << 31;
    if (a.n_faces >= cap || a.n_vertices >= cap || a.n_sources >= cap || a.n_points >= cap || a.slots > ESR_SURFACE_LIGHT_MAX_SLOTS)
        return ESR_ECAP;
    if (a.slots & (a.slots - 1)) return ESR_EINVAL;
    if (!a.n_points || !a.n_sources) return 0;
    if (!given(a.l_point, 8) || !given(a.l_normal, 8) || !given(a.l_weight, 8) || !given(a.l_radiance, 4) || !given(a.l_face, 4) ||
        !given(a.p_point, 8) || !given(a.p_normal, 4) || !given(a.out, 4))
        return ESR_EINVAL;
    if (a.mode == 0 && (!given(a.p_base, 4) || !given(a.p_rough, 4) || !given(a.p_metal, 4) || !given(a.p_wo, 4))) return ESR_EINVAL;
    if (a.n_faces && (!given(a.vertices, 8) || !given(a.triangles, 8))) return ESR_EINVAL;
    if (a.n_faces > 1 && !given(a.nodes, 16)) return ESR_EINVAL;
    LightArgs la{a, 0, 1.0 - a.eps};
    while ((1 << la.lg) < a.slots) ++la.lg;
    const int grid = esr_grid_for(a.n_points, SL_THREADS >> la.lg, SL_BLOCKS);
    if (a.mode == 0) surflight_reflect_kernel<<<grid, SL_THREADS, 0, esr_stream(stream)>>>(la);
    else surflight_irradiance_kernel<<<grid, SL_THREADS, 0, esr_stream(stream)>>>(la);
    ESR_CHECK_LAUNCH();
    return 0;
}
