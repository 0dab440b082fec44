// Path-traced light on the exported surface (esr_nerf_amd/sources.py: path_light, lit_view(paths=)).  Section X of
// include/esr_hip.h is the definition; tests/surfpath_ref.py restates it.
//
// The reference's light-transport stage is a one-sample path tracer in the volume (app/utils/pbr/functions.py:10-18,
// diffuse_scattering: a uniform random unit vector flipped into the normal's hemisphere, weighted by the Disney reflection with its
// (n . wi) 2 pi).  This kernel chains that estimator on the mesh: the stack-less walk (bvh_walk.h), the BRDF (disney.h), the
// environment (sg_env.h) and the sources as point lights (section U's per-slot term), with the path's vertex and throughput in
// registers.
//
// One kernel body (surfpath_body.h, shared with surfpath_is.hip; this file holds the draw), two instantiations (reflect /
// irradiance at the first vertex).  Kd adjacent lanes form the group of one point: lane k holds the paths k, k + Kd, ...  A wave
// holds 64 / Kd points, a block of 256 lanes 256 / Kd; the blocks stride over the points.  A lane reads its point at the start of
// every path (not kept over the paths: its 18 registers are a wave a SIMD), per segment draws the direction from Philox4x32-10
// (the counter names the point, the path, the segment: no state is kept), multiplies the throughput by the vertex's reflection
// and walks the ray; on a miss it evaluates the environment (the lobe table sits in LDS) and ends the path, on a hit it
// interpolates the next vertex and gathers one random slot of every source through the any-hit walk (next-event estimation).
// The nine sums (component, channel) of the Kd lanes are combined by the xor butterfly of surflight.hip and lane 0 stores.
// Nothing of size P N is written but the optional `trace` and `end`; no atomics, no scratch.
#include "surfpath_body.h"

namespace {

// Section X's draw: uniform on the sphere, flipped into the normal's hemisphere, weighted by the vertex's reflection
struct UniformDraw {
    static constexpr int STRIDE = 2;
    static constexpr bool TAKE_ANEW = false;
    static constexpr double kTwoPi = 2.0 * 3.14159265358979323846;
    static __device__ __forceinline__ int segment(PathVertex &v, bool first_of_mode1, uint32_t ctr0, int s, int b, KernArgs kr, double w_out[3], float wi_out[3])
    {
#pragma clang fp contract(off)
        // (drawn and flipped in locals: through the pointers the flip turns a dot product of disney_eval's around -- FRAGILE, see body)
        double w[3];
        float wi[3];
        // Marsaglia's lift of the disc pair to the sphere, binary64 (no pair among the candidates: its zeros lift to (0, 0, 1))
        double a1, a2, sd;
        disc_pair<true>(ctr0, (uint32_t)s, (uint32_t)(STRIDE * b), kr->key0, kr->key1, a1, a2, sd);
        const double q = __dsqrt_rn(1.0 - sd);
        w[0] = (2.0 * a1) * q, w[1] = (2.0 * a2) * q, w[2] = 1.0 - 2.0 * sd;
#pragma unroll
        for (int i = 0; i < 3; ++i) wi[i] = (float)w[i];
        const float sf = (wi[0] * v.n[0] + wi[1] * v.n[1]) + wi[2] * v.n[2];
        if (sf < 0.f) {
#pragma unroll
            for (int i = 0; i < 3; ++i) w[i] = -w[i], wi[i] = -wi[i];
        }
        if (first_of_mode1) {
            const double cos_x = ((double)v.n[0] * (double)wi[0] + (double)v.n[1] * (double)wi[1]) + (double)v.n[2] * (double)wi[2];
            const double wt = cos_x * kTwoPi;
#pragma unroll
            for (int c = 0; c < 3; ++c) v.T[c] = v.T[c] * wt;
        } else {
            const Disney R = disney_eval(v.base, v.rough, v.metal, v.n, wi, v.wo);
#pragma unroll
            for (int c = 0; c < 3; ++c) v.T[c] = v.T[c] * (double)R.R[c];
        }
        for (int i = 0; i < 3; ++i) w_out[i] = w[i], wi_out[i] = wi[i];
        return 0;
    }
};

__global__ void __launch_bounds__(SP_THREADS) surfpath_reflect_kernel(PathArgs) { surface_path<0, UniformDraw>(); }
__global__ void __launch_bounds__(SP_THREADS) surfpath_irradiance_kernel(PathArgs) { surface_path<1, UniformDraw>(); }

}  // namespace

ESR_API int esr_surface_path(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                             const int64_t *triangles, const float *v_normal, const float *v_base, const float *v_rough,
                             const float *v_metal, int64_t n_sources, int32_t slots, const double *l_point, const double *l_normal,
                             const double *l_weight, const float *l_radiance, const int32_t *l_face, double eps, const float *mus,
                             const float *lambdas, const float *lobes, int32_t n_sg, int64_t n_points, const double *p_point,
                             const float *p_normal, const int32_t *p_face, const float *p_base, const float *p_rough,
                             const float *p_metal, const float *p_wo, int32_t mode, int32_t n_paths, int32_t depth, double t_min,
                             int64_t seed, int64_t point_base, float *out, int32_t *n_open, int32_t *trace, uint8_t *end,
                             void *stream)
{
    const PathArgs a{nodes, n_faces, vertices, n_vertices, triangles, v_normal, v_base, v_rough, v_metal, n_sources, l_point, l_normal,
                     l_weight, l_radiance, l_face, eps, 1.0 - eps, mus, lambdas, lobes, n_points, p_point, p_normal, p_face, p_base,
                     p_rough, p_metal, p_wo, t_min, point_base, out, n_open, trace, end, (uint32_t)((uint64_t)seed & 0xFFFFFFFFu),
                     (uint32_t)((uint64_t)seed >> 32), n_sg, n_paths, depth, /* rr_start: no roulette here, unread */ 1, 0, 0, 0};
    return path_launch(a, slots, mode, stream, surfpath_reflect_kernel, surfpath_irradiance_kernel);
}
