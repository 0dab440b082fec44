// Importance-sampled path-traced light on the exported surface (esr_nerf_amd/sources.py: path_light(sampling="brdf"),
// lit_view(paths=, sampling="brdf"), bake_irradiance(paths=)).  Section Y of include/esr_hip.h is the definition;
// tests/surfpath_is_ref.py restates it.
//
// surfpath.hip (section X) chains the light-transport stage's estimator: a uniform direction weighted by the Disney reflection.
// This file is that kernel (surfpath_body.h: one loop, one ray per step, the vertex and the throughput in registers, the lobe table
// in LDS, the nine sums combined by the xor butterfly) with another draw: per segment one of two techniques is chosen by the
// vertex's material, a cosine-distributed direction (Malley: the disc pair lifted to the hemisphere) or a half vector from the
// BRDF's own lobe D = exp(kappa (n.h - 1)) / (pi r^2), kappa = 2 / r^2, whose CDF in cos(theta) inverts in closed form; the weight
// divides the reflection by the one-sample balance-heuristic density of both; and from segment rr_start on Russian roulette ends
// a path with the probability its throughput has lost.  The disc rejection already yields an independent (radius^2, angle) pair,
// so neither technique needs trigonometry.  The reference has no such sampler: an addition, as U, W and X's chaining are.
#include "bvh_walk.h"
#include "disney.h"
#include "sg_env.h"
#include "surfpath_body.h"

namespace {

// Section Y's draw: roulette, technique, direction, weight; a path that ends in it has `end` 3 (the roulette) or 4 (no direction)
struct BrdfDraw {
    static constexpr int STRIDE = 4;               // + 2: the technique's and the roulette's words
    static constexpr bool TAKE_ANEW = true;
    static constexpr double kPi64 = 3.14159265358979323846;
    static __device__ __forceinline__ int segment(PathVertex &v, bool first_of_mode1, uint32_t ctr0, int s, int b, KernArgs kr, double w[3], float wi[3])
    {
#pragma clang fp contract(off)
        int dead = 0;
        // the uniforms of the segment: the disc pair, the technique's and the roulette's
        double a1, a2, sd;
        const bool found = disc_pair<false>(ctr0, (uint32_t)s, (uint32_t)(STRIDE * b), kr->key0, kr->key1, a1, a2, sd);
        uint32_t r[4];
        philox(ctr0, (uint32_t)s, (uint32_t)(STRIDE * b + 2), 0u, kr->key0, kr->key1, r);
        const double ut = ((double)r[0] + 0.5) * 0x1p-32, ur = ((double)r[1] + 0.5) * 0x1p-32;
        // the roulette
        {
            const double m = fmax(fmax(v.T[0], v.T[1]), v.T[2]);
            double q = m >= 0.0625 ? (m <= 1.0 ? m : 1.0) : 0.0625;
            q = (m != m || b < kr->rr_start) ? 1.0 : q;
            dead = ur >= q ? 3 : 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) v.T[c] = v.T[c] / q;
        }
        const double nd[3] = {(double)v.n[0], (double)v.n[1], (double)v.n[2]};
        const double wod[3] = {(double)v.wo[0], (double)v.wo[1], (double)v.wo[2]};
        // the technique
        double qs = 0.0;
        if (!first_of_mode1) {
            const double md = (double)v.metal;
            const double ab = (((double)v.base[0] + (double)v.base[1]) + (double)v.base[2]) / 3.0;
            const double Fb = 0.04 * (1.0 - md) + ab * md, db = (1.0 - md) * ab;
            const double sum = Fb + db, r0 = Fb / sum;
            qs = r0 >= 0.125 ? (r0 <= 0.875 ? r0 : 0.875) : 0.125;
            qs = sum > 0.0 ? qs : 0.125;
        }
        const bool lobe = ut < qs;
        const double kappa = 2.0 / fmax((double)v.rough * (double)v.rough, 1e-7);
        const double ek = 1.0 / exp(kappa);                                  // (exp(-kappa); 0 where exp(kappa) overflows)
        // the local vector: the lobe's half vector (cos(theta) by the inverse CDF, the azimuth the pair's) or Malley's
        // direction (the pair lifted to the hemisphere)
        double lx = a1, ly = a2, lz = __dsqrt_rn(1.0 - sd);
        {
            const double sl = found ? sd : 1.0;
            double c = 1.0 + log(sl + (1.0 - sl) * ek) / kappa;
            c = c >= 0.0 ? (c <= 1.0 ? c : 1.0) : 0.0;
            const double sn = __dsqrt_rn((1.0 - c) * (1.0 + c)), rs = __dsqrt_rn(sl);
            lx = lobe ? (a1 * sn) / rs : lx, ly = lobe ? (a2 * sn) / rs : ly, lz = lobe ? c : lz;
        }
        // to the world through the frame of Duff et al.
        double h[3];
        {
            const double sgn = copysign(1.0, nd[2]);
            const double fa = -1.0 / (sgn + nd[2]);
            const double fb = (nd[0] * nd[1]) * fa;
            h[0] = (lx * (1.0 + ((sgn * nd[0]) * nd[0]) * fa) + ly * fb) + lz * nd[0];
            h[1] = (lx * (sgn * fb) + ly * (sgn + (nd[1] * nd[1]) * fa)) + lz * nd[1];
            h[2] = (lx * -(sgn * nd[0]) + ly * -nd[1]) + lz * nd[2];
        }
        {
            // the lobe's direction: wo mirrored at the half vector
            const double oh = (wod[0] * h[0] + wod[1] * h[1]) + wod[2] * h[2];
            dead = (!dead && lobe && !(oh > 0.0)) ? 4 : dead;
            double m[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) m[i] = (2.0 * oh) * h[i] - wod[i];
            const double len = __dsqrt_rn((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) w[i] = lobe ? m[i] / len : h[i];
        }
        const double cos_x = (nd[0] * w[0] + nd[1] * w[1]) + nd[2] * w[2];
        dead = (!dead && !(cos_x > 0.0)) ? 4 : dead;
#pragma unroll
        for (int i = 0; i < 3; ++i) wi[i] = (float)w[i];
        // the weight of the vertex: the reflection over the density of the two techniques at w
        if (first_of_mode1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v.T[c] = v.T[c] * kPi64;
        } else {
            double hv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) hv[i] = w[i] + wod[i];
            const double hl = __dsqrt_rn((hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) hv[i] = hv[i] / hl;
            const double nh = fmax((nd[0] * hv[0] + nd[1] * hv[1]) + nd[2] * hv[2], 0.0);
            const double ohp = (wod[0] * hv[0] + wod[1] * hv[1]) + wod[2] * hv[2];
            // (the densities times 2 pi, which the reflection carries: no constant but the lobe's)
            double ps = ((kappa / (1.0 - ek)) * exp(kappa * (nh - 1.0))) / (4.0 * ohp);
            ps = ohp > 0.0 ? ps : 0.0;
            // (where w + wo cancels, the density would not see the lobe that drew w: such a draw ends the path)
            dead = (!dead && lobe && !(ohp > 0.0)) ? 4 : dead;
            const double pd = qs * ps + (1.0 - qs) * (2.0 * cos_x);
            const Disney R = disney_eval(v.base, v.rough, v.metal, v.n, wi, v.wo);
#pragma unroll
            for (int c = 0; c < 3; ++c) v.T[c] = v.T[c] * ((double)R.R[c] / pd);
        }
        return dead;
    }
};

__global__ void __launch_bounds__(SP_THREADS) surfpath_is_reflect_kernel(PathArgs) { surface_path<0, BrdfDraw>(); }
__global__ void __launch_bounds__(SP_THREADS) surfpath_is_irradiance_kernel(PathArgs) { surface_path<1, BrdfDraw>(); }

}  // namespace

ESR_API int esr_surface_path_is(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                                const int64_t *triangles, const float *v_normal, const float *v_base, const float *v_rough,
                                const float *v_metal, int64_t n_sources, int32_t slots, const double *l_point,
                                const double *l_normal, const double *l_weight, const float *l_radiance, const int32_t *l_face,
                                double eps, const float *mus, const float *lambdas, const float *lobes, int32_t n_sg,
                                int64_t n_points, const double *p_point, const float *p_normal, const int32_t *p_face,
                                const float *p_base, const float *p_rough, const float *p_metal, const float *p_wo, int32_t mode,
                                int32_t n_paths, int32_t depth, int32_t rr_start, double t_min, int64_t seed, int64_t point_base,
                                float *out, int32_t *n_open, int32_t *trace, uint8_t *end, void *stream)
{
    const PathArgs a{nodes, n_faces, vertices, n_vertices, triangles, v_normal, v_base, v_rough, v_metal, n_sources, l_point, l_normal,
                     l_weight, l_radiance, l_face, eps, 1.0 - eps, mus, lambdas, lobes, n_points, p_point, p_normal, p_face, p_base,
                     p_rough, p_metal, p_wo, t_min, point_base, out, n_open, trace, end, (uint32_t)((uint64_t)seed & 0xFFFFFFFFu),
                     (uint32_t)((uint64_t)seed >> 32), n_sg, n_paths, depth, rr_start, 0, 0, 0};
    return path_launch(a, slots, mode, stream, surfpath_is_reflect_kernel, surfpath_is_irradiance_kernel);
}
