// Light of the spherical-Gaussian environment map on the exported surface (esr_nerf_amd/sources.py: environment_light,
// vertex_env_radiance, lit_view).  Section V of include/esr_hip.h is the definition; tests/surfenv_ref.py restates it.
//
// The reference defines the quantity in its evaluation decomposition (app/fine/model/esrnerf.py:983-994): over the hemisphere
// directions of diffuse_scattering_fib, lin/env_dir = mean(envmap(dir) alphainv_last R) and lin/env_indir = mean(off_marched R).
// On the surface alphainv_last is "the ray leaves the mesh" and off_marched the radiance of the face that is hit.
//
// One kernel body, four instantiations (reflect / irradiance, any-hit / nearest-hit).  Kd adjacent lanes form the group of one
// point: lane k holds the directions k, k + Kd, ...  A wave holds 64 / Kd points, a block of 256 lanes 256 / Kd; the blocks
// stride over the points.  A lane
//   loads its point once (position, normal, material, view direction: registers, kept over the directions),
//   per direction flips the table entry into the normal's hemisphere, walks the ray through bvh_walk.h,
//   evaluates the environment only where the ray left the mesh (the lobe table sits in LDS, normalised once per block),
//   or interpolates the vertex radiance of the face that was hit, evaluates the BRDF (disney.h, binary32) and
//   adds the three channel terms to its binary64 sums; the Kd lane sums are then combined by the xor butterfly of
//   surflight.hip and lane 0 of the group stores.
// Nothing of size P R is written but the optional `hit` bytes; no atomics, no scratch.
#include "bvh_walk.h"
#include "disney.h"

namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_BLOCKS = 2048;
constexpr double kTwoPi = 2.0 * 3.14159265358979323846;

struct EnvArgs {
    const esr_bvh_node_t *nodes;
    int64_t n_faces;
    const double *vertices;
    int64_t n_vertices;
    const int64_t *triangles;
    const float *dirs;
    const float *mus, *lambdas, *lobes;
    const float *vertex_radiance;
    int64_t n_points;
    const double *p_point;
    const float *p_normal;
    const int32_t *p_face;
    const float *p_base, *p_rough, *p_metal, *p_wo;
    double t_min;
    float *out;
    int32_t *n_open;
    uint8_t *hit;
    int32_t n_dirs, n_sg;
    int lg;                               // log2(Kd)
};

// As in surflight.hip: the walk leaves no scalar register free, so whatever the kernel needs outside the walk is read from the
// kernel-argument segment again where it is used.  EnvArgs is the kernel's only argument and so lies at the start of the
// segment; the empty asm only keeps the compiler from hoisting the loads back out of the loops.
typedef const __attribute__((address_space(4))) EnvArgs *KernArgs;

__device__ __forceinline__ KernArgs kernargs()
{
    KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// the environment along the unit direction w, binary32, every operation rounded on its own: the order of lts_combine_kernel
__device__ __forceinline__ void environment(const float *sg, int J, const float w[3], float L[3])
{
#pragma clang fp contract(off)
    float pre[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < J; ++j) {
        const float dtl = (w[0] * sg[3 * j] + w[1] * sg[3 * j + 1]) + w[2] * sg[3 * j + 2];
        const float e = expf(sg[6 * ESR_SURFACE_ENV_MAX_SG + j] * (dtl - 1.f));
        const float *mu = sg + 3 * ESR_SURFACE_ENV_MAX_SG + 3 * j;
        pre[0] = pre[0] + mu[0] * e, pre[1] = pre[1] + mu[1] * e, pre[2] = pre[2] + mu[2] * e;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = esr_softplus(pre[c]);
}

template <int MODE, bool NEAREST> __device__ __forceinline__ void surface_env()
{
#pragma clang fp contract(off)
    // unit lobes [J,3], mus [J,3], |lambda| [J]
    __shared__ float sg[7 * ESR_SURFACE_ENV_MAX_SG];
    const KernArgs k0 = kernargs();
    for (int j = threadIdx.x; j < k0->n_sg; j += SE_THREADS) {
        const float lx = k0->lobes[3 * j], ly = k0->lobes[3 * j + 1], lz = k0->lobes[3 * j + 2];
        const float nn = fmaxf(sqrtf((lx * lx + ly * ly) + lz * lz), 1e-12f);
        sg[3 * j] = lx / nn, sg[3 * j + 1] = ly / nn, sg[3 * j + 2] = lz / nn;
#pragma unroll
        for (int c = 0; c < 3; ++c) sg[3 * ESR_SURFACE_ENV_MAX_SG + 3 * j + c] = k0->mus[3 * j + c];
        sg[6 * ESR_SURFACE_ENV_MAX_SG + j] = fabsf(k0->lambdas[j]);
    }
    __syncthreads();
    const BvhScene scene{k0->nodes, k0->n_faces, k0->vertices, k0->n_vertices, k0->triangles};
    // (t_min and Kd are the same for every lane; kept in vector registers all the same, the scalar ones being the walk's)
    double tmin = k0->t_min;
    const int lg = k0->lg;
    int kd = 1 << lg;
    asm volatile("" : "+v"(tmin), "+v"(kd));
    const int k = threadIdx.x & (kd - 1);
    const int64_t per_block = SE_THREADS >> lg;
    for (int64_t p = (int64_t)blockIdx.x * per_block + (threadIdx.x >> lg);; p += (int64_t)gridDim.x * per_block) {
        const KernArgs kpt = kernargs();
        if (p >= kpt->n_points) break;
        double x[3];
        float n[3], base[3] = {0.f, 0.f, 0.f}, wo[3] = {0.f, 0.f, 0.f}, rough = 0.f, metal = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) x[i] = kpt->p_point[3 * p + i], n[i] = kpt->p_normal[3 * p + i];
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) base[i] = kpt->p_base[3 * p + i], wo[i] = kpt->p_wo[3 * p + i];
            rough = kpt->p_rough[p], metal = kpt->p_metal[p];
        }
        const int32_t skip = kpt->p_face ? kpt->p_face[p] : -1;
        const bool finite_x = fabs(x[0]) < INFINITY && fabs(x[1]) < INFINITY && fabs(x[2]) < INFINITY;
        double acc[3] = {0.0, 0.0, 0.0};
        int open = 0;
        for (int r = k;; r += kd) {
            const KernArgs kr = kernargs();
            if (r >= kr->n_dirs) break;
            float w[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) w[i] = kr->dirs[3 * r + i];
            const float s = (w[0] * n[0] + w[1] * n[1]) + w[2] * n[2];
            if (s < 0.f) w[0] = -w[0], w[1] = -w[1], w[2] = -w[2];
            Ray ray;
#pragma unroll
            for (int i = 0; i < 3; ++i) ray.o[i] = x[i], ray.d[i] = (double)w[i], ray.inv[i] = 1.0 / ray.d[i];
            ray.tmin = tmin;
            const bool finite = finite_x && fabsf(w[0]) < INFINITY && fabsf(w[1]) < INFINITY && fabsf(w[2]) < INFINITY;
            Best best{(double)INFINITY, 0.0, 0.0, -1};
            int n_box = 0, n_tri = 0;
            bvh_walk<!NEAREST>(scene, ray, finite, skip, (double)INFINITY, best, n_box, n_tri);
            const bool miss = best.face < 0;
            open += miss ? 1 : 0;
            const KernArgs ko = kernargs();
            if (ko->hit) ko->hit[p * ko->n_dirs + r] = miss ? 0 : 1;
            if (!miss && !NEAREST) continue;                                  // (a hit without vertex radiance: L = 0)
            double L[3];
            if (miss) {
                float e[3];
                environment(sg, ko->n_sg, w, e);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] = (double)e[c];
            } else {
                // (the walk has checked the face's three vertex ids against n_vertices)
                const int64_t *t = ko->triangles + 3 * (int64_t)best.face;
                const float *ea = ko->vertex_radiance + 3 * t[0], *eb = ko->vertex_radiance + 3 * t[1], *ec = ko->vertex_radiance + 3 * t[2];
                const double wa = (1.0 - best.u) - best.v;
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] = (wa * (double)ea[c] + best.u * (double)eb[c]) + best.v * (double)ec[c];
            }
            if (MODE == 0) {
                const Disney R = disney_eval(base, rough, metal, n, w, wo);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + L[c] * (double)R.R[c];
            } else {
                const double cos_x = ((double)n[0] * (double)w[0] + (double)n[1] * (double)w[1]) + (double)n[2] * (double)w[2];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + L[c] * cos_x;
            }
        }
        // the interleaved butterfly of the three channels and the count: every lane of the group is here (its lanes share p)
        for (int off = 1; off < kd; off <<= 1) {
            const double t0 = __shfl_xor(acc[0], off), t1 = __shfl_xor(acc[1], off), t2 = __shfl_xor(acc[2], off);
            acc[0] = acc[0] + t0, acc[1] = acc[1] + t1, acc[2] = acc[2] + t2;
            open += __shfl_xor(open, off);
        }
        if (k == 0) {
            const KernArgs ko = kernargs();
            const double R = (double)ko->n_dirs;
#pragma unroll
            for (int c = 0; c < 3; ++c) ko->out[3 * p + c] = (float)((MODE == 0 ? acc[c] : acc[c] * kTwoPi) / R);
            if (ko->n_open) ko->n_open[p] = open;
        }
    }
}

__global__ void __launch_bounds__(SE_THREADS) surfenv_reflect_any_kernel(EnvArgs) { surface_env<0, false>(); }
__global__ void __launch_bounds__(SE_THREADS) surfenv_reflect_nearest_kernel(EnvArgs) { surface_env<0, true>(); }
__global__ void __launch_bounds__(SE_THREADS) surfenv_irradiance_any_kernel(EnvArgs) { surface_env<1, false>(); }
__global__ void __launch_bounds__(SE_THREADS) surfenv_irradiance_nearest_kernel(EnvArgs) { surface_env<1, true>(); }

bool given(const void *p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
bool optional(const void *p, size_t a) { return !p || ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

ESR_API int esr_surface_env(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                            const int64_t *triangles, const float *dirs, int32_t n_dirs, const float *mus, const float *lambdas,
                            const float *lobes, int32_t n_sg, const float *vertex_radiance, int64_t n_points, const double *p_point,
                            const float *p_normal, const int32_t *p_face, const float *p_base, const float *p_rough,
                            const float *p_metal, const float *p_wo, int32_t mode, double t_min, float *out, int32_t *n_open,
                            uint8_t *hit, void *stream)
{
    if (n_faces < 0 || n_vertices < 0 || n_points < 0 || n_dirs < 1 || n_sg < 1 || (mode != 0 && mode != 1) || !(t_min >= 0.0))
        return ESR_EINVAL;
    const int64_t cap = (int64_t)1 << 31;
    if (n_faces >= cap || n_vertices >= cap || n_points >= cap || n_dirs > ESR_SURFACE_ENV_MAX_DIRS || n_sg > ESR_SURFACE_ENV_MAX_SG)
        return ESR_ECAP;
    if (!n_points) return 0;
    if (!given(dirs, 4) || !given(mus, 4) || !given(lambdas, 4) || !given(lobes, 4) || !optional(vertex_radiance, 4) ||
        !given(p_point, 8) || !given(p_normal, 4) || !optional(p_face, 4) || !given(out, 4) || !optional(n_open, 4))
        return ESR_EINVAL;
    if (mode == 0 && (!given(p_base, 4) || !given(p_rough, 4) || !given(p_metal, 4) || !given(p_wo, 4))) return ESR_EINVAL;
    if (n_faces && (!given(vertices, 8) || !given(triangles, 8))) return ESR_EINVAL;
    if (n_faces > 1 && !given(nodes, 16)) return ESR_EINVAL;
    EnvArgs a{nodes, n_faces, vertices, n_vertices, triangles, dirs, mus, lambdas, lobes, vertex_radiance, n_points, p_point,
              p_normal, p_face, p_base, p_rough, p_metal, p_wo, t_min, out, n_open, hit, n_dirs, n_sg, 0};
    while (a.lg < 6 && (1 << a.lg) < n_dirs) ++a.lg;
    const int grid = esr_grid_for(n_points, SE_THREADS >> a.lg, SE_BLOCKS);
    hipStream_t st = esr_stream(stream);
    if (mode == 0 && !vertex_radiance) surfenv_reflect_any_kernel<<<grid, SE_THREADS, 0, st>>>(a);
    else if (mode == 0) surfenv_reflect_nearest_kernel<<<grid, SE_THREADS, 0, st>>>(a);
    else if (!vertex_radiance) surfenv_irradiance_any_kernel<<<grid, SE_THREADS, 0, st>>>(a);
    else surfenv_irradiance_nearest_kernel<<<grid, SE_THREADS, 0, st>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}
