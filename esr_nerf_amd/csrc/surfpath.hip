// Path-traced light on the exported surface (esr_nerf_amd/sources.py: path_light, lit_view(paths=)).  Section X of
// include/esr_hip.h is the definition; tests/surfpath_ref.py restates it.
//
// The reference's light-transport stage is a one-sample path tracer in the volume (app/utils/pbr/functions.py:10-18,
// diffuse_scattering: a uniform random unit vector flipped into the normal's hemisphere, weighted by the Disney reflection with its
// (n . wi) 2 pi).  This kernel chains that estimator on the mesh: the stack-less walk (bvh_walk.h), the BRDF (disney.h), the
// environment (sg_env.h) and the sources as point lights (section U's per-slot term), with the path's vertex and throughput in
// registers.
//
// One kernel body, two instantiations (reflect / irradiance at the first vertex).  Kd adjacent lanes form the group of one point:
// lane k holds the paths k, k + Kd, ...  A wave holds 64 / Kd points, a block of 256 lanes 256 / Kd; the blocks stride over the
// points.  A lane
//   reads its point at the start of every path (the first vertex; not kept over the paths: its 18 registers are a wave a SIMD),
//   per segment draws the direction from Philox4x32-10 (the counter names the point, the path, the segment: no state is kept),
//   multiplies the throughput by the vertex's reflection, walks the ray,
//   on a miss evaluates the environment (the lobe table sits in LDS) and ends the path,
//   on a hit interpolates the next vertex from the face's three vertices, gathers one random slot of every source through the
//   any-hit walk (next-event estimation) and goes on from there;
// the nine sums (component, channel) of the Kd lanes are then combined by the xor butterfly of surflight.hip and lane 0 stores.
// Nothing of size P N is written but the optional `trace` and `end`; no atomics, no scratch.
#include "bvh_walk.h"
#include "disney.h"
#include "sg_env.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_BLOCKS = 2048;
constexpr double kTwoPi = 2.0 * 3.14159265358979323846;
constexpr double kInv2Pi = 1.0 / (2.0 * 3.14159265358979323846);

struct PathArgs {
    const esr_bvh_node_t *nodes;
    int64_t n_faces;
    const double *vertices;
    int64_t n_vertices;
    const int64_t *triangles;
    const float *v_normal, *v_base, *v_rough, *v_metal;
    int64_t n_sources;
    const double *l_point, *l_normal, *l_weight;
    const float *l_radiance;
    const int32_t *l_face;
    double eps, tmax;                     // the shadow segment's interval: eps < t <= 1 - eps
    const float *mus, *lambdas, *lobes;
    int64_t n_points;
    const double *p_point;
    const float *p_normal;
    const int32_t *p_face;
    const float *p_base, *p_rough, *p_metal, *p_wo;
    double t_min;
    int64_t point_base;
    float *out;
    int32_t *n_open, *trace;
    uint8_t *end;
    uint32_t key0, key1;
    int32_t n_sg, n_paths, depth;
    int lg, lgp;                          // log2(Kd), log2(Kp)
    int64_t stride;                       // the points of one trip of the grid
};

// As in surflight.hip and surfenv.hip: the walk leaves no scalar register free, so whatever the kernel needs outside the walk is
// read from the kernel-argument segment again where it is used.  PathArgs is the kernel's only argument and so lies at the start
// of the segment; the empty asm only keeps the compiler from hoisting the loads back out of the loops.
typedef const __attribute__((address_space(4))) PathArgs *KernArgs;

__device__ __forceinline__ KernArgs kernargs()
{
    KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// Philox4x32-10 of the counter (c0, c1, c2, c3) under the key (k0, k1)
__device__ __forceinline__ void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4])
{
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// Marsaglia's uniform point on the sphere from the blocks 0 .. 7 of the counter (c0, c1, c2, .), binary64
__device__ __forceinline__ void sphere_direction(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1, double w[3])
{
#pragma clang fp contract(off)
    w[0] = 0.0, w[1] = 0.0, w[2] = 1.0;
    for (uint32_t block = 0; block < 8; ++block) {
        uint32_t r[4];
        philox(c0, c1, c2, block, k0, k1, r);
        bool taken = false;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double a1 = 2.0 * ((double)r[2 * h] * 0x1p-32) - 1.0, a2 = 2.0 * ((double)r[2 * h + 1] * 0x1p-32) - 1.0;
            const double s = a1 * a1 + a2 * a2;
            if (!taken && s < 1.0) {
                const double q = __dsqrt_rn(1.0 - s);
                w[0] = (2.0 * a1) * q, w[1] = (2.0 * a2) * q, w[2] = 1.0 - 2.0 * s;
                taken = true;
            }
        }
        if (taken) break;
    }
}

template <int MODE> __device__ __forceinline__ void surface_path()
{
#pragma clang fp contract(off)
    __shared__ float sg[SG_TABLE_FLOATS];
    const KernArgs k0 = kernargs();
    sg_table_fill(sg, k0->mus, k0->lambdas, k0->lobes, k0->n_sg, SP_THREADS);
    __syncthreads();
    // (the scene, t_min and Kd are the same for every lane; kept in vector registers all the same: the scalar ones are the walk's
    // and the masks' of the loops around it -- points, paths, segments, sources)
    const esr_bvh_node_t *nodes = k0->nodes;
    const double *verts = k0->vertices;
    const int64_t *tris = k0->triangles;
    int64_t n_f = k0->n_faces, n_v = k0->n_vertices;
    double tmin = k0->t_min;
    int kd = 1 << k0->lg;
    asm volatile("" : "+v"(nodes), "+v"(verts), "+v"(tris), "+v"(n_f), "+v"(n_v), "+v"(tmin), "+v"(kd));
    const BvhScene scene{nodes, n_f, verts, n_v, tris};
    const int k = threadIdx.x & (kd - 1);
    for (int64_t p = (int64_t)blockIdx.x * (SP_THREADS >> k0->lg) + (threadIdx.x >> k0->lg);;
         p += kernargs()->stride) {
        const KernArgs kpt = kernargs();
        if (p >= kpt->n_points) break;
        const uint32_t ctr0 = (uint32_t)(kpt->point_base + p);
        double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // env_dir, env_indir, src_indir x 3 channels
        int open = 0;
        // The lane's state: path s, segment b, and src -- -1 while the segment itself is cast, else the source whose slot is
        // gathered at the vertex just reached.  One step of the loop below walks ONE ray, the segment's (nearest hit) or a shadow
        // segment's (any hit): the walk sits one loop deep inside the points' loop, as in surfenv.hip, whatever the depth.
        int s = k, b = 0;
        int64_t src = -1;
        double x[3], T[3];
        float n[3], base[3], wo[3], rough, metal;
        int32_t face;
        // the first vertex of a path is the point: read again for every path
        auto first_vertex = [&]() {
            const KernArgs kf = kernargs();
#pragma unroll
            for (int i = 0; i < 3; ++i) x[i] = kf->p_point[3 * p + i], n[i] = kf->p_normal[3 * p + i], base[i] = 0.f, wo[i] = 0.f, T[i] = 1.0;
            rough = 0.f, metal = 0.f;
            if (MODE == 0) {
#pragma unroll
                for (int i = 0; i < 3; ++i) base[i] = kf->p_base[3 * p + i], wo[i] = kf->p_wo[3 * p + i];
                rough = kf->p_rough[p], metal = kf->p_metal[p];
            }
            face = kf->p_face ? kf->p_face[p] : -1;
        };
        first_vertex();
        for (;;) {
            const KernArgs kr = kernargs();
            if (s >= kr->n_paths) break;
            const int64_t path = p * kr->n_paths + s;
            Ray ray;
            double w[3] = {0.0, 0.0, 0.0}, tmax = (double)INFINITY, G = 0.0;
            float wi[3] = {0.f, 0.f, 0.f};                                    // the segment's direction, or towards the light
            int32_t skip = face;
            int64_t slot = 0;
            bool live;
            if (src < 0) {
                // the direction: uniform on the sphere, flipped into the normal's hemisphere
                sphere_direction(ctr0, (uint32_t)s, (uint32_t)(2 * b), kr->key0, kr->key1, w);
#pragma unroll
                for (int i = 0; i < 3; ++i) wi[i] = (float)w[i];
                const float sf = (wi[0] * n[0] + wi[1] * n[1]) + wi[2] * n[2];
                if (sf < 0.f) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) w[i] = -w[i], wi[i] = -wi[i];
                }
                // 1. the weight of the vertex
                if (MODE == 1 && b == 0) {
                    const double cos_x = ((double)n[0] * (double)wi[0] + (double)n[1] * (double)wi[1]) + (double)n[2] * (double)wi[2];
                    const double wt = cos_x * kTwoPi;
#pragma unroll
                    for (int c = 0; c < 3; ++c) T[c] = T[c] * wt;
                } else {
                    const Disney R = disney_eval(base, rough, metal, n, wi, wo);
#pragma unroll
                    for (int c = 0; c < 3; ++c) T[c] = T[c] * (double)R.R[c];
                }
                // 2. the segment (a vertex with a component that is not finite hits nothing)
#pragma unroll
                for (int i = 0; i < 3; ++i) ray.o[i] = x[i], ray.d[i] = w[i], ray.inv[i] = 1.0 / w[i];
                ray.tmin = tmin;
                live = fabs(x[0]) < INFINITY && fabs(x[1]) < INFINITY && fabs(x[2]) < INFINITY;
            } else {
                // 5. next-event estimation: one slot of the source, section U's term at the vertex
                uint32_t r[4];
                philox(ctr0, (uint32_t)s, (uint32_t)(2 * b + 1), (uint32_t)(src >> 2), kr->key0, kr->key1, r);
                const int q = (int)(src & 3);
                const uint32_t word = q == 0 ? r[0] : q == 1 ? r[1] : q == 2 ? r[2] : r[3];
                const int lgp = kr->lgp;
                slot = (src << lgp) + (lgp ? (int64_t)(word >> (32 - lgp)) : 0);
                const double A = kr->l_weight[slot];
                live = A != 0.0;
                double d[3] = {0.0, 0.0, 0.0};
                if (live) {
                    double g[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) d[i] = kr->l_point[3 * slot + i] - x[i], g[i] = kr->l_normal[3 * slot + i];
                    skip = kr->l_face[slot];
                    const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                    const double rr = __dsqrt_rn(r2);
#pragma unroll
                    for (int i = 0; i < 3; ++i) w[i] = d[i] / rr, wi[i] = (float)w[i];
                    const double cos_l = -((g[0] * w[0] + g[1] * w[1]) + g[2] * w[2]);
                    const double cos_x = ((double)n[0] * w[0] + (double)n[1] * w[1]) + (double)n[2] * w[2];
                    live = r2 > 0.0 && cos_l > 0.0 && cos_x > 0.0;            // (false for a NaN)
                    G = (cos_l * A) / fmax(r2, A);
                }
                // (every component of x and d is finite on a live lane: one that is not makes r2, and so a cosine, inf or NaN)
#pragma unroll
                for (int i = 0; i < 3; ++i) ray.o[i] = x[i], ray.d[i] = d[i], ray.inv[i] = 1.0 / d[i];
                ray.tmin = kr->eps;
                tmax = kr->tmax;
            }
            Best best{tmax, 0.0, 0.0, -1};
            int n_box = 0, n_tri = 0;
            if (src < 0) bvh_walk<false>(scene, ray, live, skip, tmax, best, n_box, n_tri);
            else bvh_walk<true>(scene, ray, live, skip, tmax, best, n_box, n_tri);
            const KernArgs kh = kernargs();
            bool next_segment = false, path_ends = false;
            uint8_t code = 0;
            if (src < 0) {
                if (kh->trace) kh->trace[path * kh->depth + b] = best.face;
                if (best.face < 0) {
                    // 3. the ray leaves the mesh
                    open += b == 0 ? 1 : 0;
                    if (kh->n_sg > 0) {
                        float L[3];
                        sg_environment(sg, kh->n_sg, wi, L);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const double add = T[c] * (double)L[c];
                            if (b == 0) acc[c] = acc[c] + add;
                            else acc[3 + c] = acc[3 + c] + add;
                        }
                    }
                    code = 1, path_ends = true, ++b;
                } else {
                    // 4. the next vertex (the walk has checked the face's three vertex ids against n_vertices)
                    const int64_t *t = kh->triangles + 3 * (int64_t)best.face;
                    const int64_t ia = t[0], ib = t[1], ic = t[2];
                    const double wa = (1.0 - best.u) - best.v;
                    const float fa = (float)wa, fu = (float)best.u, fv = (float)best.v;
                    float nn[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        x[i] = (wa * kh->vertices[3 * ia + i] + best.u * kh->vertices[3 * ib + i]) + best.v * kh->vertices[3 * ic + i];
                        nn[i] = (fa * kh->v_normal[3 * ia + i] + fu * kh->v_normal[3 * ib + i]) + fv * kh->v_normal[3 * ic + i];
                        base[i] = (fa * kh->v_base[3 * ia + i] + fu * kh->v_base[3 * ib + i]) + fv * kh->v_base[3 * ic + i];
                        wo[i] = -wi[i];
                    }
                    rough = (fa * kh->v_rough[ia] + fu * kh->v_rough[ib]) + fv * kh->v_rough[ic];
                    metal = (fa * kh->v_metal[ia] + fu * kh->v_metal[ib]) + fv * kh->v_metal[ic];
                    face = best.face;
                    const float len = sqrtf((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
                    bool alive = len > 0.f && len < INFINITY;
                    if (alive) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) n[i] = nn[i] / len;
                        alive = (n[0] * wo[0] + n[1] * wo[1]) + n[2] * wo[2] > 0.f;      // (false for a NaN, and for a back face)
                    }
                    if (!alive) code = 2, path_ends = true, ++b;
                    else if (kh->n_sources > 0) src = 0;
                    else next_segment = true;
                }
            } else {
                if (live && best.face < 0) {
                    const float *E = kh->l_radiance + 3 * slot;
                    const Disney R = disney_eval(base, rough, metal, n, wi, wo);
                    const double kp = (double)(1 << kh->lgp);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double term = (((double)R.R[c] * kInv2Pi) * G) * (double)E[c];
                        acc[6 + c] = acc[6 + c] + T[c] * (kp * term);
                    }
                }
                ++src;
                next_segment = src >= kh->n_sources;
            }
            if (next_segment) {
                // 6. (the vertex is the state already)
                src = -1, ++b;
                path_ends = b >= kh->depth;
            }
            if (path_ends) {
                if (kh->trace) {
                    for (int bb = b; bb < kh->depth; ++bb) kh->trace[path * kh->depth + bb] = -2;
                }
                if (kh->end) kh->end[path] = code;
                s += kd, b = 0, src = -1;
                first_vertex();
            }
        }
        // the interleaved butterfly of the nine sums and the count: every lane of the group is here (its lanes share p)
        for (int off = 1; off < kd; off <<= 1) {
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double t = __shfl_xor(acc[c], off);
                acc[c] = acc[c] + t;
            }
            open += __shfl_xor(open, off);
        }
        if (k == 0) {
            const KernArgs ko = kernargs();
            const double N = (double)ko->n_paths;
#pragma unroll
            for (int c = 0; c < 9; ++c) ko->out[9 * p + c] = (float)(acc[c] / N);
            if (ko->n_open) ko->n_open[p] = open;
        }
    }
}

__global__ void __launch_bounds__(SP_THREADS) surfpath_reflect_kernel(PathArgs) { surface_path<0>(); }
__global__ void __launch_bounds__(SP_THREADS) surfpath_irradiance_kernel(PathArgs) { surface_path<1>(); }

bool given(const void *p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
bool optional(const void *p, size_t a) { return !p || ((uintptr_t)p & (a - 1)) == 0; }

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
    if (n_faces < 0 || n_vertices < 0 || n_sources < 0 || n_points < 0 || n_sg < 0 || (mode != 0 && mode != 1) || slots < 1 ||
        !(eps >= 0.0 && eps < 0.5) || n_paths < 1 || depth < 1 || !(t_min >= 0.0) || point_base < 0)
        return ESR_EINVAL;
    const int64_t cap = (int64_t)1 << 31;
    if (n_faces >= cap || n_vertices >= cap || n_sources >= cap || n_points >= cap || slots > ESR_SURFACE_LIGHT_MAX_SLOTS ||
        n_sg > ESR_SURFACE_ENV_MAX_SG || n_paths > ESR_SURFACE_PATH_MAX_PATHS || depth > ESR_SURFACE_PATH_MAX_DEPTH ||
        point_base > ((int64_t)1 << 32) - n_points)
        return ESR_ECAP;
    if (slots & (slots - 1)) return ESR_EINVAL;
    if (!n_points) return 0;
    if (!given(p_point, 8) || !given(p_normal, 4) || !optional(p_face, 4) || !given(out, 4) || !optional(n_open, 4) || !optional(trace, 4))
        return ESR_EINVAL;
    if (mode == 0 && (!given(p_base, 4) || !given(p_rough, 4) || !given(p_metal, 4) || !given(p_wo, 4))) return ESR_EINVAL;
    if (n_faces && (!given(vertices, 8) || !given(triangles, 8) || !given(v_normal, 4) || !given(v_base, 4) || !given(v_rough, 4) ||
                    !given(v_metal, 4)))
        return ESR_EINVAL;
    if (n_faces > 1 && !given(nodes, 16)) return ESR_EINVAL;
    if (n_sources && (!given(l_point, 8) || !given(l_normal, 8) || !given(l_weight, 8) || !given(l_radiance, 4) || !given(l_face, 4)))
        return ESR_EINVAL;
    if (n_sg && (!given(mus, 4) || !given(lambdas, 4) || !given(lobes, 4))) return ESR_EINVAL;
    PathArgs a{nodes, n_faces, vertices, n_vertices, triangles, v_normal, v_base, v_rough, v_metal, n_sources, l_point, l_normal,
               l_weight, l_radiance, l_face, eps, 1.0 - eps, mus, lambdas, lobes, n_points, p_point, p_normal, p_face, p_base,
               p_rough, p_metal, p_wo, t_min, point_base, out, n_open, trace, end, (uint32_t)((uint64_t)seed & 0xFFFFFFFFu),
               (uint32_t)((uint64_t)seed >> 32), n_sg, n_paths, depth, 0, 0, 0};
    while (a.lg < 6 && (1 << a.lg) < n_paths) ++a.lg;
    while ((1 << a.lgp) < slots) ++a.lgp;
    const int grid = esr_grid_for(n_points, SP_THREADS >> a.lg, SP_BLOCKS);
    a.stride = (int64_t)grid * (SP_THREADS >> a.lg);
    hipStream_t st = esr_stream(stream);
    if (mode == 0) surfpath_reflect_kernel<<<grid, SP_THREADS, 0, st>>>(a);
    else surfpath_irradiance_kernel<<<grid, SP_THREADS, 0, st>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}
