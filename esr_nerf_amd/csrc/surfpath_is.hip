// Importance-sampled path-traced light on the exported surface (esr_nerf_amd/sources.py: path_light(sampling="brdf"),
// lit_view(paths=, sampling="brdf"), bake_irradiance(paths=)).  Section Y of include/esr_hip.h is the definition;
// tests/surfpath_is_ref.py restates it.
//
// surfpath.hip (section X) chains the light-transport stage's estimator: a uniform direction weighted by the Disney reflection.
// This file keeps that kernel's shape -- one loop, one ray per step, the vertex and the throughput in registers, the lobe table
// in LDS, the nine sums combined by the xor butterfly -- and replaces the draw: per segment one of two techniques is chosen by
// the vertex's material, a cosine-distributed direction (Malley: the disc pair lifted to the hemisphere) or a half vector from
// the BRDF's own lobe D = exp(kappa (n.h - 1)) / (pi r^2), kappa = 2 / r^2, whose CDF in cos(theta) inverts in closed form; the
// weight divides the reflection by the one-sample balance-heuristic density of both; and from segment rr_start on Russian
// roulette ends a path with the probability its throughput has lost.  The disc rejection already yields an independent
// (radius^2, angle) pair, so neither technique needs trigonometry.
//
// The reference has no such sampler: this is an addition to its interfaces, as sections U, W and X's chaining are.
//
// philox and the disc candidates are surfpath.hip's, copied: that file is pinned to its compiled form and stays untouched.
#include "bvh_walk.h"
#include "disney.h"
#include "sg_env.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_BLOCKS = 2048;
constexpr double kPi64 = 3.14159265358979323846;
constexpr double kInv2Pi = 1.0 / (2.0 * 3.14159265358979323846);

struct PathIsArgs {
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
    int32_t n_sg, n_paths, depth, rr_start;
    int lg, lgp;                          // log2(Kd), log2(Kp)
    int64_t stride;                       // the points of one trip of the grid
};

// As in surfpath.hip: the walk leaves no scalar register free, so whatever the kernel needs outside the walk is read from the
// kernel-argument segment again where it is used.  PathIsArgs is the kernel's only argument and so lies at the start of the
// segment; the empty asm only keeps the compiler from hoisting the loads back out of the loops.
typedef const __attribute__((address_space(4))) PathIsArgs *KernArgs;

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

// The first of section X's candidate pairs over the blocks 0 .. 7 of the counter (c0, c1, c2, .) that lies strictly inside the
// unit disc and off its centre: (a1, a2, s = a1 a1 + a2 a2), binary64.  -> found
__device__ __forceinline__ bool disc_pair(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1, double &p1, double &p2, double &ps)
{
#pragma clang fp contract(off)
    p1 = 0.0, p2 = 0.0, ps = 0.0;
    bool taken = false;
    for (uint32_t block = 0; block < 8; ++block) {
        uint32_t r[4];
        philox(c0, c1, c2, block, k0, k1, r);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double a1 = 2.0 * ((double)r[2 * h] * 0x1p-32) - 1.0, a2 = 2.0 * ((double)r[2 * h + 1] * 0x1p-32) - 1.0;
            const double s = a1 * a1 + a2 * a2;
            if (!taken && s > 0.0 && s < 1.0) p1 = a1, p2 = a2, ps = s, taken = true;
        }
        if (taken) break;
    }
    return taken;
}

template <int MODE> __device__ __forceinline__ void surface_path_is()
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
    const int k = threadIdx.x & (kd - 1);
    for (int64_t p = (int64_t)blockIdx.x * (SP_THREADS >> k0->lg) + (threadIdx.x >> k0->lg);;
         p += kernargs()->stride) {
        const KernArgs kpt = kernargs();
        if (p >= kpt->n_points) break;
        const uint32_t ctr0 = (uint32_t)(kpt->point_base + p);
        double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // env_dir, env_indir, src_indir x 3 channels
        int open = 0;
        // The lane's state, as in surfpath.hip: path s, segment b, and src -- -1 while the segment itself is cast, else the source
        // whose slot is gathered at the vertex just reached.  One step of the loop below walks ONE ray.
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
            int dead = 0;                                                     // 3: the roulette ended the path, 4: no direction
            bool live;
            if (src < 0) {
                // the uniforms of the segment: the disc pair, the technique's and the roulette's
                double a1, a2, sd;
                const bool found = disc_pair(ctr0, (uint32_t)s, (uint32_t)(4 * b), kr->key0, kr->key1, a1, a2, sd);
                uint32_t r[4];
                philox(ctr0, (uint32_t)s, (uint32_t)(4 * b + 2), 0u, kr->key0, kr->key1, r);
                const double ut = ((double)r[0] + 0.5) * 0x1p-32, ur = ((double)r[1] + 0.5) * 0x1p-32;
                // the roulette (nothing below branches: a lane whose path has ended computes on and casts nothing)
                {
                    const double m = fmax(fmax(T[0], T[1]), T[2]);
                    double q = m >= 0.0625 ? (m <= 1.0 ? m : 1.0) : 0.0625;
                    q = (m != m || b < kr->rr_start) ? 1.0 : q;
                    dead = ur >= q ? 3 : 0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) T[c] = T[c] / q;
                }
                const double nd[3] = {(double)n[0], (double)n[1], (double)n[2]};
                const double wod[3] = {(double)wo[0], (double)wo[1], (double)wo[2]};
                // the technique
                double qs = 0.0;
                if (!(MODE == 1 && b == 0)) {
                    const double md = (double)metal;
                    const double ab = (((double)base[0] + (double)base[1]) + (double)base[2]) / 3.0;
                    const double Fb = 0.04 * (1.0 - md) + ab * md, db = (1.0 - md) * ab;
                    const double sum = Fb + db, r0 = Fb / sum;
                    qs = r0 >= 0.125 ? (r0 <= 0.875 ? r0 : 0.875) : 0.125;
                    qs = sum > 0.0 ? qs : 0.125;
                }
                const bool lobe = ut < qs;
                const double kappa = 2.0 / fmax((double)rough * (double)rough, 1e-7);
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
                // 1. the weight of the vertex: the reflection over the density of the two techniques at w
                if (MODE == 1 && b == 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) T[c] = T[c] * kPi64;
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
                    const Disney R = disney_eval(base, rough, metal, n, wi, wo);
#pragma unroll
                    for (int c = 0; c < 3; ++c) T[c] = T[c] * ((double)R.R[c] / pd);
                }
                // 2. the segment (a vertex with a component that is not finite hits nothing; an ended path casts nothing)
#pragma unroll
                for (int i = 0; i < 3; ++i) ray.o[i] = x[i], ray.d[i] = w[i], ray.inv[i] = 1.0 / w[i];
                ray.tmin = tmin;
                live = !dead && fabs(x[0]) < INFINITY && fabs(x[1]) < INFINITY && fabs(x[2]) < INFINITY;
            } else {
                // 5. next-event estimation: one slot of the source, section U's term at the vertex
                uint32_t r[4];
                philox(ctr0, (uint32_t)s, (uint32_t)(4 * b + 1), (uint32_t)(src >> 2), kr->key0, kr->key1, r);
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
            // (the face count is taken anew at every step: the masks the walk derives from it are then made here, not kept in
            // scalar registers over the whole kernel, where the binary64 exp and log hold their constants)
            int64_t n_f_now = n_f;
            asm volatile("" : "+v"(n_f_now));
            const BvhScene scene{nodes, n_f_now, verts, n_v, tris};
            if (src < 0) bvh_walk<false>(scene, ray, live, skip, tmax, best, n_box, n_tri);
            else bvh_walk<true>(scene, ray, live, skip, tmax, best, n_box, n_tri);
            const KernArgs kh = kernargs();
            bool next_segment = false, path_ends = false;
            uint8_t code = 0;
            if (src < 0 && dead) {
                // (segment b was not cast: its trace and the later ones' are -2)
                code = (uint8_t)dead, path_ends = true;
            } else if (src < 0) {
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
        int kd_now = kd, k_now = k;                                          // (as n_f_now above)
        asm volatile("" : "+v"(kd_now), "+v"(k_now));
        for (int off = 1; off < kd_now; off <<= 1) {
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double t = __shfl_xor(acc[c], off);
                acc[c] = acc[c] + t;
            }
            open += __shfl_xor(open, off);
        }
        if (k_now == 0) {
            const KernArgs ko = kernargs();
            const double N = (double)ko->n_paths;
#pragma unroll
            for (int c = 0; c < 9; ++c) ko->out[9 * p + c] = (float)(acc[c] / N);
            if (ko->n_open) ko->n_open[p] = open;
        }
    }
}

__global__ void __launch_bounds__(SP_THREADS) surfpath_is_reflect_kernel(PathIsArgs) { surface_path_is<0>(); }
__global__ void __launch_bounds__(SP_THREADS) surfpath_is_irradiance_kernel(PathIsArgs) { surface_path_is<1>(); }

bool given(const void *p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
bool optional(const void *p, size_t a) { return !p || ((uintptr_t)p & (a - 1)) == 0; }

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
    if (n_faces < 0 || n_vertices < 0 || n_sources < 0 || n_points < 0 || n_sg < 0 || (mode != 0 && mode != 1) || slots < 1 ||
        !(eps >= 0.0 && eps < 0.5) || n_paths < 1 || depth < 1 || rr_start < 1 || !(t_min >= 0.0) || point_base < 0)
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
    PathIsArgs a{nodes, n_faces, vertices, n_vertices, triangles, v_normal, v_base, v_rough, v_metal, n_sources, l_point, l_normal,
                 l_weight, l_radiance, l_face, eps, 1.0 - eps, mus, lambdas, lobes, n_points, p_point, p_normal, p_face, p_base,
                 p_rough, p_metal, p_wo, t_min, point_base, out, n_open, trace, end, (uint32_t)((uint64_t)seed & 0xFFFFFFFFu),
                 (uint32_t)((uint64_t)seed >> 32), n_sg, n_paths, depth, rr_start, 0, 0, 0};
    while (a.lg < 6 && (1 << a.lg) < n_paths) ++a.lg;
    while ((1 << a.lgp) < slots) ++a.lgp;
    const int grid = esr_grid_for(n_points, SP_THREADS >> a.lg, SP_BLOCKS);
    a.stride = (int64_t)grid * (SP_THREADS >> a.lg);
    hipStream_t st = esr_stream(stream);
    if (mode == 0) surfpath_is_reflect_kernel<<<grid, SP_THREADS, 0, st>>>(a);
    else surfpath_is_irradiance_kernel<<<grid, SP_THREADS, 0, st>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}
