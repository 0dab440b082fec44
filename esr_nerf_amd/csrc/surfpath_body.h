// What the two path tracers on the exported surface share: surfpath.hip (header section X, uniform directions) and surfpath_is.hip
// (section Y, directions drawn from the BRDF) are this body with their own draw: everything but step 1 of the definition, the
// host side (validation and launch) included.  Each defines a `Draw`, instantiates surface_path<MODE, Draw> in its two kernels and
// hands them to path_launch.  A Draw has
//   STRIDE      the counter words of a segment: word STRIDE b + 0 names the disc candidates, + 1 the sources' slots
//   segment()   step 1: the segment's direction w (binary64, unit) and wi = (float)w, the vertex's weight multiplied into v.T;
//               -> 0, or the `end` code of a path that ends at this vertex without a cast
#pragma once
#include "bvh_walk.h"
#include "disney.h"
#include "sg_env.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_BLOCKS = 2048;
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
    int32_t n_sg, n_paths, depth, rr_start;   // (rr_start: section Y's roulette; section X's draw does not read it)
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

// The first of the 16 candidate pairs over the blocks 0 .. 7 of the counter (c0, c1, c2, .) that lies strictly inside the unit
// disc and, unless CENTRE, off its centre: (a1, a2, s = a1 a1 + a2 a2), binary64; zeros if none does.  -> found
template <bool CENTRE>
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
            if (!taken && (CENTRE || s > 0.0) && s < 1.0) p1 = a1, p2 = a2, ps = s, taken = true;
        }
        if (taken) break;
    }
    return taken;
}

struct PathVertex {                       // a path's vertex and its throughput T
    double x[3], T[3];
    float n[3], base[3], wo[3], rough, metal;
    int32_t face;
};

template <int MODE, class Draw> __device__ __forceinline__ void surface_path()
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
    for (int64_t p = (int64_t)blockIdx.x * (SP_THREADS >> k0->lg) + (threadIdx.x >> k0->lg);; p += kernargs()->stride) {
        const KernArgs kpt = kernargs();
        if (p >= kpt->n_points) break;
        const uint32_t ctr0 = (uint32_t)(kpt->point_base + p);
        // Three arrays: nine sums in one the compiler indexes at run time (a 9-way select chain per update).  FRAGILE: a 3 x 3 array
        // turns a dot product of disney_eval's around (disney.h allows contraction; which product is fused follows the operand order
        // this text leaves): a float32 ulp in `out` that no CPU test sees.  After an edit here compare `out` with the last build's bytes.
        double env_dir[3] = {0.0, 0.0, 0.0}, env_indir[3] = {0.0, 0.0, 0.0}, src_indir[3] = {0.0, 0.0, 0.0};
        auto sum = [&](int c) -> double & { return c < 3 ? env_dir[c] : c < 6 ? env_indir[c - 3] : src_indir[c - 6]; };
        int open = 0;
        // The lane's state: path s, segment b, and src -- -1 while the segment itself is cast, else the source whose slot is
        // gathered at the vertex just reached.  One step of the loop below walks ONE ray, the segment's (nearest hit) or a shadow
        // segment's (any hit): the walk sits one loop deep inside the points' loop, as in surfenv.hip, whatever the depth.
        int s = k, b = 0;
        int64_t src = -1;
        PathVertex v;
        // the first vertex of a path is the point: read again for every path
        auto first_vertex = [&]() {
            const KernArgs kf = kernargs();
#pragma unroll
            for (int i = 0; i < 3; ++i) v.x[i] = kf->p_point[3 * p + i], v.n[i] = kf->p_normal[3 * p + i], v.base[i] = 0.f, v.wo[i] = 0.f, v.T[i] = 1.0;
            v.rough = 0.f, v.metal = 0.f;
            if (MODE == 0) {
#pragma unroll
                for (int i = 0; i < 3; ++i) v.base[i] = kf->p_base[3 * p + i], v.wo[i] = kf->p_wo[3 * p + i];
                v.rough = kf->p_rough[p], v.metal = kf->p_metal[p];
            }
            v.face = kf->p_face ? kf->p_face[p] : -1;
        };
        first_vertex();
        for (;;) {
            const KernArgs kr = kernargs();
            if (s >= kr->n_paths) break;
            const int64_t path = p * kr->n_paths + s;
            Ray ray;
            double w[3] = {0.0, 0.0, 0.0}, tmax = (double)INFINITY, G = 0.0;
            float wi[3] = {0.f, 0.f, 0.f};                                    // the segment's direction, or towards the light
            int32_t skip = v.face;
            int64_t slot = 0;
            int dead = 0;                                                     // the code of a path that ends without a cast
            bool live;
            if (src < 0) {
                // 1. the direction and the weight of the vertex (a lane whose path ends here computes on and casts nothing)
                dead = Draw::segment(v, MODE == 1 && b == 0, ctr0, s, b, kr, w, wi);
                // 2. the segment (a vertex with a component that is not finite hits nothing; an ended path casts nothing)
#pragma unroll
                for (int i = 0; i < 3; ++i) ray.o[i] = v.x[i], ray.d[i] = w[i], ray.inv[i] = 1.0 / w[i];
                ray.tmin = tmin;
                live = !dead && fabs(v.x[0]) < INFINITY && fabs(v.x[1]) < INFINITY && fabs(v.x[2]) < INFINITY;
            } else {
                // 5. next-event estimation: one slot of the source, section U's term at the vertex
                uint32_t r[4];
                philox(ctr0, (uint32_t)s, (uint32_t)(Draw::STRIDE * b + 1), (uint32_t)(src >> 2), kr->key0, kr->key1, r);
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
                    for (int i = 0; i < 3; ++i) d[i] = kr->l_point[3 * slot + i] - v.x[i], g[i] = kr->l_normal[3 * slot + i];
                    skip = kr->l_face[slot];
                    const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                    const double rr = __dsqrt_rn(r2);
#pragma unroll
                    for (int i = 0; i < 3; ++i) w[i] = d[i] / rr, wi[i] = (float)w[i];
                    const double cos_l = -((g[0] * w[0] + g[1] * w[1]) + g[2] * w[2]);
                    const double cos_x = ((double)v.n[0] * w[0] + (double)v.n[1] * w[1]) + (double)v.n[2] * w[2];
                    live = r2 > 0.0 && cos_l > 0.0 && cos_x > 0.0;            // (false for a NaN)
                    G = (cos_l * A) / fmax(r2, A);
                }
                // (every component of x and d is finite on a live lane: one that is not makes r2, and so a cosine, inf or NaN)
#pragma unroll
                for (int i = 0; i < 3; ++i) ray.o[i] = v.x[i], ray.d[i] = d[i], ray.inv[i] = 1.0 / d[i];
                ray.tmin = kr->eps;
                tmax = kr->tmax;
            }
            Best best{tmax, 0.0, 0.0, -1};
            int n_box = 0, n_tri = 0;
            // (TAKE_ANEW: the face count is taken anew at every step: the masks the walk derives from it are then made here, not
            // kept in scalar registers over the whole kernel, where section Y's binary64 exp and log hold their constants)
            int64_t n_f_now = n_f;
            if constexpr (Draw::TAKE_ANEW) asm volatile("" : "+v"(n_f_now));
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
                            const double add = v.T[c] * (double)L[c];
                            if (b == 0) env_dir[c] = env_dir[c] + add;
                            else env_indir[c] = env_indir[c] + add;
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
                        v.x[i] = (wa * kh->vertices[3 * ia + i] + best.u * kh->vertices[3 * ib + i]) + best.v * kh->vertices[3 * ic + i];
                        nn[i] = (fa * kh->v_normal[3 * ia + i] + fu * kh->v_normal[3 * ib + i]) + fv * kh->v_normal[3 * ic + i];
                        v.base[i] = (fa * kh->v_base[3 * ia + i] + fu * kh->v_base[3 * ib + i]) + fv * kh->v_base[3 * ic + i];
                        v.wo[i] = -wi[i];
                    }
                    v.rough = (fa * kh->v_rough[ia] + fu * kh->v_rough[ib]) + fv * kh->v_rough[ic];
                    v.metal = (fa * kh->v_metal[ia] + fu * kh->v_metal[ib]) + fv * kh->v_metal[ic];
                    v.face = best.face;
                    const float len = sqrtf((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
                    bool alive = len > 0.f && len < INFINITY;
                    if (alive) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) v.n[i] = nn[i] / len;
                        alive = (v.n[0] * v.wo[0] + v.n[1] * v.wo[1]) + v.n[2] * v.wo[2] > 0.f;      // (false for a NaN, and for a back face)
                    }
                    if (!alive) code = 2, path_ends = true, ++b;
                    else if (kh->n_sources > 0) src = 0;
                    else next_segment = true;
                }
            } else {
                if (live && best.face < 0) {
                    const float *E = kh->l_radiance + 3 * slot;
                    const Disney R = disney_eval(v.base, v.rough, v.metal, v.n, wi, v.wo);
                    const double kp = (double)(1 << kh->lgp);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double term = (((double)R.R[c] * kInv2Pi) * G) * (double)E[c];
                        src_indir[c] = src_indir[c] + v.T[c] * (kp * term);
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
                if (kh->trace)
                    for (int bb = b; bb < kh->depth; ++bb) kh->trace[path * kh->depth + bb] = -2;
                if (kh->end) kh->end[path] = code;
                s += kd, b = 0, src = -1;
                first_vertex();
            }
        }
        // the interleaved butterfly of the nine sums and the count: every lane of the group is here (its lanes share p)
        int kd_now = kd, k_now = k;                                          // (TAKE_ANEW: as n_f_now above)
        if constexpr (Draw::TAKE_ANEW) asm volatile("" : "+v"(kd_now), "+v"(k_now));
        for (int off = 1; off < kd_now; off <<= 1) {
#pragma unroll
            for (int c = 0; c < 9; ++c) sum(c) = sum(c) + __shfl_xor(sum(c), off);
            open += __shfl_xor(open, off);
        }
        if (k_now == 0) {
            const KernArgs ko = kernargs();
            const double N = (double)ko->n_paths;
#pragma unroll
            for (int c = 0; c < 9; ++c) ko->out[9 * p + c] = (float)(sum(c) / N);
            if (ko->n_open) ko->n_open[p] = open;
        }
    }
}

bool given(const void *p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
bool optional(const void *p, size_t a) { return !p || ((uintptr_t)p & (a - 1)) == 0; }

// Sections X's and Y's checks of a call's arguments (a: as the entry received them, lg, lgp and stride 0), then the mode's kernel
int path_launch(PathArgs a, int32_t slots, int32_t mode, void *stream, void (*reflect)(PathArgs), void (*irradiance)(PathArgs))
{
    if (a.n_faces < 0 || a.n_vertices < 0 || a.n_sources < 0 || a.n_points < 0 || a.n_sg < 0 || (mode != 0 && mode != 1) || slots < 1 ||
        !(a.eps >= 0.0 && a.eps < 0.5) || a.n_paths < 1 || a.depth < 1 || a.rr_start < 1 || !(a.t_min >= 0.0) || a.point_base < 0)
        return ESR_EINVAL;
    const int64_t cap = (int64_t)1 << 31;
    if (a.n_faces >= cap || a.n_vertices >= cap || a.n_sources >= cap || a.n_points >= cap || slots > ESR_SURFACE_LIGHT_MAX_SLOTS ||
        a.n_sg > ESR_SURFACE_ENV_MAX_SG || a.n_paths > ESR_SURFACE_PATH_MAX_PATHS || a.depth > ESR_SURFACE_PATH_MAX_DEPTH ||
        a.point_base > ((int64_t)1 << 32) - a.n_points)
        return ESR_ECAP;
    if (slots & (slots - 1)) return ESR_EINVAL;
    if (!a.n_points) return 0;
    if (!given(a.p_point, 8) || !given(a.p_normal, 4) || !optional(a.p_face, 4) || !given(a.out, 4) || !optional(a.n_open, 4) || !optional(a.trace, 4))
        return ESR_EINVAL;
    if (mode == 0 && (!given(a.p_base, 4) || !given(a.p_rough, 4) || !given(a.p_metal, 4) || !given(a.p_wo, 4))) return ESR_EINVAL;
    if (a.n_faces && (!given(a.vertices, 8) || !given(a.triangles, 8) || !given(a.v_normal, 4) || !given(a.v_base, 4) ||
                      !given(a.v_rough, 4) || !given(a.v_metal, 4)))
        return ESR_EINVAL;
    if (a.n_faces > 1 && !given(a.nodes, 16)) return ESR_EINVAL;
    if (a.n_sources && (!given(a.l_point, 8) || !given(a.l_normal, 8) || !given(a.l_weight, 8) || !given(a.l_radiance, 4) || !given(a.l_face, 4)))
        return ESR_EINVAL;
    if (a.n_sg && (!given(a.mus, 4) || !given(a.lambdas, 4) || !given(a.lobes, 4))) return ESR_EINVAL;
    while (a.lg < 6 && (1 << a.lg) < a.n_paths) ++a.lg;
    while ((1 << a.lgp) < slots) ++a.lgp;
    const int grid = esr_grid_for(a.n_points, SP_THREADS >> a.lg, SP_BLOCKS);
    a.stride = (int64_t)grid * (SP_THREADS >> a.lg);
    (mode == 0 ? reflect : irradiance)<<<grid, SP_THREADS, 0, esr_stream(stream)>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}

}  // namespace
