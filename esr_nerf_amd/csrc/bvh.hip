// Ray casting against the exported surface (esr_nerf_amd/raycast.py): a linear BVH over the faces, built on the device, and
// a nearest-hit / any-hit walk.  Section T of include/esr_hip.h is the definition; tests/raycast_ref.py restates it.
//
// The reference has nothing of the kind: it hands its mesh to trimesh (app/fine/pdra.py:781).
//
// Build (torch sorts between the first and the second pass):
//   bvh_keys_kernel   one lane per face: the face's box (binary32, rounded outward) and the 63-bit Morton key of the box's centre
//   bvh_tree_kernel   one lane per internal node: the radix tree of Karras 2012 over the sorted keys, equal keys told apart
//                     by their position; a node holds the links AND the boxes of its two children (64 bytes, one record per
//                     step of the walk)
//   bvh_fit_kernel    one lane per leaf climbs; the first lane to arrive at a node stores its box and ends, the second
//                     takes the union and goes on.  min / max are exact: the boxes do not depend on who arrived first
// Walk (bvh_nearest_kernel / bvh_anyhit_kernel, one lane per ray): the stack-less walk and the triangle test of bvh_walk.h,
// which surflight.hip shares.
#include "bvh_walk.h"

namespace {

constexpr int BV_THREADS = 256;
constexpr int BV_BLOCKS = 2048;
constexpr int64_t BV_CELLS = (int64_t)1 << 21;

typedef esr_bvh_node_t Node;

// x rounded to binary32 towards -inf / +inf: the nearest value, stepped once where it lies on the wrong side
__device__ __forceinline__ float round_down(double x)
{
    const float f = (float)x;
    return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
__device__ __forceinline__ float round_up(double x)
{
    const float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
}

// bit k of c -> bit 3 k
__device__ __forceinline__ uint64_t spread3(uint64_t c)
{
    c &= 0x1fffff;
    c = (c | c << 32) & 0x1f00000000ffffull;
    c = (c | c << 16) & 0x1f0000ff0000ffull;
    c = (c | c << 8) & 0x100f00f00f00f00full;
    c = (c | c << 4) & 0x10c30c30c30c30c3ull;
    c = (c | c << 2) & 0x1249249249249249ull;
    return c;
}

__global__ void __launch_bounds__(BV_THREADS) bvh_keys_kernel(const double *__restrict__ verts, int64_t n_v,
                                                              const int64_t *__restrict__ tris, int64_t n_f,
                                                              const double *__restrict__ scene, int64_t *__restrict__ keys,
                                                              float *__restrict__ boxes)
{
#pragma clang fp contract(off)
    const double slo[3] = {scene[0], scene[1], scene[2]}, shi[3] = {scene[3], scene[4], scene[5]};
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_f; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id[3] = {tris[3 * f], tris[3 * f + 1], tris[3 * f + 2]};
        bool ok = (uint64_t)id[0] < (uint64_t)n_v && (uint64_t)id[1] < (uint64_t)n_v && (uint64_t)id[2] < (uint64_t)n_v;
        double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
        if (ok) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double a = verts[3 * id[0] + i], b = verts[3 * id[1] + i], c = verts[3 * id[2] + i];
                ok = ok && fabs(a) < INFINITY && fabs(b) < INFINITY && fabs(c) < INFINITY;
                lo[i] = fmin(fmin(a, b), c), hi[i] = fmax(fmax(a, b), c);
            }
        }
        uint64_t key = (uint64_t)INT64_MAX;
        if (ok) {
            uint64_t cell[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double c = 0.5 * lo[i] + 0.5 * hi[i], ext = shi[i] - slo[i];
                const double x = ext > 0.0 ? floor(((c - slo[i]) / ext) * (double)BV_CELLS) : 0.0;
                cell[i] = x >= 0.0 ? (x < (double)BV_CELLS ? (uint64_t)x : (uint64_t)(BV_CELLS - 1)) : 0;   // (NaN -> 0)
            }
            key = spread3(cell[0]) << 2 | spread3(cell[1]) << 1 | spread3(cell[2]);
        }
        keys[f] = (int64_t)key;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            boxes[6 * f + i] = ok ? round_down(lo[i]) : INFINITY;
            boxes[6 * f + 3 + i] = ok ? round_up(hi[i]) : -INFINITY;
        }
    }
}

// the length of the common prefix of the (key, position) pairs i and j, -1 for a j outside the array
__device__ __forceinline__ int prefix(const int64_t *__restrict__ keys, int64_t n, int64_t ki, int64_t i, int64_t j)
{
    if (j < 0 || j >= n) return -1;
    const int64_t kj = keys[j];
    return ki == kj ? 64 + __clz((unsigned)(i ^ j)) : __clzll((unsigned long long)(ki ^ kj));
}

__global__ void __launch_bounds__(BV_THREADS) bvh_tree_kernel(const int64_t *__restrict__ keys,
                                                              const int64_t *__restrict__ order, int64_t n,
                                                              Node *__restrict__ nodes, int32_t *__restrict__ leaf_parent)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n - 1; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ki = keys[i];
        const int dir = prefix(keys, n, ki, i, i + 1) > prefix(keys, n, ki, i, i - 1) ? 1 : -1;
        const int dmin = prefix(keys, n, ki, i, i - dir);
        int64_t lmax = 2;
        while (prefix(keys, n, ki, i, i + lmax * dir) > dmin) lmax <<= 1;      // (at most 31 doublings: n < 2^31)
        int64_t l = 0;
        for (int64_t t = lmax >> 1; t > 0; t >>= 1)
            if (prefix(keys, n, ki, i, i + (l + t) * dir) > dmin) l += t;
        const int64_t j = i + l * dir;
        const int dnode = prefix(keys, n, ki, i, j);
        int64_t s = 0;
        for (int64_t t = (l + 1) >> 1;; t = (t + 1) >> 1) {
            if (prefix(keys, n, ki, i, i + (s + t) * dir) > dnode) s += t;
            if (t <= 1) break;
        }
        const int64_t g = i + s * dir + (dir < 0 ? -1 : 0);                    // the last position of the left child
        const int64_t first = dir > 0 ? i : j, last = dir > 0 ? j : i;
        const int64_t c[2] = {g, g + 1};
        const bool leaf[2] = {g == first, g + 1 == last};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            int32_t link;
            if (leaf[k]) {
                const int64_t f = order[c[k]];
                link = (uint64_t)f < (uint64_t)n ? ~(int32_t)f : ~(int32_t)c[k];      // (a face id outside the mesh: never followed)
                leaf_parent[c[k]] = (int32_t)(2 * i + k);
            } else {
                link = (int32_t)c[k];
                nodes[c[k]].parent = (int32_t)(2 * i + k);
            }
            nodes[i].child[k] = link;
        }
        nodes[i].pad = 0;
        if (i == 0) nodes[0].parent = -1;
    }
}

__global__ void __launch_bounds__(BV_THREADS) bvh_fit_kernel(Node *nodes, const int32_t *__restrict__ leaf_parent,
                                                             const int64_t *__restrict__ order,
                                                             const float *__restrict__ boxes, int64_t n, int32_t *counters,
                                                             float *root_box)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = order[i];
        float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if ((uint64_t)f < (uint64_t)n) {
#pragma unroll
            for (int k = 0; k < 6; ++k) b[k] = boxes[6 * f + k];
        }
        int32_t link = n > 1 ? leaf_parent[i] : -1;
        // every step takes the lane one level up: at most 63 + 31 of them, and no lane waits for another
        for (int level = 0; level < 128 && link >= 0; ++level) {
            const int64_t p = link >> 1;
            const int side = link & 1;
            if (p >= n - 1) break;                                             // (a link outside the tree: never followed)
            float *mine = nodes[p].box[side];
#pragma unroll
            for (int k = 0; k < 6; ++k) __hip_atomic_store(mine + k, b[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // release: the box is visible on the device before the count.  (The chip's L2 is one per XCD: the fence writes the
            // lines back, which is most of this kernel's time; the acquiring half is paid by the second arrival alone.)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const int32_t seen = __hip_atomic_fetch_add(counters + p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == 0) {
                link = -2;                                                     // the first to arrive ends here
                break;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                 // the sibling's box, stored before ITS count
            const float *other = nodes[p].box[1 - side];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                b[k] = fminf(b[k], __hip_atomic_load(other + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                b[3 + k] = fmaxf(b[3 + k], __hip_atomic_load(other + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
            link = __hip_atomic_load(&nodes[p].parent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (link == -1) {
#pragma unroll
            for (int k = 0; k < 6; ++k) root_box[k] = b[k];
        }
    }
}

struct CastArgs {
    BvhScene scene;
    const double *o, *d;
    int64_t n;
    const double *tmin, *tmax;
    double tmin_all, tmax_all;
    const int32_t *skip;
    int32_t *face;
    double *t, *bary;
    uint8_t *hit;
    int32_t *stats;
};

template <bool ANY> __device__ __forceinline__ void cast_rays(const CastArgs &a)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        Ray r;
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r.o[k] = a.o[3 * i + k], r.d[k] = a.d[3 * i + k];
            r.inv[k] = 1.0 / r.d[k];
            finite = finite && fabs(r.o[k]) < INFINITY && fabs(r.d[k]) < INFINITY;
        }
        r.tmin = a.tmin ? a.tmin[i] : a.tmin_all;
        const double tmax = a.tmax ? a.tmax[i] : a.tmax_all;
        const int32_t skip = a.skip ? a.skip[i] : -1;
        Best best{tmax, 0.0, 0.0, -1};
        int n_box = 0, n_tri = 0;
        bvh_walk<ANY>(a.scene, r, finite, skip, tmax, best, n_box, n_tri);
        if (ANY) {
            a.hit[i] = best.face >= 0 ? 1 : 0;
        } else {
            a.face[i] = best.face;
            a.t[i] = best.face >= 0 ? best.t : INFINITY;
            a.bary[2 * i] = best.face >= 0 ? best.u : 0.0;
            a.bary[2 * i + 1] = best.face >= 0 ? best.v : 0.0;
        }
        if (a.stats) a.stats[2 * i] = n_box, a.stats[2 * i + 1] = n_tri;
    }
}

__global__ void __launch_bounds__(BV_THREADS) bvh_nearest_kernel(CastArgs a) { cast_rays<false>(a); }
__global__ void __launch_bounds__(BV_THREADS) bvh_anyhit_kernel(CastArgs a) { cast_rays<true>(a); }

bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

ESR_API int esr_bvh_keys(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces,
                         const double *scene_box, int64_t *keys, float *boxes, void *stream)
{
    if (n_vertices < 0 || n_faces < 0) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31 || n_vertices >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_faces) return 0;
    if (!triangles || !scene_box || !keys || !boxes || !aligned(triangles, 8) || !aligned(scene_box, 8) || !aligned(keys, 8) ||
        !aligned(boxes, 4) || (n_vertices && (!vertices || !aligned(vertices, 8))))
        return ESR_EINVAL;
    bvh_keys_kernel<<<esr_grid_for(n_faces, BV_THREADS, BV_BLOCKS), BV_THREADS, 0, esr_stream(stream)>>>(
        vertices, n_vertices, triangles, n_faces, scene_box, keys, boxes);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_bvh_tree(const int64_t *sorted_keys, const int64_t *order, int64_t n_faces, esr_bvh_node_t *nodes,
                         int32_t *leaf_parent, void *stream)
{
    if (n_faces < 0) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31) return ESR_ECAP;
    if (n_faces < 2) return 0;
    if (!sorted_keys || !order || !nodes || !leaf_parent || !aligned(sorted_keys, 8) || !aligned(order, 8) || !aligned(nodes, 16) ||
        !aligned(leaf_parent, 4))
        return ESR_EINVAL;
    bvh_tree_kernel<<<esr_grid_for(n_faces - 1, BV_THREADS, BV_BLOCKS), BV_THREADS, 0, esr_stream(stream)>>>(
        sorted_keys, order, n_faces, nodes, leaf_parent);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_bvh_fit(esr_bvh_node_t *nodes, const int32_t *leaf_parent, const int64_t *order, const float *boxes,
                        int64_t n_faces, int32_t *counters, float *root_box, void *stream)
{
    if (n_faces < 0) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_faces) return 0;
    if (!order || !boxes || !root_box || !aligned(order, 8) || !aligned(boxes, 4) || !aligned(root_box, 4)) return ESR_EINVAL;
    if (n_faces > 1 && (!nodes || !leaf_parent || !counters || !aligned(nodes, 16) || !aligned(leaf_parent, 4) || !aligned(counters, 4)))
        return ESR_EINVAL;
    hipStream_t s = esr_stream(stream);
    if (n_faces > 1) {
        hipError_t e = hipMemsetAsync(counters, 0, (size_t)(n_faces - 1) * sizeof(int32_t), s);
        if (e != hipSuccess) return (int)e;
    }
    bvh_fit_kernel<<<esr_grid_for(n_faces, BV_THREADS, BV_BLOCKS), BV_THREADS, 0, s>>>(nodes, leaf_parent, order, boxes, n_faces,
                                                                                      counters, root_box);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_bvh_cast(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                         const int64_t *triangles, const double *rays_o, const double *rays_d, int64_t n_rays,
                         const double *t_min, const double *t_max, double t_min_all, double t_max_all, const int32_t *skip_face,
                         int32_t any_hit, int32_t *face, double *t, double *bary, uint8_t *hit, int32_t *stats, void *stream)
{
    if (n_faces < 0 || n_vertices < 0 || n_rays < 0 || (any_hit != 0 && any_hit != 1)) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31 || n_vertices >= (int64_t)1 << 31 || n_rays >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_rays) return 0;
    if (!rays_o || !rays_d || !aligned(rays_o, 8) || !aligned(rays_d, 8) || !aligned(t_min, 8) || !aligned(t_max, 8) ||
        !aligned(skip_face, 4) || !aligned(stats, 4))
        return ESR_EINVAL;
    if (any_hit ? !hit : (!face || !t || !bary || !aligned(face, 4) || !aligned(t, 8) || !aligned(bary, 8))) return ESR_EINVAL;
    if (n_faces && (!vertices || !triangles || !aligned(vertices, 8) || !aligned(triangles, 8))) return ESR_EINVAL;
    if (n_faces > 1 && (!nodes || !aligned(nodes, 16))) return ESR_EINVAL;
    CastArgs a{{nodes, n_faces, vertices, n_vertices, triangles}, rays_o, rays_d, n_rays, t_min, t_max, t_min_all, t_max_all,
               skip_face, face, t, bary, hit, stats};
    const int grid = esr_grid_for(n_rays, BV_THREADS, BV_BLOCKS);
    if (any_hit) bvh_anyhit_kernel<<<grid, BV_THREADS, 0, esr_stream(stream)>>>(a);
    else bvh_nearest_kernel<<<grid, BV_THREADS, 0, esr_stream(stream)>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}
