// Surface components: connected components of a triangle mesh and per-component reductions.
//
// What a reference user runs on the host copy of an extracted mesh (trimesh.split / scipy.sparse.csgraph after
// trimesh.Trimesh(vertices, triangles), app/fine/pdra.py:781, lts.py:659, fine.py:632); here on the device, for the
// floater filter of an extracted surface and for the list of emissive sources (esr_nerf_amd/sources.py).
//
// Contract (restated in numpy by tests/surface_ref.py):
//   - two SELECTED faces are connected iff they share a vertex id (vertex connectivity, not edge adjacency); an unselected
//     face links nothing and is labelled -1.
//   - a component is named by the smallest vertex id it contains; components that own at least one selected face are
//     numbered 0 .. K-1 in increasing order of that id.  Every output is therefore a function of the input alone.
//   - statistics per component: face count; area = sum 0.5 |(b - a) x (c - a)|; area_centroid = sum area (a + b + c) / 3;
//     the bounding box of the face vertices; with an attribute [V, C]: area_attr = sum area * mean of the three rows, and
//     peak = the largest attribute value at a face vertex.  Counts, box and peak are exact (integer adds, integer-key
//     minimum / maximum); the f64 sums are atomic adds, whose order moves the last bits from run to run.
//
// Union-find (cc_link_kernel).  parent[] only ever decreases: a root is hooked under a SMALLER root with a
// compare-and-swap that succeeds only while it still is a root, and a path is shortened with atomicMin towards an
// ancestor.  So a component's root ends as its smallest id, a stale parent is still an ancestor, and a failed
// compare-and-swap means another lane made progress: there are retries but no waiting on another wave.  The L2s of the
// XCDs are not coherent for plain accesses, so inside that launch every read of parent[] is a relaxed agent-scope atomic
// load and every write an agent-scope atomic; the launches before and after it publish parent[] at their boundaries.
//
// Statistics (cc_stats_kernel).  Marching cubes emits faces cell by cell: neighbouring faces nearly always carry one
// label and the main surface owns nearly every face, so an atomic per lane would put every add on one address.  Each lane
// keeps private sums while its whole wave reads one label (a ballot decides); a wave with mixed labels reduces each run
// of equal neighbouring labels with a segmented shuffle scan and the last lane of a run issues the atomics.  The private
// sums are reduced over the wave when the label changes and at the end, where the waves of a block that hold the same
// label combine through LDS: one atomic per quantity per block in the common case.
#include "esr_common.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_BLOCKS = 256;            // most workgroups of the per-face launches (one per CU; lanes stride the faces)
constexpr int CC_MAX_ATTR = 4;

__device__ __forceinline__ int32_t ld_parent(int32_t *parent, int32_t v)
{
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v; on the way every visited node is pointed at its grandparent (atomicMin: parents only decrease)
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t v)
{
    int32_t p = ld_parent(parent, v);
    while (p != v) {
        const int32_t g = ld_parent(parent, p);
        if (g != p) __hip_atomic_fetch_min(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = p;
        p = g;
    }
    return v;
}

__device__ __forceinline__ void cc_union(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        int32_t expect = a;                                    // hook the larger root under the smaller one
        if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

__global__ void __launch_bounds__(CC_THREADS) cc_init_kernel(int32_t *__restrict__ parent, int64_t n_v)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (int64_t)gridDim.x * blockDim.x)
        parent[v] = (int32_t)v;
}

__global__ void __launch_bounds__(CC_THREADS) cc_link_kernel(const int64_t *__restrict__ tris,
                                                             const uint8_t *__restrict__ face_mask, int64_t n_f,
                                                             int32_t *parent)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_f; f += (int64_t)gridDim.x * blockDim.x) {
        if (face_mask && !face_mask[f]) continue;
        const int32_t v0 = (int32_t)tris[3 * f], v1 = (int32_t)tris[3 * f + 1], v2 = (int32_t)tris[3 * f + 2];
        cc_union(parent, v0, v1);
        cc_union(parent, v0, v2);
    }
}

// parent[v] = root(v).  Other lanes of this launch overwrite parent[] with roots meanwhile, so the accesses stay atomic;
// whichever value a lane reads is an ancestor of the node it came from.
__global__ void __launch_bounds__(CC_THREADS) cc_flatten_kernel(int32_t *parent, int64_t n_v)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (int64_t)gridDim.x * blockDim.x) {
        int32_t r = (int32_t)v, p = ld_parent(parent, r);
        while (p != r) {
            r = p;
            p = ld_parent(parent, r);
        }
        if (r != (int32_t)v) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// owner[root] = 1 for the root of every selected face (every writer stores the same 1)
__global__ void __launch_bounds__(CC_THREADS) cc_owner_kernel(const int64_t *__restrict__ tris,
                                                              const uint8_t *__restrict__ face_mask, int64_t n_f,
                                                              const int32_t *__restrict__ parent,
                                                              int32_t *__restrict__ owner)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_f; f += (int64_t)gridDim.x * blockDim.x) {
        if (face_mask && !face_mask[f]) continue;
        owner[parent[tris[3 * f]]] = 1;
    }
}

__global__ void __launch_bounds__(CC_THREADS) cc_face_labels_kernel(const int64_t *__restrict__ tris,
                                                                    const uint8_t *__restrict__ face_mask, int64_t n_f,
                                                                    const int32_t *__restrict__ parent,
                                                                    const int32_t *__restrict__ rank,
                                                                    int32_t *__restrict__ label)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_f; f += (int64_t)gridDim.x * blockDim.x)
        label[f] = (face_mask && !face_mask[f]) ? -1 : rank[parent[tris[3 * f]]];
}

// ---------------------------------------------------------------------------------------------------------------------
// statistics

struct StatsOut {
    int64_t *n_faces;          // [K]
    double *area;              // [K]
    double *area_centroid;     // [K,3]
    double *bbox_min;          // [K,3]
    double *bbox_max;          // [K,3]
    double *area_attr;         // [K,C] or NULL
    float *peak;               // [K] or NULL
    int32_t n_attr;            // C
};

// one face's (or a run's, a wave's, a block's) contribution
struct Acc {
    uint32_t n;
    double area, ac[3], lo[3], hi[3], aa[CC_MAX_ATTR];
    float peak;
};

__device__ __forceinline__ void acc_clear(Acc &a)
{
    a.n = 0;
    a.area = 0.0;
    a.peak = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.ac[k] = 0.0;
        a.lo[k] = INFINITY;
        a.hi[k] = -INFINITY;
    }
#pragma unroll
    for (int c = 0; c < CC_MAX_ATTR; ++c) a.aa[c] = 0.0;
}

__device__ __forceinline__ void acc_merge(Acc &a, const Acc &b)
{
    a.n += b.n;
    a.area += b.area;
    a.peak = fmaxf(a.peak, b.peak);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.ac[k] += b.ac[k];
        a.lo[k] = fmin(a.lo[k], b.lo[k]);
        a.hi[k] = fmax(a.hi[k], b.hi[k]);
    }
#pragma unroll
    for (int c = 0; c < CC_MAX_ATTR; ++c) a.aa[c] += b.aa[c];
}

// `a` of lane (lane ^ m) / (lane - d)
__device__ __forceinline__ Acc acc_shfl_xor(const Acc &a, int m)
{
    Acc b;
    b.n = __shfl_xor(a.n, m);
    b.area = __shfl_xor(a.area, m);
    b.peak = __shfl_xor(a.peak, m);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.ac[k] = __shfl_xor(a.ac[k], m);
        b.lo[k] = __shfl_xor(a.lo[k], m);
        b.hi[k] = __shfl_xor(a.hi[k], m);
    }
#pragma unroll
    for (int c = 0; c < CC_MAX_ATTR; ++c) b.aa[c] = __shfl_xor(a.aa[c], m);
    return b;
}

__device__ __forceinline__ Acc acc_shfl_up(const Acc &a, int d)
{
    Acc b;
    b.n = __shfl_up(a.n, d);
    b.area = __shfl_up(a.area, d);
    b.peak = __shfl_up(a.peak, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.ac[k] = __shfl_up(a.ac[k], d);
        b.lo[k] = __shfl_up(a.lo[k], d);
        b.hi[k] = __shfl_up(a.hi[k], d);
    }
#pragma unroll
    for (int c = 0; c < CC_MAX_ATTR; ++c) b.aa[c] = __shfl_up(a.aa[c], d);
    return b;
}

// Exact minimum / maximum through integer atomics: for values >= 0 the bit pattern orders as a signed integer, for values
// < 0 it orders the other way round as an unsigned one, and either kind loses against the other as it should (the slot
// starts at +inf for a minimum, -inf for a maximum).  v + 0 turns -0 into +0.
__device__ __forceinline__ void atomic_min_f64(double *p, double v)
{
    v += 0.0;
    if (v >= 0.0) atomicMin((long long *)p, __double_as_longlong(v));
    else atomicMax((unsigned long long *)p, (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ void atomic_max_f64(double *p, double v)
{
    v += 0.0;
    if (v >= 0.0) atomicMax((long long *)p, __double_as_longlong(v));
    else atomicMin((unsigned long long *)p, (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ void atomic_max_f32(float *p, float v)
{
    v += 0.f;
    if (v >= 0.f) atomicMax((int *)p, __float_as_int(v));
    else atomicMin((unsigned *)p, __float_as_uint(v));
}

// one lane adds a finished partial to component `label`
__device__ __forceinline__ void acc_commit(const StatsOut &O, int32_t label, const Acc &a)
{
    if (label < 0 || a.n == 0) return;
    atomicAdd((unsigned long long *)O.n_faces + label, (unsigned long long)a.n);
    unsafeAtomicAdd(O.area + label, a.area);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        unsafeAtomicAdd(O.area_centroid + 3 * (int64_t)label + k, a.ac[k]);
        atomic_min_f64(O.bbox_min + 3 * (int64_t)label + k, a.lo[k]);
        atomic_max_f64(O.bbox_max + 3 * (int64_t)label + k, a.hi[k]);
    }
    if (O.n_attr) {
#pragma unroll
        for (int c = 0; c < CC_MAX_ATTR; ++c)
            if (c < O.n_attr) unsafeAtomicAdd(O.area_attr + (int64_t)O.n_attr * label + c, a.aa[c]);
        atomic_max_f32(O.peak + label, a.peak);
    }
}

// every lane gets the wave's total
__device__ __forceinline__ void acc_wave_reduce(Acc &a)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const Acc b = acc_shfl_xor(a, m);
        acc_merge(a, b);
    }
}

// one face's terms, each operation rounded on its own in the order tests/surface_ref.py writes them
__device__ __forceinline__ void face_terms(const double *__restrict__ verts, const float *__restrict__ attr, int n_attr,
                                           const int64_t v[3], Acc &t)
{
#pragma clang fp contract(off)
    double p[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) p[i][k] = verts[3 * v[i] + k];
    double e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = p[1][k] - p[0][k];
        e2[k] = p[2][k] - p[0][k];
    }
    const double cx = e1[1] * e2[2] - e1[2] * e2[1];
    const double cy = e1[2] * e2[0] - e1[0] * e2[2];
    const double cz = e1[0] * e2[1] - e1[1] * e2[0];
    const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    t.n = 1;
    t.area = area;
    t.peak = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.ac[k] = area * (((p[0][k] + p[1][k]) + p[2][k]) / 3.0);
        t.lo[k] = fmin(fmin(p[0][k], p[1][k]), p[2][k]);
        t.hi[k] = fmax(fmax(p[0][k], p[1][k]), p[2][k]);
    }
#pragma unroll
    for (int c = 0; c < CC_MAX_ATTR; ++c) {
        t.aa[c] = 0.0;
        if (c < n_attr) {
            const float x0 = attr[n_attr * v[0] + c], x1 = attr[n_attr * v[1] + c], x2 = attr[n_attr * v[2] + c];
            t.aa[c] = area * ((((double)x0 + (double)x1) + (double)x2) / 3.0);
            t.peak = fmaxf(t.peak, fmaxf(fmaxf(x0, x1), x2));
        }
    }
}

template <bool PRE_REDUCE>
__global__ void __launch_bounds__(CC_THREADS) cc_stats_kernel(const double *__restrict__ verts,
                                                              const int64_t *__restrict__ tris,
                                                              const int32_t *__restrict__ face_label, int64_t n_f,
                                                              const float *__restrict__ attr, StatsOut O)
{
    __shared__ Acc s_acc[CC_THREADS / 64];
    __shared__ int32_t s_label[CC_THREADS / 64];
    const int lane = esr_lane(), wave = threadIdx.x >> 6;
    Acc mine;                                  // this lane's private sums for component `held` (wave-uniform)
    acc_clear(mine);
    int32_t held = -1;
    // every lane of a wave runs the same number of trips: the ballots and shuffles below need all 64 lanes
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
    for (int64_t base = first; base < n_f; base += stride) {
        const int64_t f = base + lane;
        int32_t label = -1;
        Acc t;
        acc_clear(t);
        if (f < n_f) label = face_label[f];
        if (label >= 0) {
            const int64_t v[3] = {tris[3 * f], tris[3 * f + 1], tris[3 * f + 2]};
            face_terms(verts, attr, O.n_attr, v, t);
        }
        if (!PRE_REDUCE) {
            acc_commit(O, label, t);
            continue;
        }
        const uint64_t live = __ballot(label >= 0);
        if (!live) continue;
        const int32_t l0 = __shfl(label, __ffsll((long long)live) - 1);
        if (__all(label < 0 || label == l0)) {
            // one label in the wave: private sums, no traffic (lanes without a face add the identity)
            if (held != l0) {
                if (held >= 0) {
                    acc_wave_reduce(mine);
                    if (lane == 0) acc_commit(O, held, mine);
                    acc_clear(mine);
                }
                held = l0;
            }
            acc_merge(mine, t);
            continue;
        }
        // mixed labels: inclusive segmented scan over each run of equal neighbouring labels; the run's last lane commits
        const int32_t prev = __shfl_up(label, 1);
        const uint64_t heads = __ballot(lane == 0 || label != prev);
        const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Acc b = acc_shfl_up(t, d);
            if (lane - d >= head) acc_merge(t, b);
        }
        if (lane == 63 || ((heads >> (lane + 1)) & 1)) acc_commit(O, label, t);
    }
    if (!PRE_REDUCE) return;
    // the end: waves of the block that hold the same component combine through LDS
    acc_wave_reduce(mine);
    if (lane == 0) {
        s_acc[wave] = mine;
        s_label[wave] = held;
    }
    __syncthreads();
    if (lane != 0) return;
    bool same = true;
    for (int w = 1; w < CC_THREADS / 64; ++w) same &= s_label[w] == s_label[0];
    if (!same) {
        acc_commit(O, held, mine);
    } else if (wave == 0) {
        for (int w = 1; w < CC_THREADS / 64; ++w) acc_merge(mine, s_acc[w]);
        acc_commit(O, held, mine);
    }
}

__global__ void __launch_bounds__(CC_THREADS) cc_stats_init_kernel(StatsOut O, int64_t k_comp)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k_comp; i += (int64_t)gridDim.x * blockDim.x) {
        O.n_faces[i] = 0;
        O.area[i] = 0.0;
        for (int k = 0; k < 3; ++k) {
            O.area_centroid[3 * i + k] = 0.0;
            O.bbox_min[3 * i + k] = INFINITY;
            O.bbox_max[3 * i + k] = -INFINITY;
        }
        for (int c = 0; c < O.n_attr; ++c) O.area_attr[(int64_t)O.n_attr * i + c] = 0.0;
        if (O.n_attr) O.peak[i] = -INFINITY;
    }
}

bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int cc_sizes(int64_t n_vertices, int64_t n_faces)
{
    if (n_vertices < 0 || n_faces < 0) return ESR_EINVAL;
    if (n_vertices >= (int64_t)1 << 31) return ESR_ECAP;
    return 0;
}

}  // namespace

ESR_API int esr_cc_link(const int64_t *triangles, const uint8_t *face_mask, int64_t n_faces, int64_t n_vertices,
                        int32_t *parent, void *stream)
{
    const int rc = cc_sizes(n_vertices, n_faces);
    if (rc) return rc;
    if ((n_faces && !triangles) || (n_vertices && !parent) || !aligned(triangles, 8) || !aligned(parent, 4))
        return ESR_EINVAL;
    if (n_faces && !n_vertices) return ESR_EINVAL;
    if (!n_vertices) return 0;
    cc_init_kernel<<<esr_grid_for(n_vertices, CC_THREADS), CC_THREADS, 0, esr_stream(stream)>>>(parent, n_vertices);
    ESR_CHECK_LAUNCH();
    if (!n_faces) return 0;
    cc_link_kernel<<<esr_grid_for(n_faces, CC_THREADS, CC_BLOCKS), CC_THREADS, 0, esr_stream(stream)>>>(
        triangles, face_mask, n_faces, parent);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cc_flatten(const int64_t *triangles, const uint8_t *face_mask, int64_t n_faces, int64_t n_vertices,
                           int32_t *parent, int32_t *owner, void *stream)
{
    const int rc = cc_sizes(n_vertices, n_faces);
    if (rc) return rc;
    if ((n_faces && !triangles) || (n_vertices && (!parent || !owner)) || !aligned(triangles, 8) || !aligned(parent, 4) ||
        !aligned(owner, 4))
        return ESR_EINVAL;
    if (n_faces && !n_vertices) return ESR_EINVAL;
    if (!n_vertices) return 0;
    hipError_t e = hipMemsetAsync(owner, 0, sizeof(int32_t) * (size_t)n_vertices, esr_stream(stream));
    if (e != hipSuccess) return (int)e;
    cc_flatten_kernel<<<esr_grid_for(n_vertices, CC_THREADS), CC_THREADS, 0, esr_stream(stream)>>>(parent, n_vertices);
    ESR_CHECK_LAUNCH();
    if (!n_faces) return 0;
    cc_owner_kernel<<<esr_grid_for(n_faces, CC_THREADS), CC_THREADS, 0, esr_stream(stream)>>>(triangles, face_mask, n_faces,
                                                                                              parent, owner);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cc_face_labels(const int64_t *triangles, const uint8_t *face_mask, int64_t n_faces, const int32_t *parent,
                               const int32_t *rank, int32_t *face_label, void *stream)
{
    if (n_faces < 0) return ESR_EINVAL;
    if (!n_faces) return 0;
    if (!triangles || !parent || !rank || !face_label || !aligned(triangles, 8) || !aligned(parent, 4) ||
        !aligned(rank, 4) || !aligned(face_label, 4))
        return ESR_EINVAL;
    cc_face_labels_kernel<<<esr_grid_for(n_faces, CC_THREADS), CC_THREADS, 0, esr_stream(stream)>>>(
        triangles, face_mask, n_faces, parent, rank, face_label);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cc_stats(const double *vertices, const int64_t *triangles, const int32_t *face_label, int64_t n_faces,
                         int64_t n_components, const float *attr, int32_t n_attr, int32_t per_lane_atomics,
                         int64_t *n_faces_out, double *area, double *area_centroid, double *bbox_min, double *bbox_max,
                         double *area_attr, float *peak, void *stream)
{
    if (n_faces < 0 || n_components < 0 || n_attr < 0 || n_attr > CC_MAX_ATTR) return ESR_EINVAL;
    if (n_components >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_components) return 0;
    if (!n_faces_out || !area || !area_centroid || !bbox_min || !bbox_max) return ESR_EINVAL;
    if ((n_attr != 0) != (attr != nullptr) || (n_attr && (!area_attr || !peak))) return ESR_EINVAL;
    if (n_faces && (!vertices || !triangles || !face_label)) return ESR_EINVAL;
    if (!aligned(vertices, 8) || !aligned(triangles, 8) || !aligned(face_label, 4) || !aligned(attr, 4) ||
        !aligned(n_faces_out, 8) || !aligned(area, 8) || !aligned(area_centroid, 8) || !aligned(bbox_min, 8) ||
        !aligned(bbox_max, 8) || !aligned(area_attr, 8) || !aligned(peak, 4))
        return ESR_EINVAL;
    StatsOut O = {n_faces_out, area, area_centroid, bbox_min, bbox_max, area_attr, peak, n_attr};
    cc_stats_init_kernel<<<esr_grid_for(n_components, CC_THREADS), CC_THREADS, 0, esr_stream(stream)>>>(O, n_components);
    ESR_CHECK_LAUNCH();
    if (!n_faces) return 0;
    const int grid = esr_grid_for(n_faces, CC_THREADS, CC_BLOCKS);
    if (per_lane_atomics)
        cc_stats_kernel<false><<<grid, CC_THREADS, 0, esr_stream(stream)>>>(vertices, triangles, face_label, n_faces, attr, O);
    else
        cc_stats_kernel<true><<<grid, CC_THREADS, 0, esr_stream(stream)>>>(vertices, triangles, face_label, n_faces, attr, O);
    ESR_CHECK_LAUNCH();
    return 0;
}
