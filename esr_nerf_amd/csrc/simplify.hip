// Surface simplification by quadric vertex clustering (esr_nerf_amd/mesh.py: simplify, simplify_to).
//
// The reference hands its marching-cubes mesh to trimesh as it is (app/fine/pdra.py:781); nothing there simplifies it.
//
// Definition (restated exactly in tests/simplify_ref.py).  The origin o is the per-axis minimum of the vertices, a vertex
// lies in the cell floor((v - o) / h) per axis (binary64, each operation rounded), a cluster is an occupied cell and
// clusters are numbered by ascending key x << 42 | y << 21 | z.  g_k = o + (c_k + 0.5) h is the centre of cluster k's cell,
// and everything below works on r = v - g_k, the binary64 difference (one rounding), of every vertex it touches.
//   members M_k, mean xbar_k = (sum r) / |M_k| clamped into the cell box [-h/2, h/2]^3 (a member on the cell's border may
//   sit an ulp outside after the subtraction)
//   incident faces I_k: the faces with a corner in k, each once.  For a face (a, b, c):  n = (b - a) x (c - a),
//   d = -n . a,  s = |b - a|^2 |c - a|^2,  w = |n| / 2
//   A = sum n n^T, b = sum n d, c = sum d d, S = sum s, W = sum w #corners in k, P = sum w sum_{corners in k} attr[corner]
//   position: S == 0 -> y = xbar; else (A + lam S I) y* = -b + lam S xbar and y = xbar + t (y* - xbar) with the largest
//   t in [0, 1] that keeps y in the box; the new vertex is g_k + y
//   attribute: float(P / W), or for W == 0 the attribute of the member with the smallest id
// The regulariser is S, not tr A: tr A <= S, so the matrix is SPD with condition number <= 1 + 1 / lam, and a collinear
// face, whose n is a rounding residue here, still adds its s.
//
// Order of the sums (binary64, contraction off, no atomics: a function of the input and of `big` alone).  A cluster's
// faces come as the segment of the sorted (cluster << 32 | face) pairs, its members as the segment of the vertex ids
// sorted by cluster.  A cluster of at most `big` pairs and members is one lane's loop (simplify_cluster_lane_kernel): faces by
// ascending id, then members by ascending id.  A larger cluster is summed by a workgroup (simplify_cluster_group_kernel):
// thread t adds the elements t, t + 256, ... of the segment in that order, then the 256 partial sums fold,
// x[t] += x[t + off] for off = 128, 64, ... 1.  Either way a cluster's sums, mean, solve, clip and attributes are one
// launch's work, and both paths call add_face, add_member and finish below.  The workgroups of the second launch stride
// over ALL clusters and pass the small ones by on two loads: no queue, no counter, nothing to order.
#include "esr_common.h"

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_BLOCKS = 2048;
constexpr int SM_GROUP_BLOCKS = 4096;     // most workgroups of the large-cluster launch (each strides over the clusters)
constexpr int SM_MAX_C = ESR_SIMPLIFY_MAX_C;
constexpr int64_t SM_AXIS = ((int64_t)1 << 21) - 1;       // most cells on an axis
constexpr int64_t SM_NONE = INT64_MAX;                    // the pair of a repeated cluster, the key of a degenerate face

struct Acc {
    double A[6], b[3], c, S, W, M[3];
    double P[SM_MAX_C];
};

struct ClusterArgs {
    const double *verts;
    int64_t n_v;
    const int64_t *tris;
    int64_t n_f;
    const int32_t *vc;
    const int64_t *ckeys;
    int64_t n_k;
    const int64_t *mstart, *mids, *pstart, *pairs;
    int64_t n_pairs;
    const double *origin;
    double h, lam;
    const float *attr;
    int n_c;
    int64_t big;
    double *pos;
    float *attr_out;
    double *debug;
};

__device__ __forceinline__ void acc_zero(Acc &q)
{
#pragma unroll
    for (int i = 0; i < 6; ++i) q.A[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) q.b[i] = 0.0, q.M[i] = 0.0;
    q.c = q.S = q.W = 0.0;
#pragma unroll
    for (int i = 0; i < SM_MAX_C; ++i) q.P[i] = 0.0;
}

__device__ __forceinline__ void cell_centre(const ClusterArgs &a, int64_t k, double g[3])
{
#pragma clang fp contract(off)
    const int64_t key = a.ckeys[k];
    const int64_t c[3] = {(key >> 42) & 0x1fffff, (key >> 21) & 0x1fffff, key & 0x1fffff};
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = a.origin[i] + ((double)c[i] + 0.5) * a.h;
}

// one incident face of cluster k (a face that names no vertex adds nothing)
__device__ __forceinline__ void add_face(Acc &q, const ClusterArgs &a, int64_t f, int32_t k, const double g[3])
{
#pragma clang fp contract(off)
    if ((uint64_t)f >= (uint64_t)a.n_f) return;
    const int64_t id[3] = {a.tris[3 * f], a.tris[3 * f + 1], a.tris[3 * f + 2]};
    if ((uint64_t)id[0] >= (uint64_t)a.n_v || (uint64_t)id[1] >= (uint64_t)a.n_v || (uint64_t)id[2] >= (uint64_t)a.n_v) return;
    double p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) p[j][i] = a.verts[3 * id[j] + i] - g[i];
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double n0 = e1[1] * e2[2] - e1[2] * e2[1];
    const double n1 = e1[2] * e2[0] - e1[0] * e2[2];
    const double n2 = e1[0] * e2[1] - e1[1] * e2[0];
    const double d = -((n0 * p[0][0] + n1 * p[0][1]) + n2 * p[0][2]);
    const double l1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    const double l2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    q.A[0] += n0 * n0, q.A[1] += n0 * n1, q.A[2] += n0 * n2, q.A[3] += n1 * n1, q.A[4] += n1 * n2, q.A[5] += n2 * n2;
    q.b[0] += n0 * d, q.b[1] += n1 * d, q.b[2] += n2 * d;
    q.c += d * d;
    q.S += l1 * l2;
    const double w = sqrt((n0 * n0 + n1 * n1) + n2 * n2) * 0.5;
    const bool in0 = a.vc[id[0]] == k, in1 = a.vc[id[1]] == k, in2 = a.vc[id[2]] == k;
    q.W += w * (double)((int)in0 + (int)in1 + (int)in2);
#pragma unroll
    for (int ch = 0; ch < SM_MAX_C; ++ch)
        if (ch < a.n_c) {
            double s = 0.0;
            if (in0) s += (double)a.attr[id[0] * a.n_c + ch];
            if (in1) s += (double)a.attr[id[1] * a.n_c + ch];
            if (in2) s += (double)a.attr[id[2] * a.n_c + ch];
            q.P[ch] += w * s;
        }
}

__device__ __forceinline__ void add_member(Acc &q, const ClusterArgs &a, int64_t v, const double g[3])
{
#pragma clang fp contract(off)
    if ((uint64_t)v >= (uint64_t)a.n_v) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) q.M[i] += a.verts[3 * v + i] - g[i];
}

// mean, solve, clip and the stores of cluster k from its sums; n_m members, the first of them `first`
__device__ __forceinline__ void finish(const Acc &q, const ClusterArgs &a, int64_t k, const double g[3], int64_t n_m, int64_t first)
{
#pragma clang fp contract(off)
    const double hh = 0.5 * a.h;
    double xb[3], y[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xb[i] = n_m > 0 ? q.M[i] / (double)n_m : 0.0;
        xb[i] = fmin(fmax(xb[i], -hh), hh);
        y[i] = xb[i];
    }
    if (q.S > 0.0) {
        const double r = a.lam * q.S;
        const double a00 = q.A[0] + r, a01 = q.A[1], a02 = q.A[2], a11 = q.A[3] + r, a12 = q.A[4], a22 = q.A[5] + r;
        const double r0 = r * xb[0] - q.b[0], r1 = r * xb[1] - q.b[1], r2 = r * xb[2] - q.b[2];
        // L D L^T of the SPD matrix, then the two substitutions
        const double l10 = a01 / a00, l20 = a02 / a00;
        const double d1 = a11 - l10 * a01;
        const double u12 = a12 - l20 * a01;
        const double l21 = u12 / d1;
        const double d2 = (a22 - l20 * a02) - l21 * u12;
        const double z0 = r0, z1 = r1 - l10 * z0, z2 = (r2 - l20 * z0) - l21 * z1;
        const double s2 = z2 / d2, s1 = z1 / d1 - l21 * s2, s0 = (z0 / a00 - l10 * s1) - l20 * s2;
        const double dl[3] = {s0 - xb[0], s1 - xb[1], s2 - xb[2]};
        double t = 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (dl[i] > 0.0) t = fmin(t, (hh - xb[i]) / dl[i]);
            else if (dl[i] < 0.0) t = fmin(t, (-hh - xb[i]) / dl[i]);
        }
        if (!(t >= 0.0)) t = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double v = xb[i] + t * dl[i];
            y[i] = fabs(v) < INFINITY ? fmin(fmax(v, -hh), hh) : xb[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) a.pos[3 * k + i] = g[i] + y[i];
#pragma unroll
    for (int ch = 0; ch < SM_MAX_C; ++ch)
        if (ch < a.n_c) {
            float v = 0.f;
            if (q.W > 0.0) v = (float)(q.P[ch] / q.W);
            else if ((uint64_t)first < (uint64_t)a.n_v) v = a.attr[first * a.n_c + ch];
            a.attr_out[k * a.n_c + ch] = v;
        }
    if (a.debug) {
        double *o = a.debug + ESR_SIMPLIFY_DEBUG * k;
#pragma unroll
        for (int i = 0; i < 6; ++i) o[i] = q.A[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) o[6 + i] = q.b[i], o[12 + i] = xb[i];
        o[9] = q.c, o[10] = q.S, o[11] = q.W;
    }
}

// The sum of v over the workgroup in a fixed shape, x[t] += x[t + off] for off = 128, 64, ... 1: the two steps across the
// waves through LDS, the six inside wave 0 by lane shifts.  Every thread calls it; the result is thread 0's alone.  `buf`
// holds two rows used in turn (`slot` counts the calls): a row is rewritten only after the barrier of the call between.
__device__ __forceinline__ double block_sum(double v, double (*buf)[SM_THREADS], int &slot)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    double *x = buf[slot & 1];
    ++slot;
    x[t] = v;
    __syncthreads();
    double r = 0.0;
    if (t < ESR_WAVE) {
        r = (x[t] + x[t + 128]) + (x[t + 64] + x[t + 192]);
#pragma unroll
        for (int off = ESR_WAVE / 2; off > 0; off >>= 1) r = r + __shfl_down(r, off);
    }
    return r;
}

__device__ __forceinline__ void segments(const ClusterArgs &a, int64_t k, int64_t &m0, int64_t &m1, int64_t &p0, int64_t &p1)
{
    m0 = min(max(a.mstart[k], (int64_t)0), a.n_v), m1 = min(max(a.mstart[k + 1], m0), a.n_v);
    p0 = min(max(a.pstart[k], (int64_t)0), a.n_pairs), p1 = min(max(a.pstart[k + 1], p0), a.n_pairs);
}

// one lane per cluster of at most `big` pairs and members
__global__ void __launch_bounds__(SM_THREADS) simplify_cluster_lane_kernel(ClusterArgs a)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n_k; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t m0, m1, p0, p1;
        segments(a, k, m0, m1, p0, p1);
        if (p1 - p0 > a.big || m1 - m0 > a.big) continue;
        Acc q;
        double g[3];
        acc_zero(q);
        cell_centre(a, k, g);
        for (int64_t i = p0; i < p1; ++i) add_face(q, a, a.pairs[i] & 0xffffffffll, (int32_t)k, g);
        for (int64_t i = m0; i < m1; ++i) add_member(q, a, a.mids[i], g);
        finish(q, a, k, g, m1 - m0, m1 > m0 ? a.mids[m0] : (int64_t)-1);
    }
}

// one workgroup per larger cluster; the workgroups stride over all clusters and pass the others by
__global__ void __launch_bounds__(SM_THREADS) simplify_cluster_group_kernel(ClusterArgs a)
{
    __shared__ double s_buf[2][SM_THREADS];
    const int tid = threadIdx.x;
    int slot = 0;
    for (int64_t k = blockIdx.x; k < a.n_k; k += gridDim.x) {
        int64_t m0, m1, p0, p1;
        segments(a, k, m0, m1, p0, p1);
        if (!(p1 - p0 > a.big || m1 - m0 > a.big)) continue;      // (the same for every thread of the workgroup)
        Acc q;
        double g[3];
        acc_zero(q);
        cell_centre(a, k, g);
        for (int64_t i = p0 + tid; i < p1; i += SM_THREADS) add_face(q, a, a.pairs[i] & 0xffffffffll, (int32_t)k, g);
        for (int64_t i = m0 + tid; i < m1; i += SM_THREADS) add_member(q, a, a.mids[i], g);
#pragma unroll
        for (int i = 0; i < 6; ++i) q.A[i] = block_sum(q.A[i], s_buf, slot);
#pragma unroll
        for (int i = 0; i < 3; ++i) q.b[i] = block_sum(q.b[i], s_buf, slot), q.M[i] = block_sum(q.M[i], s_buf, slot);
        q.c = block_sum(q.c, s_buf, slot), q.S = block_sum(q.S, s_buf, slot), q.W = block_sum(q.W, s_buf, slot);
#pragma unroll
        for (int ch = 0; ch < SM_MAX_C; ++ch)
            if (ch < a.n_c) q.P[ch] = block_sum(q.P[ch], s_buf, slot);   // (n_c is the same for every thread)
        if (tid == 0) finish(q, a, k, g, m1 - m0, m1 > m0 ? a.mids[m0] : (int64_t)-1);
    }
}

__global__ void __launch_bounds__(SM_THREADS) simplify_cell_keys_kernel(const double *__restrict__ verts, int64_t n_v,
                                                                        const double *__restrict__ origin, double h,
                                                                        int64_t *__restrict__ keys)
{
#pragma clang fp contract(off)
    const double o[3] = {origin[0], origin[1], origin[2]};
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (int64_t)gridDim.x * blockDim.x) {
        int64_t c[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double x = floor((verts[3 * v + i] - o[i]) / h);
            // (the caller has checked the extent; a coordinate that is still out of range, NaN included, goes to an end cell)
            c[i] = x >= 0.0 ? (x < (double)SM_AXIS ? (int64_t)x : SM_AXIS - 1) : 0;
        }
        keys[v] = c[0] << 42 | c[1] << 21 | c[2];
    }
}

// the clusters of a face's corners; false for a face that names no vertex
__device__ __forceinline__ bool face_clusters(const int64_t *__restrict__ tris, const int32_t *__restrict__ vc, int64_t n_v,
                                              int64_t f, int64_t kc[3])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t id = tris[3 * f + j];
        if ((uint64_t)id >= (uint64_t)n_v) return false;
        kc[j] = (int64_t)vc[id];
    }
    return true;
}

__global__ void __launch_bounds__(SM_THREADS) simplify_pair_keys_kernel(const int64_t *__restrict__ tris, int64_t n_f,
                                                                        const int32_t *__restrict__ vc, int64_t n_v,
                                                                        int64_t *__restrict__ pairs)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_f; f += (int64_t)gridDim.x * blockDim.x) {
        int64_t kc[3] = {0, 0, 0};
        const bool ok = face_clusters(tris, vc, n_v, f, kc);
        pairs[3 * f] = ok ? kc[0] << 32 | f : SM_NONE;
        pairs[3 * f + 1] = ok && kc[1] != kc[0] ? kc[1] << 32 | f : SM_NONE;
        pairs[3 * f + 2] = ok && kc[2] != kc[0] && kc[2] != kc[1] ? kc[2] << 32 | f : SM_NONE;
    }
}

__global__ void __launch_bounds__(SM_THREADS) simplify_face_keys_kernel(const int64_t *__restrict__ tris, int64_t n_f,
                                                                        const int32_t *__restrict__ vc, int64_t n_v,
                                                                        int64_t *__restrict__ key_hi, int32_t *__restrict__ key_lo)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_f; f += (int64_t)gridDim.x * blockDim.x) {
        int64_t kc[3] = {0, 0, 0};
        const bool ok = face_clusters(tris, vc, n_v, f, kc) && kc[0] != kc[1] && kc[0] != kc[2] && kc[1] != kc[2];
        const int64_t lo = min(min(kc[0], kc[1]), kc[2]), hi = max(max(kc[0], kc[1]), kc[2]);
        const int64_t mid = kc[0] + kc[1] + kc[2] - lo - hi;
        key_hi[f] = ok ? lo << 32 | mid : SM_NONE;
        key_lo[f] = ok ? (int32_t)hi : 0;
    }
}

__global__ void __launch_bounds__(SM_THREADS) simplify_keep_kernel(const int64_t *__restrict__ order,
                                                                   const int64_t *__restrict__ key_hi,
                                                                   const int32_t *__restrict__ key_lo, int64_t n_f,
                                                                   const int64_t *__restrict__ tris,
                                                                   const int32_t *__restrict__ vc, int64_t n_v, int64_t n_k,
                                                                   uint8_t *__restrict__ keep, uint8_t *used)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_f; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = order[i];
        if ((uint64_t)f >= (uint64_t)n_f) continue;
        const int64_t hi = key_hi[f];
        bool first = hi != SM_NONE;
        if (first && i > 0) {
            const int64_t e = order[i - 1];
            if ((uint64_t)e < (uint64_t)n_f) first = key_hi[e] != hi || key_lo[e] != key_lo[f];
        }
        keep[f] = first ? 1 : 0;
        if (!first) continue;
        int64_t kc[3];
        if (!face_clusters(tris, vc, n_v, f, kc)) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if ((uint64_t)kc[j] < (uint64_t)n_k) used[kc[j]] = 1;  // (every writer stores the same byte)
    }
}

bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

ESR_API int esr_simplify_cell_keys(const double *vertices, int64_t n_vertices, const double *origin, double h, int64_t *keys,
                                   void *stream)
{
    if (n_vertices < 0 || !(h > 0.0) || !(h < INFINITY)) return ESR_EINVAL;
    if (n_vertices >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_vertices) return 0;
    if (!vertices || !origin || !keys || !aligned(vertices, 8) || !aligned(origin, 8) || !aligned(keys, 8)) return ESR_EINVAL;
    simplify_cell_keys_kernel<<<esr_grid_for(n_vertices, SM_THREADS, SM_BLOCKS), SM_THREADS, 0, esr_stream(stream)>>>(
        vertices, n_vertices, origin, h, keys);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_simplify_pair_keys(const int64_t *triangles, int64_t n_faces, const int32_t *vertex_cluster, int64_t n_vertices,
                                   int64_t *pairs, void *stream)
{
    if (n_faces < 0 || n_vertices < 0) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31 || n_vertices >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_faces) return 0;
    if (!triangles || !pairs || !aligned(triangles, 8) || !aligned(pairs, 8) ||
        (n_vertices && (!vertex_cluster || !aligned(vertex_cluster, 4))))
        return ESR_EINVAL;
    simplify_pair_keys_kernel<<<esr_grid_for(n_faces, SM_THREADS, SM_BLOCKS), SM_THREADS, 0, esr_stream(stream)>>>(
        triangles, n_faces, vertex_cluster, n_vertices, pairs);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_simplify_clusters(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces,
                                  const int32_t *vertex_cluster, const int64_t *cluster_keys, int64_t n_clusters,
                                  const int64_t *member_start, const int64_t *member_ids, const int64_t *pair_start,
                                  const int64_t *pairs, int64_t n_pairs, const double *origin, double h, double lam,
                                  const float *attr, int32_t n_attr, int64_t big, double *positions, float *attr_out,
                                  double *debug, void *stream)
{
    if (n_vertices < 0 || n_faces < 0 || n_clusters < 0 || n_pairs < 0 || n_attr < 0 || big < 1) return ESR_EINVAL;
    if (!(h > 0.0) || !(h < INFINITY) || !(lam > 0.0) || !(lam < INFINITY)) return ESR_EINVAL;
    if (n_attr > ESR_SIMPLIFY_MAX_C) return ESR_ECAP;
    if (n_faces >= (int64_t)1 << 31 || n_vertices >= (int64_t)1 << 31) return ESR_ECAP;
    if (n_pairs > 3 * n_faces || n_clusters > n_vertices) return ESR_EINVAL;
    if (!n_clusters) return 0;
    if (!vertices || !vertex_cluster || !cluster_keys || !member_start || !member_ids || !pair_start || !origin || !positions ||
        !aligned(vertices, 8) || !aligned(vertex_cluster, 4) || !aligned(cluster_keys, 8) || !aligned(member_start, 8) ||
        !aligned(member_ids, 8) || !aligned(pair_start, 8) || !aligned(origin, 8) || !aligned(positions, 8) || !aligned(debug, 8))
        return ESR_EINVAL;
    if (n_pairs && (!triangles || !pairs || !aligned(triangles, 8) || !aligned(pairs, 8))) return ESR_EINVAL;
    if (n_attr && (!attr || !attr_out || !aligned(attr, 4) || !aligned(attr_out, 4))) return ESR_EINVAL;
    ClusterArgs a{vertices, n_vertices, triangles, n_faces, vertex_cluster, cluster_keys, n_clusters, member_start, member_ids,
                  pair_start, pairs, n_pairs, origin, h, lam, attr, (int)n_attr, big, positions, attr_out, debug};
    hipStream_t s = esr_stream(stream);
    simplify_cluster_lane_kernel<<<esr_grid_for(n_clusters, SM_THREADS, SM_BLOCKS), SM_THREADS, 0, s>>>(a);
    ESR_CHECK_LAUNCH();
    simplify_cluster_group_kernel<<<esr_grid_for(n_clusters, 1, SM_GROUP_BLOCKS), SM_THREADS, 0, s>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_simplify_face_keys(const int64_t *triangles, int64_t n_faces, const int32_t *vertex_cluster, int64_t n_vertices,
                                   int64_t *key_hi, int32_t *key_lo, void *stream)
{
    if (n_faces < 0 || n_vertices < 0) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31 || n_vertices >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_faces) return 0;
    if (!triangles || !key_hi || !key_lo || !aligned(triangles, 8) || !aligned(key_hi, 8) || !aligned(key_lo, 4) ||
        (n_vertices && (!vertex_cluster || !aligned(vertex_cluster, 4))))
        return ESR_EINVAL;
    simplify_face_keys_kernel<<<esr_grid_for(n_faces, SM_THREADS, SM_BLOCKS), SM_THREADS, 0, esr_stream(stream)>>>(
        triangles, n_faces, vertex_cluster, n_vertices, key_hi, key_lo);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_simplify_keep(const int64_t *order, const int64_t *key_hi, const int32_t *key_lo, int64_t n_faces,
                              const int64_t *triangles, const int32_t *vertex_cluster, int64_t n_vertices, int64_t n_clusters,
                              uint8_t *keep, uint8_t *used, void *stream)
{
    if (n_faces < 0 || n_vertices < 0 || n_clusters < 0) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31 || n_vertices >= (int64_t)1 << 31) return ESR_ECAP;
    if (n_clusters > n_vertices || (n_clusters && !used)) return ESR_EINVAL;
    if (n_faces && (!order || !key_hi || !key_lo || !triangles || !keep || !aligned(order, 8) || !aligned(key_hi, 8) ||
                    !aligned(key_lo, 4) || !aligned(triangles, 8) || (n_vertices && (!vertex_cluster || !aligned(vertex_cluster, 4)))))
        return ESR_EINVAL;
    hipStream_t s = esr_stream(stream);
    if (n_clusters) {
        hipError_t e = hipMemsetAsync(used, 0, (size_t)n_clusters, s);
        if (e != hipSuccess) return (int)e;
    }
    if (!n_faces) return 0;
    simplify_keep_kernel<<<esr_grid_for(n_faces, SM_THREADS, SM_BLOCKS), SM_THREADS, 0, s>>>(
        order, key_hi, key_lo, n_faces, triangles, vertex_cluster, n_vertices, n_clusters, keep, used);
    ESR_CHECK_LAUNCH();
    return 0;
}
