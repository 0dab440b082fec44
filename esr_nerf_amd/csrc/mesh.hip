// Mesh export: the -sdf lattice field and marching cubes over it.
//
// Reference algorithm (paths under the reference tree):
//   app/fine/model/voxurff.py:745-770      extract_geometry: smoothed (Gaussian3DConv) or raw SDF grid, -grid_sample on a
//                                          resolution^3 lattice of the bounding box, then mcubes.marching_cubes
//   app/utils/base/functions.py:108-139    extract_fields: the lattice = torch.linspace per axis, filled block by block
//   mcubes.marching_cubes (PyMCubes)       the surface extraction, on one CPU thread over the host copy of the field
//
// Contract of the march (restated in numpy by tests/mesh_ref.py):
//   - node n is INSIDE iff u[n] > thr; u == thr is outside.
//   - each lattice edge (n, n + e_a) whose inside flags differ holds ONE vertex, shared by the (up to four) cells around
//     it, at n + t e_a in index space, t = ((double)thr - (double)u[n]) / ((double)u[n + e_a] - (double)u[n]).
//   - vertices are numbered by the owner node's linear index (i * R1 + j) * R2 + k, then by axis x < y < z; triangles are
//     listed by the cell's linear index over (R0-1) x (R1-1) x (R2-1), then in case-table order (mc_table.h, written by
//     tools/gen_mc_table.py).  (b - a) x (c - a) points from inside to outside, towards decreasing u.
//   No output slot comes from an atomic counter: count -> scan -> emit, the result is byte-identical run to run.
//
// MI355X notes.  One lane per lattice node, z (the contiguous axis) on consecutive lanes; a node is also the origin of
// the cell at its (+x, +y, +z) side, so the cell order over (R0-1)(R1-1)(R2-1) is the node order with the last layer of
// each axis skipped.  A lane reads its 8 cell corners; the neighbours come out of the same cache lines as the
// neighbouring lanes' reads, so HBM sees each field value about once per pass.  Bytes per lattice node: the field writes
// 4; count and each of the two emit passes read 4 (plus 4 written and, per surface triangle, up to 12 gathered of the
// per-node vertex ids), and the outputs add 24 per vertex and 24 per triangle.
#include "esr_collectives.h"
#include "mc_table.h"

namespace {

constexpr int MESH_THREADS = 256;        // lattice nodes per block: the unit of the block-total scan
constexpr int MESH_MAX_R = 1024;         // per axis: R0 R1 R2 <= 2^30 nodes, so a node index fits 32 bits

struct FieldParams {
    const float *sdf;
    const float *xs, *ys, *zs;
    float *u;
    int gdims[3];
    int r[3];
    float lo[3], hi[3];
};

// u[i,j,k] = -trilinear(S, (xs[i], ys[j], zs[k])): the world point -> grid index map and the 8-corner fetch of
// F.grid_sample(align_corners=True), the same helpers as the renderer's march; the negation after the fetch is exact.
__global__ void __launch_bounds__(256) mesh_field_kernel(FieldParams P)
{
    const uint32_t r1 = P.r[1], r2 = P.r[2];
    const uint32_t n = (uint32_t)P.r[0] * r1 * r2;
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
        const uint32_t k = idx % r2, j = idx / r2 % r1, i = idx / (r1 * r2);
        const float p[3] = {P.xs[i], P.ys[j], P.zs[k]};
        float g[3];
        esr_world_to_index(p, P.lo, P.hi, P.gdims, g);
        P.u[idx] = -esr_tri_fetch1(P.sdf, P.gdims, g);
    }
}

struct Lattice {
    const float *u;
    uint32_t r0, r1, r2;
    float thr;
};

__device__ __forceinline__ bool node_in(const Lattice &L, uint32_t m) { return L.u[m] > L.thr; }

// A node's classification: cmask bit a = edge (n, n + e_a) crossed (n owns its vertex); ncase = the case index of the
// cell whose origin is n, -1 when n is in the last layer of an axis.  All loads are issued unconditionally (an
// out-of-lattice neighbour reads node n itself) so the eight reads of a lane go out back to back.
struct NodeClass {
    int cmask, ncase;
    uint32_t i, j, k;
};

__device__ __forceinline__ NodeClass classify(const Lattice &L, uint32_t n)
{
    NodeClass c;
    c.k = n % L.r2;
    c.j = n / L.r2 % L.r1;
    c.i = n / (L.r1 * L.r2);
    const uint32_t s0 = L.r1 * L.r2, s1 = L.r2;
    const bool hx = c.i + 1 < L.r0, hy = c.j + 1 < L.r1, hz = c.k + 1 < L.r2, cell = hx & hy & hz;
    const uint32_t ox = hx ? s0 : 0, oy = hy ? s1 : 0, oz = hz ? 1 : 0;
    int bits = 0;
#pragma unroll
    for (int cz = 0; cz < 2; ++cz)
#pragma unroll
        for (int cy = 0; cy < 2; ++cy)
#pragma unroll
            for (int cx = 0; cx < 2; ++cx)
                bits |= (int)node_in(L, n + (cx ? ox : 0) + (cy ? oy : 0) + (cz ? oz : 0)) << (cx | cy << 1 | cz << 2);
    const int in0 = bits & 1;
    c.cmask = (int)(hx & (((bits >> 1) & 1) != in0)) | (int)(hy & (((bits >> 2) & 1) != in0)) << 1 |
              (int)(hz & (((bits >> 4) & 1) != in0)) << 2;
    c.ncase = cell ? bits : -1;
    return c;
}

__device__ __forceinline__ int ntri_of(const NodeClass &c) { return c.ncase < 0 ? 0 : ESR_MC_NTRI[c.ncase]; }

// block b's vertex and triangle totals -> counts[b], counts[nb + b]
__global__ void __launch_bounds__(MESH_THREADS) mesh_count_kernel(Lattice L, uint32_t nb, int64_t *__restrict__ counts)
{
    __shared__ int tmp[MESH_THREADS / 64];
    const uint32_t n = blockIdx.x * MESH_THREADS + threadIdx.x, nn = L.r0 * L.r1 * L.r2;
    int packed = 0;                                            // vertices | triangles << 16 (<= 768 | 1280 << 16 per block)
    if (n < nn) {
        const NodeClass c = classify(L, n);
        packed = __popc(c.cmask) | ntri_of(c) << 16;
    }
    int total;
    esr_block_scan_excl<MESH_THREADS>(packed, tmp, total);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = total & 0xffff;
        counts[nb + blockIdx.x] = total >> 16;
    }
}

// vertices of every crossed edge, and vid[n] = the id of node n's first vertex (the triangles' lookup)
__global__ void __launch_bounds__(MESH_THREADS) mesh_emit_vertices_kernel(Lattice L, const int64_t *__restrict__ offsets,
                                                                         int32_t *__restrict__ vid,
                                                                         double *__restrict__ verts)
{
    __shared__ int tmp[MESH_THREADS / 64];
    const uint32_t n = blockIdx.x * MESH_THREADS + threadIdx.x, nn = L.r0 * L.r1 * L.r2;
    NodeClass c = {0, -1, 0, 0, 0};
    if (n < nn) c = classify(L, n);
    int total;
    const int local = esr_block_scan_excl<MESH_THREADS>(__popc(c.cmask), tmp, total);
    if (n >= nn) return;
    int64_t id = offsets[blockIdx.x] + local;
    vid[n] = (int32_t)id;                                      // the host checks that every vertex id fits 31 bits
    if (!c.cmask) return;
    const double thr = (double)L.thr, u0 = (double)L.u[n];
    const uint32_t step[3] = {L.r1 * L.r2, L.r2, 1};
    const uint32_t ijk[3] = {c.i, c.j, c.k};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(c.cmask >> a & 1)) continue;
        const double u1 = (double)L.u[n + step[a]];
        const double t = (thr - u0) / (u1 - u0);
        double *v = verts + 3 * id;
        v[0] = (double)ijk[0];
        v[1] = (double)ijk[1];
        v[2] = (double)ijk[2];
        v[a] = (double)ijk[a] + t;
        ++id;
    }
}

// id of the vertex on edge (m, m + e_axis): m's first vertex id + the crossed edges of m along lower axes
__device__ __forceinline__ int64_t edge_vertex(const Lattice &L, const int32_t *__restrict__ vid, uint32_t m, uint32_t mi,
                                               uint32_t mj, int axis)
{
    int rank = 0;
    if (axis > 0) {
        const bool in0 = node_in(L, m);
        if (mi + 1 < L.r0 && node_in(L, m + L.r1 * L.r2) != in0) ++rank;
        if (axis > 1 && mj + 1 < L.r1 && node_in(L, m + L.r2) != in0) ++rank;
    }
    return (int64_t)vid[m] + rank;
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_emit_triangles_kernel(Lattice L, uint32_t nb,
                                                                          const int64_t *__restrict__ offsets,
                                                                          const int32_t *__restrict__ vid,
                                                                          int64_t *__restrict__ tris)
{
    __shared__ int tmp[MESH_THREADS / 64];
    const uint32_t n = blockIdx.x * MESH_THREADS + threadIdx.x, nn = L.r0 * L.r1 * L.r2;
    NodeClass c = {0, -1, 0, 0, 0};
    if (n < nn) c = classify(L, n);
    const int nt = ntri_of(c);
    int total;
    const int local = esr_block_scan_excl<MESH_THREADS>(nt, tmp, total);
    if (!nt) return;
    int64_t *out = tris + 3 * (offsets[nb + blockIdx.x] + local);
    for (int t = 0; t < 3 * nt; ++t) {
        const int e = ESR_MC_TRI[c.ncase][t];
        const int axis = e >> 2, b0 = e & 1, b1 = (e >> 1) & 1;
        // owner corner of the edge: 0 along `axis`, (b0, b1) along the other two axes in increasing order
        const uint32_t dx = axis == 0 ? 0 : b0, dy = axis == 0 ? b0 : (axis == 1 ? 0 : b1), dz = axis == 2 ? 0 : b1;
        const uint32_t m = n + dx * (L.r1 * L.r2) + dy * L.r2 + dz;
        out[t] = edge_vertex(L, vid, m, c.i + dx, c.j + dy, axis);
    }
}

int lattice(Lattice &L, const float *u, int32_t r0, int32_t r1, int32_t r2, float thr)
{
    if (!u || r0 < 2 || r1 < 2 || r2 < 2 || r0 > MESH_MAX_R || r1 > MESH_MAX_R || r2 > MESH_MAX_R) return ESR_EINVAL;
    L.u = u; L.r0 = r0; L.r1 = r1; L.r2 = r2; L.thr = thr;
    return 0;
}

uint32_t mesh_blocks(const Lattice &L)
{
    return (uint32_t)(((uint64_t)L.r0 * L.r1 * L.r2 + MESH_THREADS - 1) / MESH_THREADS);
}

}  // namespace

// Replaces the field half of extract_geometry: app/fine/model/voxurff.py:745-770 (the -grid_sample query) and
// app/utils/base/functions.py:108-139 (extract_fields' lattice and block loop).
ESR_API int esr_mesh_field(const float *sdf, int32_t gx, int32_t gy, int32_t gz, const float *box_host, const float *xs,
                           const float *ys, const float *zs, int32_t r0, int32_t r1, int32_t r2, float *u, void *stream)
{
    if (!sdf || !box_host || !xs || !ys || !zs || !u || gx < 1 || gy < 1 || gz < 1) return ESR_EINVAL;
    if (r0 < 2 || r1 < 2 || r2 < 2 || r0 > MESH_MAX_R || r1 > MESH_MAX_R || r2 > MESH_MAX_R) return ESR_EINVAL;
    FieldParams P;
    P.sdf = sdf; P.xs = xs; P.ys = ys; P.zs = zs; P.u = u;
    P.gdims[0] = gx; P.gdims[1] = gy; P.gdims[2] = gz;
    P.r[0] = r0; P.r[1] = r1; P.r[2] = r2;
    for (int a = 0; a < 3; ++a) {
        P.lo[a] = box_host[a];
        P.hi[a] = box_host[3 + a];
    }
    mesh_field_kernel<<<esr_grid_for((int64_t)r0 * r1 * r2, 256, 256 * 64), 256, 0, esr_stream(stream)>>>(P);
    ESR_CHECK_LAUNCH();
    return 0;
}

// Replaces the counting half of mcubes.marching_cubes.
ESR_API int64_t esr_mesh_blocks(int32_t r0, int32_t r1, int32_t r2)
{
    if (r0 < 2 || r1 < 2 || r2 < 2 || r0 > MESH_MAX_R || r1 > MESH_MAX_R || r2 > MESH_MAX_R) return ESR_EINVAL;
    return ((int64_t)r0 * r1 * r2 + MESH_THREADS - 1) / MESH_THREADS;
}

ESR_API int esr_mesh_count(const float *u, int32_t r0, int32_t r1, int32_t r2, float threshold, int64_t *counts,
                           void *stream)
{
    Lattice L;
    const int rc = lattice(L, u, r0, r1, r2, threshold);
    if (rc) return rc;
    if (!counts) return ESR_EINVAL;
    const uint32_t nb = mesh_blocks(L);
    mesh_count_kernel<<<nb, MESH_THREADS, 0, esr_stream(stream)>>>(L, nb, counts);
    ESR_CHECK_LAUNCH();
    return 0;
}

// Replaces the emitting half of mcubes.marching_cubes.
ESR_API int esr_mesh_emit(const float *u, int32_t r0, int32_t r1, int32_t r2, float threshold, const int64_t *offsets,
                          int32_t *vid, double *vertices, int64_t *triangles, void *stream)
{
    Lattice L;
    const int rc = lattice(L, u, r0, r1, r2, threshold);
    if (rc) return rc;
    if (!offsets || !vid || !vertices || !triangles) return ESR_EINVAL;
    const uint32_t nb = mesh_blocks(L);
    mesh_emit_vertices_kernel<<<nb, MESH_THREADS, 0, esr_stream(stream)>>>(L, offsets, vid, vertices);
    ESR_CHECK_LAUNCH();
    mesh_emit_triangles_kernel<<<nb, MESH_THREADS, 0, esr_stream(stream)>>>(L, nb, offsets, vid, triangles);
    ESR_CHECK_LAUNCH();
    return 0;
}
