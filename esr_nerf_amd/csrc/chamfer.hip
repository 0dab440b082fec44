// Chamfer metric of DTU (DTU_CD): triangle sampling, a cell index over a point cloud, the radius-greedy downsample and
// exact nearest-neighbour distances.
//
// Reference algorithm (paths under the reference tree):
//   utils2/metric.py:101-165   sample_single_tri + the per-triangle n1 / n2 (a multiprocessing pool over triangles)
//   utils2/metric.py:168-187   shuffle, then sklearn radius_neighbors and a Python loop: keep i unless an earlier kept
//                              point lies within thresh
//   utils2/metric.py:209-231   two sklearn kd-tree kneighbors passes (data -> stl, stl above the plane -> data_in)
//
// Contract (restated in numpy by tests/chamfer_ref.py).  Every float is f64 and every operation is separately rounded in
// the reference's order (contraction off):
//   - sampling: v1 = p1 - p0, v2 = p2 - p0, l = sqrt((x*x + y*y) + z*z), area2 = |np.cross(v1, v2)|; area2 > 0 only;
//     thr = thresh * sqrt((l1*l2)/area2), n = floor(l/thr); point (i, j), i <= n1, j <= n2 in row-major order, is kept
//     when (i+0.5)/max(n1,1e-7) + (j+0.5)/max(n2,1e-7) < 1, at (v1*a + v2*b) + p0.  count -> torch.cumsum -> fill: the
//     output order is the triangle order, no atomics.
//   - a pair is within thresh when ((dx*dx + dy*dy) + dz*dz) <= thresh*thresh (sklearn's radius_neighbors rule).
//   - nearest neighbour: sqrt(min over targets of the same squared distance), +inf when that is not < max_dist.
//
// The cell index (esr_cd_index_t): cell c = floor((p - origin) / h) per axis, key = cx << 42 | cy << 21 | cz (so the
// key order is x-major), the points sorted by key (torch.sort, stable), cell ranges start[u]..start[u+1] of the unique
// keys, and an open-addressing hash table key -> u with a power-of-two capacity >= 2 x the cell count (linear probing).
// The nearest-neighbour search adds a coarse occupancy table of the cells of coarse^3 fine cells.
//
// MI355X notes.  Everything here is latency-bound pointer chasing (hash probes, then a few dozen points per probe); one
// lane per point or query, 256 lanes per block.  The downsample is the lexicographically-first maximal independent set,
// computed in rounds: a lane decides its point when an earlier kept neighbour exists (removed) or every earlier
// neighbour is removed (kept).  Decisions are final, so a lane may read its neighbours' states while other lanes write
// them (relaxed device-scope loads and stores): a stale read only delays a decision.  A block repeats its undecided
// lanes while one of them made progress, so a dependency chain inside the block resolves in one launch -- the identity
// order over spatially sorted points chains every point to the one before it.
#include "esr_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CD_THREADS = 256;
constexpr int CD_FINE_RINGS = 2;          // nearest neighbour: fine rings searched before the coarse walk
constexpr int64_t CD_EMPTY = -1;

__device__ __forceinline__ uint64_t cd_hash(int64_t key, int64_t cap)
{
    uint64_t x = (uint64_t)key;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x & (uint64_t)(cap - 1);
}

__device__ __forceinline__ int64_t cd_key(int64_t cx, int64_t cy, int64_t cz) { return cx << 42 | cy << 21 | cz; }

// the slot value of `key`, or -1 (tables: keys [cap], -1 empty)
__device__ __forceinline__ int32_t cd_find(const int64_t *__restrict__ keys, const int32_t *__restrict__ vals, int64_t cap,
                                           int64_t key)
{
    for (uint64_t s = cd_hash(key, cap);; s = (s + 1) & (uint64_t)(cap - 1)) {
        const int64_t k = keys[s];
        if (k == key) return vals ? vals[s] : 0;
        if (k == CD_EMPTY) return -1;
    }
}

__device__ __forceinline__ double cd_d2(const double *a, const double *b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double cd_norm(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

struct Tri {
    double p0[3], v1[3], v2[3];
    double n1, n2, d1, d2;
    bool ok;
};

__device__ __forceinline__ Tri cd_tri(const double *__restrict__ V, const int64_t *__restrict__ T, int64_t t, double thresh)
{
    Tri r;
    const double *p0 = V + 3 * T[3 * t], *p1 = V + 3 * T[3 * t + 1], *p2 = V + 3 * T[3 * t + 2];
    for (int a = 0; a < 3; ++a) {
        r.p0[a] = p0[a];
        r.v1[a] = p1[a] - p0[a];
        r.v2[a] = p2[a] - p0[a];
    }
    const double *a = r.v1, *b = r.v2;
    const double l1 = cd_norm(a[0], a[1], a[2]), l2 = cd_norm(b[0], b[1], b[2]);
    const double area2 = cd_norm(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]);
    r.ok = area2 > 0.0;
    const double thr = thresh * sqrt((l1 * l2) / area2);
    r.n1 = floor(l1 / thr);
    r.n2 = floor(l2 / thr);
    // rows beyond 2^40 cannot be sampled anyway (the reference would build that grid in memory)
    r.ok = r.ok && r.n1 >= 0.0 && r.n2 >= 0.0 && r.n1 < 1099511627776.0 && r.n2 < 1099511627776.0;
    r.d1 = r.n1 > 1e-7 ? r.n1 : 1e-7;   // Python's max(n, 1e-7)
    r.d2 = r.n2 > 1e-7 ? r.n2 : 1e-7;
    return r;
}

// a + b < 1 is monotone in j along a row and in i across rows, so each row ends at its first rejected j and the rows
// end at the first empty one
template <bool FILL>
__global__ void __launch_bounds__(CD_THREADS) cd_sample_kernel(const double *__restrict__ V, const int64_t *__restrict__ T,
                                                               int64_t n_tri, double thresh, int64_t *__restrict__ counts,
                                                               const int64_t *__restrict__ offsets,
                                                               double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
    if (t >= n_tri) return;
    const Tri r = cd_tri(V, T, t, thresh);
    int64_t c = 0;
    double *o = FILL ? out + 3 * offsets[t] : nullptr;
    if (r.ok) {
        for (double i = 0.0; i <= r.n1; i += 1.0) {
            const double a = (i + 0.5) / r.d1;
            double j = 0.0;
            for (; j <= r.n2; j += 1.0) {
                const double b = (j + 0.5) / r.d2;
                if (!(a + b < 1.0)) break;
                if (FILL) {
                    for (int k = 0; k < 3; ++k) o[3 * c + k] = (r.v1[k] * a + r.v2[k] * b) + r.p0[k];
                }
                ++c;
            }
            if (j == 0.0) break;
        }
    }
    if (!FILL) counts[t] = c;
}

__global__ void __launch_bounds__(CD_THREADS) cd_keys_kernel(const double *__restrict__ P, int64_t n, esr_cd_index_t ix,
                                                             int64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
    if (i >= n) return;
    int64_t c[3];
    for (int a = 0; a < 3; ++a) {
        const double f = floor((P[3 * i + a] - ix.origin[a]) / ix.h);
        c[a] = f < 0.0 ? 0 : (f > (double)(ix.dims[a] - 1) ? ix.dims[a] - 1 : (int64_t)f);
    }
    keys[i] = cd_key(c[0], c[1], c[2]);
}

__global__ void __launch_bounds__(CD_THREADS) cd_insert_kernel(const int64_t *__restrict__ ukeys, int64_t n_u, int64_t cap,
                                                               int64_t *__restrict__ tkeys, int32_t *__restrict__ tvals)
{
    const int64_t u = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
    if (u >= n_u) return;
    const int64_t key = ukeys[u];
    for (uint64_t s = cd_hash(key, cap);; s = (s + 1) & (uint64_t)(cap - 1)) {
        const unsigned long long prev =
            atomicCAS((unsigned long long *)(tkeys + s), (unsigned long long)CD_EMPTY, (unsigned long long)key);
        if (prev == (unsigned long long)CD_EMPTY || prev == (unsigned long long)key) {
            if (tvals) tvals[s] = (int32_t)u;
            return;
        }
    }
}

__device__ __forceinline__ int8_t cd_load_state(const int8_t *s) { return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cd_store_state(int8_t *s, int8_t v) { __hip_atomic_store(s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// state: 0 undecided, 1 kept, 2 removed; point k of the ORDER (P in order; ix.ids = the order rank of each sorted point,
// ascending inside a cell).  changed[0] = 1 when any state changed.
__global__ void __launch_bounds__(CD_THREADS) cd_downsample_kernel(esr_cd_index_t ix, const double *__restrict__ P, int64_t n,
                                                                   double t2, int8_t *__restrict__ state,
                                                                   int32_t *__restrict__ changed)
{
    const int64_t k = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
    bool open = k < n && cd_load_state(state + k) == 0;
    if (!__syncthreads_or(open)) return;
    double p[3] = {0.0, 0.0, 0.0};
    int64_t c[3] = {0, 0, 0};
    if (open) {
        for (int a = 0; a < 3; ++a) {
            p[a] = P[3 * k + a];
            const double f = floor((p[a] - ix.origin[a]) / ix.h);
            c[a] = f < 0.0 ? 0 : (f > (double)(ix.dims[a] - 1) ? ix.dims[a] - 1 : (int64_t)f);
        }
    }
    bool any = false;
    for (;;) {
        bool progress = false;
        if (open) {
            bool blocked = false, kill = false;
            for (int64_t x = c[0] - 1; x <= c[0] + 1 && !kill; ++x) {
                if (x < 0 || x >= ix.dims[0]) continue;
                for (int64_t y = c[1] - 1; y <= c[1] + 1 && !kill; ++y) {
                    if (y < 0 || y >= ix.dims[1]) continue;
                    for (int64_t z = c[2] - 1; z <= c[2] + 1 && !kill; ++z) {
                        if (z < 0 || z >= ix.dims[2]) continue;
                        const int32_t u = cd_find(ix.keys, ix.cells, ix.cap, cd_key(x, y, z));
                        if (u < 0) continue;
                        for (int64_t s = ix.start[u], e = ix.start[u + 1]; s < e; ++s) {
                            const int64_t r = ix.ids[s];
                            if (r >= k) break;                        // the rest of the cell comes later in the order
                            if (!(cd_d2(p, ix.pts + 3 * s) <= t2)) continue;
                            const int8_t st = cd_load_state(state + r);
                            if (st == 1) {
                                kill = true;
                                break;
                            }
                            blocked |= st == 0;
                        }
                    }
                }
            }
            if (kill || !blocked) {
                cd_store_state(state + k, kill ? 2 : 1);
                open = false;
                progress = true;
            }
        }
        if (!__syncthreads_or(progress)) break;
        any = true;
    }
    if (any && threadIdx.x == 0) changed[0] = 1;
}

// lower bound of the distance from p to the box [lo, hi] per axis (shrunk by eps, so rounding never overestimates it)
__device__ __forceinline__ double cd_box_d2(const double p[3], const double lo[3], const double hi[3], double eps)
{
    double g[3];
    for (int a = 0; a < 3; ++a) {
        double d = lo[a] - p[a];
        d = fmax(d, p[a] - hi[a]) - eps;
        g[a] = d > 0.0 ? d : 0.0;
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

// distance from p (inside cell block centre c) to the outside of the block of cells c - k .. c + k of size h
__device__ __forceinline__ double cd_inner(const esr_cd_index_t &ix, const double p[3], const int64_t c[3], int64_t k,
                                           double h, double eps)
{
    double m = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const double lo = ix.origin[a] + (double)(c[a] - k) * h, hi = ix.origin[a] + (double)(c[a] + k + 1) * h;
        m = fmin(m, fmin(p[a] - lo, hi - p[a]));
    }
    m -= eps;
    return m > 0.0 ? m : 0.0;
}

__device__ __forceinline__ void cd_scan_cell(const esr_cd_index_t &ix, const double p[3], int64_t x, int64_t y, int64_t z,
                                             double &best)
{
    const int32_t u = cd_find(ix.keys, ix.cells, ix.cap, cd_key(x, y, z));
    if (u < 0) return;
    for (int64_t s = ix.start[u], e = ix.start[u + 1]; s < e; ++s) {
        const double d2 = cd_d2(p, ix.pts + 3 * s);
        if (d2 < best) best = d2;
    }
}

// Calls fn(x, y, z) once for every cell of ring k around c (the cells at Chebyshev distance k) that lies inside the grid
// [0, dims).  Every axis is clamped first, so the work is bounded by the cells of the ring inside the grid, however far
// c lies outside it.
template <typename F>
__device__ __forceinline__ void cd_ring(const int64_t c[3], int64_t k, const int64_t dims[3], F fn)
{
    const int64_t x0 = max(c[0] - k, (int64_t)0), x1 = min(c[0] + k, dims[0] - 1);
    const int64_t y0 = max(c[1] - k, (int64_t)0), y1 = min(c[1] + k, dims[1] - 1);
    const int64_t z0 = max(c[2] - k, (int64_t)0), z1 = min(c[2] + k, dims[2] - 1);
    if (x0 > x1 || y0 > y1 || z0 > z1) return;
    for (int64_t x = x0; x <= x1; ++x)
        for (int64_t y = y0; y <= y1; ++y) {
            if (x == c[0] - k || x == c[0] + k || y == c[1] - k || y == c[1] + k) {
                for (int64_t z = z0; z <= z1; ++z) fn(x, y, z);         // a column on the ring's x / y faces
            } else {
                if (c[2] - k >= 0) fn(x, y, c[2] - k);                  // interior column: only the two z faces
                if (k > 0 && c[2] + k < dims[2]) fn(x, y, c[2] + k);
            }
        }
}

__global__ void __launch_bounds__(CD_THREADS) cd_nn_kernel(esr_cd_index_t ix, const double *__restrict__ Q, int64_t nq,
                                                           double max_dist, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
    if (i >= nq) return;
    const double h = ix.h;
    const double p[3] = {Q[3 * i], Q[3 * i + 1], Q[3 * i + 2]};
    // margin of every lower bound below: far above the rounding of a coordinate difference at this magnitude
    double mag = 0.0;
    for (int a = 0; a < 3; ++a) mag = fmax(mag, fabs(p[a]) + fabs(ix.origin[a]) + (double)ix.dims[a] * h);
    const double eps = 1e-9 * h + 1e-14 * mag;
    double best = INFINITY;
    double glo[3], ghi[3];
    int64_t c[3];
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        glo[a] = ix.origin[a];
        ghi[a] = ix.origin[a] + (double)ix.dims[a] * h;
        const double f = floor((p[a] - ix.origin[a]) / h);
        finite &= f == f;
        c[a] = f < -0x1p52 ? -((int64_t)1 << 52) : (f > 0x1p52 ? ((int64_t)1 << 52) : (int64_t)f);
    }
    const double md = max_dist;
    const double bd = sqrt(cd_box_d2(p, glo, ghi, eps));
    if (finite && bd < md) {
        // fine rings: ring k holds the cells at Chebyshev distance k from c; everything outside rings 0..k-1 lies at least
        // cd_inner(k - 1) away
        bool done = false;
        const int64_t fdims[3] = {ix.dims[0], ix.dims[1], ix.dims[2]};
        for (int64_t k = 0; k <= CD_FINE_RINGS; ++k) {
            if (k > 0) {
                const double lb = cd_inner(ix, p, c, k - 1, h, eps);
                if (lb * lb >= best || lb >= md) {
                    done = true;
                    break;
                }
            }
            cd_ring(c, k, fdims, [&](int64_t x, int64_t y, int64_t z) { cd_scan_cell(ix, p, x, y, z, best); });
        }
        if (!done) {
            const double lb = cd_inner(ix, p, c, CD_FINE_RINGS, h, eps);
            done = lb * lb >= best || lb >= md;
        }
        // coarse walk: cells of B^3 fine cells, skipped whole when unoccupied or farther than the best / max_dist
        const int64_t B = ix.coarse;
        const double H = h * (double)B;
        int64_t cc[3], cdims[3];
        for (int a = 0; a < 3; ++a) {
            cc[a] = c[a] >= 0 ? c[a] / B : -((-c[a] + B - 1) / B);
            cdims[a] = (ix.dims[a] + B - 1) / B;
        }
        // only the rings that meet the grid: from the Chebyshev distance of cc to the grid's coarse cells to that of
        // its farthest one (a query outside the grid, or a grid of a few tiny cells, never walks empty rings)
        int64_t k_first = 0, k_last = 0;
        for (int a = 0; a < 3; ++a) {
            k_first = max(k_first, cc[a] < 0 ? -cc[a] : (cc[a] >= cdims[a] ? cc[a] - cdims[a] + 1 : (int64_t)0));
            k_last = max(k_last, max(cc[a] < 0 ? -cc[a] : cc[a], cdims[a] - 1 - cc[a]));
        }
        for (int64_t K = k_first; !done && K <= k_last; ++K) {
            if (K > 0) {
                const double lb = cd_inner(ix, p, cc, K - 1, H, eps);
                if (lb * lb >= best || lb >= md) break;
            }
            cd_ring(cc, K, cdims, [&](int64_t X, int64_t Y, int64_t Z) {
                const int64_t C0[3] = {X, Y, Z};
                double lo[3], hi[3];
                for (int a = 0; a < 3; ++a) {
                    lo[a] = ix.origin[a] + (double)C0[a] * H;
                    hi[a] = ix.origin[a] + (double)(C0[a] + 1) * H;
                }
                const double bl = cd_box_d2(p, lo, hi, eps);
                if (bl >= best || sqrt(bl) >= md) return;
                if (cd_find(ix.ckeys, nullptr, ix.ccap, cd_key(X, Y, Z)) < 0) return;
                for (int64_t x = X * B; x < min((X + 1) * B, (int64_t)ix.dims[0]); ++x)
                    for (int64_t y = Y * B; y < min((Y + 1) * B, (int64_t)ix.dims[1]); ++y)
                        for (int64_t z = Z * B; z < min((Z + 1) * B, (int64_t)ix.dims[2]); ++z) {
                            const int64_t f[3] = {x, y, z};
                            for (int a = 0; a < 3; ++a) {
                                lo[a] = ix.origin[a] + (double)f[a] * h;
                                hi[a] = ix.origin[a] + (double)(f[a] + 1) * h;
                            }
                            const double fb = cd_box_d2(p, lo, hi, eps);
                            if (fb >= best || sqrt(fb) >= md) continue;
                            cd_scan_cell(ix, p, x, y, z, best);
                        }
            });
        }
    }
    const double d = sqrt(best);
    out[i] = d < md ? d : INFINITY;
}

int cd_index_ok(const esr_cd_index_t *ix)
{
    if (!ix || !(ix->h > 0.0) || !ix->keys || !ix->cells || !ix->start || !ix->pts || ix->cap < 1 ||
        (ix->cap & (ix->cap - 1)))
        return 0;
    for (int a = 0; a < 3; ++a)
        if (ix->dims[a] < 1 || ix->dims[a] >= (1 << 21)) return 0;
    return 1;
}

}  // namespace

ESR_API int esr_cd_sample_count(const double *vertices, const int64_t *triangles, int64_t n_tri, double thresh,
                                int64_t *counts, void *stream)
{
    if (n_tri < 0 || !(thresh > 0.0) || (n_tri && (!vertices || !triangles || !counts))) return ESR_EINVAL;
    if (!n_tri) return 0;
    cd_sample_kernel<false><<<(unsigned)((n_tri + CD_THREADS - 1) / CD_THREADS), CD_THREADS, 0, esr_stream(stream)>>>(
        vertices, triangles, n_tri, thresh, counts, nullptr, nullptr);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cd_sample_fill(const double *vertices, const int64_t *triangles, int64_t n_tri, double thresh,
                               const int64_t *offsets, double *points, void *stream)
{
    if (n_tri < 0 || !(thresh > 0.0) || (n_tri && (!vertices || !triangles || !offsets || !points))) return ESR_EINVAL;
    if (!n_tri) return 0;
    cd_sample_kernel<true><<<(unsigned)((n_tri + CD_THREADS - 1) / CD_THREADS), CD_THREADS, 0, esr_stream(stream)>>>(
        vertices, triangles, n_tri, thresh, nullptr, offsets, points);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cd_cell_keys(const esr_cd_index_t *index, const double *points, int64_t n, int64_t *keys, void *stream)
{
    if (!index || !(index->h > 0.0) || n < 0 || (n && (!points || !keys))) return ESR_EINVAL;
    for (int a = 0; a < 3; ++a)
        if (index->dims[a] < 1 || index->dims[a] >= (1 << 21)) return ESR_ECAP;
    if (!n) return 0;
    cd_keys_kernel<<<(unsigned)((n + CD_THREADS - 1) / CD_THREADS), CD_THREADS, 0, esr_stream(stream)>>>(points, n, *index,
                                                                                                       keys);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cd_hash_insert(const int64_t *ukeys, int64_t n_u, int64_t cap, int64_t *table_keys, int32_t *table_vals,
                               void *stream)
{
    if (n_u < 0 || cap < 1 || (cap & (cap - 1)) || n_u >= cap || (n_u && (!ukeys || !table_keys))) return ESR_EINVAL;
    if (n_u >= (int64_t)1 << 31) return ESR_ECAP;
    if (!n_u) return 0;
    cd_insert_kernel<<<(unsigned)((n_u + CD_THREADS - 1) / CD_THREADS), CD_THREADS, 0, esr_stream(stream)>>>(
        ukeys, n_u, cap, table_keys, table_vals);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cd_downsample_round(const esr_cd_index_t *index, const double *points, int64_t n, double thresh,
                                    int8_t *state, int32_t *changed, void *stream)
{
    if (!cd_index_ok(index) || n < 0 || !(thresh > 0.0) || !(index->h >= thresh) || (n && (!points || !state || !changed)))
        return ESR_EINVAL;
    if (!n) return 0;
    cd_downsample_kernel<<<(unsigned)((n + CD_THREADS - 1) / CD_THREADS), CD_THREADS, 0, esr_stream(stream)>>>(
        *index, points, n, thresh * thresh, state, changed);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_cd_nn(const esr_cd_index_t *index, const double *queries, int64_t nq, double max_dist, double *dist,
                      void *stream)
{
    if (!cd_index_ok(index) || nq < 0 || !(max_dist > 0.0) || index->coarse < 1 || !index->ckeys || index->ccap < 1 ||
        (index->ccap & (index->ccap - 1)) || (nq && (!queries || !dist)))
        return ESR_EINVAL;
    if (!nq) return 0;
    cd_nn_kernel<<<(unsigned)((nq + CD_THREADS - 1) / CD_THREADS), CD_THREADS, 0, esr_stream(stream)>>>(*index, queries, nq,
                                                                                                       max_dist, dist);
    ESR_CHECK_LAUNCH();
    return 0;
}
