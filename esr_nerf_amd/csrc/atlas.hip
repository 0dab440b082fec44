// Texture atlas of the exported surface (esr_nerf_amd/atlas.py: build, sample; sources.py: bake_materials, bake_irradiance,
// lit_view(atlas=, textures=), write_surface_obj).  Section W of include/esr_hip.h is the definition; tests/atlas_ref.py
// restates it.
//
// Every face owns one half of a square cell of 2^l texels; the cells are packed in Z-order, largest first.  The layout is all
// integer, so nothing is searched: a face finds its cell from its sorted rank (atlas_charts_kernel) and a texel finds its face
// from its own coordinates (atlas_texels_kernel), both through the <= 16 group starts that travel as kernel arguments.
// binary64 arithmetic is one rounding per written operation, in the written order (no contraction), as in bvh.hip and
// simplify.hip: a numpy restatement gives the same bits.
#include "esr_common.h"

namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_BLOCKS = 4096;           // the texel pass strides: 2048^2 texels are four trips of the grid
constexpr int NL = ESR_ATLAS_MAX_LEVELS;

// The groups of one layout, from the level counts: descending level, `start` in sorted ranks, `unit` in cells of side 2^lmin
struct Groups {
    int64_t count[NL], start[NL], unit[NL];
    int32_t size, gutter, lmin, lmax;
};

// 0, ESR_EINVAL or ESR_ECAP (the cells do not fit the square)
int groups_from_counts(const int64_t *counts, int64_t n_faces, int32_t size, int32_t gutter, int32_t lmin, int32_t lmax, Groups &g)
{
    g.size = size, g.gutter = gutter, g.lmin = lmin, g.lmax = lmax;
    int64_t total = 0;
    for (int l = 0; l < NL; ++l) {
        if (counts[l] < 0 || ((l < lmin || l > lmax) && counts[l] != 0)) return ESR_EINVAL;
        total += counts[l];
        g.count[l] = counts[l], g.start[l] = 0, g.unit[l] = 0;
    }
    if (total != n_faces) return ESR_EINVAL;
    int64_t start = 0, unit = 0;
    for (int l = lmax; l >= lmin; --l) {
        g.start[l] = start, g.unit[l] = unit;
        start += counts[l];
        unit += ((counts[l] + 1) >> 1) << (2 * (l - lmin));
    }
    const int64_t side = (int64_t)size >> lmin;
    return unit <= side * side ? 0 : ESR_ECAP;
}

bool layout_ok(int32_t size, int32_t gutter, int32_t lmin, int32_t lmax)
{
    if (size < ESR_ATLAS_MIN_SIZE || size > ESR_ATLAS_MAX_SIZE || (size & (size - 1))) return false;
    if (gutter < 1 || gutter > size || lmin < 0 || lmin > lmax || lmax >= NL) return false;
    return ((int64_t)1 << lmin) >= 3 * (int64_t)gutter + 2 && ((int64_t)1 << lmax) <= size;
}

bool given(const void *p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
bool optional(const void *p, size_t a) { return !p || ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ uint32_t even_bits(uint64_t m)
{
    m &= 0x5555555555555555ull;
    m = (m | (m >> 1)) & 0x3333333333333333ull;
    m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0full;
    m = (m | (m >> 4)) & 0x00ff00ff00ff00ffull;
    m = (m | (m >> 8)) & 0x0000ffff0000ffffull;
    m = (m | (m >> 16)) & 0x00000000ffffffffull;
    return (uint32_t)m;
}

__device__ __forceinline__ uint32_t spread_bits(uint32_t x)      // 16 bits -> the even bits of 32
{
    x &= 0xffffu;
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// x[q] without an indexed array (which would live in scratch)
template <typename T> __device__ __forceinline__ T sel3(const T x[3], int q) { return q == 0 ? x[0] : q == 1 ? x[1] : x[2]; }

// the three vertex ids of face f if all of them are vertices
__device__ __forceinline__ bool face_ids(const int64_t *triangles, int64_t f, int64_t n_vertices, int64_t id[3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) id[k] = triangles[3 * f + k], ok = ok && id[k] >= 0 && id[k] < n_vertices;
    return ok;
}

__global__ void __launch_bounds__(AT_THREADS) atlas_levels_kernel(const double *__restrict__ vertices, int64_t n_vertices,
                                                                  const int64_t *__restrict__ triangles, int64_t n_faces, int32_t gutter,
                                                                  int32_t lmin, int32_t lmax, double rho4, int32_t *__restrict__ level,
                                                                  int32_t *__restrict__ rot, unsigned long long *__restrict__ hist)
{
#pragma clang fp contract(off)
    __shared__ int part[NL];
    if (threadIdx.x < NL) part[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t f = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * AT_THREADS) {
        int64_t id[3];
        int l = lmin, r = 0;
        if (face_ids(triangles, f, n_vertices, id)) {
            double a[3], b[3], c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = vertices[3 * id[0] + k], b[k] = vertices[3 * id[1] + k], c[k] = vertices[3 * id[2] + k];
            const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            const double e0[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
            const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
            const double c2 = (n0 * n0 + n1 * n1) + n2 * n2;
            if (fabs(c2) < INFINITY) {
                const double need = c2 * rho4;
                l = lmax;
                for (int t = lmin; t < lmax; ++t) {
                    const int64_t leg = ((int64_t)1 << t) - (3 * (int64_t)gutter + 1);
                    const double leg2 = (double)(leg * leg);
                    if (leg2 * leg2 >= need) { l = t; break; }
                }
            }
            // squared lengths of the edges opposite corner 0, 1, 2
            const double d0 = (e0[0] * e0[0] + e0[1] * e0[1]) + e0[2] * e0[2];
            const double d1 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
            const double d2 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
            double best = d0;
            if (d1 > best) best = d1, r = 1;
            if (d2 > best) r = 2;
        }
        level[f] = l, rot[f] = r;
        atomicAdd(&part[l], 1);
    }
    __syncthreads();
    if (threadIdx.x < NL && part[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)part[threadIdx.x]);
}

__global__ void __launch_bounds__(AT_THREADS) atlas_charts_kernel(Groups g, int64_t n_faces, const int64_t *__restrict__ order,
                                                                  const int32_t *__restrict__ rot,
                                                                  int32_t *__restrict__ chart, float *__restrict__ uv)
{
    for (int64_t k = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x; k < n_faces; k += (int64_t)gridDim.x * AT_THREADS) {
        const int64_t f = order[k];
        if (f < 0 || f >= n_faces) continue;
        // the group of rank k (the starts descend with the level)
        int l = g.lmin;
        for (int t = g.lmax; t > g.lmin; --t)
            if (k >= g.start[t] && k < g.start[t] + g.count[t]) l = t;
        const int64_t r = k - g.start[l];
        const uint64_t u = (uint64_t)(g.unit[l] + ((r >> 1) << (2 * (l - g.lmin))));
        const int32_t x0 = (int32_t)(even_bits(u) << g.lmin), y0 = (int32_t)(even_bits(u >> 1) << g.lmin);
        const int half = (int)(r & 1), ro = rot[f] >= 0 && rot[f] < 3 ? rot[f] : 0;
        chart[4 * f] = x0, chart[4 * f + 1] = y0, chart[4 * f + 2] = l | half << 8 | ro << 16, chart[4 * f + 3] = (int32_t)k;
        const int32_t s = 1 << l, leg = s - (3 * g.gutter + 1), gt = g.gutter;
        // a, b, c of the half's triangle in texels
        int32_t px[3], py[3];
        if (!half) px[0] = gt, py[0] = gt, px[1] = gt + leg, py[1] = gt, px[2] = gt, py[2] = gt + leg;
        else px[0] = s - gt, py[0] = s - gt, px[1] = s - gt - leg, py[1] = s - gt, px[2] = s - gt, py[2] = s - gt - leg;
        const float inv = 1.f / (float)g.size;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = (j + 3 - ro) % 3;                               // corner j of the face is corner q of the rotated order
            uv[6 * f + 2 * j] = (float)(x0 + sel3(px, q)) * inv, uv[6 * f + 2 * j + 1] = (float)(y0 + sel3(py, q)) * inv;
        }
    }
}

struct TexelArgs {
    Groups g;
    const int64_t *order;
    const int32_t *rot;
    const double *vertices;
    int64_t n_vertices;
    const int64_t *triangles;
    int64_t n_faces;
    const float *attr;
    int32_t channels;
    int32_t *face;
    float *bary, *point;
    uint8_t *flags;
    float *tex;
};

__global__ void __launch_bounds__(AT_THREADS) atlas_texels_kernel(TexelArgs a)
{
#pragma clang fp contract(off)
    const int W = a.g.size, lmin = a.g.lmin, lgw = 31 - __clz(W);
    const int64_t n_texels = (int64_t)W * W;
    const float fnan = __uint_as_float(0x7fc00000u);
    for (int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x; p < n_texels; p += (int64_t)gridDim.x * AT_THREADS) {
        const int i = (int)(p & (W - 1)), j = (int)(p >> lgw);              // column x, row y
        const int64_t m = (int64_t)(spread_bits((uint32_t)(i >> lmin)) | spread_bits((uint32_t)(j >> lmin)) << 1);
        int l = -1;
        for (int t = a.g.lmax; t >= lmin; --t) {
            const int64_t end = a.g.unit[t] + (((a.g.count[t] + 1) >> 1) << (2 * (t - lmin)));
            if (m >= a.g.unit[t] && m < end) l = t;
        }
        int64_t f = -1;
        int s = 0, il = 0, jl = 0, half = 0;
        if (l >= 0) {
            s = 1 << l, il = i & (s - 1), jl = j & (s - 1);
            half = il + jl >= s ? 1 : 0;
            const int64_t r = (((m - a.g.unit[l]) >> (2 * (l - lmin))) << 1) + half;
            if (r < a.g.count[l]) f = a.order[a.g.start[l] + r];
            if (f < 0 || f >= a.n_faces) f = -1;
        }
        a.face[p] = (int32_t)f;
        if (f < 0) {
            a.bary[2 * p] = 0.f, a.bary[2 * p + 1] = 0.f;
            a.point[3 * p] = 0.f, a.point[3 * p + 1] = 0.f, a.point[3 * p + 2] = 0.f;
            a.flags[p] = 0;
            if (a.tex)
                for (int c = 0; c < a.channels; ++c) a.tex[p * a.channels + c] = 0.f;
            continue;
        }
        const int gt = a.g.gutter, leg = s - (3 * gt + 1);
        // twice the distance of the texel centre from the legs, in texels: odd integers
        const int hx = half ? 2 * (s - gt) - (2 * il + 1) : (2 * il + 1) - 2 * gt;
        const int hy = half ? 2 * (s - gt) - (2 * jl + 1) : (2 * jl + 1) - 2 * gt;
        const double beta = (double)hx / (double)(2 * leg), gamma = (double)hy / (double)(2 * leg);
        a.flags[p] = (hx >= 0 && hy >= 0 && hx + hy <= 2 * leg) ? 1 : 0;
        const float bf = (float)beta, gf = (float)gamma;
        a.bary[2 * p] = bf, a.bary[2 * p + 1] = gf;
        int ro = a.rot[f];
        ro = ro >= 0 && ro < 3 ? ro : 0;
        int64_t id[3];
        const bool ok = face_ids(a.triangles, f, a.n_vertices, id);
        const int64_t ia = sel3(id, ro), ib = sel3(id, (ro + 1) % 3), ic = sel3(id, (ro + 2) % 3);
        if (!ok) {
            a.point[3 * p] = fnan, a.point[3 * p + 1] = fnan, a.point[3 * p + 2] = fnan;
            if (a.tex)
                for (int c = 0; c < a.channels; ++c) a.tex[p * a.channels + c] = fnan;
            continue;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double va = a.vertices[3 * ia + k], vb = a.vertices[3 * ib + k], vc = a.vertices[3 * ic + k];
            a.point[3 * p + k] = (float)((va + beta * (vb - va)) + gamma * (vc - va));
        }
        if (a.tex) {
            const float wa = (1.f - bf) - gf;
            for (int c = 0; c < a.channels; ++c) {
                const float xa = a.attr[ia * a.channels + c], xb = a.attr[ib * a.channels + c], xc = a.attr[ic * a.channels + c];
                a.tex[p * a.channels + c] = (wa * xa + bf * xb) + gf * xc;
            }
        }
    }
}

__global__ void __launch_bounds__(AT_THREADS) atlas_sample_kernel(const float *__restrict__ uv, int64_t n_faces, int32_t size,
                                                                  const float *__restrict__ tex, int32_t channels, int64_t n,
                                                                  const int32_t *__restrict__ q_face, const double *__restrict__ q_bary,
                                                                  float *__restrict__ out)
{
#pragma clang fp contract(off)
    for (int64_t q = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x; q < n; q += (int64_t)gridDim.x * AT_THREADS) {
        const int64_t f = q_face[q];
        bool live = f >= 0 && f < n_faces;
        double x = 0.0, y = 0.0;
        if (live) {
            const double bu = q_bary[2 * q], bv = q_bary[2 * q + 1], w0 = (1.0 - bu) - bv;
            const float *c = uv + 6 * f;
            const double u = (w0 * (double)c[0] + bu * (double)c[2]) + bv * (double)c[4];
            const double v = (w0 * (double)c[1] + bu * (double)c[3]) + bv * (double)c[5];
            x = u * (double)size - 0.5, y = v * (double)size - 0.5;
            live = fabs(x) < INFINITY && fabs(y) < INFINITY;
        }
        if (!live) {
            for (int c = 0; c < channels; ++c) out[q * channels + c] = 0.f;
            continue;
        }
        const double top = (double)size;
        const double xf = fmin(fmax(floor(x), -1.0), top), yf = fmin(fmax(floor(y), -1.0), top);
        // (a point outside the square keeps the weight of its own floor: the clamp moves the texels only)
        const float fx = (float)(x - floor(x)), fy = (float)(y - floor(y));
        const int i0 = min(max((int)xf, 0), size - 1), i1 = min(max((int)xf + 1, 0), size - 1);
        const int j0 = min(max((int)yf, 0), size - 1), j1 = min(max((int)yf + 1, 0), size - 1);
        const float *t00 = tex + ((int64_t)j0 * size + i0) * channels, *t10 = tex + ((int64_t)j0 * size + i1) * channels;
        const float *t01 = tex + ((int64_t)j1 * size + i0) * channels, *t11 = tex + ((int64_t)j1 * size + i1) * channels;
        const float gx = 1.f - fx, gy = 1.f - fy;
        for (int c = 0; c < channels; ++c)
            out[q * channels + c] = (t00[c] * gx + t10[c] * fx) * gy + (t01[c] * gx + t11[c] * fx) * fy;
    }
}

}  // namespace

ESR_API int esr_atlas_levels(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces, int32_t size,
                             int32_t gutter, int32_t lmin, int32_t lmax, double rho4, int32_t *level, int32_t *rot, int64_t *hist,
                             void *stream)
{
    if (n_faces < 0 || n_vertices < 0 || !layout_ok(size, gutter, lmin, lmax) || !(rho4 >= 0.0) || !(rho4 < INFINITY)) return ESR_EINVAL;
    const int64_t cap = (int64_t)1 << 31;
    if (n_faces >= cap || n_vertices >= cap) return ESR_ECAP;
    if (!given(hist, 8)) return ESR_EINVAL;
    if (n_faces && (!given(triangles, 8) || !given(level, 4) || !given(rot, 4) || (n_vertices && !given(vertices, 8)))) return ESR_EINVAL;
    hipStream_t st = esr_stream(stream);
    hipError_t e = hipMemsetAsync(hist, 0, NL * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    if (!n_faces) return 0;
    atlas_levels_kernel<<<esr_grid_for(n_faces, AT_THREADS), AT_THREADS, 0, st>>>(vertices, n_vertices, triangles, n_faces, gutter, lmin,
                                                                                 lmax, rho4, level, rot, (unsigned long long *)hist);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_atlas_charts(int64_t n_faces, const int64_t *order, const int32_t *rot, const int64_t *counts,
                             int32_t size, int32_t gutter, int32_t lmin, int32_t lmax, int32_t *chart, float *uv, void *stream)
{
    if (n_faces < 0 || !layout_ok(size, gutter, lmin, lmax) || !counts) return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31) return ESR_ECAP;
    Groups g;
    const int code = groups_from_counts(counts, n_faces, size, gutter, lmin, lmax, g);
    if (code) return code;
    if (!n_faces) return 0;
    if (!given(order, 8) || !given(rot, 4) || !given(chart, 4) || !given(uv, 4)) return ESR_EINVAL;
    atlas_charts_kernel<<<esr_grid_for(n_faces, AT_THREADS), AT_THREADS, 0, esr_stream(stream)>>>(g, n_faces, order, rot, chart, uv);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_atlas_texels(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces,
                             const int64_t *order, const int32_t *rot, const int64_t *counts, int32_t size, int32_t gutter,
                             int32_t lmin, int32_t lmax, const float *attr, int32_t channels, int32_t *face, float *bary, float *point,
                             uint8_t *flags, float *tex, void *stream)
{
    if (n_faces < 0 || n_vertices < 0 || !layout_ok(size, gutter, lmin, lmax) || !counts || channels < 0) return ESR_EINVAL;
    if ((attr != nullptr) != (tex != nullptr) || (attr != nullptr) != (channels > 0)) return ESR_EINVAL;
    const int64_t cap = (int64_t)1 << 31;
    if (n_faces >= cap || n_vertices >= cap || channels > ESR_ATLAS_MAX_CHANNELS) return ESR_ECAP;
    TexelArgs a{};
    const int code = groups_from_counts(counts, n_faces, size, gutter, lmin, lmax, a.g);
    if (code) return code;
    if (!given(face, 4) || !given(bary, 4) || !given(point, 4) || !flags || !optional(attr, 4) || !optional(tex, 4)) return ESR_EINVAL;
    if (n_faces && (!given(order, 8) || !given(rot, 4) || !given(triangles, 8) || (n_vertices && !given(vertices, 8)))) return ESR_EINVAL;
    a.order = order, a.rot = rot, a.vertices = vertices, a.n_vertices = n_vertices, a.triangles = triangles, a.n_faces = n_faces;
    a.attr = attr, a.channels = channels, a.face = face, a.bary = bary, a.point = point, a.flags = flags, a.tex = tex;
    atlas_texels_kernel<<<esr_grid_for((int64_t)size * size, AT_THREADS, AT_BLOCKS), AT_THREADS, 0, esr_stream(stream)>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_atlas_sample(const float *uv, int64_t n_faces, int32_t size, const float *tex, int32_t channels, int64_t n,
                             const int32_t *q_face, const double *q_bary, float *out, void *stream)
{
    if (n_faces < 0 || n < 0 || channels < 1 || size < ESR_ATLAS_MIN_SIZE || size > ESR_ATLAS_MAX_SIZE || (size & (size - 1)))
        return ESR_EINVAL;
    if (n_faces >= (int64_t)1 << 31 || n >= (int64_t)1 << 31 || channels > ESR_ATLAS_MAX_CHANNELS) return ESR_ECAP;
    if (!n) return 0;
    if (!given(tex, 4) || !given(q_face, 4) || !given(q_bary, 8) || !given(out, 4) || (n_faces && !given(uv, 4))) return ESR_EINVAL;
    atlas_sample_kernel<<<esr_grid_for(n, AT_THREADS), AT_THREADS, 0, esr_stream(stream)>>>(uv, n_faces, size, tex, channels, n, q_face,
                                                                                           q_bary, out);
    ESR_CHECK_LAUNCH();
    return 0;
}
