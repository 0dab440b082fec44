// Stage hand-over on the device: what runs when one stage gives its grids to the next.
//
// Reference (paths under the reference tree): app/utils/base/module.py:37-49 (DenseGrid.scale_volume_grid: F.interpolate,
// trilinear, align_corners=True), :78-114 (MaskCache: F.max_pool3d at construction, grid_sample + softplus + exp in forward),
// app/fine/model/voxurff.py:571-593 / app/coarse/model/voxurfc.py:491-513 (set_nonempty_mask), app/coarse/coarse.py:152-182
// (compute_bbox_by_coarse_geo).
//
// MI355X notes (wave64, plain C++, vector loads and stores only, no LDS tiles; none of this is matrix work and each kernel
// runs once per hand-over, so every one of them is a grid-stride element-wise kernel bound by the bytes it moves).
//   grid_resample_kernel   one lane per OUTPUT cell and all its channels; consecutive lanes take consecutive z, so a wave's
//                          stores cover one contiguous run (24 B per lane at 6 channels).  Every access is one dword: the
//                          records of a channels-last grid are only 4-byte aligned (24 B, 48 B), and a caller's pointer may
//                          be too.  All eight corner indices are in range by construction (the high corner is the low one
//                          where the low one is the last node), so the 8 * C loads of a cell are unconditional and issue back
//                          to back (the esr_ld_or0 note of esr_common.h).  Neighbouring output cells share corners through L2.
//   maxpool3d_kernel       the direct ks^3 window, clipped to the volume (the padding is -inf: a clipped tap never wins).
//   nonempty_mask_kernel   the march's own mask-cache lookup at every grid node; the true cells are summed over the wave by
//                          shuffle, one LDS slot per wave, one integer atomic per workgroup (integer addition: the same count whatever the
//                          order).
//   density_bounds_kernel  the same lookup on the alphamask density; per-lane running min / max of the active coordinates,
//                          xor-shuffle wave reduction, one 6-float partial per workgroup, a final one-workgroup pass
//                          (esr_camera_bounds' scheme); the count as above.
#include "esr_collectives.h"

#include <math.h>

namespace {

constexpr int GS_THREADS = 256;

// ---- trilinear resample, align_corners=True, channels-last ---------------------------------------------------------------
struct ResampleParams {
    const float *in;
    float *out;
    int n_in[3], n_out[3];
    float scale[3];             // (n_in - 1) / (n_out - 1) in binary32, 0 when n_out == 1
    int c_rt;
};

struct Axis {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Axis resample_axis(float scale, int dst, int n_in)
{
#pragma clang fp contract(off)
    Axis a;
    const float src = scale * (float)dst;
    a.i0 = min((int)src, n_in - 1);              // (never taken: scale * (n_out - 1) rounds to at most n_in - 1 and an ulp)
    a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
    a.l1 = src - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    return a;
}

// CT > 0: the channel count at compile time (the loops unroll: 8 * CT loads in flight); CT == 0: P.c_rt channels, one at a time
template <int CT>
__global__ void __launch_bounds__(GS_THREADS) grid_resample_kernel(ResampleParams P)
{
#pragma clang fp contract(off)
    const int C = CT ? CT : P.c_rt;
    const int oy = P.n_out[1], oz = P.n_out[2];
    const int64_t n = (int64_t)P.n_out[0] * oy * oz;
    const int64_t sy = (int64_t)P.n_in[2] * C, sx = (int64_t)P.n_in[1] * sy;        // input strides in floats
    for (int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * GS_THREADS) {
        const int z = (int)(t % oz), y = (int)(t / oz % oy), x = (int)(t / ((int64_t)oy * oz));
        const Axis ax = resample_axis(P.scale[0], x, P.n_in[0]);
        const Axis ay = resample_axis(P.scale[1], y, P.n_in[1]);
        const Axis az = resample_axis(P.scale[2], z, P.n_in[2]);
        const int64_t bx[2] = {ax.i0 * sx, ax.i1 * sx}, by[2] = {ay.i0 * sy, ay.i1 * sy};
        const int64_t bz[2] = {(int64_t)az.i0 * C, (int64_t)az.i1 * C};
        const float *__restrict__ corner[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) corner[k] = P.in + bx[k >> 2] + by[(k >> 1) & 1] + bz[k & 1];
        float *__restrict__ o = P.out + t * C;
        if (CT) {
            float v[8][CT ? CT : 1];
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int c = 0; c < CT; ++c) v[k][c] = corner[k][c];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const float lo = ay.l0 * (az.l0 * v[0][c] + az.l1 * v[1][c]) + ay.l1 * (az.l0 * v[2][c] + az.l1 * v[3][c]);
                const float hi = ay.l0 * (az.l0 * v[4][c] + az.l1 * v[5][c]) + ay.l1 * (az.l0 * v[6][c] + az.l1 * v[7][c]);
                o[c] = ax.l0 * lo + ax.l1 * hi;
            }
        } else {
            for (int c = 0; c < C; ++c) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = corner[k][c];
                const float lo = ay.l0 * (az.l0 * v[0] + az.l1 * v[1]) + ay.l1 * (az.l0 * v[2] + az.l1 * v[3]);
                const float hi = ay.l0 * (az.l0 * v[4] + az.l1 * v[5]) + ay.l1 * (az.l0 * v[6] + az.l1 * v[7]);
                o[c] = ax.l0 * lo + ax.l1 * hi;
            }
        }
    }
}

// ---- max pool, stride 1, padding ks / 2 of -inf ---------------------------------------------------------------------------
__global__ void __launch_bounds__(GS_THREADS) maxpool3d_kernel(const float *__restrict__ in, int gx, int gy, int gz, int r,
                                                               float *__restrict__ out)
{
    const int64_t n = (int64_t)gx * gy * gz;
    for (int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * GS_THREADS) {
        const int z = (int)(t % gz), y = (int)(t / gz % gy), x = (int)(t / ((int64_t)gy * gz));
        const int x0 = max(x - r, 0), x1 = min(x + r, gx - 1);
        const int y0 = max(y - r, 0), y1 = min(y + r, gy - 1);
        const int z0 = max(z - r, 0), z1 = min(z + r, gz - 1);
        float m = -INFINITY;
        for (int a = x0; a <= x1; ++a)
            for (int b = y0; b <= y1; ++b) {
                const float *__restrict__ row = in + ((int64_t)a * gy + b) * gz;
                for (int c = z0; c <= z1; ++c) {
                    const float v = row[c];
                    if (v > m || v != v) m = v;                     // (a NaN wins and stays, as in ATen's max_pool3d)
                }
            }
        out[t] = m;
    }
}

// ---- the mask-cache lookup at the nodes of a lattice ----------------------------------------------------------------------
struct NodeParams {
    const float *vol;           // [dims] f32: the pooled mask density / the alphamask density
    int dims[3];
    float lo[3], hi[3];         // the box of vol
    float act_shift, thres;
    const float *xs, *ys, *zs;  // the lattice's axes
    int n[3];
    float *sdf;
    uint8_t *mask_out;
    float *part;
    unsigned long long *count_out;
};

__device__ __forceinline__ float node_density(const NodeParams &P, int64_t t, float p[3])
{
    const int k = (int)(t % P.n[2]), j = (int)(t / P.n[2] % P.n[1]), i = (int)(t / ((int64_t)P.n[1] * P.n[2]));
    p[0] = P.xs[i]; p[1] = P.ys[j]; p[2] = P.zs[k];
    float idx[3];
    esr_world_to_index(p, P.lo, P.hi, P.dims, idx);
    return esr_tri_fetch1(P.vol, P.dims, idx);
}

// the workgroup's sum of per-lane counts added to *count_out: wave sums through the shuffle, one LDS slot per wave, one atomic
__device__ __forceinline__ void block_count_add(unsigned cnt, unsigned long long *__restrict__ count_out)
{
    __shared__ unsigned wave_cnt[GS_THREADS / ESR_WAVE];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, ESR_WAVE);
    if (esr_lane() == 0) wave_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < GS_THREADS / ESR_WAVE; ++w) s += wave_cnt[w];
        if (s) atomicAdd(count_out, s);
    }
}

__global__ void __launch_bounds__(GS_THREADS) nonempty_mask_kernel(NodeParams P)
{
    const int64_t n = (int64_t)P.n[0] * P.n[1] * P.n[2];
    unsigned cnt = 0;
    for (int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * GS_THREADS) {
        float p[3];
        const float dens = node_density(P, t, p);
        const float a = 1.f - expf(-esr_softplus(dens + P.act_shift));       // (march.hip, rayfilter.hip: the same expression)
        const bool m = a >= P.thres;
        P.mask_out[t] = m ? 1 : 0;
        if (P.sdf && !m) P.sdf[t] = 1.f;
        cnt += m ? 1u : 0u;
    }
    block_count_add(cnt, P.count_out);
}

__global__ void __launch_bounds__(GS_THREADS) density_bounds_kernel(NodeParams P)
{
    const int64_t n = (int64_t)P.n[0] * P.n[1] * P.n[2];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned cnt = 0;
    for (int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * GS_THREADS) {
        float p[3];
        const float dens = node_density(P, t, p);
        const bool active = esr_dvgo_alpha(dens, P.act_shift, 1.f) > P.thres;          // strict (coarse.py:171)
        cnt += active ? 1u : 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = active ? fminf(lo[a], p[a]) : lo[a];
            hi[a] = active ? fmaxf(hi[a], p[a]) : hi[a];
        }
    }
    esr_block_minmax3_store<GS_THREADS>(lo, hi, P.part + 6 * blockIdx.x);
    block_count_add(cnt, P.count_out);
}

__global__ void __launch_bounds__(GS_THREADS) density_bounds_final_kernel(const float *__restrict__ partials, int n_partials,
                                                                          float *__restrict__ out)
{
    esr_minmax3_partials<GS_THREADS>(partials, n_partials, out);
}

bool dims_ok(int64_t a, int64_t b, int64_t c, int64_t per_cell = 1)
{
    return a >= 1 && b >= 1 && c >= 1 && a * b * c * per_cell < ((int64_t)1 << 40);
}

float axis_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }

}  // namespace

ESR_API int esr_grid_resample(const float *in, int32_t gx, int32_t gy, int32_t gz, int32_t C, float *out, int32_t ox, int32_t oy,
                              int32_t oz, void *stream)
{
    if (!in || !out || C < 1 || C > ESR_RESAMPLE_MAX_C) return ESR_EINVAL;
    if (!dims_ok(gx, gy, gz, C) || !dims_ok(ox, oy, oz, C)) return ESR_EINVAL;
    if ((((uintptr_t)in) | ((uintptr_t)out)) & 3) return ESR_EINVAL;
    ResampleParams P;
    P.in = in; P.out = out; P.c_rt = C;
    P.n_in[0] = gx; P.n_in[1] = gy; P.n_in[2] = gz;
    P.n_out[0] = ox; P.n_out[1] = oy; P.n_out[2] = oz;
    for (int a = 0; a < 3; ++a) P.scale[a] = axis_scale(P.n_in[a], P.n_out[a]);
    const int grid = esr_grid_for((int64_t)ox * oy * oz, GS_THREADS, 256 * 16);
    hipStream_t s = esr_stream(stream);
    switch (C) {
    case 1:  grid_resample_kernel<1><<<grid, GS_THREADS, 0, s>>>(P); break;
    case 6:  grid_resample_kernel<6><<<grid, GS_THREADS, 0, s>>>(P); break;      // the fine stage's colour grids
    case 12: grid_resample_kernel<12><<<grid, GS_THREADS, 0, s>>>(P); break;     // the coarse stage's
    default: grid_resample_kernel<0><<<grid, GS_THREADS, 0, s>>>(P); break;
    }
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_maxpool3d(const float *in, int32_t gx, int32_t gy, int32_t gz, int32_t ks, float *out, void *stream)
{
    if (!in || !out || !dims_ok(gx, gy, gz) || ks < 1 || ks > 7 || !(ks & 1)) return ESR_EINVAL;
    maxpool3d_kernel<<<esr_grid_for((int64_t)gx * gy * gz, GS_THREADS, 256 * 16), GS_THREADS, 0, esr_stream(stream)>>>(
        in, gx, gy, gz, ks / 2, out);
    ESR_CHECK_LAUNCH();
    return 0;
}

static int node_params(NodeParams &P, const float *vol, int32_t mx, int32_t my, int32_t mz, const float *box_host,
                       float act_shift, float thres, const float *xs, const float *ys, const float *zs, int32_t X, int32_t Y,
                       int32_t Z)
{
    if (!vol || !box_host || !xs || !ys || !zs || !dims_ok(mx, my, mz) || !dims_ok(X, Y, Z)) return ESR_EINVAL;
    P.vol = vol; P.xs = xs; P.ys = ys; P.zs = zs;
    P.dims[0] = mx; P.dims[1] = my; P.dims[2] = mz;
    P.n[0] = X; P.n[1] = Y; P.n[2] = Z;
    for (int a = 0; a < 3; ++a) {
        P.lo[a] = box_host[a];
        P.hi[a] = box_host[3 + a];
    }
    P.act_shift = act_shift; P.thres = thres;
    P.sdf = nullptr; P.mask_out = nullptr; P.part = nullptr; P.count_out = nullptr;
    return 0;
}

ESR_API int esr_nonempty_mask(const float *pooled, int32_t mx, int32_t my, int32_t mz, const float *mask_box_host, float act_shift,
                              float thres, const float *xs, const float *ys, const float *zs, int32_t X, int32_t Y, int32_t Z,
                              float *sdf, uint8_t *mask_out, int64_t *count_out, void *stream)
{
    NodeParams P;
    const int rc = node_params(P, pooled, mx, my, mz, mask_box_host, act_shift, thres, xs, ys, zs, X, Y, Z);
    if (rc) return rc;
    if (!mask_out || !count_out) return ESR_EINVAL;
    P.sdf = sdf; P.mask_out = mask_out; P.count_out = reinterpret_cast<unsigned long long *>(count_out);
    nonempty_mask_kernel<<<esr_grid_for((int64_t)X * Y * Z, GS_THREADS, 256 * 16), GS_THREADS, 0, esr_stream(stream)>>>(P);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_density_bounds(const float *density, int32_t gx, int32_t gy, int32_t gz, const float *box_host, float act_shift,
                               float thres, const float *xs, const float *ys, const float *zs, float *part, float *out6,
                               int64_t *count_out, void *stream)
{
    NodeParams P;
    const int rc = node_params(P, density, gx, gy, gz, box_host, act_shift, thres, xs, ys, zs, gx, gy, gz);
    if (rc) return rc;
    if (!part || !out6 || !count_out) return ESR_EINVAL;
    P.part = part; P.count_out = reinterpret_cast<unsigned long long *>(count_out);
    const int grid = esr_grid_for((int64_t)gx * gy * gz, GS_THREADS, ESR_DENSITY_BOUNDS_BLOCKS);
    density_bounds_kernel<<<grid, GS_THREADS, 0, esr_stream(stream)>>>(P);
    ESR_CHECK_LAUNCH();
    density_bounds_final_kernel<<<1, GS_THREADS, 0, esr_stream(stream)>>>(part, grid, out6);
    ESR_CHECK_LAUNCH();
    return 0;
}
