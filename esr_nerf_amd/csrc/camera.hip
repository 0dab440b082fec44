// Camera-defined ray sets: rays made in the kernel from (view, pixel) instead of read from per-ray arrays.
//
// Reference (paths under the reference tree): data/esrnerf/esrnerf.py:39-59,233-259 and data/dtu/dtu.py:74-86,175-211
// (pixelcoord, pose2ray, F.normalize, the colour compositing, the per-view em_mode), app/coarse/alphamask.py:108-122 (the
// frustum bounding box).  The ray arithmetic is the device function of camera_ray.h; this file adds the three kernels around
// it.  A training set of V views is then 48 B of pose per view and the images (4 B per pixel as RGBA8) instead of 56 B per ray.
//
// MI355X notes (wave64, plain C++, vector stores only, no atomics, nothing here is matrix work).
//   camera_rays_kernel   bound by its stores (36 B per ray).  A lane owns four consecutive FLOATS of each [n,3] output, not
//                        a ray: one 16-byte store per array, a wave writes 1 KiB contiguous per instruction.  Four floats
//                        touch at most two rays; both are computed and the components picked with selects.
//   camera_batch_kernel  one lane per row.  Rows are random, so the ray itself is pure arithmetic on the row's pose; the
//                        pose table is staged in LDS up to ESR_CAMERA_LDS_VIEWS = 256 views (12 KB: at that size a
//                        256-row workgroup stages exactly what 256 distinct views would have it read; beyond it staging
//                        moves more bytes than the gather, so the table is read through L1 / L2 from global memory).  The
//                        256-entry colour table sits in LDS as well (1 KB, one entry per lane of the workgroup).  The
//                        pixel gather is uncoalesced by nature: 4 B per row as one dword for RGBA8.  Outputs are 12 B per
//                        lane, contiguous across the wave.  Index arithmetic is 32-bit once the row is known to be in
//                        range (the host refuses sets of 2^31 rays or more).
//   camera_bounds_kernel grid-stride over all rays, per-lane running min / max of the two frustum points, xor-shuffle wave
//                        reduction, one LDS slot per wave, one 6-float partial per workgroup; camera_bounds_final_kernel
//                        folds the partials in one workgroup.
#include "camera_ray.h"
#include "esr_collectives.h"

#include <math.h>

namespace {

constexpr int CAM_THREADS = 256;

__device__ __forceinline__ float pick3(const float v[3], int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }

// ---- dense ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CAM_THREADS) camera_rays_kernel(esr_camera_t cam, const float *__restrict__ poses, int v0,
                                                                  int n_rays, float *__restrict__ rays_o,
                                                                  float *__restrict__ rays_d, float *__restrict__ viewdirs)
{
    const int hw = cam.width * cam.height;
    const int64_t total = 3 * (int64_t)n_rays;                 // floats per output array
    const int64_t n_quads = (total + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * CAM_THREADS + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * CAM_THREADS) {
        const int64_t e0 = 4 * q;
        const int ra = (int)(e0 / 3);                          // the quad's first ray; its floats end in ray ra or ra + 1
        const int rb = min(ra + 1, n_rays - 1);
        float o[2][3], d[2][3], vd[2][3];
        {
            const int va = ra / hw, vb = rb / hw;
            esr_camera_ray_at(cam, poses, v0 + va, ra - va * hw, o[0], d[0], vd[0]);
            esr_camera_ray_at(cam, poses, v0 + vb, rb - vb * hw, o[1], d[1], vd[1]);
        }
        float qo[4], qd[4], qv[4];
        const int c0 = (int)(e0 - 3 * (int64_t)ra);            // component of the quad's first float: 0, 1 or 2
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k;                              // 0 .. 5: components 3 .. 5 belong to the second ray
            const bool second = c >= 3;
            const int cc = second ? c - 3 : c;
            qo[k] = second ? pick3(o[1], cc) : pick3(o[0], cc);
            qd[k] = second ? pick3(d[1], cc) : pick3(d[0], cc);
            qv[k] = second ? pick3(vd[1], cc) : pick3(vd[0], cc);
        }
        if (e0 + 4 <= total) {
            *reinterpret_cast<float4 *>(rays_o + e0) = make_float4(qo[0], qo[1], qo[2], qo[3]);
            *reinterpret_cast<float4 *>(rays_d + e0) = make_float4(qd[0], qd[1], qd[2], qd[3]);
            *reinterpret_cast<float4 *>(viewdirs + e0) = make_float4(qv[0], qv[1], qv[2], qv[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < total) { rays_o[e0 + k] = qo[k]; rays_d[e0 + k] = qd[k]; viewdirs[e0 + k] = qv[k]; }
        }
    }
}

// ---- batch ----------------------------------------------------------------------------------------------------------------
struct BatchParams {
    esr_camera_t cam;
    const float *poses;
    const int64_t *view_modes;
    const void *images;
    const float *lut;
    const int64_t *rows;
    int64_t n;
    int channels;
    float white_bg;
    float *rays_o, *rays_d, *viewdirs, *rgbs;
    int64_t *em_modes;
};

// esrnerf.py:236: rgb * mask + (1 - mask) * white_bg, four separately rounded operations (the pragma, not HIP's __fmul_rn /
// __fadd_rn: those are plain operators to the compiler and contract into a fused multiply-add like any other)
__device__ __forceinline__ float over_white(float c, float a, float white_bg)
{
#pragma clang fp contract(off)
    const float ca = c * a;
    const float rest = (1.0f - a) * white_bg;
    return ca + rest;
}

template <bool POSES_IN_LDS>
__global__ void __launch_bounds__(CAM_THREADS) camera_batch_kernel(BatchParams P)
{
    __shared__ float lut_s[256];
    __shared__ __attribute__((aligned(16))) float pose_s[POSES_IN_LDS ? 12 * ESR_CAMERA_LDS_VIEWS : 4];
    const esr_camera_t &cam = P.cam;
    if (P.channels) lut_s[threadIdx.x] = P.lut[threadIdx.x];                    // (CAM_THREADS == 256 entries)
    if (POSES_IN_LDS)
        for (int k = threadIdx.x; k < 12 * cam.n_views; k += CAM_THREADS) pose_s[k] = P.poses[k];
    __syncthreads();
    const int hw = cam.width * cam.height;
    const int64_t total = (int64_t)cam.n_views * hw;
    const float nan = __builtin_nanf("");
    for (int64_t t = (int64_t)blockIdx.x * CAM_THREADS + threadIdx.x; t < P.n; t += (int64_t)gridDim.x * CAM_THREADS) {
        const int64_t row64 = P.rows[t];
        float o[3] = {nan, nan, nan}, d[3] = {nan, nan, nan}, vd[3] = {nan, nan, nan}, rgb[3] = {nan, nan, nan};
        int64_t mode = -1;
        if ((uint64_t)row64 < (uint64_t)total) {                                 // nothing is read for a row out of range
            const int row = (int)row64;
            const int view = row / hw, pixel = row - view * hw;
            esr_camera_ray_at(cam, POSES_IN_LDS ? pose_s : P.poses, view, pixel, o, d, vd);
            mode = P.view_modes[view];
            if (P.channels == 0) {
                const float *px = static_cast<const float *>(P.images) + 3 * (int64_t)row;
                rgb[0] = px[0]; rgb[1] = px[1]; rgb[2] = px[2];
            } else if (P.channels == 4) {
                const uint32_t w = static_cast<const uint32_t *>(P.images)[row];
                const float a = lut_s[w >> 24];
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[c] = over_white(lut_s[(w >> (8 * c)) & 255u], a, P.white_bg);
            } else {
                const uint8_t *px = static_cast<const uint8_t *>(P.images) + 3 * (int64_t)row;
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[c] = lut_s[px[c]];
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P.rays_o[3 * t + a] = o[a];
            P.rays_d[3 * t + a] = d[a];
            P.viewdirs[3 * t + a] = vd[a];
            P.rgbs[3 * t + a] = rgb[a];
        }
        P.em_modes[t] = mode;
    }
}

// ---- bounds ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CAM_THREADS) camera_bounds_kernel(esr_camera_t cam, const float *__restrict__ poses,
                                                                    float near_, float far_, float *__restrict__ partials)
{
    const int hw = cam.width * cam.height;
    const int64_t total = (int64_t)cam.n_views * hw;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t t = (int64_t)blockIdx.x * CAM_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * CAM_THREADS) {
        const int row = (int)t;
        const int view = row / hw;
        float o[3], d[3], vd[3];
        esr_camera_ray_at(cam, poses, view, row - view * hw, o, d, vd);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float pn = o[a] + vd[a] * near_, pf = o[a] + vd[a] * far_;
            lo[a] = fminf(lo[a], fminf(pn, pf));
            hi[a] = fmaxf(hi[a], fmaxf(pn, pf));
        }
    }
    esr_block_minmax3_store<CAM_THREADS>(lo, hi, partials + 6 * blockIdx.x);
}

__global__ void __launch_bounds__(CAM_THREADS) camera_bounds_final_kernel(const float *__restrict__ partials, int n_partials,
                                                                          float *__restrict__ out)
{
    esr_minmax3_partials<CAM_THREADS>(partials, n_partials, out);
}

bool camera_ok(const esr_camera_t *cam)
{
    if (!cam || cam->width < 1 || cam->height < 1 || cam->n_views < 0) return false;
    if (!(cam->fx != 0.f) || !(cam->fy != 0.f)) return false;
    return (int64_t)cam->n_views * cam->width * cam->height < ((int64_t)1 << 31);
}

}  // namespace

ESR_API int esr_camera_rays(const esr_camera_t *cam, const float *poses, int32_t v0, int32_t v1, float *rays_o, float *rays_d,
                            float *viewdirs, void *stream)
{
    if (!camera_ok(cam) || v0 < 0 || v1 < v0 || v1 > cam->n_views) return ESR_EINVAL;
    const int64_t n_rays = (int64_t)(v1 - v0) * cam->width * cam->height;
    if (!n_rays) return 0;
    if (!poses || !rays_o || !rays_d || !viewdirs) return ESR_EINVAL;
    if (((uintptr_t)rays_o | (uintptr_t)rays_d | (uintptr_t)viewdirs) & 15) return ESR_EINVAL;
    const int grid = esr_grid_for((3 * n_rays + 3) / 4, CAM_THREADS);
    camera_rays_kernel<<<grid, CAM_THREADS, 0, esr_stream(stream)>>>(*cam, poses, v0, (int)n_rays, rays_o, rays_d, viewdirs);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_camera_batch(const esr_camera_t *cam, const float *poses, const int64_t *view_modes, const void *images,
                             int32_t channels, const float *lut, float white_bg, const int64_t *rows, int64_t n, float *rays_o,
                             float *rays_d, float *viewdirs, float *rgbs, int64_t *em_modes, void *stream)
{
    if (!camera_ok(cam) || n < 0 || (channels != 0 && channels != 3 && channels != 4)) return ESR_EINVAL;
    if (!n) return 0;
    if (!poses || !view_modes || !images || !rows || !rays_o || !rays_d || !viewdirs || !rgbs || !em_modes) return ESR_EINVAL;
    if (channels && !lut) return ESR_EINVAL;
    if (channels == 4 && ((uintptr_t)images & 3)) return ESR_EINVAL;
    BatchParams P;
    P.cam = *cam; P.poses = poses; P.view_modes = view_modes; P.images = images; P.lut = lut; P.rows = rows; P.n = n;
    P.channels = channels; P.white_bg = white_bg;
    P.rays_o = rays_o; P.rays_d = rays_d; P.viewdirs = viewdirs; P.rgbs = rgbs; P.em_modes = em_modes;
    const int grid = esr_grid_for(n, CAM_THREADS);
    if (cam->n_views <= ESR_CAMERA_LDS_VIEWS)
        camera_batch_kernel<true><<<grid, CAM_THREADS, 0, esr_stream(stream)>>>(P);
    else
        camera_batch_kernel<false><<<grid, CAM_THREADS, 0, esr_stream(stream)>>>(P);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_camera_bounds(const esr_camera_t *cam, const float *poses, float near_, float far_, float *partials, float *out,
                              void *stream)
{
    if (!camera_ok(cam) || !partials || !out) return ESR_EINVAL;
    const int64_t total = (int64_t)cam->n_views * cam->width * cam->height;
    if (total && !poses) return ESR_EINVAL;
    const int grid = esr_grid_for(total, CAM_THREADS, ESR_CAMERA_BOUNDS_BLOCKS);
    camera_bounds_kernel<<<grid, CAM_THREADS, 0, esr_stream(stream)>>>(*cam, poses, near_, far_, partials);
    ESR_CHECK_LAUNCH();
    camera_bounds_final_kernel<<<1, CAM_THREADS, 0, esr_stream(stream)>>>(partials, grid, out);
    ESR_CHECK_LAUNCH();
    return 0;
}
