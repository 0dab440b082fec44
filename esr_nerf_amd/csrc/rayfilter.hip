// Training-ray filter: one flag per ray, "does any in-box sample of this ray lie inside the mask cache".
//
// Reference algorithm (paths under the reference tree):
//   app/coarse/model/voxurfc.py:426-446   filter_training_rays_in_maskcache_sampling (always the fixed sampler)
//   app/fine/model/voxurff.py:463-502     the same, two branches: sdf_random_init -> fixed sampler, else the march sampler
//   app/coarse/model/voxurfc.py:448-481 = app/fine/model/voxurff.py:504-537   sample_ray_ori (the fixed sampler)
//   render_utils_kernel.cu:12-79,167-194  sample_pts_on_rays (the march sampler, called with far = 1e9)
//   app/utils/base/module.py:104-114      MaskCache.forward
// The reference materialises every sample of a chunk (points, out-of-box mask, ray / step ids), compacts by boolean mask,
// runs grid_sample on the survivors and scatters a hit flag back, chunk after chunk.  The result is one bit per ray.
//
// Two samplers, because they keep different ray sets.  Every operation below is a separately rounded binary32 operation in
// the reference's order (contraction off).
//   MARCH: esr_ray_geom with far = 1e9 (t-range, n_steps = max(ceil((t_max - t_min) |d| / stepdist), 1), start = o + d t_min,
//          dir = d / |d|), sample k = start + dir * (stepdist * k), k = 0 .. n_steps - 1: phase 1 of march_kernel
//          (csrc/march.hip) without its per-ray capacity -- a ray of any length is walked.
//   FIXED: t_min / t_max as above but clamped as torch.clamp(min=near, max=far) with the model's own far; a ray with
//          t_max <= t_min is a miss; every ray gets the same n_samples (host: int(|grid_shape + 1| / stepsize) + 1);
//          sample k = o + d * (t_min + (stepdist * k) / |d|).
// A sample is outside the box when xyz_min > p or p > xyz_max on any axis (both samplers).  An inside sample is a hit when
// 1 - exp(-softplus(density(p) + act_shift)) >= mask_thres, density = the trilinear (align_corners, zero padding) sample of
// the max-pooled mask density: the mask test of march_kernel, through the same helpers of esr_common.h.
//
// MI355X notes.  One 64-lane wave per ray (grid-stride over rays), lanes take consecutive steps, 64 per trip; a ballot of
// the hits ends the ray at the first trip that has one, lane 0 stores the uint8 flag (and, on request, the int32 index of the
// first kept step from the ballot word, or -1).  No LDS, no atomics, no intermediate buffer; the ray index is wave-uniform,
// so a ray's 24 B come through the scalar cache and the per-ray geometry lives in scalar registers.  Streamed traffic is
// 24 B read and 1 B (5 B) written per ray; the mask grid (a few tens of MB at the reference's resolution) is gathered from
// L2 / Infinity Cache.  Few enough vector registers for eight waves per SIMD (tests/test_ray_filter_isa.py).
//
// Ray source.  The kernel body is a template over where a ray comes from: ArrayRays loads it from rays_o / rays_d
// (esr_ray_filter), CameraRays makes it from (view, pixel) with the device function of camera_ray.h
// (esr_ray_filter_cameras: no ray array is read at all, 1 B (5 B) of traffic per ray).  The row, hence view and pixel, is
// wave-uniform, so the pose comes through the scalar cache as the array ray does.  Each source has its own __global__ entry
// around the one body, so the array kernels keep their symbols and their code: 58 (fixed) / 57 (march) vector registers, no
// scratch, eight waves per SIMD, before and after the body became a template.  The camera kernels: 48 / 46 vector registers, no
// scratch; the march instantiation fits eight waves per SIMD, the fixed one SEVEN: its wave-uniform ray arithmetic lives in
// scalar registers and takes 99 of them, three more than eight waves leave each (tools/kernel_meta.py).
#include "camera_ray.h"

#include <math.h>

namespace {

constexpr int RF_THREADS = 256;

struct FilterParams {
    esr_scene_t sc;
    const float *mask_density, *rays_o, *rays_d;
    int64_t n_rays;
    float far_;
    int n_samples;
    uint8_t *keep;
    int32_t *first_hit;
};

__device__ __forceinline__ bool mask_cache_hit(const esr_scene_t &sc, const float *__restrict__ mask_density,
                                               const int mdims[3], const float p[3])
{
    float idx[3];
    esr_world_to_index(p, sc.mask_min, sc.mask_max, mdims, idx);
    const float dens = esr_tri_fetch1(mask_density, mdims, idx);
    const float a = 1.f - expf(-esr_softplus(dens + sc.act_shift));
    return a >= sc.mask_thres;
}

// sample_ray_ori's t-range: torch.clamp(min=near, max=far) is min(max(x, near), far)
__device__ __forceinline__ void fixed_trange(const float o[3], const float d[3], const esr_scene_t &sc, float far_,
                                             float &tmin, float &tmax)
{
#pragma clang fp contract(off)
    float lo = 0.f, hi = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = (d[a] == 0.0f) ? (float)1e-6 : d[a];
        const float ta = __fdiv_rn(sc.xyz_max[a] - o[a], v);
        const float tb = __fdiv_rn(sc.xyz_min[a] - o[a], v);
        const float mn = fminf(ta, tb), mx = fmaxf(ta, tb);
        if (a == 0) { lo = mn; hi = mx; }
        else        { lo = fmaxf(lo, mn); hi = fminf(hi, mx); }
    }
    tmin = fminf(fmaxf(lo, sc.near_), far_);
    tmax = fminf(fmaxf(hi, sc.near_), far_);
}

// o + d * (t_min + (stepdist * k) / |d|), in that order
__device__ __forceinline__ void fixed_point(const float o[3], const float d[3], float tmin, float nrm, float stepdist,
                                            int k, float p[3])
{
#pragma clang fp contract(off)
    const float step = stepdist * (float)k;
    const float t = tmin + __fdiv_rn(step, nrm);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = o[a] + d[a] * t;
}

struct ArrayRays {
    const float *rays_o, *rays_d;
    __device__ __forceinline__ void load(int64_t r, float o[3], float d[3]) const
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) { o[a] = rays_o[3 * r + a]; d[a] = rays_d[3 * r + a]; }
    }
};

struct CameraRays {
    esr_camera_t cam;
    const float *poses;
    __device__ __forceinline__ void load(int64_t r, float o[3], float d[3]) const
    {
        const int hw = cam.width * cam.height, row = (int)r;          // (the host refuses sets of 2^31 rays or more)
        const int view = row / hw;
        float vd[3];
        esr_camera_ray_at(cam, poses, view, row - view * hw, o, d, vd);
    }
};

template <bool FIXED, class SRC>
__device__ __forceinline__ void ray_filter_body(const FilterParams &P, const SRC &src)
{
    const esr_scene_t &sc = P.sc;
    const int lane = esr_lane();
    const int mdims[3] = {sc.mx, sc.my, sc.mz};
    const int waves_per_blk = RF_THREADS / ESR_WAVE;
    const int64_t n_waves = (int64_t)gridDim.x * waves_per_blk;
    // (wave-uniform by construction; readfirstlane tells the compiler)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t r = (int64_t)blockIdx.x * waves_per_blk + wave; r < P.n_rays; r += n_waves) {
        int n_steps;
        float o[3], d[3], tmin = 0.f, nrm = 1.f;
        RayGeom g;
        src.load(r, o, d);
        if (FIXED) {
            float tmax;
            fixed_trange(o, d, sc, P.far_, tmin, tmax);
            nrm = esr_ray_norm(d);
            n_steps = (tmax <= tmin) ? 0 : P.n_samples;
        } else {
            g = esr_ray_geom(o, d, 0, sc.xyz_min, sc.xyz_max, sc.near_, 1e9f, sc.stepdist);
            n_steps = g.n_steps;
        }
        int first = -1;
        // (unsigned trip counter: n_steps <= 2^31 - 1, so c0 + 64 cannot wrap)
        for (unsigned c0 = 0; c0 < (unsigned)n_steps; c0 += ESR_WAVE) {
            const int step = (int)c0 + lane;
            float p[3];
            if (FIXED) fixed_point(o, d, tmin, nrm, sc.stepdist, step, p);
            else       esr_ray_point(g.start, g.dir, sc.stepdist, step, p);
            bool ok = (unsigned)step < (unsigned)n_steps && !esr_out_of_box(p, sc.xyz_min, sc.xyz_max);
            if (ok) ok = mask_cache_hit(sc, P.mask_density, mdims, p);
            const unsigned long long b = __ballot(ok);
            if (b) {
                first = (int)c0 + __ffsll((long long)b) - 1;
                break;
            }
        }
        if (lane == 0) {
            P.keep[r] = first >= 0 ? 1 : 0;
            if (P.first_hit) P.first_hit[r] = first;
        }
    }
}

template <bool FIXED>
__global__ void __launch_bounds__(RF_THREADS) ray_filter_kernel(FilterParams P)
{
    ray_filter_body<FIXED>(P, ArrayRays{P.rays_o, P.rays_d});
}

template <bool FIXED>
__global__ void __launch_bounds__(RF_THREADS) camera_filter_kernel(FilterParams P, CameraRays src)
{
    ray_filter_body<FIXED>(P, src);
}

}  // namespace

ESR_API int esr_ray_filter(const esr_scene_t *scene, const float *mask_density, const float *rays_o, const float *rays_d,
                           int64_t n_rays, int32_t mode, float far_, int32_t n_samples, uint8_t *keep, int32_t *first_hit,
                           void *stream)
{
    if (!scene || n_rays < 0 || (mode != ESR_RAY_FILTER_MARCH && mode != ESR_RAY_FILTER_FIXED)) return ESR_EINVAL;
    if (mode == ESR_RAY_FILTER_FIXED && n_samples < 0) return ESR_EINVAL;
    if (!n_rays) return 0;
    if (!mask_density || !rays_o || !rays_d || !keep) return ESR_EINVAL;
    if (scene->mx < 1 || scene->my < 1 || scene->mz < 1) return ESR_EINVAL;
    FilterParams P;
    P.sc = *scene;
    P.mask_density = mask_density; P.rays_o = rays_o; P.rays_d = rays_d;
    P.n_rays = n_rays; P.far_ = far_; P.n_samples = n_samples; P.keep = keep; P.first_hit = first_hit;
    const int grid = esr_grid_for(n_rays, RF_THREADS / ESR_WAVE);      // one resident wave per SIMD slot at most
    if (mode == ESR_RAY_FILTER_FIXED)
        ray_filter_kernel<true><<<grid, RF_THREADS, 0, esr_stream(stream)>>>(P);
    else
        ray_filter_kernel<false><<<grid, RF_THREADS, 0, esr_stream(stream)>>>(P);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_ray_filter_cameras(const esr_scene_t *scene, const float *mask_density, const esr_camera_t *cam,
                                   const float *poses, int32_t mode, float far_, int32_t n_samples, uint8_t *keep,
                                   int32_t *first_hit, void *stream)
{
    if (!scene || !cam || (mode != ESR_RAY_FILTER_MARCH && mode != ESR_RAY_FILTER_FIXED)) return ESR_EINVAL;
    if (mode == ESR_RAY_FILTER_FIXED && n_samples < 0) return ESR_EINVAL;
    if (cam->width < 1 || cam->height < 1 || cam->n_views < 0 || !(cam->fx != 0.f) || !(cam->fy != 0.f)) return ESR_EINVAL;
    const int64_t n_rays = (int64_t)cam->n_views * cam->width * cam->height;
    if (n_rays >= ((int64_t)1 << 31)) return ESR_EINVAL;
    if (!n_rays) return 0;
    if (!mask_density || !poses || !keep) return ESR_EINVAL;
    if (scene->mx < 1 || scene->my < 1 || scene->mz < 1) return ESR_EINVAL;
    FilterParams P;
    P.sc = *scene;
    P.mask_density = mask_density; P.rays_o = nullptr; P.rays_d = nullptr;
    P.n_rays = n_rays; P.far_ = far_; P.n_samples = n_samples; P.keep = keep; P.first_hit = first_hit;
    const CameraRays src{*cam, poses};
    const int grid = esr_grid_for(n_rays, RF_THREADS / ESR_WAVE);
    if (mode == ESR_RAY_FILTER_FIXED)
        camera_filter_kernel<true><<<grid, RF_THREADS, 0, esr_stream(stream)>>>(P, src);
    else
        camera_filter_kernel<false><<<grid, RF_THREADS, 0, esr_stream(stream)>>>(P, src);
    ESR_CHECK_LAUNCH();
    return 0;
}
