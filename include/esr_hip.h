/*
 * esr_hip.h -- C ABI of libesr_hip.so, the MI355X (gfx950) implementation of
 * ESR-NeRF's volumetric-rendering hot path.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer is CALLER-OWNED DEVICE memory, contiguous, unless marked
 *     [host]; outputs are never allocated inside the library.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     kernel is enqueued on it, nothing synchronises the device.
 *   - return value: 0 on success, otherwise the (positive) hipError_t of the
 *     failing runtime call, or a negative ESR_E* argument error.  Nothing throws
 *     across the ABI.  The Python shim re-raises non-zero codes as RuntimeError,
 *     which is what the reference's TORCH_CHECK failures surface as
 *     (app/utils/base/cuda/render_utils.cpp:46-48).
 *   - re-entrant.  The only process-wide state is an idempotent per-(kernel, device) memo of the > 64 KB
 *     dynamic-LDS opt-in (hipFuncSetAttribute); no environment variable is read on a launch path.
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   app/utils/base/cuda/render_utils.cpp:170-184  pybind module render_utils_cuda
 *   app/utils/base/cuda/total_variation.cpp:29-32 pybind module total_variation_cuda
 *   torch_scatter.segment_coo (third party; call sites app/fine/model/voxurff.py:260-272)
 *   and, for the fused fine-stage ops, the torch-level body of
 *   VoxurfF.forward_training (app/fine/model/voxurff.py:177-278).
 */
#ifndef ESR_HIP_H
#define ESR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESR_EINVAL (-1)   /* bad argument (null pointer, negative size, bad dims) */
#define ESR_ECAP   (-2)   /* a capacity limit of the kernels is exceeded          */

#define ESR_TILE 32       /* samples per tile of the tile-major activation layout  */

#define ESR_ABI_VERSION 48
int esr_abi_version(void);          /* ESR_ABI_VERSION: bumps whenever a signature below changes */
const char *esr_build_info(void);   /* "gfx950 <date>"                         */

/* ------------------------------------------------------------------------- *
 * A. Drop-in replacements of the reference's native ops (same arithmetic,
 *    same outputs, caller allocates).
 * ------------------------------------------------------------------------- */

/*
 * sample_pts_on_rays, phase 1 -- replaces infer_t_minmax + infer_n_samples +
 * N_steps.cumsum + N_steps.sum (render_utils_kernel.cu:12-55,204-212).
 * rays_o, rays_d [n_rays,3] f32; xyz_min, xyz_max [3] f32 (device, as in the
 * reference).  Outputs: t_min, t_max [n_rays] f32; n_steps, cumsum [n_rays] i64
 * (inclusive scan); total [1] i64 (device).  The caller reads `total` back to
 * size phase 2 -- the same device->host sync the reference performs at
 * render_utils_kernel.cu:212.
 */
int esr_sample_count(const float *rays_o, const float *rays_d, const float *xyz_min,
                     const float *xyz_max, float near_, float far_, float stepdist,
                     int64_t n_rays, float *t_min, float *t_max, int64_t *n_steps,
                     int64_t *cumsum, int64_t *total, void *stream);

/*
 * sample_pts_on_rays, phase 2 -- replaces __set_1_at_ray_seg_start + cumsum_ +
 * __set_step_id + infer_ray_start_dir + sample_pts_on_rays_cuda_kernel
 * (render_utils_kernel.cu:58-79,144-194,213-241).  Outputs have `total` rows:
 * ray_pts [total,3] f32, mask_outbbox [total] u8 (bool), ray_id, step_id [total] i64.
 */
int esr_sample_fill(const float *rays_o, const float *rays_d, const float *xyz_min,
                    const float *xyz_max, const float *t_min, const int64_t *cumsum,
                    float stepdist, int64_t n_rays, int64_t total, float *ray_pts,
                    uint8_t *mask_outbbox, int64_t *ray_id, int64_t *step_id, void *stream);

/*
 * alpha2weight -- replaces render_utils_kernel.cu:577-651.  alpha [n_pts] f32,
 * ray_id [n_pts] i64 sorted.  Writes weight, T [n_pts]; alphainv_last [n_rays];
 * i_start, i_end [n_rays] i64 -- all fully initialised here (0/1/1/0/0 defaults).
 */
int esr_alpha2weight_fwd(const float *alpha, const int64_t *ray_id, int64_t n_pts,
                         int64_t n_rays, float *weight, float *T, float *alphainv_last,
                         int64_t *i_start, int64_t *i_end, void *stream);

/* alpha2weight_backward -- replaces render_utils_kernel.cu:654-707. grad [n_pts]. */
int esr_alpha2weight_bwd(const float *alpha, const float *weight, const float *T,
                         const float *alphainv_last, const int64_t *i_start,
                         const int64_t *i_end, int64_t n_pts, int64_t n_rays,
                         const float *grad_weights, const float *grad_last, float *grad,
                         void *stream);

/*
 * total_variation_add_grad -- replaces total_variation_kernel.cu:13-35,68-98.
 * In place on grad; param/grad have n elements laid out [..., sz_i, sz_j, sz_k].
 * Keeps the reference's quirk: the i and k axes both use wz, wx is unused.
 */
int esr_tv_add_grad(const float *param, float *grad, float wx, float wy, float wz,
                    int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t n, int dense_mode,
                    void *stream);

/*
 * Sorted segment sum -- replaces torch_scatter.segment_coo(src, index, out,
 * reduce="sum") (voxurff.py:260-272).  out [n_seg,c] is accumulated into
 * (caller zero-fills); index [n] i64 non-decreasing.
 */
int esr_segment_sum(const float *src, const int64_t *index, int64_t n, int64_t c,
                    float *out, int64_t n_seg, void *stream);

/*
 * The reference's DOUBLE instantiation of its three live ops (AT_DISPATCH_FLOATING_TYPES, render_utils_kernel.cu:229,639,692;
 * nothing in the reference's Python produces double tensors, the shim dispatches on dtype like the reference does).  Same
 * contracts as the fp32 entry points with double tensors.  The reference's kernels keep `float` locals whatever the tensor
 * type: t_min / t_max, the sample points, the running transmittance and the backward's running sum are rounded to float on
 * the way (stored as doubles) -- restated literally, one thread per ray / sample (csrc/sampler.hip, composite.hip).
 */
int esr_sample_count_f64(const double *rays_o, const double *rays_d, const double *xyz_min, const double *xyz_max,
                         float near_, float far_, float stepdist, int64_t n_rays, double *t_min, double *t_max,
                         int64_t *n_steps, int64_t *cumsum, int64_t *total, void *stream);
int esr_sample_fill_f64(const double *rays_o, const double *rays_d, const double *xyz_min, const double *xyz_max,
                        const double *t_min, const int64_t *cumsum, float stepdist, int64_t n_rays, int64_t total,
                        double *ray_pts, uint8_t *mask_outbbox, int64_t *ray_id, int64_t *step_id, void *stream);
int esr_alpha2weight_fwd_f64(const double *alpha, const int64_t *ray_id, int64_t n_pts, int64_t n_rays, double *weight,
                             double *T, double *alphainv_last, int64_t *i_start, int64_t *i_end, void *stream);
int esr_alpha2weight_bwd_f64(const double *alpha, const double *weight, const double *T, const double *alphainv_last,
                             const int64_t *i_start, const int64_t *i_end, int64_t n_pts, int64_t n_rays,
                             const double *grad_weights, const double *grad_last, double *grad, void *stream);

/*
 * The ops the two pybind modules EXPORT but the reference's own Python never calls (render_utils.cpp:171-173,175-181,
 * total_variation.cpp:31).  Not on the accelerated path: one thread per ray / point / cell, the fp32
 * instantiation of the reference's templates statement by statement (csrc/legacy_ops.hip; float / double mixing where the
 * reference's literals put it).  Caller-allocated outputs; bool tensors are bytes.
 */
/* infer_t_minmax -- render_utils_kernel.cu:12-35,82-103: ray / box range clamped into [near, far] -> t_min, t_max [n_rays]. */
int esr_infer_t_minmax(const float *rays_o, const float *rays_d, const float *xyz_min, const float *xyz_max,
                       float near_, float far_, int64_t n_rays, float *t_min, float *t_max, void *stream);
/* infer_n_samples -- :38-55,105-121: max(ceil((t_max - t_min) |d| / stepdist), 1) -> int64 [n_rays]. */
int esr_infer_n_samples(const float *rays_d, const float *t_min, const float *t_max, float stepdist, int64_t n_rays,
                        int64_t *n_samples, void *stream);
/* infer_ray_start_dir -- :58-79,123-140: o + d t_min and d / |d| -> [n_rays,3] each. */
int esr_infer_ray_start_dir(const float *rays_o, const float *rays_d, const float *t_min, int64_t n_rays,
                            float *rays_start, float *rays_dir, void *stream);
/* sample_ndc_pts_on_rays -- :243-292: o + d step / (N - 1) -> rays_pts [n_rays,N,3], mask_outbbox [n_rays,N]. */
int esr_sample_ndc_pts(const float *rays_o, const float *rays_d, const float *xyz_min, const float *xyz_max,
                       int32_t n_samples, int64_t n_rays, float *rays_pts, uint8_t *mask_outbbox, void *stream);
/* sample_bg_pts_on_rays -- :294-360: inverted-sphere background points -> rays_pts [n_rays,N,3]. */
int esr_sample_bg_pts(const float *rays_o, const float *rays_d, const float *t_max, float bg_preserve, int32_t n_samples,
                      int64_t n_rays, float *rays_pts, void *stream);
/* maskcache_lookup -- :366-423: nearest voxel of a bool volume [sz_i,sz_j,sz_k]; outside reads 0 -> out [n_pts]. */
int esr_maskcache_lookup(const uint8_t *world, const float *xyz, const float *xyz2ijk_scale, const float *xyz2ijk_shift,
                         int32_t sz_i, int32_t sz_j, int32_t sz_k, int64_t n_pts, uint8_t *out, void *stream);
/* raw2alpha / raw2alpha_nonuni -- :431-502: e = exp(density + shift), alpha = 1 - (1 + e)^(-interval) -> exp_d, alpha [n_pts].
 * interval_per_point != NULL: the _nonuni form (one interval per point; `interval` is ignored). */
int esr_raw2alpha(const float *density, float shift, float interval, const float *interval_per_point, int64_t n_pts,
                  float *exp_d, float *alpha, void *stream);
/* raw2alpha_backward / raw2alpha_nonuni_backward -- :504-575: min(e, 1e10) (1 + e)^(-interval - 1) interval grad_back. */
int esr_raw2alpha_bwd(const float *exp_d, const float *grad_back, float interval, const float *interval_per_point,
                      int64_t n_pts, float *grad, void *stream);
/* total_variation_add_grad_new -- total_variation_kernel.cu:38-66,101-131: every term x mask[cell] mask[neighbour] (mask is a
 * float tensor like param); wx on the fastest axis, wy, wz on the slowest (the live kernel's wz-twice quirk is NOT in this one). */
int esr_tv_add_grad_masked(const float *param, float *grad, const float *mask, float wx, float wy, float wz,
                           int64_t sz_i, int64_t sz_j, int64_t sz_k, int64_t n, int dense_mode, void *stream);

/* ------------------------------------------------------------------------- *
 * B. Fused fine-stage path (VoxurfF.forward_training and its backward).
 * ------------------------------------------------------------------------- */

/* Scene constants, host struct passed by pointer [host] and copied by value. */
typedef struct esr_scene {
    float xyz_min[3], xyz_max[3];     /* sampler box == sdf/colour grid box          */
    float mask_min[3], mask_max[3];   /* mask-cache box                              */
    int32_t gx, gy, gz;               /* sdf / colour grid nodes [X,Y,Z]             */
    int32_t mx, my, mz;               /* mask-cache grid nodes                       */
    float near_, stepdist, voxel_size;
    float act_shift, mask_thres;      /* mask cache: 1-exp(-softplus(d+shift)) >= thres */
    float fast_thres;                 /* alpha > thres, then weight > thres          */
    float s_val;
    int32_t max_steps;                /* upper bound of per-ray step count (LDS sizing) */
    float grad_feat[4];               /* stencil radii of the 24-tap SDF feature (voxels) */
} esr_scene_t;

/*
 * Header the planner leaves in device memory (and the caller reads back once per
 * iteration to size the activation workspace).
 */
typedef struct esr_plan {
    int32_t n_on;        /* surviving samples on emissive-on rays   */
    int32_t n_off;       /* surviving samples on emissive-off rays  */
    int32_t tiles_on;    /* ceil(n_on / 32)                         */
    int32_t tiles_all;   /* tiles_on + ceil(n_off / 32)             */
    int32_t m0, m1, m2;  /* survivors after in-box / mask-cache / alpha>thres */
    int32_t overflow;    /* bit 0: a ray exceeded scene.max_steps; bit 1 (esr_fine_plan): the registered range flag of the
                            split-fp16 forward kernels is set (esr_mlp_split_range_flag) */
} esr_plan_t;

/*
 * The ray march: per ray (one wavefront each) sampler -> in-box -> mask cache -> SDF tap -> NeuS alpha -> alpha>thres ->
 * transmittance with the early stop -> weight>thres (voxurff.py:186-213, functions.py:72-105,
 * render_utils_kernel.cu:577-605), in three passes over ONE argument struct: esr_march_count (sizes), esr_fine_plan*
 * (offsets, below), esr_march_fill (records), and esr_march_bwd.  A pass reads and writes only the fields listed for it
 * (and for the variant `flags` / `cache` select); the others may stay set from another pass.  Variants:
 *  - flags 0: the fine stage, NeuS "interp" alpha (section SDFs interpolated towards the surviving neighbours).
 *  - ESR_MARCH_GRAD_ALPHA: cfg `neus_alpha: grad` (app/utils/base/functions.py:45-69): the section SDFs of a sample are
 *    sdf -+ 0.5 * dist * (viewdirs[ray] . grad).  Fine stage: grad = the radius-1 clamped central differences of
 *    sample_sdf_grad (app/fine/model/voxurff.py:670-721); the backward scatters through the value tap and the six gradient
 *    taps.
 *  - ESR_MARCH_COARSE: the coarse renderer (app/coarse/model/voxurfc.py:186-219): SDF tap of the SMOOTHED grid, NO alpha
 *    threshold (plan.m2 == plan.m1), alpha2weight over ALL mask-cache survivors -> weight > thres -> alpha2weight AGAIN
 *    over the survivors (weights, alphainv_last and cum_weights = sum of weights come from this second pass).  Same
 *    protocol and record layout.
 *  - both flags (voxurfc.py:171-174, 204-210): grad = the trilinear sample of the dense gradient grid `gg`
 *    (esr_central_grad_fwd of the UNSMOOTHED SDF grid); the backward adds d/d gg into `grad_gg`, which
 *    esr_central_grad_bwd folds into the SDF gradient.
 *  - cache != NULL (flags 0 only): the three passes share a CACHE.  The count pass records, for every mask-cache survivor
 *    of every ray, its SDF, step id, alpha, transmittance and survivor flags; the fill pass is then a plain copy of the
 *    recorded samples and the backward starts at its reverse scan -- the walk (mask-cache and SDF fetch per step) and the
 *    serial transmittance loop run once per step instead of three times.  Results are bit-identical to cache == NULL.
 *    The cached fill and backward read ray_stats (both) and alphainv_last (backward) as the count pass left them, and
 *    neither mask_density nor sdf.
 * Return: ESR_EINVAL for a NULL struct / scene, n_rays < 0, a count without plan, unknown flag bits, cache or dsdf_rec
 * together with a flag, gg or grad_gg without both flags, and (n_rays > 0) a NULL field the pass reads or writes;
 * ESR_ECAP (nothing written) for a scene.max_steps whose backward does not fit the LDS; 0 without a launch for n_rays == 0.
 */
#define ESR_MARCH_COARSE 1
#define ESR_MARCH_GRAD_ALPHA 2
typedef struct esr_march {
    const esr_scene_t *scene;                   /* [host]                                                            */
    const float *rays_o, *rays_d;               /* [n_rays,3]                                                        */
    const float *viewdirs;                      /* [n_rays,3] the batch's view directions; read only with
                                                   ESR_MARCH_GRAD_ALPHA                                              */
    const float *mask_density;                  /* [mx,my,mz] (max-pooled)                                           */
    const float *sdf;                           /* [gx,gy,gz]; ESR_MARCH_COARSE: the SMOOTHED grid                   */
    const float *gg;                            /* both flags: gradient grid [gx,gy,gz,3], else NULL                 */
    int32_t n_rays;
    int32_t flags;                              /* ESR_MARCH_COARSE | ESR_MARCH_GRAD_ALPHA                           */
    /* count writes (cached fill / backward read ray_stats, cached backward alphainv_last) */
    int32_t *cnt3;                              /* [n_rays] survivors of the ray                                     */
    float *alphainv_last;                       /* [n_rays]                                                          */
    float *cum_weights;                         /* [n_rays], ESR_MARCH_COARSE only (white_bg = 1 - cum_weights)      */
    int32_t *ray_stats;                         /* [n_rays,3] in-box / mask-cache / alpha>thres survivors of the ray;
                                                   esr_fine_plan sums them into m0/m1/m2                             */
    esr_plan_t *plan;                           /* count sets plan->overflow (zeroed by esr_fine_plan_begin)         */
    /* fill and backward read; fill writes one record per surviving sample at off3[ray] + rank */
    const int32_t *off3;                        /* [n_rays] (esr_fine_plan)                                          */
    int32_t *rec_ray, *rec_step;                /* [n_tiles*32]; padding entries must have been set to rec_ray = -1
                                                   by the caller                                                     */
    float *rec_w, *rec_sdf;                     /* [n_tiles*32]                                                      */
    /* backward */
    const float *dweight;                       /* [n_tiles*32] d(weights), indexed like the records                 */
    const float *dlast;                         /* [n_rays] d(alphainv_last)                                         */
    float *grad_sdf;                            /* [gx,gy,gz] atomic scatter through the compositing scan, the alpha
                                                   formula and the trilinear tap(s); ESR_MARCH_COARSE: of the SMOOTHED
                                                   grid                                                              */
    float *grad_gg;                             /* both flags: [gx,gy,gz,3], added to (zero-initialised or already
                                                   holding the normal features' share), else NULL                    */
    float *dsdf_rec;                            /* optional, flags 0: the value-tap gradient of every RECORDED sample
                                                   (the ones esr_march_fill wrote) goes to dsdf_rec [n_tiles*32]
                                                   (indexed like the records) instead of being scattered: pass that
                                                   array as `dsdf_extra` to esr_fine_feat_bwd, which folds it into the
                                                   SDF window it builds anyway (no L2 atomics for it).  Samples that
                                                   were walked but not recorded (below a threshold, yet neighbours of a
                                                   recorded one) are still scattered into grad_sdf                   */
    int32_t accumulate;                         /* 0: every recorded slot of dsdf_rec is overwritten (padding slots are
                                                   left alone; the feature backward never reads them); 1: added to
                                                   what the caller put there                                         */
    float *cache;                               /* NULL or esr_fine_march_cache_floats(scene, n_rays) floats         */
} esr_march_t;
int64_t esr_fine_march_cache_floats(const esr_scene_t *scene, int32_t n_rays);
int esr_march_count(const esr_march_t *a, void *stream);
int esr_march_fill(const esr_march_t *a, void *stream);
int esr_march_bwd(const esr_march_t *a, void *stream);

int esr_fine_plan_begin(esr_plan_t *plan, void *stream);

/*
 * plan: exclusive offsets of every ray's survivors in the compact sample list.
 * Emissive-on rays (em_modes==1) first, then -- starting at the next multiple of
 * 32 -- the off rays, both in ray order, so every 32-sample tile is on-only or
 * off-only.  off3 [n_rays] i32; *plan (device) gets the totals.
 */
int esr_fine_plan(const int32_t *cnt3, const int64_t *em_modes, const int32_t *ray_stats,
                  int32_t n_rays, int32_t *off3, esr_plan_t *plan, void *stream);
/*
 * The same in two launches, for a caller that reads the header back: _totals leaves n_on, n_off, m0, m1, m2 and the overflow
 * word in the header (many workgroups; tiles_on / tiles_all are NOT written: ceil(n_on / 32), tiles_on + ceil(n_off / 32)),
 * _offsets computes off3 (and writes all four counts).  Copy the header between the two: the one-workgroup scan of _offsets
 * then runs while the host reads it.  Header zeroed by esr_fine_plan_begin as for esr_fine_plan.
 */
int esr_fine_plan_totals(const int32_t *cnt3, const int64_t *em_modes, const int32_t *ray_stats, int32_t n_rays,
                         esr_plan_t *plan, void *stream);
int esr_fine_plan_offsets(const int32_t *cnt3, const int64_t *em_modes, int32_t n_rays, int32_t *off3, esr_plan_t *plan,
                          void *stream);

/*
 * Per-sample feature assembly (voxurff.py:219-254 + :678-721 + module.py:24-35; the LTS renderer's
 * esrnerf.py:728-765 uses the same features with three colour grids).
 * Colour grids are channel-last [gx,gy,gz,6] (torch.channels_last_3d storage of the reference's
 * [1,6,X,Y,Z] parameter).  X [n_tiles,104,32] f32, rows:
 *   0-5 colour group 0 | 6 sdf | 7-30 feat24 | 31-42 normal12 | 43-45 xyz | 46-60 sin | 61-75 cos
 *   | 76-84 viewdir PE | 85-87 zero | 88-93 colour group 1 | 94-95 zero | 96-101 colour group 2 | zero
 * gnorm [n_tiles,4,32]: |grad| per stencil radius, kept for the backward.
 */
typedef struct esr_feat_args {
    /* sample positions: either the march records ... */
    const float *rays_o, *rays_d, *viewdirs;        /* [N,3] each; viewdirs per RAY                 */
    const int32_t *rec_ray, *rec_step;              /* [tiles*32]                                   */
    const float *rec_sdf;
    /* ... or explicit points (pts != NULL): per-sample arrays, n_pts valid samples, the rest padding */
    const float *pts, *pt_viewdirs, *pt_sdf;        /* [n_pts,3] [n_pts,3] [n_pts]                  */
    int32_t n_pts;
    const float *sdf;                               /* SDF grid [gx,gy,gz]                          */
    /* grid feeding colour group g on emissive-on tiles / on the other tiles (NULL: zeros).
       fine stage: group0 = {emo, off}, group1 = {off, NULL}; LTS stage: {off,off} {emo,emo} {brdf,brdf} */
    const float *color_on[3], *color_off[3];
    int32_t tiles_on, tiles_all;
} esr_feat_args_t;

int esr_fine_feat_fwd(const esr_scene_t *scene, const esr_feat_args_t *args, float *X, float *gnorm,
                      void *stream);
/*
 * The bf16 engine's form: the input tile goes to X16 as bf16 in the row-quad layout of that engine's saved tiles
 * (esr_fine_feat_x16_bytes(n_tiles) bytes: 26 quads of 256 B per tile = rows 0..95 + the first eight rows once more with
 * the colour group of rows 88..93 in rows 0..5) -- the fp32 rows rounded to bf16, i.e. what the bf16 kernels made of
 * them on load.  X still receives the normal rows 31..42 (the backward reads them), nothing else.  Consumers:
 * esr_mlp_fwd_fine_bf16 (X16 argument; then X may be NULL) and esr_wgrad_job_t::X16.  Stencil radii outside [0, 2] voxels:
 * ESR_ECAP (use esr_fine_feat_fwd).
 */
int64_t esr_fine_feat_x16_bytes(int32_t n_tiles);
int esr_fine_feat_fwd_x16(const esr_scene_t *scene, const esr_feat_args_t *args, float *X, float *gnorm, void *X16,
                          void *stream);

/*
 * Backward.  Every net that consumed the tiles contributes a dX [n_tiles,64,32] (rows 0-42 used)
 * over its tile range: rows 6-42 (sdf value, stencil features, normals) are summed over the sources,
 * rows 0-5 go to that source's colour grid.  dsdf_extra [tiles*32] (optional) is added to the
 * SDF-value row.  With explicit points the SDF-value gradient is returned in dsdf_out [tiles*32]
 * instead of being scattered.  grad_sdf NULL: the SDF grid is frozen, only the colour grids receive
 * gradients (re-lighting fine-tune).  Scatter = LDS accumulation window + z-contiguous float atomics.
 * grad4 [tiles*32][4] (optional; needs grad_sdf): per sample the gradient w.r.t. esr_expgrad_fwd's four outputs at the
 * SAME position (value, d sdf / d x, y, z) -- scattered with esr_expgrad_bwd's weights inside this launch.  grad4_mode:
 * bit 0 = out-of-grid corners dropped (esr_expgrad_bwd's zero_pad) instead of border-replicated; bit 1 = explicit points:
 * the SDF-value gradient (what dsdf_out receives) is scattered the same way, as the value component.
 * The SDF scatter is built for stencil radii (scene->grad_feat) in [0, 2] voxels, the reference's configuration
 * (fine.yaml: [0.5, 1.0, 1.5, 2.0]); other radii return ESR_ECAP (esr_fine_feat_fwd takes any radius).
 */
typedef struct esr_feat_bwd_src {
    const float *dX;
    float *grad_color_on, *grad_color_off;          /* colour grid gradient on on-tiles / other tiles (NULL: none) */
    int32_t t0, t1;
} esr_feat_bwd_src_t;

int esr_fine_feat_bwd(const esr_scene_t *scene, const esr_feat_args_t *args, const float *X,
                      const float *gnorm, const esr_feat_bwd_src_t *src, int32_t n_src,
                      const float *dsdf_extra, float *grad_sdf, float *dsdf_out, const float *grad4,
                      int32_t grad4_mode, void *stream);

/*
 * Tiny-MLP engine (RadianceNet 85-192-192-192-3, TonemapNet 33-192-3;
 * app/utils/pbr/module.py:6-39) on f32 MFMA.  `kind`: 0 radiance, 1 tonemap.
 * Weights are the reference's nn.Linear tensors ([out,in] row-major) packed by
 * esr_mlp_pack into MFMA operand order.
 */
#define ESR_MLP_RADIANCE 0   /* 85-192-192-192-3, softplus applied by the caller kernels   */
#define ESR_MLP_TONEMAP  1   /* 33-192-3                                                  */
#define ESR_MLP_BRDF     2   /* BRDFNet 76-128-128-128-5 (app/utils/pbr/module.py:42-65)  */
#define ESR_MLP_EMIT     3   /* EmissionNet 76-128-128-128-3 (app/utils/pbr/module.py:68-83) */
#define ESR_MLP_COARSE   4   /* coarse rgbnet 57-128-128-3 (app/coarse/model/voxurfc.py:134-149), 72-row input tile */
#define ESR_MLP_MAX_LAYERS 4

typedef struct esr_mlp_weights {       /* [host] struct of device pointers */
    const float *w[ESR_MLP_MAX_LAYERS];   /* [out,in] */
    const float *b[ESR_MLP_MAX_LAYERS];   /* [out]    */
} esr_mlp_weights_t;

int64_t esr_mlp_packed_floats(int kind);     /* size of the packed buffer */
int esr_mlp_pack(int kind, const esr_mlp_weights_t *w, float *packed, void *stream);
/* Every net of a step in ONE launch (n <= 8): packed32[i] <- w[i] for net kinds[i]; where packed16 != NULL and
 * packed16[i] != NULL also its bf16 twin (esr_mlp_pack_bf16).  The reference has no counterpart: its nn.Linear
 * weights are used as they are (app/utils/pbr/module.py:6-83). */
int esr_mlp_pack_batch(int n, const int32_t *kinds, const esr_mlp_weights_t *const *w, float *const *packed32,
                       void *const *packed16, void *const *packed_split, void *stream);
/*
 * Round 4: the f32 engine's MLP FORWARD on the 16-bit matrix cores with fp32 results (csrc/mlp_split.hip): every operand as
 * two fp16 planes x = x1 + x2 (x1 = fp16(x), x2 = fp16(x - x1); the weights' planes hold 64 w), a product as
 * w1.x1 + w1.x2 + w2.x1 on v_mfma_f32_32x32x16_f16 into one fp32 accumulator -- fp32-level accuracy (2e-7 .. 6e-7 of a layer's
 * largest value against double precision, as the f32 MFMA kernels) at 16/3 of the f32 matrix rate.  packed_split[i] of
 * esr_mlp_pack_batch (or NULL) receives the net's forward and transposed weights as split planes,
 * esr_mlp_packed_split_elems(kind) fp16 values.  esr_mlp_fwd_split / esr_mlp_fwd_fine_split keep the contracts of
 * esr_mlp_fwd / esr_mlp_fwd_fine (inputs X, saved tiles H and masks M, outputs z are the f32 engine's, so the f32
 * input-gradient and weight-gradient entries follow unchanged).  Kinds: ESR_MLP_RADIANCE, _TONEMAP, _BRDF, _EMIT (the coarse
 * net: ESR_EINVAL).  The reference evaluates these layers with fp32 nn.Linear (app/utils/pbr/module.py:6-83).
 */
int64_t esr_mlp_packed_split_elems(int kind);
/* fp16-element offset, inside a net's planes buffer, of its gradient gain bound G (one fp32; see esr_mlp_split_range_flag) */
int64_t esr_mlp_split_gain_offset(int kind);
/* The split kernels' range: a first plane is fp16, so an input, a hidden activation or 64 x a weight beyond 65504 would become
 * inf.  flag (device uint32, owned by the caller, sticky; NULL unregisters) is registered for the CURRENT device and ORed with 1
 * by every later (a) esr_mlp_fwd_split / esr_mlp_fwd_fine_split launch on it when an input or a hidden activation reaches
 * 60000 (or is inf; a +NaN activation) -- the output layer's results are fp32 sums that never become planes --, (b)
 * esr_mlp_pack_batch launch when fp16(64 w) of a weight is not finite (|w| >= 1023.5), or when the net's gradient gain bound
 * (below) exceeds 2^18.  The BACKWARD needs no flag: esr_mlp_pack_batch writes, behind a net's planes, the bound
 * G = max over the hidden layers of the running product of the layers' largest column sums of |W| (and 1): no hidden
 * gradient of a tile can exceed G max |dz|; esr_mlp_dgrad_split scales each tile so that G max |dz| is in [2^14, 2^15), and its
 * `amax` output (the weight-gradient kernels' scale source) is max |dz| x max(1, G / 16).  The host side
 * (esr_nerf_amd/fine_engine.py: range_probe / range_hit / f32_only) reads the flag behind the forward of every step and
 * re-runs a step that raised it on the f32 MFMA entry points, which share every buffer format.  esr_fine_plan also copies the
 * flag into bit 1 of the plan header's overflow word (informational). */
int esr_mlp_split_range_flag(uint32_t *flag);
int esr_mlp_fwd_split(int kind, const float *packed32, const void *planes, const float *X, int32_t t0, int32_t t1,
                      float *const *H, uint32_t *const *M, int save, int color_row0, float *zout, void *stream);
int esr_mlp_fwd_fine_split(const float *packed32_off, const void *planes_off, const float *packed32_emo,
                           const void *planes_emo, const float *X, int32_t t_on, int32_t t_all, float *const *H,
                           uint32_t *const *M, int color_row_detached, float *z_off, float *z_emo, void *stream);
/* The input-gradient chain the same way (contracts of esr_mlp_dgrad / esr_mlp_dgrad_fine; the same four kinds): the split
 * buffer also holds the TRANSPOSED weights' planes.  Gradients are far below fp16's normal range, so each 32-sample tile's
 * chain runs scaled by a power of two chosen from its largest |dz| (exact), and dZ / dX are written unscaled in fp32. */
/* amax (optional, device, one float, >= 0 on entry -- normally zero): raised, with an atomic maximum, to the largest |dz| of the
 * launch's tiles x max(1, G / 16) (G: the net's gain bound, above) -- a value B with |dz| <= B and every hidden |dZ| <= 16 B;
 * esr_wgrad_job_t::amax and esr_tone_wgrad_recompute_split read it (their planes hold >= 32 B). */
int esr_mlp_dgrad_split(int kind, const void *planes, const float *dz, int32_t t0, int32_t t1, const uint32_t *const *M,
                        float *const *dZ, float *dX, float *amax, void *stream);
int esr_mlp_dgrad_fine_split(const void *planes_emo, const void *planes_off, const float *dz, int32_t t_on, int32_t t_all,
                             const uint32_t *const *M, float *const *dZ, float *dX, float *amax, void *stream);
/* out[0] = max(out[0], max |x[i]|, i < n) (device; out >= 0 on entry).  As a scale source of the split weight-gradient
 * kernels it is safe only where the caller knows its hidden gradients stay below 32 x that value (tests). */
int esr_absmax(const float *x, int64_t n, float *out, void *stream);

/*
 * Forward over tiles [t0,t1).  X: layer-1 input, tile-major [tiles,xrows,32].
 * With save != 0 every hidden layer l keeps H[l] [tiles,192,32] (read by the weight
 * gradient) and its ReLU sign bits M[l] [tiles,3,64] u32 (read by the input gradient:
 * 768 B per tile instead of 24 KB).  zout [tiles,4,32]: pre-activation outputs
 * (row 3 = 0; [tiles,8,32] for the 5-output BRDF net).  Hidden tiles are [tiles,128,32]
 * and masks [tiles,2,64] for the 128-wide nets.  color_row0 (0, 88 or 96) selects which
 * 6-row colour group of the X tile feeds the first 6 inputs.  save == 2 keeps the masks M only (for a net
 * whose weight gradient recomputes its hidden layer: esr_tone_wgrad_recompute); H may then be NULL.
 * M[l] is [tile][word wd][lane]: bit b of word wd in lane s + 32 h is feature 32 (2 wd + (b >> 4)) + acc_row(b & 15, h)
 * of sample s, with acc_row(r, h) = (r & 3) + 8 (r >> 2) + 4 h.
 */
int esr_mlp_fwd(int kind, const float *packed, const float *X, int32_t t0, int32_t t1,
                float *const *H, uint32_t *const *M, int save, int color_row0, float *zout,
                void *stream);
/*
 * The same net over two adjacent tile ranges in ONE launch: [t0,t_mid) detached (nothing saved, colour
 * rows color_row_detached), [t_mid,t1) saved with colour rows 0.  This is the fine stage's off-net
 * (app/fine/model/voxurff.py:244-254: `.detach()` on the emissive-on rays, differentiable on the off
 * rays); RadianceNet only.
 */
int esr_mlp_fwd_mixed(int kind, const float *packed, const float *X, int32_t t0, int32_t t_mid, int32_t t1,
                      float *const *H, uint32_t *const *M, int color_row_detached, float *zout, void *stream);

/*
 * The fine stage's three radiance passes of one step in ONE launch (app/fine/model/voxurff.py:243-256): the non-emissive
 * net on tiles [0,t_on) detached (colour rows color_row_detached, nothing saved) and on [t_on,t_all) saved with colour
 * rows 0, the emissive net on [0,t_on) saved with colour rows 0.  Both nets save into the same H / M arrays (disjoint
 * tiles); z_off [t_all,4,32], z_emo [t_on,4,32].  One ramp-up and one tail instead of two launches' worth.
 */
int esr_mlp_fwd_fine(const float *packed_off, const float *packed_emo, const float *X, int32_t t_on, int32_t t_all,
                     float *const *H, uint32_t *const *M, int color_row_detached, float *z_off, float *z_emo,
                     void *stream);
/* Its backward twin: input gradients of the emissive net on tiles [0,t_on) and of the non-emissive net on
 * [t_on,t_all) in one launch (the non-emissive net's on-tile pass is detached in the reference: no gradient). */
int esr_mlp_dgrad_fine(const float *packed_emo, const float *packed_off, const float *dz, int32_t t_on, int32_t t_all,
                       const uint32_t *const *M, float *const *dZ, float *dX, void *stream);
/* The bf16 engine's twins of the two entries above (weights of both nets as packed by esr_mlp_pack / esr_mlp_pack_bf16). */
int esr_mlp_fwd_fine_bf16(const float *packed32_off, const void *packed16_off, const float *packed32_emo,
                          const void *packed16_emo, const float *X, const void *X16, int32_t t_on, int32_t t_all,
                          float *const *H, uint32_t *const *M, int color_row_detached, float *z_off, float *z_emo,
                          void *stream);
int esr_mlp_dgrad_fine_bf16(const void *packed16_emo, const void *packed16_off, const float *dz, int32_t t_on, int32_t t_all,
                            const uint32_t *const *M, float *const *dZ, float *dX, void *stream);

/*
 * Input/hidden gradients over tiles [t0,t1) (a NULL dZ[l] is computed but not stored).  dz [tiles,4,32] -> dZ[l] (each
 * [tiles,192,32], pre-activation grads of hidden layer l) and dX [tiles,64,32], of which the rows that lead back to a
 * grid are written, rounded up to 4: rows 0-43 for the sample nets (colour | sdf | 24 stencil taps | 12 normal
 * components = rows 0-42; the position / view-direction encodings are inputs without a gradient in the reference too),
 * rows 0-35 for the tone mapper (33 inputs), rows 0-31 for the coarse net.  The other rows are left untouched.
 */
int esr_mlp_dgrad(int kind, const float *packed, const float *dz, int32_t t0, int32_t t1,
                  const uint32_t *const *M, float *const *dZ, float *dX, void *stream);

/*
 * Weight/bias gradients accumulated into the reference-layout tensors gw[l] [out,in],
 * gb[l] [out] over tiles [t0,t1).  scratch: >= esr_mlp_wgrad_scratch_floats() floats of
 * device workspace for the per-workgroup partial slabs (summed by a second kernel).
 */
int64_t esr_mlp_wgrad_scratch_floats(void);
int esr_mlp_wgrad(int kind, const float *X, int color_row0, const float *const *H,
                  const float *const *dZ, const float *dz, int32_t t0, int32_t t1,
                  float *const *gw, float *const *gb, float *scratch, int64_t scratch_floats,
                  void *stream);

/*
 * Weight gradients of SEVERAL nets / tile ranges in one call.  Layers of the same kernel shape share a launch (the
 * same layer of the emissive and the non-emissive RadianceNet, both hidden layers, the 3-row output layers of all
 * nets): a weight-gradient launch has a fixed cost of ~30 us whatever its tile count, and with J jobs per launch the
 * per-workgroup partial sums that have to be exchanged shrink J-fold.  Results are those of one esr_mlp_wgrad (or
 * esr_mlp_wgrad_bf16 with bf16_operands != 0) per job.  H, dZ, gw, gb are [host] arrays of device pointers.
 */
typedef struct esr_wgrad_job {
    int32_t kind, color_row0, t0, t1;
    const float *X;
    const float *const *H;
    const float *const *dZ;
    const float *dz;
    float *const *gw;
    float *const *gb;
    /* optional (bf16 operands, ESR_MLP_RADIANCE, color_row0 == 0): the net's input tile as written by
     * esr_fine_feat_fwd_x16 -- the first-layer job then stages it like a hidden layer's tile and X is not read. */
    const void *X16;
    /* optional (f32 operands; every net kind and layer shape): device pointer to the scale source B left by
     * esr_mlp_dgrad_split / esr_mlp_dgrad_fine_split (|dz| <= B, hidden |dZ| <= 16 B; the planes hold 128 B).  Non-NULL
     * selects the split-fp16 weight-gradient kernel:
     * the same fp32 operands, every value cut into two fp16 planes on its way into the 16-bit matrix cores, fp32
     * accumulation; the gradient operand is scaled by a power of two derived from *amax (csrc/mlp.hip, SPLIT). */
    const float *amax;
} esr_wgrad_job_t;
int esr_mlp_wgrad_batch(const esr_wgrad_job_t *jobs, int32_t n_jobs, int bf16_operands, float *scratch,
                        int64_t scratch_floats, void *stream);

/*
 * Weight gradients of the tone mapper (TonemapNet 33-192-3, app/utils/pbr/module.py:24-39) from its INPUTS only:
 * Xt [tiles,48,32] (the tile esr_fine_tone_in_fwd writes) and dzt [tiles,4,32] (d loss / d pre-sigmoid output).  The
 * hidden layer is recomputed inside the kernel, so the forward need not save Ht (esr_mlp_fwd with save = 2) and the
 * input-gradient pass need not store dZt (esr_mlp_dgrad with dZ[0] = NULL): 48 KB of tile traffic per 32 samples
 * less than esr_mlp_wgrad(ESR_MLP_TONEMAP).  W0 [192,33], b0 [192], W1 [3,192]: the net's parameters in the
 * reference layout; gw0 / gb0 / gw1 / gb1 receive += the gradients.  fp32.
 */
int64_t esr_tone_wgrad_scratch_floats(void);
int esr_tone_wgrad_recompute(const float *Xt, const float *dzt, const float *W0, const float *b0, const float *W1,
                             int32_t t0, int32_t t1, float *gw0, float *gb0, float *gw1, float *gb1,
                             float *scratch, int64_t scratch_floats, void *stream);
/* The same with bf16 matrix operands (fp32 accumulation): Xt, dzt and the weights stay fp32 in memory and are rounded
 * where the bf16 engine rounds them, so neither Ht nor dZt of the tone mapper is saved by the bf16 step either. */
int esr_tone_wgrad_recompute_bf16(const float *Xt, const float *dzt, const float *W0, const float *b0, const float *W1,
                                  int32_t t0, int32_t t1, float *gw0, float *gb0, float *gw1, float *gb1,
                                  float *scratch, int64_t scratch_floats, void *stream);
/* The same with the products on the 16-bit matrix cores from split fp16 planes, fp32 results (round 4; csrc/tone_wgrad.hip):
 * amax = device pointer to esr_mlp_dgrad_split's scale source of the tone mapper's pass (|dzt| <= B, |dZt| <= 16 B). */
int esr_tone_wgrad_recompute_split(const float *Xt, const float *dzt, const float *W0, const float *b0, const float *W1,
                                   const float *amax, int32_t t0, int32_t t1, float *gw0, float *gb0, float *gw1,
                                   float *gb1, float *scratch, int64_t scratch_floats, void *stream);

/*
 * bf16 variants of the MLP engine for BASELINE.json's bf16 configurations (a build-side precision choice:
 * the reference is fp32 everywhere): bf16 MFMA OPERANDS (v_mfma_f32_32x32x16_bf16), fp32 accumulation;
 * weights are rounded by esr_mlp_pack_bf16, activations when they become an operand; biases are read from
 * the esr_mlp_pack buffer.  The tiles saved for the backward -- H[l] and dZ[l] -- are bf16, hid * 32 values per tile
 * (half the bytes of the fp32 engine's) in an engine-private order: [row / 4][32 sample slots][4 rows], sample s in
 * slot 8 ((s >> 1) & 3) + 2 (s >> 3) + (s & 1) -- written 8 bytes per lane, read back only by esr_mlp_wgrad_bf16;
 * X, zout, dz, dX and the weight / bias gradients are fp32 with the layouts above, so the
 * feature / shading kernels are shared.  packed16: esr_mlp_packed_bf16_elems(kind) bf16 values.
 *
 * What is rounded, and where (round to nearest, ties to even; tests/mlp_bf16_ref64.py restates exactly this):
 *   forward          X on load (an X16 tile is that rounding, done by its writer), W by esr_mlp_pack_bf16; pre[l] = W16 h16 + b with
 *                    exact products, fp32 sums and the fp32 bias; h[l] = relu(pre[l]) is rounded ONCE, and that bf16 value is the
 *                    next layer's operand, the saved H[l] and the source of the mask bit (bit = stored H > 0 = pre > 0: a normal
 *                    fp32 does not round to zero).  zout is the fp32 sum, not rounded.
 *   input gradients  dz on load, W^T as packed; dZ[l] = mask (.) (fp32 sum) is rounded once: the stored tile and the next
 *                    operand.  dX is the fp32 sum.  These kernels write the WHOLE [64][32] tile of dX: rows 0-63 with a
 *                    reference column carry the gradient (the position / view encodings of rows 43-63 included), rows without
 *                    one are exactly 0 -- unlike esr_mlp_dgrad, which leaves the rows above its documented count untouched.
 *   weight gradients X and dz are rounded on staging, H / dZ / X16 tiles are used as stored; products exact, fp32 sums.
 *                    gb[last] sums the UNROUNDED dz, a hidden layer's gb the stored bf16 dZ.
 *   tone recompute   esr_tone_wgrad_recompute_bf16 rounds Xt (all 33 rows), W0, dzt and W1 for Ht = relu(W0 Xt + b0) and
 *                    dZt = mask (.) (W1^T dzt), both fp32 sums; dW0's columns 0-31 take r(dZt) and r(Xt) on the matrix cores;
 *                    dW0's column 32 (the 33rd input), db0, dW1 (= dzt Ht^T) and db1 are fp32 sums of the UNROUNDED
 *                    dZt, Xt row 32, dzt and Ht on the vector lanes.
 * The masks M are the [tile][word][lane] u32 arrays of esr_mlp_fwd with the same lane halves, but the bits of a word are in
 * this engine's own order: feature 32 it + acc_row(r, h) of sample s is bit 8 (it & 1) + (r >> 1) + 16 (r & 1) of word it / 2
 * in lane s + 32 h (the forward builds the word from packed bf16 pairs).  Masks written by esr_mlp_fwd_bf16 /
 * esr_mlp_fwd_fine_bf16 are therefore read by esr_mlp_dgrad_bf16 / esr_mlp_dgrad_fine_bf16 only, and vice versa.
 */
int64_t esr_mlp_packed_bf16_elems(int kind);
int esr_mlp_pack_bf16(int kind, const esr_mlp_weights_t *w, void *packed16, void *stream);
int esr_mlp_fwd_bf16(int kind, const float *packed32, const void *packed16, const float *X, int32_t t0,
                     int32_t t1, float *const *H, uint32_t *const *M, int save, int color_row0,
                     float *zout, void *stream);
int esr_mlp_dgrad_bf16(int kind, const void *packed16, const float *dz, int32_t t0, int32_t t1,
                       const uint32_t *const *M, float *const *dZ, float *dX, void *stream);
int esr_mlp_wgrad_bf16(int kind, const float *X, int color_row0, const float *const *H,
                       const float *const *dZ, const float *dz, int32_t t0, int32_t t1,
                       float *const *gw, float *const *gb, float *scratch, int64_t scratch_floats,
                       void *stream);

/*
 * Between the nets: lin = softplus(z_off) (+ softplus(z_emo) on on-tiles);
 * Xt [tiles,48,32] = [lin3 | sin15 | cos15 | 0...] (voxurff.py:783-788).
 */
int esr_fine_tone_in_fwd(const float *z_off, const float *z_emo, int32_t tiles_on,
                         int32_t tiles_all, float *lin, float *Xt, void *stream);

/*
 * rgb = sigmoid(zt); srgb_marched[ray] += w*rgb; lin_marched[ray] += w*lin
 * (segmented wave reduction + one atomic per ray segment; voxurff.py:258-272).
 * rgb [tiles,4,32] kept for the backward.  Outputs [n_rays,3] are accumulated
 * into (caller zero-fills).
 */
int esr_fine_composite_fwd(const float *zt, const float *lin, const int32_t *rec_ray,
                           const float *rec_w, int32_t tiles_all, float *rgb,
                           float *srgb_marched, float *lin_marched, void *stream);

/* d(srgb_marched), d(lin_marched) [n_rays,3] -> dweight [tiles*32], dzt [tiles,4,32]. */
int esr_fine_composite_bwd(const float *g_srgb, const float *g_lin, const float *rgb,
                           const float *lin, const int32_t *rec_ray, const float *rec_w,
                           int32_t tiles_all, float *dweight, float *dzt, void *stream);

/*
 * dXt [tiles,64,32] (tonemap input grads) + g_lin -> dz [tiles,4,32] (grad of the
 * radiance pre-activations: emo net on on-tiles, off net on off-tiles).  Xt [tiles,48,32]: the tile
 * esr_fine_tone_in_fwd wrote (its sin / cos rows are the factors of the encoding's derivative).
 */
int esr_fine_tone_in_bwd(const float *dXt, const float *Xt, const float *g_lin, const float *lin,
                         const float *z_off, const float *z_emo, const int32_t *rec_ray,
                         const float *rec_w, int32_t tiles_on, int32_t tiles_all, float *dz,
                         void *stream);
/*
 * esr_mlp_dgrad_split(ESR_MLP_TONEMAP, ..., dZ = {NULL}) over tiles [0, tiles_all) and esr_fine_tone_in_bwd as ONE launch: the
 * input-gradient kernel ends each tile with the contraction instead of storing dXt, which is never in memory.  planes: the tone
 * mapper's split planes; dzt [tiles,4,32], Mt: its output gradients and ReLU mask words; the remaining arguments and dz as
 * esr_fine_tone_in_bwd; amax as esr_mlp_dgrad_split (max |dzt| x the gain factor, for the tone mapper's weight gradients).
 */
int esr_fine_tone_dgrad_split(const void *planes, const float *dzt, const uint32_t *Mt, const float *Xt, const float *g_lin,
                              const float *z_off, const float *z_emo, const int32_t *rec_ray, const float *rec_w,
                              int32_t tiles_on, int32_t tiles_all, float *dz, float *amax, void *stream);

/*
 * Trainer-step loss of the fine stage (app/fine/fine.py:355-382) and its
 * gradient w.r.t. the three renderer outputs, one launch.  loss [1] f32 is
 * accumulated into (caller zero-fills).  Every term (loss and gradients) is
 * multiplied by `scale`: 1, or a rank's share n_local / n_global of a
 * data-parallel batch, whose mean-reduced terms are means over the GLOBAL
 * batch (no reference counterpart).
 */
int esr_fine_loss_fwd_bwd_dp(const float *srgb_marched, const float *lin_marched,
                             const float *alphainv_last, const float *rgbs, int32_t n_rays,
                             float white_bg, float weight_linear, float weight_entropy_last, float scale,
                             float *loss, float *g_srgb, float *g_lin, float *g_last,
                             void *stream);

/*
 * One mean-reduced two-operand term of the LTS / PDRA trainer losses and its gradients
 * (app/fine/lts.py:362-379: MSE(off, off_hat), MSE(emo, emo_hat), L1(normal, normal_eps);
 * app/fine/pdra.py:408-457: the L1 variants with separate weights for the two sides, the
 * emission suppression mean(emit_cert^2), L1(emit, emit_eps)).
 *   kind 0: mean((a-b)^2), kind 1: mean(|a-b|) over the elements of the rows with
 *   row_mask[row] == mask_value (row_mask NULL: all rows); b NULL stands for zeros.
 *   count_dev (device, optional): number of selected rows, so that a data-dependent
 *   selection (emit_cert = emit_marched[~uncert]) needs no host sync; 0 rows -> term 0.
 * loss[0] += w_value * term;  ga = w_a * d(term)/d(a);  gb = w_b * d(term)/d(b)  (NULL: skip).
 */
int esr_pair_loss_fwd_bwd(const float *a, const float *b, int64_t rows, int32_t cols,
                          const uint8_t *row_mask, int mask_value, const int32_t *count_dev,
                          int kind, float w_value, float w_a, float w_b, float *loss, float *ga,
                          float *gb, void *stream);

/* ------------------------------------------------------------------------- *
 * C. Light-transport-segment (LTS / PDRA) stage ops
 *    (ESRNeRF.forward_training, app/fine/model/esrnerf.py:486-851).
 * ------------------------------------------------------------------------- */

/*
 * Exact spatial gradient of the trilinear SDF interpolant -- replaces sample_sdf_expgrad
 * (esrnerf.py:1572-1596: autograd through differentiable_grid_sample,
 * app/utils/base/functions.py:142-309) by its closed form.  Points are either the
 * march records (rec_ray/rec_step, pts == NULL; padding records give zeros) or explicit
 * pts [n,3]; optional noise [n,3] * eps is added (the *_eps re-evaluations,
 * esrnerf.py:807-810).  out [n,4] = (sdf, d/dx, d/dy, d/dz) in WORLD xyz order.
 * zero_pad != 0: corners outside the grid contribute zero instead of being border-replicated
 * (F.grid_sample semantics of sample_sdf_grad, used for the perturbed emit/brdf evaluation).
 */
int esr_expgrad_fwd(const esr_scene_t *scene, const float *rays_o, const float *rays_d,
                    const int32_t *rec_ray, const int32_t *rec_step, const float *pts,
                    const float *noise, float eps, const float *sdf, int32_t n, int zero_pad,
                    float *out, void *stream);
/* g [n,4] -> atomic scatter into grad_sdf [gx,gy,gz] (the op is linear in the grid). */
int esr_expgrad_bwd(const esr_scene_t *scene, const float *rays_o, const float *rays_d,
                    const int32_t *rec_ray, const int32_t *rec_step, const float *pts,
                    const float *noise, float eps, const float *g, int32_t n, int zero_pad,
                    float *grad_sdf, void *stream);

/*
 * The light-transport step's glue (esrnerf.py:781-830: reference-order bookkeeping, surface-point gathers, perturbed
 * positions), fused: four launches for what are ~60 small torch ops in the reference.
 *   esr_lts_ref_order: perm[pos] = j for every compact slot j with rec_ray[j] >= 0, pos = its rank in the reference's
 *       ray-sorted sample order (cnt3_cumsum = inclusive int64 cumsum of cnt3); ray64[j] = (int64) rec_ray[j].
 *   esr_lts_perturb:   pts_e[k] = pts_all[perm[k]] + noise_emit[k] * emit_eps,  noise_n[perm[k]] = noise_normal[k]
 *       (noise_n [n_slots,3] zeroed by the caller).
 *   esr_lts_gather_rows: out[k][c] = src(row perm[k] -- or k when perm is NULL --, column col0 + c); src tile-major
 *       [tiles][tile_rows][32] when tile_rows > 0, else row-major with row_stride floats per row.
 *   esr_lts_gather_points: per surface point (compact slot jp[p]) position / view direction / SDF (each written twice:
 *       pts2, sdf2 [2P], vd2 rows < P), unit normal, material heads, uncertainty mask.
 */
int esr_lts_ref_order(const int32_t *rec_ray, const int32_t *cnt3, const int32_t *off3, const int64_t *cnt3_cumsum,
                      int32_t n_slots, int64_t *perm, int64_t *ray64, void *stream);
int esr_lts_perturb(const float *pts_all, const int64_t *perm, const float *noise_normal, const float *noise_emit,
                    float emit_eps, int32_t m3, float *noise_n, float *pts_e, void *stream);
int esr_lts_gather_rows(const float *src, int32_t tile_rows, int32_t row_stride, int32_t col0, int32_t n_ch,
                        const int64_t *perm, int32_t n, float *out, void *stream);
typedef struct esr_lts_gather {
    const int64_t *jp, *ray64;
    const float *pts_all, *eg, *rec_sdf, *viewdirs, *brdf_a, *emit_a;
    const uint8_t *umask_rays;
    int32_t n_pts;
    float *pts2, *vd2, *sdf2, *normal, *base, *rough, *metal, *emis;
    uint8_t *umask;
    int32_t *pt1;      /* optional: pt1[jp[p]] = p + 1 (int32 [n_slots], zeroed by the caller): slot -> surface point */
} esr_lts_gather_t;
int esr_lts_gather_points(const esr_lts_gather_t *g, void *stream);

/*
 * Hemisphere directions -- replaces diffuse_scattering (app/utils/pbr/functions.py:10-18)
 * given the standard-normal draws: normalise, flip into the hemisphere of `normal`.
 * raw, dirs [n_pts, rays_plus_one, 3]; normal [n_pts,3].
 */
int esr_lts_dirs(const float *raw, const float *normal, int32_t n_pts, int32_t rays_plus_one,
                 float *dirs, void *stream);

/*
 * Rendering-equation estimate at n_pts surface points with n_rays secondary rays each
 * (esrnerf.py:565-572 disney_reflection, :653-677 env term, means, emo_hat; pbr/module.py:133-143
 * spherical-Gaussian env map; pbr/functions.py:108-173).  The two "copies" are the camera view
 * direction and the random one (-dirs[:, n_rays]).  All arrays row-major device memory.
 */
typedef struct esr_lts_args {
    int32_t n_pts, n_rays, n_sg, pdra_mode;
    const float *base, *rough, *metal;      /* [P,3] [P] [P]  BRDF parameters at the points      */
    const float *normal, *view;             /* [P,3] unit normal (detached), [P,3] view direction */
    const float *dirs;                      /* [P, n_rays+1, 3] from esr_lts_dirs                 */
    const float *off_m, *emo_m, *last2;     /* [P*R,3] [P*R,3] [P*R] marched secondary rays       */
    const float *mus, *lambdas, *lobes;     /* [J,3] [J] [J,3] envmap parameters (J <= 64)        */
    const float *emission;                  /* [P,3]                                              */
    const uint8_t *umask;                   /* [P] uncertain-ray flags (pdra) or NULL             */
} esr_lts_args_t;

typedef struct esr_lts_grads {
    float *d_off_m, *d_emo_m, *d_last2;     /* [P*R,3] [P*R,3] [P*R]  written                     */
    float *d_base, *d_rough, *d_metal, *d_emission;   /* [P,3] [P] [P] [P,3]  written             */
    float *d_mus, *d_lambdas, *d_lobes;     /* accumulated into (caller zero-fills)               */
} esr_lts_grads_t;

/* off_hat, emo_hat [2P,3]: rows [0,P) camera direction, [P,2P) random direction. */
int esr_lts_combine_fwd(const esr_lts_args_t *args, float *off_hat, float *emo_hat, void *stream);
int esr_lts_combine_bwd(const esr_lts_args_t *args, const float *g_off_hat, const float *g_emo_hat,
                        const esr_lts_grads_t *grads, void *stream);

/*
 * Emission edit of the re-lighting fine-tune, in place on emit [n,3] -- replaces
 * app/fine/model/esrnerf.py:427-441 with rgb_to_hsv / hsv_to_rgb of
 * app/utils/pbr/functions.py:214-255.  em_modes int64 [n]: 0 emission off, 1 unchanged,
 * 2 scaled by em_intensities [n], 3 hue/saturation replaced by em_colors [n,2] (value kept),
 * 4 both.
 */
int esr_emit_edit(float *emit, const int64_t *em_modes, const float *em_intensities,
                  const float *em_colors, int32_t n, void *stream);

/*
 * Small tile-major helpers of the LTS renderer.
 *  esr_act_*: out = act(z) on the first n_ch rows of [tiles,rows,32] tiles, rest zero
 *     (act 0 softplus: radiance / emission heads, 1 sigmoid: BRDF head; pbr/module.py:21,64,83).
 *  esr_composite3_*: out[ray,c] += w * v[c] (segment sum over sorted rays, esrnerf.py:639-651,783-788)
 *     and its backward (accumulate bit 0: add into dv, bit 1: add into dweight).
 *  esr_lts_tone_in_bwd: as esr_fine_tone_in_bwd for lin = off + emo WITHOUT the detach
 *     (esrnerf.py:751-757): dz_off on all tiles, dz_emo on the on-tiles.
 *  esr_sample_points: world positions of the march records (padding -> 0).
 */
/*
 * Round 4: the same glue with FEWER launches (a light-transport step issued ~100 kernels shorter than 10 us; what they
 * cost is the host's enqueue time, tools/host_profile.py).  Batched forms: one launch, blockIdx.y = job.
 *
 * esr_act_batch: up to ESR_ACT_MAX_JOBS activation jobs.  A forward job is esr_act_fwd.  A backward job computes
 *   dz[slot][c] = act'(z) * ( g_tile[slot][c]                                  (tile-major, optional)
 *                           + src[k][c]       k = inv ? inv[slot] : slot, if 0 <= k < n_src and c < src_c   (optional)
 *                           + ex_i[p][c - ex_col0[i]]   p = pt1[slot] - 1 >= 0, for up to three extras       (optional) )
 *   i.e. the reference-order gradient rows of a head (`src`, scattered back through the inverse of esr_lts_ref_order's
 *   permutation), the rendering equation's gradients at the chosen surface points (`ex`, through pt1 of
 *   esr_lts_gather_points) and a tile-major upstream gradient, summed and multiplied by the activation's derivative in
 *   one pass -- the reference's lines are index_put / index_add_ / cat on [M3, C] tensors followed by the activation's
 *   autograd (app/fine/model/esrnerf.py:770-806, backward of :792-851).
 */
#define ESR_ACT_MAX_JOBS 4
typedef struct esr_act_job {
    const float *z;            /* [tiles, rows, 32] pre-activations                                        */
    const float *g_tile;       /* backward: tile-major upstream gradient or NULL                           */
    float *out;                /* [tiles, rows, 32]                                                        */
    int32_t tiles, rows, n_ch, act, bwd;
    const float *src;          /* backward: [n_src, src_c] row-major or NULL                               */
    int32_t src_c, n_src;
    const int32_t *inv;        /* slot -> row of src (-1: none); NULL: identity                            */
    const int32_t *pt1;        /* slot -> surface point + 1 (0: none) or NULL                              */
    const float *ex[3];        /* [P, ex_c[i]] row-major or NULL                                           */
    int32_t ex_c[3], ex_col0[3];
} esr_act_job_t;
int esr_act_batch(const esr_act_job_t *jobs, int32_t n_jobs, void *stream);

/* esr_lts_gather_rows for up to ESR_GATHER_MAX_JOBS (src, out) pairs in one launch. */
#define ESR_GATHER_MAX_JOBS 4
typedef struct esr_gather_job {
    const float *src;
    int32_t tile_rows, row_stride, col0, n_ch;
    const int64_t *perm;
    int32_t n;
    float *out;
} esr_gather_job_t;
int esr_lts_gather_rows_batch(const esr_gather_job_t *jobs, int32_t n_jobs, void *stream);

/* esr_pair_loss_fwd_bwd for up to ESR_PAIR_MAX_JOBS terms in one launch (all add into the same `loss`). */
#define ESR_PAIR_MAX_JOBS 6
typedef struct esr_pair_job {
    const float *a, *b;
    int64_t rows;
    int32_t cols;
    const uint8_t *row_mask;
    int32_t mask_value;
    const int32_t *count_dev;
    int32_t kind;
    float w_value, w_a, w_b;
    float *ga, *gb;
} esr_pair_job_t;
int esr_pair_loss_batch(const esr_pair_job_t *jobs, int32_t n_jobs, float *loss, void *stream);

/* esr_lts_ref_order that also writes the INVERSE: inv[j] = rank of compact slot j in the reference's order, -1 for a
 * padding slot (inv: int32 [n_slots]). */
int esr_lts_ref_order_inv(const int32_t *rec_ray, const int32_t *cnt3, const int32_t *off3, const int64_t *cnt3_cumsum,
                          int32_t n_slots, int64_t *perm, int64_t *ray64, int32_t *inv, void *stream);

/* esr_lts_dirs that also writes what the secondary march and the points pass read (esrnerf.py:565-591): the secondary
 * rays' origins o2 [P * n_rays, 3] (pts[p] repeated), their directions d2 [P * n_rays, 3] (dirs[:, :n_rays]) and the
 * random view direction v_rand [P, 3] = -dirs[:, n_rays]; pts [P, 3].  rays_plus_one = n_rays + 1. */
int esr_lts_dirs_rays(const float *raw, const float *normal, const float *pts, int32_t n_pts, int32_t rays_plus_one,
                      float *dirs, float *o2, float *d2, float *v_rand, void *stream);

int esr_act_fwd(const float *z, int32_t tiles, int32_t rows, int32_t n_ch, int act, float *out, void *stream);
int esr_act_bwd(const float *z, const float *g, int32_t tiles, int32_t rows, int32_t n_ch, int act,
                float *dz, void *stream);
int esr_composite3_fwd(const float *v, int32_t rows, const int32_t *rec_ray, const float *rec_w,
                       int32_t tiles, float *out, void *stream);
int esr_composite3_bwd(const float *g, const float *v, int32_t rows, const int32_t *rec_ray,
                       const float *rec_w, int32_t tiles, int accumulate, float *dv, float *dweight,
                       void *stream);
int esr_lts_tone_in_bwd(const float *dXt, const float *Xt, const float *g_lin, const float *lin, const float *z_off,
                        const float *z_emo, const int32_t *rec_ray, const float *rec_w, int32_t tiles_on,
                        int32_t tiles_all, float *dz_off, float *dz_emo, void *stream);
int esr_sample_points(const esr_scene_t *scene, const float *rays_o, const float *rays_d,
                      const int32_t *rec_ray, const int32_t *rec_step, int32_t n, float *pts, void *stream);

/* ------------------------------------------------------------------------- *
 * D. Coarse stage (VoxurfC) -- dense whole-grid operators
 * ------------------------------------------------------------------------- */

/*
 * Gaussian smoothing of the SDF grid -- replaces Gaussian3DConv.forward
 * (app/utils/base/module.py:145-177: nn.Conv3d(1,1,k, padding=k//2, padding_mode="replicate"),
 * called on every forward at app/coarse/model/voxurfc.py:202).  in/out [gx,gy,gz];
 * weights_host: k*k*k floats in HOST memory in Conv3d order (they travel as a kernel argument).
 * _bwd is the exact adjoint (a gather, no atomics): gin += conv^T(gout).
 */
int esr_gauss3d_fwd(const float *in, const float *weights_host, int ksize, int32_t gx, int32_t gy,
                    int32_t gz, float *out, void *stream);
int esr_gauss3d_bwd(const float *gout, const float *weights_host, int ksize, int32_t gx, int32_t gy,
                    int32_t gz, float *gin, void *stream);

/*
 * Dense central-difference gradient of the SDF grid -- replaces VoxurfC.neus_sdf_gradient
 * (app/coarse/model/voxurfc.py:597-616).  grad is channels-last [gx,gy,gz,3] (component a =
 * d/d grid axis a = world x,y,z), zero on the boundary layer of each axis.  _bwd: gsdf += adjoint.
 */
int esr_central_grad_fwd(const float *sdf, int32_t gx, int32_t gy, int32_t gz, float voxel_size,
                         float *grad, void *stream);
int esr_central_grad_bwd(const float *ggrad, int32_t gx, int32_t gy, int32_t gz, float voxel_size,
                         float *gsdf, void *stream);

/*
 * Per-sample features of the coarse renderer (app/coarse/model/voxurfc.py:221-250) on the march
 * records.  grad_grid [gx,gy,gz,3] (esr_central_grad_fwd), off_color / emo_color [gx,gy,gz,12]
 * channels-last.  X [tiles,72,32] rows: 0-11 off colour | 12-23 emo colour (on-tiles) | 24-26 normal
 * = g/(|g|+1e-5) | 27-29 xyz | 30-44 sin | 45-59 cos | 60-68 view PE | 69-71 zero; gnorm [tiles*32] = |g|.
 * _bwd: dX_off (all tiles) / dX_emo (on-tiles) [tiles,64,32] from esr_mlp_dgrad(ESR_MLP_COARSE) ->
 * atomic scatters into the colour-grid gradients and into g_grad_grid [gx,gy,gz,3].
 */
int esr_coarse_feat_fwd(const esr_scene_t *scene, const float *rays_o, const float *rays_d,
                        const float *viewdirs, const int32_t *rec_ray, const int32_t *rec_step,
                        int32_t tiles_on, int32_t tiles_all, const float *grad_grid,
                        const float *off_color, const float *emo_color, float *X, float *gnorm,
                        void *stream);
int esr_coarse_feat_bwd(const esr_scene_t *scene, const float *rays_o, const float *rays_d,
                        const float *viewdirs, const int32_t *rec_ray, const int32_t *rec_step,
                        int32_t tiles_on, int32_t tiles_all, const float *X, const float *gnorm,
                        const float *dX_off, const float *dX_emo, float *g_grad_grid,
                        float *g_off_color, float *g_emo_color, void *stream);

/*
 * rgb = sigmoid(z_off) + [on-tiles] sigmoid(z_emo) and its weighted segment sum per ray
 * (voxurfc.py:240-258; srgb_marched [n_rays,3] accumulated into, caller zero-fills); backward
 * with white_bg = 1 - sum of weights folded in: dweight = g_srgb[ray].rgb - g_white_bg[ray].
 */
int esr_coarse_shade_fwd(const float *z_off, const float *z_emo, const int32_t *rec_ray,
                         const float *rec_w, int32_t tiles_on, int32_t tiles_all, float *rgb,
                         float *srgb_marched, void *stream);
int esr_coarse_shade_bwd(const float *g_srgb, const float *g_white_bg, const float *rgb,
                         const float *z_off, const float *z_emo, const int32_t *rec_ray,
                         const float *rec_w, int32_t tiles_on, int32_t tiles_all, float *dz_off,
                         float *dz_emo, float *dweight, void *stream);

/* ------------------------------------------------------------------------- *
 * F. Image rendering (forward_evaluate) helpers
 * ------------------------------------------------------------------------- */

/*
 * Per-sample auxiliaries of forward_evaluate (app/fine/model/voxurff.py:431-443, app/coarse/model/voxurfc.py:
 * 395-412) from a feature tile X [tiles,xrows,32] whose rows row_nx/ny/nz hold the unit normal (fine tile:
 * 40, 36, 32 = the radius-1 finite difference; coarse tile: 24, 25, 26): aux [tiles,8,32] rows 0-2 =
 * camera-space normal colour ((n @ pos_rt) * (1,-1,-1) + 1) / 2, row 4 = step_id * stepdist, other rows 0.
 * pos_rt_host: 3x3 row-major in HOST memory.  Composite with esr_composite3_fwd(aux, 8, ...) and
 * esr_composite3_fwd(aux + 4*32, 8, ...) (column 0 of the second result is the depth).
 * esr_eval_disp: depth[i] = depth3[3i]; disp[i] = 1 / (depth + alphainv_last * far).
 */
int esr_eval_aux(const float *X, int32_t xrows, int32_t row_nx, int32_t row_ny, int32_t row_nz,
                 const int32_t *rec_ray, const int32_t *rec_step, int32_t tiles,
                 const float *pos_rt_host, float stepdist, float *aux, void *stream);
int esr_eval_disp(const float *depth3, const float *alphainv_last, float far_, int32_t n_rays,
                  float *depth, float *disp, void *stream);

/* ------------------------------------------------------------------------- *
 * E. Optimizer
 * ------------------------------------------------------------------------- */

/*
 * One fused Adam update of a parameter tensor, in place -- replaces `adam`
 * (app/utils/optimizer.py:183-228; betas (0.9, 0.99) at :60, optional per-voxel lr :98-100).
 * step >= 1 is the value AFTER the increment (bias corrections 1 - beta^step).  All pointers:
 * n contiguous fp32 device values; per_lr NULL or [n].
 */
int esr_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                  const float *per_lr, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, void *stream);

/*
 * The same update restricted to LIVE bricks (bricks of esr_brick_floats() = 128 consecutive values, as section F; the last
 * one may be ragged).  A brick is live once any of its gradients was non-zero (by value: -0.0 is zero) or its moments are;
 * it stays live.  Bricks that are neither live nor have a non-zero gradient in this call are skipped after the gradient
 * read: with g == m == v == 0, no weight decay, eps > 0 and a finite per_lr the update is the identity, so param,
 * exp_avg and exp_avg_sq hold the bytes esr_adam_step would have left.
 *   live:      [ceil(n/128)] bytes, read and updated (0 -> 1 only)
 *   zero_grad: non-zero = write zeros over every gradient brick that held a non-zero value (the buffer is all-zero after)
 *   stats:     NULL or int64[2]:  stats[0] += live bricks after the call, stats[1] += bricks with a non-zero gradient
 * There is no weight decay.  All pointers 16-byte aligned; ESR_EINVAL otherwise, for eps <= 0, and for what
 * esr_adam_step rejects.
 *   esr_brick_live_from_moments: live[b] |= any(exp_avg != 0 or exp_avg_sq != 0) over brick b (after a state load)
 */
int esr_adam_step_live(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const float *per_lr,
                       uint8_t *live, int64_t n, float lr, float beta1, float beta2, float eps, int32_t step,
                       int32_t zero_grad, int64_t *stats, void *stream);
int esr_brick_live_from_moments(const float *exp_avg, const float *exp_avg_sq, int64_t n, uint8_t *live,
                                void *stream);

/*
 * Smoothed-gradient TV term of the fine / lts trainers, forward and backward -- replaces the dense torch chain
 * neus_sdf_gradient (app/fine/model/voxurff.py:723-742) -> GradientConv (app/utils/base/module.py:180-211, 3x3x3,
 * replicate padding; the conv branch is detached) -> masked mean of squares (voxurff.py:609-617).
 *   fwd: loss[0] += weight * mean_{c, p in mask} (conv(g_c)[p] - g_c[p])^2 ;  work6 [6, X, Y, Z] keeps g and err
 *   bwd: grad_sdf += grad_out * d loss / d sdf  (from the err planes left in work6 by fwd)
 * sdf [X,Y,Z]; mask [X,Y,Z] bytes (nonempty_mask); conv_w27: HOST array, kernel order [dx][dy][dz];
 * masked_cells = number of set mask bytes (the mean runs over 3 * masked_cells values).
 */
int esr_smooth_grad_tv_fwd(const float *sdf, const uint8_t *mask, const float *conv_w27, float conv_bias,
                           int32_t gx, int32_t gy, int32_t gz, float voxel_size, int64_t masked_cells,
                           float weight, float *work6, float *loss, void *stream);
int esr_smooth_grad_tv_bwd(const float *work6, int32_t gx, int32_t gy, int32_t gz, float voxel_size,
                           int64_t masked_cells, float weight, const float *grad_out /* device scalar or NULL = 1 */,
                           float *grad_sdf, void *stream);

/*
 * HOST helper (no device work, no stream): out[0..k) = np.random.choice(n, k, replace=False) of numpy's legacy
 * RandomState (the surface-point draw of app/fine/model/esrnerf.py:792 / :470), bit for bit, on the MT19937 state
 * passed in (key: 624 words, *pos: 0..624; both updated).  Exists so that the draw can run on a worker thread
 * without the GIL while the primary pass is being enqueued.
 */
int esr_host_choice_noreplace(uint32_t *key, int32_t *pos, int64_t n, int64_t k, int64_t *out);
/*
 * The same draw on a worker thread owned by the library (one thread, jobs in submission order): _start returns at once with a
 * job handle, _wait blocks until that job is done, returns its code and releases the handle (exactly one _wait per _start;
 * key / pos / out must stay valid until then).  No interpreter involvement on the worker: starting it costs microseconds.
 */
int esr_host_choice_start(uint32_t *key, int32_t *pos, int64_t n, int64_t k, int64_t *out, void **job);
int esr_host_choice_wait(void *job);

/* ------------------------------------------------------------------------- *
 * F. Data-parallel gradient exchange (no reference counterpart: the reference is single-process,
 *    SURVEY 2a / 8(e); the sum over ranks itself is torch.distributed = RCCL)
 * ------------------------------------------------------------------------- */

/*
 * Brick-sparse view of a flat fp32 gradient buffer (16-byte aligned, n values): bricks of
 * esr_brick_floats() (= 128) consecutive values; the last brick may be ragged.
 *   esr_brick_flags:  flags[b] = 1 if any value of brick b is non-zero, else 0  (ceil(n/128) bytes)
 *   esr_brick_pack:   packed[k*128 .. ] = brick brick_idx[k] (ragged tail zero-filled), k < n_idx
 *   esr_brick_unpack: the inverse scatter (values past n are dropped)
 * brick_idx: int64 device array, strictly increasing brick numbers < ceil(n/128).
 */
int esr_brick_floats(void);
int esr_brick_flags(const float *buf, int64_t n, uint8_t *flags, void *stream);
int esr_brick_pack(const float *buf, int64_t n, const int64_t *brick_idx, int64_t n_idx, float *packed,
                   void *stream);
int esr_brick_unpack(const float *packed, const int64_t *brick_idx, int64_t n_idx, float *buf, int64_t n,
                     void *stream);
/*
 * The union's brick list on the device: idx[0..cap) = the first `cap` flagged bricks in ascending order, unused slots -1
 * (what esr_brick_pack / _unpack skip); *count = the number of flagged bricks, which may exceed cap (the caller reads it
 * later and sends the overflow in a second pass).  scratch: esr_brick_list_scratch_ints() int32.  Replaces six torch
 * launches inside the data-parallel step (esr_nerf_amd/grad_sync.py).
 */
int64_t esr_brick_list_scratch_ints(void);
int esr_brick_list(const uint8_t *flags, int64_t n_bricks, int64_t cap, int64_t *idx, int64_t *count, int32_t *scratch,
                   void *stream);

/* ------------------------------------------------------------------------- *
 * G. Mesh export (extract_geometry): the -sdf lattice field and marching cubes
 * ------------------------------------------------------------------------- */

/*
 * The field of extract_geometry -- replaces app/fine/model/voxurff.py:745-770 (-grid_sample of the SDF grid) over
 * app/utils/base/functions.py:108-139 (extract_fields' lattice).  u[i,j,k] = -trilinear(sdf, (xs[i], ys[j], zs[k])) with
 * F.grid_sample(align_corners=True)'s arithmetic.  sdf [gx,gy,gz] (raw, or smoothed by esr_gauss3d_fwd); box_host [host]
 * xyz_min[3], xyz_max[3]; xs [r0], ys [r1], zs [r2] the lattice axes (torch.linspace); u [r0,r1,r2].  2 <= r <= 1024.
 */
int esr_mesh_field(const float *sdf, int32_t gx, int32_t gy, int32_t gz, const float *box_host, const float *xs,
                   const float *ys, const float *zs, int32_t r0, int32_t r1, int32_t r2, float *u, void *stream);
/*
 * Marching cubes of u [r0,r1,r2] at `threshold` -- replaces mcubes.marching_cubes.  Count -> scan -> emit, no atomics:
 *   esr_mesh_blocks:  nb, the number of node blocks (a negative ESR_E* for bad dims); the caller allocates
 *                     counts / offsets as int64 [2, nb]
 *   esr_mesh_count:   counts[0][b] = vertices, counts[1][b] = triangles of block b
 *   esr_mesh_emit:    offsets = the exclusive scan of counts along b; vid int32 [r0*r1*r2] scratch (every vertex id must
 *                     fit 31 bits); vertices f64 [V,3] in index space, triangles i64 [F,3] (V, F = the count totals).
 * A node is inside iff u > threshold; one vertex per crossed lattice edge at n + t e_a, t = (thr - u[n]) / (u[n+e_a] - u[n])
 * in f64; vertices ordered by owner node then axis, triangles by cell then case-table order (csrc/mc_table.h);
 * (b - a) x (c - a) points towards decreasing u.
 */
int64_t esr_mesh_blocks(int32_t r0, int32_t r1, int32_t r2);
int esr_mesh_count(const float *u, int32_t r0, int32_t r1, int32_t r2, float threshold, int64_t *counts, void *stream);
int esr_mesh_emit(const float *u, int32_t r0, int32_t r1, int32_t r2, float threshold, const int64_t *offsets,
                  int32_t *vid, double *vertices, int64_t *triangles, void *stream);

/* ------------------------------------------------------------------------- *
 * H. Chamfer metric (utils2.metric.DTU_CD): triangle sampling, a cell index, the radius downsample, nearest neighbours
 * ------------------------------------------------------------------------- */

/*
 * A cell index over a point cloud of n points [host struct, device arrays].  Cell c = floor((p - origin) / h) per axis
 * (0 <= c < dims, each dims < 2^21), key = cx << 42 | cy << 21 | cz.  pts [n,3] f64 are the points sorted by key (stable);
 * ids [n] the sort's source index of each; start [n_cells + 1] i64 the range of each unique key; keys [cap] i64 / cells
 * [cap] i32 the hash table key -> unique-key rank (cap a power of two > the cell count, empty slots -1, filled by
 * esr_cd_hash_insert).  coarse, ckeys [ccap]: the occupancy table of the cells of coarse^3 fine cells (esr_cd_nn only).
 */
typedef struct {
    double origin[3];
    double h;
    int32_t dims[3];
    int32_t coarse;
    int64_t cap;
    const int64_t *keys;
    const int32_t *cells;
    const int64_t *start;
    const double *pts;
    const int32_t *ids;
    int64_t ccap;
    const int64_t *ckeys;
} esr_cd_index_t;

/*
 * Points sampled on triangles -- replaces utils2/metric.py:101-165 (sample_single_tri over a multiprocessing pool).
 * vertices [V,3] f64, triangles [n_tri,3] i64.  esr_cd_sample_count: counts [n_tri] i64 (0 for area2 == 0);
 * esr_cd_sample_fill: points [sum counts, 3] f64, triangle t's samples from row offsets[t] (the exclusive scan of counts)
 * in the reference's (i, j) row-major order.  Arithmetic: the header of csrc/chamfer.hip.
 */
int esr_cd_sample_count(const double *vertices, const int64_t *triangles, int64_t n_tri, double thresh, int64_t *counts,
                        void *stream);
int esr_cd_sample_fill(const double *vertices, const int64_t *triangles, int64_t n_tri, double thresh,
                       const int64_t *offsets, double *points, void *stream);
/* keys [n] i64 of points [n,3] f64 under index->origin / h / dims (cells clamped into the box; ESR_ECAP for dims >= 2^21) */
int esr_cd_cell_keys(const esr_cd_index_t *index, const double *points, int64_t n, int64_t *keys, void *stream);
/* inserts the n_u distinct ukeys into table_keys [cap] (pre-filled with -1), table_vals [cap] = the key's rank (or NULL) */
int esr_cd_hash_insert(const int64_t *ukeys, int64_t n_u, int64_t cap, int64_t *table_keys, int32_t *table_vals,
                       void *stream);
/*
 * One round of the radius downsample -- replaces utils2/metric.py:168-187 (radius_neighbors + the keep loop).  points
 * [n,3] f64 in the order; the index is built over the same points with h >= thresh and ids = the order rank.  state [n]
 * i8: 0 undecided, 1 kept, 2 removed (start all 0); point k becomes removed when a kept earlier point lies within thresh
 * (((dx*dx + dy*dy) + dz*dz) <= thresh*thresh) and kept when every earlier point within thresh is removed.  Sets
 * changed[0] = 1 when a state changed; rounds until one changes nothing give the sequential loop's mask exactly.
 */
int esr_cd_downsample_round(const esr_cd_index_t *index, const double *points, int64_t n, double thresh, int8_t *state,
                            int32_t *changed, void *stream);
/*
 * Nearest-neighbour distances -- replaces the kd-tree kneighbors passes of utils2/metric.py:209-231.  queries [nq,3] f64;
 * dist [nq] f64 = sqrt(min squared distance to the index's points), +inf when that is not < max_dist.
 */
int esr_cd_nn(const esr_cd_index_t *index, const double *queries, int64_t nq, double max_dist, double *dist, void *stream);

/* ------------------------------------------------------------------------- *
 * I. DVGO pre-stage (app/coarse/model/dvgo.py, the alphamask renderer)
 * ------------------------------------------------------------------------- */

/*
 * The model [host struct, device grids]: density [1,X,Y,Z], off_color and emo_color [3,X,Y,Z] (channels first, as the
 * nn.Parameters); xyz_min / xyz_max the box; step_scale = stepsize * voxel_size rounded as torch rounds it (float32);
 * interval = stepsize; n_samples = the model's N_samples (S).
 */
typedef struct {
    const float *density;
    const float *off_color;
    const float *emo_color;
    int32_t dims[3];
    float xyz_min[3];
    float xyz_max[3];
    float near_, far_, step_scale, interval, act_shift;
    int32_t n_samples;
} esr_dvgo_t;

/*
 * The rays [host struct, device arrays]: rays_o, rays_d [n,3]; nrm [n] = rays_d.norm(dim=-1) (torch's); jitter [n] the
 * training draw u (NULL: none); em_modes [n] int32 (NULL: every ray is em_all).
 */
typedef struct {
    const float *rays_o;
    const float *rays_d;
    const float *nrm;
    const float *jitter;
    const int32_t *em_modes;
    int32_t em_all;
    int64_t n_rays;
} esr_dvgo_rays_t;

/*
 * Outputs [host struct, device arrays].  Training (esr_dvgo_fwd): alpha [n,S] (kept for the backward), alphainv_cum
 * [n,S+1], weights [n,S], raw_rgb [n,S,3], rgb [n,3].  Evaluation (esr_dvgo_eval): alpha [n,S] scratch, depth, disp [n],
 * white_bg [n], off_rgb, on_rgb, emo_rgb [n,3] (rgb is off_rgb or on_rgb: the caller picks).
 */
typedef struct {
    float *alpha;
    float *alphainv_cum;
    float *weights;
    float *raw_rgb;
    float *rgb;
    float *depth;
    float *disp;
    float *white_bg;
    float *off_rgb;
    float *on_rgb;
    float *emo_rgb;
} esr_dvgo_out_t;

/*
 * Backward of esr_dvgo_fwd [host struct, device arrays]: alpha, alphainv_cum, raw_rgb as the forward wrote them; the
 * upstream gradients g_alphainv_cum [n,S+1], g_weights [n,S], g_raw_rgb [n,S,3], g_rgb [n,3] (each may be NULL: zero);
 * grad_density [X,Y,Z], grad_off, grad_emo [3,X,Y,Z] are ADDED to (float atomics: the caller zeroes them).
 */
typedef struct {
    const float *alpha;
    const float *alphainv_cum;
    const float *raw_rgb;
    const float *g_alphainv_cum;
    const float *g_weights;
    const float *g_raw_rgb;
    const float *g_rgb;
    float *grad_density;
    float *grad_off;
    float *grad_emo;
} esr_dvgo_bwd_t;

/*
 * forward_training / forward_evaluate -- replaces dvgo.py:140-263 (sample_ray, grid_sampler, activate_density,
 * get_ray_marching_ray and the colour sums).  Arithmetic and mapping: the header of csrc/dvgo.hip.
 */
int esr_dvgo_fwd(const esr_dvgo_t *model, const esr_dvgo_rays_t *rays, const esr_dvgo_out_t *out, void *stream);
int esr_dvgo_eval(const esr_dvgo_t *model, const esr_dvgo_rays_t *rays, const esr_dvgo_out_t *out, void *stream);
int esr_dvgo_bwd(const esr_dvgo_t *model, const esr_dvgo_rays_t *rays, const esr_dvgo_bwd_t *bwd, void *stream);
/*
 * voxel_count_views, one view -- replaces dvgo.py:59-93.  sum [X,Y,Z] (zeroed by the caller) += the trilinear weights of
 * the S unjittered, unmasked samples of every ray; esr_dvgo_count_add: count[i] += sum[i] > 1.
 */
int esr_dvgo_count(const esr_dvgo_t *model, const esr_dvgo_rays_t *rays, float *sum, void *stream);
int esr_dvgo_count_add(const float *sum, int64_t n, float *count, void *stream);

/* ------------------------------------------------------------------------- *
 * J. Image-level evaluation metrics (utils2/metric.py rgb_ssim / IoU, the view post-processing of app/fine/fine.py:572-605)
 * ------------------------------------------------------------------------- */

#define ESR_SSIM_MAX_TAPS 33     /* largest filter_size of esr_ssim (ESR_ECAP beyond it: the tile's LDS image)          */
#define ESR_METRICS_BLOCKS 1024  /* most workgroups of a metrics launch = doubles per `partials` sum                    */

/*
 * rgb_ssim -- replaces utils2/metric.py:31-88.  img0, img1 [H,W,3] f32; taps [host] the filter_size float64 filter
 * weights (metric.py:47-51); c1 = (k1 max_val)^2, c2 = (k2 max_val)^2.  map (or NULL) [H-fs+1, W-fs+1, 3] f64;
 * partials [ESR_METRICS_BLOCKS] f64 scratch; mean [1] f64 = the mean of the map.  One fused launch plus a one-workgroup
 * sum of the partials: no float atomics, the same bits on every call.  ESR_EINVAL for H or W < filter_size.
 * Arithmetic (float32 products, float64 behind them): the header of csrc/metrics.hip.
 */
int esr_ssim(const float *img0, const float *img1, int32_t H, int32_t W, const double *taps, int32_t filter_size, double c1,
             double c2, double *map, double *partials, double *mean, void *stream);

/*
 * One result image of a view [host struct, device arrays] -- replaces fine.py:572-587, the uint8 images of :611-617 and
 * the F.mse_loss calls of :596-601.  v [n,channels] f32 (channels 1 or 3), wbg [n] f32 or NULL (no background term):
 *   s = v + wbg * wbg_scale
 *   lin == 0: out = clamp(s, 0, 1)
 *   lin != 0: out = max(s, 0); gamma = apply_gamma_curve(clamp(s, 0, 1)) (utils2/image.py:14-26, float32)
 * out may be v.  out_u8 / gamma_u8 (or NULL) = (uint8)(clamp01(.) * 255) of the float written beside it.  target_out /
 * target_gamma (or NULL) [n,channels] f32: sqerr[0] / sqerr[1] (f64) = the sum over all elements of
 * ((double)out - (double)target)^2, deterministic; partials [2 * ESR_METRICS_BLOCKS] f64 scratch (needed with a target).
 */
typedef struct {
    const float *v;
    const float *wbg;
    float wbg_scale;
    int32_t lin;
    int64_t n;
    int32_t channels;
    float *out;
    float *gamma;
    uint8_t *out_u8;
    uint8_t *gamma_u8;
    const float *target_out;
    const float *target_gamma;
    double *partials;
    double *sqerr;
} esr_view_post_t;
int esr_view_post(const esr_view_post_t *job, void *stream);
/* sum [1] f64 = sum_i ((double)a[i] - (double)b[i])^2, a, b [n] f32; partials [ESR_METRICS_BLOCKS] f64 scratch */
int esr_sqerr_sum(const float *a, const float *b, int64_t n, double *partials, double *sum, void *stream);
/* y = apply_gamma_curve(x) (utils2/image.py:14-26), x, y [n] f32 */
int esr_gamma_curve(const float *x, int64_t n, float *y, void *stream);
/* IoU counts -- replaces utils2/metric.py:95-98.  mask1, mask2 [n] u8 / bool; counts [2] i64 = |m1 & m2|, |m1 | m2| */
int esr_mask_iou(const uint8_t *mask1, const uint8_t *mask2, int64_t n, int64_t *counts, void *stream);

/* ------------------------------------------------------------------------- *
 * K. Re-lighting edit rays (app/fine/pdra.py:934-1045, filter_edit_rays)
 * ------------------------------------------------------------------------- */

#define ESR_RELIGHT_MAX_COND 16  /* most edit conditions of a view (ESR_ECAP beyond it: they travel as kernel arguments) */

/*
 * Grey-level dilation of masks [n_cond,h,w] f32 by a ks x ks box into out (same shape, not masks itself) -- replaces
 * cv2.dilate(src, np.ones((ks, ks)), iterations=1) of pdra.py:945-962: anchor ks / 2, i.e. the window
 * dy, dx in [-(ks / 2), ks - 1 - ks / 2] (NOT symmetric for an even ks), pixels outside the image take no part.  Any
 * ks >= 1, h, w >= 1; a window that is larger than the image is clipped to it.  ESR_ECAP when the clipped tile plus halo
 * does not fit a CU's LDS (windows beyond ~130 pixels on images that large).  Bit-identical to the definition.
 */
int esr_mask_dilate(const float *masks, int32_t n_cond, int32_t h, int32_t w, int32_t ks, float *out, void *stream);
/*
 * Edit labels of n rays from their expected surface points esp [n,3] f32 -- replaces pdra.py:988-1028.  w2c [host] f32
 * [16]: the inverse of the view's pose, row-major; focal, w, h: the camera (K = [[-f,0,w/2-0.5],[0,f,h/2-0.5],[0,0,1]]);
 * masks [n_cond,h,w] f32: the DILATED masks; cond_modes [host] i64 [n_cond] (0..4, else ESR_EINVAL), cond_intensities
 * [host] f32 [n_cond] and cond_colors [host] f32 [n_cond,2] (NULL = zeros).  Outputs: keep u8 [n] (some condition
 * matched), em_modes i64 [n], em_colors f32 [n,2], em_intensities f32 [n] as esr_emit_edit takes them; uv (or NULL) f32
 * [n,2]: the projected pixel coordinates (diagnostics).  One launch, no atomics: the same bytes on every call.
 * Arithmetic, the reference quirks that are reproduced and the non-finite case: the header of csrc/relight.hip.
 */
int esr_edit_label(const float *esp, int64_t n, const float *w2c, float focal, int32_t w, int32_t h, const float *masks,
                   int32_t n_cond, const int64_t *cond_modes, const float *cond_intensities, const float *cond_colors,
                   uint8_t *keep, int64_t *em_modes, float *em_colors, float *em_intensities, float *uv, void *stream);

/* ------------------------------------------------------------------------- *
 * L. Training-ray filter (filter_training_rays_in_maskcache_sampling)
 * ------------------------------------------------------------------------- */

#define ESR_RAY_FILTER_MARCH 0   /* the march sampler, far = 1e9 (render_utils_kernel.cu:12-79,167-194)                   */
#define ESR_RAY_FILTER_FIXED 1   /* sample_ray_ori: t-range clamped to [near, far], n_samples steps for every ray          */

/*
 * keep[r] = 1 when some in-box sample of ray r lies inside the mask cache -- replaces the chunk loops of
 * app/coarse/model/voxurfc.py:426-446 (with sample_ray_ori, :448-481) and app/fine/model/voxurff.py:463-502 (both
 * branches; sample_ray_ori :504-537) and MaskCache.forward (app/utils/base/module.py:104-114) inside them.
 * scene: xyz_min / xyz_max, mask_min / mask_max, mx / my / mz, near_, stepdist (= stepsize * voxel_size in f32), act_shift
 * and mask_thres are read.  mask_density [mx,my,mz] f32 (max-pooled), rays_o / rays_d [n_rays,3] f32.
 * mode ESR_RAY_FILTER_MARCH: every step 0 .. n_steps - 1 of the march sampler with far = 1e9 (far_ and n_samples are not
 * read); there is NO per-ray step cap (unlike esr_march_count's scene.max_steps).  mode ESR_RAY_FILTER_FIXED: far_ =
 * the model's far, n_samples [host] = int(|grid_shape + 1| / stepsize) + 1; a ray with t_max <= t_min is dropped.
 * keep u8 [n_rays]; first_hit (or NULL) i32 [n_rays]: the index of the first kept step, -1 for a dropped ray.
 * n_rays == 0 launches nothing.  One wave per ray, no atomics, no workspace: the same bytes on every call.  Arithmetic
 * order of both samplers: the header of csrc/rayfilter.hip.
 */
int esr_ray_filter(const esr_scene_t *scene, const float *mask_density, const float *rays_o, const float *rays_d,
                   int64_t n_rays, int32_t mode, float far_, int32_t n_samples, uint8_t *keep, int32_t *first_hit,
                   void *stream);

/* ------------------------------------------------------------------------- *
 * M. Camera-defined ray sets (rays made in the kernel from (view, pixel))
 * ------------------------------------------------------------------------- */

/*
 * A set of n_views pinhole cameras that share their intrinsics and image size.  The ray of pixel p (i = p % width,
 * j = p / width) of a view with the camera-to-world matrix R | t (poses [n_views,3,4] f32, one convention: a loader's
 * `pose @ blender2opencv` is applied on the host):
 *   px = ((i + 0.5) - cx) / fx, py = ((j + 0.5) - cy) / fy, d = R (px, py, 1), o = t, viewdir = d / max(|d|, 1e-12)
 * in binary32 with correctly rounded division, every operation rounded on its own -- replaces pixelcoord / pose2ray /
 * F.normalize of data/esrnerf/esrnerf.py:48-59,238,252-259 and data/dtu/dtu.py:74-86,194,207-211.  One device function
 * (csrc/camera_ray.h) serves every entry below, so a ray is the same bits whichever of them made it.  A ray's row is
 * view * height * width + pixel; n_views * height * width < 2^31 (else ESR_EINVAL).
 */
typedef struct {
    float fx, fy, cx, cy;
    int32_t width, height, n_views;
} esr_camera_t;

#define ESR_CAMERA_LDS_VIEWS 256        /* esr_camera_batch stages the pose table in LDS up to this many views (12 KB)  */
#define ESR_CAMERA_BOUNDS_BLOCKS 1024   /* esr_camera_bounds: the most workgroup partials it writes (6 floats each)       */

/*
 * Dense rays of the views [v0, v1): rays_o, rays_d, viewdirs [(v1 - v0) * height * width, 3] f32 (16-byte aligned), in
 * row order -- replaces pose2ray + F.normalize (esrnerf.py:237-238,252-259, dtu.py:193-194,207-211).  v0 == v1 launches
 * nothing.  Plain stores, no atomics: the same bytes on every call.
 */
int esr_camera_rays(const esr_camera_t *cam, const float *poses, int32_t v0, int32_t v1, float *rays_o, float *rays_d,
                    float *viewdirs, void *stream);
/*
 * The batch dictionary of n ray rows (rows i64 [n], any order, repeats allowed) in ONE launch -- replaces the five row
 * gathers of a sampler's sample() over the arrays of esrnerf.py:233-248 / dtu.py:175-201.  Outputs rays_o, rays_d,
 * viewdirs, rgbs [n,3] f32 and em_modes i64 [n] = view_modes[view] (view_modes i64 [n_views]: the training loaders give
 * every ray of a view its view's mode, esrnerf.py:164-170, dtu.py:180-183).
 * images: channels == 0: f32 [n_views*height*width, 3], already composited, gathered as it is; channels == 3 / 4: u8
 * [n_views*height*width, channels].  A u8 value v becomes lut[v] (lut f32 [256] on the device: float32(arange(256) / 255.0)
 * with the division in float64, `torch.FloatTensor(np.asarray(image) / 255.0)` of esrnerf.py:159-161); with 4 channels
 * rgb = c * a + (1 - a) * white_bg, four separately rounded binary32 operations (esrnerf.py:235-236).  lut may be NULL and
 * white_bg is not read when channels == 0.
 * A row outside [0, n_views*height*width) reads nothing and yields NaN rays and colours and em_mode -1 (the host wrapper
 * refuses such rows before the launch).  n == 0 launches nothing.
 */
int esr_camera_batch(const esr_camera_t *cam, const float *poses, const int64_t *view_modes, const void *images,
                     int32_t channels, const float *lut, float white_bg, const int64_t *rows, int64_t n, float *rays_o,
                     float *rays_d, float *viewdirs, float *rgbs, int64_t *em_modes, void *stream);
/*
 * Bounding box of the frustum points o + viewdir * near_ and o + viewdir * far_ over every ray of every view -- replaces
 * the chunk loop of app/coarse/alphamask.py:108-122.  partials: f32 [ESR_CAMERA_BOUNDS_BLOCKS * 6] workspace (written
 * and read by this call only); out f32 [6]: xyz_min then xyz_max.  Wave reduction, one partial per workgroup, a final
 * one-workgroup pass; minimum and maximum do not depend on the order, so there are no atomics and the result is the
 * same bytes on every call.  n_views == 0 yields +inf / -inf.
 */
int esr_camera_bounds(const esr_camera_t *cam, const float *poses, float near_, float far_, float *partials, float *out,
                      void *stream);
/*
 * esr_ray_filter over every ray of every view, in row order, with each ray made by the device function above instead of
 * loaded from arrays (the same kernel body; everything else as esr_ray_filter says, which replaces
 * app/coarse/model/voxurfc.py:426-481 and app/fine/model/voxurff.py:463-537).  keep u8 [n_views*height*width], first_hit
 * (or NULL) i32 of that length.  The flags equal esr_ray_filter's on the rays of esr_camera_rays bit for bit.
 */
int esr_ray_filter_cameras(const esr_scene_t *scene, const float *mask_density, const esr_camera_t *cam, const float *poses,
                           int32_t mode, float far_, int32_t n_samples, uint8_t *keep, int32_t *first_hit, void *stream);

/* ------------------------------------------------------------------------- *
 * N. Stage hand-over: grid resample, mask cache, non-empty mask, density bounds
 * ------------------------------------------------------------------------- */

#define ESR_RESAMPLE_MAX_C 16           /* esr_grid_resample: the most channels per cell                                  */
#define ESR_DENSITY_BOUNDS_BLOCKS 1024  /* esr_density_bounds: the most workgroup partials it writes (6 floats each)      */

/*
 * Trilinear resample with align_corners=True of a channels-last grid: in [gx,gy,gz,C] -> out [ox,oy,oz,C] f32, C in
 * 1 .. ESR_RESAMPLE_MAX_C -- replaces F.interpolate(mode="trilinear", align_corners=True) of DenseGrid.scale_volume_grid
 * (app/utils/base/module.py:37-49) and of the fine stage's start (app/fine/fine.py:163-170) without the NCDHW copies.
 * Per axis, every operation a separately rounded binary32 one: scale = (n_in - 1) / (n_out - 1) (0 when n_out == 1),
 * src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1; the blend is
 * lx0 * (ly0 * (lz0 * v000 + lz1 * v001) + ly1 * (lz0 * v010 + lz1 * v011)) + lx1 * (the same at i1 of x), not contracted.
 * Equal sizes copy the grid bit for bit (finite values).  in and out need 4-byte alignment only and must not overlap.
 * Plain stores, no atomics: the same bytes on every call.
 */
int esr_grid_resample(const float *in, int32_t gx, int32_t gy, int32_t gz, int32_t C, float *out, int32_t ox, int32_t oy,
                      int32_t oz, void *stream);
/*
 * out[x,y,z] = max of in over the ks^3 window centred on (x,y,z), clipped to the volume -- replaces
 * F.max_pool3d(kernel_size=ks, padding=ks / 2, stride=1) of MaskCache.__init__ (module.py:92-94) on a 1-channel volume
 * [gx,gy,gz] f32.  ks odd, 1 .. 7 (else ESR_EINVAL).  Exact: bit-equal to torch for finite and infinite inputs.
 */
int esr_maxpool3d(const float *in, int32_t gx, int32_t gy, int32_t gz, int32_t ks, float *out, void *stream);
/*
 * The non-empty mask of an SDF grid [X,Y,Z] whose nodes are (xs[i], ys[j], zs[k]) (device arrays: the torch.linspace axes
 * of the grid's box) -- replaces MaskCache.forward over the meshgrid and the masked write of set_nonempty_mask
 * (app/fine/model/voxurff.py:571-593, app/coarse/model/voxurfc.py:491-513).  Per node: the march's own lookup of the pooled
 * density [mx,my,mz] in the box mask_box_host (HOST memory: min xyz then max xyz; zero padding outside),
 * a = 1 - exp(-softplus(d + act_shift)), mask_out (u8) = a >= thres; sdf (or NULL) is set to 1 where the mask is 0 and left
 * alone elsewhere.  The number of set cells is ADDED to *count_out (i64 on the device; the caller zeroes it).
 */
int esr_nonempty_mask(const float *pooled, int32_t mx, int32_t my, int32_t mz, const float *mask_box_host, float act_shift,
                      float thres, const float *xs, const float *ys, const float *zs, int32_t X, int32_t Y, int32_t Z,
                      float *sdf, uint8_t *mask_out, int64_t *count_out, void *stream);
/*
 * Bounding box of the active nodes of an alphamask density [gx,gy,gz] in the box box_host (HOST memory) -- replaces
 * compute_bbox_by_coarse_geo (app/coarse/coarse.py:152-182).  Node (i,j,k) lies at (xs[i], ys[j], zs[k]) (device arrays of
 * gx, gy, gz floats: lo * (1 - t) + hi * t over t = linspace(0, 1, n), the reference's dense_xyz per axis); its density is
 * looked up there as above, a = 1 - exp(-softplus(d + act_shift)), and it is active when a > thres (strict).  out6 f32 [6]:
 * the minimum then the maximum of the active nodes' coordinates (+inf / -inf when none is active); the number of active
 * nodes is ADDED to *count_out (i64 on the device; the caller zeroes it).  part: f32 [ESR_DENSITY_BOUNDS_BLOCKS * 6]
 * workspace.  Minimum, maximum and the integer count do not depend on the order: the same bytes on every call.
 */
int esr_density_bounds(const float *density, int32_t gx, int32_t gy, int32_t gz, const float *box_host, float act_shift,
                       float thres, const float *xs, const float *ys, const float *zs, float *part, float *out6,
                       int64_t *count_out, void *stream);

/* ------------------------------------------------------------------------- *
 * O. Surface components (connected components of a mesh, per-component sums)
 * ------------------------------------------------------------------------- */

/*
 * Connected components of the selected faces of a triangle mesh -- what a user of the reference does on the host with
 * trimesh.split / scipy.sparse.csgraph after trimesh.Trimesh(vertices, triangles) (app/fine/pdra.py:781, lts.py:659,
 * fine.py:632).  triangles [n_faces,3] i64 with every id in [0, n_vertices) (the host wrapper checks: no kernel sees an id
 * out of range); face_mask [n_faces] u8 or NULL (every face selected).
 * Connectivity is VERTEX connectivity: two selected faces are connected iff they share a vertex id (not: an edge).  An
 * unselected face links nothing.  A component is named by the smallest vertex id it contains; the components that own at
 * least one selected face are numbered 0 .. K-1 in increasing order of that id, so every output below is an exact,
 * order-independent function of the input.
 *
 * esr_cc_link: parent [n_vertices] i32 = v, then for every selected face union(v0, v1) and union(v0, v2), lock-free (the
 * larger root is hooked under the smaller one by an agent-scope compare-and-swap; parents only decrease).
 * esr_cc_flatten (its own launches: the boundary publishes parent): parent[v] = the root of v = the smallest id of v's
 * component; owner [n_vertices] i32 = 1 for a root that owns a selected face, else 0.  rank = cumsum(owner) - 1 is the
 * caller's (one device-wide scan), K = the last cumsum.
 * esr_cc_face_labels: face_label [n_faces] i32 = rank[parent[triangles[f,0]]], -1 for an unselected face.
 * ESR_ECAP for n_vertices >= 2^31; ESR_EINVAL for a pointer that is not aligned to its element.  n_faces == 0 is valid.
 */
int esr_cc_link(const int64_t *triangles, const uint8_t *face_mask, int64_t n_faces, int64_t n_vertices, int32_t *parent,
                void *stream);
int esr_cc_flatten(const int64_t *triangles, const uint8_t *face_mask, int64_t n_faces, int64_t n_vertices,
                   int32_t *parent, int32_t *owner, void *stream);
int esr_cc_face_labels(const int64_t *triangles, const uint8_t *face_mask, int64_t n_faces, const int32_t *parent,
                       const int32_t *rank, int32_t *face_label, void *stream);
/*
 * Sums over the faces of each component.  vertices [V,3] f64; face_label [n_faces] i32 in [-1, n_components) (-1: the face
 * takes no part); attr [V,n_attr] f32 with n_attr in 1 .. 4, or NULL with n_attr = 0.  Outputs (all written by this call,
 * no caller initialisation), per component: n_faces_out i64; area f64 = sum 0.5 |(b - a) x (c - a)|; area_centroid f64 [3]
 * = sum area * ((a + b) + c) / 3; bbox_min, bbox_max f64 [3] over the face vertices (+inf / -inf for a component without
 * faces); with attr: area_attr f64 [n_attr] = sum area * (((x_a + x_b) + x_c) / 3) per channel and peak f32 = the largest
 * attribute value at a face vertex (NULL otherwise).  Counts, box and peak are exact; the f64 sums are atomic adds of
 * per-wave / per-block partial sums, so their last bits depend on the order of arrival.
 * per_lane_atomics != 0 selects the form without the in-wave reduction (one atomic per face and quantity): the same
 * results, kept for timing the reduction against it.
 */
int esr_cc_stats(const double *vertices, const int64_t *triangles, const int32_t *face_label, int64_t n_faces,
                 int64_t n_components, const float *attr, int32_t n_attr, int32_t per_lane_atomics, int64_t *n_faces_out,
                 double *area, double *area_centroid, double *bbox_min, double *bbox_max, double *area_attr, float *peak,
                 void *stream);

/* ------------------------------------------------------------------------- *
 * P. PDRA ray re-split (update_ray_groups): decide, pack, count, partition
 * ------------------------------------------------------------------------- */

#define ESR_PARTITION_BLOCK 1024      /* flags (rows) per tile of esr_flag_scan_bits / esr_index_partition_bits: 16 words   */
#define ESR_PARTITION_SCAN_TILE 1024  /* tile counts per trip of the one-block scan launch of esr_flag_scan_bits            */

/* What app/fine/pdra.py:912-925 prints, plus the counts.  Minima and maxima run over the non-NaN elements ([n,3] values,
 * not per-ray maxima) of all rays, of the set (uncertain) rays and of the clear (certain) rays; an empty group holds +inf
 * and -inf.  -0.0 orders below +0.0.  n_nan = rays with a NaN channel (they are clear, so n_set + n_clear = n). */
typedef struct esr_regroup_stats_t {
    int64_t n_set, n_clear, n_nan;
    float min_all, max_all, min_set, max_set, min_clear, max_clear;
} esr_regroup_stats_t;

/*
 * flags[i] = max_c emission[i][c] > k_val, compared as binary32 -- app/fine/pdra.py:911
 * (uncert_masks = torch.max(emission, dim=-1)[0] > k_val) with the statistics of :912-925 in the same pass.  emission
 * [n,3] f32, flags u8 [n] (any alignment), stats: DEVICE memory.  A ray with a NaN channel is not set (torch.max propagates
 * the NaN and NaN > k is false).  accumulate == 0: *stats is overwritten; accumulate != 0: the call merges into what
 * *stats holds (chunk by chunk over one flag vector, no [n,3] buffer).  Counts, minima and maxima are exact and do not
 * depend on the order of arrival.
 * All entries of this section: n == 0 is success and touches no pointer; n >= 2^31 is ESR_ECAP; a NULL or
 * misaligned pointer is ESR_EINVAL; everything is enqueued on `stream` and nothing waits on the host.
 */
int esr_emit_decide(const float *emission, int64_t n, float k_val, uint8_t *flags, esr_regroup_stats_t *stats,
                    int accumulate, void *stream);
/*
 * The same flags as packed 64-bit words: what the scan and the partition below read, and what a re-split under data
 * parallelism all-reduces.  Packed format: bit b of word w is the flag of ray 64 w + b, bit 0 the least significant; the
 * bits at and above n in the last word are 0; words u64 [ceil(n / 64)], 8-byte aligned.  Shares of a flag vector that are cut
 * at word boundaries combine under an integer SUM all-reduce of the words (zero outside a rank's share).
 *
 * esr_emit_decide_bits: the decision and the statistics of esr_emit_decide (the same comparison, NaN rule, counts, minima and
 * maxima, the same `accumulate`), written as ceil(n / 64) WHOLE words, one wave ballot each, instead of n bytes: a chunk of a
 * longer flag vector starts on a word (a multiple of 64 rays), where a chunk of esr_emit_decide may start at any ray.
 */
int esr_emit_decide_bits(const float *emission, int64_t n, float k_val, uint64_t *words, esr_regroup_stats_t *stats,
                         int accumulate, void *stream);
/* flags u8 [n] (any alignment) -> words: a non-zero byte is a set bit.  Writes ceil(n / 64) whole words, the tail clear. */
int esr_flags_pack(const uint8_t *flags, int64_t n, uint64_t *words, void *stream);
/* words -> flags u8 [n]: exactly 0 or 1 per byte */
int esr_flags_unpack(const uint64_t *words, int64_t n, uint8_t *flags, void *stream);
/*
 * Counts for the partition below (two launches: a count per tile, then a one-block exclusive scan).  block_offsets i64
 * [ceil(n / ESR_PARTITION_BLOCK)]: the number of set flags in front of tile b (a tile is ESR_PARTITION_BLOCK flags = 16
 * words, counts are popcounts); totals i64 [2] = (set, clear).  Replaces the counting inside the boolean indexings of
 * utils2/utils.py:257-267.
 */
int esr_flag_scan_bits(const uint64_t *words, int64_t n, int64_t *block_offsets, int64_t *totals, void *stream);
/*
 * The stable two-way partition of RayGroupManager.filter (utils2/utils.py:264-267): set_out [totals[0]] = the rows whose flag
 * is set and clear_out [totals[1]] = the rows whose flag is clear, both in input order.  rows i64 [n] is not written; set_out
 * and clear_out must not alias it or each other; clear_out may point into the middle of a larger buffer (the certain group's
 * new vector, behind its old contents).  words and block_offsets as esr_flag_scan_bits left them.  An output of size 0 may be
 * NULL: the CALLER guarantees that a NULL output's side is empty (totals says so); the kernel cannot check it and skips the
 * stores of rows that would go to a NULL output, only two NULL outputs are ESR_EINVAL.
 */
int esr_index_partition_bits(const int64_t *rows, const uint64_t *words, const int64_t *block_offsets, int64_t n,
                             int64_t *set_out, int64_t *clear_out, void *stream);
/*
 * *out = the merge of parts [n_parts] (DEVICE memory, records as esr_emit_decide leaves them): counts are added, minima and
 * maxima are taken in esr_emit_decide's total order (-0.0 below +0.0), a group that is empty in every part keeps +inf / -inf.
 * One launch of one wave; `out` may be one of the parts.  n_parts == 0 is success and touches no pointer.
 */
int esr_regroup_stats_merge(const esr_regroup_stats_t *parts, int64_t n_parts, esr_regroup_stats_t *out, void *stream);

/* ------------------------------------------------------------------------- *
 * Q. LPIPS (AlexNet) image metric -- replaces utils2/metric.py:15-28 (rgb_lpips: lpips.LPIPS(net="alex", version "0.1"),
 *    normalize=True, eval mode).  Channels-last float32 activations [N,H,W,C]; csrc/lpips.hip.
 * ------------------------------------------------------------------------- */

#define ESR_CONV_KC 32           /* the reduction index of a packed convolution weight is padded to a multiple of this */

/* floats of a packed [Cout,Cin,kh,kw] weight: roundup(Cin kh kw, ESR_CONV_KC) * Cout; ESR_EINVAL for a size < 1 */
int64_t esr_conv_packed_floats(int32_t Cout, int32_t Cin, int32_t kh, int32_t kw);
/*
 * w [Cout,Cin,kh,kw] f32 (torch's conv2d layout) -> packed [Kp][Cout] f32, the B operand order of v_mfma_f32_32x32x2_f32
 * (reduction index slowest, output channel on the lane):
 *   packed[k][n] = w[n][c][ky][kx] for k = (ky kw + kx) Cin + c < Cin kh kw, and 0.0 for the rows up to
 *   Kp = roundup(Cin kh kw, ESR_CONV_KC)
 * Once per weight, at load time.  The zero rows are exact: they add fma(0, 0, acc) = acc.  ESR_EINVAL for a NULL pointer
 * or a size < 1, ESR_ECAP for more than 2^31 packed floats.
 */
int esr_conv_pack(const float *w, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, float *packed, void *stream);
/*
 * y = relu(conv2d(x, w, b, stride, padding = pad)) as an implicit GEMM on v_mfma_f32_32x32x2_f32 (f32 operands, f32
 * accumulation).  x [N,H,W,Cin], y [N,Ho,Wo,Cout] with Ho = (H + 2 pad - kh) / stride + 1 (floor), Wo alike; packed as
 * esr_conv_pack left it (16-byte aligned); bias [Cout].  GEMM: M = N Ho Wo output pixels, N = Cout, K = Cin kh kw.
 *
 * affine (or NULL) [2 Cin] f32 DEVICE memory, shift then scale: the convolution reads s = ((2 x - 1) - shift[c]) / scale[c]
 * in place of x -- each step a separately rounded binary32 operation, the last a correctly rounded division -- and the
 * zero padding applies to s, not to x (the scaling layer of LPIPS in front of its first convolution).
 *
 * Order of the arithmetic, which the result's bits follow from: per output value ONE chain
 *   acc = +0;  for k = 0, 1, ... Kp-1 (k = (ky kw + kx) Cin + c, ascending):  acc = fmaf(patch[k], packed[k][n], acc)
 *   y = acc + bias[n];  y = y > 0 ? y : 0 (NaN stays NaN)
 * where patch[k] is 0 for a tap outside the image and for k >= K.  No split-K and no atomics: the bits of a value do not
 * depend on the tile, the image of the batch or the call it is computed in.
 *
 * ESR_EINVAL (nothing written): a NULL or (packed) misaligned pointer, Cout % 32 != 0, any size < 1, pad < 0, an empty
 * output (H + 2 pad < kh or W + 2 pad < kw).  ESR_ECAP (nothing written): x, y or packed with more than 2^31 elements.
 */
int esr_conv_relu(const float *x, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *packed, const float *bias,
                  int32_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, const float *affine, float *y,
                  void *stream);
/*
 * F.max_pool2d(kernel_size = k, stride = stride), floor mode, no padding, on [N,H,W,C] f32: y [N,Ho,Wo,C] with
 * Ho = (H - k) / stride + 1.  A NaN in the window gives NaN, as in torch; otherwise bit-equal to torch.  ESR_EINVAL for a
 * size < 1 or H, W < k; ESR_ECAP for more than 2^31 elements.  (LPIPS's AlexNet: k = 3, stride = 2.)
 */
int esr_maxpool_nhwc(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, float *y,
                     void *stream);
/*
 * One layer's LPIPS term.  f0, f1 [npix,C] f32 (the same tap of the two images), lin_w [C] f32 (the 1x1 "lin" weight):
 *   per pixel, in binary32:  s_i = sum_c f_i[c]^2,  den_i = sqrtf(s_i) + 1e-10f,  n_i[c] = f_i[c] / den_i,
 *                            d[c] = n_0[c] - n_1[c]
 *     (s_i: lane l of the pixel's wave adds c = l, l + 64, ... in that order, product and sum separately rounded, then a
 *      butterfly over the 64 lanes with offsets 32, 16, ... 1; sqrtf and the divisions correctly rounded)
 *   in binary64 from there:  out[0] = (sum_pixels sum_c (double)lin_w[c] * ((double)d[c] * (double)d[c])) / npix
 * A pixel whose features are all zero has n = 0 / 1e-10 = 0: never NaN.  Swapping f0 and f1 gives the same bits, f0 == f1
 * gives exactly 0.0.  Sums in a fixed order (lane, wave, workgroup, then one workgroup over partials
 * [ESR_METRICS_BLOCKS] f64): no float atomics, the same bits on every call.  ESR_EINVAL for a NULL pointer, npix < 1 or
 * C < 1; ESR_ECAP for npix * C > 2^31.
 */
int esr_lpips_layer(const float *f0, const float *f1, int64_t npix, int32_t C, const float *lin_w, double *partials,
                    double *out, void *stream);

/* ------------------------------------------------------------------------- *
 * R. Surface rasteriser: the exported mesh z-buffered into camera views (face, depth, source masks).  No reference
 *    counterpart: the reference reads a view's source masks from the dataset's annotations (data/esrnerf/esrnerf.py
 *    `areas` / `em_masks`) or renders them (app/fine/pdra.py:684-688)
 * ------------------------------------------------------------------------- */

/*
 * Z-buffer of the views [v0, v1) of cam.  vertices [n_vertices,3] f64 (world), triangles [n_faces,3] i64 (an index outside
 * [0, n_vertices) is the caller's error: such a face reads nothing and covers nothing), w2c [cam.n_views,12] f64: each
 * view's world-to-camera matrix, row-major 3x4.  All of the following in binary64, each operation rounded on its own:
 *   p_c = W (p, 1);  a face with ANY vertex at z_c <= z_near is dropped and counted (there is no near-plane clipping);
 *   u = fx x_c / z_c + cx, v = fy y_c / z_c + cy;  the centre of pixel (i, j) is (i + 0.5, j + 0.5);
 *   A = (u1 - u0)(v2 - v0) - (v1 - v0)(u2 - u0);  b_k = E_k / A with E_k the same expression on the centre and the other
 *   two vertices;  covered iff A is finite, A != 0 and every b_k >= 0 (inclusive edges, both windings, no culling);
 *   z = 1 / ((b_0 / z_0 + b_1 / z_1) + b_2 / z_2), rounded once to binary32.
 * zbuf u64 [(v1 - v0), height * width] (indexed by view - v0): per pixel the minimum over the covering faces of
 * (binary32 bits of z) << 32 | face id, all ones where no face covers: the nearest face, on equal binary32 depth the smaller
 * id; 64-bit atomic minima, so the same bytes on every call.  n_dropped i32 [(v1 - v0)].  Both are cleared first.
 * A face whose clamped bounding box holds more than big_px pixel centres is rasterised by a whole workgroup instead of one
 * lane (the same expressions: the words do not depend on big_px).  queue i64 [queue_cap] and queue_count u64 [1] are
 * workspace; queue_cap >= (v1 - v0) * n_faces, so that no face can be lost (else ESR_ECAP).
 * ESR_EINVAL: a NULL or misaligned pointer, a bad view range, z_near not in (0, inf), big_px < 0, a negative size;
 * ESR_ECAP: n_faces or n_vertices >= 2^31.  Nothing is written in either case.  v0 == v1 launches nothing; n_faces == 0
 * only clears.
 */
int esr_raster_faces(const esr_camera_t *cam, const double *w2c, int32_t v0, int32_t v1, const double *vertices,
                     int64_t n_vertices, const int64_t *triangles, int64_t n_faces, double z_near, int64_t big_px,
                     uint64_t *zbuf, int32_t *n_dropped, int64_t *queue, int64_t queue_cap, uint64_t *queue_count,
                     void *stream);
/* zbuf u64 [n_px] (any number of views) -> face i32 [n_px]: the word's low half, -1 where empty; depth f32 [n_px]: the
 * word's high half as binary32, +inf where empty.  Plain stores.  ESR_ECAP for n_px >= 2^31. */
int esr_raster_resolve(const uint64_t *zbuf, int64_t n_px, int32_t *face, float *depth, void *stream);
/*
 * Per-view masks of edit conditions from a face image.  face i32 [n_views,n_px] (esr_raster_resolve), face_source i32
 * [n_faces] (-1: in no source), cond_of_source i32 [n_sources] (-1: in no condition).  masks f32 [n_views,n_cond,n_px]:
 * 1 where the pixel's face belongs to a source of that condition, else 0 -- every element written; a pixel that is empty,
 * whose face has no source or whose source has no condition is 0 in every mask.  pixels i64 [n_views,n_sources]: the
 * visible pixels of every source (integer atomics: exact).  n_cond <= ESR_RELIGHT_MAX_COND (else ESR_ECAP).
 */
int esr_source_masks(const int32_t *face, int32_t n_views, int64_t n_px, const int32_t *face_source, int64_t n_faces,
                     const int32_t *cond_of_source, int32_t n_sources, int32_t n_cond, float *masks, int64_t *pixels,
                     void *stream);

/* ------------------------------------------------------------------------- *
 * S. Surface simplification by quadric vertex clustering (esr_nerf_amd/mesh.py: simplify).  No reference counterpart:
 *    the reference hands the raw marching-cubes mesh to trimesh (app/fine/pdra.py:781)
 * ------------------------------------------------------------------------- */

#define ESR_SIMPLIFY_MAX_C 16     /* most attribute channels per vertex */
#define ESR_SIMPLIFY_DEBUG 15     /* doubles per cluster of the debug output */

/*
 * The definition.  Input: vertices [V,3] f64 (finite), triangles [F,3] i64, a cell size h > 0, lam > 0, optionally attr
 * [V,C] f32 with 1 <= C <= ESR_SIMPLIFY_MAX_C.  All arithmetic is binary64, every operation rounded on its own.
 *   grid      o = the per-axis minimum of the vertices; the cell of v is floor((v - o) / h) per axis, at most 2^21 - 1
 *             cells on an axis; a cluster is an occupied cell, clusters are numbered by ascending key x << 42 | y << 21 | z;
 *             g_k = o + (c_k + 0.5) h is the centre of cluster k's cell.  Everything below uses r = v - g_k (one rounding)
 *   members   M_k; xbar_k = (sum r) / |M_k|, clamped into the cell box [-h/2, h/2]^3
 *   faces     I_k = the faces with at least one corner in k, each counted once.  For corners a, b, c:
 *             n = (b - a) x (c - a) (not normalised: the quadric is weighted by area^2), d = -n . a,
 *             s = |b - a|^2 |c - a|^2, w = |n| / 2
 *             A = sum n n^T, b = sum n d, c = sum d d, S = sum s,
 *             P = sum w sum_{corners of f in k} attr[corner], W = sum w #corners of f in k
 *   position  S == 0: y = xbar.  Otherwise (A + lam S I) y* = -b + lam S xbar (SPD, condition number <= 1 + 1 / lam as
 *             tr A <= S), then y = xbar + t (y* - xbar) with the largest t in [0, 1] that keeps y in the box.  The new
 *             vertex is g_k + y
 *   attribute float(P / W); for W == 0 the attribute of the member with the smallest id
 *   faces'    corners -> clusters; a face with two equal corners is dropped; among the faces with the same SET of three
 *             clusters, whatever their winding, the smallest face id is kept, with its own winding and in its order;
 *             clusters that no kept face names are dropped and the rest renumbered in ascending order
 * The sums run in a fixed order (the header of csrc/simplify.hip): no atomics, the same bytes on every call for a fixed
 * `big`.  Sorting, scanning and allocation are the caller's (torch); the entry points below are the arithmetic.
 * Every entry: ESR_EINVAL for a NULL or misaligned pointer or a negative size, ESR_ECAP for n_vertices or n_faces >= 2^31;
 * nothing is launched in either case.  An index outside its array is the caller's error: it is skipped, never followed.
 */

/* keys i64 [n_vertices] = x << 42 | y << 21 | z of floor((v - origin) / h); origin f64 [3] (device) */
int esr_simplify_cell_keys(const double *vertices, int64_t n_vertices, const double *origin, double h, int64_t *keys,
                           void *stream);
/* vertex_cluster i32 [n_vertices]: the cluster of every vertex.  pairs i64 [3 n_faces]: per corner (cluster << 32 | face),
 * INT64_MAX for a corner whose cluster an earlier corner of the face has; sorted, they are every cluster's incident faces
 * by ascending id */
int esr_simplify_pair_keys(const int64_t *triangles, int64_t n_faces, const int32_t *vertex_cluster, int64_t n_vertices,
                           int64_t *pairs, void *stream);
/*
 * The per-cluster pass: a cluster's sums, mean, solve, clip and attributes in one kernel.  cluster_keys i64 [n_clusters] ascending;
 * member_ids i64 [n_vertices]: the vertex ids sorted by cluster (stable), member_start i64 [n_clusters + 1] its segments;
 * pairs i64 [n_pairs]: the sorted pair keys (an INT64_MAX tail may follow the real pairs inside n_pairs: it lies behind
 * every segment and is never read), pair_start i64 [n_clusters + 1] its segments, clamped to n_pairs.
 * positions f64 [n_clusters,3]; attr_out f32 [n_clusters,n_attr] (n_attr == 0: attr and attr_out unused); debug f64
 * [n_clusters,ESR_SIMPLIFY_DEBUG] or NULL: A00 A01 A02 A11 A12 A22, b0 b1 b2, c, S, W, xbar0 xbar1 xbar2.
 * A cluster of more than `big` (>= 1) pairs or members is summed by a workgroup in a fixed-shape tree instead of one lane
 * (a second launch of the same call, whose workgroups pass the smaller clusters by).
 * ESR_EINVAL also for h or lam not in (0, inf), big < 1, n_pairs > 3 n_faces, n_clusters > n_vertices; ESR_ECAP also for
 * n_attr > ESR_SIMPLIFY_MAX_C.
 */
int esr_simplify_clusters(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces,
                          const int32_t *vertex_cluster, const int64_t *cluster_keys, int64_t n_clusters,
                          const int64_t *member_start, const int64_t *member_ids, const int64_t *pair_start,
                          const int64_t *pairs, int64_t n_pairs, const double *origin, double h, double lam,
                          const float *attr, int32_t n_attr, int64_t big, double *positions, float *attr_out,
                          double *debug, void *stream);
/* key_hi i64 [n_faces] = smallest cluster << 32 | middle cluster, INT64_MAX for a face with two equal corners;
 * key_lo i32 [n_faces] = the largest cluster (0 for a dropped face) */
int esr_simplify_face_keys(const int64_t *triangles, int64_t n_faces, const int32_t *vertex_cluster, int64_t n_vertices,
                           int64_t *key_hi, int32_t *key_lo, void *stream);
/* order i64 [n_faces]: the face ids sorted by (key_hi, key_lo, id).  keep u8 [n_faces] = 1 for the first face of every run
 * of equal keys that is not INT64_MAX, else 0; used u8 [n_clusters] = 1 for the clusters a kept face names, else 0 */
int esr_simplify_keep(const int64_t *order, const int64_t *key_hi, const int32_t *key_lo, int64_t n_faces,
                      const int64_t *triangles, const int32_t *vertex_cluster, int64_t n_vertices, int64_t n_clusters,
                      uint8_t *keep, uint8_t *used, void *stream);

/* ------------------------------------------------------------------------- *
 * T. Ray casting against the surface (esr_nerf_amd/raycast.py): a linear BVH over the faces and a nearest-hit / any-hit
 *    walk.  No reference counterpart: the reference hands the mesh to trimesh (app/fine/pdra.py:781)
 * ------------------------------------------------------------------------- */

/*
 * One internal node, 64 bytes: the links and the boxes of its TWO CHILDREN (a step of the walk reads one record).
 *   box[k]    child k's box, binary32, lo x y z then hi x y z, rounded outward: every float64 coordinate of every vertex
 *             below the child lies in [lo, hi].  An empty box is lo = +inf, hi = -inf
 *   child[k]  >= 0: an internal node; < 0: a leaf, and ~child[k] is its face id.  Leaves have no record of their own
 *   parent    2 * (the parent's index) + (which child of it this node is); -1 for the root, node 0
 *   pad       0
 * A mesh of F >= 2 faces has F - 1 nodes and F leaves, one face each; F == 1 has no node (the one face is the tree).
 */
typedef struct __attribute__((aligned(16))) esr_bvh_node {
    float box[2][6];
    int32_t child[2];
    int32_t parent;
    int32_t pad;
} esr_bvh_node_t;

/*
 * Conventions of this section.  vertices [n_vertices,3] f64, triangles [n_faces,3] i64 (a face that names a vertex outside
 * [0, n_vertices) reads nothing and is never hit).  Every entry: a size of 0 succeeds and touches no pointer; ESR_EINVAL
 * for a negative size or a NULL or misaligned pointer (f64 / i64: 8 bytes, nodes: 16, the rest: 4); ESR_ECAP for a size
 * >= 2^31; nothing is launched in either case.  Everything is enqueued on `stream`, nothing waits on the host.  Sorting and
 * allocation are the caller's (torch).  The same input gives the same bytes on every call.
 */

/*
 * Per face f, all in binary64, each operation rounded on its own:
 *   lo, hi = the per-axis minimum / maximum of the three vertices;  boxes f32 [n_faces,6] = lo rounded DOWN to binary32,
 *   hi rounded UP (the nearest binary32, stepped once by nextafter where that lies on the wrong side)
 *   per axis  c = 0.5 lo + 0.5 hi,  ext = scene_hi - scene_lo,
 *             cell = ext > 0 ? floor(((c - scene_lo) / ext) * 2097152) : 0, clamped to [0, 2^21 - 1]
 *   keys i64 [n_faces] = the Morton code of the cells: bit k of cell x is bit 3 k + 2, of y 3 k + 1, of z 3 k (63 bits)
 * scene_box f64 [6] (device): lo x y z, hi x y z of the mesh's finite vertices.  A face with a vertex that is not finite
 * (or outside the vertex array) gets the key 2^63 - 1 and the empty box.
 */
int esr_bvh_keys(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces,
                 const double *scene_box, int64_t *keys, float *boxes, void *stream);
/*
 * The binary radix tree (Karras 2012) over sorted_keys i64 [n_faces] ascending; order i64 [n_faces] is the face id at
 * every sorted position.  Position i stands for the 95-bit string (key, i): equal keys differ in their position.  Node i
 * covers the largest range of positions around i whose strings share a longer prefix than with the position just outside;
 * it splits where the first differing bit changes; a child that is one position is a leaf.  The left child (0) holds the
 * smaller positions.  Writes child, parent and pad of nodes [n_faces - 1] (not the boxes) and leaf_parent i32 [n_faces]: the
 * `parent` word of every leaf, by sorted position.  One lane per node.  n_faces < 2 writes nothing.
 */
int esr_bvh_tree(const int64_t *sorted_keys, const int64_t *order, int64_t n_faces, esr_bvh_node_t *nodes,
                 int32_t *leaf_parent, void *stream);
/*
 * The boxes of the nodes, bottom-up: one lane per leaf stores its box (boxes [order[i]]) in its parent's record, fences
 * (device scope) and counts itself at the parent; the first to arrive ends, the second takes the union of the two boxes
 * and climbs on.  No lane waits for another.  Minimum and maximum are exact, so the bytes do not depend on the order of
 * arrival.  counters i32 [n_faces - 1] is workspace, zeroed by the call; root_box f32 [6] receives the box of the whole tree
 * (n_faces == 1: the face's box).
 */
int esr_bvh_fit(esr_bvh_node_t *nodes, const int32_t *leaf_parent, const int64_t *order, const float *boxes,
                int64_t n_faces, int32_t *counters, float *root_box, void *stream);
/*
 * Rays against the mesh through the tree, one lane per ray.  rays_o, rays_d f64 [n_rays,3]; d is not normalised and t is in
 * units of d.  t_min, t_max f64 [n_rays] or NULL (then t_min_all / t_max_all for every ray); skip_face i32 [n_rays] or NULL:
 * a face the ray never hits (-1: none).  The triangle test, binary64, every operation rounded on its own, in this order:
 *   e1 = b - a, e2 = c - a, p = d x e2, det = (e1.x p.x + e1.y p.y) + e1.z p.z, s = o - a, q = s x e1
 *   u = ((s.x p.x + s.y p.y) + s.z p.z) / det, v = ((d.x q.x + d.y q.y) + d.z q.z) / det,
 *   t = ((e2.x q.x + e2.y q.y) + e2.z q.z) / det, w = (1 - u) - v;   (x x y).x = x.y y.z - x.z y.y, and cyclically
 *   a hit iff det is finite and not 0, u >= 0, v >= 0, w >= 0 and t_min < t <= t_max (both windings; a face of zero area
 *   or one the ray lies in has det == 0)
 * any_hit == 0: face i32 [n_rays] = the face of the smallest t, among equal t the smallest id, -1 for none; t f64 [n_rays]
 * (+inf for none); bary f64 [n_rays,2] = u, v (0 for none): the weights of the face's second and third vertex.  The answer
 * does not depend on the order of the walk: a box is entered when its entry distance is <= the best t so far.
 * any_hit == 1: hit u8 [n_rays] = 1 iff some face is hit; the walk ends at the first.  (The outputs of the other mode are
 * unused and may be NULL.)  stats i32 [n_rays,2] or NULL: boxes tested, triangles tested.
 * A ray with a component of o or d that is not finite hits nothing, and so does one whose interval has a NaN end.  A
 * component of d that is 0 only asks whether o lies between the box's corners on that axis.
 * The walk keeps no stack: one bit per level (which child was entered first) in two registers covers the 63 + 31 levels
 * the tree can have, and parent links lead back up.
 */
int esr_bvh_cast(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                 const int64_t *triangles, const double *rays_o, const double *rays_d, int64_t n_rays,
                 const double *t_min, const double *t_max, double t_min_all, double t_max_all, const int32_t *skip_face,
                 int32_t any_hit, int32_t *face, double *t, double *bary, uint8_t *hit, int32_t *stats, void *stream);

/* ------------------------------------------------------------------------- *
 * U. Surface lighting (esr_nerf_amd/sources.py: direct_light, lit_view): the light that leaves the emissive sources of the
 *    exported surface and reaches a surface point directly -- reflected once by the Disney BRDF of the light-transport
 *    stage (the model's `emo` component, app/fine/model/esrnerf.py:565-572, app/utils/pbr/functions.py:108-173) or as
 *    irradiance.  An addition: the reference has no counterpart on a mesh
 * ------------------------------------------------------------------------- */

#define ESR_SURFACE_LIGHT_MAX_SLOTS 64   /* most sample slots of a source (ESR_ECAP beyond it: a source's slots sit in one wave) */

/*
 * Scene.  nodes / n_faces / vertices / n_vertices / triangles: the tree and the mesh exactly as esr_bvh_cast takes them (the
 * same pointer and alignment rules, the same n_faces == 0, 1, > 1 cases).
 * Lights.  n_sources sources (S) of `slots` sample slots each (Kp): a power of two, 1 <= Kp <= 64, the same for every
 * source; slot-major arrays
 *   l_point f64 [S,Kp,3]   l_normal f64 [S,Kp,3] (unit length)   l_weight f64 [S,Kp]   l_radiance f32 [S,Kp,3]   l_face i32 [S,Kp]
 * A slot with l_weight == 0 is unused: nothing else of it is read.
 * Points.  n_points points (P): p_point f64 [P,3], p_normal f32 [P,3] (unit length); in mode 0 also p_base f32 [P,3], p_rough
 * f32 [P], p_metal f32 [P] and p_wo f32 [P,3], the unit direction towards the viewer (unused and may be NULL in mode 1).
 *
 * Per point x (normal n), source s and slot k with point y, normal g, weight A, radiance E, face f -- binary64, every
 * operation rounded on its own (no contraction), in this order:
 *   d = y - x;  r2 = (d0 d0 + d1 d1) + d2 d2;  r = sqrt(r2);  w_i = d_i / r;
 *   cos_l = -((g0 w0 + g1 w1) + g2 w2);  cos_x = (n0 w0 + n1 w1) + n2 w2   (the binary32 normal widened)
 *   the slot is SILENT -- it contributes +0.0 and no segment is walked -- if A == 0 or if any of r2 > 0, cos_l > 0,
 *   cos_x > 0 is false (a NaN makes a comparison false).  Otherwise
 *   G = (cos_l A) / max(r2, A)        (max of two numbers: the one that is not a NaN)
 *   The clamp max(r2, A) is the usual bound of a point sample of an area light: within about one sample spacing of a
 *   source the estimate is LOW.
 *   occluded iff esr_bvh_cast's any-hit walk finds a face: o = x, d = d, eps < t <= 1 - eps (1 - eps rounded once),
 *   skip_face = f.  If not occluded, per channel c
 *     mode 0 (reflected radiance)  term_c = (((double)R_c (1 / (2 pi))) G) (double)E_c
 *            R = the binary32 Disney reflection of the light-transport combine for base, rough, metal, n, wi = (float)w, wo:
 *            it carries (n . wi) 2 pi, the weight of the hemisphere estimator, which 1 / (2 pi) (binary64, 1 / (2 pi) with
 *            pi rounded to binary64) takes back out
 *     mode 1 (irradiance)          term_c = (cos_x G) (double)E_c
 * out f32 [P,S,3]: out[p,s,c] = the binary32 rounding of the balanced pairwise binary64 sum of the Kp terms of (p, s):
 * slots 2 j and 2 j + 1 are added first, then adjacent pairs of those sums, and so on.  The order is fixed and there are
 * no atomics: the same input gives the same bytes on every call.
 * seen u8 [P,S,Kp] or NULL: 0 silent, 1 walked and not occluded, 2 walked and occluded.
 *
 * n_points == 0 or n_sources == 0 succeeds and touches no pointer.  ESR_EINVAL: a NULL struct, a negative size, a mode
 * other than 0 and 1, slots < 1 or not a power of two, eps not in [0, 0.5), a NULL or misaligned pointer (f64 / i64: 8
 * bytes, nodes: 16, the rest: 4).  ESR_ECAP: a size >= 2^31, slots > ESR_SURFACE_LIGHT_MAX_SLOTS.  Nothing is launched in
 * either case.  One launch on `stream`; nothing waits on the host.
 * Layout: Kp adjacent lanes work on one (point, source), a wave holds 64 / Kp points; the point stays in registers over the
 * sources; nothing of size P S Kp reaches memory but `seen`.
 */
typedef struct esr_surface_light {
    const esr_bvh_node_t *nodes;
    int64_t n_faces;
    const double *vertices;
    int64_t n_vertices;
    const int64_t *triangles;
    int64_t n_sources;
    int32_t slots;
    int32_t mode;
    const double *l_point, *l_normal, *l_weight;
    const float *l_radiance;
    const int32_t *l_face;
    int64_t n_points;
    const double *p_point;
    const float *p_normal, *p_base, *p_rough, *p_metal, *p_wo;
    double eps;
    float *out;
    uint8_t *seen;
} esr_surface_light_t;

int esr_surface_light(const esr_surface_light_t *args, void *stream);

/* ------------------------------------------------------------------------- *
 * V. Environment light on the surface (esr_nerf_amd/sources.py: environment_light, vertex_env_radiance, lit_view): the
 *    light of the spherical-Gaussian environment map that reaches a surface point -- directly where the hemisphere ray
 *    leaves the mesh, or once reflected where it hits a face with a known vertex radiance -- reflected by the Disney BRDF
 *    of the light-transport stage or as irradiance.  The reference's evaluation decomposition defines the quantity in the
 *    volume (app/fine/model/esrnerf.py:983-994: lin/env_dir = mean_r(envmap(dirs_r) alphainv_last_r R_r), lin/env_indir =
 *    mean_r(off_marched_r R_r) over the directions of diffuse_scattering_fib, app/utils/pbr/functions.py:21-32, 176-194);
 *    on a surface alphainv_last is "the ray leaves the mesh" and off_marched the radiance of the face that is hit
 * ------------------------------------------------------------------------- */

#define ESR_SURFACE_ENV_MAX_DIRS 4096    /* most directions of the table (ESR_ECAP beyond it) */
#define ESR_SURFACE_ENV_MAX_SG   64      /* most lobes of the environment (ESR_ECAP beyond it: the lobe table sits in LDS) */

/*
 * Scene.  nodes / n_faces / vertices / n_vertices / triangles: the tree and the mesh exactly as esr_bvh_cast takes them (the
 * same pointer and alignment rules; n_faces == 0 makes every ray a miss, n_faces == 1 is the tree-less case).
 * Directions.  dirs f32 [R,3], R = n_dirs unit directions: one table for all points.
 * Environment.  The raw model parameters mus f32 [J,3], lambdas f32 [J], lobes f32 [J,3], J = n_sg.
 * vertex_radiance f32 [n_vertices,3] or NULL: the radiance that leaves the surface at every vertex.
 * Points.  n_points points (P): p_point f64 [P,3], p_normal f32 [P,3] (unit length), p_face i32 [P] or NULL (the face the
 * point lies on, which its rays never hit; -1: none); in mode 0 also p_base f32 [P,3], p_rough f32 [P], p_metal f32 [P] and
 * p_wo f32 [P,3], the unit direction towards the viewer (unused and may be NULL in mode 1).
 *
 * Per point x with normal n, and per direction r with the table entry w = dirs[r]:
 *   1. flip (as diffuse_scattering_fib): s = (w0 n0 + w1 n1) + w2 n2 in binary32, every operation rounded on its own (no
 *      contraction); if s < 0 then w = -w.
 *   2. ray: o = x, d = (double)w, t_min < t <= +inf, skip_face = p_face[p].  The walk and the triangle test are
 *      esr_bvh_cast's: the any-hit walk if vertex_radiance is NULL, the nearest-hit walk otherwise.  (A point with a
 *      component that is not finite hits nothing: all its rays miss.)
 *   3. incoming radiance L.
 *      miss: the environment, binary32, every operation rounded on its own, in the order of the light-transport combine:
 *        l^_j = lobe_j / max(sqrt((lobe_j0^2 + lobe_j1^2) + lobe_j2^2), 1e-12)
 *        pre_c = sum over j ascending of mu_jc expf(|lambda_j| (((w0 l^_j0 + w1 l^_j1) + w2 l^_j2) - 1))
 *        L_c = softplus(pre_c) = pre_c > 20 ? pre_c : log1pf(expf(pre_c)), with the flipped w
 *      hit with vertex_radiance: binary64, every operation rounded on its own, with the hit's barycentrics u, v and the rows
 *        E_a, E_b, E_c of the face's three vertices:  L_c = (((1 - u) - v) E_a,c + u E_b,c) + v E_c,c
 *      hit without vertex_radiance: L = 0.
 *   4. term.
 *      mode 0 (reflected radiance)  term_c = (double)L_c (double)R_c,  R = the binary32 Disney reflection of the
 *             light-transport combine for base, rough, metal, n, wi = w, wo: it carries (n . wi) 2 pi, the weight of the
 *             uniform-hemisphere estimator
 *      mode 1 (irradiance)          term_c = (double)L_c cos_x,  cos_x = (n0 w0 + n1 w1) + n2 w2 in binary64 on the widened
 *             values
 *   5. sum, in a fixed order without atomics (the same input gives the same bytes on every call).  Kd = min(64, the next
 *      power of two >= R) adjacent lanes form the group of a point; lane k adds the terms of its directions r = k, k + Kd,
 *      ... ascending in binary64 (from +0.0); the Kd lane sums are combined by the balanced pairwise sum of section U (lanes
 *      2 j and 2 j + 1 first, then adjacent pairs of those sums, and so on) to S_c.
 *        mode 0:  out[p,c] = (float)(S_c / (double)R)
 *        mode 1:  out[p,c] = (float)((S_c (2 pi)) / (double)R), 2 pi from pi rounded to binary64
 * out f32 [P,3]; n_open i32 [P] or NULL: the exact number of directions that miss; hit u8 [P,R] or NULL: 1 where the
 * direction hits a face, else 0.
 *
 * n_points == 0 (with every other argument valid) succeeds and touches no pointer.  ESR_EINVAL: a negative size, n_dirs <
 * 1, n_sg < 1, a mode other than 0 and 1, t_min negative or NaN, a NULL or misaligned required pointer (f64 / i64: 8
 * bytes, nodes: 16, the rest: 4; an optional pointer that is given is held to the same alignment).  ESR_ECAP: n_dirs >
 * ESR_SURFACE_ENV_MAX_DIRS, n_sg > ESR_SURFACE_ENV_MAX_SG, a size >= 2^31.  Nothing is launched in either case.  One
 * launch on `stream`; nothing waits on the host.
 * Layout: a wave holds 64 / Kd points; the point stays in registers over the directions; the environment is evaluated only
 * on the lanes whose ray missed; the lobe table sits in LDS; nothing of size P R reaches memory but `hit`.
 */
int esr_surface_env(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                    const int64_t *triangles, const float *dirs, int32_t n_dirs, const float *mus, const float *lambdas,
                    const float *lobes, int32_t n_sg, const float *vertex_radiance, int64_t n_points, const double *p_point,
                    const float *p_normal, const int32_t *p_face, const float *p_base, const float *p_rough,
                    const float *p_metal, const float *p_wo, int32_t mode, double t_min, float *out, int32_t *n_open,
                    uint8_t *hit, void *stream);

/* ------------------------------------------------------------------------- *
 * W. Texture atlas of the surface (esr_nerf_amd/atlas.py: build, sample; sources.py: bake_materials, bake_irradiance,
 *    lit_view(atlas=, textures=), write_surface_obj): every face gets a chart of its own in a square atlas, the texels know
 *    their face, barycentrics and world point, and a texture is looked up bilinearly at a point of a face.  Nothing in the
 *    reference corresponds to it.
 * ------------------------------------------------------------------------- */

#define ESR_ATLAS_MIN_SIZE     64     /* smallest and                                                                  */
#define ESR_ATLAS_MAX_SIZE     8192   /* largest side W of the atlas, a power of two                                    */
#define ESR_ATLAS_MAX_LEVELS   16     /* entries of a level table (the levels themselves are at most 13: 2^13 = 8192)   */
#define ESR_ATLAS_MAX_CHANNELS 16     /* most channels of a texture (ESR_ECAP beyond it)                                */

/*
 * Layout (all integer).  W = size, g = gutter >= 1, lmin <= l <= lmax with 2^lmin >= 3 g + 2 and 2^lmax <= W.  A face of
 * level l owns one half of a square cell of side s = 2^l texels.  With local texel indices (i, j), i along x, the texel
 * centres at (i + 0.5, j + 0.5):
 *   half 0 owns the texels with i + j <= s - 1, half 1 the rest;  leg(l) = s - (3 g + 1);
 *   half 0's triangle is a = (g, g), b = (g + leg, g), c = (g, g + leg) in local texel units,
 *   half 1's the point reflection p -> (s - p.x, s - p.y) of it.
 * Footprint property: for every point p of a half's triangle the four texels (floor(p - 0.5) and + 1 per axis) of a bilinear
 * lookup are owned by that half and lie inside the cell (tests/test_atlas_host.py enumerates it).
 * A level table is int64 [ESR_ATLAS_MAX_LEVELS], indexed by the level itself.  From counts cnt_l:  n_l = ceil(cnt_l / 2) cells;
 * the groups descend with the level: rank start S_l = sum_{l' > l} cnt_l', unit start U_l = sum_{l' > l} n_l' 4^(l' - lmin)
 * in cells of side 2^lmin; the layout fits iff U_lmin + n_lmin <= (W / 2^lmin)^2.  The face at sorted rank k, S_l <= k < S_l +
 * cnt_l, r = k - S_l, has cell r >> 1 and half r & 1; its unit u = U_l + (r >> 1) 4^(l - lmin); the cell's origin is
 * (x0, y0) = 2^lmin (even bits of u, odd bits of u) (Z-order).
 *
 * Common to the entries: size, gutter, lmin, lmax as above (else ESR_EINVAL, as for a NULL or misaligned pointer -- f64 / i64:
 * 8 bytes, the rest: 4 -- or a negative size); ESR_ECAP for n_faces or n_vertices >= 2^31.  A face with a vertex id outside
 * [0, n_vertices) is read nowhere: level lmin, rot 0, its texels' point (and tex) NaN.  One launch on `stream` each; nothing
 * waits on the host; no float atomics: the same input gives the same bytes.
 *
 * esr_atlas_levels.  vertices f64 [V,3], triangles i64 [F,3].  Per face with the corners a, b, c, in binary64, every written
 * operation rounded once, no contraction:
 *   e1 = b - a, e2 = c - a, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), c2 = (n0 n0 + n1 n1) + n2 n2
 *   level[f] = the smallest l in [lmin, lmax] with (double)(leg(l)^2) (double)(leg(l)^2) >= c2 rho4, or lmax if there is none;
 *              lmin if c2 is not finite.  rho4 = (rho^2)^2 for a density of rho texels per world unit (finite, >= 0).
 *   rot[f] in {0, 1, 2}: with d_k = ((ex ex + ey ey) + ez ez) of the edge opposite corner k (c - b, c - a, b - a), the smallest
 *              k with the largest d_k (d1 > d0, then d2 > max; a NaN compares false).  The corners in the order rot, rot + 1,
 *              rot + 2 (mod 3) are the triangle's a, b, c: the longest edge becomes the hypotenuse.
 *   hist i64 [16] (device): zeroed here, then hist[l] = the faces of level l (LDS partial per block, one integer atomic per
 *              level).  level, rot i32 [F].
 *
 * esr_atlas_charts.  order i64 [F]: the faces sorted by descending level, by face id within a level (a stable sort of
 * lmax - level); counts i64 [16] [host]: hist read back.  ESR_EINVAL if the counts are negative, lie outside lmin .. lmax or do
 * not sum to n_faces; ESR_ECAP if the layout does not fit; nothing is written in either case.  One lane per rank k, f = order[k]:
 *   chart i32 [F,4]: chart[f] = (x0, y0, l | half << 8 | rot << 16, k)
 *   uv f32 [F,3,2]: corner j of the face is corner q = (j - rot) mod 3 of a, b, c; uv[f,j] = ((x0, y0) + that corner) / W
 *              (exact: W is a power of two), x first.
 *
 * esr_atlas_texels.  The same order, rot and counts (the same refusals).  One lane per texel, the texel (i, j) at index
 * j W + i:  m = the Z-order code of (i >> lmin, j >> lmin); the group l with U_l <= m < U_l + n_l 4^(l - lmin); the cell
 * (m - U_l) >> 2 (l - lmin); (i_loc, j_loc) = (i, j) mod s; half = i_loc + j_loc >= s; r = 2 cell + half;
 *   face i32 [W,W] = order[S_l + r], or -1 where there is no group or r >= cnt_l (the missing half of an odd group).
 *   With hx = 2 i_loc + 1 - 2 g, hy = 2 j_loc + 1 - 2 g in half 0 and hx = 2 (s - g) - (2 i_loc + 1), hy likewise, in half 1:
 *   beta = (double)hx / (double)(2 leg), gamma = (double)hy / (double)(2 leg): not clamped, the gutter carries the affine
 *   extension.  bary f32 [W,W,2] = (float)beta, (float)gamma: the weights of the rotated corners b and c.
 *   flags u8 [W,W]: bit 0 = inside the triangle, hx >= 0 and hy >= 0 and hx + hy <= 2 leg (integers).
 *   point f32 [W,W,3] = (float)((a + beta (b - a)) + gamma (c - a)) per component in binary64 with the rotated corners.
 *   tex f32 [W,W,C] with attr f32 [V,C], 1 <= C = channels <= ESR_ATLAS_MAX_CHANNELS (both or neither; NULL, NULL, 0
 *   without): in binary32, (wa x_a + bf x_b) + gf x_c with bf = (float)beta, gf = (float)gamma, wa = (1 - bf) - gf.
 *   A texel without a face has face -1 and 0 everywhere else.
 *
 * esr_atlas_sample.  n queries: q_face i32 [n], q_bary f64 [n,2], the weights of the face's second and third corner as a ray
 * cast returns them.  tex f32 [W,W,C], out f32 [n,C].  A face outside [0, n_faces) (-1: no hit) gives 0.  In binary64:
 *   w0 = (1 - bu) - bv;  u = (w0 uv[f,0].x + bu uv[f,1].x) + bv uv[f,2].x, v likewise;  x = u W - 0.5, y = v W - 0.5
 *   (not finite: 0);  i0 = floor(x), fx = (float)(x - floor(x)), likewise j0, fy;  the indices i0, i0 + 1, j0, j0 + 1
 *   clamped to [0, W - 1];  in binary32, with t_ij = tex[j, i]:
 *   out = (t00 (1 - fx) + t10 fx) (1 - fy) + (t01 (1 - fx) + t11 fx) fy.
 * ESR_ECAP for n >= 2^31 or C > ESR_ATLAS_MAX_CHANNELS; n == 0 succeeds and touches no pointer.
 */
int esr_atlas_levels(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces, int32_t size,
                     int32_t gutter, int32_t lmin, int32_t lmax, double rho4, int32_t *level, int32_t *rot, int64_t *hist,
                     void *stream);
int esr_atlas_charts(int64_t n_faces, const int64_t *order, const int32_t *rot, const int64_t *counts, int32_t size,
                     int32_t gutter, int32_t lmin, int32_t lmax, int32_t *chart, float *uv, void *stream);
int esr_atlas_texels(const double *vertices, int64_t n_vertices, const int64_t *triangles, int64_t n_faces,
                     const int64_t *order, const int32_t *rot, const int64_t *counts, int32_t size, int32_t gutter,
                     int32_t lmin, int32_t lmax, const float *attr, int32_t channels, int32_t *face, float *bary, float *point,
                     uint8_t *flags, float *tex, void *stream);
int esr_atlas_sample(const float *uv, int64_t n_faces, int32_t size, const float *tex, int32_t channels, int64_t n,
                     const int32_t *q_face, const double *q_bary, float *out, void *stream);

/* ------------------------------------------------------------------------- *
 * X. Path-traced light on the surface (esr_nerf_amd/sources.py: path_light, lit_view(paths=)): the light of the environment
 *    and of the emissive sources that reaches a surface point over up to `depth` segments, every vertex of a path reflecting
 *    by the Disney BRDF -- the light-transport stage's one-sample estimator (app/utils/pbr/functions.py:10-18,
 *    diffuse_scattering: a uniform random unit vector flipped into the normal's hemisphere, weighted by the reflection with
 *    its (n . wi) 2 pi), chained on the mesh.  A path lives in registers: nothing of size P N reaches memory but the optional
 *    `trace` and `end`.
 * ------------------------------------------------------------------------- */

#define ESR_SURFACE_PATH_MAX_PATHS 4096   /* most paths of a point (ESR_ECAP beyond it) */
#define ESR_SURFACE_PATH_MAX_DEPTH 8      /* most segments of a path (ESR_ECAP beyond it) */

/*
 * Scene.  nodes / n_faces / vertices / n_vertices / triangles exactly as esr_bvh_cast takes them.  Per-vertex attributes, f32:
 * v_normal [V,3], v_base [V,3], v_rough [V], v_metal [V] (read only at the vertices of a face that a segment hits).
 * Lights.  n_sources (S), slots (Kp), l_point, l_normal, l_weight, l_radiance, l_face, eps: the arrays of section U, with its
 * rules.  n_sources == 0: no sources, none of them is read.
 * Environment.  mus, lambdas, lobes, n_sg (J) as in section V.  n_sg == 0: no environment, none of them is read, nothing is
 * added to the two environment components (they are exactly +0).
 * Points.  The arrays of section V: p_point f64 [P,3], p_normal f32 [P,3], p_face i32 [P] or NULL, and in mode 0 p_base, p_rough,
 * p_metal, p_wo: the first vertex of every path of the point.
 * Controls.  mode 0 reflected radiance, 1 irradiance at the point; n_paths (N) in 1 .. ESR_SURFACE_PATH_MAX_PATHS; depth (D) in
 * 1 .. ESR_SURFACE_PATH_MAX_DEPTH; t_min >= 0; seed: the 64 bits of the seed; point_base >= 0: the index of point 0 in the whole
 * call a chunk belongs to (a chunked call gives the bytes of the whole call).
 *
 * Random numbers.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85), key = (low,
 * high word of seed), counter = ((uint32)(point_base + p), path s, 2 b + purpose, block) for segment b.  point_base + P <= 2^32.
 * Direction (purpose 0), binary64, every operation rounded on its own: a word x gives a = 2 (x 2^-32) - 1; block k gives the
 * candidate pairs (w0, w1) and (w2, w3); the first pair over the blocks 0 .. 7 with s = a1 a1 + a2 a2 < 1 is taken;
 * q = sqrt(1 - s), w = (2 a1 q, 2 a2 q, 1 - 2 s) (Marsaglia's uniform point on the sphere); if none of the 16 passes, w =
 * (0, 0, 1).  wi = (float)w.  Flip as in section V step 1 on wi and the vertex's normal n: s = (wi0 n0 + wi1 n1) + wi2 n2 in
 * binary32, and s < 0 negates w and wi.
 *
 * Per path, the throughput T (binary64, per channel) starts at 1; per segment b = 0 .. D - 1 from the vertex (x, n, material,
 * wo, face):
 *   1. weight.  T_c = T_c Wt_c, Wt = (double)R of the binary32 Disney reflection for base, rough, metal, n, wi, wo (it carries
 *      (n . wi) 2 pi); for b == 0 in mode 1 instead Wt = cos_x (2 pi), cos_x = (n0 wi0 + n1 wi1) + n2 wi2 in binary64 on the
 *      widened values, the same for the three channels.
 *   2. cast.  esr_bvh_cast's nearest-hit walk, o = x, d = w, t_min < t <= +inf, skip_face = face.
 *   3. miss.  With n_sg > 0: L = the environment of section V step 3 along wi, binary32 in its order; T_c (double)L_c is added
 *      to the component env_dir if b == 0, else to env_indir.  The path ends (code 1).
 *   4. hit on face f with the barycentrics u, v:  wa = (1 - u) - v;  x' = (wa A + u B) + v C per coordinate in binary64;  the
 *      attributes in binary32 with the three weights rounded once, (wa a_A + u a_B) + v a_C, no contraction;  n' = the normal
 *      divided by its binary32 length sqrt((n0 n0 + n1 n1) + n2 n2): a length that is 0 or not finite ends the path (code 2);
 *      wo' = -wi;  unless (n'0 wo'0 + n'1 wo'1) + n'2 wo'2 > 0 in binary32 the path ends (code 2: a back face).
 *   5. next-event estimation, with n_sources > 0.  For every source s one slot k = word >> (32 - log2 Kp) (0 for Kp == 1) of
 *      purpose 1, block s >> 2, word s & 3.  Its term is section U's per-slot term in mode 0 at (x', n', the interpolated
 *      material, wo'): the same silence rules, the same G, the same shadow segment (skip_face = l_face), term_c.  T_c
 *      ((double)Kp term_c) is added to the component src_indir.  A segment that hits a source's face adds no emission: the
 *      lights account for it.
 *   6. advance: (x', n', the interpolated material, wo', f) is the vertex of segment b + 1.  After segment D - 1 the path ends
 *      (code 0).
 * No Russian roulette; a lane walks at most N D (1 + S) rays.
 *
 * Sum, as section V step 5: Kd = min(64, the next power of two >= N) adjacent lanes per point; lane k adds its paths k, k + Kd,
 * ... ascending into nine binary64 sums (component, channel; from +0.0), combined by the balanced pairwise sum over the lanes.
 *   out f32 [P,3,3]: out[p, component, channel] = (float)(S / (double)N); components 0 env_dir, 1 env_indir, 2 src_indir.
 * No atomics: the same input gives the same bytes on every call and under every chunking through point_base.
 * Optional: n_open i32 [P], the paths whose segment 0 misses; trace i32 [P,N,D], the face hit by each segment, -1 where it left
 * the mesh, -2 where it was not cast; end u8 [P,N], the code above.
 *
 * n_points == 0 (with every other argument valid) succeeds and touches no pointer.  ESR_EINVAL: a negative size, a mode other
 * than 0 and 1, slots < 1 or not a power of two, eps not in [0, 0.5), n_paths < 1, depth < 1, t_min negative or NaN, point_base
 * < 0, a NULL or misaligned required pointer (f64 / i64: 8 bytes, nodes: 16, the rest: 4; an optional pointer that is given is
 * held to the same alignment; the attributes are required with n_faces > 0, the lights with n_sources > 0, the environment
 * with n_sg > 0, the material of the points in mode 0).  ESR_ECAP: a size >= 2^31, slots > ESR_SURFACE_LIGHT_MAX_SLOTS, n_sg >
 * ESR_SURFACE_ENV_MAX_SG, n_paths > ESR_SURFACE_PATH_MAX_PATHS, depth > ESR_SURFACE_PATH_MAX_DEPTH, point_base + n_points >
 * 2^32.  Nothing is launched in either case.  One launch on `stream`; nothing waits on the host.
 * Layout: a wave holds 64 / Kd points; the path's vertex and throughput stay in registers; the lobe table sits in LDS.
 */
int esr_surface_path(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                     const int64_t *triangles, const float *v_normal, const float *v_base, const float *v_rough,
                     const float *v_metal, int64_t n_sources, int32_t slots, const double *l_point, const double *l_normal,
                     const double *l_weight, const float *l_radiance, const int32_t *l_face, double eps, const float *mus,
                     const float *lambdas, const float *lobes, int32_t n_sg, int64_t n_points, const double *p_point,
                     const float *p_normal, const int32_t *p_face, const float *p_base, const float *p_rough,
                     const float *p_metal, const float *p_wo, int32_t mode, int32_t n_paths, int32_t depth, double t_min,
                     int64_t seed, int64_t point_base, float *out, int32_t *n_open, int32_t *trace, uint8_t *end,
                     void *stream);

/* ------------------------------------------------------------------------- *
 * Y. Importance-sampled path-traced light on the surface (esr_nerf_amd/sources.py: path_light(sampling="brdf"),
 *    lit_view(paths=, sampling="brdf"), bake_irradiance(paths=)): section X's quantity -- the same integrand, the same
 *    components, the same next-event estimation -- with every segment's direction drawn from the vertex's BRDF instead of
 *    uniformly: a cosine-distributed direction or a half vector from the specular lobe D = exp(kappa (n.h - 1)) / (pi r^2),
 *    kappa = 2 / r^2 (a von Mises-Fisher lobe, whose CDF in n.h inverts in closed form), combined by one-sample multiple
 *    importance sampling with the balance heuristic, and Russian roulette from segment rr_start on.  The reference has no such
 *    sampler: like sections U, W and X's chaining this is an addition to its interfaces.  It estimates what section X
 *    estimates: p > 0 wherever the integrand is not 0, but for the lobe draws with oh' <= 0 that the density step below drops
 *    (a loss of the order 1e-7 of a reflection, and only under a wo below the horizon).
 * ------------------------------------------------------------------------- */

/*
 * Arguments: those of esr_surface_path with their rules, and rr_start (after depth): the first segment at which the roulette
 * runs, >= 1; a value >= depth means no roulette.
 *
 * Random numbers.  Philox4x32-10 with section X's key; counter = ((uint32)(point_base + p), path s, 4 b + purpose, block) for
 * segment b.  Purpose 0: the disc pair, blocks 0 .. 7.  Purpose 1: the next-event slots, block s >> 2, word s & 3, exactly as X.
 * Purpose 2, block 0: word 0 is the technique's, word 1 the roulette's; a word x gives u = ((double)x + 0.5) 2^-32 (exact; never
 * 0, never 1): u_t, u_r.  Purpose 3 is not used.
 *
 * Everything below is binary64 on the widened binary32 values (n, wo, base, rough, metal of the vertex), every operation
 * rounded on its own, no contraction, sums of three terms as (a + b) + c; exp and log are the device library's binary64
 * functions (under an ulp, not correctly rounded).  Per path the throughput T starts at 1; per segment b = 0 .. D - 1 from the
 * vertex (x, n, material, wo, face), in this order:
 *
 *   Disc pair.  X's candidates: a = 2 (x 2^-32) - 1, block k gives the pairs (w0, w1) and (w2, w3); the first pair over the
 *      blocks 0 .. 7 with s = a1 a1 + a2 a2, 0 < s < 1, is taken: (a1, a2, s).  If none of the 16 passes the local direction
 *      below is (0, 0, 1) in either technique (a1 = a2 = 0, s = 0 for the cosine, s = 1 for the lobe).
 *   Roulette, for b >= rr_start.  m = maxNum(maxNum(T0, T1), T2) (a NaN channel is passed over); q = m clamped to [1/16, 1],
 *      q = 1 if m is NaN.  u_r >= q ends the path (code 3: segment b is not cast).  Otherwise T_c = T_c / q.
 *   Frame (Duff et al.).  sg = copysign(1, nz), a = -1 / (sg + nz), b = (nx ny) a,
 *      t1 = (1 + ((sg nx) nx) a, sg b, -(sg nx)), t2 = (b, sg + (ny ny) a, -ny).  A local (lx, ly, lz) is the world vector
 *      (lx t1_i + ly t2_i) + lz n_i per coordinate.
 *   Technique.  abar = ((base0 + base1) + base2) / 3, Fbar = 0.04 (1 - m) + abar m, dbar = (1 - m) abar, sum = Fbar + dbar;
 *      q_s = Fbar / sum clamped to [1/8, 7/8] if sum > 0, else (and for a NaN) 1/8.  In mode 1 at b == 0, q_s = 0.
 *      kappa = 2 / max(rough rough, 1e-7), e = 1 / exp(kappa) (0 where exp(kappa) is +inf).  The lobe is taken iff u_t < q_s.
 *   Cosine technique.  w = the world vector of (a1, a2, sqrt(1 - s)) (Malley; not normalised again).
 *   Lobe technique.  c = 1 + log(s + (1 - s) e) / kappa clamped to [0, 1]; sin = sqrt((1 - c)(1 + c)); the local half vector
 *      h = ((a1 sin) / sqrt(s), (a2 sin) / sqrt(s), c), taken to the world; oh = (wo0 h0 + wo1 h1) + wo2 h2; unless oh > 0 the
 *      path ends (code 4); w = (2 oh) h_i - wo_i, divided by its length sqrt((w0 w0 + w1 w1) + w2 w2).
 *   Density, one code path for both techniques, at the w taken.  cos = (n0 w0 + n1 w1) + n2 w2; unless cos > 0 the path ends
 *      (code 4: the integrand is 0 there, nothing is lost; a NaN ends it too).  wi = (float)w.
 *      hv = w + wo, h' = hv / sqrt((hv0 hv0 + hv1 hv1) + hv2 hv2), nh = max(n . h', 0), oh' = wo . h';
 *      A direction of the lobe technique with oh' <= 0 ends the path as well (code 4).  For unit vectors oh' = oh; but n and wo
 *      are unit only to binary32 (|wo| = 1 + d, |d| up to about 1e-7) while w is normalised in binary64, so hv = w + wo carries
 *      a term of the size d along wo and oh' = (oh + d / 2) / |h'| to first order: where w + wo cancels (oh -> 0, w -> -wo, which
 *      only a wo under the horizon of n lets pass the test on cos) oh' is negative for a positive oh up to about 3e-4.  There the
 *      density would not see the lobe that drew w, and the weight would be that of the cosine technique alone, thousands of
 *      times too large.  Dropping these draws loses integrand that is not 0, so the estimate is low by their share: the
 *      weight of such a draw is proportional to oh, the lobe's mass with oh < 3e-4 times that weight is of the order 1e-7 of a
 *      reflection -- under the binary32 rounding of the reflection itself.  This step is not in the technique's definition
 *      above; it is what makes "one code path for the density" safe.
 *      With p_s = kappa / (2 pi (1 - e)) exp(kappa (nh - 1)) / (4 oh') the lobe technique's density of w (0 unless oh' > 0)
 *      and p_c = cos / pi the cosine technique's, p = q_s p_s + (1 - q_s) p_c is the density of the direction taken (one-sample
 *      MIS, balance heuristic; p >= p_c / 8 > 0).  Computed is 2 pi p, which needs no constant:
 *      P_s = ((kappa / (1 - e)) exp(kappa (nh - 1))) / (4 oh') if oh' > 0, else 0;  P = q_s P_s + (1 - q_s) (2 cos).
 *   1. weight.  T_c = T_c ((double)R_c / P) with R the binary32 Disney reflection of section X for wi (it carries
 *      (n . wi) 2 pi).  In mode 1 at b == 0 instead T_c = T_c pi (the binary64 pi), the exact constant: the cosine technique's
 *      density is the integrand's.
 *   2. - 6.  Exactly section X's: cast (o = x, d = w), miss (code 1), hit and the next vertex (code 2), next-event estimation
 *      with the point-light term (its purpose word is 4 b + 1), advance; after segment D - 1 the path ends (code 0).
 * A lane walks at most N D (1 + S) rays.
 *
 * Sum and outputs: section X's -- Kd lanes per point, lane-strided binary64 sums from +0.0, the balanced pairwise sum over the
 * lanes, out f32 [P,3,3] = (float)(S / (double)N); n_open i32 [P]; trace i32 [P,N,D] (-2 for a segment that was not cast, the
 * one at which code 3 or 4 ended the path included); end u8 [P,N] with X's codes and 3 (the roulette), 4 (no direction in the
 * hemisphere).  No atomics: the same input gives the same bytes on every call and under every chunking through point_base.
 *
 * n_points == 0 (with every other argument valid) succeeds and touches no pointer.  ESR_EINVAL: rr_start < 1, and every case
 * of section X.  ESR_ECAP: as section X.  Nothing is launched in either case.  One launch on `stream`; nothing waits on the
 * host.  Layout as section X: the vertex and the throughput stay in registers, the lobe table sits in LDS; the frame, the
 * uniforms and the binary64 exp / log live only until the cast.
 */
int esr_surface_path_is(const esr_bvh_node_t *nodes, int64_t n_faces, const double *vertices, int64_t n_vertices,
                        const int64_t *triangles, const float *v_normal, const float *v_base, const float *v_rough,
                        const float *v_metal, int64_t n_sources, int32_t slots, const double *l_point, const double *l_normal,
                        const double *l_weight, const float *l_radiance, const int32_t *l_face, double eps, const float *mus,
                        const float *lambdas, const float *lobes, int32_t n_sg, int64_t n_points, const double *p_point,
                        const float *p_normal, const int32_t *p_face, const float *p_base, const float *p_rough,
                        const float *p_metal, const float *p_wo, int32_t mode, int32_t n_paths, int32_t depth, int32_t rr_start,
                        double t_min, int64_t seed, int64_t point_base, float *out, int32_t *n_open, int32_t *trace, uint8_t *end,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ESR_HIP_H */
