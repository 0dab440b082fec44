// Image-level evaluation metrics: SSIM, the view post-processing with its squared-error sums, and the mask IoU counts.
//
// Reference algorithm (paths under the reference tree):
//   utils2/metric.py:31-88     rgb_ssim: scipy.signal.convolve2d ("valid"), 6 calls per filtered quantity, 5 quantities
//   app/fine/fine.py:572-605   white background, clamps, apply_gamma_curve (utils2/image.py:14-26), F.mse_loss, uint8 images
//   utils2/metric.py:95-98     IoU
//
// SSIM contract (restated in numpy by tests/metrics_ref.py).  x, y are the float32 images; the three products x*x, y*y, x*y
// are rounded to float32 (the reference squares float32 tensors), everything behind them is float64: the five
// quantities x, y, xx, yy, xy are filtered along a row and then along a column with the caller's float64 taps (fused
// multiply-adds: each window sum carries one rounding per tap instead of scipy's two), and per output value
//   mu00 = mu0*mu0, mu11 = mu1*mu1, mu01 = mu0*mu1, s00 = max(0, E[xx]-mu00), s11 = max(0, E[yy]-mu11), s01 = E[xy]-mu01,
//   s01 = sign(s01) * min(sqrt(s00*s11), |s01|), ssim = ((2 mu01 + c1)(2 s01 + c2)) / ((mu00 + mu11 + c1)(s00 + s11 + c2))
// with every operation separately rounded (contraction off), so two identical images give numerator == denominator and
// 1.0 exactly, as in the reference.
//
// MI355X notes.  One kernel from the two images to per-workgroup partial sums.  An image row is 3W interleaved floats and
// the row filter reads every third of them, so a tile is addressed in float columns and the channels need no code.  A
// workgroup of 256 lanes owns 32 rows x 8 pixels (24 float columns) of the map: it stages (32+fs-1) x (24+3(fs-1)) floats
// of both images in LDS (18 KB at fs = 11), writes the row pass of the five quantities as float64 planes into LDS
// (5 x 42 x 24 x 8 B = 40 KB) and runs the column pass out of them; nothing intermediate goes to memory.  The tile is
// tall because the pass that runs on the halo is the row pass: it costs (32+10)/32 of the column pass, against (16+10)/16
// for a square tile of the same LDS size, and 58 KB keeps two workgroups on a CU.  Consecutive lanes take consecutive
// float columns: the float64 planes are read and written at stride 1 (no bank conflict), the staged floats at stride 1
// with a row change every 24 lanes.  The mean is deterministic: a lane adds its values in a fixed order, the workgroup
// reduces by a fixed tree into partials[workgroup], and a second launch of one workgroup sums the partials the same way.
#include "esr_collectives.h"

#pragma clang fp contract(off)

namespace {

constexpr int MT_THREADS = 256;
constexpr int SSIM_TH = 32;                 // map rows of a tile
constexpr int SSIM_TW = 8;                  // map pixels of a tile
constexpr int SSIM_TC = SSIM_TW * 3;        // float columns of a tile

struct SsimTaps {
    double t[ESR_SSIM_MAX_TAPS];
};

__device__ __forceinline__ double ssim_value(double mu0, double mu1, double e00, double e11, double e01, double c1, double c2)
{
    const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
    const double s00 = fmax(0.0, e00 - mu00), s11 = fmax(0.0, e11 - mu11);
    double s01 = e01 - mu01;
    const double lim = fmin(sqrt(s00 * s11), fabs(s01));
    s01 = s01 > 0.0 ? lim : (s01 < 0.0 ? -lim : 0.0);
    const double numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2);
    const double denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
    return numer / denom;
}

// FS: the filter size as a compile-time constant (loops unrolled, taps in registers), or 0: `fs` at run time.
template <int FS>
__global__ __launch_bounds__(MT_THREADS) void ssim_kernel(const float *__restrict__ img0, const float *__restrict__ img1, int H,
                                                          int W, SsimTaps taps, int fs_rt, double c1, double c2,
                                                          double *__restrict__ map, double *__restrict__ partials)
{
    extern __shared__ double lds[];
    const int fs = FS ? FS : fs_rt;
    const int tid = threadIdx.x;
    const int OH = H - fs + 1, OW = W - fs + 1, OC = OW * 3;       // the map: rows, pixels, float columns
    const int TR = SSIM_TH + fs - 1, IC = SSIM_TC + 3 * (fs - 1);  // staged rows and float columns of a tile
    double *red = lds;                                             // [MT_THREADS]
    double *tap = red + MT_THREADS;                                // [ESR_SSIM_MAX_TAPS]
    double *hq = tap + ESR_SSIM_MAX_TAPS;                          // [5][TR][SSIM_TC] row-pass results
    float *in0 = (float *)(hq + 5 * TR * SSIM_TC);                 // [TR][IC]
    float *in1 = in0 + TR * IC;
    const int plane = TR * SSIM_TC;
#pragma unroll
    for (int k = 0; k < ESR_SSIM_MAX_TAPS; ++k)
        if (tid == 0 && k < fs) tap[k] = taps.t[k];

    const int tiles_x = (OW + SSIM_TW - 1) / SSIM_TW, tiles_y = (OH + SSIM_TH - 1) / SSIM_TH;
    double acc = 0.0;
    for (int tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
        const int r0 = (tile / tiles_x) * SSIM_TH, c0 = (tile % tiles_x) * SSIM_TC;
        const int rows = min(SSIM_TH, OH - r0), cols = min(SSIM_TC, OC - c0);       // map rows / float columns of this tile
        const int in_rows = rows + fs - 1, in_cols = cols + 3 * (fs - 1);           // <= H - r0, <= 3W - c0
        __syncthreads();                                                            // the previous tile's reads are done
        for (int i = tid; i < in_rows * in_cols; i += MT_THREADS) {
            const int r = i / in_cols, c = i - r * in_cols;
            const int64_t g = (int64_t)(r0 + r) * (3 * W) + (c0 + c);
            in0[r * IC + c] = img0[g];
            in1[r * IC + c] = img1[g];
        }
        __syncthreads();
        // row pass over the staged rows: out[c] = sum_k t[k] * in[c + 3 (fs-1-k)] (convolve2d flips the kernel)
        for (int i = tid; i < in_rows * cols; i += MT_THREADS) {
            const int r = i / cols, c = i - r * cols;
            const float *p0 = in0 + r * IC + c, *p1 = in1 + r * IC + c;
            double a0 = 0.0, a1 = 0.0, a00 = 0.0, a11 = 0.0, a01 = 0.0;
#pragma unroll
            for (int k = 0; k < fs; ++k) {
                const double t = FS ? taps.t[k] : tap[k];
                const float x = p0[3 * (fs - 1 - k)], y = p1[3 * (fs - 1 - k)];
                const float xx = x * x, yy = y * y, xy = x * y;
                a0 = fma(t, (double)x, a0);
                a1 = fma(t, (double)y, a1);
                a00 = fma(t, (double)xx, a00);
                a11 = fma(t, (double)yy, a11);
                a01 = fma(t, (double)xy, a01);
            }
            double *o = hq + r * SSIM_TC + c;
            o[0] = a0;
            o[plane] = a1;
            o[2 * plane] = a00;
            o[3 * plane] = a11;
            o[4 * plane] = a01;
        }
        __syncthreads();
        // column pass and the map value
        for (int i = tid; i < rows * cols; i += MT_THREADS) {
            const int r = i / cols, c = i - r * cols;
            const double *p = hq + r * SSIM_TC + c;
            double a0 = 0.0, a1 = 0.0, a00 = 0.0, a11 = 0.0, a01 = 0.0;
#pragma unroll
            for (int k = 0; k < fs; ++k) {
                const double t = FS ? taps.t[k] : tap[k];
                const double *q = p + (fs - 1 - k) * SSIM_TC;
                a0 = fma(t, q[0], a0);
                a1 = fma(t, q[plane], a1);
                a00 = fma(t, q[2 * plane], a00);
                a11 = fma(t, q[3 * plane], a11);
                a01 = fma(t, q[4 * plane], a01);
            }
            const double v = ssim_value(a0, a1, a00, a11, a01, c1, c2);
            if (map) map[(int64_t)(r0 + r) * OC + (c0 + c)] = v;
            acc = acc + v;
        }
    }
    const double s = esr_block_sum_tree<MT_THREADS>(acc, red);
    if (tid == 0) partials[blockIdx.x] = s;
}

// out[0] = (partials[0] + ... + partials[n-1]) / div, summed in a fixed order by one workgroup
__global__ __launch_bounds__(MT_THREADS) void sum_partials_kernel(const double *__restrict__ partials, int n, double div,
                                                                  double *__restrict__ out)
{
    esr_sum_partials<MT_THREADS>(partials, n, div, out);
}

// utils2/image.py:14-26 in float32, as torch evaluates it: x <= 0.0031308 ? 12.92 x : 1.055 x^(1/2.4) - 0.055
__device__ __forceinline__ float gamma_curve(float x)
{
    return x <= 0.0031308f ? 12.92f * x : 1.055f * powf(x, (float)(1.0 / 2.4)) - 0.055f;
}

// torch's clamp: NaN stays NaN
__device__ __forceinline__ float clamp_lo(float v, float lo) { return v != v ? v : fmaxf(v, lo); }
__device__ __forceinline__ float clamp_01(float v) { return v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f); }
// (clamp01(x) * 255).astype(uint8): one float32 multiply, then truncation
__device__ __forceinline__ uint8_t to_u8(float x) { return (uint8_t)(int)(clamp_01(x) * 255.0f); }

__device__ __forceinline__ double sq_diff(float a, float b)
{
    const double d = (double)a - (double)b;
    return d * d;
}

__global__ __launch_bounds__(MT_THREADS) void view_post_kernel(esr_view_post_t p, int64_t total)
{
    __shared__ double red[MT_THREADS];
    double e_out = 0.0, e_gamma = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * MT_THREADS) {
        float s = p.v[i];
        if (p.wbg) s = s + p.wbg[i / p.channels] * p.wbg_scale;
        const float o = p.lin ? clamp_lo(s, 0.0f) : clamp_01(s);
        p.out[i] = o;
        if (p.out_u8) p.out_u8[i] = to_u8(o);
        if (p.target_out) e_out = e_out + sq_diff(o, p.target_out[i]);
        if (p.lin) {
            const float g = gamma_curve(clamp_01(s));
            if (p.gamma) p.gamma[i] = g;
            if (p.gamma_u8) p.gamma_u8[i] = to_u8(g);
            if (p.target_gamma) e_gamma = e_gamma + sq_diff(g, p.target_gamma[i]);
        }
    }
    if (p.target_out) {
        const double s = esr_block_sum_tree<MT_THREADS>(e_out, red);
        if (threadIdx.x == 0) p.partials[blockIdx.x] = s;
    }
    if (p.target_gamma) {
        const double s = esr_block_sum_tree<MT_THREADS>(e_gamma, red);
        if (threadIdx.x == 0) p.partials[ESR_METRICS_BLOCKS + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(MT_THREADS) void sqerr_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n,
                                                           double *__restrict__ partials)
{
    __shared__ double red[MT_THREADS];
    double e = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT_THREADS)
        e = e + sq_diff(a[i], b[i]);
    const double s = esr_block_sum_tree<MT_THREADS>(e, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(MT_THREADS) void gamma_kernel(const float *__restrict__ x, int64_t n, float *__restrict__ y)
{
    for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT_THREADS)
        y[i] = gamma_curve(x[i]);
}

__global__ __launch_bounds__(MT_THREADS) void mask_iou_kernel(const uint8_t *__restrict__ m1, const uint8_t *__restrict__ m2,
                                                              int64_t n, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned int inter = 0, uni = 0;
    for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT_THREADS) {
        const bool a = m1[i] != 0, b = m2[i] != 0;
        inter += a & b;
        uni += a | b;
    }
    if (inter) atomicAdd(&s_cnt[0], inter);
    if (uni) atomicAdd(&s_cnt[1], uni);
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

template <int FS>
int ssim_launch(const float *img0, const float *img1, int H, int W, const SsimTaps &taps, int fs, double c1, double c2,
                double *map, double *partials, int grid, size_t lds_bytes, hipStream_t st)
{
    static std::atomic<uint64_t> optin{0};
    if (int e = esr_lds_optin((const void *)ssim_kernel<FS>, lds_bytes, optin)) return e;
    ssim_kernel<FS><<<grid, MT_THREADS, lds_bytes, st>>>(img0, img1, H, W, taps, fs, c1, c2, map, partials);
    ESR_CHECK_LAUNCH();
    return 0;
}

}  // namespace

ESR_API int esr_ssim(const float *img0, const float *img1, int32_t H, int32_t W, const double *taps, int32_t filter_size,
                     double c1, double c2, double *map, double *partials, double *mean, void *stream)
{
    if (!img0 || !img1 || !taps || !partials || !mean || filter_size < 1 || H < filter_size || W < filter_size)
        return ESR_EINVAL;
    if (filter_size > ESR_SSIM_MAX_TAPS || (int64_t)H * W > ((int64_t)1 << 31) / 3) return ESR_ECAP;
    SsimTaps t;
    for (int k = 0; k < ESR_SSIM_MAX_TAPS; ++k) t.t[k] = k < filter_size ? taps[k] : 0.0;
    const int OH = H - filter_size + 1, OW = W - filter_size + 1;
    const int64_t tiles = (int64_t)((OW + SSIM_TW - 1) / SSIM_TW) * ((OH + SSIM_TH - 1) / SSIM_TH);
    const int grid = (int)(tiles < ESR_METRICS_BLOCKS ? tiles : ESR_METRICS_BLOCKS);
    const int TR = SSIM_TH + filter_size - 1, IC = SSIM_TC + 3 * (filter_size - 1);
    const size_t lds_bytes = sizeof(double) * (MT_THREADS + ESR_SSIM_MAX_TAPS + 5 * TR * SSIM_TC) + sizeof(float) * 2 * TR * IC;
    hipStream_t st = esr_stream(stream);
    const int e = filter_size == 11
                      ? ssim_launch<11>(img0, img1, H, W, t, filter_size, c1, c2, map, partials, grid, lds_bytes, st)
                      : ssim_launch<0>(img0, img1, H, W, t, filter_size, c1, c2, map, partials, grid, lds_bytes, st);
    if (e) return e;
    sum_partials_kernel<<<1, MT_THREADS, 0, st>>>(partials, grid, (double)OH * OW * 3, mean);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_view_post(const esr_view_post_t *job, void *stream)
{
    if (!job || job->n < 0 || (job->channels != 1 && job->channels != 3)) return ESR_EINVAL;
    if (!job->n) return 0;
    if (!job->v || !job->out || (!job->lin && (job->gamma || job->gamma_u8 || job->target_gamma))) return ESR_EINVAL;
    if ((job->target_out || job->target_gamma) && (!job->partials || !job->sqerr)) return ESR_EINVAL;
    const int64_t total = job->n * job->channels;
    const int grid = esr_grid_for(total, MT_THREADS, ESR_METRICS_BLOCKS);
    hipStream_t st = esr_stream(stream);
    view_post_kernel<<<grid, MT_THREADS, 0, st>>>(*job, total);
    ESR_CHECK_LAUNCH();
    if (job->target_out) {
        sum_partials_kernel<<<1, MT_THREADS, 0, st>>>(job->partials, grid, 1.0, job->sqerr);
        ESR_CHECK_LAUNCH();
    }
    if (job->target_gamma) {
        sum_partials_kernel<<<1, MT_THREADS, 0, st>>>(job->partials + ESR_METRICS_BLOCKS, grid, 1.0, job->sqerr + 1);
        ESR_CHECK_LAUNCH();
    }
    return 0;
}

ESR_API int esr_sqerr_sum(const float *a, const float *b, int64_t n, double *partials, double *sum, void *stream)
{
    if (n < 0 || !partials || !sum || (n && (!a || !b))) return ESR_EINVAL;
    const int grid = esr_grid_for(n, MT_THREADS, ESR_METRICS_BLOCKS);
    hipStream_t st = esr_stream(stream);
    sqerr_kernel<<<grid, MT_THREADS, 0, st>>>(a, b, n, partials);
    ESR_CHECK_LAUNCH();
    sum_partials_kernel<<<1, MT_THREADS, 0, st>>>(partials, grid, 1.0, sum);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_gamma_curve(const float *x, int64_t n, float *y, void *stream)
{
    if (n < 0 || (n && (!x || !y))) return ESR_EINVAL;
    if (!n) return 0;
    gamma_kernel<<<esr_grid_for(n, MT_THREADS, ESR_METRICS_BLOCKS), MT_THREADS, 0, esr_stream(stream)>>>(x, n, y);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_mask_iou(const uint8_t *mask1, const uint8_t *mask2, int64_t n, int64_t *counts, void *stream)
{
    if (n < 0 || !counts || (n && (!mask1 || !mask2))) return ESR_EINVAL;
    hipStream_t st = esr_stream(stream);
    hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    if (!n) return 0;
    mask_iou_kernel<<<esr_grid_for(n, MT_THREADS, ESR_METRICS_BLOCKS), MT_THREADS, 0, st>>>(mask1, mask2, n,
                                                                                           (unsigned long long *)counts);
    ESR_CHECK_LAUNCH();
    return 0;
}
