// LPIPS (AlexNet) on the device: an implicit-GEMM convolution on the f32 matrix cores, the max pool between the taps and
// the per-layer distance.
//
// Reference algorithm (paths under the reference tree):
//   utils2/metric.py:15-28     rgb_lpips: lpips.LPIPS(net="alex", version="0.1").eval()(gt, im, normalize=True)
// which is, per image [H,W,3] in [0,1]: t = 2x - 1, s = (t - shift) / scale, five AlexNet taps (each behind its ReLU), and
// per tap: unit-normalise over channels (+1e-10 on the norm), squared difference, the 1x1 "lin" weight, mean over pixels;
// the result is the sum over the taps.  The exact arithmetic of every entry: include/esr_hip.h, section Q.
//
// Layout.  Activations are channels-last [N,H,W,C] float32: the evaluation's images are [H,W,3] already, and the
// reduction index of the GEMM, k = (ky kw + kx) Cin + c, runs through memory contiguously in c (and, for one ky, in
// (kx, c): the first layer's 33-float runs).  A weight is rewritten once into packed[k][n], rows padded with zeros to a
// multiple of ESR_CONV_KC: the B operand order of v_mfma_f32_32x32x2_f32 (k on the lane half, n on the lane), so a K-slice
// of it is one coalesced copy into LDS.
//
// conv_relu_kernel.  GEMM M = N Ho Wo pixels, N = Cout, K = Cin kh kw.  A workgroup of four waves owns a 64 x 64 tile
// (pixels x channels), one 32 x 32 accumulator per wave: v_mfma_f32_32x32x2_f32 occupies the matrix pipe for 64 cycles
// and its dependent-accumulator latency is the same 64, so one accumulator per wave already issues back to back, and the
// small tile is what fills the chip in the late layers (800 x 800, three images: 7,203 pixels x 256 channels = 452 tiles
// on 256 CUs, where 128 x 128 tiles would be 114).  K advances in slices of 32: the patch slice [32][64] is gathered
// (0 for a tap outside the image or k >= K; the optional input affine is applied to in-image values only, so the zero
// padding is of the affine's output) and the weight slice [32][64] copied into LDS, double-buffered -- the next slice's
// global loads are issued before the current slice's 16 MFMAs and written to the other buffer after them, one barrier
// per slice.  A thread gathers ONE k (its decomposition into (ky, kx, c) costs two divisions per slice) for 8 pixels
// whose (image, iy0, ix0) sit in an LDS table per tile; 32 consecutive lanes read 32 consecutive k of one pixel (128
// contiguous bytes when Cin >= 32).  LDS: patch rows are padded to 65 floats, so the 32 k of a pixel go to 32 banks on
// the write and the 32 pixels of a k to 32 banks on the read; 33.8 KB per workgroup, four workgroups per CU.
// Order: every output value is ONE k-ascending chain of fused multiply-adds from +0 (the instruction's own k order is
// k0 then k1), bias and ReLU behind it; no split-K, no atomics.  The grid is capped (CV_MAX_BLOCKS resident workgroups)
// and walks the tiles with a stride, channel tiles of one pixel tile adjacent so that they share the patch in L2.
#include "esr_collectives.h"

#pragma clang fp contract(off)

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_BM = 64, CV_BN = 64, CV_KC = ESR_CONV_KC;
constexpr int CV_AS = CV_BM + 1;              // floats per patch row in LDS
constexpr int CV_PIX = CV_BM * CV_KC / CV_THREADS;   // pixels a thread gathers per slice
constexpr int CV_MAX_BLOCKS = 1024;           // 4 resident workgroups on each of 256 CUs
constexpr int LP_THREADS = 256;
static_assert(CV_KC == 32 && CV_BN == 64 && CV_THREADS == 256, "the gather / copy maps below are written for these");

struct ConvArgs {
    const float *x, *wp, *bias, *affine;
    float *y;
    int H, W, Cin, Cout, kh, kw, stride, pad, Ho, Wo, M, K, Kp, tiles_n, tiles;
};

struct ConvSlice {
    float a[CV_PIX];
    float4 b[2];
};

__global__ __launch_bounds__(CV_THREADS) void conv_relu_kernel(ConvArgs p)
{
    __shared__ float As[2][CV_KC][CV_AS];
    __shared__ float4 Bs[2][CV_KC][CV_BN / 4];
    __shared__ int p_img[CV_BM], p_iy[CV_BM], p_ix[CV_BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int kk = tid & (CV_KC - 1), pg = tid >> 5;          // this thread's k of a slice, its first pixel
    const int nslices = p.Kp / CV_KC;

    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int m0 = (tile / p.tiles_n) * CV_BM, n0 = (tile % p.tiles_n) * CV_BN;
        __syncthreads();
        if (tid < CV_BM) {
            const int m = m0 + tid;
            int img = 0, iy = -(1 << 28), ix = 0;                 // a row past M: every tap is outside
            if (m < p.M) {
                const int ox = m % p.Wo, t = m / p.Wo;
                img = t / p.Ho;
                iy = (t - img * p.Ho) * p.stride - p.pad;
                ix = ox * p.stride - p.pad;
            }
            p_img[tid] = img;
            p_iy[tid] = iy;
            p_ix[tid] = ix;
        }
        __syncthreads();

        auto gather = [&](int k0, ConvSlice &s) {
            const int k = k0 + kk;
            const bool valid = k < p.K;
            const int tap = k / p.Cin, c = k - tap * p.Cin;
            const int ky = tap / p.kw, kx = tap - ky * p.kw;
            float sh = 0.f, sc = 1.f;
            if (p.affine && valid) {
                sh = p.affine[c];
                sc = p.affine[p.Cin + c];
            }
#pragma unroll
            for (int j = 0; j < CV_PIX; ++j) {
                const int m = pg + 8 * j;
                const int iy = p_iy[m] + ky, ix = p_ix[m] + kx;
                const bool inb = valid & (iy >= 0) & (iy < p.H) & (ix >= 0) & (ix < p.W);
                const int64_t idx = (((int64_t)p_img[m] * p.H + iy) * p.W + ix) * p.Cin + c;
                float v = p.x[inb ? idx : 0];
                if (p.affine) v = __fdiv_rn((2.0f * v - 1.0f) - sh, sc);
                s.a[j] = inb ? v : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int f = tid + CV_THREADS * j, row = f >> 4, col = n0 + (f & 15) * 4;
                s.b[j] = col < p.Cout ? *(const float4 *)(p.wp + (int64_t)(k0 + row) * p.Cout + col)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        auto stage = [&](int buf, const ConvSlice &s) {
#pragma unroll
            for (int j = 0; j < CV_PIX; ++j) As[buf][kk][pg + 8 * j] = s.a[j];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int f = tid + CV_THREADS * j;
                Bs[buf][f >> 4][f & 15] = s.b[j];
            }
        };

        ConvSlice s;
        gather(0, s);
        stage(0, s);
        __syncthreads();
        const bool active = n0 + wn * 32 < p.Cout;                // wave-uniform (Cout % 32 == 0: half a channel tile)
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int sl = 0; sl < nslices; ++sl) {
            const int buf = sl & 1;
            const bool more = sl + 1 < nslices;
            if (more) gather((sl + 1) * CV_KC, s);
            if (active) {
                const float *ap = &As[buf][lane >> 5][wm * 32 + (lane & 31)];
                const float *bp = (const float *)&Bs[buf][lane >> 5][0] + wn * 32 + (lane & 31);
#pragma unroll
                for (int q = 0; q < CV_KC / 2; ++q)                // k = 2q (lanes 0..31), 2q + 1 (lanes 32..63): ascending
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * q * CV_AS], bp[2 * q * CV_BN], acc, 0, 0, 0);
            }
            if (more) stage(buf ^ 1, s);
            __syncthreads();
        }
        if (active) {
            const int ch = n0 + wn * 32 + (lane & 31);
            const float b = p.bias[ch];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const float v = acc[r] + b;
                if (m < p.M) p.y[(int64_t)m * p.Cout + ch] = v > 0.f ? v : (v == v ? 0.f : v);
            }
        }
    }
}

__global__ __launch_bounds__(LP_THREADS) void conv_pack_kernel(const float *__restrict__ w, int Cout, int Cin, int kh, int kw,
                                                               int K, int64_t total, float *__restrict__ packed)
{
    for (int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * LP_THREADS) {
        const int n = (int)(i % Cout), k = (int)(i / Cout);
        float v = 0.f;
        if (k < K) {
            const int tap = k / Cin, c = k - tap * Cin, ky = tap / kw, kx = tap - ky * kw;
            v = w[(((int64_t)n * Cin + c) * kh + ky) * kw + kx];
        }
        packed[i] = v;
    }
}

__global__ __launch_bounds__(LP_THREADS) void maxpool_nhwc_kernel(const float *__restrict__ x, int H, int W, int C, int k,
                                                                  int stride, int Ho, int Wo, int64_t total,
                                                                  float *__restrict__ y)
{
    for (int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * LP_THREADS) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int ox = (int)(t % Wo);
        t /= Wo;
        const int oy = (int)(t % Ho), n = (int)(t / Ho);
        const float *src = x + (((int64_t)n * H + oy * stride) * W + ox * stride) * C + c;
        float m = src[0];
        for (int dy = 0; dy < k; ++dy)
            for (int dx = 0; dx < k; ++dx) {
                const float v = src[((int64_t)dy * W + dx) * C];
                m = (v > m || v != v) ? v : m;                     // torch: a NaN wins
            }
        y[i] = m;
    }
}

// one wave per pixel, lanes over the channels
__global__ __launch_bounds__(LP_THREADS) void lpips_layer_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                 int64_t npix, int C, const float *__restrict__ lin_w,
                                                                 double *__restrict__ partials)
{
    __shared__ double red[LP_THREADS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int WAVES = LP_THREADS / 64;
    double acc = 0.0;
    for (int64_t px = (int64_t)blockIdx.x * WAVES + wave; px < npix; px += (int64_t)gridDim.x * WAVES) {
        const float *a = f0 + px * C, *b = f1 + px * C;
        float s0 = 0.f, s1 = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float u = a[c], v = b[c];
            s0 = s0 + u * u;
            s1 = s1 + v * v;
        }
        const float den0 = sqrtf(esr_wave_sum(s0)) + 1e-10f, den1 = sqrtf(esr_wave_sum(s1)) + 1e-10f;
        for (int c = lane; c < C; c += 64) {
            const float d = __fdiv_rn(a[c], den0) - __fdiv_rn(b[c], den1);
            acc = acc + (double)lin_w[c] * ((double)d * (double)d);
        }
    }
    const double s = esr_block_sum_tree<LP_THREADS>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// out[0] = (partials[0] + ... + partials[n-1]) / div, summed in a fixed order by one workgroup
__global__ __launch_bounds__(LP_THREADS) void lp_sum_partials_kernel(const double *__restrict__ partials, int n, double div,
                                                                     double *__restrict__ out)
{
    esr_sum_partials<LP_THREADS>(partials, n, div, out);
}

constexpr int64_t LP_CAP = (int64_t)1 << 31;

inline int64_t conv_kp(int Cin, int kh, int kw)
{
    const int64_t K = (int64_t)Cin * kh * kw;
    return (K + CV_KC - 1) / CV_KC * CV_KC;
}

}  // namespace

ESR_API int64_t esr_conv_packed_floats(int32_t Cout, int32_t Cin, int32_t kh, int32_t kw)
{
    if (Cout < 1 || Cin < 1 || kh < 1 || kw < 1) return ESR_EINVAL;
    return conv_kp(Cin, kh, kw) * Cout;
}

ESR_API int esr_conv_pack(const float *w, int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, float *packed, void *stream)
{
    if (!w || !packed || Cout < 1 || Cin < 1 || kh < 1 || kw < 1) return ESR_EINVAL;
    const int64_t K = (int64_t)Cin * kh * kw, total = conv_kp(Cin, kh, kw) * Cout;
    if (total > LP_CAP || K * Cout > LP_CAP) return ESR_ECAP;
    conv_pack_kernel<<<esr_grid_for(total, LP_THREADS), LP_THREADS, 0, esr_stream(stream)>>>(w, Cout, Cin, kh, kw, (int)K, total,
                                                                                            packed);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_conv_relu(const float *x, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *packed, const float *bias,
                          int32_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, const float *affine, float *y,
                          void *stream)
{
    if (!x || !packed || !bias || !y || ((uintptr_t)packed & 15)) return ESR_EINVAL;
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || kh < 1 || kw < 1 || stride < 1 || pad < 0 || Cout % 32) return ESR_EINVAL;
    if ((int64_t)H + 2 * (int64_t)pad < kh || (int64_t)W + 2 * (int64_t)pad < kw) return ESR_EINVAL;
    const int64_t Ho = ((int64_t)H + 2 * (int64_t)pad - kh) / stride + 1, Wo = ((int64_t)W + 2 * (int64_t)pad - kw) / stride + 1;
    const int64_t M = (int64_t)N * Ho * Wo, K = (int64_t)Cin * kh * kw, Kp = conv_kp(Cin, kh, kw);
    if ((int64_t)N * H * W * Cin > LP_CAP || (double)M * Cout > (double)LP_CAP || Kp * Cout > LP_CAP) return ESR_ECAP;
    ConvArgs a;
    a.x = x; a.wp = packed; a.bias = bias; a.affine = affine; a.y = y;
    a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.kh = kh; a.kw = kw; a.stride = stride; a.pad = pad;
    a.Ho = (int)Ho; a.Wo = (int)Wo; a.M = (int)M; a.K = (int)K; a.Kp = (int)Kp;
    a.tiles_n = (Cout + CV_BN - 1) / CV_BN;
    const int64_t tiles = (M + CV_BM - 1) / CV_BM * a.tiles_n;
    a.tiles = (int)tiles;
    const int grid = (int)(tiles < CV_MAX_BLOCKS ? tiles : CV_MAX_BLOCKS);
    conv_relu_kernel<<<grid, CV_THREADS, 0, esr_stream(stream)>>>(a);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_maxpool_nhwc(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, float *y,
                             void *stream)
{
    if (!x || !y || N < 1 || H < 1 || W < 1 || C < 1 || k < 1 || stride < 1 || H < k || W < k) return ESR_EINVAL;
    if ((int64_t)N * H * W * C > LP_CAP) return ESR_ECAP;
    const int Ho = (H - k) / stride + 1, Wo = (W - k) / stride + 1;
    const int64_t total = (int64_t)N * Ho * Wo * C;
    maxpool_nhwc_kernel<<<esr_grid_for(total, LP_THREADS), LP_THREADS, 0, esr_stream(stream)>>>(x, H, W, C, k, stride, Ho, Wo,
                                                                                               total, y);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_lpips_layer(const float *f0, const float *f1, int64_t npix, int32_t C, const float *lin_w, double *partials,
                            double *out, void *stream)
{
    if (!f0 || !f1 || !lin_w || !partials || !out || npix < 1 || C < 1) return ESR_EINVAL;
    if (npix > LP_CAP || npix * C > LP_CAP) return ESR_ECAP;
    const int grid = esr_grid_for(npix, LP_THREADS / 64, ESR_METRICS_BLOCKS);
    hipStream_t st = esr_stream(stream);
    lpips_layer_kernel<<<grid, LP_THREADS, 0, st>>>(f0, f1, npix, C, lin_w, partials);
    ESR_CHECK_LAUNCH();
    lp_sum_partials_kernel<<<1, LP_THREADS, 0, st>>>(partials, grid, (double)npix, out);
    ESR_CHECK_LAUNCH();
    return 0;
}
