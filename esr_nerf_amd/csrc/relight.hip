// Re-lighting edit rays: the dilation of a test view's emissive-source masks and the per-ray edit labels of the
// fine-tune's training rays.
//
// Reference algorithm (paths under the reference tree):
//   app/fine/pdra.py:945-962    cv2.dilate(em_masks, np.ones((ks, ks)), iterations=1) through the host
//   app/fine/pdra.py:988-1028   per chunk: w2c @ (esp, 1), K @ cam, the bound test, F.grid_sample per condition and a
//                               chain of masked assignments per condition
//
// Dilation contract (restated in numpy by tests/relight_ref.py).  OpenCV anchors a ks x ks box at ks / 2, so
//   out[c, y, x] = max over dy, dx in [-(ks / 2), ks - 1 - ks / 2] of in[c, y + dy, x + dx]
// over the pixels of the window that lie inside the image (OpenCV's border value for a dilation is the type's lowest).
// For an even ks the window is NOT symmetric: ks = 10 looks at -5 .. +4.  A maximum is exact, so the separable form (row
// maximum, then column maximum) gives the definition's bits.  The masks are finite (a NaN pixel is not propagated the way
// numpy's maximum would: `v > m` is false for it).
//
// Label contract.  Per ray, every operation a separately rounded binary32 operation in the reference's order
// (contraction off):
//   xyz = w2c . (esp, 1)  (each row summed left to right), cam = xyz[:3] / xyz[3], p = K . cam with
//   K = [[-f, 0, w/2 - 0.5], [0, f, h/2 - 0.5], [0, 0, 1]] INCLUDING the products with K's zeros (0 * inf is what makes
//   the reference's result NaN for a non-finite coordinate), (u, v) = p[:2] / p[2].
//   Out of bounds when u or v is < 0, > h - 1 OR > w - 1: the reference tests BOTH coordinates against BOTH sizes
//   (pdra.py:997), so on a non-square view the usable area is the square of the smaller size.  Reproduced.
//   An in-bounds ray samples every condition's mask with grid_sample(align_corners=True, bilinear, zero padding)
//   including the normalise / un-normalise round trip (u / (w-1) * 2 - 1, then ((g + 1) / 2) * (w-1)): whether a corner's
//   weight is exactly zero decides `> 0` on integer coordinates.  Condition i matches when the sample is > 0.
//   Defaults mode 1, colour (0, 0), intensity 0.  A matching condition sets mode = em_mode[i]; mode 0 sets intensity 0;
//   modes 2 / 4 set intensity = em_intensity[i]; modes 3 / 4 set colour = em_color[i].  Conditions run in order and a
//   later one overrides only the fields IT sets, which is what the reference's sequence of masked assignments leaves.
//   keep = any condition matched.  An out-of-bounds ray keeps the defaults and keep = 0.
//   A ray without a surviving sample has esp = (0, 0, 0) and is projected like any other point (the reference does).
//   Non-finite coordinates: +-inf fails a bound comparison (out of bounds); NaN fails none of them, so the ray counts as
//   in bounds exactly as in the reference, where its NaN sample then matches no condition -- here such a ray reads no
//   mask pixel at all and matches nothing.  Every mask read is guarded by an integer range test.
//
// MI355X notes.  esr_mask_dilate: a workgroup of 256 lanes owns a 16 x 64 tile; the tile plus its halo is staged in LDS
// (outside pixels as -inf), the row maxima go to a second LDS plane and the column pass reads them at stride 1.  The window
// is clipped to the image size first, so a box larger than the image costs an image-sized halo; a footprint beyond the
// CU's LDS is refused with ESR_ECAP.  esr_edit_label: one lane per ray, conditions in a loop, everything in registers, no
// atomics and no data-dependent allocation (two runs give the same bytes).  12 B read and 21 B written per ray (uint8 keep,
// int64 mode, 2 floats of colour, 1 of intensity) in consecutive lanes = consecutive addresses; the masks (n_cond x h x w
// floats: 7.7 MB for three conditions of an 800 x 800 view) stay in L2 / Infinity Cache.  The launch is held against the
// HBM roof at 33 B per ray; at 26 vector registers it runs eight waves per SIMD.
#include "esr_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RL_THREADS = 256;
constexpr int DIL_TH = 16;                     // rows of a dilation tile
constexpr int DIL_TW = 64;                     // columns of a dilation tile
constexpr size_t DIL_MAX_LDS = 160 * 1024;     // LDS of a CU

// ax, bx / ay, by: the window's reach to the left, right / up, down, already clipped to the image size
__global__ __launch_bounds__(RL_THREADS) void mask_dilate_kernel(const float *__restrict__ in, int h, int w, int ax, int bx,
                                                                 int ay, int by, float *__restrict__ out)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int SR = DIL_TH + ay + by, SC = DIL_TW + ax + bx;
    float *stage = lds;                        // [SR][SC]
    float *rowmax = lds + (size_t)SR * SC;     // [SR][DIL_TW]
    const int x0 = blockIdx.x * DIL_TW, y0 = blockIdx.y * DIL_TH;
    const int64_t plane = (int64_t)blockIdx.z * h * w;
    const float *src = in + plane;
    for (int i = tid; i < SR * SC; i += RL_THREADS) {
        const int r = i / SC, c = i - r * SC;
        const int gy = y0 - ay + r, gx = x0 - ax + c;
        const bool inside = gy >= 0 && gy < h && gx >= 0 && gx < w;
        stage[i] = inside ? src[(int64_t)gy * w + gx] : -INFINITY;
    }
    __syncthreads();
    const int nx = ax + bx, ny = ay + by;
    for (int i = tid; i < SR * DIL_TW; i += RL_THREADS) {
        const int r = i / DIL_TW, c = i - r * DIL_TW;
        const float *p = stage + r * SC + c;
        float m = p[0];
        for (int k = 1; k <= nx; ++k) {
            const float v = p[k];
            m = v > m ? v : m;
        }
        rowmax[i] = m;
    }
    __syncthreads();
    const int c = tid % DIL_TW;
    for (int r = tid / DIL_TW; r < DIL_TH; r += RL_THREADS / DIL_TW) {
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= h || gx >= w) continue;
        const float *p = rowmax + r * DIL_TW + c;
        float m = p[0];
        for (int k = 1; k <= ny; ++k) {
            const float v = p[k * DIL_TW];
            m = v > m ? v : m;
        }
        out[plane + (int64_t)gy * w + gx] = m;
    }
}

struct EditCam {
    float m[16];                 // w2c, row-major
    float nf, f, cx, cy;         // K's entries: -f, f, w/2 - 0.5, h/2 - 0.5
    float hm1, wm1;              // h - 1, w - 1
    int h, w;
};

struct EditConds {
    int n;
    int mode[ESR_RELIGHT_MAX_COND];
    float intensity[ESR_RELIGHT_MAX_COND];
    float color[ESR_RELIGHT_MAX_COND][2];
};

// value * weight of one corner, zero padding; the range test guards the read
__device__ __forceinline__ float rl_corner(const float *__restrict__ M, int x, int y, int w, int h, float wt)
{
    return (x >= 0 && x < w && y >= 0 && y < h) ? M[(int64_t)y * w + x] * wt : 0.f;
}

__global__ __launch_bounds__(RL_THREADS) void edit_label_kernel(const float *__restrict__ esp, int64_t n, EditCam cam,
                                                                const float *__restrict__ masks, EditConds cd,
                                                                uint8_t *__restrict__ keep, int64_t *__restrict__ em_modes,
                                                                float *__restrict__ em_colors,
                                                                float *__restrict__ em_intensities, float *__restrict__ uv)
{
    const int64_t hw = (int64_t)cam.h * cam.w;
    for (int64_t r = (int64_t)blockIdx.x * RL_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * RL_THREADS) {
        const float x = esp[3 * r], y = esp[3 * r + 1], z = esp[3 * r + 2];
        float X[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            X[j] = ((cam.m[4 * j] * x + cam.m[4 * j + 1] * y) + cam.m[4 * j + 2] * z) + cam.m[4 * j + 3] * 1.f;
        const float c0 = X[0] / X[3], c1 = X[1] / X[3], c2 = X[2] / X[3];
        // K's zeros take part: 0 * inf = NaN is the reference's result for a non-finite camera coordinate
        const float p0 = (cam.nf * c0 + 0.f * c1) + cam.cx * c2;
        const float p1 = (0.f * c0 + cam.f * c1) + cam.cy * c2;
        const float p2 = (0.f * c0 + 0.f * c1) + 1.f * c2;
        const float u = p0 / p2, v = p1 / p2;
        // pdra.py:997: both coordinates against both sizes
        const bool out_bound = (u < 0.f) | (u > cam.hm1) | (u > cam.wm1) | (v < 0.f) | (v > cam.hm1) | (v > cam.wm1);
        int mode = 1;
        float col0 = 0.f, col1 = 0.f, inten = 0.f;
        bool any = false;
        if (!out_bound) {
            const float gx = u / cam.wm1 * 2.f - 1.f, gy = v / cam.hm1 * 2.f - 1.f;
            const float ix = ((gx + 1.f) / 2.f) * cam.wm1, iy = ((gy + 1.f) / 2.f) * cam.hm1;
            // a NaN coordinate passes every comparison above; it reads nothing and matches nothing
            if (ix == ix && iy == iy && fabsf(ix) < 1e9f && fabsf(iy) < 1e9f) {
                const float fx = floorf(ix), fy = floorf(iy);
                const int xw = (int)fx, yn = (int)fy;
                const float ex = (fx + 1.f) - ix, wx = ix - fx, sy = (fy + 1.f) - iy, ny = iy - fy;
                const float w_nw = ex * sy, w_ne = wx * sy, w_sw = ex * ny, w_se = wx * ny;
                for (int i = 0; i < cd.n; ++i) {
                    const float *M = masks + i * hw;
                    float acc = 0.f;
                    acc = acc + rl_corner(M, xw, yn, cam.w, cam.h, w_nw);
                    acc = acc + rl_corner(M, xw + 1, yn, cam.w, cam.h, w_ne);
                    acc = acc + rl_corner(M, xw, yn + 1, cam.w, cam.h, w_sw);
                    acc = acc + rl_corner(M, xw + 1, yn + 1, cam.w, cam.h, w_se);
                    if (acc > 0.f) {
                        const int md = cd.mode[i];
                        any = true;
                        mode = md;
                        if (md == 0) inten = 0.f;
                        if (md == 2 || md == 4) inten = cd.intensity[i];
                        if (md == 3 || md == 4) {
                            col0 = cd.color[i][0];
                            col1 = cd.color[i][1];
                        }
                    }
                }
            }
        }
        keep[r] = any ? 1 : 0;
        em_modes[r] = mode;
        em_colors[2 * r] = col0;
        em_colors[2 * r + 1] = col1;
        em_intensities[r] = inten;
        if (uv) {
            uv[2 * r] = u;
            uv[2 * r + 1] = v;
        }
    }
}

}  // namespace

ESR_API int esr_mask_dilate(const float *masks, int32_t n_cond, int32_t h, int32_t w, int32_t ks, float *out, void *stream)
{
    if (n_cond < 0 || h < 1 || w < 1 || ks < 1) return ESR_EINVAL;
    if (!n_cond) return 0;
    if (!masks || !out || masks == out) return ESR_EINVAL;
    const int a = ks / 2, b = ks - 1 - ks / 2;
    const int ax = a < w - 1 ? a : w - 1, bx = b < w - 1 ? b : w - 1;
    const int ay = a < h - 1 ? a : h - 1, by = b < h - 1 ? b : h - 1;
    const size_t SR = DIL_TH + ay + by, SC = DIL_TW + ax + bx;
    const size_t lds_bytes = sizeof(float) * (SR * SC + SR * DIL_TW);
    const int64_t tx = (w + DIL_TW - 1) / DIL_TW, ty = (h + DIL_TH - 1) / DIL_TH;
    if (lds_bytes > DIL_MAX_LDS || ty > 65535 || n_cond > 65535 || (int64_t)h * w >= ((int64_t)1 << 31)) return ESR_ECAP;
    static std::atomic<uint64_t> optin{0};
    if (lds_bytes > 64 * 1024)                 // (the attribute is set once per device: to the most a launch may ask for)
        if (int e = esr_lds_optin((const void *)mask_dilate_kernel, DIL_MAX_LDS, optin)) return e;
    mask_dilate_kernel<<<dim3((unsigned)tx, (unsigned)ty, (unsigned)n_cond), RL_THREADS, lds_bytes, esr_stream(stream)>>>(
        masks, h, w, ax, bx, ay, by, out);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_edit_label(const float *esp, int64_t n, const float *w2c, float focal, int32_t w, int32_t h,
                           const float *masks, int32_t n_cond, const int64_t *cond_modes, const float *cond_intensities,
                           const float *cond_colors, uint8_t *keep, int64_t *em_modes, float *em_colors,
                           float *em_intensities, float *uv, void *stream)
{
    if (n < 0 || n_cond < 0 || h < 1 || w < 1 || !w2c || (n_cond && (!masks || !cond_modes))) return ESR_EINVAL;
    if (n_cond > ESR_RELIGHT_MAX_COND || (int64_t)h * w >= ((int64_t)1 << 31)) return ESR_ECAP;
    if (!n) return 0;
    if (!esp || !keep || !em_modes || !em_colors || !em_intensities) return ESR_EINVAL;
    EditCam cam;
    for (int i = 0; i < 16; ++i) cam.m[i] = w2c[i];
    cam.f = focal;
    cam.nf = -focal;
    cam.cx = (float)(w / 2.0 - 0.5);
    cam.cy = (float)(h / 2.0 - 0.5);
    cam.hm1 = (float)(h - 1);
    cam.wm1 = (float)(w - 1);
    cam.h = h;
    cam.w = w;
    EditConds cd;
    cd.n = n_cond;
    for (int i = 0; i < ESR_RELIGHT_MAX_COND; ++i) {
        const bool on = i < n_cond;
        if (on && (cond_modes[i] < 0 || cond_modes[i] > 4)) return ESR_EINVAL;
        cd.mode[i] = on ? (int)cond_modes[i] : 1;
        cd.intensity[i] = on && cond_intensities ? cond_intensities[i] : 0.f;
        cd.color[i][0] = on && cond_colors ? cond_colors[2 * i] : 0.f;
        cd.color[i][1] = on && cond_colors ? cond_colors[2 * i + 1] : 0.f;
    }
    edit_label_kernel<<<esr_grid_for(n, RL_THREADS), RL_THREADS, 0, esr_stream(stream)>>>(
        esp, n, cam, masks, cd, keep, em_modes, em_colors, em_intensities, uv);
    ESR_CHECK_LAUNCH();
    return 0;
}
