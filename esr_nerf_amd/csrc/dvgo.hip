// DVGO pre-stage (app/coarse/model/dvgo.py): the alphamask renderer's sampling, lookups and compositing.
//
// Sampling (dvgo.py:140-174).  Every operation is a separately rounded binary32 op (contraction off), in torch's order:
//   t_min, t_max   esr_ray_trange (rd == 0 -> 1e-6 for the slab test only), clamped to [near, far]
//   interpx_i      t_min + (step_scale * rng_i) / |rd|   rng_i = i (+ u for training), step_scale = stepsize * voxel_size
//                  as the caller rounded it, |rd| = torch's norm, passed in
//   p_i            o + d * interpx_i
//   masked         t_max <= t_min, or p_i outside [xyz_min, xyz_max]
// Lookups: esr_world_to_index / the 8-corner trilinear of F.grid_sample(align_corners=True, zeros).  density only at
// unmasked samples (alpha = 0 elsewhere); off_color at every sample; emo_color at every sample of an em_mode == 1 ray.
//
// Mapping: one wave per ray; lane l owns the consecutive samples [l K, min((l + 1) K, S)), K = ceil(S / 64).  The
// transmittance T (exclusive cumprod of p = max(1 - alpha, 1e-10)) is each lane's product over its run, a wave prefix
// product of the 64 run products, then the run again.  The backward's reverse recurrence R_i = g_{i+1} + p_{i+1} R_{i+1}
// is an affine map per run, composed across the wave by a suffix scan (no division by p: T underflows behind a few
// clamped samples).
//
// Grid gradients and the view count: every lane walks its samples in order and keeps the 8 corners x C channels of the
// current cell in registers.  When the next sample lies in another cell, only the corners the two cells do not share
// are added to the grid (global float atomics); the shared ones move to their place in the new cell.  At 0.5 voxel per
// step a sample changes cell about 0.8 times, so a sample costs ~3 corner adds instead of 8.
#include "esr_collectives.h"

#define DVGO_BLOCK 256
#define DVGO_WAVES (DVGO_BLOCK / ESR_WAVE)

struct DvgoGeom {
    float bmin[3], bmax[3];
    int dims[3];
    float near_, far_, step_scale;
};

__device__ __forceinline__ DvgoGeom dvgo_geom(const esr_dvgo_t &a)
{
    DvgoGeom g;
    for (int i = 0; i < 3; ++i) {
        g.bmin[i] = a.xyz_min[i];
        g.bmax[i] = a.xyz_max[i];
        g.dims[i] = a.dims[i];
    }
    g.near_ = a.near_;
    g.far_ = a.far_;
    g.step_scale = a.step_scale;
    return g;
}

// p = o + d * (t_min + (step_scale * rng) / nrm), torch's rounding
__device__ __forceinline__ void dvgo_point(const float o[3], const float d[3], float tmin, float nrm, float step_scale,
                                           float rng, float p[3])
{
#pragma clang fp contract(off)
    const float step = step_scale * rng;
    const float t = tmin + __fdiv_rn(step, nrm);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = o[a] + d[a] * t;
}

__device__ __forceinline__ float dvgo_rng(int i, float u)
{
#pragma clang fp contract(off)
    return (float)i + u;
}

// 1 - exp(-softplus(d + shift) * interval)
__device__ __forceinline__ float dvgo_alpha(float d, float shift, float interval)
{
    return esr_dvgo_alpha(d, shift, interval);          // (esr_common.h: shared with esr_density_bounds)
}

// d alpha / d d, torch's autograd of dvgo_alpha (softplus backward: z / (z + 1), z = exp(x), unless x > 20)
__device__ __forceinline__ float dvgo_alpha_grad(float d, float shift, float interval)
{
#pragma clang fp contract(off)
    const float x = d + shift;
    const float e = expf(-esr_softplus(x) * interval);
    float ds;
    if (x > 20.f) {
        ds = 1.f;
    } else {
        const float z = expf(x);
        ds = z / (z + 1.f);
    }
    return e * interval * ds;
}

__device__ __forceinline__ float dvgo_pclamp(float alpha)
{
    return fmaxf(1.f - alpha, 1e-10f);
}

// C-channel trilinear fetch of a channels-first grid [C, X, Y, Z] (zero padding)
template <int C>
__device__ __forceinline__ void dvgo_fetch(const float *__restrict__ g, const int dims[3], const float idx[3], float out[C])
{
    const int64_t plane = (int64_t)dims[0] * dims[1] * dims[2];
    Tri t = esr_tri_setup(idx);
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = 0.f;
#pragma unroll
    for (int cx = 0; cx < 2; ++cx)
#pragma unroll
        for (int cy = 0; cy < 2; ++cy)
#pragma unroll
            for (int cz = 0; cz < 2; ++cz) {
                const int x = t.i0[0] + cx, y = t.i0[1] + cy, z = t.i0[2] + cz;
                const bool inb = (x >= 0) & (x < dims[0]) & (y >= 0) & (y < dims[1]) & (z >= 0) & (z < dims[2]);
                const float w = esr_corner_w(t, idx, cx, cy, cz);
                const int64_t i = ((int64_t)x * dims[1] + y) * dims[2] + z;
#pragma unroll
                for (int c = 0; c < C; ++c) out[c] = __builtin_fmaf(esr_ld_or0(g, c * plane + i, inb), w, out[c]);
            }
}

// ---------------------------------------------------------------------------
// The per-lane cell accumulator of the scatters.  v[corner][channel], corner = cx * 4 + cy * 2 + cz; channel c is added
// to the [X, Y, Z] plane dst[c].
// ---------------------------------------------------------------------------
template <int C>
struct CellAcc {
    int base[3];
    float v[8][C];
};

template <int C>
__device__ __forceinline__ void acc_reset(CellAcc<C> &a)
{
    a.base[0] = a.base[1] = a.base[2] = INT_MIN / 2;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) a.v[k][c] = 0.f;
}

template <int C>
__device__ __forceinline__ void acc_add_corner(float *const dst[C], const int dims[3], int x, int y, int z,
                                               const float v[C])
{
    const bool inb = (x >= 0) & (x < dims[0]) & (y >= 0) & (y < dims[1]) & (z >= 0) & (z < dims[2]);
    if (!inb) return;
    const int64_t i = ((int64_t)x * dims[1] + y) * dims[2] + z;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (v[c] != 0.f) atomicAdd(dst[c] + i, v[c]);
}

// moves the accumulator to cell nb: the corners of the old cell that nb does not share are added to the grids, the
// shared ones take their place in nb
template <int C>
__device__ __forceinline__ void acc_move(CellAcc<C> &a, const int nb[3], float *const dst[C], const int dims[3])
{
    const int dx = nb[0] - a.base[0], dy = nb[1] - a.base[1], dz = nb[2] - a.base[2];
    if ((dx | dy | dz) == 0) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cx = k >> 2, cy = (k >> 1) & 1, cz = k & 1;
        const int nx = cx - dx, ny = cy - dy, nz = cz - dz;
        const bool keep = ((unsigned)nx <= 1u) & ((unsigned)ny <= 1u) & ((unsigned)nz <= 1u);
        if (!keep) acc_add_corner<C>(dst, dims, a.base[0] + cx, a.base[1] + cy, a.base[2] + cz, a.v[k]);
    }
    // shift the kept corners one axis at a time (a step of one cell along an axis keeps one face; more keeps none)
    const bool far = (dx < -1) | (dx > 1) | (dy < -1) | (dy > 1) | (dz < -1) | (dz > 1);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k & 4) continue;
        const int lo = k, hi = k | 4;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float l = a.v[lo][c], h = a.v[hi][c];
            a.v[lo][c] = dx == 1 ? h : (dx == -1 ? 0.f : l);
            a.v[hi][c] = dx == 1 ? 0.f : (dx == -1 ? l : h);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k & 2) continue;
        const int lo = k, hi = k | 2;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float l = a.v[lo][c], h = a.v[hi][c];
            a.v[lo][c] = dy == 1 ? h : (dy == -1 ? 0.f : l);
            a.v[hi][c] = dy == 1 ? 0.f : (dy == -1 ? l : h);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k & 1) continue;
        const int lo = k, hi = k | 1;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float l = a.v[lo][c], h = a.v[hi][c];
            a.v[lo][c] = dz == 1 ? h : (dz == -1 ? 0.f : l);
            a.v[hi][c] = dz == 1 ? 0.f : (dz == -1 ? l : h);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (far) a.v[k][c] = 0.f;
    a.base[0] = nb[0];
    a.base[1] = nb[1];
    a.base[2] = nb[2];
}

template <int C>
__device__ __forceinline__ void acc_flush(CellAcc<C> &a, float *const dst[C], const int dims[3])
{
#pragma unroll
    for (int k = 0; k < 8; ++k)
        acc_add_corner<C>(dst, dims, a.base[0] + (k >> 2), a.base[1] + ((k >> 1) & 1), a.base[2] + (k & 1), a.v[k]);
}

// adds val[c] * (corner weight) at the sample whose continuous index is idx
template <int C>
__device__ __forceinline__ void acc_sample(CellAcc<C> &a, const float idx[3], const float val[C], float *const dst[C],
                                           const int dims[3])
{
    const Tri t = esr_tri_setup(idx);
    acc_move<C>(a, t.i0, dst, dims);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float w = esr_corner_w(t, idx, k >> 2, (k >> 1) & 1, k & 1);
#pragma unroll
        for (int c = 0; c < C; ++c) a.v[k][c] = __builtin_fmaf(val[c], w, a.v[k][c]);
    }
}

// ---------------------------------------------------------------------------
// wave scans
// ---------------------------------------------------------------------------
// exclusive prefix product across the wave
__device__ __forceinline__ float wave_excl_prod(float x)
{
    const int lane = esr_lane();
    float incl = x;
#pragma unroll
    for (int off = 1; off < ESR_WAVE; off <<= 1) {
        const float y = __shfl_up(incl, off, ESR_WAVE);
        if (lane >= off) incl *= y;
    }
    const float prev = __shfl_up(incl, 1, ESR_WAVE);
    return lane == 0 ? 1.f : prev;
}

// x -> B + A x per lane; returns the composition of the maps of lanes l+1 .. 63 (identity for lane 63)
__device__ __forceinline__ void wave_suffix_affine(float &A, float &B)
{
    const int lane = esr_lane();
#pragma unroll
    for (int off = 1; off < ESR_WAVE; off <<= 1) {
        const float A2 = __shfl_down(A, off, ESR_WAVE), B2 = __shfl_down(B, off, ESR_WAVE);
        if (lane + off < ESR_WAVE) {
            B = B + A * B2;
            A = A * A2;
        }
    }
    const float An = __shfl_down(A, 1, ESR_WAVE), Bn = __shfl_down(B, 1, ESR_WAVE);
    A = lane == ESR_WAVE - 1 ? 1.f : An;
    B = lane == ESR_WAVE - 1 ? 0.f : Bn;
}

// per-ray set-up shared by the three ray kernels
struct DvgoRay {
    float o[3], d[3], tmin, nrm, u;
    bool miss;
    int em;
};

__device__ __forceinline__ DvgoRay dvgo_ray(const esr_dvgo_rays_t &R, const DvgoGeom &g, int64_t r)
{
    DvgoRay y;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        y.o[a] = R.rays_o[3 * r + a];
        y.d[a] = R.rays_d[3 * r + a];
    }
    float tmax;
    esr_ray_trange(y.o, y.d, g.bmin, g.bmax, g.near_, g.far_, y.tmin, tmax);
    y.miss = tmax <= y.tmin;
    y.nrm = R.nrm[r];
    y.u = R.jitter ? R.jitter[r] : 0.f;
    y.em = R.em_modes ? (R.em_modes[r] == 1) : R.em_all;
    return y;
}

// sample j of ray y: continuous grid index and the out-of-box decision
__device__ __forceinline__ bool dvgo_sample(const DvgoRay &y, const DvgoGeom &g, int j, float p[3], float idx[3])
{
    dvgo_point(y.o, y.d, y.tmin, y.nrm, g.step_scale, dvgo_rng(j, y.u), p);
    esr_world_to_index(p, g.bmin, g.bmax, g.dims, idx);
    return y.miss || esr_out_of_box(p, g.bmin, g.bmax);
}

// ---------------------------------------------------------------------------
// forward: training (5 outputs + alpha for the backward) and evaluation (7 outputs)
// ---------------------------------------------------------------------------
template <bool EVAL>
__global__ void __launch_bounds__(DVGO_BLOCK) dvgo_fwd_kernel(esr_dvgo_t P, esr_dvgo_rays_t R, esr_dvgo_out_t O)
{
    const DvgoGeom g = dvgo_geom(P);
    const int S = P.n_samples;
    const int K = (S + ESR_WAVE - 1) / ESR_WAVE;
    const int lane = esr_lane();
    const int s0 = min(lane * K, S), s1 = min(s0 + K, S);
    for (int64_t r = (int64_t)blockIdx.x * DVGO_WAVES + threadIdx.x / ESR_WAVE; r < R.n_rays;
         r += (int64_t)gridDim.x * DVGO_WAVES) {
        const DvgoRay y = dvgo_ray(R, g, r);
        float *alpha = O.alpha + r * S;
        // pass 1: alpha of the run and its product of p
        float prod = 1.f;
        for (int j = s0; j < s1; ++j) {
            float p[3], idx[3];
            const bool masked = dvgo_sample(y, g, j, p, idx);
            float a = 0.f;
            if (!masked) a = dvgo_alpha(esr_tri_fetch1(P.density, g.dims, idx), P.act_shift, P.interval);
            alpha[j] = a;
            prod *= dvgo_pclamp(a);
        }
        float T = wave_excl_prod(prod);
        // pass 2: T, weights, colours
        float acc_off[3] = {0.f, 0.f, 0.f}, acc_emo[3] = {0.f, 0.f, 0.f}, acc_depth = 0.f;
        for (int j = s0; j < s1; ++j) {
            float p[3], idx[3];
            dvgo_sample(y, g, j, p, idx);
            const float a = alpha[j];
            const float w = a * T;
            float off[3], so[3];
            dvgo_fetch<3>(P.off_color, g.dims, idx, off);
            for (int c = 0; c < 3; ++c) so[c] = esr_sigmoid(off[c]);
            if (EVAL) {
                float emo[3];
                dvgo_fetch<3>(P.emo_color, g.dims, idx, emo);
                float dd[3];
                for (int c = 0; c < 3; ++c) {
                    acc_off[c] = __builtin_fmaf(w, so[c], acc_off[c]);
                    acc_emo[c] = __builtin_fmaf(w, esr_sigmoid(emo[c]), acc_emo[c]);
                    dd[c] = y.o[c] - p[c];
                }
                const float dist = esr_ray_norm(dd);
                acc_depth = __builtin_fmaf(w, dist, acc_depth);
            } else {
                O.alphainv_cum[r * (S + 1) + j] = T;
                O.weights[r * S + j] = w;
                float rgb[3] = {so[0], so[1], so[2]};
                if (y.em) {
                    float emo[3];
                    dvgo_fetch<3>(P.emo_color, g.dims, idx, emo);
                    for (int c = 0; c < 3; ++c) rgb[c] = esr_sigmoid(emo[c]) + so[c];
                }
                for (int c = 0; c < 3; ++c) {
                    O.raw_rgb[(r * S + j) * 3 + c] = rgb[c];
                    acc_off[c] = __builtin_fmaf(w, rgb[c], acc_off[c]);
                }
            }
            T *= dvgo_pclamp(a);
        }
        if (s1 == S && s0 < s1) {
            if (EVAL) O.white_bg[r] = T;
            else O.alphainv_cum[r * (S + 1) + S] = T;
        }
        for (int c = 0; c < 3; ++c) {
            acc_off[c] = esr_wave_sum(acc_off[c]);
            if (EVAL) acc_emo[c] = esr_wave_sum(acc_emo[c]);
        }
        if (EVAL) acc_depth = esr_wave_sum(acc_depth);
        // the lane that owns the last sample holds white_bg; every lane holds the sums
        if (EVAL) {
            const float wb = __shfl(T, (S - 1) / K, ESR_WAVE);
            if (lane == 0) {
                for (int c = 0; c < 3; ++c) {
                    O.off_rgb[r * 3 + c] = acc_off[c];
                    O.emo_rgb[r * 3 + c] = acc_emo[c];
                    O.on_rgb[r * 3 + c] = acc_off[c] + acc_emo[c];
                }
                O.depth[r] = acc_depth;
                O.disp[r] = 1.f / (acc_depth + wb * g.far_);
            }
        } else if (lane == 0) {
            for (int c = 0; c < 3; ++c) O.rgb[r * 3 + c] = acc_off[c];
        }
    }
}

// ---------------------------------------------------------------------------
// backward of the training forward
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(DVGO_BLOCK) dvgo_bwd_kernel(esr_dvgo_t P, esr_dvgo_rays_t R, esr_dvgo_bwd_t B)
{
    const DvgoGeom g = dvgo_geom(P);
    const int S = P.n_samples;
    const int K = (S + ESR_WAVE - 1) / ESR_WAVE;
    const int lane = esr_lane();
    const int s0 = min(lane * K, S), s1 = min(s0 + K, S);
    const int64_t plane = (int64_t)g.dims[0] * g.dims[1] * g.dims[2];
    float *const dst[7] = {B.grad_density,         B.grad_off,         B.grad_off + plane,  B.grad_off + 2 * plane,
                           B.grad_emo,             B.grad_emo + plane, B.grad_emo + 2 * plane};
    for (int64_t r = (int64_t)blockIdx.x * DVGO_WAVES + threadIdx.x / ESR_WAVE; r < R.n_rays;
         r += (int64_t)gridDim.x * DVGO_WAVES) {
        const DvgoRay y = dvgo_ray(R, g, r);
        const float *alpha = B.alpha + r * S;
        const float *Tc = B.alphainv_cum + r * (S + 1);
        const float *raw = B.raw_rgb + r * S * 3;
        float gC[3] = {0.f, 0.f, 0.f};
        if (B.g_rgb)
            for (int c = 0; c < 3; ++c) gC[c] = B.g_rgb[r * 3 + c];
        // dL/dw_j and g_j (the total gradient on T_j)
        auto dldw = [&](int j) {
            float v = B.g_weights ? B.g_weights[r * S + j] : 0.f;
            for (int c = 0; c < 3; ++c) v = __builtin_fmaf(gC[c], raw[j * 3 + c], v);
            return v;
        };
        // pass 1: this run's affine map R_{s0-1} = Bm + Am R_{s1-1}
        float Am = 1.f, Bm = 0.f;
        for (int j = s0; j < s1; ++j) {
            const float a = alpha[j];
            const float gj = (B.g_alphainv_cum ? B.g_alphainv_cum[r * (S + 1) + j] : 0.f) + dldw(j) * a;
            Bm = __builtin_fmaf(Am, gj, Bm);
            Am *= dvgo_pclamp(a);
        }
        wave_suffix_affine(Am, Bm);
        const float gS = B.g_alphainv_cum ? B.g_alphainv_cum[r * (S + 1) + S] : 0.f;
        float Rr = __builtin_fmaf(Am, gS, Bm);        // R_{s1-1}
        // pass 2, backwards along the run: dalpha, then the grids
        CellAcc<7> acc;
        acc_reset<7>(acc);
        for (int j = s1 - 1; j >= s0; --j) {
            const float a = alpha[j], T = Tc[j];
            const float pj = dvgo_pclamp(a);
            const float dw = dldw(j);
            const float gj = (B.g_alphainv_cum ? B.g_alphainv_cum[r * (S + 1) + j] : 0.f) + dw * a;
            const float dp = T * Rr;
            float da = dw * T;
            if (1.f - a >= 1e-10f) da -= dp;
            Rr = __builtin_fmaf(pj, Rr, gj);
            float p[3], idx[3];
            const bool masked = dvgo_sample(y, g, j, p, idx);
            float val[7];
            val[0] = 0.f;
            if (!masked) val[0] = da * dvgo_alpha_grad(esr_tri_fetch1(P.density, g.dims, idx), P.act_shift, P.interval);
            const float w = a * T;
            float draw[3];
            for (int c = 0; c < 3; ++c) {
                draw[c] = B.g_raw_rgb ? B.g_raw_rgb[(r * S + j) * 3 + c] : 0.f;
                draw[c] = __builtin_fmaf(gC[c], w, draw[c]);
            }
            float off[3];
            dvgo_fetch<3>(P.off_color, g.dims, idx, off);
            for (int c = 0; c < 3; ++c) {
                const float s = esr_sigmoid(off[c]);
                val[1 + c] = draw[c] * (1.f - s) * s;
                val[4 + c] = 0.f;
            }
            if (y.em) {
                float emo[3];
                dvgo_fetch<3>(P.emo_color, g.dims, idx, emo);
                for (int c = 0; c < 3; ++c) {
                    const float s = esr_sigmoid(emo[c]);
                    val[4 + c] = draw[c] * (1.f - s) * s;
                }
            }
            acc_sample<7>(acc, idx, val, dst, g.dims);
        }
        acc_flush<7>(acc, dst, g.dims);
    }
}

// ---------------------------------------------------------------------------
// voxel_count_views: one lane per ray, every one of the S samples (no jitter, no mask), weight 1 per sample
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(DVGO_BLOCK) dvgo_count_kernel(esr_dvgo_t P, esr_dvgo_rays_t R, float *sum)
{
    const DvgoGeom g = dvgo_geom(P);
    const int S = P.n_samples;
    float *const dst[1] = {sum};
    const float one[1] = {1.f};
    for (int64_t r = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x; r < R.n_rays; r += (int64_t)gridDim.x * DVGO_BLOCK) {
        DvgoRay y = dvgo_ray(R, g, r);
        y.u = 0.f;        // the view count's samples are unjittered whatever rays->jitter holds (esr_hip.h)
        CellAcc<1> acc;
        acc_reset<1>(acc);
        for (int j = 0; j < S; ++j) {
            float p[3], idx[3];
            dvgo_sample(y, g, j, p, idx);
            acc_sample<1>(acc, idx, one, dst, g.dims);
        }
        acc_flush<1>(acc, dst, g.dims);
    }
}

__global__ void dvgo_count_add_kernel(const float *__restrict__ sum, int64_t n, float *__restrict__ count)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        count[i] += sum[i] > 1.f ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static int dvgo_check(const esr_dvgo_t *P, const esr_dvgo_rays_t *R)
{
    if (!P || !R || R->n_rays < 0 || P->n_samples < 1) return ESR_EINVAL;
    for (int a = 0; a < 3; ++a)
        if (P->dims[a] < 1) return ESR_EINVAL;
    if (R->n_rays > 0 && (!R->rays_o || !R->rays_d || !R->nrm)) return ESR_EINVAL;
    return 0;
}

static int dvgo_wave_grid(int64_t n_rays)
{
    return esr_grid_for(n_rays, DVGO_WAVES, 256 * 64);
}

ESR_API int esr_dvgo_fwd(const esr_dvgo_t *P, const esr_dvgo_rays_t *R, const esr_dvgo_out_t *O, void *stream)
{
    if (int e = dvgo_check(P, R)) return e;
    if (!O || !P->density || !P->off_color || !P->emo_color) return ESR_EINVAL;
    if (R->n_rays == 0) return 0;
    if (!O->alpha || !O->alphainv_cum || !O->weights || !O->raw_rgb || !O->rgb) return ESR_EINVAL;
    hipLaunchKernelGGL(dvgo_fwd_kernel<false>, dim3(dvgo_wave_grid(R->n_rays)), dim3(DVGO_BLOCK), 0, esr_stream(stream),
                       *P, *R, *O);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_dvgo_eval(const esr_dvgo_t *P, const esr_dvgo_rays_t *R, const esr_dvgo_out_t *O, void *stream)
{
    if (int e = dvgo_check(P, R)) return e;
    if (!O || !P->density || !P->off_color || !P->emo_color) return ESR_EINVAL;
    if (R->n_rays == 0) return 0;
    if (!O->alpha || !O->depth || !O->disp || !O->white_bg || !O->off_rgb || !O->on_rgb || !O->emo_rgb)
        return ESR_EINVAL;
    hipLaunchKernelGGL(dvgo_fwd_kernel<true>, dim3(dvgo_wave_grid(R->n_rays)), dim3(DVGO_BLOCK), 0, esr_stream(stream),
                       *P, *R, *O);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_dvgo_bwd(const esr_dvgo_t *P, const esr_dvgo_rays_t *R, const esr_dvgo_bwd_t *B, void *stream)
{
    if (int e = dvgo_check(P, R)) return e;
    if (!B || !P->density || !P->off_color || !P->emo_color || !B->grad_density || !B->grad_off || !B->grad_emo)
        return ESR_EINVAL;
    if (R->n_rays == 0) return 0;
    if (!B->alpha || !B->alphainv_cum || !B->raw_rgb) return ESR_EINVAL;
    hipLaunchKernelGGL(dvgo_bwd_kernel, dim3(dvgo_wave_grid(R->n_rays)), dim3(DVGO_BLOCK), 0, esr_stream(stream), *P,
                       *R, *B);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_dvgo_count(const esr_dvgo_t *P, const esr_dvgo_rays_t *R, float *sum, void *stream)
{
    if (int e = dvgo_check(P, R)) return e;
    if (!sum) return ESR_EINVAL;
    if (R->n_rays == 0) return 0;
    hipLaunchKernelGGL(dvgo_count_kernel, dim3(esr_grid_for(R->n_rays, DVGO_BLOCK, 256 * 64)), dim3(DVGO_BLOCK), 0,
                       esr_stream(stream), *P, *R, sum);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_dvgo_count_add(const float *sum, int64_t n, float *count, void *stream)
{
    if (n < 0 || (n > 0 && (!sum || !count))) return ESR_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(dvgo_count_add_kernel, dim3(esr_grid_for(n, 256)), dim3(256), 0, esr_stream(stream), sum, n,
                       count);
    ESR_CHECK_LAUNCH();
    return 0;
}
