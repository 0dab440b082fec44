// Wave and workgroup collectives shared by the kernels of libesr_hip.so (gfx950, wave64).  A change of a barrier or of the
// order of additions here changes result bits in every includer; the per-value float64 tests pin them.
//
// Reduction shapes that are deliberately NOT here (their bits differ from the ones below):
//   simplify.hip block_sum            double; x[t] += x[t + off]: the two steps across the waves through LDS, the six inside
//                                     wave 0 by lane shifts; the result is thread 0's alone.
//   lts.hip block_sum                 float; wave butterfly (esr_wave_sum), then a serial sum over the waves in every thread.
//   gridsetup.hip block_count_add     unsigned count, one LDS slot per wave, one integer atomic per workgroup; one user.
//   march.hip, regroup.hip, meshcc.hip (acc_*)   butterflies over several values interleaved per step: the interleaving
//                                     belongs to their kernels.
//   regroup.hip, meshcc.hip           the ordered-float atomics look alike but treat -0 differently: regroup keys on the sign
//                                     bit, meshcc adds +0 first.  Both behaviours are pinned by tests.
#pragma once
#include "esr_common.h"

#include <math.h>

// the wave's sum of `v` in every lane: a butterfly (off = 32 .. 1), each step one commutative addition, so all lanes hold
// the same bits.  No barrier; every lane of the wave calls it.
__device__ __forceinline__ float esr_wave_sum(float v)
{
#pragma unroll
    for (int off = ESR_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, ESR_WAVE);
    return v;
}

// segmented inclusive scan over the 64 lanes (segments = runs of equal id): lane l returns the sum of `v` over the lanes
// <= l of its run, added at distances off = 1, 2 .. 32.  No barrier; every lane of the wave calls it.
__device__ __forceinline__ float esr_wave_segscan_add(float v, int id, int lane)
{
#pragma unroll
    for (int off = 1; off < ESR_WAVE; off <<= 1) {
        const float u = __shfl_up(v, off);
        const int iu = __shfl_up(id, off);
        if (lane >= off && iu == id) v += u;
    }
    return v;
}

// exclusive scan of one int per lane over the block; `total` = the block's sum.  Every thread calls it; tmp [THREADS / 64]
// in LDS; two barriers, the second after the last read of tmp (the next call may rewrite it at once).
template <int THREADS>
__device__ __forceinline__ int esr_block_scan_excl(int v, int *tmp, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) tmp[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) {
        const int t = tmp[k];
        if (k < w) base += t;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// the wave's minimum of lo[] and maximum of hi[] in every lane (xor-shuffle butterfly); no barrier
__device__ __forceinline__ void esr_wave_minmax3(float lo[3], float hi[3])
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, ESR_WAVE));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, ESR_WAVE));
        }
}

// one 6-float result per workgroup from per-lane running values: wave reduction, then the workgroup's waves through LDS.
// Every thread calls it, once per kernel (one barrier, none behind the reads); threads 0 .. 5 write out6[0 .. 5].
template <int THREADS>
__device__ __forceinline__ void esr_block_minmax3_store(float lo[3], float hi[3], float *__restrict__ out6)
{
    __shared__ float part[THREADS / ESR_WAVE][6];
    esr_wave_minmax3(lo, hi);
    const int wave = threadIdx.x >> 6;
    if (esr_lane() == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[wave][a] = lo[a]; part[wave][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = part[0][threadIdx.x];
        for (int w = 1; w < THREADS / ESR_WAVE; ++w)
            v = threadIdx.x < 3 ? fminf(v, part[w][threadIdx.x]) : fmaxf(v, part[w][threadIdx.x]);
        out6[threadIdx.x] = v;
    }
}

// folds n 6-float partials (esr_block_minmax3_store's) into out6 in one workgroup: the body of a <<<1, THREADS>>> kernel
template <int THREADS>
__device__ __forceinline__ void esr_minmax3_partials(const float *__restrict__ partials, int n, float *__restrict__ out6)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < n; b += THREADS)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], partials[6 * b + a]);
            hi[a] = fmaxf(hi[a], partials[6 * b + 3 + a]);
        }
    esr_block_minmax3_store<THREADS>(lo, hi, out6);
}

// sum of the workgroup's `v` (fixed tree, red[t] += red[t + s] for s = THREADS / 2 .. 1: the same bits on every run) in
// every thread; red [THREADS] in LDS.  Every thread calls it; a barrier in front of the first write of red and one behind
// every step.
template <int THREADS>
__device__ __forceinline__ double esr_block_sum_tree(double v, double *red)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// out[0] = (partials[0] + ... + partials[n-1]) / div, summed in a fixed order by one workgroup: the body of a
// <<<1, THREADS>>> kernel
template <int THREADS>
__device__ __forceinline__ void esr_sum_partials(const double *__restrict__ partials, int n, double div,
                                                 double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double red[THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += THREADS) acc = acc + partials[i];
    const double s = esr_block_sum_tree<THREADS>(acc, red);
    if (threadIdx.x == 0) out[0] = s / div;
}
