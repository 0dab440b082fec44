// What the two sources of PDRA's ray re-split share (regroup.hip: one byte per flag; regroup_dp.hip: one bit per flag):
// the integer key space of the statistics with its reductions, the record's identity, and the one-block scan of the tile
// counts.  Every kernel here sits in the unnamed namespace: a source holds the ones it launches and no others.
#pragma once
#include "esr_common.h"

#include <math.h>

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / ESR_WAVE;
constexpr int RG_ROUNDS = ESR_PARTITION_BLOCK / RG_THREADS;
constexpr int RG_SCAN_PER_THREAD = ESR_PARTITION_SCAN_TILE / RG_THREADS;
static_assert(ESR_PARTITION_BLOCK % RG_THREADS == 0 && ESR_PARTITION_SCAN_TILE % RG_THREADS == 0, "whole rounds");

constexpr int64_t RG_MAX_N = (int64_t)1 << 31;

constexpr int32_t KEY_POS_INF = 0x7f800000;                 // key of +inf: the identity of a minimum
constexpr int32_t KEY_NEG_INF = (int32_t)0x807fffff;        // key of -inf: the identity of a maximum

__device__ __forceinline__ int32_t key_of(float v)
{
    const int32_t b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}

__device__ __forceinline__ float float_of(int32_t k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__device__ __forceinline__ void atomic_min_float(float *addr, float v)
{
    if (__float_as_int(v) >= 0) atomicMin(reinterpret_cast<int *>(addr), __float_as_int(v));
    else                        atomicMax(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}

__device__ __forceinline__ void atomic_max_float(float *addr, float v)
{
    if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int *>(addr), __float_as_int(v));
    else                        atomicMin(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}

__global__ void regroup_stats_init_kernel(esr_regroup_stats_t *stats)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        stats->n_set = 0; stats->n_clear = 0; stats->n_nan = 0;
        stats->min_all = INFINITY; stats->max_all = -INFINITY;
        stats->min_set = INFINITY; stats->max_set = -INFINITY;
        stats->min_clear = INFINITY; stats->max_clear = -INFINITY;
    }
}

// slots of the block reduction: minima 0..2 (all, set, clear), maxima 3..5, counts 6..8 (set, clear, nan)
constexpr int RG_SLOTS = 9;
#define RG_SLOTS_IDENTITY {KEY_POS_INF, KEY_POS_INF, KEY_POS_INF, KEY_NEG_INF, KEY_NEG_INF, KEY_NEG_INF, 0, 0, 0}

// ray r of emission [n,3]: its flag, and its share of this thread's nine slots
__device__ __forceinline__ bool decide_ray(const float *__restrict__ emission, int64_t r, float k_val, int32_t (&v)[RG_SLOTS])
{
    const float e[3] = {emission[3 * r], emission[3 * r + 1], emission[3 * r + 2]};
    const bool nan = e[0] != e[0] || e[1] != e[1] || e[2] != e[2];
    const float m = fmaxf(fmaxf(e[0], e[1]), e[2]);              // (only used when no channel is a NaN)
    const bool set = !nan && m > k_val;
    int32_t lo = KEY_POS_INF, hi = KEY_NEG_INF;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (e[c] == e[c]) {
            const int32_t k = key_of(e[c]);
            lo = min(lo, k);
            hi = max(hi, k);
        }
    v[0] = min(v[0], lo); v[3] = max(v[3], hi);
    if (set) { v[1] = min(v[1], lo); v[4] = max(v[4], hi); v[6] += 1; }
    else     { v[2] = min(v[2], lo); v[5] = max(v[5], hi); v[7] += 1; }
    v[8] += nan ? 1 : 0;
    return set;
}

// the nine slots of a wave's lanes into every lane
__device__ __forceinline__ void decide_wave_reduce(int32_t (&v)[RG_SLOTS])
{
#pragma unroll
    for (int s = 0; s < RG_SLOTS; ++s) {
#pragma unroll
        for (int o = ESR_WAVE / 2; o > 0; o >>= 1) {
            const int32_t other = __shfl_xor(v[s], o);
            v[s] = s < 3 ? min(v[s], other) : s < 6 ? max(v[s], other) : v[s] + other;
        }
    }
}

// the slots of a block's RG_THREADS threads into *stats: shuffles, LDS, nine vector atomics by nine lanes
__device__ __forceinline__ void decide_block_merge(int32_t (&v)[RG_SLOTS], int32_t (*red)[RG_SLOTS], esr_regroup_stats_t *stats)
{
    decide_wave_reduce(v);
    const int wave = threadIdx.x >> 6;
    if (esr_lane() == 0) {
#pragma unroll
        for (int s = 0; s < RG_SLOTS; ++s) red[wave][s] = v[s];
    }
    __syncthreads();
    if (threadIdx.x < RG_SLOTS) {
        const int s = threadIdx.x;
        int32_t a = red[0][s];
        for (int w = 1; w < RG_WAVES; ++w) {
            const int32_t b = red[w][s];
            a = s < 3 ? min(a, b) : s < 6 ? max(a, b) : a + b;
        }
        float *mins = &stats->min_all, *maxs = &stats->max_all;      // (declared in pairs: min_all, max_all, min_set, ...)
        if (s < 3)      { if (a != KEY_POS_INF) atomic_min_float(mins + 2 * s, float_of(a)); }
        else if (s < 6) { if (a != KEY_NEG_INF) atomic_max_float(maxs + 2 * (s - 3), float_of(a)); }
        else if (a)     atomicAdd(reinterpret_cast<unsigned long long *>(&stats->n_set) + (s - 6), (unsigned long long)a);
    }
}

// one block: counts -> exclusive offsets in place, totals = (set, n - set)
__global__ void __launch_bounds__(RG_THREADS) flag_scan_kernel(int64_t *__restrict__ block_offsets, int64_t n_tiles, int64_t n,
                                                               int64_t *__restrict__ totals)
{
    __shared__ int64_t wave_sum[RG_WAVES];
    const int lane = esr_lane(), wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += ESR_PARTITION_SCAN_TILE) {
        const int64_t first = t0 + (int64_t)threadIdx.x * RG_SCAN_PER_THREAD;
        int64_t c[RG_SCAN_PER_THREAD], mine = 0;
#pragma unroll
        for (int k = 0; k < RG_SCAN_PER_THREAD; ++k) {
            c[k] = first + k < n_tiles ? block_offsets[first + k] : 0;
            mine += c[k];
        }
        int64_t incl = mine;
#pragma unroll
        for (int o = 1; o < ESR_WAVE; o <<= 1) {
            const int64_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == ESR_WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry, trip = 0;
#pragma unroll
        for (int w = 0; w < RG_WAVES; ++w) {
            const int64_t s = wave_sum[w];
            if (w < wave) before += s;
            trip += s;
        }
        int64_t run = before + incl - mine;
#pragma unroll
        for (int k = 0; k < RG_SCAN_PER_THREAD; ++k) {
            if (first + k < n_tiles) block_offsets[first + k] = run;
            run += c[k];
        }
        carry += trip;
        __syncthreads();                                             // (wave_sum is rewritten by the next trip)
    }
    if (threadIdx.x == 0) {
        totals[0] = carry;
        totals[1] = n - carry;
    }
}

}  // namespace
