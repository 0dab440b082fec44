// PDRA's ray re-split: the per-ray decision with its statistics, and the stable two-way partition of an index vector.
//
// Reference algorithm (paths under the reference tree):
//   app/fine/pdra.py:911          uncert_masks = torch.max(emission, dim=-1)[0] > k_val
//   app/fine/pdra.py:912-925      the five printed numbers (max / min of all, of the uncertain and of the certain rays)
//   utils2/utils.py:234-267       RayGroupManager.filter: uncertain <- uncertain[mask], certain <- cat(certain, uncertain[~mask])
// The reference keeps an [n,3] emission buffer, takes five boolean-index passes over it for the prints (each with its own
// synchronisation) and two boolean indexings plus a concatenation per array for the regrouping.
//
// esr_emit_decide: one grid-stride launch, one thread per ray.  flag = max over the three channels > k_val as a binary32
// comparison; torch.max propagates a NaN, and NaN > k is false, so a ray with a NaN channel is clear.  Minima and maxima
// are reduced in an integer key space (key = bits for a float with a clear sign bit, bits ^ 0x7fffffff otherwise: a total
// order, -0.0 below +0.0), so they depend on no order of arrival and on no rounding mode; NaN elements take no part.  A wave
// reduces by shuffles, a block through LDS, and one lane issues nine vector atomics per block: three 64-bit adds and six
// 32-bit integer min / max on the float's bits (a non-negative float orders as a signed integer, a negative one in reverse
// as an unsigned one).  With accumulate == 0 a one-thread launch in front writes the identity (0, +inf, -inf).
//
// esr_flag_scan / esr_index_partition: three launches in stream order, no block waits for another one.
//   count     one block per tile of ESR_PARTITION_BLOCK flags: ballot + popcount per wave, four waves through LDS
//   scan      ONE block walks the tile counts, ESR_PARTITION_SCAN_TILE per trip (four per thread, shuffle scan inside a
//             wave, wave totals through LDS, a running carry), turns them into exclusive offsets in place and writes
//             totals = (set, clear)
//   scatter   one block per tile; round j of a tile covers 256 consecutive flags, one per lane, so wave w of round j owns
//             64 consecutive rows: rank inside the wave = popcount(ballot & lanes below), the (round, wave) counts go
//             through LDS, every thread sums the ones in front of its own.  A set row goes to
//             set_out[block_offsets[tile] + rank], a clear row i to clear_out[i - (set flags before i)].
// Traffic: 1 B per flag twice, 8 B read and 8 B written per row.  Both outputs are written in input order (stable).
#include "regroup_common.h"      // the key space and its reductions, the record's identity, the one-block scan

namespace {

__global__ void __launch_bounds__(RG_THREADS) emit_decide_kernel(const float *__restrict__ emission, int64_t n, float k_val,
                                                                 uint8_t *__restrict__ flags, esr_regroup_stats_t *stats)
{
    __shared__ int32_t red[RG_WAVES][RG_SLOTS];
    int32_t v[RG_SLOTS] = RG_SLOTS_IDENTITY;
    const int64_t stride = (int64_t)gridDim.x * RG_THREADS;
    for (int64_t r = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x; r < n; r += stride)
        flags[r] = decide_ray(emission, r, k_val, v) ? 1 : 0;
    decide_block_merge(v, red, stats);
}

// the 64-bit ballot of a wave's 64 consecutive flags (a lane past the end votes 0; callers take the popcount), and this
// lane's flag
__device__ __forceinline__ unsigned long long flag_ballot(const uint8_t *__restrict__ flags, int64_t i, int64_t n, bool &set)
{
    set = i < n && flags[i] != 0;
    return __ballot(set);
}

__global__ void __launch_bounds__(RG_THREADS) flag_count_kernel(const uint8_t *__restrict__ flags, int64_t n,
                                                                int64_t *__restrict__ block_counts)
{
    __shared__ int32_t cnt[RG_WAVES];
    const int64_t base = (int64_t)blockIdx.x * ESR_PARTITION_BLOCK;
    int32_t c = 0;
#pragma unroll
    for (int j = 0; j < RG_ROUNDS; ++j) {
        bool set;
        c += __popcll(flag_ballot(flags, base + j * RG_THREADS + threadIdx.x, n, set));
    }
    if (esr_lane() == 0) cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < RG_WAVES; ++w) t += cnt[w];
        block_counts[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(RG_THREADS) index_partition_kernel(const int64_t *__restrict__ rows,
                                                                     const uint8_t *__restrict__ flags,
                                                                     const int64_t *__restrict__ block_offsets, int64_t n,
                                                                     int64_t *__restrict__ set_out,
                                                                     int64_t *__restrict__ clear_out)
{
    __shared__ int32_t cnt[RG_ROUNDS][RG_WAVES];
    const int lane = esr_lane(), wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * ESR_PARTITION_BLOCK;
    const unsigned long long below = (1ull << lane) - 1ull;
    bool set[RG_ROUNDS];
    int32_t rank[RG_ROUNDS];
#pragma unroll
    for (int j = 0; j < RG_ROUNDS; ++j) {
        const unsigned long long b = flag_ballot(flags, base + j * RG_THREADS + threadIdx.x, n, set[j]);
        rank[j] = __popcll(b & below);
        if (lane == 0) cnt[j][wave] = __popcll(b);
    }
    __syncthreads();
    const int64_t tile_off = block_offsets[blockIdx.x];
    int32_t done = 0;                                                // set flags of the rounds in front of round j
#pragma unroll
    for (int j = 0; j < RG_ROUNDS; ++j) {
        int32_t here = done;                                         // ... plus those of round j's waves in front of this one
#pragma unroll
        for (int w = 0; w < RG_WAVES; ++w) {
            const int32_t c = cnt[j][w];
            if (w < wave) here += c;
            done += c;
        }
        const int64_t i = base + j * RG_THREADS + threadIdx.x;
        if (i < n) {
            const int64_t pos = tile_off + here + rank[j];           // set flags in front of row i
            const int64_t row = rows[i];
            if (set[j]) { if (set_out) set_out[pos] = row; }         // (an output of size 0 may be NULL)
            else if (clear_out) clear_out[i - pos] = row;
        }
    }
}

}  // namespace

ESR_API int esr_emit_decide(const float *emission, int64_t n, float k_val, uint8_t *flags, esr_regroup_stats_t *stats,
                            int accumulate, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!emission || !flags || !stats || ((uintptr_t)emission & 3) || ((uintptr_t)stats & 7)) return ESR_EINVAL;
    if (!accumulate) {
        regroup_stats_init_kernel<<<1, ESR_WAVE, 0, esr_stream(stream)>>>(stats);
        ESR_CHECK_LAUNCH();
    }
    emit_decide_kernel<<<esr_grid_for(n, RG_THREADS, 1024), RG_THREADS, 0, esr_stream(stream)>>>(emission, n, k_val, flags,
                                                                                                 stats);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_flag_scan(const uint8_t *flags, int64_t n, int64_t *block_offsets, int64_t *totals, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!flags || !block_offsets || !totals || ((uintptr_t)block_offsets & 7) || ((uintptr_t)totals & 7)) return ESR_EINVAL;
    const int64_t n_tiles = (n + ESR_PARTITION_BLOCK - 1) / ESR_PARTITION_BLOCK;
    flag_count_kernel<<<(int)n_tiles, RG_THREADS, 0, esr_stream(stream)>>>(flags, n, block_offsets);
    ESR_CHECK_LAUNCH();
    flag_scan_kernel<<<1, RG_THREADS, 0, esr_stream(stream)>>>(block_offsets, n_tiles, n, totals);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_index_partition(const int64_t *rows, const uint8_t *flags, const int64_t *block_offsets, int64_t n,
                                int64_t *set_out, int64_t *clear_out, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!rows || !flags || !block_offsets || (!set_out && !clear_out)) return ESR_EINVAL;
    if (((uintptr_t)rows | (uintptr_t)block_offsets | (uintptr_t)set_out | (uintptr_t)clear_out) & 7) return ESR_EINVAL;
    const int64_t n_tiles = (n + ESR_PARTITION_BLOCK - 1) / ESR_PARTITION_BLOCK;
    index_partition_kernel<<<(int)n_tiles, RG_THREADS, 0, esr_stream(stream)>>>(rows, flags, block_offsets, n, set_out,
                                                                               clear_out);
    ESR_CHECK_LAUNCH();
    return 0;
}
