// PDRA's ray re-split: the per-ray decision with its statistics, and the stable two-way partition of an index vector on
// packed flag words.
//
// Reference algorithm (paths under the reference tree):
//   app/fine/pdra.py:911          uncert_masks = torch.max(emission, dim=-1)[0] > k_val
//   app/fine/pdra.py:912-925      the five printed numbers (max / min of all, of the uncertain and of the certain rays)
//   utils2/utils.py:234-267       RayGroupManager.filter: uncertain <- uncertain[mask], certain <- cat(certain, uncertain[~mask])
// The reference keeps an [n,3] emission buffer, takes five boolean-index passes over it for the prints (each with its own
// synchronisation) and two boolean indexings plus a concatenation per array for the regrouping.
//
// The decision: one grid-stride launch, one thread per ray.  flag = max over the three channels > k_val as a binary32
// comparison; torch.max propagates a NaN, and NaN > k is false, so a ray with a NaN channel is clear.  Minima and maxima
// are reduced in an integer key space (key = bits for a float with a clear sign bit, bits ^ 0x7fffffff otherwise: a total
// order, -0.0 below +0.0), so they depend on no order of arrival and on no rounding mode; NaN elements take no part.  A wave
// reduces by shuffles, a block through LDS, and nine lanes issue nine vector atomics per block: three 64-bit adds and six
// 32-bit integer min / max on the float's bits (a non-negative float orders as a signed integer, a negative one in reverse
// as an unsigned one).  With accumulate == 0 a one-thread launch in front writes the identity (0, +inf, -inf).
//   esr_emit_decide        one byte per flag: a chunk may start at any ray of a flag vector
//   esr_emit_decide_bits   one bit per flag: a wave walks whole words and lane 0 stores the ballot, so a chunk starts on a
//                          word.  Under data parallelism every rank decides its share of the uncertain group into its words of
//                          ONE preallocated vector; shares are cut at word boundaries, so an integer SUM all-reduce of the
//                          vector (zero outside a rank's share) is the union of the decisions.
//
// Packed format: bit b of word w is the flag of ray 64 w + b, bit 0 the least significant; the bits at and above n in the
// last word are 0; words are 8-byte aligned.  Every writer here stores whole words with the tail clear, every reader masks
// the tail of the last word all the same (one scalar AND).
//
// esr_flags_pack / esr_flags_unpack   byte flags <-> words (a non-zero byte is a set bit; unpack writes 0 or 1)
// esr_flag_scan_bits / esr_index_partition_bits: three launches in stream order, no block waits for another one.
//   count     per tile of ESR_PARTITION_BLOCK flags = 16 words: one word per lane, popcount, a shuffle sum over the 16 lanes
//             of a tile (a block covers 16 tiles)
//   scan      ONE block walks the tile counts, ESR_PARTITION_SCAN_TILE per trip (four per thread, shuffle scan inside a
//             wave, wave totals through LDS, a running carry), turns them into exclusive offsets in place and writes
//             totals = (set, clear)
//   scatter   one block per tile.  The tile's 16 words are wave-uniform: they arrive by scalar loads and every wave takes
//             the popcounts of the words in front of its own with scalar instructions -- no LDS, no barrier.  A lane's flag
//             is its bit, its rank popcount(word & lanes below).  A set row goes to set_out[block_offsets[tile] + rank], a
//             clear row i to clear_out[i - (set flags before i)].
// esr_regroup_stats_merge    one wave: the records of the ranks into one, counts added, minima and maxima in the key space
// Traffic of scan + partition: 1/8 B per flag twice, 8 B read and 8 B written per row.  Both outputs are written in input
// order (stable).
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

typedef unsigned long long word_t;
constexpr int DP_TILE_WORDS = ESR_PARTITION_BLOCK / ESR_WAVE;          // 16
constexpr int DP_TILES_PER_BLOCK = RG_THREADS / DP_TILE_WORDS;         // of the count kernel: 16
static_assert(ESR_PARTITION_BLOCK % ESR_WAVE == 0 && RG_THREADS % DP_TILE_WORDS == 0, "whole words, whole tiles");
static_assert(DP_TILE_WORDS == RG_ROUNDS * RG_WAVES, "round j, wave w of the partition owns word j * RG_WAVES + w of its tile");

// word wi of the n flags (0 past the end), the bits at and above n cleared
__device__ __forceinline__ word_t load_word(const word_t *__restrict__ words, int64_t wi, int64_t n_words, int64_t n)
{
    if (wi >= n_words) return 0;
    word_t w = words[wi];
    const int tail = (int)(n & 63);
    if (wi == n_words - 1 && tail) w &= (1ull << tail) - 1ull;
    return w;
}

// A wave's 64 lanes stay on one word: the loops below run on the wave's first ray r0, which is wave-uniform, so every lane
// takes part in the ballot (a lane past the end votes 0: the tail of the last word is clear).
#define DP_FOR_EACH_WORD(r0, n) \
    for (int64_t r0 = (int64_t)blockIdx.x * RG_THREADS + (threadIdx.x & ~(ESR_WAVE - 1)); r0 < (n); r0 += (int64_t)gridDim.x * RG_THREADS)

__global__ void __launch_bounds__(RG_THREADS) emit_decide_bits_kernel(const float *__restrict__ emission, int64_t n, float k_val,
                                                                      word_t *__restrict__ words, esr_regroup_stats_t *stats)
{
    __shared__ int32_t red[RG_WAVES][RG_SLOTS];
    int32_t v[RG_SLOTS] = RG_SLOTS_IDENTITY;
    const int lane = esr_lane();
    DP_FOR_EACH_WORD(r0, n) {
        const int64_t r = r0 + lane;
        const bool set = r < n && decide_ray(emission, r, k_val, v);
        const word_t b = __ballot(set);
        if (lane == 0) words[r0 >> 6] = b;
    }
    decide_block_merge(v, red, stats);
}

__global__ void __launch_bounds__(RG_THREADS) flags_pack_kernel(const uint8_t *__restrict__ flags, int64_t n,
                                                                word_t *__restrict__ words)
{
    const int lane = esr_lane();
    DP_FOR_EACH_WORD(r0, n) {
        const int64_t r = r0 + lane;
        const word_t b = __ballot(r < n && flags[r] != 0);
        if (lane == 0) words[r0 >> 6] = b;
    }
}

__global__ void __launch_bounds__(RG_THREADS) flags_unpack_kernel(const word_t *__restrict__ words, int64_t n,
                                                                  uint8_t *__restrict__ flags)
{
    const int lane = esr_lane();
    DP_FOR_EACH_WORD(r0, n) {
        const word_t w = words[r0 >> 6];
        if (r0 + lane < n) flags[r0 + lane] = (uint8_t)((w >> lane) & 1ull);
    }
}

__global__ void __launch_bounds__(RG_THREADS) flag_count_bits_kernel(const word_t *__restrict__ words, int64_t n, int64_t n_words,
                                                                     int64_t n_tiles, int64_t *__restrict__ block_counts)
{
    const int64_t wi = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    int32_t c = __popcll(load_word(words, wi, n_words, n));
#pragma unroll
    for (int o = DP_TILE_WORDS / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    const int64_t tile = wi / DP_TILE_WORDS;
    if ((threadIdx.x & (DP_TILE_WORDS - 1)) == 0 && tile < n_tiles) block_counts[tile] = c;
}

__global__ void __launch_bounds__(RG_THREADS) index_partition_bits_kernel(const int64_t *__restrict__ rows,
                                                                          const word_t *__restrict__ words,
                                                                          const int64_t *__restrict__ block_offsets, int64_t n,
                                                                          int64_t n_words, int64_t *__restrict__ set_out,
                                                                          int64_t *__restrict__ clear_out)
{
    const int lane = esr_lane();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t base = (int64_t)blockIdx.x * ESR_PARTITION_BLOCK;
    const int64_t w0 = (int64_t)blockIdx.x * DP_TILE_WORDS;
    const word_t below = (1ull << lane) - 1ull;
    const int64_t tile_off = block_offsets[blockIdx.x];
    int32_t done = 0;                                                // set flags of the rounds in front of round j
#pragma unroll
    for (int j = 0; j < RG_ROUNDS; ++j) {
        int32_t here = done;                                         // ... plus those of round j's waves in front of this one
        word_t mine = 0;
#pragma unroll
        for (int w = 0; w < RG_WAVES; ++w) {
            const word_t word = load_word(words, w0 + j * RG_WAVES + w, n_words, n);
            const int32_t c = __popcll(word);
            if (w < wave) here += c;
            if (w == wave) mine = word;
            done += c;
        }
        const int64_t i = base + j * RG_THREADS + threadIdx.x;
        if (i < n) {
            const int64_t pos = tile_off + here + __popcll(mine & below);      // set flags in front of row i
            const int64_t row = rows[i];
            if ((mine >> lane) & 1ull) { if (set_out) set_out[pos] = row; }    // (an output of size 0 may be NULL)
            else if (clear_out) clear_out[i - pos] = row;
        }
    }
}

// one wave; `out` may be one of the parts (every read is in front of the one write)
__global__ void __launch_bounds__(ESR_WAVE) regroup_stats_merge_kernel(const esr_regroup_stats_t *parts, int64_t n_parts,
                                                                      esr_regroup_stats_t *out)
{
    int32_t k[6] = {KEY_POS_INF, KEY_POS_INF, KEY_POS_INF, KEY_NEG_INF, KEY_NEG_INF, KEY_NEG_INF};   // minima, then maxima
    long long c[3] = {0, 0, 0};
    for (int64_t p = esr_lane(); p < n_parts; p += ESR_WAVE) {
        const esr_regroup_stats_t rec = parts[p];
        const float lo[3] = {rec.min_all, rec.min_set, rec.min_clear}, hi[3] = {rec.max_all, rec.max_set, rec.max_clear};
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            k[s] = min(k[s], key_of(lo[s]));
            k[3 + s] = max(k[3 + s], key_of(hi[s]));
        }
        c[0] += rec.n_set; c[1] += rec.n_clear; c[2] += rec.n_nan;
    }
#pragma unroll
    for (int o = ESR_WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int32_t other = __shfl_xor(k[s], o);
            k[s] = s < 3 ? min(k[s], other) : max(k[s], other);
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) c[s] += __shfl_xor(c[s], o);
    }
    if (esr_lane() == 0) {
        out->n_set = c[0]; out->n_clear = c[1]; out->n_nan = c[2];
        out->min_all = float_of(k[0]); out->max_all = float_of(k[3]);
        out->min_set = float_of(k[1]); out->max_set = float_of(k[4]);
        out->min_clear = float_of(k[2]); out->max_clear = float_of(k[5]);
    }
}

__host__ inline bool misaligned8(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 7) != 0;
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

ESR_API int esr_emit_decide_bits(const float *emission, int64_t n, float k_val, uint64_t *words, esr_regroup_stats_t *stats,
                                 int accumulate, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!emission || !words || !stats || ((uintptr_t)emission & 3) || misaligned8(words, stats)) return ESR_EINVAL;
    if (!accumulate) {
        regroup_stats_init_kernel<<<1, ESR_WAVE, 0, esr_stream(stream)>>>(stats);
        ESR_CHECK_LAUNCH();
    }
    emit_decide_bits_kernel<<<esr_grid_for(n, RG_THREADS, 1024), RG_THREADS, 0, esr_stream(stream)>>>(
        emission, n, k_val, reinterpret_cast<word_t *>(words), stats);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_flags_pack(const uint8_t *flags, int64_t n, uint64_t *words, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!flags || !words || misaligned8(words)) return ESR_EINVAL;
    flags_pack_kernel<<<esr_grid_for(n, RG_THREADS), RG_THREADS, 0, esr_stream(stream)>>>(flags, n,
                                                                                          reinterpret_cast<word_t *>(words));
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_flags_unpack(const uint64_t *words, int64_t n, uint8_t *flags, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!flags || !words || misaligned8(words)) return ESR_EINVAL;
    flags_unpack_kernel<<<esr_grid_for(n, RG_THREADS), RG_THREADS, 0, esr_stream(stream)>>>(
        reinterpret_cast<const word_t *>(words), n, flags);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_flag_scan_bits(const uint64_t *words, int64_t n, int64_t *block_offsets, int64_t *totals, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!words || !block_offsets || !totals || misaligned8(words, block_offsets, totals)) return ESR_EINVAL;
    const int64_t n_words = (n + ESR_WAVE - 1) / ESR_WAVE;
    const int64_t n_tiles = (n + ESR_PARTITION_BLOCK - 1) / ESR_PARTITION_BLOCK;
    flag_count_bits_kernel<<<(int)((n_tiles + DP_TILES_PER_BLOCK - 1) / DP_TILES_PER_BLOCK), RG_THREADS, 0, esr_stream(stream)>>>(
        reinterpret_cast<const word_t *>(words), n, n_words, n_tiles, block_offsets);
    ESR_CHECK_LAUNCH();
    flag_scan_kernel<<<1, RG_THREADS, 0, esr_stream(stream)>>>(block_offsets, n_tiles, n, totals);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_index_partition_bits(const int64_t *rows, const uint64_t *words, const int64_t *block_offsets, int64_t n,
                                     int64_t *set_out, int64_t *clear_out, void *stream)
{
    if (n < 0) return ESR_EINVAL;
    if (n >= RG_MAX_N) return ESR_ECAP;
    if (!n) return 0;
    if (!rows || !words || !block_offsets || (!set_out && !clear_out)) return ESR_EINVAL;
    if (misaligned8(rows, words, block_offsets) || misaligned8(set_out, clear_out)) return ESR_EINVAL;
    const int64_t n_words = (n + ESR_WAVE - 1) / ESR_WAVE;
    const int64_t n_tiles = (n + ESR_PARTITION_BLOCK - 1) / ESR_PARTITION_BLOCK;
    index_partition_bits_kernel<<<(int)n_tiles, RG_THREADS, 0, esr_stream(stream)>>>(
        rows, reinterpret_cast<const word_t *>(words), block_offsets, n, n_words, set_out, clear_out);
    ESR_CHECK_LAUNCH();
    return 0;
}

ESR_API int esr_regroup_stats_merge(const esr_regroup_stats_t *parts, int64_t n_parts, esr_regroup_stats_t *out, void *stream)
{
    if (n_parts < 0) return ESR_EINVAL;
    if (n_parts >= RG_MAX_N) return ESR_ECAP;
    if (!n_parts) return 0;
    if (!parts || !out || misaligned8(parts, out)) return ESR_EINVAL;
    regroup_stats_merge_kernel<<<1, ESR_WAVE, 0, esr_stream(stream)>>>(parts, n_parts, out);
    ESR_CHECK_LAUNCH();
    return 0;
}
