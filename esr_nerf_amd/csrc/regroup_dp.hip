// PDRA's ray re-split under data parallelism: the flags of regroup.hip as packed 64-bit words, one bit per ray, which is a
// wave's ballot as it stands.  Every rank decides its share of the uncertain group into its words of ONE preallocated
// vector; shares are cut at word boundaries, so an integer SUM all-reduce of the vector (zero outside a rank's share) is the
// union of the decisions, and the scan and the partition read the words directly: 1/8 of the flag bytes.
//
// Packed format: bit b of word w is the flag of ray 64 w + b, bit 0 the least significant; the bits at and above n in the
// last word are 0; words are 8-byte aligned.  Every writer here stores whole words with the tail clear, every reader masks
// the tail of the last word all the same (one scalar AND).
//
// esr_emit_decide_bits   the decision and the statistics of esr_emit_decide (regroup_common.h: the same per-ray statement,
//                        the same key-space reductions and atomics); a wave walks whole words, lane 0 stores the ballot
// esr_flags_pack / esr_flags_unpack   byte flags <-> words (a non-zero byte is a set bit; unpack writes 0 or 1)
// esr_flag_scan_bits     counts per tile of ESR_PARTITION_BLOCK flags = 16 words: one word per lane, popcount, a shuffle sum
//                        over the 16 lanes of a tile (a block covers 16 tiles); then the one-block scan of regroup_common.h
// esr_index_partition_bits   one block per tile.  The tile's 16 words are wave-uniform: they arrive by scalar loads and
//                        every wave takes the popcounts of the words in front of its own with scalar instructions -- no
//                        LDS, no barrier.  A lane's flag is its bit, its rank popcount(word & lanes below).
// esr_regroup_stats_merge    one wave: the records of the ranks into one, counts added, minima and maxima in the key space
// Traffic of scan + partition: 1/8 B per flag twice, 8 B read and 8 B written per row.
#include "regroup_common.h"

namespace {

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
