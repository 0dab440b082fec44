// The f32 engine's RADIANCE FORWARD on the 16-bit matrix cores, with fp32 results (round 4).
//
// On gfx950 v_mfma_f32_32x32x2_f32 runs at 1/16 of the 16-bit MFMA rate (157 vs 2500 TFLOP/s) and ON the vector lanes; the
// radiance forward -- 142.5 GFLOP per C2 step -- was the step's dominant launch at 1.06 ms (0.85 of the f32 matrix peak).
// Here every operand is split into TWO fp16 planes, x = x1 + x2 with x1 = fp16(x), x2 = fp16(x - x1) (the subtraction is
// exact in fp32), and a product is formed as
//     w . x  =  w1 . x1  +  w1 . x2  +  w2 . x1                   (+ w2 . x2, dropped: 2^-22 relative, below fp32's own rounding)
// on v_mfma_f32_32x32x16_f16 with fp32 accumulation, all three into ONE accumulator: three 16-bit MFMAs per k-step instead
// of eight f32 ones of a quarter of the depth -- 16/3 of the f32 matrix rate.  Two fp16 planes carry 22 mantissa bits as
// long as the residual x2 is a NORMAL fp16 number (|x| >= 0.125); below that it is rounded to 2^-25 ABSOLUTE (3e-8).  The
// weights (~0.07 in a 192-wide layer) are therefore stored times 64 (mlp_common.h: SPLIT_W_SCALE; the epilogue's bias
// multiply-add takes the 1/64), activations and inputs are O(1) and stay unscaled: their worst case is the 3e-8 absolute,
// i.e. the two-plane error of a value of 0.125.  Through the four layers of the net the result differs from a
// double-precision evaluation by 4e-7 .. 8e-7 of the layer's largest value, the same as torch's own fp32 chain (5e-7;
// tools/ubench/mfma_f32_shapes.hip for the rates, tests/test_gpu_split.py for the accuracy).  With bf16 planes the same
// three products give 6e-6 .. 9e-6: fp16's three extra mantissa bits per plane are what makes two planes enough; a |value|
// above 65504 (a weight above 1023) would overflow the first plane (the fp32 MFMA path stays available: ESR_SPLIT_FWD=0).
// (Until the middle of round 4 the residual planes were scaled by 2048 and summed in accumulators of their own: three
// accumulator sets whose every value had to be fetched from the accumulation registers and recombined in the epilogue --
// the epilogue, not the matrix pipe, bounded the kernel: tools/ubench/split_stamps.hip.)
//
// Everything OUTSIDE the products is the f32 engine's: fp32 input tile X, fp32 bias add, ReLU, the saved hidden tiles H
// (fp32, tile-major) and ReLU masks in mlp.hip's formats -- the f32 input-gradient and weight-gradient kernels consume them
// unchanged -- and the fp32 output rows.
//
// Structure: mlp_bf16.hip's shared-weights scheme, re-cut for the register budget.  A layer's input AND output live in
// registers as two fp16 planes each (2 x 48 + 2 x 48), beside two accumulator pairs (main / residual sums of the tile in
// flight and of the tile in its epilogue), the staged weights and the next group's inputs: ~400 registers, i.e. ONE wave
// per SIMD, four waves (= four 32-sample tiles) per workgroup and CU.  The weights (two planes: 148 KB per hidden layer)
// are staged through LDS in STEPS of one pair of output tiles (48 KB, double-buffered): a step's chunks are contiguous in
// the packed buffer, all 256 threads request the next step's 48 KB at the top of a step and write it to the other buffer at
// its end, one barrier per step.  Inside a step the tile order of mlp_bf16.hip's lds_layer16_tiled: a tile's epilogue
// (scale + bias, ReLU, fp32 stores, mask bits, the split into the next layer's planes) is issued behind the NEXT tile's
// MFMAs.
#include "mlp_common.h"

#include <type_traits>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// in-kernel time stamps for tools/ubench/split_stamps.hip (nothing in the product build)
#ifndef ESR_SPLIT_STAMP
#define ESR_SPLIT_STAMP(i)
#endif

namespace {

constexpr int SPW = 4;                                      // waves per workgroup = tiles per group
constexpr float SPLIT_RANGE = 60000.f;                      // hidden activations at or above this raise the range flag (fp16 ends at 65504)
constexpr int WRING = 3;                                    // k-steps of weight operands in flight per wave (4 / 5 / 6: no faster,
                                                            //  docs/history.md section 10)

__device__ __forceinline__ f32x16 mfma_h(f16x8 a, f16x8 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

template <int I, int N, typename F>
__device__ __forceinline__ void sfor(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sfor<I + 1, N>(f);
    }
}

// x -> (fp16(x), fp16(x - fp16(x))) for eight values
__device__ __forceinline__ void split8(const float (&v)[8], f16x8 &p1, f16x8 &p2)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const _Float16 h = (_Float16)v[i];
        p1[i] = h;
        p2[i] = (_Float16)(v[i] - (float)h);
    }
}

// Two fp16 values into slots i0, i0 + 1 of a plane register, PINNED where they are computed: the planes of a layer are first
// read by the next layer's MFMAs, and LLVM sinks a computation towards its first use -- without the pin the conversions of
// all six tiles of a layer left their micro-slices and ran as one block of ~300 instructions behind the layer's last MFMA
// (tools/ubench/split_stamps.hip; the empty asm's operand is a VALU result: no MFMA hazard involved).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
template <int I0>
__device__ __forceinline__ void put_pair(f16x8 &dst, float a, float b)
{
    const f16x2 hh = {(_Float16)a, (_Float16)b};
    unsigned u = __builtin_bit_cast(unsigned, hh);
    asm volatile("" : "+v"(u));
    const f16x2 pinned = __builtin_bit_cast(f16x2, u);
    dst[I0] = pinned[0];
    dst[I0 + 1] = pinned[1];
}

// second plane of a value pair: fp16(v - x1) with x1 read from the packed first-plane dword -- v_fma_mix_f32 takes the fp16
// half directly (one instruction per value instead of a conversion and a subtraction; the difference is exact either way).
// Operands are VALU results (phase 1's conversion, phase 0's values): nothing here reads an MFMA result.
template <int I0>
__device__ __forceinline__ void put_residual_pair(f16x8 &dst, const f16x8 &first, float v0, float v1)
{
    const unsigned u = __builtin_bit_cast(u32x4, first)[I0 >> 1];
    unsigned r;
    float d0, d1;
    // ONE asm statement: between two statements the compiler puts an `s_nop 0` when the second reads the first's result
    // (VALU -> VALU needs none on this hardware); volatile = the pin of put_pair
    asm volatile("v_fma_mix_f32 %1, %3, -1.0, %4 op_sel_hi:[1,0,0]\n\t"
                 "v_fma_mix_f32 %2, %3, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
                 "v_cvt_pk_f16_f32 %0, %1, %2"
                 : "=v"(r), "=&v"(d0), "=&v"(d1) : "v"(u), "v"(v0), "v"(v1));
    const f16x2 pinned = __builtin_bit_cast(f16x2, r);
    dst[I0] = pinned[0];
    dst[I0 + 1] = pinned[1];
}

template <int KIND, bool BWD = false> struct SplitSteps {
    static constexpr SplitLayout L = BWD ? split_layout_t(KIND) : split_layout(KIND);
    static constexpr int BASE_CHUNK = BWD ? split_layout(KIND).total_chunks : 0;      // the transposed planes follow the forward ones
    static constexpr int NL = L.n_layers;
    static constexpr int n_steps()
    {
        int n = 0;
        for (int l = 0; l < NL; ++l) n += L.pairs[l];
        return n;
    }
    static constexpr int NS = n_steps();
    static constexpr int layer_of(int s)
    {
        int l = 0;
        while (s >= L.pairs[l]) { s -= L.pairs[l]; ++l; }
        return l;
    }
    static constexpr int pair_of(int s)
    {
        int l = 0;
        while (s >= L.pairs[l]) { s -= L.pairs[l]; ++l; }
        return s;
    }
    static constexpr int tiles_in(int s)                   // output tiles of the step (2, or 1 for an odd tail / the output layer)
    {
        const int l = layer_of(s), p = pair_of(s);
        return L.tiles_out[l] - 2 * p >= 2 ? 2 : 1;
    }
    static constexpr int chunks(int s) { return tiles_in(s) * 2 * L.ks[layer_of(s)]; }
    static constexpr int chunk0(int s) { return BASE_CHUNK + L.off_chunk[layer_of(s)] + pair_of(s) * 2 * 2 * L.ks[layer_of(s)]; }
    static constexpr int max_chunks()
    {
        int m = 0;
        for (int s = 0; s < NS; ++s) m = chunks(s) > m ? chunks(s) : m;
        return m;
    }
    static constexpr int BUF = max_chunks() * 1024;
    static constexpr int BIAS_FLOATS = 32 * MAX_HID_TILES;
    // a net whose planes fit 64 KB (the tone mapper: 60 chunks each way) keeps them RESIDENT in LDS for the kernel's whole
    // life: no per-step staging, no step barriers -- a two-layer net's steps are a handful of MFMAs each, far shorter than
    // the global -> register -> LDS round trip that used to sit between them
    static constexpr bool RES = L.total_chunks <= 64;
    static constexpr int WBYTES = RES ? L.total_chunks * 1024 : 2 * BUF;
    static constexpr int LDS_BYTES = WBYTES + NL * BIAS_FLOATS * 4;
    static constexpr int PRE = (max_chunks() * 64 + 64 * SPW - 1) / (64 * SPW);     // 16-byte pieces per thread and step
};

struct SplitSeg {
    const float *packed32;     // esr_mlp_pack buffer (biases)
    const _Float16 *planes;    // esr_mlp_pack_batch's split planes
    int t0, t1, save, crow;
    float *zout;
    int b0, nb;                // workgroups [b0, b0 + nb) of the launch
};
constexpr int MAX_SPLIT_SEG = 3;
struct SplitBatch {
    const float *X;
    float *H[3];
    unsigned *M[3];
    unsigned *range;           // optional: set to 1 when a hidden activation leaves fp16's range (esr_mlp_split_range_flag)
    int nseg;
    SplitSeg seg[MAX_SPLIT_SEG];
};

__device__ __forceinline__ void step_barrier()
{
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0): this wave's LDS reads / writes of the step are done
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// workgroups per CU the register budget is cut for: the 192-wide radiance net needs a whole SIMD's registers per wave; the
// 128-wide nets and the two-layer tone mapper fit two waves per SIMD (and 2 x 66 KB of LDS), which lets one wave's MFMAs run
// under the other's epilogue
constexpr int split_occ(int kind) { return kind == ESR_MLP_RADIANCE ? 1 : 2; }

// What a forward workgroup saves, as a COMPILE-TIME mode.  SAVE_RT: the segment's `save` decides at run time, through zero-record
// descriptors (a pass that saves nothing still issues every store, and the hardware drops it) -- the merged radiance launch, whose
// segments differ.  SAVE_MASKS / SAVE_NONE: the whole launch saves the ReLU masks only / nothing, and the instructions that would
// feed the dropped stores are not in the kernel: no H store, no descriptor and no offset pin for it; SAVE_NONE: no mask bits and no
// mask-word store either.  The two-waves-per-SIMD kernels are bound by instruction count (the tone mapper's forward: 1419 ->
// 1313 instructions without its 96 H stores per tile).  Every arithmetic instruction is the same in the same order: results are bit-identical.
constexpr int SAVE_RT = -1, SAVE_NONE = 0, SAVE_MASKS = 2;

// The body is text shared by the two kernels below (mlp_split_fwd_body.h).  As a __device__ function called from both, the same
// text compiled to other code: the radiance instantiation grew from 5217 to 5249 instructions and the 128-wide input-gradient
// kernels spilled to scratch at their 256 registers.
template <int KIND>
__global__ void __launch_bounds__(64 * SPW, split_occ(KIND)) mlp_fwd_split_kernel(SplitBatch AB)
{
    constexpr int SM = SAVE_RT;
#include "mlp_split_fwd_body.h"
}
// a launch whose every workgroup saves the masks only (SM = SAVE_MASKS) or nothing (SAVE_NONE)
template <int KIND, int SM>
__global__ void __launch_bounds__(64 * SPW, split_occ(KIND)) split_fwd_lean_kernel(SplitBatch AB)
{
#include "mlp_split_fwd_body.h"
}

// ---- the input-gradient chain on the same scheme ---------------------------------------------------------------------
// dZ[2] = mask ⊙ (W3ᵀ dz), dZ[1] = mask ⊙ (W2ᵀ dZ[2]), dZ[0] = mask ⊙ (W1ᵀ dZ[1]), dX = W0ᵀ dZ[0] (rows 0 .. 43: the rows that
// lead back to a grid) -- mlp.hip's mlp_dgrad_kernel<0> with the products on the 16-bit matrix cores.  Gradients are small
// (1e-3 .. 1e-9) where fp16's normal range ends at 6e-5, so a tile's chain runs SCALED: s = 2^k (the multiplications by s
// and 1 / s are exact, the ReLU masks do not care, and the chain is linear).  A layer can grow a value by at most the largest
// column sum of its |W|; the running product of those sums, G, comes with the planes (split_gain_kernel), and s puts
// G max |dz| of the tile into [2^14, 2^15): no plane of the chain can reach fp16's ceiling of 65504.  What counts for
// the consumers (weight gradients and grid scatters sum over samples) is the error relative to the tile's LARGEST
// gradients: 2^-22 of them, as in the forward; a sample whose gradient is 2^-20 of its tile's largest loses relative
// precision, as it does in any sum with the large ones.
struct DSplitSeg {
    const _Float16 *planes;    // the net's split planes (forward | transposed)
    int t0, t1;
    int b0, nb;
};
struct DSplitBatch {
    const float *dz;
    const unsigned *M[3];
    float *dZ[3];
    float *dX;
    float *amax;               // optional: max |dz| over the launch's tiles (atomic max of the tiles' own maxima)
    int nseg;
    DSplitSeg seg[2];
};

// Compile-time modes of the input-gradient body.  DG_RT: a NULL dZ[d] is switched off through a zero-record descriptor (per layer;
// the stores and the multiplies that feed them are issued anyway).  DG_NODZ: no hidden gradient is stored by the whole launch (the
// tone mapper: its weight gradients recompute the hidden layer) -- no dZ store, no unscaling multiply for it, and no dX store of a
// row past the descriptor's end (rows >= 36 of the tone mapper's 64).  Arithmetic and its order are those of DG_RT: bit-identical.
// DG_TONE_IN (the tone mapper): DG_NODZ, and the tile ends with the tone mapper's input stage instead of the dXt stores -- the
// 33 live rows of dXt are contracted per sample with the forward's sin / cos rows of Xt to the three pre-activation gradients, which
// are multiplied by softplus'(z) and written as the 4-row dz tile (csrc/shade.hip: tone_in_bwd_kernel, whose separate launch and
// whose 4.6 KB of dXt per tile, written and read back, this replaces).
constexpr int DG_RT = 0, DG_NODZ = 1, DG_TONE_IN = 2;

// what DG_TONE_IN reads besides the input gradients' own arguments (esr_fine_tone_in_bwd's, without dXt and lin)
struct ToneInArgs {
    const float *Xt, *g_lin, *z_off, *z_emo, *rec_w;
    const int32_t *rec_ray;
    float *dz;
    int tiles_on;
};
// Rows of the tone mapper's input: 0..2 lin[c]; 3 + 5c + i: sin(2^i lin[c]); 18 + 5c + i: cos(2^i lin[c]).  d lin[c] takes
// dXt[c], +2^i dXt[sin row] Xt[cos row] and -2^i dXt[cos row] Xt[sin row].
constexpr int TIN_ROWS = 33, TIN_XT_ROWS = 48;
constexpr int TIN_SLOTS = 17;                                // accumulator registers whose row is live in lane half 0: tile 0's 16, tile 1's first
constexpr int tin_slot_row(int k) { return 32 * (k >> 4) + acc_row(k & 15, 0); }
constexpr int tin_chan(int row) { return row < 3 ? row : (row < 18 ? row - 3 : row - 18) / 5; }
constexpr int tin_partner(int row) { return row < 3 || row >= TIN_ROWS ? -1 : row < 18 ? row + 15 : row - 15; }
constexpr float tin_coef(int row)
{
    return row >= TIN_ROWS ? 0.f : row < 3 ? 1.f : row < 18 ? (float)(1 << ((row - 3) % 5)) : -(float)(1 << ((row - 18) % 5));
}
constexpr bool tin_pair_used(int pair)                       // is there a slot whose channels (half 0's, half 1's) are pair / 3, pair % 3
{
    for (int k = 0; k < TIN_SLOTS; ++k) {
        const int row0 = tin_slot_row(k), row1 = row0 + 4;
        if (tin_chan(row0) * 3 + (row1 < TIN_ROWS ? tin_chan(row1) : 0) == pair) return true;
    }
    return false;
}

template <int KIND>
__global__ void __launch_bounds__(64 * SPW, split_occ(KIND)) mlp_dgrad_split_kernel(DSplitBatch AB)
{
    constexpr int MODE = DG_RT;
    const ToneInArgs TI = {};
#include "mlp_split_dgrad_body.h"
}
// a launch that stores no hidden gradient (DG_NODZ), and that of the tone mapper with its input stage folded in (DG_TONE_IN)
template <int KIND, int MODE>
__global__ void __launch_bounds__(64 * SPW, split_occ(KIND)) split_dgrad_lean_kernel(DSplitBatch AB, ToneInArgs TI)
{
    static_assert(MODE != DG_TONE_IN || KIND == ESR_MLP_TONEMAP, "the tone mapper's input stage");
#include "mlp_split_dgrad_body.h"
}

// workgroups per segment proportional to its tile groups (every non-empty segment >= 1); returns the grid
int share_blocks_split(SplitSeg *seg, int nseg, int cap = 256)
{
    int groups[MAX_SPLIT_SEG], total = 0;
    for (int k = 0; k < nseg; ++k) { groups[k] = (seg[k].t1 - seg[k].t0 + SPW - 1) / SPW; total += groups[k]; }
    const int grid = total < cap ? total : cap;
    int given = 0;
    for (int k = 0; k < nseg; ++k) {
        int n = (int)((int64_t)grid * groups[k] / (total > 0 ? total : 1));
        if (n < 1) n = 1;
        if (n > groups[k]) n = groups[k];
        seg[k].nb = n;
        given += n;
    }
    for (int guard = 0; given != grid && guard < 1024; ++guard) {
        int pick = -1;
        double best = 0.0;
        for (int k = 0; k < nseg; ++k) {
            if (given < grid) {
                if (seg[k].nb >= groups[k]) continue;
                const double load = (double)groups[k] / seg[k].nb;
                if (pick < 0 || load > best) { pick = k; best = load; }
            } else {
                if (seg[k].nb <= 1) continue;
                const double load = (double)groups[k] / (seg[k].nb - 1);
                if (pick < 0 || load < best) { pick = k; best = load; }
            }
        }
        if (pick < 0) break;
        seg[pick].nb += given < grid ? 1 : -1;
        given += given < grid ? 1 : -1;
    }
    int b0 = 0;
    for (int k = 0; k < nseg; ++k) { seg[k].b0 = b0; b0 += seg[k].nb; }
    return b0;
}

// per-device sticky flag registered by the caller (esr_mlp_split_range_flag); NULL: no check
std::atomic<unsigned *> g_range_flag[16];

template <int KIND, void (*KERNEL)(SplitBatch)>
int launch_split_as(const SplitBatch &B, int grid, hipStream_t s)
{
    static std::atomic<uint64_t> optin{0};
    if (int rc = esr_lds_optin(reinterpret_cast<const void *>(KERNEL), SplitSteps<KIND>::LDS_BYTES, optin)) return rc;
    KERNEL<<<grid, 64 * SPW, SplitSteps<KIND>::LDS_BYTES, s>>>(B);
    ESR_CHECK_LAUNCH();
    return 0;
}

template <int KIND>
int launch_split_k(SplitBatch &B, hipStream_t s)
{
    int dev = 0;
    B.range = (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16) ? g_range_flag[dev].load() : nullptr;
    const int grid = share_blocks_split(B.seg, B.nseg, 256 * split_occ(KIND));       // resident workgroups: one or two per CU
    // the instantiation without the stores nobody reads, where the whole launch saves the masks only (the tone mapper's training
    // forward) or nothing (evaluation, detached passes); the radiance net keeps the one run-time body (power-bound, one wave per
    // SIMD: DESIGN.md section 4)
    const int save = B.nseg == 1 ? B.seg[0].save : 1;
    if constexpr (KIND == ESR_MLP_TONEMAP)
        if (save == 2) return launch_split_as<KIND, split_fwd_lean_kernel<KIND, SAVE_MASKS>>(B, grid, s);
    if constexpr (KIND != ESR_MLP_RADIANCE)
        if (save == 0) return launch_split_as<KIND, split_fwd_lean_kernel<KIND, SAVE_NONE>>(B, grid, s);
    return launch_split_as<KIND, mlp_fwd_split_kernel<KIND>>(B, grid, s);
}
int launch_split(int kind, SplitBatch &B, hipStream_t s)
{
    switch (kind) {
    case ESR_MLP_RADIANCE: return launch_split_k<ESR_MLP_RADIANCE>(B, s);
    case ESR_MLP_TONEMAP:  return launch_split_k<ESR_MLP_TONEMAP>(B, s);
    case ESR_MLP_BRDF:     return launch_split_k<ESR_MLP_BRDF>(B, s);
    case ESR_MLP_EMIT:     return launch_split_k<ESR_MLP_EMIT>(B, s);
    default:               return ESR_EINVAL;
    }
}
bool split_kind_ok(int kind)
{
    return kind == ESR_MLP_RADIANCE || kind == ESR_MLP_TONEMAP || kind == ESR_MLP_BRDF || kind == ESR_MLP_EMIT;
}

bool crow_ok_split(int kind, int crow) { return crow == 0 || (kind != ESR_MLP_TONEMAP && (crow == 88 || crow == 96)); }

}  // namespace

// One radiance forward pass over tiles [t0, t1) (esr_mlp_fwd's contract: save 0 / 1 / 2, colour group color_row0), products
// on the 16-bit matrix cores from split fp16 planes.  packed32: esr_mlp_pack's buffer (biases); planes: the net's split
// planes (esr_mlp_pack_batch, esr_mlp_packed_split_elems values).  Radiance, tone mapper, BRDF and emission nets.
ESR_API int esr_mlp_fwd_split(int kind, const float *packed32, const void *planes, const float *X, int32_t t0, int32_t t1,
                              float *const *H, uint32_t *const *M, int save, int color_row0, float *zout, void *stream)
{
    if (!split_kind_ok(kind) || t0 < 0 || t1 < t0 || !crow_ok_split(kind, color_row0)) return ESR_EINVAL;
    if (t1 == t0) return 0;
    if (!packed32 || !planes || !X || !zout) return ESR_EINVAL;
    SplitBatch B = {};
    B.X = X;
    if (save) {
        if (!M || (save != 2 && !H)) return ESR_EINVAL;
        for (int l = 0; l < net_desc(kind).n_layers - 1; ++l) {
            if (!M[l] || (save != 2 && !H[l])) return ESR_EINVAL;
            B.H[l] = save != 2 ? H[l] : nullptr; B.M[l] = M[l];
        }
    }
    B.nseg = 1;
    B.seg[0] = SplitSeg{packed32, static_cast<const _Float16 *>(planes), t0, t1, save == 2 ? 2 : save ? 1 : 0, color_row0, zout, 0, 0};
    return launch_split(kind, B, esr_stream(stream));
}

unsigned *esr_split_range_flag_ptr()
{
    int dev = 0;
    return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16) ? g_range_flag[dev].load() : nullptr;
}

// Registers (NULL: removes) the CURRENT device's range flag: a device uint32 that every later split forward launch on this
// device ORs with 1 when a hidden activation reaches 60000 (or is inf / NaN): the products' first plane is fp16.
ESR_API int esr_mlp_split_range_flag(uint32_t *flag)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return ESR_EINVAL;
    g_range_flag[dev].store(flag);
    return 0;
}

// The fine stage's three radiance forward passes of a step as ONE launch (esr_mlp_fwd_fine's contract and argument meaning).
ESR_API int esr_mlp_fwd_fine_split(const float *packed32_off, const void *planes_off, const float *packed32_emo,
                                   const void *planes_emo, const float *X, int32_t t_on, int32_t t_all, float *const *H,
                                   uint32_t *const *M, int color_row_detached, float *z_off, float *z_emo, void *stream)
{
    if (t_on < 0 || t_all < t_on || !crow_ok_split(ESR_MLP_RADIANCE, color_row_detached)) return ESR_EINVAL;
    if (t_all == 0) return 0;
    if (!packed32_off || !planes_off || !packed32_emo || !planes_emo || !X || !H || !M || !z_off || !z_emo) return ESR_EINVAL;
    SplitBatch B = {};
    B.X = X;
    for (int l = 0; l < 3; ++l) {
        if (!H[l] || !M[l]) return ESR_EINVAL;
        B.H[l] = H[l]; B.M[l] = M[l];
    }
    const _Float16 *po = static_cast<const _Float16 *>(planes_off), *pe = static_cast<const _Float16 *>(planes_emo);
    int n = 0;
    if (t_on > 0) B.seg[n++] = SplitSeg{packed32_off, po, 0, t_on, 0, color_row_detached, z_off, 0, 0};
    if (t_all > t_on) B.seg[n++] = SplitSeg{packed32_off, po, t_on, t_all, 1, 0, z_off, 0, 0};
    if (t_on > 0) B.seg[n++] = SplitSeg{packed32_emo, pe, 0, t_on, 1, 0, z_emo, 0, 0};
    B.nseg = n;
    return launch_split(ESR_MLP_RADIANCE, B, esr_stream(stream));
}

namespace {
template <int KIND, auto KERNEL, typename... EXTRA>
int launch_dsplit_as(const DSplitBatch &B, int grid, hipStream_t s, EXTRA... extra)
{
    static std::atomic<uint64_t> optin{0};
    if (int rc = esr_lds_optin(reinterpret_cast<const void *>(KERNEL), SplitSteps<KIND, true>::WBYTES, optin)) return rc;
    KERNEL<<<grid, 64 * SPW, SplitSteps<KIND, true>::WBYTES, s>>>(B, extra...);
    ESR_CHECK_LAUNCH();
    return 0;
}

template <int KIND>
int launch_dsplit_k(DSplitBatch &B, hipStream_t s, const ToneInArgs *tone_in = nullptr)
{
    int groups[2], total = 0;
    for (int k = 0; k < B.nseg; ++k) { groups[k] = (B.seg[k].t1 - B.seg[k].t0 + SPW - 1) / SPW; total += groups[k]; }
    const int cap = 256 * split_occ(KIND);
    const int grid = total < cap ? total : cap;
    if (B.nseg == 1) { B.seg[0].b0 = 0; B.seg[0].nb = grid; }
    else {
        int n0 = (int)((int64_t)grid * groups[0] / total);
        if (n0 < 1) n0 = 1;
        if (n0 > groups[0]) n0 = groups[0];
        if (grid - n0 > groups[1]) n0 = grid - groups[1];
        if (grid - n0 < 1) n0 = grid - 1;
        B.seg[0].b0 = 0; B.seg[0].nb = n0; B.seg[1].b0 = n0; B.seg[1].nb = grid - n0;
    }
    // no hidden gradient asked for by the whole launch (the tone mapper's callers): the instantiation without the dZ stores;
    // a mixed call keeps the run-time body
    if constexpr (KIND == ESR_MLP_TONEMAP) {
        if (tone_in) return launch_dsplit_as<KIND, split_dgrad_lean_kernel<KIND, DG_TONE_IN>>(B, grid, s, *tone_in);
        bool none = true;
        for (int l = 0; l < net_desc(KIND).n_layers - 1; ++l) none = none && !B.dZ[l];
        if (none) return launch_dsplit_as<KIND, split_dgrad_lean_kernel<KIND, DG_NODZ>>(B, grid, s, ToneInArgs{});
    }
    return launch_dsplit_as<KIND, mlp_dgrad_split_kernel<KIND>>(B, grid, s);
}
int launch_dsplit(int kind, DSplitBatch &B, hipStream_t s)
{
    switch (kind) {
    case ESR_MLP_RADIANCE: return launch_dsplit_k<ESR_MLP_RADIANCE>(B, s);
    case ESR_MLP_TONEMAP:  return launch_dsplit_k<ESR_MLP_TONEMAP>(B, s);
    case ESR_MLP_BRDF:     return launch_dsplit_k<ESR_MLP_BRDF>(B, s);
    case ESR_MLP_EMIT:     return launch_dsplit_k<ESR_MLP_EMIT>(B, s);
    default:               return ESR_EINVAL;
    }
}
}  // namespace

// esr_mlp_dgrad's contract (radiance, tone mapper, BRDF and emission nets): input / hidden gradients over tiles [t0, t1) from the net's split planes.
ESR_API int esr_mlp_dgrad_split(int kind, const void *planes, const float *dz, int32_t t0, int32_t t1, const uint32_t *const *M,
                                float *const *dZ, float *dX, float *amax, void *stream)
{
    if (!split_kind_ok(kind) || t0 < 0 || t1 < t0) return ESR_EINVAL;
    if (t1 == t0) return 0;
    if (!planes || !dz || !M || !dZ || !dX) return ESR_EINVAL;
    DSplitBatch B = {};
    B.dz = dz; B.dX = dX; B.amax = amax;
    for (int l = 0; l < net_desc(kind).n_layers - 1; ++l) {
        if (!M[l]) return ESR_EINVAL;
        B.M[l] = M[l]; B.dZ[l] = dZ[l];                     // a NULL dZ[l] is computed but not stored
    }
    B.nseg = 1;
    B.seg[0] = DSplitSeg{static_cast<const _Float16 *>(planes), t0, t1, 0, 0};
    return launch_dsplit(kind, B, esr_stream(stream));
}

// esr_mlp_dgrad_fine's contract: the emissive net on tiles [0, t_on), the non-emissive net on [t_on, t_all), one launch.
ESR_API int esr_mlp_dgrad_fine_split(const void *planes_emo, const void *planes_off, const float *dz, int32_t t_on, int32_t t_all,
                                     const uint32_t *const *M, float *const *dZ, float *dX, float *amax, void *stream)
{
    if (t_on < 0 || t_all < t_on) return ESR_EINVAL;
    if (t_all == 0) return 0;
    if (!planes_emo || !planes_off || !dz || !M || !dZ || !dX) return ESR_EINVAL;
    DSplitBatch B = {};
    B.dz = dz; B.dX = dX; B.amax = amax;
    for (int l = 0; l < 3; ++l) {
        if (!M[l]) return ESR_EINVAL;
        B.M[l] = M[l]; B.dZ[l] = dZ[l];
    }
    int n = 0;
    if (t_on > 0) B.seg[n++] = DSplitSeg{static_cast<const _Float16 *>(planes_emo), 0, t_on, 0, 0};
    if (t_all > t_on) B.seg[n++] = DSplitSeg{static_cast<const _Float16 *>(planes_off), t_on, t_all, 0, 0};
    B.nseg = n;
    return launch_dsplit(ESR_MLP_RADIANCE, B, esr_stream(stream));
}

// The tone mapper's input gradients with esr_fine_tone_in_bwd folded in: from dzt over tiles [0, tiles_all) straight to the radiance
// nets' output gradients dz (the emissive net's on tiles [0, tiles_on), the other net's behind), with no dXt in memory.  The hidden
// gradient is not stored (the tone mapper's weight gradients recompute it); amax as esr_mlp_dgrad_split.
ESR_API int esr_fine_tone_dgrad_split(const void *planes, const float *dzt, const uint32_t *Mt, const float *Xt, const float *g_lin,
                                      const float *z_off, const float *z_emo, const int32_t *rec_ray, const float *rec_w,
                                      int32_t tiles_on, int32_t tiles_all, float *dz, float *amax, void *stream)
{
    if (tiles_on < 0 || tiles_all < tiles_on) return ESR_EINVAL;
    if (tiles_all == 0) return 0;
    if (!planes || !dzt || !Mt || !Xt || !g_lin || !z_off || !z_emo || !rec_ray || !rec_w || !dz) return ESR_EINVAL;
    DSplitBatch B = {};
    B.dz = dzt; B.amax = amax; B.M[0] = Mt;
    B.nseg = 1;
    B.seg[0] = DSplitSeg{static_cast<const _Float16 *>(planes), 0, tiles_all, 0, 0};
    const ToneInArgs TI = {Xt, g_lin, z_off, z_emo, rec_w, rec_ray, dz, tiles_on};
    return launch_dsplit_k<ESR_MLP_TONEMAP>(B, esr_stream(stream), &TI);
}
