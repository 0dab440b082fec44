// Body of the split-fp16 forward kernels of mlp_split.hip: #included INSIDE each kernel definition (no include guard), with
// KIND, SM (SAVE_RT / SAVE_MASKS / SAVE_NONE) and the kernel argument AB in scope.  See mlp_split.hip for the scheme.
    constexpr bool SAVE_H = SM == SAVE_RT, SAVE_M = SM != SAVE_NONE;
    using S = SplitSteps<KIND>;
    constexpr NetDesc D = net_desc(KIND);
    constexpr SplitLayout L = S::L;
    constexpr PackLayout L32 = pack_layout(KIND);
    constexpr int NL = S::NL, NHID = NL - 1, HT = D.hid_tiles, KS1 = L.ks[0], NS = S::NS;
    constexpr unsigned HBYTES = HT * 32 * 32 * 4, MBYTES = (HT / 2) * 256;
    static_assert((NL == 4 || NL == 2) && HT % 2 == 0, "the four-layer nets (radiance, BRDF, emission) and the tone mapper");
    // segment of this workgroup
    SplitSeg A = AB.seg[0];
#pragma unroll
    for (int k = 1; k < MAX_SPLIT_SEG; ++k)
        if (k < AB.nseg && (int)blockIdx.x >= AB.seg[k].b0) A = AB.seg[k];
    const int blk0 = A.b0, nblk = A.nb;
    extern __shared__ __attribute__((aligned(16))) unsigned char wl[];          // buffer 0 | buffer 1 | biases
    float *bias_l = reinterpret_cast<float *>(wl + S::WBYTES);
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, s_ = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntiles = A.t1 - A.t0, ngroups = (ntiles + SPW - 1) / SPW;
    for (int i = tid; i < NL * S::BIAS_FLOATS; i += 64 * SPW) {
        const int l = i / S::BIAS_FLOATS, k = i % S::BIAS_FLOATS;
        bias_l[i] = k < L32.tiles_out[l] * 32 ? A.packed32[L32.off_bf[l] + k] : 0.f;
    }
    const rsrc_t WP = make_rsrc(A.planes, (unsigned)(L.total_chunks * 1024));
    u32x4 pre[S::PRE];
    // request / write the chunks of step `st` (compile-time) into LDS buffer `dst`
    auto stage_load = [&](auto ST) __attribute__((always_inline)) {
        // (constexpr locals: as plain call arguments the step table's lookups -- loops over the layer list -- were evaluated at
        //  RUN time for the later steps, a chain of scalar loads per use: steps 5-8 took 10 k clocks instead of 2.5 k)
        constexpr int st = decltype(ST)::value, pieces = S::chunks(st) * 64, base = S::chunk0(st) * 1024;
#pragma unroll
        for (int k = 0; k < S::PRE; ++k)
            if (k * 64 * SPW < pieces) pre[k] = __builtin_amdgcn_raw_buffer_load_b128(WP, (tid + 64 * SPW * k) * 16, base, 0);
    };
    auto stage_store = [&](auto ST, unsigned char *dst) __attribute__((always_inline)) {
        constexpr int st = decltype(ST)::value, pieces = S::chunks(st) * 64;
#pragma unroll
        for (int k = 0; k < S::PRE; ++k)
            if (k * 64 * SPW < pieces && tid + 64 * SPW * k < pieces)
                *reinterpret_cast<u32x4 *>(dst + (size_t)(tid + 64 * SPW * k) * 16) = pre[k];
    };
    // one 16-byte piece per thread: the step's last tile issues these behind its MFMAs (the other LDS buffer is idle since
    // the previous step's barrier), instead of 12 writes + their wait between the last MFMA and the barrier
    auto stage_piece = [&](auto ST, auto KC, unsigned char *dst) __attribute__((always_inline)) {
        constexpr int st = decltype(ST)::value, k = decltype(KC)::value, pieces = S::chunks(st) * 64;
        if constexpr (k * 64 * SPW < pieces)
            if (tid + 64 * SPW * k < pieces) *reinterpret_cast<u32x4 *>(dst + (size_t)(tid + 64 * SPW * k) * 16) = pre[k];
    };
    if constexpr (S::RES) {
        for (int i = tid; i < L.total_chunks * 64; i += 64 * SPW)
            *reinterpret_cast<u32x4 *>(wl + (size_t)i * 16) = __builtin_amdgcn_raw_buffer_load_b128(WP, i * 16, S::BASE_CHUNK * 1024, 0);
    } else {
        stage_load(std::integral_constant<int, 0>{});
        stage_store(std::integral_constant<int, 0>{}, wl);
    }
    step_barrier();

    // the group's input rows: lane (h, s) needs rows 16 j + 8 h + i of its sample s (first layer's k order)
    float xn[KS1 * 8];
    auto fetch = [&](int tg) {
        const int tt = A.t0 + tg * SPW + wv;
        const int t = tt < A.t1 ? tt : A.t1 - 1;
        const rsrc_t RX = make_rsrc(AB.X + (size_t)t * D.xrows * 32, D.xrows * 32 * 4);
        const int xvoff = (h * 8 * 32 + s_) * 4, coff = A.crow * 128;
#pragma unroll
        for (int j = 0; j < KS1; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = 16 * j + 8 * h + i;
                xn[j * 8 + i] = bload1(RX, xvoff + (row < D.cw ? coff : 0), (16 * j + i) * 128);
            }
    };
    // one wave per SIMD: the next group's input rows are requested a group ahead (nobody else hides the load); two waves
    // per SIMD: the rows are loaded where they are needed -- 40 registers less, which is what makes the second wave fit
    constexpr bool PREFETCH_X = split_occ(KIND) == 1;
    constexpr int WR = PREFETCH_X ? WRING : 2;                  // (weight ring: one k-step ahead is enough beside a second wave)
    if (PREFETCH_X && (int)blockIdx.x - blk0 < ngroups) fetch((int)blockIdx.x - blk0);
    const int hvoff = tile_voff(lane);

    int rmax = 0;                                           // largest |input| / hidden activation of this wave, as bits (all >= 0)
    // LDS buffer of step st = (st + par) & 1: a net with an odd number of steps per group (the 128-wide nets: 7) starts every
    // other group in buffer 1
    for (int tg = (int)blockIdx.x - blk0, trip = 0; tg < ngroups; tg += nblk, ++trip) {
        const int par = (NS & 1) ? (trip & 1) : 0;
        const int tt = A.t0 + tg * SPW + wv;
        const bool live = tt < A.t1;                       // a wave past the range runs on the last tile, stores nothing
        const int t = live ? tt : A.t1 - 1;
        const bool save = (SM == SAVE_RT ? A.save != 0 : SAVE_M) && live;
        // the lane's tile offset, opaque per group: as a loop invariant `hvoff + row offset` was hoisted out of the group loop
        // for all 16 rows (16 registers, spilled to accumulation registers, one v_accvgpr_read per store); inside the loop
        // the constant folds into the store's immediate offset
        int hv = hvoff;
        if constexpr (SAVE_H) asm volatile("" : "+v"(hv));
        // planes: first layer's input (from X) | set A | set B; layer 0 writes A, 1 reads A writes B, 2 reads B writes A, 3 reads A
        f16x8 xi1[KS1], xi2[KS1], pa1[2 * HT], pa2[2 * HT], pb1[2 * HT], pb2[2 * HT];
        if constexpr (!PREFETCH_X) fetch(tg);
        float xmax = 0.f;                                  // largest |input| of the tile: its first plane is fp16 too
#pragma unroll
        for (int j = 0; j < KS1; ++j) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = xn[j * 8 + i];
#pragma unroll
            for (int i = 0; i < 8; i += 2) xmax = fmaxf(xmax, fmaxf(fabsf(v[i]), fabsf(v[i + 1])));      // (v_max3_f32 with |.| modifiers)
            split8(v, xi1[j], xi2[j]);
        }
        rmax = max(rmax, __float_as_int(xmax));            // (non-negative floats order like their bits; dead before the planes are live)
        ESR_SPLIT_STAMP(0);
        if constexpr (PREFETCH_X) fetch(tg + nblk < ngroups ? tg + nblk : tg);       // the next group's rows (past the end: this group again, never used)
        // one accumulator per tile (two tiles alternate: the one in flight and the one in its epilogue); bz: a tile's biases,
        // requested when its MFMAs start and used a tile later (a ds_read inside a micro-slice is a full LDS round trip in
        // front of one MFMA's worth of work: the first version of the slices waited ~100 clocks in each); ev: the pending
        // tile's finished values between the phases of its epilogue (vector registers: every touch of an accumulation
        // register costs a v_accvgpr_read / _write of its own)
        f32x16 am[2];
        float4 bz4[2][4];
        float ev[16];
        unsigned mword = 0;
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // zero-record descriptors drop the stores of a pass that saves nothing (no branch inside the MFMA stream)
        const unsigned hrec = (SAVE_H && save && A.save == 1) ? HBYTES : 0u, mrec = save ? MBYTES : 0u;

        // ---- the epilogue of a finished hidden tile, cut into 24 MICRO-SLICES (8 register pairs x 3 phases) ------------------
        // One wave per SIMD has nobody to overlap with, and the wave issues in order: independent vector instructions DO run
        // in the shadow of an MFMA's 32 clocks (tools/ubench/mfma_valu_overlap.hip: a group of one MFMA + V vector
        // instructions costs max(32, 4.75 V) + 4.5 clocks), but a tile's whole epilogue behind its MFMAs idles the pipe for its
        // length (the first version of this kernel: 0.98 ms at C2, 9 k clocks per step for 2.3 k of matrix work).  Each
        // micro-slice (5-8 vector instructions) is therefore issued right behind ONE MFMA of the FOLLOWING tile -- also across
        // a layer boundary: the last tile of layer l is finished inside the first tile of layer l + 1, whose k-steps 10 / 11
        // (the only ones that read that tile's planes) come after micro-slice 23.
        //   phase 0 (pair p): value = accumulator / 64 + bias (one fma), ReLU, the fp32 tile stores -> ev
        //   phase 1: mask bits, first plane (fp16 of the value)
        //   phase 2: second plane (fp16 of value - first plane)
        auto micro = [&](auto LC, auto IT, auto MS, f32x16 &accm, auto &o1, auto &o2) __attribute__((always_inline)) {
            constexpr int l = decltype(LC)::value, it = decltype(IT)::value, ms = decltype(MS)::value, p = ms / 3, q = ms % 3;
            constexpr int r0 = 2 * p, jj = r0 >> 3, i0 = r0 & 7;
            if constexpr (q == 0) {
                const float4 b4 = bz4[it & 1][p >> 1];
                const float bx = (p & 1) ? b4.z : b4.x, by = (p & 1) ? b4.w : b4.y;
                float v0 = fmaf(accm[r0], SPLIT_W_INV, bx), v1 = fmaf(accm[r0 + 1], SPLIT_W_INV, by);
                const int b0 = __float_as_int(v0), b1 = __float_as_int(v1);
                v0 = __int_as_float(b0 > 0 ? b0 : 0);
                v1 = __int_as_float(b1 > 0 ? b1 : 0);
                // range check: inf and +NaN order above every number as integers (volatile: left to itself the chain of maxima
                // sank to the kernel's end and kept every value alive; operands are the integer max's VALU results)
                asm volatile("v_max3_i32 %0, %0, %1, %2" : "+v"(rmax) : "v"(__float_as_int(v0)), "v"(__float_as_int(v1)));
                if constexpr (SAVE_H) {
                    const rsrc_t RH = make_rsrc(AB.H[l] + (size_t)t * (HBYTES / 4), hrec);  // fp32 tile, mlp.hip's store_tiles order
                    asm volatile("" : "+v"(hv));                   // (opaque per slice: a shared `hv + row offset` is kept in a
                    bstore1_nt(RH, v0, hv + tile_soff(0, r0), it * 4096);   //  register of its own instead of the store's immediate)
                    bstore1_nt(RH, v1, hv + tile_soff(0, r0 + 1), it * 4096);
                }
                ev[r0] = v0; ev[r0 + 1] = v1;
            } else if constexpr (q == 1) {
                const float v0 = ev[r0], v1 = ev[r0 + 1];
                if constexpr (SAVE_M) {
                    int one0, one1;                                // (operands: phase 0's integer max -- VALU results, no MFMA hazard;
                    asm volatile("v_med3_i32 %1, %3, 0, 1\n\t"     //  one statement: see put_residual_pair)
                                 "v_med3_i32 %2, %4, 0, 1\n\t"
                                 "v_lshl_or_b32 %0, %1, %5, %0\n\t"
                                 "v_lshl_or_b32 %0, %2, %6, %0"
                                 : "+v"(mword), "=&v"(one0), "=&v"(one1)
                                 : "v"(__float_as_int(v0)), "v"(__float_as_int(v1)), "n"((it & 1) * 16 + r0), "n"((it & 1) * 16 + r0 + 1));
                }
                put_pair<i0>(o1[2 * it + jj], v0, v1);
            } else {
                put_residual_pair<i0>(o2[2 * it + jj], o1[2 * it + jj], ev[r0], ev[r0 + 1]);
            }
        };
        // micro-slices of the pending tile that ride on MFMA slot u of the tile in flight: slice i on slot i % NAVAIL, where
        // NAVAIL = the slots before the tile in flight first READS the pending tile's planes (all of them for a tile of
        // the same layer; all but the last two k-steps when the pending tile is the previous layer's last tile)
        auto pending = [&](auto LC, auto IT, auto U, auto NAVAILC, f32x16 &accm, auto &o1, auto &o2) __attribute__((always_inline)) {
            constexpr int u = decltype(U)::value, navail = decltype(NAVAILC)::value;
            static_assert(navail >= 3 && navail % 3 == 0, "whole register pairs per pass");
            if constexpr (u < navail)
                sfor<0, (24 + navail - 1) / navail>([&](auto KC) {
                    constexpr int msi = u + decltype(KC)::value * navail;
                    if constexpr (msi < 24) micro(LC, IT, std::integral_constant<int, msi>{}, accm, o1, o2);
                });
            // behind the LAST micro-slice of an odd tile: the mask word of the tile pair (mlp_common.h: store_relu_mask's order)
            constexpr int l = decltype(LC)::value, it = decltype(IT)::value;
            if constexpr (u == (navail < 24 ? navail : 24) - 1 && (it & 1) && SAVE_M) {
                __builtin_amdgcn_raw_buffer_store_b32(mword, make_rsrc(AB.M[l] + (size_t)t * (MBYTES / 4), mrec), lane * 4,
                                                      (it >> 1) * 256, 0);
                mword = 0;
            }
        };

        // one layer: its steps (pairs of output tiles); `in`: the layer's input planes (= the previous layer's output planes,
        // which the pending tile of that layer is still filling during tile 0), `o`: its output planes
        auto run_layer = [&](auto LC, auto &in1, auto &in2, auto &o1, auto &o2) __attribute__((always_inline)) {
            constexpr int l = decltype(LC)::value, KS = L.ks[l], NT = L.tiles_out[l], NP = L.pairs[l];
            constexpr int s0 = [] { int s = 0; for (int k = 0; k < l; ++k) s += L.pairs[k]; return s; }();
            constexpr bool LAST = l == NL - 1;
            f32x16 zm;                                             // (output layer: its single tile's sums)
            sfor<0, NP>([&](auto PC) {
                constexpr int p = decltype(PC)::value, st = s0 + p, tin = S::tiles_in(st), nxt_st = (st + 1) % NS;
                const unsigned char *wsrc = S::RES ? wl + (S::chunk0(st) - S::BASE_CHUNK) * 1024 : wl + ((st + par) & 1) * S::BUF;
                const u32x4 *mine = reinterpret_cast<const u32x4 *>(wsrc) + lane;
                if constexpr (!S::RES) stage_load(std::integral_constant<int, nxt_st>{});
                // flat k-step index n = tt_ * KS + j; chunk of (tile tt_, plane q, k-step j) = (tt_ * 2 + q) * KS + j
                constexpr int NTOT = tin * KS;
                // weight operands: a ring of three k-steps (requested two k-steps = ~190 clocks ahead)
                // weight operands: a ring of WR k-steps, requested WR - 1 k-steps ahead (the LDS serves four streaming
                // waves at ~91 B/clk: a read waits behind ~24 KB of its neighbours' requests)
                u32x4 wb[WR][2];
                sfor<0, (WR - 1 < NTOT ? WR - 1 : NTOT)>([&](auto NC) {
                    constexpr int n0 = decltype(NC)::value, t0_ = n0 / KS, j0_ = n0 % KS;
                    wb[n0][0] = mine[((t0_ * 2 + 0) * KS + j0_) * 64];
                    wb[n0][1] = mine[((t0_ * 2 + 1) * KS + j0_) * 64];
                });
                sfor<0, NTOT>([&](auto NC) {
                    constexpr int n = decltype(NC)::value, tt_ = n / KS, j = n % KS, it = 2 * p + tt_;
                    if constexpr (n + WR - 1 < NTOT) {
                        constexpr int t2 = (n + WR - 1) / KS, j2 = (n + WR - 1) % KS;
                        wb[(n + WR - 1) % WR][0] = mine[((t2 * 2 + 0) * KS + j2) * 64];
                        wb[(n + WR - 1) % WR][1] = mine[((t2 * 2 + 1) * KS + j2) * 64];
                    }
                    if constexpr (j == 0 && !LAST && PREFETCH_X) { // this tile's biases, for its epilogue a tile from now
                        const float4 *bp = reinterpret_cast<const float4 *>(bias_l + l * S::BIAS_FLOATS + it * 32 + (lane >> 5) * 16);
#pragma unroll
                        for (int q = 0; q < 4; ++q) bz4[it & 1][q] = bp[q];
                    }
                    f32x16 &m = LAST ? zm : am[it & 1];
                    const f16x8 w1 = __builtin_bit_cast(f16x8, wb[n % WR][0]), w2 = __builtin_bit_cast(f16x8, wb[n % WR][1]);
                    // the pending tile: the previous tile of this layer, or the last tile of the previous layer
                    constexpr bool HAVE = it > 0 || l > 0;
                    constexpr int pl = it > 0 ? l : l - 1, pit = it > 0 ? it - 1 : (l > 0 ? L.tiles_out[l > 0 ? l - 1 : 0] - 1 : 0);
                    if constexpr (j == 0 && HAVE && !PREFETCH_X) { // two waves per SIMD: the PENDING tile's biases, right where its
                        const float4 *bp = reinterpret_cast<const float4 *>(bias_l + pl * S::BIAS_FLOATS + pit * 32 + (lane >> 5) * 16);
#pragma unroll                                                     // epilogue starts (one live set instead of two: 16 registers)
                        for (int q = 0; q < 4; ++q) bz4[pit & 1][q] = bp[q];
                    }
                    auto ride = [&](auto U) __attribute__((always_inline)) {
                        if constexpr (HAVE) {
                            if constexpr (it > 0) pending(std::integral_constant<int, pl>{}, std::integral_constant<int, pit>{}, U,
                                                          std::integral_constant<int, 3 * KS>{}, am[pit & 1], o1, o2);
                            else pending(std::integral_constant<int, pl>{}, std::integral_constant<int, pit>{}, U,
                                         std::integral_constant<int, 3 * (KS - 2)>{}, am[pit & 1], in1, in2);
                        }
                        if constexpr (tt_ == tin - 1 && !S::RES) { // the next step's weights: one piece per slot, last slots of the step
                            constexpr int u_ = decltype(U)::value, first = 3 * KS - S::PRE;
                            static_assert(first >= 0, "a tile has a slot for every staged piece");
                            if constexpr (u_ >= first) stage_piece(std::integral_constant<int, nxt_st>{}, std::integral_constant<int, u_ - first>{},
                                                                   wl + ((st + 1 + par) & 1) * S::BUF);
                        }
                        __builtin_amdgcn_sched_barrier(0);         // one MFMA + its micro-slice per scheduling region
                    };
                    // (three dependent MFMAs in a row: behind a micro-slice the predecessor has long finished; in the
                    //  slots without one the dependent issue costs a few clocks -- tools/ubench/mfma_valu_overlap.hip)
                    m = mfma_h(w1, in2[j], j == 0 ? zero16 : m);
                    ride(std::integral_constant<int, 3 * j + 0>{});
                    m = mfma_h(w1, in1[j], m);
                    ride(std::integral_constant<int, 3 * j + 1>{});
                    m = mfma_h(w2, in1[j], m);
                    ride(std::integral_constant<int, 3 * j + 2>{});
                });
                if constexpr (LAST) {
                    const float4 bz = *reinterpret_cast<const float4 *>(bias_l + l * S::BIAS_FLOATS + (lane >> 5) * 16);
                    const float bzv[4] = {bz.x, bz.y, bz.z, bz.w};
                    const rsrc_t RZ = make_rsrc(A.zout + (size_t)t * D.zrows * 32, live ? D.zrows * 32 * 4 : 0);
                    // rows 4 h + q of the output tile live in registers q = 0..3 of lane half h (acc_row(q, h)); the rows past
                    // out_dim are written as zeros, the rows past the tile (half 1 of a 4-row tile) are dropped by the descriptor
                    const int zvoff = (4 * h * 32 + s_) * 4;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        bstore1(RZ, 4 * h + q < D.out_dim ? fmaf(zm[q], SPLIT_W_INV, bzv[q]) : 0.f, zvoff, q * 128);
                }
                ESR_SPLIT_STAMP(1 + 3 * st);
                ESR_SPLIT_STAMP(2 + 3 * st);
                if constexpr (!S::RES) step_barrier();
                ESR_SPLIT_STAMP(3 + 3 * st);
            });
        };
        run_layer(std::integral_constant<int, 0>{}, xi1, xi2, pa1, pa2);
        if constexpr (NL == 4) {
            run_layer(std::integral_constant<int, 1>{}, pa1, pa2, pb1, pb2);
            run_layer(std::integral_constant<int, 2>{}, pb1, pb2, pa1, pa2);
        }
        run_layer(std::integral_constant<int, NL - 1>{}, pa1, pa2, pb1, pb2);      // output layer (pb: unused)
    }
    // a first plane holds |x| < 65504: an input or a hidden activation at or above SPLIT_RANGE (or inf; a +NaN activation) raises
    // the caller's sticky flag -- the host re-runs the step on the f32 MFMA kernels (fine_engine.py).  The OUTPUT layer's results
    // are fp32 sums that never become planes: nothing to check.  (A NaN input is NaN in both engines' results.)
    if (AB.range && rmax >= __float_as_int(SPLIT_RANGE)) atomicOr(AB.range, 1u);
