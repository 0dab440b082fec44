// Body of the split-fp16 input-gradient kernels of mlp_split.hip: #included INSIDE each kernel definition (no include guard), with
// KIND, MODE (DG_RT / DG_NODZ / DG_TONE_IN), the kernel argument AB and TI (ToneInArgs; read by DG_TONE_IN only) in scope.  See mlp_split.hip for the scheme.
    constexpr bool STORE_DZ = MODE == DG_RT;
    constexpr int DX_STORED = (dx_rows(KIND) + 3) / 4 * 4;       // rows of dX the descriptor lets through
    using S = SplitSteps<KIND, true>;
    constexpr NetDesc D = net_desc(KIND);
    constexpr SplitLayout L = S::L;
    constexpr int NL = S::NL, NHID = NL - 1, HT = D.hid_tiles, NS = S::NS;
    constexpr unsigned HBYTES = HT * 32 * 32 * 4, MBYTES = (HT / 2) * 256;
    static_assert((NL == 4 || NL == 2) && HT % 2 == 0 && L.ks[0] == 1 && L.tiles_out[NL - 1] == 2 && D.out_dim <= 8 && D.zrows <= 8,
                  "the four-layer nets and the tone mapper: outputs in one k-step, grid-fed input rows in two tiles");
    DSplitSeg A = AB.seg[0];
    if (AB.nseg > 1 && (int)blockIdx.x >= AB.seg[1].b0) A = AB.seg[1];
    const int blk0 = A.b0, nblk = A.nb;
    extern __shared__ __attribute__((aligned(16))) unsigned char wl[];          // buffer 0 | buffer 1
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, s_ = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntiles = A.t1 - A.t0, ngroups = (ntiles + SPW - 1) / SPW;
    const rsrc_t WP = make_rsrc(A.planes, (unsigned)((S::BASE_CHUNK + L.total_chunks) * 1024));
    u32x4 pre[S::PRE];
    auto stage_load = [&](auto ST) __attribute__((always_inline)) {
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

    // the group's output gradients (rows 0..3 of the 4-row tile: half 0's slots 0..3, everything else of the k-step is zero)
    // and ReLU masks
    float zn[D.zrows];
    unsigned mn[NHID][HT / 2];
    auto fetch = [&](int tg) {
        const int tt = A.t0 + tg * SPW + wv;
        const int t = tt < A.t1 ? tt : A.t1 - 1;
        const rsrc_t RZ = make_rsrc(AB.dz + (size_t)t * D.zrows * 32, D.zrows * 32 * 4);
#pragma unroll
        for (int i = 0; i < D.zrows; ++i) zn[i] = bload1(RZ, s_ * 4, i * 128);
#pragma unroll
        for (int l = 0; l < NHID; ++l)
            load_relu_mask<HT>(make_rsrc(AB.M[l] + (size_t)t * (MBYTES / 4), MBYTES), mn[l], lane);
    };
    if ((int)blockIdx.x - blk0 < ngroups) fetch((int)blockIdx.x - blk0);
    const int hvoff = tile_voff(lane);

    float wmax = 0.f;                                       // largest |dz| of this wave's tiles (AB.amax)
    // the net's gradient gain bound G >= 1 (mlp.hip: split_gain_kernel, behind the planes): no hidden gradient of a tile exceeds
    // G max |dz|.  ge = ceil(log2 G)
    const float *gainp = reinterpret_cast<const float *>(A.planes + (size_t)(S::BASE_CHUNK + L.total_chunks) * 512);
    const int gbits = __builtin_amdgcn_readfirstlane(__float_as_int(*gainp));
    const int kbase = __builtin_amdgcn_readfirstlane(141 + 127 - ((gbits >> 23) & 0xff) - ((gbits & 0x7fffff) ? 1 : 0));   // 141 - ge (scalar)
    // LDS buffer of step st = (st + par) & 1: a net with an odd number of steps per group (the 128-wide nets: 7) starts every
    // other group in buffer 1
    for (int tg = (int)blockIdx.x - blk0, trip = 0; tg < ngroups; tg += nblk, ++trip) {
        const int par = (NS & 1) ? (trip & 1) : 0;
        const int tt = A.t0 + tg * SPW + wv;
        const bool live = tt < A.t1;
        const int t = live ? tt : A.t1 - 1;
        int hv = hvoff;                                                       // (opaque per group: see the forward)
        asm volatile("" : "+v"(hv));
        // the tile's scale: 2^k with G x (the largest |dz| of its 32 samples) in [2^14, 2^15) (exponent arithmetic; an all-zero
        // tile: 1): every plane of the chain stays below fp16's 65504 whatever the masks and signs do
        float zmax = 0.f;
#pragma unroll
        for (int i = 0; i < D.out_dim; ++i) zmax = fmaxf(zmax, fabsf(zn[i]));
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) zmax = fmaxf(zmax, __shfl_xor(zmax, o));
        if (live) wmax = fmaxf(wmax, zmax);                                   // (the launch's maximum: one atomic per wave, at the end)
        const int ez = (__float_as_int(zmax) >> 23) & 0xff;                   // biased exponent of the maximum
        const int ks = ez == 0 ? 0 : kbase - ez;                              // scale exponent: G max lands in [2^14, 2^15)
        const int kc = ks < -100 ? -100 : (ks > 100 ? 100 : ks);
        const float sc = __int_as_float((127 + kc) << 23), isc = __int_as_float((127 - kc) << 23);
        f16x8 xi1[1], xi2[1];
        {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (h == 0 && i < D.out_dim) ? zn[i < D.out_dim ? i : 0] * sc : 0.f;
            split8(v, xi1[0], xi2[0]);
        }
        unsigned msk[NHID][HT / 2];
#pragma unroll
        for (int l = 0; l < NHID; ++l)
#pragma unroll
            for (int w = 0; w < HT / 2; ++w) msk[l][w] = mn[l][w];
        // DG_TONE_IN: what the tile's closing contraction reads, requested here, a tile's matrix work ahead of its use: the record's
        // ray first (the g_lin gather waits for it alone), the partner row of Xt of each held dXt row -- tin_slots rows per lane,
        // which row depends on the lane half -- and the pre-activations
        [[maybe_unused]] int tin_ray = -1;
        [[maybe_unused]] float tin_w = 0.f, tin_x[TIN_SLOTS], tin_z[3], tin_p[9];
        if constexpr (MODE == DG_TONE_IN) {
            tin_ray = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(TI.rec_ray + (size_t)t * 32, 128), s_ * 4, 0, 0);
            tin_w = bload1(make_rsrc(TI.rec_w + (size_t)t * 32, 128), s_ * 4, 0);
            const rsrc_t RXT = make_rsrc(TI.Xt + (size_t)t * TIN_XT_ROWS * 32, TIN_XT_ROWS * 128);
#pragma unroll
            for (int k = 0; k < TIN_SLOTS; ++k) {
                const int row0 = tin_slot_row(k), row1 = row0 + 4;
                const int p0 = tin_partner(row0) < 0 ? 0 : tin_partner(row0), p1 = tin_partner(row1) < 0 ? 0 : tin_partner(row1);
                tin_x[k] = bload1(RXT, ((h ? p1 : p0) * 32 + s_) * 4, 0);
            }
            const rsrc_t RZ3 = make_rsrc((t < TI.tiles_on ? TI.z_emo : TI.z_off) + (size_t)t * 4 * 32, 3 * 128);
#pragma unroll
            for (int c = 0; c < 3; ++c) tin_z[c] = bload1(RZ3, s_ * 4, c * 128);
#pragma unroll
            for (int c = 0; c < 9; ++c) tin_p[c] = 0.f;
        }
        fetch(tg + nblk < ngroups ? tg + nblk : tg);
        f16x8 pa1[2 * HT], pa2[2 * HT], pb1[2 * HT], pb2[2 * HT];
        f32x16 am[2];
        float ev[16];
        const float wisc = SPLIT_W_INV * isc;                                 // accumulator (64 x the scaled gradient) -> the fp32 store
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

        // micro-slices of a finished tile of transposed layer q (8 register pairs x 3 phases, as in the forward):
        //   q < 3: phase 0 value (scaled), ReLU mask of the layer below, the unscaled fp32 dZ store; phases 1 / 2 the planes
        //   q = 3: phase 0 unscaled value -> dX rows (the descriptor ends at row 44: the rows above are not written)
        auto micro = [&](auto QC, auto IT, auto MS, f32x16 &accm, auto &o1, auto &o2) __attribute__((always_inline)) {
            constexpr int q = decltype(QC)::value, it = decltype(IT)::value, ms = decltype(MS)::value, p = ms / 3, ph = ms % 3;
            constexpr int r0 = 2 * p, jj = r0 >> 3, i0 = r0 & 7;
            if constexpr (q == NL - 1 && MODE == DG_TONE_IN) {
                // the tone mapper's input stage folded in: held row r of dXt (64 / wisc x its value) times coef(r) Xt[partner(r)] into
                // the partial sum of the row's channel.  The row, hence the channel, differs between the lane halves: one partial
                // per PAIR of channels (half 0's, half 1's), sorted out per half when the tile is finished.  Plain C++: the
                // compiler places the wait states behind the MFMA.
                if constexpr (ph == 0) {
#pragma unroll
                    for (int rr = r0; rr < r0 + 2; ++rr) {
                        const int k = 16 * it + rr, row0 = 32 * it + acc_row(rr, 0), row1 = row0 + 4;
                        if (k < TIN_SLOTS) {
                            float x = tin_x[k];
                            if (tin_partner(row0) < 0) x = h ? x : 1.f;               // (a linear row: no partner factor)
                            const float cf = h ? tin_coef(row1) : tin_coef(row0);
                            float &acc = tin_p[tin_chan(row0) * 3 + (row1 < TIN_ROWS ? tin_chan(row1) : 0)];
                            acc = fmaf(accm[rr], x * cf, acc);
                        }
                    }
                }
            } else if constexpr (q == NL - 1) {
                // (a register pair whose rows are past the stored rows in BOTH lane halves: nothing to do -- DG_RT keeps issuing them)
                if constexpr (ph == 0 && (MODE == DG_RT || 32 * it + acc_row(r0, 0) < DX_STORED)) {
                    const float v0 = accm[r0] * wisc, v1 = accm[r0 + 1] * wisc;
                    const rsrc_t RX = make_rsrc(AB.dX + (size_t)t * 64 * 32, live ? dx_rows(KIND) / 4 * 4 * 128 + (dx_rows(KIND) % 4 ? 512 : 0) : 0);
                    asm volatile("" : "+v"(hv));
                    bstore1(RX, v0, hv + tile_soff(0, r0), it * 4096);           // (default policy: the scatter reads dX next)
                    bstore1(RX, v1, hv + tile_soff(0, r0 + 1), it * 4096);
                }
            } else {
                constexpr int d = NHID - 1 - q;                              // this tile is a tile of dZ[d]
                if constexpr (ph == 0) {
                    // mask bit -> 0 / ~0 with one v_bfe_i32 (in C, a shift pair or the bfe builtin became and + compare + select
                    // through vcc, with the wait states that go with vcc)
                    // (the operand is the mask word, loaded from memory a tile group ago: no MFMA result near this asm)
                    int k0, k1;
                    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(k0) : "v"(msk[d][it >> 1]), "n"((it & 1) * 16 + r0));
                    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(k1) : "v"(msk[d][it >> 1]), "n"((it & 1) * 16 + r0 + 1));
                    const int a0 = __float_as_int(accm[r0]) & k0, a1 = __float_as_int(accm[r0 + 1]) & k1;      // 64 x the masked value
                    if constexpr (STORE_DZ) {
                        const rsrc_t RD = make_rsrc(AB.dZ[d] + (size_t)t * (HBYTES / 4), (live && AB.dZ[d]) ? HBYTES : 0u);
                        asm volatile("" : "+v"(hv));
                        bstore1_nt(RD, __int_as_float(a0) * wisc, hv + tile_soff(0, r0), it * 4096);
                        bstore1_nt(RD, __int_as_float(a1) * wisc, hv + tile_soff(0, r0 + 1), it * 4096);
                    }
                    ev[r0] = __int_as_float(a0) * SPLIT_W_INV; ev[r0 + 1] = __int_as_float(a1) * SPLIT_W_INV;
                } else if constexpr (ph == 1) {
                    put_pair<i0>(o1[2 * it + jj], ev[r0], ev[r0 + 1]);
                } else {
                    put_residual_pair<i0>(o2[2 * it + jj], o1[2 * it + jj], ev[r0], ev[r0 + 1]);
                }
            }
        };
        // the pending tile's micro-slices u, u + navail, u + 2 navail, ... ride on MFMA slot u of the tile in flight (navail: as
        // in the forward)
        auto pending = [&](auto QC, auto IT, auto U, auto NAVAILC, f32x16 &accm, auto &o1, auto &o2) __attribute__((always_inline)) {
            constexpr int u = decltype(U)::value, navail = decltype(NAVAILC)::value;
            static_assert(navail >= 3 && navail % 3 == 0, "whole register pairs per pass");
            if constexpr (u < navail)
                sfor<0, (24 + navail - 1) / navail>([&](auto KC) {
                    constexpr int msi = u + decltype(KC)::value * navail;
                    if constexpr (msi < 24) micro(QC, IT, std::integral_constant<int, msi>{}, accm, o1, o2);
                });
        };
        auto run_layer = [&](auto QC, auto &in1, auto &in2, auto &o1, auto &o2) __attribute__((always_inline)) {
            constexpr int q = decltype(QC)::value, KS = L.ks[q], NT = L.tiles_out[q], NP = L.pairs[q];
            constexpr int s0 = [] { int s = 0; for (int k = 0; k < q; ++k) s += L.pairs[k]; return s; }();
            sfor<0, NP>([&](auto PC) {
                constexpr int p = decltype(PC)::value, st = s0 + p, tin = S::tiles_in(st), nxt_st = (st + 1) % NS;
                const unsigned char *wsrc = S::RES ? wl + (S::chunk0(st) - S::BASE_CHUNK) * 1024 : wl + ((st + par) & 1) * S::BUF;
                const u32x4 *mine = reinterpret_cast<const u32x4 *>(wsrc) + lane;
                if constexpr (!S::RES) stage_load(std::integral_constant<int, nxt_st>{});
                constexpr int NTOT = tin * KS;
                u32x4 wb[WRING][2];
                sfor<0, (WRING - 1 < NTOT ? WRING - 1 : NTOT)>([&](auto NC) {
                    constexpr int n0 = decltype(NC)::value, t0_ = n0 / KS, j0_ = n0 % KS;
                    wb[n0][0] = mine[((t0_ * 2 + 0) * KS + j0_) * 64];
                    wb[n0][1] = mine[((t0_ * 2 + 1) * KS + j0_) * 64];
                });
                sfor<0, NTOT>([&](auto NC) {
                    constexpr int n = decltype(NC)::value, tt_ = n / KS, j = n % KS, it = 2 * p + tt_;
                    if constexpr (n + WRING - 1 < NTOT) {
                        constexpr int t2 = (n + WRING - 1) / KS, j2 = (n + WRING - 1) % KS;
                        wb[(n + WRING - 1) % WRING][0] = mine[((t2 * 2 + 0) * KS + j2) * 64];
                        wb[(n + WRING - 1) % WRING][1] = mine[((t2 * 2 + 1) * KS + j2) * 64];
                    }
                    f32x16 &m = am[it & 1];
                    const f16x8 w1 = __builtin_bit_cast(f16x8, wb[n % WRING][0]), w2 = __builtin_bit_cast(f16x8, wb[n % WRING][1]);
                    constexpr bool HAVE = it > 0 || q > 0;
                    constexpr int pq = it > 0 ? q : q - 1, pit = it > 0 ? it - 1 : (q > 0 ? L.tiles_out[q > 0 ? q - 1 : 0] - 1 : 0);
                    auto ride = [&](auto U) __attribute__((always_inline)) {
                        if constexpr (HAVE) {
                            if constexpr (it > 0) pending(std::integral_constant<int, pq>{}, std::integral_constant<int, pit>{}, U,
                                                          std::integral_constant<int, 3 * KS>{}, am[pit & 1], o1, o2);
                            else pending(std::integral_constant<int, pq>{}, std::integral_constant<int, pit>{}, U,
                                         std::integral_constant<int, 3 * (KS - 2)>{}, am[pit & 1], in1, in2);
                        }
                        if constexpr (tt_ == tin - 1 && 3 * KS >= S::PRE && !S::RES) {
                            constexpr int u_ = decltype(U)::value, first = 3 * KS - S::PRE;
                            if constexpr (u_ >= first) stage_piece(std::integral_constant<int, nxt_st>{}, std::integral_constant<int, u_ - first>{},
                                                                   wl + ((st + 1 + par) & 1) * S::BUF);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    };
                    m = mfma_h(w1, in2[j], j == 0 ? zero16 : m);
                    ride(std::integral_constant<int, 3 * j + 0>{});
                    m = mfma_h(w1, in1[j], m);
                    ride(std::integral_constant<int, 3 * j + 1>{});
                    m = mfma_h(w2, in1[j], m);
                    ride(std::integral_constant<int, 3 * j + 2>{});
                });
                if constexpr (q == NL - 1 && p == NP - 1) {         // the very last tile (dX rows 32..63): nobody to ride on
                    sfor<0, 24>([&](auto MC) {
                        micro(QC, std::integral_constant<int, NT - 1>{}, MC, am[(NT - 1) & 1], o1, o2);
                    });
                }
                if constexpr (3 * KS < S::PRE && !S::RES)          // (the one-k-step first layer: too few slots, all pieces here)
                    stage_store(std::integral_constant<int, nxt_st>{}, wl + ((st + 1 + par) & 1) * S::BUF);
                if constexpr (!S::RES) step_barrier();
            });
        };
        run_layer(std::integral_constant<int, 0>{}, xi1, xi2, pa1, pa2);      // W3ᵀ dz -> dZ[2]   (tone mapper: W1ᵀ dz -> dZ[0])
        if constexpr (NL == 4) {
            run_layer(std::integral_constant<int, 1>{}, pa1, pa2, pb1, pb2);  // -> dZ[1]
            run_layer(std::integral_constant<int, 2>{}, pb1, pb2, pa1, pa2);  // -> dZ[0]
        }
        [[maybe_unused]] float tin_g[3] = {0.f, 0.f, 0.f};
        if constexpr (MODE == DG_TONE_IN) {                                        // (issued here: back before the last layer ends)
#pragma unroll
            for (int c = 0; c < 3; ++c) tin_g[c] = tin_ray >= 0 ? TI.g_lin[3 * (size_t)tin_ray + c] : 0.f;
        }
        run_layer(std::integral_constant<int, NL - 1>{}, pa1, pa2, pb1, pb2);      // -> dX (pb unused)
        if constexpr (MODE == DG_TONE_IN) {
            // dz[c] = (rec_w g_lin[ray, c] + sum over the channel's 11 rows) softplus'(z[c]) -- esr_fine_tone_in_bwd's result, 0 on a
            // padding lane and in row 3.  A lane's own partials: half 0 holds the rows whose FIRST channel index is c, half 1 those
            // whose second is; the other half's share comes over one exchange per channel.
            float dzc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float a = 0.f, b = 0.f;
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    if (tin_pair_used(c * 3 + o)) a += tin_p[c * 3 + o];
                    if (tin_pair_used(o * 3 + c)) b += tin_p[o * 3 + c];
                }
                const float own = h ? b : a;
                const float sum = (own + __shfl_xor(own, 32)) * wisc;
                const float sg = tin_z[c] > 20.f ? 1.f : esr_sigmoid(tin_z[c]);
                dzc[c] = tin_ray >= 0 ? (tin_w * tin_g[c] + sum) * sg : 0.f;
            }
            const rsrc_t RDZ = make_rsrc(TI.dz + (size_t)t * 4 * 32, live ? 4 * 128 : 0);
            bstore1(RDZ, h ? dzc[2] : dzc[0], (2 * h * 32 + s_) * 4, 0);              // half 0: rows 0, 1; half 1: row 2 and the zero row
            bstore1(RDZ, h ? 0.f : dzc[1], (2 * h * 32 + s_) * 4, 128);
        }
    }
    // max |dz| of the launch: one atomic per wave, and only from a wave that would raise the value (non-negative floats order
    // like their bit patterns).  One atomic per TILE -- 16 384 on one address at C2 -- took 0.14 ms to drain: twice the tone
    // mapper's whole launch.
    // (what the weight-gradient kernels scale by: max |dz| x max(1, G / 16) -- their headroom above the scale source is >= 32x, so
    //  G max |dz|, the bound of every hidden gradient, fits their planes as well)
    wmax *= fmaxf(1.f, *gainp * 0.0625f);
    if (AB.amax && lane == 0 && wmax > *reinterpret_cast<volatile float *>(AB.amax))
        atomicMax(reinterpret_cast<unsigned *>(AB.amax), __float_as_uint(wmax));
