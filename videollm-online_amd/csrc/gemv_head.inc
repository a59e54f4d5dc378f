// gemv_head.inc — first part of the GEMV body (gemv_body.inc includes it): this block's geometry and its first weight
// fragments, which go in flight before anything else.
// Expects in scope: template parameters KF, NW, XSRC, EPI, WQ; `GemvArgs a`; `float4 *red`; VLO_GEMV_BX / VLO_GEMV_BY.
// WQ = 1: the weight image is fp8 e4m3 (see gemv.hip): one 16-byte lane load carries TWO MFMA fragments.
// WQ = 2: mxfp4 (e2m1 codes + e8m0 block scales): one 16-byte lane load carries FOUR fragments, one dword of `a.wblk` their four scale bytes.
    constexpr int CTG = 2;
    float *scratch = reinterpret_cast<float *>(red + 2 * NW * CTG * 64);   // rs[16] | tmp[NW*4][16]
    float *rs_lds = scratch;
    float *tmp_lds = scratch + 16;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int m16 = lane & 15, qd = lane >> 4;
    const int KFtot = a.K >> 5;
    const int kfw0 = (VLO_GEMV_BY * NW + w) * a.KC * KF;       // first fragment of this wave's K range

    // ---- group -> tiles -----------------------------------------------------------------
    const int hd = a.kv.head_dim;
    const int tph = epi_rope(EPI) ? hd / 16 : 2;           // tiles per head
    const int hp = tph / 2;                                    // rotary pairs of tiles per head
    // a.CT == 1: one tile per group (narrow outputs such as o_proj: NT = 256 tiles -> 256 blocks instead of 128)
    const bool single = (!epi_rope(EPI) && a.CT == 1);
    const int ngroups = epi_rope(EPI) ? a.NT / 2 : (single ? a.NT : (a.NT + 1) / 2);
    auto tile_a = [&](int g) { return epi_rope(EPI) ? (g / hp) * tph + (g % hp) : (single ? g : 2 * g); };
    auto tile_b = [&](int g) { return epi_rope(EPI) ? (g / hp) * tph + (g % hp) + hp : (single ? a.NT : 2 * g + 1); };

    constexpr int WRN = WQ == 2 ? KF / 4 : WQ ? KF / 2 : KF;                      // 16-byte weight registers per chunk (KiB in flight per wave)
    const frag_ab *wbase = reinterpret_cast<const frag_ab *>(a.Wp) + (size_t)(WQ == 2 ? kfw0 / 4 : WQ ? kfw0 / 2 : kfw0) * 64 + lane;
    const size_t tile_stride = (size_t)(WQ == 2 ? KFtot / 4 : WQ ? KFtot / 2 : KFtot) * 64;
    auto item_ptr = [&](int tile, int c) { return wbase + (size_t)tile * tile_stride + (size_t)c * WRN * 64; };
    // mxfp4: the scale dwords of weight register (tile, kf4) are the 16 dwords (one per row of the tile) at (tile * KFtot / 4 + kf4) * 16, i.e. a
    // quarter of the register's own offset: the scales of an item are found from the item's weight pointer and ride the same rolling prefetch
    const unsigned *sbase = WQ == 2 ? a.wblk + (size_t)(kfw0 / 4) * 16 + m16 : nullptr;
    auto scale_ptr = [&](const frag_ab *wp) { return sbase + ((wp - wbase) >> 2); };

    // ---- XSRC_NORM: the producer's row sums of squares head the kernel's only dependency chain (sums -> LDS -> barrier -> rsqrt -> normalised
    // activations -> first MFMA), so their loads go out FIRST — eight per thread cover sq_in_parts <= 8 * NW * 4 (256 producer blocks at 8 waves);
    // they are consumed in gemv_body.inc under a counted wait, with the weight and activation loads below already in flight behind them
    constexpr int SQ_PRE = 8;
    float sq_pre[XSRC == XSRC_NORM ? SQ_PRE : 1];
    if constexpr (XSRC == XSRC_NORM) {
        const int m = threadIdx.x & 15, sl = threadIdx.x >> 4;
#pragma unroll
        for (int j = 0; j < SQ_PRE; ++j) {
            const int pp = sl + j * NW * 4;
            sq_pre[j] = a.sq_in[(pp < a.sq_in_parts ? pp : 0) * 16 + m];      // (clamped: unconditional loads; masked where they are summed)
        }
    }

    // ---- first weight fragments go in flight right behind them -------------------------------
    frag_ab wr[WRN];
    unsigned sr[WQ == 2 ? WRN : 1];           // mxfp4: the four e8m0 scale bytes of each weight register
    int g = VLO_GEMV_BX;                     // < ngroups: gemv_grid_x never launches more blocks than groups, so the loads below need no predicate
    {                                        // (a load behind a branch makes every wait that follows a vmcnt(0))
        const frag_ab *wp = item_ptr(tile_a(g), 0);
#pragma unroll
        for (int kf = 0; kf < WRN; ++kf) wr[kf] = __builtin_nontemporal_load(wp + kf * 64);
        if constexpr (WQ == 2) {
#pragma unroll
            for (int kf = 0; kf < WRN; ++kf) sr[kf] = __builtin_nontemporal_load(scale_ptr(wp) + kf * 16);
        }
    }

