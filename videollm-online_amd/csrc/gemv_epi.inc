// gemv_epi.inc — one group's finish in the weight-streaming GEMV (gemv_body.inc includes it TEXTUALLY, once per loop form): the wave's
// partial tiles go to LDS (`rb`, double-buffered by the caller), one barrier, then the cross-wave reduction and the epilogue.
// Expects in scope: g, tA, tB (the group and its two tiles), acc0, acc1 (f32x4), rb; everything gemv_body.inc has in scope.
        rb[(w * CTG + 0) * 64 + lane] = make_float4(acc0[0], acc0[1], acc0[2], acc0[3]);
        rb[(w * CTG + 1) * 64 + lane] = make_float4(acc1[0], acc1[1], acc1[2], acc1[3]);
        __syncthreads();

        // ---- cross-wave reduction + epilogue ------------------------------------------------
        if (epi_rope(EPI)) {
            // both tiles of the group are needed by the same lane (rotary pair): one wave
            if (threadIdx.x < 64) {
                const int l = lane;
                float4 sA = make_float4(0, 0, 0, 0), sB = make_float4(0, 0, 0, 0);
#pragma unroll
                for (int ww = 0; ww < NW; ++ww) {
                    sA = f4add(sA, rb[(ww * CTG + 0) * 64 + l]);
                    sB = f4add(sB, rb[(ww * CTG + 1) * 64 + l]);
                }
                if (WQ == 1) {                             // per-output-channel weight scales (packed row order; the mxfp4 image carries its block scales in the stream)
                    sA = f4mul(sA, *reinterpret_cast<const float4 *>(a.wscale + tA * 16 + (l >> 4) * 4));
                    sB = f4mul(sB, *reinterpret_cast<const float4 *>(a.wscale + tB * 16 + (l >> 4) * 4));
                }
                const int m = l & 15;
                if (m < a.n_rows) {
                    const float va[4] = {sA.x, sA.y, sA.z, sA.w}, vb[4] = {sB.x, sB.y, sB.z, sB.w};
                    {
                        const int half = hd >> 1, nh = a.num_heads, nkv = a.kv.num_kv_heads;
                        const int head = g / hp, i = (g % hp) * 16 + (l >> 4) * 4;   // column inside the head, < half
                        long long pos;
                        int page;
                        if constexpr (epi_rows(EPI)) {                    // batched step: the row's own position and page (gemv.h RopeRow)
                            const RopeRow rr = reinterpret_cast<const RopeRow *>(a.kv.page_table)[m];
                            pos = rr.pos;
                            page = rr.page;
                        } else {
                            pos = a.pos0 + m;
                            page = a.kv.page_table[pos / VLO_PAGE_TOKENS];
                        }
                        const int tok = (int)(pos % VLO_PAGE_TOKENS);
                        if (head < nh + nkv) {
                            bf16_t *dst = (head < nh)
                                ? a.out_bf16 + (size_t)m * nh * hd + (size_t)head * hd
                                : a.kv.k_pool + (size_t)a.layer * a.kv.layer_stride + (size_t)page * a.kv.page_elems +
                                      ((size_t)(head - nh) * VLO_PAGE_TOKENS + tok) * hd;
                            const ushort4 c4 = *reinterpret_cast<const ushort4 *>(a.cos_tab + pos * half + i);
                            const ushort4 s4 = *reinterpret_cast<const ushort4 *>(a.sin_tab + pos * half + i);
                            const bf16_t cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
                            bf16_t lo[4], hi[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float x1 = rbf(va[r]), x2 = rbf(vb[r]);      // projection output is bf16
                                const float c = bf2f(cc[r]), s = bf2f(ss[r]);
                                // q*cos + rotate_half(q)*sin, each product and the sum rounded to bf16 (:157-158)
                                lo[r] = f2bf(rbf(x1 * c) + rbf(-x2 * s));
                                hi[r] = f2bf(rbf(x2 * c) + rbf(x1 * s));
                            }
                            if (epi_kv_f8(EPI) && head >= nh) {
                                // fp8 pool: the bf16 K row quantised with the layer's k_scale, 4 + 4 bytes
                                const float ks = a.kv_scale[2 * a.layer];
                                uint8_t *d8 = reinterpret_cast<uint8_t *>(a.kv.k_pool) + (size_t)a.layer * a.kv.layer_stride +
                                              (size_t)page * a.kv.page_elems + ((size_t)(head - nh) * VLO_PAGE_TOKENS + tok) * hd;
                                *reinterpret_cast<unsigned *>(d8 + i) = fp8x4_quant(bf2f(lo[0]), bf2f(lo[1]), bf2f(lo[2]), bf2f(lo[3]), ks);
                                *reinterpret_cast<unsigned *>(d8 + half + i) = fp8x4_quant(bf2f(hi[0]), bf2f(hi[1]), bf2f(hi[2]), bf2f(hi[3]), ks);
                            } else {
                                *reinterpret_cast<ushort4 *>(dst + i) = *reinterpret_cast<const ushort4 *>(lo);
                                *reinterpret_cast<ushort4 *>(dst + half + i) = *reinterpret_cast<const ushort4 *>(hi);
                            }
                        } else if (epi_kv_f8(EPI)) {
                            // fp8 V^T: this lane's 4 + 4 head-dim rows of one token are bytes VLO_PAGE_TOKENS apart; the 16 lanes of a row hold
                            // 16 consecutive tokens, so each byte store of the wave covers 16 adjacent bytes
                            const float vs = a.kv_scale[2 * a.layer + 1];
                            uint8_t *d8 = reinterpret_cast<uint8_t *>(a.kv.vt_pool) + (size_t)a.layer * a.kv.layer_stride + (size_t)page * a.kv.page_elems +
                                          ((size_t)(head - nh - nkv) * hd) * VLO_PAGE_TOKENS + tok;
                            const unsigned ca = fp8x4_quant(rbf(va[0]), rbf(va[1]), rbf(va[2]), rbf(va[3]), vs);
                            const unsigned cb = fp8x4_quant(rbf(vb[0]), rbf(vb[1]), rbf(vb[2]), rbf(vb[3]), vs);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                d8[(size_t)(i + r) * VLO_PAGE_TOKENS] = (uint8_t)(ca >> (8 * r));
                                d8[(size_t)(half + i + r) * VLO_PAGE_TOKENS] = (uint8_t)(cb >> (8 * r));
                            }
                        } else {
                            bf16_t *dst = a.kv.vt_pool + (size_t)a.layer * a.kv.layer_stride + (size_t)page * a.kv.page_elems +
                                          ((size_t)(head - nh - nkv) * hd) * VLO_PAGE_TOKENS + tok;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                dst[(size_t)(i + r) * VLO_PAGE_TOKENS] = f2bf(va[r]);
                                dst[(size_t)(half + i + r) * VLO_PAGE_TOKENS] = f2bf(vb[r]);
                            }
                        }
                    }
                }
            }
        } else {
            for (int t = threadIdx.x; t < CTG * 64; t += NW * 64) {
                const int ct = t >> 6, l = t & 63;
                const int tile = ct ? tB : tA;
                float4 s = make_float4(0, 0, 0, 0);
#pragma unroll
                for (int ww = 0; ww < NW; ++ww) s = f4add(s, rb[(ww * CTG + ct) * 64 + l]);
                const int m = l & 15;
                const int col = tile * 16 + (l >> 4) * 4;
                const bool live = (m < a.n_rows) && (tile < a.NT);
                if (WQ == 1 && tile < a.NT) s = f4mul(s, *reinterpret_cast<const float4 *>(a.wscale + col));
                if (EPI == EPI_SWIGLU) {
                    // tile = 8 gate rows (fragment rows 0..7, lanes 0..31) + the 8 up rows of the same columns (lanes 32..63)
                    if (live && l < 32) {
                        float4 u = make_float4(0, 0, 0, 0);
#pragma unroll
                        for (int ww = 0; ww < NW; ++ww) u = f4add(u, rb[(ww * CTG + ct) * 64 + l + 32]);
                        if (WQ == 1) u = f4mul(u, *reinterpret_cast<const float4 *>(a.wscale + col + 8));      // the tile's up rows
                        const float gv[4] = {s.x, s.y, s.z, s.w}, uv[4] = {u.x, u.y, u.z, u.w};
                        bf16_t o[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[r] = f2bf(silu_bf16(rbf(gv[r])) * rbf(uv[r]));
                        *reinterpret_cast<ushort4 *>(a.out_bf16 + (size_t)m * a.ldo + tile * 8 + (l >> 4) * 4) = *reinterpret_cast<const ushort4 *>(o);
                    }
                } else if (EPI == EPI_RESID) {
                    float sq = 0.f;
                    if (live) {
                        bf16_t *hp4 = a.h + (size_t)m * a.ldo + col;
                        const ushort4 hv = *reinterpret_cast<const ushort4 *>(hp4);
                        const bf16_t hh[4] = {hv.x, hv.y, hv.z, hv.w};
                        const float sv[4] = {s.x, s.y, s.z, s.w};
                        bf16_t o[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {      // Linear output -> bf16, then the bf16 residual add
                            const float hn = rbf(bf2f(hh[r]) + rbf(sv[r]));
                            o[r] = f2bf(hn);
                            sq += hn * hn;
                        }
                        *reinterpret_cast<ushort4 *>(hp4) = *reinterpret_cast<const ushort4 *>(o);
                    }
                    sq += __shfl_xor(sq, 16, 64);
                    sq += __shfl_xor(sq, 32, 64);
                    sq_acc += sq;                          // meaningful in lanes 0..15 (row = lane)
                } else if (live) {
                    if (EPI == EPI_PARTIAL_F32) {
                        *reinterpret_cast<float4 *>(a.out_f32 + ((size_t)VLO_GEMV_BY * 16 + m) * a.ldo + col) = s;
                    } else if (EPI == EPI_PARTIAL_MBOX) {
                        // one naturally aligned 8-byte system-scope store per element and peer: the granule carries its own ready tag (tp.hip)
                        typedef __attribute__((address_space(1))) unsigned long long gu64_t;
                        const unsigned sv[4] = {__float_as_uint(s.x), __float_as_uint(s.y), __float_as_uint(s.z), __float_as_uint(s.w)};
                        const size_t off = a.mbox_off + (size_t)m * a.ldo + col;
#pragma unroll
                        for (int p = 0; p < 8; ++p)
                            if (p < a.mbox_T)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    __hip_atomic_store((gu64_t *)(a.mbox[p] + off + r), ((unsigned long long)a.mbox_epoch << 32) | sv[r], __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_SYSTEM);
                    } else if (col < a.N_valid) {          // N padded to 16 at pack time; N_valid % 4 == 0
                        if (a.bias) {
                            const ushort4 b = *reinterpret_cast<const ushort4 *>(a.bias + col);
                            s.x += bf2f(b.x); s.y += bf2f(b.y); s.z += bf2f(b.z); s.w += bf2f(b.w);
                        }
                        ushort4 o;
                        if (EPI == EPI_BF16_GELU_ERF) {
                            o.x = f2bf(gelu_python_bf16(rbf(s.x))); o.y = f2bf(gelu_python_bf16(rbf(s.y)));
                            o.z = f2bf(gelu_python_bf16(rbf(s.z))); o.w = f2bf(gelu_python_bf16(rbf(s.w)));
                        } else {
                            o.x = f2bf(s.x); o.y = f2bf(s.y); o.z = f2bf(s.z); o.w = f2bf(s.w);
                        }
                        *reinterpret_cast<ushort4 *>(a.out_bf16 + (size_t)m * a.ldo + col) = o;
                    }
                }
            }
        }
