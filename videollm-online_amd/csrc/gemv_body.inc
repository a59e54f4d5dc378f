// gemv_body.inc — the body of the weight-streaming GEMV (see gemv.hip for the description), included TEXTUALLY by
// gemv16_kernel (gemv.hip):  VLO_GEMV_BX / BY / GX = blockIdx.x / blockIdx.y / gridDim.x, `a` = the kernel argument,
// `red` = the block's dynamic LDS.
// Expects in scope: template parameters KF, NW, XSRC, EPI, WQ, GB; `GemvArgs a` (value or reference); `float4 *red`.
// GB = groups per batch.  GB = 1: a wave finishes one group (all its KC chunks) before the next.  GB > 1 (launched when KC > 1,
// i.e. K = 8192 at 8 waves x 16 fragments: the 70B model's qkv / o / gate-up / lm_head): the chunk loop is the OUTER loop over a
// batch of GB groups, so a chunk's activation fragments are built once per batch instead of once per group — with KC = 2 every
// (group, chunk) item re-read 16 fragments of x (as many bytes as a bf16 item's weights, twice an fp8 item's) and, under
// XSRC_NORM, re-normalised them (~800 VALU operations per item against 16 MFMAs): the fp8 gate/up GEMV of the 70B shape ran at
// 3.9 TB/s where the same stream with KC = 1 (8B shape) reaches 4.3 and its bf16 twin 5.8.
#include "gemv_head.inc"

    // ---- activation fragments of one K chunk (B operand): x[m = lane&15][k .. k+8] -------------
    // rows past the step's n_rows read the last row (finite values, one unconditional load per fragment): every epilogue writes rows < n_rows only.
    // (A predicated load per fragment — sixteen one-instruction branches — made hipcc open every weight item with `s_waitcnt vmcnt(0)`.)
    // XSRC_NORM: the raw loads (residual-stream rows + norm weights) and the arithmetic are two steps, so that with ONE chunk per wave (KC == 1: every
    // 8B / TinyLlama shape) the loads go out right behind the first weight fragments and their latency hides behind the reduction of the row sums
    // of squares below instead of following it (one memory round trip off the kernel's start).
    frag_ab xf[KF];
    frag_ab xw[XSRC == XSRC_NORM ? KF : 1];                    // XSRC_NORM: the chunk's norm-weight fragments in flight (the h fragments wait in xf and are normalised in place)
    auto issue_x = [&](int c) {
        const size_t k0 = (size_t)(kfw0 + c * KF) * 32 + qd * 8;
        const bf16_t *xr = a.x + (size_t)min(m16, a.n_rows - 1) * a.ldx + k0;
        if constexpr (XSRC == XSRC_NORM) {
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
                xf[kf] = *reinterpret_cast<const frag_ab *>(xr + kf * 32);       // raw h (rows >= n_rows: rsm = 0 in finish_x)
                xw[kf] = *reinterpret_cast<const frag_ab *>(a.norm_w + k0 + kf * 32);
            }
        } else {
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) xf[kf] = *reinterpret_cast<const frag_ab *>(xr + kf * 32);
        }
    };
    issue_x(0);                             // unconditional (KC > 1: chunk 0 is simply issued again inside the chunk loop)

    // ---- XSRC_NORM: rs[m] = rsqrt(mean(h[m]^2) + eps) from the producer's partial sums --------
    if (XSRC == XSRC_NORM) {
        const int t = threadIdx.x, m = t & 15, sl = t >> 4, nsl = NW * 4;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < SQ_PRE; ++j) s += (sl + j * nsl < a.sq_in_parts) ? sq_pre[j] : 0.f;      // loaded at the top of the kernel (gemv_head.inc)
        for (int p = sl + SQ_PRE * nsl; p < a.sq_in_parts; p += nsl) s += a.sq_in[p * 16 + m];      // (more than 8 * nsl producer blocks: never at the model shapes)
        tmp_lds[sl * 16 + m] = s;
        __syncthreads();
        if (t < 16) {
            float tot = 0.f;
            for (int i = 0; i < nsl; ++i) tot += tmp_lds[i * 16 + t];
            rs_lds[t] = (t < a.n_rows) ? 1.0f / sqrtf(tot / (float)a.K + a.eps) : 0.f;
        }
        __syncthreads();
    }
    auto finish_x = [&]() {                 // XSRC_NORM: weight * (x * rsqrt(var + eps)).to(bf16)   (HF :66-67)
        if constexpr (XSRC == XSRC_NORM) {
            const float rsm = rs_lds[m16];
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
                const frag_ab hv = xf[kf], wv = xw[kf];
                unsigned pk[4];
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const unsigned t2 = pack2bf(bf2f((bf16_t)hv[j]) * rsm, bf2f((bf16_t)hv[j + 1]) * rsm);
                    pk[j >> 1] = pack2bf(bf2f((bf16_t)wv[j]) * __uint_as_float(t2 << 16),
                                         bf2f((bf16_t)wv[j + 1]) * __uint_as_float(t2 & 0xffff0000u));
                }
                xf[kf] = __builtin_bit_cast(frag_ab, make_uint4(pk[0], pk[1], pk[2], pk[3]));
            }
        }
    };
    auto load_x = [&](int c) {              // a chunk's fragments in one go (KC > 1: inside the chunk loop)
        issue_x(c);
        finish_x();
    };
    if (a.KC == 1) finish_x();

    float sq_acc = 0.f;                    // EPI_RESID: this wave's running sum of squares for row lane&15
    int buf = 0;
    if constexpr (GB == 1) {
        for (; g < ngroups; g += VLO_GEMV_GX) {
            const int tA = tile_a(g), tB = tile_b(g);
            const bool hasB = tB < a.NT;
            const int gn = g + VLO_GEMV_GX;
            float4 *rb = red + (size_t)buf * NW * CTG * 64;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < a.KC; ++c) {
                if (a.KC > 1) load_x(c);
                // one item = this wave's K chunk of one tile: WRN weight registers against the chunk's activation fragments; register i
                // is re-loaded for the NEXT item right after the MFMA(s) that consumed it.  fp8 image: a register holds two fragments,
                // expanded e4m3 -> bf16 (exact) in VALU slots the HBM-bound loop has to spare
                auto mm = [&](f32x4 &acc, int i) {
                    if constexpr (WQ == 2) {
                        frag_ab f0, f1, f2, f3;
                        fp4x32_to_bf16(wr[i], sr[i], f0, f1, f2, f3);
                        acc = mfma_bf16(f0, xf[4 * i], acc);
                        acc = mfma_bf16(f1, xf[4 * i + 1], acc);
                        acc = mfma_bf16(f2, xf[4 * i + 2], acc);
                        acc = mfma_bf16(f3, xf[4 * i + 3], acc);
                    } else if (WQ) {
                        frag_ab f0, f1;
                        fp8x16_to_bf16(wr[i], f0, f1);
                        acc = mfma_bf16(f0, xf[2 * i], acc);
                        acc = mfma_bf16(f1, xf[2 * i + 1], acc);
                    } else {
                        acc = mfma_bf16(wr[i], xf[i], acc);
                    }
                };
                auto item = [&](f32x4 &acc, const frag_ab *np) {
                    if (np) {
#pragma unroll
                        for (int i = 0; i < WRN; ++i) {
                            mm(acc, i);
                            wr[i] = __builtin_nontemporal_load(np + i * 64);
                            if constexpr (WQ == 2) sr[i] = __builtin_nontemporal_load(scale_ptr(np) + i * 16);
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < WRN; ++i) mm(acc, i);
                    }
                };
                // item (c, A); next item is (c, B) | (c+1, A) | (next group, 0, A) | none
                item(acc0, hasB ? item_ptr(tB, c) : (c + 1 < a.KC ? item_ptr(tA, c + 1) : (gn < ngroups ? item_ptr(tile_a(gn), 0) : nullptr)));
                if (hasB) item(acc1, c + 1 < a.KC ? item_ptr(tA, c + 1) : (gn < ngroups ? item_ptr(tile_a(gn), 0) : nullptr));
            }
#include "gemv_epi.inc"
            buf ^= 1;
        }
    } else {
        // batches of GB groups (g, g + GX, ...): chunk-outer, see the header.  Item order inside a batch: (c, j, A), (c, j, B) for
        // j = 0 .. GB-1, then chunk c + 1; the rolling prefetch follows that order across chunks and batches
        auto mm = [&](f32x4 &acc, int i) {
            if constexpr (WQ == 2) {
                frag_ab f0, f1, f2, f3;
                fp4x32_to_bf16(wr[i], sr[i], f0, f1, f2, f3);
                acc = mfma_bf16(f0, xf[4 * i], acc);
                acc = mfma_bf16(f1, xf[4 * i + 1], acc);
                acc = mfma_bf16(f2, xf[4 * i + 2], acc);
                acc = mfma_bf16(f3, xf[4 * i + 3], acc);
            } else if (WQ) {
                frag_ab f0, f1;
                fp8x16_to_bf16(wr[i], f0, f1);
                acc = mfma_bf16(f0, xf[2 * i], acc);
                acc = mfma_bf16(f1, xf[2 * i + 1], acc);
            } else {
                acc = mfma_bf16(wr[i], xf[i], acc);
            }
        };
        auto item = [&](f32x4 &acc, const frag_ab *np) {
            if (np) {
#pragma unroll
                for (int i = 0; i < WRN; ++i) {
                    mm(acc, i);
                    wr[i] = __builtin_nontemporal_load(np + i * 64);
                    if constexpr (WQ == 2) sr[i] = __builtin_nontemporal_load(scale_ptr(np) + i * 16);
                }
            } else {
#pragma unroll
                for (int i = 0; i < WRN; ++i) mm(acc, i);
            }
        };
        for (int g0 = g; g0 < ngroups; g0 += VLO_GEMV_GX * GB) {
            f32x4 acc[GB][2];
#pragma unroll
            for (int j = 0; j < GB; ++j) acc[j][0] = acc[j][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int gnb = g0 + VLO_GEMV_GX * GB;                        // first group of the next batch
            for (int c = 0; c < a.KC; ++c) {
                load_x(c);
#pragma unroll
                for (int j = 0; j < GB; ++j) {
                    const int gj = g0 + j * VLO_GEMV_GX;
                    if (gj < ngroups) {                                    // block-uniform
                        const int tA = tile_a(gj), tB = tile_b(gj);
                        const bool hasB = tB < a.NT;
                        const int gj1 = gj + VLO_GEMV_GX;
                        const frag_ab *nxt = (j + 1 < GB && gj1 < ngroups) ? item_ptr(tile_a(gj1), c)
                                             : (c + 1 < a.KC ? item_ptr(tile_a(g0), c + 1) : (gnb < ngroups ? item_ptr(tile_a(gnb), 0) : nullptr));
                        item(acc[j][0], hasB ? item_ptr(tB, c) : nxt);
                        if (hasB) item(acc[j][1], nxt);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < GB; ++j) {
                const int g = g0 + j * VLO_GEMV_GX;                        // (shadows the block's first group: the epilogue text reads `g`)
                if (g < ngroups) {
                    const int tA = tile_a(g), tB = tile_b(g);
                    const f32x4 acc0 = acc[j][0], acc1 = acc[j][1];
                    float4 *rb = red + (size_t)buf * NW * CTG * 64;
#include "gemv_epi.inc"
                    buf ^= 1;
                }
            }
        }
    }
    if (EPI == EPI_RESID) {
        // deterministic block total of the row sums of squares -> sq_out[block x][16]
        __syncthreads();
        if (lane < 16) tmp_lds[w * 16 + lane] = sq_acc;
        __syncthreads();
        if (threadIdx.x < 16) {
            float tot = 0.f;
            for (int ww = 0; ww < NW; ++ww) tot += tmp_lds[ww * 16 + threadIdx.x];
            a.sq_out[(size_t)VLO_GEMV_BX * 16 + threadIdx.x] = tot;
        }
    }
