// attn_body.inc — the ONE definition of the chunk attention (algorithm: see llm_ops.hip above attn_chunk_kernel), included textually by its four
// kernels: attn_chunk_kernel, attn_chunk_f8_kernel, attn_chunk_seg_kernel, attn_chunk_seg_f8_kernel.  (A __device__ function would be the
// natural form, but no form tried keeps the kernels' machine code: profiles/attn_family_refactor.md.)
// The including kernel sets, and this file consumes (#undef at the end):
//   VLO_ATTN_F8        1: the pool holds e4m3 bytes (8-byte K / V^T pieces expanded to the bf16 fragments in registers), 0: bf16
//   VLO_ATTN_SUBCHUNK  which 16-query sub-chunk of a longer block of new tokens this workgroup serves: blockIdx.z in a solo launch (block
//                      path: queries z*16 .. z*16+n-1), 0 in a segmented launch (a segment IS one sub-chunk)
// Every name read from the including kernel is listed and type-checked here, so a kernel that does not provide one fails to compile:
    static_assert(HD % 32 == 0 && (HPW == 1 || HPW == 2), "template parameters HD, HPW");
    VLO_ATTN_NAME(q, const bf16_t *);            // the sub-chunk-0 query rows [n][nh * HD]
    VLO_ATTN_NAME(kv, KvGeom);                   // the pool; kv.page_table = the session's
    VLO_ATTN_NAME(layer, int);  VLO_ATTN_NAME(nh, int);  VLO_ATTN_NAME(G, int);  VLO_ATTN_NAME(KS, int);
    VLO_ATTN_NAME(pos0, int64_t);  VLO_ATTN_NAME(n, int);  VLO_ATTN_NAME(chunk, int);
    VLO_ATTN_NAME(scale, float);
    VLO_ATTN_NAME(part_o, float *);  VLO_ATTN_NAME(part_ml, float *);   // the launch's first partial state
#if VLO_ATTN_F8
    VLO_ATTN_NAME(kv_scale, const float *);
    const float vscale = attn_f8_scales(kv_scale, layer, scale);   // `scale` now carries k_scale; vscale multiplies the partial output
#endif
    extern __shared__ __attribute__((aligned(16))) float4 lds_o[];        // [(KS-1)*NHG][HPW][NDT][64] float4, then m/l
    constexpr int NKK = HD / 32, NDT = HD / 16;
    const int NHG = G / HPW;
    float *lds_ml = reinterpret_cast<float *>(lds_o + (size_t)(KS - 1) * NHG * HPW * NDT * 64);   // [(KS-1)*NHG][HPW][16][2]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int hg = w % NHG, ks = w / NHG;
    const int split = blockIdx.x, kvh = blockIdx.y;
    {
        const int z = VLO_ATTN_SUBCHUNK;
        q += (size_t)z * 16 * nh * HD;
        pos0 += 16 * z;
        n = min(16, n - 16 * z);
        part_o += (size_t)z * gridDim.x * nh * 16 * HD;
        part_ml += (size_t)z * gridDim.x * nh * 16 * 2;
    }
    const int L = (int)(pos0 + n);
    const int c0 = split * chunk, c1 = min(L, c0 + chunk);
    const int head0 = kvh * G + hg * HPW;
    const int qrow = lane & 15, qd = lane >> 4;

    frag_ab qf[HPW][NKK];
#pragma unroll
    for (int h = 0; h < HPW; ++h)
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            frag_ab z = {0, 0, 0, 0, 0, 0, 0, 0};
            if (qrow < n) z = *reinterpret_cast<const frag_ab *>(q + (size_t)qrow * nh * HD + (size_t)(head0 + h) * HD + kk * 32 + qd * 8);
            qf[h][kk] = z;
        }
    f32x4 O[HPW][NDT];
    float mrun[HPW], lrun[HPW];
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
        mrun[h] = -INFINITY;
        lrun[h] = 0.f;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) O[h][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int qpos = (int)pos0 + min(qrow, n - 1);
#if VLO_ATTN_F8
    typedef uint8_t kv_t;                                          // one e4m3 byte per element, same element offsets
    typedef uint2 kraw_t;                                          // 8 bytes = one fragment before expansion
#else
    typedef bf16_t kv_t;
    typedef frag_ab kraw_t;
#endif
    const kv_t *kbase = reinterpret_cast<const kv_t *>(kv.k_pool) + (size_t)layer * kv.layer_stride;
    const kv_t *vbase = reinterpret_cast<const kv_t *>(kv.vt_pool) + (size_t)layer * kv.layer_stride;

    // K fragments are fetched one 32-key block AHEAD (register double buffer), so the HBM latency of block i+1 hides
    // behind the MFMAs / softmax of block i; V^T fragments of the current block are issued first thing in the
    // iteration and are only needed after QK^T + softmax.
    auto load_k = [&](int kt0, kraw_t (&dst)[2][NKK]) {
        const int page = kv.page_table[kt0 / VLO_PAGE_TOKENS];
        const kv_t *kp = kbase + (size_t)page * kv.page_elems + ((size_t)kvh * VLO_PAGE_TOKENS + kt0 % VLO_PAGE_TOKENS) * HD;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk)
                dst[t][kk] = *reinterpret_cast<const kraw_t *>(kp + (size_t)(t * 16 + qrow) * HD + kk * 32 + qd * 8);
    };
    frag_ab kf[2][NKK];
    kraw_t kn[2][NKK];
    const int kfirst = c0 + ks * 32;
#if VLO_ATTN_F8
    if (kfirst < c1) {
        load_k(kfirst, kn);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) kf[t][kk] = fp8x8_to_bf16(kn[t][kk]);
    }
#else
    if (kfirst < c1) load_k(kfirst, kf);
#endif
    for (int kt0 = kfirst; kt0 < c1; kt0 += KS * 32) {
        const int page = kv.page_table[kt0 / VLO_PAGE_TOKENS];
        const int tok0 = kt0 % VLO_PAGE_TOKENS;
        const kv_t *vp = vbase + (size_t)page * kv.page_elems + ((size_t)kvh * HD) * VLO_PAGE_TOKENS + tok0;
        kraw_t vf[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const kv_t *vr = vp + (size_t)(dt * 16 + qrow) * VLO_PAGE_TOKENS + qd * 4;
#if VLO_ATTN_F8
            vf[dt] = make_uint2(*reinterpret_cast<const unsigned *>(vr), *reinterpret_cast<const unsigned *>(vr + 16));
#else
            const uint2 lo = *reinterpret_cast<const uint2 *>(vr);
            const uint2 hi = *reinterpret_cast<const uint2 *>(vr + 16);
            vf[dt] = __builtin_bit_cast(frag_ab, make_uint4(lo.x, lo.y, hi.x, hi.y));
#endif
        }
        const bool more = kt0 + KS * 32 < c1;
        if (more) load_k(kt0 + KS * 32, kn);
        const int kb = kt0 + qd * 4;
#pragma unroll
        for (int h = 0; h < HPW; ++h) {
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                s0 = mfma_bf16(kf[0][kk], qf[h][kk], s0);
                s1 = mfma_bf16(kf[1][kk], qf[h][kk], s1);
            }
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = (kb + r <= qpos) ? s0[r] * scale : -INFINITY;
                v[4 + r] = (kb + 16 + r <= qpos) ? s1[r] * scale : -INFINITY;
            }
            float tmax = v[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) tmax = fmaxf(tmax, v[j]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(mrun[h], tmax);
            const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __expf(mrun[h] - m_safe);
            mrun[h] = m_new;
            float psum = 0.f;
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                p[j] = __expf(v[j] - m_safe);
                psum += p[j];
            }
            const uint4 pk = make_uint4(pack2bf(p[0], p[1]), pack2bf(p[2], p[3]), pack2bf(p[4], p[5]), pack2bf(p[6], p[7]));
            const frag_ab pb = __builtin_bit_cast(frag_ab, pk);
            lrun[h] = lrun[h] * alpha + psum;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                f32x4 o = O[h][dt];
                o[0] *= alpha; o[1] *= alpha; o[2] *= alpha; o[3] *= alpha;
#if VLO_ATTN_F8
                O[h][dt] = mfma_bf16(fp8x8_to_bf16(vf[dt]), pb, o);
#else
                O[h][dt] = mfma_bf16(vf[dt], pb, o);
#endif
            }
        }
        if (more) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
#if VLO_ATTN_F8
                for (int kk = 0; kk < NKK; ++kk) kf[t][kk] = fp8x8_to_bf16(kn[t][kk]);
#else
                for (int kk = 0; kk < NKK; ++kk) kf[t][kk] = kn[t][kk];
#endif
        }
    }
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
        lrun[h] += __shfl_xor(lrun[h], 16, 64);
        lrun[h] += __shfl_xor(lrun[h], 32, 64);
    }
    // ---- merge the KS key sub-splits through LDS; waves with ks == 0 keep their state in registers
    if (KS > 1) {
        if (ks > 0) {
            const int slot = (ks - 1) * NHG + hg;
#pragma unroll
            for (int h = 0; h < HPW; ++h) {
                if (qd == 0) {
                    lds_ml[((slot * HPW + h) * 16 + qrow) * 2] = mrun[h];
                    lds_ml[((slot * HPW + h) * 16 + qrow) * 2 + 1] = lrun[h];
                }
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const f32x4 o = O[h][dt];
                    lds_o[((size_t)(slot * HPW + h) * NDT + dt) * 64 + lane] = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
        }
        __syncthreads();
        if (ks > 0) return;
#pragma unroll
        for (int h = 0; h < HPW; ++h) {
            float M = mrun[h];
            for (int k2 = 1; k2 < KS; ++k2) M = fmaxf(M, lds_ml[((((k2 - 1) * NHG + hg) * HPW + h) * 16 + qrow) * 2]);
            const float Ms = (M == -INFINITY) ? 0.f : M;
            const float w0 = __expf(mrun[h] - Ms);             // -inf -> 0
            float l = lrun[h] * w0;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) { O[h][dt][0] *= w0; O[h][dt][1] *= w0; O[h][dt][2] *= w0; O[h][dt][3] *= w0; }
            for (int k2 = 1; k2 < KS; ++k2) {
                const int slot = (k2 - 1) * NHG + hg;
                const float mk = lds_ml[((slot * HPW + h) * 16 + qrow) * 2];
                const float wk = __expf(mk - Ms);
                l += lds_ml[((slot * HPW + h) * 16 + qrow) * 2 + 1] * wk;
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const float4 o = lds_o[((size_t)(slot * HPW + h) * NDT + dt) * 64 + lane];
                    O[h][dt][0] += o.x * wk; O[h][dt][1] += o.y * wk; O[h][dt][2] += o.z * wk; O[h][dt][3] += o.w * wk;
                }
            }
            mrun[h] = M;
            lrun[h] = l;
        }
    }
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
        const size_t row = ((size_t)split * nh + head0 + h) * 16 + qrow;
        if (qd == 0) {
            part_ml[row * 2] = mrun[h];
            part_ml[row * 2 + 1] = lrun[h];
        }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
#if VLO_ATTN_F8
            const f32x4 o = O[h][dt] * vscale;                     // sum_j p_j v_code_j v_scale
#else
            const f32x4 o = O[h][dt];
#endif
            *reinterpret_cast<float4 *>(part_o + row * HD + dt * 16 + qd * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
#undef VLO_ATTN_F8
#undef VLO_ATTN_SUBCHUNK
