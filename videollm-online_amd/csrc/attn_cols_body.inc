// attn_cols_body.inc — the ONE definition of the column-packed chunk attention (algorithm: see llm_ops.hip above attn_cols_kernel), included
// textually by its four kernels: attn_cols_kernel, attn_cols_f8_kernel, attn_cols_seg_kernel, attn_cols_seg_f8_kernel.  (Why not a __device__
// function: profiles/attn_family_refactor.md.)
// The including kernel sets, and this file consumes (#undef at the end):
//   VLO_ATTN_F8        1: the pool holds e4m3 bytes (8-byte K / V^T pieces expanded to the bf16 fragments in registers), 0: bf16
// Every name read from the including kernel is listed and type-checked here, so a kernel that does not provide one fails to compile:
    static_assert(HD % 32 == 0 && NCT >= 1 && NCT <= 3, "template parameters HD, NCT");
    VLO_ATTN_NAME(q, const bf16_t *);            // the query rows [n][nh * HD]
    VLO_ATTN_NAME(kv, KvGeom);                   // the pool; kv.page_table = the session's
    VLO_ATTN_NAME(layer, int);  VLO_ATTN_NAME(nh, int);  VLO_ATTN_NAME(G, int);
    VLO_ATTN_NAME(pos0, int64_t);  VLO_ATTN_NAME(n, int);  VLO_ATTN_NAME(chunk, int);
    VLO_ATTN_NAME(scale, float);
    VLO_ATTN_NAME(part_o, float *);  VLO_ATTN_NAME(part_ml, float *);   // the launch's (segment's) first partial state
#if VLO_ATTN_F8
    VLO_ATTN_NAME(kv_scale, const float *);
    const float vscale = attn_f8_scales(kv_scale, layer, scale);   // `scale` now carries k_scale; vscale multiplies the partial output
#endif
    constexpr int NKK = HD / 32, NDT = HD / 16, KS = 8;
    extern __shared__ __attribute__((aligned(16))) float4 lds_o[];         // the block's one dynamic LDS array (shared name with attn_chunk_kernel)
    uint4 *qs = reinterpret_cast<uint4 *>(lds_o);                          // [NCT][NKK][64]   Q fragments (MFMA B operand)
    float4 *lds_po = lds_o + NCT * NKK * 64;                               // [4][NCT][NDT][64] partial O of the merge rounds
    float *lds_ml = reinterpret_cast<float *>(lds_po + 4 * NCT * NDT * 64); // [4][NCT][16][2]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int split = blockIdx.x, kvh = blockIdx.y;
    const int col = lane & 15, qd = lane >> 4;
    const int L = (int)(pos0 + n);
    const int c0 = split * chunk, c1 = min(L, c0 + chunk);

    for (int i = w; i < NCT * NKK; i += KS) {
        const int ct = i / NKK, kk = i - ct * NKK;
        const int cc = ct * 16 + col, qi = cc / G, h = cc - qi * G;
        uint4 z = make_uint4(0, 0, 0, 0);
        if (qi < n) z = *reinterpret_cast<const uint4 *>(q + (size_t)qi * nh * HD + (size_t)(kvh * G + h) * HD + kk * 32 + qd * 8);
        qs[i * 64 + lane] = z;
    }
    int qpos[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) qpos[ct] = (int)pos0 + min((ct * 16 + col) / G, n - 1);

    f32x4 O[NCT][NDT];
    float mrun[NCT], lrun[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        mrun[ct] = -INFINITY;
        lrun[ct] = 0.f;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) O[ct][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#if VLO_ATTN_F8
    typedef uint8_t kv_t;                                                   // one e4m3 byte per element, same element offsets
    typedef uint2 kraw_t;                                                   // 8 bytes = one fragment before expansion
#else
    typedef bf16_t kv_t;
    typedef frag_ab kraw_t;
#endif
    const kv_t *kbase = reinterpret_cast<const kv_t *>(kv.k_pool) + (size_t)layer * kv.layer_stride;
    const kv_t *vbase = reinterpret_cast<const kv_t *>(kv.vt_pool) + (size_t)layer * kv.layer_stride;
    const int krow = (col >> 2) * 8 + (col & 3);                           // S row `col` of tile t is key krow + 4 t of the block
    auto load_k = [&](int kt0, kraw_t (&dst)[2][NKK]) {
        const int page = kv.page_table[kt0 / VLO_PAGE_TOKENS];
        const kv_t *kp = kbase + (size_t)page * kv.page_elems + ((size_t)kvh * VLO_PAGE_TOKENS + kt0 % VLO_PAGE_TOKENS) * HD;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk)
                dst[t][kk] = *reinterpret_cast<const kraw_t *>(kp + (size_t)(krow + 4 * t) * HD + kk * 32 + qd * 8);
    };
    frag_ab kf[2][NKK];
    kraw_t kn[2][NKK];
    const int kfirst = c0 + w * 32;
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
    __syncthreads();                                                        // Q fragments staged
    for (int kt0 = kfirst; kt0 < c1; kt0 += KS * 32) {
        const int page = kv.page_table[kt0 / VLO_PAGE_TOKENS];
        const kv_t *vp = vbase + (size_t)page * kv.page_elems + ((size_t)kvh * HD) * VLO_PAGE_TOKENS + kt0 % VLO_PAGE_TOKENS;
        kraw_t vf[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) vf[dt] = *reinterpret_cast<const kraw_t *>(vp + (size_t)(dt * 16 + col) * VLO_PAGE_TOKENS + qd * 8);
        const bool more = kt0 + KS * 32 < c1;
        if (more) load_k(kt0 + KS * 32, kn);
        asm volatile("" ::: "memory");                                     // the Q fragments are re-read from LDS every block, never hoisted into registers
        const int kb = kt0 + qd * 8;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const frag_ab qf = __builtin_bit_cast(frag_ab, qs[(ct * NKK + kk) * 64 + lane]);
                s0 = mfma_bf16(kf[0][kk], qf, s0);
                s1 = mfma_bf16(kf[1][kk], qf, s1);
            }
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = (kb + r <= qpos[ct]) ? s0[r] * scale : -INFINITY;
                v[4 + r] = (kb + 4 + r <= qpos[ct]) ? s1[r] * scale : -INFINITY;
            }
            float tmax = v[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) tmax = fmaxf(tmax, v[j]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(mrun[ct], tmax);
            const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __expf(mrun[ct] - m_safe);
            mrun[ct] = m_new;
            float psum = 0.f;
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                p[j] = __expf(v[j] - m_safe);
                psum += p[j];
            }
            const uint4 pk = make_uint4(pack2bf(p[0], p[1]), pack2bf(p[2], p[3]), pack2bf(p[4], p[5]), pack2bf(p[6], p[7]));
            const frag_ab pb = __builtin_bit_cast(frag_ab, pk);
            lrun[ct] = lrun[ct] * alpha + psum;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                f32x4 o = O[ct][dt];
                o[0] *= alpha; o[1] *= alpha; o[2] *= alpha; o[3] *= alpha;
#if VLO_ATTN_F8
                uint2 vr = vf[dt];
                if constexpr (NCT * HD > 256) asm volatile("" : "+v"(vr));   // expanded per column tile, not hoisted: 3 x 128 would spill
                O[ct][dt] = mfma_bf16(fp8x8_to_bf16(vr), pb, o);
#else
                O[ct][dt] = mfma_bf16(vf[dt], pb, o);
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
    for (int ct = 0; ct < NCT; ++ct) {
        lrun[ct] += __shfl_xor(lrun[ct], 16, 64);
        lrun[ct] += __shfl_xor(lrun[ct], 32, 64);
    }
    // ---- pairwise merge of the 8 partial states: wave w + half hands its state to wave w
    for (int half = KS / 2; half >= 1; half >>= 1) {
        if (w >= half && w < 2 * half) {
            const int slot = w - half;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                if (qd == 0) {
                    lds_ml[((slot * NCT + ct) * 16 + col) * 2] = mrun[ct];
                    lds_ml[((slot * NCT + ct) * 16 + col) * 2 + 1] = lrun[ct];
                }
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const f32x4 o = O[ct][dt];
                    lds_po[((size_t)(slot * NCT + ct) * NDT + dt) * 64 + lane] = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
        }
        __syncthreads();
        if (w < half) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const float mo = lds_ml[((w * NCT + ct) * 16 + col) * 2], lo = lds_ml[((w * NCT + ct) * 16 + col) * 2 + 1];
                const float M = fmaxf(mrun[ct], mo);
                const float Ms = (M == -INFINITY) ? 0.f : M;
                const float wa = __expf(mrun[ct] - Ms), wb = __expf(mo - Ms);          // -inf -> 0
                lrun[ct] = lrun[ct] * wa + lo * wb;
                mrun[ct] = M;
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const float4 o = lds_po[((size_t)(w * NCT + ct) * NDT + dt) * 64 + lane];
                    O[ct][dt][0] = O[ct][dt][0] * wa + o.x * wb;
                    O[ct][dt][1] = O[ct][dt][1] * wa + o.y * wb;
                    O[ct][dt][2] = O[ct][dt][2] * wa + o.z * wb;
                    O[ct][dt][3] = O[ct][dt][3] * wa + o.w * wb;
                }
            }
        }
        __syncthreads();
    }
    if (w != 0) return;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int cc = ct * 16 + col, qi = cc / G, h = cc - qi * G;
        if (qi >= n) continue;
        const size_t row = ((size_t)split * nh + kvh * G + h) * 16 + qi;
        if (qd == 0) {
            part_ml[row * 2] = mrun[ct];
            part_ml[row * 2 + 1] = lrun[ct];
        }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
#if VLO_ATTN_F8
            const f32x4 o = O[ct][dt] * vscale;                              // sum_j p_j v_code_j v_scale
#else
            const f32x4 o = O[ct][dt];
#endif
            *reinterpret_cast<float4 *>(part_o + row * HD + dt * 16 + qd * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
#undef VLO_ATTN_F8
