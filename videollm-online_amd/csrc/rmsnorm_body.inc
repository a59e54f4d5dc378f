// rmsnorm_body.inc — body of add_rmsnorm_kernel and add_rmsnorm_gather_kernel (llm_ops.hip), included textually by the kernel.
// VLO_RMS_ROW = the row of h / partial the block normalises, VLO_RMS_XROW = the row of x it writes (both blockIdx.x in add_rmsnorm_kernel).
// Expects the kernel's parameters by name in scope.
    __shared__ float sm[16];
    const int m = VLO_RMS_ROW;
    bf16_t *hr = h + (size_t)m * H;
    float v[RMS_MAXCH][8];
    float ss = 0.f;
    const int nch = H >> 3;
#pragma unroll
    for (int c = 0; c < RMS_MAXCH; ++c) {
        const int ch = threadIdx.x + c * RMS_THREADS;
        if (ch < nch) {
            const uint4 raw = *reinterpret_cast<const uint4 *>(hr + ch * 8);
            const bf16_t *e = reinterpret_cast<const bf16_t *>(&raw);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c][j] = bf2f(e[j]);
            if (partial) {
                float d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int s = 0; s < ksplit; ++s) {
                    const float4 *pp = reinterpret_cast<const float4 *>(partial + ((size_t)s * 16 + m) * partial_ld + ch * 8);
                    const float4 a = pp[0], b = pp[1];
                    d[0] += a.x; d[1] += a.y; d[2] += a.z; d[3] += a.w;
                    d[4] += b.x; d[5] += b.y; d[6] += b.z; d[7] += b.w;
                }
                uint4 o;
                bf16_t *oe = reinterpret_cast<bf16_t *>(&o);
#pragma unroll
                for (int j = 0; j < 8; ++j) {          // linear output -> bf16, then bf16 residual add
                    v[c][j] = rbf(v[c][j] + rbf(d[j]));
                    oe[j] = f2bf(v[c][j]);
                }
                *reinterpret_cast<uint4 *>(hr + ch * 8) = o;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += v[c][j] * v[c][j];
        }
    }
    // norm weights are fetched BEFORE the block-wide reduction so their latency hides behind its two barriers
    uint4 wraw[RMS_MAXCH];
#pragma unroll
    for (int c = 0; c < RMS_MAXCH; ++c) {
        const int ch = threadIdx.x + c * RMS_THREADS;
        wraw[c] = (ch < nch) ? *reinterpret_cast<const uint4 *>(w + ch * 8) : make_uint4(0, 0, 0, 0);
    }
    ss = block_sum(ss, sm);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);
    const int mx = VLO_RMS_XROW;
    bf16_t *xr = x + (size_t)mx * ldx;
#pragma unroll
    for (int c = 0; c < RMS_MAXCH; ++c) {
        const int ch = threadIdx.x + c * RMS_THREADS;
        if (ch < nch) {
            const bf16_t *we = reinterpret_cast<const bf16_t *>(&wraw[c]);
            uint4 o;
            bf16_t *oe = reinterpret_cast<bf16_t *>(&o);
#pragma unroll
            for (int j = 0; j < 8; ++j) oe[j] = f2bf(bf2f(we[j]) * rbf(v[c][j] * rs));   // weight * x.to(bf16)
            bf16_t *dst = ldx ? xr + ch * 8 : x + vlo_pack64_elem(mx, ch * 8);            // ldx == 0: packed-64 (block path)
            *reinterpret_cast<uint4 *>(dst) = o;
        }
    }
