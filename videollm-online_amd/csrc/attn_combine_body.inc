// attn_combine_body.inc — the merge of one (head, query row)'s split partials (see llm_ops.hip), included TEXTUALLY by attn_combine_kernel and
// attn_combine_seg_kernel.  Expects in scope: template parameter HD; CL, SL, NJ; `red` (LDS, SL * CL float4); head, t, lane, qrow;
// part_o, part_ml, nsplit, nh (already offset to the sub-chunk / segment), out, pack_row0 (< 0: row-major out).
    const int c4 = t % CL, sl = t / CL;
    float4 o[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int sp = sl + j * SL;
        o[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sp < nsplit) o[j] = *reinterpret_cast<const float4 *>(part_o + (((size_t)sp * nh + head) * 16 + qrow) * HD + c4 * 4);
    }
    float ms = -INFINITY, ls = 0.f;
    if (lane < nsplit) {
        const float2 ml = *reinterpret_cast<const float2 *>(part_ml + (((size_t)lane * nh + head) * 16 + qrow) * 2);
        ms = ml.x;
        ls = ml.y;
    }
    const float M = wave_max(ms);
    const float wv = (ms == -INFINITY) ? 0.f : __expf(ms - M);       // 0 for lanes >= nsplit and for empty splits
    const float Ltot = wave_sum(ls * wv);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float wj = __shfl(wv, sl + j * SL, 64);
        acc.x += o[j].x * wj; acc.y += o[j].y * wj; acc.z += o[j].z * wj; acc.w += o[j].w * wj;
    }
    red[sl * CL + c4] = acc;
    __syncthreads();
    if (t < CL) {
        float4 r = red[t];
#pragma unroll
        for (int k2 = 1; k2 < SL; ++k2) {
            const float4 v = red[k2 * CL + t];
            r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
        }
        const int d = t * 4;
        const size_t at = pack_row0 < 0 ? (size_t)qrow * nh * HD + (size_t)head * HD + d : vlo_pack64_elem(pack_row0 + qrow, head * HD + d);
        ushort4 ov;
        ov.x = f2bf(r.x / Ltot); ov.y = f2bf(r.y / Ltot); ov.z = f2bf(r.z / Ltot); ov.w = f2bf(r.w / Ltot);
        *reinterpret_cast<ushort4 *>(out + at) = ov;
    }
