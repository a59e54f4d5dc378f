// stream_scan_body.inc — the bf16 softmax, interval threshold and per-block argmax of one row (see llm_ops.hip), included TEXTUALLY by
// stream_scan_kernel and stream_scan_rows_kernel.  Expects in scope: logits, V, threshold, interval_id, scr (the row's), smv, smi (LDS).
    const int NB = gridDim.x;
    float M = -INFINITY;
    for (int k = 0; k < NB; ++k) M = fmaxf(M, scr[k]);
    float S = 0.f;
    for (int k = 0; k < NB; ++k) S += scr[NB + k] * expf(scr[k] - M);
    const float p_int = rbf(expf(bf2f(logits[interval_id]) - M) / S);
    const bool zero_int = p_int < rbf(threshold);   // torch compares a bf16 tensor with a Python float in bf16
    const int per = (V + NB - 1) / NB, lo = blockIdx.x * per, hi = min(V, lo + per);
    ArgBest b = {-INFINITY, 0x7fffffff};
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        float p = rbf(expf(bf2f(logits[i]) - M) / S);
        if (i == interval_id && zero_int) p = 0.f;
        if (p > b.v) { b.v = p; b.i = i; }
    }
    b = block_argbest(b, smv, smi);
    if (threadIdx.x == 0) {
        scr[4 * NB + blockIdx.x] = b.v;
        reinterpret_cast<int *>(scr)[5 * NB + blockIdx.x] = b.i;
        if (blockIdx.x == 0) scr[6 * NB] = p_int;
    }
