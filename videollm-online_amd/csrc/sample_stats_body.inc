// sample_stats_body.inc — per-block max / sum of exp / argmax over a slice of one row of bf16 logits (see llm_ops.hip), included TEXTUALLY by
// sample_stats_kernel and sample_stats_rows_kernel.  Expects in scope: logits, V, scr (the row's), sm, smv, smi (LDS).
    const int per = (V + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = min(V, lo + per);
    float mx = -INFINITY;
    ArgBest b = {-INFINITY, 0x7fffffff};
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const float v = bf2f(logits[i]);
        mx = fmaxf(mx, v);
        if (v > b.v) { b.v = v; b.i = i; }
    }
    mx = block_max(mx, sm);
    float s = 0.f;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) s += expf(bf2f(logits[i]) - mx);
    s = block_sum(s, sm);
    b = block_argbest(b, smv, smi);
    if (threadIdx.x == 0) {
        const int NB = gridDim.x;
        scr[blockIdx.x] = mx;
        scr[NB + blockIdx.x] = (mx == -INFINITY) ? 0.f : s;
        scr[2 * NB + blockIdx.x] = b.v;
        reinterpret_cast<int *>(scr)[3 * NB + blockIdx.x] = b.i;
    }
