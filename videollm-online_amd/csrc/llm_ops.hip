// llm_ops.hip — the non-GEMV kernels of one Llama streaming step on gfx950.
//
//                           (RMSNorm, residual adds, RoPE and the KV append are fused into gemv.hip)
//   attn_chunk_kernel       n<=16 queries x growing KV, GQA, bottom-right causal mask fused,
//                           split-KV with online softmax (replaces mask build + repeat_kv + SDPA,
//                           HF:integrations/sdpa_attention.py:79-166, HF:masking_utils.py)
//   attn_combine_kernel     merge the split partials
//   embed_gather_kernel     model.get_input_embeddings() (demo/inference.py:46,66)
//   greedy / stream sample  models/modeling_live.py:177 ; demo/inference.py:76-79
//
// Rounding points mirror the reference's bf16 CPU/sdpa path (activations are bf16
// between ops, accumulation is fp32), see DESIGN.md "Numerics".
#include <stdlib.h>

#include "common.cuh"
#include "glds_asm.cuh"
#include "llm_ops.h"

// ------------------------------------------------------------------------------------
// residual add + RMSNorm.  One block per token row.
// ------------------------------------------------------------------------------------
#define RMS_THREADS 512
#define RMS_MAXCH 2   // supports H <= 8 * 512 * 2 = 8192

__global__ __launch_bounds__(RMS_THREADS) void add_rmsnorm_kernel(bf16_t *__restrict__ h, const float *__restrict__ partial,
                                                                  int ksplit, int partial_ld, const bf16_t *__restrict__ w,
                                                                  bf16_t *__restrict__ x, int H, int ldx, float eps) {
#define VLO_RMS_ROW blockIdx.x
#define VLO_RMS_XROW blockIdx.x
#include "rmsnorm_body.inc"
#undef VLO_RMS_ROW
#undef VLO_RMS_XROW
}

// the same for `count` SELECTED rows (stream lookahead: the last row of each unit of a pass): block k normalises row rows.v[k] of h and writes
// row k of the row-major x16.  The same body, so a selected row equals what add_rmsnorm_kernel writes for it bit for bit; the other rows of h
// are neither normalised nor given their pending partial sums.
__global__ __launch_bounds__(RMS_THREADS) void add_rmsnorm_gather_kernel(bf16_t *__restrict__ h, const float *__restrict__ partial,
                                                                         int ksplit, int partial_ld, const bf16_t *__restrict__ w,
                                                                         bf16_t *__restrict__ x, int H, int ldx, float eps, RowIdx rows) {
#define VLO_RMS_ROW rows.v[blockIdx.x]
#define VLO_RMS_XROW blockIdx.x
#include "rmsnorm_body.inc"
#undef VLO_RMS_ROW
#undef VLO_RMS_XROW
}

hipError_t add_rmsnorm_launch(unsigned short *h, const float *partial, int ksplit, int partial_ld, const unsigned short *w,
                              unsigned short *x, int H, int ldx, float eps, int n, hipStream_t st) {
    if (H > 8 * RMS_THREADS * RMS_MAXCH || (H & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(add_rmsnorm_kernel, dim3(n), dim3(RMS_THREADS), 0, st, h, partial, ksplit, partial_ld, w, x, H, ldx, eps);
    return hipGetLastError();
}
hipError_t add_rmsnorm_gather_launch(unsigned short *h, const float *partial, int ksplit, int partial_ld, const unsigned short *w,
                                     unsigned short *x16, int H, float eps, const RowIdx &rows, int count, int n_rows, hipStream_t st) {
    if (H > 8 * RMS_THREADS * RMS_MAXCH || (H & 7) || count < 1 || count > VLO_ROWIDX_MAX) return hipErrorInvalidValue;
    for (int k = 0; k < count; ++k)
        if (rows.v[k] < 0 || rows.v[k] >= n_rows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(add_rmsnorm_gather_kernel, dim3(count), dim3(RMS_THREADS), 0, st, h, partial, ksplit, partial_ld, w, x16, H, H, eps, rows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// What the live-step attention kernels share.  Two bodies (attn_body.inc, attn_cols_body.inc), each stamped into four kernels: solo / segmented
// launch x bf16 / fp8 pool.  The bodies check the names they read from their kernel with these:
// ------------------------------------------------------------------------------------
template <class T> struct attn_plain { typedef T type; };                        // the type without __restrict__ (kernel parameters carry it)
template <class T> struct attn_plain<T *__restrict__> { typedef T *type; };
#define VLO_ATTN_NAME(x, ...) static_assert(std::is_same<typename attn_plain<std::remove_cv_t<decltype(x)>>::type, __VA_ARGS__>::value, \
                                            "attention body: `" #x "` must be a " #__VA_ARGS__ " of the including kernel")
// fp8 pool (kv_scale = the pool's [layer][2] {k_scale, v_scale}): folds k_scale into the score scale — (q . k_code) k_scale / sqrt(d) — and
// returns v_scale, which multiplies the partial output
VLO_DEV float attn_f8_scales(const float *__restrict__ kv_scale, int layer, float &scale) {
    scale *= kv_scale[2 * layer];
    return kv_scale[2 * layer + 1];
}

// ------------------------------------------------------------------------------------
// chunk attention.  grid = (nsplit, nkv); block = NHG x KS waves:
//   NHG = G / HPW head groups (wave hg owns q heads kvh*G + hg*HPW .. +HPW),
//   KS  = in-block key sub-splits (wave ks walks every KS-th 32-key block of the block's chunk),
// so a CU holds 8 waves streaming different K/V pages while only one partial per (split, head)
// leaves the block: the KS partial (m, l, O) states are merged through LDS (flash-decoding inside
// the block), the block's result goes to the split-KV partial buffers, attn_combine_kernel merges
// the splits.  Per 32 keys:
//   S^T[key][qrow] = K[key][:] . Q[qrow][:]          (K page rows = MFMA A operand, from HBM)
//   online softmax per (head, qrow = lane&15); P^T stays in the lanes that produced it
//   O^T[d][qrow]  += V^T[d][key] . P^T[key][qrow]    (V^T page rows = MFMA A operand)
// ------------------------------------------------------------------------------------
template <int HD, int HPW>
__global__ __launch_bounds__(512) void attn_chunk_kernel(const bf16_t *__restrict__ q, KvGeom kv, int layer, int nh, int G, int KS,
                                                         int64_t pos0, int n, int chunk, float scale,
                                                         float *__restrict__ part_o, float *__restrict__ part_ml) {
#define VLO_ATTN_F8 0
#define VLO_ATTN_SUBCHUNK blockIdx.z
#include "attn_body.inc"
}
// the same over an fp8 e4m3 pool (vlo_config.kv_dtype = 1): kv_scale = the pool's [layer][2] {k_scale, v_scale}
template <int HD, int HPW>
__global__ __launch_bounds__(512) void attn_chunk_f8_kernel(const bf16_t *__restrict__ q, KvGeom kv, int layer, int nh, int G, int KS,
                                                            int64_t pos0, int n, int chunk, float scale,
                                                            float *__restrict__ part_o, float *__restrict__ part_ml, const float *__restrict__ kv_scale) {
#define VLO_ATTN_F8 1
#define VLO_ATTN_SUBCHUNK blockIdx.z
#include "attn_body.inc"
}

// ------------------------------------------------------------------------------------
// column-packed chunk attention (short steps: G * n <= 16 * NCT columns).  The G query heads that share one kv head TIMES the n new
// tokens are the COLUMNS of the MFMA tiles (column c = token c / G, head c % G), so one wave serves the whole GQA group and the 8
// waves of a block all walk DIFFERENT 32-key blocks: every K / V^T byte is fetched by exactly one wave of the chip (in
// attn_chunk_kernel the head-group waves of a block fetch the same pages twice, which halves the bytes in flight per CU).
//   * keys are permuted inside a 32-key block so that the lane holding S rows qd*4..+4 of both 16-key tiles owns the 8 CONSECUTIVE
//     keys qd*8..+8: P^T is a B operand as produced and a V^T fragment is one 16-byte load (two 8-byte loads in attn_chunk_kernel);
//   * Q fragments live in LDS (shared by the 8 waves), not in registers: the accumulators of 3 column tiles are 96 registers;
//   * the 8 partial states merge pairwise through LDS in three halving rounds; wave 0 writes the block's partial for the valid columns only.
// ------------------------------------------------------------------------------------
template <int HD, int NCT>
__global__ __launch_bounds__(512) void attn_cols_kernel(const bf16_t *__restrict__ q, KvGeom kv, int layer, int nh, int G, int64_t pos0, int n,
                                                        int chunk, float scale, float *__restrict__ part_o, float *__restrict__ part_ml) {
#define VLO_ATTN_F8 0
#include "attn_cols_body.inc"
}
// the same over an fp8 e4m3 pool (vlo_config.kv_dtype = 1): kv_scale = the pool's [layer][2] {k_scale, v_scale}
template <int HD, int NCT>
__global__ __launch_bounds__(512) void attn_cols_f8_kernel(const bf16_t *__restrict__ q, KvGeom kv, int layer, int nh, int G, int64_t pos0, int n,
                                                           int chunk, float scale, float *__restrict__ part_o, float *__restrict__ part_ml,
                                                           const float *__restrict__ kv_scale) {
#define VLO_ATTN_F8 1
#include "attn_cols_body.inc"
}

// Merge of the split-KV partials.  grid = (nh, n); block = 256 threads = SL split-lanes x CL column-lanes of 4 columns (HD = 128:
// 8 x 32).  ONE memory round trip: every thread issues its float4 partial loads (<= 64 / SL of them, all independent) and the wave's
// (m, l) loads together — the split weights do not gate the partial loads — each wave works the softmax weights of the splits out
// for itself (lane s = split s: wave_max / wave_sum, no LDS), a thread picks the weights of its splits with a lane read, and one
// LDS exchange adds the SL split-lanes.  (Round 3's kernel walked the splits with two split-lanes of 4-byte loads behind a
// shared-memory weight phase: 5.9 us per layer at 32 splits, 4.8 % of the stream's GPU time, for 16 KB per block.)
template <int HD>
__global__ __launch_bounds__(256) void attn_combine_kernel(const float *__restrict__ part_o, const float *__restrict__ part_ml,
                                                           int nsplit, int nh, bf16_t *__restrict__ out, int pack_row0) {
    constexpr int CL = HD / 4, SL = 256 / CL, NJ = VLO_MAX_SPLITS / SL;
    static_assert(VLO_MAX_SPLITS == 64, "lane s of a wave holds split s");
    __shared__ float4 red[SL * CL];
    const int head = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int qrow = blockIdx.y;
    {                                              // blockIdx.y walks all query rows, 16 per sub-chunk (z = 0 on the live path)
        const int z = qrow >> 4;
        part_o += (size_t)z * nsplit * nh * 16 * HD;
        part_ml += (size_t)z * nsplit * nh * 16 * 2;
        if (pack_row0 >= 0) pack_row0 += z * 16;
        else out += (size_t)z * 16 * nh * HD;
        qrow &= 15;
    }
#include "attn_combine_body.inc"
}
// max over lanes l, l ^ 16, l ^ 32, l ^ 48 (the four lanes that hold one score column of a 16 x 16 MFMA tile) by two row swaps
VLO_DEV float quad_lanes_maxf(float x) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    const float m = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// ------------------------------------------------------------------------------------
// Prefill attention (blocks of hundreds to thousands of new tokens, engine.hip::run_prefill): flash-style.  One workgroup = one kv head x
// QB = 128 / G consecutive queries: its 128 (query, head) columns are 8 column tiles, one per wave (8 waves), and ALL waves walk the SAME
// 32-key tiles, which are staged once per workgroup in LDS (K 32 x HD, V^T HD x 32: 16 KiB at HD = 128, double-buffered) by direct-to-LDS
// loads — a K / V^T byte leaves L2 once per 128 columns instead of once per 16-query sub-chunk (the decode-shaped kernel above re-reads
// the whole prefix for every sub-chunk: 232 TFLOP/s at 13 k tokens).  No split-KV, no merge kernel: a workgroup sees every key its
// queries may attend to and writes normalised bf16 rows.
//   * LDS layout = the MFMA A-operand fragments themselves: piece (1 KiB) = [16-byte chunk c][row r] so lane l = 16 c + r reads slot l
//     (conflict-free ds_read_b128); the direct-to-LDS destination is lane-linear, so the gather happens on the per-lane SOURCE address;
//   * keys are permuted inside a 32-key tile as in attn_cols_kernel (row r of key tile t = key (r >> 2) * 8 + (r & 3) + 4 t): the lane
//     that holds S rows 4 qd .. 4 qd + 3 of both tiles owns 8 CONSECUTIVE keys, P^T is a B operand as produced and a V^T fragment is one chunk;
//   * the loads are issued in inline asm (invisible to hipcc, which would drain them before every LDS read) into a ring of NS tile buffers and
//     retired by ONE COUNTED s_waitcnt vmcnt + a raw s_barrier per tile: NS - 1 tiles are in flight while one is multiplied (one 16-KiB tile per CU
//     in flight — NS = 2 — leaves the kernel waiting for L2 latency: a tile's MFMAs take ~0.5 us, its round trip ~2).
//   * two wave-uniform shortcuts drop work whose result is known, BIT-IDENTICALLY: a tile every key of which is visible to every query of the
//     wave skips the causal select; a tile that raised no lane's running maximum skips the rescale of the 32 accumulator registers (alpha == 1
//     exactly).  `noskip` (VLO_ATTN_NOSKIP=1, tests) takes the long way everywhere.  Measured: ~40 % fewer VALU instructions per tile and NO
//     change in time (13 312 tokens: 255.3 vs 255.8 ms) — VALU throughput is not what bounds this kernel.
// grid = (ceil(n / QB), nkv); 512 threads.  Rounding points as the other attention kernels (P -> bf16 before P.V, bf16 output).
// ------------------------------------------------------------------------------------
// ONE column tile per wave: 128 (query, head) columns per workgroup, a register budget of 128 — four waves per SIMD.  (Round 4 shipped two column tiles
// per wave, 256 columns per workgroup at 208 - 214 VGPRs / two waves per SIMD: half the LDS read traffic per FLOP, but a per-wave latency chain that two
// waves per SIMD cannot hide.  Measured on the MI355X, bit-identical outputs: 13 312 tokens 242.2 -> 232.4 ms, 2 048 tokens 33.7 -> 33.9 ms;
// profiles/r5_prefill_attention_one_column_tile.txt.  The two-tile kernel is gone.)
template <int HD, int G, int NS>
__global__ __launch_bounds__(512, 4) void attn_prefill_kernel(const bf16_t *__restrict__ q, KvGeom kv, int layer, int nh, int64_t pos0, int n, float scale_l2e,
                                                              bf16_t *__restrict__ out, int noskip, int nkv, int nqb) {
#define VLO_PF_NCT 1
#include "attn_prefill_body.inc"
#undef VLO_PF_NCT
}

// The same tiles as a two-group ping-pong with batched fragment reads (attn_prefill_pp_body.inc) — the kernel that ships; the lock-step kernel
// above stays as the reference the variants test compares it with, bit for bit (VLO_ATTN_PF=0).
template <int HD, int G, int NS>
__global__ __launch_bounds__(512, 4) void attn_prefill_pp_kernel(const bf16_t *__restrict__ q, KvGeom kv, int layer, int nh, int64_t pos0, int n, float scale_l2e,
                                                                 bf16_t *__restrict__ out, int noskip, int nkv, int nqb) {
#define VLO_PF_NCT 1
#include "attn_prefill_pp_body.inc"
#undef VLO_PF_NCT
}
// the (head dim, GQA group) pairs attn_prefill_kernel is instantiated for — attention_prefill_launch returns hipErrorNotSupported for any other; a caller
// WITHOUT a fallback (tp.hip::tp_prefill) asks first and keeps the 16-row step instead
bool attention_prefill_supported(int head_dim, int gqa_group, int kv_dtype) {
    if (kv_dtype != VLO_KV_BF16) return false;
    return (head_dim == 128 && (gqa_group == 1 || gqa_group == 2 || gqa_group == 4 || gqa_group == 8)) ||
           (head_dim == 64 && (gqa_group == 2 || gqa_group == 4 || gqa_group == 8));
}

hipError_t attention_prefill_launch(const unsigned short *q, const KvPool &kv, int layer, int num_heads, int64_t pos0, int n, unsigned short *out, hipStream_t st) {
    if (kv.dtype != VLO_KV_BF16) return hipErrorNotSupported;             // the flash kernels read bf16 pages: the caller takes attention_launch
    const int nkv = kv.num_kv_heads, hd = kv.head_dim, G = num_heads / nkv;
    if (n <= 0 || nkv * G != num_heads) return hipErrorInvalidValue;
    const float scale = (1.0f / sqrtf((float)hd)) * 1.4426950408889634f;   // log2(e) / sqrt(hd): the kernels' softmax runs on exp2 (attn_prefill_pp_body.inc)
    const char *ns = getenv("VLO_ATTN_NOSKIP");                            // read per call: the tests flip it between two passes over the same input
    const int noskip = ns && atoi(ns) != 0;
    const char *pv = getenv("VLO_ATTN_PF");                                // tests: 0 = the lock-step reference kernel
    const int variant = pv ? atoi(pv) : 1;
#define VLO_ATTN_PF(HD_, G_)                                                                                                          \
    do {                                                                                                                              \
        constexpr int QB_ = 128 / G_;                                                                                                 \
        const int nqb = (n + QB_ - 1) / QB_;                                                                                          \
        const dim3 grid((unsigned)((nqb * nkv + 7) & ~7));               /* 1-D: the kernel maps workgroups to (kv head, query block) per XCD */ \
        if (variant != 0)                                                                                                             \
            hipLaunchKernelGGL((attn_prefill_pp_kernel<HD_, G_, 4>), grid, dim3(512), 0, st, q, kv, layer, num_heads, pos0, n, scale, out, noskip, nkv, nqb); \
        else                                                                                                                          \
            hipLaunchKernelGGL((attn_prefill_kernel<HD_, G_, 4>), grid, dim3(512), 0, st, q, kv, layer, num_heads, pos0, n, scale, out, noskip, nkv, nqb); \
        return hipGetLastError();                                                                                                     \
    } while (0)
    if (hd == 128 && G == 4) VLO_ATTN_PF(128, 4);
    if (hd == 128 && G == 8) VLO_ATTN_PF(128, 8);
    if (hd == 128 && G == 2) VLO_ATTN_PF(128, 2);
    if (hd == 128 && G == 1) VLO_ATTN_PF(128, 1);
    if (hd == 64 && G == 8) VLO_ATTN_PF(64, 8);
    if (hd == 64 && G == 4) VLO_ATTN_PF(64, 4);
    if (hd == 64 && G == 2) VLO_ATTN_PF(64, 2);
#undef VLO_ATTN_PF
    return hipErrorNotSupported;                 // the caller falls back to attention_launch
}

static constexpr int kAttnWantBlocks = 256;            // split target of attention_geometry: ~one block per CU (128 / 512 measured slower)
static constexpr int kBlockSubchunks = 4;          // 16-query sub-chunks of a block-path step (64 rows)
hipError_t attention_geometry(const KvGeom &kv, int num_heads, int64_t pos0, int n, AttnGeom *g, int part_cap) {
    const int nkv = kv.num_kv_heads, hd = kv.head_dim, G = num_heads / nkv;
    const int L = (int)(pos0 + n);
    const int hpw = (G % 2 == 0) ? 2 : 1;
    const int nhg = G / hpw;
    if (nhg > 8) return hipErrorInvalidValue;
    int KS = 8 / nhg;                                   // 8 waves per block
    if (KS > 4) KS = 4;
    // n > 16 (block path): grid.z sub-chunks of 16 queries share one launch and one split geometry; sub-chunk z sees the
    // keys [0, pos0 + 16 z + n_z), splits beyond that write empty partials
    const int nz = (n + 15) / 16;
    if (nz > part_cap || nz > 65535) return hipErrorInvalidValue;
    // short steps whose G * n (head, token) columns fit 3 MFMA column tiles take the column-packed kernel: 8 key sub-splits per block
    g->nct = 0;
    if (nz == 1 && G * n <= 48 && (hd == 128 || hd == 64)) {
        g->nct = (G * n + 15) / 16;
        KS = 8;
    }
    // splits: ~one block per CU at long context; every wave should see at least one 32-key block
    int target = (L + KS * 32 - 1) / (KS * 32);
    const int want = (kAttnWantBlocks + nkv * nz - 1) / (nkv * nz);
    if (target > want) target = want;
    if (target > VLO_MAX_SPLITS / nz) target = VLO_MAX_SPLITS / nz;      // (the merge kernel holds one split per lane; 0 for nz > 64: one split below)
    if (target > part_cap / nz) target = part_cap / nz;
    if (nz > 4) target = 1;          // prefill blocks: the sub-chunks alone fill the chip, and one split keeps a row's result independent of the block's length
    if (target < 1) target = 1;
    int chunk = (L + target - 1) / target;
    chunk = (chunk + 31) & ~31;
    g->G = G; g->KS = KS; g->hpw = hpw; g->nhg = nhg; g->nz = nz; g->chunk = chunk;
    g->nsplit = (L + chunk - 1) / chunk;
    g->scale = 1.0f / sqrtf((float)hd);
    g->lds_bytes = (size_t)(KS - 1) * nhg * hpw * ((size_t)(hd / 16) * 64 * 16 + 16 * 2 * 4);
    if (g->nct) g->lds_bytes = (size_t)g->nct * ((size_t)(hd / 32) * 64 * 16 + 4 * ((size_t)(hd / 16) * 64 * 16 + 16 * 2 * 4));
    return hipSuccess;
}

// ------------------------------------------------------------------------------------
// Segmented attention (batched steps, engine.hip vlo_batch_step): blockIdx.z = one segment of the device table (llm_ops.h AttnSeg), i.e.
// one 16-query sub-chunk of one session with its own page table, position, query count, first row and split geometry — the geometry the
// session's solo launch would use, so each segment walks exactly the keys, splits and merges of that launch.  grid.x = the widest segment's
// split count; the blocks past a segment's last split leave at once (a uniform exit: no barrier has been reached).  The bodies are the solo
// kernels' .inc files; the names they read as kernel parameters of a solo launch come from the segment (attn_seg_args).
// ------------------------------------------------------------------------------------
// what a solo kernel gets as parameters, for one segment.  A kernel reads its segment and leaves first — `if (blockIdx.x >= sg.nsplit) return` —
// and takes this view afterwards (computed ahead of the exit it changes the kernels' scalar code: profiles/attn_family_refactor.md)
struct AttnSegArgs { const bf16_t *q; int64_t pos0; int n, chunk; float *part_o, *part_ml; };
template <int HD>
VLO_DEV AttnSegArgs attn_seg_args(const AttnSeg &sg, const bf16_t *q_rows, int nh, float *part_o_all, float *part_ml_all) {
    return {q_rows + (size_t)sg.row0 * nh * HD, sg.pos0, sg.n, sg.chunk, part_o_all + (size_t)sg.part0 * nh * 16 * HD,
            part_ml_all + (size_t)sg.part0 * nh * 16 * 2};
}

template <int HD, int HPW>
__global__ __launch_bounds__(512) void attn_chunk_seg_kernel(const bf16_t *__restrict__ q_rows, KvGeom kv, int layer, int nh, int G, int KS,
                                                             const AttnSeg *__restrict__ segs, float scale, float *__restrict__ part_o_all,
                                                             float *__restrict__ part_ml_all) {
    const AttnSeg sg = segs[blockIdx.z];
    if ((int)blockIdx.x >= sg.nsplit) return;
    kv.page_table = sg.page_table;
    auto [q, pos0, n, chunk, part_o, part_ml] = attn_seg_args<HD>(sg, q_rows, nh, part_o_all, part_ml_all);
#define VLO_ATTN_F8 0
#define VLO_ATTN_SUBCHUNK 0
#include "attn_body.inc"
}
template <int HD, int HPW>
__global__ __launch_bounds__(512) void attn_chunk_seg_f8_kernel(const bf16_t *__restrict__ q_rows, KvGeom kv, int layer, int nh, int G, int KS,
                                                                const AttnSeg *__restrict__ segs, float scale, float *__restrict__ part_o_all,
                                                                float *__restrict__ part_ml_all, const float *__restrict__ kv_scale) {
    const AttnSeg sg = segs[blockIdx.z];
    if ((int)blockIdx.x >= sg.nsplit) return;
    kv.page_table = sg.page_table;
    auto [q, pos0, n, chunk, part_o, part_ml] = attn_seg_args<HD>(sg, q_rows, nh, part_o_all, part_ml_all);
#define VLO_ATTN_F8 1
#define VLO_ATTN_SUBCHUNK 0
#include "attn_body.inc"
}
template <int HD, int NCT>
__global__ __launch_bounds__(512) void attn_cols_seg_kernel(const bf16_t *__restrict__ q_rows, KvGeom kv, int layer, int nh, int G,
                                                            const AttnSeg *__restrict__ segs, float scale, float *__restrict__ part_o_all,
                                                            float *__restrict__ part_ml_all) {
    const AttnSeg sg = segs[blockIdx.z];
    if ((int)blockIdx.x >= sg.nsplit) return;
    kv.page_table = sg.page_table;
    auto [q, pos0, n, chunk, part_o, part_ml] = attn_seg_args<HD>(sg, q_rows, nh, part_o_all, part_ml_all);
#define VLO_ATTN_F8 0
#include "attn_cols_body.inc"
}
template <int HD, int NCT>
__global__ __launch_bounds__(512) void attn_cols_seg_f8_kernel(const bf16_t *__restrict__ q_rows, KvGeom kv, int layer, int nh, int G,
                                                               const AttnSeg *__restrict__ segs, float scale, float *__restrict__ part_o_all,
                                                               float *__restrict__ part_ml_all, const float *__restrict__ kv_scale) {
    const AttnSeg sg = segs[blockIdx.z];
    if ((int)blockIdx.x >= sg.nsplit) return;
    kv.page_table = sg.page_table;
    auto [q, pos0, n, chunk, part_o, part_ml] = attn_seg_args<HD>(sg, q_rows, nh, part_o_all, part_ml_all);
#define VLO_ATTN_F8 1
#include "attn_cols_body.inc"
}

// merge of the split partials of every segment: grid = (nh, 16, segments); query row r of segment s goes to row s.row0 + r
template <int HD>
__global__ __launch_bounds__(256) void attn_combine_seg_kernel(const float *__restrict__ part_o, const float *__restrict__ part_ml,
                                                               const AttnSeg *__restrict__ segs, int nh, bf16_t *__restrict__ out, int packed) {
    constexpr int CL = HD / 4, SL = 256 / CL, NJ = VLO_MAX_SPLITS / SL;
    __shared__ float4 red[SL * CL];
    const int head = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const AttnSeg sg = segs[blockIdx.z];
    const int qrow = blockIdx.y, nsplit = sg.nsplit;
    if (qrow >= sg.n) return;
    part_o += (size_t)sg.part0 * nh * 16 * HD;          // (not through attn_seg_args: the compiler orders this kernel's scalar code differently then)
    part_ml += (size_t)sg.part0 * nh * 16 * 2;
    const int pack_row0 = packed ? sg.row0 : -1;
    if (!packed) out += (size_t)sg.row0 * nh * HD;
#include "attn_combine_body.inc"
}

int attention_states_bound(int num_kv_heads) {
    // attention_geometry: nsplit <= ceil(kAttnWantBlocks / (nkv * nz)) for nz sub-chunks, and nz * nsplit <= VLO_MAX_SPLITS
    const int b = (kAttnWantBlocks + num_kv_heads - 1) / num_kv_heads + kBlockSubchunks;
    return b < VLO_MAX_SPLITS ? b : VLO_MAX_SPLITS;
}

hipError_t attention_seg_plan(const KvGeom &kv, int num_heads, int B, const int *const *tables, const int64_t *lens, const int *ns,
                              const int *rows, int part_cap, AttnSeg *segs, int *nseg, AttnSegRun *runs, int *nrun, int *states) {
    AttnSeg all[VLO_ATTN_SEG_MAX];
    int fam[VLO_ATTN_SEG_MAX];
    AttnGeom geo[VLO_ATTN_SEG_MAX];
    int cnt = 0, part = 0;
    for (int b = 0; b < B; ++b) {
        AttnGeom g;
        const hipError_t e = attention_geometry(kv, num_heads, lens[b], ns[b], &g);
        if (e != hipSuccess) return e;
        if (g.nz > kBlockSubchunks) return hipErrorInvalidValue;
        for (int z = 0; z < g.nz; ++z) {
            if (cnt == VLO_ATTN_SEG_MAX) return hipErrorInvalidValue;
            AttnSeg &s = all[cnt];
            s.page_table = tables[b];
            s.pos0 = lens[b] + 16 * z;
            s.n = ns[b] - 16 * z < 16 ? ns[b] - 16 * z : 16;
            s.chunk = g.chunk;
            s.nsplit = g.nsplit;
            s.row0 = rows[b] + 16 * z;
            s.part0 = part + z * g.nsplit;          // the solo launch's layout: sub-chunk z's states follow sub-chunk z - 1's
            s.pad_ = 0;
            fam[cnt] = g.nct;
            geo[cnt] = g;
            ++cnt;
        }
        part += g.nz * g.nsplit;
    }
    if (part > part_cap) return hipErrorInvalidValue;
    int k = 0, r = 0;
    for (int f = 0; f <= 3; ++f) {                  // one launch per kernel family: attn_chunk, attn_cols NCT = 1, 2, 3
        const int first = k;
        int mx = 0;
        for (int i = 0; i < cnt; ++i)
            if (fam[i] == f) {
                segs[k++] = all[i];
                if (all[i].nsplit > mx) mx = all[i].nsplit;
                if (k - first == 1) runs[r].g = geo[i];
            }
        if (k > first) {
            runs[r].first = first;
            runs[r].count = k - first;
            runs[r].max_nsplit = mx;
            ++r;
        }
    }
    *nseg = cnt;
    *nrun = r;
    *states = part;
    return hipSuccess;
}

// ------------------------------------------------------------------------------------
// The live-step attention kernels, every instantiation ONCE: a row = one (head dim, HPW) shape of the chunk family or one (head dim, NCT) shape
// of the column-packed family, with its solo / segmented x bf16 / fp8 kernels.  Both launchers pick their kernel here, and the dynamic-LDS
// limit is raised by walking the same rows.  A new shape is one more row; a new variant of a family is one more column.
// ------------------------------------------------------------------------------------
struct AttnKernels {
    int hd, p;                                           // p = HPW (chunk rows) or NCT (column-packed rows)
    decltype(&attn_chunk_kernel<128, 1>) chunk;          // chunk rows fill these four, column-packed rows the other four
    decltype(&attn_chunk_f8_kernel<128, 1>) chunk_f8;
    decltype(&attn_chunk_seg_kernel<128, 1>) chunk_seg;
    decltype(&attn_chunk_seg_f8_kernel<128, 1>) chunk_seg_f8;
    decltype(&attn_cols_kernel<128, 1>) cols;
    decltype(&attn_cols_f8_kernel<128, 1>) cols_f8;
    decltype(&attn_cols_seg_kernel<128, 1>) cols_seg;
    decltype(&attn_cols_seg_f8_kernel<128, 1>) cols_seg_f8;
};
template <int HD, int HPW>
constexpr AttnKernels attn_chunk_row() {
    return {HD, HPW, attn_chunk_kernel<HD, HPW>, attn_chunk_f8_kernel<HD, HPW>, attn_chunk_seg_kernel<HD, HPW>, attn_chunk_seg_f8_kernel<HD, HPW>,
            nullptr, nullptr, nullptr, nullptr};
}
template <int HD, int NCT>
constexpr AttnKernels attn_cols_row() {
    return {HD, NCT, nullptr, nullptr, nullptr, nullptr,
            attn_cols_kernel<HD, NCT>, attn_cols_f8_kernel<HD, NCT>, attn_cols_seg_kernel<HD, NCT>, attn_cols_seg_f8_kernel<HD, NCT>};
}
static constexpr AttnKernels kAttnKernels[] = {
    attn_chunk_row<128, 2>(), attn_chunk_row<128, 1>(), attn_chunk_row<64, 2>(), attn_chunk_row<64, 1>(),
    attn_cols_row<128, 1>(), attn_cols_row<128, 2>(), attn_cols_row<128, 3>(), attn_cols_row<64, 1>(), attn_cols_row<64, 2>(), attn_cols_row<64, 3>()};
struct AttnCombine { int hd; decltype(&attn_combine_kernel<128>) solo; decltype(&attn_combine_seg_kernel<128>) seg; };
static constexpr AttnCombine kAttnCombine[] = {{128, attn_combine_kernel<128>, attn_combine_seg_kernel<128>},
                                               {64, attn_combine_kernel<64>, attn_combine_seg_kernel<64>}};

// the row of this shape — nct != 0: column-packed (hd, nct), else chunk (hd, hpw) — or nullptr: not instantiated.  The first lookup of the
// process raises every kernel's dynamic-LDS limit to the CU's 160 KiB (function-local static: safe from sessions stepping on threads of their own).
static const AttnKernels *attn_kernels(int hd, int hpw, int nct) {
    static const bool lds_raised = [] {
        for (const AttnKernels &r : kAttnKernels)
            for (const void *k : {(const void *)r.chunk, (const void *)r.chunk_f8, (const void *)r.chunk_seg, (const void *)r.chunk_seg_f8,
                                  (const void *)r.cols, (const void *)r.cols_f8, (const void *)r.cols_seg, (const void *)r.cols_seg_f8})
                if (k) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipGetLastError();
        return true;
    }();
    (void)lds_raised;
    for (const AttnKernels &r : kAttnKernels)
        if (r.hd == hd && (nct ? r.cols && r.p == nct : r.chunk && r.p == hpw)) return &r;
    return nullptr;
}
static const AttnCombine *attn_combine(int hd) {
    for (const AttnCombine &c : kAttnCombine)
        if (c.hd == hd) return &c;
    return nullptr;
}

hipError_t attention_launch(const unsigned short *q, const KvPool &kv, int layer, int num_heads, int64_t pos0, int n,
                            float *part_o, float *part_ml, unsigned short *out, hipStream_t st, int pack_row0, int part_cap) {
    AttnGeom ag;
    const hipError_t ge = attention_geometry(kv, num_heads, pos0, n, &ag, part_cap);
    if (ge != hipSuccess) return ge;
    const int nkv = kv.num_kv_heads, hd = kv.head_dim, G = ag.G, hpw = ag.hpw, nhg = ag.nhg, KS = ag.KS, nz = ag.nz, chunk = ag.chunk,
              nsplit = ag.nsplit;
    const float scale = ag.scale;
    dim3 grid(nsplit, nkv, nz), block(nhg * KS * 64);
    const size_t lds = ag.lds_bytes;
    const AttnKernels *k = attn_kernels(hd, hpw, ag.nct);
    const KvGeom &kg = kv;
    const bool f8 = kv.dtype == VLO_KV_FP8;
    if (!k || (f8 && !kv.scale)) return hipErrorInvalidValue;
    if (ag.nct) {
        if (f8) hipLaunchKernelGGL(k->cols_f8, grid, dim3(512), lds, st, q, kg, layer, num_heads, G, pos0, n, chunk, scale, part_o, part_ml, kv.scale);
        else hipLaunchKernelGGL(k->cols, grid, dim3(512), lds, st, q, kg, layer, num_heads, G, pos0, n, chunk, scale, part_o, part_ml);
    } else {
        if (f8) hipLaunchKernelGGL(k->chunk_f8, grid, block, lds, st, q, kg, layer, num_heads, G, KS, pos0, n, chunk, scale, part_o, part_ml, kv.scale);
        else hipLaunchKernelGGL(k->chunk, grid, block, lds, st, q, kg, layer, num_heads, G, KS, pos0, n, chunk, scale, part_o, part_ml);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const AttnCombine *c = attn_combine(hd);
    if (!c) return hipErrorInvalidValue;
    hipLaunchKernelGGL(c->solo, dim3(num_heads, n), dim3(256), 0, st, part_o, part_ml, nsplit, num_heads, out, pack_row0);
    return hipGetLastError();
}

hipError_t attention_seg_launch(const unsigned short *q, const KvPool &kv, int layer, int num_heads, const AttnSeg *segs_dev, int nseg,
                                const AttnSegRun *runs, int nrun, float *part_o, float *part_ml, unsigned short *out, bool packed, hipStream_t st) {
    const int nkv = kv.num_kv_heads, hd = kv.head_dim;
    const bool f8 = kv.dtype == VLO_KV_FP8;
    if (f8 && !kv.scale) return hipErrorInvalidValue;
    if (nseg < 1 || nseg > VLO_ATTN_SEG_MAX) return hipErrorInvalidValue;
    const KvGeom &kg = kv;
    for (int r = 0; r < nrun; ++r) {
        const AttnGeom &g = runs[r].g;
        const AttnSeg *sd = segs_dev + runs[r].first;
        const dim3 grid(runs[r].max_nsplit, nkv, runs[r].count), block(g.nhg * g.KS * 64);
        const size_t lds = g.lds_bytes;
        const AttnKernels *k = attn_kernels(hd, g.hpw, g.nct);
        if (!k) return hipErrorInvalidValue;
        if (g.nct) {
            if (f8) hipLaunchKernelGGL(k->cols_seg_f8, grid, dim3(512), lds, st, q, kg, layer, num_heads, g.G, sd, g.scale, part_o, part_ml, kv.scale);
            else hipLaunchKernelGGL(k->cols_seg, grid, dim3(512), lds, st, q, kg, layer, num_heads, g.G, sd, g.scale, part_o, part_ml);
        } else {
            if (f8) hipLaunchKernelGGL(k->chunk_seg_f8, grid, block, lds, st, q, kg, layer, num_heads, g.G, g.KS, sd, g.scale, part_o, part_ml, kv.scale);
            else hipLaunchKernelGGL(k->chunk_seg, grid, block, lds, st, q, kg, layer, num_heads, g.G, g.KS, sd, g.scale, part_o, part_ml);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const AttnCombine *c = attn_combine(hd);
    if (!c) return hipErrorInvalidValue;
    hipLaunchKernelGGL(c->seg, dim3(num_heads, 16, nseg), dim3(256), 0, st, part_o, part_ml, segs_dev, num_heads, out, (int)packed);
    return hipGetLastError();
}

// dst[i] = src[i] (bf16 rows of `cols` elements): one block per row
__global__ void copy_rows_indexed_kernel(RowCopy rc, int n16) {
    const uint4 *src = reinterpret_cast<const uint4 *>(rc.src[blockIdx.x]);
    uint4 *dst = reinterpret_cast<uint4 *>(rc.dst[blockIdx.x]);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
}
hipError_t copy_rows_indexed_launch(const RowCopy &rc, int count, int cols, hipStream_t st) {
    if (count < 1 || count > VLO_ROWCOPY_MAX || (cols & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_rows_indexed_kernel, dim3(count), dim3(256), 0, st, rc, cols / 8);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// embedding gather, row copy, KV read-back (tests)
// ------------------------------------------------------------------------------------
__global__ void embed_gather_kernel(const bf16_t *__restrict__ table, const int64_t *__restrict__ ids, int H, int64_t vocab,
                                    bf16_t *__restrict__ out) {
    int64_t id = ids[blockIdx.x];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const uint4 *src = reinterpret_cast<const uint4 *>(table + (size_t)id * H);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)blockIdx.x * H);
    for (int i = threadIdx.x; i < H / 8; i += blockDim.x) dst[i] = src[i];
}
hipError_t embed_gather_launch(const unsigned short *table, const int64_t *ids, int k, int H, int64_t vocab,
                               unsigned short *out, hipStream_t st) {
    hipLaunchKernelGGL(embed_gather_kernel, dim3(k), dim3(256), 0, st, table, ids, H, vocab, out);
    return hipGetLastError();
}

// step input (demo/inference.py:65-68: `torch.cat([embed(last_ids), frame_embeds])`) in ONE launch: the token ids arrive from the HOST
// as kernel arguments (no `torch.tensor(ids, device=...)` upload), blocks [0, k) gather their embedding row, blocks [k, k + rows) copy
// a frame-token row of the connector's output.
__global__ void step_input_kernel(const bf16_t *__restrict__ table, StepIds ids, int k, const bf16_t *__restrict__ frame_rows, int H,
                                  int64_t vocab, bf16_t *__restrict__ out) {
    const int r = blockIdx.x;
    const uint4 *src;
    if (r < k) {
        int64_t id = ids.v[r];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        src = reinterpret_cast<const uint4 *>(table + (size_t)id * H);
    } else {
        src = reinterpret_cast<const uint4 *>(frame_rows + (size_t)(r - k) * H);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)r * H);
    for (int i = threadIdx.x; i < H / 8; i += blockDim.x) dst[i] = src[i];
}
hipError_t step_input_launch(const unsigned short *table, const StepIds &ids, int k, const unsigned short *frame_rows, int rows, int H,
                             int64_t vocab, unsigned short *out, hipStream_t st) {
    hipLaunchKernelGGL(step_input_kernel, dim3(k + rows), dim3(256), 0, st, table, ids, k, frame_rows, H, vocab, out);
    return hipGetLastError();
}

// the step inputs of SEVERAL consecutive frame steps in one launch (stream lookahead): unit u = the embeddings of its ids, then frame rows
// [u * rows_per_unit, (u + 1) * rows_per_unit).  Block r finds its unit in the row table (at most VLO_STEPS_UNITS_MAX entries, kernel arguments)
// and copies its row exactly as step_input_kernel does.
__global__ void steps_input_kernel(const bf16_t *__restrict__ table, StepsIds ids, int units, const bf16_t *__restrict__ frame_rows,
                                   int rows_per_unit, int H, int64_t vocab, bf16_t *__restrict__ out) {
    const int r = blockIdx.x;
    int u = 0;
    while (u + 1 < units && r >= ids.row0[u + 1]) ++u;
    const int j = r - ids.row0[u], k = ids.id0[u + 1] - ids.id0[u];
    const uint4 *src;
    if (j < k) {
        int64_t id = ids.v[ids.id0[u] + j];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        src = reinterpret_cast<const uint4 *>(table + (size_t)id * H);
    } else {
        src = reinterpret_cast<const uint4 *>(frame_rows + ((size_t)u * rows_per_unit + (j - k)) * H);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)r * H);
    for (int i = threadIdx.x; i < H / 8; i += blockDim.x) dst[i] = src[i];
}
hipError_t steps_input_launch(const unsigned short *table, const StepsIds &ids, int units, const unsigned short *frame_rows, int rows_per_unit,
                              int H, int64_t vocab, unsigned short *out, hipStream_t st) {
    if (units < 1 || units > VLO_STEPS_UNITS_MAX || rows_per_unit < 0 || (H & 7) || ids.row0[0] != 0 || ids.id0[0] != 0) return hipErrorInvalidValue;
    for (int u = 0; u < units; ++u) {
        const int k = ids.id0[u + 1] - ids.id0[u];
        if (k < 0 || k > (u ? VLO_STEPS_IDS_LATER : VLO_STEP_IDS_MAX) || ids.row0[u + 1] != ids.row0[u] + k + rows_per_unit) return hipErrorInvalidValue;
    }
    if (ids.row0[units] < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(steps_input_kernel, dim3(ids.row0[units]), dim3(256), 0, st, table, ids, units, frame_rows, rows_per_unit, H, vocab, out);
    return hipGetLastError();
}

__global__ void copy_rows_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
hipError_t copy_rows_launch(const unsigned short *src, unsigned short *dst, int rows, int H, hipStream_t st) {
    const size_t n16 = (size_t)rows * H / 8;
    int blocks = (int)((n16 + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(blocks), dim3(256), 0, st, (const uint4 *)src, (uint4 *)dst, n16);
    return hipGetLastError();
}

__global__ void read_kv_kernel(KvGeom kv, int layer, int which, int kvh, int64_t t0, bf16_t *__restrict__ dst) {
    const int64_t t = t0 + blockIdx.x;
    const int page = kv.page_table[t / VLO_PAGE_TOKENS];
    const int tok = (int)(t % VLO_PAGE_TOKENS);
    const int hd = kv.head_dim;
    for (int d = threadIdx.x; d < hd; d += blockDim.x) {
        bf16_t v;
        if (which == 0)
            v = kv.k_pool[(size_t)layer * kv.layer_stride + (size_t)page * kv.page_elems + ((size_t)kvh * VLO_PAGE_TOKENS + tok) * hd + d];
        else
            v = kv.vt_pool[(size_t)layer * kv.layer_stride + (size_t)page * kv.page_elems + ((size_t)kvh * hd + d) * VLO_PAGE_TOKENS + tok];
        dst[(size_t)blockIdx.x * hd + d] = v;
    }
}
// fp8 pool: bf16(code * scale) — the value attention multiplies with (exact when the scale is a power of two)
__global__ void read_kv_f8_kernel(KvGeom kv, int layer, int which, int kvh, int64_t t0, const float *__restrict__ kv_scale, bf16_t *__restrict__ dst) {
    const int64_t t = t0 + blockIdx.x;
    const int page = kv.page_table[t / VLO_PAGE_TOKENS];
    const int tok = (int)(t % VLO_PAGE_TOKENS);
    const int hd = kv.head_dim;
    const float sc = kv_scale[2 * layer + which];
    const uint8_t *k8 = reinterpret_cast<const uint8_t *>(kv.k_pool), *v8 = reinterpret_cast<const uint8_t *>(kv.vt_pool);
    for (int d = threadIdx.x; d < hd; d += blockDim.x) {
        uint8_t c;
        if (which == 0)
            c = k8[(size_t)layer * kv.layer_stride + (size_t)page * kv.page_elems + ((size_t)kvh * VLO_PAGE_TOKENS + tok) * hd + d];
        else
            c = v8[(size_t)layer * kv.layer_stride + (size_t)page * kv.page_elems + ((size_t)kvh * hd + d) * VLO_PAGE_TOKENS + tok];
        dst[(size_t)blockIdx.x * hd + d] = f2bf(fp8_to_f32(c) * sc);
    }
}
hipError_t read_kv_launch(const KvPool &kv, int layer, int which, int kv_head, int64_t t0, int64_t t1, unsigned short *dst,
                          hipStream_t st) {
    if (t1 <= t0) return hipSuccess;
    const KvGeom &kg = kv;
    if (kv.dtype == VLO_KV_FP8) {
        if (!kv.scale) return hipErrorInvalidValue;
        hipLaunchKernelGGL(read_kv_f8_kernel, dim3((unsigned)(t1 - t0)), dim3(64), 0, st, kg, layer, which, kv_head, t0, kv.scale, dst);
    } else {
        hipLaunchKernelGGL(read_kv_kernel, dim3((unsigned)(t1 - t0)), dim3(64), 0, st, kg, layer, which, kv_head, t0, dst);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// samplers over the L2-resident bf16 logits [V]: SAMPLE_BLOCKS blocks scan a slice each, a one-wave
// kernel merges the partials (3 short launches instead of one ~90 us single-block scan).
// ------------------------------------------------------------------------------------
#define SAMPLE_BLOCKS 64
#define SAMPLE_THREADS 256

struct ArgBest { float v; int i; };
VLO_DEV ArgBest better(ArgBest a, ArgBest b) {      // larger value wins; ties -> smaller index (torch argmax)
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
    return a;
}
VLO_DEV ArgBest wave_argbest(ArgBest x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgBest y;
        y.v = __shfl_xor(x.v, o, 64);
        y.i = __shfl_xor(x.i, o, 64);
        x = better(x, y);
    }
    return x;
}
VLO_DEV ArgBest block_argbest(ArgBest x, float *smv, int *smi) {
    x = wave_argbest(x);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) { smv[w] = x.v; smi[w] = x.i; }
    __syncthreads();
    ArgBest r = {smv[0], smi[0]};
    for (int k = 1; k < nw; ++k) r = better(r, (ArgBest){smv[k], smi[k]});
    return r;
}

// scratch layout (floats): [0, NB) block max | [NB, 2NB) block sum of exp(x - block max) | [2NB, 3NB) best value |
//                          [3NB, 4NB) best index (int bits)
// Every kernel has a grid.y = row twin for batched steps that runs the SAME body (a textual include or a shared device function) on its row,
// so a row's reduction order is the solo kernel's.
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_stats_kernel(const bf16_t *__restrict__ logits, int V, float *__restrict__ scr) {
    __shared__ float sm[16];
    __shared__ float smv[16];
    __shared__ int smi[16];
#include "sample_stats_body.inc"
}

// rows x V logits: row blockIdx.y, scratch VLO_SAMPLE_SCRATCH_FLOATS per row
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_stats_rows_kernel(const bf16_t *__restrict__ logits_rows, int V, float *__restrict__ scr_rows) {
    __shared__ float sm[16];
    __shared__ float smv[16];
    __shared__ int smi[16];
    const bf16_t *__restrict__ logits = logits_rows + (size_t)blockIdx.y * V;
    float *__restrict__ scr = scr_rows + (size_t)blockIdx.y * VLO_SAMPLE_SCRATCH_FLOATS;
#include "sample_stats_body.inc"
}

// force_mode: 0 = plain argmax; 1 = argmax but never eos (scheduled mode, mid-response);
//             2 = argmax computed, eos written (scheduled mode, last token)
VLO_DEV void greedy_final_body(const float *__restrict__ scr, int NB, int V, int64_t *tok_out, int eos, int force_mode) {
    ArgBest b = {-INFINITY, 0x7fffffff};
    for (int k = threadIdx.x; k < NB; k += 64) b = better(b, (ArgBest){scr[2 * NB + k], reinterpret_cast<const int *>(scr)[3 * NB + k]});
    b = wave_argbest(b);
    if (threadIdx.x == 0) {
        int t = b.i;
        if (force_mode == 1 && t == eos) t = (eos + 1) % V;
        if (force_mode == 2) t = eos;
        *tok_out = t;
    }
}
__global__ __launch_bounds__(64) void greedy_final_kernel(const float *__restrict__ scr, int NB, int V, int64_t *tok_out, int eos,
                                                          int force_mode) {
    greedy_final_body(scr, NB, V, tok_out, eos, force_mode);
}
__global__ __launch_bounds__(64) void greedy_final_rows_kernel(const float *__restrict__ scr, int NB, int V, int64_t *tok_out) {
    greedy_final_body(scr + (size_t)blockIdx.y * VLO_SAMPLE_SCRATCH_FLOATS, NB, V, tok_out + blockIdx.y, 0, 0);
}
hipError_t greedy_sample_launch(const unsigned short *logits, int V, int64_t *tok_out, int eos, int force_mode, float *scratch,
                                hipStream_t st) {
    hipLaunchKernelGGL(sample_stats_kernel, dim3(SAMPLE_BLOCKS), dim3(SAMPLE_THREADS), 0, st, logits, V, scratch);
    hipLaunchKernelGGL(greedy_final_kernel, dim3(1), dim3(64), 0, st, scratch, SAMPLE_BLOCKS, V, tok_out, eos, force_mode);
    return hipGetLastError();
}
hipError_t greedy_sample_rows_launch(const unsigned short *logits, int rows, int V, int64_t *tok_out, float *scratch, hipStream_t st) {
    if (rows < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_stats_rows_kernel, dim3(SAMPLE_BLOCKS, rows), dim3(SAMPLE_THREADS), 0, st, logits, V, scratch);
    hipLaunchKernelGGL(greedy_final_rows_kernel, dim3(1, rows), dim3(64), 0, st, scratch, SAMPLE_BLOCKS, V, tok_out);
    return hipGetLastError();
}

// demo/inference.py:76-79: softmax over a bf16 tensor (fp32 inside, bf16 out), threshold on p[interval], argmax of p.
// Every block recomputes the global (max, sum) from the NB partials, then scans its slice of p.
__global__ __launch_bounds__(SAMPLE_THREADS) void stream_scan_kernel(const bf16_t *__restrict__ logits, int V, float threshold,
                                                                     int interval_id, float *__restrict__ scr) {
    __shared__ float smv[16];
    __shared__ int smi[16];
#include "stream_scan_body.inc"
}
__global__ __launch_bounds__(SAMPLE_THREADS) void stream_scan_rows_kernel(const bf16_t *__restrict__ logits_rows, int V, float threshold,
                                                                          int interval_id, float *__restrict__ scr_rows) {
    __shared__ float smv[16];
    __shared__ int smi[16];
    const bf16_t *__restrict__ logits = logits_rows + (size_t)blockIdx.y * V;
    float *__restrict__ scr = scr_rows + (size_t)blockIdx.y * VLO_SAMPLE_SCRATCH_FLOATS;
#include "stream_scan_body.inc"
}
VLO_DEV void stream_final_body(const float *__restrict__ scr, int NB, int64_t *tok_out, float *p_interval_out) {
    ArgBest b = {-INFINITY, 0x7fffffff};
    for (int k = threadIdx.x; k < NB; k += 64) b = better(b, (ArgBest){scr[4 * NB + k], reinterpret_cast<const int *>(scr)[5 * NB + k]});
    b = wave_argbest(b);
    if (threadIdx.x == 0) {
        *tok_out = b.i;
        if (p_interval_out) *p_interval_out = scr[6 * NB];
    }
}
__global__ __launch_bounds__(64) void stream_final_kernel(const float *__restrict__ scr, int NB, int64_t *tok_out, float *p_interval_out) {
    stream_final_body(scr, NB, tok_out, p_interval_out);
}
__global__ __launch_bounds__(64) void stream_final_rows_kernel(const float *__restrict__ scr, int NB, int64_t *tok_out, float *p_interval_out) {
    const int r = blockIdx.y;
    stream_final_body(scr + (size_t)r * VLO_SAMPLE_SCRATCH_FLOATS, NB, tok_out + r, p_interval_out ? p_interval_out + r : nullptr);
}
hipError_t stream_sample_launch(const unsigned short *logits, int V, float threshold, int interval_id, int64_t *tok_out,
                                float *p_interval_out, float *scratch, hipStream_t st) {
    if (interval_id < 0 || interval_id >= V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_stats_kernel, dim3(SAMPLE_BLOCKS), dim3(SAMPLE_THREADS), 0, st, logits, V, scratch);
    hipLaunchKernelGGL(stream_scan_kernel, dim3(SAMPLE_BLOCKS), dim3(SAMPLE_THREADS), 0, st, logits, V, threshold, interval_id, scratch);
    hipLaunchKernelGGL(stream_final_kernel, dim3(1), dim3(64), 0, st, scratch, SAMPLE_BLOCKS, tok_out, p_interval_out);
    return hipGetLastError();
}
// the finishing launch of the sampler over the `rows` unit-end rows of a lookahead pass: wave r of the ONE block finishes row r as
// stream_final_body does (one partial per lane, the same wave_argbest), then thread 0 writes the first-speaker count
// *n_accept = (smallest r with tok[r] != interval_id) + 1, or rows when every row stays silent.
__global__ __launch_bounds__(64 * VLO_ROWIDX_MAX) void stream_final_steps_kernel(const float *__restrict__ scr_rows, int NB, int rows, int interval_id,
                                                                               int64_t *tok_out, float *p_interval_out, int *n_accept) {
    __shared__ int toks[VLO_ROWIDX_MAX];
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (r < rows) {
        const float *scr = scr_rows + (size_t)r * VLO_SAMPLE_SCRATCH_FLOATS;
        ArgBest b = {-INFINITY, 0x7fffffff};
        for (int k = lane; k < NB; k += 64) b = better(b, (ArgBest){scr[4 * NB + k], reinterpret_cast<const int *>(scr)[5 * NB + k]});
        b = wave_argbest(b);
        if (lane == 0) {
            toks[r] = b.i;
            tok_out[r] = b.i;
            if (p_interval_out) p_interval_out[r] = scr[6 * NB];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = rows;
        for (int k = rows - 1; k >= 0; --k)
            if (toks[k] != interval_id) acc = k + 1;
        *n_accept = acc;
    }
}
hipError_t stream_sample_steps_launch(const unsigned short *logits, int rows, int V, float threshold, int interval_id, int64_t *tok_out,
                                      float *p_interval_out, int *n_accept_out, float *scratch, hipStream_t st) {
    if (interval_id < 0 || interval_id >= V || rows < 1 || rows > VLO_ROWIDX_MAX || !n_accept_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_stats_rows_kernel, dim3(SAMPLE_BLOCKS, rows), dim3(SAMPLE_THREADS), 0, st, logits, V, scratch);
    hipLaunchKernelGGL(stream_scan_rows_kernel, dim3(SAMPLE_BLOCKS, rows), dim3(SAMPLE_THREADS), 0, st, logits, V, threshold, interval_id, scratch);
    hipLaunchKernelGGL(stream_final_steps_kernel, dim3(1), dim3(64 * rows), 0, st, scratch, SAMPLE_BLOCKS, rows, interval_id, tok_out, p_interval_out,
                       n_accept_out);
    return hipGetLastError();
}
hipError_t stream_sample_rows_launch(const unsigned short *logits, int rows, int V, float threshold, int interval_id, int64_t *tok_out,
                                     float *p_interval_out, float *scratch, hipStream_t st) {
    if (interval_id < 0 || interval_id >= V || rows < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_stats_rows_kernel, dim3(SAMPLE_BLOCKS, rows), dim3(SAMPLE_THREADS), 0, st, logits, V, scratch);
    hipLaunchKernelGGL(stream_scan_rows_kernel, dim3(SAMPLE_BLOCKS, rows), dim3(SAMPLE_THREADS), 0, st, logits, V, threshold, interval_id, scratch);
    hipLaunchKernelGGL(stream_final_rows_kernel, dim3(1, rows), dim3(64), 0, st, scratch, SAMPLE_BLOCKS, tok_out, p_interval_out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Teacher-forced evaluation helpers (models/modeling_live.py:29-42, 44-168, 170-171)
// ------------------------------------------------------------------------------------
// joint_embed (:38-41): rank of every placeholder position among the placeholders (exclusive scan, one block).
__global__ __launch_bounds__(1024) void placeholder_rank_kernel(const int64_t *__restrict__ ids, int k, int64_t v_id,
                                                                int *__restrict__ src_idx, int *__restrict__ count_out) {
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (int i0 = 0; i0 < k; i0 += 1024) {
        const int i = i0 + threadIdx.x;
        const int f = (i < k && ids[i] == v_id) ? 1 : 0;
        int inc = f;                                   // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int before = base_s;
        for (int j = 0; j < w; ++j) before += wsum[j];
        if (i < k) src_idx[i] = f ? before + inc - 1 : -1;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int j = 0; j < 16; ++j) t += wsum[j];
            base_s += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count_out = base_s;
}
// rows with src_idx >= 0 take frame-token row src_idx, the others the (clamped) embedding-table row
__global__ void joint_gather_kernel(const bf16_t *__restrict__ table, const int64_t *__restrict__ ids, const int *__restrict__ src_idx,
                                    const bf16_t *__restrict__ frame_rows, int n_frame_rows, int H, int64_t vocab,
                                    bf16_t *__restrict__ out) {
    const int r = src_idx[blockIdx.x];
    const uint4 *src;
    if (r >= 0) {
        if (r >= n_frame_rows) return;                 // count mismatch: the host reports the error
        src = reinterpret_cast<const uint4 *>(frame_rows + (size_t)r * H);
    } else {
        int64_t id = ids[blockIdx.x];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        src = reinterpret_cast<const uint4 *>(table + (size_t)id * H);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)blockIdx.x * H);
    for (int i = threadIdx.x; i < H / 8; i += blockDim.x) dst[i] = src[i];
}
hipError_t joint_embed_launch(const unsigned short *table, const int64_t *ids, int k, int64_t v_id, const unsigned short *frame_rows,
                              int n_frame_rows, int H, int64_t vocab, int *src_idx_scratch, int *count_out, unsigned short *out,
                              hipStream_t st) {
    hipLaunchKernelGGL(placeholder_rank_kernel, dim3(1), dim3(1024), 0, st, ids, k, v_id, src_idx_scratch, count_out);
    hipLaunchKernelGGL(joint_gather_kernel, dim3(k), dim3(256), 0, st, table, ids, src_idx_scratch, frame_rows, n_frame_rows, H, vocab,
                       out);
    return hipGetLastError();
}

// trim_past_key_values(past, 0, stop) as a fork: copy the pages holding positions [0, stop) of every layer into the
// pages of another session.  grid = (pages, layers, 2 {K, V^T}).
__global__ void kv_copy_pages_kernel(KvGeom kv, const int *__restrict__ src_pt, const int *__restrict__ dst_pt) {
    unsigned short *pool = blockIdx.z == 0 ? kv.k_pool : kv.vt_pool;
    const size_t lay = (size_t)blockIdx.y * kv.layer_stride;
    const uint4 *src = reinterpret_cast<const uint4 *>(pool + lay + (size_t)src_pt[blockIdx.x] * kv.page_elems);
    uint4 *dst = reinterpret_cast<uint4 *>(pool + lay + (size_t)dst_pt[blockIdx.x] * kv.page_elems);
    const int n16 = (int)(kv.page_elems / 8);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
}
hipError_t kv_copy_pages_launch(const KvPool &kv, const int *src_pt, const int *dst_pt, int pages, int layers, hipStream_t st) {
    if (pages <= 0) return hipSuccess;
    KvGeom g = kv;
    if (kv.dtype == VLO_KV_FP8) {
        // the kernel moves 16-bit elements: an e4m3 page of page_elems bytes is page_elems / 2 of them, its strides likewise (page_elems is a
        // multiple of VLO_PAGE_TOKENS * 64, so the halves stay whole 16-byte vectors)
        g.layer_stride /= 2;
        g.page_elems /= 2;
    }
    hipLaunchKernelGGL(kv_copy_pages_kernel, dim3(pages, layers, 2), dim3(256), 0, st, g, src_pt, dst_pt);
    return hipGetLastError();
}

// vlo_session_evict: forget cache positions [t0, t0 + d) of a bf16 pool.  Tokens [t0 + d, len) move down by d slots IN PLACE, their keys
// rotated back by d positions (rot = cos / sin of d * inv_freq, vlo.h), V^T shifted bit for bit along its token axis.
// The move overlaps itself, so its order matters.  Data of different (layer, kv head, K | V^T) never meet, nor do different hd rows of V^T:
// a block owns one such slice (grid.x: kvh K slices of whole token rows, then kvh * HD / 64 V^T slices of 64 hd rows; grid.y = layer) and walks
// its destination tokens in ascending CHUNKS (K: 16384 / HD tokens, V^T: 128).  A chunk [a, b) reads tokens [a + d, b + d) (V^T: from the
// aligned 8-token vector holding a + d on), d >= 1: nothing below a — so no chunk reads what an EARLIER chunk stored — but possibly its own
// range: every thread loads all the chunk needs into registers, __syncthreads(), then stores.  The loads of chunk c + 1 start at b or above,
// which the stores of chunk c ([a, b)) cannot touch: they are issued before those stores (the prefetch; one barrier per chunk).
// A thread's 4 items of a chunk are fixed at compile time: 8 uint4 in flight per thread and set, no indexing by a run-time value.
#define EVICT_K_ITEMS 4
#define EVICT_V_ITEMS 4
template <int HD>
__global__ __launch_bounds__(256) void kv_evict_kernel(KvGeom kv, long long t0, long long d, long long len, KvEvictRot rot) {
    constexpr int PT = VLO_PAGE_TOKENS;
    const int tid = threadIdx.x;
    const long long nl = len - d;                              // the new length: destination tokens are [t0, nl)
    const size_t lay = (size_t)blockIdx.y * kv.layer_stride;
    const int *__restrict__ pt = kv.page_table;
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    if ((int)blockIdx.x < kv.num_kv_heads) {
        // ---- K: whole token rows of one kv head.  item = (token, 16-byte unit u): pairs (8u + k, 8u + k + HD / 2), k < 8
        constexpr int U = HD / 16, CT = 256 * EVICT_K_ITEMS / U, TS = 256 / U;
        const int u = tid % U, tl = tid / U;
        float c[8], s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { c[k] = rot.c[u * 8 + k]; s[k] = rot.s[u * 8 + k]; }
        bf16_t *base = kv.k_pool + lay + (size_t)blockIdx.x * PT * HD + u * 8;
        auto row = [&](long long t) { return base + (size_t)pt[t / PT] * kv.page_elems + (size_t)(t % PT) * HD; };
        uint4 cl[EVICT_K_ITEMS], ch[EVICT_K_ITEMS], nxl[EVICT_K_ITEMS], nxh[EVICT_K_ITEMS];
        auto load = [&](long long cs, uint4 *lo, uint4 *hi) {
#pragma unroll
            for (int i = 0; i < EVICT_K_ITEMS; ++i) {
                const long long t = cs + tl + i * TS;
                lo[i] = hi[i] = z4;
                if (t >= t0 && t < nl) {
                    const bf16_t *src = row(t + d);
                    lo[i] = *reinterpret_cast<const uint4 *>(src);
                    hi[i] = *reinterpret_cast<const uint4 *>(src + HD / 2);
                }
            }
        };
        long long cs = t0 / CT * CT;
        load(cs, cl, ch);
        for (; cs < nl; cs += CT) {
            if (cs + CT < nl) load(cs + CT, nxl, nxh);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < EVICT_K_ITEMS; ++i) {
                const long long t = cs + tl + i * TS;
                if (t >= t0 && t < nl) {
                    const unsigned lw[4] = {cl[i].x, cl[i].y, cl[i].z, cl[i].w}, hw[4] = {ch[i].x, ch[i].y, ch[i].z, ch[i].w};
                    unsigned ol[4], oh[4];
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        // k'[i] = k[i] c + k[i + hd/2] s ; k'[i + hd/2] = k[i + hd/2] c - k[i] s, evaluated as written: two rounded fp32 products and
                        // one rounded sum, never contracted into a fused multiply-add (when the two terms cancel, the fused form differs from the stated
                        // one by many bf16 ulps of the small result)
#pragma clang fp contract(off)
                        const float a0 = __uint_as_float(lw[w] << 16), a1 = __uint_as_float(lw[w] & 0xffff0000u);
                        const float b0 = __uint_as_float(hw[w] << 16), b1 = __uint_as_float(hw[w] & 0xffff0000u);
                        const float c0 = c[2 * w], c1 = c[2 * w + 1], s0 = s[2 * w], s1 = s[2 * w + 1];
                        ol[w] = pack2bf(a0 * c0 + b0 * s0, a1 * c1 + b1 * s1);
                        oh[w] = pack2bf(b0 * c0 - a0 * s0, b1 * c1 - a1 * s1);
                    }
                    bf16_t *dst = row(t);
                    *reinterpret_cast<uint4 *>(dst) = make_uint4(ol[0], ol[1], ol[2], ol[3]);
                    *reinterpret_cast<uint4 *>(dst + HD / 2) = make_uint4(oh[0], oh[1], oh[2], oh[3]);
                }
            }
#pragma unroll
            for (int i = 0; i < EVICT_K_ITEMS; ++i) { cl[i] = nxl[i]; ch[i] = nxh[i]; }
        }
        return;
    }
    // ---- V^T: 64 hd rows of one kv head; the token axis is contiguous, so the move is a shift by d ELEMENTS: a destination vector of 8
    // tokens starting at g is elements [sh, sh + 8) of the two aligned source vectors A = (g + d) / 8 and A + 1, sh = d % 8 (a funnel shift)
    const int vs = (int)blockIdx.x - kv.num_kv_heads;
    const int head = vs / (HD / 64), r0 = vs % (HD / 64) * 64;
    const int sh = (int)(d & 7);
    constexpr int VR = 256 * EVICT_V_ITEMS / 64, CV = VR * 8;   // vectors per row and tokens of a chunk
    bf16_t *base = kv.vt_pool + lay + ((size_t)head * HD + r0) * PT;
    // address of the aligned vector with GLOBAL index A (tokens 8A .. 8A + 7) of row r
    auto vec = [&](long long A, int r) { return reinterpret_cast<uint4 *>(base + (size_t)pt[A / (PT / 8)] * kv.page_elems + (size_t)r * PT) + A % (PT / 8); };
    uint4 ca[EVICT_V_ITEMS], cb[EVICT_V_ITEMS], na[EVICT_V_ITEMS], nb[EVICT_V_ITEMS];
    auto load = [&](long long cs, uint4 *a, uint4 *b) {
#pragma unroll
        for (int i = 0; i < EVICT_V_ITEMS; ++i) {
            const int idx = tid + 256 * i;
            const long long g = cs + (idx % VR) * 8;
            a[i] = b[i] = z4;
            if (g + 8 > t0 && g < nl) {                        // some destination token of the vector is moved: g + d < len
                const long long A = (g + d) >> 3;
                a[i] = *vec(A, idx / VR);
                if (sh && (A + 1) * 8 < len) b[i] = *vec(A + 1, idx / VR);   // tokens >= len feed no moved element
            }
        }
    };
    long long cs = t0 / CV * CV;
    load(cs, ca, cb);
    for (; cs < nl; cs += CV) {
        if (cs + CV < nl) load(cs + CV, na, nb);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EVICT_V_ITEMS; ++i) {
            const int idx = tid + 256 * i;
            const long long g = cs + (idx % VR) * 8;
            if (g + 8 > t0 && g < nl) {
                unsigned w[8] = {ca[i].x, ca[i].y, ca[i].z, ca[i].w, cb[i].x, cb[i].y, cb[i].z, cb[i].w};
                if (sh & 4) {
#pragma unroll
                    for (int m = 0; m < 6; ++m) w[m] = w[m + 2];
                }
                if (sh & 2) {
#pragma unroll
                    for (int m = 0; m < 5; ++m) w[m] = w[m + 1];
                }
                if (sh & 1) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) w[m] = (w[m] >> 16) | (w[m + 1] << 16);
                }
                uint4 *dst = vec(g >> 3, idx / VR);
                if (g >= t0 && g + 8 <= nl) {
                    *dst = make_uint4(w[0], w[1], w[2], w[3]);
                } else {                                       // the vector holding t0 or the new end: only the moved tokens are written
                    bf16_t *d16 = reinterpret_cast<bf16_t *>(dst);
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (g + k >= t0 && g + k < nl) d16[k] = (bf16_t)(w[k >> 1] >> ((k & 1) * 16));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < EVICT_V_ITEMS; ++i) { ca[i] = na[i]; cb[i] = nb[i]; }
    }
}
hipError_t kv_evict_launch(const KvPool &kv, int layers, int64_t t0, int64_t d, int64_t len, const KvEvictRot &rot, hipStream_t st) {
    if (kv.dtype != VLO_KV_BF16) return hipErrorNotSupported;
    if (t0 < 0 || d <= 0 || t0 + d >= len) return hipErrorInvalidValue;   // nothing to move is the caller's case
    const KvGeom &g = kv;
    if (kv.head_dim == 128)
        hipLaunchKernelGGL(kv_evict_kernel<128>, dim3(kv.num_kv_heads * 3, layers), dim3(256), 0, st, g, (long long)t0, (long long)d, (long long)len, rot);
    else if (kv.head_dim == 64)
        hipLaunchKernelGGL(kv_evict_kernel<64>, dim3(kv.num_kv_heads * 2, layers), dim3(256), 0, st, g, (long long)t0, (long long)d, (long long)len, rot);
    else
        return hipErrorNotSupported;
    return hipGetLastError();
}

// vlo_session_evict_ranges: forget R disjoint ranges [a_j, b_j) of a bf16 pool in ONE pass.  The survivors keep their order; the run between
// range j and range j + 1 is SEGMENT j: destination tokens [w_j, w_{j+1}) (w_0 = a_0, w_R = the new length), all moved down by the same
// D_j = sum_{i <= j} (b_i - a_i), their keys rotated back by D_j positions with row j of the (c, s) table (rounded once, whatever R is), V^T
// shifted bit for bit.  The table {w, D, c, s} is device memory (64 x 128 floats do not fit in kernel arguments); a block copies w, D and
// — K blocks — its rows of (c, s) into LDS first.
// The decomposition and the hazard argument are kv_evict_kernel's: a block owns one (layer, kv head, K | 64-row V^T slice) and walks its
// DESTINATION tokens in ascending chunks.  A destination token t of segment j reads token t + D_j, and D_j >= 1 is non-decreasing along the
// tail, so a chunk [a, b) reads nothing below a + 1 (V^T: nothing below the aligned vector holding a, which starts at a: its first vector
// (g + D_j) / 8 with g >= a a multiple of 8) — never what an EARLIER chunk stored, all of which lies below a.  It may read its own range:
// every thread loads all the chunk needs into registers, __syncthreads(), then stores.  A later chunk reads from b + 1 (V^T: b) on, which the
// stores of this chunk ([a, b)) cannot touch, so the loads of chunk c + 1 are issued before the stores of chunk c (one barrier per chunk).
// Every item finds its segment by bisection of w in LDS (<= 6 steps); a thread's 4 items and their segment numbers are fixed-index registers.
// V^T: a destination vector of 8 tokens wholly inside one segment is the funnel shift of two aligned source vectors with sh = D_j & 7; one
// that straddles a segment boundary, w_0 or the new end is read and written element by element, only where its tokens are moved.  No element
// is read at or beyond len, no page-table entry beyond the page of token len - 1.
template <int HD>
__global__ __launch_bounds__(256) void kv_evict_ranges_kernel(KvGeom kv, const KvEvictTable *__restrict__ tab, int R, long long len) {
    constexpr int PT = VLO_PAGE_TOKENS, HH = HD / 2;
    __shared__ long long sw[VLO_EVICT_MAX_RANGES + 1], sD[VLO_EVICT_MAX_RANGES];
    __shared__ __attribute__((aligned(16))) float sc[VLO_EVICT_MAX_RANGES][HH];
    __shared__ __attribute__((aligned(16))) float ss[VLO_EVICT_MAX_RANGES][HH];
    const int tid = threadIdx.x;
    const bool is_k = (int)blockIdx.x < kv.num_kv_heads;
    for (int i = tid; i <= R; i += 256) sw[i] = tab->w[i];
    for (int i = tid; i < R; i += 256) sD[i] = tab->D[i];
    if (is_k)
        for (int i = tid; i < R * HH; i += 256) {
            sc[i / HH][i % HH] = tab->c[i / HH][i % HH];
            ss[i / HH][i % HH] = tab->s[i / HH][i % HH];
        }
    __syncthreads();
    const long long t0 = sw[0], nl = sw[R];                    // destination tokens are [t0, nl)
    // the segment of destination token t, t0 <= t < nl: the largest j with w_j <= t
    auto seg = [&](long long t) {
        int lo = 0, hi = R;
        while (hi - lo > 1) {
            const int m = (lo + hi) >> 1;
            if (sw[m] <= t) lo = m; else hi = m;
        }
        return lo;
    };
    const size_t lay = (size_t)blockIdx.y * kv.layer_stride;
    const int *__restrict__ pt = kv.page_table;
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    if (is_k) {
        // ---- K: whole token rows of one kv head.  item = (token, 16-byte unit u): pairs (8u + k, 8u + k + HD / 2), k < 8
        constexpr int U = HD / 16, CT = 256 * EVICT_K_ITEMS / U, TS = 256 / U;
        const int u = tid % U, tl = tid / U;
        bf16_t *base = kv.k_pool + lay + (size_t)blockIdx.x * PT * HD + u * 8;
        auto row = [&](long long t) { return base + (size_t)pt[t / PT] * kv.page_elems + (size_t)(t % PT) * HD; };
        uint4 cl[EVICT_K_ITEMS], ch[EVICT_K_ITEMS], nxl[EVICT_K_ITEMS], nxh[EVICT_K_ITEMS];
        int cj[EVICT_K_ITEMS], nj[EVICT_K_ITEMS];
        auto load = [&](long long cs, uint4 *lo, uint4 *hi, int *sj) {
#pragma unroll
            for (int i = 0; i < EVICT_K_ITEMS; ++i) {
                const long long t = cs + tl + i * TS;
                lo[i] = hi[i] = z4;
                sj[i] = 0;
                if (t >= t0 && t < nl) {
                    const int j = seg(t);
                    const bf16_t *src = row(t + sD[j]);
                    lo[i] = *reinterpret_cast<const uint4 *>(src);
                    hi[i] = *reinterpret_cast<const uint4 *>(src + HH);
                    sj[i] = j;
                }
            }
        };
        long long cs = t0 / CT * CT;
        load(cs, cl, ch, cj);
        for (; cs < nl; cs += CT) {
            if (cs + CT < nl) load(cs + CT, nxl, nxh, nj);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < EVICT_K_ITEMS; ++i) {
                const long long t = cs + tl + i * TS;
                if (t >= t0 && t < nl) {
                    const float4 *pc = reinterpret_cast<const float4 *>(&sc[cj[i]][u * 8]), *ps = reinterpret_cast<const float4 *>(&ss[cj[i]][u * 8]);
                    const float4 c0 = pc[0], c1 = pc[1], s0 = ps[0], s1 = ps[1];
                    const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                    const unsigned lw[4] = {cl[i].x, cl[i].y, cl[i].z, cl[i].w}, hw[4] = {ch[i].x, ch[i].y, ch[i].z, ch[i].w};
                    unsigned ol[4], oh[4];
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        // kv_evict_kernel's arithmetic, evaluated as written: two rounded fp32 products, one rounded sum, never a fused multiply-add
#pragma clang fp contract(off)
                        const float a0 = __uint_as_float(lw[w] << 16), a1 = __uint_as_float(lw[w] & 0xffff0000u);
                        const float b0 = __uint_as_float(hw[w] << 16), b1 = __uint_as_float(hw[w] & 0xffff0000u);
                        const float e0 = c[2 * w], e1 = c[2 * w + 1], f0 = s[2 * w], f1 = s[2 * w + 1];
                        ol[w] = pack2bf(a0 * e0 + b0 * f0, a1 * e1 + b1 * f1);
                        oh[w] = pack2bf(b0 * e0 - a0 * f0, b1 * e1 - a1 * f1);
                    }
                    bf16_t *dst = row(t);
                    *reinterpret_cast<uint4 *>(dst) = make_uint4(ol[0], ol[1], ol[2], ol[3]);
                    *reinterpret_cast<uint4 *>(dst + HH) = make_uint4(oh[0], oh[1], oh[2], oh[3]);
                }
            }
#pragma unroll
            for (int i = 0; i < EVICT_K_ITEMS; ++i) { cl[i] = nxl[i]; ch[i] = nxh[i]; cj[i] = nj[i]; }
        }
        return;
    }
    // ---- V^T: 64 hd rows of one kv head, the token axis contiguous.  item = (hd row, aligned destination vector of 8 tokens starting at g)
    const int vs = (int)blockIdx.x - kv.num_kv_heads;
    const int head = vs / (HD / 64), r0 = vs % (HD / 64) * 64;
    constexpr int VR = 256 * EVICT_V_ITEMS / 64, CV = VR * 8;   // vectors per row and tokens of a chunk
    constexpr int ELEMENTWISE = 8;                              // the mode of a straddling vector (a whole one carries its sh = D_j & 7 < 8)
    bf16_t *base = kv.vt_pool + lay + ((size_t)head * HD + r0) * PT;
    // address of the aligned vector with GLOBAL index A (tokens 8A .. 8A + 7) of row r
    auto vec = [&](long long A, int r) { return reinterpret_cast<uint4 *>(base + (size_t)pt[A / (PT / 8)] * kv.page_elems + (size_t)r * PT) + A % (PT / 8); };
    uint4 ca[EVICT_V_ITEMS], cb[EVICT_V_ITEMS], na[EVICT_V_ITEMS], nb[EVICT_V_ITEMS];
    int cm[EVICT_V_ITEMS], nm[EVICT_V_ITEMS];
    auto load = [&](long long cs, uint4 *a, uint4 *b, int *mode) {
#pragma unroll
        for (int i = 0; i < EVICT_V_ITEMS; ++i) {
            const int idx = tid + 256 * i, r = idx / VR;
            const long long g = cs + (idx % VR) * 8;
            a[i] = b[i] = z4;
            mode[i] = 0;
            if (g + 8 > t0 && g < nl) {                        // some destination token of the vector is moved
                int j = seg(g > t0 ? g : t0);
                if (g >= sw[j] && g + 8 <= sw[j + 1]) {        // wholly inside segment j: tokens g + D_j .. g + D_j + 7 < len
                    const long long D = sD[j], A = (g + D) >> 3;
                    a[i] = *vec(A, r);
                    if ((D & 7) && (A + 1) * 8 < len) b[i] = *vec(A + 1, r);
                    mode[i] = (int)(D & 7);
                } else {                                       // straddles a boundary: the moved tokens one by one, each from its own segment
                    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const long long t = g + k;
                        if (t >= t0 && t < nl) {
                            while (t >= sw[j + 1]) ++j;        // t < nl = w_R: ends at j <= R - 1
                            const long long src = t + sD[j];   // < len
                            const bf16_t v = base[(size_t)pt[src / PT] * kv.page_elems + (size_t)r * PT + src % PT];
                            w[k >> 1] |= (unsigned)v << ((k & 1) * 16);
                        }
                    }
                    a[i] = make_uint4(w[0], w[1], w[2], w[3]);
                    mode[i] = ELEMENTWISE;
                }
            }
        }
    };
    long long cs = t0 / CV * CV;
    load(cs, ca, cb, cm);
    for (; cs < nl; cs += CV) {
        if (cs + CV < nl) load(cs + CV, na, nb, nm);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EVICT_V_ITEMS; ++i) {
            const int idx = tid + 256 * i;
            const long long g = cs + (idx % VR) * 8;
            if (g + 8 > t0 && g < nl) {
                unsigned w[8] = {ca[i].x, ca[i].y, ca[i].z, ca[i].w, cb[i].x, cb[i].y, cb[i].z, cb[i].w};
                uint4 *dst = vec(g >> 3, idx / VR);
                if (cm[i] != ELEMENTWISE) {
                    const int sh = cm[i];
                    if (sh & 4) {
#pragma unroll
                        for (int m = 0; m < 6; ++m) w[m] = w[m + 2];
                    }
                    if (sh & 2) {
#pragma unroll
                        for (int m = 0; m < 5; ++m) w[m] = w[m + 1];
                    }
                    if (sh & 1) {
#pragma unroll
                        for (int m = 0; m < 4; ++m) w[m] = (w[m] >> 16) | (w[m + 1] << 16);
                    }
                    *dst = make_uint4(w[0], w[1], w[2], w[3]);
                } else {                                       // only the moved tokens are written
                    bf16_t *d16 = reinterpret_cast<bf16_t *>(dst);
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (g + k >= t0 && g + k < nl) d16[k] = (bf16_t)(w[k >> 1] >> ((k & 1) * 16));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < EVICT_V_ITEMS; ++i) { ca[i] = na[i]; cb[i] = nb[i]; cm[i] = nm[i]; }
    }
}
hipError_t kv_evict_ranges_launch(const KvPool &kv, int layers, const KvEvictTable *tab_dev, int n_seg, int64_t len, hipStream_t st) {
    if (kv.dtype != VLO_KV_BF16) return hipErrorNotSupported;
    if (!tab_dev || n_seg < 1 || n_seg > VLO_EVICT_MAX_RANGES) return hipErrorInvalidValue;
    const KvGeom &g = kv;
    if (kv.head_dim == 128)
        hipLaunchKernelGGL(kv_evict_ranges_kernel<128>, dim3(kv.num_kv_heads * 3, layers), dim3(256), 0, st, g, tab_dev, n_seg, (long long)len);
    else if (kv.head_dim == 64)
        hipLaunchKernelGGL(kv_evict_ranges_kernel<64>, dim3(kv.num_kv_heads * 2, layers), dim3(256), 0, st, g, tab_dev, n_seg, (long long)len);
    else
        return hipErrorNotSupported;
    return hipGetLastError();
}

// Per-row statistics of a bf16 logits matrix [n][ld] (one block per row): everything stream_evaluate reads from the
// logits (models/modeling_live.py:95-97, 107-112, 140-144) without materialising softmax rows:
//   lse[r]          log sum exp (fp32)                  -> cross entropy = lse - label_logit
//   argmax[r]       first maximum of the logits         (:97)
//   label_logit[r]  logits[r][labels[r]] (0 when the label is outside [0, V))
//   p_interval[r]   softmax(logits)[interval] rounded to bf16 as the reference's bf16 softmax does (:107,:110)
//   p_argmax[r]     first maximum of the bf16-rounded softmax row (:112; rounding can merge near-ties into exact ties,
//                   which argmax then resolves to the lower index — not always the logits' argmax)
__global__ __launch_bounds__(256) void logit_rows_kernel(const bf16_t *__restrict__ logits, int V, int64_t ld,
                                                         const int64_t *__restrict__ labels, int interval_id, float *__restrict__ lse,
                                                         int64_t *__restrict__ amax, float *__restrict__ label_logit,
                                                         float *__restrict__ p_interval, int64_t *__restrict__ p_amax) {
    __shared__ float sm[16];
    __shared__ float smv[16];
    __shared__ int smi[16];
    const bf16_t *x = logits + (size_t)blockIdx.x * ld;
    float mx = -INFINITY;
    ArgBest b = {-INFINITY, 0x7fffffff};
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        const float v = bf2f(x[i]);
        mx = fmaxf(mx, v);
        if (v > b.v) { b.v = v; b.i = i; }
    }
    const float M = block_max(mx, sm);
    float s = 0.f;
    for (int i = threadIdx.x; i < V; i += blockDim.x) s += expf(bf2f(x[i]) - M);
    const float S = block_sum(s, sm);
    b = block_argbest(b, smv, smi);
    ArgBest pb = {-INFINITY, 0x7fffffff};
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        const float p = rbf(expf(bf2f(x[i]) - M) / S);
        if (p > pb.v) { pb.v = p; pb.i = i; }
    }
    pb = block_argbest(pb, smv, smi);
    if (threadIdx.x == 0) {
        const int r = blockIdx.x;
        lse[r] = M + logf(S);
        amax[r] = b.i;
        const int64_t lab = labels ? labels[r] : -1;
        label_logit[r] = (lab >= 0 && lab < V) ? bf2f(x[lab]) : 0.f;
        p_interval[r] = (interval_id >= 0 && interval_id < V) ? rbf(expf(bf2f(x[interval_id]) - M) / S) : 0.f;
        p_amax[r] = pb.i;
    }
}
hipError_t logit_rows_launch(const unsigned short *logits, int n, int V, int64_t ld, const int64_t *labels, int interval_id, float *lse,
                             int64_t *amax, float *label_logit, float *p_interval, int64_t *p_amax, hipStream_t st) {
    hipLaunchKernelGGL(logit_rows_kernel, dim3(n), dim3(256), 0, st, logits, V, ld, labels, interval_id, lse, amax, label_logit,
                       p_interval, p_amax);
    return hipGetLastError();
}
