// llm_ops.h — host-visible launchers of llm_ops.hip (Llama step kernels other than the GEMVs)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VLO_PAGE_TOKENS 256      // tokens per KV page (multiple of 32)
#define VLO_MAX_SPLITS 64        // max KV splits of the attention kernel

// Paged KV pool geometry.  One page id addresses, for every layer, a K block
// [kvh][PAGE][hd] and a V^T block [kvh][hd][PAGE] (V is stored transposed so the
// P.V MFMA can take it as an A operand straight from HBM).
struct KvGeom {
    unsigned short *k_pool;      // [layer][page][kvh][PAGE][hd]   bf16
    unsigned short *vt_pool;     // [layer][page][kvh][hd][PAGE]   bf16
    const int *page_table;       // logical page -> physical page (device)
    int64_t layer_stride;        // elements between layers  (= pool_pages * page_elems)
    int64_t page_elems;          // kvh * PAGE * hd
    int num_kv_heads, head_dim;
};

// KV storage formats (vlo_config.kv_dtype)
enum { VLO_KV_BF16 = 0, VLO_KV_FP8 = 1 };
// Host-side view of a session's pool: the geometry every kernel takes (KvGeom, whose layout the bf16 kernels' ISA depends on) plus the
// storage format.  VLO_KV_FP8: k_pool / vt_pool hold one OCP e4m3 byte per element at the SAME element offsets (layer_stride and page_elems
// count elements), and `scale` is the device array [layer][2] = {k_scale, v_scale}; code = e4m3_rne(clamp(x / scale, -448, 448)).
struct KvPool : KvGeom {
    int dtype = VLO_KV_BF16;
    const float *scale = nullptr;
};

// "packed-64" activation layout of the 64-token block path (prefill.hip): the B-operand fragments of
// v_mfma_f32_16x16x32_bf16 stored contiguously, so one fragment load is one coalesced 1 KiB read instead of 16 half-used
// cache lines of a row-major matrix.  Element (row < 64, k) lives at
//   ((k / 32 * 4 + row / 16) * 64 + (k % 32 / 8) * 16 + row % 16) * 8 + k % 8
__host__ __device__ inline size_t vlo_pack64_elem(int row, int k) {
    return ((size_t)((k >> 5) * 4 + (row >> 4)) * 64 + (size_t)(((k & 31) >> 3) * 16 + (row & 15))) * 8 + (k & 7);
}

// h[m] (+)= bf16(sum_s partial[s][m]) ; x[m] = RMSNorm(h[m]) * w     (rows m < n).  ldx == 0: x is written packed-64.
hipError_t add_rmsnorm_launch(unsigned short *h, const float *partial, int ksplit, int partial_ld,
                              const unsigned short *w, unsigned short *x, int H, int ldx, float eps, int n,
                              hipStream_t st);

// the same for `count` <= VLO_ROWIDX_MAX SELECTED rows (the row indices travel in the kernel arguments): x16[k] = RMSNorm(h[rows.v[k]]) * w,
// row-major [count][H], each row bit-equal to what add_rmsnorm_launch writes for it (the pending partial sums are folded into those rows of h
// first); the other rows of h (n_rows in all: the bound the indices are checked against) are left as they are
#define VLO_ROWIDX_MAX 16
struct RowIdx { int v[VLO_ROWIDX_MAX]; };
hipError_t add_rmsnorm_gather_launch(unsigned short *h, const float *partial, int ksplit, int partial_ld, const unsigned short *w,
                                     unsigned short *x16, int H, float eps, const RowIdx &rows, int count, int n_rows, hipStream_t st);

// copy `rows` embedding rows into the residual stream h and write their sums of squares to sq_out[0..rows)

// chunk attention (n <= 16 queries at positions pos0..pos0+n-1 against keys [0, pos0+n); the block path passes n <= 64
// = up to four 16-query sub-chunks in one launch)
// pack_row0 >= 0: `out` is a packed-64 matrix and query i goes to row pack_row0 + i (block path); -1: row-major [n][nh*hd]
// part_cap: capacity of part_o / part_ml in (16-query sub-chunk x split) partial states of [nh][16][hd] / [nh][16][2] floats: the
// session's buffers hold VLO_MAX_SPLITS (n <= 64); the prefill path brings VLO_PREFILL_TOKENS / 16 and runs a whole block of new
// tokens as ONE launch (grid.z = its 16-query sub-chunks, one split each)
hipError_t attention_launch(const unsigned short *q, const KvPool &kv, int layer, int num_heads, int64_t pos0, int n,
                            float *part_o, float *part_ml, unsigned short *out, hipStream_t st, int pack_row0 = -1, int part_cap = VLO_MAX_SPLITS);

// flash-style attention for a block of n new tokens at positions pos0 .. pos0 + n - 1 whose keys are already appended (prefill path):
// out bf16 [n][nh * hd] row-major.  hipErrorNotSupported for GQA shapes it is not instantiated for (the caller uses attention_launch).
// The flash kernels read bf16 pools only: an fp8 pool takes attention_launch.
bool attention_prefill_supported(int head_dim, int gqa_group, int kv_dtype);   // is attn_prefill_kernel instantiated for this shape (else attention_prefill_launch returns hipErrorNotSupported)
hipError_t attention_prefill_launch(const unsigned short *q, const KvPool &kv, int layer, int num_heads, int64_t pos0, int n, unsigned short *out,
                                    hipStream_t st);

// launch geometry of the chunk attention for n new tokens at cache length pos0 (what attention_launch computes first)
struct AttnGeom { int G, KS, hpw, nhg, nz, chunk, nsplit, nct; float scale; size_t lds_bytes; };
hipError_t attention_geometry(const KvGeom &kv, int num_heads, int64_t pos0, int n, AttnGeom *g, int part_cap = VLO_MAX_SPLITS);

// ---- batched steps (engine.hip vlo_batch_step): rows of several sessions in one launch ----------------------------------------------
// One SEGMENT = one 16-query sub-chunk of one session: its own page table, cache position, query count, the split geometry that
// attention_geometry gives that session stepped ALONE (so a batched row equals the solo row bit for bit), its first q / output row and
// its first partial state.  The table lives in device memory (uploaded once per batch step, read by every layer).
struct AttnSeg {
    const int *page_table;       // the session's logical -> physical page table (device)
    long long pos0;              // position of the sub-chunk's first query
    int n;                       // queries (1..16)
    int chunk, nsplit;           // the solo launch's split geometry
    int row0;                    // first query row in q (row-major [rows][nh * hd]) and first output row (row-major, or packed-64 row)
    int part0;                   // first partial state (units of [nh][16][hd] floats / [nh][16][2] floats)
    int pad_;
};
// a run of segments whose solo launches take the same kernel (g.nct: attn_cols NCT, 0 = attn_chunk); max_nsplit = the launch's grid.x
struct AttnSegRun { int first, count, max_nsplit; AttnGeom g; };
#define VLO_ATTN_SEG_MAX 20      // segments of one batch step: <= 16 sessions, <= 64 rows (sum of ceil(n_b / 16) <= 16 + 3)
// split states one session of n new tokens may take in the launch attention_geometry plans for it (the batch's partial buffers hold this many
// per session)
int attention_states_bound(int num_kv_heads);
// plans the segments of B sessions (tables[b], lens[b] = cache length before the step, ns[b] new tokens, rows[b] = first row), grouped by
// kernel family: segs[0 .. *nseg) (host copy of the device table), runs[0 .. *nrun), *states = partial states used.  part_cap: states available
hipError_t attention_seg_plan(const KvGeom &kv, int num_heads, int B, const int *const *tables, const int64_t *lens, const int *ns,
                              const int *rows, int part_cap, AttnSeg *segs, int *nseg, AttnSegRun *runs, int *nrun, int *states);
// the planned launches + one segmented combine.  segs_dev = the device copy of the planned table; packed: `out` is packed-64 (block path)
hipError_t attention_seg_launch(const unsigned short *q, const KvPool &kv, int layer, int num_heads, const AttnSeg *segs_dev, int nseg,
                                const AttnSegRun *runs, int nrun, float *part_o, float *part_ml, unsigned short *out, bool packed, hipStream_t st);
// dst[i][0 .. cols) = src[i][0 .. cols) for i < count (bf16 rows anywhere in device memory, 16-byte aligned, cols % 8 == 0): gathers the
// last row of each session of a batch, scatters the batch's logits rows to the sessions
#define VLO_ROWCOPY_MAX 16
struct RowCopy { const unsigned short *src[VLO_ROWCOPY_MAX]; unsigned short *dst[VLO_ROWCOPY_MAX]; };
hipError_t copy_rows_indexed_launch(const RowCopy &rc, int count, int cols, hipStream_t st);

hipError_t embed_gather_launch(const unsigned short *table, const int64_t *ids, int k, int H, int64_t vocab,
                               unsigned short *out, hipStream_t st);

// samplers on bf16 logits [V]
#define VLO_SAMPLE_SCRATCH_FLOATS 512     // >= 6 * SAMPLE_BLOCKS + 1
// `scratch`: VLO_SAMPLE_SCRATCH_FLOATS floats of device memory owned by the session
hipError_t greedy_sample_launch(const unsigned short *logits, int V, int64_t *tok_out, int eos, int force_mode,
                                float *scratch, hipStream_t st);
hipError_t stream_sample_launch(const unsigned short *logits, int V, float threshold, int interval_id,
                                int64_t *tok_out, float *p_interval_out, float *scratch, hipStream_t st);
// the same for `rows` rows of bf16 logits [rows][V] in one launch sequence (grid.y = row; scratch: VLO_SAMPLE_SCRATCH_FLOATS per row,
// tok_out / p_interval_out: one entry per row); each row's reduction order is the solo kernels', so its result equals theirs bit for bit
hipError_t greedy_sample_rows_launch(const unsigned short *logits, int rows, int V, int64_t *tok_out, float *scratch, hipStream_t st);
hipError_t stream_sample_rows_launch(const unsigned short *logits, int rows, int V, float threshold, int interval_id, int64_t *tok_out,
                                     float *p_interval_out, float *scratch, hipStream_t st);

// stream_sample_rows_launch for the unit-end rows of a lookahead pass (rows <= VLO_ROWIDX_MAX) with the first-speaker reduction folded into
// the finishing launch: *n_accept_out (device int) = (smallest r with tok[r] != interval_id) + 1, or rows when every row stays silent
hipError_t stream_sample_steps_launch(const unsigned short *logits, int rows, int V, float threshold, int interval_id, int64_t *tok_out,
                                      float *p_interval_out, int *n_accept_out, float *scratch, hipStream_t st);

#define VLO_STEP_IDS_MAX 32
struct StepIds { int64_t v[VLO_STEP_IDS_MAX]; };      // token ids handed to step_input_kernel by value (kernel arguments)
hipError_t step_input_launch(const unsigned short *table, const StepIds &ids, int k, const unsigned short *frame_rows, int rows, int H,
                             int64_t vocab, unsigned short *out, hipStream_t st);
// the multi-unit form: unit u has ids v[id0[u] .. id0[u + 1]) (at most VLO_STEP_IDS_MAX for unit 0, VLO_STEPS_IDS_LATER for each later one) and
// occupies output rows [row0[u], row0[u + 1]) = its id embeddings followed by frame rows [u * rows_per_unit, (u + 1) * rows_per_unit)
#define VLO_STEPS_UNITS_MAX 16
#define VLO_STEPS_IDS_LATER 4
struct StepsIds {
    int64_t v[VLO_STEP_IDS_MAX + (VLO_STEPS_UNITS_MAX - 1) * VLO_STEPS_IDS_LATER];
    int id0[VLO_STEPS_UNITS_MAX + 1], row0[VLO_STEPS_UNITS_MAX + 1];
};
hipError_t steps_input_launch(const unsigned short *table, const StepsIds &ids, int units, const unsigned short *frame_rows, int rows_per_unit,
                              int H, int64_t vocab, unsigned short *out, hipStream_t st);
hipError_t copy_rows_launch(const unsigned short *src, unsigned short *dst, int rows, int H, hipStream_t st);
hipError_t read_kv_launch(const KvPool &kv, int layer, int which, int kv_head, int64_t t0, int64_t t1, unsigned short *dst,
                          hipStream_t st);

// ---- teacher-forced evaluation helpers (models/modeling_live.py:29-42, 44-168, 170-171)
// out[i] = ids[i] == v_id ? frame_rows[rank of i among placeholder positions] : table[clamp(ids[i])];
// *count_out (device int) = number of placeholder positions; src_idx_scratch: k device ints
hipError_t joint_embed_launch(const unsigned short *table, const int64_t *ids, int k, int64_t v_id, const unsigned short *frame_rows,
                              int n_frame_rows, int H, int64_t vocab, int *src_idx_scratch, int *count_out, unsigned short *out,
                              hipStream_t st);
// copy `pages` whole KV pages (all layers, K and V^T) from the physical pages src_pt[i] to dst_pt[i] (device int arrays); the page's BYTES
hipError_t kv_copy_pages_launch(const KvPool &kv, const int *src_pt, const int *dst_pt, int pages, int layers, hipStream_t st);
// vlo_session_evict on a bf16 pool (head_dim 64 or 128): tokens [t0 + d, len) of every layer move down by d slots in place (0 <= t0, d >= 1,
// t0 + d < len), K rotated back by d positions with rot = {(float)cos, (float)sin of (double)d * inv_freq[i]}, i < head_dim / 2 (kernel
// arguments), V^T moved bit for bit.  Reads kv.page_table up to the page of token len - 1.
struct KvEvictRot { float c[64], s[64]; };
hipError_t kv_evict_launch(const KvPool &kv, int layers, int64_t t0, int64_t d, int64_t len, const KvEvictRot &rot, hipStream_t st);
// vlo_session_evict_ranges on a bf16 pool (head_dim 64 or 128): n_seg survivor runs move down in ONE pass.  Segment j < n_seg is destination
// tokens [w[j], w[j + 1]) (ascending, non-empty; w[n_seg] = the new length), each read from w + D[j] (1 <= D[0] < D[1] < ..., w[n_seg] +
// D[n_seg - 1] = len) with K rotated back by D[j] positions: c[j][i], s[j][i] = (float)cos, (float)sin of (double)D[j] * inv_freq[i],
// i < head_dim / 2 — kv_evict_launch's arithmetic, so n_seg = 1 gives its result bit for bit.  V^T moves bit for bit; tokens below w[0] are
// untouched.  `tab_dev` is DEVICE memory that stays valid and unchanged until the kernel has run.
#define VLO_EVICT_MAX_RANGES 64      // = include/vlo.h
struct KvEvictTable {
    long long w[VLO_EVICT_MAX_RANGES + 1], D[VLO_EVICT_MAX_RANGES];
    float c[VLO_EVICT_MAX_RANGES][64], s[VLO_EVICT_MAX_RANGES][64];
};
hipError_t kv_evict_ranges_launch(const KvPool &kv, int layers, const KvEvictTable *tab_dev, int n_seg, int64_t len, hipStream_t st);
// per-row logit statistics, see llm_ops.hip
hipError_t logit_rows_launch(const unsigned short *logits, int n, int V, int64_t ld, const int64_t *labels, int interval_id, float *lse,
                             int64_t *amax, float *label_logit, float *p_interval, int64_t *p_amax, hipStream_t st);
