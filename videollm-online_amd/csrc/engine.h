// engine.h — internal structures behind the opaque vlo_engine / vlo_session handles
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vlo.h"
#include "gemv.h"
#include "prefill.h"

struct RawTensor {
    void *ptr = nullptr;
    int dtype = 0;
    std::vector<int64_t> shape;
};

struct PackedLinear {
    void *Wp = nullptr;
    int N = 0, K = 0, NT = 0;
    int NT_gemm = 0;          // tiles the image is ALLOCATED (and zero-filled) for: NT rounded up to 16 where a GEMM reads whole 256-column tiles of a
                              // width that is not one (a TP rank's lm_head shard: 16 032 -> 16 128 columns); 0 = NT
    int wq = 0;               // 1: Wp is the fp8 e4m3 image (gemv.hip) and wscale holds the per-output-channel scales; 2: the mxfp4 image + wblk
    float *wscale = nullptr;  // fp32 [NT * 16], packed row order
    unsigned *wblk = nullptr; // wq = 2: the e8m0 block scales, one dword per weight register and row: [NT][K / 128][16] (gemv.hip)
    GemvPlan plan{};
    Gemm64Plan plan64{};      // the 64-token block path over the same packed image (prefill.hip)
};

struct LayerWeights {
    PackedLinear qkv, o, gate_up, down;
    void *ln_in = nullptr, *ln_post = nullptr;
};

struct VitState;

// Prefill workspaces (~275 MB per set at the 8B shape, + the fp8 scratches, + 64 MiB of partials under TP) are pooled per engine: a destroyed
// session hands its set back, the next session that needs one takes it.  The pool keeps at most VLO_PREFILL_POOL_MAX idle sets — more are freed
// on release — so the resident cost is bounded by (live sessions that ran a prefill) + 2 sets.  A pooled set's spare rows hold whatever the
// last block left there: finite or not, they are computed and dropped (no output row depends on another row's X).
#define VLO_PREFILL_POOL_MAX 2
struct PrefillWs {
    unsigned short *ph = nullptr, *px = nullptr, *pqkv = nullptr, *pq = nullptr, *pact = nullptr;
    void *wexp = nullptr;
    size_t wexp_bytes = 0;
    float *partial = nullptr;
    void *xq = nullptr;
};

#define VLO_EVICT_SLOTS 4            // ring of vlo_session_evict_ranges table buffers (see vlo_engine)
struct vlo_engine {
    vlo_config cfg{};
    int device = 0;
    int head_dim = 0;
    // tensor-parallel shard of this engine (== the global dims when tp_size == 1): q heads, kv heads, MLP columns,
    // vocabulary rows owned by this rank (HF tp plan: q/k/v/gate/up column-wise, o/down row-wise, lm_head column-wise)
    int tp_rank = 0, tp_size = 1;
    int nh_l = 0, nkv_l = 0, I_l = 0, V_l = 0;
    bool finalized = false;
    bool has_connector = false;
    std::map<std::string, RawTensor> raw;      // row-major weights staged on the device until finalize
    std::vector<void *> owned;                 // device allocations freed at destroy
    int64_t weight_bytes = 0;

    std::vector<LayerWeights> layers;
    PackedLinear lm_head, conn0, conn2;
    void *norm_w = nullptr, *embed = nullptr, *conn0_b = nullptr, *conn2_b = nullptr;
    void *conn_x = nullptr, *conn_mid = nullptr, *conn_out = nullptr;   // connector scratch: 2 slots of 32 rows each (two encode branches may run concurrently)
    void *cos_tab = nullptr, *sin_tab = nullptr;
    int64_t max_positions = 0;
    std::vector<float> inv_freq_h;               // the inv_freq the tables were built from (loaded "rope.inv_freq" or the powf() one): vlo_session_evict

    // paged KV pool (bf16, or one e4m3 byte per element when cfg.kv_dtype = 1)
    void *k_pool = nullptr, *vt_pool = nullptr;
    std::vector<float> kv_scale_h;               // kv_dtype = 1: [layer][2] {k_scale, v_scale} as loaded (1.0 when not), device copy kv_scale
    float *kv_scale = nullptr;
    int pool_pages = 0;
    int64_t page_elems = 0, layer_stride = 0;
    std::vector<int> free_pages;
    std::mutex pool_mu;

    // vlo_session_evict_ranges: the segment / (c, s) table of a call changes with every call and is too large for kernel arguments.  As a
    // batch's step tables (vlo_batch): slot k is written on the host (pinned evict_stage[k]), copied to evict_dev[k] on the call's stream and read
    // by its kernel; evict_ev[k], recorded behind the kernel, must have completed before the host rewrites the slot.  Allocated on first use,
    // guarded by evict_mu (sessions of one engine may evict from threads and streams of their own)
    KvEvictTable *evict_stage = nullptr, *evict_dev = nullptr;
    hipEvent_t evict_ev[VLO_EVICT_SLOTS] = {};
    bool evict_used[VLO_EVICT_SLOTS] = {};
    int evict_slot = 0;
    std::mutex evict_mu;


    VitState *vit = nullptr;
    void *ingest = nullptr;                      // ingest.hip: cached tap tables + scratch of vlo_frame_ingest

    // prefill-path workspaces (~275 MB at the 8B shape, + the fp8 expansion scratch) are POOLED per engine: a session takes a set at its first
    // prefill block and hands it back when it is destroyed — stream_evaluate forks a session per turn, serving holds many sessions; each set is
    // allocated (hipMalloc + a blocking memset) once and owned by exactly one session at a time (sessions step on streams of their own).
    // Guarded by pool_mu; freed with the engine.
    std::vector<PrefillWs> prefill_free;

    // live timing of the dominant kernel (vlo_profile_*)
    int prof_stride = 0;
    int64_t prof_seen = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;   // pool
    size_t prof_used = 0;
    int64_t prof_launches = 0;
    double prof_ms = 0.0;
};

// What one pass over the decoder layers writes (engine.hip decoder_layers).  The 16-row pipeline keeps every matrix row-major; the 64-token
// block path keeps x, attn and act packed-64 (llm_ops.h) and does not use partial / sq.
struct StepWs {
    unsigned short *h = nullptr, *x = nullptr, *q = nullptr, *attn = nullptr, *act = nullptr;   // residual stream, normed rows, q after RoPE, attention out, MLP act
    float *partial = nullptr;                    // down-proj split-K partial sums [ksplit][16][H], combined by the next add_rmsnorm
    float *sq[2] = {nullptr, nullptr};           // row sum-of-squares partials handed from EPI_RESID to XSRC_NORM
    float *part_o = nullptr, *part_ml = nullptr; // split-KV attention partial states: part_cap of [nh][16][hd] / [nh][16][2] floats
    int part_cap = 0;
};

struct vlo_session {
    vlo_engine *e = nullptr;
    int64_t len = 0;
    bool has_logits = false;
    std::vector<int> pages;
    std::vector<void *> owned;
    StepWs ws;                                   // the 16-row pipeline's set (h, x, act, attn: 32 rows; q: 16)
    StepWs bws;                                  // the 64-token block path's set: allocated on first use, shares ws's attention partials
    unsigned short *emb1 = nullptr;
    unsigned short *logits = nullptr, *last_logits = nullptr;
    unsigned short *logits_local = nullptr;      // TP: this rank's vocabulary shard [16][V_l]
    float *partial_o = nullptr;                  // TP: o_proj partial sums [16][H] awaiting the all-reduce
    int64_t *tok = nullptr;
    float *sample_scratch = nullptr;
    // stream lookahead (vlo_stream_steps): a pass of pend_units > 0 units has appended K / V behind `len` and awaits vlo_stream_steps_commit;
    // until then `len` is the length before the pass, unit k ends at row pend_end[k] and `logits` holds the unit-end rows [pend_units][vocab]
    int pend_units = 0;
    int pend_end[VLO_ROWIDX_MAX] = {};
    float *steps_scratch = nullptr;              // the rows sampler's scratch [VLO_ROWIDX_MAX][VLO_SAMPLE_SCRATCH_FLOATS]: allocated on first use
    int64_t *host_tok = nullptr;                 // pinned, 8 slots: tokens read back by the greedy loop (double-buffered)
    hipEvent_t tok_ev[2] = {nullptr, nullptr};   // "token i is on the host" (created on first use)
    int *page_table = nullptr, *host_pt = nullptr;
    // workspaces of the prefill path (blocks of up to VLO_PREFILL_TOKENS tokens as real GEMMs, prefill.h; allocated on first use):
    // residual stream, normed rows / attention output (the GEMMs' X operand: 256 spare rows), qkv projection, q after RoPE, MLP act
    unsigned short *ph = nullptr, *px = nullptr, *pqkv = nullptr, *pq = nullptr, *pact = nullptr;
    float *ppart_o = nullptr, *ppart_ml = nullptr;   // attention partials of a whole prefill block (VLO_PREFILL_TOKENS / 16 sub-chunk states): only for the fallback kernel
    // prefill path of an fp8 engine: bf16 expansion of ONE projection's image (the largest), rewritten before each GEMM.  Per SESSION: sessions
    // step on streams of their own, a scratch shared through the engine would be overwritten under another session's GEMM
    void *pf_wexp = nullptr;
    size_t pf_wexp_bytes = 0;
    // prefill_act_dtype = 1: the e4m3 codes of ONE projection's X operand ([VLO_PREFILL_TOKENS + 256][widest layer K] bytes) followed by its
    // row scales ([VLO_PREFILL_TOKENS + 256] floats), rewritten before each GEMM (prefill.h::quantize_rows_fp8_launch)
    void *pxq = nullptr;
    unsigned short *plogits = nullptr;           // TP prefill, every row's logits: this rank's PADDED vocabulary shard of one row chunk, bf16 [VLO_TP_LOGIT_ROWS][NT_gemm * 16]
    float *ppartial = nullptr;                   // TP prefill: this rank's o-proj / down-proj partial sums fp32 [VLO_PREFILL_TOKENS][H] awaiting the all-reduce
};

// ---- batched steps (vlo_batch_*): the rows of up to VLO_BATCH_MAX sessions in one weight pass ------------------------------------------
#define VLO_BATCH_MAX 16
#define VLO_BATCH_SLOTS 4           // ring of per-step table buffers (see vlo_batch)
// the per-step tables every layer of a batched step reads: the qkv epilogue's row table (EPI_ROPE_ROWS) and the attention segments
struct BatchTables {
    RopeRow rows[VLO_BLOCK_TOKENS];
    AttnSeg segs[VLO_ATTN_SEG_MAX];
};
struct vlo_batch {
    vlo_engine *e = nullptr;
    int max_sessions = 0;
    std::vector<void *> owned;
    StepWs ws;                                   // up to 64 rows, serving both layouts; part_cap = max_sessions * attention_states_bound(nkv)
    unsigned short *xl = nullptr;                // [16][H]: the normed last row of each session, the lm_head's input
    unsigned short *emb = nullptr;               // [16][H]: the next step's input rows of the greedy loop
    unsigned short *logits = nullptr;            // [max_sessions][V]: row b = session b of the last step
    float *sample_scratch = nullptr;             // [max_sessions][VLO_SAMPLE_SCRATCH_FLOATS]
    int64_t *tok = nullptr;                      // [max_sessions]
    int64_t *host_tok = nullptr;                 // pinned [VLO_BATCH_MAX]
    // the tables change every step: slot k is written on the host (pinned stage[k]), copied to tables_dev[k] on the step's stream and read by
    // its kernels; slot_ev[k], recorded behind the step's last launch, must have completed before the host rewrites stage[k] (the queued copy
    // of a step still in flight reads it) — with VLO_BATCH_SLOTS slots the host waits only when it runs that many steps ahead
    BatchTables *stage = nullptr, *tables_dev = nullptr;
    hipEvent_t slot_ev[VLO_BATCH_SLOTS] = {};
    bool slot_used[VLO_BATCH_SLOTS] = {};
    int slot = 0;
    int last_B = 0;                              // rows of `logits` written by the last vlo_batch_step (0: none)
};

int dev_alloc(void **p, size_t bytes);
// helpers shared with tp.hip
int ensure_pages(vlo_session *s, int64_t new_len, hipStream_t st);
GemvArgs gemv_args(const PackedLinear &pl, const unsigned short *x, int ldx, int n_rows);
GemvArgs qkv_args(const vlo_engine *e, int layer, const StepWs &w, int n_rows, int64_t pos0);   // w.x -> w.q; the epilogue comes from rope_epi
KvPool kv_geom(const vlo_session *s);
// the qkv projection's append target: sets a.kv (+ a.kv_scale) and returns the epilogue, EPI_ROPE or EPI_ROPE_F8
inline int rope_epi(GemvArgs &a, const KvPool &kv) {
    a.kv = kv;
    if (kv.dtype != VLO_KV_FP8) return EPI_ROPE;
    a.kv_scale = kv.scale;
    return EPI_ROPE_F8;
}
int ensure_prefill_ws(vlo_session *s);                        // prefill-path workspaces of a session (sized for the engine's shard)
bool prefill_ok(const vlo_engine *e);                         // do this engine's (shard) shapes take the prefill GEMMs
// layer_proj: a decoder-layer projection (takes the native fp8 MFMA when the engine asks for it); false = the lm_head (bf16 activations always)
int prefill_gemm(vlo_session *s, const unsigned short *X, const PackedLinear &pl, int m, int N, int K, void *out, int ldo, int kind, hipStream_t st,
                 bool layer_proj = true);
void ingest_create(vlo_engine *e);
void ingest_destroy(vlo_engine *e);
int connector_run(vlo_engine *e, int slot, const void *feats_dev, int rows, void *out_dev, hipStream_t st);   // slot 0 / 1: scratch set
int session_fork_shard(vlo_session *src, int64_t n_tokens, vlo_session **out, void *stream);   // one KV shard (engine.hip)
int session_crop_shard(vlo_session *s, int64_t n_tokens);
int session_evict_shard(vlo_session *s, int64_t t0, int64_t t1, void *stream);
// vlo_session_evict_ranges in two halves, so that a tensor-parallel call is validated as a whole before any shard moves: evict_ranges_normalize
// checks `ranges_host` ([n][2], 0 <= a <= b <= len, ascending, non-overlapping) and returns the non-empty ranges with touching ones merged
// (at most VLO_EVICT_MAX_RANGES, else VLO_E_INVALID); session_evict_ranges_shard evicts such a list from ONE KV shard
int evict_ranges_normalize(const int64_t *ranges_host, int n, int64_t len, std::vector<std::pair<int64_t, int64_t>> *out);
int session_evict_ranges_shard(vlo_session *s, const std::vector<std::pair<int64_t, int64_t>> &ranges, void *stream);
int vlo_fail(int code, const std::string &msg);   // sets the thread-local error string, returns code
