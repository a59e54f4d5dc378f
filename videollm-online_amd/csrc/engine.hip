// engine.hip — host side of libvlo.so: the C ABI declared in include/vlo.h.
//
// Owns: packed weights in HBM, the paged KV pool, per-session workspaces; sequences the
// gfx950 kernels of one Llama streaming step (gemv.hip, llm_ops.hip) and of the SigLIP
// encode (vit.hip) on caller-provided HIP streams.  No torch types, no CPU fallback:
// every entry point either runs the HIP path or returns an error.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vlo.h"
#include "common.cuh"
#include "engine.h"
#include "gemv.h"
#include "llm_ops.h"
#include "vit.h"

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int vlo_fail(int code, const std::string &msg) { return fail(code, msg); }
const char *vlo_last_error(void) { return g_err.c_str(); }
int vlo_abi_version(void) { return VLO_ABI_VERSION; }
#ifndef VLO_BUILD_ID
#define VLO_BUILD_ID "unstamped"
#endif
const char *vlo_build_id(void) { return "VLO_BUILD_ID=" VLO_BUILD_ID; }

#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess)                                                                                 \
            return fail(VLO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " @" + __FILE__ + ":" + \
                                       std::to_string(__LINE__));                                             \
    } while (0)

// ------------------------------------------------------------------------------------
// small device utilities
// ------------------------------------------------------------------------------------
__global__ void convert_kernel(const void *src, int sdt, void *dst, int ddt, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v;
        if (sdt == VLO_DT_F32) v = ((const float *)src)[i];
        else if (sdt == VLO_DT_BF16) v = bf2f(((const bf16_t *)src)[i]);
        else v = h2f(((const f16_t *)src)[i]);
        if (ddt == VLO_DT_F32) ((float *)dst)[i] = v;
        else if (ddt == VLO_DT_BF16) ((bf16_t *)dst)[i] = f2bf(v);
        else ((f16_t *)dst)[i] = f2h(v);
    }
}
__global__ void sum_partials_kernel(const float *P, int ksplit, int ld, float *y, int n, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * N) return;
    const int m = i / N, c = i % N;
    float s = 0.f;
    for (int k = 0; k < ksplit; ++k) s += P[((size_t)k * 16 + m) * ld + c];
    y[i] = s;
}

static size_t dt_size(int dt) { return dt == VLO_DT_F32 ? 4 : (dt == VLO_DT_FP8_E4M3 || dt == VLO_DT_E8M0 ? 1 : 2); }

int dev_alloc(void **p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
    return VLO_OK;
}
// allocate, zero, remember: device memory for *p that is freed with its owner (`owned`).  Chains through rc: nothing happens after an earlier
// failure, and a buffer that exists (kept from an earlier, partly failed attempt) stays
template <typename T>
static void alloc_owned(int &rc, std::vector<void *> &owned, T **p, size_t bytes, bool zero = true) {
    if (rc || *p) return;
    void *q = nullptr;
    if ((rc = dev_alloc(&q, bytes))) return;
    owned.push_back(q);
    if (zero) hipMemset(q, 0, bytes);
    *p = (T *)q;
}
// the activations of a StepWs for up to VLO_BLOCK_TOKENS rows (a session's block set, a batch's set)
static void alloc_block_rows(int &rc, std::vector<void *> &owned, const vlo_engine *e, StepWs &w, bool zero) {
    const size_t H = e->cfg.hidden_size, I = e->I_l, qd = (size_t)e->nh_l * e->head_dim, R = VLO_BLOCK_TOKENS;
    alloc_owned(rc, owned, &w.h, R * H * 2, zero);
    alloc_owned(rc, owned, &w.x, R * H * 2, zero);
    alloc_owned(rc, owned, &w.q, R * qd * 2, zero);
    alloc_owned(rc, owned, &w.attn, R * qd * 2, zero);
    alloc_owned(rc, owned, &w.act, R * I * 2, zero);
}

// ------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------
static bool name_is(const std::string &n, const char *suffix) {
    const size_t l = strlen(suffix);
    return n.size() >= l && n.compare(n.size() - l, l, suffix) == 0;
}

int vlo_engine_create(const vlo_config *cfg, int device, vlo_engine **out) {
    if (!cfg || !out) return fail(VLO_E_INVALID, "null argument");
    if (cfg->abi_version != VLO_ABI_VERSION) return fail(VLO_E_INVALID, "vlo_config.abi_version mismatch");
    if (cfg->hidden_size <= 0 || cfg->num_heads <= 0 || cfg->num_kv_heads <= 0 || cfg->hidden_size % cfg->num_heads ||
        cfg->num_heads % cfg->num_kv_heads || cfg->num_layers <= 0 || cfg->vocab_size <= 0 || cfg->intermediate_size <= 0)
        return fail(VLO_E_INVALID, "bad Llama dimensions");
    const int hd = cfg->hidden_size / cfg->num_heads;
    if (hd != 64 && hd != 128) return fail(VLO_E_UNSUPPORTED, "head_dim must be 64 or 128");
    if (cfg->weight_dtype < 0 || cfg->weight_dtype > 2) return fail(VLO_E_INVALID, "weight_dtype must be 0 (bf16), 1 (fp8 e4m3) or 2 (mxfp4)");
    if (cfg->prefill_act_dtype != 0 && !(cfg->prefill_act_dtype == 1 && cfg->weight_dtype == 1))
        return fail(VLO_E_INVALID, "prefill_act_dtype must be 0 (bf16), or 1 (fp8 e4m3 per-row-scaled, native fp8 MFMA) on an engine with weight_dtype = 1");
    if (cfg->kv_dtype != VLO_KV_BF16 && cfg->kv_dtype != VLO_KV_FP8) return fail(VLO_E_INVALID, "kv_dtype must be 0 (bf16) or 1 (fp8 e4m3)");
    if ((cfg->hidden_size & 31) || (cfg->intermediate_size & 31) || (cfg->vocab_size & 3))
        return fail(VLO_E_UNSUPPORTED, "hidden/intermediate must be multiples of 32, vocab of 4");
    const int T = cfg->tp_size > 1 ? cfg->tp_size : 1;
    if (T > 1) {
        if (cfg->tp_rank < 0 || cfg->tp_rank >= T) return fail(VLO_E_INVALID, "tp_rank out of range");
        if (cfg->num_kv_heads % T || cfg->num_heads % T || cfg->intermediate_size % (T * 32) || cfg->vocab_size % (T * 16))
            return fail(VLO_E_UNSUPPORTED, "tp_size must divide kv heads, heads, intermediate_size/32 and vocab_size/16");
        if (T > 8) return fail(VLO_E_UNSUPPORTED, "tp_size > 8");
        if (cfg->weight_dtype == 2)
            return fail(VLO_E_UNSUPPORTED, "weight_dtype = 2 (mxfp4) with tp_size > 1: the mxfp4 GEMV has no plans for the shards' reduction lengths");
    }
    HIP_TRY(hipSetDevice(device));
    vlo_engine *e = new vlo_engine();
    e->cfg = *cfg;
    e->device = device;
    e->head_dim = hd;
    e->tp_size = T;
    e->tp_rank = T > 1 ? cfg->tp_rank : 0;
    e->nh_l = cfg->num_heads / T;
    e->nkv_l = cfg->num_kv_heads / T;
    e->I_l = cfg->intermediate_size / T;
    e->V_l = cfg->vocab_size / T;
    if (e->cfg.kv_pool_tokens <= 0) e->cfg.kv_pool_tokens = 16384;
    if (cfg->kv_dtype == VLO_KV_FP8) e->kv_scale_h.assign((size_t)cfg->num_layers * 2, 1.0f);
    ingest_create(e);
    *out = e;
    return VLO_OK;
}

void vlo_engine_destroy(vlo_engine *e) {
    if (!e) return;
    hipSetDevice(e->device);
    for (auto &kv : e->raw) hipFree(kv.second.ptr);
    for (void *p : e->owned) hipFree(p);
    for (const PrefillWs &w : e->prefill_free)
        for (void *p : {(void *)w.ph, (void *)w.px, (void *)w.pqkv, (void *)w.pq, (void *)w.pact, w.wexp, (void *)w.partial, w.xq}) if (p) hipFree(p);
    for (auto &pr : e->prof_events) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    if (e->evict_stage) hipHostFree(e->evict_stage);
    if (e->evict_dev) hipFree(e->evict_dev);
    for (hipEvent_t ev : e->evict_ev) if (ev) hipEventDestroy(ev);
    vit_destroy(e);
    ingest_destroy(e);
    delete e;
}

int64_t vlo_engine_weight_bytes(const vlo_engine *e) { return e ? e->weight_bytes : 0; }

int vlo_engine_load_weight(vlo_engine *e, const char *name, const void *data, int dtype, const int64_t *shape, int ndim) {
    if (!e || !name || !data || !shape || ndim < 1 || ndim > 4) return fail(VLO_E_INVALID, "bad load_weight arguments");
    if (e->finalized) return fail(VLO_E_STATE, "engine already finalized");
    HIP_TRY(hipSetDevice(e->device));
    const std::string n(name);
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    {   // static per-layer KV scales of an fp8 KV pool: "model.layers.{i}.self_attn.k_scale" / "v_scale" (vlo_config.kv_dtype)
        int layer = -1, pos = 0;
        char kv = 0;
        if (sscanf(name, "model.layers.%d.self_attn.%c_scale%n", &layer, &kv, &pos) == 2 && pos == (int)n.size() && (kv == 'k' || kv == 'v')) {
            if (e->cfg.kv_dtype != VLO_KV_FP8) return fail(VLO_E_INVALID, n + ": KV scales are accepted by an engine created with kv_dtype = 1");
            if (layer < 0 || layer >= e->cfg.num_layers || dtype != VLO_DT_F32 || numel != 1)
                return fail(VLO_E_INVALID, n + ": expected one f32 element of a layer < num_layers");
            float v = 0.f;
            HIP_TRY(hipMemcpy(&v, data, sizeof(float), hipMemcpyDefault));
            if (!std::isfinite(v) || !(v > 0.f)) return fail(VLO_E_INVALID, n + ": the scale must be finite and > 0");
            e->kv_scale_h[(size_t)layer * 2 + (kv == 'v')] = v;
            return VLO_OK;
        }
    }
    // storage dtype inside the engine: LLM + connector bf16; ViT matmul weights f16, the rest of the ViT f32
    int ddt = VLO_DT_BF16;
    if (n == "rope.inv_freq") ddt = VLO_DT_F32;
    const bool streamed = n.rfind("vision.", 0) != 0 && n.rfind("connector.", 0) != 0 &&
                          (name_is(n, "proj.weight") || n == "lm_head.weight" || name_is(n, "proj.weight_scale") || n == "lm_head.weight_scale");
    if (dtype == VLO_DT_FP4_E2M1X2 || dtype == VLO_DT_E8M0) {
        // mxfp4 storage of the streamed projections (vlo_config.weight_dtype = 2): e2m1 codes, two per byte, logical shape [N][K], and
        // "<name>_scale" e8m0 [N][K / 32]; quantised by the caller, kept as given
        if (e->cfg.weight_dtype != 2 || !streamed)
            return fail(VLO_E_INVALID, n + ": mxfp4 codes / e8m0 scales are accepted for the Llama projections of an engine created with weight_dtype = 2");
        if (name_is(n, "_scale") ? dtype != VLO_DT_E8M0 : dtype != VLO_DT_FP4_E2M1X2)
            return fail(VLO_E_INVALID, n + ": expected e2m1 codes (VLO_DT_FP4_E2M1X2) and e8m0 scales (VLO_DT_E8M0)");
        if (ndim != 2) return fail(VLO_E_INVALID, n + ": expected a matrix");
        const size_t bytes = dtype == VLO_DT_E8M0 ? numel : numel / 2;
        if (dtype == VLO_DT_FP4_E2M1X2 && (shape[1] & 31)) return fail(VLO_E_INVALID, n + ": K must be a multiple of the 32-element scale block");
        if (dtype == VLO_DT_E8M0) {             // checked before anything is allocated (the source may be host or device memory).  255 = NaN;
            std::vector<uint8_t> host(bytes);   // 0 and 1 would make the code 0.5 a bf16 sub-normal
            HIP_TRY(hipMemcpy(host.data(), data, bytes, hipMemcpyDefault));
            for (size_t i = 0; i < bytes; ++i)
                if (host[i] < 2 || host[i] > 254)
                    return fail(VLO_E_INVALID, n + ": e8m0 scale byte " + std::to_string((int)host[i]) + " outside [2, 254]");
        }
        void *dst = nullptr;
        HIP_TRY(hipMalloc(&dst, bytes ? bytes : 16));
        const hipError_t ce = hipMemcpy(dst, data, bytes, hipMemcpyDefault);
        if (ce != hipSuccess) {
            hipFree(dst);
            HIP_TRY(ce);
        }
        auto it = e->raw.find(n);
        if (it != e->raw.end()) hipFree(it->second.ptr);
        RawTensor t;
        t.ptr = dst;
        t.dtype = dtype;
        t.shape.assign(shape, shape + ndim);
        e->raw[n] = t;
        return VLO_OK;
    }
    if (dtype == VLO_DT_FP8_E4M3 || name_is(n, "_scale")) {
        // fp8 storage of the streamed projections (vlo_config.weight_dtype = 1): quantised by the caller, kept as given.  An mxfp4 engine takes
        // its lm_head this way too (the output layer is usually kept at 8 bits)
        const bool lm_head_of_fp4 = e->cfg.weight_dtype == 2 && (n == "lm_head.weight" || n == "lm_head.weight_scale");
        if ((e->cfg.weight_dtype != 1 && !lm_head_of_fp4) || !streamed)
            return fail(VLO_E_INVALID, n + ": fp8 weights / scales are accepted for the Llama projections of an engine created with weight_dtype = 1");
        if (name_is(n, "_scale") ? dtype != VLO_DT_F32 : dtype != VLO_DT_FP8_E4M3) return fail(VLO_E_INVALID, n + ": expected fp8 e4m3 data and f32 scales");
        ddt = dtype;
    }
    if (n.rfind("vision.", 0) == 0) {
        const bool is_mat = name_is(n, "proj.weight") || name_is(n, "fc1.weight") || name_is(n, "fc2.weight") ||
                            name_is(n, "patch_embedding.weight") || name_is(n, "in_proj_weight");
        ddt = is_mat ? VLO_DT_F16 : VLO_DT_F32;
    }
    void *stage = nullptr, *dst = nullptr;
    HIP_TRY(hipMalloc(&dst, numel * dt_size(ddt)));
    if (dtype == ddt) {
        HIP_TRY(hipMemcpy(dst, data, numel * dt_size(ddt), hipMemcpyDefault));
    } else {
        HIP_TRY(hipMalloc(&stage, numel * dt_size(dtype)));
        HIP_TRY(hipMemcpy(stage, data, numel * dt_size(dtype), hipMemcpyDefault));
        int blocks = (int)((numel + 255) / 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(convert_kernel, dim3(blocks), dim3(256), 0, 0, stage, dtype, dst, ddt, numel);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipFree(stage));
    }
    auto it = e->raw.find(n);
    if (it != e->raw.end()) hipFree(it->second.ptr);
    RawTensor t;
    t.ptr = dst;
    t.dtype = ddt;
    t.shape.assign(shape, shape + ndim);
    e->raw[n] = t;
    return VLO_OK;
}

static int take(vlo_engine *e, const std::string &name, std::vector<int64_t> shape, RawTensor *out) {
    auto it = e->raw.find(name);
    if (it == e->raw.end()) return fail(VLO_E_MISSING, "missing weight: " + name);
    if (!shape.empty() && it->second.shape != shape) {
        std::string s = "bad shape for " + name + ": got [";
        for (auto d : it->second.shape) s += std::to_string(d) + ",";
        s += "]";
        return fail(VLO_E_INVALID, s);
    }
    *out = it->second;
    return VLO_OK;
}

// pack rows [row0, row0+N) x columns [col0, col0+K) of the full bf16 linear `name` [Nfull][Kfull] into dst tiles
// (see gemv.hip); the slice is this rank's tensor-parallel shard (the whole matrix when tp_size == 1)
static int pack_into(vlo_engine *e, const std::string &name, int Nfull, int Kfull, int row0, int N, int col0, int K, PackedLinear &pl,
                     int tile_stride, int tile_offset, int half = -1) {
    RawTensor t;
    int rc = take(e, name, {Nfull, Kfull}, &t);
    if (rc) return rc;
    const int NT = half < 0 ? (N + 15) / 16 : (N + 7) / 8;
    if (pl.wq == 2) {
        RawTensor sc;
        if (t.dtype != VLO_DT_FP4_E2M1X2)
            return fail(VLO_E_INVALID, name + ": this engine streams mxfp4 weights (weight_dtype = 2): load it as VLO_DT_FP4_E2M1X2 with its e8m0 _scale");
        if ((rc = take(e, name + "_scale", {Nfull, Kfull / 32}, &sc))) return rc;
        if (sc.dtype != VLO_DT_E8M0) return fail(VLO_E_INVALID, name + "_scale: expected e8m0 block scales");
        const uint8_t *src = (const uint8_t *)t.ptr + ((size_t)row0 * Kfull + col0) / 2;
        const uint8_t *ssrc = (const uint8_t *)sc.ptr + ((size_t)row0 * Kfull + col0) / 32;
        HIP_TRY(pack_weight_mxfp4_launch(src, ssrc, pl.Wp, pl.wblk, N, K, Kfull / 2, Kfull / 32, NT, tile_stride, tile_offset, half, 0));
        return VLO_OK;
    }
    if (pl.wq) {
        RawTensor sc;
        if (t.dtype != VLO_DT_FP8_E4M3) return fail(VLO_E_INVALID, name + ": this engine streams fp8 weights (weight_dtype = 1): load it as VLO_DT_FP8_E4M3 with its _scale");
        if ((rc = take(e, name + "_scale", {Nfull}, &sc))) return rc;
        const uint8_t *src = (const uint8_t *)t.ptr + (size_t)row0 * Kfull + col0;
        HIP_TRY(pack_weight_fp8_launch(src, (const float *)sc.ptr + row0, pl.Wp, pl.wscale, N, K, Kfull, NT, tile_stride, tile_offset, half, 0));
        return VLO_OK;
    }
    if (t.dtype != VLO_DT_BF16) return fail(VLO_E_INVALID, name + ": expected a bf16 matrix");
    const unsigned short *src = (const unsigned short *)t.ptr + (size_t)row0 * Kfull + col0;
    HIP_TRY(pack_weight_launch(src, pl.Wp, N, K, Kfull, NT, tile_stride, tile_offset, half, 0));
    return VLO_OK;
}

// wq = the image format (PackedLinear::wq): 0 bf16, 1 fp8 e4m3 + per-channel scales, 2 mxfp4 (codes + e8m0 block scales)
static int make_linear(vlo_engine *e, PackedLinear *pl, int N, int K, bool allow_ksplit, int wq = 0, bool pad_for_gemm = false) {
    const bool fp8 = wq == 1;
    pl->N = N;
    pl->K = K;
    pl->NT = (N + 15) / 16;
    pl->NT_gemm = pad_for_gemm ? (pl->NT + 15) & ~15 : pl->NT;
    pl->wq = wq;
    if (gemv_plan(K, allow_ksplit, &pl->plan, wq))
        return fail(VLO_E_UNSUPPORTED, std::string(wq == 2 ? "no mxfp4 GEMV plan for K=" : "no GEMV plan for K=") + std::to_string(K));
    if (fp8 && ((pl->plan.KF & 1) || !(pl->plan.NW == 8 || (pl->plan.NW == 4 && pl->plan.KF == 14)) || (K & 63)))      // (4 x 14: K = 1792, gemv.hip)
        return fail(VLO_E_UNSUPPORTED, "fp8 weight image needs an even fragment count per wave (K=" + std::to_string(K) + ")");
    if (gemm64_plan(K, &pl->plan64, wq))
        return fail(VLO_E_UNSUPPORTED, "no block-GEMM plan for K=" + std::to_string(K));
    if (wq == 2) {                               // codes: half a byte per weight; scales: one byte per 32 weights, as dwords per (tile, 128 k, row)
        if (K & 127) return fail(VLO_E_UNSUPPORTED, "mxfp4 weight image needs K % 128 == 0 (K=" + std::to_string(K) + ")");
        const size_t cbytes = (size_t)pl->NT_gemm * 16 * K / 2, sbytes = (size_t)pl->NT_gemm * 16 * K / 32;
        int rc = dev_alloc(&pl->Wp, cbytes);
        if (rc) return rc;
        e->owned.push_back(pl->Wp);
        if ((rc = dev_alloc((void **)&pl->wblk, sbytes))) return rc;
        e->owned.push_back(pl->wblk);
        e->weight_bytes += (int64_t)(cbytes + sbytes);
        if (pl->NT_gemm > pl->NT) {              // the pad tiles: zero codes, scale byte 127
            HIP_TRY(hipMemset((char *)pl->Wp + (size_t)pl->NT * 16 * K / 2, 0, (size_t)(pl->NT_gemm - pl->NT) * 16 * K / 2));
            HIP_TRY(hipMemset((char *)pl->wblk + (size_t)pl->NT * 16 * K / 32, 0x7f, (size_t)(pl->NT_gemm - pl->NT) * 16 * K / 32));
        }
        return VLO_OK;
    }
    const size_t bytes = (size_t)pl->NT_gemm * 16 * K * (fp8 ? 1 : 2);
    int rc = dev_alloc(&pl->Wp, bytes);
    if (rc) return rc;
    e->owned.push_back(pl->Wp);
    e->weight_bytes += (int64_t)bytes;
    if (pl->NT_gemm > pl->NT)                    // the pad tiles: zero weights (and zero scales below) = zero logits in columns nobody reads
        HIP_TRY(hipMemset((char *)pl->Wp + (size_t)pl->NT * 16 * K * (fp8 ? 1 : 2), 0, (size_t)(pl->NT_gemm - pl->NT) * 16 * K * (fp8 ? 1 : 2)));
    if (fp8) {
        if ((rc = dev_alloc((void **)&pl->wscale, (size_t)pl->NT_gemm * 16 * 4))) return rc;
        e->owned.push_back(pl->wscale);
        HIP_TRY(hipMemset(pl->wscale, 0, (size_t)pl->NT_gemm * 16 * 4));
        e->weight_bytes += (int64_t)pl->NT_gemm * 16 * 4;
    }
    return VLO_OK;
}

static int take_vec(vlo_engine *e, const std::string &name, int64_t n, void **out) {
    RawTensor t;
    int rc = take(e, name, {n}, &t);
    if (rc) return rc;
    *out = t.ptr;
    e->owned.push_back(t.ptr);
    e->raw.erase(name);
    e->weight_bytes += n * (int64_t)dt_size(t.dtype);
    return VLO_OK;
}

static void drop_raw(vlo_engine *e, const std::string &name) {
    auto it = e->raw.find(name);
    if (it != e->raw.end()) {
        hipFree(it->second.ptr);
        e->raw.erase(it);
    }
}

int vlo_engine_finalize(vlo_engine *e) {
    if (!e) return fail(VLO_E_INVALID, "null engine");
    if (e->finalized) return VLO_OK;
    HIP_TRY(hipSetDevice(e->device));
    const vlo_config &c = e->cfg;
    const int H = c.hidden_size, hd = e->head_dim;
    const int r = e->tp_rank;
    const int Ifull = c.intermediate_size, I = e->I_l;                 // this rank's MLP columns
    const int NqF = c.num_heads * hd, NkvF = c.num_kv_heads * hd;       // full projection widths
    const int Nq = e->nh_l * hd, Nkv = e->nkv_l * hd, Nqkv = Nq + 2 * Nkv;   // this rank's heads
    int rc;
    const int wfmt = c.weight_dtype;                 // the image format of the seven decoder projections
    e->layers.resize(c.num_layers);
    for (int l = 0; l < c.num_layers; ++l) {
        LayerWeights &L = e->layers[l];
        const std::string p = "model.layers." + std::to_string(l) + ".";
        if ((rc = make_linear(e, &L.qkv, Nqkv, H, false, wfmt))) return rc;
        if ((rc = pack_into(e, p + "self_attn.q_proj.weight", NqF, H, r * Nq, Nq, 0, H, L.qkv, 1, 0))) return rc;
        if ((rc = pack_into(e, p + "self_attn.k_proj.weight", NkvF, H, r * Nkv, Nkv, 0, H, L.qkv, 1, Nq / 16))) return rc;
        if ((rc = pack_into(e, p + "self_attn.v_proj.weight", NkvF, H, r * Nkv, Nkv, 0, H, L.qkv, 1, (Nq + Nkv) / 16))) return rc;
        if ((rc = make_linear(e, &L.o, H, Nq, e->tp_size > 1, wfmt))) return rc;          // TP: fp32 partial sums, all-reduced
        if ((rc = pack_into(e, p + "self_attn.o_proj.weight", H, NqF, 0, H, r * Nq, Nq, L.o, 1, 0))) return rc;
        if ((rc = make_linear(e, &L.gate_up, 2 * I, H, false, wfmt))) return rc;       // SwiGLU epilogue needs whole K
        if (wfmt == 2 && L.gate_up.plan.KF > 16)      // (gemv.hip: no norm-on-load kernel at 28 fragments per chunk)
            return fail(VLO_E_UNSUPPORTED, "no mxfp4 norm-on-load GEMV plan for K=" + std::to_string(H));
        if (I % 16) return fail(VLO_E_UNSUPPORTED, "intermediate_size (per rank) must be a multiple of 16");
        // gate and up share every tile (8 + 8 rows): I/8 single tiles, SwiGLU inside one tile
        if ((rc = pack_into(e, p + "mlp.gate_proj.weight", Ifull, H, r * I, I, 0, H, L.gate_up, 1, 0, 0))) return rc;
        if ((rc = pack_into(e, p + "mlp.up_proj.weight", Ifull, H, r * I, I, 0, H, L.gate_up, 1, 0, 1))) return rc;
        if ((rc = make_linear(e, &L.down, H, I, true, wfmt))) return rc;
        if ((rc = pack_into(e, p + "mlp.down_proj.weight", H, Ifull, 0, H, r * I, I, L.down, 1, 0))) return rc;
        if ((rc = take_vec(e, p + "input_layernorm.weight", H, &L.ln_in))) return rc;
        if ((rc = take_vec(e, p + "post_attention_layernorm.weight", H, &L.ln_post))) return rc;
        HIP_TRY(hipDeviceSynchronize());
        for (const char *sfx : {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                                "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight"}) {
            drop_raw(e, p + sfx);
            drop_raw(e, p + sfx + "_scale");
        }
    }
    if ((rc = take_vec(e, "model.norm.weight", H, &e->norm_w))) return rc;
    // a tensor-parallel rank's vocabulary shard is padded to whole 256-column GEMM tiles (Llama-3 at T = 8: 16 032 -> 16 128), so that every row's
    // logits of a long input take the GEMM path like every other projection (tp.hip::tp_prefill)
    int lm_wq = wfmt;                                // an mxfp4 engine's lm_head: mxfp4 or fp8 per channel, whichever was loaded
    if (wfmt == 2) {
        auto it = e->raw.find("lm_head.weight");
        if (it != e->raw.end() && it->second.dtype == VLO_DT_FP8_E4M3) lm_wq = 1;
    }
    if ((rc = make_linear(e, &e->lm_head, e->V_l, H, false, lm_wq, e->tp_size > 1))) return rc;
    if ((rc = pack_into(e, "lm_head.weight", c.vocab_size, H, r * e->V_l, e->V_l, 0, H, e->lm_head, 1, 0))) return rc;
    {   // embedding table stays row-major (gather), replicated on every rank
        RawTensor t;
        if ((rc = take(e, "model.embed_tokens.weight", {c.vocab_size, H}, &t))) return rc;
        e->embed = t.ptr;
        e->owned.push_back(t.ptr);
        e->raw.erase("model.embed_tokens.weight");
    }
    // connector (optional: an LLM-only engine may omit it); replicated
    if (e->raw.count("connector.0.weight")) {
        const int Hv = c.vision_hidden_size;
        if ((rc = make_linear(e, &e->conn0, H, Hv, false))) return rc;
        if ((rc = pack_into(e, "connector.0.weight", H, Hv, 0, H, 0, Hv, e->conn0, 1, 0))) return rc;
        if ((rc = make_linear(e, &e->conn2, H, H, false))) return rc;
        if ((rc = pack_into(e, "connector.2.weight", H, H, 0, H, 0, H, e->conn2, 1, 0))) return rc;
        if ((rc = take_vec(e, "connector.0.bias", H, &e->conn0_b))) return rc;
        if ((rc = take_vec(e, "connector.2.bias", H, &e->conn2_b))) return rc;
        e->has_connector = true;
    }
    HIP_TRY(hipDeviceSynchronize());
    drop_raw(e, "lm_head.weight");
    drop_raw(e, "lm_head.weight_scale");
    drop_raw(e, "connector.0.weight");
    drop_raw(e, "connector.2.weight");

    // RoPE tables: cos/sin of pos * inv_freq in fp32, cast to bf16 (HF:modeling_llama.py:113-127)
    {
        const int half = hd / 2;
        std::vector<float> inv(half);
        if (e->raw.count("rope.inv_freq")) {
            RawTensor t;
            if ((rc = take(e, "rope.inv_freq", {half}, &t))) return rc;
            HIP_TRY(hipMemcpy(inv.data(), t.ptr, half * sizeof(float), hipMemcpyDeviceToHost));
            drop_raw(e, "rope.inv_freq");
        } else {
            for (int i = 0; i < half; ++i) inv[i] = 1.0f / powf(c.rope_theta, (float)(2 * i) / (float)hd);
        }
        e->inv_freq_h = inv;
        e->pool_pages = (int)((c.kv_pool_tokens + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS);
        e->max_positions = (int64_t)e->pool_pages * VLO_PAGE_TOKENS;
        std::vector<unsigned short> ct((size_t)e->max_positions * half), st((size_t)e->max_positions * half);
        auto tobf = [](float f) {
            unsigned u;
            memcpy(&u, &f, 4);
            u += 0x7fffu + ((u >> 16) & 1u);
            return (unsigned short)(u >> 16);
        };
        for (int64_t p = 0; p < e->max_positions; ++p)
            for (int i = 0; i < half; ++i) {
                const float ang = inv[i] * (float)p;
                ct[p * half + i] = tobf(cosf(ang));
                st[p * half + i] = tobf(sinf(ang));
            }
        if ((rc = dev_alloc(&e->cos_tab, ct.size() * 2))) return rc;
        if ((rc = dev_alloc(&e->sin_tab, st.size() * 2))) return rc;
        e->owned.push_back(e->cos_tab);
        e->owned.push_back(e->sin_tab);
        HIP_TRY(hipMemcpy(e->cos_tab, ct.data(), ct.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->sin_tab, st.data(), st.size() * 2, hipMemcpyHostToDevice));
    }
    // KV pool
    {
        e->page_elems = (int64_t)e->nkv_l * VLO_PAGE_TOKENS * hd;
        e->layer_stride = e->page_elems * e->pool_pages;
        const size_t bytes = (size_t)e->layer_stride * c.num_layers * (c.kv_dtype == VLO_KV_FP8 ? 1 : 2);   // element counts are the same
        if (c.kv_dtype == VLO_KV_FP8) {        // scales not loaded stay 1.0 (vlo_engine_create)
            if ((rc = dev_alloc((void **)&e->kv_scale, e->kv_scale_h.size() * sizeof(float)))) return rc;
            e->owned.push_back(e->kv_scale);
            HIP_TRY(hipMemcpy(e->kv_scale, e->kv_scale_h.data(), e->kv_scale_h.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if ((rc = dev_alloc(&e->k_pool, bytes))) return rc;
        if ((rc = dev_alloc(&e->vt_pool, bytes))) return rc;
        e->owned.push_back(e->k_pool);
        e->owned.push_back(e->vt_pool);
        HIP_TRY(hipMemset(e->k_pool, 0, bytes));
        HIP_TRY(hipMemset(e->vt_pool, 0, bytes));
        e->free_pages.clear();
        for (int p = e->pool_pages - 1; p >= 0; --p) e->free_pages.push_back(p);
    }
    if (c.has_vit) {
        if (!e->has_connector) return fail(VLO_E_MISSING, "vision tower needs the connector weights");
        if ((rc = vit_finalize(e))) return rc;
    }
    HIP_TRY(hipDeviceSynchronize());
    e->finalized = true;
    return VLO_OK;
}

double vlo_step_algorithmic_bytes(const vlo_engine *e, int64_t Lc, int n) {
    if (!e) return 0;
    const vlo_config &c = e->cfg;
    const double H = c.hidden_size, I = c.intermediate_size, hd = e->head_dim;
    const double per_layer = (H * (c.num_heads * hd) * 2 + H * (c.num_kv_heads * hd) * 2 + 3.0 * H * I) * 2.0;
    double W = per_layer * c.num_layers + (double)c.vocab_size * H * 2.0;
    if (c.weight_dtype == 1) {      // fp8 image: one byte per weight + one fp32 scale per output channel
        const double rows_per_layer = (c.num_heads + 2.0 * c.num_kv_heads) * hd + H + 2.0 * I + H;
        W = W / 2.0 + (rows_per_layer * c.num_layers + c.vocab_size) * 4.0;
    } else if (c.weight_dtype == 2) {   // mxfp4 image: half a byte per weight + one scale byte per 32; the lm_head as it was loaded
        const double lm = (double)c.vocab_size * H;
        W = per_layer * c.num_layers / 2.0 * (0.5 + 1.0 / 32.0) + (e->lm_head.wq == 1 ? lm + c.vocab_size * 4.0 : lm * (0.5 + 1.0 / 32.0));
    }
    const double kv = 2.0 * c.num_layers * c.num_kv_heads * hd * (c.kv_dtype == VLO_KV_FP8 ? 1.0 : 2.0);   // K + V bytes per token
    return W + kv * (double)(Lc + n) + kv * n + 2.0 * n * H * 2.0;
}

// ------------------------------------------------------------------------------------
// sessions
// ------------------------------------------------------------------------------------
int vlo_session_create(vlo_engine *e, int64_t max_tokens_hint, vlo_session **out) {
    if (!e || !out) return fail(VLO_E_INVALID, "null argument");
    if (!e->finalized) return fail(VLO_E_STATE, "engine not finalized");
    HIP_TRY(hipSetDevice(e->device));
    (void)max_tokens_hint;                      // (ABI: the workspaces do not depend on it)
    const vlo_config &c = e->cfg;
    const int H = c.hidden_size, I = e->I_l, hd = e->head_dim, nh = e->nh_l;
    vlo_session *s = new vlo_session();
    s->e = e;
    StepWs &w = s->ws;
    int rc = 0;
    auto A = [&](auto **p, size_t bytes) { alloc_owned(rc, s->owned, p, bytes); };
    A(&w.h, (size_t)32 * H * 2);
    A(&w.x, (size_t)32 * H * 2);
    A(&w.act, (size_t)32 * I * 2);
    A(&w.attn, (size_t)32 * nh * hd * 2);
    A(&w.q, (size_t)16 * nh * hd * 2);
    int ksmax = 1;
    for (auto &L : e->layers) ksmax = std::max(ksmax, L.down.plan.ksplit);
    A(&w.partial, (size_t)ksmax * 16 * H * 4);
    A(&w.sq[0], (size_t)(512 + 16) * 16 * 4);      // row sum-of-squares partials: [gemv grid.x <= 512][16] (+ row offset slack)
    A(&w.sq[1], (size_t)(512 + 16) * 16 * 4);
    w.part_cap = VLO_MAX_SPLITS;
    A(&w.part_o, (size_t)w.part_cap * nh * 16 * hd * 4);
    A(&w.part_ml, (size_t)w.part_cap * nh * 16 * 2 * 4);
    A(&s->logits, (size_t)16 * c.vocab_size * 2);
    if (e->tp_size > 1) {
        int ks_o = 1;
        for (auto &L : e->layers) ks_o = std::max(ks_o, L.o.plan.ksplit);
        A(&s->logits_local, (size_t)16 * e->V_l * 2);
        A(&s->partial_o, (size_t)ks_o * 16 * H * 4);
    }
    A(&s->tok, 64);
    A(&s->sample_scratch, VLO_SAMPLE_SCRATCH_FLOATS * 4);
    A(&s->emb1, (size_t)32 * H * 2);
    A(&s->page_table, (size_t)e->pool_pages * 4);
    if (rc) {
        vlo_session_destroy(s);
        return rc;
    }
    if (hipHostMalloc((void **)&s->host_tok, 64, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&s->host_pt, (size_t)e->pool_pages * 4, hipHostMallocDefault) != hipSuccess) {
        vlo_session_destroy(s);
        return fail(VLO_E_HIP, "hipHostMalloc failed");
    }
    s->last_logits = s->logits;
    HIP_TRY(hipDeviceSynchronize());
    *out = s;
    return VLO_OK;
}

int vlo_session_reset(vlo_session *s) {
    if (!s) return fail(VLO_E_INVALID, "null session");
    if (!s->pages.empty()) {
        // pages go back to the shared pool and the pinned page-table mirror will be rewritten from slot 0: queued kernels of
        // this session that still write K/V into those pages, and a queued page-table upload, must have drained first
        HIP_TRY(hipSetDevice(s->e->device));
        HIP_TRY(hipDeviceSynchronize());
    }
    std::lock_guard<std::mutex> g(s->e->pool_mu);
    for (int p : s->pages) s->e->free_pages.push_back(p);
    s->pages.clear();
    s->len = 0;
    s->has_logits = false;
    s->pend_units = 0;                           // a pending lookahead pass is dropped with its pages
    return VLO_OK;
}
int64_t vlo_session_len(const vlo_session *s) { return s ? s->len : -1; }

static void release_prefill_ws(vlo_session *s);      // (defined with the prefill path below)
void vlo_session_destroy(vlo_session *s) {
    if (!s) return;
    hipSetDevice(s->e->device);
    hipDeviceSynchronize();
    release_prefill_ws(s);
    vlo_session_reset(s);
    for (void *p : s->owned) hipFree(p);
    if (s->host_tok) hipHostFree(s->host_tok);
    for (hipEvent_t ev : s->tok_ev) if (ev) hipEventDestroy(ev);
    if (s->host_pt) hipHostFree(s->host_pt);
    delete s;
}

// a session between vlo_stream_steps and vlo_stream_steps_commit takes no other call (reset and destroy drop the pending pass)
static int pending_refusal(const vlo_session *s, const char *what) {
    if (!s || !s->pend_units) return VLO_OK;
    return fail(VLO_E_STATE, std::string(what) + ": a vlo_stream_steps pass is pending (call vlo_stream_steps_commit or vlo_session_reset)");
}

int ensure_pages(vlo_session *s, int64_t new_len, hipStream_t st) {
    vlo_engine *e = s->e;
    if (new_len > e->max_positions) return fail(VLO_E_NOMEM, "sequence exceeds kv_pool_tokens");
    const int need = (int)((new_len + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS);
    const int have = (int)s->pages.size();
    if (need <= have) return VLO_OK;
    {
        std::lock_guard<std::mutex> g(e->pool_mu);
        if ((int)e->free_pages.size() < need - have) return fail(VLO_E_NOMEM, "KV pool exhausted");
        for (int i = have; i < need; ++i) {
            const int p = e->free_pages.back();
            e->free_pages.pop_back();
            s->pages.push_back(p);
            s->host_pt[i] = p;      // pinned mirror is append-only => safe source for the async copy
        }
    }
    HIP_TRY(hipMemcpyAsync(s->page_table + have, s->host_pt + have, (size_t)(need - have) * 4, hipMemcpyHostToDevice, st));
    return VLO_OK;
}

KvPool kv_geom(const vlo_session *s) {
    const vlo_engine *e = s->e;
    KvPool g;
    g.k_pool = (unsigned short *)e->k_pool;
    g.vt_pool = (unsigned short *)e->vt_pool;
    g.page_table = s->page_table;
    g.layer_stride = e->layer_stride;
    g.page_elems = e->page_elems;
    g.num_kv_heads = e->nkv_l;
    g.head_dim = e->head_dim;
    g.dtype = e->cfg.kv_dtype;
    g.scale = e->kv_scale;
    return g;
}

// ---- live timing of the dominant kernel -------------------------------------------------
static void prof_flush(vlo_engine *e) {
    for (size_t i = 0; i < e->prof_used; ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(e->prof_events[i].second) == hipSuccess &&
            hipEventElapsedTime(&ms, e->prof_events[i].first, e->prof_events[i].second) == hipSuccess) {
            e->prof_ms += ms;
            e->prof_launches++;
        }
    }
    e->prof_used = 0;
}
static void prof_acquire(vlo_engine *e, hipEvent_t *a, hipEvent_t *b) {
    if (e->prof_used == e->prof_events.size()) {
        if (e->prof_events.size() >= 4096) {
            prof_flush(e);
        } else {
            hipEvent_t x, y;
            if (hipEventCreate(&x) != hipSuccess || hipEventCreate(&y) != hipSuccess) return;
            e->prof_events.push_back({x, y});
        }
    }
    *a = e->prof_events[e->prof_used].first;
    *b = e->prof_events[e->prof_used].second;
    e->prof_used++;
}
int vlo_profile_enable(vlo_engine *e, int stride) {
    if (!e) return fail(VLO_E_INVALID, "null engine");
    prof_flush(e);
    e->prof_stride = stride > 0 ? stride : 0;
    e->prof_seen = 0;
    e->prof_launches = 0;
    e->prof_ms = 0.0;
    return VLO_OK;
}
int vlo_profile_read(vlo_engine *e, int64_t *launches, double *total_ms, double *bytes_per_launch) {
    if (!e || !e->finalized) return fail(VLO_E_INVALID, "bad profile_read arguments");
    HIP_TRY(hipSetDevice(e->device));
    prof_flush(e);
    if (launches) *launches = e->prof_launches;
    if (total_ms) *total_ms = e->prof_ms;
    if (bytes_per_launch) {
        // gate+up weights [2I][H] bf16 streamed once + h [n<=16][H] in + act [n][I] out (n = 11 nominal)
        const double H = e->cfg.hidden_size, I = e->cfg.intermediate_size;
        const double wbytes = e->cfg.weight_dtype == 2 ? 2.0 * I * H * (0.5 + 1.0 / 32.0)                    // mxfp4: codes + e8m0 block scales
                              : e->cfg.weight_dtype == 1 ? 2.0 * I * H + 2.0 * I * 4.0 : 2.0 * I * H * 2.0;   // fp8: codes + fp32 scales
        *bytes_per_launch = wbytes + 11.0 * H * 2.0 + 11.0 * I * 2.0;
    }
    return VLO_OK;
}

int vlo_profile_calibrate(vlo_engine *e, void *stream, double *empty_bracket_us) {
    if (!e || !empty_bracket_us) return fail(VLO_E_INVALID, "bad profile_calibrate arguments");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const int N = 64;
    hipEvent_t a[N], b[N];
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < N; ++i) {
        HIP_TRY(hipEventCreate(&a[i]));
        HIP_TRY(hipEventCreate(&b[i]));
    }
    for (int i = 0; i < N; ++i) {
        HIP_TRY(hipEventRecord(a[i], st));
        HIP_TRY(hipEventRecord(b[i], st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    double tot = 0.0;
    for (int i = 0; i < N; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, a[i], b[i]));
        tot += ms;
        hipEventDestroy(a[i]);
        hipEventDestroy(b[i]);
    }
    *empty_bracket_us = tot * 1e3 / N;
    return VLO_OK;
}

GemvArgs gemv_args(const PackedLinear &pl, const unsigned short *x, int ldx, int n_rows) {
    GemvArgs a{};
    a.Wp = pl.Wp;
    a.wq = pl.wq;
    if (pl.wq == 2) a.wblk = pl.wblk;
    else a.wscale = pl.wscale;
    a.x = x;
    a.K = pl.K;
    a.ldx = ldx;
    a.NT = pl.NT;
    a.N_valid = pl.N;
    a.n_rows = n_rows;
    return a;
}

GemvArgs qkv_args(const vlo_engine *e, int layer, const StepWs &w, int n_rows, int64_t pos0) {
    GemvArgs a = gemv_args(e->layers[layer].qkv, w.x, e->cfg.hidden_size, n_rows);
    a.out_bf16 = w.q; a.cos_tab = (const unsigned short *)e->cos_tab; a.sin_tab = (const unsigned short *)e->sin_tab;
    a.layer = layer; a.num_heads = e->nh_l; a.pos0 = pos0;
    return a;
}

// Where the rows of a pass sit in the KV cache: the one thing a solo step and a batched step differ in.
//   solo    (segs == nullptr): consecutive positions pos0 .. pos0 + M - 1 of one session, whose page table is kv.page_table
//   batched (segs != nullptr): each row's position and page in the device row table `rows` (EPI_ROPE_ROWS), attention per planned segment
struct KvRows {
    KvPool kv;
    int64_t pos0 = 0;
    const RopeRow *rows = nullptr;
    const AttnSeg *segs = nullptr; const AttnSegRun *runs = nullptr; int nseg = 0, nrun = 0;   // device table + its host-side launch plan (attention_seg_plan)
};
// the last layer's down-proj partial sums, not yet folded into h: the caller's final add_rmsnorm combines them (16-row pipeline; none on the block path)
struct PendingDown { const float *partial = nullptr; int ksplit = 0; };

// The decoder layers of one pass over M new rows whose embeddings are in w.h.  Two pipelines over the same packed weights:
//
// 16-row (M <= 16; GEMVs, every matrix row-major), 7 launches per layer:
//   add_rmsnorm   [+ down-proj split-K combine + residual of the previous layer]      -> x
//   qkv GEMV      [RoPE + paged KV append in the epilogue]                             -> q, K, V^T
//   attention, combine                                                                 -> attn
//   o GEMV        [residual add + row sum-of-squares partials in the epilogue]         -> h, sq
//   gate/up GEMV  [post-attention RMSNorm fused into the operand load | SwiGLU]        -> act
//   down GEMV     [K split over blocks, fp32 partials]                                 -> partial (left pending for the caller after the last layer)
//
// block (16 < M <= 64; gemm64 of prefill.hip, x / attn / act packed-64), 8 launches per layer:
//   RMSNorm rows -> qkv GEMM [RoPE + KV append] -> attention over the (up to four) 16-query sub-chunks, combine -> o GEMM [residual add]
//   -> RMSNorm rows -> gate/up GEMM [SwiGLU] -> down GEMM [residual add]
// Same rounding points as the 16-row pipeline (projection outputs and residual sums are bf16, accumulation fp32); only the fp32 summation
// order inside a dot product differs (K is split over the waves of a block differently).
//
// profile: bracket the gate/up GEMV for vlo_profile_read (solo 16-row steps only).
static int decoder_layers(vlo_engine *e, const StepWs &w, int M, bool block, const KvRows &at, bool profile, hipStream_t st, PendingDown *pending) {
    const vlo_config &c = e->cfg;
    const int H = c.hidden_size, I = e->I_l, hd = e->head_dim, nh = e->nh_l;
    const int ldx = block ? 0 : H;                     // 0: packed-64
    const bool batched = at.segs != nullptr;
    KvPool kv_append = at.kv;
    if (batched) kv_append.page_table = reinterpret_cast<const int *>(at.rows);   // EPI_ROPE_ROWS reads the row table through kv.page_table (gemv.h)
    const float *prev = nullptr;
    int prev_ks = 0;
    for (int l = 0; l < c.num_layers; ++l) {
        const LayerWeights &L = e->layers[l];
        HIP_TRY(add_rmsnorm_launch(w.h, prev, prev_ks, H, (const unsigned short *)L.ln_in, w.x, H, ldx, c.rms_eps, M, st));
        {   // qkv [RoPE + KV append: at pos0 + row, or at each row's own position and page]
            GemvArgs a = qkv_args(e, l, w, M, at.pos0);
            int epi = rope_epi(a, kv_append);
            if (batched) epi = epi == EPI_ROPE_F8 ? EPI_ROPE_ROWS_F8 : EPI_ROPE_ROWS;
            if (block) HIP_TRY(gemm64_launch(a, L.qkv.plan64, epi, st));
            else HIP_TRY(gemv_launch(a, L.qkv.plan, XSRC_PLAIN, epi, st));
        }
        // one launch for the (up to four) 16-query sub-chunks of a block; its keys are already appended
        if (batched) HIP_TRY(attention_seg_launch(w.q, at.kv, l, nh, at.segs, at.nseg, at.runs, at.nrun, w.part_o, w.part_ml, w.attn, block, st));
        else HIP_TRY(attention_launch(w.q, at.kv, l, nh, at.pos0, M, w.part_o, w.part_ml, w.attn, st, block ? 0 : -1, w.part_cap));
        int sq_parts = 0;
        {   // o_proj + residual
            GemvArgs a = gemv_args(L.o, w.attn, nh * hd, M);
            a.h = w.h; a.ldo = H;
            if (block) {
                HIP_TRY(gemm64_launch(a, L.o.plan64, EPI_RESID, st));
            } else {
                a.sq_out = w.sq[0];
                sq_parts = gemv_grid_x(a, L.o.plan, EPI_RESID);
                HIP_TRY(gemv_launch(a, L.o.plan, XSRC_PLAIN, EPI_RESID, st));
            }
        }
        if (block) {
            HIP_TRY(add_rmsnorm_launch(w.h, nullptr, 0, H, (const unsigned short *)L.ln_post, w.x, H, 0, c.rms_eps, M, st));
            GemvArgs a = gemv_args(L.gate_up, w.x, H, M);              // gate/up + SwiGLU
            a.out_bf16 = w.act; a.ldo = I;
            HIP_TRY(gemm64_launch(a, L.gate_up.plan64, EPI_SWIGLU, st));
            GemvArgs d = gemv_args(L.down, w.act, I, M);               // down_proj + residual
            d.h = w.h; d.ldo = H;
            HIP_TRY(gemm64_launch(d, L.down.plan64, EPI_RESID, st));
            continue;
        }
        {   // gate/up + SwiGLU
            hipEvent_t ev0 = nullptr, ev1 = nullptr;
            if (profile && e->prof_stride > 0 && (e->prof_seen++ % e->prof_stride) == 0) prof_acquire(e, &ev0, &ev1);
            GemvArgs a = gemv_args(L.gate_up, w.h, H, M);
            a.norm_w = (const unsigned short *)L.ln_post; a.sq_in = w.sq[0]; a.sq_in_parts = sq_parts; a.eps = c.rms_eps;
            a.out_bf16 = w.act; a.ldo = I;
            if (ev0) hipEventRecord(ev0, st);
            HIP_TRY(gemv_launch(a, L.gate_up.plan, XSRC_NORM, EPI_SWIGLU, st));
            if (ev1) hipEventRecord(ev1, st);
        }
        {   // down_proj: fp32 K-slice partials, combined by the next add_rmsnorm
            GemvArgs a = gemv_args(L.down, w.act, I, M);
            a.out_f32 = w.partial; a.ldo = H;
            HIP_TRY(gemv_launch(a, L.down.plan, XSRC_PLAIN, EPI_PARTIAL_F32, st));
            prev = w.partial;
            prev_ks = L.down.plan.ksplit;
        }
    }
    pending->partial = prev;
    pending->ksplit = prev_ks;
    return VLO_OK;
}

static KvRows solo_rows(const vlo_session *s) {   // a solo step's rows: consecutive positions behind the session's cache
    KvRows at;
    at.kv = kv_geom(s); at.pos0 = s->len;
    return at;
}

// one chunk of m <= 16 new tokens whose embeddings are at `src`: the 16-row pipeline
static int run_chunk(vlo_session *s, const unsigned short *src, int m, bool want_last, bool want_all, hipStream_t st) {
    vlo_engine *e = s->e;
    const vlo_config &c = e->cfg;
    const StepWs &w = s->ws;
    const int H = c.hidden_size;
    int rc;
    if ((rc = ensure_pages(s, s->len + m, st))) return rc;
    HIP_TRY(copy_rows_launch(src, w.h, m, H, st));
    PendingDown pd;
    if ((rc = decoder_layers(e, w, m, false, solo_rows(s), true, st, &pd))) return rc;
    if (want_last || want_all) {
        HIP_TRY(add_rmsnorm_launch(w.h, pd.partial, pd.ksplit, H, (const unsigned short *)e->norm_w, w.x, H, H, c.rms_eps, m, st));
        const int r0 = want_all ? 0 : m - 1, nr = want_all ? m : 1;        // only the rows that are read
        GemvArgs a = gemv_args(e->lm_head, w.x + (size_t)r0 * H, H, nr);
        a.out_bf16 = s->logits; a.ldo = c.vocab_size;
        HIP_TRY(gemv_launch(a, e->lm_head.plan, XSRC_PLAIN, EPI_BF16, st));
        s->last_logits = s->logits + (size_t)(nr - 1) * c.vocab_size;
        s->has_logits = true;
    }
    s->len += m;
    return VLO_OK;
}

// ---- block path: up to 64 new tokens per weight pass (prefill.hip) ---------------------------------------------------
static int ensure_block_ws(vlo_session *s) {
    StepWs &w = s->bws;
    if (w.act) return VLO_OK;                   // the LAST buffer allocated below: set only when all of them exist
    HIP_TRY(hipSetDevice(s->e->device));
    int rc = 0;
    alloc_block_rows(rc, s->owned, s->e, w, false);
    w.part_o = s->ws.part_o; w.part_ml = s->ws.part_ml; w.part_cap = s->ws.part_cap;   // one pass at a time per session: shared with the 16-row set
    return rc;
}

// The end of a block / prefill pass that was asked for logits: the session keeps the last row's.  all_logits: the caller's matrix, every row
// already written by the pass — the last row is copied out of it; else row m - 1 of x (the final-normed rows, row-major) goes through the GEMV.
static int last_row_logits(vlo_session *s, const unsigned short *x, int m, const unsigned short *all_logits, hipStream_t st) {
    const vlo_engine *e = s->e;
    const int H = e->cfg.hidden_size, V = e->cfg.vocab_size;
    if (all_logits) {
        HIP_TRY(hipMemcpyAsync(s->logits, all_logits + (size_t)(m - 1) * V, (size_t)V * 2, hipMemcpyDeviceToDevice, st));
    } else {                                    // only the row that is read
        GemvArgs a = gemv_args(e->lm_head, x + (size_t)(m - 1) * H, H, 1);
        a.out_bf16 = s->logits; a.ldo = V;
        HIP_TRY(gemv_launch(a, e->lm_head.plan, XSRC_PLAIN, EPI_BF16, st));
    }
    s->last_logits = s->logits;
    s->has_logits = true;
    return VLO_OK;
}

// one block of 16 < m <= 64 new tokens: the block pipeline
static int run_block(vlo_session *s, const unsigned short *src, int m, bool want_last, unsigned short *all_logits, hipStream_t st) {
    vlo_engine *e = s->e;
    const vlo_config &c = e->cfg;
    const StepWs &w = s->bws;
    const int H = c.hidden_size, V = c.vocab_size;
    int rc;
    if ((rc = ensure_block_ws(s))) return rc;
    if ((rc = ensure_pages(s, s->len + m, st))) return rc;
    HIP_TRY(copy_rows_launch(src, w.h, m, H, st));
    PendingDown pd;                             // (nothing pending on the block path: its down GEMM adds into h)
    if ((rc = decoder_layers(e, w, m, true, solo_rows(s), false, st, &pd))) return rc;
    if (want_last || all_logits) {
        HIP_TRY(add_rmsnorm_launch(w.h, nullptr, 0, H, (const unsigned short *)e->norm_w, w.x, H, all_logits ? 0 : H, c.rms_eps, m, st));
        if (all_logits) {                       // every row, straight into the caller's matrix
            GemvArgs a = gemv_args(e->lm_head, w.x, H, m);
            a.out_bf16 = all_logits; a.ldo = V;
            HIP_TRY(gemm64_launch(a, e->lm_head.plan64, EPI_BF16, st));
        }
        if ((rc = last_row_logits(s, w.x, m, all_logits, st))) return rc;
    }
    s->len += m;
    return VLO_OK;
}

// ---- prefill path: up to VLO_PREFILL_TOKENS new tokens per weight pass, the projections as MFMA-bound GEMMs (prefill.h) ------------------
int ensure_prefill_ws(vlo_session *s) {
    if (s->pact) return VLO_OK;                 // the LAST buffer taken below: set only when all of them exist
    vlo_engine *e = s->e;
    {
        std::lock_guard<std::mutex> g(e->pool_mu);
        if (!e->prefill_free.empty()) {         // a set another session handed back (engine.h: pooled per engine)
            const PrefillWs w = e->prefill_free.back();
            e->prefill_free.pop_back();
            s->ph = w.ph; s->px = w.px; s->pqkv = w.pqkv; s->pq = w.pq;
            s->pf_wexp = w.wexp; s->pf_wexp_bytes = w.wexp_bytes; s->ppartial = w.partial; s->pxq = w.xq;
            s->pact = w.pact;
            return VLO_OK;
        }
    }
    const size_t H = e->cfg.hidden_size, I = e->I_l, qd = (size_t)e->nh_l * e->head_dim, kvd = (size_t)e->nkv_l * e->head_dim;
    const size_t R = VLO_PREFILL_TOKENS, RX = R + 256;        // X operands: the GEMM reads whole 256-row tiles
    struct { unsigned short **p; size_t elems; } want[] = {{&s->ph, R * H}, {&s->px, RX * std::max(H, qd)}, {&s->pqkv, R * (qd + 2 * kvd)},
                                                            {&s->pq, R * qd}, {&s->pact, RX * I}};
    HIP_TRY(hipSetDevice(e->device));
    for (auto &w : want) {
        if (*w.p) continue;
        void *p = nullptr;
        int rc = dev_alloc(&p, w.elems * 2);
        if (rc) return rc;                      // (a partly built set is freed with the session: release_prefill_ws)
        HIP_TRY(hipMemset(p, 0, w.elems * 2));  // the spare rows are read (and dropped) by the GEMMs: keep them finite
        *w.p = (unsigned short *)p;
    }
    return VLO_OK;
}

// a destroyed session's prefill set goes back to its engine's pool (the device is idle: vlo_session_destroy synchronises first)
static void release_prefill_ws(vlo_session *s) {
    if (!s->ph && !s->px && !s->pqkv && !s->pq && !s->pact && !s->pf_wexp && !s->ppartial && !s->pxq) return;
    vlo_engine *e = s->e;
    if (!s->pact) {                             // an allocation failed half way: nothing reusable
        for (void *p : {(void *)s->ph, (void *)s->px, (void *)s->pqkv, (void *)s->pq, s->pf_wexp, (void *)s->ppartial, s->pxq}) if (p) hipFree(p);
    } else {
        PrefillWs w;
        w.ph = s->ph; w.px = s->px; w.pqkv = s->pqkv; w.pq = s->pq; w.pact = s->pact;
        w.wexp = s->pf_wexp; w.wexp_bytes = s->pf_wexp_bytes; w.partial = s->ppartial; w.xq = s->pxq;
        std::unique_lock<std::mutex> g(e->pool_mu);
        if (e->prefill_free.size() < VLO_PREFILL_POOL_MAX) {
            e->prefill_free.push_back(w);
        } else {                                // a burst of long-prompt sessions does not pin its peak for the engine's lifetime (engine.h)
            g.unlock();
            for (void *p : {(void *)w.ph, (void *)w.px, (void *)w.pqkv, (void *)w.pq, (void *)w.pact, w.wexp, (void *)w.partial, w.xq}) if (p) hipFree(p);
        }
    }
    s->ph = s->px = s->pqkv = s->pq = s->pact = nullptr;
    s->pf_wexp = nullptr; s->pf_wexp_bytes = 0; s->ppartial = nullptr; s->pxq = nullptr;
}

// partial states for the fallback attention kernel (shapes attn_prefill_kernel is not instantiated for): 67 MB at the 8B shape,
// so only sessions that take the fallback pay for them
static int ensure_prefill_partials(vlo_session *s) {
    if (s->ppart_ml) return VLO_OK;
    vlo_engine *e = s->e;
    void *po = nullptr, *pm = nullptr;
    int rc = dev_alloc(&po, (size_t)(VLO_PREFILL_TOKENS / 16) * e->nh_l * 16 * e->head_dim * 4);
    if (rc) return rc;
    s->owned.push_back(po);
    if ((rc = dev_alloc(&pm, (size_t)(VLO_PREFILL_TOKENS / 16) * e->nh_l * 16 * 2 * 4))) return rc;
    s->owned.push_back(pm);
    s->ppart_o = (float *)po; s->ppart_ml = (float *)pm;
    return VLO_OK;
}

// One projection of a prefill block: out = X W^T through the GEMM of prefill.h (kind = LLM_GEMM_*).  fp8 engines: the projection's e4m3 image is
// expanded to bf16 (exactly) into the session's scratch right before its GEMM — 3 bytes of extra traffic per weight against hundreds of tokens of
// MFMA work per weight — and its per-channel scales go to the GEMM's epilogue.  Shared with tp.hip (a rank's shard of a tensor-parallel prefill).
int prefill_gemm(vlo_session *s, const unsigned short *X, const PackedLinear &pl, int m, int N, int K, void *out, int ldo, int kind, hipStream_t st,
                 bool layer_proj) {
    vlo_engine *e = s->e;
    if (!pl.wq) { HIP_TRY(llm_gemm_launch(X, pl.Wp, m, N, K, out, ldo, kind, st)); return VLO_OK; }
    if (layer_proj && e->cfg.prefill_act_dtype == 1 && llm_gemm_fp8_ok(N, K)) {
        // native fp8 MFMA (prefill.h): X quantised per row into the session's code scratch (codes, then the scales), W = the fp8 image as stored.
        // Rows past m keep whatever the scratch held: they are computed and dropped, no output row depends on another row's X.
        const size_t RX = VLO_PREFILL_TOKENS + 256;
        const LayerWeights &L0 = e->layers[0];
        const size_t kmax = (size_t)std::max({L0.qkv.K, L0.o.K, L0.gate_up.K, L0.down.K});
        if ((size_t)K > kmax) return fail(VLO_E_STATE, "prefill_gemm: a layer projection wider than the layer's widest K");
        if (!s->pxq) {
            void *p = nullptr;
            int rc2 = dev_alloc(&p, RX * kmax + RX * sizeof(float));
            if (rc2) return rc2;
            HIP_TRY(hipMemset(p, 0, RX * kmax + RX * sizeof(float)));
            HIP_TRY(hipDeviceSynchronize());
            s->pxq = p;
        }
        float *xs = reinterpret_cast<float *>((char *)s->pxq + RX * kmax);
        HIP_TRY(quantize_rows_fp8_launch(X, m, K, s->pxq, xs, st));
        HIP_TRY(llm_gemm_fp8_launch(s->pxq, xs, pl.Wp, pl.wscale, m, N, K, out, ldo, kind, st));
        return VLO_OK;
    }
    // sized for the largest projection of a layer at the first use (not grown projection by projection); the lm_head image may grow it once more
    const LayerWeights &L0 = e->layers[0];
    const int NTg = std::max(pl.NT, N / 16);                  // (N may be the padded width of a TP lm_head shard: pl.NT_gemm tiles)
    const size_t img = (size_t)NTg * 16 * K * 2;
    auto bytes = [](const PackedLinear &q) { return (size_t)q.NT * 16 * q.K * 2; };
    const size_t need = std::max({img, bytes(L0.qkv), bytes(L0.o), bytes(L0.gate_up), bytes(L0.down)});
    if (s->pf_wexp_bytes < need) {
        HIP_TRY(hipStreamSynchronize(st));                       // (grows at most twice per pooled set: the largest layer projection, then the lm_head image)
        void *p = nullptr;
        int rc2 = dev_alloc(&p, need);
        if (rc2) return rc2;
        if (s->pf_wexp) hipFree(s->pf_wexp);                     // the superseded scratch: nothing reads it after the synchronise above
        s->pf_wexp = p; s->pf_wexp_bytes = need;
    }
    if (pl.wq == 2) {                                            // mxfp4: codes x block scales -> bf16, nothing left for the epilogue
        HIP_TRY(expand_mxfp4_image_launch(pl.Wp, pl.wblk, s->pf_wexp, NTg, K, st));
        HIP_TRY(llm_gemm_launch(X, s->pf_wexp, m, N, K, out, ldo, kind, st));
        return VLO_OK;
    }
    HIP_TRY(expand_fp8_image_launch(pl.Wp, s->pf_wexp, NTg, K, st));
    HIP_TRY(llm_gemm_launch(X, s->pf_wexp, m, N, K, out, ldo, kind, st, pl.wscale));
    return VLO_OK;
}

// one block of VLO_PREFILL_MIN <= m <= VLO_PREFILL_TOKENS new tokens.  Per decoder layer: RMSNorm rows -> qkv GEMM -> RoPE + KV append ->
// attention in one launch (the block path's kernel, grid.z = 16-query sub-chunks: the whole block's keys are already appended) ->
// o GEMM [residual add] -> RMSNorm rows -> gate/up GEMM [SwiGLU] -> down GEMM [residual add].  Rounding points as run_chunk / run_block
// (projection outputs, RoPE products and sums, residual sums in bf16; accumulation fp32); only the summation order over K differs.
static int run_prefill(vlo_session *s, const unsigned short *src, int m, bool want_last, unsigned short *all_logits, hipStream_t st) {
    vlo_engine *e = s->e;
    const vlo_config &c = e->cfg;
    const int H = c.hidden_size, I = e->I_l, hd = e->head_dim, nh = e->nh_l, nkv = e->nkv_l, V = c.vocab_size;
    const int qd = nh * hd, Nqkv = qd + 2 * nkv * hd;
    int rc;
    if ((rc = ensure_prefill_ws(s))) return rc;
    if ((rc = ensure_pages(s, s->len + m, st))) return rc;
    const KvPool kv = kv_geom(s);
    HIP_TRY(copy_rows_launch(src, s->ph, m, H, st));
    auto gemm = [&](const unsigned short *X, const PackedLinear &pl, int N, int K, unsigned short *out, int ldo, int kind) -> int {
        return prefill_gemm(s, X, pl, m, N, K, out, ldo, kind, st);
    };
    for (int l = 0; l < c.num_layers; ++l) {
        const LayerWeights &L = e->layers[l];
        HIP_TRY(add_rmsnorm_launch(s->ph, nullptr, 0, H, (const unsigned short *)L.ln_in, s->px, H, H, c.rms_eps, m, st));
        if ((rc = gemm(s->px, L.qkv, Nqkv, H, s->pqkv, Nqkv, LLM_GEMM_BF16))) return rc;
        HIP_TRY(rope_kv_append_launch(s->pqkv, m, nh, (const unsigned short *)e->cos_tab, (const unsigned short *)e->sin_tab, kv, l, s->len, s->pq, st));
        // the whole block's keys are appended: ONE attention launch, grid.z = the block's 16-query sub-chunks (causal mask per sub-chunk,
        // one split each); the output lands in px (the o-proj's X operand)
        hipError_t ae = attention_prefill_launch(s->pq, kv, l, nh, s->len, m, s->px, st);
        if (ae == hipErrorNotSupported) {
            if ((rc = ensure_prefill_partials(s))) return rc;
            ae = attention_launch(s->pq, kv, l, nh, s->len, m, s->ppart_o, s->ppart_ml, s->px, st, -1, VLO_PREFILL_TOKENS / 16);
        }
        HIP_TRY(ae);
        if ((rc = gemm(s->px, L.o, H, qd, s->ph, H, LLM_GEMM_RESID))) return rc;
        HIP_TRY(add_rmsnorm_launch(s->ph, nullptr, 0, H, (const unsigned short *)L.ln_post, s->px, H, H, c.rms_eps, m, st));
        if ((rc = gemm(s->px, L.gate_up, 2 * I, H, s->pact, I, LLM_GEMM_SWIGLU))) return rc;
        if ((rc = gemm(s->pact, L.down, H, I, s->ph, H, LLM_GEMM_RESID))) return rc;
    }
    if (want_last || all_logits) {
        HIP_TRY(add_rmsnorm_launch(s->ph, nullptr, 0, H, (const unsigned short *)e->norm_w, s->px, H, H, c.rms_eps, m, st));
        if (all_logits) {                       // every row, straight into the caller's matrix
            if (V % 256 == 0) {
                if ((rc = prefill_gemm(s, s->px, e->lm_head, m, V, H, all_logits, V, LLM_GEMM_BF16, st, false))) return rc;   // logits: bf16 activations always
            } else {                            // vocabularies that are not whole 256-column tiles: 16 rows at a time through the GEMV
                for (int r0 = 0; r0 < m; r0 += 16) {
                    GemvArgs a = gemv_args(e->lm_head, s->px + (size_t)r0 * H, H, std::min(16, m - r0));
                    a.out_bf16 = all_logits + (size_t)r0 * V; a.ldo = V;
                    HIP_TRY(gemv_launch(a, e->lm_head.plan, XSRC_PLAIN, EPI_BF16, st));
                }
            }
        }
        if ((rc = last_row_logits(s, s->px, m, all_logits, st))) return rc;
    }
    s->len += m;
    return VLO_OK;
}

// shapes the prefill GEMMs take (bf16 image, or the fp8 image expanded per GEMM): every projection width a multiple of 256, every K of 128 —
// of THIS rank's shard under tensor parallelism (tp.hip::tp_prefill: column-sharded q|k|v and gate|up, row-sharded o and down)
bool prefill_ok(const vlo_engine *e) {
    static const bool on = getenv("VLO_PREFILL") ? atoi(getenv("VLO_PREFILL")) != 0 : true;
    const vlo_config &c = e->cfg;
    const int hd = e->head_dim, qd = e->nh_l * hd, Nqkv = qd + 2 * e->nkv_l * hd;
    return on && !(Nqkv & 255) && !(c.hidden_size & 255) && !((2 * e->I_l) & 255) && !(e->I_l & 127) && !(qd & 127) && (hd == 64 || hd == 128);
}

int vlo_llm_step(vlo_session *s, const void *embeds_dev, int n, void *last_logits_dev, void *all_logits_dev, void *stream) {
    if (!s || !embeds_dev || n <= 0) return fail(VLO_E_INVALID, "bad llm_step arguments");
    if (int prc = pending_refusal(s, "llm_step")) return prc;
    vlo_engine *e = s->e;
    if (e->tp_size > 1) return fail(VLO_E_STATE, "tensor-parallel engine: step it through vlo_tp_llm_step");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const int H = e->cfg.hidden_size, V = e->cfg.vocab_size;
    int rc;
    // inputs longer than one 16-row chunk go through the 64-token block path (one weight pass per 64 tokens); the live
    // frame / decode steps (n <= 16) keep the fused 16-row pipeline.  VLO_BLOCK_PATH=0 forces 16-row chunks everywhere.
    static const bool block_path = getenv("VLO_BLOCK_PATH") ? atoi(getenv("VLO_BLOCK_PATH")) != 0 : true;
    for (int c0 = 0; c0 < n;) {
        const int left = n - c0;
        const unsigned short *src = (const unsigned short *)embeds_dev + (size_t)c0 * H;
        unsigned short *all = all_logits_dev ? (unsigned short *)all_logits_dev + (size_t)c0 * V : nullptr;
        if (block_path && left >= VLO_PREFILL_MIN && prefill_ok(e)) {
            // long inputs: blocks of up to VLO_PREFILL_TOKENS tokens with the projections as GEMMs; what is left below VLO_PREFILL_MIN
            // goes through the 64-token block path (so a remainder never starts a new kind of weight pass for a handful of tokens)
            const int m = std::min(VLO_PREFILL_TOKENS, left);
            if ((rc = run_prefill(s, src, m, c0 + m == n, all, st))) return rc;
            c0 += m;
            continue;
        }
        if (block_path && left > 16) {
            const int m = std::min(VLO_BLOCK_TOKENS, left);
            if ((rc = run_block(s, src, m, c0 + m == n, all, st))) return rc;
            c0 += m;
            continue;
        }
        const int m = std::min(16, left);
        if ((rc = run_chunk(s, src, m, c0 + m == n, all != nullptr, st))) return rc;
        if (all) HIP_TRY(hipMemcpyAsync(all, s->logits, (size_t)m * V * 2, hipMemcpyDeviceToDevice, st));
        c0 += m;
    }
    if (last_logits_dev) HIP_TRY(hipMemcpyAsync(last_logits_dev, s->last_logits, (size_t)V * 2, hipMemcpyDeviceToDevice, st));
    return VLO_OK;
}

int vlo_stream_sample(vlo_session *s, float threshold, int interval_id, int64_t *tok_dev, float *p_interval_dev, void *stream) {
    if (!s || !tok_dev) return fail(VLO_E_INVALID, "bad stream_sample arguments");
    if (int prc = pending_refusal(s, "stream_sample")) return prc;
    if (!s->has_logits) return fail(VLO_E_STATE, "no logits: call vlo_llm_step first");
    HIP_TRY(hipSetDevice(s->e->device));
    HIP_TRY(stream_sample_launch(s->last_logits, s->e->cfg.vocab_size, threshold, interval_id, tok_dev, p_interval_dev,
                                 s->sample_scratch, (hipStream_t)stream));
    return VLO_OK;
}

int vlo_embed(vlo_engine *e, const int64_t *ids_dev, int k, void *out_dev, void *stream) {
    if (!e || !ids_dev || !out_dev || k <= 0) return fail(VLO_E_INVALID, "bad embed arguments");
    if (!e->finalized) return fail(VLO_E_STATE, "engine not finalized");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(embed_gather_launch((const unsigned short *)e->embed, ids_dev, k, e->cfg.hidden_size, e->cfg.vocab_size,
                                (unsigned short *)out_dev, (hipStream_t)stream));
    return VLO_OK;
}

int vlo_step_input(vlo_engine *e, const int64_t *ids_host, int k, const void *frame_rows_dev, int rows, void *out_dev, void *stream) {
    if (!e || !out_dev || k < 0 || rows < 0 || k + rows <= 0 || (k > 0 && !ids_host) || (rows > 0 && !frame_rows_dev))
        return fail(VLO_E_INVALID, "bad step_input arguments");
    if (!e->finalized) return fail(VLO_E_STATE, "engine not finalized");
    HIP_TRY(hipSetDevice(e->device));
    const int H = e->cfg.hidden_size;
    unsigned short *out = (unsigned short *)out_dev;
    // ids travel as kernel arguments, VLO_STEP_IDS_MAX per launch; the frame rows ride on the last launch
    int done = 0;
    do {
        StepIds ids{};
        const int kk = std::min(VLO_STEP_IDS_MAX, k - done);
        for (int i = 0; i < kk; ++i) ids.v[i] = ids_host[done + i];
        const bool last = done + kk == k;
        HIP_TRY(step_input_launch((const unsigned short *)e->embed, ids, kk, (const unsigned short *)frame_rows_dev, last ? rows : 0, H,
                                  e->cfg.vocab_size, out + (size_t)done * H, (hipStream_t)stream));
        done += kk;
    } while (done < k);
    return VLO_OK;
}

int vlo_steps_input(vlo_engine *e, const int64_t *ids_host, const int *k_host, int units, const void *frame_rows_dev, int rows_per_unit,
                    void *out_dev, void *stream) {
    if (!e || !out_dev || !k_host || units < 1 || units > VLO_STEPS_UNITS_MAX || rows_per_unit < 0 || (rows_per_unit > 0 && !frame_rows_dev))
        return fail(VLO_E_INVALID, "bad steps_input arguments (1.." + std::to_string(VLO_STEPS_UNITS_MAX) + " units)");
    if (!e->finalized) return fail(VLO_E_STATE, "engine not finalized");
    StepsIds ids{};
    for (int u = 0; u < units; ++u) {
        const int k = k_host[u], kmax = u ? VLO_STEPS_IDS_LATER : VLO_STEP_IDS_MAX;
        if (k < 0 || k > kmax || (k > 0 && !ids_host) || k + rows_per_unit < 1)
            return fail(VLO_E_INVALID, "steps_input: unit " + std::to_string(u) + " carries " + std::to_string(k) + " ids (at most " + std::to_string(kmax) +
                                           "; a unit has at least one row)");
        for (int i = 0; i < k; ++i) ids.v[ids.id0[u] + i] = ids_host[ids.id0[u] + i];
        ids.id0[u + 1] = ids.id0[u] + k;
        ids.row0[u + 1] = ids.row0[u] + k + rows_per_unit;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(steps_input_launch((const unsigned short *)e->embed, ids, units, (const unsigned short *)frame_rows_dev, rows_per_unit, e->cfg.hidden_size,
                               e->cfg.vocab_size, (unsigned short *)out_dev, (hipStream_t)stream));
    return VLO_OK;
}

// ---- stream lookahead: a backlog of silent frame steps of ONE session in one weight pass -------------------------------------------------
// After a silent frame the sampled token is the interval token, so the next step's input is known before it runs: `units` queued step inputs
// go through the decoder as one causal pass of n rows (run_chunk's sequence up to 16 rows, run_block's above), only the unit-end rows take
// the final norm and the lm_head (one 16-row GEMV: the head's weights are streamed once), and the rows sampler decides each.  The pass
// leaves the session PENDING: its K / V lie behind `len`, the commit keeps the units up to the first that speaks and crops the rest.
int vlo_stream_steps(vlo_session *s, const void *embeds_dev, int n, const int *unit_end_host, int units, float threshold, int interval_id,
                     int64_t *tok_dev, float *p_interval_dev, int *n_accept_dev, void *stream) {
    if (!s || !embeds_dev || !unit_end_host || !tok_dev || !n_accept_dev) return fail(VLO_E_INVALID, "bad stream_steps arguments");
    vlo_engine *e = s->e;
    if (e->tp_size > 1) return fail(VLO_E_STATE, "tensor-parallel engine: stream_steps is not supported");
    if (int prc = pending_refusal(s, "stream_steps")) return prc;
    if (units < 1 || units > VLO_ROWIDX_MAX) return fail(VLO_E_INVALID, "stream_steps: " + std::to_string(units) + " units (1.." + std::to_string(VLO_ROWIDX_MAX) + ")");
    if (n < 1 || n > VLO_BLOCK_TOKENS) return fail(VLO_E_INVALID, "stream_steps: " + std::to_string(n) + " rows (1.." + std::to_string(VLO_BLOCK_TOKENS) + ")");
    for (int k = 0; k < units; ++k)
        if (unit_end_host[k] < (k ? unit_end_host[k - 1] + 1 : 0) || unit_end_host[k] >= n)
            return fail(VLO_E_INVALID, "stream_steps: unit_end must be strictly ascending inside [0, n)");
    if (unit_end_host[units - 1] != n - 1) return fail(VLO_E_INVALID, "stream_steps: the last unit must end at row n - 1");
    const vlo_config &c = e->cfg;
    const int H = c.hidden_size, V = c.vocab_size;
    if (interval_id < 0 || interval_id >= V) return fail(VLO_E_INVALID, "stream_steps: interval_id outside the vocabulary");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const bool block = n > 16;
    int rc = 0;
    if (block && (rc = ensure_block_ws(s))) return rc;
    alloc_owned(rc, s->owned, &s->steps_scratch, (size_t)VLO_ROWIDX_MAX * VLO_SAMPLE_SCRATCH_FLOATS * 4);
    if (rc) return rc;
    if ((rc = ensure_pages(s, s->len + n, st))) return rc;          // all or nothing: a pool that cannot hold the pass leaves the session as it was
    const StepWs &w = block ? s->bws : s->ws;
    HIP_TRY(copy_rows_launch((const unsigned short *)embeds_dev, w.h, n, H, st));
    PendingDown pd;
    if ((rc = decoder_layers(e, w, n, block, solo_rows(s), false, st, &pd))) return rc;
    // ---- the tail: final norm of the unit-end rows only (gathered into x rows 0 .. units - 1), one lm_head GEMV, the rows sampler
    RowIdx rows{};
    for (int k = 0; k < units; ++k) rows.v[k] = unit_end_host[k];
    HIP_TRY(add_rmsnorm_gather_launch(w.h, pd.partial, pd.ksplit, H, (const unsigned short *)e->norm_w, w.x, H, c.rms_eps, rows, units, n, st));
    GemvArgs a = gemv_args(e->lm_head, w.x, H, units);
    a.out_bf16 = s->logits; a.ldo = V;
    HIP_TRY(gemv_launch(a, e->lm_head.plan, XSRC_PLAIN, EPI_BF16, st));
    HIP_TRY(stream_sample_steps_launch(s->logits, units, V, threshold, interval_id, tok_dev, p_interval_dev, n_accept_dev, s->steps_scratch, st));
    s->has_logits = false;                       // the old last row's logits are overwritten; the commit names the new last row
    s->pend_units = units;
    for (int k = 0; k < units; ++k) s->pend_end[k] = unit_end_host[k];
    return VLO_OK;
}

int vlo_stream_steps_commit(vlo_session *s, int keep_units) {
    if (!s) return fail(VLO_E_INVALID, "null session");
    if (!s->pend_units) return fail(VLO_E_STATE, "stream_steps_commit: no pass is pending");
    if (keep_units < 1 || keep_units > s->pend_units)
        return fail(VLO_E_INVALID, "stream_steps_commit: keep " + std::to_string(keep_units) + " of " + std::to_string(s->pend_units) + " units");
    vlo_engine *e = s->e;
    const int64_t nl = s->len + s->pend_end[keep_units - 1] + 1;
    const size_t keep = (size_t)((nl + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS);
    if (keep < s->pages.size()) {
        // as session_crop_shard: pages wholly behind the kept units go back to the pool once the pass that wrote them has drained
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipDeviceSynchronize());
        std::lock_guard<std::mutex> g(e->pool_mu);
        while (s->pages.size() > keep) {
            e->free_pages.push_back(s->pages.back());
            s->pages.pop_back();
        }
    }
    s->len = nl;
    s->last_logits = s->logits + (size_t)(keep_units - 1) * e->cfg.vocab_size;
    s->has_logits = true;
    s->pend_units = 0;
    return VLO_OK;
}

int vlo_greedy_generate(vlo_session *s, const void *embeds_dev, int m, int eos_token_id, int64_t *out_ids_dev, int max_new,
                        int force_len, int *n_written, void *stream) {
    if (!s || !embeds_dev || !out_ids_dev || m <= 0 || max_new <= 0) return fail(VLO_E_INVALID, "bad greedy_generate arguments");
    if (int prc = pending_refusal(s, "greedy_generate")) return prc;
    vlo_engine *e = s->e;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const int V = e->cfg.vocab_size;
    if (force_len > max_new) force_len = max_new;
    int rc = vlo_llm_step(s, embeds_dev, m, nullptr, nullptr, stream);
    if (rc) return rc;
    for (hipEvent_t &ev : s->tok_ev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    const bool forced = force_len > 0;
    int i = 0;
    for (;; ++i) {
        int mode = 0;
        if (forced) mode = (i == force_len - 1) ? 2 : 1;
        HIP_TRY(greedy_sample_launch(s->last_logits, V, out_ids_dev + i, eos_token_id, mode, s->sample_scratch, st));
        const bool last = (i == max_new - 1) || (forced && i == force_len - 1);
        if (forced) {
            // scheduled speech (throughput runs): the token count is known, the host never has to look at a token
            if (last) break;
            HIP_TRY(embed_gather_launch((const unsigned short *)e->embed, out_ids_dev + i, 1, e->cfg.hidden_size, V, s->emb1, st));
            if ((rc = vlo_llm_step(s, s->emb1, 1, nullptr, nullptr, stream))) return rc;
            continue;
        }
        // the reference reads every token on the host (`if new_token_id == eos_token_id`, :179).  Here the read is asynchronous
        // and the NEXT step is enqueued before the host waits for it, so the GPU never idles across the host round trip; if the
        // token turns out to be EOS, the speculative step is undone by forgetting its one KV position (nothing reads it again).
        volatile int64_t *slot = s->host_tok + (i & 1);
        HIP_TRY(hipMemcpyAsync((void *)slot, out_ids_dev + i, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(s->tok_ev[i & 1], st));
        // speculate only when the step needs nothing it could fail to get: a position inside the pages the session already owns.
        // (An EOS on the last KV slot, or one page short of an exhausted pool, must end the response as the reference's loop
        // does, not fail on a step that would be thrown away.)
        const bool spec = !last && s->len + 1 <= (int64_t)s->pages.size() * VLO_PAGE_TOKENS && s->len + 1 <= e->max_positions;
        if (spec) {
            HIP_TRY(embed_gather_launch((const unsigned short *)e->embed, out_ids_dev + i, 1, e->cfg.hidden_size, V, s->emb1, st));
            if ((rc = vlo_llm_step(s, s->emb1, 1, nullptr, nullptr, stream))) return rc;
        }
        HIP_TRY(hipEventSynchronize(s->tok_ev[i & 1]));
        if (*slot == eos_token_id) {
            if (spec) s->len -= 1;           // the EOS token is never fed to the model (:179-181)
            // same session state after EOS on both paths: the logits that produced EOS are consumed (the speculative step has
            // overwritten them anyway), a sampler call needs a new step first
            s->has_logits = false;
            break;
        }
        if (last) break;
        if (!spec) {                         // the blocking order of the reference: token known, then the step (which may need a page)
            HIP_TRY(embed_gather_launch((const unsigned short *)e->embed, out_ids_dev + i, 1, e->cfg.hidden_size, V, s->emb1, st));
            if ((rc = vlo_llm_step(s, s->emb1, 1, nullptr, nullptr, stream))) { if (n_written) *n_written = i + 1; return rc; }
        }
    }
    HIP_TRY(hipStreamSynchronize(st));        // the ids are read by the caller right away
    if (n_written) *n_written = i + 1;
    return VLO_OK;
}

// ---- batched steps: the live steps of several sessions in one weight pass ---------------------------------------------------------------
// A step streams the whole weight image whatever its row count (gemv_plan depends on K only; rows past n_rows are loaded anyway), so the rows
// of B sessions share it: the qkv epilogue takes each row's position and KV page from a row table (EPI_ROPE_ROWS), attention runs one segment
// per (session, 16-query sub-chunk) with that session's page table and its solo split geometry (llm_ops.h AttnSeg), the combine writes every
// segment's rows back in place, and the last row of each session goes through the lm_head and back to the session.
int vlo_batch_create(vlo_engine *e, int max_sessions, vlo_batch **out) {
    if (!e || !out) return fail(VLO_E_INVALID, "null argument");
    if (!e->finalized) return fail(VLO_E_STATE, "engine not finalized");
    if (e->tp_size > 1) return fail(VLO_E_STATE, "tensor-parallel engine: batched steps are not supported");
    if (max_sessions < 1 || max_sessions > VLO_BATCH_MAX) return fail(VLO_E_INVALID, "max_sessions must be 1.." + std::to_string(VLO_BATCH_MAX));
    const vlo_config &c = e->cfg;
    if (c.vocab_size & 7) return fail(VLO_E_UNSUPPORTED, "batched steps need vocab_size % 8 == 0");
    HIP_TRY(hipSetDevice(e->device));
    const size_t H = c.hidden_size, hd = e->head_dim, V = c.vocab_size;
    vlo_batch *b = new vlo_batch();
    b->e = e;
    b->max_sessions = max_sessions;
    StepWs &w = b->ws;
    int ksmax = 1;
    for (auto &L : e->layers) ksmax = std::max(ksmax, L.down.plan.ksplit);
    w.part_cap = max_sessions * attention_states_bound(e->nkv_l);
    int rc = 0;
    auto A = [&](auto **p, size_t bytes) { alloc_owned(rc, b->owned, p, bytes); };
    alloc_block_rows(rc, b->owned, e, w, true);
    A(&b->xl, (size_t)16 * H * 2);
    A(&b->emb, (size_t)16 * H * 2);
    A(&w.partial, (size_t)ksmax * 16 * H * 4);
    A(&w.sq[0], (size_t)(512 + 16) * 16 * 4);
    A(&w.sq[1], (size_t)(512 + 16) * 16 * 4);
    A(&w.part_o, (size_t)w.part_cap * e->nh_l * 16 * hd * 4);
    A(&w.part_ml, (size_t)w.part_cap * e->nh_l * 16 * 2 * 4);
    A(&b->logits, (size_t)max_sessions * V * 2);
    A(&b->sample_scratch, (size_t)max_sessions * VLO_SAMPLE_SCRATCH_FLOATS * 4);
    A(&b->tok, (size_t)max_sessions * 8);
    A(&b->tables_dev, sizeof(BatchTables) * VLO_BATCH_SLOTS);
    if (rc) {
        vlo_batch_destroy(b);
        return rc;
    }
    if (hipHostMalloc((void **)&b->host_tok, VLO_BATCH_MAX * 8, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&b->stage, sizeof(BatchTables) * VLO_BATCH_SLOTS, hipHostMallocDefault) != hipSuccess) {
        vlo_batch_destroy(b);
        return fail(VLO_E_HIP, "hipHostMalloc failed");
    }
    for (hipEvent_t &ev : b->slot_ev)
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            vlo_batch_destroy(b);
            return fail(VLO_E_HIP, "hipEventCreate failed");
        }
    HIP_TRY(hipDeviceSynchronize());
    *out = b;
    return VLO_OK;
}

void vlo_batch_destroy(vlo_batch *b) {
    if (!b) return;
    hipSetDevice(b->e->device);
    hipDeviceSynchronize();
    for (void *p : b->owned) hipFree(p);
    if (b->host_tok) hipHostFree(b->host_tok);
    if (b->stage) hipHostFree(b->stage);
    for (hipEvent_t ev : b->slot_ev) if (ev) hipEventDestroy(ev);
    delete b;
}

// the refusals every batched call shares
static int batch_check(const vlo_batch *b, vlo_session *const *ss, int B, const int *n, int *rows_total) {
    if (!b || !ss || !n) return fail(VLO_E_INVALID, "null argument");
    if (B < 1 || B > b->max_sessions) return fail(VLO_E_INVALID, "batch of " + std::to_string(B) + " sessions (max_sessions " + std::to_string(b->max_sessions) + ")");
    if (b->e->tp_size > 1) return fail(VLO_E_STATE, "tensor-parallel engine: batched steps are not supported");
    int M = 0;
    for (int i = 0; i < B; ++i) {
        if (!ss[i]) return fail(VLO_E_INVALID, "null session " + std::to_string(i));
        if (ss[i]->e != b->e) return fail(VLO_E_INVALID, "session " + std::to_string(i) + " belongs to another engine");
        if (int prc = pending_refusal(ss[i], "batched step")) return prc;
        for (int j = 0; j < i; ++j)
            if (ss[j] == ss[i]) return fail(VLO_E_INVALID, "session " + std::to_string(i) + " repeats session " + std::to_string(j));
        if (n[i] < 1) return fail(VLO_E_INVALID, "session " + std::to_string(i) + " appends " + std::to_string(n[i]) + " tokens (>= 1)");
        M += n[i];
    }
    *rows_total = M;
    return VLO_OK;
}

// KV pages of every session for its new length, all or nothing: no page is taken unless all fit (and whatever was taken goes back on failure)
static int batch_pages(vlo_session *const *ss, int B, const int *n, hipStream_t st) {
    vlo_engine *e = ss[0]->e;
    int need = 0;
    for (int i = 0; i < B; ++i) {
        const int64_t L = ss[i]->len + n[i];
        if (L > e->max_positions) return fail(VLO_E_NOMEM, "session " + std::to_string(i) + ": sequence exceeds kv_pool_tokens");
        need += std::max(0, (int)((L + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS) - (int)ss[i]->pages.size());
    }
    {
        std::lock_guard<std::mutex> g(e->pool_mu);
        if ((int)e->free_pages.size() < need)
            return fail(VLO_E_NOMEM, "KV pool exhausted: the batch needs " + std::to_string(need) + " pages, " + std::to_string(e->free_pages.size()) + " free");
    }
    size_t had[VLO_BATCH_MAX];
    for (int i = 0; i < B; ++i) had[i] = ss[i]->pages.size();
    for (int i = 0; i < B; ++i) {
        const int rc = ensure_pages(ss[i], ss[i]->len + n[i], st);
        if (rc) {                                      // another thread took pages in between: hand back what this call took
            std::lock_guard<std::mutex> g(e->pool_mu);
            for (int j = 0; j < i; ++j) {
                for (size_t p = had[j]; p < ss[j]->pages.size(); ++p) e->free_pages.push_back(ss[j]->pages[p]);
                ss[j]->pages.resize(had[j]);
            }
            return rc;
        }
    }
    return VLO_OK;
}

int vlo_batch_step(vlo_batch *b, vlo_session *const *ss, int B, const void *embeds_dev, const int *n_host, void *last_logits_dev, void *stream) {
    int M = 0, rc;
    if ((rc = batch_check(b, ss, B, n_host, &M))) return rc;
    if (!embeds_dev) return fail(VLO_E_INVALID, "null embeddings");
    if (M > VLO_BLOCK_TOKENS) return fail(VLO_E_INVALID, "batch of " + std::to_string(M) + " rows: at most " + std::to_string(VLO_BLOCK_TOKENS) + " (split the batch)");
    vlo_engine *e = b->e;
    const vlo_config &c = e->cfg;
    const StepWs &w = b->ws;
    const int H = c.hidden_size, V = c.vocab_size;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = batch_pages(ss, B, n_host, st))) return rc;

    // ---- this step's tables (slot k of the ring)
    const int k = b->slot;
    if (b->slot_used[k]) HIP_TRY(hipEventSynchronize(b->slot_ev[k]));      // the step that last used slot k has read it
    BatchTables &T = b->stage[k];
    const int *tables[VLO_BATCH_MAX];
    int64_t lens[VLO_BATCH_MAX];
    int rows[VLO_BATCH_MAX];
    for (int i = 0, r = 0; i < B; ++i) {
        const vlo_session *s = ss[i];
        tables[i] = s->page_table;
        lens[i] = s->len;
        rows[i] = r;
        for (int j = 0; j < n_host[i]; ++j, ++r) {
            const int64_t pos = s->len + j;
            T.rows[r].pos = (int)pos;
            T.rows[r].page = s->pages[pos / VLO_PAGE_TOKENS];
        }
    }
    BatchTables *Td = b->tables_dev + k;
    AttnSegRun runs[4];
    KvRows at;
    at.kv = kv_geom(ss[0]);                            // pool geometry (each segment / row carries its own pages)
    at.rows = Td->rows; at.segs = Td->segs; at.runs = runs;
    int states = 0;
    HIP_TRY(attention_seg_plan(at.kv, e->nh_l, B, tables, lens, n_host, rows, w.part_cap, T.segs, &at.nseg, runs, &at.nrun, &states));
    HIP_TRY(hipMemcpyAsync(Td, &T, sizeof(BatchTables), hipMemcpyHostToDevice, st));

    // ---- the decoder layers: the 16-row pipeline (M <= 16) or the block pipeline (17..64 rows)
    HIP_TRY(copy_rows_launch((const unsigned short *)embeds_dev, w.h, M, H, st));
    PendingDown pd;
    if ((rc = decoder_layers(e, w, M, M > 16, at, false, st, &pd))) return rc;
    // ---- each session's last row: final norm, gathered into B rows, one lm_head pass, scattered to the sessions
    HIP_TRY(add_rmsnorm_launch(w.h, pd.partial, pd.ksplit, H, (const unsigned short *)e->norm_w, w.x, H, H, c.rms_eps, M, st));
    RowCopy g{}, sc{};
    for (int i = 0; i < B; ++i) {
        g.src[i] = w.x + (size_t)(rows[i] + n_host[i] - 1) * H;
        g.dst[i] = b->xl + (size_t)i * H;
        sc.src[i] = b->logits + (size_t)i * V;
        sc.dst[i] = ss[i]->logits;
    }
    HIP_TRY(copy_rows_indexed_launch(g, B, H, st));
    {
        GemvArgs a = gemv_args(e->lm_head, b->xl, H, B);
        a.out_bf16 = b->logits; a.ldo = V;
        HIP_TRY(gemv_launch(a, e->lm_head.plan, XSRC_PLAIN, EPI_BF16, st));
    }
    HIP_TRY(copy_rows_indexed_launch(sc, B, V, st));
    if (last_logits_dev) HIP_TRY(hipMemcpyAsync(last_logits_dev, b->logits, (size_t)B * V * 2, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipEventRecord(b->slot_ev[k], st));
    b->slot_used[k] = true;
    b->slot = (k + 1) % VLO_BATCH_SLOTS;
    for (int i = 0; i < B; ++i) {
        vlo_session *s = ss[i];
        s->last_logits = s->logits;
        s->has_logits = true;
        s->len += n_host[i];
    }
    b->last_B = B;
    return VLO_OK;
}

int vlo_batch_stream_sample(vlo_batch *b, float threshold, int interval_id, int64_t *tok_dev, float *p_interval_dev, void *stream) {
    if (!b || !tok_dev) return fail(VLO_E_INVALID, "bad batch_stream_sample arguments");
    if (!b->last_B) return fail(VLO_E_STATE, "no logits: call vlo_batch_step first");
    HIP_TRY(hipSetDevice(b->e->device));
    HIP_TRY(stream_sample_rows_launch(b->logits, b->last_B, b->e->cfg.vocab_size, threshold, interval_id, tok_dev, p_interval_dev,
                                      b->sample_scratch, (hipStream_t)stream));
    return VLO_OK;
}

// Non-speculative: per decode step one batched argmax, one copy of the active sessions' tokens to the host, then the host drops the sessions
// that are done and steps the others.  Each session's ids, length and logits end as vlo_greedy_generate leaves them (force_len = 0).
int vlo_batch_greedy_generate(vlo_batch *b, vlo_session *const *ss, int B, const void *embeds_dev, const int *m_host, int eos_token_id,
                              int64_t *out_ids_dev, int max_new, int *n_written_host, void *stream) {
    int M = 0, rc;
    if ((rc = batch_check(b, ss, B, m_host, &M))) return rc;
    if (!embeds_dev || !out_ids_dev || !n_written_host || max_new <= 0) return fail(VLO_E_INVALID, "bad batch_greedy_generate arguments");
    vlo_engine *e = b->e;
    const int H = e->cfg.hidden_size, V = e->cfg.vocab_size;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    std::vector<std::vector<int64_t>> ids(B);
    auto finish = [&]() -> int {                   // the ids go to the caller's rows (each row's first n_written entries)
        for (int i = 0; i < B; ++i) {
            n_written_host[i] = (int)ids[i].size();
            if (!ids[i].empty())
                HIP_TRY(hipMemcpy(out_ids_dev + (size_t)i * max_new, ids[i].data(), ids[i].size() * 8, hipMemcpyHostToDevice));
        }
        b->last_B = 0;                             // the batch's logits rows no longer follow the sessions' order
        return VLO_OK;
    };
    for (int i = 0; i < B; ++i) n_written_host[i] = 0;
    if (M <= 16) {
        if ((rc = vlo_batch_step(b, ss, B, embeds_dev, m_host, nullptr, stream))) return rc;
    } else {                                       // long prefixes: each session's own vlo_llm_step, then its logits row into the batch's matrix
        RowCopy g{};
        for (int i = 0, r = 0; i < B; r += m_host[i], ++i) {
            if ((rc = vlo_llm_step(ss[i], (const unsigned short *)embeds_dev + (size_t)r * H, m_host[i], nullptr, nullptr, stream))) return rc;
            g.src[i] = ss[i]->last_logits;
            g.dst[i] = b->logits + (size_t)i * V;
        }
        HIP_TRY(copy_rows_indexed_launch(g, B, V, st));
    }
    std::vector<vlo_session *> act(ss, ss + B);
    std::vector<int> idx(B);
    for (int i = 0; i < B; ++i) idx[i] = i;
    for (int i = 0;; ++i) {
        const int nA = (int)act.size();
        HIP_TRY(greedy_sample_rows_launch(b->logits, nA, V, b->tok, b->sample_scratch, st));
        HIP_TRY(hipMemcpyAsync(b->host_tok, b->tok, (size_t)nA * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<vlo_session *> keep;
        std::vector<int> keep_idx;
        StepIds next{};
        for (int r = 0; r < nA; ++r) {
            const int64_t t = b->host_tok[r];
            ids[idx[r]].push_back(t);
            if (t == eos_token_id) {
                act[r]->has_logits = false;        // the EOS is not fed; the logits that produced it are consumed (vlo_greedy_generate)
            } else if (i < max_new - 1) {
                next.v[keep.size()] = t;
                keep.push_back(act[r]);
                keep_idx.push_back(idx[r]);
            }
        }
        if (keep.empty()) break;
        const int k = (int)keep.size();
        HIP_TRY(step_input_launch((const unsigned short *)e->embed, next, k, nullptr, 0, H, V, b->emb, st));
        const std::vector<int> ones(k, 1);
        if ((rc = vlo_batch_step(b, keep.data(), k, b->emb, ones.data(), nullptr, stream))) {
            const std::string msg = vlo_last_error();
            finish();
            return fail(rc, msg);
        }
        act.swap(keep);
        idx.swap(keep_idx);
    }
    return finish();
}

// connector scratch (allocated outside any stream capture)
int vlo_connector_reserve(vlo_engine *e) {
    if (e->conn_x) return VLO_OK;
    const int H = e->cfg.hidden_size, Hv = e->cfg.vision_hidden_size;
    int rc;
    if ((rc = dev_alloc(&e->conn_x, (size_t)2 * 32 * Hv * 2))) return rc;
    if ((rc = dev_alloc(&e->conn_mid, (size_t)2 * 32 * H * 2))) return rc;
    if ((rc = dev_alloc(&e->conn_out, (size_t)2 * 32 * H * 2))) return rc;
    e->owned.push_back(e->conn_x);
    e->owned.push_back(e->conn_mid);
    e->owned.push_back(e->conn_out);
    HIP_TRY(hipMemset(e->conn_x, 0, (size_t)2 * 32 * Hv * 2));
    HIP_TRY(hipMemset(e->conn_mid, 0, (size_t)2 * 32 * H * 2));
    return VLO_OK;
}

int connector_run(vlo_engine *e, int slot, const void *feats_dev, int rows, void *out_dev, hipStream_t st) {
    const int H = e->cfg.hidden_size, Hv = e->cfg.vision_hidden_size;
    int rc;
    if ((rc = vlo_connector_reserve(e))) return rc;
    unsigned short *cx = (unsigned short *)e->conn_x + (size_t)slot * 32 * Hv, *cm = (unsigned short *)e->conn_mid + (size_t)slot * 32 * H,
                   *co = (unsigned short *)e->conn_out + (size_t)slot * 32 * H;
    for (int r0 = 0; r0 < rows; r0 += 16) {
        const int m = std::min(16, rows - r0);
        HIP_TRY(copy_rows_launch((const unsigned short *)feats_dev + (size_t)r0 * Hv, cx, m, Hv, st));
        {
            GemvArgs a = gemv_args(e->conn0, cx, Hv, m);
            a.out_bf16 = cm; a.ldo = H; a.bias = (const unsigned short *)e->conn0_b;
            HIP_TRY(gemv_launch(a, e->conn0.plan, XSRC_PLAIN, EPI_BF16_GELU_ERF, st));
        }
        {
            GemvArgs a = gemv_args(e->conn2, cm, H, m);
            a.out_bf16 = co; a.ldo = H; a.bias = (const unsigned short *)e->conn2_b;
            HIP_TRY(gemv_launch(a, e->conn2.plan, XSRC_PLAIN, EPI_BF16, st));
        }
        HIP_TRY(copy_rows_launch(co, (unsigned short *)out_dev + (size_t)r0 * H, m, H, st));
    }
    return VLO_OK;
}

int vlo_connector(vlo_engine *e, const void *feats_dev, int rows, void *out_dev, void *stream) {
    if (!e || !feats_dev || !out_dev || rows <= 0) return fail(VLO_E_INVALID, "bad connector arguments");
    if (!e->finalized || !e->has_connector) return fail(VLO_E_STATE, "connector weights not loaded");
    HIP_TRY(hipSetDevice(e->device));
    return connector_run(e, 0, feats_dev, rows, out_dev, (hipStream_t)stream);
}

int vlo_visual_embed(vlo_engine *e, const uint8_t *frames_dev, int B, void *out_dev, void *stream) {
    if (!e || !frames_dev || !out_dev || B <= 0) return fail(VLO_E_INVALID, "bad visual_embed arguments");
    if (!e->finalized || !e->cfg.has_vit || !e->vit) return fail(VLO_E_STATE, "engine built without a vision tower");
    HIP_TRY(hipSetDevice(e->device));
    return vit_visual_embed(e, frames_dev, B, out_dev, (hipStream_t)stream);
}

int vlo_vision_tokens(vlo_engine *e, const uint8_t *frames_dev, int B, void *out_dev, void *stream) {
    if (!e || !frames_dev || !out_dev || B <= 0) return fail(VLO_E_INVALID, "bad vision_tokens arguments");
    if (!e->finalized || !e->cfg.has_vit || !e->vit) return fail(VLO_E_STATE, "engine built without a vision tower");
    HIP_TRY(hipSetDevice(e->device));
    return vit_vision_tokens(e, frames_dev, B, out_dev, (hipStream_t)stream);
}

int vlo_session_read_kv(vlo_session *s, int layer, int which, int kv_head, int64_t t0, int64_t t1, void *dst_dev, void *stream) {
    if (!s || !dst_dev || layer < 0 || layer >= s->e->cfg.num_layers || kv_head < 0 || kv_head >= s->e->nkv_l ||
        t0 < 0 || t1 > s->len || t1 < t0)
        return fail(VLO_E_INVALID, "bad read_kv arguments");
    if (int prc = pending_refusal(s, "read_kv")) return prc;
    HIP_TRY(hipSetDevice(s->e->device));
    HIP_TRY(read_kv_launch(kv_geom(s), layer, which, kv_head, t0, t1, (unsigned short *)dst_dev, (hipStream_t)stream));
    return VLO_OK;
}

// ---- teacher-forced evaluation surface (models/modeling_live.py:29-42, 44-168, 170-171) -------------------------------
int vlo_joint_embed(vlo_engine *e, const int64_t *ids_dev, int k, int64_t v_placeholder_id, const void *frame_rows_dev,
                    int n_frame_rows, void *out_dev, void *stream) {
    if (!e || !ids_dev || !out_dev || k <= 0 || n_frame_rows < 0 || (n_frame_rows > 0 && !frame_rows_dev))
        return fail(VLO_E_INVALID, "bad joint_embed arguments");
    if (!e->finalized) return fail(VLO_E_STATE, "engine not finalized");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    int *scratch = nullptr;
    HIP_TRY(hipMalloc((void **)&scratch, ((size_t)k + 1) * sizeof(int)));
    hipError_t he = joint_embed_launch((const unsigned short *)e->embed, ids_dev, k, v_placeholder_id, (const unsigned short *)frame_rows_dev,
                                       n_frame_rows, e->cfg.hidden_size, e->cfg.vocab_size, scratch, scratch + k,
                                       (unsigned short *)out_dev, st);
    int count = -1;
    if (he == hipSuccess) he = hipMemcpyAsync(&count, scratch + k, sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    hipFree(scratch);
    HIP_TRY(he);
    // `inputs_embeds[v_mask] = self.visual_embed(frames)` raises on a shape mismatch (:41)
    if (count != n_frame_rows)
        return fail(VLO_E_INVALID, std::to_string(count) + " placeholder positions but " + std::to_string(n_frame_rows) +
                                       " frame-token embeddings");
    return VLO_OK;
}

int vlo_logit_rows(vlo_engine *e, const void *logits_dev, int n, const int64_t *labels_dev, int interval_id, float *lse_dev,
                   int64_t *argmax_dev, float *label_logit_dev, float *p_interval_dev, int64_t *p_argmax_dev, void *stream) {
    if (!e || !logits_dev || n <= 0 || !lse_dev || !argmax_dev || !label_logit_dev || !p_interval_dev || !p_argmax_dev)
        return fail(VLO_E_INVALID, "bad logit_rows arguments");
    HIP_TRY(hipSetDevice(e->device));
    const int V = e->cfg.vocab_size;
    HIP_TRY(logit_rows_launch((const unsigned short *)logits_dev, n, V, V, labels_dev, interval_id, lse_dev, argmax_dev, label_logit_dev,
                              p_interval_dev, p_argmax_dev, (hipStream_t)stream));
    return VLO_OK;
}

// fork / crop of ONE KV shard (a whole TP = 1 session, or one rank's shard of a tensor-parallel session: tp.hip)
int session_fork_shard(vlo_session *src, int64_t n_tokens, vlo_session **out, void *stream) {
    if (!src || !out || n_tokens < 0 || n_tokens > src->len) return fail(VLO_E_INVALID, "bad session_fork arguments");
    if (int prc = pending_refusal(src, "session_fork")) return prc;
    vlo_engine *e = src->e;
    hipStream_t st = (hipStream_t)stream;
    vlo_session *d = nullptr;
    int rc = vlo_session_create(e, n_tokens, &d);
    if (rc) return rc;
    if ((rc = ensure_pages(d, n_tokens, st))) {
        vlo_session_destroy(d);
        return rc;
    }
    const int pages = (int)((n_tokens + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS);
    hipError_t he = kv_copy_pages_launch(kv_geom(src), src->page_table, d->page_table, pages, e->cfg.num_layers, st);
    if (he != hipSuccess) {
        vlo_session_destroy(d);
        HIP_TRY(he);
    }
    d->len = n_tokens;
    *out = d;
    return VLO_OK;
}

int vlo_session_fork(vlo_session *src, int64_t n_tokens, vlo_session **out, void *stream) {
    if (src && src->e->tp_size > 1) return fail(VLO_E_STATE, "a tensor-parallel shard is forked through vlo_tp_session_fork");
    return session_fork_shard(src, n_tokens, out, stream);
}

int session_crop_shard(vlo_session *s, int64_t n_tokens) {
    if (!s || n_tokens < 0 || n_tokens > s->len) return fail(VLO_E_INVALID, "bad session_crop arguments");
    if (int prc = pending_refusal(s, "session_crop")) return prc;
    vlo_engine *e = s->e;
    const size_t keep = (size_t)((n_tokens + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS);
    if (keep < s->pages.size()) {
        // pages go back to the pool (and page-table slots will be rewritten): let queued kernels that still read them drain
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipDeviceSynchronize());
        std::lock_guard<std::mutex> g(e->pool_mu);
        while (s->pages.size() > keep) {
            e->free_pages.push_back(s->pages.back());
            s->pages.pop_back();
        }
    }
    s->len = n_tokens;
    s->has_logits = false;
    return VLO_OK;
}

int vlo_session_crop(vlo_session *s, int64_t n_tokens) {
    if (s && s->e->tp_size > 1) return fail(VLO_E_STATE, "a tensor-parallel shard is cropped through vlo_tp_session_crop");
    return session_crop_shard(s, n_tokens);
}

// eviction of ONE KV shard: positions [t0, t1) leave the cache, the tail moves down by d = t1 - t0 slots with its keys rotated back by d
// positions (llm_ops.hip kv_evict_kernel), so `len` is again the next position and no step kernel changes
int session_evict_shard(vlo_session *s, int64_t t0, int64_t t1, void *stream) {
    if (!s) return fail(VLO_E_INVALID, "bad session_evict arguments");
    if (int prc = pending_refusal(s, "session_evict")) return prc;
    vlo_engine *e = s->e;
    if (e->cfg.kv_dtype != VLO_KV_BF16)
        return fail(VLO_E_UNSUPPORTED, "session_evict: an fp8 KV pool is not re-rotated (every eviction would re-round the surviving keys to e4m3)");
    if (t0 < 0 || t1 < t0 || t1 > s->len) return fail(VLO_E_INVALID, "bad session_evict arguments: need 0 <= t0 <= t1 <= len");
    const int64_t d = t1 - t0;
    if (d == 0) return VLO_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (t1 < s->len) {
        const int half = e->head_dim / 2;
        if (half > 64 || (int)e->inv_freq_h.size() != half) return fail(VLO_E_UNSUPPORTED, "session_evict: head_dim must be 64 or 128");
        KvEvictRot rot{};
        for (int i = 0; i < half; ++i) {
            const double a = (double)d * (double)e->inv_freq_h[i];
            rot.c[i] = (float)cos(a);
            rot.s[i] = (float)sin(a);
        }
        const hipError_t he = kv_evict_launch(kv_geom(s), e->cfg.num_layers, t0, d, s->len, rot, (hipStream_t)stream);
        if (he == hipErrorNotSupported) return fail(VLO_E_UNSUPPORTED, "session_evict: head_dim must be 64 or 128");
        HIP_TRY(he);
    }
    const int64_t nl = s->len - d;
    const size_t keep = (size_t)((nl + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS);
    if (keep < s->pages.size()) {
        // as session_crop_shard: the pages go back to the pool only after the move above (it reads them) and any queued kernel that still
        // reads them have drained.  The page-table prefix that stays is unchanged: nothing to upload
        HIP_TRY(hipDeviceSynchronize());
        std::lock_guard<std::mutex> g(e->pool_mu);
        while (s->pages.size() > keep) {
            e->free_pages.push_back(s->pages.back());
            s->pages.pop_back();
        }
    }
    s->len = nl;                                 // has_logits stays: the last row's logits are still the last row's
    return VLO_OK;
}

int vlo_session_evict(vlo_session *s, int64_t t0, int64_t t1, void *stream) {
    if (s && s->e->tp_size > 1) return fail(VLO_E_STATE, "a tensor-parallel shard is evicted through vlo_tp_session_evict");
    return session_evict_shard(s, t0, t1, stream);
}

// ---- eviction of several ranges in one pass (vlo.h vlo_session_evict_ranges) --------------------------------------------------------------
int evict_ranges_normalize(const int64_t *ranges_host, int n, int64_t len, std::vector<std::pair<int64_t, int64_t>> *out) {
    out->clear();
    if (n < 0 || (n > 0 && !ranges_host)) return fail(VLO_E_INVALID, "bad session_evict_ranges arguments");
    int64_t prev = 0;
    for (int j = 0; j < n; ++j) {
        const int64_t a = ranges_host[2 * j], b = ranges_host[2 * j + 1];
        if (a < prev || b < a || b > len)
            return fail(VLO_E_INVALID, "bad session_evict_ranges arguments: range " + std::to_string(j) + " = [" + std::to_string(a) + ", " + std::to_string(b) +
                                           "): need 0 <= a <= b <= len, ascending, non-overlapping");
        prev = b;
        if (a == b) continue;
        if (!out->empty() && out->back().second == a) out->back().second = b;
        else out->emplace_back(a, b);
    }
    if (out->size() > VLO_EVICT_MAX_RANGES)
        return fail(VLO_E_INVALID, "session_evict_ranges: " + std::to_string(out->size()) + " ranges after merging (at most " + std::to_string(VLO_EVICT_MAX_RANGES) + " per call)");
    return VLO_OK;
}

// the engine's table ring, allocated at the first call that moves something
static int evict_ring(vlo_engine *e) {
    if (e->evict_dev) return VLO_OK;
    if (!e->evict_stage && hipHostMalloc((void **)&e->evict_stage, sizeof(KvEvictTable) * VLO_EVICT_SLOTS, hipHostMallocDefault) != hipSuccess) {
        e->evict_stage = nullptr;
        return fail(VLO_E_HIP, "hipHostMalloc failed");
    }
    for (hipEvent_t &ev : e->evict_ev)
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    void *p = nullptr;
    if (int rc = dev_alloc(&p, sizeof(KvEvictTable) * VLO_EVICT_SLOTS)) return rc;
    e->evict_dev = (KvEvictTable *)p;
    return VLO_OK;
}

// `ranges`: what evict_ranges_normalize returned for this shard's length.  The survivor run behind range j is segment j; a last range that
// ends at len leaves no run behind it (a crop)
int session_evict_ranges_shard(vlo_session *s, const std::vector<std::pair<int64_t, int64_t>> &ranges, void *stream) {
    if (!s) return fail(VLO_E_INVALID, "bad session_evict_ranges arguments");
    if (int prc = pending_refusal(s, "session_evict_ranges")) return prc;
    vlo_engine *e = s->e;
    if (e->cfg.kv_dtype != VLO_KV_BF16)
        return fail(VLO_E_UNSUPPORTED, "session_evict_ranges: an fp8 KV pool is not re-rotated (every eviction would re-round the surviving keys to e4m3)");
    if (ranges.empty()) return VLO_OK;
    if (ranges.size() > VLO_EVICT_MAX_RANGES || ranges.front().first < 0 || ranges.back().second > s->len)
        return fail(VLO_E_INVALID, "bad session_evict_ranges arguments");
    HIP_TRY(hipSetDevice(e->device));
    const int n_seg = (int)ranges.size() - (ranges.back().second == s->len ? 1 : 0);
    int64_t D = 0;
    for (const auto &r : ranges) D += r.second - r.first;
    const int64_t nl = s->len - D;
    if (n_seg > 0) {
        const int half = e->head_dim / 2;
        if (half > 64 || (e->head_dim != 64 && e->head_dim != 128) || (int)e->inv_freq_h.size() != half)
            return fail(VLO_E_UNSUPPORTED, "session_evict_ranges: head_dim must be 64 or 128");
        std::lock_guard<std::mutex> g(e->evict_mu);
        if (int rc = evict_ring(e)) return rc;
        const int k = e->evict_slot;
        if (e->evict_used[k]) HIP_TRY(hipEventSynchronize(e->evict_ev[k]));   // the call that last used slot k has read it
        KvEvictTable &T = e->evict_stage[k];
        int64_t Dj = 0;
        for (int j = 0; j < n_seg; ++j) {
            Dj += ranges[j].second - ranges[j].first;
            T.w[j] = ranges[j].second - Dj;
            T.D[j] = Dj;
            for (int i = 0; i < half; ++i) {
                const double a = (double)Dj * (double)e->inv_freq_h[i];
                T.c[j][i] = (float)cos(a);
                T.s[j][i] = (float)sin(a);
            }
        }
        T.w[n_seg] = nl;
        // sources end where the last segment's do: at len, or at the start of a last range that reaches len
        const int64_t src_end = nl + Dj;
        hipStream_t st = (hipStream_t)stream;
        HIP_TRY(hipMemcpyAsync(e->evict_dev + k, &T, sizeof(KvEvictTable), hipMemcpyHostToDevice, st));
        const hipError_t he = kv_evict_ranges_launch(kv_geom(s), e->cfg.num_layers, e->evict_dev + k, n_seg, src_end, st);
        if (he == hipErrorNotSupported) return fail(VLO_E_UNSUPPORTED, "session_evict_ranges: head_dim must be 64 or 128");
        HIP_TRY(he);
        HIP_TRY(hipEventRecord(e->evict_ev[k], st));
        e->evict_used[k] = true;
        e->evict_slot = (k + 1) % VLO_EVICT_SLOTS;
    }
    const size_t keep = (size_t)((nl + VLO_PAGE_TOKENS - 1) / VLO_PAGE_TOKENS);
    if (keep < s->pages.size()) {
        // as session_evict_shard: the pages go back only after the move and any queued kernel that still reads them have drained
        HIP_TRY(hipDeviceSynchronize());
        std::lock_guard<std::mutex> g(e->pool_mu);
        while (s->pages.size() > keep) {
            e->free_pages.push_back(s->pages.back());
            s->pages.pop_back();
        }
    }
    s->len = nl;                                 // has_logits stays, as in session_evict_shard
    return VLO_OK;
}

int vlo_session_evict_ranges(vlo_session *s, const int64_t *ranges_host, int n, void *stream) {
    if (!s) return fail(VLO_E_INVALID, "bad session_evict_ranges arguments");
    if (s->e->tp_size > 1) return fail(VLO_E_STATE, "a tensor-parallel shard is evicted through vlo_tp_session_evict_ranges");
    if (int prc = pending_refusal(s, "session_evict_ranges")) return prc;
    if (s->e->cfg.kv_dtype != VLO_KV_BF16)
        return fail(VLO_E_UNSUPPORTED, "session_evict_ranges: an fp8 KV pool is not re-rotated (every eviction would re-round the surviving keys to e4m3)");
    std::vector<std::pair<int64_t, int64_t>> ranges;
    if (int rc = evict_ranges_normalize(ranges_host, n, s->len, &ranges)) return rc;
    return session_evict_ranges_shard(s, ranges, stream);
}

// device scratch of the test / micro-benchmark entry points: freed on every return path
struct ScratchBufs {
    std::vector<void *> ptrs;
    std::vector<hipEvent_t> events;
    ~ScratchBufs() {
        for (void *p : ptrs) hipFree(p);
        for (hipEvent_t e : events) hipEventDestroy(e);
    }
    hipError_t alloc(void **p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    hipError_t event(hipEvent_t *ev) {
        const hipError_t e = hipEventCreate(ev);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
};

int vlo_test_gemv(const void *x_dev, const void *W_dev, float *y_dev, int n, int N, int K, void *stream) {
    if (!x_dev || !W_dev || !y_dev || n <= 0 || n > 16 || N <= 0 || (N & 3)) return fail(VLO_E_INVALID, "bad test_gemv arguments");
    hipStream_t st = (hipStream_t)stream;
    GemvPlan plan;
    // VLO_TEST_GEMV_WHOLE_K=1 (tests): one K slice per block, the waves walk KC chunks — the plan the step's whole-K launches use
    const bool whole_k = getenv("VLO_TEST_GEMV_WHOLE_K") && atoi(getenv("VLO_TEST_GEMV_WHOLE_K"));
    if (gemv_plan(K, !whole_k, &plan)) return fail(VLO_E_UNSUPPORTED, "no GEMV plan for K");
    const int NT = (N + 15) / 16;
    ScratchBufs sc;
    void *Wp = nullptr, *xp = nullptr;
    float *P = nullptr, *Y = nullptr;
    HIP_TRY(sc.alloc(&Wp, (size_t)NT * 16 * K * 2));
    HIP_TRY(sc.alloc(&xp, (size_t)32 * K * 2));
    HIP_TRY(sc.alloc((void **)&P, (size_t)plan.ksplit * 16 * NT * 16 * 4));
    HIP_TRY(sc.alloc((void **)&Y, (size_t)16 * NT * 16 * 4));
    HIP_TRY(hipMemsetAsync(xp, 0, (size_t)32 * K * 2, st));
    HIP_TRY(hipMemcpyAsync(xp, x_dev, (size_t)n * K * 2, hipMemcpyDeviceToDevice, st));
    HIP_TRY(pack_weight_launch(W_dev, Wp, N, K, K, NT, 1, 0, -1, st));
    GemvArgs a{};
    a.Wp = Wp; a.x = (const unsigned short *)xp; a.out_f32 = P;
    a.K = K; a.ldx = K; a.ldo = NT * 16; a.NT = NT; a.N_valid = N; a.n_rows = n;
    HIP_TRY(gemv_launch(a, plan, XSRC_PLAIN, EPI_PARTIAL_F32, st));
    // partial layout is [ksplit][16][ldo]; y is [n][N]: sum into a padded buffer, then copy the rows (ldo may exceed N)
    hipLaunchKernelGGL(sum_partials_kernel, dim3((n * NT * 16 + 255) / 256), dim3(256), 0, st, P, plan.ksplit, NT * 16, Y, n, NT * 16);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(y_dev, (size_t)N * 4, Y, (size_t)NT * 16 * 4, (size_t)N * 4, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // the scratch is freed when `sc` goes out of scope
    return VLO_OK;
}

int vlo_test_gemv_fp8(const void *x_dev, const void *Wq_dev, const float *scale_dev, float *y_dev, int n, int N, int K, void *stream) {
    if (!x_dev || !Wq_dev || !scale_dev || !y_dev || n <= 0 || n > 16 || N <= 0 || (N & 3)) return fail(VLO_E_INVALID, "bad test_gemv_fp8 arguments");
    hipStream_t st = (hipStream_t)stream;
    GemvPlan plan;
    const bool whole_k = getenv("VLO_TEST_GEMV_WHOLE_K") && atoi(getenv("VLO_TEST_GEMV_WHOLE_K"));
    if (gemv_plan(K, !whole_k, &plan)) return fail(VLO_E_UNSUPPORTED, "no GEMV plan for K");
    if ((plan.KF & 1) || !(plan.NW == 8 || (plan.NW == 4 && plan.KF == 14)) || (K & 63)) return fail(VLO_E_UNSUPPORTED, "fp8 weight image needs an even fragment count per wave for this K");
    const int NT = (N + 15) / 16;
    ScratchBufs sc;
    void *Wp = nullptr, *xp = nullptr;
    float *P = nullptr, *Y = nullptr, *sp = nullptr;
    HIP_TRY(sc.alloc(&Wp, (size_t)NT * 16 * K));
    HIP_TRY(sc.alloc(&xp, (size_t)32 * K * 2));
    HIP_TRY(sc.alloc((void **)&sp, (size_t)NT * 16 * 4));
    HIP_TRY(sc.alloc((void **)&P, (size_t)plan.ksplit * 16 * NT * 16 * 4));
    HIP_TRY(sc.alloc((void **)&Y, (size_t)16 * NT * 16 * 4));
    HIP_TRY(hipMemsetAsync(xp, 0, (size_t)32 * K * 2, st));
    HIP_TRY(hipMemcpyAsync(xp, x_dev, (size_t)n * K * 2, hipMemcpyDeviceToDevice, st));
    HIP_TRY(pack_weight_fp8_launch(Wq_dev, scale_dev, Wp, sp, N, K, K, NT, 1, 0, -1, st));
    GemvArgs a{};
    a.Wp = Wp; a.wq = 1; a.wscale = sp; a.x = (const unsigned short *)xp; a.out_f32 = P;
    a.K = K; a.ldx = K; a.ldo = NT * 16; a.NT = NT; a.N_valid = N; a.n_rows = n;
    HIP_TRY(gemv_launch(a, plan, XSRC_PLAIN, EPI_PARTIAL_F32, st));
    hipLaunchKernelGGL(sum_partials_kernel, dim3((n * NT * 16 + 255) / 256), dim3(256), 0, st, P, plan.ksplit, NT * 16, Y, n, NT * 16);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(y_dev, (size_t)N * 4, Y, (size_t)NT * 16 * 4, (size_t)N * 4, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VLO_OK;
}

int vlo_test_gemv_mxfp4(const void *x_dev, const void *codes_dev, const void *scale_dev, float *y_dev, int n, int N, int K, void *stream) {
    if (!x_dev || !codes_dev || !scale_dev || !y_dev || n <= 0 || n > 16 || N <= 0 || (N & 3)) return fail(VLO_E_INVALID, "bad test_gemv_mxfp4 arguments");
    hipStream_t st = (hipStream_t)stream;
    GemvPlan plan;
    const bool whole_k = getenv("VLO_TEST_GEMV_WHOLE_K") && atoi(getenv("VLO_TEST_GEMV_WHOLE_K"));
    if ((K & 127) || gemv_plan(K, !whole_k, &plan, 2)) return fail(VLO_E_UNSUPPORTED, "no mxfp4 GEMV plan for K=" + std::to_string(K));
    const int NT = (N + 15) / 16;
    ScratchBufs sc;
    void *Wp = nullptr, *Sp = nullptr, *xp = nullptr;
    float *P = nullptr, *Y = nullptr;
    HIP_TRY(sc.alloc(&Wp, (size_t)NT * 16 * K / 2));
    HIP_TRY(sc.alloc(&Sp, (size_t)NT * 16 * K / 32));
    HIP_TRY(sc.alloc(&xp, (size_t)32 * K * 2));
    HIP_TRY(sc.alloc((void **)&P, (size_t)plan.ksplit * 16 * NT * 16 * 4));
    HIP_TRY(sc.alloc((void **)&Y, (size_t)16 * NT * 16 * 4));
    HIP_TRY(hipMemsetAsync(xp, 0, (size_t)32 * K * 2, st));
    HIP_TRY(hipMemcpyAsync(xp, x_dev, (size_t)n * K * 2, hipMemcpyDeviceToDevice, st));
    HIP_TRY(pack_weight_mxfp4_launch(codes_dev, scale_dev, Wp, Sp, N, K, K / 2, K / 32, NT, 1, 0, -1, st));
    GemvArgs a{};
    a.Wp = Wp; a.wq = 2; a.wblk = (const unsigned *)Sp; a.x = (const unsigned short *)xp; a.out_f32 = P;
    a.K = K; a.ldx = K; a.ldo = NT * 16; a.NT = NT; a.N_valid = N; a.n_rows = n;
    HIP_TRY(gemv_launch(a, plan, XSRC_PLAIN, EPI_PARTIAL_F32, st));
    hipLaunchKernelGGL(sum_partials_kernel, dim3((n * NT * 16 + 255) / 256), dim3(256), 0, st, P, plan.ksplit, NT * 16, Y, n, NT * 16);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(y_dev, (size_t)N * 4, Y, (size_t)NT * 16 * 4, (size_t)N * 4, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VLO_OK;
}

int vlo_test_gemm_fp8(const void *x_dev, const void *Wq_dev, const float *scale_dev, float *y_dev, void *xq_dev, float *xscale_dev, int M, int N, int K,
                      int iters, double *avg_us, void *stream) {
    if (!x_dev || !Wq_dev || !scale_dev || !y_dev || M <= 0 || !llm_gemm_fp8_ok(N, K)) return fail(VLO_E_INVALID, "bad test_gemm_fp8 arguments (N, K multiples of 256)");
    hipStream_t st = (hipStream_t)stream;
    const int NT = N / 16;
    const size_t RX = (size_t)((M + 255) / 256) * 256 + 256;
    ScratchBufs sc;
    void *Wp = nullptr, *xq = nullptr;
    float *sp = nullptr, *xs = nullptr;
    HIP_TRY(sc.alloc(&Wp, (size_t)N * K));
    HIP_TRY(sc.alloc(&xq, RX * K));
    HIP_TRY(sc.alloc((void **)&sp, (size_t)N * 4));
    HIP_TRY(sc.alloc((void **)&xs, RX * 4));
    HIP_TRY(hipMemsetAsync(xq, 0, RX * K, st));
    HIP_TRY(hipMemsetAsync(xs, 0, RX * 4, st));
    HIP_TRY(pack_weight_fp8_launch(Wq_dev, scale_dev, Wp, sp, N, K, K, NT, 1, 0, -1, st));
    HIP_TRY(quantize_rows_fp8_launch((const unsigned short *)x_dev, M, K, xq, xs, st));
    HIP_TRY(llm_gemm_fp8_launch(xq, xs, Wp, sp, M, N, K, y_dev, N, LLM_GEMM_F32, st));
    if (xq_dev) HIP_TRY(hipMemcpyAsync(xq_dev, xq, (size_t)M * K, hipMemcpyDeviceToDevice, st));
    if (xscale_dev) HIP_TRY(hipMemcpyAsync(xscale_dev, xs, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
    if (iters > 0 && avg_us) {                   // the GEMM alone, back to back (tools/probe_prefill.py --gemm)
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, st));
        for (int i = 0; i < iters; ++i) HIP_TRY(llm_gemm_fp8_launch(xq, xs, Wp, sp, M, N, K, y_dev, N, LLM_GEMM_F32, st));
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *avg_us = (double)ms * 1e3 / iters;
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
    HIP_TRY(hipStreamSynchronize(st));
    return VLO_OK;
}

int vlo_bench_gemv(int N, int K, int n_rows, int epi, int iters, int nbuf, double *avg_us) {
    const int fp8 = (epi & 0x100) ? 1 : 0;          // bit 8 of `epi`: time the fp8 e4m3 weight image instead of the bf16 one
    const int fp4 = (epi & 0x200) ? 1 : 0;          // bit 9: the mxfp4 image
    epi &= 0xff;
    if (N <= 0 || K <= 0 || n_rows <= 0 || n_rows > 16 || iters <= 0 || nbuf <= 0 || !avg_us) return fail(VLO_E_INVALID, "bad bench_gemv arguments");
    GemvPlan plan;
    if (fp8 && fp4) return fail(VLO_E_INVALID, "bench_gemv: one weight format at a time");
    if (gemv_plan(K, epi == EPI_PARTIAL_F32, &plan, fp4 ? 2 : 0)) return fail(VLO_E_UNSUPPORTED, "no GEMV plan for K");
    const int NT = (N + 15) / 16;
    const size_t wbytes = fp4 ? (size_t)NT * 16 * K / 2 : (size_t)NT * 16 * K * (fp8 ? 1 : 2);
    if (fp8 && ((plan.KF & 1) || plan.NW != 8)) return fail(VLO_E_UNSUPPORTED, "no fp8 GEMV for this K");
    ScratchBufs sc;
    std::vector<void *> Wp(nbuf, nullptr);
    void *x = nullptr, *o32 = nullptr, *o16 = nullptr, *hbuf = nullptr, *sq = nullptr, *nw = nullptr, *tab = nullptr, *kvp = nullptr;
    int *pt = nullptr;
    for (int i = 0; i < nbuf; ++i) {
        HIP_TRY(sc.alloc(&Wp[i], wbytes));
        HIP_TRY(hipMemset(Wp[i], 0x3c, wbytes));      // 0x3c3c = a small finite bf16
    }
    const size_t wide = (size_t)std::max(K, NT * 16);
    HIP_TRY(sc.alloc(&x, 32 * wide * 2));
    HIP_TRY(hipMemset(x, 0x3c, 32 * wide * 2));
    HIP_TRY(sc.alloc(&hbuf, 32 * wide * 2));
    HIP_TRY(hipMemset(hbuf, 0x3c, 32 * wide * 2));
    HIP_TRY(sc.alloc(&nw, wide * 2));
    HIP_TRY(hipMemset(nw, 0x3c, wide * 2));
    HIP_TRY(sc.alloc(&sq, 1024 * 16 * 4));
    HIP_TRY(hipMemset(sq, 0, 1024 * 16 * 4));
    HIP_TRY(sc.alloc(&o32, (size_t)plan.ksplit * 16 * NT * 16 * 4));
    HIP_TRY(sc.alloc(&o16, (size_t)16 * NT * 16 * 2));
    HIP_TRY(sc.alloc(&tab, (size_t)VLO_PAGE_TOKENS * 64 * 2));
    HIP_TRY(hipMemset(tab, 0x3c, (size_t)VLO_PAGE_TOKENS * 64 * 2));
    HIP_TRY(sc.alloc(&kvp, (size_t)NT * 16 * VLO_PAGE_TOKENS * 2));
    HIP_TRY(sc.alloc((void **)&pt, 64));
    HIP_TRY(hipMemset(pt, 0, 64));
    GemvArgs a{};
    void *wsc = nullptr;
    if (fp8) {
        HIP_TRY(sc.alloc(&wsc, (size_t)NT * 16 * 4));
        HIP_TRY(hipMemset(wsc, 0x3c, (size_t)NT * 16 * 4));
        a.wq = 1; a.wscale = (const float *)wsc;
    }
    if (fp4) {                                       // codes 0x3c = {4, 1.5}; scale bytes 0x7c = 2^-3: every weight finite and small
        HIP_TRY(sc.alloc(&wsc, (size_t)NT * 16 * K / 32));
        HIP_TRY(hipMemset(wsc, 0x7c, (size_t)NT * 16 * K / 32));
        a.wq = 2; a.wblk = (const unsigned *)wsc;
    }
    a.x = (const unsigned short *)x; a.out_f32 = (float *)o32; a.out_bf16 = (unsigned short *)o16;
    a.K = K; a.ldx = K; a.ldo = (epi == EPI_SWIGLU) ? NT * 8 : NT * 16; a.NT = NT; a.N_valid = N; a.n_rows = n_rows;   // SwiGLU: 8 output columns per tile
    int xsrc = XSRC_PLAIN;
    if (epi == EPI_SWIGLU) {
        xsrc = XSRC_NORM;
        a.norm_w = (const unsigned short *)nw; a.sq_in = (const float *)sq; a.sq_in_parts = 128; a.eps = 1e-5f;
    }
    if (epi == EPI_RESID) { a.h = (unsigned short *)hbuf; a.sq_out = (float *)sq; }
    if (epi == EPI_ROPE) {
        // N = (nh + 2*nkv) * 128 with nkv = nh / 4 (Llama-3 GQA); one page, positions 0..n_rows-1
        const int heads = N / 128, nkv = heads / 6, nh = heads - 2 * nkv;
        a.cos_tab = a.sin_tab = (const unsigned short *)tab;
        a.kv.k_pool = a.kv.vt_pool = (unsigned short *)kvp; a.kv.page_table = pt; a.kv.layer_stride = 0;
        a.kv.page_elems = (int64_t)nkv * VLO_PAGE_TOKENS * 128; a.kv.num_kv_heads = nkv; a.kv.head_dim = 128;
        a.layer = 0; a.num_heads = nh; a.pos0 = 0;
    }
    hipEvent_t e0, e1;
    HIP_TRY(sc.event(&e0));
    HIP_TRY(sc.event(&e1));
    for (int i = 0; i < 3; ++i) { a.Wp = Wp[i % nbuf]; HIP_TRY(gemv_launch(a, plan, xsrc, epi, 0)); }
    HIP_TRY(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) { a.Wp = Wp[i % nbuf]; HIP_TRY(gemv_launch(a, plan, xsrc, epi, 0)); }
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = (double)ms * 1e3 / iters;
    return VLO_OK;                         // `sc` frees the scratch and the events
}

int vlo_debug_read(vlo_session *s, int which, void *dst_dev, int64_t bytes, void *stream) {
    if (!s || !dst_dev || bytes <= 0) return fail(VLO_E_INVALID, "bad debug_read arguments");
    if (int prc = pending_refusal(s, "debug_read")) return prc;
    const StepWs &w = s->ws;
    if (which == 5 && bytes > (int64_t)16 * s->e->cfg.vocab_size * 2) return fail(VLO_E_INVALID, "debug_read: the logits buffer holds 16 rows");
    const void *src = which == 0 ? (void *)w.q : which == 1 ? (void *)w.attn : which == 2 ? (void *)w.h : which == 3 ? (void *)w.act
                    : which == 5 ? (void *)s->logits : (void *)w.x;
    HIP_TRY(hipMemcpyAsync(dst_dev, src, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VLO_OK;
}

/* host-side geometry of the 64-token block path, for unit tests: plan (NW, KF, KC) for a K, packed-64 element offset */
int vlo_debug_gemm64_plan(int K, int *out3) {
    Gemm64Plan p;
    if (!out3 || gemm64_plan(K, &p)) return fail(VLO_E_UNSUPPORTED, "no block-GEMM plan for K=" + std::to_string(K));
    out3[0] = p.NW; out3[1] = p.KF; out3[2] = p.KC;
    return VLO_OK;
}
int64_t vlo_debug_pack64_elem(int row, int k) { return (row < 0 || row >= VLO_BLOCK_TOKENS || k < 0) ? -1 : (int64_t)vlo_pack64_elem(row, k); }

int vlo_debug_gemv_plan(int K, int allow_ksplit, int *out4) {
    GemvPlan p;
    const int wq = (allow_ksplit & 0x200) ? 2 : 0;       // bit 9 (as in vlo_bench_gemv's `epi`): the mxfp4 image's plan
    if (!out4 || gemv_plan(K, (allow_ksplit & 0xff) != 0, &p, wq)) return fail(VLO_E_UNSUPPORTED, "no GEMV plan for K=" + std::to_string(K));
    out4[0] = p.NW; out4[1] = p.KF; out4[2] = p.KC; out4[3] = p.ksplit;
    return VLO_OK;
}
