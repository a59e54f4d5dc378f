"""Checkpoint loader for the engine: base Llama safetensors + the reference's PEFT adapter + SigLIP.

What the reference does at load time (models/modeling_live.py:184-222): ``from_pretrained`` the base
Llama, then ``PeftModel.from_pretrained(model, resume_from_checkpoint)`` which leaves LoRA *un-merged*
(every target Linear computes ``W x + (alpha/r) B (A x)`` at run time, r=128, alpha=256 —
models/arguments_live.py:16-19) and restores the fully-trained ``connector`` from ``modules_to_save``;
``set_vision_inside`` then loads ``AutoModel.from_pretrained(siglip).vision_model``
(models/vision_live.py:54-57).

Here the adapter is merged once, in fp32 (``W' = W + (alpha/r) B A``), rounded to bf16 and handed to
``Engine.load_weight`` under the HF names the engine expects, so the streamed weight image needs no
run-time LoRA work.  Merged != bit-identical to the reference's un-merged bf16 arithmetic; parity of a
real checkpoint is therefore judged against the fp32 gold path.
SURVEY.md §8(f) rank 1."""
from __future__ import annotations

import json
import os
import re

import torch

LORA_TARGETS = re.compile(r"model.*(q_proj|k_proj|v_proj|o_proj|gate_proj|up_proj|down_proj)|lm_head$")  # arguments_live.py:16


class _TensorSource:
    """name -> tensor over one or many .safetensors files (lazy, one tensor in memory at a time)."""

    def __init__(self, path: str):
        from safetensors import safe_open
        self._open = safe_open
        self.files = {}
        if os.path.isdir(path):
            idx = [f for f in os.listdir(path) if f.endswith(".safetensors.index.json")]
            if idx:
                wm = json.load(open(os.path.join(path, idx[0])))["weight_map"]
                self.files = {k: os.path.join(path, v) for k, v in wm.items()}
            else:
                for f in sorted(os.listdir(path)):
                    if f.endswith(".safetensors"):
                        with safe_open(os.path.join(path, f), "pt") as h:
                            for k in h.keys():
                                self.files[k] = os.path.join(path, f)
        else:
            with safe_open(path, "pt") as h:
                self.files = {k: path for k in h.keys()}
        if not self.files:
            raise FileNotFoundError(f"no safetensors tensors under {path}")

    def keys(self):
        return self.files.keys()

    def __contains__(self, k):
        return k in self.files

    def get(self, k) -> torch.Tensor:
        with self._open(self.files[k], "pt") as h:
            return h.get_tensor(k)


def _adapter_maps(adapter_dir: str):
    """PEFT adapter_model.safetensors -> ({module: (A, B)}, {connector key: tensor}, scale)."""
    cfg = json.load(open(os.path.join(adapter_dir, "adapter_config.json")))
    scale = cfg.get("lora_alpha", 256) / cfg.get("r", 128)
    src = _TensorSource(os.path.join(adapter_dir, "adapter_model.safetensors"))
    lora, extra = {}, {}
    for k in src.keys():
        name = k
        for pre in ("base_model.model.",):
            if name.startswith(pre):
                name = name[len(pre):]
        name = name.replace(".modules_to_save.default", "").replace(".default", "")
        m = re.match(r"(.*)\.lora_([AB])\.weight$", name)
        if m:
            lora.setdefault(m.group(1), {})[m.group(2)] = k
        elif name.startswith("connector."):
            extra[name] = k
    return src, lora, extra, scale


FP8_E4M3_MAX = 448.0


def is_kv_scale(name: str) -> bool:
    """a static per-layer KV-cache scale of an fp8-KV engine: model.layers.{i}.self_attn.k_scale / v_scale"""
    return name.startswith("model.layers.") and name.endswith((".self_attn.k_scale", ".self_attn.v_scale"))


def round_to_e4m3(x: torch.Tensor) -> torch.Tensor:
    """fp32 values in [-448, 448] rounded to the nearest OCP e4m3 value, ties to even, returned as fp32.  Written out with
    frexp / ldexp / round so that every device rounds alike (the first hardware run showed torch's own float -> float8
    conversion on the GPU disagreeing with its CPU conversion on ~6e-4 of the values, sub-normals included): a binade
    [2^e, 2^(e+1)) holds 8 steps of 2^(e-3); below 2^-6 the step is 2^-9."""
    _, ex = torch.frexp(x)                              # |x| = m * 2^ex, m in [0.5, 1)  ->  e = ex - 1
    step_exp = (ex - 4).clamp_min(-9)
    return torch.ldexp(torch.round(torch.ldexp(x, -step_exp)), step_exp).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX)


def quantize_fp8_per_channel(W: torch.Tensor):
    """Symmetric per-output-channel quantisation of a Linear weight [out, in] to OCP fp8 e4m3 (BASELINE.json configs[4],
    SURVEY.md §8(f)-1 "fp8 + per-channel scales"): scale[n] = max|W[n]| * (1/448) (1 for an all-zero row),
    q[n] = e4m3_rne(W[n] / scale[n]).  Returns (q as torch.float8_e4m3fn [out, in], scale f32 [out]); W ~= q * scale[:, None].
    The engine streams q (one byte per weight) and applies scale[n] to the fp32 dot product."""
    Wf = W.float()
    amax = Wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax * (1.0 / FP8_E4M3_MAX), torch.ones_like(amax))
    q = round_to_e4m3((Wf / scale[:, None]).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX))
    return q.to(torch.float8_e4m3fn), scale                # exact: q already holds e4m3 values


MXFP4_BLOCK = 32
_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# (midpoint between codes c and c + 1 as fp32 bits, whether the tie goes up): ties go to the even code
_E2M1_MIDPOINTS = ((0x3E800000, False), (0x3F400000, True), (0x3FA00000, False), (0x3FE00000, True), (0x40200000, False), (0x40600000, True),
                   (0x40A00000, False))        # 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5


def quantize_mxfp4(W: torch.Tensor):
    """OCP MXFP4 quantisation of a Linear weight [out, in] (include/vlo.h vlo_config.weight_dtype = 2): per block of 32 elements along `in`,
    E = clamp(floor(log2(max|x|)) - 2, -125, 127) (the shared exponent minus e2m1's largest), scale byte = E + 127, code = the e2m1 value nearest
    to clamp(x / 2^E, -6, 6), ties to the even code; an all-zero block gets scale byte 127 and codes 0.  Returns (codes uint8 [out, in / 2] with
    element 2j in the low nibble of byte j — sign bit 3, exponent bits 2:1, mantissa bit 0 — and scale uint8 [out, in / 32]).
    log2 comes from frexp and the rounding from integer compares on the fp32 bit patterns, so that every device quantises alike (see
    round_to_e4m3)."""
    N, K = W.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4: in_features {K} is not a multiple of {MXFP4_BLOCK}")
    x = W.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = x.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)                           # amax = m * 2^ex, m in [0.5, 1)  ->  floor(log2(amax)) = ex - 1
    E = torch.where(amax > 0, (ex - 3).clamp(-125, 127), torch.zeros_like(ex))
    y = torch.ldexp(x, -E[..., None]).clamp_(-6.0, 6.0)  # exact: a power-of-two scaling
    bits = y.abs().contiguous().view(torch.int32)       # non-negative floats order like their bit patterns
    code = torch.zeros_like(bits)
    for mid, up in _E2M1_MIDPOINTS:
        code += (bits >= mid) if up else (bits > mid)
    code |= (y < 0).to(torch.int32) << 3
    code = code.reshape(N, K).to(torch.uint8)
    return code[:, 0::2] | (code[:, 1::2] << 4), (E + 127).to(torch.uint8)


def dequantize_mxfp4(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """(codes uint8 [N, K / 2], scale uint8 [N, K / 32]) -> the fp32 weights [N, K] an mxfp4 engine multiplies by: e2m1(code) * 2^(scale - 127),
    every one of them a bf16 value for scale bytes in [2, 254]."""
    codes, scale = codes.view(torch.uint8), scale.view(torch.uint8)
    N, K = codes.shape[0], 2 * codes.shape[1]
    c = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(N, K).long()
    lut = torch.tensor(_E2M1_VALUES + tuple(-v for v in _E2M1_VALUES), dtype=torch.float32, device=codes.device)
    v = lut[c].reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    return torch.ldexp(v, (scale.to(torch.int32) - 127)[..., None]).reshape(N, K)


def merge_lora(W: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale: float) -> torch.Tensor:
    """W [out,in] + scale * B [out,r] @ A [r,in], accumulated in fp32, rounded once to bf16."""
    return (W.float() + scale * (B.float() @ A.float())).to(torch.bfloat16)


def iter_llm_weights(base_dir: str, adapter_dir: str | None = None, device: str = "cpu"):
    """Yields (hf_name, bf16 tensor) for every Llama + connector weight, LoRA merged; a quantised checkpoint's static KV-cache scales
    (model.layers.{i}.self_attn.k_scale / v_scale) come as they are stored, in fp32."""
    base = _TensorSource(base_dir)
    src = lora = extra = None
    scale = 1.0
    if adapter_dir:
        src, lora, extra, scale = _adapter_maps(adapter_dir)
        bad = [m for m in lora if not LORA_TARGETS.search(m)]
        if bad:
            raise ValueError(f"adapter targets modules outside the reference's lora_modules pattern: {bad[:4]}")
    seen = set()
    for k in base.keys():
        if "rotary_emb.inv_freq" in k:
            continue
        W = base.get(k).to(device)
        if is_kv_scale(k):
            yield k, W.float()
            continue
        mod = k[:-len(".weight")] if k.endswith(".weight") else None
        if lora and mod in lora:
            ab = lora[mod]
            if set(ab) != {"A", "B"}:
                raise ValueError(f"incomplete LoRA pair for {mod}")
            W = merge_lora(W, src.get(ab["A"]).to(device), src.get(ab["B"]).to(device), scale)
            seen.add(mod)
        yield k, W.to(torch.bfloat16)
    if lora:
        missing = set(lora) - seen
        if missing:
            raise KeyError(f"adapter has LoRA weights for modules absent from the base checkpoint: {sorted(missing)[:4]}")
    if extra:
        for name, k in extra.items():
            yield name, src.get(k).to(device).to(torch.bfloat16)
    if "lm_head.weight" not in base and "model.embed_tokens.weight" in base:   # tied embeddings
        yield "lm_head.weight", base.get("model.embed_tokens.weight").to(device).to(torch.bfloat16)


def iter_vision_weights(siglip_dir: str, device: str = "cpu"):
    """Yields ('vision.<SiglipVisionModel key>', fp32 tensor) from a google/siglip-* checkpoint
    (keys 'vision_model.*'; the text tower and logit scale/bias are skipped)."""
    srcs = _TensorSource(siglip_dir)
    n = 0
    for k in srcs.keys():
        if not k.startswith("vision_model."):
            continue
        n += 1
        yield "vision." + k[len("vision_model."):], srcs.get(k).to(device).float()
    if n == 0:
        raise KeyError(f"no 'vision_model.*' tensors under {siglip_dir}")


def load_engine_weights(engine, base_dir: str, adapter_dir: str | None = None, siglip_dir: str | None = None,
                        device: str | None = None):
    """Stream a real checkpoint into an (un-finalized) Engine; merges LoRA on `device` (default: the GPU)."""
    dev = device or str(engine.device)
    fp8_kv = getattr(engine.cfg, "kv_dtype", "bf16") == "fp8"
    for name, t in iter_llm_weights(base_dir, adapter_dir, dev):
        if is_kv_scale(name) and not fp8_kv:
            continue                          # the scales of an fp8 KV cache mean nothing to a bf16 one
        engine.load_weight(name, t)
    if siglip_dir:
        for name, t in iter_vision_weights(siglip_dir, dev):
            engine.load_weight(name, t)
    return engine
