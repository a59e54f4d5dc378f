"""The fp8 (e4m3) KV cache on the MI355X (include/vlo.h vlo_config.kv_dtype = 1; EngineConfig.kv_dtype = "fp8"), through the product's C ABI.

Rule (restated on the oracle's cache hook, as in test_emul_kv_fp8_cpu.py): K after RoPE and V of layer i are stored as
e4m3_rne(clamp(x / s_i, -448, 448)) with static per-layer k_scale / v_scale s_i and read back as code * s_i, the current step's own keys
included.  Parity: err(engine, fp32 gold) <= 1.25 err(bf16 reference, fp32 gold) + 1e-3 max|logit|, both legs under that rule."""
import dataclasses

import pytest
import torch

from oracle import vlo_oracle as O
from parity_util import within_band

pytestmark = pytest.mark.gpu


def kv_quant(x, s):
    return (O.e4m3_rne((x.float() / s).clamp(-448.0, 448.0)) * s).to(x.dtype)


class Fp8KVCache(O.KVCacheOracle):
    def __init__(self, num_layers, k_scale, v_scale):
        super().__init__(num_layers)
        self.ks = [torch.tensor(v, dtype=torch.float32) for v in k_scale]
        self.vs = [torch.tensor(v, dtype=torch.float32) for v in v_scale]

    def update(self, i, k, v):
        return super().update(i, kv_quant(k, self.ks[i].to(k.device)), kv_quant(v, self.vs[i].to(v.device)))


def _cfg(spec, kv_pool_tokens=4096, **kw):
    from videollm_online_amd.engine import EngineConfig
    return EngineConfig(hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                        num_attention_heads=spec.num_heads, num_key_value_heads=spec.num_kv_heads, vocab_size=spec.vocab_size,
                        rope_theta=spec.rope_theta, rms_norm_eps=spec.rms_eps, vision_hidden_size=spec.vision_hidden_size,
                        kv_pool_tokens=kv_pool_tokens, **kw)


def _scales(spec, ks, vs):
    return {**{f"model.layers.{i}.self_attn.k_scale": torch.tensor(ks[i]) for i in range(spec.num_layers)},      # 0-d, as vLLM stores them
            **{f"model.layers.{i}.self_attn.v_scale": torch.tensor(vs[i]) for i in range(spec.num_layers)}}


def _engine(spec, w, kv_dtype="fp8", scales=None, tp=1, **kw):
    from videollm_online_amd.engine import Engine, TpGroup
    cfg = _cfg(spec, kv_dtype=kv_dtype, **kw)
    e = TpGroup(cfg, tp) if tp > 1 else Engine(cfg)
    e.load_weights(w)
    if scales is not None:
        e.load_weights(_scales(spec, *scales))
    e.load_weight("rope.inv_freq", O.rope_inv_freq(spec.head_dim, spec.rope_theta))
    e.finalize()
    return e


def _steps(spec, ref, toks, seed):                   # test_gpu_fp8.py's step mix: block path, frame step, 4, decode, 13
    g = torch.Generator().manual_seed(seed + 100)
    frame = lambda: torch.randn(10, spec.hidden_size, generator=g).bfloat16()
    return [torch.cat([ref.embed(torch.tensor(toks.start_ids)), frame()]),
            torch.cat([ref.embed(torch.tensor([toks.interval_id])), frame()]),
            ref.embed(torch.tensor(toks.stream_generation_ids)),
            ref.embed(torch.tensor([17])),
            torch.cat([ref.embed(torch.tensor([toks.eos_token_id] + toks.stream_prompt_ids)), frame()])]


def _check(tag, i, allr, rl, gl):
    e = (allr.float() - gl).abs().max().item()
    r = (rl.float() - gl).abs().max().item()
    slack = 1e-3 * gl.abs().max().item()
    print(f"[{tag}] step {i}: engine err {e:.4g} ref err {r:.4g}")
    assert within_band(e, r, slack, f"test_gpu_kv_fp8.py:{tag}"), f"{tag} step {i}: {e} vs {r}"


def _stream(tag, eng, spec, w, scales, steps, oracle_w=None, keep=None):
    ow = oracle_w or w
    ref = O.LlamaOracle(spec, ow, torch.bfloat16, keep_fp32=keep) if keep else O.LlamaOracle(spec, ow, torch.bfloat16)
    gold = O.LlamaOracle(spec, ow, torch.float32)
    rc, gc = Fp8KVCache(spec.num_layers, *scales), Fp8KVCache(spec.num_layers, *scales)
    sess = eng.new_session()
    for i, x in enumerate(steps):
        rl, rc = ref.forward(x, rc)
        gl, gc = gold.forward(x, gc)
        last, allr = eng.llm_step(sess, x.cuda(), want_last=True, want_all=True)
        torch.cuda.synchronize()
        assert sess.get_seq_length() == len(rc)
        _check(tag, i, allr.cpu(), rl, gl)
    return sess


# ---- 1. bit-exact stores at the 8B width, all three append sites, several pages ---------------------------------------------------
def test_layer0_kv_bit_equal_to_quantised_bf16_engine():
    spec = O.LLM_SPECS["llama-3-8b-2l"]
    w = O.init_llm_weights(spec, seed=6)
    s = 2.0 ** -2
    bf = _engine(spec, w, "bf16")
    f8 = _engine(spec, w, "fp8", ([s] * 2, [s] * 2))
    g = torch.Generator(device="cuda").manual_seed(1)
    sb, s8 = bf.new_session(), f8.new_session()
    for n in (300, 45, 64, 11, 1, 13):           # >= 256: long-input prefill (rope_kv_append); 45 / 64: block path; <= 16: the GEMV epilogue
        x = torch.randn(n, spec.hidden_size, generator=g, device="cuda").bfloat16()
        bf.llm_step(sb, x, want_last=False)
        f8.llm_step(s8, x, want_last=False)
    L = len(sb)
    assert L == len(s8) == 434
    st = torch.tensor(s, device="cuda")
    for h in range(spec.num_kv_heads):
        for which in (0, 1):
            a, b = sb.read_kv(0, which, h, 0, L), s8.read_kv(0, which, h, 0, L)
            assert torch.equal(b.view(torch.int16), kv_quant(a, st).view(torch.int16)), (which, h)
    sb.close(), s8.close(), bf.close(), f8.close()


# ---- 2. stream parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["llama-3-8b-2l", "tinyllama-2l"])
@pytest.mark.parametrize("scales", [([1.0, 1.0], [1.0, 1.0]), ([0.37, 0.11], [0.052, 0.6])])
def test_stream_parity(name, scales):
    spec = O.LLM_SPECS[name]
    w = O.init_llm_weights(spec, seed=6)
    toks = O.default_tokens(spec, seed=7, n_start=35)
    eng = _engine(spec, w, "fp8", scales)
    sess = _stream(f"fp8 kv {name}", eng, spec, w, scales, _steps(spec, O.LlamaOracle(spec, w, torch.bfloat16), toks, 6))
    sess.close()
    eng.close()


# ---- 3. attention at stream lengths against fp32 torch over the dequantised KV -----------------------------------------------------
@pytest.mark.parametrize("Lc", [13245, 66000])
def test_attention_at_stream_length_vs_torch_fp32(Lc):
    import ctypes as C
    from videollm_online_amd import _C
    from videollm_online_amd.engine import _ptr, _stream_handle
    spec = O.LLM_SPECS["llama-3-8b-2l"]
    w = O.init_llm_weights(spec, seed=6)
    eng = _engine(spec, w, "fp8", ([0.5, 0.25], [0.25, 0.5]), kv_pool_tokens=Lc + 512)     # powers of two: the read-back is exact
    nh, nkv, hd, H = spec.num_heads, spec.num_kv_heads, spec.head_dim, spec.hidden_size
    g = torch.Generator(device="cuda").manual_seed(Lc)
    sess = eng.new_session()
    fill = (torch.randn(Lc, H, generator=g, device="cuda") * 0.5).bfloat16()
    eng.llm_step(sess, fill, want_last=False)
    del fill
    layer = spec.num_layers - 1
    L, worst = Lc, 0.0
    for n in (11, 1, 4, 8, 13, 16, 12):
        eng.llm_step(sess, (torch.randn(n, H, generator=g, device="cuda") * 0.5).bfloat16())
        pos = torch.arange(L, L + n, device="cuda")
        L += n
        q = torch.empty(16, nh * hd, dtype=torch.bfloat16, device="cuda")
        a = torch.empty(16, nh * hd, dtype=torch.bfloat16, device="cuda")
        _C.check(_C.lib().vlo_debug_read(sess._h, 0, _ptr(q), q.numel() * 2, _stream_handle()))
        _C.check(_C.lib().vlo_debug_read(sess._h, 1, _ptr(a), a.numel() * 2, _stream_handle()))
        q, a = q[:n].view(n, nh, hd).float(), a[:n].view(n, nh, hd).float()
        for kvh in range(nkv):
            K = sess.read_kv(layer, 0, kvh, 0, L).float()
            V = sess.read_kv(layer, 1, kvh, 0, L).float()
            for h in range(kvh * (nh // nkv), (kvh + 1) * (nh // nkv)):
                s = ((q[:, h] @ K.T) * hd ** -0.5).masked_fill(torch.arange(L, device="cuda")[None, :] > pos[:, None], float("-inf"))
                ref = torch.softmax(s, dim=-1) @ V
                err, scale = (a[:, h] - ref).abs().max().item(), ref.abs().max().item()
                worst = max(worst, err / scale)
                assert err <= 2 ** -7 * scale + 1e-4, (Lc, n, kvh, h, err, scale)
    print(f"[fp8 kv attention Lc={Lc}] worst relative error {worst:.2e}")
    sess.close()
    eng.close()


# ---- 4. a long input (the prefill path's attention falls back to the chunk kernel) and 16-row steps after it ---------------------------
def test_long_input_then_steps():
    spec = O.LLM_SPECS["llama-3-8b-2l"]
    w = O.init_llm_weights(spec, seed=6)
    scales = ([0.37, 0.11], [0.052, 0.6])
    eng = _engine(spec, w, "fp8", scales)
    ref = O.LlamaOracle(spec, w, torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    steps = [torch.randn(300, spec.hidden_size, generator=g).bfloat16()] + [torch.randn(n, spec.hidden_size, generator=g).bfloat16()
                                                                             for n in (16, 11, 1)]
    sess = _stream("fp8 kv long input", eng, spec, w, scales, steps)
    del ref
    sess.close()
    eng.close()


# ---- 5. fork / crop and a greedy response on an fp8 pool -------------------------------------------------------------------------
def test_fork_crop_greedy():
    spec = O.LLM_SPECS["tinyllama-2l"]
    w = O.init_llm_weights(spec, seed=6)
    toks = O.default_tokens(spec, seed=7, n_start=35)
    eng = _engine(spec, w, "fp8", ([0.37, 0.11], [0.052, 0.6]))
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda n: torch.randn(n, spec.hidden_size, generator=g, device="cuda").bfloat16()
    head, extra, tail = [rnd(200), rnd(100)], [rnd(11)], [rnd(11), rnd(1)]       # fork at 300: mid-page
    a = eng.new_session()
    for x in head + extra:
        eng.llm_step(a, x, want_last=False)
    fresh = eng.new_session()
    for x in head:
        eng.llm_step(fresh, x, want_last=False)
    want = [eng.llm_step(fresh, x, want_all=True)[1].clone() for x in tail]
    b = a.fork(300)
    torch.cuda.synchronize()
    assert len(b) == 300 and len(a) == 311
    for x, r in zip(tail, want):
        assert torch.equal(eng.llm_step(b, x, want_all=True)[1], r)
    a.crop(300)
    for x, r in zip(tail, want):
        assert torch.equal(eng.llm_step(a, x, want_all=True)[1], r)
    ids = torch.zeros(6, dtype=torch.long, device="cuda")
    n = eng.greedy_generate(b, eng.embed(torch.tensor(toks.stream_generation_ids)), toks.eos_token_id, ids, force_len=5)
    assert n == 5 and ids[4].item() == toks.eos_token_id
    for s in (a, b, fresh):
        s.close()
    eng.close()


# ---- 6. tensor parallelism: the scales are replicated, nothing new is sharded ------------------------------------------------------
@pytest.mark.parametrize("tp", [2, 8])
def test_tp_logical_ranks(tp):
    spec = O.LLM_SPECS["llama-3-8b-2l"]
    w = O.init_llm_weights(spec, seed=6)
    toks = O.default_tokens(spec, seed=7, n_start=35)
    scales = ([0.37, 0.11], [0.052, 0.6])
    grp = _engine(spec, w, "fp8", scales, tp=tp)
    sess = _stream(f"fp8 kv tp{tp}", grp, spec, w, scales, _steps(spec, O.LlamaOracle(spec, w, torch.bfloat16), toks, 6)[:4])
    sess.close()
    grp.close()


# ---- 7. fp8 weights and fp8 KV together at the 70B width (2 layers): the shape config 5 would run -----------------------------------
def test_fp8_weights_and_fp8_kv_70b_width():
    from videollm_online_amd.checkpoint import quantize_fp8_per_channel
    spec = dataclasses.replace(O.LLM_SPECS["llama-3-70b-1l"], num_layers=2)
    w = O.init_llm_weights(spec, seed=10)
    toks = O.default_tokens(spec, seed=7, n_start=35)
    eng_w, ora_w, keep = {}, {}, set()
    for k, v in w.items():
        if k.endswith(O.FP8_STREAMED):
            q, s = quantize_fp8_per_channel(v.cuda())
            eng_w[k], eng_w[k + "_scale"] = q, s
            ora_w[k] = q.cpu().float() * s.cpu()[:, None]
            keep.add(k)
        else:
            eng_w[k] = ora_w[k] = v
    scales = ([0.37, 0.11], [0.052, 0.6])
    eng = _engine(spec, eng_w, "fp8", scales, weight_dtype="fp8")
    ref = O.LlamaOracle(spec, ora_w, torch.bfloat16, keep_fp32=keep)
    sess = _stream("fp8 w + fp8 kv 70b-2l", eng, spec, w, scales, _steps(spec, ref, toks, 10), oracle_w=ora_w, keep=keep)
    sess.close()
    eng.close()
