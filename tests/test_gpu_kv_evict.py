"""KV eviction with RoPE re-rotation (include/vlo.h vlo_session_evict, Session.evict, LiveInfer(kv_budget=...)) on the MI355X, toy specs.

The rule is restated in torch in tests/kv_evict_util.py; the oracle's caches (bf16 reference, fp32 gold) are evicted the same way and give the
legs of the project's 3-way band.  The 700-token fill is ONE llm_step (the prefill path), so three KV pages are in play."""
import collections
import types

import pytest
import torch

from oracle import vlo_oracle as O
from tests.kv_evict_util import band_check, bits, check_kv_after_evict, evict_oracle_cache, step_inputs

pytestmark = pytest.mark.gpu

TINY_MHA = O.LlmSpec(128, 192, 2, 2, 2, 256, 10000.0, 1e-5, vision_hidden_size=128)       # head dim 64, one query head per kv head
SPECS = {"toy": O.LLM_SPECS["toy"], "toy128": O.LLM_SPECS["toy128"], "tiny-mha": TINY_MHA}  # toy: hd 64 GQA; toy128: hd 128 GQA
FILL = 700


def inv_freq(spec):
    return O.rope_inv_freq(spec.head_dim, spec.rope_theta)


def make_engine(spec, w, pool=8192, **kw):
    from videollm_online_amd.engine import Engine, EngineConfig
    cfg = EngineConfig(hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                       num_attention_heads=spec.num_heads, num_key_value_heads=spec.num_kv_heads, vocab_size=spec.vocab_size,
                       rope_theta=spec.rope_theta, rms_norm_eps=spec.rms_eps, vision_hidden_size=spec.vision_hidden_size, kv_pool_tokens=pool, **kw)
    eng = Engine(cfg)
    eng.load_weights(w)
    eng.load_weight("rope.inv_freq", inv_freq(spec))
    eng.finalize()
    return eng


def read_all(spec, s):
    L = s.get_seq_length()
    return {(layer, which, h): s.read_kv(layer, which, h, 0, L).cpu()
            for layer in range(spec.num_layers) for which in (0, 1) for h in range(spec.num_kv_heads)}


class Filled:
    """an engine, a session filled by one long step, its K / V as read then, the oracle's two caches after the same input: computed once"""

    def __init__(self, name):
        self.spec = spec = SPECS[name]
        self.w = O.init_llm_weights(spec, seed=3)
        self.toks = O.default_tokens(spec)
        self.ref, self.gold = O.LlamaOracle(spec, self.w, torch.bfloat16), O.LlamaOracle(spec, self.w, torch.float32)
        self.eng = make_engine(spec, self.w)
        self.s = self.eng.new_session()
        x = step_inputs(spec, self.ref, self.toks, 1, [FILL])[0]
        self.eng.llm_step(self.s, x.cuda(), want_last=False)
        _, self.rc = self.ref.forward(x, None, logits_from=FILL - 1)
        _, self.gc = self.gold.forward(x, None, logits_from=FILL - 1)
        self.len = FILL
        assert self.s.get_seq_length() == FILL == len(self.rc)
        self.before = read_all(spec, self.s)


_filled = {}


@pytest.fixture(scope="module")
def filled():
    def get(name):
        if name not in _filled:
            _filled[name] = Filled(name)
        return _filled[name]
    yield get
    for f in _filled.values():
        f.eng.close()
    _filled.clear()


def run_after(f, eng, s, rc, gc, tag, seed, lens=(11, 11, 11, 1, 1), step=None):
    step = step or (lambda x: eng.llm_step(s, x.cuda())[0])
    for i, x in enumerate(step_inputs(f.spec, f.ref, f.toks, seed, lens)):
        rl, rc = f.ref.forward(x, rc)
        gl, gc = f.gold.forward(x, gc)
        last = step(x).cpu()
        assert s.get_seq_length() == len(rc)
        band_check(tag, i, last, rl[-1], gl[-1])
    return rc, gc


RANGES = [(10, 310), (7, 44), (256, 512), (300, 301)]     # d > a page; odd d (V^T misaligned); page-aligned; one token


@pytest.mark.parametrize("rng", RANGES, ids=[f"{a}-{b}" for a, b in RANGES])
@pytest.mark.parametrize("name", list(SPECS))
def test_kv_and_parity_after_evict(filled, name, rng):
    f = filled(name)
    t0, t1 = rng
    s = f.s.fork(f.len)
    s.evict(t0, t1)
    assert s.get_seq_length() == f.len - (t1 - t0)
    iv = inv_freq(f.spec)
    check_kv_after_evict(f"gpu {name}", f.before, read_all(f.spec, s), t0, t1, iv)
    if name != "tiny-mha":
        # the band legs are the project's toy specs.  tiny-mha (this file's extra MHA shape) takes the bit-level KV check only: one row of its
        # 256-word vocabulary is too few logits for a max-error ratio (measured 1.28 / 1.33 on an 11-row step after [10, 310) / [300, 301)
        # with the KV check above at 100 %; tests/parity_util.py notes the same of a single row of the 64-wide toy model)
        run_after(f, f.eng, s, evict_oracle_cache(f.rc, t0, t1, iv), evict_oracle_cache(f.gc, t0, t1, iv), f"gpu {name} [{t0}, {t1})", 11)
    s.close()


@pytest.mark.parametrize("name", ["toy", "toy128"])
def test_interleaved_evictions_stay_in_band(filled, name):
    f = filled(name)
    s = f.s.fork(f.len)
    iv = inv_freq(f.spec)
    rc, gc = f.rc, f.gc
    for j, (t0, t1) in enumerate([(35, 46), (35, 58), (20, 21), (35, 420)]):
        s.evict(t0, t1)
        rc, gc = evict_oracle_cache(rc, t0, t1, iv), evict_oracle_cache(gc, t0, t1, iv)
        rc, gc = run_after(f, f.eng, s, rc, gc, f"gpu {name} eviction {j}", 20 + j, lens=(11, 1))
    s.close()


def test_evict_to_the_end_is_crop(filled):
    f = filled("toy128")
    a, b = f.s.fork(f.len), f.s.fork(f.len)
    a.evict(270, f.len)
    b.crop(270)
    assert a.get_seq_length() == b.get_seq_length() == 270
    ka, kb = read_all(f.spec, a), read_all(f.spec, b)
    for key in ka:
        assert torch.equal(bits(ka[key]), bits(kb[key])), key
    x = step_inputs(f.spec, f.ref, f.toks, 5, [11])[0].cuda()
    assert torch.equal(bits(f.eng.llm_step(a, x)[0]), bits(f.eng.llm_step(b, x)[0]))
    a.close()
    b.close()


def test_pages_come_back_and_errors():
    spec = SPECS["toy"]
    w = O.init_llm_weights(spec, seed=3)
    toks = O.default_tokens(spec)
    ref, gold = O.LlamaOracle(spec, w, torch.bfloat16), O.LlamaOracle(spec, w, torch.float32)
    eng = make_engine(spec, w, pool=1024)
    a, b = eng.new_session(), eng.new_session()
    xa = step_inputs(spec, ref, toks, 1, [1000])[0]
    eng.llm_step(a, xa.cuda(), want_last=False)
    _, rc = ref.forward(xa, None, logits_from=999)
    _, gc = gold.forward(xa, None, logits_from=999)
    before = read_all(spec, a)
    xb = step_inputs(spec, ref, toks, 9, [300])[0].cuda()
    with pytest.raises(RuntimeError, match="libvlo error -3"):
        eng.llm_step(b, xb, want_last=False)
    assert a.get_seq_length() == 1000 and b.get_seq_length() == 0
    for t0, t1 in ((-1, 5), (5, 1001), (7, 6)):
        with pytest.raises(RuntimeError, match="libvlo error -1"):
            a.evict(t0, t1)
    a.evict(9, 9)
    now = read_all(spec, a)
    assert a.get_seq_length() == 1000 and all(torch.equal(bits(now[k]), bits(before[k])) for k in now)
    a.evict(20, 620)
    assert a.get_seq_length() == 400
    eng.llm_step(b, xb, want_last=False)
    assert b.get_seq_length() == 300
    iv = inv_freq(spec)
    f = types.SimpleNamespace(spec=spec, ref=ref, gold=gold, toks=toks)
    run_after(f, eng, a, evict_oracle_cache(rc, 20, 620, iv), evict_oracle_cache(gc, 20, 620, iv), "gpu pages come back", 13, lens=(11,))
    eng.close()
    # an fp8 KV pool is refused, the session unchanged
    e8 = make_engine(spec, w, pool=1024, kv_dtype="fp8")
    s8 = e8.new_session()
    e8.llm_step(s8, xa[:45].cuda(), want_last=False)
    k8 = read_all(spec, s8)
    with pytest.raises(RuntimeError, match="libvlo error -6.*fp8"):
        s8.evict(5, 20)
    now = read_all(spec, s8)
    assert s8.get_seq_length() == 45 and all(torch.equal(bits(now[k]), bits(k8[k])) for k in now)
    e8.close()


def test_evict_between_batched_steps(filled):
    """two sessions stepped in a batch, one of them evicted between the steps: each session's logits equal stepping it alone after the
    same eviction, bit for bit"""
    f = filled("toy")
    eng = f.eng
    batch = eng.new_batch(2)
    a, b = f.s.fork(f.len), f.s.fork(300)
    xs1 = [x.cuda() for x in step_inputs(f.spec, f.ref, f.toks, 31, [11, 1])]
    xs2 = [x.cuda() for x in step_inputs(f.spec, f.ref, f.toks, 32, [1, 11])]
    batch.step([a, b], xs1)
    a.evict(35, 290)
    La, Lb = a.get_seq_length(), b.get_seq_length()
    assert La == f.len + 11 - 255
    fa, fb = a.fork(La), b.fork(Lb)
    last = batch.step([a, b], xs2)
    for i, (fork, x) in enumerate(zip((fa, fb), xs2)):
        want, _ = eng.llm_step(fork, x)
        assert torch.equal(bits(last[i]), bits(want)), (i, (last[i].float() - want.float()).abs().max().item())
    batch.close()
    for s in (a, b, fa, fb):
        s.close()


def test_greedy_loop_after_eviction(filled):
    """the greedy ids after an eviction are the evicted oracle's, except at a near-tie of the oracle's own logits (the rule of
    tests/test_gpu_long.py::Follower._judge, teacher-forced with the engine's tokens)"""
    from tests.test_gpu_long import Follower
    f = filled("toy128")
    s = f.s.fork(f.len)
    s.evict(35, 300)
    rc = evict_oracle_cache(f.rc, 35, 300, inv_freq(f.spec))
    x = step_inputs(f.spec, f.ref, f.toks, 41, [4])[0]
    out = torch.zeros(24, dtype=torch.long, device="cuda")
    n = f.eng.greedy_generate(s, x.cuda(), f.toks.eos_token_id, out)
    ids = out[:n].tolist()
    assert n >= 1
    judge = types.SimpleNamespace(stats=collections.Counter(), flip_margins=[])
    for i, t in enumerate(ids):
        logits, rc = f.ref.forward(x, rc)
        Follower._judge(judge, "greedy", int(logits[-1].argmax(dim=-1)), t, logits[-1])
        x = f.ref.embed(torch.tensor([t]))
    print(f"[kv evict gpu greedy] {n} tokens, identical {judge.stats['greedy_same']}, near-tie {judge.stats['greedy_near_tie']}")
    assert judge.stats["greedy_same"] >= 1
    s.close()


def test_tensor_parallel_evict():
    from videollm_online_amd.engine import EngineConfig, TpGroup
    spec = SPECS["toy128"]
    w = O.init_llm_weights(spec, seed=3)
    toks = O.default_tokens(spec)
    ref, gold = O.LlamaOracle(spec, w, torch.bfloat16), O.LlamaOracle(spec, w, torch.float32)
    cfg = EngineConfig(hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                       num_attention_heads=spec.num_heads, num_key_value_heads=spec.num_kv_heads, vocab_size=spec.vocab_size, rope_theta=spec.rope_theta,
                       rms_norm_eps=spec.rms_eps, vision_hidden_size=spec.vision_hidden_size, kv_pool_tokens=2048)
    grp = TpGroup(cfg, 2)
    grp.load_weights(w)
    grp.load_weight("rope.inv_freq", inv_freq(spec))
    grp.finalize()
    s = grp.new_session()
    x = step_inputs(spec, ref, toks, 1, [FILL])[0]
    grp.llm_step(s, x.cuda(), want_last=False)
    _, rc = ref.forward(x, None, logits_from=FILL - 1)
    _, gc = gold.forward(x, None, logits_from=FILL - 1)
    with pytest.raises(RuntimeError, match="libvlo error -1"):
        s.evict(5, FILL + 1)
    s.evict(7, 310)
    assert s.get_seq_length() == FILL - 303
    iv = inv_freq(spec)
    f = types.SimpleNamespace(spec=spec, ref=ref, gold=gold, toks=toks)
    run_after(f, grp, s, evict_oracle_cache(rc, 7, 310, iv), evict_oracle_cache(gc, 7, 310, iv), "gpu tp2", 11, lens=(11, 11, 1),
              step=lambda xx: grp.llm_step(s, xx.cuda())[0])
    s.close()
    grp.close()


# ---- LiveInfer with a KV budget ---------------------------------------------------------------------------------------------------------
def _liveinfer(pool, **kw):
    from videollm_online_amd.engine import Engine, EngineConfig
    from videollm_online_amd.inference import LiveInfer, StreamTokens
    from videollm_online_amd.modeling_live import LiveModel
    spec, vspec = O.LLM_SPECS["toy"], O.VIT_SPECS["toy"]
    w, vw = O.init_llm_weights(spec, seed=3), O.init_vit_weights(vspec, seed=1)
    toks = O.default_tokens(spec, seed=7, n_start=19)
    cfg = EngineConfig(hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                       num_attention_heads=spec.num_heads, num_key_value_heads=spec.num_kv_heads, vocab_size=spec.vocab_size, rope_theta=spec.rope_theta,
                       rms_norm_eps=spec.rms_eps, vision_hidden_size=spec.vision_hidden_size, kv_pool_tokens=pool,
                       frame_num_tokens=vspec.frame_num_tokens, frame_token_pooled=vspec.pooled,
                       vit=dict(hidden_size=vspec.hidden_size, intermediate_size=vspec.intermediate_size, num_layers=vspec.num_layers,
                                num_heads=vspec.num_heads, image_size=vspec.image_size, patch_size=vspec.patch_size, ln_eps=vspec.ln_eps))
    eng = Engine(cfg)
    eng.load_weights(w)
    eng.load_weights(vw)
    eng.load_weight("rope.inv_freq", inv_freq(spec))
    eng.finalize()
    model = LiveModel(eng, eos_token_id=toks.eos_token_id, frame_token_interval_id=toks.interval_id, frame_resolution=vspec.image_size)
    st = StreamTokens(toks.start_ids, toks.stream_prompt_ids, toks.stream_generation_ids, toks.eos_token_id, toks.interval_id, dict(toks.query_ids))
    return eng, LiveInfer(model, tokens=st, frame_fps=2, schedule=lambda i: (i % 7 == 6, 4), max_new_tokens=8, **kw)


def _drive(li, frames, n):
    li.load_video(frames)
    lens = []
    for i in range(n):
        li.input_video_stream(i / 2)
        li()
        lens.append(li.past_key_values.get_seq_length())
    return lens


def test_liveinfer_kv_budget():
    from videollm_online_amd.trace import EVICT
    N = 120
    frames = O.synthetic_frames(N, O.VIT_SPECS["toy"].image_size, seed=1234).cuda()
    eng, li = _liveinfer(4096)
    lens = _drive(li, frames, N)
    plain = list(li.trace)
    assert lens[-1] > 1300 and all(e[0] != EVICT for e in plain)
    eng.close()
    # a budget the stream never reaches: the same trace, event for event
    eng, li = _liveinfer(4096, kv_budget=4000)
    _drive(li, frames, N)
    assert list(li.trace) == plain
    eng.close()
    # a pool of 1 024 tokens cannot hold the stream ...
    eng, li = _liveinfer(1024)
    with pytest.raises(RuntimeError, match="libvlo error -3"):
        _drive(li, frames, N)
    eng.close()
    # ... and holds it under a budget: bounded length, whole run
    budget = 640
    eng, li = _liveinfer(1024, kv_budget=budget)
    lens = _drive(li, frames, N)
    ev = [e for e in li.trace if e[0] == EVICT]
    assert max(lens) <= budget and len(ev) >= 2
    assert all(e.t0 == 19 and e.kv_len <= budget - 256 for e in ev)
    assert len([e for e in li.trace if e[0] == "frame"]) == N                    # every frame was stepped
    print(f"[kv evict gpu liveinfer] {N} frames under kv_budget {budget}: {len(ev)} evictions, max length {max(lens)}, final {lens[-1]}")
    eng.close()
