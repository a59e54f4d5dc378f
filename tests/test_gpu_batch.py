"""Batched steps (include/vlo.h vlo_batch_*, engine.Batch) on the MI355X.

The project's parity rule: on the 16-row path a session stepped inside a batch equals the same session stepped alone (vlo_llm_step on a
fork) bit for bit — last-row logits and the K / V it appended; on the 64-row block path its logits are within the 1.25 band of the oracle.
Shapes: 8B width (2 layers), TinyLlama width, 70B width with fp8 weights; bf16 and fp8 KV; one segment at 13 245 cached tokens batched with
short ones, so the segments of one launch have different split counts."""
import os
import sys

import pytest
import torch

from oracle import vlo_oracle as O
from parity_util import within_band

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

SHAPES = {
    "8b": dict(hidden_size=4096, intermediate_size=14336, num_attention_heads=32, num_key_value_heads=8, vocab_size=128256, rope_theta=500000.0),
    "tinyllama": dict(hidden_size=2048, intermediate_size=5632, num_attention_heads=32, num_key_value_heads=4, vocab_size=32000, rope_theta=10000.0),
    "70b": dict(hidden_size=8192, intermediate_size=28672, num_attention_heads=64, num_key_value_heads=8, vocab_size=128256, rope_theta=500000.0),
}


def _engine(shape, layers=2, kv_pool_tokens=40000, **kw):
    from probe_llm import random_llm_weights_to_engine
    from videollm_online_amd.engine import Engine, EngineConfig
    cfg = EngineConfig(**SHAPES[shape], num_hidden_layers=layers, kv_pool_tokens=kv_pool_tokens, **kw)
    eng = Engine(cfg)
    random_llm_weights_to_engine(eng, cfg, seed=7)
    eng.finalize()
    return eng


def _rows(eng, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, eng.cfg.hidden_size, generator=g, device="cuda").bfloat16()


def _grown(eng, lens, seed):
    out = []
    for i, L in enumerate(lens):
        s = eng.new_session()
        eng.llm_step(s, _rows(eng, L, seed + i), want_last=False)
        out.append(s)
    return out


def _same_as_solo(eng, batch, sessions, xs):
    lens = [s.get_seq_length() for s in sessions]
    forks = [s.fork(L) for s, L in zip(sessions, lens)]
    last = batch.step(sessions, xs)
    nkv = eng.cfg.num_key_value_heads
    for b, (s, f, x, L) in enumerate(zip(sessions, forks, xs, lens)):
        want, _ = eng.llm_step(f, x)
        assert s.get_seq_length() == f.get_seq_length() == L + x.shape[0]
        assert torch.equal(last[b].view(torch.int16), want.view(torch.int16)), (b, (last[b].float() - want.float()).abs().max().item())
        for layer in range(eng.cfg.num_hidden_layers):
            for h in (0, nkv - 1):
                for which in (0, 1):
                    got, ref = s.read_kv(layer, which, h, L, L + x.shape[0]), f.read_kv(layer, which, h, L, L + x.shape[0])
                    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (b, layer, h, which)
    return forks


CASES = [("8b", {}), ("8b", dict(kv_dtype="fp8")), ("tinyllama", {}), ("70b", dict(weight_dtype="fp8", kv_dtype="fp8"))]


@pytest.mark.parametrize("shape,kw", CASES, ids=["8b", "8b-kvfp8", "tinyllama", "70b-fp8w-kvfp8"])
def test_16_row_batch_bit_equal_to_solo(shape, kw):
    eng = _engine(shape, **kw)
    batch = eng.new_batch(4)
    # a long segment (split geometry of ~13 k keys) next to short ones; 250 + 11 rows cross a page boundary
    ss = _grown(eng, [13245, 40, 259, 250], seed=1)
    _same_as_solo(eng, batch, ss, [_rows(eng, n, 100 + i) for i, n in enumerate([1, 1, 3, 11])])
    _same_as_solo(eng, batch, ss, [_rows(eng, 1, 200 + i) for i in range(4)])
    batch.close()
    eng.close()


def test_16_decode_rows_bit_equal_to_solo():
    eng = _engine("8b", kv_pool_tokens=16 * 2048)
    batch = eng.new_batch(16)
    ss = _grown(eng, [1 + 97 * i for i in range(16)], seed=2)
    _same_as_solo(eng, batch, ss, [_rows(eng, 1, 300 + i) for i in range(16)])
    batch.close()
    eng.close()


def test_samplers_equal_solo():
    eng = _engine("8b", kv_pool_tokens=16 * 2048)
    batch = eng.new_batch(5)
    ss = _grown(eng, [5, 600, 1300, 9, 33], seed=3)
    forks = _same_as_solo(eng, batch, ss, [_rows(eng, n, 400 + i) for i, n in enumerate([1, 2, 1, 10, 1])])
    iid = 5
    p0 = sorted(float(eng.stream_sample(f, 0.0, iid)[1]) for f in forks)
    thr = (p0[1] + p0[2]) / 2 if p0[1] != p0[2] else p0[2] * 1.5
    solo = [eng.stream_sample(f, thr, iid) for f in forks]
    tok, p = batch.stream_sample(thr, iid)
    assert tok.tolist() == [int(t) for t, _ in solo]
    assert torch.equal(p.cpu(), torch.cat([q for _, q in solo]).cpu())
    # greedy: each session's ids, length and end state equal vlo_greedy_generate on a fork; EOS = a token one session emits second
    max_new = 6
    xs = [_rows(eng, 2, 500 + i) for i in range(3)]
    free = []
    for s, x in zip(ss[:3], xs):
        out = torch.zeros(max_new, dtype=torch.long, device="cuda")
        n = eng.greedy_generate(s.fork(s.get_seq_length()), x, -1, out)
        free.append(out[:n].tolist())
    eos = free[0][1]
    forks = [s.fork(s.get_seq_length()) for s in ss[:3]]
    outs = [torch.zeros(max_new, dtype=torch.long, device="cuda") for _ in range(3)]
    want = [eng.greedy_generate(f, x, eos, o) for f, x, o in zip(forks, xs, outs)]
    got_out = [torch.zeros(max_new, dtype=torch.long, device="cuda") for _ in range(3)]
    got = batch.greedy_generate(ss[:3], xs, eos, got_out)
    assert got == want and want[0] == 2
    for g, o, n in zip(got_out, outs, want):
        assert g[:n].tolist() == o[:n].tolist()
    assert [s.get_seq_length() for s in ss[:3]] == [f.get_seq_length() for f in forks]
    batch.close()
    eng.close()


def test_block_path_batch_within_band():
    """4 frame steps (4 x 11 rows: the 64-row block path) at TinyLlama width, 2 layers, against the oracle per session"""
    from videollm_online_amd.engine import Engine, EngineConfig
    sh = SHAPES["tinyllama"]
    spec = O.LlmSpec(sh["hidden_size"], sh["intermediate_size"], 2, sh["num_attention_heads"], sh["num_key_value_heads"], sh["vocab_size"],
                     sh["rope_theta"], 1e-5, vision_hidden_size=1024)
    w = O.init_llm_weights(spec, seed=9)
    cfg = EngineConfig(**sh, num_hidden_layers=2, kv_pool_tokens=8192, vision_hidden_size=1024)
    eng = Engine(cfg)
    eng.load_weights(w)
    eng.load_weight("rope.inv_freq", O.rope_inv_freq(spec.head_dim, spec.rope_theta))
    eng.finalize()
    ref, gold = O.LlamaOracle(spec, w, torch.bfloat16), O.LlamaOracle(spec, w, torch.float32)
    g = torch.Generator().manual_seed(3)
    hist = [torch.randn(L, spec.hidden_size, generator=g).bfloat16() for L in (45, 7, 300, 30)]
    xs = [torch.randn(11, spec.hidden_size, generator=g).bfloat16() for _ in range(4)]
    ss = []
    for h in hist:
        s = eng.new_session()
        eng.llm_step(s, h.cuda(), want_last=False)
        ss.append(s)
    batch = eng.new_batch(4)
    last = batch.step(ss, [x.cuda() for x in xs]).cpu()
    for i in range(4):
        rc, gc = O.KVCacheOracle(spec.num_layers), O.KVCacheOracle(spec.num_layers)
        for x in (hist[i], xs[i]):
            rl, rc = ref.forward(x, rc)
            gl, gc = gold.forward(x, gc)
        e = (last[i].float() - gl[-1]).abs().max().item()
        r = (rl[-1].float() - gl[-1]).abs().max().item()
        assert within_band(e, r, 1e-3 * gl[-1].abs().max().item(), "test_gpu_batch.py:block"), (i, e, r)
    batch.close()
    eng.close()
