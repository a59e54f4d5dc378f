"""KV eviction with RoPE re-rotation (include/vlo.h vlo_session_evict / vlo_tp_session_evict) on the emulated library (tests/hip_emul: the
engine's sources compiled for the CPU), through the C ABI, at toy sizes.  The rule is restated in torch in tests/kv_evict_util.py; the same
eviction applied to the oracle's caches (one bf16 reference, one fp32 gold that rotates without rounding) gives the parity legs of the
project's 3-way band.

About 9 minutes of emulation, 5 of them the 1 000-token fill of the pages-come-back case (attention over a growing cache, every GPU thread an
OS thread).  VLO_EMUL_FULL=1 adds the 700-token cases (an eviction longer than a page, a page-aligned one)."""
import ctypes as C
import os

import pytest
import torch

from oracle import vlo_oracle as O
from tests.kv_evict_util import band_check, bits, check_kv_after_evict, evict_oracle_cache, step_inputs

FULL = os.environ.get("VLO_EMUL_FULL") == "1"
TINY = O.LlmSpec(128, 192, 2, 2, 2, 256, 10000.0, 1e-5, vision_hidden_size=128)        # head dim 64, MHA (two kv heads: T = 2 shards)
TINY_GQA = O.LlmSpec(128, 192, 2, 2, 1, 256, 10000.0, 1e-5, vision_hidden_size=128)    # head dim 64, 2 query heads per kv head
TINY_HD128 = O.LlmSpec(256, 192, 2, 2, 1, 256, 10000.0, 1e-5, vision_hidden_size=128)  # head dim 128, GQA
SPECS = {"TINY": TINY, "TINY_GQA": TINY_GQA, "TINY_HD128": TINY_HD128}
FILL = [150, 150]                # ~300 tokens: crosses one page boundary
FILL_FULL = [175, 175, 175, 175]  # 700 tokens: three pages


@pytest.fixture(scope="module")
def E():
    import resource
    soft, _ = resource.getrlimit(resource.RLIMIT_NPROC)
    if soft != resource.RLIM_INFINITY and soft < 4096:
        pytest.skip(f"the emulation runs every GPU thread of a block as an OS thread (up to 1024): RLIMIT_NPROC = {soft}")
    from tests.hip_emul import emul_engine
    if emul_engine.lib() is None:
        pytest.skip("no clang++ to build the emulated library")
    return emul_engine


def inv_freq(spec):
    return O.rope_inv_freq(spec.head_dim, spec.rope_theta)


def evict(E, s, t0, t1):
    return E.lib().vlo_session_evict(s, t0, t1, None)


def read_all(E, spec, s, kv_heads=None):
    L = int(E.lib().vlo_session_len(s))
    out = {}
    for layer in range(spec.num_layers):
        for which in (0, 1):
            for h in range(spec.num_kv_heads if kv_heads is None else kv_heads):
                t = torch.zeros(L, spec.head_dim, dtype=torch.bfloat16)
                E.check(E.lib().vlo_session_read_kv(s, layer, which, h, 0, L, C.c_void_p(t.data_ptr()), None))
                out[(layer, which, h)] = t
    return out


class Filled:
    """an engine, a session filled with `lens` tokens, its K / V as read then, and the oracle's two caches after the same inputs"""

    def __init__(self, E, spec, lens, pool=1024):
        self.spec = spec
        self.w = O.init_llm_weights(spec, seed=3)
        self.toks = O.default_tokens(spec)
        self.ref, self.gold = O.LlamaOracle(spec, self.w, torch.bfloat16), O.LlamaOracle(spec, self.w, torch.float32)
        self.eng = E.EmulEngine(spec, kv_pool_tokens=pool).load_weights(self.w, inv_freq(spec))
        self.s = self.eng.new_session()
        self.rc = self.gc = None
        for x in step_inputs(spec, self.ref, self.toks, 1, lens):
            self.eng.llm_step(self.s, x, want_all=False)
            _, self.rc = self.ref.forward(x, self.rc, logits_from=x.shape[0] - 1)
            _, self.gc = self.gold.forward(x, self.gc, logits_from=x.shape[0] - 1)
        self.len = sum(lens)
        assert self.eng.session_len(self.s) == self.len == len(self.rc)
        self.before = read_all(E, spec, self.s)


_filled = {}


@pytest.fixture(scope="module")
def filled(E):
    def get(name, full=False):
        key = (name, full)
        if key not in _filled:
            _filled[key] = Filled(E, SPECS[name], FILL_FULL if full else FILL, pool=16384)
        return _filled[key]
    yield get
    for f in _filled.values():
        f.eng.close()
    _filled.clear()


def clone_cache(c):
    out = O.KVCacheOracle(len(c.k))
    out.k, out.v = [k.clone() for k in c.k], [v.clone() for v in c.v]
    return out


RANGES = [(5, 47), (3, 40), (0, 11), (260, 290)]          # even d; odd d (V^T misaligned); no sink; t0 in the second page
RANGES_FULL = [(10, 310), (256, 512)]                     # d > a page; page-aligned
CASES = [(n, False, r) for n in ("TINY_GQA", "TINY_HD128") for r in RANGES] + \
        ([(n, True, r) for n in ("TINY_GQA", "TINY_HD128") for r in RANGES_FULL] if FULL else [])


@pytest.mark.parametrize("name,full,rng", CASES, ids=[f"{n}-{r[0]}-{r[1]}" for n, _, r in CASES])
def test_kv_after_evict_follows_the_rule(E, filled, name, full, rng):
    f = filled(name, full)
    t0, t1 = rng
    s = f.eng.fork(f.s, f.len)
    assert evict(E, s, t0, t1) == 0, E.lib().vlo_last_error()
    assert f.eng.session_len(s) == f.len - (t1 - t0)
    check_kv_after_evict(f"emul {name}", f.before, read_all(E, f.spec, s), t0, t1, inv_freq(f.spec))


def run_after(f, s, rc, gc, tag, seed, lens=(11, 11, 11, 1, 1)):
    for i, x in enumerate(step_inputs(f.spec, f.ref, f.toks, seed, lens)):
        rl, rc = f.ref.forward(x, rc)
        gl, gc = f.gold.forward(x, gc)
        last, allr = f.eng.llm_step(s, x)
        assert f.eng.session_len(s) == len(rc) and torch.equal(last, allr[-1])
        band_check(tag, i, allr[-1], rl[-1], gl[-1])
    return rc, gc


PARITY = [("TINY_GQA", False, (3, 40)), ("TINY_HD128", False, (5, 47))] + ([("TINY_GQA", True, (10, 310)), ("TINY_HD128", True, (256, 512))] if FULL else [])


@pytest.mark.parametrize("name,full,rng", PARITY, ids=[f"{n}-{r[0]}-{r[1]}" for n, _, r in PARITY])
def test_parity_after_eviction(E, filled, name, full, rng):
    """3 frame steps and 2 decode steps after one eviction: last-row logits within the band of the oracle evicted the same way"""
    f = filled(name, full)
    t0, t1 = rng
    s = f.eng.fork(f.s, f.len)
    assert evict(E, s, t0, t1) == 0
    iv = inv_freq(f.spec)
    run_after(f, s, evict_oracle_cache(f.rc, t0, t1, iv), evict_oracle_cache(f.gc, t0, t1, iv), f"emul {name} one eviction", 11)


@pytest.mark.parametrize("name", ["TINY_GQA", "TINY_HD128"])
def test_parity_with_interleaved_evictions(E, filled, name):
    """4 evictions interleaved with steps: keys that survive several re-rotations (each one more bf16 rounding, on both bf16 legs)"""
    f = filled(name)
    s = f.eng.fork(f.s, f.len)
    rc, gc = clone_cache(f.rc), clone_cache(f.gc)
    iv = inv_freq(f.spec)
    for j, (t0, t1) in enumerate([(35, 46), (35, 58), (20, 21), (35, 290)]):
        assert evict(E, s, t0, t1) == 0
        rc, gc = evict_oracle_cache(rc, t0, t1, iv), evict_oracle_cache(gc, t0, t1, iv)
        rc, gc = run_after(f, s, rc, gc, f"emul {name} eviction {j}", 20 + j, lens=(11, 1) if j < 3 else (11, 11, 11, 1, 1))


def test_evict_to_the_end_is_crop(E, filled):
    f = filled("TINY_GQA")
    a, b = f.eng.fork(f.s, f.len), f.eng.fork(f.s, f.len)
    assert evict(E, a, 270, f.len) == 0
    f.eng.crop(b, 270)
    assert f.eng.session_len(a) == f.eng.session_len(b) == 270
    ka, kb = read_all(E, f.spec, a), read_all(E, f.spec, b)
    for key in ka:
        assert torch.equal(bits(ka[key]), bits(kb[key])), key
    x = step_inputs(f.spec, f.ref, f.toks, 5, [11])[0]
    assert torch.equal(bits(f.eng.llm_step(a, x)[1]), bits(f.eng.llm_step(b, x)[1]))


def test_pages_come_back(E):
    spec = TINY_GQA
    f = Filled(E, spec, [250, 250, 250, 250], pool=1024)              # session A at 1 000 of 1 024 tokens
    try:
        b = f.eng.new_session()
        xb = step_inputs(spec, f.ref, f.toks, 9, [300])[0]
        last = torch.zeros(spec.vocab_size, dtype=torch.bfloat16)
        rc = E.lib().vlo_llm_step(b, C.c_void_p(xb.data_ptr()), 300, C.c_void_p(last.data_ptr()), None, None)
        assert rc == -3                                               # VLO_E_NOMEM
        assert f.eng.session_len(f.s) == 1000 and f.eng.session_len(b) == 0
        now = read_all(E, spec, f.s)
        for key in now:
            assert torch.equal(bits(now[key]), bits(f.before[key])), key
        assert evict(E, f.s, 20, 620) == 0
        assert f.eng.session_len(f.s) == 400
        f.eng.llm_step(b, xb, want_all=False)                         # two pages came back: B's 300 tokens fit now
        assert f.eng.session_len(b) == 300
        iv = inv_freq(spec)
        run_after(f, f.s, evict_oracle_cache(f.rc, 20, 620, iv), evict_oracle_cache(f.gc, 20, 620, iv), "emul pages come back", 13, lens=(11,))
    finally:
        f.eng.close()


def test_argument_and_config_errors(E, filled):
    f = filled("TINY_GQA")
    s = f.eng.fork(f.s, f.len)
    for t0, t1 in ((-1, 5), (5, f.len + 1), (7, 6)):
        assert evict(E, s, t0, t1) == -1, (t0, t1)                    # VLO_E_INVALID
    assert evict(E, s, 9, 9) == 0                                     # no-op
    assert f.eng.session_len(s) == f.len
    now = read_all(E, f.spec, s)
    for key in now:
        assert torch.equal(bits(now[key]), bits(f.before[key])), key
    # an fp8 KV pool is refused cleanly
    from tests.test_emul_kv_fp8_cpu import loaded
    f8 = loaded(E, TINY_GQA, f.w, 1)
    s8 = f8.new_session()
    f8.llm_step(s8, step_inputs(f.spec, f.ref, f.toks, 1, [45])[0], want_all=False)
    k8 = read_all(E, f.spec, s8)
    assert evict(E, s8, 5, 20) == -6                                  # VLO_E_UNSUPPORTED
    assert b"fp8" in E.lib().vlo_last_error()
    assert f8.session_len(s8) == 45
    now = read_all(E, f.spec, s8)
    for key in now:
        assert torch.equal(bits(now[key]), bits(k8[key])), key
    f8.close()


def test_tensor_parallel_evict(E):
    """T = 2 logical ranks: every shard evicted alike, then steps in band against the evicted oracle"""
    spec = TINY
    w = O.init_llm_weights(spec, seed=6)
    toks = O.default_tokens(spec)
    ref, gold = O.LlamaOracle(spec, w, torch.bfloat16), O.LlamaOracle(spec, w, torch.float32)
    iv = inv_freq(spec)
    grp = E.EmulTpGroup(spec, 2, w, iv)
    try:
        s = grp.new_session()
        rc = gc = None
        for x in step_inputs(spec, ref, toks, 3, [45, 45, 11]):
            grp.llm_step(s, x, want_all=False)
            _, rc = ref.forward(x, rc, logits_from=x.shape[0] - 1)
            _, gc = gold.forward(x, gc, logits_from=x.shape[0] - 1)
        assert E.lib().vlo_tp_session_evict(s, 12, 102, None) == -1 and E.lib().vlo_tp_session_evict(s, 5, 4, None) == -1
        assert E.lib().vlo_tp_session_evict(s, 35, 72, None) == 0
        assert grp.session_len(s) == 101 - 37
        rc, gc = evict_oracle_cache(rc, 35, 72, iv), evict_oracle_cache(gc, 35, 72, iv)
        for i, x in enumerate(step_inputs(spec, ref, toks, 4, [11, 1])):
            rl, rc = ref.forward(x, rc)
            gl, gc = gold.forward(x, gc)
            last, allr = grp.llm_step(s, x)
            assert grp.session_len(s) == len(rc)
            band_check("emul tp2", i, allr[-1], rl[-1], gl[-1])
    finally:
        grp.close()
