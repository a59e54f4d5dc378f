"""Batched steps (include/vlo.h vlo_batch_*) on the emulated library (tests/hip_emul: the engine's sources compiled for the CPU), through
the C ABI, at toy sizes.

On the 16-row path a session stepped inside a batch must end exactly where vlo_llm_step leaves it: the same last-row logits and the same
K / V bytes, bit for bit (every kernel of the step treats rows independently and the attention segments keep the solo launch's split
geometry).  The 64-row block path is held to the project's 3-way band against the oracle.  Each session is forked before the batched
step, and the fork is stepped alone for the comparison."""
import ctypes as C
import os

import pytest
import torch

from oracle import vlo_oracle as O
from tests.parity_util import within_band
from tests.test_emul_kv_fp8_cpu import TINY, TINY_GQA, TINY_HD128, E, inputs, loaded  # noqa: F401  (E: the module's fixture)

FULL = os.environ.get("VLO_EMUL_FULL") == "1"             # the longer cases (as in test_emul_kv_fp8_cpu.py)
SPECS = {"TINY": TINY, "TINY_GQA": TINY_GQA, "TINY_HD128": TINY_HD128}
SCALES = {"TINY": ([1.0, 1.0], [1.0, 1.0]), "TINY_GQA": ([0.37, 0.052], [0.21, 1.7]), "TINY_HD128": ([0.11, 0.6], [0.45, 0.093])}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Batch:
    def __init__(self, E, eng, max_sessions):
        self.E, self.eng = E, eng
        h = C.c_void_p()
        E.check(E.lib().vlo_batch_create(eng._h, max_sessions, C.byref(h)))
        self._h = h

    def step_rc(self, sessions, xs):
        """(return code, last logits [B][V]) of vlo_batch_step"""
        B, V = len(sessions), self.eng.spec.vocab_size
        x = torch.cat([t.bfloat16() for t in xs]).contiguous() if xs else torch.zeros(1, self.eng.spec.hidden_size, dtype=torch.bfloat16)
        n = (C.c_int * max(B, 1))(*[t.shape[0] for t in xs])
        ss = (C.c_void_p * max(B, 1))(*[s.value if s is not None else None for s in sessions])
        last = torch.zeros(max(B, 1), V, dtype=torch.bfloat16)
        rc = self.E.lib().vlo_batch_step(self._h, ss, B, _ptr(x), n, _ptr(last), None)
        return rc, last[:B]

    def step(self, sessions, xs):
        rc, last = self.step_rc(sessions, xs)
        self.E.check(rc)
        return last

    def stream_sample(self, B, threshold, interval_id):
        tok, p = torch.zeros(B, dtype=torch.long), torch.zeros(B, dtype=torch.float32)
        self.E.check(self.E.lib().vlo_batch_stream_sample(self._h, threshold, interval_id, _ptr(tok), _ptr(p), None))
        return tok.tolist(), p.tolist()

    def greedy(self, sessions, xs, eos, max_new):
        B = len(sessions)
        x = torch.cat([t.bfloat16() for t in xs]).contiguous()
        m = (C.c_int * B)(*[t.shape[0] for t in xs])
        ss = (C.c_void_p * B)(*[s.value for s in sessions])
        ids = torch.zeros(B, max_new, dtype=torch.long)
        nw = (C.c_int * B)()
        self.E.check(self.E.lib().vlo_batch_greedy_generate(self._h, ss, B, _ptr(x), m, eos, _ptr(ids), max_new, nw, None))
        return [ids[b, :nw[b]].tolist() for b in range(B)]

    def close(self):
        self.E.lib().vlo_batch_destroy(self._h)


def rows(spec, seed, n):
    return torch.randn(n, spec.hidden_size, generator=torch.Generator().manual_seed(seed)).bfloat16()


def grown(eng, spec, lens, seed):
    """sessions prefixed to the given lengths (random embedding rows, stepped alone)"""
    out = []
    for i, L in enumerate(lens):
        s = eng.new_session()
        done = 0
        while done < L:
            k = min(64, L - done)
            eng.llm_step(s, rows(spec, seed * 1000 + i * 50 + done, k), want_all=False)
            done += k
        out.append(s)
    return out


def read_kv(E, eng, s, layer, which, kvh, t0, t1):
    out = torch.zeros(t1 - t0, eng.spec.head_dim, dtype=torch.bfloat16)
    E.check(E.lib().vlo_session_read_kv(s, layer, which, kvh, t0, t1, _ptr(out), None))
    return out


def assert_same_as_solo(E, eng, batch, sessions, xs):
    spec = eng.spec
    lens = [eng.session_len(s) for s in sessions]
    forks = [eng.fork(s, L) for s, L in zip(sessions, lens)]
    last = batch.step(sessions, xs)
    for b, (s, f, x, L) in enumerate(zip(sessions, forks, xs, lens)):
        want, _ = eng.llm_step(f, x, want_all=False)
        assert eng.session_len(s) == eng.session_len(f) == L + x.shape[0]
        assert torch.equal(last[b].view(torch.int16), want.view(torch.int16)), (b, (last[b].float() - want.float()).abs().max())
        for layer in range(spec.num_layers):
            for h in range(spec.num_kv_heads):
                for which in (0, 1):
                    got = read_kv(E, eng, s, layer, which, h, L, L + x.shape[0])
                    ref = read_kv(E, eng, f, layer, which, h, L, L + x.shape[0])
                    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (b, layer, h, which)
    return forks


# ---- 1. the 16-row path equals solo stepping, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("spec_name,kv_dtype", [("TINY_GQA", 1)] +
                         ([("TINY", 0), ("TINY_HD128", 1), ("TINY", 1), ("TINY_GQA", 0), ("TINY_HD128", 0)] if FULL else []))
def test_16_row_batch_bit_equal_to_solo(E, spec_name, kv_dtype):
    spec = SPECS[spec_name]
    w = O.init_llm_weights(spec, seed=11)
    eng = loaded(E, spec, w, kv_dtype, SCALES[spec_name] if kv_dtype else None, kv_pool_tokens=256 * 24)
    b = Batch(E, eng, 4)
    # lengths on both sides of a page boundary: 250 + 11 rows cross it, 259 starts on the second page
    ss = grown(eng, spec, [3, 20, 259, 250], seed=1)
    xs = [rows(spec, 100 + i, n) for i, n in enumerate([1, 1, 3, 11])]
    assert_same_as_solo(E, eng, b, ss, xs)
    # a second step on the same sessions (the table ring's next slot), n = 1 each
    xs = [rows(spec, 200 + i, 1) for i in range(4)]
    assert_same_as_solo(E, eng, b, ss, xs)
    b.close()
    eng.close()


def test_16_sessions_of_one_row(E):
    spec = TINY_GQA
    w = O.init_llm_weights(spec, seed=12)
    eng = loaded(E, spec, w, 0, kv_pool_tokens=256 * 40)
    b = Batch(E, eng, 16)
    ss = grown(eng, spec, [1 + 3 * i for i in range(16)], seed=2)
    assert_same_as_solo(E, eng, b, ss, [rows(spec, 400 + i, 1) for i in range(16)])
    b.close()
    eng.close()


# ---- 2. the block path (17..64 rows) within the band of the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("spec_name", ["TINY_HD128"] + (["TINY_GQA"] if FULL else []))
def test_block_path_batch_within_band(E, spec_name):
    spec = SPECS[spec_name]
    w = O.init_llm_weights(spec, seed=13)
    toks = O.default_tokens(spec)
    ref, gold = O.LlamaOracle(spec, w, torch.bfloat16), O.LlamaOracle(spec, w, torch.float32)
    eng = loaded(E, spec, w, 0, kv_pool_tokens=256 * 12)
    b = Batch(E, eng, 4)
    hist = [inputs(spec, ref, toks, 20 + i, [L]) for i, L in enumerate([45, 7, 250, 30])]
    ss = []
    for h in hist:
        s = eng.new_session()
        for x in h:
            eng.llm_step(s, x, want_all=False)
        ss.append(s)
    xs = [inputs(spec, ref, toks, 40 + i, [11])[0] for i in range(4)]          # 4 x 11 = 44 rows: the block path
    last = b.step(ss, xs)
    for i, s in enumerate(ss):
        rc, gc = O.KVCacheOracle(spec.num_layers), O.KVCacheOracle(spec.num_layers)
        for x in hist[i] + [xs[i]]:
            rl, rc = ref.forward(x, rc)
            gl, gc = gold.forward(x, gc)
        e = (last[i].float() - gl[-1]).abs().max().item()
        r = (rl[-1].float() - gl[-1]).abs().max().item()
        slack = 1e-3 * gl[-1].abs().max().item()
        print(f"[emul batch block {spec_name}] session {i}: engine err {e:.4g} ref-bf16 err {r:.4g}")
        assert within_band(e, r, slack, f"test_emul_batch_cpu.py:{spec_name}"), (i, e, r)
        assert eng.session_len(s) == len(rc)
    b.close()
    eng.close()


# ---- 3. the batched samplers equal the solo samplers ------------------------------------------------------------------------------------
def test_batched_stream_sample_equals_solo(E):
    spec = TINY_GQA
    w = O.init_llm_weights(spec, seed=14)
    toks = O.default_tokens(spec)
    eng = loaded(E, spec, w, 0, kv_pool_tokens=256 * 16)
    b = Batch(E, eng, 5)
    ss = grown(eng, spec, [5, 60, 130, 9, 33], seed=3)
    xs = [rows(spec, 500 + i, n) for i, n in enumerate([1, 2, 1, 10, 1])]
    forks = assert_same_as_solo(E, eng, b, ss, xs)
    iid = toks.interval_id
    solo0 = [eng.stream_sample(f, 0.0, iid) for f in forks]
    p = sorted(pp for _, pp in solo0)
    thr = (p[1] + p[2]) / 2 if p[1] != p[2] else p[2] * 1.5     # some rows fall below the threshold, some do not
    solo = [eng.stream_sample(f, thr, iid) for f in forks]
    got_tok, got_p = b.stream_sample(len(ss), thr, iid)
    assert got_tok == [t for t, _ in solo]
    assert got_p == [pp for _, pp in solo]
    assert any(pp < thr for pp in got_p) and any(pp >= thr for pp in got_p)
    # the sessions' own samplers read the rows the batch handed back
    assert [eng.stream_sample(s, thr, iid) for s in ss] == solo
    b.close()
    eng.close()


def test_batched_greedy_generate_equals_solo(E):
    """Ids, lengths and end states equal vlo_greedy_generate on forks.  One EOS id per call: chosen as a token one session first emits at
    step k (k = 2, then 5) and another never does, so the sessions of a call stop at different steps (k and max_new)."""
    spec = TINY_GQA
    w = O.init_llm_weights(spec, seed=15)
    eng = loaded(E, spec, w, 0, kv_pool_tokens=256 * 48)
    max_new = 6
    cands = grown(eng, spec, [4 + 5 * i for i in range(6)], seed=4)
    prefix = [rows(spec, 600 + i, 1 + i % 3) for i in range(6)]
    free = [eng.greedy_generate(eng.fork(s, eng.session_len(s)), x, -1, max_new) for s, x in zip(cands, prefix)]
    b = Batch(E, eng, 3)
    for k in (2, 5):
        pick = None
        for t in range(spec.vocab_size):
            first = [ids.index(t) + 1 if t in ids else None for ids in free]
            a = [i for i, f in enumerate(first) if f == k]
            d = [i for i, f in enumerate(first) if f is None]
            if a and d:
                pick = (t, [a[0], d[0]])
                break
        assert pick is not None, free
        eos, chosen = pick
        sessions = [eng.fork(cands[i], eng.session_len(cands[i])) for i in chosen]
        forks = [eng.fork(cands[i], eng.session_len(cands[i])) for i in chosen]
        xs = [prefix[i] for i in chosen]
        want = [eng.greedy_generate(f, x, eos, max_new) for f, x in zip(forks, xs)]
        assert [len(ids) for ids in want] == [k, max_new]
        assert b.greedy(sessions, xs, eos, max_new) == want
        assert [eng.session_len(s) for s in sessions] == [eng.session_len(f) for f in forks]
        # the session that stopped on EOS holds no logits, the other one the logits of its last token (vlo_greedy_generate's end states)
        assert E.lib().vlo_stream_sample(sessions[0], 0.0, 0, _ptr(torch.zeros(1, dtype=torch.long)), None, None) == -4
        assert eng.stream_sample(sessions[1], 0.0, 0) == eng.stream_sample(forks[1], 0.0, 0)
    # the long-prefix form (sum m > 16: each prefix stepped alone) ends the same way
    sessions = [eng.fork(s, eng.session_len(s)) for s in cands[:3]]
    forks = [eng.fork(s, eng.session_len(s)) for s in cands[:3]]
    xs = [rows(spec, 700 + i, 9) for i in range(3)]
    want = [eng.greedy_generate(f, x, eos, max_new) for f, x in zip(forks, xs)]
    assert b.greedy(sessions, xs, eos, max_new) == want
    assert [eng.session_len(s) for s in sessions] == [eng.session_len(f) for f in forks]
    b.close()
    eng.close()


# ---- 4. refusals, and a pool that cannot hold the whole batch ---------------------------------------------------------------------------
def test_refusals_leave_sessions_unchanged(E):
    spec = TINY
    w = O.init_llm_weights(spec, seed=16)
    eng = loaded(E, spec, w, 0, kv_pool_tokens=256 * 5)
    other = loaded(E, spec, w, 0, kv_pool_tokens=256 * 2)
    L = E.lib()
    h = C.c_void_p()
    for bad in (0, 17, -1):
        assert L.vlo_batch_create(eng._h, bad, C.byref(h)) == -1
    b = Batch(E, eng, 3)
    (s0,) = grown(eng, spec, [250], seed=5)
    s1, s2, s3 = eng.fork(s0, 250), eng.fork(s0, 250), eng.fork(s0, 250)
    eng.llm_step(s3, rows(spec, 805, 7), want_all=False)               # 257 tokens: 2 pages; with s0, 5 of 5 pages are taken
    eng.crop(s0, 0)                                                    # one page free
    o1 = other.new_session()
    x1 = rows(spec, 800, 1)

    def refused(sessions, xs, code=-1, what=None):
        lens = [eng.session_len(s) for s in (s1, s2, s3)]
        rc, _ = b.step_rc(sessions, xs)
        assert rc == code, (rc, L.vlo_last_error())
        if what:
            assert what in L.vlo_last_error().decode(), L.vlo_last_error()
        assert [eng.session_len(s) for s in (s1, s2, s3)] == lens

    refused([], [], what="batch of 0")
    refused([s1, s2, s3, s1], [x1] * 4, what="max_sessions")
    refused([s1, None], [x1, x1], what="null session")
    refused([s1, s2, s1], [x1] * 3, what="repeats")
    refused([s1, o1], [x1, x1], what="another engine")
    refused([s1, s2], [x1, x1[:0]], what="appends 0")
    refused([s1, s2, s3], [rows(spec, 801, 30)] * 3, what="at most 64")
    # 11 rows each: s1 and s2 both need their second page, one is free -> nothing is taken, nobody advances
    refused([s1, s2], [rows(spec, 802, 11)] * 2, code=-3, what="KV pool exhausted")
    # the free page is still there: a batch in which only one of them needs it goes through
    b.step([s3, s1], [x1, rows(spec, 803, 11)])
    assert [eng.session_len(s) for s in (s1, s2, s3)] == [261, 250, 258]
    refused([s2], [rows(spec, 804, 11)], code=-3, what="KV pool exhausted")
    b.close()
    eng.close()
    other.close()


def test_tensor_parallel_engine_refused(E):
    spec = TINY
    w = O.init_llm_weights(spec, seed=17)
    eng = E.EmulEngine(spec, kv_pool_tokens=1024, tp_rank=0, tp_size=2).load_weights(w, O.rope_inv_freq(spec.head_dim, spec.rope_theta))
    h = C.c_void_p()
    assert E.lib().vlo_batch_create(eng._h, 2, C.byref(h)) == -4
    assert b"tensor-parallel" in E.lib().vlo_last_error()
    eng.close()
