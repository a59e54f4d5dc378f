"""Eviction of several KV ranges in one pass (include/vlo.h vlo_session_evict_ranges / vlo_tp_session_evict_ranges) on the emulated library
(tests/hip_emul: the engine's sources compiled for the CPU), through the C ABI, at toy sizes.  The multi-range rule is restated in torch in
tests/kv_evict_ranges_util.py; the oracle's caches evicted the same way give the parity legs of the project's 3-way band.

One 300-token fill per spec, forked per case."""
import pytest
import torch

from oracle import vlo_oracle as O
from tests.kv_evict_ranges_util import (SET_A, SET_B, check_kv_after_evict_ranges, evict_ranges_oracle_cache, ranges_arg)
from tests.kv_evict_util import band_check, bits, step_inputs
from tests.test_emul_kv_evict_cpu import FILL, SPECS, TINY, TINY_GQA, Filled, inv_freq, read_all, run_after

SET_C = [(0, 5), (250, 262), (299, 300)]                     # no sink; crosses the page boundary; the last range ends at len
SET_D = [(20 + 10 * i, 23 + 10 * i) for i in range(25)]      # 25 ranges, shifts 3 .. 75
SETS = {"A": SET_A, "B": SET_B, "C": SET_C, "D": SET_D}
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -6


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


_filled = {}


@pytest.fixture(scope="module")
def filled(E):
    def get(name):
        if name not in _filled:
            _filled[name] = Filled(E, SPECS[name], FILL, pool=16384)
        return _filled[name]
    yield get
    for f in _filled.values():
        f.eng.close()
    _filled.clear()


def evict_ranges(E, s, ranges):
    arr, n = ranges_arg(ranges)
    return E.lib().vlo_session_evict_ranges(s, arr, n, None)


def unchanged(E, f, s, before, length):
    now = read_all(E, f.spec, s)
    return f.eng.session_len(s) == length and all(torch.equal(bits(now[k]), bits(before[k])) for k in now)


@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("name", ["TINY_GQA", "TINY_HD128"])
def test_kv_after_evict_ranges_follows_the_rule(E, filled, name, which):
    f = filled(name)
    ranges = SETS[which]
    s = f.eng.fork(f.s, f.len)
    assert evict_ranges(E, s, ranges) == 0, E.lib().vlo_last_error()
    assert f.eng.session_len(s) == f.len - sum(b - a for a, b in ranges)
    check_kv_after_evict_ranges(f"emul {name} {which}", f.before, read_all(E, f.spec, s), ranges, inv_freq(f.spec))


@pytest.mark.parametrize("name", ["TINY_GQA", "TINY_HD128"])
def test_parity_after_evict_ranges(E, filled, name):
    """3 frame steps and 2 decode steps after set A: last-row logits within the band of both oracle caches evicted the same way"""
    f = filled(name)
    s = f.eng.fork(f.s, f.len)
    assert evict_ranges(E, s, SET_A) == 0
    iv = inv_freq(f.spec)
    run_after(f, s, evict_ranges_oracle_cache(f.rc, SET_A, iv), evict_ranges_oracle_cache(f.gc, SET_A, iv), f"emul {name} ranges A", 11)


@pytest.mark.parametrize("name", ["TINY_GQA", "TINY_HD128"])
def test_one_range_is_session_evict(E, filled, name):
    f = filled(name)
    a, b = f.eng.fork(f.s, f.len), f.eng.fork(f.s, f.len)
    assert evict_ranges(E, a, [(5, 47)]) == 0
    assert E.lib().vlo_session_evict(b, 5, 47, None) == 0
    assert f.eng.session_len(a) == f.eng.session_len(b) == f.len - 42
    ka, kb = read_all(E, f.spec, a), read_all(E, f.spec, b)
    for key in ka:
        assert torch.equal(bits(ka[key]), bits(kb[key])), key


def test_touching_and_empty_ranges_are_merged(E, filled):
    f = filled("TINY_GQA")
    a, b = f.eng.fork(f.s, f.len), f.eng.fork(f.s, f.len)
    assert evict_ranges(E, a, [(5, 9), (9, 9), (9, 20)]) == 0
    assert evict_ranges(E, b, [(5, 20)]) == 0
    assert f.eng.session_len(a) == f.eng.session_len(b) == f.len - 15
    ka, kb = read_all(E, f.spec, a), read_all(E, f.spec, b)
    for key in ka:
        assert torch.equal(bits(ka[key]), bits(kb[key])), key
    assert evict_ranges(E, a, []) == 0 and evict_ranges(E, a, [(7, 7), (30, 30)]) == 0      # nothing left: a no-op
    assert unchanged(E, f, a, kb, f.len - 15)


def test_argument_and_config_errors(E, filled):
    f = filled("TINY_GQA")
    s = f.eng.fork(f.s, f.len)
    bad = {"65 ranges": [(2 * i, 2 * i + 1) for i in range(65)], "overlapping": [(5, 20), (19, 30)], "descending": [(40, 50), (10, 20)],
           "b > len": [(5, 10), (290, f.len + 1)], "b < a": [(9, 5)], "a < 0": [(-1, 5)]}
    for tag, ranges in bad.items():
        assert evict_ranges(E, s, ranges) == E_INVALID, tag
        assert unchanged(E, f, s, f.before, f.len), tag
    assert evict_ranges(E, s, [(2 * i, 2 * i + 1) for i in range(64)]) == 0                   # the cap itself is accepted
    assert f.eng.session_len(s) == f.len - 64
    # an fp8 KV pool is refused cleanly
    from tests.test_emul_kv_fp8_cpu import loaded
    f8 = loaded(E, TINY_GQA, f.w, 1)
    s8 = f8.new_session()
    f8.llm_step(s8, step_inputs(f.spec, f.ref, f.toks, 1, [45])[0], want_all=False)
    k8 = read_all(E, f.spec, s8)
    assert evict_ranges(E, s8, [(5, 20), (25, 30)]) == E_UNSUPPORTED
    assert b"fp8" in E.lib().vlo_last_error()
    now = read_all(E, f.spec, s8)
    assert f8.session_len(s8) == 45 and all(torch.equal(bits(now[k]), bits(k8[k])) for k in now)
    f8.close()


def test_pending_lookahead_pass_refuses(E, filled):
    from tests.stream_steps_cases import Abi
    f = filled("TINY_GQA")
    abi = Abi(E.lib(), f.eng._h, f.spec, "cpu")
    s = f.eng.fork(f.s, f.len)
    x = step_inputs(f.spec, f.ref, f.toks, 17, [11])[0]
    abi.steps(s, x, [10], 0.725, f.toks.interval_id)
    assert evict_ranges(E, s, SET_A) == E_STATE
    assert b"pending" in E.lib().vlo_last_error()
    abi.commit(s, 1)
    assert f.eng.session_len(s) == f.len + 11
    assert evict_ranges(E, s, SET_A) == 0
    assert f.eng.session_len(s) == f.len + 11 - 33


def test_tensor_parallel_evict_ranges(E):
    """T = 2 logical ranks: every shard evicted alike with set A, then two steps in band against the evicted oracle"""
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
        call = lambda ranges: E.lib().vlo_tp_session_evict_ranges(s, *ranges_arg(ranges), None)
        assert call([(12, 102)]) == E_INVALID and call([(30, 40), (35, 50)]) == E_INVALID
        assert grp.session_len(s) == 101
        # a shard does not go through the single-GPU entry
        assert evict_ranges(E, grp.engines[0].new_session(), [(0, 0)]) == E_STATE
        assert call(SET_A) == 0, E.lib().vlo_last_error()
        assert grp.session_len(s) == 101 - 33
        rc, gc = evict_ranges_oracle_cache(rc, SET_A, iv), evict_ranges_oracle_cache(gc, SET_A, iv)
        for i, x in enumerate(step_inputs(spec, ref, toks, 4, [11, 1])):
            rl, rc = ref.forward(x, rc)
            gl, gc = gold.forward(x, gc)
            last, allr = grp.llm_step(s, x)
            assert grp.session_len(s) == len(rc)
            band_check("emul tp2 ranges", i, allr[-1], rl[-1], gl[-1])
    finally:
        grp.close()
