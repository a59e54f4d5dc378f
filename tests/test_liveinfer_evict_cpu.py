"""The bounded-context policy of LiveInfer (videollm-online_amd/inference.py: kv_budget / kv_sink, KvBudget) on the CPU: a fake model and a
fake KV session stand in for the engine, so only the host bookkeeping runs — which steps become spans, when ONE eviction is issued and of
what range.  The engine's side of an eviction is checked in tests/test_emul_kv_evict_cpu.py and tests/test_gpu_kv_evict.py."""
import collections
import random

import pytest

from videollm_online_amd import trace as T
from videollm_online_amd.inference import KV_PAGE_TOKENS, KvBudget, LiveInfer, StreamTokens

FRAME_TOKENS = 10
TOKS = StreamTokens(start_ids=list(range(100, 135)), stream_prompt_ids=[7, 8], stream_generation_ids=[9, 10, 11, 12], eos_token_id=2,
                    interval_id=11)


class FakeSession:
    """what LiveInfer uses of a KV handle, plus a log of the evict calls"""

    def __init__(self):
        self.len = 0
        self.evicts = []

    def __len__(self):
        return self.len

    def get_seq_length(self):
        return self.len

    def __bool__(self):
        return True

    def evict(self, t0, t1, stream=None):
        assert 0 <= t0 <= t1 <= self.len
        self.evicts.append((t0, t1, self.len, stream))
        self.len -= t1 - t0

    def close(self):
        pass


def fake_liveinfer(kv_budget, kv_sink=None):
    """a LiveInfer whose device plumbing is replaced by stand-ins: the constructor's policy arguments and the methods that record steps
    and enforce the budget are the product's own"""
    li = LiveInfer.__new__(LiveInfer)
    li.frame_num_tokens = FRAME_TOKENS
    li._start_ids, li._added_stream_prompt_ids = list(TOKS.start_ids), list(TOKS.stream_prompt_ids)
    li._added_stream_generation_ids = list(TOKS.stream_generation_ids)
    li._record, li._main = 4096, "main-stream"
    li._kv_budget = None
    if kv_budget is not None:
        li._kv_budget = KvBudget(kv_budget, len(li._start_ids) if kv_sink is None else kv_sink, 1 + len(li._added_stream_prompt_ids) + FRAME_TOKENS)
    li.past_key_values = None
    li.reset()
    li.past_key_values = FakeSession()
    return li


def stream(li, frames, seed=0, respond_every=9):
    """the token flow of a live stream: frame steps (the first carries the start prompt; one after a response carries [eos] + the stream
    prompt) and a response every few frames (a prefix step, then one-token decode steps), each followed by the product's budget check"""
    rng = random.Random(seed)
    s = li.past_key_values
    after_response = False
    for f in range(frames):
        n = (len(TOKS.start_ids) if s.len == 0 else 1 + (len(TOKS.stream_prompt_ids) if after_response else 0)) + FRAME_TOKENS
        li._log_step(s.len, n)
        s.len += n
        li._enforce_kv_budget(f / 2)
        yield s.len, n
        after_response = False
        if f % respond_every == respond_every - 1:
            m = len(TOKS.stream_generation_ids)
            k = rng.randint(1, 30)
            li._log_step(s.len, m)
            for j in range(k - 1):
                li._log_step(s.len + m + j, 1)
            s.len += m + k - 1
            li._enforce_kv_budget(f / 2)
            yield s.len, m + k - 1
            after_response = True


def test_liveinfer_constructor_takes_the_policy_arguments():
    import inspect
    p = inspect.signature(LiveInfer.__init__).parameters
    assert p["kv_budget"].default is None and p["kv_sink"].default is None


@pytest.mark.parametrize("budget,sink", [(600, None), (1024, None), (700, 0), (900, 100)])
def test_budget_holds_and_evictions_are_whole_oldest_spans(budget, sink):
    li = fake_liveinfer(budget, sink)
    s = li.past_key_values
    sink_n = len(TOKS.start_ids) if sink is None else sink
    # an independent model of the spans: every step's tokens past the sink, oldest first
    spans = collections.deque()
    orig_log = li._log_step

    def log(Lc, n):
        orig_log(Lc, n)
        k = Lc + n - max(Lc, sink_n)
        if k > 0:
            spans.append(k)
    li._log_step = log
    seen = 0
    appended_at_last_evict = None
    appended = 0
    last_len = 0
    for (L, n) in stream(li, 400):
        assert L <= budget + n                                   # never more than the budget plus the step that crossed it
        assert L <= budget or len(spans) == 1
        appended += n
        for (t0, t1, len_before, st) in s.evicts[seen:]:
            assert st == "main-stream" and t0 == sink_n          # the sink is never touched
            d = 0
            while d < t1 - t0:
                d += spans.popleft()                             # whole oldest spans, in order
            assert d == t1 - t0 and len(spans) >= 1              # ... and never the newest
            assert len_before > budget and len_before - d <= budget - KV_PAGE_TOKENS
            if appended_at_last_evict is not None:
                assert appended - appended_at_last_evict >= KV_PAGE_TOKENS     # steady state: at most one eviction per page appended
            appended_at_last_evict = appended
        assert len(s.evicts) - seen <= 1                         # ONE evict call per check
        seen = len(s.evicts)
        assert sum(spans) + min(sink_n, L) == L == s.len         # the spans always describe the cache
        last_len = L
    assert len(s.evicts) >= 5 and last_len <= budget + 64
    ev = [e for e in li.trace if e[0] == T.EVICT]
    assert len(ev) == len(s.evicts)
    for e, (t0, t1, len_before, _) in zip(ev, s.evicts):
        assert isinstance(e, T.EvictEvent) and len(e) == len(T.EVICT_FIELDS)
        assert (e.t0, e.t1, e.kv_len) == (t0, t1, len_before - (t1 - t0))


def test_no_budget_never_evicts():
    li = fake_liveinfer(None)
    list(stream(li, 400))
    assert li.past_key_values.evicts == [] and li.past_key_values.len > 4000
    assert all(e[0] != T.EVICT for e in li.trace)


def test_too_small_budget_is_refused():
    longest = 1 + len(TOKS.stream_prompt_ids) + FRAME_TOKENS
    need = len(TOKS.start_ids) + longest + KV_PAGE_TOKENS
    with pytest.raises(ValueError):
        fake_liveinfer(need - 1)
    fake_liveinfer(need)
    with pytest.raises(ValueError):
        fake_liveinfer(900, kv_sink=900 - KV_PAGE_TOKENS)
    with pytest.raises(ValueError):
        KvBudget(1000, -1, 13)


def test_reset_clears_the_spans():
    li = fake_liveinfer(600)
    list(stream(li, 20))
    assert len(li._kv_budget.spans) > 0
    li.reset()
    assert len(li._kv_budget.spans) == 0 and li.past_key_values is None


def test_evict_event_schema():
    assert T.EVICT_FIELDS == ("kind", "video_time", "t0", "t1", "kv_len")
    e = T.evict_event(1.5, 35, 290, 400)
    assert e == ("evict", 1.5, 35, 290, 400)
    assert T.FRAME_FIELDS == ("kind", "video_time", "token", "kv_len", "sampled") and T.RESPONSE_FIELDS == ("kind", "video_time", "query", "output_ids")
