"""LiveInfer(kv_budget=..., kv_policy="oldest" | "frames_first") on the CPU (videollm-online_amd/inference.py KvBudget): a fake KV session
that keeps one TAG per cached token and applies evict / evict_ranges to that list stands in for the engine, so only the host bookkeeping
runs — which tokens are frame pieces, which are text, what leaves first.  The engine's side is tests/test_emul_kv_evict_ranges_cpu.py and
tests/test_gpu_kv_evict_ranges.py.

The run: 400 frames at 2 FPS; the first step carries the start prompt (the sink); a query with its response after frame 5; a scheduled
response every 50 frames; the frame after a response carries [eos] + the stream prompt.  Budget 640."""
import inspect

import pytest

from videollm_online_amd import trace as T
from videollm_online_amd.inference import KV_EVICT_MAX_RANGES, KV_PAGE_TOKENS, KvBudget, LiveInfer, StreamTokens

FRAME_TOKENS = 10
TOKS = StreamTokens(start_ids=list(range(100, 135)), stream_prompt_ids=[7, 8], stream_generation_ids=[9, 10, 11, 12], eos_token_id=2,
                    interval_id=11)
SINK = len(TOKS.start_ids)
LONGEST_STEP = 1 + len(TOKS.stream_prompt_ids) + FRAME_TOKENS
BUDGET, FRAMES = 640, 400
QUERY_IDS = list(range(200, 212))


class TagSession:
    """what LiveInfer uses of a KV handle; the cache is a list of tags, ("sink" | "frame" | "text", serial)"""

    def __init__(self):
        self.tags = []
        self.newest = 0                    # where the newest step starts (an eviction below it moves it down)
        self.evicts, self.calls = [], []   # (t0, t1, length before, stream) / ([(a, b)], length before, stream)

    def __len__(self):
        return len(self.tags)

    get_seq_length = __len__

    def __bool__(self):
        return True

    def append(self, tags):
        self.tags += tags

    def evict(self, t0, t1, stream=None):
        assert 0 <= t0 <= t1 <= len(self.tags)
        self.evicts.append((t0, t1, len(self.tags), stream))
        del self.tags[t0:t1]
        self.newest -= t1 - t0

    def evict_ranges(self, ranges, stream=None):
        ranges = [tuple(r) for r in ranges]
        L, prev = len(self.tags), SINK
        assert 1 <= len(ranges) <= KV_EVICT_MAX_RANGES
        for a, b in ranges:
            assert prev <= a < b <= L, (ranges, L)                      # ascending, non-empty, above the sink
            assert prev < a or prev == SINK, ("touching ranges are merged", ranges)
            assert b <= self.newest, ("never inside the newest step", (a, b), self.newest)
            prev = b
        self.calls.append((ranges, L, stream))
        for a, b in reversed(ranges):
            del self.tags[a:b]
        self.newest -= sum(b - a for a, b in ranges)

    def close(self):
        pass


def fake_liveinfer(policy, budget=BUDGET):
    """a LiveInfer whose device plumbing is replaced by stand-ins (as tests/test_liveinfer_evict_cpu.py): the policy arguments and the methods
    that record steps and enforce the budget are the product's own"""
    li = LiveInfer.__new__(LiveInfer)
    li.frame_num_tokens, li.frame_token_interval_id = FRAME_TOKENS, TOKS.interval_id
    li._start_ids, li._added_stream_prompt_ids = list(TOKS.start_ids), list(TOKS.stream_prompt_ids)
    li._added_stream_generation_ids = list(TOKS.stream_generation_ids)
    li._record, li._main = 65536, "main-stream"
    li._kv_budget = KvBudget(budget, SINK, LONGEST_STEP, *(() if policy is None else (policy,)))
    li.past_key_values = None
    li.reset()
    li.past_key_values = TagSession()
    return li


def stream(li, frames, response_tokens, respond_every=50, query_at=5):
    """the token flow of a live stream through the product's _log_step / _enforce_kv_budget; yields the length after every enforce"""
    s = li.past_key_values
    serial = [0]

    def text(n):
        serial[0] += n
        return [("text", i) for i in range(serial[0] - n, serial[0])]

    def step(tags, lead):
        s.newest = len(s)
        li._log_step(len(s), len(tags), lead=lead)
        s.append(tags)

    def respond(prefix, f):
        step(text(len(prefix)), None)
        for _ in range(response_tokens - 1):                             # the last token (eos) is never fed
            step(text(1), None)
        li._enforce_kv_budget(f / 2)

    after_response = False
    for f in range(frames):
        if len(s) == 0:
            lead, head = list(TOKS.start_ids), [("sink", i) for i in range(SINK)]
        elif after_response:
            lead = [TOKS.eos_token_id] + TOKS.stream_prompt_ids
            head = text(len(lead))
        else:
            lead, head = [TOKS.interval_id], [("frame", f)]              # a silent continuation: the interval id belongs to the frame
        step(head + [("frame", f)] * FRAME_TOKENS, lead)
        li._enforce_kv_budget(f / 2)
        yield len(s)
        after_response = False
        if f == query_at or f % respond_every == respond_every - 1:
            respond(QUERY_IDS if f == query_at else TOKS.stream_generation_ids, f)
            yield len(s)
            after_response = True


# the evict calls (t0, t1, length before) of KvBudget as it stood before kv_policy existed, on this very run with 16-token responses
OLDEST_RECORDED = [
    (35, 305, 645), (35, 310, 650), (35, 309, 658), (35, 310, 650), (35, 309, 650), (35, 310, 650), (35, 309, 650), (35, 310, 650),
    (35, 309, 650), (35, 310, 650), (35, 309, 650), (35, 310, 650), (35, 309, 650), (35, 310, 650), (35, 309, 650),
]


@pytest.mark.parametrize("policy", [None, "oldest"])
def test_oldest_is_todays_call_sequence(policy):
    li = fake_liveinfer(policy)
    lens = list(stream(li, FRAMES, 16))
    s = li.past_key_values
    assert s.calls == []                                                 # never an evict_ranges call
    assert [(t0, t1, L) for t0, t1, L, _ in s.evicts] == OLDEST_RECORDED
    assert all(st == "main-stream" for *_, st in s.evicts) and max(lens) <= BUDGET
    ev = [e for e in li.trace if e[0] == T.EVICT]
    assert [(e.t0, e.t1, e.kv_len) for e in ev] == [(t0, t1, L - (t1 - t0)) for t0, t1, L in OLDEST_RECORDED]


def test_frames_first_keeps_the_dialogue():
    li = fake_liveinfer("frames_first")
    s = li.past_key_values
    lens = list(stream(li, FRAMES, 16))
    assert max(lens) <= BUDGET                                           # the bound holds after every enforce
    assert s.evicts == [] and len(s.calls) >= 5
    n_text = sum(1 for kind, _ in s.tags if kind == "text")
    all_text = 1 + max(i for kind, i in s.tags if kind == "text")
    assert SINK + all_text + LONGEST_STEP <= BUDGET - KV_PAGE_TOKENS     # the text alone fits: no text piece ever has to go ...
    assert n_text == all_text                                            # ... and none went
    assert s.tags[:SINK] == [("sink", i) for i in range(SINK)]
    assert sorted(f for kind, f in s.tags if kind == "frame") == [f for kind, f in s.tags if kind == "frame"]   # order kept
    assert ("frame", FRAMES - 1) in s.tags
    for ranges, L, st in s.calls:
        assert st == "main-stream" and L > BUDGET and L - sum(b - a for a, b in ranges) <= BUDGET - KV_PAGE_TOKENS
    # one event per range, ascending, in the coordinates before its call; kv_len is the length after the call
    ev = [(e.t0, e.t1, e.kv_len) for e in li.trace if e[0] == T.EVICT]
    want = [(a, b, L - sum(y - x for x, y in ranges)) for ranges, L, _ in s.calls for a, b in ranges]
    assert ev == want
    assert all(isinstance(e, T.EvictEvent) and len(e) == len(T.EVICT_FIELDS) for e in li.trace if e[0] == T.EVICT)
    assert sum(m for _, m, _ in li._kv_budget.pieces) + SINK == len(s)   # the pieces always describe the cache


def test_frames_first_falls_back_to_the_oldest_text():
    """responses so long that the text alone exceeds the budget: the bound still holds, frames leave first, then the oldest text"""
    li = fake_liveinfer("frames_first")
    s = li.past_key_values
    gone_before = 0
    for L in stream(li, 120, 90, respond_every=5):
        assert L <= BUDGET
        kept = [i for kind, i in s.tags if kind == "text"]
        if kept:
            assert kept == list(range(kept[0], kept[-1] + 1))            # what is left of the text is its newest part: the oldest went first
            if kept[0] > gone_before:                                    # text left in this enforce: no frame older than the newest step stayed
                assert all(kind != "frame" for kind, _ in s.tags[SINK:s.newest])
                gone_before = kept[0]
    assert gone_before > 0 and s.evicts == []
    assert s.tags[:SINK] == [("sink", i) for i in range(SINK)]


def test_more_than_64_ranges_take_several_calls():
    """135 one-frame ranges between kept text pieces: three calls, each in the coordinates the cache has before it"""
    kb = KvBudget(2048, SINK, LONGEST_STEP, "frames_first")
    s = TagSession()
    s.append([("sink", i) for i in range(SINK)])
    for f in range(150):                                                 # every frame step carries a 3-id text prefix: frames never touch
        kb.note_step(len(s), 3 + FRAME_TOKENS, [2, 7, 8], FRAME_TOKENS, TOKS.interval_id)
        s.newest = len(s)
        s.append([("text", 3 * f + j) for j in range(3)] + [("frame", f)] * FRAME_TOKENS)
    assert len(s) == SINK + 150 * 13 == 1985
    kb.budget = 900                                                      # now over the budget by far
    out = kb.enforce_ranges(s, "st")
    # 1 985 - 10 m <= 900 - 256 needs m = 135 frames = 64 + 64 + 7 ranges
    assert [len(r) for r, _, _ in s.calls] == [64, 64, 7] and len(out) == 135
    assert len(s) == 1985 - 1350 <= 900 - KV_PAGE_TOKENS
    assert sum(1 for kind, _ in s.tags if kind == "text") == 450 and [f for kind, f in s.tags if kind == "frame"] == [f for f in range(135, 150) for _ in range(10)]
    assert [x[2] for x in out] == [1985 - 640] * 64 + [1985 - 1280] * 64 + [1985 - 1350] * 7
    assert [x[:2] for x in out[:2]] == [(38, 48), (51, 61)] and [x[:2] for x in out[64:66]] == [(38 + 3 * 64, 48 + 3 * 64), (51 + 3 * 64, 61 + 3 * 64)]


def test_policy_arguments():
    p = inspect.signature(LiveInfer.__init__).parameters
    assert p["kv_policy"].default is None
    with pytest.raises(ValueError, match="kv_policy without kv_budget"):
        LiveInfer(None, kv_policy="frames_first")
    with pytest.raises(ValueError, match="kv_policy"):
        LiveInfer(None, kv_budget=640, kv_policy="newest")
    with pytest.raises(ValueError, match="kv_policy"):
        KvBudget(640, SINK, LONGEST_STEP, "newest")
    assert KvBudget(640, SINK, LONGEST_STEP).policy == "oldest"
