"""The host policy of LiveInfer(lookahead=K) (videollm-online_amd/inference.py::_lookahead_pass) on the CPU: a fake engine and a fake KV
session stand in for the device, the "model" is a script that says which frames speak.  What runs is the product's own queue logic: how a
backlog of frames is cut into units (the reference's query rules, the schedule, the 64-row and K caps), what goes back to the queue, and the
events, step log and KV length it leaves — all of which must equal what the per-frame loop (lookahead = 1) leaves on the same script.
The engine's side of a pass is checked in tests/test_emul_stream_steps_cpu.py and tests/test_gpu_stream_steps.py."""
import collections
import random

import pytest
import torch

from videollm_online_amd import inference as I
from videollm_online_amd import trace as T
from videollm_online_amd.inference import KvBudget, LiveInfer, StreamTokens

FRAME_TOKENS = 10
EOS, IID, SPEAK = 2, 11, 9
QUERY = "q"


def tokens(n_start=19):
    return StreamTokens(start_ids=list(range(100, 100 + n_start)), stream_prompt_ids=[7, 8], stream_generation_ids=[SPEAK, 10, 12, 13],
                        eos_token_id=EOS, interval_id=IID, query_ids={QUERY: [20, 21, 22, 23, 24]})


class Rows:
    """stand-in for a staged step input: which ids and which frame each unit holds"""

    def __init__(self, units):
        self.units = units                                    # [(ids, frame index)]
        self.shape = (sum(len(i) + FRAME_TOKENS for i, _ in units), 8)


class FakeStream:
    def __init__(self):
        self.waited = 0

    def wait_event(self, ev):
        assert ev == "ready"
        self.waited += 1

    def synchronize(self):
        pass


class FakeSession:
    def __init__(self, script):
        self.script, self.len, self.last_frame, self.pending = script, 0, None, None
        self.passes, self.evicts = [], []

    def __len__(self):
        return self.len

    def __bool__(self):
        return True

    def close(self):
        pass

    def evict(self, t0, t1, stream=None):
        assert self.pending is None and 0 <= t0 <= t1 <= self.len
        self.evicts.append((t0, t1))
        self.len -= t1 - t0

    def stream_steps(self, x, ends, thr, iid, tok_out, p_out, accept_out, stream=None):
        assert self.pending is None and len(ends) == len(x.units) and ends[-1] == x.shape[0] - 1
        assert 1 <= len(ends) <= 16 and x.shape[0] <= 64
        toks = [self.script(f) for _, f in x.units]
        for k, t in enumerate(toks):
            tok_out[k] = t
        accept_out[0] = next((k + 1 for k, t in enumerate(toks) if t != iid), len(toks))
        self.pending = (x, ends)
        self.passes.append([(len(i), f) for i, f in x.units])

    def commit_steps(self, keep):
        x, ends = self.pending
        assert 1 <= keep <= len(ends)
        self.len += ends[keep - 1] + 1
        self.last_frame = x.units[keep - 1][1]
        self.pending = None


class FakeEngine:
    def __init__(self):
        self.calls = collections.Counter()

    def step_input(self, ids, frame, out):
        self.calls["step_input"] += 1
        return Rows([(list(ids), frame)])

    def steps_input(self, ids_per_unit, frames, out):
        self.calls["steps_input"] += 1
        assert len(ids_per_unit[0]) <= 32 and all(len(i) <= 4 for i in ids_per_unit[1:])
        return Rows([(list(i), f) for i, f in zip(ids_per_unit, frames)])

    def llm_step(self, session, x, want_last=False):
        self.calls["llm_step"] += 1
        assert session.pending is None
        session.len += x.shape[0]
        session.last_frame = x.units[-1][1]

    def stream_sample(self, session, thr, iid, tok_out=None, p_out=None):
        self.calls["stream_sample"] += 1
        tok_out[0] = session.script(session.last_frame)


class FakeModel:
    def __init__(self, script):
        self.script = script

    def new_cache(self):
        return FakeSession(self.script)


def fake_liveinfer(script, lookahead, toks=None, schedule=None, kv_budget=None):
    """a LiveInfer whose device plumbing is replaced by stand-ins; _call_for_streaming and everything under it is the product's"""
    toks = toks or tokens()
    li = LiveInfer.__new__(LiveInfer)
    li.model, li.engine = FakeModel(script), FakeEngine()
    li.frame_num_tokens, li.frame_token_interval_id, li.eos_token_id = FRAME_TOKENS, IID, EOS
    li.frame_token_interval_threshold, li.frame_fps = 0.725, 2
    li.tokens = toks
    li._start_ids, li._added_stream_prompt_ids = list(toks.start_ids), list(toks.stream_prompt_ids)
    li._added_stream_generation_ids = list(toks.stream_generation_ids)
    li._record, li._main, li.prefetch, li.schedule = 4096, FakeStream(), False, schedule
    li._stage = Rows([([0] * 70, None)])                       # (only its row count is read)
    li.lookahead = lookahead
    li._tok_dev, li._p_dev, li._tok_host = torch.zeros(1, dtype=torch.long), torch.zeros(1), torch.zeros(1, dtype=torch.long)
    li._toks_dev, li._ps_dev = torch.zeros(16, dtype=torch.long), torch.zeros(16)
    li._accept_dev, li._toks_host, li._accept_host = torch.zeros(1, dtype=torch.int32), torch.zeros(16, dtype=torch.long), torch.zeros(1, dtype=torch.int32)
    li._kv_budget = None
    if kv_budget is not None:
        li._kv_budget = KvBudget(kv_budget, len(li._start_ids), 1 + len(li._added_stream_prompt_ids) + FRAME_TOKENS)
    li.past_key_values = None
    li.reset()
    return li


def queue_frames(li, lo, hi):
    for i in range(lo, hi):
        li.frame_embeds_queue.append((i / 2, (i, "ready")))
    li.last_frame_idx = hi - 1


def respond(li, video_time, query, n_tokens=3):
    """what _call_for_response leaves behind, without a model: the prompt step, n - 1 fed-back tokens, [eos] as last_ids"""
    ids = li.tokens.query_ids[query] if query is not None else li._added_stream_generation_ids
    s = li.past_key_values
    li._log_step(s.len, len(ids))
    for j in range(n_tokens - 1):
        li._log_step(s.len + len(ids) + j, 1)
    s.len += len(ids) + n_tokens - 1
    li.last_ids = [EOS]
    li.trace.append(T.response_event(video_time, query, [5] * (n_tokens - 1) + [EOS]))
    li._enforce_kv_budget(video_time)


def drive(li, n_frames, chunk, queries=()):
    """queue `chunk` frames at a time (a backlog), then call the stream until the queue is empty, answering as __call__ does"""
    for t, q in queries:
        li.query_queue.append((t, q))
    for lo in range(0, n_frames, chunk):
        queue_frames(li, lo, min(n_frames, lo + chunk))
        while li.frame_embeds_queue:
            queued = [t for t, _ in li.frame_embeds_queue]
            assert queued == sorted(queued)                    # requeued frames come back in order, in front
            vt, q = li._call_for_streaming()
            if vt is not None:
                respond(li, vt, q)
    return li


def outcome(li):
    return list(li.trace), list(li.step_log), len(li.past_key_values), li._frames_done, list(li.query_queue), li.last_ids


SCRIPTS = {
    "silent": lambda f: IID,
    "every7th": lambda f: 33 if f % 7 == 6 else IID,
    "bursts": lambda f: 44 if f % 11 in (3, 4, 9) else IID,
    "first": lambda f: 55 if f == 0 else IID,
}


@pytest.mark.parametrize("lookahead", [2, 4, 5, 16])
@pytest.mark.parametrize("script", list(SCRIPTS))
@pytest.mark.parametrize("queries", [(), ((0.0, QUERY),), ((3.2, QUERY), (3.4, QUERY), (9.5, QUERY)), ((7.0, QUERY), (30.0, QUERY))],
                         ids=["noq", "q0", "qbetween", "qat"])
def test_same_outcome_as_the_per_frame_loop(lookahead, script, queries):
    a = drive(fake_liveinfer(SCRIPTS[script], 1), 40, 9, queries)
    b = drive(fake_liveinfer(SCRIPTS[script], lookahead), 40, 9, queries)
    assert outcome(b) == outcome(a)
    assert a.engine.calls["steps_input"] == 0 and a.lookahead_passes == 0          # the default never takes the new path
    assert b.engine.calls["llm_step"] == 0 and b.lookahead_passes == b.engine.calls["steps_input"] == len(b.past_key_values.passes)
    frames = sum(1 for e in b.trace if e[0] == T.FRAME)
    assert b._frames_done == 40 and frames == sum(1 for e in a.trace if e[0] == T.FRAME) <= 40     # one event per committed frame (none for a rule-2 frame)
    assert sum(len(p) for p in b.past_key_values.passes) == 40 + b.lookahead_discarded


def test_units_are_cut_at_queries():
    # a query due between frames 2 and 3 ends the run before frame 3 (rule 1); one at frame 6's time makes frame 6 the run's last unit (rule 2)
    li = fake_liveinfer(SCRIPTS["silent"], 16)
    drive(li, 10, 10, ((1.2, QUERY), (3.0, QUERY)))
    assert [[f for _, f in p] for p in li.past_key_values.passes] == [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9]]
    kinds = [(e[0], e[1]) for e in li.trace]
    assert kinds == [("frame", 0.0), ("frame", 0.5), ("frame", 1.0), ("response", 1.2), ("frame", 1.5), ("frame", 2.0), ("frame", 2.5),
                     ("response", 3.0), ("frame", 3.5), ("frame", 4.0), ("frame", 4.5)]
    # unit 0 of each pass carries the step's text ids: the start prompt, then [eos] + the stream prompt after a response
    assert [p[0][0] for p in li.past_key_values.passes] == [19, 3, 3] and all(k == 1 for p in li.past_key_values.passes for k, _ in p[1:])


def test_discarded_units_go_back_in_order():
    li = fake_liveinfer(lambda f: 77 if f in (2, 3) else IID, 5, toks=tokens(n_start=5))      # 15 + 4 x 11 = 59 rows: five units fit
    queue_frames(li, 0, 8)
    assert li._call_for_streaming() == (1.0, None)             # frame 2 speaks: units 3 and 4 of [0..4] are thrown away
    assert [f for _, (f, _) in li.frame_embeds_queue] == [3, 4, 5, 6, 7]
    assert (li.lookahead_passes, li.lookahead_discarded, li._frames_done) == (1, 2, 3)
    assert [e[:4] for e in li.trace] == [("frame", 0.0, IID, 15), ("frame", 0.5, IID, 26), ("frame", 1.0, 77, 37)]
    respond(li, 1.0, None)
    assert li._call_for_streaming() == (1.5, None)             # frame 3 speaks at once: the whole rest of its pass goes back
    assert [f for _, (f, _) in li.frame_embeds_queue] == [4, 5, 6, 7] and li.lookahead_discarded == 2 + 4
    respond(li, 1.5, None)
    assert li._call_for_streaming() == (None, None)
    assert li._frames_done == 8 and not li.frame_embeds_queue and li.past_key_values.pending is None
    assert li._main.waited == 5 + 5 + 4                        # every unit's ready event is waited on, each time it is staged


def test_schedule_cuts_the_run_after_the_scheduled_speaker():
    sched = lambda i: (i % 5 == 4, 6)
    a = drive(fake_liveinfer(SCRIPTS["bursts"], 1, schedule=sched), 23, 23)
    b = drive(fake_liveinfer(SCRIPTS["bursts"], 16, schedule=sched), 23, 23)
    assert outcome(b) == outcome(a)
    assert [[f for _, f in p] for p in b.past_key_values.passes] == [[0, 1, 2, 3], [4], [5, 6, 7, 8, 9], [10, 11, 12, 13, 14], [15, 16, 17, 18, 19],
                                                                     [20, 21, 22]]
    assert b.lookahead_discarded == 0                          # keep is every unit
    # the tokens are the forced ones, the sampler's own choice is recorded beside them
    assert all(e.token == (SPEAK if int(e.video_time * 2) % 5 == 4 else IID) and e.sampled == SCRIPTS["bursts"](int(e.video_time * 2))
               for e in b.trace if e[0] == T.FRAME)


def test_row_and_unit_caps():
    li = drive(fake_liveinfer(SCRIPTS["silent"], 16), 40, 40)
    sizes = [len(p) for p in li.past_key_values.passes]
    rows = [sum(k + FRAME_TOKENS for k, _ in p) for p in li.past_key_values.passes]
    assert sizes[0] == 4 and rows[0] == 29 + 33                # 19 start ids: a fifth unit would make 73 rows
    assert set(sizes[1:-1]) == {5} and max(rows) <= 64         # 5 x 11 = 55; six would be 66
    li = drive(fake_liveinfer(SCRIPTS["silent"], 3), 40, 40)
    assert max(len(p) for p in li.past_key_values.passes) == 3
    # a text prefix the first unit cannot carry (more than 32 ids) is stepped alone, the backlog behind it in passes
    li = drive(fake_liveinfer(SCRIPTS["silent"], 4, toks=tokens(n_start=35)), 9, 9)
    assert li.engine.calls["llm_step"] == 1 and [[f for _, f in p] for p in li.past_key_values.passes] == [[1, 2, 3, 4], [5, 6, 7, 8]]
    assert [n for _, n in li.step_log] == [45] + [11] * 8


def test_lookahead_one_is_todays_path_and_bad_values_are_refused():
    import inspect
    assert inspect.signature(LiveInfer.__init__).parameters["lookahead"].default == 1
    li = drive(fake_liveinfer(SCRIPTS["every7th"], 1), 20, 5)
    assert li.engine.calls["steps_input"] == 0 and li.engine.calls["llm_step"] == 20 and li.lookahead_passes == li.lookahead_discarded == 0
    assert (I.LOOKAHEAD_MAX_UNITS, I.LOOKAHEAD_MAX_ROWS, I.LOOKAHEAD_IDS_MAX) == (16, 64, 32)


def test_kv_budget_is_enforced_once_per_pass():
    budget = 19 + 13 + 256 + 20
    rng = random.Random(3)
    speak = {f for f in range(300) if rng.random() < 0.05}
    li = fake_liveinfer(lambda f: 66 if f in speak else IID, 5, kv_budget=budget)
    s = None
    for lo in range(0, 300, 7):
        queue_frames(li, lo, min(300, lo + 7))
        while li.frame_embeds_queue:
            n_ev = len(li.past_key_values.evicts) if li.past_key_values else 0
            vt, q = li._call_for_streaming()
            s = li.past_key_values
            assert s.len <= budget                             # after every pass (and every per-frame step) the cache is inside the budget
            if vt is not None:
                respond(li, vt, q)
                assert s.len <= budget
            assert len(s.evicts) - n_ev <= 3
    ev = [e for e in li.trace if e[0] == T.EVICT]
    assert len(ev) == len(s.evicts) >= 3 and all((e.t0, e.t1) == x for e, x in zip(ev, s.evicts))
    assert s.len == sum(n for _, n in li.step_log) - sum(t1 - t0 for t0, t1 in s.evicts)
