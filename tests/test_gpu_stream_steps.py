"""Stream lookahead on the MI355X: the C-level cases of tests/stream_steps_cases.py on libvlo.so (toy128, units of 11 rows: one unit is the
16-row pipeline, three are 33 rows of the block path), then LiveInfer(lookahead=...) end to end against the oracle's per-frame loop."""
import dataclasses

import pytest
import torch

from oracle import vlo_oracle as O
from tests import stream_steps_cases as K
from tests.test_gpu_liveinfer import NEAR_TIE, _build, _drive

pytestmark = pytest.mark.gpu

F = 10                    # frame rows of a unit: 1 + 10 = 11 rows
HIST = 300                # a non-empty cache that already spans two KV pages


def _cfg(spec, **kw):
    from videollm_online_amd.engine import EngineConfig
    kw.setdefault("kv_pool_tokens", 256 * 64)
    return EngineConfig(hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                        num_attention_heads=spec.num_heads, num_key_value_heads=spec.num_kv_heads, vocab_size=spec.vocab_size,
                        rope_theta=spec.rope_theta, rms_norm_eps=spec.rms_eps, vision_hidden_size=spec.vision_hidden_size, **kw)


def _engine(spec, w, **kw):
    from videollm_online_amd.engine import Engine
    eng = Engine(_cfg(spec, **kw))
    eng.load_weights({k: v for k, v in w.items() if not k.startswith("vision.")})
    eng.load_weight("rope.inv_freq", O.rope_inv_freq(spec.head_dim, spec.rope_theta))
    eng.finalize()
    return eng


def _abi(eng, spec):
    from videollm_online_amd import _C
    return K.Abi(_C.lib(), eng._h, spec, "cuda")


@pytest.fixture(scope="module")
def model():
    spec = O.LLM_SPECS["toy128"]
    w = O.init_llm_weights(spec, seed=3)
    eng = _engine(spec, w)
    m = K.Model(_abi(eng, spec), spec, w, HIST)
    m.eng = eng
    yield m
    m.abi.close()
    eng.close()


def test_one_unit_equals_step_and_sample(model):
    K.case_one_unit(model, F)


def test_last_unit_bit_equal_every_unit_in_band(model):
    K.case_units_last_bit_equal(model, F, tag="gpu stream_steps toy128")


def test_five_units_of_eleven_rows(model):
    """55 rows: the widest pass of 11-row units (bit equality of the last unit and K / V only: the band is checked on three units)"""
    K.case_units_last_bit_equal(model, F, units=5, band=False)


def test_commit_leaves_the_kept_unit_last(model):
    K.case_commit_state(model, F)


def test_discarded_rows_are_never_read(model):
    K.case_discarded_rows_unread(model, F, tag="gpu stream_steps discarded toy128")


def test_page_comes_back_with_the_commit():
    spec = O.LLM_SPECS["toy128"]
    w = O.init_llm_weights(spec, seed=3)
    eng = _engine(spec, w, kv_pool_tokens=256 * 3)
    abi = _abi(eng, spec)
    try:
        K.case_page_boundary(abi, spec, O.LlamaOracle(spec, w, torch.bfloat16), 11, F, L=240)     # 240 + 11 = 251 <= 256 < 240 + 33
    finally:
        abi.close()
        eng.close()


def test_refusals_leave_the_session_unchanged(model):
    K.case_refusals(model, F)


def test_tensor_parallel_engine_refused():
    spec = O.LLM_SPECS["toy128"]
    w = O.init_llm_weights(spec, seed=3)
    eng = _engine(spec, w, kv_pool_tokens=1024, tp_rank=0, tp_size=2)
    abi = _abi(eng, spec)
    try:
        K.case_tensor_parallel_refused(abi, spec)
    finally:
        abi.close()
        eng.close()


@pytest.mark.parametrize("kw", [dict(kv_dtype="fp8"), dict(weight_dtype="fp8"), dict(weight_dtype="mxfp4")], ids=["kv_fp8", "w_fp8", "w_mxfp4"])
def test_other_storage_formats_last_unit_bit_equal(kw):
    spec = O.LLM_SPECS["toy128"]
    if kw.get("weight_dtype") == "fp8":                         # toy128's down-proj K = 1408 has no fp8 GEMV plan (11 fragments per wave): 1536
        spec = dataclasses.replace(spec, intermediate_size=1536)
    w = O.init_llm_weights(spec, seed=5)
    eng = _engine(spec, w, kv_pool_tokens=2048, **kw)           # bf16 weights are quantised on the way in
    abi = _abi(eng, spec)
    try:
        K.case_units_last_bit_equal(K.Model(abi, spec, w, 40), F, band=False)
    finally:
        abi.close()
        eng.close()


def test_steps_input_equals_step_input(model):
    K.case_steps_input(model.abi, model.spec, F)


def test_engine_wrappers(model):
    """Engine.steps_input / Session.stream_steps / Session.commit_steps: the thin Python forms of the three calls"""
    spec, eng = model.spec, model.eng
    g = torch.Generator().manual_seed(31)
    frames = torch.randn(3 * F, spec.hidden_size, generator=g).bfloat16().cuda()
    ids = [[7, 8, 9], [model.iid], [model.iid]]
    stage = torch.empty(64, spec.hidden_size, dtype=torch.bfloat16, device="cuda")
    x = eng.steps_input(ids, [frames[k * F:(k + 1) * F] for k in range(3)], stage)
    want = torch.cat([eng.step_input(u, frames[k * F:(k + 1) * F], torch.empty(16, spec.hidden_size, dtype=torch.bfloat16, device="cuda")).clone()
                      for k, u in enumerate(ids)])
    assert torch.equal(x.view(torch.int16), want.view(torch.int16))
    # scattered frame tensors are gathered first
    scattered = [frames[k * F:(k + 1) * F].clone() for k in (2, 0, 1)]
    x2 = eng.steps_input(ids, scattered, torch.empty_like(stage))
    assert torch.equal(x2[3:3 + F].view(torch.int16), frames[2 * F:].view(torch.int16))
    s = eng.new_session()
    eng.llm_step(s, model.hist.cuda(), want_last=False)
    L = len(s)
    ends = [2 + F, 3 + 2 * F, 4 + 3 * F]
    tok = torch.zeros(16, dtype=torch.long, device="cuda")
    p = torch.zeros(16, dtype=torch.float32, device="cuda")
    acc = torch.zeros(1, dtype=torch.int32, device="cuda")
    s.stream_steps(x, ends, 0.3, model.iid, tok, p, acc)
    assert len(s) == L
    s.commit_steps(2)
    assert len(s) == L + ends[1] + 1
    rc, t, pp = model.abi.sample_rc(s._h, 0.3, model.iid)
    assert rc == 0 and (t, pp) == (int(tok[1]), float(p[1]))
    s.close()


# ---- LiveInfer ------------------------------------------------------------------------------------------------------------------------------
# Case 9 needs a stream that is SILENT most of the time, which random weights never are: the interval token would have to be the argmax of
# 2048 logits.  So the lm_head row of the interval token is designed, on the CPU with the oracle alone: the oracle's loop is run, the final
# normed hidden row of every decision (frame steps and response steps) is recorded, and the interval row is the minimum-norm solution of
#   x_t . w = (largest other logit of that row) + GAP   for a frame that shall stay silent,
#   x_t . w = (largest other logit of that row) - GAP   for a frame that shall speak and for every response step.
# Nothing upstream of the lm_head depends on that row, so the hidden rows move only where the sampled tokens move, and two or three rounds
# reach a fixed point.  GAP = 16 logits: p[interval] of a silent frame is then >= 1 / (1 + 2047 e^-16) > 0.999 and every designed decision's
# top-2 margin is far above NEAR_TIE, whatever the engine's fp16 vision tower does to the frame rows.
# Recorded choice: toy128 weights seed 3, ViT seed 1, tokens seed 7 / n_start 19, frames synthetic_frames(16, seed=1234), max_new = 4, threshold
# 0.725 (the default), frame 14 speaks: the third unit of the fourth pass of 4, fifteen frame events before the response (whose own greedy
# tokens are near-tied under random weights); among frames 8..15 it is the one whose speaking token has the clearest top-2 margin (0.69; frames
# 8..13 have 0.03..0.19, too close to NEAR_TIE).
GAP = 16.0
SPEAKS = (14,)
N_FRAMES = 16


class _Recording(O.LlamaOracle):
    """LlamaOracle that records, per forward call, the final-normed hidden state of the last row and its logits"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.rows = []

    def forward(self, x, cache, **kw):
        last = self.spec.num_layers - 1
        taps = {"_layers": (last,)}
        logits, cache = super().forward(x, cache, taps=taps, **kw)
        self.rows.append((O.rmsnorm(taps[f"h{last}"][-1:], self.W["model.norm.weight"], self.spec.rms_eps)[0].float(), logits[-1].float()))
        return logits, cache


def _oracle_run(spec, vspec, w, vw, toks, frames, max_new):
    llm = _Recording(spec, w, torch.bfloat16)
    o = O.LiveInferOracle(llm, vw, vspec, toks, frame_fps=2, max_new=max_new)
    o.load_video(frames)
    o.input_video_stream((len(frames) - 1) / 2)              # every frame queued at once: the backlog
    while o.frame_embeds_queue:
        o()
    return o, llm


def designed_weights(spec, vspec, w, vw, toks, frames, max_new, rounds=5):
    """(weights with the designed interval row, the oracle's trace under them)"""
    iid = toks.interval_id
    w = dict(w)
    w["lm_head.weight"] = w["lm_head.weight"].clone()
    prev = None
    for _ in range(rounds):
        o, llm = _oracle_run(spec, vspec, w, vw, toks, frames, max_new)
        sig = [(e[0], e[1], e[2] if e[0] == "frame" else tuple(e[3])) for e in o.trace]
        want = [("frame", i / 2) for i in range(len(frames))]
        got_frames = [(e[0], e[1]) for e in o.trace if e[0] == "frame"]
        speaks = tuple(int(e[1] * 2) for e in o.trace if e[0] == "frame" and e[2] != iid)
        if sig == prev and speaks == SPEAKS and got_frames == want:
            return w, o.trace
        prev = sig
        # which forward call made which decision: one per frame event, len(ids) per response event
        X, t, k = [], [], 0
        for e in o.trace:
            calls = 1 if e[0] == "frame" else len(e[3])
            for j in range(calls):
                x, logits = llm.rows[k + j]
                other = logits.clone()
                other[iid] = -float("inf")
                silent = e[0] == "frame" and int(e[1] * 2) not in SPEAKS
                X.append(x)
                t.append(other.max().item() + (GAP if silent else -GAP))
            k += calls
        assert k == len(llm.rows)
        X, t = torch.stack(X).double(), torch.tensor(t, dtype=torch.float64)
        w["lm_head.weight"][iid] = torch.linalg.lstsq(X, t[:, None]).solution[:, 0].to(torch.bfloat16)
    raise AssertionError(f"the interval row did not reach a fixed point: frames {speaks} speak")


def _compare(got, ref, min_compared):
    """the rule of test_free_running_stream_matches_oracle: identical events; a divergence only at a near-tie of the reference, then stop"""
    compared, diverged = 0, False
    for i, ev in enumerate(got):
        assert i < len(ref), "engine produced more events than the reference"
        r = ref[i]
        assert ev[0] == r[0] and ev[1] == r[1], f"event {i}: kind/time {ev[:2]} vs {r[:2]}"
        if ev[0] == "frame":
            if ev[2] != r[2]:
                margin, runner = r[5]
                assert margin < NEAR_TIE and ev[2] == runner, f"event {i}: token {ev[2]} vs {r[2]} (margin {margin}, runner-up {runner})"
                diverged = True
                break
            assert ev[3] == r[4], f"event {i}: KV length {ev[3]} vs {r[4]}"
        else:
            assert ev[2] == r[2]
            for j, t in enumerate(ev[3]):
                if j >= len(r[3]) or t != r[3][j]:
                    margin, runner = r[4][j]
                    assert margin < NEAR_TIE and t == runner, f"event {i} token {j}: {t} vs {r[3][j]} (margin {margin})"
                    diverged = True
                    break
            if diverged:
                break
        compared += 1
    if not diverged:
        assert len(got) == len(ref)
    assert compared >= min_compared, f"diverged after {compared} events"
    return compared, diverged


def _toy():
    spec, vspec = O.LLM_SPECS["toy128"], O.VIT_SPECS["toy"]
    return spec, vspec, O.init_llm_weights(spec, seed=3), O.init_vit_weights(vspec, seed=1), O.default_tokens(spec, seed=7, n_start=19)


def test_backlog_stream_matches_oracle():
    spec, vspec, w, vw, toks = _toy()
    frames = O.synthetic_frames(N_FRAMES, vspec.image_size, seed=1234)
    wd, ref = designed_weights(spec, vspec, w, vw, toks, frames, max_new=4)
    # the oracle's own trace has what the case is about: a speaking frame that is neither first nor last of its pass of 4, and clear margins
    frame_events = [e for e in ref if e[0] == "frame"]
    assert [int(e[1] * 2) for e in frame_events if e[2] != toks.interval_id] == list(SPEAKS) and SPEAKS[0] % 4 not in (0, 3)
    assert all(e[5][0] >= NEAR_TIE for e in frame_events), [e[5][0] for e in frame_events]
    eng, li = _build(spec, vspec, wd, vw, toks, max_new_tokens=4, lookahead=4)
    li.load_video(frames.cuda())
    li.input_video_stream((N_FRAMES - 1) / 2)
    while li.frame_embeds_queue:
        li()
    compared, diverged = _compare(list(li.trace), ref, min_compared=8)
    print(f"[liveinfer lookahead=4] {compared}/{len(ref)} events identical, diverged={diverged}, passes {li.lookahead_passes}, "
          f"discarded {li.lookahead_discarded}")
    assert li.lookahead_passes >= 2 and li.lookahead_discarded >= 1
    if not diverged:
        assert len(li.past_key_values) == ref[-1][4] == sum(n for _, n in li.step_log)
        assert li._frames_done == N_FRAMES
    li.reset()
    eng.close()


def _count_calls(monkeypatch):
    from videollm_online_amd.engine import Engine, Session
    calls = {"steps_input": 0, "stream_steps": 0, "commit_steps": 0}
    for cls, name in ((Engine, "steps_input"), (Session, "stream_steps"), (Session, "commit_steps")):
        orig = getattr(cls, name)

        def wrapped(self, *a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(cls, name, wrapped)
    return calls


def test_default_makes_no_new_call(monkeypatch):
    spec, vspec, w, vw, toks = _toy()
    frames = O.synthetic_frames(6, vspec.image_size, seed=1234).cuda()
    calls = _count_calls(monkeypatch)
    out = []
    for kw in ({}, dict(lookahead=1)):
        eng, li = _build(spec, vspec, w, vw, toks, max_new_tokens=5, **kw)
        _drive(li, frames, 6, query_at=1.2)
        out.append((list(li.trace), list(li.step_log), li.lookahead_passes, li.lookahead_discarded))
        li.reset()
        eng.close()
    assert out[0] == out[1] and out[0][2:] == (0, 0) and len(out[0][0]) > 0
    assert calls == {"steps_input": 0, "stream_steps": 0, "commit_steps": 0}


def test_forced_mode_same_schedule(monkeypatch):
    """the schedule of test_scheduled_mode_is_deterministic_and_counts_tokens, with every frame queued at once"""
    spec, vspec, w, vw, toks = _toy()
    frames = O.synthetic_frames(12, vspec.image_size, seed=1234).cuda()
    sched = lambda i: (i % 5 == 4, 6)
    calls = _count_calls(monkeypatch)
    out = []
    for la in (1, 5):
        eng, li = _build(spec, vspec, w, vw, toks, schedule=sched, max_new_tokens=20, lookahead=la)
        li.load_video(frames)
        li.input_query_stream("Please narrate the video in real time.", video_time=0.0)
        li.input_video_stream(11 / 2)
        while li.frame_embeds_queue:
            li()
        resp = [e for e in li.trace if e[0] == "response"]
        out.append(([round(e[1] * 2) for e in resp], [len(e[3]) for e in resp], len(li.past_key_values),
                    [(e[1], e[2], e[3]) for e in li.trace if e[0] == "frame"], list(li.step_log)))
        assert len(li.past_key_values) == sum(n for _, n in li.step_log)
        if la == 5:
            assert li.lookahead_passes >= 3 and li.lookahead_discarded == 0          # keep is every unit: the run is cut at the scheduled speaker
        li.reset()
        eng.close()
    assert out[0][0] == [0, 4, 9] and out[0][1] == [6, 6, 6]
    assert out[1] == out[0]
    assert calls["stream_steps"] == calls["commit_steps"] == calls["steps_input"] >= 3


def test_kv_budget_holds_after_every_pass():
    spec, vspec, w, vw, toks = _toy()
    T = 60
    frames = O.synthetic_frames(T, vspec.image_size, seed=99).cuda()
    budget = 19 + 13 + 256 + 12                                    # sink + longest step + a page, and a little
    eng, li = _build(spec, vspec, w, vw, toks, schedule=lambda i: (False, 0), lookahead=4, kv_budget=budget, prefetch_frames=8)
    after = []
    orig = li._lookahead_pass

    def checked():
        out = orig()
        after.append(len(li.past_key_values))
        return out
    li._lookahead_pass = checked
    li.load_video(frames)
    for t in range(0, T, 6):                                       # a backlog of 6 frames per call
        li.input_video_stream((t + 5) / 2)
        li()
    assert li._frames_done == T and li.lookahead_passes == len(after) >= T // 4
    assert max(after) <= budget, (max(after), budget)
    ev = [e for e in li.trace if e[0] == "evict"]
    assert len(ev) >= 1 and li._kv_budget.evictions == len(ev)
    assert len(li.past_key_values) == sum(n for _, n in li.step_log) - sum(e[3] - e[2] for e in ev)
    li.reset()
    eng.close()
