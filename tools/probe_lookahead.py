"""Stream-lookahead probe at the true Llama-3-8B shape (random weights generated on the GPU): one vlo_stream_steps pass over `units` queued
frame steps of 11 rows against the same units stepped one by one through vlo_llm_step + vlo_stream_sample (the per-frame loop), measured in
the same process, alternated, with device events after a warm-up; the session is cropped back between rounds.

  (a) units in {1, 2, 3, 5} at Lc in {4096, 15519}: median of --iters rounds
  (b) end to end: LiveInfer on a resident all-silent stream that is 5 frames behind at every call, lookahead = 1 against 5, frames/s
  --trace U: only (a) at Lc = 15519 with U units, 3 rounds — the run to put under `rocprofv3 --kernel-trace --stats`

    python tools/probe_lookahead.py [--only a] [--iters 10] [--frames 300]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from videollm_online_amd.engine import Engine, EngineConfig
from videollm_online_amd.synthetic import LLM_SHAPES, VIT_SHAPES, gpu_random_weights, gpu_synthetic_frames, stream_tokens

ROWS = 11          # one frame step: [interval id] + 10 frame tokens
IID = 11


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def case(eng, s, Lc, units, iters):
    """session s at cache length Lc; each timed call is followed by a crop back to Lc (not timed)"""
    H = eng.cfg.hidden_size
    x = torch.randn(units * ROWS, H, device="cuda").bfloat16()
    ends = [(u + 1) * ROWS - 1 for u in range(units)]
    tok = torch.zeros(16, dtype=torch.long, device="cuda")
    p = torch.zeros(16, dtype=torch.float32, device="cuda")
    acc = torch.zeros(1, dtype=torch.int32, device="cuda")

    def solo():
        for u in range(units):
            eng.llm_step(s, x[u * ROWS:(u + 1) * ROWS], want_last=False)
            eng.stream_sample(s, 0.725, IID, tok_out=tok, p_out=p)

    def lookahead():
        s.stream_steps(x, ends, 0.725, IID, tok, p, acc)

    def back(pending):
        torch.cuda.synchronize()
        if pending:
            s.commit_steps(units)
        s.crop(Lc)

    for fn, pending in ((solo, False), (lookahead, True)):           # warm-up
        fn()
        back(pending)
    t_solo, t_la = [], []
    for _ in range(iters):                                           # alternated
        t_solo.append(timed(solo))
        back(False)
        t_la.append(timed(lookahead))
        back(True)
    t_solo.sort()
    t_la.sort()
    ms_s, ms_l = t_solo[len(t_solo) // 2], t_la[len(t_la) // 2]
    alg = eng.step_algorithmic_bytes(Lc, units * ROWS)
    print(f"(a) Lc={Lc} units={units} ({units * ROWS} rows): one pass {ms_l:.3f} ms | {units} solo steps + samples {ms_s:.3f} ms "
          f"(one {ms_s / units:.3f} ms) | pass / solo {ms_l / ms_s:.2f} | pass / one solo {ms_l / (ms_s / units):.2f}x | "
          f"alg {alg / 1e9:.2f} GB -> {alg / (ms_l * 1e-3) / 1e12:.2f} TB/s", flush=True)


def end_to_end(eng, cfg, n_frames, behind):
    from videollm_online_amd.inference import LiveInfer
    from videollm_online_amd.modeling_live import LiveModel
    toks = stream_tokens(cfg.vocab_size)
    model = LiveModel(eng, eos_token_id=toks.eos_token_id, frame_token_interval_id=toks.interval_id)
    frames = gpu_synthetic_frames(n_frames, seed=1234)
    out = {}
    for la in (1, behind, 1, behind):                                # two alternated rounds each; the second is reported
        li = LiveInfer(model, tokens=toks, frame_fps=2, prefetch=True, prefetch_frames=behind, schedule=lambda i: (False, 0), lookahead=la)
        li.load_video(frames)
        li.input_video_stream(0.0)                                   # the first frame carries the 35-id start prompt: stepped alone, not timed
        li()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(behind, n_frames, behind):                    # every call finds `behind` frames queued
            li.input_video_stream(i / 2)
            li()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        done = li._frames_done - 1
        out[la] = (done / dt, li.lookahead_passes, len(li.past_key_values))
        li.reset()
    for la, (fps, passes, kv) in out.items():
        print(f"(b) LiveInfer lookahead={la}: {fps:.1f} frames/s ({n_frames} resident all-silent frames, {behind} queued per call, "
              f"{passes} passes, KV {kv} at the end)", flush=True)
    print(f"(b) lookahead={behind} / lookahead=1: {out[behind][0] / out[1][0]:.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ab")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--units", default="1,2,3,5")
    ap.add_argument("--lcs", default="4096,15519")
    ap.add_argument("--frames", type=int, default=301)
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    vit = VIT_SHAPES["siglip-l16-384"] if "b" in args.only and not args.trace else None
    cfg = EngineConfig(**LLM_SHAPES["llama-3-8b"], vision_hidden_size=1024, vit=vit, kv_pool_tokens=15519 + 4096 + 1024)
    eng = Engine(cfg)
    gpu_random_weights(eng, cfg, seed=0)
    eng.finalize()
    print(f"Llama-3-8B shape, random weights, packed weights {eng.weight_bytes / 1e9:.2f} GB", flush=True)
    H = cfg.hidden_size
    if args.trace:
        s = eng.new_session()
        eng.llm_step(s, torch.randn(15519, H, device="cuda").bfloat16(), want_last=False)
        case(eng, s, 15519, args.trace, 3)
        s.close()
    elif "a" in args.only:
        for Lc in [int(v) for v in args.lcs.split(",")]:
            s = eng.new_session()
            eng.llm_step(s, torch.randn(Lc, H, device="cuda").bfloat16(), want_last=False)
            for units in [int(v) for v in args.units.split(",")]:
                case(eng, s, Lc, units, args.iters)
            s.close()
    if "b" in args.only and not args.trace:
        end_to_end(eng, cfg, args.frames, 5)
    eng.close()


if __name__ == "__main__":
    main()
