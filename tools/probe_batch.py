"""Batched-step probe at the true Llama-3-8B shape (random weights generated on the GPU): the time of one vlo_batch_step against B solo
vlo_llm_step calls, measured in the same process, alternated, with device events after a warm-up.

  (a) decode batches: B in {1, 2, 4, 8, 16} sessions of n = 1 at Lc in {4096, 15519}
  (b) frame-step batches: B in {1, 2, 4, 5} sessions of n = 11 at Lc = 15519 (B >= 2: the 64-row block path)
  (c) a mix: one frame step and five decode rows in one 16-row batch
  (d) --kv fp8: the same grid on an fp8 KV cache

    python tools/probe_batch.py [--kv fp8] [--only a] [--iters 10]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from probe_llm import SHAPES, random_llm_weights_to_engine
from videollm_online_amd.engine import Engine, EngineConfig


def timed(fn, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def case(eng, batch, Lc, ns, iters, tag):
    """sessions at cache length Lc appending ns[b] rows; each timed call is followed by a crop back to Lc (not timed)"""
    H = eng.cfg.hidden_size
    ss = []
    for b in range(len(ns)):
        s = eng.new_session()
        eng.llm_step(s, torch.randn(Lc, H, device="cuda").bfloat16(), want_last=False)
        ss.append(s)
    xs = [torch.randn(n, H, device="cuda").bfloat16() for n in ns]

    def crop():
        torch.cuda.synchronize()
        for s in ss:
            s.crop(Lc)

    def solo():
        for s, x in zip(ss, xs):
            eng.llm_step(s, x, want_last=True)

    def batched():
        batch.step(ss, xs)

    for fn in (solo, batched):                       # warm-up
        fn()
        crop()
    t_solo, t_batch = [], []
    for _ in range(iters):                           # alternated: one solo round, one batched step
        t_solo.append(timed(solo, 1))
        crop()
        t_batch.append(timed(batched, 1))
        crop()
    t_solo.sort()
    t_batch.sort()
    ms_s, ms_b = t_solo[len(t_solo) // 2], t_batch[len(t_batch) // 2]
    alg = eng.weight_bytes + sum(eng.step_algorithmic_bytes(Lc, n) - eng.weight_bytes for n in ns)
    print(f"{tag}: B={len(ns)} n={ns} Lc={Lc}: batch {ms_b:.3f} ms | {len(ns)} solo steps {ms_s:.3f} ms "
          f"(one solo step {ms_s / len(ns):.3f} ms) | batch / one solo {ms_b / (ms_s / len(ns)):.2f}x | "
          f"alg {alg / 1e9:.2f} GB -> {alg / (ms_b * 1e-3) / 1e12:.2f} TB/s", flush=True)
    for s in ss:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--only", default="abc")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bs", default="1,2,4,8,16", help="(a): batch sizes")
    ap.add_argument("--lcs", default="4096,15519", help="(a): cache lengths")
    ap.add_argument("--fbs", default="1,2,4,5", help="(b): batch sizes")
    args = ap.parse_args()
    cfg = EngineConfig(**SHAPES["llama-3-8b"], kv_pool_tokens=16 * 15872 + 4096, kv_dtype=args.kv)
    eng = Engine(cfg)
    random_llm_weights_to_engine(eng, cfg)
    eng.finalize()
    batch = eng.new_batch(16)
    print(f"Llama-3-8B shape, random weights, kv {args.kv}, packed weights {eng.weight_bytes / 1e9:.2f} GB", flush=True)
    if "a" in args.only:
        for Lc in [int(v) for v in args.lcs.split(",")]:
            for B in [int(v) for v in args.bs.split(",")]:
                case(eng, batch, Lc, [1] * B, args.iters, f"(a{'-fp8' if args.kv == 'fp8' else ''}) decode")
    if "b" in args.only:
        for B in [int(v) for v in args.fbs.split(",")]:
            case(eng, batch, 15519, [11] * B, args.iters, f"(b{'-fp8' if args.kv == 'fp8' else ''}) frame")
    if "c" in args.only:
        case(eng, batch, 15519, [11, 1, 1, 1, 1, 1], args.iters, f"(c{'-fp8' if args.kv == 'fp8' else ''}) mix")
    batch.close()
    eng.close()


if __name__ == "__main__":
    main()
