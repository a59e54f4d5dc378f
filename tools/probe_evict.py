"""KV-eviction probe at the true Llama-3-8B shape (random weights generated on the GPU), bf16 KV.

  (a) evict(35, 35 + d) for d in {256, 253} at len in {4096, 15519, 66000}, beside a hipMemcpyAsync device-to-device copy of the same byte
      count (kv_bytes_per_token x tail) timed in the same run: microseconds, GB/s over 2 x bytes (read + write), ratio to the copy.
      The eviction is timed with device events around the one kernel (tails that free no page: the call does not synchronise).
  (b) 1 200 frame steps (n = 11) with and without kv_budget = 4096 (the policy of inference.KvBudget on a bare session): ms per step over
      the last 100 frames.

    python tools/probe_evict.py [--only ab] [--frames 1200]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from probe_llm import SHAPES, random_llm_weights_to_engine
from videollm_online_amd.engine import Engine, EngineConfig
from videollm_online_amd.inference import KvBudget


def fill(eng, s, L, H):
    while s.get_seq_length() < L:
        n = min(4096, L - s.get_seq_length())
        eng.llm_step(s, torch.randn(n, H, device="cuda").bfloat16(), want_last=False)


def part_a(eng, iters):
    cfg = eng.cfg
    H = cfg.hidden_size
    per_tok = 2 * cfg.num_hidden_layers * cfg.num_key_value_heads * eng.head_dim * 2
    for L in (4096, 15519, 66000):
        s = eng.new_session()
        fill(eng, s, L, H)
        for d in (256, 253):
            tail = L - 35 - d
            nbytes = per_tok * tail
            src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            te, tc = [], []
            for it in range(iters + 1):
                f = s.fork(L)
                torch.cuda.synchronize()
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                dst.copy_(src, non_blocking=True)                 # hipMemcpyAsync device to device
                e1.record()
                f.evict(35, 35 + d)
                e2.record()
                torch.cuda.synchronize()
                if it:                                            # the first round warms up
                    tc.append(e0.elapsed_time(e1) * 1e3)
                    te.append(e1.elapsed_time(e2) * 1e3)
                assert f.get_seq_length() == L - d
                f.close()
            te.sort()
            tc.sort()
            ue, uc = te[len(te) // 2], tc[len(tc) // 2]
            print(f"(a) len {L} evict(35, {35 + d}): tail {tail} tokens, {nbytes / 1e6:.1f} MB | evict {ue:.1f} us = {2 * nbytes / ue / 1e3:.0f} GB/s | "
                  f"copy {uc:.1f} us = {2 * nbytes / uc / 1e3:.0f} GB/s | evict / copy {ue / uc:.2f}x", flush=True)
            del src, dst
        s.close()


def part_b(eng, frames):
    H = eng.cfg.hidden_size
    for budget in (None, 4096):
        s = eng.new_session()
        kb = KvBudget(budget, 35, 13) if budget else None
        x0 = torch.randn(35 + 10, H, device="cuda").bfloat16()
        x = torch.randn(11, H, device="cuda").bfloat16()
        ms = []
        for i in range(frames):
            xi = x0 if i == 0 else x
            torch.cuda.synchronize()
            t = time.perf_counter()
            L0 = s.get_seq_length()
            eng.llm_step(s, xi, want_last=False)
            if kb is not None:
                kb.note_step(L0, xi.shape[0])
                kb.enforce(s)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        last = ms[-100:]
        print(f"(b) {frames} frame steps (n = 11), kv_budget {budget}: final length {s.get_seq_length()}, evictions {kb.evictions if kb else 0} | "
              f"last 100 frames: mean {sum(last) / len(last):.3f} ms, median {sorted(last)[len(last) // 2]:.3f} ms, max {max(last):.3f} ms per step (eviction included)", flush=True)
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ab")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1200)
    args = ap.parse_args()
    cfg = EngineConfig(**SHAPES["llama-3-8b"], kv_pool_tokens=2 * 66048 + 4096)
    eng = Engine(cfg)
    random_llm_weights_to_engine(eng, cfg)
    eng.finalize()
    print(f"Llama-3-8B shape, random weights, bf16 KV, packed weights {eng.weight_bytes / 1e9:.2f} GB", flush=True)
    if "a" in args.only:
        part_a(eng, args.iters)
    if "b" in args.only:
        part_b(eng, args.frames)
    eng.close()


if __name__ == "__main__":
    main()
