"""KV-eviction probe at the true Llama-3-8B shape (random weights generated on the GPU), bf16 KV.

  (a) evict(35, 35 + d) for d in {256, 253} at len in {4096, 15519, 66000}, beside a hipMemcpyAsync device-to-device copy of the same byte
      count (kv_bytes_per_token x tail) timed in the same run: microseconds, GB/s over 2 x bytes (read + write), ratio to the copy.
      The eviction is timed with device events around the one kernel (tails that free no page: the call does not synchronise).
  (b) 1 200 frame steps (n = 11) with and without kv_budget = 4096 (the policy of inference.KvBudget on a bare session): ms per step over
      the last 100 frames.

  (c) the ranges mode (vlo_session_evict_ranges) at len in {4096, 15519}: every other one of 46 frame runs of 11 tokens behind a 35-token sink
      (23 ranges, 253 tokens) dropped by ONE evict_ranges call, by the same 23 ranges as single evict calls (highest first, so the coordinates
      hold) and beside a device-to-device copy of the bytes the one call moves; a single range through both entries (median and spread of the
      repeats); and the keys of the one-call and the 23-call eviction against the exact (float64) rotation of the original keys, in bf16 ulps.

    python tools/probe_evict.py [--only abc] [--frames 1200]
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


DECIMATE = [(35 + 22 * i, 46 + 22 * i) for i in range(23)]


def timed(iters, make, *calls):
    """[sorted microseconds of each call]: every round on a fresh fork per call, device events around the call, the first round warms up"""
    out = [[] for _ in calls]
    for it in range(iters + 1):
        for k, call in enumerate(calls):
            f = make()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(f)
            e1.record()
            torch.cuda.synchronize()
            if it:
                out[k].append(e0.elapsed_time(e1) * 1e3)
            if f is not None:
                f.close()
    return [sorted(t) for t in out]


def med(t):
    return t[len(t) // 2]


def key_error(eng, s, L, inv_freq):
    """K of the one-call and of the 23-call eviction against the float64 rotation of the original keys: (max, rms) of the error in bf16 ulps
    of the rotated PAIR's magnitude hypot(k[i], k[i + hd/2]) — what the rotation preserves and every rounding scales with (an element's own
    magnitude can be arbitrarily small where the two terms cancel)"""
    one, seq = s.fork(L), s.fork(L)
    one.evict_ranges(DECIMATE)
    for a, b in reversed(DECIMATE):
        seq.evict(a, b)
    nl = L - 253
    assert one.get_seq_length() == seq.get_seq_length() == nl
    shift = torch.zeros(nl, dtype=torch.float64, device="cuda")          # D(p) of every destination token
    srcpos = torch.arange(nl, device="cuda")
    D = 0
    for j, (a, b) in enumerate(DECIMATE):
        D += b - a
        shift[b - D:] = D
    srcpos = srcpos + shift.long()
    ang = shift[:, None] * inv_freq.double().cuda()[None, :]
    c, sn = torch.cos(ang), torch.sin(ang)
    stats = {"one call": [0.0, 0.0, 0], "23 calls": [0.0, 0.0, 0]}
    h2 = eng.head_dim // 2
    for layer in (0, eng.cfg.num_hidden_layers // 2, eng.cfg.num_hidden_layers - 1):
        for h in range(eng.cfg.num_key_value_heads):
            k0 = s.read_kv(layer, 0, h, 0, L).double()[srcpos]
            exact = torch.cat([k0[:, :h2] * c + k0[:, h2:] * sn, k0[:, h2:] * c - k0[:, :h2] * sn], dim=1)[35:]
            mag = torch.hypot(exact[:, :h2], exact[:, h2:]).clamp_min(1e-30)
            ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7).repeat(1, 2)
            for tag, f in (("one call", one), ("23 calls", seq)):
                err = ((f.read_kv(layer, 0, h, 35, nl).double() - exact).abs() / ulp)
                st = stats[tag]
                st[0], st[1], st[2] = max(st[0], err.max().item()), st[1] + (err ** 2).sum().item(), st[2] + err.numel()
    one.close()
    seq.close()
    return {tag: (mx, (sq / n) ** 0.5) for tag, (mx, sq, n) in stats.items()}


def part_c(eng, iters):
    cfg = eng.cfg
    H = cfg.hidden_size
    per_tok = 2 * cfg.num_hidden_layers * cfg.num_key_value_heads * eng.head_dim * 2
    inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, eng.head_dim, 2, dtype=torch.float32) / eng.head_dim))
    for L in (4096, 15519):
        s = eng.new_session()
        fill(eng, s, L, H)
        moved = L - 253 - 35
        nbytes = per_tok * moved
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def sequential(f):
            for a, b in reversed(DECIMATE):
                f.evict(a, b)
        t_one, t_seq, t_copy = timed(iters, lambda: s.fork(L), lambda f: f.evict_ranges(DECIMATE), sequential, lambda f: dst.copy_(src, non_blocking=True))
        print(f"(c) len {L}, 23 ranges of 11 tokens: {moved} tokens moved, {nbytes / 1e6:.1f} MB | one evict_ranges {med(t_one):.1f} us = "
              f"{2 * nbytes / med(t_one) / 1e3:.0f} GB/s | 23 evict calls {med(t_seq):.1f} us | copy {med(t_copy):.1f} us | 23 calls / one call "
              f"{med(t_seq) / med(t_one):.2f}x | one call / copy {med(t_one) / med(t_copy):.2f}x", flush=True)
        del src, dst
        for d in (256, 253):
            t_new, t_old = timed(iters, lambda: s.fork(L), lambda f: f.evict_ranges([(35, 35 + d)]), lambda f: f.evict(35, 35 + d))
            print(f"(c) len {L}, the single range (35, {35 + d}): evict_ranges {med(t_new):.1f} us [{t_new[0]:.1f} .. {t_new[-1]:.1f}] | "
                  f"evict {med(t_old):.1f} us [{t_old[0]:.1f} .. {t_old[-1]:.1f}] | ratio {med(t_new) / med(t_old):.3f}", flush=True)
        if L == 4096:
            for tag, (mx, rms) in key_error(eng, s, L, inv_freq).items():
                print(f"(c) len {L}, keys after the decimation by {tag} against the exact rotation of the original keys: max {mx:.3f}, rms {rms:.4f} bf16 ulps of the pair magnitude", flush=True)
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
    if "c" in args.only:
        part_c(eng, args.iters)
    eng.close()


if __name__ == "__main__":
    main()
