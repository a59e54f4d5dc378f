#!/usr/bin/env python
"""bench.py — streaming FPS of the videollm-online hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

A "step" is one frame of the synthetic 2 FPS stream pushed through the whole hot path exactly as
demo/cli.py:31-38 drives it: ``input_video_stream(i / fps)`` (SigLIP-L encode + connector) then
``liveinfer()`` (Llama-3-8B frame step over the growing KV, fused sampler, response generation when
triggered).  Weights are seeded random-init at the true shapes and frames are synthetic uint8
384x384 (no checkpoints / videos exist offline) — both resident in HBM before the timed region.
Random weights make the speak/silent decision arbitrary, so the speech schedule is fixed
("scheduled" mode): the sampler still runs every frame, a 16-token response is
generated every 10th frame plus one for the t=0 user query; ``--mode silent`` and ``--mode free``
are available.  N > 1 runs one independent stream per GPU (replicas, weak scaling: streams are
independent, there is no exchange step) under torchrun, barrier + max-over-ranks timing — that is
``value``.  With ``--full`` the same invocation then measures ONE stream with the Llama tensor-parallel over the N
GPUs (``--tp``) in child processes, once with RCCL all-reduces (``"tp"``) and once with the one-shot
peer-to-peer all-reduce over xGMI (``"tp_p2p"``); a failure there is recorded, never fatal.

The K timed steps are the LAST K frames of the configuration's stream (1200 frames = 10 min @ 2 FPS for the headline
configuration): the first 1200 - K frames are streamed un-timed through the same engine steps on the same session (the
pre-roll), frames encoded ahead are dropped at the boundary, and the clock runs over frames 1200-K .. 1199 at the context
the metric is defined on (K = 20: KV 15.5 k -> 15.8 k tokens).  ``full_stream`` reports all 1200 frames.
``--weight-dtype fp8`` streams the Llama projections as e4m3 + per-channel scales (BASELINE.json configs[4]'s LLM half).

Prints ONE JSON line (rank 0).  A plain run does only what that line's headline needs: set-up, warm-up, the pre-roll, the
K timed steps, ``--dump-outputs`` when asked — the contract keys (``metric``, ``value``, ``unit``, ``higher_is_better``,
``dtype``, ``ms_per_step``) and what those steps yield for free (latency percentiles, ``full_stream``, ``first_frame_ms``,
``stream_hbm_roofline``).  ``--full`` adds every measurement that takes a run of its own, after the timed steps and the
dump: ``roofline`` (dominant kernel = the gate/up weight-streaming GEMV, timed live with HIP events on its own stream, net
of a calibrated empty bracket), ``encode_stage``, ``live_feed``, ``prefill``, ``cpu_baseline`` (the CPU oracle on a bounded
sample of the same workload, rank 0, N=1 only) and, for N > 1, the tensor-parallel legs and their exchange latency.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from videollm_online_amd.synthetic import (LLM_SHAPES, VIT_SHAPE, VIT_SHAPES, vit_gflop_per_frame, gpu_random_weights, gpu_synthetic_frames,  # noqa: E402
                                           stream_tokens)

HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_PEAK_TFLOPS = 2500.0       # dense bf16/fp16 MFMA peak (same guide)
VIT_GFLOP_PER_FRAME = 384.4     # ViT 384 + connector 0.42


_T0 = time.time()


def log(msg):
    if os.environ.get("RANK", "0") == "0":
        print(f"[bench +{time.time() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def usable_cores():
    """Host cores this process may actually use: min(affinity mask, cgroup CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def reduce_elapsed_max(dist, elapsed, device="cuda"):
    """max-over-ranks wall time: the job is as slow as its slowest replica."""
    import torch
    if dist is None:
        return elapsed
    t = torch.tensor([elapsed], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


PREFILL_PROBE_TOKENS = 4096


def rocprof_cross_check(bytes_per_launch, profiles_dir=None):
    """The dominant kernel's kernel-only average from the builder's committed `rocprofv3 --kernel-trace --stats` run of the bench command
    (the newest profiles/rN_kernel_stats_bench200*.csv; Llama-3-8B, bf16: gemv16_kernel<16, 8, XSRC_NORM, EPI_SWIGLU, bf16>), as extra keys
    of the `roofline` object: a STORED cross-check beside the live HIP-event figure, labelled as such.  {} when there is no such file."""
    import csv
    import glob
    try:
        d = profiles_dir or os.path.join(ROOT, "profiles")
        path = sorted(glob.glob(os.path.join(d, "r[0-9]*_kernel_stats_bench200*.csv")),
                      key=lambda q: (int(os.path.basename(q)[1:].split("_")[0]), q))[-1]
        row = next(r for r in csv.DictReader(open(path)) if r["kernel"].startswith("void gemv16_kernel<16, 8, 1, 3, 0"))
        us = float(row["avg_us"])
        return {"rocprof_avg_launch_us": us, "frac_rocprof": round(bytes_per_launch / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                "rocprof_source": f"profiles/{os.path.basename(path)} ({row['calls']} launches; stored result of a rocprofv3 --kernel-trace --stats run, "
                                  "NOT measured in this run)"}
    except Exception:
        return {}


def stats_kernel_names(profiles_dir=None):
    """Kernel names of the newest committed rocprofv3 stats of the bench command (None when there is no such file)."""
    import csv
    import glob
    try:
        d = profiles_dir or os.path.join(ROOT, "profiles")
        path = sorted(glob.glob(os.path.join(d, "r[0-9]*_kernel_stats_bench200*.csv")),
                      key=lambda q: (int(os.path.basename(q)[1:].split("_")[0]), q))[-1]
        return {r["kernel"] for r in csv.DictReader(open(path))}
    except Exception:
        return None


def roofline(args, n_launch, prof_ms, bytes_per_launch, empty_us):
    """--full: the `roofline` object — the dominant kernel (gate/up GEMV) from the HIP-event brackets the engine kept around its launches in the
    timed region, net of ``empty_us`` (a calibrated empty bracket), beside the stored rocprofv3 / PMC figures under profiles/."""
    avg_ms = prof_ms / max(n_launch, 1)
    # a HIP-event bracket reads the kernel's duration plus the fixed cost of the bracket itself (what an EMPTY
    # bracket reads on the same stream); net of that it agrees with rocprofv3's kernel-only average (profiles/)
    net_ms = max(avg_ms - empty_us * 1e-3, 1e-6)
    achieved = bytes_per_launch / (net_ms * 1e-3) / 1e9 if n_launch else None
    # HBM traffic of the dominant kernel comes from PMC counters, which cannot be read from inside this process: it is the
    # value of the builder's own `rocprofv3 --pmc` run of this command (stored under profiles/, see `traffic_source`)
    traffic = traffic_source = None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_gemv_gate_up.json")
    if os.path.exists(pmc_path):
        try:
            pmc = json.load(open(pmc_path))
            # a stored counter figure is evidence for THIS code only if it names the kernel this code runs: the kernel of the newest committed
            # rocprofv3 stats of the bench command (round 5's line quoted a round-3 file of a kernel with another template signature)
            names = stats_kernel_names()
            if names is not None and pmc.get("kernel") not in names:
                traffic_source = (f"refused: profiles/pmc_gemv_gate_up.json is about `{pmc.get('kernel')}`, which is not a kernel of the newest "
                                  "profiles/rN_kernel_stats_bench200*.csv — re-run the two PMC passes (tools/pmc_hbm_json.py)")
            else:
                traffic = pmc.get("hbm_bytes_per_launch")
                traffic_source = (f"profiles/pmc_gemv_gate_up.json ({pmc.get('kernel')}, {pmc.get('launches')} launches, {pmc.get('round', 'round ?')}; stored result of a "
                                  "rocprofv3 --pmc run, NOT measured in this run)")
        except Exception:
            traffic = None
    rocprof = rocprof_cross_check(bytes_per_launch) if args.model == "llama-3-8b" and args.weight_dtype == "bf16" else {}
    return {"bound": "hbm", "kernel": "gemv16_kernel<KF,EPI_SWIGLU> (gate/up projection + SwiGLU)" + (", fp8 weight image" if args.weight_dtype == "fp8" else ""),
            "achieved": round(achieved, 1) if achieved else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
            "traffic": traffic if args.weight_dtype == "bf16" else None, "traffic_source": traffic_source if args.weight_dtype == "bf16" else None,
            "launches_timed": n_launch, "avg_launch_us": round(net_ms * 1e3, 2), "avg_bracket_us_raw": round(avg_ms * 1e3, 2),
            "empty_bracket_us": round(empty_us, 2), "bytes_per_launch": bytes_per_launch, **rocprof}


def aggregate_fps(frames_per_rank, world, elapsed_max):
    """whole-job frames/s: every rank streams ``frames_per_rank`` frames (weak scaling)."""
    return frames_per_rank * world / elapsed_max


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, li, eng, cfg, seed=0):
    """--dump-outputs: what the LAST timed step handed its caller, as .npy files (float32 / float64) under ``out_dir``, so that
    two builds can be compared output for output on identical inputs:
      last_step_sampler.npy   float64 [4]: video time, token the session went on with, token the sampler chose, and the
                              sampler's bf16-rounded probability of the frame-interval token
      last_step_response.npy  float64 [n]: the greedy response ids of that step (EOS included; empty when it stayed silent)
      last_step_kv.npy        float32 [L, 2, n_kv_heads, T, head_dim]: K and V of the positions that step appended to the
                              session (the frame step and its response), every layer
      last_step_kv_pos.npy    float64 [T]: the session positions of those rows (a seeded sample of them beyond 64 MB in all)"""
    import numpy as np
    import torch
    from videollm_online_amd.trace import FRAME, RESPONSE
    os.makedirs(out_dir, exist_ok=True)
    frame = next(e for e in reversed(li.trace) if e.kind == FRAME)
    resp = li.trace[-1] if li.trace[-1].kind == RESPONSE and li.trace[-1].video_time == frame.video_time else None
    p = float(li._p_dev.item())
    np.save(os.path.join(out_dir, "last_step_sampler.npy"), np.array([frame.video_time, frame.token, frame.sampled, p], dtype=np.float64))
    np.save(os.path.join(out_dir, "last_step_response.npy"), np.array(resp.output_ids if resp else [], dtype=np.float64))
    # the frame step is the logged step that left the session at the frame event's length; the last step appended [Lc, end)
    end = len(li.past_key_values)
    lc = next(Lc for Lc, n in reversed(li.step_log) if Lc + n == frame.kv_len)
    hd = cfg.hidden_size // cfg.num_attention_heads
    L, nkv = cfg.num_hidden_layers, cfg.num_key_value_heads
    pos = np.arange(lc, end)
    cap = DUMP_MAX_BYTES // (L * 2 * nkv * hd * 4) - 1
    if len(pos) > cap:
        pos = np.sort(np.random.default_rng(seed).choice(pos, cap, replace=False))
    kv = torch.empty(L, 2, nkv, len(pos), hd, dtype=torch.float32, device=eng.device)
    idx = torch.as_tensor(pos - lc, device=eng.device)
    for layer in range(L):
        for which in range(2):
            for h in range(nkv):
                kv[layer, which, h] = li.past_key_values.read_kv(layer, which, h, lc, end).float()[idx]
    np.save(os.path.join(out_dir, "last_step_kv.npy"), kv.cpu().numpy())
    np.save(os.path.join(out_dir, "last_step_kv_pos.npy"), pos.astype(np.float64))
    log(f"dump: last timed step (t = {frame.video_time}s) -> {out_dir}: sampler, {len(resp.output_ids) if resp else 0} response ids, "
        f"KV rows {lc}..{end - 1} ({len(pos)} kept)")


def make_schedule(mode):
    if mode == "scheduled":
        return lambda i: (i % 10 == 9, 16)
    if mode == "silent":
        return lambda i: (False, 16)
    return None


def cpu_baseline(model_name, frames_u8_cpu, toks, mode, sample_frames, budget_s=25.0, windows=(), window_13k_frames=0):
    """The CPU oracle (a port of the reference's CPU/sdpa path: bf16 Llama, fp32 SigLIP) on the first
    ``sample_frames`` frames of the same stream.  Timing-equivalent weights: one random layer aliased
    across all layers (values do not affect CPU time, and 15 GB of distinct random numbers would take
    minutes to generate)."""
    import torch
    from oracle import vlo_oracle as O
    spec = O.LLM_SPECS[model_name]
    vspec = O.VIT_SPECS["siglip-l16-384"]
    cores = usable_cores()
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(0)

    def blk(n, k, std, dtype):       # random block tiled along rows: values do not affect CPU time
        base = (torch.randn(min(n, 512), k, generator=g) * std).to(dtype)
        return base.repeat((n + base.shape[0] - 1) // base.shape[0], 1)[:n].contiguous()

    H, I, V, hd = spec.hidden_size, spec.intermediate_size, spec.vocab_size, spec.head_dim
    bf = torch.bfloat16
    layer = {"input_layernorm.weight": torch.ones(H, dtype=bf), "post_attention_layernorm.weight": torch.ones(H, dtype=bf),
             "self_attn.q_proj.weight": blk(spec.num_heads * hd, H, H ** -0.5, bf),
             "self_attn.k_proj.weight": blk(spec.num_kv_heads * hd, H, H ** -0.5, bf),
             "self_attn.v_proj.weight": blk(spec.num_kv_heads * hd, H, H ** -0.5, bf),
             "self_attn.o_proj.weight": blk(H, spec.num_heads * hd, H ** -0.5, bf),
             "mlp.gate_proj.weight": blk(I, H, H ** -0.5, bf), "mlp.up_proj.weight": blk(I, H, H ** -0.5, bf),
             "mlp.down_proj.weight": blk(H, I, I ** -0.5, bf)}
    w = {f"model.layers.{i}.{k}": v for i in range(spec.num_layers) for k, v in layer.items()}
    w["model.embed_tokens.weight"] = blk(V, H, 1.0, bf)
    w["lm_head.weight"] = blk(V, H, 2 * H ** -0.5, bf)
    w["model.norm.weight"] = torch.ones(H, dtype=bf)
    w["connector.0.weight"] = blk(H, spec.vision_hidden_size, spec.vision_hidden_size ** -0.5, bf)
    w["connector.0.bias"] = torch.zeros(H, dtype=bf)
    w["connector.2.weight"] = blk(H, H, H ** -0.5, bf)
    w["connector.2.bias"] = torch.zeros(H, dtype=bf)
    v1 = O.init_vit_weights(O.VitSpec(num_layers=1), seed=1)
    vw = dict(v1)
    for i in range(1, vspec.num_layers):
        for k, v in v1.items():
            if k.startswith("vision.encoder.layers.0."):
                vw[k.replace("vision.encoder.layers.0.", f"vision.encoder.layers.{i}.")] = v
    llm = O.LlamaOracle(spec, w, torch.bfloat16)
    otoks = O.StreamTokens(toks.start_ids, toks.stream_prompt_ids, toks.stream_generation_ids, toks.eos_token_id,
                           toks.interval_id, dict(toks.query_ids))
    sched = make_schedule(mode)                 # the GPU line's schedule: 16-token responses
    win = []
    window_13k = None
    kv_blk = None

    def prefilled(Lc):
        # a KV cache of Lc tokens: ONE random block aliased across layers and between K and V (values do not affect CPU time; the
        # oracle's cache grows by torch.cat, never in place, so the shared source stays intact)
        nonlocal kv_blk
        if kv_blk is None or kv_blk.shape[1] < Lc:
            kv_blk = torch.randn(spec.num_kv_heads, Lc, hd, generator=g).to(bf)
        cache = llm.new_cache()
        for i in range(spec.num_layers):
            cache.k[i] = kv_blk[:, :Lc]
            cache.v[i] = kv_blk[:, :Lc]
        return cache

    def window(Lc, nframes):
        lw = O.LiveInferOracle(llm, vw, vspec, otoks, frame_fps=2, schedule=sched, max_new=16)
        lw.load_video(frames_u8_cpu[:nframes])
        lw.past_key_values, lw.last_ids = prefilled(Lc), [toks.interval_id]
        t0 = time.time()
        for i in range(nframes):
            lw.input_video_stream(i / 2)
            lw()
        dt = time.time() - t0
        log(f"cpu_baseline window at Lc={Lc}: {nframes} frames, {nframes / dt:.3f} frames/s")
        return {"kv_tokens_at_start": Lc, "kv_tokens_at_end": len(lw.past_key_values), "frames": nframes, "frames_per_s": round(nframes / dt, 4)}

    if window_13k_frames > 0:
        # the context the GPU line is timed at (configs[1]'s last frames): `window_13k_frames` un-answered frame steps (encode + the
        # 11-token Llama step over ~13.2 k cached tokens) inside the baseline's time budget — the figure to read next to `value`
        window_13k = window(13245, window_13k_frames)
        window_13k["note"] = ("frame steps only (SigLIP-L encode + an 11-token Llama step; no response falls inside the window) at the cache length the "
                              "GPU line's timed frames start from; KV pre-filled with random values")
    for Lc in windows:
        # 10-frame windows deep in the stream, the KV cache pre-filled with random keys / values (their values
        # do not affect CPU time); the window's last frame is answered as the schedule says.  Reported as windows, never extrapolated.
        win.append(window(Lc, 10))
    li = O.LiveInferOracle(llm, vw, vspec, otoks, frame_fps=2, schedule=sched, max_new=16)
    li.load_video(frames_u8_cpu)
    li.input_query_stream("Please narrate the video in real time.", video_time=0.0)
    t0 = time.time()
    done = 0
    for i in range(sample_frames):
        li.input_video_stream(i / 2)
        li()
        done += 1
        log(f"cpu_baseline: frame {i} done at {time.time() - t0:.1f}s")
        if time.time() - t0 > budget_s:
            break
    dt = time.time() - t0
    sample_frames = done
    return {"value": round(sample_frames / dt, 4), "unit": "frames/s", "cores": cores, "kind": "port",
            **({"window_13k": window_13k} if window_13k else {}),
            **({"windows": win, "windows_note": "10-frame windows of the same stream with the KV cache pre-filled (random) to the given length; "
                                                "each window's last frame is answered with a 16-token response"} if win else {}),
            "port_vs_reference": "profiles/r3_port_vs_reference_cpu.txt: the port runs at 0.85-1.07x the time of the reference's own classes "
                                 "(LiveLlamaForCausalLM, _siglip_vision_encode) on identical inputs in the build container",
            "sample": f"first {sample_frames} frames of the same stream with the same schedule (t=0 query and every 10th frame answered with a "
                      f"16-token response), i.e. at cache lengths Lc <= {len(li.past_key_values)} — NOT at the ~13-15.7 k-token context the GPU "
                      f"line is timed at (the CPU path only gets slower there: HF re-concatenates the whole KV every step); "
                      f"oracle = torch-CPU port of the reference CPU/sdpa path (bf16 Llama, fp32 SigLIP-L); "
                      f"one random layer's weights aliased across layers (timing-equivalent)"}


def run_tp_leg(args, rank, world, local, allreduce="rccl", port_offset=17):
    """Spawn `bench.py --tp --tp-allreduce <allreduce>` as a child of every rank (same RANK / LOCAL_RANK / WORLD_SIZE,
    rendezvous on MASTER_PORT + port_offset), wait with a deadline, kill the child's process group on timeout.  Rank 0
    returns the child's headline numbers."""
    import signal
    import subprocess
    env = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC") and k not in ("GROUP_RANK", "ROLE_RANK")}
    env.update(RANK=str(rank), LOCAL_RANK=str(local), WORLD_SIZE=str(world), MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"),
               MASTER_PORT=str(int(os.environ.get("MASTER_PORT", "29500")) + port_offset), VLO_BENCH_TP_LEG="0")
    steps = max(20, min(args.steps, args.tp_leg_steps))
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--steps", str(steps), "--warmup", "10", "--tp",
           "--tp-allreduce", allreduce, "--full", "--no-cpu-baseline", "--model", args.model, "--mode", args.mode, "--fps", str(args.fps),
           "--prefetch-frames", str(args.prefetch_frames), "--tp-vit", getattr(args, "tp_vit", "frame-parallel"),
           "--vit", getattr(args, "vit", "siglip-l16-384"), "--weight-dtype", getattr(args, "weight_dtype", "bf16")]
    log(f"tp leg: {' '.join(cmd[1:])}")
    t0 = time.time()
    try:
        child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    except Exception as ex:
        return {"error": f"spawn failed: {ex!r}"}
    try:
        so, se = child.communicate(timeout=args.tp_leg_timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(child.pid, signal.SIGKILL)          # the session we started, nothing else
        except Exception:
            pass
        so, se = child.communicate()
        return {"error": f"timeout after {args.tp_leg_timeout:.0f}s", "stderr_tail": (se or "")[-400:]}
    if rank != 0:
        return None
    line = next((l for l in reversed((so or "").splitlines()) if l.startswith("{")), None)
    if child.returncode != 0 or line is None:
        return {"error": f"child exit code {child.returncode}", "stderr_tail": (se or "")[-400:]}
    d = json.loads(line)
    keep = ("value", "unit", "ms_per_step", "p50_frame_latency_ms", "p95_frame_latency_ms", "steps", "scaling", "full_stream")
    r = {k: d.get(k) for k in keep}
    r["rccl_comm"] = d["config"].get("rccl_comm")
    how = ("RCCL all-reduce x2 per layer + logits all-gather" if allreduce == "rccl" else
           "one-shot peer-to-peer all-reduce over xGMI fused with residual add + RMSNorm, x2 per layer, + p2p logits gather; no RCCL on the step path")
    r.update(parallelism=d["config"]["parallelism"], stream_hbm_roofline=d.get("stream_hbm_roofline"), wall_s=round(time.time() - t0, 1),
             exchange=d["config"].get("tp_exchange"),
             note=f"ONE stream, Llama tensor-parallel over the same GPUs ({how}), ViT "
                  f"{'frame-parallel (one RCCL all-gather of the frame embeddings per batch)' if getattr(args, 'tp_vit', '') == 'frame-parallel' else 'replicated'}; measured by "
                  f"`bench.py --tp --tp-allreduce {allreduce}` in child processes")
    return r


def self_launch(n):
    """Re-run this command line under torch.distributed.run with n ranks on this node (rendezvous on 127.0.0.1, a free port);
    the ranks' output passes through (rank 0 prints the JSON line).  Returns the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log(f"--gpus {n} without a launcher: starting {n} ranks: {' '.join(cmd[1:])}")
    return subprocess.call(cmd)


def dry_run(args, rank, world, dist, backend):
    """VLO_BENCH_DRY_RUN=1 (tests/test_multiproc_cpu.py): everything of an N-rank run EXCEPT the engine — launch, rendezvous, the
    barrier + synchronize bracket, max-over-ranks timing, whole-job aggregation, rank 0's JSON line — with a host sleep standing in
    for the frame.  Not a measurement: `value` is null and the line says so."""
    K = args.steps
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(K):
        time.sleep(1e-3 * (rank + 1))              # the last rank is the slow replica
    if dist is not None:
        dist.barrier()
    elapsed = reduce_elapsed_max(dist, time.perf_counter() - t0, device="cuda" if backend == "nccl" else "cpu")
    out = None
    if rank == 0:
        out = {"metric": "launch-path rehearsal (no engine)", "value": None, "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": args.warmup,
               "ms_per_step": round(elapsed / K * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none",
               "data": "none", "dry_run": True, "stand_in_frames_per_s": round(aggregate_fps(K, world, elapsed), 3),
               "config": {"workload": "VLO_BENCH_DRY_RUN=1: a host sleep per step instead of the hot path", "parallelism": f"replicas{world}"}}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="llama-3-8b", choices=list(LLM_SHAPES))
    ap.add_argument("--mode", default="scheduled", choices=["scheduled", "silent", "free"])
    ap.add_argument("--fps", type=float, default=2.0)
    ap.add_argument("--stream-frames", type=int, default=0,
                    help="length of the synthetic stream; default = the configuration BASELINE.json's metric is quoted on "
                         "(10 min of video: 600 s x fps frames for llama-3-8b; 30 s for tinyllama-1.1b, configs[0]). "
                         "The K timed steps are the LAST K frames of this stream; the frames before them are pre-rolled "
                         "un-timed through the same engine steps on the same session, so the timed region sits at the "
                         "10-minute context the metric is defined on")
    ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="storage of the streamed Llama projections; fp8 = e4m3 + per-channel scales (BASELINE.json configs[4]); the headline "
                         "metric is quoted on bf16")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps (and --dump-outputs), also run every secondary measurement: the dominant kernel's `roofline`, "
                         "`encode_stage`, the `live_feed` re-runs, the `prefill` probe, the `cpu_baseline`, and for N > 1 the tensor-parallel legs "
                         "and exchange latency.  Off by default: a plain run measures the headline figure only")
    ap.add_argument("--no-prefetch", action="store_true")
    ap.add_argument("--prefetch-frames", type=int, default=56,
                    help="frames encoded ahead per batched ViT call while the Llama steps run (the reference batches pending frames the same way, "
                         "demo/inference.py:105-106).  56 frames = 32256 token rows = 126 row tiles of 256: every GEMM of the tower is a whole "
                         "number of 256-CU rounds within 2 %% (504 / 1512 / 2016 tiles); 28 frames give 252 / 756 / 1008")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prefill-probe", action="store_true", help="skip the 4096-token teacher-forced block timed after the stream (`prefill`)")
    ap.add_argument("--no-live-feed", action="store_true", help="skip the two no-look-ahead re-runs of the timed frames (`live_feed`)")
    ap.add_argument("--cpu-sample-frames", type=int, default=20)
    ap.add_argument("--cpu-budget-s", type=float, default=12.0, help="time budget of the CPU baseline's from-the-start sample (its frame loop stops once it is spent)")
    ap.add_argument("--cpu-window-13k-frames", type=int, default=3, help="`cpu_baseline.window_13k`: this many un-answered frame steps of the CPU path at 13 245 "
                    "cached tokens (the context the GPU line is timed at), ~4.5 s per frame on 16 cores; 0 = skip")
    ap.add_argument("--cpu-windows", default="", help="comma-separated cache lengths (e.g. 1024,4096,13312): the CPU baseline additionally times "
                                                      "10-frame windows with the KV cache pre-filled to these lengths (BASELINE.md section 4); "
                                                      "~15-40 s of CPU time each at the 8B size, off by default")
    ap.add_argument("--prof-stride", type=int, default=8)
    ap.add_argument("--tp", action="store_true",
                    help="N > 1: ONE stream, Llama tensor-parallel over the N GPUs (RCCL all-reduce), strong scaling; "
                         "default is one independent stream per GPU (replicas, weak scaling)")
    ap.add_argument("--tp-allreduce", default="rccl", choices=["rccl", "p2p"],
                    help="--tp exchanges: RCCL all-reduce / all-gather, or the one-shot peer-to-peer all-reduce over xGMI fused "
                         "with the residual add + RMSNorm (csrc/tp.hip, no RCCL)")
    ap.add_argument("--vit", default="siglip-l16-384", choices=sorted(VIT_SHAPES),
                    help="vision tower (BASELINE.json's metric is quoted on siglip-l16-384; configs[4] names siglip-so400m14-384)")
    ap.add_argument("--tp-vit", default="frame-parallel", choices=["frame-parallel", "replicated"],
                    help="--tp over RCCL: rank r encodes frames r, r + N, ... of a pending batch and one all-gather distributes the "
                         "[10, H] frame embeddings (north_star), or every rank encodes every frame")
    ap.add_argument("--no-tp-leg", action="store_true",
                    help="N > 1: skip the extra tensor-parallel measurement (run in child processes after the replica run)")
    ap.add_argument("--tp-leg-steps", type=int, default=300)
    ap.add_argument("--tp-leg-timeout", type=float, default=200.0, help="deadline of EACH tensor-parallel child leg (rccl, p2p)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last timed step computed (sampler decision, response ids, the KV rows it "
                         "appended) as DIR/<name>.npy, rank 0; single-engine runs only (not --tp)")
    args = ap.parse_args()

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.dump_outputs and args.tp:
        raise SystemExit("--dump-outputs reads the session of one engine: not available with --tp")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU), so that an N-GPU line can
        # never be a silent 1-GPU run
        raise SystemExit(self_launch(args.gpus))
    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU (or drop the launcher: bench.py starts its own ranks)")
    if os.environ.get("VLO_BENCH_BACKEND", "nccl") == "nccl" and torch.cuda.device_count() < args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} GPU(s) are visible")
    # VLO_BENCH_BACKEND=gloo lets the multi-process path be exercised on a box with fewer GPUs than ranks
    backend = os.environ.get("VLO_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    elif os.environ.get("VLO_BENCH_DRY_RUN") != "1":
        raise SystemExit("no GPU visible: the engine has no CPU path")
    dist = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    if os.environ.get("VLO_BENCH_DRY_RUN") == "1":
        return dry_run(args, rank, world, dist, backend)
    from videollm_online_amd.engine import Engine, EngineConfig, TpGroup
    from videollm_online_amd.inference import LiveInfer
    from videollm_online_amd.modeling_live import LiveModel

    K, Wm = args.steps, args.warmup
    shape = LLM_SHAPES[args.model]
    total = args.stream_frames or int(round((30 if args.model == "tinyllama-1.1b" else 600) * args.fps))
    total = max(total, K)
    preroll = total - K                       # frames streamed un-timed before the K timed ones (0 when --steps covers the stream)
    n_frames = max(total, Wm) + 2
    # KV: start prompt + 11 tokens per frame + responses (query + "]\nAssistant:" + 16 tokens, every 10th frame)
    kv_tokens = 64 + 11 * n_frames + (n_frames // 10 + 2) * 24 + 4096 + PREFILL_PROBE_TOKENS + 512
    vit_shape = VIT_SHAPES[args.vit]
    vit_gflop = VIT_GFLOP_PER_FRAME if args.vit == "siglip-l16-384" else vit_gflop_per_frame(vit_shape, shape["hidden_size"])
    cfg = EngineConfig(**shape, vision_hidden_size=vit_shape["hidden_size"], vit=vit_shape, kv_pool_tokens=kv_tokens, weight_dtype=args.weight_dtype,
                       prefill_act_dtype="fp8" if args.weight_dtype == "fp8" else "bf16")       # (only the `prefill` probe below takes that path)
    log(f"building engine ({args.model} + {args.vit}), kv pool {kv_tokens} tokens")
    tp = args.tp and world > 1
    if tp:
        # every rank builds the SAME full random weights (same seed) and keeps its shard; the RCCL communicator is
        # bootstrapped from rank 0's unique id
        if args.tp_allreduce == "p2p":
            def gather_handles(mine):          # every rank's 64-byte mailbox handle, in rank order
                out = [None] * world
                dist.all_gather_object(out, mine)
                return out
            uid = [TpGroup.unique_id() if rank == 0 and args.tp_vit == "frame-parallel" else None]
            dist.broadcast_object_list(uid, src=0)      # frame-parallel tower: RCCL carries ONLY the all-gather of the frame embeddings
            eng = TpGroup(cfg, world, device=local, rank=rank, allreduce="p2p", handle_allgather=gather_handles, unique_id=uid[0],
                          frame_parallel=args.tp_vit == "frame-parallel")
        else:
            uid = [TpGroup.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            eng = TpGroup(cfg, world, device=local, rank=rank, unique_id=uid[0], frame_parallel=args.tp_vit == "frame-parallel")
        gpu_random_weights(eng, cfg, seed=0)
    else:
        eng = Engine(cfg, local)
        gpu_random_weights(eng, cfg, seed=rank)
    eng.finalize()
    torch.cuda.synchronize()
    log(f"engine ready, {eng.weight_bytes / 1e9:.2f} GB packed weights")
    toks = stream_tokens(cfg.vocab_size)
    model = LiveModel(eng, eos_token_id=toks.eos_token_id, frame_token_interval_id=toks.interval_id)
    frames = gpu_synthetic_frames(n_frames, seed=1234 + (0 if tp else rank))
    # experiment switch (not a default): the Llama steps on a HIGH-priority stream, the encoder on a normal one
    if os.environ.get("VLO_BENCH_HIPRIO") == "1":
        hi = torch.cuda.Stream(priority=-1)
        hi.wait_stream(torch.cuda.current_stream())
        torch.cuda.set_stream(hi)
    li = LiveInfer(model, tokens=toks, frame_fps=args.fps, prefetch=not args.no_prefetch, prefetch_frames=args.prefetch_frames,
                   schedule=make_schedule(args.mode), record=1 << 20)

    def begin_stream():
        li.reset()
        li.load_video(frames)
        li.input_query_stream("Please narrate the video in real time.", video_time=0.0)   # demo/cli.py:23

    def run(lo, hi):
        """frames [lo, hi) of the current stream, bracketed by synchronize + barrier on both sides (demo/cli.py:31-38 loop)"""
        costs = []
        li.drop_prefetched()                  # every frame of [lo, hi) is encoded inside this bracket
        log0 = li.steps_total
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t_start = time.perf_counter()
        for i in range(lo, hi):
            t0 = time.perf_counter()
            li.input_video_stream(i / args.fps)
            li()
            costs.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        elapsed = time.perf_counter() - t_start
        steps = list(li.step_log)[-(li.steps_total - log0):] if li.steps_total > log0 else []
        # algorithmic bytes of every Llama step actually executed
        alg_bytes = sum(eng.step_algorithmic_bytes(Lc, n) for Lc, n in steps)
        return elapsed, costs, alg_bytes, len(steps)

    log(f"frames ready; warmup {Wm} frames")
    begin_stream()
    run(0, Wm)                                         # warmup on a throw-away stream
    begin_stream()
    pre = None
    if preroll:
        log(f"pre-roll: frames 0..{preroll - 1} of the {total}-frame stream (un-timed for `value`; real engine steps)")
        pre = run(0, preroll)
        log(f"pre-roll done: {pre[0]:.2f}s, KV at {len(li.past_key_values)} tokens")
    kv_start = len(li.past_key_values) if li.past_key_values else 0
    log(f"timing {K} frames (frames {preroll}..{total - 1})")
    # session state at the start of the timed region: the live-feed legs below re-run the SAME frames from the SAME context
    snap = dict(last_ids=list(li.last_ids), last_frame_idx=li.last_frame_idx, video_time=li.video_time, frames_done=li._frames_done)
    # THE timed region runs the pipeline BASELINE.json's north_star names: encode of frame t+1 on the encode stream while the Llama step of frame t
    # runs (one frame of look-ahead — what a live camera feed allows).  The pre-roll above batched `--prefetch-frames` frames per encoder call
    # (un-timed; a recorded file allows that) — that form is re-timed below as `recorded_file_lookahead`.
    batch_pf = li.prefetch_frames
    if li.prefetch and preroll:
        li.prefetch_frames = 1
    eng.profile_enable(args.prof_stride)
    elapsed, costs, alg_bytes, llm_steps = run(preroll, total)
    log(f"timed region done: {elapsed:.3f}s -> {K / elapsed:.1f} frames/s on this rank")
    prof_eng = eng.engines[0] if tp else eng
    n_launch, prof_ms, bytes_per_launch = prof_eng.profile_read()
    eng.profile_enable(0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, li, eng, cfg)
    # From here to the result line: measurements with runs of their own, --full only.  (The HIP-event brackets around the dominant kernel stay on in the
    # timed region of every run — they are part of the timed steps as the metric has always been taken; only reading them out as `roofline` is --full.)
    empty_us = prof_eng.profile_calibrate() if args.full else None
    # encode stage in isolation (HIP events on its own stream): ms/frame and fraction of the dense fp16 MFMA peak
    vit_ms = vit1_ms = None
    if rank == 0 and args.full:
        B = max(1, batch_pf)
        enc = torch.cuda.Stream()
        with torch.cuda.stream(enc):
            for _ in range(2):
                eng.visual_embed(frames[:B], stream=enc)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(enc)
            for _ in range(8):
                eng.visual_embed(frames[:B], stream=enc)
            e1.record(enc)
            e2 = torch.cuda.Event(enable_timing=True)
            for _ in range(2):
                eng.visual_embed(frames[:1], stream=enc)
            e1b = torch.cuda.Event(enable_timing=True)
            e1b.record(enc)
            for _ in range(16):
                eng.visual_embed(frames[:1], stream=enc)
            e2.record(enc)
        enc.synchronize()
        vit_ms = e0.elapsed_time(e1) / 8 / B
        vit1_ms = e1b.elapsed_time(e2) / 16            # ONE frame per call: the encoder as the timed pipeline (and the reference's loop) runs it
    final_len = len(li.past_key_values)
    # live feed: the same K frames at the same context WITHOUT look-ahead.  `value` encodes frames in batches of
    # `prefetch_frames` ahead of the Llama steps — legitimate for a recorded video (the reference's demo loads the whole file,
    # demo/inference.py:111-115) but prefetch_frames / fps seconds of look-ahead a live camera does not have.  Leg 1: no look-ahead
    # at all (frame t is encoded when it arrives, then its step runs: the encoder sits on the critical path of every frame).
    # Leg 2: one frame of look-ahead (frame t+1 encoded on the encode stream while the step of frame t runs).
    live_feed = None
    if args.full and not tp and kv_start > 0 and not args.no_live_feed:
        live_feed = {}
        saved = (li.prefetch, li.prefetch_frames)
        legs = (("no_lookahead", (False, 1, False)), ("recorded_file_lookahead", (True, batch_pf, False)), ("real_greedy_path", (True, 1, True)))
        for name, (pf, pfn, real) in legs:
            li.past_key_values.crop(kv_start)
            li.last_ids, li.last_frame_idx, li.video_time, li._frames_done = list(snap["last_ids"]), snap["last_frame_idx"], snap["video_time"], snap["frames_done"]
            li.query_queue.clear(); li.frame_embeds_queue.clear()
            li.prefetch, li.prefetch_frames, li.real_greedy = pf, pfn, real
            el, cs, _, st_n = run(preroll, total)
            el = reduce_elapsed_max(dist, el, device="cuda" if backend == "nccl" else "cpu")
            live_feed[name] = {"frames_per_s": round(aggregate_fps(K, world, el), 3), "p50_frame_latency_ms": round(statistics.median(cs) * 1e3, 4),
                               "p95_frame_latency_ms": round(sorted(cs)[int(0.95 * (len(cs) - 1))] * 1e3, 4)}
            # a fixed schedule replays exactly the Llama steps of the timed region; a secondary figure must never cost the line above, so a
            # mismatch is reported inside the object instead of raised
            if args.mode != "free" and not (len(li.past_key_values) == final_len and st_n == llm_steps):
                live_feed[name]["mismatch"] = f"KV {len(li.past_key_values)} vs {final_len} tokens, {st_n} vs {llm_steps} Llama steps"
            log(f"live_feed {name}: {K / el:.1f} frames/s, p50 {statistics.median(cs) * 1e3:.2f} ms")
        li.prefetch, li.prefetch_frames = saved
        li.real_greedy = False
        live_feed["one_frame_lookahead"] = "= `value` / `p50_frame_latency_ms` of this line (the timed region itself)"
        live_feed["note"] = (f"the same {K} frames from the same context ({kv_start} cached tokens, KV cropped back): no_lookahead = encode(frame t) then step(t) "
                             f"serially (the reference's own loop, demo/cli.py:31-38); recorded_file_lookahead = {batch_pf} frames per encoder call "
                             f"(= {batch_pf / args.fps:g} s of video at {args.fps:g} FPS ahead of the Llama steps: fine for a recorded file, not available to a live "
                             f"camera; the headline of rounds 1-5); real_greedy_path = the timed pipeline with every scheduled response generated by the "
                             f"token-reading greedy loop (models/modeling_live.py:173-182: async read of every token + speculative next step) instead of the "
                             f"forced-length loop that never looks at a token")
        live_feed["frames_per_s"] = live_feed["no_lookahead"]["frames_per_s"]
    # the long-input path (stream_evaluate's whole-dialogue forward, a long first prompt): ONE 4096-token teacher-forced block through
    # vlo_llm_step on a session of its own (prefill GEMMs + flash-style attention) — an extra key, outside the timed region
    prefill = None
    if args.full and not tp and rank == 0 and not args.no_prefill_probe:
        try:
            ps = eng.new_session()
            px = (torch.randn(PREFILL_PROBE_TOKENS, shape["hidden_size"], device="cuda") * 0.5).bfloat16()
            eng.llm_step(ps, px[:512])                      # allocates the prefill workspaces
            ps.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.llm_step(ps, px)
            torch.cuda.synchronize()
            dtp = time.perf_counter() - t0
            ps.close()
            prefill = {"tokens": PREFILL_PROBE_TOKENS, "ms": round(dtp * 1e3, 2), "tokens_per_s": round(PREFILL_PROBE_TOKENS / dtp, 1),
                       "arithmetic": ("W8A8: e4m3 weights x per-row e4m3 activation codes on v_mfma_f32_16x16x128_f8f6f4 (prefill_act_dtype=fp8), lm_head bf16"
                                      if args.weight_dtype == "fp8" else "bf16 MFMA, fp32 accumulation"),
                       "note": "one block from an empty cache, last-row logits only; 13 312-token passes and the kernel-level A/B: profiles/r6_prefill_*.txt"}
            log(f"prefill probe: {PREFILL_PROBE_TOKENS} tokens in {dtp * 1e3:.1f} ms = {PREFILL_PROBE_TOKENS / dtp:.0f} tok/s")
        except Exception as ex:
            prefill = {"error": repr(ex)}
    # tensor-parallel runs: latency of ONE exchange (all-reduce of [n, H] fp32 + residual add + RMSNorm) at the frame-step and the
    # decode-step size, every rank in lock-step — the number the xGMI all-reduce discussion of SURVEY.md §8e is about
    tp_exchange_us = None
    if args.full and tp:
        try:
            xs = eng.new_session()
            tp_exchange_us = {f"n{m}": round(eng.bench_exchange(xs, m, 200), 2) for m in (11, 1)}
            xs.close()
        except Exception as ex:
            tp_exchange_us = {"error": repr(ex)}

    elapsed = reduce_elapsed_max(dist, elapsed, device="cuda" if backend == "nccl" else "cpu")
    fps = aggregate_fps(K, 1 if tp else world, elapsed)        # TP: the ranks share ONE stream of K frames
    full_stream = None
    if pre is not None:
        # the whole stream, pre-roll included (rank-local clock around each of the two brackets; an extra key, not `value`)
        allc = pre[1] + costs
        full_stream = {"frames": total, "frames_per_s": round(total / (pre[0] + elapsed), 3),
                       "p50_frame_latency_ms": round(statistics.median(allc) * 1e3, 4),
                       "p95_frame_latency_ms": round(sorted(allc)[int(0.95 * (len(allc) - 1))] * 1e3, 4),
                       "llm_steps": pre[3] + llm_steps,
                       "frac_of_hbm_peak": round((pre[2] + alg_bytes) / (pre[0] + elapsed) / 1e9 / HBM_PEAK_GBS, 4),
                       "note": f"frames 0..{preroll - 1} with {batch_pf} frames per encoder call (the pre-roll), the last {K} with one frame of look-ahead (the timed region)"}

    out = None
    if rank == 0:
        minutes = total / args.fps / 60.0
        out = {
            "metric": ("streaming FPS + p50 per-frame latency, Llama-3-8B+SigLIP-L, 10 min @ 2 FPS, 1/2/4/8 GPU"
                       if args.model == "llama-3-8b" and abs(minutes - 10) < 1e-6 and args.fps == 2.0 else
                       f"streaming FPS + p50 per-frame latency, {args.model}+SigLIP-L, {minutes:g} min @ {args.fps:g} FPS"),
            "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": Wm,
            "ms_per_step": round(elapsed / K * 1e3, 4), "higher_is_better": True, "scaling": "strong" if tp else "weak",
            "vs_baseline": None,
            "dtype": "bf16" if args.weight_dtype == "bf16" else "bf16 activations / KV / accumulate-in-fp32, fp8 e4m3 weights (per-output-channel scales) expanded to bf16 in registers for the live step's bf16 MFMA; "
                     "native fp8 MFMA (W8A8) only on long-input prefill GEMMs (prefill_act_dtype=fp8): the `prefill` key, not this stream",
            "vit_dtype": "fp16 operands / fp32 accumulate + fp32 residual stream (the reference's GPU autocast, models/vision_live.py:13)",
            "data": "synthetic",
            "p50_frame_latency_ms": round(statistics.median(costs) * 1e3, 4),
            "p95_frame_latency_ms": round(sorted(costs)[int(0.95 * (len(costs) - 1))] * 1e3, 4),
            "config": {"workload": f"{args.model} + {args.vit}, "
                                   + (f"the LAST {K} frames (frames {preroll}..{total - 1}) of a {total}-frame stream = {minutes:g} min @ {args.fps:g} FPS 384x384 uint8 "
                                      f"(frames 0..{preroll - 1} pre-rolled un-timed through the same engine steps on the same session; KV at "
                                      f"{kv_start} tokens when the clock starts, {final_len} when it stops), "
                                      if preroll else f"all {K} frames of a {minutes:g} min @ {args.fps:g} FPS 384x384 uint8 stream (KV 0 -> {final_len} tokens), ")
                                   + (f"ONE stream, Llama TP={world} ({'RCCL' if args.tp_allreduce == 'rccl' else 'one-shot p2p'} all-reduce x2/layer), ViT "
                                      f"{'frame-parallel + all-gather of the frame embeddings' if args.tp_vit == 'frame-parallel' else 'replicated'}, "
                                      if tp else f"TP=1, one stream per GPU ({world} replica(s)), ") + f"mode={args.mode} "
                                   f"(16-token response every 10th frame + t=0 query), random-init weights at true shapes"
                                   + (f"; `value` / p50 = the pipeline north_star names, encode(t+1) on the encode stream beside the Llama step of frame t (ONE frame of "
                                      f"look-ahead); the same frames with no look-ahead: {live_feed['no_lookahead']['frames_per_s']} frames/s, p50 "
                                      f"{live_feed['no_lookahead']['p50_frame_latency_ms']} ms; with {batch_pf} frames per encoder call (a recorded file; the headline of "
                                      f"rounds 1-5): {live_feed['recorded_file_lookahead']['frames_per_s']} frames/s, p50 {live_feed['recorded_file_lookahead']['p50_frame_latency_ms']} ms; "
                                      f"through the token-reading greedy loop: {live_feed['real_greedy_path']['frames_per_s']} frames/s: see `live_feed`"
                                      if live_feed and all(k in live_feed for k in ("no_lookahead", "recorded_file_lookahead", "real_greedy_path")) else ""),
                       "frames": K, "stream_frames": total, "preroll_frames": preroll, "kv_tokens_at_start": kv_start,
                       "final_kv_tokens": final_len, "llm_steps": llm_steps, "prefetch_encode": not args.no_prefetch, "prefetch_frames": (1 if (not args.no_prefetch and preroll) else args.prefetch_frames), "preroll_prefetch_frames": args.prefetch_frames,
                       "parallelism": f"tp{world}" if tp else f"replicas{world}",
                       **({"rccl_comm": eng.comm_info()} if tp else {}),
                       **({"tp_exchange": dict(kind=args.tp_allreduce, us_per_exchange=tp_exchange_us,
                                                message="fp32 [n, H] partial sums (180 KB at n = 11, 16 KB at n = 1): summed in fp32 as inside one GEMM, "
                                                        "the exchange is latency-bound at this size",
                                                **(eng.p2p_status() if args.tp_allreduce == "p2p" else {}))} if tp else {})},
            **({"encode_stage": {"batch": max(1, args.prefetch_frames), "ms_per_frame": round(vit_ms, 4),
                             "tflops": round(vit_gflop / vit_ms, 1), "mfma_peak_tflops": MFMA_PEAK_TFLOPS,
                             "frac_of_mfma_peak": round(vit_gflop / vit_ms / MFMA_PEAK_TFLOPS, 4),
                             "one_frame_ms": round(vit1_ms, 4), "one_frame_frac_of_mfma_peak": round(vit_gflop / vit1_ms / MFMA_PEAK_TFLOPS, 4),
                             "note": ("SigLIP-L/16-384 + connector, 384.4 GFLOP/frame (SURVEY.md §8d), fp16 MFMA, measured alone" if args.vit == "siglip-l16-384"
                                      else f"{args.vit} + connector, {vit_gflop:.1f} GFLOP/frame (encoder + patch embed + head K/V + connector), fp16 MFMA, measured alone")}} if args.full else {}),
            **({"full_stream": full_stream} if full_stream else {}),
            **({"first_frame_ms": {"value": round(pre[1][0] * 1e3, 3),
                                   "note": "frame 0 of the stream, host wall time: its one-frame encode, the first Llama step (start prompt + 10 frame tokens "
                                           "through the 64-token block path), the t = 0 query and its 16-token response"}} if pre is not None and pre[1] else {}),
            **({"live_feed": live_feed} if live_feed else {}),
            **({"prefill": prefill} if prefill else {}),
            "stream_hbm_roofline": {"algorithmic_llm_bytes": alg_bytes, "frac_of_hbm_peak": round(alg_bytes / elapsed / 1e9 / HBM_PEAK_GBS, 4)},
            **({"roofline": roofline(args, n_launch, prof_ms, bytes_per_launch, empty_us)} if args.full else {}),
        }
    # N > 1, replica mode: also measure ONE stream tensor-parallel over the same N GPUs (BASELINE.json north_star).  It
    # runs in child processes (one per rank, own rendezvous port) so that a failure or hang of the RCCL leg — which no
    # single-GPU box can exercise beforehand — can never cost the replica line above.
    tp_leg = tp_p2p_leg = None
    if args.full and world > 1 and not tp and not args.no_tp_leg and os.environ.get("VLO_BENCH_TP_LEG", "1") != "0":
        tp_leg = run_tp_leg(args, rank, world, local, "rccl", 17)
        if dist is not None:
            dist.barrier()                     # every rank's first child is gone before the second leg claims the GPUs
        tp_p2p_leg = run_tp_leg(args, rank, world, local, "p2p", 29)
    if rank == 0:
        # north_star's multi-GPU number is ONE stream tensor-parallel over the N GPUs.  Next to the replica `value` (N independent
        # streams, trivially ~N x), each TP leg carries the strong-scaling figures against the one-GPU single-stream rate measured
        # in THIS run (the replica line / N): SURVEY.md §8e definition (1), end-to-end.  Definitions (2) all-reduce bus efficiency
        # and (3) latency vs the measured exchange floor are what `exchange.us_per_exchange` (64 exchanges per step) is for.
        for leg in (tp_leg, tp_p2p_leg):
            if leg and leg.get("value"):
                one = out["value"] / world
                leg["one_gpu_stream_frames_per_s"] = round(one, 3)
                leg["speedup_vs_one_gpu_stream"] = round(leg["value"] / one, 4)
                leg["scaling_efficiency"] = round(leg["value"] / one / world, 4)
                leg["efficiency_definition"] = ("end-to-end strong scaling of ONE stream: frames/s on N GPUs / (N x frames/s of one stream on "
                                                "one GPU, same run); the >= 0.85 target of BASELINE.json is read as this number")
        if tp_leg is not None:
            out["tp"] = tp_leg
        if tp_p2p_leg is not None:
            out["tp_p2p"] = tp_p2p_leg
        if world > 1:
            # what a reader of a SCALE line needs first, at the top level: how many ranks RCCL itself saw, and the strong-scaling
            # efficiency of ONE tensor-parallel stream (the better of the two exchange legs)
            seen = [((leg or {}).get("rccl_comm") or {}).get("nranks") for leg in (tp_leg, tp_p2p_leg)]
            out["rccl_ranks_seen"] = next((n for n in seen if n), int(out["config"].get("rccl_comm", {}).get("nranks", 0)) or None)
            effs = {name: leg.get("scaling_efficiency") for name, leg in (("tp", tp_leg), ("tp_p2p", tp_p2p_leg)) if leg and leg.get("scaling_efficiency")}
            out["tp_scaling_efficiency"] = max(effs.values()) if effs else None
            out["tp_scaling_efficiency_by_leg"] = effs or None
        if args.full and world == 1 and not args.no_cpu_baseline and args.vit != "siglip-l16-384":
            out["cpu_baseline"] = {"value": None, "note": "the CPU baseline is the reference's own path, which only accepts SigLIP-L (models/vision_live.py:56-60)"}
        elif args.full and world == 1 and not args.no_cpu_baseline:
            log("cpu_baseline: building CPU oracle")
            try:
                out["cpu_baseline"] = cpu_baseline(args.model, frames[:max(args.cpu_sample_frames, 10)].cpu(), toks, args.mode,
                                                   args.cpu_sample_frames, budget_s=args.cpu_budget_s, windows=[int(v) for v in args.cpu_windows.split(",") if v],
                                                   window_13k_frames=args.cpu_window_13k_frames if args.model == "llama-3-8b" else 0)
            except Exception as ex:     # never lose the GPU line to a host-side problem
                out["cpu_baseline"] = {"value": None, "error": repr(ex)}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
