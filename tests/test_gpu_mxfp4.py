"""MXFP4 weight streaming (include/vlo.h vlo_config.weight_dtype = 2; EngineConfig(weight_dtype="mxfp4")) on the MI355X: the Llama projections
are stored as OCP e2m1 codes with one e8m0 scale per 32 elements along K (4.25 bits per weight), expanded to bf16 in registers — exactly,
code * 2^(scale - 127) is a bf16 value — and multiplied on the bf16 matrix cores; activations, KV cache and accumulation are unchanged.

Parity target = the reference's arithmetic on the dequantised weights (checkpoint.dequantize_mxfp4), 3-way as for the fp8 image:
err(engine, fp32 gold) <= 1.5 * err(bf16-activation reference, fp32 gold) + 1e-3 * max|logit| — plus the GEMV alone against an fp64 matmul of
the dequantised weights, where only the fp32 accumulation error remains."""
import os
import sys

import pytest
import torch

from oracle import vlo_oracle as O
from parity_util import fmt, ulp_report

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu


# ---- the GEMV alone --------------------------------------------------------------------------------------------------------------------
# the kernel variant is chosen by K (4096, 8192: 8 waves x 16 fragments; 14336, 28672: 8 x 28 with 2 / 4 K slices); N stays small.
# (11, 1000, 8192): N is not a multiple of 16 — a padded tile; (5, 6144, 4096): more groups than one round of blocks
@pytest.mark.parametrize("n,N,K", [(1, 256, 4096), (11, 512, 14336), (16, 256, 8192), (11, 256, 28672), (11, 1000, 8192), (5, 6144, 4096)])
def test_mxfp4_gemv_matches_dequantized_matmul(n, N, K):
    from videollm_online_amd.checkpoint import dequantize_mxfp4, quantize_mxfp4
    from videollm_online_amd.engine import test_gemv_mxfp4
    g = torch.Generator().manual_seed(n * 1000 + N + K)
    x = torch.randn(n, K, generator=g).bfloat16()
    W = (torch.randn(N, K, generator=g) * K ** -0.5 * (1 + torch.rand(N, 1, generator=g) * 3)).bfloat16()     # rows of different scale
    codes, scale = quantize_mxfp4(W.cuda())
    y = test_gemv_mxfp4(x.cuda(), codes, scale).cpu()
    ref = x.double() @ dequantize_mxfp4(codes.cpu(), scale.cpu()).double().T
    err = (y.double() - ref).abs().max().item()
    tol = 2e-5 * max(1.0, ref.abs().max().item()) * (K / 256) ** 0.5 + 1e-5
    print(f"[mxfp4 gemv n={n} N={N} K={K}] err {err:.3g} tol {tol:.3g}")
    assert err < tol, err


def test_expansion_is_exact_for_every_code_and_scale():
    """One-hot activation rows read single weights back through the GEMV: y[m][n] = W[n][m] with nothing to round.  Row n carries scale byte
    n + 2 (2 .. 252: every scale whose products are all finite in bf16), columns 0 .. 15 the sixteen codes: the bits the hardware conversion
    (v_cvt_scalef32_pk_bf16_fp4) gives for every (code, scale) against dequantize_mxfp4 — the values the integer arm of csrc/common.cuh gives
    in tests/test_emul_mxfp4_cpu.py.
    Scale bytes 253 and 254 — accepted at load — take
    the products past bf16's largest binade (4 and 6 at 253; 2, 3, 4 and 6 at 254), which must come out as infinities of the code's sign: each
    (code, scale) of those two bytes has a row of its own whose other codes are 0, read by the one row of x that is 1 in its column (the other
    rows of x meet 0 * inf there and are not looked at)."""
    from videollm_online_amd.checkpoint import dequantize_mxfp4
    from videollm_online_amd.engine import test_gemv_mxfp4
    N, K = 284, 128
    codes = torch.zeros(N, K // 2, dtype=torch.uint8)
    codes[:251, :8] = torch.tensor([(2 * j + 1) << 4 | (2 * j) for j in range(8)], dtype=torch.uint8)
    scale = torch.full((N, K // 32), 127, dtype=torch.uint8)
    scale[:251, 0] = torch.arange(2, 253, dtype=torch.uint8)
    top = [(s, c) for s in (253, 254) for c in range(16)]              # rows 251 .. 282: code c alone in column c under scale byte s
    for i, (s, c) in enumerate(top):
        codes[251 + i, c // 2] = c << (4 * (c & 1))
        scale[251 + i, 0] = s
    x = torch.zeros(16, K, dtype=torch.bfloat16)
    x[torch.arange(16), torch.arange(16)] = 1.0
    y = test_gemv_mxfp4(x.cuda(), codes.cuda(), scale.cuda()).cpu()
    want = dequantize_mxfp4(codes, scale)[:, :16].T.contiguous()        # [16 codes][N rows]; fp32 overflows where bf16 does (same exponent range)
    assert torch.isfinite(want[:, :251]).all()
    bad = [(int(m), int(n) + 2, y[m, n].item(), want[m, n].item()) for m, n in (y[:, :251] != want[:, :251]).nonzero()[:8]]
    inf = 0
    for i, (s, c) in enumerate(top):
        got, w = y[c, 251 + i].item(), want[c, 251 + i].item()
        inf += w in (float("inf"), float("-inf"))
        if not got == w:                                               # inf == inf; a NaN equals nothing
            bad.append((c, s, got, w))
    assert inf == 4 + 8                                                # +-{4, 6} at 253, +-{2, 3, 4, 6} at 254
    assert not bad, bad


def test_quantizer_on_the_gpu_matches_the_cpu():
    """checkpoint.quantize_mxfp4 on the GPU against the same function on the CPU: the scale bytes must be equal; a code may differ only where
    a boundary value moved by ONE grid step, on at most 1e-5 of the values (the bound of the fp8 quantiser's test; the rule is written with
    frexp / ldexp and integer compares, which leave no rounding to differ in — the counts are printed)."""
    from videollm_online_amd.checkpoint import quantize_mxfp4
    g = torch.Generator().manual_seed(1)
    for N, K in ((1024, 8192), (512, 14336), (2048, 2048)):
        W = (torch.randn(N, K, generator=g) * K ** -0.5 * (1 + torch.rand(N, 1, generator=g) * 3)).bfloat16()
        c, s = quantize_mxfp4(W.cuda())
        cc, sc = quantize_mxfp4(W)
        c = c.cpu()
        lo, hi = (c & 15).int() - (cc & 15).int(), (c >> 4).int() - (cc >> 4).int()
        d = torch.cat([lo.flatten(), hi.flatten()])
        print(f"[mxfp4 quantizer {N}x{K}] {int((s.cpu() != sc).sum())} of {sc.numel()} scale bytes differ; {int((d != 0).sum())} of {d.numel()} codes differ "
              f"(max code step {int(d.abs().max())})")
        assert torch.equal(s.cpu(), sc)
        assert (d != 0).float().mean().item() <= 1e-5 and int(d.abs().max()) <= 1


# ---- engines -----------------------------------------------------------------------------------------------------------------------------
def _cfg(spec, **kw):
    from videollm_online_amd.engine import EngineConfig
    return EngineConfig(hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                        num_attention_heads=spec.num_heads, num_key_value_heads=spec.num_kv_heads, vocab_size=spec.vocab_size,
                        rope_theta=spec.rope_theta, rms_norm_eps=spec.rms_eps, vision_hidden_size=spec.vision_hidden_size,
                        kv_pool_tokens=2048, weight_dtype="mxfp4", **kw)


def _oracle_weights(w, lm_head):
    """The weights an mxfp4 engine holds, dequantised for the oracle, by the product's quantisers on the GPU — the functions and the device
    Engine.load_weight uses for bf16 weights handed to it, so both sides hold ONE quantisation.  lm_head: "fp8" (what the Python layer does
    with a bf16 lm_head) or "mxfp4".  Returns (oracle weights, names the bf16 oracle keeps in fp32, the lm_head's codes + scales)."""
    from videollm_online_amd.checkpoint import dequantize_mxfp4, quantize_fp8_per_channel, quantize_mxfp4
    ora_w, keep, lm = {}, set(), None
    for k, v in w.items():
        if not k.endswith(O.FP8_STREAMED) or k.startswith(("vision.", "connector.")):
            ora_w[k] = v
        elif k == "lm_head.weight" and lm_head == "fp8":
            q, s = quantize_fp8_per_channel(v.cuda())
            ora_w[k] = q.cpu().float() * s.cpu()[:, None]
            keep.add(k)
        else:
            c, s = quantize_mxfp4(v.cuda())
            ora_w[k] = dequantize_mxfp4(c, s).cpu()
            keep.add(k)
            if k == "lm_head.weight":
                lm = (c, s)
    return ora_w, keep, lm


class _Model:
    """weights, oracles (bf16 reference + fp32 gold on the dequantised weights) and a finalized mxfp4 engine of one spec, built once per module"""

    def __init__(self, name, seed, lm_head):
        from videollm_online_amd.engine import Engine
        self.spec = spec = O.LLM_SPECS[name]
        self.w = w = O.init_llm_weights(spec, seed=seed)
        ora_w, keep, lm = _oracle_weights(w, lm_head)
        self.ref, self.gold = O.LlamaOracle(spec, ora_w, torch.bfloat16, keep_fp32=keep), O.LlamaOracle(spec, ora_w, torch.float32)
        self.toks = O.default_tokens(spec, seed=7, n_start=35)
        self.eng = eng = Engine(_cfg(spec))
        for k, v in w.items():                                 # bf16 in: quantised on the way (projections mxfp4, lm_head fp8) ...
            if k == "lm_head.weight" and lm is not None:       # ... unless the lm_head comes pre-quantised as mxfp4
                eng.load_weight(k, lm[0])
                eng.load_weight(k + "_scale", lm[1])
            else:
                eng.load_weight(k, v)
        eng.load_weight("rope.inv_freq", O.rope_inv_freq(spec.head_dim, spec.rope_theta))
        eng.finalize()


@pytest.fixture(scope="module")
def m8b():
    m = _Model("llama-3-8b-2l", 6, "fp8")
    yield m
    m.eng.close()


def _steps(spec, ref, toks, seed):
    """the five-step sequence of tests/test_gpu_fp8.py"""
    g = torch.Generator().manual_seed(seed + 100)
    H = spec.hidden_size
    frame = lambda: torch.randn(10, H, generator=g).bfloat16()
    return [torch.cat([ref.embed(torch.tensor(toks.start_ids)), frame()]),         # 45 tokens: the 64-token block path on the mxfp4 image
            torch.cat([ref.embed(torch.tensor([toks.interval_id])), frame()]),      # n = 11
            ref.embed(torch.tensor(toks.stream_generation_ids)),                    # n = 4
            ref.embed(torch.tensor([17])),                                         # n = 1
            torch.cat([ref.embed(torch.tensor([toks.eos_token_id] + toks.stream_prompt_ids)), frame()])]   # n = 13


def _check(tag, i, allr, rl, gl):
    e = (allr.float() - gl).abs().max().item()
    r = (rl.float() - gl).abs().max().item()
    scale = gl.abs().max().item()
    print(f"[{tag}] step {i}: engine err {e:.4g} ref err {r:.4g} scale {scale:.3g} | engine vs ref: {fmt(ulp_report(allr, rl))}")
    assert e <= 1.5 * r + 1e-3 * scale, f"{tag} step {i}: engine err {e} vs reference err {r}"


def _run(tag, m, sess, xs):
    rc = gc = None
    for i, x in enumerate(xs):
        rl, rc = m.ref.forward(x, rc)
        gl, gc = m.gold.forward(x, gc)
        last, allr = m.eng.llm_step(sess, x.cuda(), want_last=True, want_all=True)
        torch.cuda.synchronize()
        assert sess.get_seq_length() == len(rc) and torch.equal(last, allr[-1])
        _check(tag, i, allr.cpu(), rl, gl)


def test_mxfp4_llm_stream_parity_8b_width(m8b):
    m, w = m8b, m8b.w
    proj = 2 * sum(v.numel() for k, v in w.items() if k.endswith(O.FP8_STREAMED) and k != "lm_head.weight")
    bound = 0.30 * proj + 0.56 * 2 * w["lm_head.weight"].numel() + 2 * w["model.embed_tokens.weight"].numel()
    print(f"[mxfp4 8b-2l] weight bytes {m.eng.weight_bytes} (bound {bound:.0f}; the seven projections in bf16: {proj})")
    assert m.eng.weight_bytes < bound                  # 4.25 bits per weight = 0.266 of bf16
    sess = m.eng.new_session()
    _run("mxfp4 8b-2l", m, sess, _steps(m.spec, m.ref, m.toks, 6))
    ids = torch.zeros(6, dtype=torch.long, device="cuda")
    n = m.eng.greedy_generate(sess, m.eng.embed(torch.tensor(m.toks.stream_generation_ids)), m.toks.eos_token_id, ids, force_len=5)
    assert n == 5 and ids[4].item() == m.toks.eos_token_id
    sess.close()


def test_mxfp4_llm_stream_parity_70b_width():
    """H 8192, I 28672, 64 q / 8 kv heads at TP = 1 with the lm_head pre-quantised as mxfp4: K = 8192 walks two chunks per wave (the batch loop
    over four groups, every epilogue the step uses, lm_head included), K = 28672 four K slices of 8 waves x 28 fragments"""
    m = _Model("llama-3-70b-1l", 8, "mxfp4")
    sess = m.eng.new_session()
    _run("mxfp4 70b-1l", m, sess, _steps(m.spec, m.ref, m.toks, 8)[:4])
    sess.close()
    m.eng.close()


@pytest.mark.parametrize("tokens", [150, 700])
def test_mxfp4_block_and_prefill_paths_teacher_forced_rows(m8b, tokens):
    """150 tokens: blocks of 64 + 64 + 22 through gemm64_kernel<KF, EPI, WQ = 2>; 700 tokens: the prefill path, every projection's image
    expanded to bf16 (expand_mxfp4_image_kernel) right before its ping-pong GEMM.  Every row's logits, then n = 11 and n = 1 on the 16-row
    path over the KV those rows appended."""
    m = m8b
    sess = m.eng.new_session()
    g = torch.Generator().manual_seed(31 + tokens)
    ids = torch.randint(0, m.spec.vocab_size, (tokens,), generator=g)
    _run(f"mxfp4 8b-2l {tokens} rows", m, sess, [m.ref.embed(ids), torch.randn(11, m.spec.hidden_size, generator=g).bfloat16(),
                                                 m.ref.embed(torch.tensor([5]))])
    sess.close()


def test_mxfp4_batched_steps_bit_equal_to_solo(m8b):
    """Two sessions stepped through Batch.step (n = 11 and n = 1 rows, then one row each) equal the same sessions stepped alone on forks, bit
    for bit, in the last-row logits and in the K / V they appended: the batched step's guarantee on the mxfp4 image."""
    eng = m8b.eng
    g = torch.Generator(device="cuda").manual_seed(3)
    rows = lambda n: torch.randn(n, eng.cfg.hidden_size, generator=g, device="cuda").bfloat16()
    sessions = []
    for L in (40, 259):
        s = eng.new_session()
        eng.llm_step(s, rows(L), want_last=False)
        sessions.append(s)
    batch = eng.new_batch(2)
    nkv = eng.cfg.num_key_value_heads
    for xs in ([rows(11), rows(1)], [rows(1), rows(1)]):
        lens = [s.get_seq_length() for s in sessions]
        forks = [s.fork(L) for s, L in zip(sessions, lens)]
        last = batch.step(sessions, xs)
        for b, (s, f, x, L) in enumerate(zip(sessions, forks, xs, lens)):
            want, _ = eng.llm_step(f, x)
            assert s.get_seq_length() == f.get_seq_length() == L + x.shape[0]
            assert torch.equal(last[b].view(torch.int16), want.view(torch.int16)), (b, (last[b].float() - want.float()).abs().max().item())
            for layer in range(eng.cfg.num_hidden_layers):
                for h in (0, nkv - 1):
                    for which in (0, 1):
                        got, ref = s.read_kv(layer, which, h, L, L + x.shape[0]), f.read_kv(layer, which, h, L, L + x.shape[0])
                        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (b, layer, h, which)
        for f in forks:
            f.close()
    batch.close()
    for s in sessions:
        s.close()


def test_refused_configurations():
    from videollm_online_amd.engine import Engine, TpGroup
    spec = O.LLM_SPECS["tinyllama-2l"]                      # down-proj K = 5632 = 44 x 128, but 176 fragments fit none of the mxfp4 plans
    eng = Engine(_cfg(spec))
    eng.load_weights(O.init_llm_weights(spec, seed=5))
    with pytest.raises(RuntimeError, match="no mxfp4 GEMV plan for K=5632"):
        eng.finalize()
    eng.close()
    with pytest.raises((RuntimeError, ValueError), match="tp_size|tensor parallel"):
        TpGroup(_cfg(O.LLM_SPECS["llama-3-8b-2l"]), 2)
