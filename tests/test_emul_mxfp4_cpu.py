"""MXFP4 weight streaming (include/vlo.h vlo_config.weight_dtype = 2: OCP e2m1 codes + one e8m0 scale per 32 elements along K) on the emulated
library (tests/hip_emul: the engine's sources compiled for the CPU, which takes the integer arm of the code expansion in csrc/common.cuh),
through the C ABI, at toy sizes.

Numerics contract: W4A16 with exact expansion — the kernels multiply bf16(code * 2^(scale - 127)), which IS code * 2^(scale - 127), against the
unchanged bf16 activations, so the parity target is the reference's arithmetic on the dequantised weights: the GEMV alone against an fp64
matmul, the stream in the project's 3-way band with both legs (bf16 reference, fp32 gold) on checkpoint.dequantize_mxfp4's weights."""
import ctypes as C

import pytest
import torch

from tests.parity_util import within_band

from oracle import vlo_oracle as O

# every K a multiple of 128: hidden 128 (q|k|v, o, gate|up, lm_head), intermediate 256 (down); head dim 64
TOY = O.LlmSpec(128, 256, 2, 2, 2, 256, 10000.0, 1e-5, vision_hidden_size=128)
# the fp8 image needs K >= 512 (an even fragment count on 8 waves): the engine whose lm_head is fp8 per channel.  Head dim 128, 2 query heads per
# kv head; its mxfp4 projections walk KC = 4 / 8 chunks on one wave
TOY_512 = O.LlmSpec(512, 1024, 2, 4, 2, 256, 10000.0, 1e-5, vision_hidden_size=128)
TOY_I192 = O.LlmSpec(128, 192, 2, 2, 2, 256, 10000.0, 1e-5, vision_hidden_size=128)     # down-proj K = 192: no whole weight registers


@pytest.fixture(scope="module")
def E():
    import resource
    soft, _ = resource.getrlimit(resource.RLIMIT_NPROC)
    if soft != resource.RLIM_INFINITY and soft < 4096:
        pytest.skip(f"the emulation runs every GPU thread of a block as an OS thread (up to 1024): RLIMIT_NPROC = {soft}")
    from tests.hip_emul import emul_engine
    if emul_engine.lib() is None:
        pytest.skip("no clang++ to build the emulated library")
    return emul_engine


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def gemv_mxfp4(E, x, codes, scale):
    x, codes, scale = x.to(torch.bfloat16).contiguous(), codes.contiguous(), scale.contiguous()
    N, K = codes.shape[0], 2 * codes.shape[1]
    y = torch.zeros(x.shape[0], N, dtype=torch.float32)
    E.check(E.lib().vlo_test_gemv_mxfp4(_ptr(x), _ptr(codes), _ptr(scale), _ptr(y), x.shape[0], N, K, None))
    return y


def make_engine(E, spec, weight_dtype=2, tp_size=1):
    """EmulEngine created with vlo_config.weight_dtype = weight_dtype whose load_weights tags uint8 tensors as the Python layer does: the
    "_scale" of an mxfp4 matrix is VLO_DT_E8M0, the matrix VLO_DT_FP4_E2M1X2 with its logical shape; raises on a refused call"""
    from videollm_online_amd import _C

    class Mxfp4Engine(E.EmulEngine):
        def __init__(self):
            E.EmulEngine.__init__(self, spec, weight_dtype=weight_dtype, tp_size=tp_size)

        def load_weight(self, name, t):
            t = t.detach().contiguous()
            shape = tuple(t.shape)
            if t.dtype == torch.uint8:
                dt = _C.DT_E8M0 if name.endswith("_scale") else _C.DT_FP4_E2M1X2
                if dt == _C.DT_FP4_E2M1X2:
                    shape = (shape[0], 2 * shape[1])
            elif t.dtype == torch.float8_e4m3fn:
                dt, t = _C.DT_FP8_E4M3, t.view(torch.uint8)
            else:
                dt = {torch.float32: _C.DT_F32, torch.bfloat16: _C.DT_BF16}[t.dtype]
            return E.lib().vlo_engine_load_weight(self._h, name.encode(), _ptr(t), dt, (C.c_int64 * len(shape))(*shape), len(shape))

        def load_weights(self, weights, inv_freq=None):
            for name, t in weights.items():
                E.check(self.load_weight(name, t))
            if inv_freq is not None:
                E.check(self.load_weight("rope.inv_freq", inv_freq.float()))
            E.check(E.lib().vlo_engine_finalize(self._h))
            return self

        def weight_bytes(self):
            return int(E.lib().vlo_engine_weight_bytes(self._h))

    return Mxfp4Engine()


def quantized(w, lm_head):
    """(engine weights, oracle weights = the same codes dequantised, names the bf16 oracle keeps in fp32).  lm_head: "fp8" or "mxfp4"."""
    from videollm_online_amd.checkpoint import dequantize_mxfp4, quantize_fp8_per_channel, quantize_mxfp4
    eng_w, ora_w, keep = {}, {}, set()
    for k, v in w.items():
        if not k.endswith(O.FP8_STREAMED) or k.startswith(("vision.", "connector.")):
            eng_w[k] = ora_w[k] = v
        elif k == "lm_head.weight" and lm_head == "fp8":
            q, s = quantize_fp8_per_channel(v)
            eng_w[k], eng_w[k + "_scale"], ora_w[k] = q, s, q.float() * s[:, None]
            keep.add(k)
        else:
            c, s = quantize_mxfp4(v)
            eng_w[k], eng_w[k + "_scale"], ora_w[k] = c, s, dequantize_mxfp4(c, s)
            keep.add(k)
    return eng_w, ora_w, keep


def _steps(spec, ref, toks, seed, lens):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        ids = torch.tensor([toks.interval_id] + toks.stream_prompt_ids + toks.stream_generation_ids)[:max(1, n - 10)]
        rows = [ref.embed(ids)]
        if n > len(ids):
            rows.append(torch.randn(n - len(ids), spec.hidden_size, generator=g).bfloat16())
        out.append(torch.cat(rows)[:n])
    return out


# ---- the GEMV alone ----------------------------------------------------------------------------------------------------------------------
# K = 128: 1 wave x 4 fragments; K = 256: the same with 2 K slices; K = 4096: 8 waves x 16 fragments (the 8B plan); N = 40: a padded tile
@pytest.mark.parametrize("n,N,K", [(1, 40, 128), (11, 64, 256), (16, 48, 4096)])
def test_mxfp4_gemv_matches_dequantized_matmul(E, n, N, K):
    from videollm_online_amd.checkpoint import dequantize_mxfp4, quantize_mxfp4
    assert E.gemv_plan(K, 0x200)[0] * E.gemv_plan(K, 0x200)[1] * E.gemv_plan(K, 0x200)[2] * 32 == K
    g = torch.Generator().manual_seed(n * 1000 + N + K)
    x = torch.randn(n, K, generator=g).bfloat16()
    W = (torch.randn(N, K, generator=g) * K ** -0.5 * (1 + torch.rand(N, 1, generator=g) * 3)).bfloat16()
    codes, scale = quantize_mxfp4(W)
    y = gemv_mxfp4(E, x, codes, scale)
    ref = x.double() @ dequantize_mxfp4(codes, scale).double().T
    err = (y.double() - ref).abs().max().item()
    tol = 2e-5 * max(1.0, ref.abs().max().item()) * (K / 256) ** 0.5 + 1e-5
    print(f"[emul mxfp4 gemv n={n} N={N} K={K}] err {err:.3g} tol {tol:.3g}")
    assert err < tol, err


GEMV_BATCH_CHILD = r"""
import ctypes as C, sys, torch
sys.path.insert(0, %r)
from tests.hip_emul import emul_engine as E
from videollm_online_amd.checkpoint import dequantize_mxfp4, quantize_mxfp4
K, N, n = 8192, 22 * 16 + 8, 11          # 23 column tiles (the last one half full) = 12 groups, the last with ONE tile, on VLO_GEMV_CUS = 2 blocks:
g = torch.Generator().manual_seed(8192)  # each block walks 6 groups (a batch of 4 + a batch of 2)
x = torch.randn(n, K, generator=g).bfloat16()
W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
assert E.gemv_plan(K, 0x200) == (8, 16, 2, 1), E.gemv_plan(K, 0x200)        # 8 waves x 16 fragments, KC = 2 chunks, one K slice
codes, scale = quantize_mxfp4(W)
y = torch.zeros(n, N, dtype=torch.float32)
p = lambda t: C.c_void_p(t.data_ptr())
E.check(E.lib().vlo_test_gemv_mxfp4(p(x), p(codes), p(scale), p(y), n, N, K, None))
ref = x.double() @ dequantize_mxfp4(codes, scale).double().T
assert (y.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item()) * (K / 256) ** 0.5 + 1e-5
torch.save(y, sys.argv[1])
print("OKGEMV")
"""


def test_mxfp4_gemv_chunk_outer_batches(E, tmp_path):
    """K = 8192 as the step launches it (one K slice, KC = 2 chunks of 8 waves x 16 fragments): the batch loop over 4 groups (gemv_body.inc
    GB = 4) with full and partial batches and a one-tile last group, against the fp64 matmul — and bit-identical to the group-outer loop
    (VLO_GEMV_BATCH=0).  The grid size and the loop form are read once per process: a child process each."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for batch in ("1", "0"):
        f = str(tmp_path / f"b{batch}.pt")
        env = dict(os.environ, VLO_TEST_GEMV_WHOLE_K="1", VLO_GEMV_CUS="2", VLO_GEMV_BATCH=batch)
        r = subprocess.run([sys.executable, "-c", GEMV_BATCH_CHILD % root, f], env=env, capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0 and "OKGEMV" in r.stdout, r.stderr[-2000:]
        outs[batch] = torch.load(f)
    assert torch.equal(outs["1"], outs["0"])


def test_expansion_is_exact_for_every_code_and_scale(E):
    """One-hot activation rows read single weights back through the GEMV: y[m][n] = W[n][m] with nothing to round.  Row n carries scale byte
    n + 2 (2 .. 252: every scale whose products are all finite in bf16), columns 0 .. 15 the sixteen codes: the expansion's bits for every
    (code, scale) against dequantize_mxfp4.
    Scale bytes 253 and 254 — accepted at load — take
    the products past bf16's largest binade (4 and 6 at 253; 2, 3, 4 and 6 at 254), which must come out as infinities of the code's sign: each
    (code, scale) of those two bytes has a row of its own whose other codes are 0, read by the one row of x that is 1 in its column (the other
    rows of x meet 0 * inf there and are not looked at)."""
    from videollm_online_amd.checkpoint import dequantize_mxfp4
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
    y = gemv_mxfp4(E, x, codes, scale)
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


# ---- an mxfp4 engine end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm_head", ["fp8", "mxfp4"])
def test_mxfp4_engine_stream(E, lm_head):
    """A 45-token prompt (the 64-token block path, gemm64_kernel<KF, EPI, WQ = 2>), then frame and decode steps on the 16-row path (n = 11, 4,
    1, 13) against LlamaOracle bf16 / fp32 on the dequantised weights"""
    spec = TOY_512 if lm_head == "fp8" else TOY
    w = O.init_llm_weights(spec, seed=21)
    eng_w, ora_w, keep = quantized(w, lm_head)
    ref, gold = O.LlamaOracle(spec, ora_w, torch.bfloat16, keep_fp32=keep), O.LlamaOracle(spec, ora_w, torch.float32)
    toks = O.default_tokens(spec, n_start=35)
    eng = make_engine(E, spec).load_weights(eng_w, O.rope_inv_freq(spec.head_dim, spec.rope_theta))
    H, I, V = spec.hidden_size, spec.intermediate_size, spec.vocab_size
    kvw = spec.num_kv_heads * spec.head_dim
    proj = spec.num_layers * (2 * H * H + 2 * kvw * H + 3 * H * I)     # q, o; k, v; gate, up, down
    lm = V * H * (1 if lm_head == "fp8" else 0.5 + 1 / 32) + (4 * V if lm_head == "fp8" else 0)
    # bf16: the norm weights and the connector (two Linears with bias); the gathered embedding table is not counted
    small = 2 * ((2 * spec.num_layers + 1) * H + H * spec.vision_hidden_size + H * H + 2 * H)
    assert eng.weight_bytes() == int(proj * (0.5 + 1 / 32) + lm + small), (eng.weight_bytes(), proj, lm, small)
    s = eng.new_session()
    rc = gc = None
    for i, x in enumerate(_steps(spec, ref, toks, 22, [45, 11, 4, 1, 13])):
        rl, rc = ref.forward(x, rc)
        gl, gc = gold.forward(x, gc)
        last, allr = eng.llm_step(s, x)
        assert eng.session_len(s) == len(rc) and torch.equal(last, allr[-1])
        e = (allr.float() - gl).abs().max().item()
        r = (rl.float() - gl).abs().max().item()
        scale = gl.abs().max().item()
        print(f"[emul mxfp4 lm_head={lm_head}] step {i}: engine err {e:.4g} ref-bf16 err {r:.4g} scale {scale:.3g}")
        assert within_band(e, r, 1e-3 * scale, "test_emul_mxfp4_cpu.py:stream"), f"step {i}: {e} vs {r}"
    eng.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
VLO_E_INVALID, VLO_E_UNSUPPORTED = -1, -6


def _one_matrix():
    from videollm_online_amd.checkpoint import quantize_mxfp4
    W = (torch.randn(128, 128, generator=torch.Generator().manual_seed(1)) * 0.1).bfloat16()
    return quantize_mxfp4(W)


@pytest.mark.parametrize("bad", [255, 1, 0])
def test_scale_bytes_outside_the_range_are_refused(E, bad):
    codes, scale = _one_matrix()
    eng = make_engine(E, TOY)
    name = "model.layers.0.self_attn.q_proj.weight"
    assert eng.load_weight(name, codes) == 0
    assert eng.load_weight(name + "_scale", scale) == 0
    scale = scale.clone()
    scale[5, 2] = bad
    assert eng.load_weight(name + "_scale", scale) == VLO_E_INVALID
    assert b"outside [2, 254]" in E.lib().vlo_last_error()
    eng.close()


@pytest.mark.parametrize("weight_dtype", [0, 1])
def test_fp4_data_is_refused_by_bf16_and_fp8_engines(E, weight_dtype):
    codes, scale = _one_matrix()
    eng = make_engine(E, TOY, weight_dtype=weight_dtype)
    name = "model.layers.0.self_attn.q_proj.weight"
    assert eng.load_weight(name, codes) == VLO_E_INVALID
    assert eng.load_weight(name + "_scale", scale) == VLO_E_INVALID
    eng.close()


def test_fp4_data_is_refused_outside_the_streamed_projections(E):
    codes, scale = _one_matrix()
    eng = make_engine(E, TOY)
    assert eng.load_weight("connector.2.weight", codes) == VLO_E_INVALID
    assert eng.load_weight("model.embed_tokens.weight", codes) == VLO_E_INVALID
    eng.close()


def test_tensor_parallel_mxfp4_is_refused_at_create(E):
    with pytest.raises(RuntimeError, match=r"error -6.*tp_size"):
        make_engine(E, TOY, tp_size=2)


def test_bf16_projection_on_an_mxfp4_engine_is_refused_at_finalize(E):
    w = O.init_llm_weights(TOY, seed=21)
    eng = make_engine(E, TOY)
    with pytest.raises(RuntimeError, match="VLO_DT_FP4_E2M1X2"):
        eng.load_weights(w)
    eng.close()


def test_a_k_without_a_plan_is_refused_at_finalize(E):
    """intermediate 192: the down-proj's K is not a multiple of 128"""
    w = O.init_llm_weights(TOY_I192, seed=21)
    eng_w, _, _ = quantized(w, "fp8")
    eng = make_engine(E, TOY_I192)
    with pytest.raises(RuntimeError, match=r"error -6.*K=192"):
        eng.load_weights(eng_w)
    eng.close()


def test_bf16_and_fp8_plans_are_where_they_were(E):
    """the plans of the other two formats for every K the suite queries (tests/test_cabi.py), recorded before the mxfp4 list existed"""
    want = {4096: (8, 16, 1, 1), 14336: (8, 14, 4, 1), 2048: (8, 8, 1, 1), 5632: (8, 11, 2, 1), 8192: (8, 16, 2, 1), 28672: (8, 16, 7, 1),
            1024: (8, 4, 1, 1), 7168: (8, 14, 2, 1), 3584: (8, 14, 1, 1), 1792: (4, 14, 1, 1), 512: (8, 2, 1, 1), 1408: (4, 11, 1, 1),
            256: (8, 1, 1, 1), 704: (2, 11, 1, 1), 128: (4, 1, 1, 1)}
    for K, plan in want.items():
        assert E.gemv_plan(K, False) == plan, (K, E.gemv_plan(K, False))
    for K, plan in {4096: (8, 16, 1, 1), 8192: (8, 16, 2, 1), 14336: (8, 28, 2, 1), 28672: (8, 28, 4, 1), 128: (1, 4, 1, 1), 256: (1, 4, 2, 1)}.items():
        assert E.gemv_plan(K, 0x200) == plan, (K, E.gemv_plan(K, 0x200))
    assert E.gemv_plan(14336, 0x201) == (8, 28, 1, 2) and E.gemv_plan(28672, 0x201) == (8, 28, 1, 4)
    with pytest.raises(RuntimeError):
        E.gemv_plan(192, 0x200)
