"""Stream lookahead (include/vlo.h vlo_stream_steps / vlo_stream_steps_commit / vlo_steps_input) on the emulated library (tests/hip_emul: the
engine's sources compiled for the CPU), through the C ABI, at toy sizes: head dim 64 and 128, units of 4..6 rows, so that a pass of three or
four units is 12..20 rows — both sides of the 16-row / block-path threshold.  The cases live in tests/stream_steps_cases.py and run on the
MI355X as well (tests/test_gpu_stream_steps.py)."""
import pytest
import torch

from oracle import vlo_oracle as O
from tests import stream_steps_cases as K
from tests.test_emul_kv_fp8_cpu import TINY, TINY_GQA, TINY_HD128, E, loaded  # noqa: F401  (E: the module's fixture)

# (spec, frame rows per unit): 3 units are 12 rows (16-row pipeline) / 18 rows (block path)
SHAPES = {"hd64-12rows": (TINY_GQA, 3), "hd128-18rows": (TINY_HD128, 5)}
HIST = 45
_models = {}


@pytest.fixture(scope="module")
def model(E):
    def get(name):
        if name not in _models:
            spec, F = SHAPES[name]
            w = O.init_llm_weights(spec, seed=21)
            eng = loaded(E, spec, w, 0, kv_pool_tokens=256 * 48)
            _models[name] = (K.Model(K.Abi(E.lib(), eng._h, spec, "cpu"), spec, w, HIST), F, eng)
        return _models[name][:2]
    yield get
    for m, _, eng in _models.values():
        m.abi.close()
        eng.close()
    _models.clear()


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_unit_equals_step_and_sample(model, name):
    K.case_one_unit(*model(name))


@pytest.mark.parametrize("name", list(SHAPES))
def test_last_unit_bit_equal_every_unit_in_band(model, name):
    m, F = model(name)
    K.case_units_last_bit_equal(m, F, tag=f"emul stream_steps {name}")


def test_four_units_of_five_rows_block_path_hd64(model):
    m, _ = model("hd64-12rows")
    K.case_units_last_bit_equal(m, 4, units=4, tag="emul stream_steps hd64 4 x 5 rows")


@pytest.mark.parametrize("name", list(SHAPES))
def test_commit_leaves_the_kept_unit_last(model, name):
    K.case_commit_state(*model(name))


@pytest.mark.parametrize("name", list(SHAPES))
def test_discarded_rows_are_never_read(model, name):
    m, F = model(name)
    K.case_discarded_rows_unread(m, F, tag=f"emul stream_steps discarded {name}")


def test_page_comes_back_with_the_commit(E):
    spec, F = TINY_GQA, 4
    w = O.init_llm_weights(spec, seed=22)
    eng = loaded(E, spec, w, 0, kv_pool_tokens=256 * 3)
    abi = K.Abi(E.lib(), eng._h, spec, "cpu")
    try:
        K.case_page_boundary(abi, spec, O.LlamaOracle(spec, w, torch.bfloat16), 11, F, L=248)     # 248 + 5 = 253 <= 256 < 248 + 15
    finally:
        abi.close()
        eng.close()


def test_refusals_leave_the_session_unchanged(model):
    K.case_refusals(*model("hd64-12rows"))


def test_tensor_parallel_engine_refused(E):
    spec = TINY
    w = O.init_llm_weights(spec, seed=23)
    eng = E.EmulEngine(spec, kv_pool_tokens=1024, tp_rank=0, tp_size=2).load_weights(w, O.rope_inv_freq(spec.head_dim, spec.rope_theta))
    abi = K.Abi(E.lib(), eng._h, spec, "cpu")
    try:
        K.case_tensor_parallel_refused(abi, spec)
    finally:
        abi.close()
        eng.close()


# ---- other storage formats: the last unit (block path, 18 rows) equals vlo_llm_step over the same rows -----------------------------------------
def _format_engine(E, fmt):
    from videollm_online_amd.checkpoint import quantize_fp8_per_channel
    if fmt == "kv_fp8":
        spec = TINY_HD128
        w = O.init_llm_weights(spec, seed=24)
        return spec, loaded(E, spec, w, 1, ([0.11, 0.6], [0.45, 0.093]), kv_pool_tokens=1024), w
    if fmt == "w_fp8":
        spec = O.LlmSpec(512, 512, 1, 4, 1, 256, 10000.0, 1e-5, vision_hidden_size=128)      # K = 512: the smallest the fp8 image takes
        w = O.init_llm_weights(spec, seed=25)
        eng_w = {}
        for k, v in w.items():
            if k.endswith(O.FP8_STREAMED):
                eng_w[k], eng_w[k + "_scale"] = quantize_fp8_per_channel(v)
            else:
                eng_w[k] = v
        return spec, E.EmulEngine(spec, kv_pool_tokens=1024, weight_dtype=1).load_weights(eng_w, O.rope_inv_freq(spec.head_dim, spec.rope_theta)), w
    from tests.test_emul_mxfp4_cpu import TOY, make_engine, quantized
    spec = TOY
    w = O.init_llm_weights(spec, seed=26)
    eng_w, _, _ = quantized(w, "mxfp4")                    # (K = 128: the fp8 image of an lm_head needs K >= 512)
    return spec, make_engine(E, spec).load_weights(eng_w, O.rope_inv_freq(spec.head_dim, spec.rope_theta)), w


@pytest.mark.parametrize("fmt", ["kv_fp8", "w_fp8", "w_mxfp4"])
def test_other_storage_formats_last_unit_bit_equal(E, fmt):
    spec, eng, w = _format_engine(E, fmt)
    abi = K.Abi(E.lib(), eng._h, spec, "cpu")
    try:
        K.case_units_last_bit_equal(K.Model(abi, spec, w, 20), 5, band=False)
    finally:
        abi.close()
        eng.close()


def test_steps_input_equals_step_input(model):
    m, F = model("hd64-12rows")
    K.case_steps_input(m.abi, m.spec, F)
