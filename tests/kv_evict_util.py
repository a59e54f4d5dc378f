"""KV eviction with RoPE re-rotation (include/vlo.h vlo_session_evict), restated in torch for the emulation and GPU tests.

The rule: forgetting cache positions [t0, t1) moves tokens [t1, len) down by d = t1 - t0 slots and rotates their stored (post-RoPE) keys
back by d positions, HF's half-split pairing, with c_i = (float)cos((double)d * inv_freq_f32[i]), s_i = (float)sin(...):
    k'[i] = k[i] c_i + k[i + hd/2] s_i        k'[i + hd/2] = k[i + hd/2] c_i - k[i] s_i
in fp32 from the stored values, rounded once to the cache's dtype.  V moves bit for bit."""
import torch

from oracle import vlo_oracle as O
from tests.parity_util import bf16_ulp, within_band


def rot_cs(d: int, inv_freq: torch.Tensor):
    a = float(d) * inv_freq.float().double()                         # float64 angles from the fp32 inv_freq
    return torch.cos(a).float(), torch.sin(a).float()


def rerotate(k: torch.Tensor, d: int, inv_freq: torch.Tensor) -> torch.Tensor:
    """k [..., hd] (bf16: one bf16 rounding of the fp32 result; fp32: no rounding) rotated back by d positions"""
    c, s = rot_cs(d, inv_freq)
    h = k.shape[-1] // 2
    k1, k2 = k[..., :h].float(), k[..., h:].float()
    return torch.cat([k1 * c + k2 * s, k2 * c - k1 * s], dim=-1).to(k.dtype)


def evict_oracle_cache(cache: O.KVCacheOracle, t0: int, t1: int, inv_freq: torch.Tensor) -> O.KVCacheOracle:
    """the same eviction on the oracle's cache (k, v: [kvh, T, hd] per layer), in the cache's own dtype"""
    out = O.KVCacheOracle(len(cache.k))
    for i, (k, v) in enumerate(zip(cache.k, cache.v)):
        out.k[i] = torch.cat([k[:, :t0], rerotate(k[:, t1:], t1 - t0, inv_freq)], dim=1)
        out.v[i] = torch.cat([v[:, :t0], v[:, t1:]], dim=1)
    return out


def bits(t):
    return t.contiguous().view(torch.int16)


def check_kv_after_evict(tag, before, after, t0, t1, inv_freq):
    """before / after: {(layer, which, kv_head): bf16 [len, hd]} read with vlo_session_read_kv around ONE eviction of [t0, t1).
    V: bit-equal to V with the range deleted.  K below t0: bit-equal.  K from t0 on against the torch restatement applied to the K read
    before: every element within 1 bf16 ulp (of the larger magnitude), at least 99 % bit-equal.  The engine evaluates the rule as written
    (two rounded fp32 products, one rounded sum, no fused multiply-add), as torch does here, so the share is expected to be 100 %; a fused
    evaluation would miss the 1-ulp bound wherever the two terms cancel."""
    d = t1 - t0
    n_eq = n_all = 0
    for (layer, which, h), b in before.items():
        a = after[(layer, which, h)]
        assert a.shape[0] == b.shape[0] - d
        if which == 1:
            assert torch.equal(bits(a), bits(torch.cat([b[:t0], b[t1:]]))), (tag, "V", layer, h)
            continue
        assert torch.equal(bits(a[:t0]), bits(b[:t0])), (tag, "K below t0", layer, h)
        want, got = rerotate(b[t1:], d, inv_freq), a[t0:]
        err = (got.float() - want.float()).abs()
        ulp = bf16_ulp(torch.maximum(got.float().abs(), want.float().abs()))
        assert bool((err <= ulp).all()), (tag, "K", layer, h, (err / ulp).max().item())
        n_eq += int((bits(got) == bits(want)).sum())
        n_all += got.numel()
    share = n_eq / max(n_all, 1)
    print(f"[kv evict {tag}] [{t0}, {t1}): re-rotated K bit-equal to the torch rule: {share:.4%} of {n_all}")
    assert n_all == 0 or share >= 0.99, (tag, share)


def band_check(tag, i, out, rl, gl):
    """the project's 3-way band: err(engine, fp32 gold) <= BAND * err(bf16 reference, fp32 gold) + 1e-3 * scale"""
    e = (out.float() - gl).abs().max().item()
    r = (rl.float() - gl).abs().max().item()
    scale = gl.abs().max().item()
    print(f"[kv evict {tag}] step {i}: engine err {e:.4g} ref-bf16 err {r:.4g} scale {scale:.3g}")
    assert within_band(e, r, 1e-3 * scale, f"kv_evict:{tag}"), f"{tag} step {i}: {e} vs {r}"


def step_inputs(spec, ref, toks, seed, lens):
    """embedding rows of steps of the given lengths: text ids first, random 'frame' rows after (as the neighbouring emulation tests build them)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        ids = torch.tensor([toks.interval_id] + toks.stream_prompt_ids + toks.stream_generation_ids)[:max(1, n - 10)]
        rows = [ref.embed(ids)]
        if n > len(ids):
            rows.append(torch.randn(n - len(ids), spec.hidden_size, generator=g).bfloat16())
        out.append(torch.cat(rows)[:n])
    return out
