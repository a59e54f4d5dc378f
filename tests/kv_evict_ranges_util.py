"""Eviction of several KV ranges in one pass (include/vlo.h vlo_session_evict_ranges), restated in torch on top of tests/kv_evict_util.py.

The rule: ranges [a_j, b_j) (ascending, disjoint, coordinates before the call) leave the cache.  The survivors keep their order; the run behind
range j — source positions [b_j, a_{j+1}), the last one ending at len — moves down by D_j = sum_{i <= j} (b_i - a_i) slots and its stored keys
are rotated back by D_j positions with kv_evict_util.rerotate: ONE bf16 rounding of the fp32 result, whatever the number of ranges below.
Positions below a_0 are untouched.  V moves bit for bit."""
import torch

from oracle import vlo_oracle as O
from tests.kv_evict_util import bits, rerotate
from tests.parity_util import bf16_ulp


def normalize(ranges):
    """drop empty ranges, merge touching ones (what the engine does before it counts them)"""
    out = []
    for a, b in ranges:
        if a == b:
            continue
        if out and out[-1][1] == a:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def segments(ranges, length):
    """[(src0, src1, D_j)]: the survivor runs behind each range (empty ones left out) and their shifts"""
    rs = normalize(ranges)
    out, D = [], 0
    for j, (a, b) in enumerate(rs):
        D += b - a
        end = rs[j + 1][0] if j + 1 < len(rs) else length
        if end > b:
            out.append((b, end, D))
    return out


def evicted_k(k, ranges, inv_freq, dim=0):
    """k [..., T, hd] with T on `dim` (bf16: one rounding per survivor; fp32: none) after the eviction"""
    rs = normalize(ranges)
    if not rs:
        return k
    parts = [k.narrow(dim, 0, rs[0][0])]
    for s0, s1, D in segments(rs, k.shape[dim]):
        parts.append(rerotate(k.narrow(dim, s0, s1 - s0), D, inv_freq))
    return torch.cat(parts, dim=dim)


def evicted_v(v, ranges, dim=0):
    keep = torch.ones(v.shape[dim], dtype=torch.bool)
    for a, b in ranges:
        keep[a:b] = False
    return v.index_select(dim, keep.nonzero().flatten())


def evict_ranges_oracle_cache(cache: O.KVCacheOracle, ranges, inv_freq: torch.Tensor) -> O.KVCacheOracle:
    """the same eviction on the oracle's cache (k, v: [kvh, T, hd] per layer), in the cache's own dtype"""
    out = O.KVCacheOracle(len(cache.k))
    for i, (k, v) in enumerate(zip(cache.k, cache.v)):
        out.k[i] = evicted_k(k, ranges, inv_freq, dim=1)
        out.v[i] = evicted_v(v, ranges, dim=1)
    return out


def evicted_kv(before, ranges, inv_freq):
    """the restatement applied to a {(layer, which, kv_head): bf16 [len, hd]} dictionary as read with vlo_session_read_kv"""
    return {key: (evicted_v(t, ranges) if key[1] == 1 else evicted_k(t, ranges, inv_freq)) for key, t in before.items()}


def check_kv_after_evict_ranges(tag, before, after, ranges, inv_freq, want=None):
    """before / after: {(layer, which, kv_head): bf16 [len, hd]} around ONE evict_ranges call (`want`: the expected dictionary when it is not
    the restatement applied once to `before`).  tests/kv_evict_util.py check_kv_after_evict's conditions: V bit-equal to V with the ranges
    deleted; K below a_0 bit-equal; every moved K element within 1 bf16 ulp of the restatement and at least 99 % of them bit-equal (the
    engine evaluates the rule as written, as torch does, so 100 % is expected; the share is printed)."""
    rs = normalize(ranges)
    want = evicted_kv(before, rs, inv_freq) if want is None else want
    d = sum(b - a for a, b in rs)
    a0 = rs[0][0] if rs else 0
    n_eq = n_all = 0
    for (layer, which, h), b in before.items():
        a, w = after[(layer, which, h)], want[(layer, which, h)]
        assert a.shape[0] == b.shape[0] - d == w.shape[0], (tag, a.shape, b.shape, d)
        if which == 1:
            assert torch.equal(bits(a), bits(w)), (tag, "V", layer, h)
            continue
        assert torch.equal(bits(a[:a0]), bits(w[:a0])), (tag, "K below a_0", layer, h)
        got, exp = a[a0:], w[a0:]
        err = (got.float() - exp.float()).abs()
        ulp = bf16_ulp(torch.maximum(got.float().abs(), exp.float().abs()))
        assert bool((err <= ulp).all()), (tag, "K", layer, h, (err / ulp).max().item())
        n_eq += int((bits(got) == bits(exp)).sum())
        n_all += got.numel()
    share = n_eq / max(n_all, 1)
    print(f"[kv evict ranges {tag}] {len(rs)} ranges, {d} tokens: re-rotated K bit-equal to the torch rule: {share:.4%} of {n_all}")
    assert n_all == 0 or share >= 0.99, (tag, share)


def ranges_arg(ranges):
    """[(a, b), ...] -> (ctypes int64 [n][2], n) for the C entry points"""
    import ctypes as C
    flat = [int(v) for r in ranges for v in r]
    return (C.c_int64 * max(len(flat), 1))(*flat), len(ranges)


SET_A = [(19, 30), (41, 52), (63, 74)]                       # runs of 11 tokens; shifts 11 / 22 / 33: odd and even sh
SET_B = [(7, 8), (9, 10), (11, 12)]                          # one-token runs: three shifts inside one 8-token V^T vector
