"""The C-level cases of the stream lookahead (include/vlo.h vlo_stream_steps / vlo_stream_steps_commit / vlo_steps_input), written once against the
C ABI and run twice: tests/test_emul_stream_steps_cpu.py on the emulated library (host tensors), tests/test_gpu_stream_steps.py on libvlo.so
(cuda tensors, the null stream).  Not a test module itself.

A unit is one frame step's input: [interval id] + F frame rows.  The parity rule: what the pass and vlo_llm_step compute over the SAME rows on
the SAME path (16-row pipeline up to 16 rows, block path above) is bit-equal — the last unit's logits and every K / V row; an earlier unit's
logits are held to the project's 3-way band (tests/parity_util.py) against the oracle stepped unit by unit."""
import ctypes as C

import torch

from oracle import vlo_oracle as O
from tests.parity_util import within_band

E_INVALID, E_NOMEM, E_STATE = -1, -3, -4


def bits(t):
    return t.contiguous().view(torch.int16)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Abi:
    """One engine of one loaded library, driven through include/vlo.h with tensors on ``device``."""

    def __init__(self, lib, engine_handle, spec, device):
        self.L, self.h, self.spec, self.dev = lib, engine_handle, spec, device
        self.sessions = []

    def err(self):
        return self.L.vlo_last_error().decode()

    def ok(self, rc):
        assert rc == 0, (rc, self.err())

    def new_session(self):
        h = C.c_void_p()
        self.ok(self.L.vlo_session_create(self.h, 0, C.byref(h)))
        self.sessions.append(h)
        return h

    def fork_rc(self, s, n):
        h = C.c_void_p()
        rc = self.L.vlo_session_fork(s, n, C.byref(h), None)
        if rc == 0:
            self.sessions.append(h)
        return rc, h

    def fork(self, s, n=None):
        rc, h = self.fork_rc(s, self.len(s) if n is None else n)
        self.ok(rc)
        return h

    def len(self, s):
        return int(self.L.vlo_session_len(s))

    def close(self):
        for s in self.sessions:
            self.L.vlo_session_destroy(s)
        self.sessions = []

    def step_rc(self, s, x, want_all=False):
        x = x.to(self.dev, torch.bfloat16).contiguous()
        n, V = x.shape[0], self.spec.vocab_size
        last = torch.zeros(V, dtype=torch.bfloat16, device=self.dev)
        allr = torch.zeros(n, V, dtype=torch.bfloat16, device=self.dev) if want_all else None
        rc = self.L.vlo_llm_step(s, _ptr(x), n, _ptr(last), _ptr(allr), None)
        return rc, last.cpu(), (allr.cpu() if want_all else None)

    def step(self, s, x, want_all=False):
        rc, last, allr = self.step_rc(s, x, want_all)
        self.ok(rc)
        return last, allr

    def sample_rc(self, s, thr, iid):
        tok = torch.zeros(1, dtype=torch.long, device=self.dev)
        p = torch.zeros(1, dtype=torch.float32, device=self.dev)
        rc = self.L.vlo_stream_sample(s, thr, iid, _ptr(tok), _ptr(p), None)
        return rc, int(tok.cpu()), float(p.cpu())

    def steps_rc(self, s, x, ends, thr, iid, n=None, units=None):
        """(rc, tok [units], p [units], n_accept) of vlo_stream_steps; ``n`` / ``units`` override the counts handed to the call (refusals)"""
        x = x.to(self.dev, torch.bfloat16).contiguous()
        u = len(ends) if units is None else units
        tok = torch.full((max(u, 1),), -7, dtype=torch.long, device=self.dev)
        p = torch.zeros(max(u, 1), dtype=torch.float32, device=self.dev)
        acc = torch.full((1,), -7, dtype=torch.int32, device=self.dev)
        arr = (C.c_int * max(len(ends), 1))(*ends)
        rc = self.L.vlo_stream_steps(s, _ptr(x), x.shape[0] if n is None else n, arr, u, thr, iid, _ptr(tok), _ptr(p), _ptr(acc), None)
        return rc, tok.cpu().tolist(), p.cpu().tolist(), int(acc.cpu())

    def steps(self, s, x, ends, thr, iid):
        rc, tok, p, acc = self.steps_rc(s, x, ends, thr, iid)
        self.ok(rc)
        return tok, p, acc

    def commit_rc(self, s, keep):
        return self.L.vlo_stream_steps_commit(s, keep)

    def commit(self, s, keep):
        self.ok(self.commit_rc(s, keep))

    def logits_rows(self, s, units):
        """rows [units][vocab] of the session's logits buffer (vlo_debug_read which = 5)"""
        out = torch.zeros(units, self.spec.vocab_size, dtype=torch.bfloat16, device=self.dev)
        self.ok(self.L.vlo_debug_read(s, 5, _ptr(out), out.numel() * 2, None))
        return out.cpu()

    def kv_rc(self, s, layer, which, h, t0, t1):
        out = torch.zeros(t1 - t0, self.spec.head_dim, dtype=torch.bfloat16, device=self.dev)
        rc = self.L.vlo_session_read_kv(s, layer, which, h, t0, t1, _ptr(out), None)
        return rc, out.cpu()

    def kv(self, s, t0=0, t1=None):
        t1 = self.len(s) if t1 is None else t1
        out = {}
        for layer in range(self.spec.num_layers):
            for which in (0, 1):
                for h in range(self.spec.num_kv_heads):
                    rc, t = self.kv_rc(s, layer, which, h, t0, t1)
                    self.ok(rc)
                    out[(layer, which, h)] = t
        return out

    def state(self, s, iid):
        """what a refused call must leave alone: length, every K / V row, the sampler's view of the last-row logits"""
        return self.len(s), self.kv(s), self.sample_rc(s, 0.0, iid)


def same_kv(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def same_state(a, b):
    assert a[0] == b[0] and a[2] == b[2], (a[0], b[0], a[2], b[2])
    same_kv(a[1], b[1])


def unit_rows(spec, ref, iid, seed, units, F):
    """``units`` step inputs of 1 + F rows each: the interval token's embedding, then F random frame rows"""
    g = torch.Generator().manual_seed(seed)
    head = ref.embed(torch.tensor([iid]))
    return [torch.cat([head, torch.randn(F, spec.hidden_size, generator=g).bfloat16()]) for _ in range(units)]


def ends_of(xs):
    out, r = [], 0
    for x in xs:
        r += x.shape[0]
        out.append(r - 1)
    return out


class Model:
    """An engine (Abi), its oracles, and one session filled with ``hist_len`` rows; the oracles' caches after the same rows."""

    def __init__(self, abi, spec, w, hist_len, seed=1, keep_fp32=(), oracle_w=None):
        self.abi, self.spec = abi, spec
        ow = w if oracle_w is None else oracle_w
        self.ref, self.gold = O.LlamaOracle(spec, ow, torch.bfloat16, keep_fp32=keep_fp32), O.LlamaOracle(spec, ow, torch.float32)
        self.iid = O.default_tokens(spec).interval_id
        self.hist = torch.randn(hist_len, spec.hidden_size, generator=torch.Generator().manual_seed(seed)).bfloat16()
        self.s = abi.new_session()
        abi.step(self.s, self.hist)
        self._caches = None

    def caches(self):
        """fresh copies of the (bf16 reference, fp32 gold) caches after the history"""
        if self._caches is None:
            n = self.hist.shape[0]
            _, rc = self.ref.forward(self.hist, None, logits_from=n)
            _, gc = self.gold.forward(self.hist.float(), None, logits_from=n)
            self._caches = (rc, gc)
        L = self.hist.shape[0]
        return O.cache_prefix(self._caches[0], L), O.cache_prefix(self._caches[1], L)

    def band(self, tag, got, rl, gl):
        e = (got.float() - gl).abs().max().item()
        r = (rl.float() - gl).abs().max().item()
        print(f"[{tag}] engine err {e:.4g} ref-bf16 err {r:.4g}")
        assert within_band(e, r, 1e-3 * gl.abs().max().item(), tag), (tag, e, r)


# ---- 1. one unit equals vlo_llm_step + vlo_stream_sample --------------------------------------------------------------------------------
def case_one_unit(m, F, thr=0.3):
    A = m.abi
    (x,) = unit_rows(m.spec, m.ref, m.iid, 11, 1, F)
    a, b = A.fork(m.s), A.fork(m.s)
    L = A.len(a)
    assert L > 0
    tok, p, acc = A.steps(a, x, [F], thr, m.iid)
    assert A.len(a) == L                                   # pending: the old length
    A.commit(a, 1)
    last, _ = A.step(b, x)
    rc, tok_b, p_b = A.sample_rc(b, thr, m.iid)
    assert rc == 0 and A.len(a) == A.len(b) == L + 1 + F
    assert torch.equal(bits(A.logits_rows(a, 1)[0]), bits(last))
    assert (tok[0], p[0]) == (tok_b, p_b)
    assert acc == 1
    same_kv(A.kv(a), A.kv(b))


# ---- 2. several units: the last unit and all K / V equal vlo_llm_step over the same rows; every unit inside the band ------------------------
def case_units_last_bit_equal(m, F, units=3, band=True, tag="stream_steps"):
    A = m.abi
    xs = unit_rows(m.spec, m.ref, m.iid, 12, units, F)
    x, ends = torch.cat(xs), ends_of(xs)
    a, b = A.fork(m.s), A.fork(m.s)
    L = A.len(a)
    A.steps(a, x, ends, 0.3, m.iid)
    A.commit(a, units)
    rows = A.logits_rows(a, units)
    last, _ = A.step(b, x)
    assert A.len(a) == A.len(b) == L + x.shape[0]
    assert torch.equal(bits(rows[-1]), bits(last)), (rows[-1].float() - last.float()).abs().max()
    same_kv(A.kv(a, L), A.kv(b, L))
    if band:
        rc, gc = m.caches()
        for k, xk in enumerate(xs):
            rl, rc = m.ref.forward(xk, rc)
            gl, gc = m.gold.forward(xk.float(), gc)
            m.band(f"{tag} unit {k} of {units} x {1 + F} rows", rows[k], rl[-1], gl[-1])
    return rows


# ---- 3. commit(keep) leaves the session at unit keep - 1 ------------------------------------------------------------------------------------
def case_commit_state(m, F, units=3):
    A = m.abi
    xs = unit_rows(m.spec, m.ref, m.iid, 13, units, F)
    x, ends = torch.cat(xs), ends_of(xs)
    probe = A.fork(m.s)
    tok0, p0, _ = A.steps(probe, x, ends, 0.0, m.iid)
    A.commit(probe, units)
    # an interval id that makes unit 0 silent at threshold 0 (its own argmax), and a threshold above its probability that makes it speak
    iid = tok0[0]
    for thr in (0.0, 2.0):
        want_acc = None
        for keep in (range(1, units + 1) if thr == 0.0 else (units,)):
            s = A.fork(m.s)
            L = A.len(s)
            tok, p, acc = A.steps(s, x, ends, thr, iid)
            restated = next((k + 1 for k in range(units) if tok[k] != iid), units)
            assert acc == restated, (tok, iid, acc)
            want_acc = acc if want_acc is None else want_acc
            assert acc == want_acc
            A.commit(s, keep)
            assert A.len(s) == L + ends[keep - 1] + 1
            rc, t, pp = A.sample_rc(s, thr, iid)
            assert rc == 0 and (t, pp) == (tok[keep - 1], p[keep - 1]), (keep, t, pp, tok, p)
        if thr == 0.0:
            assert tok[0] == iid and want_acc == next((k + 1 for k in range(units) if tok0[k] != iid), units)
        else:
            assert want_acc == 1                            # p[interval] < 2 always: zeroed, unit 0 speaks


# ---- 4. rows of discarded units are never read again ----------------------------------------------------------------------------------------
def case_discarded_rows_unread(m, F, tag="stream_steps discarded"):
    A = m.abi
    x0, x1 = unit_rows(m.spec, m.ref, m.iid, 14, 2, F)
    s = A.fork(m.s)
    L = A.len(s)
    x = torch.cat([x0, x0 * 8, x0 * 8])
    A.steps(s, x, ends_of([x0, x0, x0]), 0.3, m.iid)
    A.commit(s, 1)
    assert A.len(s) == L + 1 + F
    last, _ = A.step(s, x1)
    rc, gc = m.caches()
    for xk in (x0, x1):
        rl, rc = m.ref.forward(xk, rc)
        gl, gc = m.gold.forward(xk.float(), gc)
    m.band(tag, last, rl[-1], gl[-1])


# ---- 5. a page taken by the pass comes back with the commit ---------------------------------------------------------------------------------
def case_page_boundary(abi, spec, ref, iid, F, L, page=256):
    """``abi``: an engine whose pool holds exactly 3 pages.  A at L tokens and B just below the boundary hold one page each; the pass of A takes
    the last free page, commit(1) ends below the boundary and hands it back."""
    A = abi
    xs = unit_rows(spec, ref, iid, 15, 3, F)
    x, ends = torch.cat(xs), ends_of(xs)
    assert L + ends[0] + 1 <= page < L + x.shape[0]
    g = torch.Generator().manual_seed(16)
    a = A.new_session()
    A.step(a, torch.randn(L, spec.hidden_size, generator=g).bfloat16())
    b = A.new_session()
    A.step(b, torch.randn(page - 4, spec.hidden_size, generator=g).bfloat16())
    xb = torch.randn(1 + F, spec.hidden_size, generator=g).bfloat16()
    assert F + 1 > 4
    A.steps(a, x, ends, 0.3, iid)
    rc, _, _ = A.step_rc(b, xb)
    assert rc == E_NOMEM, (rc, A.err())
    assert A.len(b) == page - 4
    A.commit(a, 1)
    assert A.len(a) == L + ends[0] + 1
    A.step(b, xb)
    assert A.len(b) == page - 4 + 1 + F
    # ... and with the pool full again a pass that needs a page fails whole
    before = A.len(a)
    rc, _, _, _ = A.steps_rc(a, x, ends, 0.3, iid)
    assert rc == E_NOMEM and A.len(a) == before
    assert A.commit_rc(a, 1) == E_STATE                     # nothing is pending after the refusal


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def case_refusals(m, F):
    A, iid = m.abi, m.iid
    xs = unit_rows(m.spec, m.ref, iid, 17, 3, F)
    x, ends = torch.cat(xs), ends_of(xs)
    n = x.shape[0]
    s = A.fork(m.s)
    A.step(s, xs[0])                                        # a session that holds logits
    before = A.state(s, iid)

    def refused(code, *a, **k):
        rc = A.steps_rc(s, *a, **k)[0]
        assert rc == code, (rc, A.err(), a[1:], k)
        assert A.len(s) == before[0] and A.commit_rc(s, 1) == E_STATE     # (K / V and logits: compared once, after all of them)

    refused(E_INVALID, x, [ends[1], ends[0], ends[2]], 0.3, iid)          # not ascending
    refused(E_INVALID, x, [ends[0], ends[0], ends[2]], 0.3, iid)          # not strictly
    refused(E_INVALID, x, [ends[0], ends[1], n - 2], 0.3, iid)            # last entry not n - 1
    refused(E_INVALID, x, [ends[0], ends[1], n], 0.3, iid)                # past the rows
    big = torch.zeros(65, m.spec.hidden_size, dtype=torch.bfloat16)
    refused(E_INVALID, big, [10, 64], 0.3, iid)                           # n = 65
    refused(E_INVALID, big, list(range(17)), 0.3, iid, n=17)              # units = 17
    refused(E_INVALID, x, ends, 0.3, iid, n=0)
    refused(E_INVALID, x, ends, 0.3, iid, units=0)
    refused(E_INVALID, x, ends, 0.3, m.spec.vocab_size)                   # interval id outside the vocabulary
    assert A.commit_rc(s, 1) == E_STATE                                   # no pass pending
    same_state(A.state(s, iid), before)

    # while a pass is pending every other call is VLO_E_STATE and changes nothing: the twin commits the same pass undisturbed
    twin, s2 = A.fork(s), A.fork(s)
    L = A.len(s2)
    tok, p, acc = A.steps(s2, x, ends, 0.3, iid)
    tok_t, p_t, acc_t = A.steps(twin, x, ends, 0.3, iid)
    assert (tok, p, acc) == (tok_t, p_t, acc_t)
    assert A.len(s2) == L
    assert A.step_rc(s2, xs[0])[0] == E_STATE
    assert A.sample_rc(s2, 0.3, iid)[0] == E_STATE
    assert A.fork_rc(s2, L)[0] == E_STATE
    assert A.L.vlo_session_crop(s2, L - 1) == E_STATE
    assert A.L.vlo_session_evict(s2, 1, 2, None) == E_STATE
    assert A.kv_rc(s2, 0, 0, 0, 0, 1)[0] == E_STATE
    assert A.steps_rc(s2, x, ends, 0.3, iid)[0] == E_STATE
    assert "pending" in A.err()
    ids = torch.zeros(4, dtype=torch.long, device=A.dev)
    nw = C.c_int(0)
    xg = xs[0].to(A.dev)
    assert A.L.vlo_greedy_generate(s2, _ptr(xg), xg.shape[0], -1, _ptr(ids), 4, 0, C.byref(nw), None) == E_STATE
    for keep in (0, 4, -1):
        assert A.commit_rc(s2, keep) == E_INVALID
    assert A.len(s2) == L
    A.commit(s2, 2)
    A.commit(twin, 2)
    same_state(A.state(s2, iid), A.state(twin, iid))
    assert A.len(s2) == L + ends[1] + 1

    # reset while pending drops the pass
    s3 = A.fork(s)
    A.steps(s3, x, ends, 0.3, iid)
    A.ok(A.L.vlo_session_reset(s3))
    assert A.len(s3) == 0 and A.commit_rc(s3, 1) == E_STATE
    last, _ = A.step(s3, m.hist)                                          # the session is usable again, from empty
    ref_last, _ = A.step(A.new_session(), m.hist)
    assert torch.equal(bits(last), bits(ref_last))


def case_tensor_parallel_refused(abi, spec):
    """``abi``: rank 0 of a tp_size = 2 engine"""
    s = abi.new_session()
    x = torch.zeros(4, spec.hidden_size, dtype=torch.bfloat16)
    rc = abi.steps_rc(s, x, [3], 0.3, 5)[0]
    assert rc == E_STATE and "tensor-parallel" in abi.err()
    assert abi.len(s) == 0


# ---- 8. vlo_steps_input equals `units` calls of vlo_step_input -------------------------------------------------------------------------------
def case_steps_input(abi, spec, F):
    A, H, V = abi, spec.hidden_size, spec.vocab_size
    g = torch.Generator().manual_seed(18)

    def steps_input_rc(ids_per_unit, frames, rows_per_unit):
        ks = [len(u) for u in ids_per_unit]
        flat = [i for u in ids_per_unit for i in u]
        total = sum(ks) + len(ks) * rows_per_unit
        out = torch.zeros(max(total, 1), H, dtype=torch.bfloat16, device=A.dev)
        rc = A.L.vlo_steps_input(A.h, (C.c_int64 * max(len(flat), 1))(*flat), (C.c_int * max(len(ks), 1))(*ks), len(ks),
                                 _ptr(frames) if rows_per_unit else None, rows_per_unit, _ptr(out), None)
        return rc, out.cpu()

    def step_input(ids, frame):
        rows = 0 if frame is None else frame.shape[0]
        out = torch.zeros(len(ids) + rows, H, dtype=torch.bfloat16, device=A.dev)
        A.ok(A.L.vlo_step_input(A.h, (C.c_int64 * max(len(ids), 1))(*ids), len(ids), _ptr(frame), rows, _ptr(out), None))
        return out.cpu()

    rnd = lambda k: torch.randint(0, V, (k,), generator=g).tolist()
    for ids in ([rnd(19), [11], [11], [11]], [rnd(32), rnd(4), rnd(1), rnd(4), rnd(2)], [[V + 5], [-3]], [rnd(1)] * 16, [[], rnd(2)]):
        frames = torch.randn(len(ids) * F, H, generator=g).bfloat16().to(A.dev)
        rc, got = steps_input_rc(ids, frames, F)
        assert rc == 0, A.err()
        want = torch.cat([step_input(u, frames[k * F:(k + 1) * F]) for k, u in enumerate(ids)])
        assert torch.equal(bits(got), bits(want)), [len(u) for u in ids]
    ids = [rnd(3), rnd(2)]
    rc, got = steps_input_rc(ids, None, 0)                                # ids only
    assert rc == 0 and torch.equal(bits(got), bits(torch.cat([step_input(u, None) for u in ids])))
    frames = torch.randn(17 * F, H, generator=g).bfloat16().to(A.dev)
    for bad in ([rnd(33)], [rnd(3), rnd(5)], [rnd(1)] * 17, []):
        assert steps_input_rc(bad, frames, F)[0] == E_INVALID, [len(u) for u in bad]
    assert steps_input_rc([[], []], None, 0)[0] == E_INVALID              # a unit without a row
