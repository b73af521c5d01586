"""Planted-key probes of the attention kernels at every dispatch and key edge (`pytest -m gpu`).

attn_body / attn_kernel, attn_combine_kernel, attn_oproj_kernel and attn_prefill_kernel through Session.forward,
sd_batch_forward, sd_session_forward_tree and the fp8 arena, on the one-layer probe models of tests/attn_probe.py: a
filler context with ONE marker key that owns > 99 % of the softmax row of every query that may see it.  The layouts, their
classes of marker position and the branches they sit on come from attn_probe (test_attn_probe_cpu.py shows on the oracle
alone that losing or leaking the marker moves the probed row by >= 20x the bar used here, and pins the dispatch
arithmetic).

Bars, none taken from the code under test: fp32 - max-abs 1e-3 against the fp32 oracle (north_star); 16-bit and fp8 -
_assert_within_reference_error of test_gpu_production_parity: HIP's error against the fp32 oracle at most 1.5x the
same-dtype oracle's own (+ the helper's absolute terms), per layout over all its logit rows; with the fp8 arena the
same-dtype oracle carries models_ref._kv_fp8's emulation with the arena's scales folded in (attn_probe.fp8_scaled_sd; its
error against the fp32 oracle on these layouts, measured on the CPU: at most 0.186, at D = 32, see test_attn_probe_cpu.py's
printout - the 1.5x rule holds unchanged, no separate fp8 number is needed).  Every fp8 arena gets NON-UNIT scales
(attn_probe.fp8_scales: powers of two, K's and V's different per head), so a scale that is dropped, or taken from the wrong
(k|v, head) entry, changes scores or outputs by a factor of 2 or more.

Rows that may not see the marker (forbidden-key layouts: the key just behind the probed row - a later row of the call, or
the stale arena slot behind the call's last row; a non-ancestor tree node) must ALSO be bit-identical to a run with the
filler in the marker's place.  That run happens in a second, fresh session of the same type which receives exactly the same
sequence of calls with F for M, so every arena slot a probed row may read holds the same bits in both.

Every test builds its model once, keeps ONE arena and re-plants keys by position (layer 0's K / V rows depend on token and
position alone), so a layout costs a few launches and one n-row oracle forward."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import attn_probe as P
from test_gpu_production_parity import _assert_within_reference_error

pytestmark = pytest.mark.gpu

_ORACLES = {}
_SD = {}


def _sd(name):
    if name not in _SD:
        _SD[name] = P.probe_state_dict(name)
    return _SD[name]


def _oracle(name, dt, kvq=None):
    key = (name, dt, kvq)
    if key not in _ORACLES:
        _ORACLES[key] = P.ProbeOracle(name, P.DTYPES[dt], kvq, sd=_sd(name))
    return _ORACLES[key]


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine)


class _Env:
    """Tunables are sampled when a session is created: set them around the creation (and the runs), always restore."""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Runner:
    """One model + one arena.  `slots` mirrors which token's K / V row every arena slot holds; a layout re-plants only the
    slots that differ (runs of consecutive positions, n_logits = 0).  with_marker = False feeds F wherever the layout has
    M - the same calls otherwise.  max_seq: arena slots (attn_probe.MAX_SEQ unless given)."""

    def __init__(self, hip, name, dt, kv_dtype=None, with_marker=True, model=None, max_seq=None):
        self.hip, self.cfg = hip, P.probe_config(name)
        self.max_seq = P.MAX_SEQ if max_seq is None else max_seq
        dtype = P.DTYPES[dt]
        self.m = model or hip.engine.SpecDecModel.from_state_dict(self.cfg, P.cast_sd(_sd(name), dtype), dtype=dtype)
        self.ses = self.m.new_session(self.max_seq, kv_dtype=kv_dtype)
        if kv_dtype == "fp8":                                      # before any row is stored: the store divides by the scale
            sc = P.fp8_scales(name).to(self.ses.kv_scale.device)
            assert sc.shape == self.ses.kv_scale.shape
            self.ses.kv_scale.copy_(sc)
            torch.cuda.synchronize()
        self.with_marker = with_marker
        self.slots = np.full(self.max_seq, -1, dtype=np.int64)

    def _dev(self, toks):
        t = np.array(toks, dtype=np.int64)
        if not self.with_marker:
            t[t == P.M_TOK] = P.F_TOK
        return torch.from_numpy(t.astype(np.int32)).cuda()

    def plant(self, want, lo, hi):
        idx = np.nonzero(self.slots[lo:hi] != want[lo:hi])[0] + lo
        if idx.size == 0:
            return
        for run in np.split(idx, np.nonzero(np.diff(idx) > 1)[0] + 1):
            a, b = int(run[0]), int(run[-1]) + 1
            self.ses.forward(self._dev(want[a:b]), 0, pos0=a)
            self.slots[a:b] = want[a:b]

    def run(self, lay, n_logits=None):
        t = P.layout_tokens(lay)
        pos0 = lay.S - lay.n
        self.plant(t, 0, pos0)
        if lay.S < self.max_seq:
            self.plant(t, lay.S, lay.S + 1)                        # the stale slot behind the last key
        nl = lay.n if n_logits is None else n_logits
        out = self.ses.forward(self._dev(t[pos0:lay.S]), nl, pos0=pos0).float().cpu().clone()
        self.slots[pos0:lay.S] = t[pos0:lay.S]
        return out

    def run_tree(self, lay):
        t, pos, bits = P.tree_inputs(lay)
        self.plant(t, 0, lay.base)
        tok = self._dev(t[lay.base:])
        N = lay.N
        logits = torch.empty((N, self.cfg.vocab_size), dtype=torch.float32, device="cuda")
        self.hip.engine.check(self.hip.lib.sd_session_forward_tree(
            self.ses.handle, tok.data_ptr(), (C.c_int32 * N)(*[int(x) for x in pos]), (C.c_uint64 * N)(*bits), N, lay.base,
            logits.data_ptr(), logits.stride(0), torch.cuda.current_stream().cuda_stream), "sd_session_forward_tree")
        self.slots[lay.base:lay.base + N] = t[lay.base:]
        return logits.cpu()


class _Stats:
    def __init__(self, label):
        self.label, self.ratio, self.rms_ratio, self.e32, self.count, self.t0 = label, 0.0, 0.0, 0.0, 0, time.time()

    def judge(self, got, truth, ref16, what):
        """The file's bars for one layout's logit rows."""
        self.count += 1
        assert bool(torch.isfinite(got).all()), (self.label, what)
        if ref16 is None:
            e = float((got - truth).abs().max())
            self.e32 = max(self.e32, e)
            assert e <= P.FP32_TOL, (self.label, what, e)
            return
        errs = P.errors(got, ref16, truth)
        self.ratio = max(self.ratio, errs[0] / max(errs[1], 1e-9))
        self.rms_ratio = max(self.rms_ratio, errs[2] / max(errs[3], 1e-9))
        _assert_within_reference_error(errs, f"{self.label} {what}")

    def report(self):
        print(f"{self.label}: {self.count} layouts in {time.time() - self.t0:.1f} s; worst HIP / reference error ratio "
              f"max {self.ratio:.2f} rms {self.rms_ratio:.2f}; worst fp32 error {self.e32:.2e}")


def _run_causal(hip, label, name, dt, layouts, kvq=None, env=None, tail=None, check=None):
    """Every layout on a marker runner and on a filler runner (same calls, F for M), the marker runner's rows against the
    oracle, the rows in front of a forbidden key bit-identical between the two.  tail: logit rows per call (prefill)."""
    o32 = _oracle(name, "fp32")
    o16 = None if dt == "fp32" else _oracle(name, dt, kvq)
    st = _Stats(f"{label} {name} {dt}{' fp8-kv' if kvq else ''}")
    with _Env(**(env or {})):
        a = Runner(hip, name, dt, kv_dtype=kvq)
        b = Runner(hip, name, dt, kv_dtype=kvq, with_marker=False, model=a.m)
        if check is not None:                                      # (on both runners: they must see the same calls)
            check(a)
            check(b)
        for lay in layouts:
            nl = lay.n if tail is None else min(tail, lay.n)
            got, base = a.run(lay, nl), b.run(lay, nl)
            truth = o32.logits(lay)[lay.n - nl:]
            ref16 = None if o16 is None else o16.logits(lay)[lay.n - nl:]
            st.judge(got, truth, ref16, lay)
            if lay.cls == "forbidden":
                r = lay.probe - (lay.n - nl)
                assert torch.equal(got[:r + 1], base[:r + 1]), (st.label, lay, "rows in front of the forbidden key changed")
    st.report()


# --------------------------------------------------------------------------- a. causal decode and verify
@pytest.mark.parametrize("name,dt", P.CAUSAL_MODELS, ids=[f"{n}-{d}" for n, d in P.CAUSAL_MODELS])
def test_causal_planted_key_at_every_key_edge(hip, name, dt):
    """Default split settings; S in {1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 383, 384, 385, 511, 512, 513, 1025}
    visible keys, n in {1, 2, 3, 4, 5, 8, 9, 16} new rows (9 = groups of 8 + 1), the marker - one per run - at key 0, the
    last cached key, a row's own position, the key just behind a row (forbidden; behind the last row it is a stale arena
    slot, which the clamped loads must never read into a result), the first / last key of a split chunk, the first key past
    the V-prefetch window, key 255 and key 256.  Thinning (attn_probe.causal_layouts): every S meets every class with one
    n, n walking round-robin, then every (n, class) pair the walk missed is added at the smallest S where it exists - about
    100 layouts per model.  Branches: register softmax up to 256 (groups of 5..8 rows) / 512 keys, LDS beyond; half-wave
    (groups of 5..8 rows: `half = nr > 4`) and full-wave (<= 4 rows) softmax; pv 1 / 3 / 5 / 8; prefetch tail (D = 128, S 257..384); second MFMA K batch (> 256 keys per
    workgroup); split chunk edges at S >= 385; D = 16 bf16 takes the scalar score path; bf16 rows <= 4 the small path."""
    _run_causal(hip, "causal", name, dt, P.causal_layouts(P.head_dim(name)))


# --------------------------------------------------------------------------- b. alternative split settings
@pytest.mark.parametrize("name,dt", P.SPLIT_MODELS, ids=[f"{n}-{d}" for n, d in P.SPLIT_MODELS])
def test_causal_planted_key_under_other_split_settings(hip, name, dt):
    """SD_ATTN_SPLIT_KEYS / SD_ATTN_KEYS_PER_SPLIT = (64, 32) with S in {65, 96, 97, 250}, n in {1, 5, 8}: 32-key chunks,
    some wholly beyond the causal range of the group's first rows (their partial must be skipped by the combine);
    (4096, 256) with S in {512, 513, 600}, n in {1, 4, 5}: unsplit past both in-register limits (LDS softmax in full-wave, n <= 4,
    and half-wave, n = 5, form), past the D = 64 prefetch window (tail loop) and with a third MFMA K batch.  Every class of marker
    position that exists at a shape is run."""
    for (sk, kp), lays in P.split_cases(P.head_dim(name)):         # (the table test_attn_probe_cpu.py checks)
        _run_causal(hip, f"split({sk},{kp})", name, dt, lays, env=dict(SD_ATTN_SPLIT_KEYS=sk, SD_ATTN_KEYS_PER_SPLIT=kp))


# --------------------------------------------------------------------------- c. batched streams
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_batched_streams_planted_key_per_stream(hip, dt):
    """One sd_batch_forward over four streams with cache lengths (3, 390, 17, 256) and n_new drawn from {1, 5, 9}: the pass
    splits two ways (390 + n > 384 keys) and every group cuts its own keys in two 16-aligned chunks: the 3-key stream's
    second chunk is empty (s_hi == 0, loads clamped to the head's first key), the 17-key stream's holds 2..10 keys.  Marker per stream: key 0; the first key of the second chunk; the stale slot behind the last row
    (forbidden: bit-identical to the filler run); the last cached key (255).  Each stream against its own oracle forward."""
    name = "llama_d128"
    o32 = _oracle(name, "fp32")
    o16 = None if dt == "fp32" else _oracle(name, dt)
    st = _Stats(f"batch {name} {dt}")
    cfg, dtype = P.probe_config(name), P.DTYPES[dt]
    m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(_sd(name), dtype), dtype=dtype)
    for n_new in P.BATCH_NEW:
        lays = P.batch_layouts(n_new)
        outs = []
        for with_marker in (True, False):
            sess, seqs = [], []
            for lay in lays:
                t = P.layout_tokens(lay)
                if not with_marker:
                    t[t == P.M_TOK] = P.F_TOK
                dev = torch.from_numpy(t.astype(np.int32)).cuda()
                ses = m.new_session(448)
                ses.forward(dev[lay.S:lay.S + 1], 0, pos0=lay.S)    # the stale slot behind the stream's last row
                ses.forward(dev[:lay.S - lay.n], 0, pos0=0)
                assert ses.cache_len == lay.S - lay.n
                sess.append(ses)
                seqs.append(dev)
            out = hip.engine.batch_forward(sess, seqs, list(n_new), list(n_new)).float().cpu().clone()
            outs.append(torch.split(out, list(n_new)))
        for i, lay in enumerate(lays):
            st.judge(outs[0][i], o32.logits(lay), None if o16 is None else o16.logits(lay), (n_new, lay))
            if lay.cls == "forbidden":
                assert torch.equal(outs[0][i], outs[1][i]), (n_new, lay)
    st.report()


# --------------------------------------------------------------------------- d. tree
@pytest.mark.parametrize("name,dt,kvq", P.TREE_MODELS, ids=["fp32", "bf16", "bf16-fp8kv"])
def test_tree_planted_key_at_ancestor_and_non_ancestor_nodes(hip, name, dt, kvq):
    """sd_session_forward_tree, GQA D = 64: 9, 40 and 64 nodes behind 0, 1, 150 and 380 cached keys, unsplit (default
    settings; 380 + N splits two ways) and split into 32-key chunks (64, 32).  Marker at the probed node's root ancestor,
    at a non-ancestor node in front of it (forbidden: the node's row bit-identical to the filler run - visibility comes
    from g = s + kb - tree_base, wrong by one chunk or one node shows here), at the last cached key, and at node 63 (mask
    bit 63).  All N rows against the oracle's tree forward; fp8 arena on bf16 with non-unit scales
    (attn_probe.fp8_scales; base 380 + N splits, so both V-scale sites run) and the oracle's e4m3 emulation."""
    o32 = _oracle(name, "fp32")
    o16 = None if dt == "fp32" else _oracle(name, dt, kvq)
    for env in ({}, dict(SD_ATTN_SPLIT_KEYS=64, SD_ATTN_KEYS_PER_SPLIT=32)):
        st = _Stats(f"tree {'split(64,32)' if env else 'default'} {name} {dt}{' fp8-kv' if kvq else ''}")
        with _Env(**env):
            a = Runner(hip, name, dt, kv_dtype=kvq)
            b = Runner(hip, name, dt, kv_dtype=kvq, with_marker=False, model=a.m)
            for lay in P.tree_layouts():
                got, base = a.run_tree(lay), b.run_tree(lay)
                st.judge(got, P.tree_logits(o32, lay), None if o16 is None else P.tree_logits(o16, lay), lay)
                if lay.cls == "forbidden":
                    assert torch.equal(got[lay.probe], base[lay.probe]), (st.label, lay)
                if lay.cls == "node63":                            # no other node may see node 63
                    assert torch.equal(got[:63], base[:63]), (st.label, lay)
        st.report()


# --------------------------------------------------------------------------- e. fp8 KV, causal
@pytest.mark.parametrize("name", P.FP8_MODELS)
def test_fp8_kv_causal_planted_key(hip, name):
    """bf16 with the e4m3 arena, D in {32, 64, 128}, S in {17, 257, 385}, n in {1, 5}, every class that exists there: the
    arena's scales are non-unit and differ between K and V and between heads (attn_probe.fp8_scales, written into
    Session.kv_scale before the first row is stored), so the 1 / scale at the store, the K scale on the scores and the V scale
    at both of its sites - the unsplit epilogue (S = 17, 257; P.V from the prefetched rows and, at D = 128, S = 257, from the
    tail loop) and the split partials (S = 385) - each change the result by a factor >= 2 when missing or mis-indexed.
    Reference arithmetic: the bf16 oracle with models_ref._kv_fp8 on every new K / V row (as the TP8 test) and the scales
    folded into its weights; its own error against the fp32 oracle on these layouts is at most 0.186 (CPU measurement), and
    the project's 1.5x rule is used unchanged."""
    _run_causal(hip, "fp8", name, "bf16", P.fp8_layouts(P.head_dim(name)), kvq="fp8")


# --------------------------------------------------------------------------- f. fused attention + O
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_fused_attention_oproj_planted_key(hip, dt):
    """attn_oproj_kernel (one launch for attention + O; D = 128, <= 16 rows in <= 2 groups, s_max <= SD_ATTN_SPLIT_KEYS)
    on the layouts of (a) with S <= 384, and the same layouts through the two launches (SD_FUSE_ATTN_O=0) in a second
    session; both held to the oracle, not to each other.  Sessions are created under SD_SMALL_PATH=0 so that bf16 steps of
    <= 4 rows take forward_impl.  Route: the fused pass has one GEMM-class launch fewer than the two-launch pass (the O
    projection) and one attention-class launch in both (session profile)."""
    lays = P.fused_layouts()
    assert all(l.S <= 384 and l.n <= 16 for l in lays)
    counts = {}

    def route(tag):
        def check(r):
            r.run(P.Layout(300, 5, 0, 4, "key0"))
            r.ses.profile(True)
            r.run(P.Layout(300, 5, 0, 4, "key0"))
            prof = r.ses.profile_read()
            r.ses.profile(False)
            counts[tag] = (prof["gemm"][1], prof["attention"][1])
        return check
    _run_causal(hip, "fused attn+O", "llama_d128", dt, lays, env=dict(SD_SMALL_PATH=0), check=route("fused"))
    _run_causal(hip, "two launches", "llama_d128", dt, lays, env=dict(SD_SMALL_PATH=0, SD_FUSE_ATTN_O=0), check=route("two"))
    assert counts["fused"][1] == counts["two"][1] == 1 and counts["fused"][0] + 1 == counts["two"][0], counts


# --------------------------------------------------------------------------- g. matrix-core prefill attention
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_prefill_attention_planted_key(hip, dt):
    """attn_prefill_kernel (D = 128, 16-bit, >= 32 consecutive rows): ONE call of 81, 200 and 256 rows at pos0 0 and 37,
    logits of the last 64 rows (a one-layer model: the logits are the only observable of a prefill row, and enough).
    Marker at key 0, at pos0 - 1, at a probed row's own position and at its successor (forbidden, as a later row of the
    call and as the stale slot behind it).  Again with SD_PREFILL_ATTN=0 (attn_kernel's 8-row groups over the same rows).  Route: the
    session profile counts one attention-class launch either way, so it cannot tell the two kernels apart; what selects
    attn_prefill_kernel is prefill_attn_ok - SD_PREFILL_ATTN != 0, a 16-bit model, tab.contig (a call of more than
    SD_MAX_ROWS = 80 rows: hence 81), no tree, no fp8 arena, head_dim == 128, n_rows >= 32, and a score tile within the
    launch's LDS budget (keys <= 293 here)."""
    lays = P.prefill_layouts()
    _run_causal(hip, "prefill mfma", "llama_d128", dt, lays, env=dict(SD_PREFILL_ATTN=1), tail=64)
    _run_causal(hip, "prefill attn_kernel", "llama_d128", dt, lays, env=dict(SD_PREFILL_ATTN=0), tail=64)
