"""The device-RNG decode loops are lossless (`pytest -m gpu`): the first M tokens they emit are distributed as the target
model's own sampling.  Every case draws N runs on a FIXED seed list (tests/lossless.py:CASES, SEED_BASE + i), classifies
them into the cells of the target tree and holds one Pearson X2 against the exact cell probabilities of the fp32 oracle.
Bars, dof, N and the planted defects each case can see were derived on the CPU (tests/test_lossless_cpu.py prints the
table); nothing here comes from the code under test.  gamma = 2, M = 4 throughout (M >= gamma + 2), random_seed = None.

A failed fit on a fixed seed list is deterministic - a finding.  Order of blame: tests/test_gpu_philox.py (the generator),
the kernel-level case there, the AR control below, then the loop.

16-bit: no filtered (top_k) case is admissible - tests/test_lossless_cpu.py finds no prompt whose k-th logit gap is 8x the
same-dtype oracle's logit error at every prefix - so the 16-bit cases run plain softmax with rank cells, against the
noncentral bar with noncentrality 2.25 * lambda_ref.  At their N the shared-uniform defect is NOT visible in 16-bit (the
fp32 cases see it); resample-from-p, resample-from-|p-q|, bonus-from-the-previous-row and p-one-row-early are.
lambda_ref is measured where the test runs, on the oracle in the engine's dtype: the host's bf16 matmul decides its last
digits (2.1 and 2.5 seen on two hosts for bf16_plain, bars 127.0 and 129.0), so the 16-bit bars below are "about".

Seconds in the docstrings: measured on an MI355X, where the existing queue tests (tests/test_gpu_spec_queue.py) take
0.1 - 0.4 s each; the tiny pairs run about 3000 (fp32) to 5000 (bf16) queue prompts a second, most of it host bookkeeping.

Out of scope: multi_speculative_sampling(strategy="iid") and the beam variant - the reference's "longest accepted replica
wins" rule is not distribution-preserving, so token parity with the oracle stays their check."""
import time

import numpy as np
import pytest
import torch

import lossless as LL

pytestmark = pytest.mark.gpu
SLOTS = 16


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


_ENGINES = {}


def _engines(hip, kind):
    if kind not in _ENGINES:
        dc, dsd, tc, tsd = LL.models(kind)
        _ENGINES[kind] = (hip.engine.SpecDecModel.from_state_dict(dc, dsd, dtype=LL.DTYPES[kind]),
                          hip.engine.SpecDecModel.from_state_dict(tc, tsd, dtype=LL.DTYPES[kind]))
    return _ENGINES[kind]


def _seeds(n, first=0):
    return [LL.SEED_BASE + first + i for i in range(n)]


def _first_tokens(outs, L, M):
    return np.array([o[0, L:L + M].tolist() for o in outs], dtype=np.int64)


def _fit(cs, samples, t0, what):
    assert samples.shape == (cs.N, cs.M), samples.shape
    x2, dof, outside = LL.x2_of(cs, samples)
    print(f"{what} [{cs.name}]: X2 {x2:.1f} on {dof} dof, bar {cs.bar:.1f} (N {cs.N}, lambda_ref {cs.lam:.2f}, "
          f"{outside} samples outside the support), {time.time() - t0:.1f} s")
    assert dof == cs.dof
    if cs.kind == "fp32":
        assert outside == 0, f"{outside} samples in cells of expected mass 0"
    assert x2 < cs.bar, (what, cs.name, x2, cs.bar)


def _queue(hip, cs, seeds, shared=False, **over):
    dm, tm = _engines(hip, cs.kind)
    kw = dict(gamma=cs.gamma, temperature=cs.temperature, top_k=cs.top_k, top_p=0.0, seeds=seeds, slots=SLOTS)
    kw.update(over)
    prompts = [cs.prompt] * len(seeds)
    if shared:
        return hip.S.speculative_sampling_queue_shared(prompts, dm, tm, -1, None, cs.M, shared_prefix=cs.prompt.shape[1], **kw)
    return hip.S.speculative_sampling_queue(prompts, dm, tm, -1, None, cs.M, **kw)


# --------------------------------------------------------------------------------------------------------- the queue
@pytest.mark.parametrize("name", ["fp32_filtered", "fp32_plain", "bf16_plain", "fp16_plain"])
def test_queue_output_is_distributed_as_the_target(hip, name):
    """speculative_sampling_queue, the same prompt N times on 16 slots, seeds SEED_BASE + i.
    fp32_filtered  T 2, top_k 3: N 20000, 81 cells, dof 79, bar 179.0.  Sees every planted defect (simulator X2: resample_p
                   10666, |p-q| 2e7, shared uniform 506, bonus from previous row 1e7, early p 151095, same noise 1050).  7.8 s.
    fp32_plain     T 1: N 20000, 121 rank cells, dof 69, bar 164.2.  Sees resample_p 1944, |p-q| 5097, shared uniform 332,
                   bonus 16051, early p 27201; does NOT see same noise (214).  6.9 s.
    bf16_plain     T 1: N 8000, dof 37, lambda_ref 2.1 (cap 8.2), bar 127.0.  Sees resample_p 617, |p-q| 1204, bonus 879,
                   early p 4179; does NOT see shared uniform (51) - nor same noise (not simulated at V = 8192).  2.2 s.
    fp16_plain     as bf16 with lambda_ref 0.03, bar 113.9.  2.0 s."""
    cs = LL.case(name)
    t0 = time.time()
    outs = _queue(hip, cs, _seeds(cs.N))
    _fit(cs, _first_tokens(outs, cs.prompt.shape[1], cs.M), t0, "queue")


def test_queue_shared_prefix_route_is_distributed_as_the_target(hip):
    """speculative_sampling_queue_shared with the whole prompt shared (every admission is a KV copy), bf16: bars and visible
    defects of bf16_plain above.  0.8 s."""
    cs = LL.case("bf16_plain")
    t0 = time.time()
    outs = _queue(hip, cs, _seeds(cs.N), shared=True)
    _fit(cs, _first_tokens(outs, cs.prompt.shape[1], cs.M), t0, "queue_shared")


@pytest.mark.parametrize("pair", [("rows_fp32_a", "rows_fp32_b"), ("rows_bf16_a", "rows_bf16_b")], ids=["fp32", "bf16"])
def test_queue_per_prompt_parameters_each_group_fits_its_own_target(hip, pair):
    """Per-prompt temperature (and, in fp32, top_k) alternating between two requests in one queue call - the row_params
    route, which token parity cannot hold in 16-bit.  Each group is tested against its own expected cells.
    fp32: (T 2, k 3) N 10000, dof 79, bar 179.0 / (T 1.3, k 0) N 10000, dof 45, bar 126.9: 7.0 s.  bf16: T 1 / T 0.8, N 8000 each,
    dof 37 / 49, lambda_ref 2.1 / 6.0 (caps 8.2 / 10.9), bars 127.0 / 165.1: 3.4 s.  Each group sees resample_p, |p-q|, bonus from
    the previous row and early p (the (T 2, k 3) group also same noise); none sees a shared uniform at these N."""
    a, b = LL.case(pair[0]), LL.case(pair[1])
    assert a.N == b.N and a.kind == b.kind and torch.equal(a.prompt, b.prompt)
    t0 = time.time()
    n = 2 * a.N
    outs = _queue(hip, a, _seeds(n), temperature=[a.temperature, b.temperature] * a.N, top_k=[a.top_k, b.top_k] * a.N)
    toks = _first_tokens(outs, a.prompt.shape[1], a.M)
    _fit(a, toks[0::2], t0, "queue rows, even prompts")
    _fit(b, toks[1::2], t0, "queue rows, odd prompts")


def test_queue_seeds_that_differ_in_the_high_word_only(hip):
    """seeds 77 + i * 2^32: a loop that drops the seed's high word gives N identical runs.  fp32 filtered, N 4000,
    dof 74, bar 171.6; the four gross defects are visible too.  1.3 s."""
    cs = LL.case("fp32_filtered_high_seeds")
    t0 = time.time()
    outs = _queue(hip, cs, [77 + i * LL.HIGH_SEED_STEP for i in range(cs.N)])
    _fit(cs, _first_tokens(outs, cs.prompt.shape[1], cs.M), t0, "queue, high-word seeds")


# --------------------------------------------------------------------------------------------------------- batch, AR, single
def _lockstep(hip, cs, fn):
    """N / 16 calls of 16 streams on the same prompt; call c's streams run on seeds SEED_BASE + 16 c + j."""
    assert cs.N % SLOTS == 0
    outs = []
    for c in range(cs.N // SLOTS):
        outs += fn([cs.prompt] * SLOTS, _seeds(SLOTS, SLOTS * c))
    return _first_tokens(outs, cs.prompt.shape[1], cs.M)


@pytest.mark.parametrize("name", ["batch_fp32_filtered", "batch_bf16_plain"])
def test_batch_output_is_distributed_as_the_target_and_streams_are_independent(hip, name):
    """speculative_sampling_batch, 16 streams x N / 16 calls, and the independence of neighbouring streams (seeds s, s + 1):
    the contingency table of (stream 2j's first-token class, stream 2j + 1's), all 8 disjoint neighbour pairs of a call,
    against chi2.isf(1e-9) on the table's own dof.  Classes: the token's rank cell at the root.
    batch_fp32_filtered  N 8000 (500 calls), dof 79, bar 179.0; table 3 x 3, dof 4, bar 47.9.  4.1 s.
    batch_bf16_plain     N 8000, dof 37, lambda_ref 2.1, bar 127.0; table 4 x 4, dof 9, bar 60.7.  3.2 s.
    Both see resample_p, |p-q|, bonus from the previous row and early p; neither sees a shared uniform or same noise."""
    cs = LL.case(name)
    dm, tm = _engines(hip, cs.kind)
    t0 = time.time()
    toks = _lockstep(hip, cs, lambda ps, sd: hip.S.speculative_sampling_batch(
        ps, dm, tm, -1, None, cs.M, gamma=cs.gamma, temperature=cs.temperature, top_k=cs.top_k, top_p=0.0, seeds=sd))
    _fit(cs, toks, t0, "batch")
    root = [int(t) for t in cs.tree.tokens[0]]
    cls = np.array([root.index(t) if t in root else len(root) for t in toks[:, 0].tolist()])
    x2, dof, emin = LL.independence(cls[0::2], cls[1::2], len(root) + 1)
    bar = LL.bar_fp32(dof)
    print(f"batch [{name}]: neighbour streams X2 {x2:.1f} on {dof} dof, bar {bar:.1f}, smallest expected count {emin:.1f}")
    assert dof >= 4 and x2 < bar


@pytest.mark.parametrize("name", ["batch_fp32_filtered", "batch_bf16_plain"])
def test_autoregressive_batch_control_fits_the_same_bars(hip, name):
    """The control: autoregressive_sampling_batch IS the target's own sampling.  If it fits and a speculative case does not,
    the loop is at fault; if neither fits in 16-bit, the allowance is (and is fixed from the oracle).  Cases and bars of the
    batch test; 1.9 s each."""
    cs = LL.case(name)
    _, tm = _engines(hip, cs.kind)
    t0 = time.time()
    toks = _lockstep(hip, cs, lambda ps, sd: hip.S.autoregressive_sampling_batch(
        ps, tm, cs.M, -1, cs.temperature, cs.top_k, 0.0, seeds=sd))
    _fit(cs, toks, t0, "AR control")


@pytest.mark.parametrize("name", ["single_fp32_filtered", "single_bf16_plain"])
def test_single_stream_loop_is_distributed_as_the_target(hip, name):
    """speculative_sampling(rng=DeviceNoise(seed)) -> sd_spec_generate, one call per run.
    single_fp32_filtered  N 4000, dof 74, bar 171.6.  5.0 s.
    single_bf16_plain     N 8000, dof 37, lambda_ref 2.1, bar 127.0.  7.3 s.
    At these N only the gross defects are claimed (tests/test_lossless_cpu.py: resample_p, |p-q|, bonus from the previous row,
    early p)."""
    cs = LL.case(name)
    dm, tm = _engines(hip, cs.kind)
    t0 = time.time()
    prompt = cs.prompt.cuda()
    outs = [hip.S.speculative_sampling(prompt, dm, tm, -1, None, cs.M, gamma=cs.gamma, temperature=cs.temperature,
                                       top_k=cs.top_k, top_p=0.0, rng=hip.noise.DeviceNoise(s)).cpu() for s in _seeds(cs.N)]
    _fit(cs, _first_tokens(outs, cs.prompt.shape[1], cs.M), t0, "single stream")
