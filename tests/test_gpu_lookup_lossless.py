"""The prompt-lookup loops are lossless (`pytest -m gpu`): the first M = 4 tokens they emit are distributed as the target's own
sampling, whatever the lookup proposes.  tests/lossless.py's Tree, pearson, ALPHA, seed list and bars, gamma = 2; the cases, their
planted prompts and what they can see are tests/lookup_lossless.py's, derived on the oracle alone (tests/test_lookup_cpu.py prints
the table).  Expected cells and bars come from the oracle only, never from the engine.

The prompts are planted so that drafts ARE accepted: on the fp32 case the first iteration accepts at least one draft with
probability 0.64 and both with 0.35, on the bf16 case 0.42 and 0.18 - so the accepted-draft path, the residual after a lookup
draft and the bonus row all carry weight in the fit.  Each case sees resample_p, resample_abs and bonus_prev_row (simulator X2 far
above the bar); none claims shared_uniform (as the speculative cases at these N), and early_p / same_noise have no counterpart in
a loop without draft rows or draft noise."""
import time

import numpy as np
import pytest
import torch

import lookup_lossless as K
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


def _target(hip, kind):
    if kind not in _ENGINES:
        _, _, tc, tsd = LL.models(kind)
        _ENGINES[kind] = hip.engine.SpecDecModel.from_state_dict(tc, tsd, dtype=LL.DTYPES[kind])
    return _ENGINES[kind]


def _fit(cs, outs, t0, what):
    L = cs.prompt.shape[1]
    samples = np.array([o[0, L:L + cs.M].tolist() for o in outs], dtype=np.int64)
    assert samples.shape == (cs.N, cs.M), samples.shape
    x2, dof, outside = LL.x2_of(cs, samples)
    print(f"{what} [{cs.name}]: X2 {x2:.1f} on {dof} dof, bar {cs.bar:.1f} (N {cs.N}, lambda_ref {cs.lam:.2f}, "
          f"{outside} samples outside the support), {time.time() - t0:.1f} s")
    assert dof == cs.dof
    if cs.kind == "fp32":
        assert outside == 0, f"{outside} samples in cells of expected mass 0"
    assert x2 < cs.bar, (what, cs.name, x2, cs.bar)


@pytest.mark.parametrize("name", ["lookup_batch_fp32_filtered", "lookup_batch_bf16_plain"])
def test_lock_step_lookup_output_is_distributed_as_the_target(hip, name):
    """prompt_lookup_sampling_batch in calls of 16 streams on the planted prompt, call c's streams on seeds SEED_BASE + 16 c + j.
    lookup_batch_fp32_filtered  T 2, top_k 3, N 8000, 81 cells, dof 80, bar 180.5.
    lookup_batch_bf16_plain     T 1, N 8000, rank cells, the noncentral bar with lambda_ref measured on the bf16 oracle where
                                the test runs (4.5 and bar 147.5 seen)."""
    cs = K.case(name)
    tm = _target(hip, cs.kind)
    t0 = time.time()
    outs, acc = [], 0
    prompts = [cs.prompt.cuda()] * SLOTS
    for c in range(cs.N // SLOTS):
        o, ds = hip.S.prompt_lookup_sampling_batch(prompts, tm, -1, None, cs.M, cs.gamma, cs.temperature, cs.top_k, 0.0, K.NGRAM_MAX,
                                                   K.NGRAM_MIN, details=True,
                                                   seeds=[LL.SEED_BASE + SLOTS * c + j for j in range(SLOTS)])
        outs += [x.cpu() for x in o]
        acc += sum(d["acc_len"][0] > 0 for d in ds)
    p_any = K.condition(cs.tree, cs.prompt)[0]
    print(f"{name}: the first iteration accepted a draft in {acc} of {cs.N} runs (expected share {p_any:.3f})")
    assert abs(acc / cs.N - p_any) < 0.05                          # (6 sigma at N = 8000 is 0.033)
    _fit(cs, outs, t0, "lookup batch")


def test_single_stream_lookup_output_is_distributed_as_the_target(hip):
    """prompt_lookup_sampling(rng=DeviceNoise(seed)) -> sd_lookup_generate, one call per run: T 2, top_k 3, N 4000, dof 72,
    bar 168.6."""
    cs = K.case("lookup_single_fp32_filtered")
    tm = _target(hip, cs.kind)
    t0 = time.time()
    prompt = cs.prompt.cuda()
    outs = [hip.S.prompt_lookup_sampling(prompt, tm, -1, None, cs.M, cs.gamma, cs.temperature, cs.top_k, 0.0, K.NGRAM_MAX, K.NGRAM_MIN,
                                         rng=hip.noise.DeviceNoise(LL.SEED_BASE + i)).cpu() for i in range(cs.N)]
    _fit(cs, outs, t0, "lookup single stream")
