"""The planted-key probes of tests/attn_probe.py, checked on the oracle alone (no GPU): every layout that
test_gpu_attention_edges.py runs must (1) discriminate - the probed row's fp32 oracle logits move by at least 20x the GPU
test's tolerance when the marker is lost (replaced by the filler) or, for a forbidden key, leaked into the row - and (2) be
passed by the reference itself: the oracle in the GPU test's dtype is finite and inside the 16-bit bar of the fp32 oracle.
The dispatch arithmetic the layouts rely on is pinned as plain Python mirrors of launch_attn / attn_body."""
import functools

import pytest
import torch

import attn_probe as P
from test_gpu_production_parity import _assert_within_reference_error


def test_tol16_is_the_rule_of_assert_within_reference_error():
    """attn_probe.tol16 is the max-abs side of the project's 16-bit rule: the largest error the helper lets through."""
    for e_ref in (0.0, 0.01, 0.3):
        _assert_within_reference_error((P.tol16(e_ref), e_ref, 0.0, 0.0), "at the bar")
        with pytest.raises(AssertionError):
            _assert_within_reference_error((P.tol16(e_ref) * 1.001 + 1e-6, e_ref, 0.0, 0.0), "past the bar")


def test_dispatch_arithmetic_the_layouts_rely_on():
    # split at s_max > 384 keys, ceil(s / 256) chunks (at most 8), each rounded up to 16 keys
    assert [P.nsplit_for(s) for s in (384, 385, 512, 513, 1025)] == [1, 2, 2, 3, 5]
    assert [P.chunk_keys(s, P.nsplit_for(s)) for s in (384, 385, 511, 512, 513, 1025)] == [384, 208, 256, 256, 176, 208]
    assert P.chunk_edges(385, 2) == [0, 207, 208, 384]
    assert P.chunk_edges(1025, 5) == [0, 207, 208, 415, 416, 623, 624, 831, 832, 1024]
    # (64, 32): 8 chunks of 16 keys at 65..128 keys - with 8 new rows the last chunks lie past row 0's causal range
    assert P.nsplit_for(65, 1, 64, 32) == 3 and P.chunk_keys(65, 3) == 32
    assert P.nsplit_for(250, 1, 64, 32) == 8 and P.chunk_keys(250, 8) == 32
    assert "chunk-past-causal-range" in P.branches(64, 97, 8, 64, 32)
    # (4096, 256): unsplit past both in-register limits and past the D = 64 prefetch window
    assert P.nsplit_for(600, 1, 4096, 256) == 1
    assert (P.in_register_limit(4), P.in_register_limit(5)) == (512, 256)
    assert "lds-softmax" in P.branches(64, 513, 4, 4096, 256) and "register-softmax" in P.branches(64, 512, 4, 4096, 256)
    assert "lds-softmax" in P.branches(64, 512, 5, 4096, 256) and "prefetch-tail" in P.branches(64, 513, 1, 4096, 256)
    assert [P.v_prefetch_keys(d) for d in (128, 64, 32)] == [256, 512, 1024]
    # at D = 128 the prefetch tail runs only for unsplit contexts of 257..384 keys; there the second MFMA K batch runs too
    assert "prefetch-tail" in P.branches(128, 257, 1) and "prefetch-tail" in P.branches(128, 384, 1)
    assert "prefetch-tail" not in P.branches(128, 256, 1) and "prefetch-tail" not in P.branches(128, 385, 1)
    assert "mfma-batch2" in P.branches(128, 300, 5) and "mfma-batch2" not in P.branches(128, 256, 5)
    assert [P.pv_width(n) for n in (1, 2, 3, 4, 5, 8)] == [1, 3, 3, 5, 5, 8] and P.groups_of(9) == [8, 1]
    # a batched pass over cache lengths (3, 390, 17, 256) splits 2 ways and every group cuts its OWN keys in two: the
    # 3-key stream's second chunk is empty, the 17-key stream's holds 2..10 keys, the long streams' about half
    for n_new in P.BATCH_NEW:
        lays = P.batch_layouts(n_new)
        assert P.chunk_keys(lays[0].S, 2) >= lays[0].S and P.batch_second_chunk_keys(lays[0]) == 0
        assert P.chunk_keys(lays[2].S, 2) == 16 and P.batch_second_chunk_keys(lays[2]) == lays[2].S - 16 and 2 <= lays[2].S - 16 <= 10
        assert P.batch_second_chunk_keys(lays[1]) > 180 and P.batch_second_chunk_keys(lays[3]) > 110
        assert lays[1].marker == P.chunk_keys(lays[1].S, 2)        # the first key of stream 1's second chunk
    # half = nr > 4 in attn_body: 5..8 rows half-wave, <= 4 rows full-wave
    assert "half-wave" in P.branches(128, 64, 5) and "full-wave" in P.branches(128, 64, 4)
    assert set(P.branches(128, 64, 9)) >= {"half-wave", "full-wave"}


def test_causal_table_meets_every_s_and_every_n_with_every_class():
    for D in (128, 64, 32, 16):
        lays = P.causal_layouts(D)
        # (under the default split a workgroup gets past its V-prefetch window at D = 128 only: 257..384 unsplit keys; the
        #  D = 64 window of 512 keys is passed under the (4096, 256) setting)
        classes = set(P.CLASSES) - (set() if D == 128 else {"past_prefetch"})
        for n in P.CAUSAL_N:
            assert {l.cls for l in lays if l.n == n} == classes, (D, n)
        for S in P.CAUSAL_S:
            have = {l.cls for l in lays if l.S == S}
            assert {"own", "forbidden"} <= have
            if S > 1:
                assert {"key0", "last_cached"} <= have, (D, S)
            if S > 257 + 16:
                assert {"key255", "key256"} <= have, (D, S)
            if S > 384:
                assert "chunk_edge" in have, (D, S)
        assert all(0 <= l.probe < l.n <= l.S and 0 <= l.marker <= l.S for l in lays)


@functools.lru_cache(maxsize=None)
def _oracle(name, dt, kvq=None):
    return P.ProbeOracle(name, P.DTYPES[dt], kvq)


def _check(o32, o16, lay, disc, logits):
    truth = logits(o32, lay)
    d = disc(o32, lay)
    if o16 is None:
        assert d >= 20 * P.FP32_TOL, (lay, d)
        return d / P.FP32_TOL, 0.0
    ref16 = logits(o16, lay)
    assert bool(torch.isfinite(ref16).all())
    errs = P.errors(ref16, ref16, truth)
    _assert_within_reference_error(errs, str(lay))                # the reference alone passes the GPU test's rule
    assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02, (lay, errs[1])      # ... and the bf16 bar of the forward tests
    assert d >= 20 * P.tol16(errs[1]), (lay, d, errs[1])
    return d / P.tol16(errs[1]), errs[1]


@pytest.mark.parametrize("label,name,dt,kvq", sorted({(c[0], c[1], c[2], c[3]) for c in P.all_cases()}, key=str))
def test_causal_layouts_discriminate_and_the_reference_alone_passes(label, name, dt, kvq):
    o32 = _oracle(name, "fp32")
    o16 = None if dt == "fp32" else _oracle(name, dt, kvq)
    worst, e_max, count = float("inf"), 0.0, 0
    for c in P.all_cases():
        if (c[0], c[1], c[2], c[3]) != (label, name, dt, kvq):
            continue
        for lay in c[4]:
            r, e = _check(o32, o16, lay, P.discrimination, lambda o, l: o.logits(l))
            worst, e_max, count = min(worst, r), max(e_max, e), count + 1
    print(f"{label} {name} {dt} {kvq}: {count} layouts, least discrimination {worst:.0f}x the tolerance, "
          f"reference error at most {e_max:.4f}")


@pytest.mark.parametrize("name,dt,kvq", P.TREE_MODELS)
def test_tree_layouts_discriminate_and_the_reference_alone_passes(name, dt, kvq):
    o32 = _oracle(name, "fp32")
    o16 = None if dt == "fp32" else _oracle(name, dt, kvq)
    worst = float("inf")
    for lay in P.tree_layouts():
        r, _ = _check(o32, o16, lay, P.tree_discrimination, lambda o, l: P.tree_logits(o, l))
        worst = min(worst, r)
    print(f"tree {name} {dt} {kvq}: least discrimination {worst:.0f}x the tolerance")


def test_fp8_scales_are_non_unit_and_folded_exactly():
    """The arena scales the fp8 tests set: powers of two, none 1, K != V per head, heads differ; the oracle's folded weights
    are still bf16 numbers and give the unscaled model's fp32 logits when nothing is quantised."""
    for name in P.FP8_MODELS:
        sc = P.fp8_scales(name)
        assert sc.shape == (1, 2, P.probe_config(name).num_key_value_heads)
        assert bool((sc != 1).all()) and bool((sc[0, 0] != sc[0, 1]).all()) and sc[0, 0, 0] != sc[0, 0, 1]
        assert torch.equal(torch.log2(sc), torch.log2(sc).round())
        sd = P.probe_state_dict(name)
        folded = P.fp8_scaled_sd(name, sd)
        assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in folded.values())
        lay = P.Layout(40, 5, 7, 4, "key0")
        a = P.ProbeOracle(name, sd=sd).logits(lay)
        b = P.ProbeOracle(name, sd=folded).logits(lay)
        assert float((a - b).abs().max()) <= 1e-4


def test_probe_weights_are_bf16_numbers():
    for name in P.MODELS:
        for k, v in P.probe_state_dict(name).items():
            assert torch.equal(v, v.to(torch.bfloat16).float()), (name, k)
