"""The tensor-parallel probes of tests/tp_probe.py, checked with no GPU: the planner's answers for the shards' O / down
projections cover every reduce-route class, the 64-row shards are 64-row shards, the session's slab reservation covers
every listed route, the plants are zero exactly where they claim, and - on the oracle alone - every admitted plant moves
every observed logit row by >= 20x the GPU test's bar under every fault of the reduce it is there for, while the
reference itself stays inside the bars.  `pytest -s` prints the coverage table and the discrimination factors."""
import pytest
import torch

import gemm_route_classes as G
import tp_probe as P
from llmspeculativesampling_amd import _lib
from test_gpu_production_parity import _assert_within_reference_error

_SHARDS = [(name, world) for name in P.MODELS for world in P.WORLDS[name]]


def test_every_reduce_route_class_is_covered_and_none_lies_past_the_row_limit():
    seen = {}
    print()
    for name, world in _SHARDS:
        mr = P.shard_max_rows(name, world)
        for n in P.probe_rows(name, world):
            for m, nl, routes in P.call_routes(name, world, "bf16", n):
                assert m <= mr
                for role, (cls, S, ksp) in routes.items():
                    assert cls != "none", (name, world, n, m, role)      # no pass of a listed call is without a kernel
                    seen.setdefault(cls, []).append((name, world, role, m))
            print(f"{name} world {world} rows {n:>3}: " + "; ".join(
                f"{m} rows (" + ", ".join(f"{role} {cls} S={S}" for role, (cls, S, _) in r.items()) + ")"
                for m, _, r in P.call_routes(name, world, "bf16", n)) + f"  folds + sums = {P.expected_other(name, world, 'bf16', n)}")
        # "none" occurs only above the shard's row limit, at every row count the planner can be asked for
        for role, (N, K) in P.shard_shapes(name, world).items():
            for M in range(1, G.MAX_ROWS + 1):
                if P.route_class(N, K, M)[0] == "none":
                    assert M > mr, (name, world, role, M, mr)
                    seen.setdefault("none", []).append((name, world, role, M))
    for cls in P.CLASSES:
        assert seen.get(cls), cls
        print(f"{cls:<20} {len(seen[cls]):>4} points, first {seen[cls][0]}")
    assert set(seen) == set(P.CLASSES), set(seen) - set(P.CLASSES)


def test_the_shards_whose_projection_has_no_kernel_past_64_rows_stop_at_64():
    assert P.shard_max_rows("tp_h1024", 4) == 64 and P.shard_shapes("tp_h1024", 4)["o"] == (1024, 256)
    assert P.shard_max_rows("tp_h4096", 8) == 64 and P.shard_shapes("tp_h4096", 8) == {"o": (4096, 512), "down": (4096, 128)}
    assert P.shard_max_rows("tp_h1024", 2) == 256 and P.shard_max_rows("tp_h4096", 2) == 256
    assert P.shard_shapes("tp_h1024", 2) == {"o": (1024, 512), "down": (1024, 2048)}
    assert P.shard_shapes("tp_h4096", 2) == {"o": (4096, 2048), "down": (4096, 512)}
    assert 65 in P.probe_rows("tp_h1024", 4) and P.call_chunks(145, 64) == [(64, 0), (64, 47), (17, 17)]


def test_the_sessions_slab_reservation_covers_every_listed_route():
    n = 0
    for name, world in _SHARDS:
        handle, keep = P.shard_handle(name, world)
        mr = _lib.lib.sd_model_max_rows(handle)
        have = _lib.lib.sd_session_part_floats(handle, mr)
        for role, (N, K) in P.shard_shapes(name, world).items():
            for M in range(1, mr + 1):
                for need in (G.ONE_SLAB, 0):
                    r = G.route(N, K, M, need)
                    assert r.kind != _lib.SD_GEMM_NONE and 0 < r.part_floats <= have, (name, world, role, M, need, r, have)
                    n += 1
        _lib.lib.sd_model_destroy(handle)
        del keep
    assert n > 1000


def test_plants_are_zero_exactly_outside_their_slice_and_the_gains_are_exact():
    for g in P.RANK_GAINS + tuple(P.slab_gain(S) for S in range(2, 17)):
        assert g > 1 and float(torch.tensor(g).to(torch.bfloat16)) == g and (int(g) & (int(g) - 1)) == 0
    assert all(a != b for a, b in zip(P.RANK_GAINS, P.RANK_GAINS[1:]))
    for name, world in _SHARDS:
        base = P.base_state_dict(name)
        for v in base.values():
            assert torch.equal(v, v.to(torch.bfloat16).float())
        for r in range(world):
            sd = P.rank_state_dict(name, world, r)
            for k, v in sd.items():
                assert torch.equal(v, v.to(torch.bfloat16).float()), (name, k)
                if not k.endswith(P._ROW_PAR):
                    assert v is base[k]
                    continue
                lo, hi = P.rank_slice(name, k, r, world)
                assert hi - lo == v.shape[1] // world and lo == r * (hi - lo)
                assert torch.equal(v[:, lo:hi], base[k][:, lo:hi] * P.RANK_GAINS[r]) and bool((v[:, lo:hi] != 0).any())
                assert not bool(v[:, :lo].any()) and not bool(v[:, hi:].any())
                # what the engine hands rank q: all zero unless q is the planted rank
                for q in range(world):
                    assert bool(P.shard_tensor(P.probe_config(name), k, v, q, world).any()) == (q == r)
        for role, n, S, ksp, r, s in P.slab_cases(name, world):
            key = P.slab_key(name, role)
            N, K = P.shard_shapes(name, world)[role]
            assert P.reduce_routes(name, world, n)[role][1:] == (S, ksp) and S > 1 and (S - 1) * ksp < K // 32 <= S * ksp
            v = P.plant_state_dict(name, world, ("slab", role, n, S, ksp, r, s))[key]
            local = P.shard_tensor(P.probe_config(name), key, v, r, world)
            a, b = s * ksp * 32, min(K, (s + 1) * ksp * 32)          # the slab's k-range in the shard's local k order
            assert local.shape == (N, K) and bool(local[:, a:b].any())
            assert not bool(local[:, :a].any()) and not bool(local[:, b:].any())
            assert torch.equal(local[:, a:b], P.shard_tensor(P.probe_config(name), key, base[key], r, world)[:, a:b] * P.slab_gain(S))
            for q in range(world):
                if q != r:
                    assert not bool(P.shard_tensor(P.probe_config(name), key, v, q, world).any())
        assert not P.slab_cases(name, world) or {c[5] for c in P.slab_cases(name, world)} >= {0}


def _bar(o32, o16, toks, pos0):
    """The GPU test's max-abs bar for one call, from the reference's own error (bf16) or the fp32 constant."""
    nl = min(len(toks), P.MAX_LOGIT_ROWS)
    truth = o32.run(toks, pos0)[0][-nl:]
    if o16 is None:
        return P.FP32_TOL, 0.0
    ref16 = o16.run(toks, pos0)[0][-nl:]
    assert bool(torch.isfinite(ref16).all())
    errs = P.errors(ref16, ref16, truth)
    _assert_within_reference_error(errs, str((o32.name, len(toks), pos0)))
    assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02, (o32.name, len(toks), pos0, errs[1])    # the cap of test_seam_probe_cpu
    return P.tol16(errs[1]), errs[1]


@pytest.mark.parametrize("name,world", _SHARDS, ids=[f"{n}-w{w}" for n, w in _SHARDS])
def test_every_admitted_plant_shows_every_fault_and_the_reference_alone_passes(name, world):
    """Per dtype the GPU file runs, on EVERY call of every plant: the same-dtype reference stays inside the bars and the cap,
    and the lock-step sharded oracle without a fault equals the unsharded one to 1e-4 of the logit scale (and so lies
    inside the GPU bar).  On tp_probe.fault_calls - every row count, the two prefixes in turn - each fault of the plant moves
    every observed row by >= 20x the bar, or the plant is listed in tp_probe.REJECTED with the factor measured here."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    print()
    bad = []
    for dt in P.GPU_DTYPES[name]:
        for label, spec in P.plant_list(name, world, dt):
            sd = P.plant_state_dict(name, world, spec)
            o32 = P.TpOracle(name, sd=sd)
            o16 = None if dt == "fp32" else P.TpOracle(name, P.DTYPES[dt], sd=sd)
            calls = P.plant_calls(name, world, dt, spec)
            fault_calls = P.fault_calls(name, world, dt, spec)
            assert fault_calls and set(fault_calls) <= set(calls)
            worst, agree, e_max = float("inf"), 0.0, 0.0
            for n, pos0 in calls:                                   # EVERY call: the reference's own error, the two oracle paths
                toks, nl = P.tokens(n), min(n, P.MAX_LOGIT_ROWS)
                tol, e_ref = _bar(o32, o16, toks, pos0)
                e_max = max(e_max, e_ref)
                truth = o32.run(toks, pos0)[0]
                clean = o32.sharded(world, toks, pos0)
                gap = float((clean - truth).abs().max())
                agree = max(agree, gap / max(float(truth.abs().max()), 1e-9))
                assert gap <= 1e-4 * float(truth.abs().max()) and gap <= tol, (name, world, label, n, pos0, gap)
                if (n, pos0) in fault_calls:
                    for f in P.plant_faults(name, world, spec):
                        worst = min(worst, P.moved(o32.sharded(world, toks, pos0, f), clean, nl) / tol)
            key = (name, world, dt, label)
            print(f"{name} world {world} {dt} {label}: {len(calls)} calls ({len(fault_calls)} with faults), reference error <= {e_max:.4f}, sharded oracle within "
                  f"{agree:.1e} of the logit scale, least movement under a fault {worst:.1f}x the bar"
                  f"{' (REJECTED: claims nothing)' if key in P.REJECTED else ''}")
            if key in P.REJECTED:
                ok = abs(worst - P.REJECTED[key]) <= 0.25 * P.REJECTED[key]      # (the listed factor, all under 20; the bf16 bar moves with the CPU's rounding)
            else:
                ok = worst >= P.FACTOR
            if not ok:
                bad.append((key, round(worst, 1)))
    assert not bad, bad                                             # (all of them at once: the table is edited in one go)
    assert all(k[:2] != (name, world) or k[3] in dict(P.plant_list(name, world, k[2])) for k in P.REJECTED)
    assert all(f < P.FACTOR for f in P.REJECTED.values())


def test_a_faulted_oracle_is_what_the_fault_says():
    """The fault injection itself, on the smallest probe: dropping rank r equals the sharded forward of weights whose rank-r
    slices are zero; reading rank 1 over rank 0 at world 2 doubles rank 1's share."""
    name, world, toks = "tp_h1024", 2, P.tokens(5)
    o = P.TpOracle(name)
    for r in range(world):
        sd = dict(P.base_state_dict(name))
        for k in list(sd):
            if k.endswith(P._ROW_PAR):
                lo, hi = P.rank_slice(name, k, r, world)
                w = sd[k].clone()
                w[:, lo:hi] = 0
                sd[k] = w
        want = P.TpOracle(name, sd=sd).run(toks)[0]
        got = o.sharded(world, toks, 0, P.Fault("drop", a=r))
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), r
    # rank 1 read in rank 0's place: rank 0's columns contribute nothing, rank 1's twice
    sd = dict(P.base_state_dict(name))
    for k in list(sd):
        if k.endswith(P._ROW_PAR):
            lo, hi = P.rank_slice(name, k, 0, world)
            w = sd[k].clone()
            w[:, lo:hi] = 0
            w[:, hi:] *= 2.0
            sd[k] = w
    want = P.TpOracle(name, sd=sd).run(toks)[0]
    got = o.sharded(world, toks, 0, P.Fault("dup", a=1, b=0))
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert P.moved(got, o.sharded(world, toks), 5) > 0
    key = P.slab_key(name, "down")
    lo, hi = P.slab_range(name, key, world, 1, 16, 2)
    sd = dict(P.base_state_dict(name))
    w = sd[key].clone()
    w[:, lo:hi] = 0
    sd[key] = w
    want = P.TpOracle(name, sd=sd).run(toks)[0]
    got = o.sharded(world, toks, 0, P.Fault("slab", key=key, lo=lo, hi=hi))
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert P.moved(got, o.sharded(world, toks), 5) > 0
