"""The layer-seam probes of tests/seam_probe.py, checked on the oracle alone (no GPU): every pass that
test_gpu_layer_seams.py feeds must (i) be passed by the reference itself - the oracle in the GPU test's dtype is finite,
inside _assert_within_reference_error and inside the 16-bit bar of the fp32 oracle - and (ii) discriminate: the fp32
oracle's logits of the planted rows move by at least 20x the GPU test's tolerance when ONE norm site leaves the planted
column out of its statistics (family A), or when an ordinary token takes a degenerate row's place (family B).  The route
arithmetic the row counts rely on is pinned as plain Python mirrors of plan_forward.  `pytest -s` prints the floors."""
import os
import re

import pytest
import torch

import seam_probe as S
from test_gpu_production_parity import _assert_within_reference_error

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llmspeculativesampling_amd", "csrc")
FACTOR = 20                       # the house condition of test_attn_probe_cpu.py


def _define(header, name):
    with open(os.path.join(_CSRC, header)) as f:
        return int(re.search(rf"^#define {name} (\d+)", f.read(), re.M).group(1))


def test_route_mirrors_match_the_sources():
    """rn_threads, SMALL_MAX_ROWS and the norm-on-load condition, against the constants and the expressions of the host
    code (engine.hip is read as text: the mirror must be edited when the expression is)."""
    assert _define("model_kernels.h", "RN_RG") == S.RN_RG == 2
    assert _define("small_kernels.h", "SMALL_MAX_ROWS") == S.SMALL_MAX_ROWS == 4
    with open(os.path.join(_CSRC, "engine.hip")) as f:
        src = f.read()
    assert "std::min<size_t>(1024, std::max<size_t>(64, align_up((H / 4 + RN_RG - 1) / RN_RG, 64)))" in src
    assert "return tab.n_rows <= 8 && c.hidden % 1024 == 0 && c.hidden <= 8192;" in src
    assert "tab.n_rows > SMALL_MAX_ROWS || tab.n_logit_rows > SMALL_MAX_ROWS" in src
    # small_split, which seam_probe.gemm_slabs(small=True) restates: the one-row plan, at most 16 slabs
    assert "gemm_split(N, K, 1, S_out, ksp_out);" in src
    assert "if (*S_out > 16) { *ksp_out = (KS + 15) / 16; *S_out = (KS + *ksp_out - 1) / *ksp_out; }" in src
    assert [S.rn_threads(h) for h in (96, 128, 256, 1024, 4096, 8192)] == [64, 64, 64, 128, 512, 1024]
    # the register-group edge is a column of the row only where the second group is used at all
    assert S.stat_columns("llama_h1024")[-3:] == [511, 512, 1023] and 4 * S.rn_threads(256) == 256
    assert S.stat_columns("llama_h256") == [0, 3, 4, 7, 8, 15, 16, 255]
    assert S.stat_columns("llama_h8192")[-3:] == [4095, 4096, 8191]
    cfg = S.probe_config("llama_h1024")
    assert [S.norm_on_load_ok(cfg, "bf16", n) for n in (1, 8, 9)] == [True, True, False]
    assert not S.norm_on_load_ok(cfg, "fp32", 1) and not S.norm_on_load_ok(cfg, "bf16", 1, env_norm_on_load=0)
    assert not S.norm_on_load_ok(S.probe_config("llama_h256"), "bf16", 1)
    assert [S.small_path_ok(cfg, "bf16", n) for n in (1, 4, 5)] == [True, True, False]
    assert not S.small_path_ok(cfg, "fp16", 1) and not S.small_path_ok(cfg, "bf16", 1, env_small_path=0)
    assert S.small_path_ok(S.probe_config("opt_pre_h256"), "bf16", 4)
    assert not S.small_path_ok(S.probe_config("opt_post_h128"), "bf16", 1)
    assert not S.small_path_ok(S.probe_config("opt_proj_h128"), "bf16", 1)


def test_probe_weights_are_bf16_numbers_and_the_plants_are_in_place():
    for name in S.MODELS:
        sd = S.probe_state_dict(name)
        for k, v in sd.items():
            assert torch.equal(v, v.to(torch.bfloat16).float()), (name, k)
            assert bool(torch.isfinite(v.to(torch.float16)).all()), (name, k)
        cfg = S.probe_config(name)
        emb = sd["model.embed_tokens.weight" if cfg.arch == "llama" else "model.decoder.embed_tokens.weight"]
        for t in S.plants("A", name):
            c = S.plant_column(name, t)
            assert float(emb[t, c]) == S.MAG[name] and float(emb[t].abs().topk(2).values[1]) < S.MAG[name] / 16
        assert float(emb[S.B_TOK0].abs().max()) == 0.0 and bool((emb[S.B_TOK0 + 1] == S.TINY).all())
        assert float(emb[S.B_TOK0 + 2].sum()) == 0.0 and float(emb[S.B_TOK0 + 1].pow(2).mean() + 1e-5) == float(torch.tensor(1e-5))
        ln = emb[S.B_TOK0 + 3].double()
        assert float(ln.mean() ** 2 / ln.var(unbiased=False)) > 1e3
    assert S.plant_column("llama_h256", S.ORD_TOK0) == -1 and not S.plants("A", "opt_proj_h128")


def test_dropping_a_column_is_restored_and_counts_every_norm_call():
    import torch.nn.functional as F
    from oracle import models_ref
    rms = models_ref._rms_norm
    for name in ("llama_h256", "opt_pre_h256", "opt_post_h128"):
        d = S.stat_discrimination(S.SeamOracle(name), S.passes("A", name, 4)[0])
        assert list(d) == S.norm_sites(name) and all(v > 0 for v in d.values())
    assert models_ref._rms_norm is rms and models_ref.F is F


_CASES = sorted(S.all_passes().items())


@pytest.mark.parametrize("name,dt", [k for k, _ in _CASES], ids=[f"{n}-{d}" for (n, d), _ in _CASES])
def test_every_pass_discriminates_and_the_reference_alone_passes(name, dt):
    o32 = S.SeamOracle(name)
    o16 = None if dt == "fp32" else S.SeamOracle(name, S.DTYPES[dt])
    floor, at_drop, e_max, count = {}, float("inf"), 0.0, {"A": 0, "B": 0, "E": 0}
    site_d, rows_d = S.A_SITES_DROPPED.get((name, dt), (None, None))
    for fam, toks, pos0 in sorted(S.all_passes()[(name, dt)]):
        nl = min(len(toks), S.MAX_LOGIT_ROWS)                      # the rows whose logits the GPU test sees
        truth = o32.run(toks, pos0)[0][-nl:]
        if o16 is None:
            tol = S.FP32_TOL
        else:
            ref16 = o16.run(toks, pos0)[0][-nl:]
            assert bool(torch.isfinite(ref16).all()), (fam, toks, pos0)
            errs = S.errors(ref16, ref16, truth)
            _assert_within_reference_error(errs, str((fam, toks, pos0)))
            assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02, (fam, toks, pos0, errs[1])
            tol, e_max = S.tol16(errs[1]), max(e_max, errs[1])
        count[fam] += 1
        if fam == "A":
            for site, d in S.stat_discrimination(o32, toks, pos0).items():
                if site == site_d and (rows_d is None or len(toks) in rows_d):
                    at_drop = min(at_drop, d / tol)
                else:
                    floor[site] = min(floor.get(site, float("inf")), d / tol)
        elif fam == "B":
            floor["B"] = min(floor.get("B", float("inf")), S.degenerate_discrimination(o32, toks, pos0) / tol)
    assert site_d is None or (dt != "fp32" and at_drop < FACTOR)   # one site at most (a dict), none in fp32, none that reaches the factor
    for site, f in floor.items():
        assert f >= FACTOR, (name, dt, site, f)
    print(f"\n{name} {dt}: {count['A']} A / {count['B']} B passes, magnitude {S.MAG[name]:g}, least discrimination "
          f"{min(floor.values()):.0f}x the tolerance ({', '.join(f'{k} {v:.0f}x' for k, v in floor.items())}), "
          f"reference error at most {e_max:.4f}")
    if site_d:
        print(f"  dropped under the cap: {site_d}{'' if rows_d is None else ' at rows ' + str(rows_d)}: {at_drop:.1f}x (not claimed)")


@pytest.mark.parametrize("name,dt", S.TREE_CASES)
def test_tree_pass_reference_alone_passes_and_slots_differ_from_positions(name, dt):
    """The tree pass of the GPU file on the oracle alone: the 16-bit reference inside the bars; a node's K row written
    with its SLOT as the position (the defect the pass is there for) moves that K row by far more than the arena bar."""
    pos, bits = S.tree_shape(S.TREE_NODES, S.TREE_BASE)
    assert pos[8] == S.TREE_BASE + 1 != S.TREE_BASE + 8
    toks = S.tree_tokens(name)
    truth, past32 = S.SeamOracle(name).tree(toks, S.TREE_BASE, pos, bits)
    slot_pos = [S.TREE_BASE + i for i in range(S.TREE_NODES)]
    _, wrong = S.SeamOracle(name).tree(toks, S.TREE_BASE, slot_pos, bits)
    moved = float((wrong[0][0] - past32[0][0])[0, :, S.TREE_BASE + 8].abs().max())
    if dt != "fp32":
        ref16, past16 = S.SeamOracle(name, S.DTYPES[dt]).tree(toks, S.TREE_BASE, pos, bits)
        errs = S.errors(ref16, ref16, truth)
        _assert_within_reference_error(errs, "tree")
        assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02
        tol = S.tol16(float((past16[0][0].float() - past32[0][0]).abs().max()))
    else:
        tol = 1e-4 * max(1.0, float(past32[0][0].abs().max()))
    print(f"\ntree {name} {dt}: layer-0 K row of node 8 moves by {moved / tol:.0f}x the bar when its slot is its position")
    assert moved >= FACTOR * tol


def test_planted_slabs_reach_every_fold_loop_and_discriminate():
    """Family C on the oracle alone, and the (consumer, S) table: the union of the S values holds a scalar tail (S % 4), a
    4-burst alone (4 .. 7) and an 8-burst; the small path's split is the one-row plan capped at 16 slabs."""
    import gemm_route_classes as G
    assert S.fold_loops(3) == {"tail": 0} and S.fold_loops(5) == {"burst4": 0, "tail": 4} and S.fold_loops(8) == {"burst8": 0}
    assert S.fold_loops(13) == {"burst8": 0, "burst4": 8, "tail": 12} and S.slab_classes(13) == [0, 8, 12]
    assert S.fold_loops(16) == {"burst8": 0} and S.fold_loops(7) == {"burst4": 0, "tail": 4}
    for N, K in ((256, 4096), (1024, 1024)):                         # small_split == the planner's one-row split up to 16 slabs
        for units in (None, 48, 128, 208, 256, 4096):
            env = {} if units is None else {"SD_GEMM_UNITS": units}
            with G.tunables({k: str(v) for k, v in env.items()}):
                r = G.route(N, K, 1, 0)
            Ss, ksp = S.gemm_slabs(N, K, 3, env, small=True)
            assert Ss <= 16 and (Ss - 1) * ksp < K // 32 <= Ss * ksp and (r.S > 16 or (Ss, ksp) == (r.S, r.ksp)), (N, K, units)
    table, seen = {}, set()
    for case in S.C_CASES:
        label, name, dt, env, n, weight, consumer = case
        Sn, ksp = S.c_slabs(case)
        assert Sn > 1 and (Sn - 1) * ksp < S.slab_state_dict(name, weight, ksp, 0)[weight].shape[1] // 32 <= Sn * ksp, case
        assert f"S{Sn}" in label
        table.setdefault(consumer, []).append(Sn)
        seen.add(Sn)
        toks = S.c_tokens(n)
        worst, e_max = float("inf"), 0.0
        for s in S.slab_classes(Sn):
            sd = S.slab_state_dict(name, weight, ksp, s)
            assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())
            nl = min(n, S.MAX_LOGIT_ROWS)
            truth = S.SeamOracle(name, sd=sd).forward(toks)[0][-nl:]
            ref16 = S.SeamOracle(name, S.DTYPES[dt], sd=sd).forward(toks)[0][-nl:]
            assert bool(torch.isfinite(ref16).all())
            errs = S.errors(ref16, ref16, truth)
            _assert_within_reference_error(errs, f"{label} slab {s}")
            assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02, (label, s, errs[1])
            d = S.slab_discrimination(name, weight, ksp, s, toks) / S.tol16(errs[1])
            assert d >= FACTOR, (label, s, d)
            worst, e_max = min(worst, d), max(e_max, errs[1])
        print(f"\nC {label} {name} {dt}: S = {Sn}, ksp = {ksp}, slabs {S.slab_classes(Sn)} ({S.fold_loops(Sn)}), least "
              f"discrimination {worst:.0f}x the tolerance, reference error at most {e_max:.4f}")
    print("\n(consumer, S) table of family C:", {k: sorted(v) for k, v in table.items()})
    assert any(x % 4 for x in seen) and any(4 <= x <= 7 for x in seen) and any(x >= 8 for x in seen)
    print("S >= 13 (all three loops in one fold) reachable at K <= 4096:", any(x >= 13 for x in seen))


@pytest.mark.parametrize("name,dt", sorted(S.D_MODELS))
def test_activation_columns_hit_their_gates_and_discriminate(name, dt):
    """Family D on the oracle alone: in every pass the gate pre-activation of the decisive column is where the token puts
    it (past expf's overflow for +-96, at +-20, at +-2^-10, exactly 0 for an ordinary token); the 16-bit reference is
    inside the bars; negating the gate row moves every D row's logits by >= 20x the tolerance."""
    worst, worst8, e_max, count, lo, hi = float("inf"), float("inf"), 0.0, 0, 0.0, 0.0
    assert all(set(rows) <= set(S.D_ROWS[n]) for _, n, _, _, _, rows in S.D_CASES)
    for j in S.act_columns(name):
        sd = S.act_state_dict(name, j)
        assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())
        o32 = S.SeamOracle(name, sd=sd)
        o16 = None if dt == "fp32" else S.SeamOracle(name, S.DTYPES[dt], sd=sd)
        for n in S.D_ROWS[name]:
            for toks in S.act_passes(n):
                g = S.act_gates(o32, j, toks)
                for r, t in enumerate(toks):
                    want = S.D_GATES[t - S.D_TOK0] if S.D_TOK0 <= t < S.D_TOK0 + len(S.D_GATES) else 0.0
                    assert abs(float(g[r]) - want) <= 0.02 * abs(want), (name, j, toks, r, float(g[r]), want)
                    if abs(want) > 90:
                        assert abs(float(g[r])) > S.SILU_OVERFLOW
                        lo, hi = min(lo, float(g[r])), max(hi, float(g[r]))
                truth = o32.forward(toks)[0]
                tol = S.FP32_TOL
                if o16 is not None:
                    ref16 = o16.forward(toks)[0]
                    assert bool(torch.isfinite(ref16).all())
                    errs = S.errors(ref16, ref16, truth)
                    _assert_within_reference_error(errs, str((name, j, toks)))
                    assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02, (name, j, toks, errs[1])
                    tol, e_max = S.tol16(errs[1]), max(e_max, errs[1])
                d = S.act_discrimination(name, j, toks) / tol
                assert d >= FACTOR, (name, dt, j, toks, d)
                d8 = S.act_discrimination(name, j, toks, swap_up=True) / tol       # the up value of the column 8 away
                assert d8 >= FACTOR, (name, dt, j, toks, d8)
                worst, worst8, count = min(worst, d), min(worst8, d8), count + 1
    print(f"\nD {name} {dt}: {count} passes over columns {S.act_columns(name)}, gates reach {lo:.1f} .. {hi:.1f}, least "
          f"discrimination {worst:.0f}x the tolerance (up value from the column 8 away: {worst8:.0f}x), reference error at "
          f"most {e_max:.4f}")


@pytest.mark.parametrize("name,dt", S.HEAD_MODELS)
def test_planted_head_columns_are_the_maximum_and_discriminate(name, dt):
    worst, e_max = float("inf"), 0.0
    for v in S.head_columns(name):
        sd = S.head_state_dict(name, v)
        assert all(torch.equal(t, t.to(torch.bfloat16).float()) for t in sd.values())
        for n in S.HEAD_ROWS:
            toks = S.head_tokens(n)
            truth = S.SeamOracle(name, sd=sd).forward(toks)[0]
            assert truth.argmax(-1).tolist() == [v] * n, (name, v, n)
            tol = S.FP32_TOL
            if dt != "fp32":
                ref16 = S.SeamOracle(name, S.DTYPES[dt], sd=sd).forward(toks)[0]
                assert bool(torch.isfinite(ref16).all()) and ref16.argmax(-1).tolist() == [v] * n
                errs = S.errors(ref16, ref16, truth)
                _assert_within_reference_error(errs, str((name, v, n)))
                assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02, (name, v, n, errs[1])
                tol, e_max = S.tol16(errs[1]), max(e_max, errs[1])
            d = S.head_discrimination(name, v, toks) / tol
            assert d >= FACTOR, (name, dt, v, n, d)
            worst = min(worst, d)
    print(f"\nD head {name} {dt}: columns {S.head_columns(name)}, least discrimination {worst:.0f}x the tolerance, "
          f"reference error at most {e_max:.4f}")


@pytest.mark.parametrize("name,dt", [(c[0], c[1]) for c in S.KV_CASES if c[0].startswith("opt")])
def test_written_kv_rows_see_the_learned_position_offset(name, dt):
    """The K / V comparison of the GPU file notices a wrong pos_off: with the learned-position table shifted by the
    offset (row p where row p + 2 belongs) layer 0's K rows of the pass, or its logits, move by >= 20x their bar."""
    sd = dict(S.probe_state_dict(name))
    k = "model.decoder.embed_positions.weight"
    sd[k] = torch.roll(sd[k], 2, 0)
    worst = float("inf")
    for _, _, pos0s, n in [c for c in S.KV_CASES if (c[0], c[1]) == (name, dt)]:
        for pos0 in pos0s:
            toks = S.kv_pass(name, dt, n)[1]
            good, bad = S.SeamOracle(name).run(toks, pos0), S.SeamOracle(name, sd=sd).run(toks, pos0)
            gk, bk = (x[1][0][0][0, :, pos0:] for x in (good, bad))
            if dt == "fp32":
                tol_k, tol_l = 1e-4 * max(1.0, float(gk.abs().max())), S.FP32_TOL
            else:
                ref16 = S.SeamOracle(name, S.DTYPES[dt]).run(toks, pos0)
                tol_k = S.tol16(float((ref16[1][0][0][0, :, pos0:].float() - gk).abs().max()))
                tol_l = S.tol16(float((ref16[0] - good[0]).abs().max()))
            d = max(float((bk - gk).abs().max()) / tol_k, float((bad[0] - good[0]).abs().max()) / tol_l)
            assert d >= FACTOR, (name, dt, pos0, d)
            worst = min(worst, d)
    print(f"\nkv {name} {dt}: a learned-position table read 2 rows off moves the K rows or the logits by >= {worst:.0f}x their bar")


@pytest.mark.parametrize("name,dt", S.RELU_MODELS)
def test_opt_fc1_bias_edges(name, dt):
    """OPT's twin of family D.  "cancel": the exact pre-activation 2^-12 (a dot of 4 (1 + 2^-6 + 2^-14) against a bias of
    -4 (1 + 2^-6)) decides the logits, the 16-bit reference is inside the bars, and losing it - as a dot rounded to 16 bits
    before the bias add does - moves every row by >= 20x the tolerance.  The bias alone at -0.0 and at the smallest
    positive bf16 subnormal cannot reach any logit (ReLU gives 0 / 2^-133): measured here, and therefore not run on the GPU."""
    assert S.R_A * S.R_A + S.R_BIAS == 2.0 ** -12
    worst, e_max, dead = float("inf"), 0.0, 0.0
    for j in S.act_columns(name):
        for kind in S.R_KINDS:
            sd = S.relu_state_dict(name, j, kind)
            assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())
            for n in S.RELU_ROWS:
                toks = S.head_tokens(n)
                d = S.relu_discrimination(name, j, kind, toks)
                if kind != "cancel":
                    dead = max(dead, d)
                    continue
                truth, tol = S.SeamOracle(name, sd=sd).forward(toks)[0], S.FP32_TOL
                if dt != "fp32":
                    ref16 = S.SeamOracle(name, S.DTYPES[dt], sd=sd).forward(toks)[0]
                    assert bool(torch.isfinite(ref16).all())
                    errs = S.errors(ref16, ref16, truth)
                    _assert_within_reference_error(errs, str((name, j, n)))
                    assert errs[1] <= 0.04 * float(truth.abs().max()) + 0.02, (name, j, n, errs[1])
                    tol, e_max = S.tol16(errs[1]), max(e_max, errs[1])
                assert d >= FACTOR * tol, (name, dt, j, n, d / tol)
                worst = min(worst, d / tol)
    assert dead < S.FP32_TOL / FACTOR                               # inadmissible: no defect at these values can move a logit
    print(f"\nD relu {name} {dt}: cancel case least discrimination {worst:.0f}x the tolerance, reference error at most "
          f"{e_max:.4f}; bias at -0.0 / 2^-133: largest movement {dead:.1e} (dropped: cannot discriminate)")
