"""Fixes every free choice of tests/test_gpu_lossless.py on the CPU, from the oracle alone, and prints what it found: the
chosen inputs, N / dof / bar per case, lambda_ref with its cap, the k-th-gap search for a 16-bit filtered case and the
defect-power table (tests/lossless.py has the helper).  Needs no GPU.

Conditions every case must meet (checked below):
  * M >= gamma + 2: the all-accept bonus token and the first token of the next iteration are both observed.  With
    gamma = 4, M = 4 the "bonus from the previous row" defect is invisible (shown below).
  * both branches carry weight: the draft / target acceptance rate at the chosen inputs lies in 30 .. 80 %.
  * random_seed stays None (the reference's reseed-before-every-uniform quirk IS the shared-uniform defect).
  * power: every defect a case claims (lossless.CLAIMS) gives X2 >= 2 x bar on the simulator at the case's N, and the
    correct simulator and the autoregressive control stay under the bar.
  * 16-bit: bar = the 1 - 1e-9 quantile of ncx2(dof, 2.25 * lambda_ref), with 2.25 * lambda_ref <= dof / 2.
  * fp32: the central chi2.isf(1e-9, dof).  The suite holds fp32 logits to 1e-3 of the oracle: a conditional then moves by a
    factor within e^(+-2e-3 / T), a cell (M = 4 conditionals) by at most 8.1e-3 relative at T = 1, so
    lambda <= N * sum p * (8.1e-3)^2 = 1.3 at N = 20000 against dof >= 45 - a shift of the bar's argument by under 1 %.
  * OPT in 16-bit is excluded (the reference rounds p / E to 16 bits there: its own distribution is not the softmax)."""
import numpy as np
import pytest

import lossless as LL

SIM_SEED = 2024


def test_cells_partition_the_outcomes_and_the_statistic_pools_small_cells():
    for name in ("fp32_filtered", "fp32_plain"):
        cs = LL.case(name)
        t = cs.tree
        assert abs(t.prob.sum() - 1.0) < 1e-12, (name, t.prob.sum())
        assert len(t.prefixes) == sum(LL.RANKS ** d for d in range(cs.M)) and len(set(t.cells)) == len(t.cells)
        assert len(t.cells) == (LL.RANKS ** cs.M if t.filtered else LL.RANKS ** cs.M + len(t.prefixes))
    # a hand-made tree: two positions, V = 4, plain scheme with 3 ranks -> "other" is token 3 at the root
    P = {(): np.array([0.5, 0.3, 0.15, 0.05]), (0,): np.array([0.1, 0.2, 0.3, 0.4]), (1,): np.array([0.25] * 4),
         (2,): np.array([0.7, 0.1, 0.1, 0.1])}
    t = LL.Tree(lambda pre: P[pre], lambda pre: P[pre], 2, filtered=False)
    assert abs(t.prob.sum() - 1.0) < 1e-12
    assert t.prob[t.cell_index[(LL.OTHER,)]] == pytest.approx(0.05)
    assert t.prob[t.cell_index[(0, LL.OTHER)]] == pytest.approx(0.5 * 0.1)          # token 0 is the rank-4 token after (0,)
    counts, outside = t.classify(np.array([[3, 0], [0, 0], [0, 3], [2, 0], [1, 2]]))
    assert outside == 0 and counts[t.cell_index[(LL.OTHER,)]] == 1 and counts[t.cell_index[(0, LL.OTHER)]] == 1
    assert counts[t.cell_index[(0, 3)]] == 1 and counts[t.cell_index[(2, 0)]] == 1 and counts.sum() == 5
    # pooling: N = 200 -> the three cells of expected count 3 become one; a sample outside a filtered support is reported apart
    x2, dof = LL.pearson(np.round(200 * t.prob), 0, t.prob, 200)
    keep, rest = LL.pooled(t.prob, 200)
    assert len(rest) == 3 and dof == len(keep) == len(t.cells) - 3 and x2 < 1e-9
    f = LL.Tree(lambda pre: np.array([0.5, 0.5, 0.0, 0.0]), None, 2, filtered=True)
    counts, outside = f.classify(np.array([[0, 1], [2, 0], [1, 3]]))
    assert outside == 2 and counts.sum() == 1
    # ... and has no pooled cell to go to when every cell of the support stands alone: X2 is inf
    assert LL.pearson(np.array([25, 25, 25, 23]), 2, f.prob, 100)[0] == float("inf")
    assert LL.pearson(np.array([25, 25, 25, 25]), 0, f.prob, 100) == (0.0, 3)


def test_simulator_is_exact_on_a_table_and_every_defect_changes_the_law():
    """The correct simulator and the control reproduce the target on a small position-dependent table at N = 200000
    (X2 under the 1e-9 bar), and each planted defect is far outside it."""
    rng = np.random.default_rng(1)
    V = 6
    tab = {}

    def row(pre, salt):
        key = (pre, salt)
        if key not in tab:
            r = np.random.default_rng([salt, len(pre)] + list(pre)).random(V) ** 2
            tab[key] = r / r.sum()
        return tab[key]
    t = LL.Tree(lambda pre: row(pre, 1), lambda pre: row(pre, 2), 4, filtered=False)
    N = 200000
    bar = LL.bar_fp32(LL._dof(t.prob, N))
    for defect in (None,) + LL.DEFECTS:
        s, (tests, acc) = LL.simulate(t, 2, N, rng, defect)
        c, o = t.classify(s)
        x2, dof = LL.pearson(c, o, t.prob, N)
        print(f"table V=6: {defect}: X2 {x2:.0f} on {dof} dof (bar {bar:.0f}), acceptance {acc / tests:.2f}")
        assert (x2 < bar) if defect is None else (x2 > 4 * bar), (defect, x2, bar)
    c, o = t.classify(LL.simulate_ar(t, N, rng))
    assert LL.pearson(c, o, t.prob, N)[0] < bar


def test_chosen_inputs_meet_the_conditions_and_the_power_table():
    print(f"\ngamma {LL.GAMMA}, M {LL.M_TOKENS}, seeds SEED_BASE + i = {LL.SEED_BASE:#x} + i, random_seed None, simulator seed {SIM_SEED}")
    assert LL.M_TOKENS >= LL.GAMMA + 2
    print(f"{'case':26s} {'N':>6s} {'dof':>4s} {'lam_ref':>8s} {'cap':>6s} {'bar':>7s} {'acc':>5s} | correct AR | "
          + " ".join(f"{d:>14s}" for d in LL.DEFECTS))
    for name, spec in LL.CASES.items():
        cs = LL.case(name)
        rng = np.random.default_rng(SIM_SEED)
        assert spec["N"] == cs.N and cs.gamma == LL.GAMMA and cs.M == LL.M_TOKENS
        if cs.kind != "fp32":
            assert cs.top_k == 0, "no 16-bit filtered case is admissible (see the gap search below)"
            assert 2.25 * cs.lam <= cs.dof / 2, (name, cs.lam, cs.dof)
            assert cs.bar == LL.bar_16bit(cs.dof, cs.lam) > LL.bar_fp32(cs.dof)
        else:
            assert cs.lam == 0.0 and cs.bar == LL.bar_fp32(cs.dof)
        s, (tests, acc) = LL.simulate(cs.tree, cs.gamma, cs.N, rng)
        rate = acc / tests
        assert 0.30 <= rate <= 0.80, (name, rate)
        x2_ok = LL.x2_of(cs, s)[0]
        x2_ar = LL.x2_of(cs, LL.simulate_ar(cs.tree, cs.N, rng))[0]
        assert x2_ok < cs.bar and x2_ar < cs.bar, (name, x2_ok, x2_ar, cs.bar)
        cells = []
        for d in LL.DEFECTS:
            if d == "same_noise" and cs.kind != "fp32":
                assert d not in LL.CLAIMS[name]
                cells.append(f"{'not simulated':>14s}")
                continue
            x2 = LL.x2_of(cs, LL.simulate(cs.tree, cs.gamma, cs.N, rng, d)[0])[0]
            claimed = d in LL.CLAIMS[name]
            if claimed:
                assert x2 >= 2 * cs.bar, (name, d, x2, cs.bar)
            cells.append(f"{min(x2, 9.9e9):>11.0f}{' ok' if claimed else ' --'}")
        print(f"{name:26s} {cs.N:6d} {cs.dof:4d} {cs.lam:8.2f} {cs.dof / 4.5:6.1f} {cs.bar:7.1f} {rate:5.2f} | {x2_ok:6.0f} {x2_ar:4.0f} | "
              + " ".join(cells))
    print("ok = claimed (X2 >= 2 x bar), -- = this case cannot see the defect")
    for name in ("fp32_filtered", "bf16_plain"):
        cs = LL.case(name)
        print(f"{name}: prompt default_rng({LL.CASES[name]['prompt'][0]}).integers(3, V, {LL.CASES[name]['prompt'][1]}), T {cs.temperature}, "
              f"top_k {cs.top_k}, {len(cs.tree.cells)} cells")


def test_models_are_the_suites_own():
    """The fp32 pair is _pair("corr") and the 16-bit model BF16_CFG of tests/test_gpu_native_parity.py, tensor for tensor."""
    import torch
    import test_gpu_native_parity as NP
    assert LL.CFG16 == NP.BF16_CFG
    for mine, theirs in zip(LL.fp32_pair(), NP._pair("corr")):
        if isinstance(mine, dict):
            assert mine.keys() == theirs.keys() and all(torch.equal(mine[k], theirs[k]) for k in mine)
        else:
            assert mine == theirs


def test_m_equal_gamma_hides_the_bonus_row_defect():
    """Why M >= gamma + 2: at gamma = 4, M = 4 no bonus token is among the observed four, and 'bonus from the previous row'
    fits like the correct loop; at gamma = 2, M = 4 it is the largest signal of all."""
    cs = LL.case("fp32_filtered")
    rng = np.random.default_rng(SIM_SEED)
    hidden = LL.x2_of(cs, LL.simulate(cs.tree, 4, cs.N, rng, "bonus_prev_row")[0])[0]
    seen = LL.x2_of(cs, LL.simulate(cs.tree, 2, cs.N, rng, "bonus_prev_row")[0])[0]
    print(f"bonus_prev_row at M = 4: gamma 4 -> X2 {hidden:.0f}, gamma 2 -> X2 {seen:.0f}, bar {cs.bar:.0f}")
    assert hidden < cs.bar < 2 * cs.bar < seen


def test_no_16bit_filtered_case_is_admissible():
    """A 16-bit top_k case needs a prompt where, at every prefix of the tree, the gap between the k-th and (k + 1)-th scaled
    logit is >= 8 x the same-dtype oracle's worst logit error on that tree (rounding then cannot move the k-th token).  With
    40 prefixes and V = 8192 the smallest gap is ~1e-2 at best and the error 7e-2 (bf16) / 9e-3 (fp16): none of the prompts
    tried (8 here; 24 per dtype when the cases were chosen) comes within a factor of 5, and the same-dtype oracle puts up to
    35 % of a conditional's mass outside the fp32 support.  So the 16-bit cases run plain softmax with rank cells only."""
    for kind in ("bf16", "fp16"):
        best = 0.0
        for seed in range(8):
            gap, err, leak = LL.kth_gap(kind, (seed, 24), 2.0, 3)
            best = max(best, gap / err)
            print(f"{kind} prompt seed {seed}: smallest k-th gap {gap:.4f}, worst logit error {err:.4f} (ratio {gap / err:.2f}, 8 needed), "
                  f"mass outside the fp32 support {leak:.3f}")
        assert best < 8.0, "an admissible prompt exists: add the 16-bit filtered case"
