"""Conditions on the inputs of tests/test_gpu_sampler_routes.py, decided by the oracle alone (no GPU):
the fp32 cases keep the top-p cut at least 1e-5 of cumulative mass away from top_p, at most 5 % of the 16-bit cases are
denominator-sensitive, the (route, family) table is complete, and the oracle's stable and unstable tie orders agree up to
tied logits on every case."""
import numpy as np
import torch

import sampler_rows as R


def test_case_table_covers_every_route_family_pair():
    have = set()
    for c in R.CASES:
        for entry, (s, cl) in c["want"].items():
            assert not s & cl, (c["id"], entry)
            for name, pred in R.REQUIRED_ROUTES.items():
                if pred(s, cl):
                    have.add((name, c["family"]))
    missing = [pr for pr in R.REQUIRED_PAIRS if pr not in have]
    assert not missing, missing
    sizes = {c["V"] for c in R.CASES}
    assert {4096, 4100, 8192, 32000, 32001, 32016, 35840, 35844, 50257, 50272, 65536, 65552, 128256} <= sizes
    settings = {(c["T"], c["k"], c["p"]) for c in R.CASES}
    assert {(1.0, 20, 0.9), (1.0, 1, 0.0), (1.0, 64, 0.0), (1.0, 65, 0.0), (1.0, 64, 0.5), (0.7, 0, 0.9), (1.0, 0, 0.999),
            (1.0, 2000, 0.99), (1.0, 0, 0.0)} <= settings
    assert any(c["k"] == c["V"] and c["p"] == 0.0 for c in R.CASES)


def test_fp32_cases_keep_the_cut_margin():
    bad = []
    for c in R.CASES:
        if c["dt"] == 0 and not c.get("error"):
            m = R.cut_margin(c["make"](), c["T"], c["k"], c["p"])
            if m < 1e-5:
                bad.append((c["id"], m))
    assert not bad, bad


def test_at_most_five_percent_of_lowprec_cases_are_denominator_sensitive():
    n = sens = 0
    for c in R.CASES:
        if c["dt"] and not c.get("error"):
            n += 1
            if R.lowprec_alternative(c["make"](), c["T"], c["k"], c["p"], c["dt"]) is not None:
                sens += 1
                print("denominator-sensitive:", c["id"])
    print(f"denominator-sensitive 16-bit cases: {sens} of {n}")
    assert n >= 40 and sens <= 0.05 * n, (sens, n)


def test_oracle_stable_and_unstable_orders_agree_up_to_tied_logits():
    """and: error cases raise in the oracle, every other case does not"""
    from test_gpu_parity import assert_rows_equal_up_to_tied_logits
    tied = 0
    for c in R.CASES:
        x = c["make"]()
        exp = R.expected(x, c["T"], c["k"], c["p"], c["dt"])
        assert (exp is None) == bool(c.get("error")), c["id"]
        if exp is None:
            continue
        st, un = exp
        tied += not torch.equal(st, un)
        z = R.scaled(x, c["T"], c["dt"])[0].numpy()
        if c["dt"]:
            assert_rows_equal_up_to_tied_logits(st[0].numpy(), un[0].numpy(), z)
        else:
            # fp32: torch's own row sum depends on where the kept entries sit, so the two results differ in a last bit; the
            # kept sets must hold the same logit values (every token that differs has a twin with the same logit)
            np.testing.assert_array_equal(np.sort(z[st[0].numpy() > 0]), np.sort(z[un[0].numpy() > 0]))
            np.testing.assert_allclose(np.sort(st[0].numpy()), np.sort(un[0].numpy()), rtol=1e-6, atol=0)
    print("cases whose kept set depends on the tie order:", tied)
    assert tied >= 5                                    # the table does contain rows the unstable sort decides differently


def test_tie_rate_of_bf16_valued_rows():
    """the headline input: bf16-valued fp32 rows at (1, 20, 0.9) - a tie at the k-th value in about half of them"""
    ties = 0
    for s in range(40):
        z = R.bf16_valued(100 + s, 32000)[0]
        top = torch.topk(z, 21)[0]
        ties += bool(top[19] == top[20])
    print("rows with a tie at the k-th value:", ties, "of 40")
    assert ties >= 10
