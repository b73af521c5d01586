"""The device RNG against an independent implementation (`pytest -m gpu`): sd_philox_uniform must equal
tests/philox_reference.py bit for bit, sd_philox_exp must lie within 4 fp32 ulp of the float64 -log(u) of the reference's
exact u (u is exact, so the only error is the device's logf and one rounding).  The sweep walks the fields where an
implementation goes wrong: the element (word choice elem & 3, block elem >> 2, up to OPT's 50271), the draw index across
2^32, the seed's high word and bit 63, neighbouring seeds, and a uniform call of more than one block (draw + i in 64 bits).
The replay tests (tests/philox_replay.py) feed the device's own variates to the oracle and so cannot see any of this.

Then the kernel-level companion of tests/test_gpu_lossless.py: sd_sample + sd_accept_resample_batch on probability tables that
depend on the position only, so that a failed fit of a model-level case can be pinned on the kernels or cleared of them."""
import ctypes as C

import numpy as np
import pytest
import torch

import lossless as LL
import philox_reference as PR
import sampler_rows as R

pytestmark = pytest.mark.gpu

SEEDS = [987654321, 987654322,                       # s and s + 1
         0xABCDEF01 << 32,                           # only high-word bits
         (1 << 63) | 5,                              # bit 63
         0x8000000500000007]
DRAWS = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3]
V_SWEEP = 50272                                      # elements 0 .. 50271: every elem & 3 at 12568 blocks


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib
    return types.SimpleNamespace(lib=_lib.lib, L=_lib)


def _st():
    return torch.cuda.current_stream().cuda_stream


def test_philox_uniform_equals_the_reference_bit_for_bit(hip):
    n = 1000                                         # four blocks of 256: element i is draw + i
    u = torch.empty(n, dtype=torch.float32, device="cuda")
    for seed in SEEDS:
        for draw in DRAWS + [2 ** 32 - 300]:         # the last one crosses 2^32 inside the call
            assert hip.lib.sd_philox_uniform(seed, draw, n, u.data_ptr(), _st()) == 0
            want = PR.uniform(seed, draw, n).astype(np.float32)
            got = u.cpu().numpy()
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (hex(seed), draw, bad[:8], got[bad[:8]], want[bad[:8]])


def test_philox_exp_within_4_ulp_of_the_reference(hip):
    e = torch.empty(V_SWEEP, dtype=torch.float32, device="cuda")
    worst, seen = 0.0, {}
    for seed in SEEDS:
        for draw in DRAWS:
            assert hip.lib.sd_philox_exp(seed, draw, V_SWEEP, e.data_ptr(), _st()) == 0
            got = e.cpu().numpy().astype(np.float64)
            want = PR.exponential(seed, draw, V_SWEEP)
            ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
            err = np.abs(got - want) / ulp
            i = int(err.argmax())
            assert err[i] <= 4.0, (hex(seed), draw, i, got[i], want[i], err[i])
            worst = max(worst, float(err[i]))
            seen[(seed, draw)] = got[:4096].copy()
    print(f"sd_philox_exp: worst error {worst:.2f} fp32 ulp over {len(SEEDS) * len(DRAWS)} draws x {V_SWEEP} elements")
    # the reference says these streams differ; so they do on the device (a dropped high word makes two of them equal)
    keys = list(seen)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            assert (seen[keys[a]] != seen[keys[b]]).mean() > 0.99, (keys[a], keys[b])


# ------------------------------------------------------------------------------------------------- kernel-level companion
GAMMA_K = 2
N_K = 4000                                           # runs per table; 16 per launch


def _norm(x):
    return (x / x.sum()).astype(np.float32)


def _tables():
    """name -> (P, Q): (gamma + 1, V) float32 probability rows that depend on the position only."""
    rng = np.random.default_rng(7)
    out = {}
    V = 64
    p = np.stack([_norm(rng.random(V) ** 3) for _ in range(GAMMA_K + 1)])
    q = np.stack([_norm(rng.random(V) ** 3) for _ in range(GAMMA_K + 1)])
    out["p_equals_q"] = (p, p.copy())
    out["generic"] = (p, q)
    pd, qd = np.zeros_like(p), np.zeros_like(q)
    pd[:, :V // 2], qd[:, V // 2:] = p[:, :V // 2], q[:, V // 2:]
    out["disjoint_supports"] = (np.stack([_norm(r) for r in pd]), np.stack([_norm(r) for r in qd]))
    qz = q.copy()
    qz[:, ::2] = 0.0                                 # q = 0 on half of p's support
    out["q_zero_where_p_positive"] = (p, np.stack([_norm(r) for r in qz]))
    V = 32000
    ids = rng.choice(V, size=20, replace=False)
    ps, qs = np.zeros((GAMMA_K + 1, V), np.float32), np.zeros((GAMMA_K + 1, V), np.float32)
    for r in range(GAMMA_K + 1):
        ps[r, ids], qs[r, ids] = _norm(rng.random(20) ** 2), _norm(rng.random(20) ** 2)
    out["support20_in_32000"] = (ps, qs)
    # the adversarial pairs of tests/sampler_rows.py, as probability rows of the oracle
    import oracle
    g = torch.Generator().manual_seed(3)
    V = 32000
    # target rows: 20 equal maxima / strong tokens that share a slot of the dense residual sum / probabilities that underflow
    x = torch.cat([R.plateau_max(11, V, 20), R.same_slot(12, V), R.wide_range(13, V, clip=False)], 0)
    with R.stable_ties(True):
        pa = oracle.norm_logits(x, 1.0, 20, 0.9).numpy()
        qa = oracle.norm_logits(x + 0.5 * torch.randn(x.shape, generator=g), 1.0, 50, 0.0).numpy()
    out["sampler_rows_adversarial"] = (pa.astype(np.float32), qa.astype(np.float32))
    return out


@pytest.mark.parametrize("name", ["p_equals_q", "generic", "disjoint_supports", "q_zero_where_p_positive",
                                  "support20_in_32000", "sampler_rows_adversarial"])
def test_accept_resample_kernels_emit_the_p_rows(hip, name):
    """One iteration per run, fp32 sampling mode, the loop's draw layout (drafts at d .. d + gamma - 1, uniforms at
    d + gamma + 1 .., residual / bonus at d + 2 gamma + 1): draft with sd_sample from the q rows, then
    sd_accept_resample_batch (16 runs per launch; in every second chunk one run takes sd_accept_resample instead).  With
    tables that depend on the position only the emitted tokens are independent, so: the first token is distributed exactly as p_0 on all N runs; token j, on the runs that accepted j drafts
    (which is when the iteration emits one), exactly as p_j.  Pearson X2 per position over the tokens of expected count
    >= 8 (rest pooled), bar chi2.isf(1e-9, dof); a token outside p_j's support fails outright.  N = 4000 runs, the dense
    passes of the kernel (no candidate lists; the filtered model-level cases take the list route), 0.1 - 0.8 s per table.
    What it sees: a wrong residual (resampling from p fails four of the six tables - not p_equals_q, which never rejects, nor
    disjoint_supports, where max(p - q, 0) IS p), a wrong bonus row, a wrong variate.  What it does not: one uniform shared by
    the accept tests stays just under the bars at this N - the fp32 model-level cases of N = 20000 are its check."""
    lib = hip.lib
    P, Q = _tables()[name]
    V, g, L = P.shape[1], GAMMA_K, 3
    S = L + g + 1
    p_hist, q_hist = torch.zeros((S, V), device="cuda"), torch.zeros((S, V), device="cuda")
    p_hist[L - 1:L + g] = torch.from_numpy(P).cuda()
    q_hist[L - 1:L + g] = torch.from_numpy(Q).cuda()
    res_sz = C.sizeof(hip.L.SdAcceptResult)
    B = 16
    seqs = torch.zeros((B, S + 8), dtype=torch.int32, device="cuda")
    res = torch.zeros((B, res_sz), dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    emitted = [[] for _ in range(g + 1)]
    for c in range(N_K // B):
        items = (hip.L.SdAcceptItem * B)()
        lptr = (C.c_void_p * B)()
        for s in range(B):
            seed, d = LL.SEED_BASE + c * B + s, 0
            for i in range(g):
                hip.L.check(lib.sd_sample(q_hist[L - 1 + i].data_ptr(), V, None, seed, d + i, seqs[s, L + i:].data_ptr(),
                                          err.data_ptr(), 0, _st()))
            it = items[s]
            it.p_hist, it.q_hist, it.seq, it.L = p_hist.data_ptr(), q_hist.data_ptr(), seqs[s].data_ptr(), L
            it.r, it.exp_noise = None, None
            it.philox_seed, it.draw_scan, it.draw_resample = seed, d + g + 1, d + 2 * g + 1
            it.res, it.err_flags, it.n_err = res[s].data_ptr(), None, 0
            lptr[s] = None
        if c % 2:                                    # odd chunks: all 16 runs in one launch
            hip.L.check(lib.sd_accept_resample_batch(items, B, V, V, g, 0, lptr, _st()))
        else:                                        # even chunks: run 0 through the single-stream entry, 15 in the batch
            it = items[0]
            hip.L.check(lib.sd_accept_resample(it.p_hist, it.q_hist, V, V, it.seq, L, g, None, it.philox_seed, it.draw_scan,
                                               it.draw_resample, it.res, None, 0, 0, None, _st()))
            rest = (hip.L.SdAcceptItem * (B - 1))(*list(items)[1:])
            hip.L.check(lib.sd_accept_resample_batch(rest, B - 1, V, V, g, 0, lptr, _st()))
        torch.cuda.synchronize()
        assert int(err) == 0
        rb, sq = res.cpu().numpy(), seqs.cpu().numpy()
        for s in range(B):
            a = hip.L.SdAcceptResult.from_buffer_copy(rb[s].tobytes())
            assert 0 <= a.n_accepted <= g and a.n == L + a.n_accepted - 1 and int(sq[s, a.n + 1]) == a.next_token
            for j in range(a.n_accepted + 1):
                emitted[j].append(int(sq[s, L + j]))
    from scipy import stats
    for j in range(g + 1):
        toks = np.array(emitted[j])
        n = len(toks)
        if n < 200:
            print(f"{name}: position {j} emitted on {n} runs only - not tested")
            assert j > 0
            continue
        p = P[j].astype(np.float64)
        p = p / p.sum()
        counts = np.bincount(toks, minlength=V)
        assert counts[p == 0].sum() == 0, (name, j, "token outside the support of p")
        x2, dof = LL.pearson(counts, 0, p, n)
        bar = stats.chi2.isf(LL.ALPHA, dof)
        print(f"{name}: position {j}, {n} runs: X2 {x2:.1f} on {dof} dof, bar {bar:.1f}")
        assert x2 < bar
    assert len(emitted[0]) == N_K
    if name == "p_equals_q":
        assert len(emitted[g]) == N_K                # ratio 1: nothing is ever rejected
    if name == "disjoint_supports":
        assert len(emitted[1]) == 0                  # p(x) = 0 for every drafted x: always rejected
