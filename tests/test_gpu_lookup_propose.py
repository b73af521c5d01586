"""sd_lookup_propose on the device (`pytest -m gpu`): tokens, info and every float of the gamma one-hot rows bit-equal to
tests/lookup_reference.py, with guard rows, pad columns and guard tokens around everything the launch may write; then the accept
kernels on the proposer's one-hot rows (the kernel-level companion of tests/test_gpu_lookup_lossless.py, in the style of
test_gpu_philox.py's)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lookup_reference as R
import lossless as LL

pytestmark = pytest.mark.gpu

GUARD_TOK = -777


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib
    return types.SimpleNamespace(lib=_lib.lib, L=_lib)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(hip, seqs, V, gamma, N, m, pad=5):
    """Every sequence of `seqs` through the proposer, 16 items per launch.  Per item the token buffer holds L + gamma tokens and
    two guards, the rows buffer one guard row, the gamma rows and one guard row, all NaN, with ld = V + pad; the q_hist pointer
    is set back by L - 1 rows, so only the rows the launch may touch exist.  -> [(match length, c)] from the device."""
    ld = V + pad
    out = []
    for lo in range(0, len(seqs), 16):
        chunk = seqs[lo:lo + 16]
        items = (hip.L.SdLookupItem * len(chunk))()
        keep = []
        for it, s in zip(items, chunk):
            L = len(s)
            tok = torch.full((L + gamma + 2,), GUARD_TOK, dtype=torch.int32)
            tok[:L] = torch.as_tensor(np.asarray(s), dtype=torch.int32)
            tok = tok.cuda()
            rows = torch.full((gamma + 2, ld), float("nan"), dtype=torch.float32, device="cuda")
            info = torch.full((4,), GUARD_TOK, dtype=torch.int32, device="cuda")
            it.seq, it.L, it.info = tok.data_ptr(), L, info.data_ptr()
            it.q_hist = rows[1].data_ptr() - (L - 1) * ld * 4
            keep.append((tok, rows, info))
        hip.L.check(hip.lib.sd_lookup_propose(items, len(chunk), V, ld, gamma, N, m, _st()), "sd_lookup_propose")
        torch.cuda.synchronize()
        for s, (tok, rows, info) in zip(chunk, keep):
            L = len(s)
            want, k, c = R.propose(s, gamma, N, m)
            tok, rows, info = tok.cpu().numpy(), rows.cpu().numpy(), info.cpu().numpy()
            assert info.tolist() == [k, c, GUARD_TOK, GUARD_TOK], (L, info, k, c)
            np.testing.assert_array_equal(tok[:L], np.asarray(s))
            np.testing.assert_array_equal(tok[L:L + gamma], want)
            assert tok[L + gamma:].tolist() == [GUARD_TOK] * 2
            np.testing.assert_array_equal(rows[1:gamma + 1, :V].view(np.uint32), R.onehot_rows(want, V).view(np.uint32))
            assert np.isnan(rows[0]).all() and np.isnan(rows[gamma + 1]).all() and np.isnan(rows[1:gamma + 1, V:]).all()
            out.append((k, c))
    return out


LENGTHS = [1, 2, 9, 63, 64, 65, 256, 257, 1025, 4097]
PLANTS = [1, 63, 64, 65, 255, 256, 257, "last", None]


def test_one_planted_match_at_every_block_edge(hip):
    """Distinct tokens, so nothing matches, and then the last token planted in front of c: the only countable match sits at
    c in {1, 63, 64, 65, 255, 256, 257, L - 1} (one lane and stride each side of a wave and of the workgroup) or nowhere, for every
    L of the list; V = 50272 (13 windows per row), 16 items of different L and outcomes per launch."""
    V, seqs, want = 50272, [], []
    for L in LENGTHS:
        for c in PLANTS:
            c = L - 1 if c == "last" else c
            s = np.arange(10, 10 + L)
            if c is not None:
                if not 1 <= c <= L - 1:
                    continue
                s[c - 1] = s[L - 1]
            seqs.append(s)
            want.append((0, L - 1) if c is None else (1, c))
    order = np.random.default_rng(0).permutation(len(seqs))        # mix the lengths within a launch
    got = _check(hip, [seqs[i] for i in order], V, 4, 3, 1)
    assert got == [want[i] for i in order]


def test_choice_among_matches_periods_and_long_keys(hip):
    A, B, C_, D, E, X, Y = 3, 4, 5, 6, 7, 8, 9
    cases = [
        ([A, B, X, A, B, Y, A, B], 3, 1, (2, 5)),                  # two matches of equal length: the more recent one
        ([X, A, B, C_, D, Y, C_, E, B, C_], 3, 1, (2, 4)),         # a longer older match against a shorter recent one
        ([A, B, C_, D, Y, C_, E, A, C_], 3, 2, (0, 8)),            # m = 2 cuts the two matches of length 1
        ([A] * 9, 3, 1, (3, 8)),                                   # period 1: the match overlaps the key
        ([A, B] * 5, 3, 1, (3, 8)),                                # period 2
        ([A, B, C_] * 4, 3, 1, (3, 9)),                            # period 3
        ([A, B, C_, D, A, B, C_, D], 8, 1, (4, 4)),                # N = 8 with c < 8: the match length stops at c
        ([A, B, C_, D, E, X, Y, A, B, C_, D, E, X, Y], 8, 8, (0, 13)),   # ... and a match of 7 does not count at m = 8
        ([A, B, C_, D, E, X, Y, D] * 2 + [A], 8, 1, (8, 9)),       # a full key of 8
    ]
    for gamma in (16, 1):
        got = _check(hip, [np.array(s) for s, *_ in cases], 64, gamma, 8, 1)    # (N = 8, m = 1 for all: the reference decides)
        assert len(got) == len(cases)
    for s, N, m, want in cases:
        assert _check(hip, [np.array(s)], 64, 16, N, m) == [want], (s, N, m)


@pytest.mark.parametrize("V", [5, 4099, 50272])
def test_rows_of_any_width_and_alignment(hip, V):
    """ld = V + 5 (odd: the rows start at every offset from a 16-byte boundary), NaN everywhere before the launch, the pad
    columns and the guard rows unchanged; token ids 0 and V - 1 among the drafted ones, and ids past V (all-zero rows)."""
    rng = np.random.default_rng(V)
    seqs = [rng.integers(0, V, size=L) for L in (1, 2, 9, 63, 64, 65, 256, 257)]
    seqs.append(np.array([0, V - 1, 1 % V, 0]))                    # drafts V - 1, 1, 0, V - 1
    seqs.append(np.array([V - 1, 0, 0, V - 1]))
    seqs.append(np.array([V, V + 7, 2 % V, V]))                    # ids outside [0, V): copied, never an index
    got = _check(hip, seqs, V, 4, 3, 1)
    assert got[-3] == (1, 1) and got[-2] == (1, 1) and got[-1] == (1, 1)
    for pad in (0, 1, 2, 3):
        _check(hip, seqs[-3:], V, 3, 3, 1, pad=pad)


# ------------------------------------------------------------------------------------------------- accept kernels on one-hot rows
GAMMA_K, N_K = 2, 4000                                             # test_gpu_philox.py's N and bar (LL.ALPHA)


def _tables(V, drafted):
    rng = np.random.default_rng(7)
    norm = lambda x: (x / x.sum()).astype(np.float32)
    generic = np.stack([norm(rng.random(V) ** 3) for _ in range(GAMMA_K + 1)])
    one, zero = generic.copy(), generic.copy()
    for i, t in enumerate(drafted):                               # the drafted token carries 0.6 of its row: every position is reached
        generic[i, t] = 1.5 * (generic[i].sum() - generic[i, t])
        generic[i] = norm(generic[i])
    for i, t in enumerate(drafted):
        one[i] = 0.0
        one[i, t] = 1.0
        zero[i, t] = 0.0
        zero[i] = norm(zero[i])
    return {"p_one_at_the_draft": one, "p_zero_at_the_draft": zero, "generic": generic}


@pytest.mark.parametrize("name", ["p_one_at_the_draft", "p_zero_at_the_draft", "generic"])
def test_accept_kernels_on_the_proposers_rows_emit_the_p_rows(hip, name):
    """The q rows come from sd_lookup_propose (prompt X A B X: the match at c = 1 drafts A, B), the p tables depend on the
    position only; one iteration per run with the loop's draw layout (uniforms at d + gamma + 1 .., residual / bonus at
    d + 2 gamma + 1), through sd_accept_resample_batch and, for one run of every second chunk, sd_accept_resample.  p[j] = 1
    always accepts all gamma; p[j] = 0 never accepts and the emitted token is distributed as p_0; a generic p gives Pearson X2
    against p_j per position on the runs that emitted one there, bar chi2.isf(ALPHA, dof)."""
    lib = hip.lib
    V, g, B = 64, GAMMA_K, 16
    prompt = [40, 17, 23, 40]
    L = len(prompt)
    drafted, k, c = R.propose(prompt, g, 3, 1)
    assert (drafted.tolist(), k, c) == ([17, 23], 1, 1)
    P = _tables(V, drafted.tolist())[name]
    S = L + g + 1
    p_hist = torch.zeros((S, V), device="cuda")
    p_hist[L - 1:L + g] = torch.from_numpy(P).cuda()
    q_hist = torch.full((B, S, V), float("nan"), device="cuda")
    seqs = torch.zeros((B, S + 8), dtype=torch.int32, device="cuda")
    seqs[:, :L] = torch.tensor(prompt, dtype=torch.int32)
    info = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    res_sz = C.sizeof(hip.L.SdAcceptResult)
    res = torch.zeros((B, res_sz), dtype=torch.uint8, device="cuda")
    litems = (hip.L.SdLookupItem * B)(*[hip.L.SdLookupItem(seqs[s].data_ptr(), L, q_hist[s].data_ptr(), info[s].data_ptr())
                                        for s in range(B)])
    emitted = [[] for _ in range(g + 1)]
    for ch in range(N_K // B):
        hip.L.check(lib.sd_lookup_propose(litems, B, V, V, g, 3, 1, _st()), "sd_lookup_propose")
        items = (hip.L.SdAcceptItem * B)()
        lptr = (C.c_void_p * B)()
        for s in range(B):
            it = items[s]
            it.p_hist, it.q_hist, it.seq, it.L = p_hist.data_ptr(), q_hist[s].data_ptr(), seqs[s].data_ptr(), L
            it.philox_seed, it.draw_scan, it.draw_resample = LL.SEED_BASE + ch * B + s, g + 1, 2 * g + 1
            it.res, it.err_flags, it.n_err = res[s].data_ptr(), None, 0
        if ch % 2:
            hip.L.check(lib.sd_accept_resample_batch(items, B, V, V, g, 0, lptr, _st()))
        else:
            it = items[0]
            hip.L.check(lib.sd_accept_resample(it.p_hist, it.q_hist, V, V, it.seq, L, g, None, it.philox_seed, it.draw_scan,
                                               it.draw_resample, it.res, None, 0, 0, None, _st()))
            rest = (hip.L.SdAcceptItem * (B - 1))(*list(items)[1:])
            hip.L.check(lib.sd_accept_resample_batch(rest, B - 1, V, V, g, 0, lptr, _st()))
        torch.cuda.synchronize()
        rb, sq = res.cpu().numpy(), seqs.cpu().numpy()
        for s in range(B):
            a = hip.L.SdAcceptResult.from_buffer_copy(rb[s].tobytes())
            assert 0 <= a.n_accepted <= g and a.n == L + a.n_accepted - 1 and int(sq[s, a.n + 1]) == a.next_token
            assert list(a.q_at[:g]) == [1.0] * g and list(a.drafted[:g]) == drafted.tolist()
            for j in range(a.n_accepted + 1):
                emitted[j].append(int(sq[s, L + j]))
    from scipy import stats
    assert len(emitted[0]) == N_K
    if name == "p_one_at_the_draft":
        assert len(emitted[g]) == N_K and set(emitted[0]) == {17} and set(emitted[1]) == {23}
    if name == "p_zero_at_the_draft":
        assert len(emitted[1]) == 0
    for j in range(g + 1):
        toks = np.array(emitted[j], dtype=np.int64)
        n = len(toks)
        if n < 200:
            print(f"{name}: position {j} emitted on {n} runs only - not tested")
            assert j > 0
            continue
        p = P[j].astype(np.float64)
        p = p / p.sum()
        counts = np.bincount(toks, minlength=V)
        assert counts[p == 0].sum() == 0, (name, j, "token outside the support of p")
        if (p > 0).sum() == 1:
            continue                                              # (a point mass: the support check is the test)
        x2, dof = LL.pearson(counts, 0, p, n)
        bar = stats.chi2.isf(LL.ALPHA, dof)
        print(f"{name}: position {j}, {n} runs: X2 {x2:.1f} on {dof} dof, bar {bar:.1f}")
        assert x2 < bar
