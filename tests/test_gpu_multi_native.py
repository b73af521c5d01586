"""The native width-w loop (sd_spec_multi_generate) and its two kernels.

Every comparison here is exact (torch.equal, ints, float32 bit patterns): the fused scan + resample launch runs the device
functions of the two-launch pair, the winner broadcast moves bytes, and the native loop enqueues the forwards the Python
loop enqueues, so there is no tolerance to choose.  Run with ``pytest -m gpu`` on an MI355X.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import oracle
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict
from test_multi_native_cpu import multi_blocks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    from llmspeculativesampling_amd.sampling import multi
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise, multi=multi)


def _st():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------- 1. fused kernel vs the two-launch pair
def _prob_rows(gen, W, S, V, bf16):
    """(W, S, V) rows with the support a top-k 20 / top-p norm leaves; bf16-valued for the 16-bit dtype_mode."""
    z = torch.randn((W, S, V), generator=gen, device="cuda") * 3.0
    kth = z.topk(20, dim=-1).values[..., -1:]
    p = torch.softmax(z.masked_fill(z < kth, float("-inf")), dim=-1)
    return p.bfloat16().float().contiguous() if bf16 else p.contiguous()


def _run_pair_and_fused(hip, P, Q, seq, L, gamma, r, seed, d_scan, d_res, mode):
    """-> (block bytes, token buffers) of sd_accept_multi + sd_multi_resample and of sd_multi_accept_resample."""
    W, _, V = P.shape
    outs = []
    for fused in (False, True):
        sq = seq.clone()
        items = (hip.L.SdMultiItem * W)()
        for w in range(W):
            items[w].p_hist, items[w].q_hist, items[w].seq = P[w].data_ptr(), Q[w].data_ptr(), sq[w].data_ptr()
        res = torch.zeros(C.sizeof(hip.L.SdMultiResult), dtype=torch.uint8, device="cuda")
        rp = r.data_ptr() if r is not None else None
        if fused:
            hip.L.check(hip.lib.sd_multi_accept_resample(items, W, V, V, L, gamma, rp, seed, d_scan, d_res, res.data_ptr(),
                                                         mode, _st()), "sd_multi_accept_resample")
        else:
            hip.L.check(hip.lib.sd_accept_multi(items, W, V, L, gamma, rp, seed, d_scan, res.data_ptr(), _st()),
                        "sd_accept_multi")
            torch.cuda.synchronize()
            choice = hip.L.SdMultiResult.from_buffer_copy(res.cpu().numpy().tobytes()).choice
            hip.L.check(hip.lib.sd_multi_resample(P[choice].data_ptr(), Q[choice].data_ptr(), V, V, sq[choice].data_ptr(),
                                                  gamma, None, seed, d_res, res.data_ptr(), mode, _st()),
                        "sd_multi_resample")
        torch.cuda.synchronize()
        outs.append((res.cpu(), sq.cpu()))
    return outs


FUSED_SHAPES = list(itertools.product([1, 2, 5, 16], [1, 4, 16], [1024, 32000, 50272], [0, 16]))


@pytest.mark.parametrize("W,gamma,V,mode", FUSED_SHAPES,
                         ids=[f"w{w}_g{g}_V{v}_{'bf16' if m else 'fp32'}" for w, g, v, m in FUSED_SHAPES])
def test_fused_multi_accept_resample_equals_the_two_launch_pair(hip, W, gamma, V, mode):
    """sd_multi_accept_resample against sd_accept_multi followed by sd_multi_resample on the same arenas and Philox
    position: the whole sd_multi_result and every token buffer, byte for byte, on rows built to hit a tie between two
    replicas, nothing accepted anywhere, an early all-accept, q == 0 at a drafted token (inf and NaN ratios), an all-zero
    residual (the fallback to p_n), a resample that raises, and r_const, next to plain Philox rows."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * W + 10 * gamma + V % 7 + mode)
    L = 3
    S = L + gamma + 1
    P0, Q0 = _prob_rows(gen, W, S, V, bool(mode)), _prob_rows(gen, W, S, V, bool(mode))
    # drafted tokens come from the draft rows' support, half of them their mode
    tok = Q0.argmax(dim=-1)
    alt = torch.multinomial(Q0.reshape(-1, V), 1, generator=gen).reshape(W, S)
    seq0 = torch.zeros((W, S + 2), dtype=torch.int32, device="cuda")
    seq0[:, :L] = 7
    for i in range(gamma):
        seq0[:, L + i] = (tok if i % 2 == 0 else alt)[:, L + i - 1].to(torch.int32)
    seed = 99 + W
    SdMR = hip.L.SdMultiResult

    def block(b):
        return SdMR.from_buffer_copy(b.numpy().tobytes())

    def at(w, i):                                                  # (row, token) of replica w's i-th drafted token
        return w, L + i - 1, int(seq0[w, L + i])

    scenarios = {}
    scenarios["philox"] = (P0, Q0, None)
    # r_const: one uniform repeated, as the random_seed quirk hands it over
    scenarios["r_const"] = (P0, Q0, torch.full((W * gamma,), 0.37, device="cuda"))
    # nothing accepted anywhere: p == 0 at every replica's first drafted token -> replica 0 wins with l = 0
    P = P0.clone()
    for w in range(W):
        P[at(w, 0)] = 0.0
    scenarios["none_accepted"] = (P, Q0, None)
    # q == 0 at a drafted token: p > 0 -> inf ratio (accepted), p == 0 -> NaN ratio (rejects)
    P, Q = P0.clone(), Q0.clone()
    Q[at(0, 0)] = 0.0
    P[at(0, 0)] = 0.25
    if W > 1:
        Q[at(1, 0)] = 0.0
        P[at(1, 0)] = 0.0
    scenarios["q_zero"] = (P, Q, None)
    # an all-zero residual at the rejected row: q = 2 p there (ratio 1/2 < r) -> max_fn(p - q) == 0 -> sample(p_n)
    P, Q = P0.clone(), Q0.clone()
    for w in range(W):
        Q[w, L - 1] = (P[w, L - 1] * 2.0)
    scenarios["zero_residual"] = (P, Q, torch.full((W * gamma,), 0.9, device="cuda"))
    # the resample itself raises: p_n and q_n all zero -> NaN ratio rejects, the residual and the fallback row are all-zero
    # -> flags bit1, next_token -1, no token written
    P, Q = P0.clone(), Q0.clone()
    P[:, L - 1] = 0.0
    Q[:, L - 1] = 0.0
    scenarios["resample_raises"] = (P, Q, None)
    if W > 1:
        # a tie: replicas 0 and 1 hold the same rows and tokens and see the same uniform; both accept exactly
        # min(2, gamma - 1) tokens (ratio 1, then p == 0), every other replica rejects at once -> the first one wins
        P, Q, sq = P0.clone(), Q0.clone(), seq0.clone()
        P[1], Q[1], sq[1] = P[0], Q[0], sq[0]
        keep = min(2, gamma - 1)
        for w in range(W):
            for i in range(gamma):
                row, j = L + i - 1, int(sq[w, L + i])
                if w < 2 and i < keep:
                    P[w, row, j] = Q[w, row, j]
                elif i == (keep if w < 2 else 0):
                    P[w, row, j] = 0.0
        scenarios["tie"] = (P, Q, torch.full((W * gamma,), 0.5, device="cuda"), sq)
        # replica 0 rejects its first token, replica 1 accepts all gamma (p == q) and ends the scan
        P, Q = P0.clone(), Q0.clone()
        P[at(0, 0)] = 0.0
        P[1] = Q[1]
        scenarios["early_all_accept"] = (P, Q, None)
    for name, sc in scenarios.items():
        Pn, Qn, r = sc[:3]
        sq = sc[3] if len(sc) > 3 else seq0
        (a_res, a_seq), (b_res, b_seq) = _run_pair_and_fused(hip, Pn, Qn, sq, L, gamma, r, seed, 11, 11 + W * gamma, mode)
        assert torch.equal(a_res, b_res), (name, "result block")
        assert torch.equal(a_seq, b_seq), (name, "token buffers")
        out = block(b_res)
        assert out.width == W and out.gamma == gamma
        if name == "resample_raises":
            assert (out.choice, out.chosen.n_accepted, out.chosen.next_token) == (0, 0, -1) and out.chosen.flags & 2, name
            assert torch.equal(b_seq, sq.cpu()), name
            continue
        assert out.chosen.next_token >= 0 and int(b_seq[out.choice, out.chosen.n + 1]) == out.chosen.next_token, name
        if name == "none_accepted":
            assert (out.choice, out.chosen.n_accepted, out.chosen.n, out.n_uniform) == (0, 0, L - 1, W), name
        if name == "tie":
            assert (out.choice, out.chosen.n_accepted) == (0, min(2, gamma - 1)), name
        if name == "early_all_accept":
            assert (out.choice, out.chosen.n_accepted, out.n_uniform) == (1, gamma, 1 + gamma) and out.chosen.flags & 4, name
        if name == "zero_residual":
            assert out.chosen.n_accepted == 0 and out.chosen.flags & 1 and not out.chosen.flags & 2, name
        if name == "q_zero":
            assert np.isinf(np.float32(out.p_at[0]) / np.float32(out.q_at[0])), name
            if W > 1:
                assert out.q_at[16] == 0.0 and out.p_at[16] == 0.0 and not (out.choice == 1 and out.chosen.n_accepted > 0), name


# --------------------------------------------------------------------------- 2. adopt kernel vs slicing
ADOPT_ARENAS = [  # (id, torch dtype of the typed view, n_layers, n_kv_heads, head_dim) for draft / target
    ("fp32_d32_d64", torch.float32, (2, 4, 32), (3, 4, 64)),
    ("bf16_d64_d128_gqa", torch.bfloat16, (2, 2, 64), (2, 2, 128)),
    ("fp8_d32_d128", torch.uint8, (1, 4, 32), (2, 8, 128)),
    ("bf16_d32_fp_gqa", torch.bfloat16, (2, 1, 32), (2, 2, 64)),
]


@pytest.mark.parametrize("name,dtype,dshape,tshape", ADOPT_ARENAS, ids=[a[0] for a in ADOPT_ARENAS])
def test_multi_adopt_kernel_equals_the_slice_copies_of_the_python_loop(hip, name, dtype, dshape, tshape):
    """sd_multi_adopt on arenas of distinct random bytes, for every `choice`, all-accept / partial / no accept and an empty
    range, against ``kv[:, :, :, lo:hi].copy_`` and ``seq[L:n+2].copy_`` as multi.py makes them: every byte of every
    replica's two arenas and token buffer - the ranges were copied and nothing outside them was touched."""
    W, L, gamma, max_seq = 4, 9, 4, 24
    seq_cap = max_seq + 1
    gen = torch.Generator(device="cuda").manual_seed(5)
    esz = torch.empty((), dtype=dtype).element_size()

    def arenas(shape):
        nl, hkv, D = shape
        return [torch.randint(0, 256, (nl, 2, hkv, max_seq, D * esz), generator=gen, dtype=torch.uint8, device="cuda")
                for _ in range(W)]

    d0, t0 = arenas(dshape), arenas(tshape)
    s0 = [torch.randint(0, 1 << 30, (seq_cap,), generator=gen, dtype=torch.int32, device="cuda") for _ in range(W)]

    def typed(a):                                                  # the tensor the Python loop slices
        return a.view(dtype)

    cases = []                                                     # (n, all_accept, d_lo, t_lo)
    for l, allacc in ((0, False), (2, False), (gamma, True), (gamma, False)):
        n = L + l - 1
        for d_lo, t_lo in ((L - 2, L - 1), (L - 1, L - 1)):
            cases.append((n, allacc, d_lo, t_lo))
        nd, nt = min(L + gamma - 1, n + 1), (L + gamma if allacc else n + 1)
        cases.append((n, allacc, nd, nt))                          # empty ranges: lo == hi
    for choice in range(W):
        for n, allacc, d_lo, t_lo in cases:
            d, t, s = [a.clone() for a in d0], [a.clone() for a in t0], [a.clone() for a in s0]
            wd, wt, ws = [a.clone() for a in d0], [a.clone() for a in t0], [a.clone() for a in s0]
            new_draft = min(L + gamma - 1, n + 1)
            new_target = L + gamma if allacc else n + 1
            for w in range(W):
                if w != choice:
                    ws[w][L:n + 2].copy_(ws[choice][L:n + 2])
                    if new_draft > d_lo:
                        typed(wd[w])[:, :, :, d_lo:new_draft].copy_(typed(wd[choice])[:, :, :, d_lo:new_draft])
                    if new_target > t_lo:
                        typed(wt[w])[:, :, :, t_lo:new_target].copy_(typed(wt[choice])[:, :, :, t_lo:new_target])
            blk = hip.L.SdMultiResult()
            blk.choice, blk.width, blk.gamma = choice, W, gamma
            blk.chosen.n, blk.chosen.n_accepted, blk.chosen.flags = n, n - L + 1, (4 if allacc else 0)
            res = torch.frombuffer(bytearray(bytes(blk)), dtype=torch.uint8).cuda()
            items = (hip.L.SdMultiAdoptItem * W)()
            for w in range(W):
                items[w].draft_kv, items[w].target_kv, items[w].seq = d[w].data_ptr(), t[w].data_ptr(), s[w].data_ptr()
            hip.L.check(hip.lib.sd_multi_adopt(items, W, res.data_ptr(), L, gamma, d_lo, t_lo,
                                               dshape[0] * 2 * dshape[1], max_seq, dshape[2] * esz,
                                               tshape[0] * 2 * tshape[1], max_seq, tshape[2] * esz, seq_cap, _st()),
                        "sd_multi_adopt")
            torch.cuda.synchronize()
            for w in range(W):
                tag = (choice, n, allacc, d_lo, t_lo, w)
                assert torch.equal(d[w], wd[w]), ("draft arena",) + tag
                assert torch.equal(t[w], wt[w]), ("target arena",) + tag
                assert torch.equal(s[w], ws[w]), ("tokens",) + tag


def test_multi_adopt_unaligned_buffers_and_foreign_result_block(hip):
    """Token runs start at any 4-byte offset and a caller's arena need not be 16-byte aligned: the byte head / tail path.
    A result block that does not describe the iteration (choice or n out of range) copies nothing."""
    W, L, gamma, max_seq, D = 3, 6, 3, 16, 24                      # 24-byte rows: no run is a multiple of 16
    gen = torch.Generator(device="cuda").manual_seed(9)
    raw = [torch.randint(0, 256, (2 * max_seq * D + 8,), generator=gen, dtype=torch.uint8, device="cuda") for _ in range(W)]
    off = [4, 4, 8]                                                # replica 2 is not congruent to the others mod 16
    s0 = [torch.randint(0, 1 << 30, (max_seq + 3,), generator=gen, dtype=torch.int32, device="cuda") for _ in range(W)]
    for choice, n, bogus in ((0, L + 1, False), (2, L - 1, False), (1, L + gamma - 1, False), (5, L, True), (0, L + gamma, True)):
        kv = [r.clone() for r in raw]
        s = [x.clone() for x in s0]
        want = [r.clone() for r in raw]
        ws = [x.clone() for x in s0]
        view = lambda bufs, w: bufs[w][off[w]:off[w] + 2 * max_seq * D].view(2, max_seq, D)   # noqa: E731
        hi = min(L + gamma - 1, n + 1)
        if not bogus:
            for w in range(W):
                if w != choice:
                    view(want, w)[:, L - 1:hi].copy_(view(want, choice)[:, L - 1:hi])
                    ws[w][L:n + 2].copy_(ws[choice][L:n + 2])
        blk = hip.L.SdMultiResult()
        blk.choice, blk.chosen.n = choice, n
        res = torch.frombuffer(bytearray(bytes(blk)), dtype=torch.uint8).cuda()
        items = (hip.L.SdMultiAdoptItem * W)()
        for w in range(W):
            items[w].draft_kv, items[w].target_kv, items[w].seq = kv[w].data_ptr() + off[w], None, s[w].data_ptr()
        hip.L.check(hip.lib.sd_multi_adopt(items, W, res.data_ptr(), L, gamma, L - 1, 0, 2, max_seq, D, 0, max_seq, D,
                                           max_seq + 3, _st()), "sd_multi_adopt")
        torch.cuda.synchronize()
        for w in range(W):
            assert torch.equal(kv[w], want[w]) and torch.equal(s[w], ws[w]), (choice, n, w)


# --------------------------------------------------------------------------- 3. native loop vs Python loop
def _models(hip, kind, dtype=torch.float32, frac=0.12):
    if kind == "opt":
        dc, tc = load_config("tiny-opt-pre"), load_config("tiny-opt-post")
        dsd, tsd = make_state_dict(dc, 11), make_state_dict(tc, 12)
    elif kind == "opt_post":
        dc = tc = load_config("tiny-opt-post")
        dsd = make_state_dict(dc, 11)
        tsd = perturb_state_dict(dsd, 12, frac)
    elif kind == "bf16":
        dc = tc = ModelConfig(arch="llama", vocab_size=8192, hidden_size=256, intermediate_size=704, num_hidden_layers=2,
                              num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-6)
        dsd = make_state_dict(dc, 5, dtype=torch.bfloat16)
        tsd = {k: v.to(torch.bfloat16) for k, v in perturb_state_dict({a: b.float() for a, b in dsd.items()}, 6, 0.05).items()}
    else:
        dc = tc = load_config("tiny-llama-gqa" if kind == "gqa" else "tiny-llama-target")
        dsd = make_state_dict(dc, 11)
        tsd = dsd if kind == "same" else perturb_state_dict(dsd, 12, frac)
    dm = hip.engine.SpecDecModel.from_state_dict(dc, dsd, dtype=dtype)
    tm = dm if tsd is dsd else hip.engine.SpecDecModel.from_state_dict(tc, tsd, dtype=dtype)
    return dc, dsd, tc, tsd, dm, tm


def _both_loops(hip, monkeypatch, prompt, dm, tm, eos, max_len, seed=77, **kw):
    """-> [(tokens, details, (seed, draw))] of the Python loop (SD_MULTI_NATIVE=0) and of the native loop."""
    runs = []
    for native in (False, True):
        if native:
            monkeypatch.delenv("SD_MULTI_NATIVE", raising=False)
        else:
            monkeypatch.setenv("SD_MULTI_NATIVE", "0")
        nz = hip.noise.DeviceNoise(seed)
        out, d = hip.S.multi_speculative_sampling(prompt, dm, tm, eos, None, max_len, strategy="iid", details=True, rng=nz, **kw)
        runs.append((out, d, (nz.seed, nz.draw)))
    monkeypatch.delenv("SD_MULTI_NATIVE", raising=False)
    return runs


def _assert_same_run(py, nat):
    (a, da, pa), (b, db, pb) = py, nat
    assert torch.equal(a, b), (a.tolist(), b.tolist())
    assert da["acc_len"] == db["acc_len"]
    ra, rb = np.float64(da["acc_rate"]), np.float64(db["acc_rate"])
    assert ra.tobytes() == rb.tobytes() or (np.isnan(ra) and np.isnan(rb)), (ra, rb)
    assert da["target_call_times"] == db["target_call_times"] and da["approx_call_times"] == db["approx_call_times"]
    assert pa == pb, ("final Philox position", pa, pb)
    assert set(da) == set(db)


def _prompt(V, n, seed=3):
    return torch.from_numpy(np.random.default_rng(seed).integers(3, V, size=(1, n))).cuda()


@pytest.mark.parametrize("kind", ["llama", "gqa", "opt", "opt_post"])
def test_native_multi_loop_equals_python_loop_fp32_pairs(hip, monkeypatch, kind):
    dc, _, _, _, dm, tm = _models(hip, kind)
    py, nat = _both_loops(hip, monkeypatch, _prompt(dc.vocab_size, 11), dm, tm, -1, 24, gamma=4, width=4, top_k=20, top_p=0.9)
    _assert_same_run(py, nat)
    assert nat[0].shape[1] >= 11 + 24 and nat[1]["target_call_times"] > 0
    assert nat[1]["approx_time"] > 0 and nat[1]["target_time"] > 0 and nat[1]["other_time"] > 0   # HIP events / host CPU time


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("gamma", [1, 2, 4, 8])
def test_native_multi_loop_equals_python_loop_widths_and_gammas(hip, monkeypatch, width, gamma):
    """(width 16, gamma 8): 16 x 9 verify rows go through two target passes of 8 replicas."""
    dc, _, _, _, dm, tm = _models(hip, "llama")
    py, nat = _both_loops(hip, monkeypatch, _prompt(dc.vocab_size, 9, seed=width), dm, tm, -1, 20, gamma=gamma, width=width,
                          top_k=20, top_p=0.9)
    _assert_same_run(py, nat)


def test_native_multi_loop_bf16_pair(hip, monkeypatch):
    dc, _, _, _, dm, tm = _models(hip, "bf16", dtype=torch.bfloat16)
    py, nat = _both_loops(hip, monkeypatch, _prompt(dc.vocab_size, 24), dm, tm, -1, 40, seed=123, gamma=4, width=4, top_k=20,
                          top_p=0.9)
    _assert_same_run(py, nat)
    assert 0 < sum(nat[1]["acc_len"]) < 4 * len(nat[1]["acc_len"])


def test_native_multi_loop_edge_shapes(hip, monkeypatch):
    dc, _, _, _, dm, tm = _models(hip, "llama")
    V = dc.vocab_size
    kw = dict(top_k=20, top_p=0.9)
    # a one-token prompt: no prefill, the first verify carries gamma + 1 rows at position 0
    _assert_same_run(*_both_loops(hip, monkeypatch, _prompt(V, 1), dm, tm, -1, 9, gamma=3, width=3, **kw))
    # max_len 0 returns the prompt with zero calls
    p = _prompt(V, 12)
    py, nat = _both_loops(hip, monkeypatch, p, dm, tm, -1, 0, gamma=4, width=2, **kw)
    _assert_same_run(py, nat)
    assert torch.equal(nat[0], p) and nat[1]["target_call_times"] == 0 and nat[1]["acc_len"] == []
    # T reached in the middle of an iteration
    py, nat = _both_loops(hip, monkeypatch, _prompt(V, 7), dm, tm, -1, 3, gamma=5, width=2, **kw)
    _assert_same_run(py, nat)
    assert nat[1]["target_call_times"] >= 1 and nat[0].shape[1] >= 10
    # the random_seed quirk: the stream restarts at (random_seed, 0) before every scan
    py, nat = _both_loops(hip, monkeypatch, _prompt(V, 10), dm, tm, -1, 20, gamma=4, width=4, random_seed=42, **kw)
    _assert_same_run(py, nat)
    assert nat[2][0] == 42


def test_native_multi_loop_eos_among_accepted_tokens(hip, monkeypatch):
    dc, _, _, _, dm, tm = _models(hip, "llama", frac=0.05)
    p = _prompt(dc.vocab_size, 10)
    kw = dict(gamma=4, width=2, top_k=5, top_p=0.0)
    (full, d, _), _ = _both_loops(hip, monkeypatch, p, dm, tm, -1, 40, **kw)
    pos, eos = 10, None
    for l in d["acc_len"]:                                         # the first accepted draft that is new to the sequence
        for j in range(l):
            t = int(full[0, pos + j])
            if eos is None and t not in full[0, :pos + j].tolist():
                eos = t
        pos += l + 1
    assert eos is not None, d["acc_len"]
    py, nat = _both_loops(hip, monkeypatch, p, dm, tm, eos, 40, **kw)
    _assert_same_run(py, nat)
    assert nat[0].shape[1] < 10 + 40 and int(nat[0][0, -1]) == eos and nat[0][0].tolist().count(eos) == 1


def test_native_multi_loop_accept_lengths_span_zero_to_gamma(hip, monkeypatch):
    """A perturbed pair at widths 1, 2 and 4: the winner broadcast sees the partial range (n + 1), the all-accept range
    (L + gamma) and a rejected first token."""
    dc, _, _, _, dm, tm = _models(hip, "llama", frac=0.15)
    gamma, seen = 4, set()
    for width in (1, 2, 4):
        py, nat = _both_loops(hip, monkeypatch, _prompt(dc.vocab_size, 10, seed=width), dm, tm, -1, 80, gamma=gamma, width=width,
                              top_k=20, top_p=0.9)
        _assert_same_run(py, nat)
        print("width", width, "acc_len", nat[1]["acc_len"])
        seen |= set(nat[1]["acc_len"])
    assert 0 in seen and gamma in seen and seen & set(range(1, gamma)), seen


# --------------------------------------------------------------------------- 4. native loop vs the oracle
class MultiPhiloxNoise:
    """oracle.noise interface fed from the Philox stream in the draw order of sd_spec_multi_generate: a (rows, V) draw takes
    `rows` consecutive draw indices, one per row; a scan reserves width * gamma indices whatever it consumes; with a truthy
    random_seed the stream restarts at (random_seed, 0) before the scan, whose uniforms are torch.Generator(seed).rand(1)."""

    def __init__(self, lib, seed, width, gamma):
        self.lib, self.seed, self.reserve = lib, int(seed) & 0xFFFFFFFFFFFFFFFF, width * gamma
        self.c, self.uni_start, self.seeded = 0, None, None

    def exponential(self, like):
        if self.uni_start is not None:
            self.c, self.uni_start = self.uni_start + self.reserve, None
        self.seeded = None
        rows, V = like.reshape(-1, like.shape[-1]).shape
        out = torch.empty((rows, V), dtype=torch.float32, device="cuda")
        for r in range(rows):
            assert self.lib.sd_philox_exp(self.seed, self.c + r, V, out[r].data_ptr(), _st()) == 0
        self.c += rows
        return out.cpu().reshape(like.shape)

    def uniform(self):
        if self.seeded is not None:
            return torch.rand(1, generator=torch.Generator().manual_seed(self.seeded))
        if self.uni_start is None:
            self.uni_start = self.c
        out = torch.empty(1, dtype=torch.float32, device="cuda")
        assert self.lib.sd_philox_uniform(self.seed, self.c, 1, out.data_ptr(), _st()) == 0
        self.c += 1
        return out.cpu()

    def reseed(self, seed):
        self.seed, self.c, self.uni_start, self.seeded = int(seed) & 0xFFFFFFFFFFFFFFFF, 0, 0, int(seed)


@pytest.mark.parametrize("kind,width,gamma,kw", [("llama", 2, 2, {}), ("llama", 4, 4, {}), ("llama", 2, 4, {"random_seed": 42}),
                                                 ("opt", 4, 2, {}), ("gqa", 2, 4, {}), ("same", 4, 4, {})],
                         ids=["llama_w2_g2", "llama_w4_g4", "llama_w2_g4_seeded", "opt_w4_g2", "gqa_w2_g4", "same_w4_g4"])
def test_native_multi_loop_equals_oracle_on_the_device_rng_stream(hip, kind, width, gamma, kw):
    dc, dsd, tc, tsd, dm, tm = _models(hip, kind)
    prompt = torch.from_numpy(np.random.default_rng(5).integers(3, dc.vocab_size, size=(1, 13)))
    seed = 4242
    want, wd = oracle.multi_speculative_sampling(prompt, oracle.RefCausalLM(dc, dsd), oracle.RefCausalLM(tc, tsd), 2, None, 20,
                                                 gamma=gamma, width=width, strategy="iid", top_k=20, top_p=0.9, details=True,
                                                 noise=MultiPhiloxNoise(hip.lib, seed, width, gamma), **kw)
    nz = hip.noise.DeviceNoise(seed)
    got, gd = hip.S.multi_speculative_sampling(prompt.cuda(), dm, tm, 2, None, 20, gamma=gamma, width=width, strategy="iid",
                                               top_k=20, top_p=0.9, details=True, rng=nz, **kw)
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    assert gd["acc_len"] == wd["acc_len"]
    assert gd["target_call_times"] == wd["target_call_times"] and gd["approx_call_times"] == wd["approx_call_times"]
    if kind == "same":
        assert all(a == gamma for a in gd["acc_len"])


# --------------------------------------------------------------------------- 5. errors
def test_native_multi_loop_errors_are_printed_and_swallowed_like_the_python_loop(hip, monkeypatch, capsys):
    """The constructions of test_error_paths_match_reference_exceptions: a NaN row in the lm_head.  As the target it is a
    'norm logits error'; as the draft its NaN probability row also fails the draft sample, and a sample word goes before a
    norm word ('prob error').  The other source of 'prob error', a raising resample, cannot be reached through forwards
    (a row that passed the norm's check is non-negative with a positive maximum); its device side is the
    "resample_raises" rows of the fused-kernel test above."""
    cfg = load_config("tiny-llama-draft")
    sd = make_state_dict(cfg, 21)
    bad = {k: v.clone() for k, v in sd.items()}
    bad["lm_head.weight"][7, :] = float("nan")
    good = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    broken = hip.engine.SpecDecModel.from_state_dict(cfg, bad, dtype=torch.float32)
    prompt = torch.arange(3, 12, dtype=torch.int64)[None].cuda()
    for dm, tm in ((good, broken), (broken, good)):
        texts = []
        runs = []
        for native in (False, True):
            monkeypatch.setenv("SD_MULTI_NATIVE", "1" if native else "0")
            nz = hip.noise.DeviceNoise(3)
            out, d = hip.S.multi_speculative_sampling(prompt, dm, tm, 2, None, 8, gamma=4, width=2, strategy="iid", top_k=20,
                                                      top_p=0.9, details=True, rng=nz)
            texts.append(capsys.readouterr().out.strip())
            runs.append((out, d, (nz.seed, nz.draw)))
        assert texts[0] == texts[1] == ("norm logits error" if tm is broken else "prob error"), texts
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[1][0], prompt)
        assert runs[0][1]["target_call_times"] == runs[1][1]["target_call_times"] == 1
        assert runs[0][1]["acc_len"] == runs[1][1]["acc_len"] == [] and runs[0][2] == runs[1][2]
    monkeypatch.delenv("SD_MULTI_NATIVE", raising=False)


def test_native_multi_loop_refuses_bad_width_and_gamma_before_any_launch(hip):
    """width / gamma outside 1..16 and 2 * width beyond a pass: SD_ERR_INVALID, surfaced as SpecDecError; nothing is
    dereferenced or launched (every pointer handed over is null)."""
    sampling, scratch, state = multi_blocks(hip.L)
    for width, gamma in ((17, 4), (0, 4), (4, 17), (4, 0)):
        rc = hip.lib.sd_spec_multi_generate(None, width, gamma, 64, sampling, 0, None, scratch, None, None, state, None)
        assert rc == hip.L.SD_ERR_INVALID
        with pytest.raises(hip.L.SpecDecError, match="width|gamma"):
            hip.multi._check_native(rc)
    cfg = load_config("tiny-llama-draft")
    m = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, 21), dtype=torch.float32)
    prompt = torch.arange(3, 12, dtype=torch.int64)[None].cuda()
    real = hip.engine.Session.__init__

    def small_pass(self, *a, **k):                                 # a session whose verify pass holds 6 rows: 2 * 4 > 6
        real(self, *a, **k)
        self.max_pass_rows = 6
    try:
        hip.engine.Session.__init__ = small_pass
        with pytest.raises(hip.L.SpecDecError, match="2 rows per replica"):
            hip.S.multi_speculative_sampling(prompt, m, m, 2, None, 8, gamma=2, width=4, strategy="iid",
                                             rng=hip.noise.DeviceNoise(1))
    finally:
        hip.engine.Session.__init__ = real


# --------------------------------------------------------------------------- 6. host-RNG modes stay on the Python loop
def test_host_rng_never_reaches_the_native_loop(hip, monkeypatch):
    """A G7 case (recorded host noise) with the native entry patched to raise."""
    from golden_io import events_ragged, load, model_pair
    meta, G7 = load("g7_multi")
    case = meta[0]
    dcfg, dsd, tcfg, tsd = model_pair(case)
    dm = hip.engine.SpecDecModel.from_state_dict(dcfg, dsd, dtype=torch.float32)
    tm = dm if case["target_spec"][0] == "same" else hip.engine.SpecDecModel.from_state_dict(tcfg, tsd, dtype=torch.float32)
    prompt = torch.from_numpy(G7[case["id"] + "_prompt"].astype(np.int64))[None].cuda()

    def boom(*a, **k):
        raise AssertionError("the native loop was entered under host RNG")
    monkeypatch.setattr(hip.multi, "_native_multi_loop", boom)
    nz = hip.noise.ReplayNoise(events_ragged(G7, case["id"]), "cuda")
    out = hip.S.multi_speculative_sampling(prompt, dm, tm, case["eos"], None, case["max_len"], width=case["width"],
                                           strategy="iid", rng=nz, **case["kwargs"])
    np.testing.assert_array_equal(out.cpu().numpy()[0], G7[case["id"] + "_out"])
    with pytest.raises(AssertionError, match="native loop was entered"):
        hip.S.multi_speculative_sampling(prompt, dm, tm, case["eos"], None, case["max_len"], width=case["width"],
                                         strategy="iid", rng=hip.noise.DeviceNoise(1), **case["kwargs"])
