"""Token-tree speculative sampling (`pytest -m gpu`): draw and accept walk against numpy, the level-by-level tree forward
against the oracle, the loop's greedy identity and losslessness."""
import ctypes as C

import numpy as np
import pytest
import torch

import lossless as LL
import oracle
from llmspeculativesampling_amd.config import load_config
from llmspeculativesampling_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


_st = lambda: torch.cuda.current_stream().cuda_stream                                                  # noqa: E731
_dev = lambda a, dtype=None: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)  # noqa: E731


def topology(branching):
    """parent / level / child0 / n_child of the breadth-first numbering (include/specdec.h), in plain python."""
    parent, level, start = [0], [0], [0]
    for d, b in enumerate(branching, 1):
        prev = [i for i in range(len(level)) if level[i] == d - 1]
        start.append(len(level))
        for u in prev:
            parent += [u] * b
            level += [d] * b
    n = len(level)
    child0 = [next((i for i in range(1, n) if parent[i] == u), 0) for u in range(n)]
    n_child = [sum(parent[i] == u for i in range(1, n)) for u in range(n)]
    return n, parent, level, child0, n_child, start


# --------------------------------------------------------------------------------------------------------- 1. the draw
@pytest.mark.parametrize("b", [1, 3, 8])
@pytest.mark.parametrize("V", [40, 1000, 4099])
def test_draw_equals_the_sorted_keys(hip, V, b):
    """Rows: dense; two entries with mass (a top_k = 2 row: the tail is -1); a planted exact tie of the two largest keys (the
    lower id first); a dense row under an absent parent (all -1).  Keys q / e in float32, as the kernel: tokens and order equal."""
    rng = np.random.default_rng(V * 10 + b)
    q = rng.random((4, V)).astype(F32)
    q[1] = 0
    q[1, [V - 3, 7]] = [0.25, 0.75]
    e = rng.exponential(size=(4, V)).astype(F32) + F32(1e-3)
    q[2, [V - 5, 11]], e[2, [V - 5, 11]] = 2.0, 1e-4
    parent = np.array([5, 6, 7, -1], dtype=np.int32)
    out = torch.full((4, 8), -7, dtype=torch.int32, device="cuda")
    qd, pd, ed = _dev(q), _dev(parent), _dev(e)
    hip.L.check(hip.lib.sd_tree_draw(qd.data_ptr(), 4, V, V, b, pd.data_ptr(), ed.data_ptr(), V, 0, 0, out.data_ptr(), 8, _st()),
                "sd_tree_draw")
    want = np.full((4, 8), -7)
    for r in range(3):
        key = np.where(q[r] > 0, q[r] / e[r], F32(-1))
        order = [t for t in np.lexsort((np.arange(V), -key)) if q[r, t] > 0][:b]
        want[r, :b] = order + [-1] * (b - len(order))
    want[3, :b] = -1
    assert out.cpu().numpy().tolist() == want.tolist()
    assert want[2, 0] == 11 and (b == 1 or want[2, 1] == V - 5) and (b < 3 or want[1, 2] == -1)


# --------------------------------------------------------------------------------------------------------- 2. the walk
LOW, MID, HIGH, TOK_A = 0, 10, 20, 9       # rejected children: slot 0 LOW, later slots MID + slot; accepted: HIGH + slot; TOK_A: p > 0, residual 0


def _rows(rng, n, V, equal):
    """q: mass 1/4 on tokens 0..9, 1/4 on 10..19, 1/2 on the rest; p = 0.3 q / 1.05 q there and g q on the rest, g spread over
    0.3 .. 2.35 (token V - 1: the largest).  A 'low' child is rejected outright, a 'mid' child after one rejection (ratio about
    0.25); _aim then tunes the one token of the rest that a node's planted accept uses."""
    q = rng.uniform(0.5, 1.5, size=(n, V))
    for lo, hi, mass in ((0, 10, 0.25), (10, 20, 0.25), (20, V, 0.5)):
        q[:, lo:hi] *= mass / q[:, lo:hi].sum(1, keepdims=True)
    p = q.copy()
    if not equal:
        p[:, :10] *= 0.3
        p[:, 10:20] *= 1.05
        p[:, 20:] *= np.append(rng.uniform(0.3, 2.35, size=(n, V - 21)), np.full((n, 1), 3.0), axis=1)
        p[:, 20:] *= (1 - p[:, :20].sum(1, keepdims=True)) / p[:, 20:].sum(1, keepdims=True)
    return p.astype(F32), q.astype(F32)


def _aim(pu, qu, xs, x):
    """Sets p_u[x] so that x's ratio p'/q' is 0.6 after the rejections of xs: a rejection maps every surviving ratio h to
    (h - 1) (1 - q'[y]) / sum, so the wanted start is the inverse of the composed map (thrice: x's own mass moves the sums)."""
    for _ in range(3):
        P, Q, al, be = pu.astype(np.float64), qu.astype(np.float64), 1.0, 0.0
        for y in xs:
            R = np.maximum(P - Q, 0)
            k = (1 - Q[y]) / R.sum()
            al, be, P, Q = al * k, (be - 1) * k, R / R.sum(), np.where(np.arange(len(Q)) == y, 0, Q) / (1 - Q[y])
        pu[x] = F32((0.6 - be) / al * qu[x])


def _plan(V, branching, pattern):
    """The float64 walk with its decisions planted: (tokens, p, q, final noise, uniforms, path, final token, bonus, rejections).
    The child to accept (token HIGH + slot) is given the p that puts its ratio p'/q' at 0.6 when the walk reaches it, fresh and
    after k - 1 rejections alike, so r = ratio (1 - 2m) is the operand that decides; r = ratio (1 + 2m) rejects (capped
    below 1); m = rejections so far * (V + 4) * 2^-23, the worst-case fp32 summation error of the renormalisations."""
    (n, parent, level, child0, n_child, _), D = topology(branching), len(branching)
    rng = np.random.default_rng(V + n)
    p, q = _rows(rng, n, V, pattern == "equal")
    want_at = {"first": lambda d: 0, "equal": lambda d: 0, "kth": lambda d: branching[d] - 1, "none_root": lambda d: None,
               "none_last": lambda d: 0 if d < D - 1 else None, "absent": lambda d: min(1, branching[d] - 1)}[pattern]
    tok = np.zeros(n, dtype=np.int32)
    for i in range(1, n):
        c, w = i - child0[parent[i]], want_at(level[i] - 1)
        tok[i] = -1 if pattern == "absent" and (i == 1 or tok[parent[i]] < 0) else (HIGH if c == w else MID if c else LOW) + c
        if c == w and pattern != "equal" and tok[i] >= 0:
            _aim(p[parent[i]], q[parent[i]], [tok[i - j] for j in range(c, 0, -1) if tok[i - j] >= 0], tok[i])
    e = rng.uniform(1.0, 2.0, size=V).astype(F32)
    e[TOK_A], e[V - 1] = 1e-4, 1e-2
    u, path, r, rounds, bonus = 0, [0], [], 0, False
    P, Q = p[0].astype(np.float64), q[0].astype(np.float64)
    while n_child[u]:
        acc = -1
        for c in range(n_child[u]):
            node = child0[u] + c
            if tok[node] < 0:
                continue
            m = rounds * (V + 4) * 2.0 ** -23
            if c == want_at(level[u]):
                ratio = min(1.0, P[tok[node]] / Q[tok[node]])
                assert pattern == "equal" or 0.3 < ratio < 0.9, ratio       # (the plant itself: the accept must hang on r)
                r.append(min(F32(ratio * (1 - 2 * m)), np.nextafter(F32(ratio), F32(0))))
                acc = node
                break
            x = tok[node]
            r.append(min(F32(min(1.0, P[x] / Q[x]) * (1 + 2 * m)), F32(1 - 2.0 ** -24)))
            rounds += 1
            P = np.maximum(P - Q, 0)
            P, Q = P / P.sum(), np.where(np.arange(V) == x, 0, Q)
            Q = Q / Q.sum()
        if acc < 0:
            break
        u = acc
        path.append(u)
        P, Q = p[u].astype(np.float64), q[u].astype(np.float64)
    else:
        bonus = True
    return tok, p, q, e, r, path, int(np.argmax(np.where(P > 0, P / e, -1))), bonus, rounds


@pytest.mark.parametrize("pattern", ["first", "kth", "none_root", "none_last", "absent", "equal"])
@pytest.mark.parametrize("branching", [(1,), (2, 1), (3, 2, 1), (4, 2, 2), (7, 8)], ids=str)
@pytest.mark.parametrize("V", [40, 4099])
def test_accept_walk_equals_the_float64_walk(hip, V, branching, pattern):
    """Path, depth, final token, flags and uniform count of the planted walk (_plan).  Final draw: TOK_A (p > 0, no residual mass
    once a 'low' child was rejected) has the smallest noise, token V - 1 (residual mass at every stage) the second smallest -
    resampling from p or |p - q| returns TOK_A."""
    tok, p, q, e, r, path, final, bonus, rounds = _plan(V, branching, pattern)
    n, parent, level, child0, n_child, _ = topology(branching)
    D = len(branching)
    topo = hip.L.SdTreeTopology()
    hip.L.check(hip.lib.sd_tree_topology_fill((C.c_int32 * D)(*branching), D, topo), "sd_tree_topology_fill")
    assert (topo.n, list(topo.parent[:n]), list(topo.level[:n]), list(topo.child0[:n]), list(topo.n_child[:n])) == \
        (n, parent, level, child0, n_child)
    res = torch.zeros(C.sizeof(hip.L.SdTreeResult), dtype=torch.uint8, device="cuda")
    idx = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    work = torch.zeros(2 * V, dtype=torch.float32, device="cuda")
    tok_dev, root = _dev(tok), torch.zeros(1, dtype=torch.int32, device="cuda")
    pd, qd, rd, ed = _dev(p), _dev(q), _dev(np.array(r + [0.5] * (n - len(r)), dtype=F32)), _dev(e)
    hip.L.check(hip.lib.sd_tree_accept(topo, tok_dev.data_ptr(), pd.data_ptr(), qd.data_ptr(), V, V, work.data_ptr(), rd.data_ptr(),
                                       ed.data_ptr(), 0, 0, 0, res.data_ptr(), idx.data_ptr(), root.data_ptr(), None, 0, _st()),
                "sd_tree_accept")
    got = hip.L.SdTreeResult.from_buffer_copy(res.cpu().numpy().tobytes())
    a = len(path) - 1
    assert (got.depth, list(got.path[:a + 1]), got.next_token, got.flags, got.n_uniform) == (a, path, final, 4 if bonus else 0, len(r))
    assert idx[:a + 1].tolist() == path and int(root) == final and list(got.tokens[:a + 1]) == [int(tok[i]) for i in path]
    assert bonus == (pattern in ("first", "equal", "kth") or (pattern == "absent" and branching[0] > 1))
    assert final == (TOK_A if bonus or not rounds else V - 1)     # (a bonus draw and a walk without a rejection read p itself)


# --------------------------------------------------------------------------------------------------------- 3. incremental forward
ATOL_PROBS, ATOL_KV = 1e-5, 1e-4             # the fp32 bars of test_gpu_native_parity.py::test_tree_attention_forward_and_rollback_golden


@pytest.mark.parametrize("name", ["tiny-llama-draft", "tiny-llama-target", "tiny-opt-pre"])
def test_tree_forward_level_by_level_equals_one_pass_and_the_oracle(hip, name):
    """A (3, 2, 1) tree behind 5 cached keys, fp32, level by level and in one call (first == 0 is sd_session_forward_tree's
    table): node probabilities and, after sd_session_compact_kv of the last node's path, the kept K and V rows against the oracle."""
    cfg = load_config(name)
    sd = make_state_dict(cfg, 31)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    n, parent, level, _, _, start = topology((3, 2, 1))
    base, V = 5, cfg.vocab_size
    rng = np.random.default_rng(4)
    prompt, toks = rng.integers(3, V, size=base), rng.integers(3, V, size=n)
    bits = [0] * n
    for i in range(n):
        bits[i] = (bits[parent[i]] if i else 0) | 1 << i
    pos = [base + d for d in level]
    path = [n - 1]
    while path[0]:
        path.insert(0, parent[path[0]])
    lm = oracle.RefCausalLM(cfg, sd)
    mask = torch.ones((1, n, base + n), dtype=torch.bool)
    mask[0, :, base:] = torch.tensor([[(b >> j) & 1 == 1 for j in range(n)] for b in bits])
    o = lm(torch.from_numpy(toks[None]), past_key_values=lm(torch.from_numpy(prompt[None])).past_key_values,
           extra_attention_mask=mask, position_ids=torch.tensor([pos]))
    want = torch.softmax(o.logits.float()[0], -1)
    keep = list(range(base)) + [base + i for i in path]
    want_kv = torch.stack([torch.stack([kv[j][0][:, keep] for j in (0, 1)]) for kv in o.past_key_values])   # [layer][k|v][head][kept][D]
    pos_c, bits_c, tok_dev, idx = (C.c_int32 * n)(*pos), (C.c_uint64 * n)(*bits), _dev(toks, torch.int32), _dev(path, torch.int32)
    for levels in (list(zip(start, start[1:] + [n])), [(0, n)]):     # level by level (the leaves too), then the whole tree at once
        ses = m.new_session(64)
        ses.forward(_dev(prompt, torch.int32), 0)
        logits = torch.zeros((n, V), dtype=torch.float32, device="cuda")
        args = (ses.handle, tok_dev.data_ptr(), pos_c, bits_c)
        for first, end in levels:
            hip.L.check(hip.lib.sd_session_forward_tree_from(*args, first, end, base, end - first, logits[first].data_ptr(), V, _st())
                        if len(levels) > 1 else hip.lib.sd_session_forward_tree(*args, n, base, logits.data_ptr(), V, _st()), "tree forward")
        np.testing.assert_allclose(torch.softmax(logits, -1).cpu().numpy(), want.numpy(), atol=ATOL_PROBS)
        hip.L.check(hip.lib.sd_session_compact_kv(ses.handle, base, idx.data_ptr(), len(path), _st()), "sd_session_compact_kv")
        np.testing.assert_allclose(ses.kv[:, :, :, :len(keep)].float().cpu().numpy(), want_kv.numpy(), atol=ATOL_KV)


# --------------------------------------------------------------------------------------------------------- 4. greedy identity
@pytest.mark.parametrize("same", [False, True], ids=["pair", "draft_is_target"])
@pytest.mark.parametrize("branching", [(1, 1, 1), (3, 2, 1), (8,)], ids=str)
def test_greedy_tree_decoding_equals_greedy_autoregressive_decoding(hip, branching, same):
    """top_k = 1, fp32 tiny pair: autoregressive_sampling's tokens; with draft == target every iteration ends at a leaf."""
    dc, dsd, tc, tsd = LL.fp32_pair()
    tm = hip.engine.SpecDecModel.from_state_dict(tc, tsd, dtype=torch.float32)
    dm = tm if same else hip.engine.SpecDecModel.from_state_dict(dc, dsd, dtype=torch.float32)
    prompt = LL.make_prompt(tc, 5, 7).cuda()
    want = hip.S.autoregressive_sampling(prompt, tm, 24, -1, 1, 1, 0.0, rng=hip.noise.DeviceNoise(1))
    got, det = hip.S.tree_speculative_sampling(prompt, dm, tm, -1, None, 24, branching=branching, top_k=1, details=True,
                                               rng=hip.noise.DeviceNoise(2))
    assert got[0, :want.shape[1]].tolist() == want[0].tolist()
    assert det["target_call_times"] == len(det["acc_len"]) and (not same or set(det["acc_len"]) == {len(branching)})


# --------------------------------------------------------------------------------------------------------- 5. lossless
@pytest.mark.parametrize("name,same", [("single_fp32_filtered", False), ("single_bf16_plain", False), ("single_fp32_filtered", True)],
                         ids=["fp32", "bf16", "fp32_draft_is_target"])
def test_tree_loop_is_distributed_as_the_target(hip, name, same):
    """One call per run on the cases, seeds, cells and bars of test_gpu_lossless.py's single-stream test; branching (2, 2)."""
    cs = LL.case(name)
    dc, dsd, tc, tsd = LL.models(cs.kind)
    tm = hip.engine.SpecDecModel.from_state_dict(tc, tsd, dtype=LL.DTYPES[cs.kind])
    dm = tm if same else hip.engine.SpecDecModel.from_state_dict(dc, dsd, dtype=LL.DTYPES[cs.kind])
    prompt, L = cs.prompt.cuda(), cs.prompt.shape[1]
    outs = [hip.S.tree_speculative_sampling(prompt, dm, tm, -1, None, cs.M, branching=(2, 2), temperature=cs.temperature,
                                            top_k=cs.top_k, top_p=0.0, rng=hip.noise.DeviceNoise(LL.SEED_BASE + i)).cpu()
            for i in range(cs.N)]
    samples = np.array([o[0, L:L + cs.M].tolist() for o in outs], dtype=np.int64)
    x2, dof, outside = LL.x2_of(cs, samples)
    print(f"tree loop [{cs.name}, draft is target {same}]: X2 {x2:.1f} on {dof} dof, bar {cs.bar:.1f} (N {cs.N}), {outside} samples "
          f"outside the support")
    assert samples.shape == (cs.N, cs.M) and dof == cs.dof
    assert cs.kind != "fp32" or outside == 0
    assert x2 < cs.bar
