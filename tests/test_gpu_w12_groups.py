"""Escapes through every burst shape of the GEMMs that stream 12-bit weight records: a wave takes a group of four k-steps
(the finishing GEMM also a tail of one to three) at a time, and the finishing GEMM decodes the burst straight-line and
repairs its escapes behind one branch, so what is planted (tests/w12_groups.py) is escapes in each tile of a group alone, in all four with counts 1, 2, 3
and 6, in the first and the last group of a wave's range, next to groups without, in the tails, at the first and the last
element of a tile and twice in one lane - in gate/up of layer 0, QKV of layer 1 and down of layer 0.  The plan is checked on
the host (no GPU); on the GPU the forward pass on records must equal the bf16 route on the same weights bit for bit."""
import os

import numpy as np
import pytest
import torch

import w12_groups as G

# intermediate 2816: the harness of test_gpu_w12.py (down: 4 slabs of 22 k-steps, waves of 6 = a group and a tail of two);
# 2560: 3 slabs of 27 / 27 / 26 k-steps, waves of 7 | 6 | 5 = tails of three, two and one
INTERMEDIATE = (2816, 2560)
PREFILL, PASSES = 37, (1, 2, 3, 4, 5, 8)


@pytest.mark.parametrize("inter", INTERMEDIATE)
def test_plan_on_host(inter):
    """Every planted tile has exactly its count (it had none before), nothing else changed, every matrix is packable, and
    the cases the kernels distinguish are all there."""
    p = G.plan(inter)
    seen = G.check(p)
    for kind in ("gate_up", "qkv", "down"):
        whats = seen[kind]
        for t in range(4):
            assert any(w.startswith(f"tile {t} alone") for w in whats), (kind, t)
        assert any("first group" in w for w in whats) and any("last group" in w for w in whats)
        assert "all four tiles: 1, 2, 3, 6" in whats and "all four tiles: 6, 3, 2, 1" in whats
    N, K, S, ksp = p.geometry["down"]
    tails = sorted({len(b[2]) for b in G.bursts(K // 32, S, ksp) if b[3]})
    assert tails == {2816: [2], 2560: [1, 2, 3]}[inter]
    for n in tails:
        for what in (f"tail of {n}: last valid tile", f"tail of {n}: every tile", f"tail of {n} with none behind a group with some"):
            assert what in seen["down"]
    for kind in ("gate_up", "qkv"):                          # K = 1024: a wave owns eight k-steps, two groups, no tail
        N, K, S, ksp = p.geometry[kind]
        assert [len(b[2]) for b in G.bursts(K // 32, S, ksp)] == [4] * 8


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine
    return types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine)


def _run(hip, inter, w12):
    """prefill, then the <= 8-row passes: (logits, written KV rows) of every pass and the records-launch counter after each.
    SD_SMALL_PATH=0, sampled when the session is created, keeps the 1..4-row passes on the route of the 13b target."""
    p = G.plan(inter)
    m = hip.engine.SpecDecModel.synthetic(p.cfg, seed=G.SEED, dtype=torch.bfloat16, max_pos=128, method="numpy",
                                          transform=p.transform, w12=w12)
    old = os.environ.get("SD_SMALL_PATH")
    os.environ["SD_SMALL_PATH"] = "0"
    try:
        ses = m.new_session(128)
    finally:
        if old is None:
            del os.environ["SD_SMALL_PATH"]
        else:
            os.environ["SD_SMALL_PATH"] = old
    ids = torch.from_numpy(np.random.default_rng(8).integers(3, p.cfg.vocab_size, size=128)).to(torch.int32).cuda()
    outs, counts, pos = [], [], 0
    for n in (PREFILL,) + PASSES:
        logits = ses.forward(ids[pos:pos + n], min(n, 9)).clone()
        outs.append((logits, ses.kv[:, :, :, pos:pos + n, :].clone()))
        counts.append(ses.w12_launches())
        pos += n
    torch.cuda.synchronize()
    return m.w12_packed, outs, counts


@pytest.mark.gpu
@pytest.mark.parametrize("inter", INTERMEDIATE)
def test_planted_groups_are_bit_identical(hip, inter):
    """The reference is the bf16 route (w12=False) on the same planted weights.  Records are read by QKV of layer 1, gate/up
    of both layers and down of layer 0: four launches per <= 8-row pass, none in the prefill, none on the bf16 model."""
    G.check(G.plan(inter))                                   # the planted counts are exact and every matrix is packable
    packed0, ref, counts0 = _run(hip, inter, False)
    assert packed0 == {} and counts0 == [0] * len(counts0)
    packed, got, counts = _run(hip, inter, True)
    assert packed == {"qkv": [1], "gate_up": [0, 1], "down": [0]}
    assert counts[0] == 0 and np.diff(counts).tolist() == [4] * len(PASSES)
    for i, ((la, ka), (lb, kb)) in enumerate(zip(got, ref)):
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), f"logits of pass {i}"
        assert torch.equal(ka.view(torch.int16), kb.view(torch.int16)), f"KV rows of pass {i}"
