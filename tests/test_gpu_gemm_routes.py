"""Every kernel instance, wave grid and cut the GEMM planner selects, run once as an integer-exact GEMM (`pytest -m gpu`).

tests/gemm_route_classes.py enumerates the planner's classes through sd_gemm_route - over the layer shapes of the packaged
configs, the public Llama / OPT cards, their tensor-parallel shards and synthetic edges, at 1..256 rows, for x_tiled,
row-major, fused-plan and one-slab calls, under the default tunables and the ones that reach further instances - and keeps
the smallest witness of each class.  Here every witness runs through sd_gemm_bf16_need (launch_gemm<EPI_PART> on the route
the query reported + the slab fold) with W in {-2..2} and X in {-4..4}: every product and partial sum is an integer below
2^24 (8 K <= 294 912), so the fp32 result is the same in any summation order and must equal the integer matmul bit for bit.
No tolerance anywhere.

Unlike a fresh buffer, a session's operand rows past M hold what an earlier, larger pass left there, and its slab buffer old
slabs: so the operand's padding rows, `part` and `out` are NaN before every call, and guard bytes behind `part` and `out`
must survive it.  A kernel that folds a padding row into a real one, reads a slab it did not write or writes past its slabs
shows up as NaN or a guard hit, not as a small difference."""
import ctypes as C

import pytest
import torch

import gemm_route_classes as G
from llmspeculativesampling_amd import _lib
from test_gemm_routes_cpu import COUNTS, WITNESS_SHAPES            # (pinned there: collecting this file costs no sweep)

pytestmark = pytest.mark.gpu

GUARD_BYTE, GUARD_FLOATS = 0x5A, 4096


@pytest.fixture(scope="module")
def witness_list():
    return G.witnesses(G.RUN_NEEDS)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _guarded(floats):
    """`floats` NaN floats followed by GUARD_FLOATS floats of guard bytes."""
    buf = torch.full(((floats + GUARD_FLOATS) * 4,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    buf[:floats * 4].view(torch.float32).fill_(float("nan"))
    return buf, buf[:floats * 4].view(torch.float32)


def test_the_cases_below_cover_every_witness(witness_list):
    """One witness per class, every class once, and every witness sits on a shape that has a case below: the planner on
    this machine (its CU count) selects what tests/test_gemm_routes_cpu.py counted."""
    keys = [w[5] for w in witness_list]
    assert len(keys) == len(set(keys)) == COUNTS["with_tunables"]
    assert sum(1 for w in witness_list if not w[4]) == COUNTS["runnable"]
    assert sorted({(w[0], w[1]) for w in witness_list}) == sorted(WITNESS_SHAPES)


@pytest.mark.parametrize("shape", WITNESS_SHAPES, ids=[f"{n}x{k}" for n, k in WITNESS_SHAPES])
def test_every_planned_instance_is_integer_exact(witness_list, shape):
    N, K = shape
    mine = [w for w in witness_list if (w[0], w[1]) == shape]
    assert mine, shape
    lib = _lib.lib
    g = torch.Generator(device="cuda").manual_seed(N * 31 + K)
    W = torch.randint(-2, 3, (N, K), device="cuda", generator=g, dtype=torch.int8).to(torch.bfloat16)
    Wp = torch.empty_like(W)
    _lib.check(lib.sd_pack_weight_bf16(W.data_ptr(), Wp.data_ptr(), N, K, _st()), "sd_pack_weight_bf16")
    Wd = W.double().t().contiguous()
    del W
    for _, _, M, need, env, key in mine:
        at = (N, K, M, G.need_name(need), env, key)
        Mpad = (M + 15) // 16 * 16
        X = torch.randint(-4, 5, (M, K), device="cuda", generator=g, dtype=torch.int8).to(torch.bfloat16)
        want = (X.double() @ Wd).float()
        # the operand as a session holds it: Mpad rows, the rows past M stale (NaN) in either layout
        Xbuf = torch.full((Mpad * K,), float("nan"), dtype=torch.bfloat16, device="cuda")
        if need & G.ROWMAJOR:
            Xbuf[:M * K].copy_(X.reshape(-1))
        else:
            _lib.check(lib.sd_pack_activation_bf16(X.data_ptr(), Xbuf.data_ptr(), M, K, _st()), "sd_pack_activation_bf16")
        with G.tunables(env):
            r = G.route(N, K, M, need)
            assert G.class_key(N, K, M, need, r) == key, at       # the class this witness stands for is the one that runs
            part_floats = r.part_floats
            assert part_floats == r.S * Mpad * N
            part_buf, part = _guarded(part_floats)
            out_buf, out = _guarded(M * N)
            S = C.c_int(0)
            rc = lib.sd_gemm_bf16_need(Wp.data_ptr(), Xbuf.data_ptr(), M, N, K, need, part.data_ptr(), part_floats,
                                       out.data_ptr(), C.byref(S), _st())
        assert rc == 0, (at, lib.sd_last_error())
        torch.cuda.synchronize()
        assert S.value == r.S, at
        got = out.view(M, N)
        bad = int((got != want).sum())                             # (NaN != anything: an unwritten or poisoned element counts)
        assert bad == 0 and torch.equal(got, want), (at, f"{bad} of {M * N} elements differ", r)
        assert bool((part_buf[part_floats * 4:] == GUARD_BYTE).all()), (at, "wrote past the slabs")
        assert bool((out_buf[M * N * 4:] == GUARD_BYTE).all()), (at, "wrote past out")
        del part_buf, part, out_buf, out, Xbuf, want
