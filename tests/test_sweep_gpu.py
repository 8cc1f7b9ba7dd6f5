"""Oracle sweep: every tree, tree-put and list-form kernel instantiation in
liblfa.so against the reference (oracle.allreduce / oracle.write,
tests/_half_ref.py for the half types).

The launchers (lfa_k_launch.hpp, lfa_k_iov.hpp) choose a kernel by op,
element type, leaf count, output count, size and the operands' alignment; the
other tests sample that thinly.  Here every reducing pair (133) runs at every
fan-in that selects another body, on every path the element size has, and
every write pair (148) through the binary list form, on inputs whose result
depends on every operand (tests/_sweep.py; tests/test_sweep_cpu.py holds the
inputs and this harness to account without a GPU).  One ~40 KiB shape: two
whole workgroup tiles of the widest body, a partial tile, a partial wave and a
ragged tail.  Every case is one arena: after the call the sentinels between
the operands are intact and the inputs unchanged.

Each test counts the cases it ran against the product of its lists, so a
pair that was skipped fails the test.
"""
import json
import os

import numpy as np
import pytest
import torch

import oracle
from libfabric_amd import atomic
from tests import _sweep as S
from tests._cmp import assert_parity

pytestmark = pytest.mark.gpu

OPS = range(10)


@pytest.fixture(scope="module")
def manifest(golden_dir):
    with open(os.path.join(golden_dir, "manifest.json")) as f:
        return json.load(f)


def _upload(arena: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(arena).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _view(t: torch.Tensor, seg) -> torch.Tensor:
    lo, nb = seg
    return t[lo:lo + nb]


def test_pair_lists_match_the_library(manifest):
    rp, wp = S.reduce_pairs(), S.write_pairs(manifest)
    assert len(rp) == S.N_REDUCE_PAIRS == 133 and len(wp) == S.N_WRITE_PAIRS == 148
    valid = {(op, dt) for op in range(12) for dt in range(18) if atomic.reduce_valid(dt, op) == 0}
    assert valid == set(wp) and {p for p in valid if p[0] <= 9} == set(rp)
    assert sum(len(S.dts_of(op)) for op in OPS) == 133


@pytest.mark.parametrize("op", OPS)
def test_tree_every_pair(op):
    """lfa_reduce_tree_async: 2, 3, 5, 8, 9, 17 and 32 inputs (every leaf body
    with and without pair leaves, both sides of the 8-leaf put-body rule, the
    3..8-input LDS cap) on the vector, co-aligned-off-boundary, element and
    bytes paths, and on the vector path with the output aliasing the highest
    input and input 0."""
    rng = np.random.default_rng(2000 + op)
    ran = 0
    for dt in S.dts_of(op):
        assert atomic.reduce_valid(dt, op) == 0
        n = S.lanes(S.esz_of(dt))
        for case in S.tree_cases(op, dt, rng):
            t = _upload(case.arena)
            atomic.reduce_tree(op, dt, _view(t, case.outs[0]), [_view(t, s) for s in case.ins], n)
            case.check(dt, t.cpu().numpy())
            ran += 1
    assert ran == S.n_tree_cases(op)
    assert ran == sum(7 * (S.N_PATHS[S.esz_of(dt)] + 2) for dt in S.dts_of(op))


@pytest.mark.parametrize("op", OPS)
def test_tree_put_every_pair(op):
    """lfa_reduce_tree_put_async: 1, 3, 5, 9, 17 and 32 inputs (every leaf
    count, U = 4 and U = 2) to 2 outputs and to 6 (the one-workgroup-per-CU
    form where it applies, the ordinary one elsewhere), on every path; every
    output checked."""
    rng = np.random.default_rng(3000 + op)
    ran = 0
    for dt in S.dts_of(op):
        n = S.lanes(S.esz_of(dt))
        for case in S.put_cases(op, dt, rng):
            t = _upload(case.arena)
            atomic.reduce_tree_put(op, dt, [_view(t, s) for s in case.outs],
                                   [_view(t, s) for s in case.ins], n)
            case.check(dt, t.cpu().numpy())
            ran += 1
    assert ran == S.n_put_cases(op)
    assert ran == sum(6 * S.N_PATHS[S.esz_of(dt)] * 2 for dt in S.dts_of(op))


def test_writev_every_pair(manifest):
    """lfa_atomic_writev_async (combine_iov per (op, type)): 37 segments on
    the vector, element and bytes paths in one launch, per segment against
    the oracle."""
    ran = 0
    for op, dt in S.write_pairs(manifest):
        case = S.writev_case(op, dt, np.random.default_rng(4000 + 32 * op + dt))
        t = _upload(case.arena)
        atomic.writev(op, dt, [_view(t, s) for s in case.dst], [_view(t, s) for s in case.src[0]])
        case.check(dt, t.cpu().numpy())
        ran += 1
    assert ran == 148


@pytest.mark.parametrize("nsrc", S.TREEV_NSRC)
def test_treev_every_pair(nsrc):
    """lfa_reduce_treev_async (reduce_iov per (op, type, 2 / 4 / 8 leaves):
    2 and 3 inputs take the 2-leaf body, 5 the 4-leaf one, 8 and 15 the 8-leaf
    one): 19 segments, aliased and unaliased on every path, per segment
    against the reference."""
    ran = 0
    for op, dt in S.reduce_pairs():
        case = S.treev_case(op, dt, nsrc, np.random.default_rng(5000 + 32 * op + dt))
        t = _upload(case.arena)
        atomic.reduce_treev(op, dt, [_view(t, s) for s in case.dst],
                            [[_view(t, case.src[k][i]) for k in range(nsrc)]
                             for i in range(len(case.dst))])
        case.check(dt, t.cpu().numpy())
        ran += 1
    assert ran == 133


NT_CASES = {"float_sum": (S.SUM, 8), "int64_min": (S.MIN, 6), "uint8_bxor": (S.BXOR, 1)}
# 16-byte vectors per workgroup of the body each fan-in takes from 192 MiB of
# output: reduce_tree_lds<.., 2, 4, 1> (4 waves x 64), reduce_tree_chunk<.., 1>
# (kBlock), reduce_tree_chunk<.., 2> (2 x kBlock)
NT_TILE_VECS = {2: 256, 3: 256, 9: 512, 17: 512}


@pytest.mark.parametrize("case", sorted(NT_CASES))
@pytest.mark.parametrize("nsrc", sorted(NT_TILE_VECS))
def test_tree_nt_forms(nsrc, case):
    """The three tree bodies that only run from 192 MiB of output, at 200 MiB
    plus a ragged tail, inputs generated on the device; the reference on
    5000-element windows at both ends and in the middle, and on one from 777
    elements before the last whole workgroup tile of the body to 777 past it."""
    op, dt = NT_CASES[case]
    nd = oracle.DT_NP[dt]
    e = nd.itemsize
    n = ((200 << 20) + 4 * 1000 + e * 3) // e
    assert n * e // 16 * 16 >= 192 << 20
    g = torch.Generator(device="cuda").manual_seed(100 * nsrc + dt)

    def operand():
        if dt == 8:
            return torch.rand(n, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1)
        if dt == 6:
            return torch.randint(-2**62, 2**62, (n,), device="cuda", generator=g,
                                 dtype=torch.int64)
        return torch.randint(0, 256, (n,), device="cuda", generator=g, dtype=torch.uint8)
    srcs = [operand() for _ in range(nsrc)]
    out = torch.zeros_like(srcs[0])
    try:
        atomic.reduce_tree(op, dt, out.view(torch.uint8), [s.view(torch.uint8) for s in srcs], n)
        torch.cuda.synchronize()
        tile = NT_TILE_VECS[nsrc] * 16 // e
        for lo, ln in ((0, 5000), (n // 2, 5000), (n - 5000, 5000),
                       ((n * e // 16 // NT_TILE_VECS[nsrc] - 1) * tile - 777,
                        max(5000, tile + 1554))):
            hi = min(n, lo + ln)
            want = oracle.allreduce(op, dt, [s[lo:hi].cpu().numpy().view(nd).copy()
                                             for s in srcs])[0]
            assert_parity(dt, out[lo:hi].cpu().numpy().view(np.uint8), want.view(np.uint8),
                          f"nt tree {case} nsrc={nsrc} [{lo},{hi})")
    finally:
        del srcs, out
        torch.cuda.empty_cache()
