"""The oracle sweep proves itself before it meets a GPU (tests/_sweep.py).

1. The inputs are informative: for every reducing pair at 5 and 32 inputs,
   replacing any one input by its neighbour changes the REFERENCE result on at
   least 0.5 % of the bulk lanes, so a body that dropped or duplicated a leaf
   cannot pass (the 64 edge lanes at the end are left out of the count: they
   alone are 2.5 % of the lanes), and for the float, complex and half types at
   least 90 % of the reference's lanes are not NaN.  Conditions on the inputs, met by the
   reference alone; tests/_sweep.py's generators are what gets fixed if they
   fail, not the bounds.
2. The layouts, the arena carving and the comparison code are right: the full
   case list of tests/test_sweep_gpu.py, run through the host combine
   (lfa_host_reduce_tree, lfa_host_writev) against the reference.
"""
import json
import os

import numpy as np
import pytest

from libfabric_amd import atomic
from tests import _sweep as S

OPS = range(10)
SENS_LANES = 2600
SENS_NSRC = (5, 32)
MIN_CHANGED = 0.005
MIN_NOT_NAN = 0.90


@pytest.fixture(scope="module")
def manifest(golden_dir):
    with open(os.path.join(golden_dir, "manifest.json")) as f:
        return json.load(f)


def test_pair_lists(manifest):
    """133 reducing and 148 write pairs, and the library takes exactly them."""
    rp, wp = S.reduce_pairs(), S.write_pairs(manifest)
    assert len(rp) == len(set(rp)) == S.N_REDUCE_PAIRS == 133
    assert len(wp) == len(set(wp)) == S.N_WRITE_PAIRS == 148
    assert sum(len(S.dts_of(op)) for op in OPS) == 133
    valid = {(op, dt) for op in range(12) for dt in range(18) if atomic.reduce_valid(dt, op) == 0}
    assert valid == set(wp)
    assert {p for p in valid if p[0] <= 9} == set(rp)
    for op, dt in wp:
        assert atomic.reduce_datatype_size(dt) == S.esz_of(dt)


def test_layouts_take_their_paths():
    """layout()'s offsets send lfa_split.h's rule down the path they name, at
    every element size and operand count the sweep uses."""
    for esz in (1, 2, 4, 8, 16):
        assert len(S.paths_of(esz)) == S.N_PATHS[esz]
        n = S.lanes(esz)
        assert n == {1: 41555, 16: 2600}.get(esz, n)
        nvec = n * esz // 16
        # two whole 16-KiB workgroup tiles, a partial tile, a partial wave
        assert nvec // 1024 == 2 and nvec % 1024 and nvec % 64
        for path in S.paths_of(esz):
            for ndst, nsrc in [(1, k) for k in S.TREE_NSRC] + \
                    [(j, k) for j in S.PUT_NDST for k in S.PUT_NSRC]:
                _, outs, ins = S.layout(esz, path, ndst, nsrc)
                assert S.expect_path(esz, outs, ins) == path, (esz, path, ndst, nsrc)
    assert S.layout(4, "vec")[0] * 4 % 16          # a ragged tail


@pytest.mark.parametrize("op", OPS)
def test_inputs_are_informative(op):
    rng = np.random.default_rng(1000 + op)
    checked = 0
    for dt in S.dts_of(op):
        for nsrc in SENS_NSRC:
            data = S.inputs(op, dt, nsrc, SENS_LANES, rng)
            want = S.reference(op, dt, data).reshape(SENS_LANES, -1)
            if S.is_float(dt):
                share = 1.0 - S.nan_lanes(dt, want.reshape(-1)).mean()
                assert share >= MIN_NOT_NAN, (op, dt, nsrc, share)
            for k in range(nsrc):
                other = list(data)
                other[k] = data[(k + 1) % nsrc]
                got = S.reference(op, dt, other).reshape(SENS_LANES, -1)
                changed = (got != want).any(axis=1)[:SENS_LANES - S.EDGE_LANES].mean()
                assert changed >= MIN_CHANGED, (op, dt, nsrc, k, changed)
            checked += 1
    assert checked == len(S.dts_of(op)) * len(SENS_NSRC)


def _view(arena, seg):
    lo, nb = seg
    return arena[lo:lo + nb]


@pytest.mark.parametrize("op", OPS)
def test_host_tree_every_case(op):
    rng = np.random.default_rng(2000 + op)
    ran = 0
    for dt in S.dts_of(op):
        esz = S.esz_of(dt)
        for case in S.tree_cases(op, dt, rng):
            a = case.arena.copy()
            atomic.host_reduce_tree(op, dt, _view(a, case.outs[0]),
                                    [_view(a, s) for s in case.ins], S.lanes(esz))
            case.check(dt, a)
            ran += 1
    assert ran == S.n_tree_cases(op)


@pytest.mark.parametrize("op", OPS)
def test_host_put_every_case(op):
    """The tree-put cases, one host tree per output."""
    rng = np.random.default_rng(3000 + op)
    ran = 0
    for dt in S.dts_of(op):
        esz = S.esz_of(dt)
        for case in S.put_cases(op, dt, rng):
            a = case.arena.copy()
            for o in case.outs:
                atomic.host_reduce_tree(op, dt, _view(a, o), [_view(a, s) for s in case.ins],
                                        S.lanes(esz))
            case.check(dt, a)
            ran += 1
    assert ran == S.n_put_cases(op)


def test_host_writev_every_pair(manifest):
    ran = 0
    for op, dt in S.write_pairs(manifest):
        case = S.writev_case(op, dt, np.random.default_rng(4000 + 32 * op + dt))
        a = case.arena.copy()
        atomic.host_writev(op, dt, [_view(a, s) for s in case.dst],
                           [_view(a, s) for s in case.src[0]])
        case.check(dt, a)
        ran += 1
    assert ran == 148


@pytest.mark.parametrize("nsrc", S.TREEV_NSRC)
def test_host_treev_every_pair(nsrc):
    """The list-form tree cases, one host tree per segment."""
    ran = 0
    for op, dt in S.reduce_pairs():
        case = S.treev_case(op, dt, nsrc, np.random.default_rng(5000 + 32 * op + dt))
        a = case.arena.copy()
        esz = S.esz_of(dt)
        for i, d in enumerate(case.dst):
            atomic.host_reduce_tree(op, dt, _view(a, d),
                                    [_view(a, case.src[k][i]) for k in range(nsrc)], d[1] // esz)
        case.check(dt, a)
        ran += 1
    assert ran == 133


def test_check_sees_a_stray_write_and_a_changed_input():
    """Case.check itself: a byte in a gap, a byte of an input, a wrong lane."""
    rng = np.random.default_rng(7)
    data = S.inputs(S.SUM, 4, 3, S.lanes(4), rng)
    case = S.carve(4, data, S.reference(S.SUM, 4, data), "vec", ndst=2, what="self-check")
    good = case.arena.copy()
    for lo, nb in case.outs:
        good[lo:lo + nb] = case.want
    case.check(4, good)
    for at in (case.outs[0][0] - 1, case.ins[1][0] + 5, case.outs[1][0] + 9):
        bad = good.copy()
        bad[at] ^= 0x10
        with pytest.raises(AssertionError):
            case.check(4, bad)
