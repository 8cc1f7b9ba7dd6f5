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
3. The same for the three binary tables (tests/test_sweep_tables_gpu.py): the
   pair lists, inputs under which a compare holds on 1/3 or 2/3 of the lanes
   and a fetch changes dst, the edge pairs that separate a compare of bits from
   one of values, and the full case list through lfa_host_write,
   lfa_host_readwrite and lfa_host_swap.
4. The forced large-size forms (tests/test_sweep_forms_gpu.py): the case
   counts, the form tests/_sweep.py's model names for each as_bytes, the tile
   shapes lanes() gives the tapered grids and the tree bodies, and the case
   list through the host forms.  For launch_fetch's forms, which taper a
   quarter: a count of their own (fetch_lanes), held to two whole head
   workgroups, two whole tail workgroups and a partial one with a whole and a
   partial wave; the thresholds and tile sizes held to the source text; and
   every readwrite and compare case through lfa_host_readwrite / lfa_host_swap.
5. The one-shot sweep (tests/test_sweep_oneshot_gpu.py): the layout model
   against lfa_signal.h's text and lfa_coll_block, the case lists against
   their literals (all 931 instantiations, every path), the inputs at 8 ranks,
   and the protocol against a numpy emulation of the kernels, with and without
   seeded faults.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from libfabric_amd import atomic
from tests import _iov_layout as L
from tests import _sweep as S

OPS = range(10)
TILE_VECS = L.TILE // 16    # 16-byte vectors per workgroup tile
WAVE_VECS = 4 * 64          # per wave of it: 4 KiB
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
    every element size and operand count the sweep uses.  The one shape,
    lanes(esz), gives launch_write and launch_fetch (16-KiB workgroup tiles
    of 4 waves x 4 KiB, as the tree's widest body) two whole LDS tiles, a
    partial tile with whole and partial waves, and a ragged tail."""
    for esz in (1, 2, 4, 8, 16):
        assert len(S.paths_of(esz)) == S.N_PATHS[esz]
        n = S.lanes(esz)
        assert n == {1: 41555, 16: 2600}.get(esz, n)
        nvec = n * esz // 16
        # two whole 16-KiB workgroup tiles, a partial tile, a partial wave
        assert nvec // 1024 == 2 and nvec % 1024 and nvec % 64
        # launch_write and launch_fetch cut the same 16-KiB tiles, 4 waves x
        # 4 KiB (256 vectors): with or without an element head the partial
        # tile holds whole wave tiles and a partial one, whose last 64-lane
        # step is partial too
        assert TILE_VECS == 4 * WAVE_VECS == 1024
        for body in (nvec, (n * esz - (16 - esz)) // 16):      # vec path, head path
            assert body // TILE_VECS == 2 and body % TILE_VECS // WAVE_VECS >= 1
            assert body % WAVE_VECS and body % 64
        assert n * esz % 16 or esz == 16                        # a ragged tail
        for path in S.paths_of(esz):
            for ndst, nsrc in [(1, k) for k in S.TREE_NSRC] + \
                    [(j, k) for j in S.PUT_NDST for k in S.PUT_NSRC]:
                _, outs, ins = S.layout(esz, path, ndst, nsrc)
                assert S.expect_path(esz, outs, ins) == path, (esz, path, ndst, nsrc)
            # the binary tables' operands in launcher order, whoever is odd
            for names in S.TABLE_OPERANDS.values():
                for k in range(4):
                    offs, odd = S.table_layout(esz, path, names, k)
                    assert S.expect_path(esz, offs[:1], offs[1:]) == path
                    assert (odd is not None) == (path in S.ODD)
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


# ------------------------------------------------------- binary tables ----

SWAP_MIN_TAKEN, SWAP_MAX_TAKEN = 0.25, 0.75     # the class shares are 1/3 and 2/3
MSWAP_MIN_CHANGED = 0.5
RW_MIN_CHANGED = 0.25
# cases per path as pairs with that path: every pair has vec; the 16-byte
# types have neither head nor elem, the 1-byte types no bytes path
N_WRITE_CASES = {"vec": 148, "head": 148 - 22, "elem": 148 - 22, "bytes": 148 - 22}
N_RW_CASES = {"vec": 145, "head": 145 - 24, "elem": 145 - 24, "bytes": 145 - 24}
N_SWAP_CASES = {"vec": 84, "head": 84 - 14, "elem": 84 - 14, "bytes": 84 - 14}


def _table_entries(name, rows, first_op=0):
    tbl = (ctypes.c_void_p * (rows * 16)).in_dll(atomic.lib(), name)
    return {(first_op + i // 16, i % 16) for i in range(rows * 16) if tbl[i]}


def test_table_pair_lists(manifest):
    """145 fetch and 84 compare pairs: the oracle's, the golden manifest's
    and the library's non-NULL table entries are one list; and the cases each
    table's sweep runs per path."""
    rp, sp, wp = S.rw_pairs(), S.swap_pairs(), S.write_pairs(manifest)
    assert len(rp) == len(set(rp)) == S.N_RW_PAIRS == 145
    assert len(sp) == len(set(sp)) == S.N_SWAP_PAIRS == 84
    assert {(c["op"], c["dt"]) for c in manifest["readwrite"]} == set(rp)
    assert {(c["op"], c["dt"]) for c in manifest["swap"]} == set(sp)
    assert len(manifest["readwrite"]) == 145 and len(manifest["swap"]) == 84
    assert _table_entries("lfa_atomic_readwrite_handlers", 12) == set(rp)
    assert _table_entries("lfa_atomic_swap_handlers", 7, 12) == set(sp)
    for op, dt in rp + sp:
        assert atomic.datatype_size(dt) == S.esz_of(dt)
    for pairs, per_path, total in ((wp, N_WRITE_CASES, 526), (rp, N_RW_CASES, 508),
                                   (sp, N_SWAP_CASES, 294)):
        for path in S.PATHS:
            assert S.n_table_cases([dt for _, dt in pairs], (path,)) == per_path[path]
        assert S.n_table_cases([dt for _, dt in pairs]) == sum(per_path.values()) == total


def _taken(dt, old, new):
    """Per lane: the reference changed dst (src differs from dst in bits on
    every lane, so: the swap was taken)."""
    e = S.esz_of(dt)
    return (old.reshape(-1, e) != new.reshape(-1, e)).any(axis=1)


@pytest.mark.parametrize("op", S.SWAP_OPS)
def test_swap_inputs_are_informative(op):
    """Under the reference alone: every compare holds on a share of the bulk
    lanes in [0.25, 0.75]; each MSWAP operand decides dst on at least half."""
    rng = np.random.default_rng(6000 + op)
    dts = S.table_dts(S.swap_pairs(), op)
    bulk = SENS_LANES - S.EDGE_LANES
    for dt in dts:
        d, s, c = S.swap_inputs(op, dt, SENS_LANES, rng)
        want = S.reference_swap(op, dt, d, s, c)
        if op != S.MSWAP:
            e = S.esz_of(dt)
            assert (d.reshape(-1, e) != s.reshape(-1, e)).any(axis=1).all(), (op, dt)
            share = _taken(dt, d, want)[:bulk].mean()
            assert SWAP_MIN_TAKEN <= share <= SWAP_MAX_TAKEN, (op, dt, share)
            continue
        for k in range(3):
            other = [d, s, c]
            other[k] = S.swap_inputs(op, dt, SENS_LANES, rng)[k]
            changed = _taken(dt, want, S.reference_swap(op, dt, *other))[:bulk].mean()
            assert changed >= MSWAP_MIN_CHANGED, (op, dt, k, changed)
    assert len(dts) == {S.CSWAP: 13, S.CSWAP_NE: 13, S.MSWAP: 10}.get(op, 12)


@pytest.mark.parametrize("dt", [8, 9, 10])
def test_swap_edge_lanes_separate_bits_from_values(dt):
    """FLOAT, DOUBLE, FLOAT_COMPLEX: every edge pair is among the last 64
    lanes, and on the +-0 and the same-NaN lanes both CSWAP (bits: -0 is not
    +0, a NaN is its own bits) and CSWAP_NE (values: -0 is +0, a NaN differs
    from itself) answer the opposite of "cmp and dst are equal values", as
    include/lfa_atomic.h states them."""
    ft = np.dtype(np.float64) if dt == 9 else np.dtype(np.float32)
    ub = np.uint64 if dt == 9 else np.uint32
    step = 2 if dt == 10 else 1
    sub = np.finfo(ft).smallest_subnormal
    for op in (S.CSWAP, S.CSWAP_NE):
        d, s, c = S.swap_inputs(op, dt, SENS_LANES, np.random.default_rng(6100 + op))
        lo = (SENS_LANES - S.EDGE_LANES) * S.esz_of(dt)
        dv, cv = d[lo:].view(ft)[::step], c[lo:].view(ft)[::step]
        db, cb = d[lo:].view(ub)[::step], c[lo:].view(ub)[::step]
        dneg, cneg = np.signbit(dv), np.signbit(cv)
        zeros = (dv == 0) & (cv == 0) & (dneg != cneg)
        same_nan = np.isnan(dv) & (db == cb)
        present = {
            "+0,-0": zeros & ~dneg, "-0,+0": zeros & dneg, "nan,same nan": same_nan,
            "nan,-nan": np.isnan(dv) & np.isnan(cv) & (db != cb),
            "1,nan": (dv == 1) & np.isnan(cv), "nan,1": np.isnan(dv) & (cv == 1),
            "inf,inf": (dv == np.inf) & (cv == np.inf),
            "-inf,inf": (dv == -np.inf) & (cv == np.inf),
            "subnormal,0": (dv == sub) & (cv == 0) & ~cneg,
        }
        assert set(present) == set(S.SWAP_EDGE_PAIRS)
        for name, lanes in present.items():
            assert lanes.any(), (op, dt, name)
        taken = _taken(dt, d, S.reference_swap(op, dt, d, s, c))[-S.EDGE_LANES:]
        veq = S.values_equal(dt, c, d)[-S.EDGE_LANES:]
        assert veq[zeros].all() and not veq[same_nan].any()
        assert not taken[zeros].any() and taken[same_nan].all(), (op, dt)
        assert (taken != veq)[zeros | same_nan].all(), (op, dt)


@pytest.mark.parametrize("op", [op for op in S.RW_OPS if op != S.READ])
def test_readwrite_inputs_are_informative(op):
    """The reference's new dst differs from the old one on at least 25 % of
    the bulk lanes: a kernel that wrote the new value to res, or left dst
    alone, cannot pass."""
    rng = np.random.default_rng(6200 + op)
    dts = S.table_dts(S.rw_pairs(), op)
    for dt in dts:
        d, s = S.inputs(S.SUM if op == S.WRITE else op, dt, 2, SENS_LANES, rng)
        changed = _taken(dt, d, S.reference_readwrite(op, dt, d, s))
        share = changed[:SENS_LANES - S.EDGE_LANES].mean()
        assert share >= RW_MIN_CHANGED, (op, dt, share)
    assert dts


@pytest.mark.parametrize("op", S.WRITE_OPS)
def test_host_write_every_case(op, manifest):
    """tests/test_sweep_tables_gpu.py's write cases through lfa_host_write."""
    dts = S.table_dts(S.write_pairs(manifest), op)
    cases = list(S.write_cases(op, dts, np.random.default_rng(7000 + op)))
    for dt, case in cases:
        a = case.arena.copy()
        atomic.host_write(op, dt, case.view(a, "dst"), case.view(a, "src"),
                          S.lanes(S.esz_of(dt)))
        case.check(dt, a)
    assert len(cases) == S.n_table_cases(dts) == sum(S.N_PATHS[S.esz_of(dt)] for dt in dts)
    S.assert_every_operand_was_odd("write", op, cases)


@pytest.mark.parametrize("op", S.RW_OPS)
def test_host_readwrite_every_case(op):
    dts = S.table_dts(S.rw_pairs(), op)
    cases = list(S.readwrite_cases(op, dts, np.random.default_rng(8000 + op)))
    for dt, case in cases:
        a = case.arena.copy()
        atomic.host_readwrite(op, dt, case.view(a, "dst"),
                              case.view(a, "src") if "src" in case.at else None,
                              case.view(a, "res"), S.lanes(S.esz_of(dt)))
        case.check(dt, a)
    assert len(cases) == S.n_table_cases(dts) == sum(S.N_PATHS[S.esz_of(dt)] for dt in dts)
    S.assert_every_operand_was_odd("readwrite", op, cases)


@pytest.mark.parametrize("op", S.SWAP_OPS)
def test_host_swap_every_case(op):
    dts = S.table_dts(S.swap_pairs(), op)
    cases = list(S.swap_cases(op, dts, np.random.default_rng(9000 + op)))
    for dt, case in cases:
        a = case.arena.copy()
        atomic.host_swap(op, dt, case.view(a, "dst"), case.view(a, "src"),
                         case.view(a, "cmp"), case.view(a, "res"), S.lanes(S.esz_of(dt)))
        case.check(dt, a)
    assert len(cases) == S.n_table_cases(dts) == sum(S.N_PATHS[S.esz_of(dt)] for dt in dts)
    S.assert_every_operand_was_odd("swap", op, cases)


def test_table_check_sees_its_faults():
    """TableCase.check itself, on a compare and on a fetch case: a byte in a
    gap, a changed src, a changed cmp, res holding the new value, one wrong
    lane of dst."""
    rng = np.random.default_rng(8)
    (_, sw), = S.swap_cases(S.CSWAP_LE, [4], rng, paths=("vec",))
    (_, rw), = S.readwrite_cases(S.SUM, [8], rng, paths=("head",))
    for dt, case in ((4, sw), (8, rw)):
        good = case.arena.copy()
        case.view(good, "res")[:] = case.view(case.arena, "dst")
        case.view(good, "dst")[:] = case.want
        case.check(dt, good)
        faults = {"gap": case.at["dst"][0] - 1, "src": case.at["src"][0] + 5,
                  "dst lane": case.at["dst"][0] + 4 * 9 + 2}
        if "cmp" in case.at:
            faults["cmp"] = case.at["cmp"][0] + case.at["cmp"][1] - 1
        for what, at in faults.items():
            bad = good.copy()
            bad[at] ^= 0x10
            with pytest.raises(AssertionError):
                case.check(dt, bad)
        bad = good.copy()
        case.view(bad, "res")[:] = case.want
        with pytest.raises(AssertionError, match="res is not the old dst"):
            case.check(dt, bad)


# ----------------------------------------------------- large-size forms ----
# tests/test_sweep_forms_gpu.py's cases: (pairs on the vec path, on the head
# path) per forced form, from the pair lists above
N_WRITE_FORM_CASES = 2 * (148 + 126)            # taper and nt, every write pair
N_TREE_FORM_CASES = 133 * 7 * 3                 # 7 fan-ins, plain and two aliasings


def test_form_shapes():
    """lanes() at the forced forms: the body (2597 or 2598 vectors on the vec
    path, 2600 of 16-byte elements, 2596 or 2597 behind an element head) gives the write taper (last 1/8) 2 whole
    4-KiB-per-wave head workgroups, 2 whole tail workgroups and a partial
    one, and the tree bodies 10 (256-vector workgroups: LDS form, chunk
    U = 1) or 5 (512: chunk U = 2) whole workgroup tiles and a partial one."""
    for esz in (1, 2, 4, 8, 16):
        n = S.lanes(esz)
        bodies = [n * esz // 16] + ([(n * esz - (16 - esz)) // 16] if esz < 16 else [])
        assert all(2596 <= nvec <= 2600 for nvec in bodies), (esz, bodies)
        for nvec in bodies:
            assert (nvec // 256, nvec // 512) == (10, 5) and nvec % 256 and nvec % 512
            nhead, whole, part = S.model_taper(nvec, 8)
            assert (nhead, whole) == (2, 2) and 0 < part < 256 and part % 64


def test_form_case_lists(manifest):
    """The forced-form generators: their counts, the form the model names
    for each as_bytes, and that every large-only form of the table is among
    them; forced sizes are the thresholds themselves."""
    wp = S.write_pairs(manifest)
    rng = np.random.default_rng(1)
    forms = set()
    total = 0
    for op in S.WRITE_OPS:
        for form, as_bytes, dt, case in S.write_form_cases(op, S.table_dts(wp, op), rng):
            assert S.model_write_form(as_bytes) == form and case.path in S.FORM_PATHS
            assert S.model_write_form(as_bytes - 16) != form
            forms.add(form)
            total += 1
    assert total == N_WRITE_FORM_CASES == 548
    assert sum(S.n_tree_form_cases(op) for op in OPS) == N_TREE_FORM_CASES == 2793
    for nsrc, form in S.TREE_AS_FORMS.items():
        for esz in (1, 2, 4, 8, 16):
            assert S.model_tree_form(S.TREE_AS, nsrc, esz) == form
            assert S.model_tree_form(S.TREE_AS - 16, nsrc, esz) in S.SMALL_FORMS
        forms.add((form, S.leaves_of(nsrc)))
    assert tuple(S.TREE_AS_FORMS) == S.TREE_NSRC
    # one fan-in per large-only tree instantiation, both large write forms
    assert forms == {"combine_lds_taper sc1", "combine_lds nt", ("lds", 2), ("chunk1 nt", 2), ("chunk1 nt", 4),
                     ("chunk1 nt", 8), ("chunk2 nt", 8), ("chunk2 nt", 16), ("chunk2 nt", 32)}


@pytest.mark.parametrize("op", S.WRITE_OPS)
def test_host_write_form_cases(op, manifest):
    """The forced-form cases through the host forms, which have no forms:
    this checks the cases and the check, as the host sweeps above do."""
    dts = S.table_dts(S.write_pairs(manifest), op)
    ran = 0
    for _, _, dt, case in S.write_form_cases(op, dts, np.random.default_rng(17000 + op)):
        a = case.arena.copy()
        atomic.host_write(op, dt, case.view(a, "dst"), case.view(a, "src"),
                          S.lanes(S.esz_of(dt)))
        case.check(dt, a)
        ran += 1
    assert ran == 2 * S.n_table_cases(dts, S.FORM_PATHS)


@pytest.mark.parametrize("op", OPS)
def test_host_tree_form_cases(op):
    rng = np.random.default_rng(12000 + op)
    ran = 0
    for dt in S.dts_of(op):
        for _, _, case in S.tree_form_cases(op, dt, rng):
            a = case.arena.copy()
            atomic.host_reduce_tree(op, dt, _view(a, case.outs[0]),
                                    [_view(a, s) for s in case.ins], S.lanes(S.esz_of(dt)))
            case.check(dt, a)
            ran += 1
    assert ran == S.n_tree_form_cases(op) == 21 * len(S.dts_of(op))


# launch_fetch's forms (tests/test_sweep_forms_gpu.py): nt for every pair,
# tapered write-through for the two-input readwrite pairs (all but ATOMIC_READ)
N_RW_FORM_CASES = (145 + 121) + (132 + 110)     # 24 sixteen-byte pairs, 2 of them ATOMIC_READ's
N_SWAP_FORM_CASES = 84 + 70
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "libfabric_amd", "csrc")


def test_fetch_form_constants_are_the_sources():
    """The thresholds and the taper's tile sizes the model and fetch_lanes
    assume are launch_fetch's, read from the source text: 64 and 192 MiB in
    lfa_split.h; 4 waves x 64 lanes x U = 4 vectors per head workgroup, 4 x 64
    per tail workgroup, the last 1/4 tapered, in lfa_k_launch.hpp."""
    split = open(os.path.join(CSRC, "lfa_split.h")).read()
    assert _define(split, "LFA_FETCH_TAPER_BYTES") == "(size_t)64 << 20"
    assert _define(split, "LFA_SC1_BYTES") == "(size_t)192 << 20"
    assert dict(S.FETCH_AS) == {"fetch_lds_taper sc1": 64 << 20, "fetch_lds_taper nt": 192 << 20}
    assert re.search(r"enum lfa_fetch_form \{\s*LFA_FETCH_LDS,[^}]*LFA_FETCH_TAPER_SC1,[^}]*"
                     r"LFA_FETCH_TAPER_NT\b", split)           # FETCH_FORMS' order
    kern = open(os.path.join(CSRC, "lfa_kernels.hpp")).read()
    assert re.search(r"^constexpr int kLdsWaves = 4;", kern, re.M)
    launch = open(os.path.join(CSRC, "lfa_k_launch.hpp")).read()
    body = launch[launch.index("static int launch_fetch("):launch.index("static int launch_readwrite(")]
    assert "kFetchTaperBytes" not in launch
    assert re.search(r"constexpr int U = 4;", body)
    assert re.search(r"constexpr size_t hv = \(size_t\)kLdsWaves \* 64 \* U, "
                     r"tv = \(size_t\)kLdsWaves \* 64;", body)
    assert re.findall(r"lfa_split_taper\(([^)]*)\)", body) == ["nvec, 4, hv, tv"]
    assert re.findall(r"switch \(([^\n]*)\) \{", body) == ["form"]
    assert "form = lfa_form_fetch(lfa_form_bytes(nvec, as_bytes), FF::kIn);" in body
    assert re.findall(r"fetch_lds_taper<([^>]*)>", body) == ["U, 1, kStoreNt, FF", "U, 1, kStoreSc1, FF"]
    hv, tv, div = 4 * 64 * 4, 4 * 64, 4
    assert (hv, tv, div) == (1024, 256, 4) == S.model_taper.__defaults__ + (4,)


def test_fetch_form_shapes():
    """fetch_lanes() under launch_fetch's taper (the last 1/4 in 256-vector
    workgroups behind 1024-vector ones), at every element size on the vec
    path and behind an element head: at least two whole head workgroups (a
    wrong block stride shows), at least two whole tail workgroups, a last
    partial one with a whole wave and a partial wave, and an element tail after
    the last vector below 16 bytes: on both paths at 1, 2 and 4 bytes; at 8
    bytes on the vec path only, as no count can do better there (the head
    path's single head element leaves count - 1 elements, so one of count and
    count - 1 is a whole number of 2-element vectors).  lanes() itself gives
    ONE head workgroup here, which is why these forms have a count of their
    own."""
    for esz in (1, 2, 4, 8, 16):
        n = S.fetch_lanes(esz)
        assert n == (48 * 1024 + 16 * 101) // esz + 1
        bodies = [(n * esz // 16, n * esz % 16)]
        if esz < 16:            # head path: (16 - esz) bytes of head elements first
            bodies.append(((n * esz - (16 - esz)) // 16, (n * esz - (16 - esz)) % 16))
        for nvec, tail_bytes in bodies:
            assert 3172 <= nvec <= 3174, (esz, nvec)
            nhead, whole, part = S.model_taper(nvec, 4)
            assert nhead >= 2 and whole >= 2, (esz, nvec)
            assert (nhead, whole) == (2, 4) and 100 <= part <= 102
            assert part >= 64 and part % 64, (esz, nvec)        # a whole wave, a partial one
            assert nhead * 1024 + whole * 256 + part == nvec
            assert tail_bytes % esz == 0
        tails = [t >= esz for _, t in bodies]
        assert tails == {8: [True, False], 16: [False]}.get(esz, [True, True]), (esz, bodies)
        assert S.model_taper(S.lanes(esz) * esz // 16, 4)[0] == 1


def test_fetch_form_case_lists():
    """The fetch and compare form generators: the totals, the form the model
    names for each as_bytes and functor shape, both paths, the count."""
    rp, sp = S.rw_pairs(), S.swap_pairs()
    rng = np.random.default_rng(2)
    seen, total = set(), 0
    for op in S.RW_OPS:
        dts = S.table_dts(rp, op)
        cases = list(S.readwrite_form_cases(op, dts, rng))
        assert len(cases) == S.n_fetch_form_cases("readwrite", op, dts)
        assert len(cases) == (1 if op == S.READ else 2) * S.n_table_cases(dts, S.FORM_PATHS)
        for form, as_bytes, dt, case in cases:
            assert S.model_fetch_form(as_bytes, S.fetch_nin("readwrite", op)) == form
            assert case.path in S.FORM_PATHS
            assert case.at["dst"][1] == S.fetch_lanes(S.esz_of(dt)) * S.esz_of(dt)
            assert ("src" in case.at) == (op != S.READ) and "res" in case.at
            seen.add((form, S.fetch_nin("readwrite", op), (op, dt), case.path))
        total += len(cases)
    assert total == N_RW_FORM_CASES == S.N_RW_FORM_CASES == 508
    total = 0
    for op in S.SWAP_OPS:
        dts = S.table_dts(sp, op)
        cases = list(S.swap_form_cases(op, dts, rng))
        assert len(cases) == S.n_fetch_form_cases("swap", op, dts)
        for form, as_bytes, dt, case in cases:
            assert S.model_fetch_form(as_bytes, 3) == form == "fetch_lds_taper nt"
            assert case.path in S.FORM_PATHS and set(case.at) == {"dst", "src", "cmp", "res"}
            assert case.at["dst"][1] == S.fetch_lanes(S.esz_of(dt)) * S.esz_of(dt)
            seen.add((form, 3, (op, dt), case.path))
        total += len(cases)
    assert total == N_SWAP_FORM_CASES == S.N_SWAP_FORM_CASES == 154
    # every pair under nt on the vec path; every two-input pair under sc1 too
    for form, nin, pairs in (("fetch_lds_taper nt", None, rp + sp),
                             ("fetch_lds_taper sc1", 2, [p for p in rp if p[0] != S.READ])):
        got = {p for f, k, p, path in seen if f == form and path == "vec"}
        assert got == set(pairs), form
        head = {p for f, k, p, path in seen if f == form and path == "head"}
        assert head == {p for p in pairs if S.esz_of(p[1]) < 16}, form
    assert {(f, k) for f, k, *_ in seen} == {("fetch_lds_taper nt", 1), ("fetch_lds_taper nt", 2),
                                             ("fetch_lds_taper nt", 3), ("fetch_lds_taper sc1", 2)}


@pytest.mark.parametrize("op", S.RW_OPS)
def test_host_readwrite_form_cases(op):
    """The fetch form cases through lfa_host_readwrite, which has no forms:
    this pins fetch_lanes, the layouts and the references before a kernel
    sees them."""
    dts = S.table_dts(S.rw_pairs(), op)
    ran = 0
    for _, _, dt, case in S.readwrite_form_cases(op, dts, np.random.default_rng(18000 + op)):
        a = case.arena.copy()
        atomic.host_readwrite(op, dt, case.view(a, "dst"),
                              case.view(a, "src") if "src" in case.at else None,
                              case.view(a, "res"), S.fetch_lanes(S.esz_of(dt)))
        case.check(dt, a)
        ran += 1
    assert ran == (1 if op == S.READ else 2) * S.n_table_cases(dts, S.FORM_PATHS) and ran


@pytest.mark.parametrize("op", S.SWAP_OPS)
def test_host_swap_form_cases(op):
    dts = S.table_dts(S.swap_pairs(), op)
    ran = 0
    for _, _, dt, case in S.swap_form_cases(op, dts, np.random.default_rng(19000 + op)):
        a = case.arena.copy()
        atomic.host_swap(op, dt, case.view(a, "dst"), case.view(a, "src"),
                         case.view(a, "cmp"), case.view(a, "res"), S.fetch_lanes(S.esz_of(dt)))
        case.check(dt, a)
        ran += 1
    assert ran == S.n_table_cases(dts, S.FORM_PATHS) and ran


# ------------------------------------------------------------- one-shot ----
# tests/test_sweep_oneshot_gpu.py's cases, its layout model and its protocol

SIGNAL_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "libfabric_amd", "csrc", "lfa_signal.h")


def _define(text, name):
    m = re.search(rf"^#define {name} +\(?([^/\n]*?)\)? *(/\*.*)?$", text, re.M)
    assert m, name
    return m.group(1).strip()


def test_oneshot_layout_model():
    """The model's constants are lfa_signal.h's (read from its text), its
    scatter partition is lfa_coll_block's, the chunk and grid rules give the
    shapes the cases are meant to have, and the LL interleave round-trips."""
    from libfabric_amd import coll
    text = open(SIGNAL_H).read()
    assert _define(text, "LFA_SIG_MAX") == "32" and S.SIG_MAX == 32
    assert _define(text, "LFA_SIG_AREA_BYTES") == "1u << 20" and S.SIG_AREA == 1 << 20
    assert _define(text, "LFA_SIG_OS_OFF") == "256" and S.SIG_OS_OFF == 256
    assert _define(text, "LFA_SIG_OS_CHUNKS") == "128" and S.SIG_OS_CHUNKS == 128
    assert _define(text, "LFA_OS_MAX_RANKS") == "8" and S.OS_MAX_RANKS == 8
    assert _define(text, "LFA_OS_LL_BYTES") == "16u << 10" and S.LL_BYTES == 16 << 10
    assert _define(text, "LFA_SIG_LL_SLOT") == "2u * LFA_OS_LL_BYTES" and S.LL_SLOT == 2 * S.LL_BYTES
    assert _define(text, "LFA_SIG_LL_PARITY") == "LFA_OS_MAX_RANKS * LFA_SIG_LL_SLOT"
    assert S.LL_PARITY == S.OS_MAX_RANKS * S.LL_SLOT
    assert _define(text, "LFA_SIG_LL_OFF") == "64u << 10" and S.LL_OFF == 64 << 10
    assert _define(text, "LFA_SIG_NONE") == "0xffffffffffffffffull" and S.SIG_NONE == 2**64 - 1
    assert coll.sig_area_bytes() == S.SIG_AREA and coll.SIG_NONE == S.SIG_NONE
    # the areas do not overlap (the header's own #error, on the model's numbers)
    assert S.SIG_OS_OFF + 4 * S.SIG_OS_CHUNKS * S.SIG_MAX <= S.LL_OFF
    assert S.LL_OFF + 2 * S.LL_PARITY <= S.SIG_AREA - 64
    for n in range(1, 9):
        for count in (0, 1, n - 1, n, 1000, 8 * 2071 - 1):
            soff, slen = S.os_parts(S.OS_SCATTER, n, count, 4)
            assert [(o // 4, ln // 4) for o, ln in zip(soff, slen)] == \
                [coll.block(count, n, r) for r in range(n)]
    assert S.os_parts(3, 5, 10, 8) == ([0] * 5, [0, 0, 0, 80, 0])
    assert S.os_parts(S.OS_ALL, 3, 10, 8) == ([0] * 3, [80] * 3)
    # flagged: 4 KiB chunks up to 128 of them, then wider ones; LL: 4 KiB per workgroup
    assert S.os_grid(S.FLAG, 1) == (4096, 1) and S.os_grid(S.FLAG, 4097) == (4096, 2)
    assert S.os_grid(S.FLAG, 128 * 4096) == (4096, 128)
    assert S.os_grid(S.FLAG, S.OS_BIG_PART) == (4144, 128) and S.OS_BIG_PART % 16 == 0
    assert S.os_grid(S.LL, 1) == (None, 1) and S.os_grid(S.LL, 4097) == (None, 2)
    assert S.os_grid(S.LL, S.LL_BYTES) == (None, 4)
    for esz in (1, 2, 4, 8, 16):
        for kernel in (S.FLAG, S.LL):
            most = S.os_count(kernel, S.OS_ALL, 2, esz) * esz
            assert most == S.OS_PART[kernel] + S.OS_ODD * esz and most <= S.LL_BYTES
            assert S.os_grid(kernel, most)[1] == 3 and most % 4096      # the last one partial
            assert (most % 16 != 0) == (esz < 16)                       # a tail below 16 bytes
            for n in (3, 8):
                soff, slen = S.os_parts(S.OS_SCATTER, n, S.os_count(kernel, S.OS_SCATTER, n, esz),
                                        esz)
                assert max(slen) == most and slen[-1] == most - esz
    rng = np.random.default_rng(3)
    for nb in (1, 15, 16, 17, 4099):
        part = rng.integers(0, 256, nb, dtype=np.uint8)
        data, flags = S.ll_unpack(S.ll_pack(part, 0xFFFFFFFF))
        assert data.size == -(-nb // 16) * 16 and flags.size * 4 == data.size
        assert np.array_equal(data[:nb], part) and not data[nb:].any()
        assert (flags == 0xFFFFFFFF).all()


def test_oneshot_case_lists():
    """Every one of the 931 instantiations launch_oneshot chooses among (133
    pairs x NLEAF 1, 2, 4, 8 flagged and 2, 4, 8 LL) is run; every pair meets
    every path its element size has on both kernels; every op meets every
    (path, NLEAF); the cases have the shapes their names say."""
    seen, total = set(), 0
    for op in OPS:
        cases = list(S.os_cases(op, np.random.default_rng(op)))
        assert len(cases) == S.N_OS_PAIR_CASES * len(S.dts_of(op)) + S.N_OS_OP_CASES
        total += len(cases)
        for kernel in (S.FLAG, S.LL):
            mine = [c for c in cases if c.kernel == kernel]
            for dt in S.dts_of(op):
                assert {c.path for c in mine if c.dt == dt} == set(S.paths_of(S.esz_of(dt)))
            assert {(c.path, c.nleaf) for c in mine if c.mode != S.OS_SCATTER} == \
                {(p, k) for p in S.PATHS for k in S.OS_NLEAF[kernel]}, (op, kernel)
            assert {c.mode for c in mine} == {S.OS_ALL, S.OS_SCATTER} | \
                ({1, 3} if kernel == S.FLAG else set())
            for nleaf in S.OS_NLEAF[kernel]:
                assert {c.epoch for c in mine if c.nleaf == nleaf} >= set(S.OS_EPOCHS)
            assert {c.grid for c in mine if c.done} == {1, 3}
        for c in cases:
            seen.add((c.op, c.dt, c.kernel, c.nleaf))
            esz = S.esz_of(c.dt)
            assert c.ll == S.OS_LL_ARG[c.kernel]
            # what the launcher derives from the addresses, per path
            if c.path == "bytes":
                assert c.unal and not (c.vec and c.kernel == S.FLAG)
            else:
                assert not c.unal and c.vec == (c.path == "vec" and (
                    c.mode != S.OS_SCATTER or all(o % 16 == 0 for o in c.soff)))
            assert c.slot_bytes % 256 == 0 and c.slot_bytes - 256 < c.most <= c.slot_bytes
            assert c.most % esz == 0 and (c.kernel == S.FLAG or c.most <= S.LL_BYTES)
        assert {c.n for c in cases if c.kernel == S.FLAG} == set(range(1, 9))
        assert any(c.chunk == 4144 and c.grid == 128 for c in cases)
        assert any(c.kernel == S.LL and c.most == S.LL_BYTES for c in cases)
        assert any(c.kernel == S.FLAG and c.most == S.LL_BYTES + S.esz_of(c.dt) for c in cases)
        assert sum(1 for c in cases if c.count == 1) == 3
        assert sum(1 for c in cases if c.mode == S.OS_SCATTER and c.want[-1] is None) == 4
    assert total == S.N_OS_CASES == 2455
    assert len(seen) == S.N_OS_INSTANCES == 931
    assert seen == {(op, dt, k, nl) for op, dt in S.reduce_pairs()
                    for k in (S.FLAG, S.LL) for nl in S.OS_NLEAF[k]}


@pytest.mark.parametrize("op", OPS)
def test_oneshot_inputs_stay_visible_at_8_ranks(op):
    """S.inputs at the one-shot rows' shape and 8 ranks: replacing any one
    input by its neighbour changes the reference on at least 0.5 % of the bulk
    lanes, for every type of the op (the condition of
    test_inputs_are_informative, at this sweep's own shape)."""
    rng = np.random.default_rng(21000 + op)
    for dt in S.dts_of(op):
        n = S.os_count(S.FLAG, S.OS_ALL, 8, S.esz_of(dt))
        data = S.inputs(op, dt, 8, n, rng)
        want = S.reference(op, dt, data).reshape(n, -1)
        for k in range(8):
            other = list(data)
            other[k] = data[(k + 1) % 8]
            got = S.reference(op, dt, other).reshape(n, -1)
            changed = (got != want).any(axis=1)[:n - S.EDGE_LANES].mean()
            assert changed >= MIN_CHANGED, (op, dt, k, changed)


@pytest.mark.parametrize("op", OPS)
def test_oneshot_protocol_on_the_emulation(op):
    """Every case of the op through os_run against OsEmu, the numpy emulation
    of push, post, wait and reduce: the windows, the untouched check, the
    pre-posted flags at every epoch and the final check hold together."""
    ran = 0
    for case in S.os_cases(op, np.random.default_rng(22000 + op)):
        S.os_run(case, S.OsEmu())
        ran += 1
    assert ran == S.N_OS_PAIR_CASES * len(S.dts_of(op)) + S.N_OS_OP_CASES


WRONG_RESULT = r" rank \d: .*differ"      # Case.check's comparison of a rank's result
OS_FAULT_SEEN_BY = {            # fault -> (op, what os_run says)
    "swap_node": (S.MIN, WRONG_RESULT),             # +-0 lanes: the order alone decides
    "leaf0_for_7": (S.BAND, WRONG_RESULT),
    "vhi_hi": (S.SUM, WRONG_RESULT),
    "soff_rank": (S.SUM, r": slot \d at member \d differs"),
    "post_minus_1": (S.SUM, "timed out"),
    "no_zero_fill": (S.SUM, r": LL slot \d at member \d differs"),
}


@pytest.mark.parametrize("fault", S.OS_FAULTS)
def test_oneshot_protocol_sees_seeded_faults(fault):
    """Each fault, emulated one at a time, fails at least one case of one op
    (float for MIN and SUM) with the message that names what went wrong."""
    op, msg = OS_FAULT_SEEN_BY[fault]
    dt = 8 if op in (S.MIN, S.SUM) else 5
    failed = []
    for case in S.os_pair_cases(op, dt, np.random.default_rng(23000)):
        try:
            S.os_run(case, S.OsEmu(fault))
        except AssertionError as e:
            assert re.search(msg, str(e)), (fault, str(e))
            failed.append(case.what)
    assert failed, fault


@pytest.mark.parametrize("op", [S.MIN, S.BAND])
@pytest.mark.parametrize("kernel", [S.FLAG, S.LL])
def test_rotated_inputs_are_blind_to_a_leaf_read_twice(op, kernel):
    """The gap this sweep closes, on the emulation: with three operands in
    rotation over 8 ranks (every input there at least twice) a body that reads
    leaf 0 in place of leaf 7 passes MIN and BAND; with S.inputs it fails."""
    dt, rng = 5, np.random.default_rng(24000 + op)
    n = S.os_count(kernel, S.OS_ALL, 8, 4)
    pool = [rng.integers(0, 256, 4 * n, dtype=np.uint8) for _ in range(3)]
    blind = S.OsCase(op, dt, 8, S.OS_ALL, n, kernel, "vec", 1, [pool[k % 3] for k in range(8)])
    S.os_run(blind, S.OsEmu("leaf0_for_7"))
    seeing = S.OsCase(op, dt, 8, S.OS_ALL, n, kernel, "vec", 1, S.inputs(op, dt, 8, n, rng))
    with pytest.raises(AssertionError, match=WRONG_RESULT):
        S.os_run(seeing, S.OsEmu("leaf0_for_7"))
