"""Oracle sweep of the forms the write, tree and fetch launchers only take at
large sizes, run at the sweep's own ~40 KiB shape (~50 KiB for the fetch forms).

tests/test_sweep_gpu.py and tests/test_sweep_tables_gpu.py run every (op,
datatype) pair, but at one small shape, where each launcher of
lfa_k_launch.hpp picks its small-size form.  The forms it switches to by size
are separate template instantiations for every pair:

  launch_write      combine_lds_taper<.., sc1>       from 32 MiB
                    combine_lds<.., nt> (drained)    from 192 MiB
  launch_tree_body  reduce_tree_lds<.., 2, 4, 1>     2 inputs, from 192 MiB
                    reduce_tree_chunk<.., NLEAF, 1>  3..8 inputs, from 192 MiB
                    reduce_tree_chunk<.., NLEAF, 2>  9..32 inputs, from 192 MiB
  launch_fetch      fetch_lds_taper<4, 1, sc1, RwF>  readwrite but ATOMIC_READ,
                                                     from 64 MiB
                    fetch_lds_taper<4, 1, nt, RwF>   every readwrite pair, from 192 MiB
                    fetch_lds_taper<4, 1, nt, SwapF> every compare pair, from 192 MiB

The few tests at those sizes (test_tree_nt_forms,
test_nt_store_path_every_op_family, the tapered-tail tests,
test_fetch_compare_nt_path) stay the proof that
the real sizes work end to end, for a handful of pairs on windows of the
buffer.  Here every pair runs every one of these forms: lfa__write_as,
lfa__tree_as, lfa__readwrite_as and lfa__swap_as choose the form as if the
vector body were `as_bytes` bytes
(lfa_split.h) and take the split, the grid and the arguments from the real
size, so the kernels are the product's own instantiations on tests/_sweep.py's
arenas.  The fetch cases have a count of their own (fetch_lanes: launch_fetch
tapers a quarter, and lanes() would leave it one head workgroup) and the
tables' own check: res byte for byte the old dst, src and cmp unchanged, dst
exact for the compare table and ATOMIC_READ.  Every form is correct at any vector count: a tile that runs past it
takes the guarded path, and the tapered grid of a small body has fewer head
workgroups (tests/test_sweep_cpu.py holds lanes() to two whole head tiles,
whole and partial tail tiles, and 5 to 10 whole workgroup tiles of the tree
bodies; tests/test_split_cpu.py holds the choice of form to a model of the
table above).

Each case meets the existing check: sentinels intact, inputs unchanged,
outputs the oracle's under assert_parity / assert_half.  Each test counts its
cases against a literal, so a skipped pair fails.
"""
import json
import os

import numpy as np
import pytest
import torch

from libfabric_amd import atomic
from tests import _sweep as S

pytestmark = pytest.mark.gpu

OPS = range(10)
# form-pairs x (vec, head) paths, from the pair lists: 22 of the 148 write
# pairs are 16-byte types, which have no head path
N_WRITE = 2 * (148 + 126)
N_TREE = 133 * 7 * 3
# nt: (pairs + pairs below 16 bytes); tapered write-through: the same without
# ATOMIC_READ's 13 pairs (2 of the 24 sixteen-byte pairs are its)
N_RW = (145 + 121) + (132 + 110)
N_SWAP = 84 + 70


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


def _n_cases(dts) -> int:
    return S.n_table_cases(dts, S.FORM_PATHS)


def test_pair_lists_match_the_library(manifest):
    """The lists the forced forms run over are the library's, and the form
    cases come to the literals."""
    wp = S.write_pairs(manifest)
    assert {(op, dt) for op in range(12) for dt in range(18)
            if atomic.reduce_valid(dt, op) == 0} == set(wp)
    assert {p for p in wp if p[0] <= 9} == set(S.reduce_pairs())
    assert len(wp) == 148 and len(S.reduce_pairs()) == 133
    assert sum(2 * _n_cases(S.table_dts(wp, op)) for op in S.WRITE_OPS) == N_WRITE == 548
    assert sum(S.n_tree_form_cases(op) for op in OPS) == N_TREE == 2793
    rp, sp = S.rw_pairs(), S.swap_pairs()
    assert len(rp) == 145 and len(sp) == 84
    assert sum(S.n_fetch_form_cases("readwrite", op, S.table_dts(rp, op))
               for op in S.RW_OPS) == N_RW == 508
    assert sum(S.n_fetch_form_cases("swap", op, S.table_dts(sp, op))
               for op in S.SWAP_OPS) == N_SWAP == 154


@pytest.mark.parametrize("op", S.WRITE_OPS)
def test_write_forms_every_pair(op, manifest):
    """combine_lds_taper (as 32 MiB) and the nt-drained combine_lds (as
    192 MiB) for every type of the op, on the vec and head paths."""
    dts = S.table_dts(S.write_pairs(manifest), op)
    cases = list(S.write_form_cases(op, dts, np.random.default_rng(17000 + op)))
    for form, as_bytes, dt, case in cases:
        t = _upload(case.arena)
        atomic.write_as(op, dt, case.view(t, "dst"), case.view(t, "src"),
                        S.lanes(S.esz_of(dt)), as_bytes)
        case.what = f"{case.what} as {form}"
        case.check(dt, t.cpu().numpy())
    assert len(cases) == 2 * _n_cases(dts) and dts
    assert {f for f, *_ in cases} == {f for f, _ in S.WRITE_AS}


@pytest.mark.parametrize("op", OPS)
def test_tree_forms_every_pair(op):
    """As 192 MiB of output: reduce_tree_lds at 2 inputs, reduce_tree_chunk
    U = 1 at 3, 5 and 8 (2, 4 and 8 leaves), U = 2 with nt stores at 9, 17 and
    32 (8, 16 and 32 leaves); plain, and with the output aliasing the highest
    input and input 0."""
    rng = np.random.default_rng(12000 + op)
    ran = 0
    for dt in S.dts_of(op):
        n = S.lanes(S.esz_of(dt))
        for form, as_bytes, case in S.tree_form_cases(op, dt, rng):
            t = _upload(case.arena)
            atomic.reduce_tree_as(op, dt, _view(t, case.outs[0]),
                                  [_view(t, s) for s in case.ins], n, as_bytes)
            case.check(dt, t.cpu().numpy())
            ran += 1
    assert ran == S.n_tree_form_cases(op) == 21 * len(S.dts_of(op)) and ran


@pytest.mark.parametrize("op", S.RW_OPS)
def test_readwrite_forms_every_pair(op):
    """fetch_lds_taper with nt stores (as 192 MiB) for every type of the op
    and, for every op but ATOMIC_READ, with write-through stores (as 64 MiB),
    on the vec and head paths."""
    dts = S.table_dts(S.rw_pairs(), op)
    cases = list(S.readwrite_form_cases(op, dts, np.random.default_rng(18000 + op)))
    for form, as_bytes, dt, case in cases:
        t = _upload(case.arena)
        atomic.readwrite_as(op, dt, case.view(t, "dst"),
                            case.view(t, "src") if "src" in case.at else None,
                            case.view(t, "res"), S.fetch_lanes(S.esz_of(dt)), as_bytes)
        case.what = f"{case.what} as {form}"
        case.check(dt, t.cpu().numpy())
    assert len(cases) == S.n_fetch_form_cases("readwrite", op, dts) and dts
    # 2 forms x (types on the vec path + on the head path, which the row's two
    # 16-byte types do not have); ATOMIC_READ, 13 types, has one form
    assert len(cases) == 24 if op == S.READ else len(cases) == {13: 48, 12: 44, 10: 36}[len(dts)]
    assert {f for f, *_ in cases} == {"fetch_lds_taper nt"} | \
        (set() if op == S.READ else {"fetch_lds_taper sc1"})
    assert {c.path for *_, c in cases} == set(S.FORM_PATHS)


@pytest.mark.parametrize("op", S.SWAP_OPS)
def test_swap_forms_every_pair(op):
    """fetch_lds_taper with nt stores (as 192 MiB) over the three-input
    compare functor for every type of the op, on the vec and head paths."""
    dts = S.table_dts(S.swap_pairs(), op)
    cases = list(S.swap_form_cases(op, dts, np.random.default_rng(19000 + op)))
    for form, as_bytes, dt, case in cases:
        t = _upload(case.arena)
        atomic.swap_as(op, dt, case.view(t, "dst"), case.view(t, "src"), case.view(t, "cmp"),
                       case.view(t, "res"), S.fetch_lanes(S.esz_of(dt)), as_bytes)
        case.what = f"{case.what} as {form}"
        case.check(dt, t.cpu().numpy())
    assert len(cases) == S.n_fetch_form_cases("swap", op, dts) == _n_cases(dts) and dts
    assert len(cases) == {13: 24, 12: 22, 10: 18}[len(dts)]
    assert {f for f, *_ in cases} == {"fetch_lds_taper nt"}
    assert {c.path for *_, c in cases} == set(S.FORM_PATHS)


def test_entries_at_as_zero_and_their_validation(manifest):
    """lfa__write_as, lfa__tree_as, lfa__readwrite_as and lfa__swap_as with
    as_bytes = 0 give a correct result
    (one pair each, the same check), and refuse what the public calls refuse.
    Which instantiation ran is not visible from here."""
    rng = np.random.default_rng(5)
    (_, _, dt, case), *_ = S.write_form_cases(S.SUM, [8], rng)
    t = _upload(case.arena)
    atomic.write_as(S.SUM, dt, case.view(t, "dst"), case.view(t, "src"), S.lanes(4), 0)
    case.check(dt, t.cpu().numpy())
    (_, _, case), *_ = S.tree_form_cases(S.SUM, 8, rng)
    t = _upload(case.arena)
    atomic.reduce_tree_as(S.SUM, 8, _view(t, case.outs[0]), [_view(t, s) for s in case.ins],
                          S.lanes(4), 0)
    case.check(8, t.cpu().numpy())
    # validation is the public calls'
    with pytest.raises(atomic.LfaError) as e:
        atomic.write_as(S.READ, 8, t, t, 1, 0)
    assert e.value.rc == -atomic.LFA_EOPNOTSUPP
    with pytest.raises(atomic.LfaError) as e:
        atomic.reduce_tree_as(S.SUM, 8, t, [], 1, 0)
    assert e.value.rc == -atomic.LFA_EINVAL
    # the fetch and compare entries: one pair of each table at as_bytes = 0
    (_, _, dt, case), *_ = S.readwrite_form_cases(S.SUM, [8], rng)
    t = _upload(case.arena)
    atomic.readwrite_as(S.SUM, dt, case.view(t, "dst"), case.view(t, "src"), case.view(t, "res"),
                        S.fetch_lanes(4), 0)
    case.check(dt, t.cpu().numpy())
    (_, _, dt, case), *_ = S.swap_form_cases(S.CSWAP_LE, [8], rng)
    t = _upload(case.arena)
    atomic.swap_as(S.CSWAP_LE, dt, case.view(t, "dst"), case.view(t, "src"), case.view(t, "cmp"),
                   case.view(t, "res"), S.fetch_lanes(4), 0)
    case.check(dt, t.cpu().numpy())
    # an op outside the table, then a null res, at as_bytes 0 and forced
    for as_bytes in (0, 192 * S.MIB):
        with pytest.raises(atomic.LfaError) as e:
            atomic.readwrite_as(S.CSWAP, 8, t, t, t, 1, as_bytes)
        assert e.value.rc == -atomic.LFA_EOPNOTSUPP
        with pytest.raises(atomic.LfaError) as e:
            atomic.swap_as(S.SUM, 8, t, t, t, t, 1, as_bytes)
        assert e.value.rc == -atomic.LFA_EOPNOTSUPP
        with pytest.raises(atomic.LfaError) as e:
            atomic.readwrite_as(S.SUM, 8, t, t, None, 1, as_bytes)
        assert e.value.rc == -atomic.LFA_EINVAL
        with pytest.raises(atomic.LfaError) as e:
            atomic.swap_as(S.CSWAP, 8, t, t, t, None, 1, as_bytes)
        assert e.value.rc == -atomic.LFA_EINVAL
    assert np.array_equal(t.cpu().numpy()[:64], case.arena[:64])      # the refused calls ran nothing
