"""The one-shot kernel's slot layout is checked on the host before any launch
(lfa_kernels.hpp launch_oneshot): both epoch parities live in FIXED halves of
SYM_IN, parity_off apart, and a layout whose n slots do not fit below
parity_off is refused.  Round 3's mixed in-flight failure came from parity
bases that moved with each operation's slot size; these
tests pin the argument rules without a GPU (every case returns before the
first HIP call)."""
import ctypes

import pytest

from libfabric_amd import coll
from libfabric_amd.atomic import LFA_EINVAL, LFA_EOPNOTSUPP

FI_SUM, FI_FLOAT = 2, 8
LL_BYTES = 16 << 10                  # lfa_signal.h LFA_OS_LL_BYTES
BASE = 1 << 30                       # never dereferenced: every case is refused


def _args(n=4, count=1024, slot=4096, parity_off=1 << 20, sym_align=0, mode=-1):
    sym = (ctypes.c_void_p * n)(*[BASE + k * (4 << 20) + sym_align for k in range(n)])
    a = coll.OneShot(BASE - (1 << 20), BASE - (2 << 20), count, mode,
                     ctypes.cast(sym, ctypes.c_void_p), slot, parity_off, 2 << 20, n, 0, 1,
                     BASE - (3 << 20), 1, 1000)
    return a, sym


@pytest.mark.parametrize("kw", [
    dict(parity_off=3 * 4096),                 # 4 slots of 4 KiB do not fit below it
    dict(parity_off=0),
    dict(parity_off=(1 << 20) + 16),           # not a multiple of 256
    dict(slot=4096 + 16),                      # slot not a multiple of 256
    dict(slot=2048),                           # smaller than the 4 KiB part
    dict(sym_align=16),                        # workspace not 256-B aligned
])
def test_layout_refused(kw):
    a, _sym = _args(**kw)
    with pytest.raises(coll.CollError) as e:
        coll.oneshot_reduce(FI_SUM, FI_FLOAT, a, None)
    assert e.value.rc == -LFA_EINVAL


@pytest.mark.parametrize("ll", [-1, 0, 1])
@pytest.mark.parametrize("kw", [dict(parity_off=0), dict(slot=2048), dict(sym_align=16)])
def test_oneshot_as_validation_is_the_public_entry(kw, ll):
    """lfa__oneshot_as (test-only: the kernel chosen per call) refuses what
    lfa_oneshot_reduce_async refuses, whatever ll says."""
    a, _sym = _args(**kw)
    with pytest.raises(coll.CollError) as e:
        coll.oneshot_reduce_as(FI_SUM, FI_FLOAT, a, None, ll)
    assert e.value.rc == -LFA_EINVAL
    with pytest.raises(coll.CollError) as e:
        coll.oneshot_reduce_as(11, FI_FLOAT, a, None, ll)       # ATOMIC_WRITE does not reduce
    assert e.value.rc == -LFA_EOPNOTSUPP
    with pytest.raises(coll.CollError) as e:
        coll.oneshot_reduce(11, FI_FLOAT, a, None)
    assert e.value.rc == -LFA_EOPNOTSUPP


@pytest.mark.parametrize("kw", [
    dict(n=1, mode=-1),                         # one member: nothing to exchange
    dict(count=LL_BYTES // 4 + 1, slot=LL_BYTES + 256, mode=-1),    # a part above LFA_OS_LL_BYTES
    dict(count=4 * (LL_BYTES // 4) + 4, slot=LL_BYTES + 256, mode=-2),  # scatter: a block above it
    dict(mode=0), dict(mode=3),                 # reduce to a root: the flagged kernel only
])
def test_oneshot_as_refuses_ll_where_the_launcher_never_takes_it(kw):
    """ll = 1 where launch_oneshot's rule forbids the LL kernel apart from the
    environment switch: -LFA_EINVAL before the first HIP call (these pointers
    are never dereferenced), not a silent fall-back to the flagged kernel."""
    a, _sym = _args(**kw)
    with pytest.raises(coll.CollError) as e:
        coll.oneshot_reduce_as(FI_SUM, FI_FLOAT, a, None, 1)
    assert e.value.rc == -LFA_EINVAL


def test_struct_matches_header():
    """ctypes mirror of struct lfa_oneshot: parity_off right after
    slot_bytes (lfa_signal.h)."""
    f = [name for name, _ in coll.OneShot._fields_]
    assert f.index("parity_off") == f.index("slot_bytes") + 1
    assert coll.OneShot.parity_off.offset == coll.OneShot.slot_bytes.offset + 8
