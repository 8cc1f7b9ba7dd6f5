"""Tensor-level access to the gfx950 combine kernels (liblfa.so).

Mirrors the reference's L4 combine interface (include/ofi_atomic.h:45-90):

  datatype_size(dt)                 ofi_datatype_size        util_atomic.c:58
  atomic_valid(dt, op, flags)       ofi_atomic_valid         util_atomic.c:1088
  write_handler(op, dt)             ofi_atomic_write_handlers[op][dt]
  write(op, dt, dst, src, cnt)      ofi_atomic_write_handler(op, dt, dst, src, cnt)
                                    — asynchronous on a HIP stream
  reduce_tree(op, dt, dst, srcs)    prov/coll's log2(N) REDUCE items fused into
                                    one pass (coll_coll.c:349-449 order)
  writev / reduce_treev / host_writev  the fi_ioc (list) forms of write /
                                    reduce_tree / host_write: every segment of
                                    a list in one launch (fi_atomicv's shape)
  readwritev / swapv / host_readwritev / host_swapv  the same for the fetch
                                    and compare tables (fi_fetch_atomicv,
                                    fi_compare_atomicv)
  host_readwrite / host_swap        the fetch and compare tables on host
                                    buffers (lfa_host_readwrite / lfa_host_swap)
  write_as / reduce_tree_as / readwrite_as / swap_as
                                    test-only: write / reduce_tree / readwrite
                                    / swap with the vector body's form chosen
                                    as if the body were `as_bytes` bytes
  reduce_valid / reduce_datatype_size  what write / reduce_tree / the
                                    collectives take: the table's columns plus
                                    DT.FLOAT16 and DT.BFLOAT16

Tensors are raw device storage: ``dt`` says how the bytes are interpreted,
``cnt`` defaults to ``dst.nbytes // datatype_size(dt)``.  Errors raise
``LfaError`` carrying the negative errno the C ABI returned.
"""
from __future__ import annotations

import ctypes

import torch

from ._native import LFA_IOV_MAX, lfa_ioc, lib  # noqa: F401  (re-exported)
from .enums import DT, OP

LFA_EOPNOTSUPP = 95
LFA_EINVAL = 22


class LfaError(RuntimeError):
    def __init__(self, rc: int, what: str):
        super().__init__(f"{what} failed: {rc}")
        self.rc = rc


def datatype_size(dt: int) -> int:
    return int(lib().lfa_datatype_size(int(dt)))


def atomic_valid(dt: int, op: int, flags: int = 0) -> int:
    return int(lib().lfa_atomic_valid(int(dt), int(op), int(flags)))


def reduce_datatype_size(dt: int) -> int:
    """Element size of what can be reduced: datatype_size for the 16 table
    columns, 2 for DT.FLOAT16 / DT.BFLOAT16, else 0."""
    return int(lib().lfa_reduce_datatype_size(int(dt)))


def reduce_valid(dt: int, op: int) -> int:
    """0 where write / reduce_tree / the collectives take (dt, op):
    atomic_valid(dt, op, 0) for the table columns, the float column's write
    rows for DT.FLOAT16 / DT.BFLOAT16; else -95."""
    return int(lib().lfa_reduce_valid(int(dt), int(op)))


_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


def write_handler(op: int, dt: int):
    """The synchronous table entry lfa_atomic_write_handlers[op][dt] or None."""
    tbl = (ctypes.c_void_p * (12 * 16)).in_dll(lib(), "lfa_atomic_write_handlers")
    p = tbl[int(op) * 16 + int(dt)]
    return _FN(p) if p else None


def _stream_handle(stream) -> int | None:
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def _check_dev(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (got {t.device})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def write(op: int, dt: int, dst: torch.Tensor, src: torch.Tensor,
          cnt: int | None = None, stream=None) -> None:
    """dst[i] = dst[i] OP src[i] on the GPU (enqueued, not waited for)."""
    _check_dev(dst, "dst")
    _check_dev(src, "src")
    esz = reduce_datatype_size(dt)
    if cnt is None:
        cnt = dst.nbytes // esz
    if cnt * esz > dst.nbytes or cnt * esz > src.nbytes:
        raise ValueError("cnt exceeds buffer size")
    rc = lib().lfa_atomic_write_async(int(op), int(dt), dst.data_ptr(),
                                      src.data_ptr(), cnt,
                                      _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_atomic_write_async({OP(op).name},{DT(dt).name})")


def write_ptr(op: int, dt: int, dst: int, src: int, cnt: int,
              stream=None) -> int:
    """Raw-pointer form (returns the C return code)."""
    return int(lib().lfa_atomic_write_async(int(op), int(dt), dst, src, cnt,
                                            _stream_handle(stream)))


def readwrite(op: int, dt: int, dst: torch.Tensor, src: torch.Tensor | None,
              res: torch.Tensor, cnt: int | None = None, stream=None) -> None:
    """res = dst; dst = dst OP src (ofi_atomic_readwrite_handler; ATOMIC_READ
    ignores src, ATOMIC_WRITE exchanges)."""
    _check_dev(dst, "dst")
    _check_dev(res, "res")
    esz = datatype_size(dt)
    if cnt is None:
        cnt = dst.nbytes // esz
    rc = lib().lfa_atomic_readwrite_async(
        int(op), int(dt), dst.data_ptr(), src.data_ptr() if src is not None else None,
        res.data_ptr(), cnt, _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_atomic_readwrite_async({op},{DT(dt).name})")


def swap(op: int, dt: int, dst: torch.Tensor, src: torch.Tensor, cmp: torch.Tensor,
         res: torch.Tensor, cnt: int | None = None, stream=None) -> None:
    """res = dst; dst = src where (cmp OP dst) (ofi_atomic_swap_handler)."""
    for name, t in (("dst", dst), ("src", src), ("cmp", cmp), ("res", res)):
        _check_dev(t, name)
    esz = datatype_size(dt)
    if cnt is None:
        cnt = dst.nbytes // esz
    rc = lib().lfa_atomic_swap_async(int(op), int(dt), dst.data_ptr(), src.data_ptr(),
                                     cmp.data_ptr(), res.data_ptr(), cnt,
                                     _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_atomic_swap_async({op},{DT(dt).name})")


def reduce_tree(op: int, dt: int, dst: torch.Tensor, srcs: list[torch.Tensor],
                cnt: int | None = None, stream=None) -> None:
    """dst = recursive-doubling tree of srcs (rank order = list order)."""
    _check_dev(dst, "dst")
    for i, s in enumerate(srcs):
        _check_dev(s, f"srcs[{i}]")
    esz = reduce_datatype_size(dt)
    if cnt is None:
        cnt = dst.nbytes // esz
    if any(cnt * esz > s.nbytes for s in srcs) or cnt * esz > dst.nbytes:
        raise ValueError("cnt exceeds buffer size")
    arr = (ctypes.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    rc = lib().lfa_reduce_tree_async(int(op), int(dt), dst.data_ptr(), arr,
                                     len(srcs), cnt, _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_reduce_tree_async({OP(op).name},{DT(dt).name})")


def reduce_tree_put(op: int, dt: int, dsts: list[torch.Tensor], srcs: list[torch.Tensor],
                    cnt: int | None = None, stream=None) -> None:
    """Every dsts[j] = recursive-doubling tree of srcs, one pass, system-scope
    accesses (lfa_reduce_tree_put_async, the LFA_ALGO_P2P kernel)."""
    for i, t in enumerate(list(dsts) + list(srcs)):
        _check_dev(t, f"operand {i}")
    esz = reduce_datatype_size(dt)
    if cnt is None:
        cnt = dsts[0].nbytes // esz
    if any(cnt * esz > t.nbytes for t in list(dsts) + list(srcs)):
        raise ValueError("cnt exceeds buffer size")
    sa = (ctypes.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
    da = (ctypes.c_void_p * len(dsts))(*[t.data_ptr() for t in dsts])
    rc = lib().lfa_reduce_tree_put_async(int(op), int(dt), da, len(dsts), sa, len(srcs),
                                         cnt, _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_reduce_tree_put_async({OP(op).name},{DT(dt).name})")


# ------------------------------------------------- forced forms (tests) ----
# write / reduce_tree / readwrite / swap with the vector body's form chosen as
# if the body were `as_bytes` bytes (lfa_split.h: lfa_form_write /
# lfa_form_tree / lfa_form_fetch); everything else about the launch follows
# the real size.  For tests/test_sweep_forms_gpu.py, which runs the forms a
# launcher only takes from 32, 64 or 192 MiB on small buffers; no product caller.

def write_as(op: int, dt: int, dst: torch.Tensor, src: torch.Tensor, cnt: int,
             as_bytes: int, stream=None) -> None:
    _check_dev(dst, "dst")
    _check_dev(src, "src")
    esz = reduce_datatype_size(dt)
    if cnt * esz > dst.nbytes or cnt * esz > src.nbytes:
        raise ValueError("cnt exceeds buffer size")
    rc = lib().lfa__write_as(int(op), int(dt), dst.data_ptr(), src.data_ptr(), cnt,
                             _stream_handle(stream), as_bytes)
    if rc:
        raise LfaError(rc, f"lfa__write_as({op},{dt},{as_bytes})")


def reduce_tree_as(op: int, dt: int, dst: torch.Tensor, srcs: list[torch.Tensor], cnt: int,
                   as_bytes: int, stream=None) -> None:
    _check_dev(dst, "dst")
    for i, s in enumerate(srcs):
        _check_dev(s, f"srcs[{i}]")
    esz = reduce_datatype_size(dt)
    if any(cnt * esz > s.nbytes for s in srcs) or cnt * esz > dst.nbytes:
        raise ValueError("cnt exceeds buffer size")
    arr = (ctypes.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    rc = lib().lfa__tree_as(int(op), int(dt), dst.data_ptr(), arr, len(srcs), cnt,
                            _stream_handle(stream), as_bytes)
    if rc:
        raise LfaError(rc, f"lfa__tree_as({op},{dt},{as_bytes})")


def readwrite_as(op: int, dt: int, dst: torch.Tensor, src: torch.Tensor | None,
                 res: torch.Tensor | None, cnt: int, as_bytes: int, stream=None) -> None:
    """readwrite under lfa_form_fetch(as_bytes).  res may be None: the entry
    refuses it as the public call does."""
    _check_dev(dst, "dst")
    esz = datatype_size(dt)
    if any(t is not None and cnt * esz > t.nbytes for t in (dst, src, res)):
        raise ValueError("cnt exceeds buffer size")
    rc = lib().lfa__readwrite_as(int(op), int(dt), dst.data_ptr(),
                                 src.data_ptr() if src is not None else None,
                                 res.data_ptr() if res is not None else None, cnt,
                                 _stream_handle(stream), as_bytes)
    if rc:
        raise LfaError(rc, f"lfa__readwrite_as({op},{dt},{as_bytes})")


def swap_as(op: int, dt: int, dst: torch.Tensor, src: torch.Tensor, cmp: torch.Tensor,
            res: torch.Tensor | None, cnt: int, as_bytes: int, stream=None) -> None:
    """swap under lfa_form_fetch(as_bytes); res may be None, as above."""
    for name, t in (("dst", dst), ("src", src), ("cmp", cmp)):
        _check_dev(t, name)
    esz = datatype_size(dt)
    if any(t is not None and cnt * esz > t.nbytes for t in (dst, src, cmp, res)):
        raise ValueError("cnt exceeds buffer size")
    rc = lib().lfa__swap_as(int(op), int(dt), dst.data_ptr(), src.data_ptr(), cmp.data_ptr(),
                            res.data_ptr() if res is not None else None, cnt,
                            _stream_handle(stream), as_bytes)
    if rc:
        raise LfaError(rc, f"lfa__swap_as({op},{dt},{as_bytes})")


# ------------------------------------------------------------- list forms --

def _ioc_array(ptrs: list[int], counts: list[int]):
    arr = (lfa_ioc * max(len(ptrs), 1))()
    for i, (p, n) in enumerate(zip(ptrs, counts)):
        arr[i].addr = p
        arr[i].count = n
    return arr


def _seg_counts(dsts, esz: int) -> list[int]:
    return [d.nbytes // esz for d in dsts]


def writev(op: int, dt: int, dsts: list[torch.Tensor], srcs: list[torch.Tensor],
           stream=None) -> None:
    """dsts[i] = dsts[i] OP srcs[i] for every i in ONE launch
    (lfa_atomic_writev_async, the fi_ioc form of ``write``).  Segment i has
    dsts[i].nbytes // size(dt) elements; srcs[i] must hold as many."""
    if len(dsts) != len(srcs):
        raise ValueError("dsts and srcs differ in length")
    for i, (d, s) in enumerate(zip(dsts, srcs)):
        _check_dev(d, f"dsts[{i}]")
        _check_dev(s, f"srcs[{i}]")
    esz = reduce_datatype_size(dt)
    da = _ioc_array([d.data_ptr() for d in dsts], _seg_counts(dsts, esz) if esz else [])
    sa = _ioc_array([s.data_ptr() for s in srcs], _seg_counts(srcs, esz) if esz else [])
    rc = lib().lfa_atomic_writev_async(int(op), int(dt), da, sa, len(dsts),
                                       _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_atomic_writev_async({OP(op).name},{DT(dt).name})")


def reduce_treev(op: int, dt: int, dsts: list[torch.Tensor],
                 srcs: list[list[torch.Tensor]], stream=None) -> None:
    """dsts[i] = recursive-doubling tree of srcs[i] for every i in ONE launch
    (lfa_reduce_treev_async); every srcs[i] has the same length, and dsts[i]
    may be one of its own srcs[i]."""
    if len(dsts) != len(srcs):
        raise ValueError("dsts and srcs differ in length")
    nsrc = len(srcs[0]) if srcs else 1
    esz = reduce_datatype_size(dt)
    for i, (d, row) in enumerate(zip(dsts, srcs)):
        if len(row) != nsrc:
            raise ValueError("every segment needs the same number of inputs")
        _check_dev(d, f"dsts[{i}]")
        for k, s in enumerate(row):
            _check_dev(s, f"srcs[{i}][{k}]")
            if s.nbytes < d.nbytes:
                raise ValueError(f"srcs[{i}][{k}] is shorter than dsts[{i}]")
    da = _ioc_array([d.data_ptr() for d in dsts], _seg_counts(dsts, esz) if esz else [])
    flat = [s.data_ptr() for row in srcs for s in row]
    sa = (ctypes.c_void_p * max(len(flat), 1))(*flat)
    rc = lib().lfa_reduce_treev_async(int(op), int(dt), da, sa, nsrc, len(dsts),
                                      _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_reduce_treev_async({OP(op).name},{DT(dt).name})")


def host_writev(op: int, dt: int, dsts, srcs) -> None:
    """The list form on HOST buffers (numpy arrays or CPU tensors):
    lfa_host_writev, what one host_write per segment gives."""
    if len(dsts) != len(srcs):
        raise ValueError("dsts and srcs differ in length")
    esz = reduce_datatype_size(dt)
    da = _ioc_array([_host_ptr(d) for d in dsts], _seg_counts(dsts, esz) if esz else [])
    sa = _ioc_array([_host_ptr(s) for s in srcs], _seg_counts(srcs, esz) if esz else [])
    rc = lib().lfa_host_writev(int(op), int(dt), da, sa, len(dsts))
    if rc:
        raise LfaError(rc, f"lfa_host_writev({op},{dt})")


def _fetch_lists(dt: int, ptr, dsts, **others):
    """The lfa_ioc arrays of a fetch / compare list call: dsts, then every
    list of `others` in order (None stays None: ATOMIC_READ's srcs)."""
    esz = datatype_size(dt)
    out = []
    for name, lst in (("dsts", dsts), *others.items()):
        if lst is None:
            out.append(None)
            continue
        if len(lst) != len(dsts):
            raise ValueError(f"dsts and {name} differ in length")
        out.append(_ioc_array([ptr(t, f"{name}[{i}]") for i, t in enumerate(lst)],
                              _seg_counts(lst, esz) if esz else []))
    return out


def _dev_ptr(t: torch.Tensor, name: str) -> int:
    _check_dev(t, name)
    return t.data_ptr()


def readwritev(op: int, dt: int, dsts: list[torch.Tensor], srcs: list[torch.Tensor] | None,
               ress: list[torch.Tensor], stream=None) -> None:
    """ress[i] = dsts[i]; dsts[i] = dsts[i] OP srcs[i] for every i in ONE launch
    (lfa_atomic_readwritev_async, the fi_ioc form of ``readwrite``).
    ATOMIC_READ ignores srcs, which may be None."""
    da, sa, ra = _fetch_lists(dt, _dev_ptr, dsts, srcs=srcs, ress=ress)
    rc = lib().lfa_atomic_readwritev_async(int(op), int(dt), da, sa, ra, len(dsts),
                                           _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_atomic_readwritev_async({op},{dt})")


def swapv(op: int, dt: int, dsts: list[torch.Tensor], srcs: list[torch.Tensor],
          cmps: list[torch.Tensor], ress: list[torch.Tensor], stream=None) -> None:
    """ress[i] = dsts[i]; dsts[i] = srcs[i] where (cmps[i] OP dsts[i]) for every
    i in ONE launch (lfa_atomic_swapv_async, the fi_ioc form of ``swap``)."""
    da, sa, ca, ra = _fetch_lists(dt, _dev_ptr, dsts, srcs=srcs, cmps=cmps, ress=ress)
    rc = lib().lfa_atomic_swapv_async(int(op), int(dt), da, sa, ca, ra, len(dsts),
                                      _stream_handle(stream))
    if rc:
        raise LfaError(rc, f"lfa_atomic_swapv_async({op},{dt})")


def host_readwritev(op: int, dt: int, dsts, srcs, ress) -> None:
    """``readwritev`` on HOST buffers (numpy arrays or CPU tensors):
    lfa_host_readwritev, what one host_readwrite per segment gives."""
    da, sa, ra = _fetch_lists(dt, lambda a, _: _host_ptr(a), dsts, srcs=srcs, ress=ress)
    rc = lib().lfa_host_readwritev(int(op), int(dt), da, sa, ra, len(dsts))
    if rc:
        raise LfaError(rc, f"lfa_host_readwritev({op},{dt})")


def host_swapv(op: int, dt: int, dsts, srcs, cmps, ress) -> None:
    """``swapv`` on HOST buffers: lfa_host_swapv, what one host_swap per
    segment gives."""
    da, sa, ca, ra = _fetch_lists(dt, lambda a, _: _host_ptr(a), dsts, srcs=srcs, cmps=cmps,
                                  ress=ress)
    rc = lib().lfa_host_swapv(int(op), int(dt), da, sa, ca, ra, len(dsts))
    if rc:
        raise LfaError(rc, f"lfa_host_swapv({op},{dt})")


# ------------------------------------------------------- host-memory forms --

def _host_ptr(a) -> int:
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise ValueError("host form called with a device tensor")
        return a.data_ptr()
    return a.ctypes.data


def host_write(op: int, dt: int, dst, src, cnt: int | None = None) -> None:
    """dst[i] = dst[i] OP src[i] for HOST buffers (numpy arrays or CPU
    tensors), lfa_host_write: the kernels' functors run on the host."""
    esz = reduce_datatype_size(dt)
    if cnt is None:
        cnt = dst.nbytes // esz
    rc = lib().lfa_host_write(int(op), int(dt), _host_ptr(dst), _host_ptr(src), cnt)
    if rc:
        raise LfaError(rc, f"lfa_host_write({op},{dt})")


def host_readwrite(op: int, dt: int, dst, src, res, cnt: int | None = None) -> None:
    """res = dst; dst = dst OP src for HOST buffers (lfa_host_readwrite);
    ATOMIC_READ takes src=None."""
    if cnt is None:
        cnt = dst.nbytes // datatype_size(dt)
    rc = lib().lfa_host_readwrite(int(op), int(dt), _host_ptr(dst),
                                  _host_ptr(src) if src is not None else None,
                                  _host_ptr(res), cnt)
    if rc:
        raise LfaError(rc, f"lfa_host_readwrite({op},{dt})")


def host_swap(op: int, dt: int, dst, src, cmp, res, cnt: int | None = None) -> None:
    """res = dst; dst = src where (cmp OP dst) for HOST buffers (lfa_host_swap)."""
    if cnt is None:
        cnt = dst.nbytes // datatype_size(dt)
    rc = lib().lfa_host_swap(int(op), int(dt), _host_ptr(dst), _host_ptr(src),
                             _host_ptr(cmp), _host_ptr(res), cnt)
    if rc:
        raise LfaError(rc, f"lfa_host_swap({op},{dt})")


def host_reduce_tree(op: int, dt: int, dst, srcs, cnt: int | None = None) -> None:
    """dst = prov/coll's recursive-doubling tree of HOST buffers srcs."""
    esz = reduce_datatype_size(dt)
    if cnt is None:
        cnt = dst.nbytes // esz
    arr = (ctypes.c_void_p * len(srcs))(*[_host_ptr(s) for s in srcs])
    rc = lib().lfa_host_reduce_tree(int(op), int(dt), _host_ptr(dst), arr, len(srcs), cnt)
    if rc:
        raise LfaError(rc, f"lfa_host_reduce_tree({op},{dt})")
