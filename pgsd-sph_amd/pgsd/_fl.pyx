# cython: language_level=3, binding=True
"""PGSD file layer API, MI355X-native (compiled part; import it as ``pgsd.fl``).

Mirror of the reference's Cython module ``pgsd.fl`` (/root/reference/pgsd/pgsd/fl.pyx): same
``open`` / ``PGSDFile`` surface, argument meaning, return shapes and exceptions, bound -- like the
reference -- with Cython to the C ABI of the library underneath (``libpgsd_amd.so``, declared in
``libpgsd_amd.pxd`` from ``include/pgsd.h``); the handle is embedded in the object (fl.pyx:284) and every
C call runs without the GIL (fl.pyx:352-860).  On top of the reference's host-array ``write_chunk`` the
same method accepts **device-resident** data (a torch tensor on the GPU or a :class:`DeviceField`), which
is packed by the HIP kernels and streamed to the file without a host copy in Python;
:meth:`PGSDFile.write_chunks` packs several per-particle chunks with one fused launch.
"""
import collections
import ctypes
import errno as _errno
import logging
import os
from pickle import PickleError

import numpy

from libc.errno cimport errno
from libc.stdint cimport int32_t, uint8_t, uint32_t, uint64_t, uintptr_t
from libc.stdlib cimport calloc, free
from libc.string cimport memset
from cpython.buffer cimport PyObject_GetBuffer, PyBuffer_Release, PyBUF_ANY_CONTIGUOUS, PyBUF_SIMPLE

from . cimport libpgsd_amd as C
from . import _lib

logger = logging.getLogger('pgsd.fl')

if C.pgsd_abi_version() != C.PGSD_ABI_VERSION:
    raise ImportError("pgsd/_fl was built against ABI version %d of include/pgsd.h, libpgsd_amd.so has %d: rebuild "
                      "(`make -C pgsd-sph_amd/csrc`)" % (C.PGSD_ABI_VERSION, C.pgsd_abi_version()))

_NP_TO_PGSD = {
    numpy.dtype('uint8'): 1, numpy.dtype('uint16'): 2, numpy.dtype('uint32'): 3, numpy.dtype('uint64'): 4,
    numpy.dtype('int8'): 5, numpy.dtype('int16'): 6, numpy.dtype('int32'): 7, numpy.dtype('int64'): 8,
    numpy.dtype('float32'): 9, numpy.dtype('float64'): 10,
}
_PGSD_TO_NP = {v: k for k, v in _NP_TO_PGSD.items()}
_TORCH_DTYPE_TO_PGSD = {}   # torch.dtype -> pgsd type id, filled on first use
_TORCH_HAS_GPU = None       # torch.cuda.is_available(), asked once


def _pgsd_type(dtype, name=''):
    """numpy dtype / torch dtype / name -> pgsd type id (ValueError like fl.pyx:633)."""
    try:
        if not isinstance(dtype, numpy.dtype):
            t = _TORCH_DTYPE_TO_PGSD.get(dtype)
            if t is not None:
                return t
            s = str(dtype)
            is_torch = s.startswith('torch.')
            if is_torch:
                s = s[6:]
            t = _NP_TO_PGSD[numpy.dtype(s)]
            if is_torch:
                _TORCH_DTYPE_TO_PGSD[dtype] = t
            return t
        return _NP_TO_PGSD[dtype]
    except (KeyError, TypeError):
        raise ValueError("invalid type for chunk: " + name)


cdef _raise_on_error(int retval, extra, int err=0):
    """Error code -> exception, the mapping of fl.pyx:35-61 plus the device/comm codes."""
    if retval == 0:
        return
    if retval == C.PGSD_ERROR_IO:
        err = err or _errno.EIO
        raise IOError(err, os.strerror(err), extra)
    elif retval == C.PGSD_ERROR_NOT_A_PGSD_FILE:
        raise RuntimeError("Not a PGSD file: " + extra)
    elif retval == C.PGSD_ERROR_INVALID_PGSD_FILE_VERSION:
        raise RuntimeError("Unsupported PGSD file version: " + extra)
    elif retval == C.PGSD_ERROR_FILE_CORRUPT:
        raise RuntimeError("Corrupt PGSD file: " + extra)
    elif retval == C.PGSD_ERROR_MEMORY_ALLOCATION_FAILED:
        raise MemoryError("Memory allocation failed: " + extra)
    elif retval == C.PGSD_ERROR_NAMELIST_FULL:
        raise RuntimeError("PGSD namelist is full: " + extra)
    elif retval == C.PGSD_ERROR_FILE_MUST_BE_WRITABLE:
        raise RuntimeError("File must be writable: " + extra)
    elif retval == C.PGSD_ERROR_FILE_MUST_BE_READABLE:
        raise RuntimeError("File must be readable: " + extra)
    elif retval == C.PGSD_ERROR_INVALID_ARGUMENT:
        raise RuntimeError("Invalid pgsd argument: " + extra)
    elif retval in (C.PGSD_ERROR_DEVICE, C.PGSD_ERROR_NO_DEVICE, C.PGSD_ERROR_COMM):
        msg = C.pgsd_last_error_string()
        raise RuntimeError("PGSD device/communicator error (%d): %s: %s"
                           % (retval, msg.decode('utf-8', 'replace') if msg != NULL else '', extra))
    else:
        raise RuntimeError("Unknown error: " + extra)


def _device_index_of(field):
    """GPU index of the array behind a field (a DeviceField made from a tensor keeps it alive; or a tensor), or None."""
    keep = field.keepalive if isinstance(field, DeviceField) else field
    for t in (keep if isinstance(keep, (list, tuple)) else [keep]):
        index = getattr(getattr(t, 'device', None), 'index', None)
        if index is not None:
            return index
    return None


cdef class DeviceField:
    """Describe rows that live in GPU memory: ``chunk[i, c] = src[order[i]][col0 + c]``.

    Args:
        ptr (int): device address of the source array's first row.
        dtype: element type of the source array (numpy dtype or name).
        N (int): number of rows to write.
        M (int): number of columns of the chunk.
        stride (int): elements between consecutive source rows (4 for a HOOMD ``Scalar4``).
        col0 (int): first source column.
        out_dtype: element type of the chunk (default: ``dtype``); ``float64`` sources can be
            written as ``float32`` chunks.
        order (int): device address of an optional ``uint32[N]`` gather index (e.g. HOOMD's
            reverse-tag array) or ``None``.
        bitcast (bool): reinterpret the low bytes instead of converting the value (HOOMD
            keeps the type id in ``position.w`` as ``__int_as_scalar``).
        keepalive: any object that must stay alive until the frame is written.
    """
    cdef public object dtype, out_dtype, keepalive
    cdef public object ptr, order
    cdef public Py_ssize_t N, M, stride, col0
    cdef public bint bitcast
    cdef uint32_t _src_type, _out_type

    def __init__(self, ptr, dtype, N, M, stride=None, col0=0, out_dtype=None, order=None,
                 bitcast=False, keepalive=None):
        self.ptr = int(ptr)
        self.dtype = numpy.dtype(dtype)
        self.N = int(N)
        self.M = int(M)
        self.stride = int(stride if stride is not None else M)
        self.col0 = int(col0)
        self.out_dtype = numpy.dtype(out_dtype) if out_dtype is not None else self.dtype
        self.order = int(order) if order else None
        self.bitcast = bool(bitcast)
        self.keepalive = keepalive
        self._src_type = _pgsd_type(self.dtype)
        self._out_type = 0      # resolved (with the chunk's name in the error) when written

    @classmethod
    def from_tensor(cls, t, out_dtype=None, order=None, bitcast=False, columns=None):
        """Build from a torch GPU tensor of shape (N,), (N, M) or a column slice of (N, S)."""
        if columns is None and order is None and t.dim() == 2 and t.is_contiguous():
            # the common case (a whole row-major array), without the general path's dozen tensor queries
            N, M = t.shape
            return cls(t.data_ptr(), str(t.dtype)[6:], N, M, stride=max(M, 1), col0=0, out_dtype=out_dtype,
                       order=None, bitcast=bitcast, keepalive=[t])
        if t.dim() == 1:
            t2 = t.unsqueeze(1)
        elif t.dim() == 2:
            t2 = t
        else:
            raise ValueError("PGSD can only write 1 or 2 dimensional arrays")
        N, M = int(t2.shape[0]), int(t2.shape[1])
        if columns is not None:
            c0, c1 = columns
            t2 = t2[:, c0:c1]
            M = c1 - c0
        if M > 1 and t2.stride(1) != 1:
            t2 = t2.contiguous()
        stride = int(t2.stride(0)) if N > 1 else max(M, 1)
        itemsize = t2.element_size()
        col0 = 0
        ptr = t2.data_ptr()
        if stride < M:
            t2 = t2.contiguous()
            stride, ptr = M, t2.data_ptr()
        elif stride > M:
            # column slice of a wider row-major array: address whole rows so that the kernel
            # streams aligned, contiguous source tiles
            c = t2.storage_offset() % stride
            if c + M <= stride and t2.storage_offset() >= c:
                col0 = c
                ptr -= c * itemsize
        keep = [t2]
        order_ptr = None
        if order is not None:
            if str(order.dtype) not in ('torch.int32', 'torch.uint32'):
                raise ValueError("order must be a 32-bit integer tensor")
            order = order.contiguous()
            order_ptr = order.data_ptr()
            keep.append(order)
            N = int(order.shape[0])
        s = str(t2.dtype)[6:]
        return cls(ptr, s, N, M, stride=stride, col0=col0,
                   out_dtype=out_dtype, order=order_ptr, bitcast=bitcast, keepalive=keep)

    @classmethod
    def from_device_array(cls, a, out_dtype=None, bitcast=False, columns=None, order=None):
        """Build from any object that describes GPU memory through ``__cuda_array_interface__`` (version 2 or 3; the
        protocol ROCm builds of HOOMD's GPU snapshots, CuPy, Numba and PyTorch share): shape ``(N,)``, ``(N, M)`` or a
        column range ``columns=(c0, c1)`` of ``(N, S)`` -- a ``Scalar4`` array --, row-major, rows possibly strided.
        ``order``: an optional 32-bit integer array of the same kind (gather index).  The arrays must be complete when
        the chunk is written (the protocol's ``stream`` entry is not waited on: order the producer against
        :meth:`PGSDFile.set_source_stream`, or synchronise it)."""
        if _is_device_tensor(a):
            return cls.from_tensor(a, out_dtype=out_dtype, order=order, bitcast=bitcast, columns=columns)
        ptr, dt, N, S, row = _rows2d(a, "device array")
        c0, c1 = (0, S) if columns is None else (int(columns[0]), int(columns[1]))
        if not (0 <= c0 < c1 <= S) or row < S:
            raise ValueError("columns outside the array's rows")
        keep = [a]
        order_ptr = None
        if order is not None:
            if _is_device_tensor(order):
                o_ptr, o_dt, o_n = order.data_ptr(), numpy.dtype(str(order.dtype)[6:]), int(order.shape[0])
                dense = order.dim() == 1 and order.is_contiguous()
            else:
                oi = order.__cuda_array_interface__
                o_ptr, o_dt, o_n = int(oi['data'][0]), numpy.dtype(oi['typestr']), int(oi['shape'][0])
                dense = len(oi['shape']) == 1 and oi.get('strides') in (None, (4,))
            if o_dt not in (numpy.dtype('<i4'), numpy.dtype('<u4')) or not dense:
                raise ValueError("order must be a contiguous 32-bit integer device array")
            order_ptr, N = o_ptr, o_n
            keep.append(order)
        return cls(ptr, dt, N, c1 - c0, stride=max(row, 1), col0=c0, out_dtype=out_dtype, order=order_ptr,
                   bitcast=bitcast, keepalive=keep)

    cdef void fill_desc(self, C.pgsd_field_desc* d):
        d.src = <const void*><uintptr_t>self.ptr
        d.order = <const uint32_t*><uintptr_t>(self.order if self.order is not None else 0)
        d.src_type = self._src_type
        d.src_stride = <uint32_t>self.stride
        d.src_col0 = <uint32_t>self.col0
        d.bitcast = 1 if self.bitcast else 0

    cdef uint32_t out_type(self, name) except 0:
        if self._out_type == 0:
            self._out_type = _pgsd_type(self.out_dtype, name)
        return self._out_type

    def _desc(self):
        """ctypes ``FieldDesc`` of this field (tests and tools that call the C ABI directly)."""
        d = _lib.FieldDesc()
        d.src = self.ptr
        d.order = self.order
        d.src_type = self._src_type
        d.src_stride = self.stride
        d.src_col0 = self.col0
        d.bitcast = 1 if self.bitcast else 0
        return d


def _is_device_tensor(x):
    return hasattr(x, 'data_ptr') and getattr(x, 'is_cuda', False)


def _is_device_array(x):
    """A torch GPU tensor, or any other object that describes GPU memory through ``__cuda_array_interface__``."""
    if _is_device_tensor(x):
        return True
    if hasattr(x, 'data_ptr'):
        return False                    # a torch tensor in host memory (its __cuda_array_interface__ raises)
    try:
        return isinstance(getattr(x, '__cuda_array_interface__', None), dict)
    except Exception:
        return False


cdef class DeviceBuffer:
    """Device memory owned by ``libpgsd_amd.so`` (``pgsd_device_alloc``), described through
    ``__cuda_array_interface__`` (version 3) so that PyTorch, CuPy, Numba or HOOMD take it without a copy
    (``torch.as_tensor(buf, device='cuda')``).  What :mod:`pgsd.fl` / :mod:`pgsd.hoomd` keep in HBM themselves lives
    here -- references of the GPU-side elision, rows of device reads when no tensor library is importable, index
    lists of :func:`select_rows` -- so the Python device path needs no tensor library: torch is an optional
    PRODUCER of source arrays, never a requirement.

    Args:
        shape: tuple of ints (or an int).
        dtype: numpy dtype of an element.
        device (int): HIP device ordinal (-1: the current one).
        pattern: optional host array / bytes repeated over the whole buffer (rows of a default value).
    """
    cdef public object dtype, shape, strides, base
    cdef public Py_ssize_t nbytes
    cdef public int device
    cdef uintptr_t _ptr
    cdef bint _owner

    def __init__(self, shape, dtype=numpy.uint8, device=-1, pattern=None):
        self.dtype = numpy.dtype(dtype)
        self.shape = (int(shape),) if isinstance(shape, (int, numpy.integer)) else tuple(int(x) for x in shape)
        self.strides = None
        self.base = None
        self.device = int(device)
        n = 1
        for x in self.shape:
            n *= x
        self.nbytes = n * self.dtype.itemsize
        cdef size_t c_bytes = self.nbytes, c_pat = 0
        cdef const void* c_ptr = NULL
        cdef int c_dev = self.device
        cdef void* got
        pat = None
        if pattern is not None:
            pat = numpy.ascontiguousarray(pattern).view(numpy.uint8).reshape(-1)
            if pat.size > 0:
                c_pat = pat.size
                c_ptr = <const void*><uintptr_t>pat.ctypes.data
        with nogil:
            got = C.pgsd_device_alloc(c_dev, c_bytes, c_ptr, c_pat)
        if got == NULL:
            msg = C.pgsd_last_error_string()
            raise RuntimeError("pgsd_device_alloc(%d bytes) failed: %s"
                               % (self.nbytes, msg.decode('utf-8', 'replace') if msg != NULL else ''))
        self._ptr = <uintptr_t>got
        self._owner = True

    def __dealloc__(self):
        if self._owner and self._ptr != 0:
            C.pgsd_device_free(self.device, <void*>self._ptr)
            self._ptr = 0

    @property
    def ptr(self):
        return int(self._ptr)

    def data_ptr(self):
        return int(self._ptr)

    def numel(self):
        n = 1
        for x in self.shape:
            n *= x
        return n

    def element_size(self):
        return self.dtype.itemsize

    def is_contiguous(self):
        return self.strides is None

    def __len__(self):
        return self.shape[0] if self.shape else 1

    @property
    def __cuda_array_interface__(self):
        return {'shape': self.shape, 'typestr': self.dtype.str, 'data': (int(self._ptr), False), 'version': 3,
                'strides': self.strides}

    def view(self, dtype=None, shape=None, strides=None, offset_bytes=0):
        """Another description of (a part of) the same memory; the view keeps this buffer alive.  ``strides`` in
        bytes (0 repeats a row: the default rows of :meth:`pgsd.hoomd.HOOMDTrajectory.read_frame_device`)."""
        cdef DeviceBuffer v = DeviceBuffer.__new__(DeviceBuffer)
        v.dtype = numpy.dtype(dtype) if dtype is not None else self.dtype
        if shape is None:
            if self.nbytes % v.dtype.itemsize != 0:
                raise ValueError("the buffer is not a whole number of such elements")
            shape = ((self.nbytes - int(offset_bytes)) // v.dtype.itemsize,)
        v.shape = (int(shape),) if isinstance(shape, (int, numpy.integer)) else tuple(int(x) for x in shape)
        v.strides = tuple(int(x) for x in strides) if strides is not None else None
        n = 1
        for x in v.shape:
            n *= x
        # the bytes the view can reach must lie inside this buffer
        if v.strides is None:
            reach = n * v.dtype.itemsize
        else:
            reach = v.dtype.itemsize if n > 0 else 0
            for x, st in zip(v.shape, v.strides):
                reach += (x - 1) * st if x > 0 else 0
        if offset_bytes < 0 or int(offset_bytes) + reach > self.nbytes:
            raise ValueError("the view does not fit the buffer")
        v.nbytes = n * v.dtype.itemsize
        v.device = self.device
        v.base = self
        v._ptr = self._ptr + <uintptr_t>int(offset_bytes)
        v._owner = False
        return v

    def clone(self):
        """A buffer of its own with the same (dense) contents: one device-to-device copy."""
        if self.strides is not None:
            raise ValueError("only dense buffers are cloned")
        cdef DeviceBuffer c = DeviceBuffer(self.shape, self.dtype, self.device)
        cdef int rc, dev = self.device
        cdef size_t n = self.nbytes
        cdef uintptr_t d = c._ptr, s = self._ptr
        with nogil:
            rc = C.pgsd_device_copy(dev, <void*>d, <const void*>s, n)
        _raise_on_error(rc, "DeviceBuffer.clone")
        return c

    def to_host(self):
        """The contents as a numpy array (one device-to-host copy; dense buffers only)."""
        if self.strides is not None:
            raise ValueError("only dense buffers are copied to the host")
        out = numpy.empty(self.shape, dtype=self.dtype)
        cdef int rc, dev = self.device
        cdef size_t n = self.nbytes
        cdef uintptr_t d = out.ctypes.data, s = self._ptr
        if n:
            with nogil:
                rc = C.pgsd_device_copy(dev, <void*>d, <const void*>s, n)
            _raise_on_error(rc, "DeviceBuffer.to_host")
        return out


def _device_memory(x, what="array"):
    """(address, bytes) of a DENSE array in GPU memory: a :class:`DeviceBuffer`, a torch GPU tensor or any object with
    ``__cuda_array_interface__``."""
    if isinstance(x, DeviceBuffer):
        if not x.is_contiguous():
            raise ValueError("%s must be dense" % what)
        return x.ptr, int(x.nbytes)
    if _is_device_tensor(x):
        if not x.is_contiguous():
            raise ValueError("%s must be a contiguous GPU tensor" % what)
        return int(x.data_ptr()), int(x.numel() * x.element_size())
    iface = getattr(x, '__cuda_array_interface__', None) if not hasattr(x, 'data_ptr') else None
    if not isinstance(iface, dict):
        raise ValueError("%s must live in GPU memory (DeviceBuffer, torch GPU tensor or __cuda_array_interface__)" % what)
    dt = numpy.dtype(iface['typestr'])
    shape = tuple(int(v) for v in iface['shape'])
    n = 1
    for v in shape:
        n *= v
    strides = iface.get('strides')
    if strides is not None:
        expect, acc = [], dt.itemsize
        for v in reversed(shape):
            expect.append(acc)
            acc *= v
        if n > 0 and tuple(int(v) for v in strides) != tuple(reversed(expect)):
            raise ValueError("%s must be dense (C-contiguous)" % what)
    return (int(iface['data'][0]) if n > 0 else 0), n * dt.itemsize


def _device_to_host(x):
    """A host copy (numpy) of a dense array in GPU memory, typed and shaped like it (no tensor library needed)."""
    if isinstance(x, DeviceBuffer):
        return x.to_host()
    if _is_device_tensor(x):
        return x.detach().cpu().numpy()
    iface = x.__cuda_array_interface__
    out = numpy.empty(tuple(int(v) for v in iface['shape']), dtype=numpy.dtype(iface['typestr']))
    cdef uintptr_t s = _device_memory(x)[0], d = out.ctypes.data
    cdef size_t n = out.nbytes
    cdef int rc
    if n:
        with nogil:
            rc = C.pgsd_device_copy(-1, <void*>d, <const void*>s, n)
        _raise_on_error(rc, "device to host copy")
    return out



def _device_empty(shape, dtype, device):
    """An uninitialised array in the memory of GPU ``device``: a torch tensor where torch is importable, a
    :class:`DeviceBuffer` (the library's own device memory) otherwise.  This and the helpers below are the one place
    where that choice is made: what they return is taken by every reader of GPU arrays here (`_device_memory`,
    `_rows2d`, `_device_to_host`), so a caller need not know which of the two it holds."""
    torch = _lib._torch
    if torch is None:
        return DeviceBuffer(shape, dtype, device)
    return torch.empty(shape, dtype=getattr(torch, numpy.dtype(dtype).name), device=torch.device('cuda', device))


def _device_rows(shape, dtype, device, row):
    """An array of ``shape`` in GPU memory whose rows (last axis) all equal the host array ``row``."""
    row = numpy.ascontiguousarray(row, dtype=dtype)
    if _lib._torch is None:
        return DeviceBuffer(shape, dtype, device, pattern=row)      # ONE row repeated by the allocation
    return _device_empty(shape, dtype, device).copy_(_lib._torch.from_numpy(row))


def _device_from_host(array, device):
    """A copy of a host array in GPU memory, typed and shaped like it."""
    a = numpy.ascontiguousarray(array)
    if _lib._torch is None:
        return DeviceBuffer((max(a.size, 1),), a.dtype, device, pattern=a if a.size else None).view(shape=a.shape)
    return _lib._torch.from_numpy(a).to(_lib._torch.device('cuda', device))


def _device_head(x, k):
    """The first ``k`` entries of a 1-D array in GPU memory, as a view."""
    return x.view(shape=(int(k),)) if isinstance(x, DeviceBuffer) else x[:int(k)]


def _device_head_rows(x, k):
    """The first ``k`` rows of a dense 2-D array in GPU memory, as a view."""
    return x.view(shape=(int(k),) + tuple(x.shape[1:])) if isinstance(x, DeviceBuffer) else x[:int(k)]


def _device_at(x, i):
    """``x[i]`` of a dense array in GPU memory, as a view."""
    if not isinstance(x, DeviceBuffer):
        return x[i]
    return x.view(shape=x.shape[1:], offset_bytes=i * (x.nbytes // x.shape[0]))


def _device_row_views(words, fields, n):
    """For every ``(first word, M, numpy dtype)`` of ``fields`` an ``(n,)`` / ``(n, M)`` view of the int32 GPU array
    ``words`` whose ``n`` rows are all the same ``M`` words (row stride 0): no n-row allocation, no copy."""
    torch = _lib._torch
    views, typed = [], {}
    for off, M, dt in fields:
        shape = (n, M) if M > 1 else (n,)
        if torch is None:
            # one strided view per field
            views.append(words.view(dtype=dt, shape=shape, strides=(0, dt.itemsize)[:len(shape)], offset_bytes=4 * off))
            continue
        base = typed.get(dt)
        if base is None:
            base = typed[dt] = words.view(getattr(torch, dt.name))  # one re-typed view of the words per element type
        views.append(base.as_strided(shape, (0, 1)[:len(shape)], off))
    return views


def _index_rows(rows):
    """(address, entries) of a dense array of 32-bit row indices in GPU memory."""
    es = rows.element_size() if hasattr(rows, 'element_size') else \
        numpy.dtype(rows.__cuda_array_interface__['typestr']).itemsize
    if es != 4:
        raise ValueError("rows must hold 32-bit row indices")
    ptr, nbytes = _device_memory(rows, "rows")
    return ptr, nbytes // 4


cdef uint32_t _no_rows = 0      # where an empty row list stands: it may have no address of its own, and nothing of it is read


def _row_list(who, rows, n):
    """(address, entries) of the first ``n`` entries (default: all) of a row list in GPU memory.  An empty list is still
    a list -- its result is that of no entry, not of every row -- and gets an address that is valid."""
    p_rows, n_rows = _index_rows(rows)
    count = n_rows if n is None else int(n)
    if count >= (1 << 32):
        raise ValueError("%s: a row list holds fewer than 2^32 entries" % who)
    if count < 0 or count > n_rows:
        raise ValueError("%s: rows holds fewer entries than n" % who)
    return (<uintptr_t>&_no_rows if count == 0 else p_rows), count


def _box_vectors(box):
    """:func:`pgsd.hoomd.box_vectors` of a float32 ``(Lx, Ly, Lz, xy, xz, yz)``, as the pair passes receive them."""
    from . import hoomd as _hoomd
    c_box = numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6]
    if c_box.shape[0] != 6:
        raise ValueError("box must hold 6 values")
    return numpy.ascontiguousarray(_hoomd.box_vectors(c_box), dtype=numpy.float64)


def _cell_counts(who, cells):
    """(the grid as a list, its uint32 array) of a pair pass's ``cells``."""
    grid = [int(v) for v in cells]
    if len(grid) != 3 or any(not 0 <= v < (1 << 32) for v in grid):
        raise ValueError("%s: cells holds three counts, each 1 to 1024" % who)
    return grid, numpy.array(grid, dtype=numpy.uint32)


def _sph_kernel(who, kernel):
    """The library's index of an SPH kernel's name."""
    from . import hoomd as _hoomd
    if kernel not in _hoomd.SPH_KERNELS:
        raise ValueError("%s: the kernel is one of %s: %r" % (who, ', '.join(_hoomd.SPH_KERNELS), kernel))
    return _hoomd.SPH_KERNELS.index(kernel)


def _sph_defaults(who, defaults, density):
    """(the mass and density that stand for a chunk stored nowhere as float64[2], whether there is a volume sum)."""
    c_defaults = numpy.ascontiguousarray(
        numpy.array([1.0, float('nan')] if defaults is None else defaults, dtype=numpy.float64).reshape(-1))
    if c_defaults.shape[0] != 2:
        raise ValueError("%s: defaults holds a mass and a density" % who)
    return c_defaults, density is not None or c_defaults[1] == c_defaults[1]


def _force_defaults(who, defaults):
    """The mass, density and pressure that stand for a chunk stored nowhere as float64[3]; ``None``: the schema's."""
    c_defaults = numpy.ascontiguousarray(
        numpy.array([1.0, 0.0, 0.0] if defaults is None else defaults, dtype=numpy.float64).reshape(-1))
    if c_defaults.shape[0] != 3:
        raise ValueError("%s: defaults holds a mass, a density and a pressure" % who)
    return c_defaults


def _force_terms(who, viscosity, gravity):
    """(``mu`` as a float or ``None``, the gravity as float64[3]) of :meth:`PGSDFile.sph_accelerations_device`, checked."""
    mu = None
    if viscosity is not None:
        mu = float(viscosity)
        if not 0.0 <= mu < float('inf'):
            raise ValueError("%s: viscosity is a finite number, at least 0, or None: %r" % (who, viscosity))
    c_gravity = numpy.ascontiguousarray(
        numpy.array([0.0, 0.0, 0.0] if gravity is None else gravity, dtype=numpy.float64).reshape(-1))
    if c_gravity.shape[0] != 3 or not numpy.isfinite(c_gravity).all():
        raise ValueError("%s: gravity holds three finite numbers, or is None" % who)
    return mu, c_gravity


def _sample_defaults(who, defaults):
    """The mass and the density that stand for a chunk stored nowhere as float64[2]; ``None``: the schema's."""
    c_defaults = numpy.ascontiguousarray(
        numpy.array([1.0, 0.0] if defaults is None else defaults, dtype=numpy.float64).reshape(-1))
    if c_defaults.shape[0] != 2:
        raise ValueError("%s: defaults holds a mass and a density" % who)
    return c_defaults


def _sample_values(who, values):
    """``values`` of :meth:`PGSDFile.sph_samples_device`, checked as far as it goes without the file: per value ``(chunk
    or None, columns or None, default)``; ``columns`` is ``None`` where the stored chunk's own width is meant."""
    values = tuple(values)
    if len(values) > 4:
        raise ValueError("%s: values holds at most 4 chunks: %d" % (who, len(values)))
    out, total = [], 0
    for k, v in enumerate(values):
        v = tuple(v) if isinstance(v, (tuple, list)) else ()
        if len(v) == 2 and isinstance(v[1], str):
            out.append((v, None, 0.0))
            continue
        if len(v) != 3 or (v[0] is not None and (not isinstance(v[0], (tuple, list)) or len(v[0]) != 2)):
            raise ValueError("%s: value %d is (frame, name) of a stored chunk or (chunk or None, columns, default)" % (who, k))
        try:
            columns, default = int(v[1]), float(v[2])
        except (TypeError, ValueError):
            raise ValueError("%s: value %d is (frame, name) of a stored chunk or (chunk or None, columns, default)" % (who, k))
        if not 1 <= columns <= 4:
            raise ValueError("%s: value %d has 1 to 4 columns: %r" % (who, k, v[1]))
        if v[0] is None and default != default:
            raise ValueError("%s: value %d is stored nowhere and its default is no number" % (who, k))
        total += columns
        out.append((None if v[0] is None else tuple(v[0]), columns, default))
    if total > 8:
        raise ValueError("%s: the values hold at most 8 columns together: %d" % (who, total))
    return out


def _sample_points(who, points):
    """``points`` of :meth:`PGSDFile.sph_samples_device`, checked: ``(host float64 K x 3 or None, the device array or None,
    K)``."""
    bad = "%s: points holds K x 3 float32 or float64 values (numpy) or K x 3 float64 values in GPU memory" % who
    if isinstance(points, numpy.ndarray) or isinstance(points, (list, tuple)):
        a = numpy.asarray(points)
        if a.dtype not in (numpy.float32, numpy.float64) or (a.size and (a.ndim != 2 or a.shape[1] != 3)):
            raise ValueError(bad)
        a = numpy.ascontiguousarray(a.astype(numpy.float64).reshape(-1, 3))
        if a.shape[0] >= (1 << 32):
            raise ValueError("%s: a call takes fewer than 2^32 points" % who)
        return a, None, a.shape[0]
    if not (isinstance(points, DeviceBuffer) or _is_device_tensor(points) or hasattr(points, '__cuda_array_interface__')):
        raise ValueError(bad)
    shape = tuple(int(v) for v in points.shape)
    if not str(points.dtype).endswith('float64') or len(shape) != 2 or shape[1] != 3:
        raise ValueError(bad)
    if shape[0] >= (1 << 32):
        raise ValueError("%s: a call takes fewer than 2^32 points" % who)
    return None, points, shape[0]


def _body_terms(who, viscosity, about):
    """(``mu`` as a float or ``None``, ``about`` as float64[3]) of :meth:`PGSDFile.sph_body_force_device`, checked."""
    mu = None
    if viscosity is not None:
        mu = float(viscosity)
        if not 0.0 <= mu < float('inf'):
            raise ValueError("%s: viscosity is a finite number, at least 0, or None: %r" % (who, viscosity))
    c_about = numpy.ascontiguousarray(
        numpy.array([0.0, 0.0, 0.0] if about is None else about, dtype=numpy.float64).reshape(-1))
    if c_about.shape[0] != 3 or not numpy.isfinite(c_about).all():
        raise ValueError("%s: about holds three finite numbers, or is None" % who)
    return mu, c_about


def _moments_defaults(who, defaults):
    """The row that stands for every row of a chunk stored nowhere -- mass, v[3], energy, x[3] -- as float64[8]."""
    c_defaults = numpy.ascontiguousarray(
        numpy.array([1, 0, 0, 0, 0, 0, 0, 0] if defaults is None else defaults, dtype=numpy.float64).reshape(-1))
    if c_defaults.shape[0] != 8:
        raise ValueError("%s: defaults holds mass, v[3], energy, x[3]" % who)
    return c_defaults


def _cell_ordered_lists(who, rows, cell, n):
    """(address of ``rows``, address of ``cell``, entries) of a row list in cell order and its ids, ``n`` entries each."""
    p_rows, count = _row_list(who, rows, n)
    return p_rows, _row_list(who, cell, count)[0], count


def _per_entry(count, shape_tail, dtype, device):
    """(array, address) of a per-entry output in the memory of GPU ``device``: ``count`` entries (room for one at least)
    of ``shape_tail``; ``(None, 0)`` where ``device`` is ``None``: the output is not wanted."""
    if device is None:
        return None, 0
    out = _device_empty((max(count, 1),) + tuple(shape_tail), dtype, device)
    return out, out.data_ptr()


cdef _raise_refused(who, int retval, fallback, extra, int err):
    """A reduction's return code -> exception: a refusal is a ValueError that carries the library's message."""
    if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
        msg = C.pgsd_last_error_string()
        raise ValueError("%s: %s" % (who, msg.decode('utf-8', 'replace') if msg != NULL else fallback))
    _raise_on_error(retval, extra, err)


def _rows2d(x, what):
    """(address, numpy dtype, rows, width, row stride in elements) of a 1-D or row-major 2-D array in GPU memory, rows
    possibly strided: a torch GPU tensor, a :class:`DeviceBuffer` or any object with ``__cuda_array_interface__``
    (version 2 or 3)."""
    if _is_device_tensor(x):
        t2 = x.unsqueeze(1) if x.dim() == 1 else x
        if t2.dim() != 2 or (t2.shape[1] > 1 and t2.stride(1) != 1):
            raise ValueError("%s must be 1-D or row-major 2-D" % what)
        rows, width = int(t2.shape[0]), int(t2.shape[1])
        return t2.data_ptr(), _PGSD_TO_NP[_pgsd_type(t2.dtype)], rows, width, int(t2.stride(0)) if rows > 1 else width
    iface = getattr(x, '__cuda_array_interface__', None) if not hasattr(x, 'data_ptr') or isinstance(x, DeviceBuffer) else None
    if not isinstance(iface, dict) or 'data' not in iface or 'shape' not in iface or 'typestr' not in iface:
        raise ValueError("%s must live in GPU memory (torch GPU tensor, DeviceBuffer or __cuda_array_interface__)" % what)
    dt = numpy.dtype(iface['typestr'])
    if dt.byteorder == '>':
        raise ValueError("big-endian device arrays are not supported")
    shape = tuple(int(v) for v in iface['shape'])
    if len(shape) == 1:
        shape = (shape[0], 1)
    if len(shape) != 2:
        raise ValueError("%s must be 1-D or row-major 2-D" % what)
    rows, width = shape
    st = iface.get('strides')
    if st is None:
        stride = width
    else:
        if (width > 1 and int(st[1]) != dt.itemsize) or int(st[0]) % dt.itemsize != 0:
            raise ValueError("%s must be 1-D or row-major 2-D with element-aligned rows" % what)
        stride = int(st[0]) // dt.itemsize if rows > 1 else width
    return (int(iface['data'][0]) if rows * width > 0 else 0), dt, rows, width, stride


def select_rows(flags):
    """Stream compaction on the GPU for filtered snapshots.

    Args:
        flags: uint8 / bool array of length N in GPU memory (torch GPU tensor, :class:`DeviceBuffer` or any
            ``__cuda_array_interface__`` object of one-byte elements); non-zero = keep the particle.

    Returns:
        ``(index, count)``: ``index`` holds the kept rows in ascending order as 32-bit integers (usable as
        ``order=`` of :meth:`DeviceField.from_tensor` / :meth:`DeviceField.from_device_array`) -- an int32 GPU tensor
        of ``count`` entries when ``flags`` is a torch tensor, a :class:`DeviceBuffer` view otherwise; ``count``
        (int) is this rank's number of rows, i.e. what goes into the row-count allgather
        (``pgsd.dist.partition_rows``) that fixes every rank's file offsets.

    Wave-level ballot/popcount scans produce per-workgroup counts, one workgroup scans them
    into offsets, a scatter pass writes the indices (pgsd_select_rows in the C ABI; the scratch space is the
    library's).
    """
    cdef uintptr_t stream = 0, p_flags, p_index
    cdef uint64_t n, k = 0
    cdef int retval
    if _is_device_tensor(flags):
        torch = _lib._torch
        f8 = flags.contiguous().view(torch.uint8) if flags.dtype in (torch.bool, torch.uint8, torch.int8) \
            else (flags != 0).to(torch.uint8)
        n = int(f8.numel())
        index = torch.empty((max(n, 1),), dtype=torch.int32, device=f8.device)
        stream = torch.cuda.current_stream(f8.device).cuda_stream
        p_flags, p_index = f8.data_ptr(), index.data_ptr()
        keep = (f8, index)
    else:
        ptr, nbytes = _device_memory(flags, "flags")
        iface = flags.__cuda_array_interface__
        if numpy.dtype(iface['typestr']).itemsize != 1:
            raise ValueError("flags must have one-byte elements")
        n = nbytes
        index = DeviceBuffer((max(n, 1),), numpy.int32, getattr(flags, 'device', -1) if isinstance(flags, DeviceBuffer) else -1)
        p_flags, p_index = ptr, index.ptr
        keep = (flags, index)
    with nogil:
        retval = C.pgsd_select_rows(<const uint8_t*>p_flags, n, <uint32_t*>p_index, &k, <void*>stream)
    _raise_on_error(retval, "select_rows")
    return _device_head(index, k), int(k)


RowPlanModel = collections.namedtuple('RowPlanModel', ['blocks', 'runs', 'rows2', 'staged_rows'])

# A plan takes the sparse route while its touched fraction T * R / N is at most this (PGSD_PLAN_SPARSE_MAX, read once).
# Measured (profiles/r07_read_tracks_bench.jsonl, sweep_f): the sparse route is ahead of the whole-chunk route up to a
# touched fraction of 0.9 and level with it, inside the repeats' spread, at 1.0.
_PLAN_SPARSE_MAX = float(os.environ.get('PGSD_PLAN_SPARSE_MAX', '0.9'))


def row_plan_model(rows, N, block_rows):
    """The numpy model of a row plan (:meth:`PGSDFile.plan_rows` computes exactly this on the GPU).

    A chunk's ``N`` rows are cut into blocks of ``block_rows`` rows.  Returns a ``RowPlanModel``:

    * ``blocks``: the ascending blocks that hold at least one entry of ``rows`` (uint32); block ``blocks[s]`` has slot
      ``s`` in the compact staging, which is the touched blocks in file order;
    * ``runs``: ``(n_runs, 2)`` uint32 rows ``(first block, number of blocks)`` of adjacent touched blocks -- the
      pieces of the file a sparse read fetches;
    * ``rows2``: ``slot(rows[k] // R) * R + rows[k] % R`` (uint32), the index of row ``rows[k]`` in that staging;
    * ``staged_rows``: the staging's height, ``T * R`` less what a touched short last block lacks.

    ``rows`` need not be ascending and may repeat; an entry ``>= N`` touches nothing and becomes ``0xFFFFFFFF``.
    """
    R, N = int(block_rows), int(N)
    if R < 1 or N < 0 or N + R >= 1 << 32:
        raise ValueError("row_plan_model: block_rows >= 1 and N + block_rows < 2^32")
    rows = numpy.ascontiguousarray(rows).reshape(-1).astype(numpy.int64, copy=False)
    if rows.size and rows.min() < 0:
        rows = rows & 0xFFFFFFFF            # int32 bit patterns of uint32 entries
    ok = rows < N
    b = rows[ok] // R
    blocks = numpy.unique(b)
    rows2 = numpy.full(rows.shape, 0xFFFFFFFF, dtype=numpy.uint32)
    rows2[ok] = (numpy.searchsorted(blocks, b) * R + rows[ok] % R).astype(numpy.uint32)
    if blocks.size:
        starts = numpy.flatnonzero(numpy.concatenate(([True], numpy.diff(blocks) != 1)))
        counts = numpy.diff(numpy.concatenate((starts, [blocks.size])))
        runs = numpy.stack((blocks[starts], counts), axis=1).astype(numpy.uint32)
    else:
        runs = numpy.zeros((0, 2), dtype=numpy.uint32)
    nb = (N + R - 1) // R
    staged = int(blocks.size) * R
    if blocks.size and int(blocks[-1]) == nb - 1:
        staged -= nb * R - N
    return RowPlanModel(blocks.astype(numpy.uint32), runs, rows2, staged)


cdef class RowPlan:
    """A plan for sparse indexed reads (:meth:`PGSDFile.plan_rows`): which blocks of ``block_rows`` rows the entries of
    ``rows`` touch, merged into runs, and ``rows2``, the entries' positions in a compact staging of those blocks.  One
    plan serves every chunk of ``N`` rows of the file it was made on, in every frame.  Pass it as
    ``read_chunk_device(..., rows=plan)``.

    Attributes:
        n (int): entries.  N (int): rows of the chunks the plan is for.  block_rows (int): R.
        touched_blocks (int): T.  runs (int): number of runs of adjacent touched blocks.
        rows: the caller's index list (kept alive).  rows2 (`DeviceBuffer`): uint32, ``n`` entries.
        threshold (float): the plan takes the sparse route while ``touched_fraction <= threshold``.
    """
    cdef C.pgsd_row_plan* _plan
    cdef public object rows, rows2, file
    cdef public double threshold

    def __cinit__(self):
        self._plan = NULL

    def __dealloc__(self):
        if self._plan != NULL:
            C.pgsd_row_plan_destroy(self._plan)
            self._plan = NULL

    cdef uint64_t _count(self, int i):
        cdef uint64_t counts[6]
        cdef const uint32_t* lists[5]
        memset(counts, 0, sizeof(counts))
        C.pgsd_row_plan_query(self._plan, counts, lists)
        return counts[i]

    @property
    def n(self):
        return int(self._count(0))

    @property
    def N(self):
        return int(self._count(1))

    @property
    def block_rows(self):
        return int(self._count(2))

    @property
    def touched_blocks(self):
        return int(self._count(3))

    @property
    def runs(self):
        return int(self._count(4))

    @property
    def staged_rows(self):
        return int(self._count(5))

    @property
    def touched_fraction(self):
        """``T * R / N`` (at most 1; 0 for an empty chunk): the share of a chunk the sparse route reads."""
        N = self.N
        return min(1.0, float(self.touched_blocks * self.block_rows) / float(N)) if N else 0.0

    @property
    def sparse(self):
        """Whether a read through this plan takes the sparse route."""
        return self.touched_fraction <= self.threshold

    def blocks(self):
        """The touched blocks (host, uint32, ascending)."""
        cdef uint64_t counts[6]
        cdef const uint32_t* lists[5]
        C.pgsd_row_plan_query(self._plan, counts, lists)
        out = numpy.empty((int(counts[3]),), dtype=numpy.uint32)
        cdef uint32_t[::1] v = out
        cdef uint64_t i
        for i in range(counts[3]):
            v[i] = lists[2][i]
        return out

    def run_list(self):
        """``(runs, 2)`` uint32: first block and number of blocks of every run."""
        cdef uint64_t counts[6]
        cdef const uint32_t* lists[5]
        C.pgsd_row_plan_query(self._plan, counts, lists)
        out = numpy.empty((int(counts[4]), 2), dtype=numpy.uint32)
        cdef uint32_t[:, ::1] v = out
        cdef uint64_t i
        for i in range(counts[4]):
            v[i, 0] = lists[3][i]
            v[i, 1] = lists[4][i]
        return out


def open(name, mode, application=None, schema=None, schema_version=None, comm=None):
    """Open a PGSD file and return a :py:class:`PGSDFile` (fl.pyx:149-228).

    Valid modes: ``'r'``, ``'r+'``, ``'w'``, ``'x'``, ``'a'``.  When creating a file
    (``'w'``, ``'x'``, ``'a'`` on a missing file) ``application``, ``schema`` and
    ``schema_version`` are required.

    ``comm`` (not in the reference, whose communicator is always ``MPI_COMM_WORLD``): a communicator made by
    ``pgsd.dist.create_shm`` / ``create_rccl`` that is NOT the process default -- several ranks in one process
    (one thread per GPU), each with a file object of its own.  It must outlive the file object.
    """
    return PGSDFile(str(name), mode, application, schema, schema_version, comm)


cdef class PGSDFile:
    """PGSD file access interface (fl.pyx:231-1052)."""
    cdef C.pgsd_handle _handle          # embedded, by value (fl.pyx:284)
    cdef bint _is_open
    cdef object _mode, _name, _comm
    cdef list _keepalive, _async_keep
    cdef bint _explicit_stream, _deferred_rows, _local_reads, _frame_exchange_on
    cdef object _source_stream

    def __init__(self, name, mode, application, schema, schema_version, comm=None):
        cdef C.pgsd_open_flag c_flags
        cdef int exclusive_create = 0
        cdef int overwrite = 0
        cdef int retval, err
        self._is_open = False
        self._comm = comm
        self._mode = mode
        # mode -> flags, fl.pyx:301-317
        if mode == 'w':
            c_flags = C.PGSD_OPEN_READWRITE
            overwrite = 1
        elif mode == 'r':
            c_flags = C.PGSD_OPEN_READONLY
        elif mode == 'r+':
            c_flags = C.PGSD_OPEN_READWRITE
        elif mode == 'x':
            c_flags = C.PGSD_OPEN_READWRITE
            overwrite = 1
            exclusive_create = 1
        elif mode == 'a':
            c_flags = C.PGSD_OPEN_READWRITE
            if not os.path.exists(name):
                overwrite = 1
        else:
            raise ValueError("Invalid mode: " + mode)

        # One process per rank under torchrun: make sure the library knows about the other ranks
        # (a rank that believes it is alone would overwrite its neighbours' rows).
        if comm is None and C.pgsd_comm_size() == 1 and _lib._torch is not None:
            tdist = _lib._torch.distributed
            if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
                from . import dist as _dist
                _dist.init_from_torch()

        self._name = name
        self._keepalive = []
        self._explicit_stream = False
        self._frame_exchange_on = False
        self._source_stream = -1       # what the pipeline was last told (-1: nothing yet)
        self._deferred_rows = False
        self._local_reads = False
        self._async_keep = []
        memset(&self._handle, 0, sizeof(self._handle))

        cdef const C.pgsd_comm* c_comm = NULL
        if comm is not None:
            c_comm = <const C.pgsd_comm*><uintptr_t>ctypes.addressof(comm)
        name_b = name.encode('utf-8')
        cdef const char* c_name = name_b
        cdef const char* c_app
        cdef const char* c_schema
        cdef uint32_t c_version
        if overwrite:
            if application is None:
                raise ValueError("Provide application when creating a file")
            if schema is None:
                raise ValueError("Provide schema when creating a file")
            if schema_version is None:
                raise ValueError("Provide schema_version when creating a file")
            logger.info('overwriting file: ' + name + ' with mode: ' + mode
                        + ', application: ' + application + ', schema: ' + schema
                        + ', and schema_version: ' + str(schema_version))
            app_b, schema_b = application.encode('utf-8'), schema.encode('utf-8')
            c_app, c_schema = app_b, schema_b
            c_version = C.pgsd_make_version(schema_version[0], schema_version[1])
            with nogil:
                if c_comm == NULL:
                    retval = C.pgsd_create_and_open(&self._handle, c_name, c_app, c_schema, c_version, c_flags,
                                                    exclusive_create)
                else:
                    retval = C.pgsd_create_and_open_on(c_comm, &self._handle, c_name, c_app, c_schema, c_version,
                                                       c_flags, exclusive_create)
                err = errno
        else:
            logger.info('opening file: ' + name + ' with mode: ' + mode)
            with nogil:
                if c_comm == NULL:
                    retval = C.pgsd_open(&self._handle, c_name, c_flags)
                else:
                    retval = C.pgsd_open_on(c_comm, &self._handle, c_name, c_flags)
                err = errno
        _raise_on_error(retval, name, err)
        self._is_open = True

        # validate schema, fl.pyx:371-378
        if schema is not None:
            schema_truncated = schema
            if len(schema_truncated) > 64:
                schema_truncated = schema_truncated[0:63]
            if self.schema != schema_truncated:
                raise RuntimeError('file ' + name + ' has incorrect schema: ' + self.schema)

    # ------------------------------------------------------------------ helpers
    def _h(self):
        """ctypes pointer to the embedded handle: for tests and tools that call the C ABI directly."""
        return ctypes.cast(<uintptr_t>&self._handle, _lib.HP)

    def _async_frames_kept(self):
        """Number of asynchronously sealed frames whose source arrays are still held (tests)."""
        return len(self._async_keep)

    cdef int _check_open(self) except -1:
        if not self._is_open:
            raise ValueError("File is not open")
        return 0

    # ------------------------------------------------------------------ lifecycle
    def close(self, write_all=True):
        """Close the file (fl.pyx:382-419). May be called more than once."""
        cdef int retval, err
        if self._is_open:
            logger.info('closing file: ' + self._name)
            with nogil:
                retval = C.pgsd_close(&self._handle)
                err = errno
            self._is_open = False
            self._keepalive = []
            self._async_keep = []
            _raise_on_error(retval, self._name, err)

    def end_frame(self, write_all=True, wait=True):
        """Complete the current frame (fl.pyx:460-506).

        With ``wait=True`` (default, the reference's behaviour) the frame is in the file on
        return.  ``wait=False`` seals the frame but lets its device chunks finish in the
        background (``pgsd_end_frame_async``): call :meth:`wait_packed` before overwriting the
        source arrays and :meth:`frame_sync` (or any later synchronous call) before relying on the
        file contents.
        """
        cdef int retval, err, prc = 0
        self._check_open()
        if wait:
            with nogil:
                retval = C.pgsd_end_frame(&self._handle)
                err = errno
            # a synchronous seal drains the pipeline: nothing sealed earlier still reads its sources
            self._keepalive = []
            self._async_keep = []
        else:
            with nogil:
                retval = C.pgsd_end_frame_async(&self._handle)
                err = errno
            self._async_keep.append(self._keepalive)
            self._keepalive = []
            # The pack kernels read the source arrays, the copies and writes read the staging arena: once
            # a frame's kernels are done its sources may go.  Only the newest frames can still be packing;
            # keep two, sync-free, so a long run of append(wait=False) does not pin every frame's tensors.
            if len(self._async_keep) > 2:
                with nogil:
                    prc = C.pgsd_device_wait_packed(&self._handle)
                _raise_on_error(prc, self._name)
                self._async_keep = self._async_keep[-1:]
        _raise_on_error(retval, self._name, err)

    def frame_sync(self):
        """Wait until every asynchronously sealed frame of this rank is in the file."""
        cdef int retval, err
        self._check_open()
        with nogil:
            retval = C.pgsd_frame_sync(&self._handle)
            err = errno
        self._async_keep = []
        _raise_on_error(retval, self._name, err)

    def flush(self, write_all=True):
        """Flush all buffered frames to the file (fl.pyx:508-524)."""
        cdef int retval, err
        self._check_open()
        with nogil:
            retval = C.pgsd_flush(&self._handle)
            err = errno
        self._async_keep = []
        _raise_on_error(retval, self._name, err)

    @property
    def frame_exchange(self):
        """bool: batch the exchange between the ranks per frame (``pgsd_set_frame_exchange``).

        Off (default): every chunk write exchanges the ranks' sizes at once, like the reference's per-chunk
        collectives.  On: replicated small chunks and all device chunks are queued and ONE allgather at
        :meth:`end_frame` carries their sizes and the ranks' status -- a frame of small chunks, fused device
        chunks (``offset='auto'``) and ``end_frame`` costs one collective.  The file is byte-identical
        either way."""
        self._check_open()
        return bool(self._frame_exchange_on)

    @frame_exchange.setter
    def frame_exchange(self, on):
        cdef int retval, err, flag = 1 if on else 0
        self._check_open()
        with nogil:
            retval = C.pgsd_set_frame_exchange(&self._handle, flag)
            err = errno
        _raise_on_error(retval, self._name, err)
        self._frame_exchange_on = flag != 0

    @property
    def deferred_rows(self):
        """bool: with :attr:`frame_exchange` on, host arrays written with ``write_all=True`` wait for the frame's
        exchange like every other chunk instead of forcing one at once (``pgsd_set_deferred_rows``): the file object
        keeps the arrays alive until then, and the CALLER must not change them before :meth:`end_frame` /
        :meth:`flush` / :meth:`exchange_now` (the rule device tensors follow anyway).  A frame then costs one
        exchange whatever it holds."""
        return bool(self._deferred_rows)

    @deferred_rows.setter
    def deferred_rows(self, on):
        cdef int retval, err, flag = 1 if on else 0
        self._check_open()
        with nogil:
            retval = C.pgsd_set_deferred_rows(&self._handle, flag)
            err = errno
        _raise_on_error(retval, self._name, err)
        self._deferred_rows = bool(on)

    @property
    def local_reads(self):
        """bool: reads on a writable file take no part in a collective flush (``pgsd_set_local_reads``): for rows the
        caller knows to be in the file -- this rank's own rows of a sealed frame, or a file opened after they were
        written.  Default False: a read flushes first, collectively, like the reference's (pgsd.c:2436-2537).

        With several ranks the LOOKUP in front of a read (:meth:`chunk_exists`, :meth:`read_chunk`,
        :meth:`find_matching_chunk_names`) is local too while this is on: it sees what the last collective flush
        committed.  A frame that held buffered small chunks only is not flushed by :meth:`end_frame`
        (pgsd.c:1941-1950), so its chunks are reported missing until the next :meth:`flush`; the library then leaves
        a note in ``pgsd_last_error_string()``.  On ONE rank the flush concerns nobody else and runs as ever."""
        return bool(self._local_reads)

    @local_reads.setter
    def local_reads(self, on):
        cdef int retval, err, flag = 1 if on else 0
        self._check_open()
        with nogil:
            retval = C.pgsd_set_local_reads(&self._handle, flag)
            err = errno
        _raise_on_error(retval, self._name, err)
        self._local_reads = bool(on)

    def set_partition(self, rows):
        """Declare every rank's row count (``pgsd_set_partition``): while declared, chunk writes exchange nothing --
        chunks written with ``offset='auto'`` are partitioned by ``rows`` (this rank must bring ``rows[rank]``),
        every other chunk must have the same size on every rank -- and a frame costs no collective at all.
        ``None`` clears the declaration.  Every rank must declare the same vector."""
        cdef int retval, err
        cdef uint32_t n = 0
        cdef const uint64_t[::1] view
        cdef const uint64_t* ptr = NULL
        self._check_open()
        if rows is not None:
            arr = numpy.ascontiguousarray(rows, dtype=numpy.uint64)
            if arr.ndim != 1 or arr.shape[0] != self._handle.nprocs:
                raise ValueError("the partition must have one row count per rank")
            view = arr
            ptr = &view[0]
            n = arr.shape[0]
        with nogil:
            retval = C.pgsd_set_partition(&self._handle, ptr, n)
            err = errno
        _raise_on_error(retval, self._name, err)

    def exchange_now(self):
        """Perform the pending frame exchange now (collective; nothing is flushed)."""
        cdef int retval, err
        self._check_open()
        with nogil:
            retval = C.pgsd_frame_exchange(&self._handle)
            err = errno
        _raise_on_error(retval, self._name, err)

    @property
    def collective_count(self):
        """int: allgathers / barriers this handle has issued on its communicator."""
        cdef C.pgsd_exchange_stats st
        self._check_open()
        _raise_on_error(C.pgsd_get_exchange_stats(&self._handle, &st, 0), self._name)
        return int(st.collectives)

    def exchange_stats(self, reset=False):
        """dict ``count``, ``total_us``, ``max_us``, ``min_us``: the allgathers this handle issued and their wall
        time on this rank (transport latency + the wait for the slowest rank)."""
        cdef C.pgsd_exchange_stats st
        self._check_open()
        _raise_on_error(C.pgsd_get_exchange_stats(&self._handle, &st, 1 if reset else 0), self._name)
        return {"count": int(st.count), "total_us": float(st.total_us), "max_us": float(st.max_us),
                "min_us": float(st.min_us)}

    # ------------------------------------------------------------------ writing
    def write_chunk(self, name, data, offset=None, rank=0, write_all=True):
        """Write a data chunk to the current frame (fl.pyx:526-654).

        Args:
            name (str): chunk name.
            data: numpy array / array-like with <= 2 dimensions (host path, as in the
                reference), or a torch GPU tensor / :class:`DeviceField` (device path).
            offset: ``None`` or the integer array of every rank's row count; with ``rank`` it
                gives ``N_global = offset.sum()`` and this rank's first row
                ``offset[:rank].sum()`` (fl.pyx:594-598).  ``'auto'``: rows partitioned in rank order,
                counts taken from the library's own size exchange.
            rank (int): this rank.
            write_all (bool): ``True``: every rank writes its rows of a per-particle chunk;
                ``False``: replicated small chunk.
        """
        self._check_open()
        if isinstance(data, DeviceField) or _is_device_array(data):
            return self._write_chunk_device(name, data, offset, rank, write_all)

        data_array = numpy.ascontiguousarray(data)
        if data_array is not data:
            logger.warning('implicit data copy when writing chunk: ' + name)
        if data_array.ndim > 2:
            raise ValueError("PGSD can only write 1 or 2 dimensional arrays: " + name)
        cdef uint64_t N, N_global, stride
        cdef uint32_t M
        if data_array.ndim == 1:
            N, M = data_array.shape[0], 1
        elif data_array.ndim == 2:
            N, M = data_array.shape[0], data_array.shape[1]
        else:
            data_array = data_array.reshape([1, 1])
            N, M = 1, 1
        py_ng, py_stride = self._partition_args(offset, rank, N, M)
        N_global, stride = py_ng, py_stride
        cdef C.pgsd_type pgsd_type = <C.pgsd_type><int>_pgsd_type(data_array.dtype, name)
        cdef Py_buffer view
        cdef const void* ptr = NULL
        cdef bint have_view = False
        if data_array.size:
            PyObject_GetBuffer(data_array, &view, PyBUF_ANY_CONTIGUOUS)
            ptr = view.buf
            have_view = True
        if self._deferred_rows and write_all:
            self._keepalive.append(data_array)     # the rows are read at the frame's exchange, not now
        name_b = name.encode('utf-8')
        cdef const char* c_name = name_b
        cdef bint c_all = bool(write_all)
        cdef uint64_t global_size = N_global * M     # wraps like the C expression
        cdef int retval, err
        with nogil:
            retval = C.pgsd_write_chunk(&self._handle, c_name, pgsd_type, N, M, N_global, M, stride, global_size,
                                        c_all, 0, ptr)
            err = errno
        if have_view:
            PyBuffer_Release(&view)
        _raise_on_error(retval, self._name, err)

    @staticmethod
    def _partition_args(offset, rank, N, M):
        """``offset`` of :meth:`write_chunk` -> (N_global, element offset of this rank), fl.pyx:594-598.
        ``'auto'``: the library derives both from its own size exchange (PGSD_PARTITION_AUTO)."""
        if isinstance(offset, str):
            if offset != 'auto':
                raise ValueError("offset must be None, 'auto' or the array of every rank's row count")
            return _lib.PARTITION_AUTO, 0
        if offset is None:
            return N, 0
        offset = numpy.asarray(offset)
        return int(offset.sum()), M * int(offset[0:rank].sum())

    cdef _sync_source_stream(self):
        """Tell the pipeline which stream produced the arrays: PyTorch's current stream.  (The raw-handle
        query and the remembered last value keep this at ~1 us per call: `torch.cuda.current_stream()` builds
        a Stream object, 10-15 us, once per device write of a small frame.)"""
        global _TORCH_HAS_GPU
        torch = _lib._torch
        if torch is None:
            return
        if _TORCH_HAS_GPU is None:
            _TORCH_HAS_GPU = bool(torch.cuda.is_available())
        if not _TORCH_HAS_GPU:
            return                      # the device call itself reports the missing GPU
        try:
            stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
        except AttributeError:  # pragma: no cover - other torch versions
            stream = torch.cuda.current_stream().cuda_stream
        cdef uintptr_t s
        if stream != self._source_stream:
            s = stream
            _raise_on_error(C.pgsd_device_set_source_stream(&self._handle, <void*>s), self._name)
            self._source_stream = stream

    def set_source_stream(self, stream):
        """Name the HIP stream (integer handle) on which the particle arrays are produced;
        device writes are ordered after the work already enqueued there."""
        self._check_open()
        cdef uintptr_t s = int(stream) if stream else 0
        _raise_on_error(C.pgsd_device_set_source_stream(&self._handle, <void*>s), self._name)
        self._explicit_stream = True
        self._source_stream = stream

    def _write_chunk_device(self, name, data, offset, rank, write_all):
        if not self._explicit_stream:
            self._sync_source_stream()
        cdef DeviceField f = data if isinstance(data, DeviceField) else DeviceField.from_device_array(data)
        cdef uint64_t N = f.N, N_global, stride
        cdef uint32_t M = f.M
        py_ng, py_stride = self._partition_args(offset, rank, N, M)
        N_global, stride = py_ng, py_stride
        cdef C.pgsd_field_desc desc
        f.fill_desc(&desc)
        cdef C.pgsd_type t = <C.pgsd_type><int>f.out_type(name)
        self._keepalive.append(f)
        name_b = name.encode('utf-8')
        cdef const char* c_name = name_b
        cdef bint c_all = bool(write_all)
        cdef uint64_t global_size = N_global * M
        cdef int retval, err
        with nogil:
            retval = C.pgsd_write_chunk_device(&self._handle, c_name, t, N, M, N_global, M, stride, global_size, c_all, 0,
                                               &desc)
            err = errno
        _raise_on_error(retval, self._name, err)

    def write_chunks(self, fields, offset=None, rank=0):
        """Write several per-particle chunks of the same N with ONE fused pack launch.

        Args:
            fields: list of ``(name, data)`` with ``data`` a torch GPU tensor or a
                :class:`DeviceField`; all must have the same number of rows.
            offset, rank: as in :meth:`write_chunk` (``write_all`` is implied); ``offset='auto'`` lets the
                library derive the partition from its own size exchange, so no row-count allgather of the
                caller is needed.
        """
        self._check_open()
        if not self._explicit_stream:
            self._sync_source_stream()
        cdef Py_ssize_t n = len(fields), i
        if n == 0:
            return
        cdef C.pgsd_chunk_req* reqs = <C.pgsd_chunk_req*>calloc(n, sizeof(C.pgsd_chunk_req))
        if reqs == NULL:
            raise MemoryError()
        cdef DeviceField f
        cdef uint64_t N = 0, N_global, row0
        cdef int retval, err
        names = []
        try:
            for i in range(n):
                name, data = fields[i]
                f = data if isinstance(data, DeviceField) else DeviceField.from_device_array(data)
                if i == 0:
                    N = f.N
                elif <uint64_t>f.N != N:
                    raise ValueError("all fields of a fused write must have the same number of rows")
                name_b = name.encode('utf-8')
                names.append(name_b)
                reqs[i].name = name_b
                reqs[i].type = f.out_type(name)
                reqs[i].M = <uint32_t>f.M
                f.fill_desc(&reqs[i].src)
                self._keepalive.append(f)
            py_ng, py_row0 = self._partition_args(offset, rank, N, 1)
            N_global, row0 = py_ng, py_row0
            with nogil:
                retval = C.pgsd_write_chunks_device(&self._handle, <uint32_t>n, reqs, N, N_global, row0)
                err = errno
        finally:
            free(reqs)
        _raise_on_error(retval, self._name, err)

    def stage_chunks(self, fields):
        """Launch the fused pack of ``fields`` (as in :meth:`write_chunks`) NOW and return a ticket; the chunks get
        their place in the frame later, with :meth:`write_staged` (``pgsd_stage_chunks_device``).  The kernel -- and
        for small frames the PCIe crossing -- then runs under whatever the caller does in between."""
        self._check_open()
        if not self._explicit_stream:
            self._sync_source_stream()
        cdef Py_ssize_t n = len(fields), i
        if n == 0:
            raise ValueError("no fields to stage")
        cdef C.pgsd_chunk_req* reqs = <C.pgsd_chunk_req*>calloc(n, sizeof(C.pgsd_chunk_req))
        if reqs == NULL:
            raise MemoryError()
        cdef DeviceField f
        cdef uint64_t N = 0, ticket = 0
        cdef int retval, err
        names = []
        sizes = []
        try:
            for i in range(n):
                name, data = fields[i]
                f = data if isinstance(data, DeviceField) else DeviceField.from_device_array(data)
                if i == 0:
                    N = f.N
                elif <uint64_t>f.N != N:
                    raise ValueError("all fields of a fused write must have the same number of rows")
                name_b = name.encode('utf-8')
                names.append(name_b)
                reqs[i].name = name_b
                reqs[i].type = f.out_type(name)
                reqs[i].M = <uint32_t>f.M
                f.fill_desc(&reqs[i].src)
                self._keepalive.append(f)
                sizes.append(int(f.N) * int(f.M) * f.out_dtype.itemsize)
            with nogil:
                retval = C.pgsd_stage_chunks_device(&self._handle, <uint32_t>n, reqs, N, &ticket)
                err = errno
        finally:
            free(reqs)
        _raise_on_error(retval, self._name, err)
        # (ticket, rows, packed bytes of every chunk, the GPU the pipeline -- and with it the staging -- lives on: the
        # handle's own answer, whatever kind of array the sources are and whatever a tensor library's "current device" is)
        return (int(ticket), int(N), tuple(sizes), self.pipeline_device())

    def pipeline_device(self):
        """int: the HIP device this file's pipeline runs on (created on the device given to :meth:`configure_device`,
        else on the device that is current at the first device call)."""
        cdef int dev
        self._check_open()
        with nogil:
            dev = C.pgsd_device_of(&self._handle)
        if dev < 0:
            _raise_on_error(dev, self._name)
        return dev

    def write_staged(self, ticket, first, count, offset=None, rank=0):
        """Write chunks ``[first, first + count)`` of a :meth:`stage_chunks` ticket at this point of the frame
        (``offset`` / ``rank`` as in :meth:`write_chunks`)."""
        self._check_open()
        cdef uint64_t c_ticket = ticket[0], N = ticket[1], N_global, row0
        cdef uint32_t c_first = first, c_count = count
        py_ng, py_row0 = self._partition_args(offset, rank, N, 1)
        N_global, row0 = py_ng, py_row0
        cdef int retval, err
        with nogil:
            retval = C.pgsd_write_staged_chunks(&self._handle, c_ticket, c_first, c_count, N_global, row0)
            err = errno
        _raise_on_error(retval, self._name, err)

    def compare_staged(self, ticket, first, refs):
        """Do the packed rows of staged chunks ``first, first + 1, ...`` of a :meth:`stage_chunks` ticket equal
        ``refs[i]`` -- dense arrays in GPU memory (:class:`DeviceBuffer`, torch GPU tensors, ``__cuda_array_interface__``
        objects) holding the same rows of another frame as the chunk stores them (:meth:`read_chunk_device`,
        :meth:`copy_staged`), or ``None`` (not compared: ``False``)?  A reference SHORTER
        than the chunk repeats (rows of a default value: at least 4096 bytes, a multiple of 16 bytes and of whole
        rows).  One kernel behind the pack, one stream wait (``pgsd_compare_staged_chunks``).  Equality is
        ``numpy.array_equal``'s: integer chunks by their bytes, float chunks by value (a NaN equals nothing, +0.0 equals
        -0.0).  Returns a list of bool."""
        self._check_open()
        if not self._explicit_stream:
            self._sync_source_stream()      # the comparison is ordered behind this stream's writes to the references
        cdef Py_ssize_t n = len(refs), i
        if n == 0:
            return []
        cdef uint64_t c_ticket = ticket[0], rows = ticket[1]
        cdef uint32_t c_first = first, c_count = n
        cdef const void** ptrs = <const void**>calloc(n, sizeof(void*))
        cdef uint64_t* sizes = <uint64_t*>calloc(n, sizeof(uint64_t))
        cdef uint8_t* eq = <uint8_t*>calloc(n, 1)
        cdef uintptr_t p
        cdef int retval, err
        if ptrs == NULL or eq == NULL or sizes == NULL:
            free(ptrs)
            free(sizes)
            free(eq)
            raise MemoryError()
        try:
            for i in range(n):
                r = refs[i]
                if r is None:
                    continue
                addr, have = _device_memory(r, "a reference")
                if first + i >= len(ticket[2]):
                    raise ValueError("the ticket has no chunk %d" % (first + i))
                if have > ticket[2][first + i]:
                    # the kernel reads as many bytes of the reference as the packed chunk has: never fewer at hand
                    # (a shorter one repeats; the library checks its shape)
                    raise ValueError("reference %d holds more than the %d bytes of the packed chunk" % (i, ticket[2][first + i]))
                sizes[i] = have
                p = addr
                # an empty tensor has no address: any non-null one says "there is a reference" (no byte is read)
                ptrs[i] = <const void*>p if p != 0 else <const void*>ptrs
            with nogil:
                retval = C.pgsd_compare_staged_chunks(&self._handle, c_ticket, c_first, c_count, ptrs, sizes, eq)
                err = errno
            _raise_on_error(retval, self._name, err)
            return [bool(eq[i]) for i in range(n)]
        finally:
            free(ptrs)
            free(sizes)
            free(eq)

    def copy_staged(self, ticket, first, sizes):
        """Keep the packed bytes of staged chunks ``first, first + 1, ...`` of a ticket: returns one :class:`DeviceBuffer`
        of ``sizes[i]`` bytes per chunk (``None`` where ``sizes[i]`` is ``None``), filled asynchronously behind the
        pack (``pgsd_copy_staged_chunks``) -- references for :meth:`compare_staged` in later frames.  The buffers are
        the library's own, on the GPU the staging lives on (which need not be a tensor library's current device)."""
        self._check_open()
        cdef Py_ssize_t n = len(sizes), i
        if n == 0:
            return []
        for i in range(n):
            if sizes[i] is not None and (first + i >= len(ticket[2]) or int(sizes[i]) != ticket[2][first + i]):
                raise ValueError("chunk %d of the ticket has %d packed bytes" % (first + i, ticket[2][first + i]
                                                                                 if first + i < len(ticket[2]) else -1))
        device = ticket[3] if len(ticket) > 3 and ticket[3] is not None else self.pipeline_device()
        cdef uint64_t c_ticket = ticket[0]
        cdef uint32_t c_first = first, c_count = n
        cdef void** ptrs = <void**>calloc(n, sizeof(void*))
        cdef uintptr_t p
        cdef int retval, err
        if ptrs == NULL:
            raise MemoryError()
        out = []
        try:
            for i in range(n):
                if sizes[i] is None:
                    out.append(None)
                    continue
                t = DeviceBuffer((int(sizes[i]),), numpy.uint8, device)
                out.append(t)
                p = t.ptr
                ptrs[i] = <void*>p
            with nogil:
                retval = C.pgsd_copy_staged_chunks(&self._handle, c_ticket, c_first, c_count, ptrs)
                err = errno
            _raise_on_error(retval, self._name, err)
            return out
        finally:
            free(ptrs)

    def wait_packed(self):
        """Block until the pack kernels of the open frame are done (sources may be reused)."""
        cdef int retval
        self._check_open()
        with nogil:
            retval = C.pgsd_device_wait_packed(&self._handle)
        _raise_on_error(retval, self._name)

    def configure_device(self, device=-1, slab_bytes=0, n_slabs=0, n_writers=0, profile=False, prealloc_mib=0):
        """(Re)create the device pipeline of this file with explicit staging parameters.  ``prealloc_mib`` > 0: that
        much HBM staging and the whole ring of pinned slabs are allocated by this call instead of when a frame first
        needs them -- a simulation pays for its allocations before the run, not during a snapshot."""
        cdef C.pgsd_device_config cfg
        cdef int retval
        self._check_open()
        memset(&cfg, 0, sizeof(cfg))
        cfg.device = device
        cfg.slab_bytes = slab_bytes
        cfg.n_slabs = n_slabs
        cfg.n_writers = n_writers
        cfg.profile = 1 if profile else 0
        cfg.prealloc_mib = prealloc_mib
        with nogil:
            retval = C.pgsd_device_configure(&self._handle, &cfg)
        _raise_on_error(retval, self._name)
        self._source_stream = -1       # a new pipeline: it has to be told again

    def device_stats(self, reset=False):
        """dict of pipeline counters (pack launches/ms/bytes, D2H and write bytes/ms)."""
        cdef C.pgsd_device_stats st
        self._check_open()
        _raise_on_error(C.pgsd_device_get_stats(&self._handle, &st, 1 if reset else 0), self._name)
        return {"pack_launches": st.pack_launches, "pack_ms": st.pack_ms, "pack_rows": st.pack_rows,
                "pack_bytes_out": st.pack_bytes_out, "pack_bytes_in": st.pack_bytes_in, "d2h_bytes": st.d2h_bytes,
                "written_bytes": st.written_bytes, "d2h_ms": st.d2h_ms, "write_ms": st.write_ms,
                "side_bytes": st.side_bytes, "side_ms": st.side_ms, "side_on": st.side_on}

    def device_read_stats(self, reset=False):
        """dict: file bytes the device read path has ``pread`` (``pread_bytes``) and bytes it has copied host-to-device
        (``h2d_bytes``) since the pipeline was created or the counters were last reset.  Small reads go through a
        pinned, device-mapped arena and copy nothing."""
        cdef uint64_t a = 0, b = 0
        self._check_open()
        _raise_on_error(C.pgsd_device_read_counters(&self._handle, &a, &b, 1 if reset else 0), self._name)
        return {"pread_bytes": int(a), "h2d_bytes": int(b)}

    def plan_rows(self, rows, N, threshold=None):
        """Plan sparse indexed reads of ``rows`` from chunks of ``N`` rows (computed on the GPU; see :class:`RowPlan` and
        :func:`row_plan_model`, which it equals exactly).

        Args:
            rows: 32-bit row indices in GPU memory (torch GPU tensor, :class:`DeviceBuffer` or
                ``__cuda_array_interface__``), in any order, repeats allowed.
            N (int): the row count of the chunks the plan will be used on.
            threshold (float): touched fraction up to which reads through the plan take the sparse route
                (default: ``PGSD_PLAN_SPARSE_MAX``).
        """
        self._check_open()
        p_rows, n = _index_rows(rows)
        cdef RowPlan plan = RowPlan.__new__(RowPlan)
        plan.rows = rows
        plan.rows2 = DeviceBuffer((max(n, 1),), numpy.uint32, self.pipeline_device()).view(shape=(n,))
        plan.file = self
        plan.threshold = _PLAN_SPARSE_MAX if threshold is None else float(threshold)
        if not self._explicit_stream:
            self._sync_source_stream()      # the plan is ordered behind this stream's use of `rows`
        cdef uintptr_t c_rows = p_rows, c_rows2 = plan.rows2.ptr
        cdef uint64_t c_n = n, c_N = int(N)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_row_plan_create(&self._handle, <const uint32_t*>c_rows, c_n, c_N, <uint32_t*>c_rows2, &plan._plan)
            err = errno
        if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
            msg = C.pgsd_last_error_string()
            raise ValueError("plan_rows: %s" % (msg.decode('utf-8', 'replace') if msg != NULL else ""))
        _raise_on_error(retval, self._name, err)
        return plan

    # ------------------------------------------------------------------ reading
    cdef const C.pgsd_index_entry* _find(self, frame, name) except? NULL:
        name_b = name.encode('utf-8')
        cdef const char* c_name = name_b
        cdef uint64_t c_frame = int(frame)
        cdef const C.pgsd_index_entry* e
        with nogil:
            e = C.pgsd_find_chunk(&self._handle, c_frame, c_name)
        return e

    def chunk_exists(self, frame, name, write_all=False):
        """Test if a chunk exists (fl.pyx:656-715)."""
        self._check_open()
        return self._find(frame, name) != NULL

    cdef int _entry(self, frame, name, C.pgsd_index_entry* entry) except -1:
        """A copy of a chunk's index entry (a later flush may move the index storage): KeyError if the frame holds no
        such chunk, ValueError if its element type is unknown."""
        self._check_open()
        cdef const C.pgsd_index_entry* e = self._find(frame, name)
        if e == NULL:
            raise KeyError("frame " + str(frame) + " / chunk " + name + " not found in: " + self._name)
        if e.type not in _PGSD_TO_NP:
            raise ValueError("invalid type for chunk: " + name)
        entry[0] = e[0]
        return 0

    cdef const C.pgsd_index_entry* _optional(self, chunk, C.pgsd_index_entry* entry) except? NULL:
        """:meth:`_entry` of an optional ``(frame, name)``: ``entry``, filled in, or NULL for ``None``."""
        if chunk is None:
            return NULL
        self._entry(chunk[0], chunk[1], entry)
        return entry

    cdef int _entries(self, chunks, C.pgsd_index_entry* entries, const C.pgsd_index_entry** given) except -1:
        """The five chunk slots of a grouped reduction, each ``(frame, name)`` or ``None``: :meth:`_entry` of every chunk
        that is given, NULL for the others."""
        cdef int i
        for i in range(5):
            given[i] = NULL
            if chunks[i] is not None:
                frame, name = chunks[i]
                self._entry(frame, name, &entries[i])
                given[i] = &entries[i]
        self._check_open()
        return 0

    cdef _read_entry(self, const C.pgsd_index_entry* e, uint64_t height, uint64_t c_N, uint32_t c_M, uint32_t c_off,
                     bint c_all):
        """`pgsd_read_chunk` into a new numpy array of ``height`` rows: ``(height,)`` for Nx1 chunks, ``(height, M)``
        otherwise."""
        data_array = numpy.empty(dtype=_PGSD_TO_NP[e.type], shape=[height, e.M])
        cdef Py_buffer view
        cdef int retval, err
        if height != 0 and e.M != 0:
            PyObject_GetBuffer(data_array, &view, PyBUF_ANY_CONTIGUOUS)
            with nogil:
                retval = C.pgsd_read_chunk(&self._handle, view.buf, e, c_N, c_M, c_off, c_all)
                err = errno
            PyBuffer_Release(&view)
            _raise_on_error(retval, self._name, err)
        if e.M == 1:
            return data_array.reshape([height])
        return data_array

    def read_chunk(self, frame, name, N=0, M=0, offset=0, r_all=False):
        """Read a data chunk and return it as a numpy array (fl.pyx:717-874).

        ``(N,)`` for Nx1 chunks, ``(N, M)`` otherwise.  With ``r_all=True`` only ``N`` rows of
        ``M`` columns starting at row ``offset`` are read (every rank reads its partition).
        """
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        return self._read_entry(&entry, entry.N, int(N), int(M), int(offset), bool(r_all))

    def read_rows(self, frame, name, row0, n):
        """Rows ``[row0, row0 + n)`` of a chunk as an ``(n,)`` / ``(n, M)`` numpy array: `pgsd_read_chunk` with
        ``all == true`` (pgsd.c:2498-2534) into an array of THAT height -- :meth:`read_chunk` with ``r_all=True``
        allocates the chunk's full height like the reference's binding (fl.pyx:838-860), every rank the global array."""
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        if int(row0) < 0 or int(n) < 0 or int(row0) + int(n) > entry.N or int(row0) >= (1 << 32):
            raise ValueError("row range outside the chunk: " + name)
        return self._read_entry(&entry, int(n), int(n), entry.M, int(row0), True)

    def select_domain_device(self, frame, name, box, domain, dimensions=3):
        """The rows of a position chunk that lie in one spatial domain, selected on the GPU.

        Args:
            frame (int), name (str): the position chunk (N x 3 float32 or float64).
            box: ``[Lx, Ly, Lz, xy, xz, yz]`` (rounded to float32, as a file stores it).
            domain: a :class:`pgsd.hoomd.Domain` or a pair ``(lo, hi)`` of three fractions each, ``0 <= lo < hi <= 1``.
            dimensions (int): 3, or 2 to ignore z.

        Returns:
            ``(rows, count)`` typed like :func:`select_rows`: the ascending rows whose fractional coordinates (HOOMD's
            ``BoxDim::makeFraction`` in float64, wrapped into [0, 1)) lie in ``[lo, hi)`` on every axis -- an int32 GPU
            tensor of ``count`` entries where torch is importable, a :class:`DeviceBuffer` view otherwise.  Exactly
            :func:`pgsd.hoomd.domain_rows`.  The staged position rows are kept until the next :meth:`wait_read`: a
            ``read_chunk_device(..., rows=rows)`` of the same chunk before it reads no file bytes again.
        """
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        lo, hi = (domain.lo, domain.hi) if hasattr(domain, 'lo') else domain
        c_box = numpy.ascontiguousarray(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
        c_lo = numpy.ascontiguousarray(lo, dtype=numpy.float64).reshape(3)
        c_hi = numpy.ascontiguousarray(hi, dtype=numpy.float64).reshape(3)
        if c_box.shape[0] != 6:
            raise ValueError("box must hold 6 values")
        rows = _device_empty((max(int(entry.N), 1),), numpy.int32, self.pipeline_device())
        if not self._explicit_stream:
            self._sync_source_stream()      # the selection is ordered behind this stream's use of `rows`
        cdef uintptr_t c_rows = rows.data_ptr(), c_pbox = c_box.ctypes.data, c_plo = c_lo.ctypes.data, c_phi = c_hi.ctypes.data
        cdef uint32_t c_dims = int(dimensions)
        cdef uint64_t k = 0
        cdef int retval, err
        with nogil:
            retval = C.pgsd_select_domain_device(&self._handle, &entry, <const float*>c_pbox, c_dims,
                                                 <const double*>c_plo, <const double*>c_phi, <uint32_t*>c_rows, &k)
            err = errno
        if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
            msg = C.pgsd_last_error_string()
            raise ValueError("select_domain_device: %s" % (msg.decode('utf-8', 'replace') if msg != NULL else name))
        _raise_on_error(retval, self._name, err)
        return _device_head(rows, k), int(k)

    def domain_histogram_device(self, frame, name, box, bins, dimensions=3):
        """Per-axis histograms of a position chunk's fractional coordinates, counted on the GPU.

        Args:
            frame, name, box, dimensions: as :meth:`select_domain_device`.
            bins (int): bins per axis, a power of two in [2, 4096].

        Returns:
            A ``(3, bins)`` int64 numpy array: row ``a`` counts the rows whose wrapped fraction ``f[a]`` -- the value
            :meth:`select_domain_device` compares -- has ``int(f[a] * bins) == k``; NaN fractions are counted nowhere
            and the z row is zero when ``dimensions == 2``.  Exactly :func:`pgsd.hoomd.axis_histograms`.  The staged
            position rows are kept until the next :meth:`wait_read`: a :meth:`domain_counts_device` or a selection of
            the same chunk before it reads no file bytes again.  Needs no tensor library.
        """
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        c_box = numpy.ascontiguousarray(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
        if c_box.shape[0] != 6:
            raise ValueError("box must hold 6 values")
        if not 0 <= int(bins) < (1 << 32):
            raise ValueError("domain_histogram_device: bins must be a power of two in [2, 4096]")
        hist = numpy.zeros((3, int(bins) if int(bins) <= 4096 else 1), dtype=numpy.uint64)  # (the library refuses the rest)
        cdef uintptr_t c_pbox = c_box.ctypes.data, c_hist = hist.ctypes.data
        cdef uint32_t c_dims = int(dimensions), c_bins = int(bins)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_domain_histogram_device(&self._handle, &entry, <const float*>c_pbox, c_dims, c_bins,
                                                    <uint64_t*>c_hist)
            err = errno
        if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
            msg = C.pgsd_last_error_string()
            raise ValueError("domain_histogram_device: %s" % (msg.decode('utf-8', 'replace') if msg != NULL else name))
        _raise_on_error(retval, self._name, err)
        return hist.astype(numpy.int64)

    def domain_counts_device(self, frame, name, box, n, bounds, dimensions=3):
        """The number of rows of a position chunk in every cell of a rectilinear decomposition, counted on the GPU.

        Args:
            frame, name, box, dimensions: as :meth:`select_domain_device`.
            n: ``(nx, ny, nz)``, each 1 to 64, at most 4096 cells; ``nz == 1`` when ``dimensions == 2``.
            bounds: three sequences, per axis its ``n[a] - 1`` interior cell boundaries, strictly ascending inside
                (0, 1) -- :func:`pgsd.hoomd.grid_bounds` without each list's leading 0 and trailing 1.

        Returns:
            ``(counts, nowhere)``: ``counts`` a flat int64 numpy array of ``nx * ny * nz`` entries in
            :func:`pgsd.hoomd.domain_grid`'s rank order -- entry ``r`` is the count :meth:`select_domain_device` returns
            for cell ``r`` --, ``nowhere`` the number of rows with a NaN fraction.  Exactly
            :func:`pgsd.hoomd.domain_counts`.  Staging as :meth:`domain_histogram_device`.  Needs no tensor library.
        """
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        c_box = numpy.ascontiguousarray(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
        if c_box.shape[0] != 6:
            raise ValueError("box must hold 6 values")
        cells = [int(v) for v in n]
        if len(cells) != 3 or len(bounds) != 3:
            raise ValueError("domain_counts_device: n holds three cell counts and bounds three lists")
        if any(not 0 <= v < (1 << 32) for v in cells):
            raise ValueError("domain_counts_device: every axis takes 1 to 64 cells, at most 4096 in all")
        inner = [numpy.asarray(b, dtype=numpy.float64).reshape(-1) for b in bounds]
        if any(inner[a].shape[0] != max(cells[a] - 1, 0) for a in range(3)):
            raise ValueError("domain_counts_device: axis a takes n[a] - 1 interior bounds")
        c_n = numpy.array(cells, dtype=numpy.uint32)
        c_b = numpy.ascontiguousarray(numpy.concatenate(inner + [numpy.zeros(1)]))     # (never empty: a valid pointer)
        n_cells = cells[0] * cells[1] * cells[2]
        counts = numpy.zeros(n_cells if 1 <= n_cells <= 4096 else 1, dtype=numpy.uint64)    # (the library refuses the rest)
        cdef uintptr_t c_pbox = c_box.ctypes.data, c_pn = c_n.ctypes.data, c_pb = c_b.ctypes.data
        cdef uintptr_t c_counts = counts.ctypes.data
        cdef uint32_t c_dims = int(dimensions)
        cdef uint64_t nowhere = 0
        cdef int retval, err
        with nogil:
            retval = C.pgsd_domain_counts_device(&self._handle, &entry, <const float*>c_pbox, c_dims,
                                                 <const uint32_t*>c_pn, <const double*>c_pb, <uint64_t*>c_counts, &nowhere)
            err = errno
        if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
            msg = C.pgsd_last_error_string()
            raise ValueError("domain_counts_device: %s" % (msg.decode('utf-8', 'replace') if msg != NULL else name))
        _raise_on_error(retval, self._name, err)
        return counts.astype(numpy.int64), int(nowhere)

    def chunk_stats_device(self, frame, name, rows=None, n=None, norm2=False):
        """Per-column statistics of a chunk, or of a row list over it, reduced on the GPU.

        Args:
            frame (int), name (str): the chunk: N x M float32, float64, int32 or uint32 elements, ``1 <= M <= 4``.
            rows: ``None`` for all rows, or 32-bit row indices in GPU memory (e.g. :meth:`select_domain_device`'s), any
                order, repeats allowed: the statistics are those of ``chunk[rows]`` in list order.
            n (int): the number of entries of ``rows`` to take (default: all of them).
            norm2 (bool): append the column ``(x*x + y*y) + z*z`` (float64) of a float chunk of three columns; its
                ``max`` is the square of the largest speed.

        Returns:
            A :class:`pgsd.hoomd.FieldStats`: per column ``count``, ``nan``, ``inf`` (int64), ``min``, ``max``, ``sum``
            (float64) and the property ``mean``.  Exactly :func:`pgsd.hoomd.column_stats`, the sum included: its order
            is part of the definition.  The chunk is staged whole unless a selection, a census, an ordering or an earlier
            statistics call of the same chunk left it staged; the staged rows are kept until the next :meth:`wait_read`.
            An entry outside the chunk raises ValueError.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        cdef uintptr_t c_rows = 0
        count = 0
        if rows is not None:
            c_rows, count = _row_list("chunk_stats_device", rows, n)
        elif n is not None:
            raise ValueError("chunk_stats_device: n goes with rows")
        columns = int(entry.M) + (1 if norm2 else 0)
        counts = numpy.zeros((max(columns, 1) if columns <= 5 else 1, 3), dtype=numpy.uint64)     # (the library refuses the rest)
        values = numpy.zeros(counts.shape, dtype=numpy.float64)
        if rows is not None and not self._explicit_stream:
            self._sync_source_stream()      # the reduction is ordered behind this stream's use of `rows`
        cdef uintptr_t c_counts = counts.ctypes.data, c_values = values.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_norm2 = 1 if norm2 else 0
        cdef int retval, err
        with nogil:
            retval = C.pgsd_chunk_stats_device(&self._handle, &entry, <const uint32_t*>c_rows, c_n, c_norm2,
                                               <uint64_t*>c_counts, <double*>c_values)
            err = errno
        _raise_refused("chunk_stats_device", retval, name, self._name, err)
        counts = counts.astype(numpy.int64)
        return _hoomd.FieldStats(counts[:, 0].copy(), counts[:, 1].copy(), counts[:, 2].copy(), values[:, 0].copy(),
                                 values[:, 1].copy(), values[:, 2].copy())

    def frame_moments_device(self, chunks, defaults=None, type0=0, n_types=1, rows=None, n=None):
        """Mass, momentum, kinetic and internal energy and first moment per particle type, reduced on the GPU in one
        pass over up to five chunks.

        Args:
            chunks: five entries in the order typeid, mass, velocity, energy, position, each ``(frame, name)`` -- any
                chunk of the file, so that an elided chunk can come from frame 0 -- or ``None``: stored nowhere.  The
                typeid chunk is N x 1 uint32 or int32, mass and energy N x 1, velocity and position N x 3, the four
                float32 or float64, all the same; every chunk has the same N.  Without a typeid chunk every entry
                belongs to one group and ``n_types`` is 1.
            defaults: eight values -- mass, v[3], energy, x[3] --: the row that stands for every row of a chunk that is
                ``None`` (default: the schema's, 1, 0, 0, 0, 0, 0, 0, 0).
            type0, n_types: the types ``[type0, type0 + n_types)``, ``1 <= n_types <= 4``.
            rows: ``None`` for all rows, or 32-bit row indices in GPU memory, any order, repeats allowed.
            n (int): the number of entries of ``rows`` to take (default: all of them); without ``rows`` and without a
                chunk, the number of entries.

        Returns:
            A :class:`pgsd.hoomd.Moments`.  Exactly :func:`pgsd.hoomd.particle_moments`, the sums included: their order
            is part of the definition.  The chunks are staged whole unless a selection, a census, an ordering, a
            statistics or an earlier moments call left them staged; the staged rows are kept until the next
            :meth:`wait_read`.  An entry outside the chunks raises ValueError.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entries[5]
        cdef const C.pgsd_index_entry* given[5]
        chunks = list(chunks)
        if len(chunks) != 5:
            raise ValueError("frame_moments_device: chunks holds typeid, mass, velocity, energy, position (or None)")
        self._entries(chunks, entries, given)
        c_defaults = _moments_defaults("frame_moments_device", defaults)
        if not 0 <= int(type0) < (1 << 32) or not 0 <= int(n_types) < (1 << 32):
            raise ValueError("frame_moments_device: a call takes 1 to 4 types from a type id on")
        cdef uintptr_t c_rows = 0
        count = 0
        if rows is not None:
            c_rows, count = _row_list("frame_moments_device", rows, n)
        elif n is not None:
            if any(c is not None for c in chunks):
                raise ValueError("frame_moments_device: n goes with rows, or with no chunk at all")
            count = int(n)
            if count < 0:
                raise ValueError("frame_moments_device: n is a number of entries")
        elif all(c is None for c in chunks):
            raise ValueError("frame_moments_device: without a chunk and without rows, n says how many entries there are")
        T = int(n_types) if 1 <= int(n_types) <= 4 else 1         # (the library refuses the rest)
        counts = numpy.zeros(2 * T + 1, dtype=numpy.uint64)
        sums = numpy.zeros((T, 9), dtype=numpy.float64)
        if rows is not None and not self._explicit_stream:
            self._sync_source_stream()      # the reduction is ordered behind this stream's use of `rows`
        cdef uintptr_t c_counts = counts.ctypes.data, c_sums = sums.ctypes.data, c_pdef = c_defaults.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_type0 = int(type0), c_ntypes = int(n_types)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_frame_moments_device(&self._handle, given[0], given[1], given[2], given[3], given[4],
                                                 <const double*>c_pdef, c_type0, c_ntypes, <const uint32_t*>c_rows, c_n,
                                                 <uint64_t*>c_counts, <double*>c_sums)
            err = errno
        _raise_refused("frame_moments_device", retval, "refused", self._name, err)
        counts = counts.astype(numpy.int64)
        return _hoomd.Moments.from_sums(counts[0:2 * T:2].copy(), counts[1:2 * T:2].copy(), int(counts[2 * T]), sums)

    def cell_offsets_device(self, cell, n, n_cells):
        """The CSR offsets of a cell list in cell order, on the GPU.

        Args:
            cell: int32 cell ids in GPU memory, non-decreasing, in ``[0, n_cells]`` (:meth:`order_rows_by_cell_device`'s).
            n (int): the number of entries to take (``None``: all of ``cell``).
            n_cells (int): the cells of the grid, 1 to 2^20; the id ``n_cells`` is "nowhere".

        Returns:
            ``n_cells + 2`` int32 offsets in GPU memory: entry ``c`` is the first position of cell ``c``, the last entry
            is ``n``.  Exactly :func:`pgsd.hoomd.cell_offsets`.  Ids that descend or lie outside the range raise
            ValueError.  Needs no tensor library.
        """
        self._check_open()
        c_cell, count = _row_list("cell_offsets_device", cell, n)
        cells = int(n_cells)
        if not 0 <= cells < (1 << 32):
            raise ValueError("cell_offsets_device: a grid holds 1 to 2^20 cells")
        offs = _device_empty((cells + 2 if 1 <= cells <= (1 << 20) else 2,), numpy.int32, self.pipeline_device())
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `cell`
        cdef uintptr_t p_cell = c_cell, p_offs = _device_memory(offs)[0]
        cdef uint64_t c_n = count
        cdef uint32_t c_cells = cells
        cdef int retval, err
        with nogil:
            retval = C.pgsd_cell_offsets_device(&self._handle, <const int32_t*>p_cell, c_n, c_cells, <uint32_t*>p_offs)
            err = errno
        _raise_refused("cell_offsets_device", retval, "refused", self._name, err)
        return offs

    def cell_moments_device(self, chunks, rows, cell, n, n_cells, defaults=None):
        """Mass, momentum, kinetic and internal energy and first moment per grid cell of a row list in cell order,
        reduced on the GPU in one segmented pass.

        Args:
            chunks: four entries in the order mass, velocity, energy, position, each ``(frame, name)`` or ``None``:
                stored nowhere, as :meth:`frame_moments_device` takes them.
            rows, cell: 32-bit row indices and int32 cell ids in GPU memory, one id per entry, non-decreasing, in
                ``[0, n_cells]`` -- what :meth:`order_rows_by_cell_device` leaves.
            n (int): the number of entries to take (``None``: all of ``rows``).
            n_cells (int): the cells of the grid, 1 to 2^20.
            defaults: as :meth:`frame_moments_device`'s.

        Returns:
            A :class:`pgsd.hoomd.CellMoments` (``grid`` and ``cell_volume`` unset).  Exactly
            :func:`pgsd.hoomd.cell_moments`, the sums included: their order is part of the definition.  The chunks are
            staged whole unless an earlier call left them staged; the staged rows are kept until the next
            :meth:`wait_read`.  Ids that descend or lie outside the range and an entry outside the chunks raise
            ValueError.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entries[5]
        cdef const C.pgsd_index_entry* given[5]
        chunks = list(chunks)
        if len(chunks) != 4:
            raise ValueError("cell_moments_device: chunks holds mass, velocity, energy, position (or None)")
        self._entries([None] + chunks, entries, given)
        c_defaults = _moments_defaults("cell_moments_device", defaults)
        c_rows, c_cell, count = _cell_ordered_lists("cell_moments_device", rows, cell, n)
        cells = int(n_cells)
        if not 0 <= cells < (1 << 32):
            raise ValueError("cell_moments_device: a grid holds 1 to 2^20 cells")
        T = cells if 1 <= cells <= (1 << 20) else 1           # (the library refuses the rest)
        counts = numpy.zeros(2 * T + 1, dtype=numpy.uint64)
        sums = numpy.zeros((T, 9), dtype=numpy.float64)
        if not self._explicit_stream:
            self._sync_source_stream()      # the reduction is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell
        cdef uintptr_t c_counts = counts.ctypes.data, c_sums = sums.ctypes.data, c_pdef = c_defaults.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_cells = cells
        cdef int retval, err
        with nogil:
            retval = C.pgsd_cell_moments_device(&self._handle, given[1], given[2], given[3], given[4], <const double*>c_pdef,
                                                <const uint32_t*>p_rows, <const int32_t*>p_cell, c_n, c_cells,
                                                <uint64_t*>c_counts, <double*>c_sums)
            err = errno
        _raise_refused("cell_moments_device", retval, "refused", self._name, err)
        counts = counts.astype(numpy.int64)
        return _hoomd.CellMoments.from_sums(counts[0:2 * T:2].copy(), counts[1:2 * T:2].copy(), int(counts[2 * T]), sums)

    def neighbours_device(self, frame, name, box, r, cells, rows, cell, n=None, dimensions=3, bins=0, return_rows=False):
        """The neighbour census of a row list in cell order inside the range ``r``, on the GPU: the code base's pair pass.

        Args:
            frame (int), name (str): the position chunk, N x 3 float32 or float64.
            box: ``(Lx, Ly, Lz, xy, xz, yz)``; the kernel receives :func:`pgsd.hoomd.box_vectors` of it.
            r (float): the range, finite and positive, at most half the box's nearest plane distance on every axis.
            cells: ``(cx, cy, cz)``, no narrower than ``r`` (:func:`pgsd.hoomd.neighbour_grid_for`), up to 2^20 cells.
            rows, cell: 32-bit row indices and int32 cell ids in GPU memory, one id per entry, non-decreasing, in
                ``[0, n_cells]`` -- what :meth:`order_rows_by_cell_device` leaves for the same grid.
            n (int): the number of entries to take (``None``: all of ``rows``).
            dimensions (int): 2 never looks at z.
            bins (int): 0, or 1 to 1024 bins of the pair histogram over :func:`pgsd.hoomd.neighbour_edges2`, which are
                computed here on the host and handed to the kernel as they are.
            return_rows (bool): keep the per-entry results in GPU memory.

        Returns:
            A :class:`pgsd.hoomd.Neighbours`: exactly :func:`pgsd.hoomd.particle_neighbours` of the same list -- every
            counter and index, ``closest2`` bit for bit.  With ``return_rows`` its ``rows`` and ``cell`` are the arguments
            and ``count``, ``nearest`` (int32, typed like the row lists: ``0xFFFFFFFF``, no neighbour, reads ``-1``) and
            ``nearest2`` (float64) are arrays of ``n`` entries in GPU memory; otherwise the five are ``None``.  The chunk
            is staged whole unless the ordering left it staged; the staged rows are kept until the next
            :meth:`wait_read`.  What the library refuses (:c:func:`pgsd_neighbours_device`) raises ValueError and
            computes nothing.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("neighbours_device", cells)
        k_bins = int(bins)
        if not 0 <= k_bins < (1 << 32):
            raise ValueError("neighbours_device: bins is 0 or 1 to 1024")
        range_ = float(r)
        if 1 <= k_bins <= 1024 and range_ > 0.0 and range_ < float('inf'):
            c_edges = numpy.ascontiguousarray(_hoomd.neighbour_edges2(range_, k_bins), dtype=numpy.float64)
        else:
            c_edges = numpy.zeros(1 + (k_bins if k_bins <= 1024 else 0), dtype=numpy.float64)   # (the library refuses the rest)
        c_rows, c_cell, count = _cell_ordered_lists("neighbours_device", rows, cell, n)
        summary = numpy.zeros(8 + 257 + (k_bins if k_bins <= 1024 else 0), dtype=numpy.uint64)
        closest2 = numpy.zeros(1, dtype=numpy.float64)
        cdef uintptr_t p_count, p_nearest2, p_nearest
        device = self.pipeline_device() if return_rows else None
        out_count, p_count = _per_entry(count, (), numpy.int32, device)
        out_nearest, p_nearest = _per_entry(count, (), numpy.int32, device)
        out_nearest2, p_nearest2 = _per_entry(count, (), numpy.float64, device)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_edges = c_edges.ctypes.data, p_summary = summary.ctypes.data, p_closest2 = closest2.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0, c_bins = k_bins
        cdef double c_r = range_
        cdef int retval, err
        with nogil:
            retval = C.pgsd_neighbours_device(&self._handle, &entry, <const double*>p_vectors, c_r, c_dims,
                                              <const uint32_t*>p_cells, <const uint32_t*>p_rows, <const int32_t*>p_cell, c_n,
                                              c_bins, <const double*>p_edges, <uint32_t*>p_count, <double*>p_nearest2,
                                              <uint32_t*>p_nearest, <uint64_t*>p_summary, <double*>p_closest2)
            err = errno
        _raise_refused("neighbours_device", retval, "refused", self._name, err)
        got = _hoomd.Neighbours(range_, k_bins, grid, int(dimensions), summary, closest2[0])
        if return_rows:
            got.rows, got.cell = _device_head(rows, count), _device_head(cell, count)
            got.count, got.nearest = _device_head(out_count, count), _device_head(out_nearest, count)
            got.nearest2 = _device_head(out_nearest2, count)
        return got

    def neighbour_list_device(self, frame, name, box, r, cells, rows, cell, n=None, dimensions=3, half=False,
                              distances=False):
        """The neighbours of a row list in cell order inside the range ``r`` as a CSR pair list, on the GPU: what
        :meth:`neighbours_device` counts, handed over.

        Args:
            frame, name, box, r, cells, rows, cell, n, dimensions: as :meth:`neighbours_device` takes them.
            half (bool): the segment of entry ``i`` keeps only ``j > i`` by list position.
            distances (bool): also return the squared distance of every pair.

        Returns:
            A :class:`pgsd.hoomd.NeighbourList`: exactly :func:`pgsd.hoomd.neighbour_list` of the same list -- every offset
            and index, ``distance2`` bit for bit.  Its ``rows`` and ``cell`` are the arguments; ``offsets`` (uint64, ``n +
            1``), ``neighbours`` (uint32) and, when asked for, ``distance2`` (float64) are library-owned
            :class:`DeviceBuffer` s on the pipeline's device, the last two of exactly ``pairs`` entries (an empty view of a
            one-entry allocation where there is no pair).  Two passes: :c:func:`pgsd_neighbour_offsets_device` counts and
            scans, the segments are allocated, :c:func:`pgsd_neighbour_list_device` fills them.  The chunk is staged whole
            unless the ordering left it staged; the staged rows are kept until the next :meth:`wait_read`.  What the
            library refuses raises ValueError.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("neighbour_list_device", cells)
        range_ = float(r)
        c_rows, c_cell, count = _cell_ordered_lists("neighbour_list_device", rows, cell, n)
        device = self.pipeline_device()
        summary = numpy.zeros(4, dtype=numpy.uint64)
        offsets = DeviceBuffer((count + 1,), numpy.uint64, device)
        if not self._explicit_stream:
            self._sync_source_stream()      # the passes are ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_summary = summary.ctypes.data, p_offsets = offsets.ptr, p_neighbours, p_distance2 = 0
        cdef uint64_t c_n = count, c_capacity
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0, c_flags = 1 if half else 0
        cdef double c_r = range_
        cdef int retval, err
        with nogil:
            retval = C.pgsd_neighbour_offsets_device(&self._handle, &entry, <const double*>p_vectors, c_r, c_dims,
                                                     <const uint32_t*>p_cells, <const uint32_t*>p_rows,
                                                     <const int32_t*>p_cell, c_n, c_flags, <uint64_t*>p_offsets,
                                                     <uint64_t*>p_summary)
            err = errno
        _raise_refused("neighbour_list_device", retval, "refused", self._name, err)
        pairs = int(summary[2])
        neighbours = DeviceBuffer((max(pairs, 1),), numpy.uint32, device).view(shape=(pairs,))
        distance2 = DeviceBuffer((max(pairs, 1),), numpy.float64, device).view(shape=(pairs,)) if distances else None
        p_neighbours = neighbours.ptr
        if distances:
            p_distance2 = distance2.ptr
        c_capacity = pairs
        with nogil:
            retval = C.pgsd_neighbour_list_device(&self._handle, &entry, <const double*>p_vectors, c_r, c_dims,
                                                  <const uint32_t*>p_cells, <const uint32_t*>p_rows, <const int32_t*>p_cell,
                                                  c_n, c_flags, <const uint64_t*>p_offsets, c_capacity,
                                                  <uint32_t*>p_neighbours, <double*>p_distance2)
            err = errno
        _raise_refused("neighbour_list_device", retval, "refused", self._name, err)
        return _hoomd.NeighbourList(range_, grid, int(dimensions), bool(half), summary, _device_head(rows, count),
                                    _device_head(cell, count), offsets, neighbours, distance2)

    def components_device(self, frame, name, box, r, cells, rows, cell, n=None, dimensions=3):
        """The connected components of a row list in cell order within the linking length ``r``, on the GPU: the
        friends-of-friends grouping whose edges are the pairs of :meth:`neighbour_list_device` with ``half=True``.

        Args:
            frame, name, box, r, cells, rows, cell, n, dimensions: as :meth:`neighbours_device` takes them.

        Returns:
            A :class:`pgsd.hoomd.Components`: exactly :func:`pgsd.hoomd.neighbour_components` of the same list -- every
            label, id, size and summary word.  Its ``rows`` and ``cell`` are the arguments; ``label`` and ``component``
            (uint32, ``n``) and ``sizes`` (uint32, ``components``: a view of an allocation of ``max(n, 1)`` entries) are
            library-owned :class:`DeviceBuffer` s on the pipeline's device.  One call,
            :c:func:`pgsd_components_device`.  The chunk is staged whole unless the ordering left it staged; the staged
            rows are kept until the next :meth:`wait_read`.  What the library refuses raises ValueError.  Needs no tensor
            library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("components_device", cells)
        range_ = float(r)
        c_rows, c_cell, count = _cell_ordered_lists("components_device", rows, cell, n)
        device = self.pipeline_device()
        summary = numpy.zeros(6, dtype=numpy.uint64)
        label = DeviceBuffer((max(count, 1),), numpy.uint32, device).view(shape=(count,))
        component = DeviceBuffer((max(count, 1),), numpy.uint32, device).view(shape=(count,))
        sizes = DeviceBuffer((max(count, 1),), numpy.uint32, device)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_summary = summary.ctypes.data, p_label = label.ptr, p_component = component.ptr, p_sizes = sizes.ptr
        cdef uint64_t c_n = count
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef double c_r = range_
        cdef int retval, err
        with nogil:
            retval = C.pgsd_components_device(&self._handle, &entry, <const double*>p_vectors, c_r, c_dims,
                                              <const uint32_t*>p_cells, <const uint32_t*>p_rows, <const int32_t*>p_cell, c_n,
                                              0, <uint32_t*>p_label, <uint32_t*>p_component, <uint32_t*>p_sizes,
                                              <uint64_t*>p_summary)
            err = errno
        _raise_refused("components_device", retval, "refused", self._name, err)
        return _hoomd.Components(range_, grid, int(dimensions), summary, _device_head(rows, count), _device_head(cell, count),
                                 label, component, sizes.view(shape=(int(summary[2]),)))

    def component_moments_device(self, chunks, box, rows, label, component, n, components, defaults=None, dimensions=3):
        """Mass, momentum, energies, centre and extent per connected component of a row list, on the GPU: what each piece
        of a :meth:`components_device` result is.

        Args:
            chunks: four entries in the order mass, velocity, energy, position, each ``(frame, name)`` or ``None``:
                stored nowhere, as :meth:`cell_moments_device` takes them.  The position is required.
            box: ``(Lx, Ly, Lz, xy, xz, yz)``; dimensions: 2 or 3.
            rows, label, component: 32-bit arrays in GPU memory, ``n`` entries each: the list and what
                :meth:`components_device` returned for it (``rows``, ``label``, ``component`` of its result).
            n (int): the entries (``None``: all of ``rows``); components (int): the result's ``components``.
            defaults: as :meth:`frame_moments_device`'s.

        Returns:
            A :class:`pgsd.hoomd.ComponentMoments` whose tables are library-owned :class:`DeviceBuffer` s on the
            pipeline's device, allocated at ``max(components, 1)`` rows and viewed at ``components``: exactly
            :func:`pgsd.hoomd.component_moments`, every float bit for bit.  ``to_host()`` copies the tables.  One call,
            :c:func:`pgsd_component_moments_device`.  The chunks are staged whole unless an earlier call left them
            staged; the staged rows are kept until the next :meth:`wait_read`.  Labels and ids that are not a components
            result of the list and an entry outside the chunks raise ValueError.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entries[5]
        cdef const C.pgsd_index_entry* given[5]
        chunks = list(chunks)
        if len(chunks) != 4:
            raise ValueError("component_moments_device: chunks holds mass, velocity, energy, position (or None)")
        self._entries([None] + chunks, entries, given)
        c_defaults = _moments_defaults("component_moments_device", defaults)
        c_vectors = _box_vectors(box)
        c_rows, count = _row_list("component_moments_device", rows, n)
        c_label = _row_list("component_moments_device", label, count)[0]
        c_component = _row_list("component_moments_device", component, count)[0]
        pieces = int(components)
        if not 0 <= pieces < (1 << 32):
            raise ValueError("component_moments_device: a list of n entries has 1 to n components")
        device = self.pipeline_device()
        T = max(pieces, 1)
        summary = numpy.zeros(6, dtype=numpy.uint64)
        sums = DeviceBuffer((T, 9), numpy.float64, device).view(shape=(pieces, 9))
        extent = DeviceBuffer((T, 6), numpy.float64, device).view(shape=(pieces, 6))
        origin = DeviceBuffer((T, 3), numpy.float64, device).view(shape=(pieces, 3))
        flags = DeviceBuffer((T, 2), numpy.uint32, device).view(shape=(pieces, 2))
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of the lists
        cdef uintptr_t p_rows = c_rows, p_label = c_label, p_component = c_component
        cdef uintptr_t p_def = c_defaults.ctypes.data, p_vectors = c_vectors.ctypes.data, p_summary = summary.ctypes.data
        cdef uintptr_t p_sums = sums.ptr, p_extent = extent.ptr, p_origin = origin.ptr, p_flags = flags.ptr
        cdef uint64_t c_n = count, c_pieces = pieces
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef int retval, err
        with nogil:
            retval = C.pgsd_component_moments_device(&self._handle, given[1], given[2], given[3], given[4],
                                                     <const double*>p_def, <const double*>p_vectors, c_dims,
                                                     <const uint32_t*>p_rows, <const uint32_t*>p_label,
                                                     <const uint32_t*>p_component, c_n, c_pieces, 0, <double*>p_sums,
                                                     <double*>p_extent, <double*>p_origin, <uint32_t*>p_flags,
                                                     <uint64_t*>p_summary)
            err = errno
        _raise_refused("component_moments_device", retval, "refused", self._name, err)
        return _hoomd.ComponentMoments.from_tables(summary, sums, extent, origin, flags)

    def sph_sums_device(self, frame, name, box, h, cells, rows, cell, n=None, mass=None, density=None, defaults=None,
                        dimensions=3, kernel='wendland_c2', surface_below=None, return_rows=False):
        """The SPH kernel sums of a row list in cell order on the GPU: summation density, number density and Shepard sum
        over the kernel support ``2h``, in the order that is part of their definition.

        Args:
            frame (int), name (str): the position chunk, N x 3 float32 or float64.
            box: ``(Lx, Ly, Lz, xy, xz, yz)``; the kernel receives :func:`pgsd.hoomd.box_vectors` of it.
            h (float): the smoothing length, finite and positive; the support ``2h`` is at most half the box's nearest
                plane distance on every axis.
            cells: ``(cx, cy, cz)``, no narrower than ``2h`` (:func:`pgsd.hoomd.neighbour_grid_for` of ``2h``).
            rows, cell: 32-bit row indices and int32 cell ids in GPU memory, one id per entry, non-decreasing, in
                ``[0, n_cells]`` -- what :meth:`order_rows_by_cell_device` leaves for the same grid.
            n (int): the number of entries to take (``None``: all of ``rows``).
            mass, density: ``(frame, name)`` of an N x 1 float32 or float64 chunk, or ``None``: stored nowhere.
            defaults: ``(mass, density)`` that stand for a chunk stored nowhere; ``None``: every mass is 1.0 and, without a
                density chunk, there is no volume sum (a NaN as the density default says the same).
            dimensions (int): 2 never looks at z and takes the 2-D normalisation.
            kernel (str): ``'wendland_c2'`` or ``'cubic_spline'``.
            surface_below (float): count the entries whose Shepard sum is below it (``None``: no count).
            return_rows (bool): keep the per-entry results in GPU memory.

        Returns:
            A :class:`pgsd.hoomd.KernelSums`: exactly :func:`pgsd.hoomd.sph_kernel_sums` of the same list -- every counter
            and index, every float bit for bit.  With ``return_rows`` its ``rows`` and ``cell`` are the arguments and
            ``number``, ``density`` and ``shepard`` (``None`` without a volume) are float64 arrays of ``n`` entries in GPU
            memory; otherwise the five are ``None``.  The chunks are staged whole unless an earlier call left them
            staged; the staged rows are kept until the next :meth:`wait_read`.  What the library refuses
            (:c:func:`pgsd_sph_sums_device`) raises ValueError and computes nothing.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry, e_mass, e_density
        self._entry(frame, name, &entry)
        cdef const C.pgsd_index_entry* p_mass = self._optional(mass, &e_mass)
        cdef const C.pgsd_index_entry* p_density = self._optional(density, &e_density)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("sph_sums_device", cells)
        cdef uint32_t c_kernel = _sph_kernel("sph_sums_device", kernel)
        c_defaults, volume = _sph_defaults("sph_sums_device", defaults, density)
        c_rows, c_cell, count = _cell_ordered_lists("sph_sums_device", rows, cell, n)
        summary = numpy.zeros(13, dtype=numpy.uint64)
        cdef uintptr_t p_number, p_rho, p_shepard
        device = self.pipeline_device() if return_rows else None
        out_number, p_number = _per_entry(count, (), numpy.float64, device)
        out_rho, p_rho = _per_entry(count, (), numpy.float64, device)
        out_shepard, p_shepard = _per_entry(count, (), numpy.float64, device if volume else None)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_defaults = c_defaults.ctypes.data, p_summary = summary.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef double c_h = float(h), c_surface = float('nan') if surface_below is None else float(surface_below)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_sums_device(&self._handle, &entry, p_mass, p_density, <const double*>p_defaults,
                                            <const double*>p_vectors, c_h, c_kernel, c_dims, <const uint32_t*>p_cells,
                                            <const uint32_t*>p_rows, <const int32_t*>p_cell, c_n, c_surface,
                                            <double*>p_number, <double*>p_rho, <double*>p_shepard, <uint64_t*>p_summary)
            err = errno
        _raise_refused("sph_sums_device", retval, "refused", self._name, err)
        got = _hoomd.KernelSums(c_h, kernel, grid, int(dimensions), summary, volume, surface_below)
        if return_rows:
            got.rows, got.cell = _device_head(rows, count), _device_head(cell, count)
            got.number, got.density = _device_head(out_number, count), _device_head(out_rho, count)
            got.shepard = _device_head(out_shepard, count) if volume else None
        return got

    def smoothing_range_device(self, slength, N, rows=None, n=None, default=1.0):
        """The range of a smoothing-length chunk over a row list, reduced on the GPU: what chooses the grid of
        :meth:`sph_adaptive_sums_device` without copying a row to the host.

        Args:
            slength: ``(frame, name)`` of an N x 1 float32 or float64 chunk, or ``None``: stored nowhere, ``default``
                stands for every row and nothing is read.
            N (int): the rows of the frame.
            rows: ``None`` for all rows, or 32-bit row indices in GPU memory, any order, repeats allowed.
            n (int): the number of entries of ``rows`` to take (default: all of them).

        Returns:
            ``(n, bad, h_min, h_max)``: exactly :func:`pgsd.hoomd.smoothing_range`.  The chunk is staged whole unless an
            earlier call left it staged and is kept until the next :meth:`wait_read`.  An entry outside the chunk raises
            ValueError.  Needs no tensor library.
        """
        cdef C.pgsd_index_entry e_slength
        cdef const C.pgsd_index_entry* p_slength = self._optional(slength, &e_slength)
        cdef uintptr_t c_rows = 0
        count = 0
        if rows is not None:
            c_rows, count = _row_list("smoothing_range_device", rows, n)
        elif n is not None:
            raise ValueError("smoothing_range_device: n goes with rows")
        words = numpy.zeros(4, dtype=numpy.uint64)
        if rows is not None and not self._explicit_stream:
            self._sync_source_stream()      # the reduction is ordered behind this stream's use of `rows`
        cdef uintptr_t p_words = words.ctypes.data
        cdef uint64_t c_n = count, c_N = int(N)
        cdef double c_default = float(default)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_smoothing_range_device(&self._handle, p_slength, c_default, <const uint32_t*>c_rows, c_n, c_N,
                                                       <uint64_t*>p_words)
            err = errno
        _raise_refused("smoothing_range_device", retval, "refused", self._name, err)
        f = words[2:].view(numpy.float64)
        return int(words[0]), int(words[1]), float(f[0]), float(f[1])

    def sph_adaptive_sums_device(self, frame, name, box, h_max, cells, rows, cell, n=None, slength=None, mass=None,
                                 density=None, defaults=None, dimensions=3, kernel='wendland_c2', mode='gather',
                                 surface_below=None, return_rows=False):
        """The SPH kernel sums of a row list in cell order on the GPU with the smoothing length stored per particle: the
        neighbour count inside each entry's own support, number density, summation density, Shepard sum and, in gather
        mode, the grad-h factor ``omega``, in the order that is part of their definition.

        Args:
            frame, name, box, cells, rows, cell, n, mass, density, dimensions, kernel, surface_below: as
                :meth:`sph_sums_device` takes them; the grid is no narrower than ``2*h_max``.
            h_max (float): the declared bound of the listed valid smoothing lengths (:meth:`smoothing_range_device`),
                finite and positive; a listed valid ``h`` above it refuses the call.
            slength: ``(frame, name)`` of an N x 1 float32 or float64 chunk, or ``None``: stored nowhere.
            defaults: ``(mass, density, slength)`` that stand for a chunk stored nowhere; ``None``: 1.0, no volume sum
                without a density chunk (a NaN says the same) and 1.0.
            mode (str): ``'gather'`` (support ``2 h_i``) or ``'mean'`` (support ``h_i + h_j``).
            return_rows (bool): keep the per-entry results in GPU memory.

        Returns:
            A :class:`pgsd.hoomd.AdaptiveSums`: exactly :func:`pgsd.hoomd.sph_adaptive_sums` of the same list -- every
            counter and index, every float bit for bit -- with ``h_max`` the declared one.  With ``return_rows`` its
            ``rows`` and ``cell`` are the arguments and ``count`` (uint32), ``number``, ``density``, ``shepard`` (``None``
            without a volume) and ``omega`` (``None`` in mean mode) are arrays of ``n`` entries in GPU memory; otherwise
            they are ``None``; ``slength`` is always ``None``.  What the library refuses
            (:c:func:`pgsd_sph_adaptive_sums_device`) raises ValueError and computes nothing.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry, e_mass, e_density, e_slength
        self._entry(frame, name, &entry)
        cdef const C.pgsd_index_entry* p_mass = self._optional(mass, &e_mass)
        cdef const C.pgsd_index_entry* p_density = self._optional(density, &e_density)
        cdef const C.pgsd_index_entry* p_slength = self._optional(slength, &e_slength)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("sph_adaptive_sums_device", cells)
        cdef uint32_t c_kernel = _sph_kernel("sph_adaptive_sums_device", kernel)
        if mode not in _hoomd.SPH_MODES:
            raise ValueError("sph_adaptive_sums_device: the mode is one of %s: %r" % (', '.join(_hoomd.SPH_MODES), mode))
        cdef uint32_t c_mode = _hoomd.SPH_MODES.index(mode)
        c_defaults = numpy.ascontiguousarray(
            numpy.array([1.0, float('nan'), 1.0] if defaults is None else defaults, dtype=numpy.float64).reshape(-1))
        if c_defaults.shape[0] != 3:
            raise ValueError("sph_adaptive_sums_device: defaults holds a mass, a density and a smoothing length")
        volume = density is not None or c_defaults[1] == c_defaults[1]
        gather = c_mode == 0
        c_rows, c_cell, count = _cell_ordered_lists("sph_adaptive_sums_device", rows, cell, n)
        summary = numpy.zeros(22, dtype=numpy.uint64)
        cdef uintptr_t p_count, p_number, p_rho, p_shepard, p_omega
        device = self.pipeline_device() if return_rows else None
        out_count, p_count = _per_entry(count, (), numpy.uint32, device)
        out_number, p_number = _per_entry(count, (), numpy.float64, device)
        out_rho, p_rho = _per_entry(count, (), numpy.float64, device)
        out_shepard, p_shepard = _per_entry(count, (), numpy.float64, device if volume else None)
        out_omega, p_omega = _per_entry(count, (), numpy.float64, device if gather else None)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_defaults = c_defaults.ctypes.data, p_summary = summary.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef double c_h = float(h_max), c_surface = float('nan') if surface_below is None else float(surface_below)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_adaptive_sums_device(&self._handle, &entry, p_mass, p_density, p_slength,
                                                     <const double*>p_defaults, <const double*>p_vectors, c_h, c_kernel,
                                                     c_mode, c_dims, <const uint32_t*>p_cells, <const uint32_t*>p_rows,
                                                     <const int32_t*>p_cell, c_n, c_surface, <uint32_t*>p_count,
                                                     <double*>p_number, <double*>p_rho, <double*>p_shepard,
                                                     <double*>p_omega, <uint64_t*>p_summary)
            err = errno
        _raise_refused("sph_adaptive_sums_device", retval, "refused", self._name, err)
        got = _hoomd.AdaptiveSums(c_h, kernel, mode, grid, int(dimensions), summary, volume, surface_below)
        if return_rows:
            got.rows, got.cell = _device_head(rows, count), _device_head(cell, count)
            got.count = _device_head(out_count, count)
            got.number, got.density = _device_head(out_number, count), _device_head(out_rho, count)
            got.shepard = _device_head(out_shepard, count) if volume else None
            got.omega = _device_head(out_omega, count) if gather else None
        return got

    def sph_gradients_device(self, frame, name, box, h, cells, rows, cell, n=None, velocity=None, mass=None, density=None,
                             defaults=None, dimensions=3, kernel='wendland_c2', return_rows=False):
        """The SPH kernel gradients of a row list in cell order on the GPU: the density rate of the continuity equation,
        the velocity divergence and curl and the colour gradient (the surface normal) over the kernel support ``2h``,
        in the order that is part of their definition.

        Args:
            frame, name, box, h, cells, rows, cell, n, mass, density, defaults, dimensions, kernel: as
                :meth:`sph_sums_device` takes them.
            velocity: ``(frame, name)`` of an N x 3 float32 or float64 chunk, or ``None``: stored nowhere, every velocity
                is the zero vector.
            return_rows (bool): keep the per-entry results in GPU memory.

        Returns:
            A :class:`pgsd.hoomd.KernelGradients`: exactly :func:`pgsd.hoomd.sph_kernel_gradients` of the same list --
            every counter and index, every float bit for bit.  With ``return_rows`` its ``rows`` and ``cell`` are the
            arguments, ``density_rate`` and ``divergence`` are float64 arrays of ``n`` entries and ``curl`` and ``normal``
            of ``n x 3`` in GPU memory (the last three ``None`` without a volume); otherwise the six are ``None``.  The
            chunks are staged whole unless an earlier call left them staged; the staged rows are kept until the next
            :meth:`wait_read`.  What the library refuses (:c:func:`pgsd_sph_gradients_device`) raises ValueError and
            computes nothing.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry, e_velocity, e_mass, e_density
        self._entry(frame, name, &entry)
        cdef const C.pgsd_index_entry* p_velocity = self._optional(velocity, &e_velocity)
        cdef const C.pgsd_index_entry* p_mass = self._optional(mass, &e_mass)
        cdef const C.pgsd_index_entry* p_density = self._optional(density, &e_density)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("sph_gradients_device", cells)
        cdef uint32_t c_kernel = _sph_kernel("sph_gradients_device", kernel)
        c_defaults, volume = _sph_defaults("sph_gradients_device", defaults, density)
        c_rows, c_cell, count = _cell_ordered_lists("sph_gradients_device", rows, cell, n)
        summary = numpy.zeros(13, dtype=numpy.uint64)
        cdef uintptr_t p_rate, p_divergence, p_curl, p_normal
        device = self.pipeline_device() if return_rows else None
        out_rate, p_rate = _per_entry(count, (), numpy.float64, device)
        out_divergence, p_divergence = _per_entry(count, (), numpy.float64, device if volume else None)
        out_curl, p_curl = _per_entry(count, (3,), numpy.float64, device if volume else None)
        out_normal, p_normal = _per_entry(count, (3,), numpy.float64, device if volume else None)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_defaults = c_defaults.ctypes.data, p_summary = summary.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef double c_h = float(h)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_gradients_device(&self._handle, &entry, p_velocity, p_mass, p_density,
                                                 <const double*>p_defaults, <const double*>p_vectors, c_h, c_kernel, c_dims,
                                                 <const uint32_t*>p_cells, <const uint32_t*>p_rows, <const int32_t*>p_cell,
                                                 c_n, <double*>p_rate, <double*>p_divergence, <double*>p_curl,
                                                 <double*>p_normal, <uint64_t*>p_summary)
            err = errno
        _raise_refused("sph_gradients_device", retval, "refused", self._name, err)
        got = _hoomd.KernelGradients(c_h, kernel, grid, int(dimensions), summary, volume)
        if return_rows:
            got.rows, got.cell = _device_head(rows, count), _device_head(cell, count)
            got.density_rate = _device_head(out_rate, count)
            if volume:
                got.divergence = _device_head(out_divergence, count)
                got.curl, got.normal = _device_head_rows(out_curl, count), _device_head_rows(out_normal, count)
        return got

    def sph_tensors_device(self, frame, name, box, h, cells, rows, cell, n=None, velocity=None, mass=None, density=None,
                           defaults=None, dimensions=3, kernel='wendland_c2', det_min=0.25, return_rows=False):
        """The SPH gradient tensors of a row list in cell order on the GPU: the kernel-gradient correction matrix, its
        determinant, the corrected velocity-gradient tensor and the shear rate over the kernel support ``2h``, in the
        order that is part of their definition.

        Args:
            frame, name, box, h, cells, rows, cell, n, velocity, mass, density, dimensions, kernel: as
                :meth:`sph_gradients_device` takes them.
            defaults: ``(mass, density)`` that stand for a chunk stored nowhere; ``None``: the schema's 1.0 and 0.0 (the
                density default is a number here: there is no "no volume").
            det_min (float): an entry is corrected where ``det_min < det < inf``; a number, at least 0.
            return_rows (bool): keep the per-entry results in GPU memory.

        Returns:
            A :class:`pgsd.hoomd.KernelTensors`: exactly :func:`pgsd.hoomd.sph_gradient_tensors` of the same list --
            every counter and index, every float bit for bit.  With ``return_rows`` its ``rows`` and ``cell`` are the
            arguments and ``correction`` (``n x 6``), ``determinant`` (``n``), ``velocity_gradient`` (``n x 9``) and
            ``shear_rate`` (``n``) are float64 arrays in GPU memory; otherwise the six are ``None``.  The chunks are
            staged whole unless an earlier call left them staged; the staged rows are kept until the next
            :meth:`wait_read`.  What the library refuses (:c:func:`pgsd_sph_tensors_device`) raises ValueError and
            computes nothing.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry, e_velocity, e_mass, e_density
        self._entry(frame, name, &entry)
        cdef const C.pgsd_index_entry* p_velocity = self._optional(velocity, &e_velocity)
        cdef const C.pgsd_index_entry* p_mass = self._optional(mass, &e_mass)
        cdef const C.pgsd_index_entry* p_density = self._optional(density, &e_density)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("sph_tensors_device", cells)
        cdef uint32_t c_kernel = _sph_kernel("sph_tensors_device", kernel)
        c_defaults = _sph_defaults("sph_tensors_device", [1.0, 0.0] if defaults is None else defaults, density)[0]
        c_rows, c_cell, count = _cell_ordered_lists("sph_tensors_device", rows, cell, n)
        summary = numpy.zeros(14, dtype=numpy.uint64)
        cdef uintptr_t p_correction, p_determinant, p_gradient, p_shear
        device = self.pipeline_device() if return_rows else None
        out_correction, p_correction = _per_entry(count, (6,), numpy.float64, device)
        out_determinant, p_determinant = _per_entry(count, (), numpy.float64, device)
        out_gradient, p_gradient = _per_entry(count, (9,), numpy.float64, device)
        out_shear, p_shear = _per_entry(count, (), numpy.float64, device)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_defaults = c_defaults.ctypes.data, p_summary = summary.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef double c_h = float(h), c_det_min = float(det_min)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_tensors_device(&self._handle, &entry, p_velocity, p_mass, p_density,
                                               <const double*>p_defaults, <const double*>p_vectors, c_h, c_kernel, c_dims,
                                               c_det_min, <const uint32_t*>p_cells, <const uint32_t*>p_rows,
                                               <const int32_t*>p_cell, c_n, <double*>p_correction, <double*>p_determinant,
                                               <double*>p_gradient, <double*>p_shear, <uint64_t*>p_summary)
            err = errno
        _raise_refused("sph_tensors_device", retval, "refused", self._name, err)
        got = _hoomd.KernelTensors(c_h, kernel, grid, int(dimensions), summary, c_det_min)
        if return_rows:
            got.rows, got.cell = _device_head(rows, count), _device_head(cell, count)
            got.correction = _device_head_rows(out_correction, count)
            got.determinant = _device_head(out_determinant, count)
            got.velocity_gradient = _device_head_rows(out_gradient, count)
            got.shear_rate = _device_head(out_shear, count)
        return got

    def sph_accelerations_device(self, frame, name, box, h, cells, rows, cell, n=None, velocity=None, mass=None, density=None,
                                 pressure=None, defaults=None, viscosity=None, gravity=None, dimensions=3,
                                 kernel='wendland_c2', return_rows=False):
        """The SPH accelerations of a row list in cell order on the GPU: the pressure acceleration, Morris' laminar viscous
        acceleration and their sum with gravity over the kernel support ``2h``, in the order that is part of their
        definition.

        Args:
            frame, name, box, h, cells, rows, cell, n, velocity, mass, density, dimensions, kernel: as
                :meth:`sph_gradients_device` takes them.
            pressure: ``(frame, name)`` of an N x 1 float32 or float64 chunk, or ``None``: stored nowhere.
            defaults: ``(mass, density, pressure)`` that stand for a chunk stored nowhere; ``None``: 1.0, 0.0 and 0.0, the
                schema's (the density is a number here: a density of 0 gives what IEEE gives).
            viscosity (float): the dynamic viscosity ``mu``, finite and at least 0; ``None``: no viscous term.
            gravity: three finite floats; ``None``: ``(0, 0, 0)``.
            return_rows (bool): keep the per-entry results in GPU memory.

        Returns:
            A :class:`pgsd.hoomd.KernelAccelerations`: exactly :func:`pgsd.hoomd.sph_accelerations` of the same list --
            every counter and index, every float bit for bit.  With ``return_rows`` its ``rows`` and ``cell`` are the
            arguments and ``pressure_acc``, ``viscous_acc`` (``None`` without a viscosity) and ``total`` are float64
            arrays of ``n x 3`` in GPU memory; otherwise the five are ``None``.  The chunks are staged whole unless an
            earlier call left them staged; the staged rows are kept until the next :meth:`wait_read`.  What the library
            refuses (:c:func:`pgsd_sph_accelerations_device`) raises ValueError and computes nothing.  Needs no tensor
            library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry, e_velocity, e_mass, e_density, e_pressure
        self._entry(frame, name, &entry)
        cdef const C.pgsd_index_entry* p_velocity = self._optional(velocity, &e_velocity)
        cdef const C.pgsd_index_entry* p_mass = self._optional(mass, &e_mass)
        cdef const C.pgsd_index_entry* p_density = self._optional(density, &e_density)
        cdef const C.pgsd_index_entry* p_pressure = self._optional(pressure, &e_pressure)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("sph_accelerations_device", cells)
        cdef uint32_t c_kernel = _sph_kernel("sph_accelerations_device", kernel)
        c_defaults = _force_defaults("sph_accelerations_device", defaults)
        mu, c_gravity = _force_terms("sph_accelerations_device", viscosity, gravity)
        c_rows, c_cell, count = _cell_ordered_lists("sph_accelerations_device", rows, cell, n)
        summary = numpy.zeros(12, dtype=numpy.uint64)
        cdef uintptr_t p_pacc, p_vacc, p_total
        device = self.pipeline_device() if return_rows else None
        out_pacc, p_pacc = _per_entry(count, (3,), numpy.float64, device)
        out_vacc, p_vacc = _per_entry(count, (3,), numpy.float64, device if mu is not None else None)
        out_total, p_total = _per_entry(count, (3,), numpy.float64, device)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows` and `cell`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_defaults = c_defaults.ctypes.data, p_summary = summary.ctypes.data, p_gravity = c_gravity.ctypes.data
        cdef uint64_t c_n = count
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef double c_h = float(h), c_mu = -1.0 if mu is None else mu
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_accelerations_device(&self._handle, &entry, p_velocity, p_mass, p_density, p_pressure,
                                                     <const double*>p_defaults, <const double*>p_vectors, c_h, c_kernel,
                                                     c_dims, <const uint32_t*>p_cells, c_mu, <const double*>p_gravity,
                                                     <const uint32_t*>p_rows, <const int32_t*>p_cell, c_n, <double*>p_pacc,
                                                     <double*>p_vacc, <double*>p_total, <uint64_t*>p_summary)
            err = errno
        _raise_refused("sph_accelerations_device", retval, "refused", self._name, err)
        got = _hoomd.KernelAccelerations(c_h, kernel, grid, int(dimensions), summary, mu, tuple(c_gravity.tolist()))
        if return_rows:
            got.rows, got.cell = _device_head(rows, count), _device_head(cell, count)
            got.pressure_acc, got.total = _device_head_rows(out_pacc, count), _device_head_rows(out_total, count)
            if mu is not None:
                got.viscous_acc = _device_head_rows(out_vacc, count)
        return got

    def sph_body_force_device(self, frame, name, box, h, cells, body_rows, body_cell, fluid_rows, fluid_cell, n_body=None,
                              n_fluid=None, velocity=None, mass=None, density=None, pressure=None, defaults=None,
                              viscosity=None, about=None, dimensions=3, kernel='wendland_c2', return_rows=False):
        """The force and the torque the fluid exerts on a body, on the GPU: a pair pass between two row lists in cell order
        on one grid -- the targets (the body) and the sources (the fluid) -- and the ordered sums of the targets' force and
        torque terms.

        Args:
            frame, name, box, h, cells, velocity, mass, density, pressure, defaults, viscosity, dimensions, kernel: as
                :meth:`sph_accelerations_device` takes them.
            body_rows, body_cell, n_body: the targets -- a row list in GPU memory in cell order
                (:meth:`order_rows_by_cell_device`), its ids and its entries (``None``: all of ``body_rows``).
            fluid_rows, fluid_cell, n_fluid: the sources, likewise, ordered on the same grid.
            about: three finite floats, the point the torque is taken about; ``None``: ``(0, 0, 0)``.
            return_rows (bool): keep the per-target results in GPU memory.

        Returns:
            A :class:`pgsd.hoomd.KernelBodyForce`: exactly :func:`pgsd.hoomd.sph_body_force` of the same lists -- every
            counter and index, every float bit for bit.  With ``return_rows`` its ``rows`` and ``cell`` are the targets'
            arguments and ``contacts`` (uint32, ``n``), ``pressure_acc`` and ``viscous_acc`` (float64, ``n x 3``; ``None``
            without a viscosity) are arrays in GPU memory; otherwise the five are ``None``.  The chunks are staged whole
            unless an earlier call left them staged; the staged rows are kept until the next :meth:`wait_read`.  What
            the library refuses (:c:func:`pgsd_sph_body_force_device`) raises ValueError and computes nothing.  Needs no
            tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry, e_velocity, e_mass, e_density, e_pressure
        self._entry(frame, name, &entry)
        cdef const C.pgsd_index_entry* p_velocity = self._optional(velocity, &e_velocity)
        cdef const C.pgsd_index_entry* p_mass = self._optional(mass, &e_mass)
        cdef const C.pgsd_index_entry* p_density = self._optional(density, &e_density)
        cdef const C.pgsd_index_entry* p_pressure = self._optional(pressure, &e_pressure)
        c_vectors = _box_vectors(box)
        grid, c_cells = _cell_counts("sph_body_force_device", cells)
        cdef uint32_t c_kernel = _sph_kernel("sph_body_force_device", kernel)
        c_defaults = _force_defaults("sph_body_force_device", defaults)
        mu, c_about = _body_terms("sph_body_force_device", viscosity, about)
        c_rows, c_cell, count = _cell_ordered_lists("sph_body_force_device", body_rows, body_cell, n_body)
        c_rows2, c_cell2, count2 = _cell_ordered_lists("sph_body_force_device", fluid_rows, fluid_cell, n_fluid)
        summary = numpy.zeros(22, dtype=numpy.uint64)
        cdef uintptr_t p_contacts, p_pacc, p_vacc
        device = self.pipeline_device() if return_rows else None
        out_contacts, p_contacts = _per_entry(count, (), numpy.uint32, device)
        out_pacc, p_pacc = _per_entry(count, (3,), numpy.float64, device)
        out_vacc, p_vacc = _per_entry(count, (3,), numpy.float64, device if mu is not None else None)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of the lists
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_rows2 = c_rows2, p_cell2 = c_cell2
        cdef uintptr_t p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_defaults = c_defaults.ctypes.data, p_summary = summary.ctypes.data, p_about = c_about.ctypes.data
        cdef uint64_t c_n = count, c_n2 = count2
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef double c_h = float(h), c_mu = -1.0 if mu is None else mu
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_body_force_device(&self._handle, &entry, p_velocity, p_mass, p_density, p_pressure,
                                                  <const double*>p_defaults, <const double*>p_vectors, c_h, c_kernel, c_dims,
                                                  <const uint32_t*>p_cells, c_mu, <const double*>p_about,
                                                  <const uint32_t*>p_rows, <const int32_t*>p_cell, c_n,
                                                  <const uint32_t*>p_rows2, <const int32_t*>p_cell2, c_n2,
                                                  <uint32_t*>p_contacts, <double*>p_pacc, <double*>p_vacc,
                                                  <uint64_t*>p_summary)
            err = errno
        _raise_refused("sph_body_force_device", retval, "refused", self._name, err)
        got = _hoomd.KernelBodyForce(c_h, kernel, grid, int(dimensions), summary, mu, tuple(c_about.tolist()))
        if return_rows:
            got.rows, got.cell = _device_head(body_rows, count), _device_head(body_cell, count)
            got.contacts, got.pressure_acc = _device_head(out_contacts, count), _device_head_rows(out_pacc, count)
            if mu is not None:
                got.viscous_acc = _device_head_rows(out_vacc, count)
        return got

    def sph_samples_device(self, frame, name, box, h, cells, rows, cell, points, n=None, values=(), mass=None, density=None,
                           defaults=None, dimensions=3, kernel='wendland_c2', normalise=False):
        """The SPH interpolant of a row list in cell order at points of the caller's choosing, on the GPU: per point the
        entries strictly inside the kernel support ``2h`` of it, the density, the Shepard sum and the value columns, in
        the order that is part of their definition.

        Args:
            frame, name, box, h, cells, rows, cell, n, mass, density, dimensions, kernel: as :meth:`sph_sums_device` takes
                them.
            points: ``K x 3`` float32 or float64 values as a numpy array (converted to float64 and uploaded) or ``K x 3``
                float64 values in GPU memory; every per-point result is in their order.
            values: up to 4 values, each ``(frame, name)`` of a stored N x M float32 or float64 chunk, ``1 <= M <= 4``, or
                ``(chunk or None, columns, default)``: a chunk of that width, or one stored nowhere whose every element is
                ``default``.  At most 8 columns together, concatenated in the order given.
            defaults: ``(mass, density)`` that stand for a chunk stored nowhere; ``None``: 1.0 and 0.0, the schema's (the
                density is a number here: a density of 0 gives what IEEE gives).
            normalise (bool): divide every value by the Shepard sum (a point with no entry in reach: NaN).

        Returns:
            A :class:`pgsd.hoomd.KernelSamples`: exactly :func:`pgsd.hoomd.sph_samples` of the same list and points --
            every counter and index, every float bit for bit -- with ``count`` (uint32, ``K``), ``density``, ``shepard``
            (float64, ``K``) and ``values`` (float64, ``K x C``) in GPU memory.  The chunks are staged whole unless an
            earlier call left them staged; the staged rows are kept until the next :meth:`wait_read`.  What the library
            refuses (:c:func:`pgsd_sph_samples_device`) raises ValueError and computes nothing.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry, e_mass, e_density
        cdef C.pgsd_index_entry e_values[4]
        cdef const C.pgsd_index_entry* p_values[4]
        cdef uint32_t c_columns[4]
        cdef double c_value_defaults[4]
        cdef int k
        self._entry(frame, name, &entry)
        cdef const C.pgsd_index_entry* p_mass = self._optional(mass, &e_mass)
        cdef const C.pgsd_index_entry* p_density = self._optional(density, &e_density)
        c_vectors = _box_vectors(box)
        c_box = numpy.ascontiguousarray(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
        grid, c_cells = _cell_counts("sph_samples_device", cells)
        cdef uint32_t c_kernel = _sph_kernel("sph_samples_device", kernel)
        c_defaults = _sample_defaults("sph_samples_device", defaults)
        asked = _sample_values("sph_samples_device", values)
        widths = []
        for k in range(4):
            p_values[k] = NULL
            c_columns[k] = 0
            c_value_defaults[k] = 0.0
            if k < len(asked):
                chunk, columns, default = asked[k]
                p_values[k] = self._optional(chunk, &e_values[k])
                if columns is None:
                    columns = int(e_values[k].M)
                    if not 1 <= columns <= 4:
                        raise ValueError("sph_samples_device: value %d has 1 to 4 columns: %r" % (k, columns))
                c_columns[k] = columns
                c_value_defaults[k] = default
                widths.append(columns)
        if sum(widths) > 8:
            raise ValueError("sph_samples_device: the values hold at most 8 columns together: %d" % sum(widths))
        host_points, device_points, n_points = _sample_points("sph_samples_device", points)
        c_rows, c_cell, count = _cell_ordered_lists("sph_samples_device", rows, cell, n)
        device = self.pipeline_device()
        if device_points is None:
            device_points = _device_from_host(host_points if n_points else numpy.zeros((1, 3)), device)
        cdef uintptr_t p_points = _device_memory(device_points, "points")[0]
        summary = numpy.zeros(11, dtype=numpy.uint64)
        cdef uintptr_t p_count, p_dens, p_shep, p_vals
        total = sum(widths)
        out_count, p_count = _per_entry(n_points, (), numpy.uint32, device)
        out_dens, p_dens = _per_entry(n_points, (), numpy.float64, device)
        out_shep, p_shep = _per_entry(n_points, (), numpy.float64, device)
        out_vals, p_vals = _per_entry(n_points, (max(total, 1),), numpy.float64, device)
        if not self._explicit_stream:
            self._sync_source_stream()      # the pass is ordered behind this stream's use of `rows`, `cell` and `points`
        cdef uintptr_t p_rows = c_rows, p_cell = c_cell, p_vectors = c_vectors.ctypes.data, p_cells = c_cells.ctypes.data
        cdef uintptr_t p_defaults = c_defaults.ctypes.data, p_summary = summary.ctypes.data, p_box = c_box.ctypes.data
        cdef uint64_t c_n = count, c_K = n_points
        cdef uint32_t c_dims = int(dimensions) if 0 <= int(dimensions) < (1 << 32) else 0
        cdef uint32_t c_normalise = 1 if normalise else 0
        cdef double c_h = float(h)
        cdef int retval, err
        with nogil:
            retval = C.pgsd_sph_samples_device(&self._handle, &entry, p_mass, p_density, p_values, c_columns,
                                               c_value_defaults, <const double*>p_defaults, <const float*>p_box,
                                               <const double*>p_vectors, c_h, c_kernel, c_dims, <const uint32_t*>p_cells,
                                               <const uint32_t*>p_rows, <const int32_t*>p_cell, c_n, <const double*>p_points,
                                               c_K, c_normalise, <uint32_t*>p_count, <double*>p_dens, <double*>p_shep,
                                               <double*>p_vals, <uint64_t*>p_summary)
            err = errno
        _raise_refused("sph_samples_device", retval, "refused", self._name, err)
        got = _hoomd.KernelSamples(c_h, kernel, grid, int(dimensions), summary, bool(normalise), widths)
        got.count, got.density = _device_head(out_count, n_points), _device_head(out_dens, n_points)
        got.shepard = _device_head(out_shep, n_points)
        got.values = _device_head_rows(out_vals, n_points)
        if not total:       # (no value column: K x 0)
            got.values = out_vals.view(shape=(n_points, 0)) if isinstance(out_vals, DeviceBuffer) else out_vals[:n_points, :0]
        return got

    def frame_displacements_device(self, chunks, vectors_a, vectors_b, minimum_image=False, dimensions=3, type0=0,
                                   n_types=1, rows=None, n=None, out=None):
        """Drift, squared displacement and the largest move between two frames per particle type, reduced on the GPU in
        one pass over up to five chunks.

        Args:
            chunks: five entries in the order position a, image a, position b, image b, typeid, each ``(frame, name)``
                -- any chunk of the file, so that an elided chunk can come from frame 0 -- or ``None``: stored nowhere
                (the images: ``(0, 0, 0)`` in every row; the typeid: one group, ``n_types`` is 1).  The positions are
                N x 3 float32 or float64, both the same, the images N x 3 int32, the typeid N x 1 uint32 or int32;
                every chunk has the same N.
            vectors_a, vectors_b: :func:`pgsd.hoomd.box_vectors` of each frame's box.
            minimum_image (bool): fold the difference into frame b's box; allowed without image chunks only.
            dimensions (int): 2 leaves z unfolded.
            type0, n_types: the types ``[type0, type0 + n_types)``, ``1 <= n_types <= 4``.
            rows: ``None`` for all rows, or 32-bit row indices in GPU memory, any order, repeats allowed.
            n (int): the number of entries of ``rows`` to take (default: all of them).
            out: ``None``, or GPU memory of at least ``entries x 3`` float64 (a :class:`DeviceBuffer` or a tensor): entry
                ``k``'s displacement is stored at ``out[k]``.

        Returns:
            A :class:`pgsd.hoomd.Displacements`.  Exactly :func:`pgsd.hoomd.particle_displacements`, the sums included:
            their order is part of the definition.  The chunks are staged whole unless an earlier call left them staged
            (two chunks that are one stored chunk are staged once); the staged rows are kept until the next
            :meth:`wait_read`.  An entry outside the chunks raises ValueError.  Needs no tensor library.
        """
        from . import hoomd as _hoomd       # (the result type; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entries[5]
        cdef const C.pgsd_index_entry* given[5]
        chunks = list(chunks)
        if len(chunks) != 5:
            raise ValueError("frame_displacements_device: chunks holds position a, image a, position b, image b, typeid "
                             "(the images and the typeid may be None)")
        if chunks[0] is None or chunks[2] is None:
            raise ValueError("frame_displacements_device: both positions are chunks of the file")
        self._entries(chunks, entries, given)
        c_va = numpy.ascontiguousarray(numpy.asarray(vectors_a, dtype=numpy.float64).reshape(-1))
        c_vb = numpy.ascontiguousarray(numpy.asarray(vectors_b, dtype=numpy.float64).reshape(-1))
        if c_va.shape[0] != 6 or c_vb.shape[0] != 6:
            raise ValueError("frame_displacements_device: box vectors hold six values (pgsd.hoomd.box_vectors)")
        if not 0 <= int(type0) < (1 << 32) or not 0 <= int(n_types) < (1 << 32) or not 0 <= int(dimensions) < (1 << 32):
            raise ValueError("frame_displacements_device: a call takes 1 to 4 types from a type id on, in 2 or 3 dimensions")
        cdef uintptr_t c_rows = 0, c_out = 0
        count = int(entries[0].N)
        if rows is not None:
            c_rows, count = _row_list("frame_displacements_device", rows, n)
        elif n is not None:
            raise ValueError("frame_displacements_device: n goes with rows")
        if out is not None:
            p_out, out_bytes = _device_memory(out, "out")
            if out_bytes < count * 24:
                raise ValueError("frame_displacements_device: out holds fewer than entries x 3 float64 values")
            c_out = p_out
        T = int(n_types) if 1 <= int(n_types) <= 4 else 1         # (the library refuses the rest)
        counts = numpy.zeros(3 * T + 1, dtype=numpy.uint64)
        values = numpy.zeros((T, 5), dtype=numpy.float64)
        if (rows is not None or out is not None) and not self._explicit_stream:
            self._sync_source_stream()      # the reduction is ordered behind this stream's use of `rows` and `out`
        cdef uintptr_t c_counts = counts.ctypes.data, c_values = values.ctypes.data
        cdef uintptr_t c_pva = c_va.ctypes.data, c_pvb = c_vb.ctypes.data
        cdef uint64_t c_n = count if rows is not None else 0
        cdef uint32_t c_type0 = int(type0), c_ntypes = int(n_types), c_dims = int(dimensions)
        cdef uint32_t c_flags = 1 if minimum_image else 0
        cdef int retval, err
        with nogil:
            retval = C.pgsd_frame_displacements_device(&self._handle, given[0], given[1], given[2], given[3], given[4],
                                                       <const double*>c_pva, <const double*>c_pvb, c_flags, c_dims, c_type0,
                                                       c_ntypes, <const uint32_t*>c_rows, c_n, <double*>c_out,
                                                       <uint64_t*>c_counts, <double*>c_values)
            err = errno
        _raise_refused("frame_displacements_device", retval, "refused", self._name, err)
        entry = counts[2:3 * T:3].astype(numpy.int64)            # (UINT64_MAX, no entry, becomes -1)
        counts = counts.astype(numpy.int64)
        return _hoomd.Displacements.from_sums(counts[0:3 * T:3].copy(), counts[1:3 * T:3].copy(), entry, int(counts[3 * T]),
                                              values)

    def select_halo_device(self, frame, name, box, domain, ghost, dimensions=3):
        """A domain plus the ghost layer its neighbours reach, selected on the GPU from one position chunk.

        Args:
            frame, name, box, domain, dimensions: as :meth:`select_domain_device`.
            ghost: the layer's width as a real distance (:func:`pgsd.hoomd.ghost_fractions` turns it into fractions of
                the box) or three fractions ``(gx, gy, gz)``.

        Returns:
            ``(rows, n_owned, n_ghost, shift)``: ``rows`` (int32, typed like :meth:`select_domain_device`'s) holds the
            owned rows -- exactly that method's -- and behind them the ghost rows, each ascending; ``shift`` is an
            ``n_ghost x 3`` int32 array of the same kind, the box vectors to add to each ghost so that it lies next to
            the domain.  Exactly :func:`pgsd.hoomd.halo_rows`, whose band bounds (:func:`pgsd.hoomd.halo_bands`) are
            the ones handed to the kernel.  The staged position rows are kept as :meth:`select_domain_device` keeps them.
        """
        from . import hoomd as _hoomd       # (the model's helpers; pgsd.hoomd imports this module, hence not at the top)
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        cell = domain if hasattr(domain, 'lo') else _hoomd.Domain(*domain)
        bands, divided = _hoomd.halo_bands(cell, _hoomd._ghost_arg(box, ghost, dimensions), dimensions)
        c_box = numpy.ascontiguousarray(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
        c_lo = numpy.ascontiguousarray(cell.lo, dtype=numpy.float64).reshape(3)
        c_hi = numpy.ascontiguousarray(cell.hi, dtype=numpy.float64).reshape(3)
        c_bands = numpy.ascontiguousarray(bands, dtype=numpy.float64).reshape(24)
        c_div = numpy.ascontiguousarray(divided, dtype=numpy.uint32).reshape(3)
        if c_box.shape[0] != 6:
            raise ValueError("box must hold 6 values")
        device = self.pipeline_device()
        rows = _device_empty((max(int(entry.N), 1),), numpy.int32, device)
        # (the number of ghosts is the call's result: room for every row, and a copy of the ghosts' own behind it)
        room = _device_empty((max(int(entry.N), 1), 3), numpy.int32, device)
        if not self._explicit_stream:
            self._sync_source_stream()      # the selection is ordered behind this stream's use of `rows`
        cdef uintptr_t c_rows = rows.data_ptr(), c_shift = room.data_ptr(), c_pbox = c_box.ctypes.data
        cdef uintptr_t c_plo = c_lo.ctypes.data, c_phi = c_hi.ctypes.data, c_pb = c_bands.ctypes.data, c_pd = c_div.ctypes.data
        cdef uint32_t c_dims = int(dimensions)
        cdef uint64_t k[2]
        cdef int retval, err
        k[0] = k[1] = 0
        with nogil:
            retval = C.pgsd_select_halo_device(&self._handle, &entry, <const float*>c_pbox, c_dims, <const double*>c_plo,
                                               <const double*>c_phi, <const double*>c_pb, <const uint32_t*>c_pd,
                                               <uint32_t*>c_rows, <int32_t*>c_shift, k)
            err = errno
        if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
            msg = C.pgsd_last_error_string()
            raise ValueError("select_halo_device: %s" % (msg.decode('utf-8', 'replace') if msg != NULL else name))
        _raise_on_error(retval, self._name, err)
        n_owned, n_ghost = int(k[0]), int(k[1])
        if isinstance(room, DeviceBuffer):
            shift = room.view(shape=(n_ghost, 3)).clone()
        else:
            shift = room[:n_ghost].clone()
        return _device_head(rows, n_owned + n_ghost), n_owned, n_ghost, shift

    def order_rows_by_cell_device(self, frame, name, box, cells, rows, n=None, n_owned=None, shift=None, dimensions=3):
        """Sort a row list by the grid cell of its rows' positions, on the GPU and in place.

        Args:
            frame, name, box, dimensions: as :meth:`select_domain_device` (the position chunk the rows index).
            cells: ``(cx, cy, cz)``, each 1 to 1024; ``cz == 1`` when ``dimensions == 2``.
            rows: 32-bit row indices in GPU memory (e.g. :meth:`select_domain_device`'s), any order, repeats allowed.
            n (int): the number of entries to sort (default: all of ``rows``).
            n_owned (int): entries ``[0, n_owned)`` and ``[n_owned, n)`` -- :meth:`select_halo_device`'s owned and ghost
                runs -- are sorted separately and stay in that order (default: ``n``, one run).
            shift: the ghost run's ``(n - n_owned) x 3`` int32 array in GPU memory, permuted with its rows.

        Returns:
            The sorted cell ids of the ``n`` entries, int32 in GPU memory, typed like :func:`select_rows`' lists.  ``rows``
            (and ``shift``) are reordered in place by a stable sort on :func:`pgsd.hoomd.cell_ids`: exactly
            :func:`pgsd.hoomd.cell_order`.  After a selection of the same chunk (before the next :meth:`wait_read`) the
            staged position rows are used and no file byte is read.  An entry outside the chunk raises ValueError and
            leaves ``rows`` as it was.  Needs no tensor library.
        """
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        c_box = numpy.ascontiguousarray(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
        if c_box.shape[0] != 6:
            raise ValueError("box must hold 6 values")
        grid = [int(v) for v in cells]
        if len(grid) != 3 or any(not 0 <= v < (1 << 32) for v in grid):
            raise ValueError("order_rows_by_cell_device: cells holds three counts, each 1 to 1024")
        c_cells = numpy.array(grid, dtype=numpy.uint32)
        p_rows, n_rows = _index_rows(rows)
        count = n_rows if n is None else int(n)
        owned = count if n_owned is None else int(n_owned)
        if count >= (1 << 32):
            raise ValueError("order_rows_by_cell_device: a row list holds fewer than 2^32 entries")
        if count < 0 or count > n_rows:
            raise ValueError("order_rows_by_cell_device: rows holds fewer entries than n")
        if owned < 0 or owned > count:
            raise ValueError("order_rows_by_cell_device: n_owned exceeds the number of entries")
        cdef uintptr_t c_shift = 0
        if shift is not None:
            if (shift.element_size() if hasattr(shift, 'element_size')
                    else numpy.dtype(shift.__cuda_array_interface__['typestr']).itemsize) != 4:
                raise ValueError("order_rows_by_cell_device: shift holds 32-bit integers")
            p_shift, shift_bytes = _device_memory(shift, "shift")
            if shift_bytes < 12 * (count - owned):
                raise ValueError("order_rows_by_cell_device: shift holds fewer than 3 x (n - n_owned) entries")
            c_shift = p_shift
        cell = _device_empty((max(count, 1),), numpy.int32, self.pipeline_device())
        if not self._explicit_stream:
            self._sync_source_stream()      # the sort is ordered behind this stream's use of `rows` and `shift`
        cdef uintptr_t c_rows = p_rows, c_cell = cell.data_ptr(), c_pbox = c_box.ctypes.data, c_pc = c_cells.ctypes.data
        cdef uint32_t c_dims = int(dimensions)
        cdef uint64_t c_n = count, c_owned = owned
        cdef int retval, err
        with nogil:
            retval = C.pgsd_order_rows_by_cell_device(&self._handle, &entry, <const float*>c_pbox, c_dims,
                                                      <const uint32_t*>c_pc, <uint32_t*>c_rows, c_n, c_owned,
                                                      <int32_t*>c_shift, <int32_t*>c_cell)
            err = errno
        if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
            msg = C.pgsd_last_error_string()
            raise ValueError("order_rows_by_cell_device: %s" % (msg.decode('utf-8', 'replace') if msg != NULL else name))
        _raise_on_error(retval, self._name, err)
        return _device_head(cell, count)

    def select_where_device(self, terms, domain=None, box=None, dimensions=3):
        """The rows of a frame that satisfy every term of a predicate over per-particle chunks, selected on the GPU.

        Args:
            terms: up to 4 tuples ``(frame, name, column, value)``: element ``(row, column)`` of chunk ``name`` of
                ``frame`` (uint32, int32, float32 or float64; all chunks of one N) must lie in ``value`` -- a range, the
                tuple ``(lo, hi)`` with ``None`` for unbounded (``lo <= float64(x) < hi``; NaN never does), or a set of
                integers in [0, 64) as a list, set or 64-bit mask (integer chunks only).
            domain: ``None``, or ``(frame, name, domain)``: the rows must also lie in ``domain`` (a
                :class:`pgsd.hoomd.Domain` or a pair ``(lo, hi)``) by the position chunk ``name`` of ``frame``, as
                :meth:`select_domain_device` decides it with ``box`` and ``dimensions``.

        Returns:
            ``(rows, count)`` typed like :meth:`select_domain_device`: the ascending rows -- exactly
            :func:`pgsd.hoomd.where_rows`, intersected with :func:`pgsd.hoomd.domain_rows`.  The staged chunks are kept
            until the next :meth:`wait_read`: a ``read_chunk_device(..., rows=rows)`` of one of them before it reads no
            file bytes again.
        """
        cdef C.pgsd_index_entry c_chunks[4]
        cdef uint32_t c_columns[4]
        cdef uint32_t c_kinds[4]
        cdef double c_los[4]
        cdef double c_his[4]
        cdef uint64_t c_sets[4]
        cdef C.pgsd_index_entry c_pos
        cdef uint32_t n_terms = 0, c_dims = int(dimensions)
        cdef bint has_domain = domain is not None
        terms = list(terms)
        if len(terms) > 4:
            raise ValueError("select_where_device: a predicate has at most 4 terms")
        memset(c_sets, 0, sizeof(c_sets))
        memset(c_los, 0, sizeof(c_los))
        memset(c_his, 0, sizeof(c_his))
        for frame, name, column, value in terms:
            self._entry(frame, name, &c_chunks[n_terms])
            c_columns[n_terms] = int(column)
            if isinstance(value, tuple):
                lo, hi = value
                c_kinds[n_terms] = 0
                c_los[n_terms] = float('nan') if lo is None else float(lo)
                c_his[n_terms] = float('nan') if hi is None else float(hi)
                if (lo is not None and lo != lo) or (hi is not None and hi != hi):
                    c_los[n_terms], c_his[n_terms] = 0.0, 0.0     # a NaN bound of the caller's: nothing is kept
            else:
                mask = 0
                for member in ([] if isinstance(value, int) else value):
                    if not 0 <= int(member) < 64:
                        raise ValueError("select_where_device: set members lie in [0, 64)")
                    mask |= 1 << int(member)
                c_kinds[n_terms] = 1
                c_sets[n_terms] = int(value) if isinstance(value, int) else mask
            n_terms += 1
        N = int(c_chunks[0].N) if n_terms else 0
        c_box = c_lo = c_hi = None
        if has_domain:
            frame, name, cell = domain
            self._entry(frame, name, &c_pos)
            lo, hi = (cell.lo, cell.hi) if hasattr(cell, 'lo') else cell
            c_box = numpy.ascontiguousarray(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
            c_lo = numpy.ascontiguousarray(lo, dtype=numpy.float64).reshape(3)
            c_hi = numpy.ascontiguousarray(hi, dtype=numpy.float64).reshape(3)
            if c_box.shape[0] != 6:
                raise ValueError("box must hold 6 values")
            if n_terms == 0:
                N = int(c_pos.N)
        rows = _device_empty((max(N, 1),), numpy.int32, self.pipeline_device())
        if not self._explicit_stream:
            self._sync_source_stream()      # the selection is ordered behind this stream's use of `rows`
        cdef uintptr_t c_rows = rows.data_ptr(), c_pbox = 0, c_plo = 0, c_phi = 0
        if has_domain:
            c_pbox, c_plo, c_phi = c_box.ctypes.data, c_lo.ctypes.data, c_hi.ctypes.data
        cdef uint64_t k = 0
        cdef int retval, err
        with nogil:
            retval = C.pgsd_select_where_device(&self._handle, n_terms, c_chunks, c_columns, c_kinds, c_los, c_his, c_sets,
                                                &c_pos if has_domain else NULL,
                                                <const float*>c_pbox, c_dims, <const double*>c_plo, <const double*>c_phi,
                                                <uint32_t*>c_rows, &k)
            err = errno
        if retval == C.PGSD_ERROR_INVALID_ARGUMENT:
            msg = C.pgsd_last_error_string()
            raise ValueError("select_where_device: %s" % (msg.decode('utf-8', 'replace') if msg != NULL else ""))
        _raise_on_error(retval, self._name, err)
        return _device_head(rows, k), int(k)

    def read_chunk_device(self, frame, name, out=None, N=None, offset=0, columns=None, order=None,
                          bitcast=False, wait=True, fill=None, rows=None):
        """Read rows ``[offset, offset + N)`` of a chunk straight into GPU memory.

        The rows are ``pread`` into pinned slabs, copied to HBM and unpacked by a HIP kernel
        (device twin of :meth:`read_chunk` with ``r_all=True``; every rank reads its own
        partition).

        Args:
            frame (int), name (str): the chunk.
            out: destination torch GPU tensor of shape ``(N,)``, ``(N, M)`` or wider ``(N, S)``
                (e.g. a ``Scalar4`` array); ``None`` allocates a dense ``(N, M)`` tensor of the
                chunk's type on the current device.
            N (int): number of rows (default: all rows after ``offset``).
            offset (int): first row.
            columns (tuple): ``(c0, c1)`` columns of ``out`` that receive the chunk's M columns.
            order: optional int32 GPU tensor; row ``i`` goes to ``out[order[i]]``.
            bitcast (bool): reinterpret equal-sized elements (uint32 type id -> float ``w`` slot).
            wait (bool): block until the data is in ``out`` (else call :meth:`wait_read`).
            fill: value for the columns of ``out``'s rows that no chunk read before the same :meth:`wait_read`
                writes (``pgsd_field_dst.fill_rest``): velocity into a ``Scalar4`` array with ``fill=1.0`` gives
                ``(vx, vy, vz, 1.0)`` rows, stored whole.  ``None``: those columns keep what they hold.  Where
                several reads before one :meth:`wait_read` write the same column, the one submitted last wins.
            rows: an indexed read -- a :class:`RowPlan` (:meth:`plan_rows`: only the file blocks its rows touch are
                read while they are few, see there), or 32-bit row indices in GPU memory, in any order, repeats
                allowed (e.g. from :func:`select_rows` or :meth:`select_domain_device`); row ``k`` of ``out`` takes
                chunk row ``rows[k]``.  ``N`` defaults to ``len(rows)``, ``offset`` must be 0 and ``order`` ``None``.
                The whole chunk is staged and gathered at :meth:`wait_read`, which raises if an entry lies outside
                the chunk; nothing is written to row ``k`` of ``out`` for such an entry, the ``fill`` included.

        Returns:
            the destination tensor.
        """
        cdef C.pgsd_index_entry entry
        self._entry(frame, name, &entry)
        eN, eM = int(entry.N), int(entry.M)
        cdef uintptr_t p_rows = 0
        cdef RowPlan plan = None
        if isinstance(rows, RowPlan):
            # a plan: the sparse route while few blocks are touched, today's whole-chunk route with its rows otherwise
            plan = rows
            if plan.N != eN:
                raise ValueError("the plan was made for chunks of %d rows, %s has %d" % (plan.N, name, eN))
            if N is not None and int(N) != plan.n:
                raise ValueError("a read through a plan takes all of its rows")
            rows = plan.rows
            if plan.sparse:
                N = plan.n
            else:
                plan = None
        index_rows = rows                   # (`rows` is reused below for the destination's height)
        if index_rows is not None and (order is not None or int(offset) != 0):
            raise ValueError("an indexed read (rows=) takes neither order nor offset")
        if index_rows is not None and plan is None:
            p_rows, n_rows = _index_rows(index_rows)
            if N is None:
                N = n_rows
            if N > n_rows or N > eN:
                raise ValueError("rows holds fewer entries than requested")
        if N is None:
            N = eN - int(offset)
        if N < 0 or int(offset) + N > eN:
            raise ValueError("row range outside the chunk: " + name)
        if out is None:
            # on the GPU the pipeline runs on (not a tensor library's "current device")
            out = _device_empty((N, eM) if eM > 1 else (N,), _PGSD_TO_NP[entry.type], self.pipeline_device())
        cdef uintptr_t p_dst, p_order = 0
        p_dst, out_dtype, rows, width, stride = _rows2d(out, "out")
        c0 = 0 if columns is None else int(columns[0])
        if columns is not None and int(columns[1]) - c0 != eM:
            raise ValueError("columns must span the chunk's %d columns" % eM)
        if c0 + eM > max(stride, width):
            raise ValueError("chunk does not fit the destination rows")
        if order is None and rows < N:
            raise ValueError("destination has fewer rows than requested")
        if order is not None:
            p_order = _device_memory(order, "order")[0]
        cdef C.pgsd_field_dst dst
        memset(&dst, 0, sizeof(dst))
        dst.dst = <void*>p_dst
        dst.order = <const uint32_t*>p_order
        dst.dst_type = _pgsd_type(out_dtype, name)
        dst.dst_stride = stride
        dst.dst_col0 = c0
        dst.bitcast = 1 if bitcast else 0
        if fill is not None:
            dst.fill_rest = 1
            dst.fill_bits = int(numpy.array([fill], dtype=out_dtype).view(numpy.dtype('u%d' % out_dtype.itemsize))[0])
        self._keepalive.append((out, order, index_rows, plan))
        if not self._explicit_stream:
            self._sync_source_stream()      # the unpack is ordered behind this stream's use of `out`
        cdef uint64_t c_N = N, c_off = int(offset)
        cdef int retval, err
        if plan is not None:
            with nogil:
                retval = C.pgsd_read_rows_planned_device(&self._handle, &entry, plan._plan, &dst)
                err = errno
        elif index_rows is not None:
            with nogil:
                retval = C.pgsd_read_rows_device(&self._handle, &entry, <const uint32_t*>p_rows, c_N, &dst)
                err = errno
        else:
            with nogil:
                retval = C.pgsd_read_chunk_device(&self._handle, &entry, c_N, c_off, &dst)
                err = errno
        _raise_on_error(retval, self._name, err)
        if wait:
            self.wait_read()
        return out

    def wait_read(self):
        """Block until every :meth:`read_chunk_device` issued so far has landed in GPU memory."""
        cdef int retval, err
        self._check_open()
        with nogil:
            retval = C.pgsd_device_wait_read(&self._handle)
            err = errno
        if self._mode == 'r':
            self._keepalive = []
        _raise_on_error(retval, self._name, err)

    def find_matching_chunk_names(self, match, write_all=False):
        """All chunk names in the file that start with ``match`` (fl.pyx:876-945)."""
        self._check_open()
        retval = []
        match_b = match.encode('utf-8')
        cdef const char* c_match = match_b
        cdef const char* found
        with nogil:
            found = C.pgsd_find_matching_chunk_name(&self._handle, c_match, NULL)
        while found != NULL:
            retval.append(found.decode('utf-8'))
            with nogil:
                found = C.pgsd_find_matching_chunk_name(&self._handle, c_match, found)
        return retval

    def allgather(self, send):
        """Allgather the bytes of the 1-D uint8 array ``send`` over the file's communicator
        (``pgsd_handle_allgather``); returns a ``(nprocs, len(send))`` uint8 array."""
        self._check_open()
        send = numpy.ascontiguousarray(send, dtype=numpy.uint8)
        out = numpy.zeros((self.nprocs, send.size), dtype=numpy.uint8)
        cdef const uint8_t[::1] s = send
        cdef uint8_t[:, ::1] o = out
        cdef size_t nbytes = send.size
        cdef int retval
        if nbytes == 0:
            return out
        with nogil:
            retval = C.pgsd_handle_allgather(&self._handle, &s[0], &o[0, 0], nbytes)
        _raise_on_error(retval, self._name)
        return out

    # ------------------------------------------------------------------ protocol
    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.close()

    def __reduce__(self):
        """Allows filehandles to be pickled when in read only mode (fl.pyx:971-978)."""
        if self._mode not in ['rb', 'r']:
            raise PickleError("Only read only GSDFiles can be pickled.")
        return (PGSDFile, (self._name, self._mode, self.application, self.schema, self.schema_version))

    def __dealloc__(self):
        if self._is_open:
            with nogil:
                C.pgsd_close(&self._handle)
            self._is_open = False

    # ------------------------------------------------------------------ properties
    @property
    def name(self):
        return self._name

    @property
    def mode(self):
        return self._mode

    @property
    def pgsd_version(self):
        cdef uint32_t v = self._handle.header.pgsd_version
        return (v >> 16, v & 0xffff)

    @property
    def schema_version(self):
        cdef uint32_t v = self._handle.header.schema_version
        return (v >> 16, v & 0xffff)

    @property
    def schema(self):
        return self._handle.header.schema.decode('utf-8')

    @property
    def application(self):
        return self._handle.header.application.decode('utf-8')

    @property
    def rank(self):
        """int: this process's (or thread's) rank in the communicator the file was opened on."""
        return int(self._handle.rank)

    @property
    def nprocs(self):
        """int: number of ranks of the communicator the file was opened on."""
        return int(self._handle.nprocs)

    @property
    def nframes(self):
        self._check_open()
        return C.pgsd_get_nframes(&self._handle)

    @property
    def nnames(self):
        self._check_open()
        return C.pgsd_get_nnames(&self._handle)

    @property
    def file_size(self):
        """Logical end of the file as the writer tracks it (bytes)."""
        return int(self._handle.file_size)

    @property
    def maximum_write_buffer_size(self):
        self._check_open()
        return C.pgsd_get_maximum_write_buffer_size(&self._handle)

    @maximum_write_buffer_size.setter
    def maximum_write_buffer_size(self, size):
        cdef uint64_t c = size
        cdef int retval
        self._check_open()
        with nogil:
            retval = C.pgsd_set_maximum_write_buffer_size(&self._handle, c)
        _raise_on_error(retval, self._name)

    @property
    def index_entries_to_buffer(self):
        self._check_open()
        return C.pgsd_get_index_entries_to_buffer(&self._handle)

    @index_entries_to_buffer.setter
    def index_entries_to_buffer(self, number):
        cdef uint64_t c = number
        cdef int retval
        self._check_open()
        with nogil:
            retval = C.pgsd_set_index_entries_to_buffer(&self._handle, c)
        _raise_on_error(retval, self._name)
