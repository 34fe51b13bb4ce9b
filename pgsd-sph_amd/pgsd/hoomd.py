"""Read and write HOOMD / HOOMD-SPH schema PGSD files, MI355X-native.

Same surface as the reference's ``pgsd.hoomd`` (/root/reference/pgsd/pgsd/hoomd.py):
``open``, ``HOOMDTrajectory``, ``Frame`` (``ConfigurationData``, ``ParticleData``,
``ConstraintData``), ``read_log``; the same chunk names, dtypes, shapes and frame-0 /
default-value fallbacks on read (hoomd.py:724-902).

The reference's writer is disabled (``append`` raises NotImplementedError, hoomd.py:568; its
intended policy survives only as comments, hoomd.py:569-642).  Here ``append`` is real and
follows that policy: per-particle arrays are partitioned over the ranks
(``write_all=True, offset=part_dist``), configuration scalars, ``N``, ``types`` and
``type_shapes`` are replicated small chunks (``write_all=False``).  Per-particle attributes may
be **GPU-resident** (torch tensors or :class:`pgsd.fl.DeviceField`), in which case all of them
are packed by one fused HIP launch and streamed to the file; the per-rank row counts come
from one allgather over the installed communicator (RCCL over xGMI on GPU ranks).
"""
from collections import OrderedDict
import json
import logging
import hashlib
import warnings

import numpy

try:
    from . import fl
except ImportError:  # pragma: no cover - the shared library is missing
    fl = None

from .version import __version__ as _pgsd_version

logger = logging.getLogger('pgsd.hoomd')


_HOST_TYPES = (numpy.ndarray, numpy.generic, int, float, list, tuple, str)


def _is_device(x):
    if isinstance(x, _HOST_TYPES):      # the common case first: no attribute lookups on the torch side
        return False
    return fl is not None and (isinstance(x, fl.DeviceField) or fl._is_device_array(x))


_READER_FIELDS = {}


def _reader_fields(path, container):
    """(name, default, chunk name, upstream-only attribute?) of the per-row chunks of a container, built once."""
    fields = _READER_FIELDS.get(path)
    if fields is None:
        items = [(n, d, False) for n, d in container._default_value.items()]
        if path == 'particles':
            items += [(n, d, True) for n, d in container._extra_default_value.items()]
        fields = tuple((n, d, path + '/' + n, opt) for n, d, opt in items if n not in ('N', 'types', 'type_shapes'))
        _READER_FIELDS[path] = fields
    return fields


_SCHEMA_NAMES = []


def _schema_names(frame):
    """(path, chunk names in the order of the `_default_value` tables) of the three containers, built once."""
    if not _SCHEMA_NAMES:
        for path in ('configuration', 'particles', 'constraints'):
            container = getattr(frame, path)
            names = list(container._default_value)
            if path == 'particles':
                names += list(container._extra_default_value)
            _SCHEMA_NAMES.append((path, tuple(names)))
    return _SCHEMA_NAMES


def _rows(x):
    if fl is not None and isinstance(x, fl.DeviceField):
        return x.N
    shape = getattr(x, 'shape', None)
    if shape is None:                   # a bare __cuda_array_interface__ object
        shape = x.__cuda_array_interface__['shape']
    return int(shape[0])


class ConfigurationData(object):
    """Store configuration data (hoomd.py:45-108).

    Attributes:
        step (int): time step of this frame (:chunk:`configuration/step`).
        dimensions (int): number of dimensions (:chunk:`configuration/dimensions`); defaults to
            2 when the box has Lz == 0, else 3.
        box ((6,) float32): [lx, ly, lz, xy, xz, yz] (:chunk:`configuration/box`).
    """

    _default_value = OrderedDict()
    _default_value['step'] = numpy.uint64(0)
    _default_value['dimensions'] = numpy.uint8(3)
    _default_value['box'] = numpy.array([1, 1, 1, 0, 0, 0], dtype=numpy.float32)

    def __init__(self):
        self.step = None
        self.dimensions = None
        self._box = None

    def _get_box(self):
        return self._box

    def _set_box(self, value):
        # setting a box also fixes `dimensions` while the user has not chosen one: 2 for a flat box
        # (Lz == 0), else 3 (hoomd.py:89-99)
        self._box = value
        if self.dimensions is not None:
            return
        try:
            flat = value[2] == 0
        except TypeError:
            return
        self.dimensions = 2 if flat else 3

    box = property(_get_box, _set_box)

    def validate(self):
        """Convert ``box`` to a (6,) float32 array; ignore attributes that are ``None``."""
        logger.debug('Validating ConfigurationData')
        if self.box is not None:
            self.box = numpy.ascontiguousarray(self.box, dtype=numpy.float32)
            self.box = self.box.reshape([6])


def _field(dtype, M, default, upstream=False):
    return (dtype, M, dtype(default) if M == 1 else numpy.array(default, dtype=dtype), upstream)


# Every per-particle chunk in schema order: name -> (dtype, columns, default value, upstream-only?).  The first block
# is the PGSD-SPH schema the reference implements (hoomd.py:167-184), the second the upstream HOOMD attributes that the
# reference documents (hoomd.py:133-158) but leaves out of its reader.  `ParticleData._default_value` and
# `_extra_default_value` are made from this table.
_PARTICLE_FIELDS = OrderedDict([
    ('typeid', _field(numpy.uint32, 1, 0)), ('mass', _field(numpy.float32, 1, 1.0)),
    ('body', _field(numpy.int32, 1, -1)),
    ('position', _field(numpy.float32, 3, [0, 0, 0])), ('velocity', _field(numpy.float32, 3, [0, 0, 0])),
    ('slength', _field(numpy.float32, 1, 1.0)), ('density', _field(numpy.float32, 1, 0.0)),
    ('pressure', _field(numpy.float32, 1, 0.0)), ('energy', _field(numpy.float32, 1, 0.0)),
    ('auxiliary1', _field(numpy.float32, 3, [0, 0, 0])), ('auxiliary2', _field(numpy.float32, 3, [0, 0, 0])),
    ('auxiliary3', _field(numpy.float32, 3, [0, 0, 0])), ('auxiliary4', _field(numpy.float32, 3, [0, 0, 0])),
    ('image', _field(numpy.int32, 3, [0, 0, 0])),
    ('charge', _field(numpy.float32, 1, 0.0, True)), ('diameter', _field(numpy.float32, 1, 1.0, True)),
    ('moment_inertia', _field(numpy.float32, 3, [0, 0, 0], True)),
    ('orientation', _field(numpy.float32, 4, [1, 0, 0, 0], True)),
    ('angmom', _field(numpy.float32, 4, [0, 0, 0, 0], True)),
])

# HOOMD's Scalar4 arrays as `read_frame_device(scalar4=True)` assembles them: attribute -> (xyz chunk, w chunk,
# w is bit-cast?, default w)
_SCALAR4 = {'pos4': ('particles/position', 'particles/typeid', True, 0.0),
            'vel4': ('particles/velocity', 'particles/mass', False, 1.0)}


class ParticleData(object):
    """Store particle data chunks (hoomd.py:111-270).

    ``N`` is the number of particles **this rank** holds when writing and the global number
    when reading.  Array attributes may be numpy arrays / array-likes, or GPU-resident torch
    tensors / :class:`pgsd.fl.DeviceField` objects (write only).
    """

    _default_value = OrderedDict(
        [('N', numpy.uint32(0)), ('types', ['A'])]
        + [(name, field[2]) for name, field in _PARTICLE_FIELDS.items() if not field[3]]
        + [('type_shapes', [{}])])

    # upstream HOOMD attributes: written when set, read back when present in the file
    _extra_default_value = OrderedDict((name, field[2]) for name, field in _PARTICLE_FIELDS.items() if field[3])

    def __init__(self):
        self.N = 0
        self.types = None
        self.type_shapes = None
        for name in _PARTICLE_FIELDS:
            setattr(self, name, None)

    def validate(self):
        """Convert host arrays to contiguous arrays of the schema dtype and shape
        (hoomd.py:206-270); device-resident attributes are only shape-checked."""
        logger.debug('Validating ParticleData')
        for name, (dt, M, _, _) in _PARTICLE_FIELDS.items():
            value = getattr(self, name)
            if value is None:
                continue
            if _is_device(value):
                if _rows(value) != self.N:
                    raise ValueError("particles/%s has %d rows, expected N=%d" % (name, _rows(value), self.N))
                continue
            value = numpy.ascontiguousarray(value, dtype=dt)
            setattr(self, name, value.reshape([self.N]) if M == 1 else value.reshape([self.N, M]))
        if self.types is not None and (not len(set(self.types)) == len(self.types)):
            raise ValueError("Type names must be unique.")


class BondData(object):
    """Topology container of the upstream schema (hoomd.py:273-362): ``M`` particles per group (2 bonds / pairs, 3
    angles, 4 dihedrals / impropers), ``N``, ``types``, ``typeid`` (N,) uint32, ``group`` (N, M) int32.  The reference
    keeps the class but no :class:`Frame` of it carries topology (``Frame.__init__``, hoomd.py:450-456; the sections
    are commented out of its writer, hoomd.py:585-590), and neither does this one: the class is here so that code
    written against the reference imports and validates the same way."""

    def __init__(self, M):
        self.M = M
        self.N = 0
        self.types = None
        self.typeid = None
        self.group = None
        self._default_value = OrderedDict(
            [('N', numpy.uint32(0)), ('types', []), ('typeid', numpy.uint32(0)),
             ('group', numpy.array([0] * M, dtype=numpy.int32))])

    def validate(self):
        logger.debug('Validating BondData')
        for name, dtype, shape in (('typeid', numpy.uint32, [self.N]), ('group', numpy.int32, [self.N, self.M])):
            value = getattr(self, name)
            if value is not None:
                setattr(self, name, numpy.ascontiguousarray(value, dtype=dtype).reshape(shape))
        if self.types is not None and len(set(self.types)) != len(self.types):
            raise ValueError("Type names must be unique.")


class ConstraintData(object):
    """Store constraint data (hoomd.py:365-421): ``N``, ``value`` (N,) float32, ``group`` (N, 2) int32."""

    def __init__(self):
        self.M = 2
        self.N = 0
        self.value = None
        self.group = None
        self._default_value = OrderedDict()
        self._default_value['N'] = numpy.uint32(0)
        self._default_value['value'] = numpy.float32(0)
        self._default_value['group'] = numpy.array([0] * self.M, dtype=numpy.int32)

    def validate(self):
        logger.debug('Validating ConstraintData')
        if self.value is not None:
            self.value = numpy.ascontiguousarray(self.value, dtype=numpy.float32)
            self.value = self.value.reshape([self.N])
        if self.group is not None:
            self.group = numpy.ascontiguousarray(self.group, dtype=numpy.int32)
            self.group = self.group.reshape([self.N, self.M])


class Frame(object):
    """System state at one point in time (hoomd.py:424-467).

    Attributes:
        configuration (`ConfigurationData`), particles (`ParticleData`),
        constraints (`ConstraintData`), state (dict), log (dict of array-likes).
        num_procs (int): number of writer ranks this frame was partitioned for.
        part_dist: optional integer array with every rank's local particle count; when
            ``None``, `HOOMDTrajectory.append` obtains it with one allgather.
    """

    def __init__(self, num_procs=0):
        self.configuration = ConfigurationData()
        self.particles = ParticleData()
        self.constraints = ConstraintData()
        self.state = {}
        self.log = {}
        self.num_procs = num_procs
        self.part_dist = None

    def validate(self):
        """Validate all contained frame data."""
        self.configuration.validate()
        self.particles.validate()
        self.constraints.validate()


class Domain(object):
    """One cell of a spatial domain decomposition: fractional box coordinates ``lo[a] <= s[a] < hi[a]`` per axis.

    Args:
        lo, hi: three fractions each (x, y, z), ``0 <= lo < hi <= 1``.
    """

    def __init__(self, lo, hi):
        lo = tuple(float(v) for v in lo)
        hi = tuple(float(v) for v in hi)
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError("a domain has three lower and three upper bounds")
        if not all(0.0 <= a < b <= 1.0 for a, b in zip(lo, hi)):
            raise ValueError("a domain needs 0 <= lo < hi <= 1 on every axis: %r, %r" % (lo, hi))
        self.lo, self.hi = lo, hi

    def __eq__(self, other):
        return isinstance(other, Domain) and (self.lo, self.hi) == (other.lo, other.hi)

    def __hash__(self):
        return hash((self.lo, self.hi))

    def __repr__(self):
        return "Domain(lo=%r, hi=%r)" % (self.lo, self.hi)


def _split_bounds(n, split, axis):
    """Cell boundaries along one axis: n cells, `split` = the widths of the first n - 1 as fractions of the box."""
    n = int(n)
    if n < 1:
        raise ValueError("n%s must be at least 1" % axis)
    if split is None:
        return [i / n for i in range(n)] + [1.0]
    widths = [float(w) for w in split]
    if len(widths) != n - 1 or any(not w > 0.0 for w in widths):
        raise ValueError("%s_split must hold n%s - 1 = %d positive widths" % (axis, axis, n - 1))
    bounds = [0.0]
    for w in widths:
        bounds.append(bounds[-1] + w)
    if not bounds[-1] < 1.0:
        raise ValueError("%s_split widths must sum to less than 1" % axis)
    return bounds + [1.0]


def grid_bounds(nx, ny, nz, x_split=None, y_split=None, z_split=None):
    """``(bx, by, bz)``: the cell boundaries of an nx x ny x nz domain decomposition along each axis -- ``n + 1`` ascending
    fractions from 0.0 to 1.0 --, with `domain_grid`'s split lists.  Cell ``i`` of an axis is ``[b[i], b[i + 1])``."""
    return (_split_bounds(nx, x_split, 'x'), _split_bounds(ny, y_split, 'y'), _split_bounds(nz, z_split, 'z'))


def domain_grid(nx, ny, nz, x_split=None, y_split=None, z_split=None):
    """The cells of an nx x ny x nz domain decomposition as `Domain` objects, in HOOMD's rank order (``Index3D``:
    rank = x + nx * (y + ny * z), x fastest).  ``x_split`` etc. are the widths of the first n - 1 cells along that axis
    as fractions of the box, as in HOOMD's domain-decomposition split lists; ``None``: equal cells."""
    bx, by, bz = grid_bounds(nx, ny, nz, x_split, y_split, z_split)
    return [Domain((bx[i], by[j], bz[k]), (bx[i + 1], by[j + 1], bz[k + 1]))
            for k in range(int(nz)) for j in range(int(ny)) for i in range(int(nx))]


def _domain_bounds(domain):
    if isinstance(domain, Domain):
        return domain.lo, domain.hi
    d = Domain(*domain)
    return d.lo, d.hi


def domain_rows(position, box, domain, dimensions=3):
    """The rows of ``position`` (N x 3) inside ``domain``, ascending: the definition the GPU selection
    (`pgsd.fl.PGSDFile.select_domain_device`, ``read_frame_device(domain=...)``) matches bit for bit.

    HOOMD's ``BoxDim::makeFraction`` in float64, in exactly this operation order, box = ``[Lx, Ly, Lz, xy, xz, yz]``
    rounded to float32 as a file stores it::

        sx = ((x + Lx/2) - ((xz - yz*xy)*z + xy*y)) / Lx
        sy = ((y + Ly/2) - yz*z) / Ly
        sz = (z + Lz/2) / Lz
        s  = s - floor(s); s = 0 where s >= 1          # periodic wrap, per axis
        inside: lo[a] <= s[a] < hi[a] for x, y (and z unless dimensions == 2)
    """
    lo, hi = _domain_bounds(domain)
    f = _wrapped_fractions(position, box, dimensions)
    inside = numpy.ones(f[0].shape[0], dtype=bool)
    for a in range(len(f)):
        inside &= (lo[a] <= f[a]) & (f[a] < hi[a])
    return numpy.flatnonzero(inside)


def _wrapped_fractions(position, box, dimensions, unwrapped=False):
    """The fractional coordinates `domain_rows` documents, wrapped into [0, 1): one float64 array per axis that takes
    part (x, y, and z unless ``dimensions == 2``).  `domain_rows` and `halo_rows` both compare these.  ``unwrapped``: the
    same fractions ``s`` before the wrap (`sph_samples` judges a point outside the box on them)."""
    dimensions = int(dimensions)
    if dimensions not in (2, 3):
        raise ValueError("dimensions must be 2 or 3")
    b = numpy.asarray(box, dtype=numpy.float32).reshape(-1)
    if b.shape[0] < 6:
        raise ValueError("box must hold 6 values")
    Lx, Ly, Lz, xy, xz, yz = (numpy.float64(v) for v in b[:6])
    if not (Lx > 0 and Ly > 0 and (dimensions == 2 or Lz > 0)):
        raise ValueError("box lengths must be positive (Lz unless dimensions == 2)")
    p = numpy.asarray(position)
    p = p.astype(numpy.float64).reshape(-1, 3) if p.size else numpy.zeros((0, 3))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with numpy.errstate(invalid='ignore', divide='ignore'):
        s = [((x + Lx / 2) - ((xz - yz * xy) * z + xy * y)) / Lx,
             ((y + Ly / 2) - yz * z) / Ly,
             (z + Lz / 2) / Lz]
        if unwrapped:
            return s[:2 if dimensions == 2 else 3]
        out = []
        for a in range(2 if dimensions == 2 else 3):
            f = s[a] - numpy.floor(s[a])
            f[f >= 1.0] = 0.0
            out.append(f)
    return out


_CENSUS_MAX_BINS = 4096
_CENSUS_MAX_AXIS_CELLS = 64
_CENSUS_MAX_CELLS = 4096


def _census_bins(bins):
    bins = int(bins)
    if bins < 2 or bins > _CENSUS_MAX_BINS or bins & (bins - 1):
        raise ValueError("bins must be a power of two in [2, %d]: %r" % (_CENSUS_MAX_BINS, bins))
    return bins


def axis_histograms(position, box, bins, dimensions=3):
    """Per-axis histograms of the particles' fractional coordinates: a ``(3, bins)`` int64 array, the definition the GPU
    census (`pgsd.fl.PGSDFile.domain_histogram_device`, `HOOMDTrajectory.axis_histograms_device`) equals exactly.

    With ``f[a]`` the wrapped fraction `domain_rows` compares, row ``a`` counts in bin ``int(f[a] * bins)`` every row
    whose ``f[a]`` is no NaN (NaN and infinite coordinates give one; such a row is counted in no bin of that axis).
    ``bins`` is a power of two in [2, 4096]: ``f`` lies in [0, 1), so the product is exact and below ``bins`` -- no
    clamp --, and every bin edge ``k / bins`` is an exact float64: the cumulative histogram at ``k`` IS the number of
    rows `domain_rows` gives the slab ``[0, k / bins)``.  With ``dimensions == 2`` the z row is zero."""
    bins = _census_bins(bins)
    f = _wrapped_fractions(position, box, dimensions)
    hist = numpy.zeros((3, bins), dtype=numpy.int64)
    for a in range(len(f)):
        fa = f[a][f[a] == f[a]]
        hist[a] = numpy.bincount((fa * bins).astype(numpy.int64), minlength=bins)
    return hist


def _census_cells(nx, ny, nz, dimensions):
    n = (int(nx), int(ny), int(nz))
    if any(v < 1 or v > _CENSUS_MAX_AXIS_CELLS for v in n) or n[0] * n[1] * n[2] > _CENSUS_MAX_CELLS:
        raise ValueError("a census takes 1 to %d cells per axis and at most %d in all: %r"
                         % (_CENSUS_MAX_AXIS_CELLS, _CENSUS_MAX_CELLS, n))
    if int(dimensions) == 2 and n[2] != 1:
        raise ValueError("dimensions == 2 takes nz == 1: z is not looked at, several z cells would each own every row")
    return n


def _interior_bounds(bounds):
    """The interior boundaries of `grid_bounds`' three lists, checked: strictly ascending inside (0, 1)."""
    inner = [numpy.array(b[1:-1], dtype=numpy.float64) for b in bounds]
    for a, b in enumerate(inner):
        edges = numpy.concatenate(([0.0], b, [1.0]))
        if not numpy.all(edges[:-1] < edges[1:]):
            raise ValueError("the cell boundaries on axis %s do not ascend strictly inside (0, 1)" % 'xyz'[a])
    return inner


def domain_counts(position, box, nx, ny, nz, x_split=None, y_split=None, z_split=None, dimensions=3):
    """``(counts, nowhere)``: the number of particles in every cell of `domain_grid` ``(nx, ny, nz, x_split, y_split,
    z_split)`` -- a flat int64 array in its rank order, ``rank = x + nx * (y + ny * z)`` --, the definition the GPU
    census (`pgsd.fl.PGSDFile.domain_counts_device`, `HOOMDTrajectory.domain_counts_device`) equals exactly.

    A row's cell on an axis is the number of that axis' interior boundaries ``b`` (`grid_bounds`) with ``b <= f``, so
    ``counts[r] == len(domain_rows(position, box, domain_grid(...)[r], dimensions))``.  A row whose fraction is NaN on an
    axis that takes part belongs to no cell and is counted in ``nowhere``: ``counts.sum() + nowhere == N``.  Each of
    ``nx``, ``ny``, ``nz`` is at most 64, their product at most 4096; ``dimensions == 2`` needs ``nz == 1``."""
    n = _census_cells(nx, ny, nz, dimensions)
    inner = _interior_bounds(grid_bounds(n[0], n[1], n[2], x_split, y_split, z_split))
    f = _wrapped_fractions(position, box, dimensions)
    rows = f[0].shape[0]
    somewhere = numpy.ones(rows, dtype=bool)
    cell = numpy.zeros(rows, dtype=numpy.int64)
    stride = 1
    for a in range(len(f)):
        ok = f[a] == f[a]
        somewhere &= ok
        cell += numpy.searchsorted(inner[a], numpy.where(ok, f[a], 0.0), side='right') * stride   # bounds <= f
        stride *= n[a]
    counts = numpy.bincount(cell[somewhere], minlength=n[0] * n[1] * n[2]).astype(numpy.int64)
    return counts, int(rows - numpy.count_nonzero(somewhere))


def balanced_splits(hist_row, n, min_bins=1):
    """The split list -- the widths of the first ``n - 1`` cells, as `domain_grid` takes them -- that cuts one axis into
    ``n`` slabs of nearly equal particle counts, from that axis' row of `axis_histograms`.  Integer arithmetic only.

    With ``cum(k)`` the sum of bins ``[0, k)`` and ``total = cum(bins)``, boundary ``j`` (``1 <= j < n``) is the
    smallest bin edge ``k`` with ``cum(k) * n >= j * total``, then forced into ``[k_(j-1) + min_bins, bins - (n - j) *
    min_bins]`` (``k_0 = 0``): every slab is at least ``min_bins`` bins wide -- ``ceil(ghost_fraction * bins)`` keeps
    a cell no narrower than its ghost layer.  An empty histogram gives equal edges ``max(j * bins // n, j * min_bins)``,
    forced the same way.  The widths ``(k_j - k_(j-1)) / bins`` are dyadic, so `domain_grid`'s running sums are exact
    and its boundaries are these edges.  Where nothing was forced, every slab's count differs from ``total / n`` by
    less than the largest bin's count.  ``n == 1`` gives ``[]``; ``n * min_bins > bins`` raises ValueError."""
    h = [int(v) for v in numpy.asarray(hist_row).reshape(-1)]
    bins = _census_bins(len(h))
    n, min_bins = int(n), int(min_bins)
    if n < 1 or min_bins < 1:
        raise ValueError("n and min_bins must be at least 1")
    if n * min_bins > bins:
        raise ValueError("%d slabs of at least %d bins do not fit into %d bins" % (n, min_bins, bins))
    if any(v < 0 for v in h):
        raise ValueError("a histogram holds counts >= 0")
    cum = [0]
    for v in h:
        cum.append(cum[-1] + v)
    total = cum[-1]
    edges, k = [0], 0
    for j in range(1, n):
        if total == 0:
            k = max(j * bins // n, j * min_bins)
        else:
            while cum[k] * n < j * total:
                k += 1
        edges.append(min(max(k, edges[-1] + min_bins), bins - (n - j) * min_bins))
    return [(edges[j] - edges[j - 1]) / bins for j in range(1, n)]


def _balanced_axis_splits(hist, n, min_bins, dimensions):
    return (balanced_splits(hist[0], n[0], min_bins), balanced_splits(hist[1], n[1], min_bins),
            None if int(dimensions) == 2 else balanced_splits(hist[2], n[2], min_bins))


def balanced_grid(position, box, nx, ny, nz, bins=1024, min_bins=1, dimensions=3):
    """``(domains, (x_split, y_split, z_split))``: the decomposition whose slabs hold nearly equal particle counts on
    every axis -- `axis_histograms` at ``bins`` bins, `balanced_splits` per axis, `domain_grid` over the result (the
    marginal quantiles, the first step of HOOMD's load balancer; `domain_counts` tells how even the cells came out).
    The z split is ``None`` when ``dimensions == 2``."""
    n = _census_cells(nx, ny, nz, dimensions)
    splits = _balanced_axis_splits(axis_histograms(position, box, bins, dimensions), n, min_bins, dimensions)
    return domain_grid(n[0], n[1], n[2], *splits), splits


def ghost_fractions(box, width, dimensions=3):
    """``(gx, gy, gz)``: a ghost layer of the real width ``width`` (HOOMD's ``r_ghost``) as a fraction of the box along
    each axis -- ``width`` over the box's nearest plane distance on that axis (``BoxDim::getNearestPlaneDistance``),
    in float64 from the float32 box values ``[Lx, Ly, Lz, xy, xz, yz]`` a file stores::

        npd_x = Lx / sqrt(1 + xy*xy + (xy*yz - xz)**2),   npd_y = Ly / sqrt(1 + yz*yz),   npd_z = Lz

    ``gz`` is 0 when ``dimensions == 2``.  ``width`` must be finite and >= 0.  Host arithmetic only: the GPU selection
    receives the band bounds computed from these fractions (`halo_bands`) and never repeats it."""
    dimensions = int(dimensions)
    if dimensions not in (2, 3):
        raise ValueError("dimensions must be 2 or 3")
    width = float(width)
    if not (width >= 0.0 and width < float('inf')):
        raise ValueError("the ghost layer width must be finite and >= 0: %r" % (width,))
    b = numpy.asarray(box, dtype=numpy.float32).reshape(-1)
    if b.shape[0] < 6:
        raise ValueError("box must hold 6 values")
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in b[:6])
    if not (Lx > 0 and Ly > 0 and (dimensions == 2 or Lz > 0)):
        raise ValueError("box lengths must be positive (Lz unless dimensions == 2)")
    npd_x = Lx / numpy.sqrt(1.0 + xy * xy + (xy * yz - xz) * (xy * yz - xz))
    npd_y = Ly / numpy.sqrt(1.0 + yz * yz)
    return (float(width / npd_x), float(width / npd_y), 0.0 if dimensions == 2 else float(width / Lz))


_HALO_EMPTY = (1.0, 0.0)


def halo_bands(domain, g, dimensions=3):
    """The ghost bands of `halo_rows` around ``domain`` for the layer fractions ``g = (gx, gy, gz)``: ``(bands,
    divided)`` -- ``bands`` a 3 x 8 float64 array, per axis the half-open intervals ``[below), [below, wrapped), [above),
    [above, wrapped)`` as ``lo, hi`` pairs, an empty one stored as ``[1, 0)``; ``divided`` three flags (uint32), 0 for an
    axis with ``lo == 0 and hi == 1`` (and for z when ``dimensions == 2``), which has no bands.  The one place the
    bounds are computed: the model compares against them and the GPU selection receives them as they are."""
    lo, hi = _domain_bounds(domain)
    if int(dimensions) not in (2, 3):
        raise ValueError("dimensions must be 2 or 3")
    g = tuple(float(v) for v in g)
    if len(g) != 3 or any(not (v >= 0.0 and v < float('inf')) for v in g):
        raise ValueError("the ghost layer fractions must be three finite values >= 0: %r" % (g,))
    bands = numpy.empty((3, 8), dtype=numpy.float64)
    bands[:, 0::2], bands[:, 1::2] = _HALO_EMPTY
    divided = numpy.zeros(3, dtype=numpy.uint32)
    for a in range(2 if int(dimensions) == 2 else 3):
        l, h, w = float(lo[a]), float(hi[a]), g[a]
        if l == 0.0 and h == 1.0:
            continue
        if 2.0 * w > 1.0 - (h - l):
            raise ValueError("the ghost layer would show a particle twice on axis %s: 2 * %r > 1 - (%r - %r)"
                             % ('xyz'[a], w, h, l))
        divided[a] = 1
        bands[a, 0:2] = max(l - w, 0.0), l
        if l - w < 0.0:
            bands[a, 2:4] = (l - w) + 1.0, 1.0
        bands[a, 4:6] = h, min(h + w, 1.0)
        if h + w > 1.0:
            bands[a, 6:8] = 0.0, (h + w) - 1.0
    return bands, divided


# the slots of an axis' four bands in halo_bands' order, and the number of box vectors each adds
_HALO_BAND_SHIFT = (0, -1, 0, 1)


def _ghost_arg(box, ghost, dimensions):
    """``ghost`` of `halo_rows` / ``read_frame_device``: a width (a real distance) or three fractions -> fractions."""
    if isinstance(ghost, (int, float, numpy.integer, numpy.floating)):
        return ghost_fractions(box, ghost, dimensions)
    g = tuple(float(v) for v in ghost)
    if len(g) != 3:
        raise ValueError("ghost is a width or three fractions (gx, gy, gz)")
    return g


def halo_rows(position, box, domain, ghost, dimensions=3):
    """A cell plus the ghost layer its neighbours reach: ``(owned, ghost_rows, shift)`` -- the definition the GPU
    selection (`pgsd.fl.PGSDFile.select_halo_device`, ``read_frame_device(domain=..., ghost=...)``) equals exactly.

    ``owned`` is `domain_rows`.  ``ghost`` is the layer's width as a real distance (`ghost_fractions` turns it into
    fractions, like HOOMD's ``r_ghost``) or three fractions ``(gx, gy, gz)``.  With ``f[a]`` the wrapped fractional
    coordinate `domain_rows` computes, an axis that the domain does not divide (``lo == 0 and hi == 1``; z when
    ``dimensions == 2``) has no bands and every ``f`` counts as inside on it.  A divided axis has four half-open bands,
    whose bounds `halo_bands` computes once in float64::

        below            [max(lo - g, 0), lo)      shift  0
        below, wrapped   [(lo - g) + 1, 1)         shift -1    (when lo - g < 0)
        above            [hi, min(hi + g, 1))      shift  0
        above, wrapped   [0, (hi + g) - 1)         shift +1    (when hi + g > 1)

    A row's state on an axis is the first match of: inside (``lo <= f < hi``), the bands in this order, else out.  A
    row is a ghost when it is inside or in a band on every axis and in a band on at least one; ``ghost_rows`` are those
    rows, ascending (int64 like ``owned``), disjoint from ``owned``.  ``shift`` (``len(ghost_rows) x 3`` int32) holds
    each axis' band shift, 0 where the axis is inside: the number of box vectors to add so that the ghost lies next to
    the cell, ``r' = r + sx*a1 + sy*a2 + sz*a3`` with HOOMD's lattice vectors ``a1 = (Lx, 0, 0)``, ``a2 = (xy*Ly, Ly,
    0)``, ``a3 = (xz*Lz, yz*Lz, Lz)``.  Nothing in the library applies it.

    A layer that would show a particle twice -- ``2*g > 1 - (hi - lo)`` on a divided axis -- raises ValueError;
    ``g == 0`` on every axis gives no ghosts."""
    bands, divided = halo_bands(domain, _ghost_arg(box, ghost, dimensions), dimensions)
    lo, hi = _domain_bounds(domain)
    f = _wrapped_fractions(position, box, dimensions)
    n = f[0].shape[0]
    owned = numpy.ones(n, dtype=bool)
    reached = numpy.ones(n, dtype=bool)         # inside or in a band on every axis so far
    in_band = numpy.zeros(n, dtype=bool)        # in a band on at least one
    shift = numpy.zeros((n, 3), dtype=numpy.int32)
    for a in range(len(f)):
        inside = (lo[a] <= f[a]) & (f[a] < hi[a])
        owned &= inside
        if not divided[a]:
            continue
        open_ = ~inside                         # no earlier state has matched
        here = numpy.zeros(n, dtype=bool)
        for slot in range(4):
            hit = open_ & (bands[a, 2 * slot] <= f[a]) & (f[a] < bands[a, 2 * slot + 1])
            shift[hit, a] = _HALO_BAND_SHIFT[slot]
            here |= hit
            open_ &= ~hit
        reached &= inside | here
        in_band |= here
    ghost_rows = numpy.flatnonzero(reached & in_band)
    return numpy.flatnonzero(owned), ghost_rows, shift[ghost_rows]


_ORDER_MAX_AXIS_CELLS = 1024


def _order_cells(cells, dimensions):
    c = tuple(int(v) for v in cells)
    if len(c) != 3 or any(v < 1 or v > _ORDER_MAX_AXIS_CELLS for v in c):
        raise ValueError("a cell grid takes three counts (cx, cy, cz), each 1 to %d: %r" % (_ORDER_MAX_AXIS_CELLS, cells))
    if int(dimensions) == 2 and c[2] != 1:
        raise ValueError("dimensions == 2 takes cz == 1: z is not looked at")
    return c


def cell_ids(position, box, cells, dimensions=3):
    """The cell of every row of ``position`` (N x 3) in a uniform ``cells = (cx, cy, cz)`` grid over the box: an int64
    array, the definition the GPU ordering (`pgsd.fl.PGSDFile.order_rows_by_cell_device`,
    ``read_frame_device(cell_order=...)``) equals exactly.

    With ``f[a]`` the wrapped fraction `domain_rows` compares, ``i_a = min(int(f[a] * c_a), c_a - 1)`` in float64 and
    ``id = i_x + cx * (i_y + cy * i_z)`` -- x fastest, like `domain_grid`'s ranks.  Each count is 1 to 1024;
    ``dimensions == 2`` needs ``cz == 1`` and does not look at z.  A row whose fraction is NaN on an axis that takes part
    (NaN or infinite coordinates) gets ``cx * cy * cz``, the "nowhere" id, which sorts behind every cell.  The ``min``
    never binds: ``f <= 1 - 2**-53`` and for every ``c <= 1024`` the float64 product ``f * c`` rounds below ``c``."""
    c = _order_cells(cells, dimensions)
    f = _wrapped_fractions(position, box, dimensions)
    rows = f[0].shape[0]
    somewhere = numpy.ones(rows, dtype=bool)
    ids = numpy.zeros(rows, dtype=numpy.int64)
    stride = 1
    for a in range(len(f)):
        ok = f[a] == f[a]
        somewhere &= ok
        ids += numpy.minimum((numpy.where(ok, f[a], 0.0) * c[a]).astype(numpy.int64), c[a] - 1) * stride
        stride *= c[a]
    ids[~somewhere] = c[0] * c[1] * c[2]
    return ids


def cell_order(position, box, rows, cells, dimensions=3, n_owned=None):
    """``(rows_sorted, cell_sorted, perm)``: the row list ``rows`` of ``position`` ordered by cell -- a stable sort
    (``numpy.argsort(kind='stable')``) on ``cell_ids(position[rows], box, cells, dimensions)``, so the rows of one cell
    keep their relative order (ascending file rows for a selection's list).  ``rows_sorted = rows[perm]`` and
    ``cell_sorted`` are int64, ``perm`` the permutation applied.

    With ``n_owned`` the owned run ``rows[:n_owned]`` and the ghost run ``rows[n_owned:]`` of `halo_rows` are sorted
    separately and stay in that order; each run's ids ascend on their own, and `halo_rows`' shift rows are permuted with
    ``perm[n_owned:] - n_owned``.  An entry outside ``position`` raises ValueError."""
    p = numpy.asarray(position)
    p = p.reshape(-1, 3) if p.size else numpy.zeros((0, 3))
    rows = numpy.asarray(rows, dtype=numpy.int64).reshape(-1)
    n = rows.shape[0]
    n_owned = n if n_owned is None else int(n_owned)
    if n_owned < 0 or n_owned > n:
        raise ValueError("n_owned exceeds the number of entries: %r of %d" % (n_owned, n))
    _order_cells(cells, dimensions)
    if n and (rows.min() < 0 or rows.max() >= p.shape[0]):
        raise ValueError("an entry of the row list lies outside the position array")
    ids = cell_ids(p[rows], box, cells, dimensions)
    perm = numpy.concatenate((numpy.argsort(ids[:n_owned], kind='stable'),
                              numpy.argsort(ids[n_owned:], kind='stable') + n_owned)).astype(numpy.int64)
    return rows[perm], ids[perm], perm


def cell_grid_for(box, width, dimensions=3):
    """``(cx, cy, cz)``: the largest cell counts whose cells are no narrower than the real distance ``width`` (an
    interaction range, a neighbour-search cell) -- ``c_a = clamp(floor(1 / g_a), 1, 1024)`` with ``g =``
    `ghost_fractions` ``(box, width, dimensions)``, the width as a fraction of the box's nearest plane distance on each
    axis; ``cz == 1`` when ``dimensions == 2``.  A width of 0 gives 1024 on every axis that takes part."""
    g = ghost_fractions(box, width, dimensions)
    counts = []
    for a in range(3):
        if a == 2 and int(dimensions) == 2:
            counts.append(1)
        elif g[a] > 0.0:
            counts.append(int(min(max(numpy.floor(1.0 / g[a]), 1.0), float(_ORDER_MAX_AXIS_CELLS))))
        else:
            counts.append(_ORDER_MAX_AXIS_CELLS)
    return tuple(counts)


_WHERE_MAX_TERMS = 4
_WHERE_SET_BITS = 64


def _where_terms(where, types=None):
    """The terms of a group predicate (`where_rows`), checked and in the dict's order: ``(name, column, lo, hi, mask)``
    per term -- ``mask`` is ``None`` for a range (``lo`` / ``hi``: float or ``None`` for unbounded), else the 64-bit
    set mask (``lo`` and ``hi`` are ``None``).  ValueError for everything `where_rows` lists."""
    if not isinstance(where, dict):
        raise ValueError("where must be a dict of attribute -> (lo, hi) range or list of integers")
    if len(where) > _WHERE_MAX_TERMS:
        raise ValueError("where takes at most %d terms" % _WHERE_MAX_TERMS)
    terms = []
    for key, value in where.items():
        name, column = key if isinstance(key, tuple) and len(key) == 2 else (key, 0)
        if name == 'type':
            if column != 0 or isinstance(value, tuple) or isinstance(value, str):
                raise ValueError("'type' takes a list of type names")
            names = list(types) if types is not None else []
            unknown = [t for t in value if t not in names]
            if unknown:
                raise ValueError("unknown particle type %r (types: %r)" % (unknown[0], names))
            name, value = 'typeid', [names.index(t) for t in value]
        if not isinstance(name, str) or name not in _PARTICLE_FIELDS:
            raise ValueError("%r is not a per-particle attribute of ParticleData" % (name,))
        dt, M = _PARTICLE_FIELDS[name][:2]
        column = int(column)
        if not 0 <= column < M:
            raise ValueError("particles/%s has %d column(s): no column %d" % (name, M, column))
        if isinstance(value, tuple):
            if len(value) != 2:
                raise ValueError("a range is a pair (lo, hi): %r" % (value,))
            lo, hi = (None if v is None else float(v) for v in value)
            terms.append((name, column, lo, hi, None))
        elif isinstance(value, (list, set, frozenset)):
            if numpy.dtype(dt).kind not in 'iu':
                raise ValueError("particles/%s holds floats: a set needs an integer attribute" % name)
            mask = 0
            for member in value:
                if int(member) != member or not 0 <= int(member) < _WHERE_SET_BITS:
                    raise ValueError("set members are integers in [0, %d): %r" % (_WHERE_SET_BITS, member))
                mask |= 1 << int(member)
            terms.append((name, column, None, None, mask))
        else:
            raise ValueError("a term is a (lo, hi) tuple or a list / set of integers: %r" % (value,))
    return terms


def _where_term_keeps(x, lo, hi, mask):
    """One term of `where_rows` over the values ``x`` of its column: a bool per row."""
    if mask is not None:
        small = (x >= 0) & (x < _WHERE_SET_BITS)
        bits = numpy.uint64(mask) >> numpy.where(small, x, 0).astype(numpy.uint64)
        return small & ((bits & numpy.uint64(1)) != 0)
    v = x.astype(numpy.float64)
    keep = ~numpy.isnan(v)
    with numpy.errstate(invalid='ignore'):
        if lo is not None:
            keep &= numpy.float64(lo) <= v
        if hi is not None:
            keep &= v < numpy.float64(hi)
    return keep


def where_rows(arrays, where, types=None):
    """The rows that satisfy EVERY term of ``where``, ascending (int32): the definition the GPU selection
    (`pgsd.fl.PGSDFile.select_where_device`, ``read_frame_device(where=...)``) matches exactly.

    Args:
        arrays (dict): attribute name -> ``N (x M)`` host array (all of the same N).
        where (dict): at most 4 terms.  A key is an attribute name of `ParticleData` (column 0) or a pair
            ``(name, column)``; ``'type'`` is ``'typeid'`` with a list of type names looked up in ``types``.  A value is

            * a range, the tuple ``(lo, hi)`` with ``None`` for unbounded: with ``v = float64(x)`` (exact for float32,
              int32 and uint32) the row is kept iff ``lo <= v < hi``.  NaN is never kept, ``-0.0 >= 0.0`` holds as in
              numpy, ``lo >= hi`` selects nothing (and so does a bound that is NaN);
            * a set, a list or set of integers in [0, 64), on integer attributes only (``typeid``, ``body``, ``image``
              columns): the row is kept iff ``0 <= x < 64`` and ``x`` is a member.  Negative values never match.

            An empty dict selects every row.
        types (list): the frame's type names, for ``'type'``.

    ValueError: an unknown attribute or type name, a column the attribute does not have, a set on a float attribute, a
    set member outside [0, 64), more than 4 terms.
    """
    terms = _where_terms(where, types)
    for name in set(t[0] for t in terms):
        if name not in arrays or arrays[name] is None:
            raise ValueError("arrays holds no '%s'" % name)
    first = next((a for a in arrays.values() if a is not None), None)
    N = 0 if first is None else int(numpy.asarray(first).shape[0])
    keep = numpy.ones(N, dtype=bool)
    for name, column, lo, hi, mask in terms:
        a = numpy.asarray(arrays[name])
        if a.shape[0] != N:
            raise ValueError("'%s' has %d rows, expected %d" % (name, a.shape[0], N))
        a = a.reshape(N, a.shape[1] if a.ndim == 2 else 1)      # (not -1: a frame may hold no particle)
        if column >= a.shape[1]:
            raise ValueError("'%s' has %d column(s): no column %d" % (name, a.shape[1], column))
        if mask is not None and a.dtype.kind not in 'iu':
            raise ValueError("'%s' holds floats: a set needs integers" % name)
        keep &= _where_term_keeps(a[:, column], lo, hi, mask)
    return numpy.flatnonzero(keep).astype(numpy.int32)


def _particle_arrays(particles):
    """The per-particle arrays a `ParticleData` holds, by name (`where_rows`'s ``arrays``)."""
    return dict((name, getattr(particles, name)) for name in _PARTICLE_FIELDS if getattr(particles, name, None) is not None)


# ---- frame statistics: the definition the GPU reduction (`pgsd.fl.PGSDFile.chunk_stats_device`) equals exactly
_STATS_LANES = 256          # the row layout of the selection kernels: a tile of 4096 entries, lane k % 256,
_STATS_STEPS = 16           # step (k % 4096) / 256
_STATS_TILE = _STATS_LANES * _STATS_STEPS
_STATS_TYPES = (numpy.float32, numpy.float64, numpy.int32, numpy.uint32)
_STATS_FIELDS = ('position', 'velocity', 'density', 'pressure', 'energy')


class FieldStats(object):
    """Per-column statistics of a per-particle array (`column_stats`): arrays of one entry per column.

    Attributes:
        count, nan, inf (int64): the entries, those that are NaN, those that are +-infinity.
        min, max (float64): over the entries that are no NaN (infinities take part); ``+inf`` / ``-inf`` when there is
            none.  The sign of a zero is not specified.
        sum (float64): the sum of the finite entries in `column_stats`' order.
        mean (property): ``sum / (count - nan - inf)``, NaN where no entry is finite.

    With ``norm2`` the last column is the squared norm of the rows: ``max[-1]`` is the square of the largest speed.
    """

    __slots__ = ('count', 'nan', 'inf', 'min', 'max', 'sum')

    def __init__(self, count, nan, inf, min, max, sum):
        self.count = numpy.asarray(count, dtype=numpy.int64)
        self.nan = numpy.asarray(nan, dtype=numpy.int64)
        self.inf = numpy.asarray(inf, dtype=numpy.int64)
        self.min = numpy.asarray(min, dtype=numpy.float64)
        self.max = numpy.asarray(max, dtype=numpy.float64)
        self.sum = numpy.asarray(sum, dtype=numpy.float64)

    @property
    def mean(self):
        finite = self.count - self.nan - self.inf
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(finite > 0, self.sum / numpy.maximum(finite, 1), numpy.nan)

    def __repr__(self):
        return "FieldStats(count=%r, nan=%r, inf=%r, min=%r, max=%r, sum=%r)" % tuple(
            getattr(self, name).tolist() for name in self.__slots__)


def _block_tree(p):
    """The block tree over the last axis (256 lane sums): inside each run of 64 lanes ``p[i] += p[i + h]`` for
    ``h = 32 .. 1``, then ``(w0 + w1) + (w2 + w3)``."""
    w = p.reshape(p.shape[:-1] + (_STATS_LANES // 64, 64))
    for h in (32, 16, 8, 4, 2, 1):
        w = w[..., :h] + w[..., h:2 * h]
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _ordered_sum(v):
    """The sum of the float64 values ``v`` (entries that do not count replaced by ``+0.0``) in `column_stats`' order."""
    n = v.shape[0]
    tiles = (n + _STATS_TILE - 1) // _STATS_TILE
    a = numpy.zeros(tiles * _STATS_TILE, dtype=numpy.float64)
    a[:n] = v
    a = a.reshape(tiles, _STATS_STEPS, _STATS_LANES)
    lane = numpy.zeros((tiles, _STATS_LANES), dtype=numpy.float64)
    for step in range(_STATS_STEPS):
        lane = lane + a[:, step, :]
    tile_sums = _block_tree(lane)                               # one sum per tile
    rounds = (tiles + _STATS_LANES - 1) // _STATS_LANES
    b = numpy.zeros(rounds * _STATS_LANES, dtype=numpy.float64)
    b[:tiles] = tile_sums
    b = b.reshape(rounds, _STATS_LANES)
    lane = numpy.zeros(_STATS_LANES, dtype=numpy.float64)
    for r in range(rounds):
        lane = lane + b[r]
    return float(_block_tree(lane))


def column_stats(values, rows=None, norm2=False):
    """Per-column statistics of ``values``: the definition the GPU reduction (`pgsd.fl.PGSDFile.chunk_stats_device`,
    `HOOMDTrajectory.frame_stats_device`) equals exactly, the sums bit for bit.

    Args:
        values: an ``N`` or ``N x M`` array of float32, float64, int32 or uint32, ``M <= 4``.
        rows: ``None``, or row indices in any order, repeats allowed: the statistics of ``values[rows]`` in list order.
        norm2 (bool): append one column (float arrays with ``M == 3`` only) whose per-row value is
            ``(x*x + y*y) + z*z`` in float64, in exactly that association and without a fused multiply-add.  Its ``max``
            is the square of the largest speed; a row with a NaN component counts in ``nan``, a row whose value is
            infinite in ``inf``.

    Every element is first converted to float64 (exact for all four types).  `FieldStats` says what is returned.  **The
    order of the sum** is the row layout of the selection kernels: entry ``k`` (of the list, or row ``k``) belongs to
    tile ``k // 4096``, lane ``k % 256``, step ``(k % 4096) // 256``.

    1. A lane starts at ``+0.0`` and adds its 16 entries in step order; an entry that is not finite, or lies past the
       end, is ``+0.0`` (the identity: a running sum that starts at ``+0.0`` is never ``-0.0``).
    2. The 256 lane sums of a tile are combined by the block tree: inside each of the four waves (lanes ``64 w ..
       64 w + 63``) ``p[i] += p[i + h]`` for ``h = 32, 16, 8, 4, 2, 1``, then ``(w0 + w1) + (w2 + w3)``.
    3. The tile sums are combined the same way: lane ``t`` starts at ``+0.0`` and adds tiles ``t, t + 256, ...`` in
       that order, then the block tree.

    ValueError: another element type, more than two dimensions, ``M`` of 0 or above 4, ``norm2`` on integers or with
    ``M != 3``, a row index outside ``[0, N)``.
    """
    values = numpy.asarray(values)
    if values.dtype.type not in _STATS_TYPES:
        raise ValueError("statistics take float32, float64, int32 or uint32 arrays: %s" % values.dtype)
    if values.ndim not in (1, 2):
        raise ValueError("statistics take an N or N x M array")
    N = values.shape[0]
    M = values.shape[1] if values.ndim == 2 else 1
    if not 1 <= M <= 4:
        raise ValueError("statistics take 1 to 4 columns: %d" % M)
    if norm2 and (values.dtype.kind != 'f' or M != 3):
        raise ValueError("norm2 needs a float array of three columns")
    values = values.reshape(N, M)
    if rows is not None:
        rows = numpy.asarray(rows).reshape(-1)
        if rows.size and rows.dtype.kind not in 'iu':
            raise ValueError("rows holds integer row indices")
        rows = rows.astype(numpy.int64)
        if rows.size and (rows.min() < 0 or rows.max() >= N):
            raise ValueError("an entry of the row list lies outside the array")
        values = values[rows]
    v = values.astype(numpy.float64)
    if norm2:
        with numpy.errstate(over='ignore', invalid='ignore'):
            q = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        v = numpy.concatenate([v, q.reshape(-1, 1)], axis=1)
    n, C = v.shape
    is_nan, is_inf = numpy.isnan(v), numpy.isinf(v)
    lo, hi, total = numpy.empty(C), numpy.empty(C), numpy.empty(C)
    for c in range(C):
        kept = v[~is_nan[:, c], c]
        lo[c] = kept.min(initial=numpy.inf)
        hi[c] = kept.max(initial=-numpy.inf)
        total[c] = _ordered_sum(numpy.where(is_nan[:, c] | is_inf[:, c], 0.0, v[:, c]))
    return FieldStats(numpy.full(C, n), is_nan.sum(axis=0), is_inf.sum(axis=0), lo, hi, total)


def _stats_norm2(dtype, M):
    """Does a field of this element type and width get the norm column?"""
    return numpy.dtype(dtype).kind == 'f' and M == 3


def _stats_fields(fields):
    """The field names of a statistics call, checked."""
    names = [fields] if isinstance(fields, str) else list(fields)
    for name in names:
        if not isinstance(name, str) or name not in _PARTICLE_FIELDS:
            raise ValueError("%r is not a per-particle attribute of ParticleData" % (name,))
    return names


def frame_stats(frame_or_arrays, fields=_STATS_FIELDS, where=None, types=None, domain=None, box=None, dimensions=3):
    """`column_stats` of the per-particle arrays ``fields`` over a selection: the host twin of
    `HOOMDTrajectory.frame_stats_device`, which equals it exactly.

    Args:
        frame_or_arrays: a `Frame` (``types``, ``box`` and ``dimensions`` default to its own) or a dict of attribute
            name -> ``N (x M)`` host array.
        fields: attribute names of `ParticleData`.
        where (dict): a group predicate, as `where_rows` takes it.
        domain (`Domain`): a cell, as `domain_rows` takes it, over ``arrays['position']`` and ``box``.

    With ``where`` and ``domain`` the rows satisfy both; with neither the statistics are those of every row.  Float
    fields of three columns get the ``norm2`` column.  Returns a dict from field name to `FieldStats`.

    ValueError: what `where_rows`, `domain_rows` and `column_stats` refuse; a field the arrays do not hold; a domain
    without box or position.
    """
    if hasattr(frame_or_arrays, 'particles'):
        frame = frame_or_arrays
        arrays = _particle_arrays(frame.particles)
        types = frame.particles.types if types is None else types
        box = frame.configuration.box if box is None else box
        if frame.configuration.dimensions is not None:
            dimensions = int(frame.configuration.dimensions)
    else:
        arrays = dict((k, v) for k, v in frame_or_arrays.items() if v is not None)
    names = _stats_fields(fields)
    rows = None
    if where is not None:
        rows = where_rows(arrays, where, types)
    if domain is not None:
        if box is None or 'position' not in arrays:
            raise ValueError("a domain needs box and the 'position' array")
        inside = domain_rows(arrays['position'], box, domain, dimensions)
        rows = inside if rows is None else numpy.intersect1d(rows, inside)
    out = OrderedDict()
    for name in names:
        if name not in arrays:
            raise ValueError("arrays holds no '%s'" % name)
        a = numpy.asarray(arrays[name])
        out[name] = column_stats(a, rows, norm2=_stats_norm2(a.dtype, a.shape[1] if a.ndim == 2 else 1))
    return out


# ---- conservation sums: the definition the GPU reduction (`pgsd.fl.PGSDFile.frame_moments_device`) equals exactly
_MOMENTS_QUANTITIES = 9     # mass, momentum x 3, kinetic, internal, first moment x 3
_MOMENTS_MAX_TYPES = 4      # types per call (and per launch)
_MOMENTS_INPUTS = (('mass', 1, 1.0), ('velocity', 3, (0.0, 0.0, 0.0)), ('energy', 1, 0.0), ('position', 3, (0.0, 0.0, 0.0)))


class Moments(object):
    """Conservation sums per particle type (`particle_moments`): arrays of one entry (or one row) per type.

    Attributes:
        count, bad (int64, T): the entries of the type, and those of them at which at least one of the nine per-entry
            values is not finite.
        other (int): the entries of no type of the call.
        mass, kinetic, internal (float64, T): ``sum m``, ``sum (0.5 m) |v|^2``, ``sum m e`` (``energy`` is specific).
        momentum, first_moment (float64, T x 3): ``sum m v``, ``sum m x``.
        centre_of_mass, mean_velocity (properties, T x 3): ``first_moment / mass`` and ``momentum / mass``, NaN where
            the mass is 0.

    Every sum is over the finite values only and in `column_stats`' order.
    """

    __slots__ = ('count', 'bad', 'other', 'mass', 'momentum', 'kinetic', 'internal', 'first_moment')

    def __init__(self, count, bad, other, mass, momentum, kinetic, internal, first_moment):
        self.count = numpy.asarray(count, dtype=numpy.int64).reshape(-1)
        T = self.count.shape[0]
        self.bad = numpy.asarray(bad, dtype=numpy.int64).reshape(T)
        self.other = int(other)
        self.mass = numpy.asarray(mass, dtype=numpy.float64).reshape(T)
        self.momentum = numpy.asarray(momentum, dtype=numpy.float64).reshape(T, 3)
        self.kinetic = numpy.asarray(kinetic, dtype=numpy.float64).reshape(T)
        self.internal = numpy.asarray(internal, dtype=numpy.float64).reshape(T)
        self.first_moment = numpy.asarray(first_moment, dtype=numpy.float64).reshape(T, 3)

    @classmethod
    def from_sums(cls, count, bad, other, sums):
        """From the ``T x 9`` table of sums in the order of the per-entry values."""
        s = numpy.asarray(sums, dtype=numpy.float64).reshape(-1, _MOMENTS_QUANTITIES)
        return cls(count, bad, other, s[:, 0].copy(), s[:, 1:4].copy(), s[:, 4].copy(), s[:, 5].copy(), s[:, 6:9].copy())

    @property
    def sums(self):
        """The ``T x 9`` table of sums in the order of the per-entry values."""
        return numpy.concatenate([self.mass[:, None], self.momentum, self.kinetic[:, None], self.internal[:, None],
                                  self.first_moment], axis=1)

    @property
    def centre_of_mass(self):
        return self._per_mass(self.first_moment)

    @property
    def mean_velocity(self):
        return self._per_mass(self.momentum)

    def _per_mass(self, a):
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(self.mass[:, None] != 0, a / self.mass[:, None], numpy.nan)

    def total(self):
        """All types as one: a `Moments` of one row whose sums are the types' added in ascending type order by plain
        float64 additions; ``other`` stays."""
        s = self.sums
        acc = numpy.zeros(_MOMENTS_QUANTITIES, dtype=numpy.float64)
        for t in range(s.shape[0]):
            acc = s[t].copy() if t == 0 else acc + s[t]
        return Moments.from_sums([int(self.count.sum())], [int(self.bad.sum())], self.other, acc)

    @staticmethod
    def concatenate(parts, n_entries):
        """The `Moments` of consecutive groups of types (each over the same ``n_entries`` entries) as one."""
        count = numpy.concatenate([p.count for p in parts])
        return Moments.from_sums(count, numpy.concatenate([p.bad for p in parts]), int(n_entries) - int(count.sum()),
                                 numpy.concatenate([p.sums for p in parts], axis=0))

    def __repr__(self):
        return "Moments(%s)" % ', '.join("%s=%r" % (name, getattr(self, name).tolist() if name != 'other' else self.other)
                                         for name in self.__slots__)


def _list_rows(rows, N):
    """A row list as `column_stats` takes it, checked: int64 indices into ``N`` rows."""
    rows = numpy.asarray(rows).reshape(-1)
    if rows.size and rows.dtype.kind not in 'iu':
        raise ValueError("rows holds integer row indices")
    rows = rows.astype(numpy.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= N):
        raise ValueError("an entry of the row list lies outside the array")
    return rows


def particle_moments(mass, velocity, energy=None, position=None, typeid=None, type0=0, n_types=1, rows=None, N=None):
    """Mass, momentum, kinetic and internal energy and first moment per particle type: the definition the GPU reduction
    (`pgsd.fl.PGSDFile.frame_moments_device`, `HOOMDTrajectory.frame_moments_device`) equals exactly, the sums bit for
    bit.

    Args:
        mass (N), velocity (N x 3), energy (N), position (N x 3): float32 or float64 arrays, all that are arrays of one
            element type.  Each may instead be a default row -- a scalar, or three values -- that stands for N copies of
            it (converted to the arrays' element type; to float64 when there is no array), or ``None``: the schema's
            default, 1.0, (0, 0, 0), 0.0 and (0, 0, 0).
        typeid (N): uint32 or int32, or ``None``: no types, every entry belongs to the one group and ``n_types`` is 1.
        type0, n_types: the types ``[type0, type0 + n_types)``, ``1 <= n_types <= 4``.
        rows: as `column_stats` takes them: any order, repeats allowed, list order is entry order.
        N (int): the number of rows when no input is an array (else it must agree with them).

    Every element is converted to float64 first.  Per entry nine values, in float64, in exactly this association and
    without a fused multiply-add: ``m``; ``m * v[a]``; ``(0.5 * m) * ((vx*vx + vy*vy) + vz*vz)``; ``m * e``;
    ``m * x[a]``.  Per type ``t`` the result (`Moments`) holds the entries with ``typeid == t``, those of them with a
    value that is not finite (``inf * 0`` included), and per value the sum **in `column_stats`' order** of the sequence
    whose entry ``k`` is the value where ``typeid[k] == t`` and the value is finite, and ``+0.0`` otherwise: each value
    skips only its own non-finite entries, and a type with no entry has sums of ``+0.0``.  ``other`` counts the entries
    of no type of the range; a negative int32 id is one.

    ValueError: other element types, mixed float types, wrong shapes or lengths, ``n_types`` of 0 or above 4, a typeid
    of float elements, no typeid with ``n_types != 1``, no array and no ``N``, what `column_stats` refuses for ``rows``.
    """
    arrays, dt, n_rows = _moments_arrays(mass, velocity, energy, position, N)
    if not isinstance(n_types, (int, numpy.integer)) or not 1 <= n_types <= _MOMENTS_MAX_TYPES:
        raise ValueError("a call takes 1 to 4 types: %r" % (n_types,))
    if not isinstance(type0, (int, numpy.integer)) or not 0 <= type0 < 2 ** 32:
        raise ValueError("type0 is a type id: %r" % (type0,))
    if typeid is not None:
        typeid = numpy.asarray(typeid)
        if typeid.dtype.type not in (numpy.uint32, numpy.int32):
            raise ValueError("typeid holds uint32 or int32 elements: %s" % typeid.dtype)
        if typeid.ndim != 1:
            raise ValueError("typeid is an array of N values")
        if n_rows is not None and typeid.shape[0] != n_rows:
            raise ValueError("the arrays differ in their number of rows (typeid has %d)" % typeid.shape[0])
        n_rows = typeid.shape[0]
    elif n_types != 1:
        raise ValueError("without a typeid there is one group: n_types must be 1")
    n_rows, rows, n = _moments_rows(n_rows, rows)
    values, finite, all_finite = _moments_values(arrays, dt, rows, n)
    if typeid is None:
        group = numpy.zeros(n, dtype=numpy.int64)
    else:
        group = (typeid if rows is None else typeid[rows]).astype(numpy.int64) - int(type0)
    count, bad = numpy.zeros(n_types, numpy.int64), numpy.zeros(n_types, numpy.int64)
    sums = numpy.zeros((n_types, _MOMENTS_QUANTITIES), dtype=numpy.float64)
    for t in range(n_types):
        mine = group == t
        count[t], bad[t] = mine.sum(), (mine & ~all_finite).sum()
        for q in range(_MOMENTS_QUANTITIES):
            sums[t, q] = _ordered_sum(numpy.where(mine & finite[q], values[q], 0.0))
    return Moments.from_sums(count, bad, n - int(count.sum()), sums)


def _moments_arrays(mass, velocity, energy, position, N):
    """The four float inputs of `particle_moments` (and `cell_moments`), checked: ``(arrays, dt, n_rows)`` -- per name
    the array or the default row, the arrays' element type (``None`` without an array) and their number of rows
    (``N`` without an array)."""
    given = dict(zip(('mass', 'velocity', 'energy', 'position'), (mass, velocity, energy, position)))
    arrays, dt, n_rows = {}, None, None if N is None else int(N)
    for name, M, default in _MOMENTS_INPUTS:
        a = numpy.asarray(default if given[name] is None else given[name])
        if a.ndim == (1 if M == 1 else 2):          # an array of N rows
            if a.dtype.type not in (numpy.float32, numpy.float64):
                raise ValueError("moments take float32 or float64 arrays: %s is %s" % (name, a.dtype))
            if dt is not None and a.dtype != dt:
                raise ValueError("moments take arrays of one float type, not float32 and float64 mixed")
            if M == 3 and a.shape[1] != 3:
                raise ValueError("%s is an N x 3 array" % name)
            if n_rows is not None and a.shape[0] != n_rows:
                raise ValueError("the arrays differ in their number of rows (%s has %d)" % (name, a.shape[0]))
            dt, n_rows = a.dtype, a.shape[0]
        elif a.ndim != (0 if M == 1 else 1) or (M == 3 and a.shape[0] != 3) or a.dtype.kind not in 'fiu':
            raise ValueError("%s is %s" % (name, "an array of N values or one value" if M == 1 else
                                           "an N x 3 array or three values"))
        arrays[name] = a
    return arrays, dt, n_rows


def _moments_rows(n_rows, rows):
    """``(n_rows, rows, n)``: the number of rows settled, the row list checked, the number of entries."""
    if n_rows is None:
        raise ValueError("no input is an array: N says how many rows there are")
    if n_rows < 0:
        raise ValueError("N is a number of rows")
    if rows is not None:
        rows = _list_rows(rows, n_rows)
    return n_rows, rows, n_rows if rows is None else rows.shape[0]


def _moments_values(arrays, dt, rows, n, x=None):
    """The nine float64 values per entry of `particle_moments`: ``(values, finite, all_finite)``, nine arrays of ``n``
    values, the same of flags "is finite", and their conjunction.  The one place where the values are formed.  ``x``:
    three float64 arrays of ``n`` values that stand in for the position's columns (`component_moments`: the
    displacements from the root)."""
    dt = numpy.dtype(numpy.float64) if dt is None else dt

    def column(name, c):
        a, M = arrays[name], 1 if name in ('mass', 'energy') else 3
        if a.ndim == (1 if M == 1 else 2):
            a = a if M == 1 else a[:, c]
            return (a if rows is None else a[rows]).astype(numpy.float64)
        return numpy.full(n, numpy.float64(a.astype(dt).reshape(-1)[c]))

    m, e = column('mass', 0), column('energy', 0)
    v = [column('velocity', a) for a in range(3)]
    x = [column('position', a) for a in range(3)] if x is None else [numpy.asarray(c, dtype=numpy.float64) for c in x]
    with numpy.errstate(over='ignore', invalid='ignore', under='ignore'):
        values = ([m] + [m * v[a] for a in range(3)]
                  + [(0.5 * m) * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), m * e] + [m * x[a] for a in range(3)])
    finite = [numpy.isfinite(q) for q in values]
    all_finite = numpy.logical_and.reduce(finite) if n else numpy.zeros(0, dtype=bool)
    return values, finite, all_finite


# ---- cell fields: the definition the GPU reduction (`pgsd.fl.PGSDFile.cell_moments_device`) equals exactly
_CELLS_MAX_CELLS = 2 ** 20
_CELLS_PIECE = 1024          # entries of a piece of a cell's sum
_CELLS_LANES = 64


class CellMoments(object):
    """Conservation sums per grid cell (`cell_moments`): arrays of one entry (or one row) per cell, x fastest like
    `cell_ids`.

    Attributes:
        count, bad (int64, n_cells): the entries of the cell, and those of them at which at least one of the nine
            per-entry values is not finite.
        nowhere (int): the entries with the id ``n_cells``, summed nowhere.
        mass, kinetic, internal (float64, n_cells); momentum, first_moment (float64, n_cells x 3): as `Moments`'.
        grid: ``(cx, cy, cz)`` or ``None``; cell_volume (float): the box volume (in 2-D the area) over ``n_cells``, or
            ``None``.
        mean_velocity, centre_of_mass (properties, n_cells x 3): NaN where the mass is 0.
        density (property): ``mass / cell_volume``.

    Every sum is over the finite values only and in the cell's own order (`cell_moments`).
    """

    __slots__ = ('count', 'bad', 'nowhere', 'mass', 'momentum', 'kinetic', 'internal', 'first_moment', 'grid', 'cell_volume')

    def __init__(self, count, bad, nowhere, mass, momentum, kinetic, internal, first_moment, grid=None, cell_volume=None):
        self.count = numpy.asarray(count, dtype=numpy.int64).reshape(-1)
        T = self.count.shape[0]
        self.bad = numpy.asarray(bad, dtype=numpy.int64).reshape(T)
        self.nowhere = int(nowhere)
        self.mass = numpy.asarray(mass, dtype=numpy.float64).reshape(T)
        self.momentum = numpy.asarray(momentum, dtype=numpy.float64).reshape(T, 3)
        self.kinetic = numpy.asarray(kinetic, dtype=numpy.float64).reshape(T)
        self.internal = numpy.asarray(internal, dtype=numpy.float64).reshape(T)
        self.first_moment = numpy.asarray(first_moment, dtype=numpy.float64).reshape(T, 3)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.cell_volume = None if cell_volume is None else float(cell_volume)

    @classmethod
    def from_sums(cls, count, bad, nowhere, sums, grid=None, cell_volume=None):
        """From the ``n_cells x 9`` table of sums in the order of the per-entry values."""
        s = numpy.asarray(sums, dtype=numpy.float64).reshape(-1, _MOMENTS_QUANTITIES)
        return cls(count, bad, nowhere, s[:, 0].copy(), s[:, 1:4].copy(), s[:, 4].copy(), s[:, 5].copy(), s[:, 6:9].copy(),
                   grid, cell_volume)

    @property
    def sums(self):
        """The ``n_cells x 9`` table of sums in the order of the per-entry values."""
        return numpy.concatenate([self.mass[:, None], self.momentum, self.kinetic[:, None], self.internal[:, None],
                                  self.first_moment], axis=1)

    @property
    def centre_of_mass(self):
        return self._per_mass(self.first_moment)

    @property
    def mean_velocity(self):
        return self._per_mass(self.momentum)

    @property
    def density(self):
        if self.cell_volume is None:
            raise ValueError("the cell volume is not known: density needs a box (frame_cell_moments)")
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return self.mass / self.cell_volume

    def _per_mass(self, a):
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(self.mass[:, None] != 0, a / self.mass[:, None], numpy.nan)

    def as_grid(self, name):
        """Attribute or property ``name`` shaped ``(cz, cy, cx)`` (``(cz, cy, cx, 3)`` for a vector)."""
        if self.grid is None:
            raise ValueError("the grid is not known: as_grid needs cell counts (frame_cell_moments)")
        a = numpy.asarray(getattr(self, name))
        cx, cy, cz = self.grid
        return a.reshape((cz, cy, cx) + a.shape[1:])

    def __repr__(self):
        return "CellMoments(n_cells=%d, grid=%r, entries=%d, nowhere=%d)" % (self.count.shape[0], self.grid,
                                                                            int(self.count.sum()), self.nowhere)


def _cell_list(cell, n_cells):
    """A list of cell ids, checked: int64 ids in ``[0, n_cells]``."""
    if not isinstance(n_cells, (int, numpy.integer)) or not 1 <= n_cells <= _CELLS_MAX_CELLS:
        raise ValueError("a grid holds 1 to 2^20 cells: %r" % (n_cells,))
    cell = numpy.asarray(cell).reshape(-1)
    if cell.size and cell.dtype.kind not in 'iu':
        raise ValueError("cell holds integer cell ids")
    cell = cell.astype(numpy.int64)
    if cell.size and (cell.min() < 0 or cell.max() > n_cells):
        raise ValueError("a cell id lies outside [0, n_cells]")
    return cell


def cell_offsets(cell_sorted, n_cells):
    """The CSR offsets of a list of cell ids in cell order: int64, ``n_cells + 2`` entries,
    ``numpy.searchsorted(cell_sorted, arange(n_cells + 2), side='left')``.  Entry ``c`` is the first position of cell
    ``c`` (``n_cells`` is `cell_ids`' "nowhere" id) and the last entry is the list's length.  The definition of
    `pgsd.fl.PGSDFile.cell_offsets_device`.  ValueError for ids that descend or lie outside ``[0, n_cells]``."""
    cell = _cell_list(cell_sorted, n_cells)
    if cell.size > 1 and (cell[1:] < cell[:-1]).any():
        raise ValueError("the cell ids descend: the list is not in cell order")
    return numpy.searchsorted(cell, numpy.arange(int(n_cells) + 2, dtype=numpy.int64), side='left').astype(numpy.int64)


def _cell_ordered_sums(values, cell_sorted, offs, n_cells):
    """Per cell the sum of ``values`` (float64, in cell order, non-finite values replaced by ``+0.0`` already) in the
    order of `cell_moments`: one ``lanes[piece, lane]`` array and a loop over the 16 steps, the wave tree, then the
    pieces of every cell in sequence."""
    k = numpy.nonzero(cell_sorted < n_cells)[0]
    within = k - offs[cell_sorted[k]]                        # the entry's place in its cell
    per_cell = (numpy.diff(offs[:n_cells + 1]) + _CELLS_PIECE - 1) // _CELLS_PIECE
    piece0 = numpy.concatenate(([0], numpy.cumsum(per_cell)))  # the first piece of every cell, all pieces numbered
    piece = piece0[cell_sorted[k]] + within // _CELLS_PIECE
    lane, step = within % _CELLS_LANES, (within % _CELLS_PIECE) // _CELLS_LANES
    lanes = numpy.zeros((int(piece0[-1]), _CELLS_LANES), dtype=numpy.float64)
    for t in range(_CELLS_PIECE // _CELLS_LANES):
        at = step == t      # (one entry per lane and step: the indexed add is one float64 addition per touched lane)
        lanes[piece[at], lane[at]] = lanes[piece[at], lane[at]] + values[k[at]]
    h = _CELLS_LANES // 2
    while h >= 1:
        lanes = lanes[:, :h] + lanes[:, h:2 * h]
        h //= 2
    pieces = lanes[:, 0]
    sums = numpy.zeros(n_cells, dtype=numpy.float64)
    for j in range(int(per_cell.max()) if n_cells and per_cell.size else 0):
        has = per_cell > j
        sums[has] = sums[has] + pieces[piece0[:-1][has] + j]
    return sums


def cell_moments(mass, velocity, energy=None, position=None, cell=None, n_cells=None, rows=None, N=None):
    """Mass, momentum, kinetic and internal energy and first moment per grid cell: the definition the GPU reduction
    (`pgsd.fl.PGSDFile.cell_moments_device`, `HOOMDTrajectory.cell_moments_device`) equals exactly, the sums bit for bit.

    Args:
        mass, velocity, energy, position, rows, N: exactly `particle_moments`', and so are the nine float64 values per
            entry.
        cell: an integer array with one id per **list entry** (per row without ``rows``), in ``[0, n_cells]``, in any
            order; ``n_cells`` is `cell_ids`' "nowhere" id.
        n_cells (int): the cells, 1 to 2^20.

    Per cell ``c < n_cells`` the result (`CellMoments`) holds the entries of the cell, those of them with a value that
    is not finite, and the nine sums; ``nowhere`` counts the entries with id ``n_cells``, which are summed nowhere.

    **The order of a cell's sum.**  The cell's entries are taken in list order (the order a stable sort by cell leaves
    them in); a value that is not finite counts as ``+0.0``, each value for itself.  The sequence is cut into pieces of
    1024 consecutive entries counted from the cell's first entry.  In a piece lane ``l`` of 64 starts at ``+0.0`` and adds
    the piece's entries ``l, l + 64, ..., l + 960`` in that order, an entry past the end being ``+0.0``; the 64 lane sums
    go through the wave tree of `column_stats`, ``p[i] += p[i + h]`` for ``h = 32 .. 1``; the cell's sum starts at
    ``+0.0`` and adds the piece sums in ascending piece order.  A cell without entries has sums of ``+0.0``.  No fused
    multiply-add anywhere.

    ValueError: what `particle_moments` refuses for its inputs; ``n_cells`` outside 1 to 2^20; ``cell`` of another
    length than the list, of non-integers or with an id outside ``[0, n_cells]``.
    """
    arrays, dt, n_rows = _moments_arrays(mass, velocity, energy, position, N)
    n_rows, rows, n = _moments_rows(n_rows, rows)
    if cell is None or n_cells is None:
        raise ValueError("cell_moments takes one cell id per entry (cell) and the number of cells (n_cells)")
    cell = _cell_list(cell, n_cells)
    n_cells = int(n_cells)
    if cell.shape[0] != n:
        raise ValueError("cell holds one id per list entry: %d ids for %d entries" % (cell.shape[0], n))
    values, finite, all_finite = _moments_values(arrays, dt, rows, n)
    perm = numpy.argsort(cell, kind='stable')
    cell_sorted = cell[perm]
    offs = cell_offsets(cell_sorted, n_cells)
    count = numpy.diff(offs[:n_cells + 1])
    bad = numpy.bincount(cell_sorted[~all_finite[perm]], minlength=n_cells + 1)[:n_cells] if n else numpy.zeros(n_cells, numpy.int64)
    sums = numpy.zeros((n_cells, _MOMENTS_QUANTITIES), dtype=numpy.float64)
    for q in range(_MOMENTS_QUANTITIES):
        sums[:, q] = _cell_ordered_sums(numpy.where(finite[q], values[q], 0.0)[perm], cell_sorted, offs, n_cells)
    return CellMoments.from_sums(count, bad, int(offs[n_cells + 1] - offs[n_cells]), sums)


def frame_cell_moments(frame_or_arrays, cells, centre=True, where=None, types=None, domain=None, box=None, dimensions=3):
    """`cell_moments` of a frame's ``mass``, ``velocity``, ``energy`` and ``position`` over a selection, per cell of a
    uniform ``cells = (cx, cy, cz)`` grid over the box: the host twin of `HOOMDTrajectory.cell_moments_device`, which
    equals it exactly.

    The rows come from `where_rows`, `domain_rows` or their intersection, as `frame_moments` forms them, and
    ``cell = cell_ids(position[rows], box, cells, dimensions)``; ``cx * cy * cz <= 2**20``.  ``cell_volume`` is the box
    volume (in 2-D the area) over the number of cells: the cells are equal in fractional coordinates and therefore in
    volume, in a triclinic box too.  A position that is stored nowhere puts every row into the origin's cell.
    ``centre=False`` leaves the position out of the sums (not out of the cells).  Returns a `CellMoments`.
    """
    if hasattr(frame_or_arrays, 'particles'):
        frame = frame_or_arrays
        arrays = _particle_arrays(frame.particles)
        types = frame.particles.types if types is None else types
        box = frame.configuration.box if box is None else box
        if frame.configuration.dimensions is not None:
            dimensions = int(frame.configuration.dimensions)
        N = int(frame.particles.N)
    else:
        arrays = dict((k, v) for k, v in frame_or_arrays.items() if v is not None)
        if not arrays:
            raise ValueError("arrays holds no per-particle array")
        N = len(next(iter(arrays.values())))
    if box is None:
        raise ValueError("a cell grid needs the box")
    grid = _order_cells(cells, dimensions)
    n_cells = grid[0] * grid[1] * grid[2]
    if n_cells > _CELLS_MAX_CELLS:
        raise ValueError("a grid holds at most 2^20 cells: %r" % (cells,))
    rows = None
    if where is not None:
        rows = where_rows(arrays, where, types)
    if domain is not None:
        if 'position' not in arrays:
            raise ValueError("a domain needs box and the 'position' array")
        inside = domain_rows(arrays['position'], box, domain, dimensions)
        rows = inside if rows is None else numpy.intersect1d(rows, inside)
    n = N if rows is None else len(rows)
    if arrays.get('position') is None:
        cell = numpy.repeat(cell_ids(numpy.zeros((1, 3), numpy.float32), box, grid, dimensions), n)
    else:
        p = numpy.asarray(arrays['position']).reshape(-1, 3)
        cell = cell_ids(p if rows is None else p[numpy.asarray(rows, dtype=numpy.int64)], box, grid, dimensions)
    got = cell_moments(arrays.get('mass'), arrays.get('velocity'), arrays.get('energy'),
                       arrays.get('position') if centre else None, cell=cell, n_cells=n_cells, rows=rows, N=N)
    b = numpy.asarray(box, dtype=numpy.float64).reshape(-1)
    got.grid = grid
    got.cell_volume = (b[0] * b[1] * (b[2] if int(dimensions) == 3 else 1.0)) / n_cells
    return got


# ---- neighbour census: the definition the GPU pair pass (`pgsd.fl.PGSDFile.neighbours_device`) equals exactly
_NEIGHBOURS_NONE = 0xFFFFFFFF       # no list position: `nearest` of an entry without a neighbour, `closest` of no pair
_NEIGHBOURS_COUNT_BINS = 257        # count_hist: 0 .. 255 neighbours, then 256 and more
_NEIGHBOURS_MAX_BINS = 1024         # pair_hist
_NEIGHBOURS_SUMMARY_WORDS = 8       # n, nowhere, pairs, count_min, count_max, closest, closest_rows[2]
_NEIGHBOURS_PAIRS_PER_STEP = 1 << 22


def pair_distance2(xi, xj, vectors, dimensions=3):
    """The squared distance of the pair ``i -> j`` under HOOMD's single-shift minimum image: the arithmetic of one pair of
    `particle_neighbours` and of the GPU pair kernel, float64 throughout (float32 positions are converted exactly, no
    fused multiply-add).

    ``xi``, ``xj``: ``... x 3`` positions that broadcast; ``vectors``: `box_vectors` ``(Lx, Ly, Lz, xy*Ly, xz*Lz,
    yz*Lz)``.  ``d = xj - xi`` per axis; then, z first (only if ``dimensions == 3``): if ``d_z >= Lz/2`` the vector
    ``(xz*Lz, yz*Lz, Lz)`` is subtracted from ``(d_x, d_y, d_z)``, else if ``d_z < -(Lz/2)`` it is added; y the same
    with ``Ly/2`` and ``(xy*Ly, Ly)`` on ``(d_x, d_y)``; x the same with ``Lx/2`` and ``Lx`` on ``d_x``.  With
    ``dimensions == 2`` ``d_z`` is 0 and z is never looked at.  ``d2 = (d_x*d_x + d_y*d_y) + d_z*d_z``.

    One shift per axis and no division: this is not the ``rint(d / L)`` fold of `displacement_vectors`.  It has HOOMD's
    range of validity -- a stored position more than one image outside the box is not folded fully, and its pairs are
    whatever this formula gives, here and on the GPU alike."""
    dx, dy, dz = pair_displacement(xi, xj, vectors, dimensions)
    with numpy.errstate(over='ignore', invalid='ignore'):
        return (dx * dx + dy * dy) + dz * dz


def pair_displacement(xi, xj, vectors, dimensions=3):
    """The displacement ``(dx, dy, dz)`` of the pair ``i -> j`` -- ``x_j - x_i`` under HOOMD's single-shift minimum image
    -- with exactly `pair_distance2`'s arithmetic, which is ``(dx*dx + dy*dy) + dz*dz`` of it: float64 throughout, float32
    positions converted exactly before the subtraction, z folded first (only if ``dimensions == 3``), then y, then x,
    one shift per axis; with ``dimensions == 2`` ``dz`` is 0 and z is never looked at.  The arithmetic of one pair of
    `sph_kernel_gradients` and of its GPU kernel."""
    dimensions = int(dimensions)
    if dimensions not in (2, 3):
        raise ValueError("dimensions must be 2 or 3")
    v = numpy.asarray(vectors, dtype=numpy.float64).reshape(-1)
    if v.shape[0] != 6:
        raise ValueError("box vectors hold six values (pgsd.hoomd.box_vectors)")
    a = numpy.asarray(xi).astype(numpy.float64)
    b = numpy.asarray(xj).astype(numpy.float64)
    with numpy.errstate(over='ignore', invalid='ignore'):
        dx = b[..., 0] - a[..., 0]
        dy = b[..., 1] - a[..., 1]
        if dimensions == 3:
            dz = b[..., 2] - a[..., 2]
            h = v[2] / 2
            up, down = dz >= h, dz < -h
            dx = numpy.where(up, dx - v[4], numpy.where(down, dx + v[4], dx))
            dy = numpy.where(up, dy - v[5], numpy.where(down, dy + v[5], dy))
            dz = numpy.where(up, dz - v[2], numpy.where(down, dz + v[2], dz))
        else:
            dz = numpy.zeros(numpy.broadcast(dx, dy).shape, dtype=numpy.float64)
        h = v[1] / 2
        up, down = dy >= h, dy < -h
        dx = numpy.where(up, dx - v[3], numpy.where(down, dx + v[3], dx))
        dy = numpy.where(up, dy - v[1], numpy.where(down, dy + v[1], dy))
        h = v[0] / 2
        up, down = dx >= h, dx < -h
        dx = numpy.where(up, dx - v[0], numpy.where(down, dx + v[0], dx))
        return dx, dy, dz


def _neighbour_range(r):
    r = float(r)
    if not (r > 0.0 and r < float('inf')):
        raise ValueError("the neighbour range must be finite and positive: %r" % (r,))
    return r


def neighbour_grid_for(box, r, dimensions=3):
    """``(cx, cy, cz)``: the grid `particle_neighbours` searches with for the range ``r`` -- `cell_grid_for` ``(box, r,
    dimensions)``, and while ``cx*cy*cz > 2**20`` (`cell_offsets`' limit) the largest count ``c`` replaced by
    ``(c + 1) // 2``, the lowest axis on a tie.  The coarsening only makes cells wider."""
    c = list(cell_grid_for(box, _neighbour_range(r), dimensions))
    while c[0] * c[1] * c[2] > _CELLS_MAX_CELLS:
        a = c.index(max(c))
        c[a] = (c[a] + 1) // 2
    return tuple(c)


def _neighbour_grid(box, r, cells, dimensions):
    """The grid of a neighbour search, checked (`particle_neighbours` lists what is refused)."""
    r = _neighbour_range(r)
    dimensions = int(dimensions)
    g = ghost_fractions(box, r, dimensions)
    for a in range(2 if dimensions == 2 else 3):
        if g[a] > 0.5:
            raise ValueError("the range %r exceeds half the box's nearest plane distance on axis %d: an image would "
                             "count twice" % (r, a))
    if cells is None:
        return neighbour_grid_for(box, r, dimensions)
    grid = _order_cells(cells, dimensions)
    widest = cell_grid_for(box, r, dimensions)
    for a in range(3):
        if grid[a] > widest[a]:
            raise ValueError("cells %r are narrower than the range %r on axis %d (at most %d cells)"
                             % (tuple(cells), r, a, widest[a]))
    if grid[0] * grid[1] * grid[2] > _CELLS_MAX_CELLS:
        raise ValueError("a grid holds at most 2^20 cells: %r" % (tuple(cells),))
    return grid


def neighbour_edges2(r, bins):
    """The ``bins + 1`` squared bin edges of `particle_neighbours`' ``pair_hist``, float64: ``(k * (r / bins))**2`` for
    ``k < bins`` and ``r*r`` for ``k == bins``.  Host arithmetic: the GPU receives these and never recomputes them."""
    r = _neighbour_range(r)
    bins = int(bins)
    if not 1 <= bins <= _NEIGHBOURS_MAX_BINS:
        raise ValueError("bins is 0 (no pair histogram) or 1 to %d: %r" % (_NEIGHBOURS_MAX_BINS, bins))
    w = numpy.float64(r) / numpy.float64(bins)
    e = numpy.arange(bins + 1, dtype=numpy.float64) * w
    e = e * e
    e[bins] = numpy.float64(r) * numpy.float64(r)
    return e


class Neighbours(object):
    """The neighbour census of a list in cell order (`particle_neighbours`).

    Attributes:
        r (float), bins (int), grid (``(cx, cy, cz)``), dimensions (int): what was asked.
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere).
        count (uint32), nearest2 (float64), nearest (uint32): per entry, in list order, the neighbours, the smallest
            squared distance among them (``+inf`` without one) and the smallest list position that attains it
            (``0xFFFFFFFF`` without one).  The five per-entry arrays are numpy arrays from the model; from the GPU they
            are ``None`` unless ``return_rows`` left them in GPU memory.
        n, nowhere (int): the entries, and those without a cell.
        pairs (int): the sum of ``count``: ORDERED pairs (at an exact half-box tie in a tilted box ``i -> j`` and
            ``j -> i`` may differ, so it need not be even).
        count_hist (uint64, 257): bin ``k < 256``: the entries that have a cell and ``k`` neighbours; bin 256: 256 or more.
        count_min, count_max (int): over the entries that have a cell (0 where there is none).
        closest2 (float): the smallest ``nearest2``; closest (int): the smallest list position that attains it
            (``0xFFFFFFFF``: no pair); closest_rows: that entry's row and its nearest's row (``None``: no pair).
        pair_hist (uint64, bins) or ``None``; edges2 (float64, bins + 1) or ``None``: `neighbour_edges2`.
        mean_count, isolated, closest_distance (properties); `rdf`.
    """

    __slots__ = ('r', 'bins', 'grid', 'dimensions', 'rows', 'cell', 'count', 'nearest2', 'nearest', 'n', 'nowhere', 'pairs',
                 'count_hist', 'count_min', 'count_max', 'closest2', 'closest', 'closest_rows', 'pair_hist', 'edges2')

    def __init__(self, r, bins, grid, dimensions, summary, closest2, rows=None, cell=None, count=None, nearest2=None,
                 nearest=None):
        """``summary``: the uint64 words of `pgsd_neighbours_device` -- n, nowhere, pairs, count_min, count_max, closest,
        the closest pair's two rows, the 257 words of ``count_hist``, then ``bins`` words of ``pair_hist``."""
        s = numpy.asarray(summary, dtype=numpy.uint64).reshape(-1)
        self.r, self.bins, self.dimensions = float(r), int(bins), int(dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        if s.shape[0] != _NEIGHBOURS_SUMMARY_WORDS + _NEIGHBOURS_COUNT_BINS + self.bins:
            raise ValueError("the summary holds %d words" % (_NEIGHBOURS_SUMMARY_WORDS + _NEIGHBOURS_COUNT_BINS + self.bins))
        self.n, self.nowhere, self.pairs, self.count_min, self.count_max, self.closest = (int(v) for v in s[:6])
        self.closest_rows = None if self.closest == _NEIGHBOURS_NONE else (int(s[6]), int(s[7]))
        self.count_hist = s[_NEIGHBOURS_SUMMARY_WORDS:_NEIGHBOURS_SUMMARY_WORDS + _NEIGHBOURS_COUNT_BINS].copy()
        self.pair_hist = s[_NEIGHBOURS_SUMMARY_WORDS + _NEIGHBOURS_COUNT_BINS:].copy() if self.bins else None
        self.edges2 = neighbour_edges2(self.r, self.bins) if self.bins else None
        self.closest2 = float(closest2)
        self.rows, self.cell, self.count, self.nearest2, self.nearest = rows, cell, count, nearest2, nearest

    @property
    def summary(self):
        """The uint64 words this was made from."""
        rows = (_NEIGHBOURS_NONE, _NEIGHBOURS_NONE) if self.closest_rows is None else self.closest_rows
        head = numpy.array([self.n, self.nowhere, self.pairs, self.count_min, self.count_max, self.closest, rows[0], rows[1]],
                           dtype=numpy.uint64)
        return numpy.concatenate([head, self.count_hist] + ([self.pair_hist] if self.bins else []))

    @property
    def mean_count(self):
        """Neighbours per entry that has a cell (NaN where there is none)."""
        somewhere = self.n - self.nowhere
        return self.pairs / somewhere if somewhere else float('nan')

    @property
    def isolated(self):
        """The entries that have a cell and no neighbour."""
        return int(self.count_hist[0])

    @property
    def closest_distance(self):
        return float(numpy.sqrt(self.closest2))

    def rdf(self, volume):
        """``(r_mid, g)``: the radial distribution function from ``pair_hist`` -- per bin the ordered pairs over what an
        ideal gas of the same density ``(n - nowhere) / volume`` gives, ``(n - nowhere) * density * shell``, with the
        shell volumes between the edges, ``4/3 pi (r_k+1^3 - r_k^3)`` (``pi (r_k+1^2 - r_k^2)`` and an area for
        ``dimensions == 2``).  Host arithmetic on the counts: not part of what the GPU equals exactly."""
        if not self.bins:
            raise ValueError("rdf needs the pair histogram (bins >= 1)")
        edges = numpy.sqrt(self.edges2)
        if self.dimensions == 2:
            shell = numpy.pi * (edges[1:] ** 2 - edges[:-1] ** 2)
        else:
            shell = 4.0 / 3.0 * numpy.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
        somewhere = self.n - self.nowhere
        with numpy.errstate(divide='ignore', invalid='ignore'):
            g = self.pair_hist.astype(numpy.float64) / (somewhere * (somewhere / float(volume)) * shell)
        return 0.5 * (edges[1:] + edges[:-1]), g

    def __repr__(self):
        return "Neighbours(r=%r, grid=%r, n=%d, nowhere=%d, pairs=%d, count=[%d, %d], closest2=%r)" % (
            self.r, self.grid, self.n, self.nowhere, self.pairs, self.count_min, self.count_max, self.closest2)


def _axis_offsets(c):
    """The cell offsets of one axis of `particle_neighbours`: -1 and +1 are the same cell at two cells."""
    return (0,) if c == 1 else (0, 1) if c == 2 else (-1, 0, 1)


def particle_neighbours(position, box, r, rows=None, cells=None, dimensions=3, bins=0):
    """The neighbour census of a row list inside the range ``r``: per entry the number of neighbours and the nearest one,
    and over the list the count histogram, the closest pair and -- with ``bins`` -- the pair histogram g(r) is made
    from.  The definition the GPU pair pass (`pgsd.fl.PGSDFile.neighbours_device`,
    `HOOMDTrajectory.frame_neighbours_device`) equals exactly: every result is an integer count or a minimum, so none
    depends on the order of traversal, and the arithmetic of one pair is `pair_distance2`.

    Args:
        position: ``N x 3`` float32 or float64.
        box: ``(Lx, Ly, Lz, xy, xz, yz)``.
        r (float): the range, finite and positive.
        rows: the list (any order, repeats allowed; ``None``: every row).  It is put into cell order by `cell_order`;
            everything per entry is in that order, and both ``i`` and ``j`` come from it.
        cells: ``(cx, cy, cz)`` or ``None``: `neighbour_grid_for`.
        dimensions: 2 never looks at z.
        bins: 0, or 1 to 1024 bins of ``pair_hist`` over `neighbour_edges2`; a neighbour pair's bin is
            ``numpy.searchsorted(edges2, d2, side='right') - 1``.

    **Candidates.**  Entry ``j`` is a candidate of entry ``i`` when ``j != i`` as a list position (the same row listed
    twice is two entries at distance 0), both have a cell (an id below ``n_cells``) and ``j``'s cell is periodically
    adjacent to ``i``'s: per axis the offsets ``{0}`` at one cell, ``{0, +1}`` at two (-1 and +1 are the same cell and
    must not count twice) and ``{-1, 0, +1}`` otherwise, indices wrapping modulo the count.  ``j`` is a neighbour when
    ``pair_distance2(x_i, x_j) < r*r``, strictly, ``r*r`` formed once in float64.  This is what a cell list evaluates;
    it equals a search over all pairs except where the rounding of a wrapped fraction puts a pair at distance ``r``
    minus a few ulp into cells two apart.

    ValueError: ``r`` not finite or not positive; ``r`` above half the nearest plane distance of an axis that takes part
    (`ghost_fractions` ``> 0.5``: an image would count twice); ``cells`` with a count above `cell_grid_for` ``(box, r)``'s
    (narrower than ``r``) or more than 2^20 cells; ``bins`` outside 0 to 1024; what `cell_order` refuses.

    Returns a `Neighbours`.
    """
    dimensions = int(dimensions)
    grid = _neighbour_grid(box, r, cells, dimensions)
    r = float(r)
    bins = int(bins)
    if bins:
        edges2 = neighbour_edges2(r, bins)
    p = numpy.asarray(position)
    p = p.reshape(-1, 3) if p.size else numpy.zeros((0, 3), dtype=numpy.float32)
    if p.dtype not in (numpy.float32, numpy.float64):
        raise ValueError("position holds float32 or float64 values")
    rows = numpy.arange(p.shape[0], dtype=numpy.int64) if rows is None else rows
    rows_sorted, cell_sorted, _ = cell_order(p, box, rows, grid, dimensions)
    n = rows_sorted.shape[0]
    cx, cy, cz = grid
    n_cells = cx * cy * cz
    vectors = box_vectors(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
    r2 = numpy.float64(r) * numpy.float64(r)
    offs = cell_offsets(cell_sorted, n_cells)
    xs = p[rows_sorted].astype(numpy.float64)
    count = numpy.zeros(n, dtype=numpy.uint32)
    nearest2 = numpy.full(n, numpy.inf, dtype=numpy.float64)
    nearest = numpy.full(n, _NEIGHBOURS_NONE, dtype=numpy.int64)
    pair_hist = numpy.zeros(bins, dtype=numpy.uint64)
    somewhere = int(offs[n_cells])                       # the entries that have a cell come first
    ids = cell_sorted[:somewhere]
    ix, iy, iz = ids % cx, (ids // cx) % cy, ids // (cx * cy)
    for oz in _axis_offsets(cz):
        for oy in _axis_offsets(cy):
            for ox in _axis_offsets(cx):
                other = ((ix + ox) % cx) + cx * (((iy + oy) % cy) + cy * ((iz + oz) % cz))
                first, length = offs[other], offs[other + 1] - offs[other]
                ends = numpy.cumsum(length)
                lo = 0
                while lo < somewhere:                   # entries [lo, hi): at most _NEIGHBOURS_PAIRS_PER_STEP candidates
                    base = int(ends[lo - 1]) if lo else 0
                    hi = max(int(numpy.searchsorted(ends, base + _NEIGHBOURS_PAIRS_PER_STEP, side='right')), lo + 1)
                    hi = min(hi, somewhere)
                    ln = length[lo:hi]
                    total = int(ln.sum())
                    if total:
                        i = numpy.repeat(numpy.arange(lo, hi, dtype=numpy.int64), ln)
                        start = numpy.cumsum(ln) - ln
                        j = numpy.repeat(first[lo:hi] - start, ln) + numpy.arange(total, dtype=numpy.int64)
                        d2 = pair_distance2(xs[i], xs[j], vectors, dimensions)
                        near = (d2 < r2) & (i != j)
                        count += numpy.bincount(i[near], minlength=n).astype(numpy.uint32)
                        if bins:
                            pair_hist += numpy.bincount(numpy.searchsorted(edges2, d2[near], side='right') - 1,
                                                        minlength=bins).astype(numpy.uint64)
                        has = ln > 0                    # (reduceat over the non-empty segments: i ascends)
                        seg = start[has]
                        who = numpy.arange(lo, hi, dtype=numpy.int64)[has]
                        best2 = numpy.minimum.reduceat(numpy.where(near, d2, numpy.inf), seg)
                        at = numpy.minimum.reduceat(numpy.where(near & (d2 == numpy.repeat(best2, ln[has])), j,
                                                                _NEIGHBOURS_NONE), seg)
                        better = (best2 < nearest2[who]) | ((best2 == nearest2[who]) & (at < nearest[who]))
                        nearest2[who[better]] = best2[better]
                        nearest[who[better]] = at[better]
                    lo = hi
    nearest = nearest.astype(numpy.uint32)
    summary = numpy.zeros(_NEIGHBOURS_SUMMARY_WORDS + _NEIGHBOURS_COUNT_BINS + bins, dtype=numpy.uint64)
    summary[0], summary[1], summary[2] = n, n - somewhere, int(count.astype(numpy.uint64).sum())
    summary[5] = summary[6] = summary[7] = _NEIGHBOURS_NONE
    closest2 = numpy.inf
    if somewhere:
        summary[3], summary[4] = count[:somewhere].min(), count[:somewhere].max()
        summary[8:8 + _NEIGHBOURS_COUNT_BINS] = numpy.bincount(numpy.minimum(count[:somewhere], 256),
                                                               minlength=_NEIGHBOURS_COUNT_BINS)
        k = int(numpy.argmin(nearest2))                 # (the first position that attains the minimum)
        if nearest[k] != _NEIGHBOURS_NONE:
            closest2 = nearest2[k]
            summary[5], summary[6], summary[7] = k, rows_sorted[k], rows_sorted[nearest[k]]
    summary[8 + _NEIGHBOURS_COUNT_BINS:] = pair_hist
    return Neighbours(r, bins, grid, dimensions, summary, closest2, rows_sorted, cell_sorted, count, nearest2, nearest)


def frame_neighbours(frame_or_arrays, r, bins=0, cells=None, where=None, types=None, domain=None, box=None, dimensions=3):
    """`particle_neighbours` of a frame's ``position`` over a selection: the host twin of
    `HOOMDTrajectory.frame_neighbours_device`, which equals it exactly.  The selection -- `where_rows`, `domain_rows` or
    their intersection, as `frame_moments` forms it -- is the list: both ``i`` and ``j`` come from it.  A position that
    is stored nowhere puts every row at the origin.  Returns a `Neighbours`."""
    if hasattr(frame_or_arrays, 'particles'):
        frame = frame_or_arrays
        arrays = _particle_arrays(frame.particles)
        types = frame.particles.types if types is None else types
        box = frame.configuration.box if box is None else box
        if frame.configuration.dimensions is not None:
            dimensions = int(frame.configuration.dimensions)
        N = int(frame.particles.N)
    else:
        arrays = dict((k, v) for k, v in frame_or_arrays.items() if v is not None)
        if not arrays:
            raise ValueError("arrays holds no per-particle array")
        N = len(next(iter(arrays.values())))
    if box is None:
        raise ValueError("a neighbour search needs the box")
    rows = None
    if where is not None:
        rows = where_rows(arrays, where, types)
    if domain is not None:
        if 'position' not in arrays:
            raise ValueError("a domain needs box and the 'position' array")
        inside = domain_rows(arrays['position'], box, domain, dimensions)
        rows = inside if rows is None else numpy.intersect1d(rows, inside)
    position = arrays.get('position')
    if position is None:
        position = numpy.zeros((N, 3), dtype=numpy.float32)
    return particle_neighbours(position, box, r, rows=rows, cells=cells, dimensions=dimensions, bins=bins)


# ---- neighbour lists: the definition the GPU passes (`pgsd.fl.PGSDFile.neighbour_list_device`) equal exactly
_NLIST_SUMMARY_WORDS = 4            # n, nowhere, pairs, longest


def neighbour_list_bytes(n, pairs, distances=False):
    """The bytes a `NeighbourList` of ``n`` entries and ``pairs`` pairs occupies: ``8 (n + 1) + 4 pairs``, plus ``8
    pairs`` with distances -- what a restart budgets in HBM before it asks for the list."""
    return 8 * (int(n) + 1) + (12 if distances else 4) * int(pairs)


class NeighbourList(object):
    """The neighbours of a list in cell order as a CSR pair list (`neighbour_list`).

    Attributes:
        r (float), grid (``(cx, cy, cz)``), dimensions (int), half (bool): what was asked.
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere), as on `Neighbours`.
        offsets (uint64, ``n + 1``): ``offsets[0] == 0``, ``offsets[k + 1] - offsets[k]`` the length of entry ``k``'s
            segment, ``offsets[n] == pairs``.
        neighbours (uint32, ``pairs``): the LIST POSITIONS of the neighbours, segment after segment.
        distance2 (float64, ``pairs``) or ``None``: `pair_distance2` of each pair, where distances were asked for.
        n, nowhere (int): the entries, and those without a cell; pairs (int): the entries of ``neighbours``; longest
            (int): the largest segment length (0 at ``n == 0``).
        counts (property), `of`, `pair_rows`: host-side conveniences over numpy arrays; on a list whose arrays were left in
            GPU memory they raise ValueError -- copy the arrays to the host first.
    """

    __slots__ = ('r', 'grid', 'dimensions', 'half', 'rows', 'cell', 'offsets', 'neighbours', 'distance2', 'n', 'nowhere',
                 'pairs', 'longest')

    def __init__(self, r, grid, dimensions, half, summary, rows=None, cell=None, offsets=None, neighbours=None,
                 distance2=None):
        """``summary``: the four uint64 words of `pgsd_neighbour_offsets_device` -- n, nowhere, pairs, longest."""
        s = numpy.asarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _NLIST_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _NLIST_SUMMARY_WORDS)
        self.r, self.dimensions, self.half = float(r), int(dimensions), bool(half)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.n, self.nowhere, self.pairs, self.longest = (int(v) for v in s)
        self.rows, self.cell, self.offsets, self.neighbours, self.distance2 = rows, cell, offsets, neighbours, distance2

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return numpy.array([self.n, self.nowhere, self.pairs, self.longest], dtype=numpy.uint64)

    @property
    def nbytes(self):
        """`neighbour_list_bytes` of this list."""
        return neighbour_list_bytes(self.n, self.pairs, self.distance2 is not None)

    def _host(self, name):
        x = getattr(self, name)
        if not isinstance(x, numpy.ndarray):
            raise ValueError("NeighbourList.%s is %s: this works on numpy arrays (copy the arrays to the host first)"
                             % (name, "not set" if x is None else "in GPU memory"))
        return x

    @property
    def counts(self):
        """The segment lengths (uint64, ``n``): the differences of ``offsets``."""
        return numpy.diff(self._host('offsets'))

    def of(self, k):
        """The neighbours of entry ``k``: its slice of ``neighbours`` (a view)."""
        offsets, neighbours = self._host('offsets'), self._host('neighbours')
        k = int(k)
        if not 0 <= k < self.n:
            raise IndexError("entry %d of a list of %d" % (k, self.n))
        return neighbours[int(offsets[k]):int(offsets[k + 1])]

    def pair_rows(self):
        """``pairs x 2``: ``(rows[i], rows[j])`` of every pair, in list order."""
        rows, neighbours = self._host('rows'), self._host('neighbours')
        i = numpy.repeat(numpy.arange(self.n, dtype=numpy.int64), self.counts.astype(numpy.int64))
        return numpy.stack([rows[i], rows[neighbours.astype(numpy.int64)]], axis=1)

    def __repr__(self):
        return "NeighbourList(r=%r, grid=%r, half=%r, n=%d, nowhere=%d, pairs=%d, longest=%d)" % (
            self.r, self.grid, self.half, self.n, self.nowhere, self.pairs, self.longest)


def neighbour_list(position, box, r, rows=None, cells=None, dimensions=3, half=False, distances=False):
    """The neighbours of a row list inside the range ``r`` as a CSR pair list: what `particle_neighbours` counts, handed
    over.  The definition the GPU passes (`pgsd.fl.PGSDFile.neighbour_list_device`,
    `HOOMDTrajectory.frame_neighbour_list_device`) equal exactly.

    The grid, every refusal, the list in cell order (`cell_order`), the candidates, the arithmetic of one pair
    (`pair_distance2`, strict ``d2 < r*r`` with ``r*r`` formed once) and the treatment of entries without a cell are
    `particle_neighbours`' for the same ``r``; ``position``, ``box``, ``rows``, ``cells`` and ``dimensions`` are its
    arguments.  A list has an order, and that is what is new here:

    **The segment of entry** ``i`` holds the list positions ``j`` of its neighbours, ``j != i`` as a list position (a row
    listed twice is two entries, each the other's neighbour at distance 0), in THE ORDER of `sph_kernel_sums`: ``oz``
    over `_axis_offsets` ``(cz)``, inside it ``oy``, inside it ``ox``, the cell ``((ix+ox) % cx, (iy+oy) % cy, (iz+oz) %
    cz)``, inside a cell ascending list position (the walk is `_sph_near_pairs`, shared with the sums).  An entry without
    a cell has an empty segment and appears in nobody's.

    ``half=True``: the segment of ``i`` keeps only ``j > i`` by list position -- the same filter of the same full segment,
    in the same order.  At an exact half-box tie in a tilted box ``i -> j`` and ``j -> i`` may differ (`Neighbours`
    ``.pairs``); the half list is then whatever the filter gives: a pair is listed iff ``i -> j`` with ``i < j`` is inside
    the range.

    ``distances=True`` adds ``distance2``: ``pair_distance2(x_i, x_j)`` of each pair, bit for bit.

    Returns a `NeighbourList`.  If a frame is read with ``read_frame_device(..., cell_order=grid)`` for the same
    selection and grid and without a ghost layer, list position ``k`` is row ``k`` of the restarted arrays, so
    ``neighbours`` indexes them directly (with a ghost layer the owned and the ghost run are sorted separately: not
    covered).
    """
    dimensions = int(dimensions)
    grid = _neighbour_grid(box, r, cells, dimensions)
    r = float(r)
    # (the list ahead of the pair loop is the SPH sums': h is not looked at by the walk, the support stands for r)
    t = _sph_list((dimensions, 1.0, 0, r, grid), position, box, rows, ())
    n = t.n
    parts = [(numpy.zeros(0, numpy.int64), numpy.zeros(0, numpy.int64), numpy.zeros(0, numpy.float64))]
    for i, j, _, d2 in _sph_near_pairs(t):
        keep = (j > i) if half else (j != i)
        parts.append((i[keep], j[keep], d2[keep]))
    i = numpy.concatenate([p[0] for p in parts])
    # (stable: an entry's pairs keep the order of the steps, which is the order of the cells, and inside a step ascending j)
    order = numpy.argsort(i, kind='stable')
    counts = numpy.bincount(i, minlength=n).astype(numpy.uint64)
    offsets = numpy.zeros(n + 1, dtype=numpy.uint64)
    numpy.cumsum(counts, out=offsets[1:])
    neighbours = numpy.concatenate([p[1] for p in parts])[order].astype(numpy.uint32)
    distance2 = numpy.concatenate([p[2] for p in parts])[order] if distances else None
    summary = [n, n - t.somewhere, int(offsets[n]), int(counts.max()) if n else 0]
    return NeighbourList(r, grid, dimensions, half, summary, t.rows_sorted, t.cell_sorted, offsets, neighbours, distance2)


def frame_neighbour_list(frame_or_arrays, r, half=False, distances=False, cells=None, where=None, types=None, domain=None,
                         box=None, dimensions=3):
    """`neighbour_list` of a frame's ``position`` over a selection: the host twin of
    `HOOMDTrajectory.frame_neighbour_list_device`, which equals it exactly.  The selection is `frame_neighbours`' and is
    the list: both ``i`` and ``j`` come from it.  A position that is stored nowhere puts every row at the origin.

    If the frame is read with ``read_frame_device(idx, where=..., domain=..., cell_order=grid)`` for the same selection
    and the same grid, without a ghost layer, list position ``k`` is row ``k`` of the restarted arrays, so ``neighbours``
    indexes them directly.  Returns a `NeighbourList`."""
    _neighbour_range(r)
    _, position, box, dimensions, _, rows = _sph_frame_list(frame_or_arrays, float(r), where, types, domain, box, dimensions)
    return neighbour_list(position, box, r, rows=rows, cells=cells, dimensions=dimensions, half=half, distances=distances)


# ---- components: the definition the GPU pass (`pgsd.fl.PGSDFile.components_device`) equals exactly
_COMPONENTS_SUMMARY_WORDS = 6       # n, nowhere, components, singletons, largest, largest_label


class Components(object):
    """The connected components of a list in cell order within a linking length (`neighbour_components`).

    Attributes:
        r (float), grid (``(cx, cy, cz)``), dimensions (int): what was asked.
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere), as on `NeighbourList`.
        label (uint32, ``n``): the smallest LIST POSITION in the entry's component.
        component (uint32, ``n``): the dense id -- the number of components whose label is smaller.
        sizes (uint32, ``components``): ``sizes[c]`` is the number of entries with ``component == c``.
        n, nowhere (int): the entries, and those without a cell; components (int); singletons (int): the components of
            one entry, the nowhere entries among them; largest (int): the largest size; largest_label (int): the label of
            the largest component, among equal sizes the smallest.  All six are 0 at ``n == 0``.
        `members`, `fragments`: host-side conveniences over numpy arrays; on a result whose arrays were left in GPU memory
            they raise ValueError -- copy the arrays to the host first.
    """

    __slots__ = ('r', 'grid', 'dimensions', 'rows', 'cell', 'label', 'component', 'sizes', 'n', 'nowhere', 'components',
                 'singletons', 'largest', 'largest_label')

    def __init__(self, r, grid, dimensions, summary, rows=None, cell=None, label=None, component=None, sizes=None):
        """``summary``: the six uint64 words of `pgsd_components_device` -- n, nowhere, components, singletons, largest,
        largest_label."""
        s = numpy.asarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _COMPONENTS_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _COMPONENTS_SUMMARY_WORDS)
        self.r, self.dimensions = float(r), int(dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.n, self.nowhere, self.components, self.singletons, self.largest, self.largest_label = (int(v) for v in s)
        self.rows, self.cell, self.label, self.component, self.sizes = rows, cell, label, component, sizes

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return numpy.array([self.n, self.nowhere, self.components, self.singletons, self.largest, self.largest_label],
                           dtype=numpy.uint64)

    def _host(self, name):
        x = getattr(self, name)
        if not isinstance(x, numpy.ndarray):
            raise ValueError("Components.%s is %s: this works on numpy arrays (copy the arrays to the host first)"
                             % (name, "not set" if x is None else "in GPU memory"))
        return x

    def members(self, c):
        """The list positions of the entries of component ``c``, ascending (the first one is its label)."""
        component = self._host('component')
        c = int(c)
        if not 0 <= c < self.components:
            raise IndexError("component %d of %d" % (c, self.components))
        return numpy.nonzero(component == c)[0]

    def fragments(self, min_size=1):
        """The ids of the components with at least ``min_size`` entries, ascending."""
        return numpy.nonzero(self._host('sizes') >= int(min_size))[0]

    def __repr__(self):
        return ("Components(r=%r, grid=%r, n=%d, nowhere=%d, components=%d, singletons=%d, largest=%d, largest_label=%d)"
                % (self.r, self.grid, self.n, self.nowhere, self.components, self.singletons, self.largest,
                   self.largest_label))


def neighbour_components(position, box, r, rows=None, cells=None, dimensions=3):
    """The connected components of a row list within the linking length ``r`` -- the friends-of-friends grouping: which
    pieces has the fluid broken into.  The definition the GPU pass (`pgsd.fl.PGSDFile.components_device`,
    `HOOMDTrajectory.frame_components_device`) equals exactly.

    The grid, every refusal, the list in cell order and the entries without a cell are `neighbour_list`'s for the same
    arguments, and so are the arithmetic of one pair and the strict test ``d2 < r*r``.

    **Edges.**  The edges are exactly the pairs of ``neighbour_list(..., half=True)``: ``i`` and ``j`` (``i < j`` by list
    position) are joined iff ``i -> j`` is inside the range.  At an exact half-box tie in a tilted box ``i -> j`` and ``j
    -> i`` may differ (`Neighbours` ``.pairs``); the edge is then whatever the half list gives.  A row listed twice is two
    entries at distance 0, and the two are joined.  An entry without a cell has no edge: it is a component of its own, so
    the sizes add up to ``n``.

    **The result** is unique and depends on no order of evaluation: ``label`` is the smallest list position in the entry's
    component, ``component`` the number of components whose label is smaller (components are numbered in ascending order
    of their smallest member), ``sizes[c]`` the entries with ``component == c``; ``largest_label`` is the label of the
    largest component, among equal sizes the smallest label.

    Returns a `Components`.  If a frame is read with ``read_frame_device(..., cell_order=grid)`` for the same selection
    and grid and without a ghost layer, list position ``k`` is row ``k`` of the restarted arrays, so ``label`` indexes
    them directly and ``component[k]`` belongs to restarted row ``k``.
    """
    nl = neighbour_list(position, box, r, rows=rows, cells=cells, dimensions=dimensions, half=True)
    n = nl.n
    i = numpy.repeat(numpy.arange(n, dtype=numpy.int64), nl.counts.astype(numpy.int64))
    j = nl.neighbours.astype(numpy.int64)
    label = numpy.arange(n, dtype=numpy.int64)
    while True:                                         # the smallest label travels along the edges, then down the trees
        low = numpy.minimum(label[i], label[j])
        before = label.copy()
        numpy.minimum.at(label, i, low)
        numpy.minimum.at(label, j, low)
        while True:
            down = label[label]
            if numpy.array_equal(down, label):
                break
            label = down
        if numpy.array_equal(label, before):
            break
    roots = numpy.nonzero(label == numpy.arange(n, dtype=numpy.int64))[0]
    component = numpy.searchsorted(roots, label)
    sizes = numpy.bincount(component, minlength=roots.shape[0]).astype(numpy.uint32)
    summary = [n, nl.nowhere, roots.shape[0], int((sizes == 1).sum()), 0, 0]
    if n:
        c = int(numpy.argmax(sizes))                    # (the first id that attains the maximum: the smallest label)
        summary[4], summary[5] = int(sizes[c]), int(roots[c])
    return Components(nl.r, nl.grid, nl.dimensions, summary, nl.rows, nl.cell, label.astype(numpy.uint32),
                      component.astype(numpy.uint32), sizes)


def frame_components(frame_or_arrays, r, cells=None, where=None, types=None, domain=None, box=None, dimensions=3):
    """`neighbour_components` of a frame's ``position`` over a selection: the host twin of
    `HOOMDTrajectory.frame_components_device`, which equals it exactly.  The selection is `frame_neighbour_list`'s and is
    the list: both ends of an edge come from it.  A position that is stored nowhere puts every row at the origin.

    If the frame is read with ``read_frame_device(idx, where=..., domain=..., cell_order=grid)`` for the same selection
    and the same grid, without a ghost layer, list position ``k`` is row ``k`` of the restarted arrays, so ``label``
    indexes them directly.  Returns a `Components`."""
    _neighbour_range(r)
    _, position, box, dimensions, _, rows = _sph_frame_list(frame_or_arrays, float(r), where, types, domain, box, dimensions)
    return neighbour_components(position, box, r, rows=rows, cells=cells, dimensions=dimensions)


# ---- component fields: the definition the GPU pass (`pgsd.fl.PGSDFile.component_moments_device`) equals exactly
_CMOM_SUMMARY_WORDS = 6     # n, components, bad, wide, heaviest, widest


class ComponentMoments(object):
    """What each connected component of a `Components` result is (`component_moments`): arrays of one entry (or one row)
    per component, in the order of the dense ids.

    Attributes:
        sizes (``components``): the entries of the component (``components_of.sizes``; ``None`` without it).
        bad (uint32): the entries at which at least one of the nine per-entry values is not finite.
        wide (uint32): 1 if the extent reaches half a box length on an axis: the piece percolates, or nearly does, and
            its `centre_of_mass`, ``lo``, ``hi`` and `span` are reported but not meaningful.  0 guarantees that the
            displacements are the piece's one consistent unwrapping.
        mass, kinetic, internal (float64); momentum (float64, x 3): as `CellMoments`'.
        first_moment (float64, x 3): the sum of ``m d``, ``d`` the displacement from the component's root to the entry.
        origin (float64, x 3): the root's position; lo, hi (float64, x 3): the extent of the finite ``d``.
        n, components, bad_entries, wide_components, heaviest_id, widest_id (int): the summary words.
        components_of: the `Components` this was made from, or ``None``.
        mean_velocity, centre_of_mass, span (properties), `heaviest`: host-side conveniences over numpy arrays; on a
            result whose tables were left in GPU memory they raise ValueError -- `to_host` copies the tables first.
    """

    __slots__ = ('sizes', 'bad', 'wide', 'mass', 'momentum', 'kinetic', 'internal', 'first_moment', 'origin', 'lo', 'hi',
                 'n', 'components', 'bad_entries', 'wide_components', 'heaviest_id', 'widest_id', 'components_of', '_tables')

    def __init__(self, summary, bad, wide, mass, momentum, kinetic, internal, first_moment, origin, lo, hi, sizes=None,
                 components_of=None, tables=None):
        s = numpy.asarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _CMOM_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _CMOM_SUMMARY_WORDS)
        self.n, self.components, self.bad_entries, self.wide_components, self.heaviest_id, self.widest_id = (int(v) for v in s)
        self.bad, self.wide, self.mass, self.momentum, self.kinetic, self.internal = bad, wide, mass, momentum, kinetic, internal
        self.first_moment, self.origin, self.lo, self.hi = first_moment, origin, lo, hi
        self.sizes, self.components_of, self._tables = sizes, components_of, tables

    @classmethod
    def from_tables(cls, summary, sums, extent, origin, flags, sizes=None, components_of=None):
        """From the tables of `pgsd_component_moments_device`: ``sums`` (``components x 9``, the order of the per-entry
        values), ``extent`` (``x 6``: lo, hi), ``origin`` (``x 3``), ``flags`` (``x 2`` uint32: bad, wide).  numpy arrays
        are cut into the attributes; tables in GPU memory become strided views of them."""
        if isinstance(sums, numpy.ndarray):
            s = numpy.asarray(sums, dtype=numpy.float64).reshape(-1, _MOMENTS_QUANTITIES)
            e = numpy.asarray(extent, dtype=numpy.float64).reshape(-1, 6)
            f = numpy.asarray(flags, dtype=numpy.uint32).reshape(-1, 2)
            o = numpy.asarray(origin, dtype=numpy.float64).reshape(-1, 3)
            return cls(summary, f[:, 0].copy(), f[:, 1].copy(), s[:, 0].copy(), s[:, 1:4].copy(), s[:, 4].copy(),
                       s[:, 5].copy(), s[:, 6:9].copy(), o.copy(), e[:, 0:3].copy(), e[:, 3:6].copy(), sizes, components_of)
        T = int(sums.shape[0])

        def cut(table, width, item, first, M):
            shape, strides = ((T,), (width * item,)) if M == 1 else ((T, M), (width * item, item))
            if T == 0:                          # (no component: an empty view has nothing to stride over)
                return table.view(shape=shape)
            return table.view(shape=shape, strides=strides, offset_bytes=first * item)

        return cls(summary, cut(flags, 2, 4, 0, 1), cut(flags, 2, 4, 1, 1), cut(sums, 9, 8, 0, 1), cut(sums, 9, 8, 1, 3),
                   cut(sums, 9, 8, 4, 1), cut(sums, 9, 8, 5, 1), cut(sums, 9, 8, 6, 3), origin, cut(extent, 6, 8, 0, 3),
                   cut(extent, 6, 8, 3, 3), sizes, components_of, (sums, extent, origin, flags))

    def to_host(self):
        """The same result over numpy arrays: four device-to-host copies of the tables (and one of ``sizes``); a result
        that is on the host already is returned as it is."""
        if self._tables is None:
            return self
        sizes = self.sizes
        if sizes is not None and not isinstance(sizes, numpy.ndarray):
            sizes = fl._device_to_host(sizes)
        return ComponentMoments.from_tables(self.summary, *[fl._device_to_host(t) for t in self._tables], sizes=sizes,
                                            components_of=self.components_of)

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return numpy.array([self.n, self.components, self.bad_entries, self.wide_components, self.heaviest_id,
                            self.widest_id], dtype=numpy.uint64)

    def _host(self, name):
        x = getattr(self, name)
        if not isinstance(x, numpy.ndarray):
            raise ValueError("ComponentMoments.%s is %s: this works on numpy arrays (to_host() copies the tables first)"
                             % (name, "not set" if x is None else "in GPU memory"))
        return x

    def _per_mass(self, a):
        mass = self._host('mass')
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(mass[:, None] != 0, a / mass[:, None], numpy.nan)

    @property
    def mean_velocity(self):
        return self._per_mass(self._host('momentum'))

    @property
    def centre_of_mass(self):
        """``origin + first_moment / mass``: NaN where the mass is 0; not folded into the box."""
        return self._host('origin') + self._per_mass(self._host('first_moment'))

    @property
    def span(self):
        with numpy.errstate(over='ignore'):
            return self._host('hi') - self._host('lo')

    def heaviest(self, k=1):
        """The ids of the ``k`` largest masses, heaviest first; among equal masses the smaller id first (a mass sum that
        is a NaN counts as ``-inf``)."""
        mass = self._host('mass')
        key = numpy.where(numpy.isnan(mass), -numpy.inf, mass)
        return numpy.argsort(-key, kind='stable')[:max(int(k), 0)]

    def __repr__(self):
        return ("ComponentMoments(n=%d, components=%d, bad=%d, wide=%d, heaviest=%d, widest=%d)"
                % (self.n, self.components, self.bad_entries, self.wide_components, self.heaviest_id, self.widest_id))


def _first_largest(values):
    """The smallest index that attains the largest value; a NaN counts as ``-inf``; 0 for no value."""
    v = numpy.asarray(values, dtype=numpy.float64)
    return int(numpy.argmax(numpy.where(numpy.isnan(v), -numpy.inf, v))) if v.size else 0


def component_moments(mass, velocity, energy, position, box, label, component, rows=None, N=None, dimensions=3):
    """What each connected component is: mass, momentum, kinetic and internal energy, centre and extent per component of
    a `neighbour_components` result.  The definition the GPU pass (`pgsd.fl.PGSDFile.component_moments_device`,
    `HOOMDTrajectory.frame_component_moments_device`) equals exactly, every float bit for bit.

    Args:
        mass, velocity, energy, rows, N: exactly `cell_moments`'; position: an ``N x 3`` array (required).
        box: ``(Lx, Ly, Lz, xy, xz, yz)``, taken as float32 like `neighbour_components` takes it.
        label, component: one entry per **list entry** -- `Components` ``.label`` and ``.component`` of the same list.

    ``components`` is ``component.max() + 1`` (0 for no entry).  Per component ``c``:

    **Origin.**  ``origin[c]`` is the float64 position of the component's ROOT, the entry at list position ``label``
    (the component's smallest member); float32 positions are converted exactly.

    **Displacement.**  The root has ``d = (+0.0, +0.0, +0.0)`` by definition -- no subtraction is made.  Every other entry
    ``k`` has ``d = pair_displacement(x_root, x_k, box_vectors(box), dimensions)``: HOOMD's single-shift minimum image
    from the root to the entry.

    **Nine sums.**  `cell_moments`' nine values with the position replaced by ``d``, in `cell_moments`' order over the
    component's entries in list order (pieces of 1024 counted from the component's first entry, 64 striding lanes, the
    wave tree, the pieces in sequence, a value that is not finite counting as ``+0.0``, each value for itself).
    ``bad[c]`` counts the entries with at least one value that is not finite.

    **Extent.**  ``lo[c]`` and ``hi[c]`` start at ``+0.0``, the root's own displacement, and take every other entry's
    ``d_a`` that is finite by strict comparisons (``d_a < lo_a``, ``d_a > hi_a``): neither is ever ``-0.0`` and the result
    depends on no order.

    **Wide.**  ``wide[c]`` is 1 if ``hi_a - lo_a >= L_a / 2`` on an axis ``a < dimensions``.  The linking length is at
    most half the nearest plane distance, so while every span stays below ``L_a / 2`` the displacements are the piece's
    one consistent unwrapping (`DESIGN.md` has the argument); a wide piece percolates, or nearly does, and its centre and
    extent are reported but not meaningful.

    **Summary.**  ``n``; ``components``; the bad entries; the wide components; ``heaviest``: the id of the largest mass
    sum, among equals the smallest id; ``widest``: the id of the largest ``max_a (hi_a - lo_a)``, among equals the
    smallest id (a NaN counts as ``-inf``).  All 0 for no entry.

    ValueError: what `cell_moments` refuses for its inputs; no position array; lengths that differ; ``label[k] > k``;
    ``label[label[k]] != label[k]``; ``component[k] != component[label[k]]``; ids that are not the dense ascending
    numbering of the labels.  Returns a `ComponentMoments`.
    """
    dimensions = int(dimensions)
    if dimensions not in (2, 3):
        raise ValueError("dimensions must be 2 or 3")
    if position is None or numpy.asarray(position).ndim != 2:
        raise ValueError("component_moments takes the position array: a component's origin and extent need it")
    arrays, dt, n_rows = _moments_arrays(mass, velocity, energy, position, N)
    n_rows, rows, n = _moments_rows(n_rows, rows)
    vectors = box_vectors(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
    label = numpy.asarray(label).reshape(-1)
    component = numpy.asarray(component).reshape(-1)
    if label.shape[0] != n or component.shape[0] != n:
        raise ValueError("label and component hold one entry per list entry: %d and %d for %d entries"
                         % (label.shape[0], component.shape[0], n))
    if n and (label.dtype.kind not in 'iu' or component.dtype.kind not in 'iu'):
        raise ValueError("label and component hold integers")
    label, component = label.astype(numpy.int64), component.astype(numpy.int64)
    at = numpy.arange(n, dtype=numpy.int64)
    if n:
        if (label < 0).any() or (label > at).any():
            raise ValueError("a label lies above its entry: label[k] <= k")
        if (label[label] != label).any():
            raise ValueError("a label is no root: label[label[k]] == label[k]")
        if (component != component[label]).any():
            raise ValueError("an entry's id differs from its root's")
        roots = numpy.nonzero(label == at)[0]
        if not numpy.array_equal(component, numpy.searchsorted(roots, label)):
            raise ValueError("the ids are not the dense ascending numbering of the labels")
    components = int(component.max()) + 1 if n else 0
    # the displacement from the root to the entry; the root's own is +0.0 by definition
    x = numpy.asarray(arrays['position'])
    listed = (x if rows is None else x[rows]).astype(numpy.float64)
    d = [numpy.zeros(n, dtype=numpy.float64) for _ in range(3)]
    if n:
        moved = pair_displacement(listed[label], listed, vectors, dimensions)
        for a in range(3):
            d[a] = numpy.where(label == at, 0.0, moved[a])
    values, finite, all_finite = _moments_values(arrays, dt, rows, n, x=d)
    perm = numpy.argsort(component, kind='stable')
    sorted_ids = component[perm]
    offs = numpy.searchsorted(sorted_ids, numpy.arange(components + 2, dtype=numpy.int64), side='left').astype(numpy.int64)
    sums = numpy.zeros((components, _MOMENTS_QUANTITIES), dtype=numpy.float64)
    for q in range(_MOMENTS_QUANTITIES):
        if components:
            sums[:, q] = _cell_ordered_sums(numpy.where(finite[q], values[q], 0.0)[perm], sorted_ids, offs, components)
    bad = numpy.bincount(component[~all_finite], minlength=components).astype(numpy.uint32) if n else numpy.zeros(0, numpy.uint32)
    lo, hi = numpy.zeros((components, 3), dtype=numpy.float64), numpy.zeros((components, 3), dtype=numpy.float64)
    for a in range(3):
        take = numpy.isfinite(d[a]) & (label != at)
        # (the strict comparisons against +0.0 made first: a -0.0 never reaches a bound, whatever minimum / maximum do)
        low, high = numpy.where(d[a] < 0, d[a], 0.0), numpy.where(d[a] > 0, d[a], 0.0)
        numpy.minimum.at(lo[:, a], component[take], low[take])
        numpy.maximum.at(hi[:, a], component[take], high[take])
    with numpy.errstate(over='ignore'):
        span = hi - lo
    wide = numpy.zeros(components, dtype=numpy.uint32)
    for a in range(dimensions):
        wide |= (span[:, a] >= vectors[a] / 2).astype(numpy.uint32)
    origin = listed[perm[offs[:components]]] if n else numpy.zeros((0, 3), dtype=numpy.float64)
    summary = [n, components, int((~all_finite).sum()), int(wide.sum()), _first_largest(sums[:, 0]),
               _first_largest(span.max(axis=1) if components else [])]
    extent = numpy.concatenate([lo, hi], axis=1)
    return ComponentMoments.from_tables(summary, sums, extent, origin, numpy.stack([bad, wide], axis=1))


def frame_component_moments(frame_or_arrays, r, cells=None, where=None, types=None, domain=None, box=None, dimensions=3):
    """`frame_components` of a frame, then `component_moments` of its ``mass``, ``velocity``, ``energy`` and ``position``
    over the same list: the host twin of `HOOMDTrajectory.frame_component_moments_device`, which equals it exactly.  The
    selection, the grid and the refusals are `frame_components`'.  Returns a `ComponentMoments` whose ``components_of``
    is the `Components` and whose ``sizes`` is its ``sizes``."""
    _neighbour_range(r)
    arrays, position, box, dimensions, _, rows = _sph_frame_list(frame_or_arrays, float(r), where, types, domain, box,
                                                                 dimensions)
    comps = neighbour_components(position, box, r, rows=rows, cells=cells, dimensions=dimensions)
    got = component_moments(arrays.get('mass'), arrays.get('velocity'), arrays.get('energy'), position, box, comps.label,
                            comps.component, rows=comps.rows, N=len(position), dimensions=dimensions)
    got.components_of, got.sizes = comps, comps.sizes
    return got


# ---- SPH kernel sums: the definition the GPU pass (`pgsd.fl.PGSDFile.sph_sums_device`) equals exactly
SPH_KERNELS = ('wendland_c2', 'cubic_spline')
_SPH_SUMMARY_WORDS = 13     # n, nowhere, not_finite, surface, deviation_at, deviation_row, 3 x (min, max), deviation


def _sph_kernel_id(kernel):
    if kernel not in SPH_KERNELS:
        raise ValueError("the kernel is one of %s: %r" % (', '.join(SPH_KERNELS), kernel))
    return SPH_KERNELS.index(kernel)


def _sph_length(h):
    h = float(h)
    if not (h > 0.0 and h < float('inf')):
        raise ValueError("the smoothing length must be finite and positive: %r" % (h,))
    return h


def sph_sigma(kernel, h, dimensions=3):
    """The normalisation of an SPH kernel of support ``2h``, float64 on the host: ``21/(16 pi h^3)`` and ``7/(4 pi h^2)``
    for ``wendland_c2`` in 3-D and 2-D, ``1/(pi h^3)`` and ``10/(7 pi h^2)`` for ``cubic_spline``."""
    k, h = _sph_kernel_id(kernel), numpy.float64(_sph_length(h))
    if int(dimensions) == 3:
        return float((21.0 / (16.0 * numpy.pi * (h * h * h))) if k == 0 else (1.0 / (numpy.pi * (h * h * h))))
    return float((7.0 / (4.0 * numpy.pi * (h * h))) if k == 0 else (10.0 / (7.0 * numpy.pi * (h * h))))


def sph_weight(q, kernel='wendland_c2'):
    """``w(q)`` of one pair, float64 without contraction, for ``q = |x_i - x_j| * (1/h)`` below 2.  ``wendland_c2``:
    ``t = 1.0 - 0.5*q``, ``t2 = t*t``, ``w = (t2*t2) * (2.0*q + 1.0)``.  ``cubic_spline``: ``q2 = q*q``; where ``q < 1.0``
    ``w = (1.0 - 1.5*q2) + 0.75*(q2*q)``, otherwise ``u = 2.0 - q`` and ``w = 0.25*((u*u)*u)``."""
    q = numpy.asarray(q, dtype=numpy.float64)
    if _sph_kernel_id(kernel) == 0:
        t = 1.0 - 0.5 * q
        t2 = t * t
        return (t2 * t2) * (2.0 * q + 1.0)
    q2 = q * q
    u = 2.0 - q
    return numpy.where(q < 1.0, (1.0 - 1.5 * q2) + 0.75 * (q2 * q), 0.25 * ((u * u) * u))


class KernelSums(object):
    """The SPH kernel sums of a list in cell order (`sph_kernel_sums`).

    Attributes:
        h (float), kernel (str), grid (``(cx, cy, cz)``), dimensions (int), surface_below (float or ``None``), volume
            (bool: was a ``density`` given): what was asked; sigma (float): `sph_sigma`.
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere).
        number, density, shepard (float64): per entry, in list order, ``sigma * sum w``, ``sigma * sum m_j w`` and
            ``sigma * sum (m_j / rho_j) w`` over the entries inside ``2h``, the entry itself among them; ``+0.0`` for an
            entry nowhere.  ``shepard`` is ``None`` without ``density``.  The five per-entry arrays are numpy arrays from
            the model; from the GPU they are ``None`` unless ``return_rows`` left them in GPU memory.
        n, nowhere (int): the entries, and those without a cell.
        number_min, number_max, density_min, density_max, shepard_min, shepard_max (float): over the entries that have a
            cell, by strict compares from ``+inf`` / ``-inf`` (a NaN never replaces a value); the last two ``None``
            without ``density``.
        not_finite (int): the entries that have a cell and whose ``density`` sum is NaN or infinite.
        deviation (float), deviation_at (int), deviation_row (int): ``density_i - float64(rho_i)`` where its magnitude is
            the largest over the entries that have a cell, sign kept, the smaller list position on a tie, a NaN never;
            the position and its row.  All ``None`` without ``density`` or where no entry has a number for it.
        surface (int or ``None``): the entries that have a cell and ``shepard < surface_below``.
    """

    __slots__ = ('h', 'kernel', 'grid', 'dimensions', 'surface_below', 'volume', 'sigma', 'rows', 'cell', 'number', 'density',
                 'shepard', 'n', 'nowhere', 'not_finite', 'surface', 'deviation', 'deviation_at', 'deviation_row',
                 'number_min', 'number_max', 'density_min', 'density_max', 'shepard_min', 'shepard_max', '_words')

    def __init__(self, h, kernel, grid, dimensions, summary, volume, surface_below=None, rows=None, cell=None, number=None,
                 density=None, shepard=None):
        """``summary``: the 13 uint64 words of `pgsd_sph_sums_device` -- n, nowhere, not_finite, surface, deviation_at,
        deviation_row, then as float64 bit patterns the minimum and maximum of number, density and shepard and the
        deviation."""
        s = numpy.ascontiguousarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _SPH_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _SPH_SUMMARY_WORDS)
        self._words = s.copy()
        self.h, self.kernel, self.dimensions, self.volume = float(h), kernel, int(dimensions), bool(volume)
        self.sigma = sph_sigma(kernel, h, dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.surface_below = None if surface_below is None else float(surface_below)
        self.n, self.nowhere, self.not_finite = int(s[0]), int(s[1]), int(s[2])
        f = s[6:13].view(numpy.float64)
        self.number_min, self.number_max, self.density_min, self.density_max = (float(v) for v in f[:4])
        self.shepard_min, self.shepard_max = (float(f[4]), float(f[5])) if self.volume else (None, None)
        self.surface = int(s[3]) if self.volume and self.surface_below is not None else None
        found = self.volume and int(s[4]) != _NEIGHBOURS_NONE
        self.deviation = float(f[6]) if found else None
        self.deviation_at, self.deviation_row = (int(s[4]), int(s[5])) if found else (None, None)
        self.rows, self.cell, self.number, self.density, self.shepard = rows, cell, number, density, shepard

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return self._words.copy()

    def __repr__(self):
        return "KernelSums(h=%r, kernel=%r, grid=%r, n=%d, nowhere=%d, density=[%r, %r], deviation=%r)" % (
            self.h, self.kernel, self.grid, self.n, self.nowhere, self.density_min, self.density_max, self.deviation)


def _sph_summary(n, somewhere, rows_sorted, number, density, shepard, rho, surface_below):
    """The summary words from the per-entry results (``shepard``, ``rho`` None without a density): no float is summed, so
    no order enters."""
    words = numpy.zeros(_SPH_SUMMARY_WORDS, dtype=numpy.uint64)
    f = words[6:13].view(numpy.float64)
    words[0], words[1] = n, n - somewhere
    words[4] = words[5] = _NEIGHBOURS_NONE
    f[0:6:2], f[1:6:2], f[6] = numpy.inf, -numpy.inf, 0.0
    with numpy.errstate(invalid='ignore', over='ignore'):
        for k, v in enumerate((number, density, shepard)):
            if v is None or not somewhere:
                continue
            v = v[:somewhere]
            ok = v[v == v]
            if ok.size:
                f[2 * k], f[2 * k + 1] = min(numpy.inf, ok.min()), max(-numpy.inf, ok.max())
        words[2] = int(numpy.count_nonzero(~numpy.isfinite(density[:somewhere])))
        if shepard is not None and somewhere:
            if surface_below is not None:
                words[3] = int(numpy.count_nonzero(shepard[:somewhere] < numpy.float64(surface_below)))
            dev = density[:somewhere] - rho[:somewhere]
            size = numpy.where(dev == dev, numpy.abs(dev), -1.0)
            k = int(numpy.argmax(size))                 # (the first position that attains the maximum)
            if size[k] >= 0.0:
                words[4], words[5], f[6] = k, rows_sorted[k], dev[k]
    return words


def _sph_asked(box, h, cells, dimensions, kernel):
    """``(dimensions, h, kernel id, support 2h, grid)`` of `sph_kernel_sums` and `sph_kernel_gradients`, checked."""
    dimensions = int(dimensions)
    h = _sph_length(h)
    kid = _sph_kernel_id(kernel)
    support = float(numpy.float64(2.0) * numpy.float64(h))
    return dimensions, h, kid, support, _neighbour_grid(box, support, cells, dimensions)


class _SphList(object):
    """What `sph_kernel_sums` and `sph_kernel_gradients` share ahead of their pair loops: the list in cell order
    (``rows_sorted``, ``cell_sorted``, ``n``, ``somewhere``: the entries that have a cell come first), the CSR offsets,
    the compacted float64 positions ``xs`` and columns (``None``: not given), ``vectors``, ``r2``, ``inv_h``, ``sigma``."""
    __slots__ = ('dimensions', 'grid', 'n', 'somewhere', 'rows_sorted', 'cell_sorted', 'offs', 'xs', 'columns', 'vectors',
                 'r2', 'inv_h', 'sigma')


def _sph_list(asked, position, box, rows, columns):
    """``columns``: ``(name, values or None, width)`` each; a column comes back as float64, in list order."""
    t = _SphList()
    t.dimensions, h, kid, support, t.grid = asked
    p = numpy.asarray(position)
    p = p.reshape(-1, 3) if p.size else numpy.zeros((0, 3), dtype=numpy.float32)
    if p.dtype not in (numpy.float32, numpy.float64):
        raise ValueError("position holds float32 or float64 values")
    given = []
    for name, v, width in columns:
        if v is not None:
            v = numpy.asarray(v)
            if v.dtype not in (numpy.float32, numpy.float64) or v.size != p.shape[0] * width:
                raise ValueError("%s holds %s float32 or float64 value%s per row of position"
                                 % (name, 'one' if width == 1 else 'three', '' if width == 1 else 's'))
            v = (v.reshape(-1) if width == 1 else v.reshape(-1, width)).astype(numpy.float64)
        given.append(v)
    rows = numpy.arange(p.shape[0], dtype=numpy.int64) if rows is None else rows
    t.rows_sorted, t.cell_sorted, _ = cell_order(p, box, rows, t.grid, t.dimensions)
    t.n = t.rows_sorted.shape[0]
    n_cells = t.grid[0] * t.grid[1] * t.grid[2]
    t.vectors = box_vectors(numpy.asarray(box, dtype=numpy.float32).reshape(-1)[:6])
    t.r2 = numpy.float64(support) * numpy.float64(support)
    t.inv_h = numpy.float64(1.0) / numpy.float64(h)
    t.sigma = numpy.float64(sph_sigma(SPH_KERNELS[kid], h, t.dimensions))
    t.offs = cell_offsets(t.cell_sorted, n_cells)
    at = t.rows_sorted.astype(numpy.int64)
    t.xs = p[at].astype(numpy.float64)
    t.columns = [None if v is None else v[at] for v in given]
    t.somewhere = int(t.offs[n_cells])                   # the entries that have a cell come first
    return t


def _sph_near_pairs(t):
    """The pairs of a `_SphList` inside the support, in THE ORDER of `sph_kernel_sums`: steps of ``(i, j, (dx, dy, dz),
    d2)`` arrays, the pairs of a step sorted by ``i`` and, inside one candidate cell, by ascending ``j``.  `numpy.add.at`
    adds the pairs of a step one after the other, so that together with the order of the steps each entry's sum is the
    sequential one of the definition."""
    return _sph_pairs_around(t, t.xs[:t.somewhere], t.cell_sorted[:t.somewhere])


def _sph_pairs_around(t, centres, ids):
    """`_sph_near_pairs` with the centres handed in: ``centres`` (float64, ``K x 3``) and their cells ``ids`` (each inside
    the grid) stand where the list's own entries do, ``i`` counts the centres, ``j`` the entries of the list, and ``d =
    pair_displacement(centres[i], xs[j])``.  The cells, their order and the order inside a step are the same."""
    cx, cy, cz = t.grid
    offs, xs, somewhere = t.offs, t.xs, ids.shape[0]
    ix, iy, iz = ids % cx, (ids // cx) % cy, ids // (cx * cy)
    for oz in _axis_offsets(cz):
        for oy in _axis_offsets(cy):
            for ox in _axis_offsets(cx):
                other = ((ix + ox) % cx) + cx * (((iy + oy) % cy) + cy * ((iz + oz) % cz))
                first, length = offs[other], offs[other + 1] - offs[other]
                ends = numpy.cumsum(length)
                lo = 0
                while lo < somewhere:               # entries [lo, hi): at most _NEIGHBOURS_PAIRS_PER_STEP candidates
                    base = int(ends[lo - 1]) if lo else 0
                    hi = max(int(numpy.searchsorted(ends, base + _NEIGHBOURS_PAIRS_PER_STEP, side='right')), lo + 1)
                    hi = min(hi, somewhere)
                    ln = length[lo:hi]
                    total = int(ln.sum())
                    if total:
                        i = numpy.repeat(numpy.arange(lo, hi, dtype=numpy.int64), ln)
                        start = numpy.cumsum(ln) - ln
                        j = numpy.repeat(first[lo:hi] - start, ln) + numpy.arange(total, dtype=numpy.int64)
                        d = pair_displacement(centres[i], xs[j], t.vectors, t.dimensions)
                        with numpy.errstate(invalid='ignore', over='ignore'):
                            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                            near = d2 < t.r2
                        yield i[near], j[near], (d[0][near], d[1][near], d[2][near]), d2[near]
                    lo = hi


def sph_kernel_sums(position, box, h, mass=None, density=None, rows=None, cells=None, dimensions=3, kernel='wendland_c2',
                    surface_below=None):
    """The SPH kernel sums of a row list: per entry ``i`` the number density ``sigma * sum_j W_ij``, the summation density
    ``rho_i = sigma * sum_j m_j W_ij`` and the Shepard sum ``sigma * sum_j (m_j / rho_j) W_ij`` over the entries ``j``
    inside the kernel support ``2h``, and over the list their ranges, the largest deviation of the summation density
    from the stored one and the entries below a Shepard threshold (the free surface).  The definition the GPU pass
    (`pgsd.fl.PGSDFile.sph_sums_device`, `HOOMDTrajectory.frame_kernel_sums_device`) equals exactly, the floats bit for
    bit -- so the ORDER of every sum is part of it.

    Args:
        position: ``N x 3`` float32 or float64; box: ``(Lx, Ly, Lz, xy, xz, yz)``.
        h (float): the smoothing length, finite and positive; the support, the range of the search, is ``2h``.
        mass, density: ``N`` float32 or float64 values, or ``None``: every ``m_j`` is 1.0; no volume sum, no deviation, no
            surface count.
        rows: the list (any order, repeats allowed; ``None``: every row), put into cell order by `cell_order`; both ``i``
            and ``j`` come from it and everything per entry is in that order.
        cells: ``(cx, cy, cz)`` or ``None``: `neighbour_grid_for` ``(box, 2*h)``.  The grid and every refusal are
            `particle_neighbours`' for the range ``2*h``.
        kernel: ``'wendland_c2'`` or ``'cubic_spline'`` (`sph_weight`); surface_below: a float or ``None``.

    **One pair**, float64 throughout without contraction, float32 inputs converted exactly: ``d2 = pair_distance2(x_i,
    x_j)``; ``j`` contributes when ``d2 < r2``, strictly, with ``r2 = (2h)*(2h)`` formed once; ``i`` itself contributes
    (``d2 = 0``, ``w = 1``) and a row listed twice is two entries; ``rr = sqrt(d2)``, ``q = rr * inv_h`` with ``inv_h =
    1/h`` formed once, ``w = sph_weight(q)``.  Three accumulators per entry start at ``+0.0``: ``a_n += w``, ``a_m += m_j
    * w``, ``a_v += V_j * w`` with ``V_j = m_j / rho_j``, one float64 division of the stored values taken as it is
    (``rho_j = 0`` gives what IEEE gives).

    **The order.**  Candidate cells are visited with ``oz`` over `_axis_offsets` ``(cz)``, inside it ``oy``, inside it
    ``ox``, each tuple in its own order; the cell is ``((ix+ox) % cx, (iy+oy) % cy, (iz+oz) % cz)``; inside a cell the
    order is ascending list position.  After the last candidate ``number = sigma*a_n``, ``density = sigma*a_m``,
    ``shepard = sigma*a_v`` with `sph_sigma`.  An entry without a cell contributes to nobody and its values are ``+0.0``.

    Returns a `KernelSums`.
    """
    asked = _sph_asked(box, h, cells, dimensions, kernel)
    if surface_below is not None:
        surface_below = float(surface_below)
        if surface_below != surface_below:
            raise ValueError("surface_below is a number or None")
    t = _sph_list(asked, position, box, rows, (('mass', mass, 1), ('density', density, 1)))
    dimensions, h, kid, grid = asked[0], asked[1], asked[2], asked[4]
    n, sigma, rows_sorted, cell_sorted, somewhere = t.n, t.sigma, t.rows_sorted, t.cell_sorted, t.somewhere
    mass, density = t.columns
    m = numpy.ones(n, dtype=numpy.float64) if mass is None else mass
    rho = density
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        vol = None if rho is None else m / rho
    a_n, a_m = numpy.zeros(n, dtype=numpy.float64), numpy.zeros(n, dtype=numpy.float64)
    a_v = None if vol is None else numpy.zeros(n, dtype=numpy.float64)
    with numpy.errstate(invalid='ignore', over='ignore'):
        for i, j, d, d2 in _sph_near_pairs(t):
            w = sph_weight(numpy.sqrt(d2) * t.inv_h, kernel)
            numpy.add.at(a_n, i, w)
            numpy.add.at(a_m, i, m[j] * w)
            if a_v is not None:
                numpy.add.at(a_v, i, vol[j] * w)
        number, rho_sum = sigma * a_n, sigma * a_m
        shepard = None if a_v is None else sigma * a_v
    for v in (number, rho_sum, shepard):
        if v is not None:
            v[somewhere:] = 0.0
    words = _sph_summary(n, somewhere, rows_sorted, number, rho_sum, shepard, rho, surface_below)
    return KernelSums(h, SPH_KERNELS[kid], grid, dimensions, words, density is not None, surface_below, rows_sorted,
                      cell_sorted, number, rho_sum, shepard)


def _uniform_slength(lo, hi):
    """``h=None``: the frame's smoothing length, if its smallest and largest value are equal."""
    if not lo == hi:
        raise ValueError("h=None needs one smoothing length for the frame: slength ranges from %r to %r (a per-particle "
                         "smoothing length is not supported; pass h)" % (lo, hi))
    return float(lo)


def _sph_frame_list(frame_or_arrays, h, where, types, domain, box, dimensions):
    """The selection of `frame_kernel_sums` and `frame_kernel_gradients` and the ``h=None`` rule: ``(arrays, position, box,
    dimensions, h, rows)``."""
    if hasattr(frame_or_arrays, 'particles'):
        frame = frame_or_arrays
        arrays = _particle_arrays(frame.particles)
        types = frame.particles.types if types is None else types
        box = frame.configuration.box if box is None else box
        if frame.configuration.dimensions is not None:
            dimensions = int(frame.configuration.dimensions)
        N = int(frame.particles.N)
    else:
        arrays = dict((k, v) for k, v in frame_or_arrays.items() if v is not None)
        if not arrays:
            raise ValueError("arrays holds no per-particle array")
        N = len(next(iter(arrays.values())))
    if box is None:
        raise ValueError("a kernel sum needs the box")
    if h is None:
        s = arrays.get('slength')
        if s is None or numpy.asarray(s).size == 0:
            h = float(_PARTICLE_FIELDS['slength'][2])
        else:
            s = numpy.asarray(s).reshape(-1).astype(numpy.float64)
            s = s[s == s]                               # (`column_stats`' minimum and maximum: over what is no NaN)
            h = _uniform_slength(float(s.min()) if s.size else numpy.inf, float(s.max()) if s.size else -numpy.inf)
    rows = None
    if where is not None:
        rows = where_rows(arrays, where, types)
    if domain is not None:
        if 'position' not in arrays:
            raise ValueError("a domain needs box and the 'position' array")
        inside = domain_rows(arrays['position'], box, domain, dimensions)
        rows = inside if rows is None else numpy.intersect1d(rows, inside)
    position = arrays.get('position')
    if position is None:
        position = numpy.zeros((N, 3), dtype=numpy.float32)
    return arrays, position, box, dimensions, h, rows


def frame_kernel_sums(frame_or_arrays, h=None, kernel='wendland_c2', cells=None, where=None, types=None, domain=None,
                      surface_below=None, box=None, dimensions=3):
    """`sph_kernel_sums` of a frame's ``position``, ``mass`` and ``density`` over a selection: the host twin of
    `HOOMDTrajectory.frame_kernel_sums_device`, which equals it exactly.  The selection -- `where_rows`, `domain_rows` or
    their intersection, as `frame_neighbours` forms it -- is the list: both ``i`` and ``j`` come from it.  ``h=None``
    takes the frame's ``slength`` if its smallest and largest value (over every row) are equal and raises ValueError if
    they differ; a ``slength`` stored nowhere is the schema default 1.0.  A position that is stored nowhere puts every
    row at the origin; without a ``mass`` array every mass is 1.0, without a ``density`` array there is no volume sum.
    Returns a `KernelSums`."""
    arrays, position, box, dimensions, h, rows = _sph_frame_list(frame_or_arrays, h, where, types, domain, box, dimensions)
    return sph_kernel_sums(position, box, h, mass=arrays.get('mass'), density=arrays.get('density'), rows=rows, cells=cells,
                           dimensions=dimensions, kernel=kernel, surface_below=surface_below)


# ---- SPH sums with a per-particle smoothing length: the definition the GPU pass (`pgsd.fl.PGSDFile.sph_adaptive_sums_device`)
# equals exactly
SPH_MODES = ('gather', 'mean')
_SPHA_SUMMARY_WORDS = 22    # n, nowhere, bad_h, not_finite, surface, deviation_at, deviation_row, count_min, count_max,
#                             count_min_at, 5 x (min, max): slength, number, density, shepard, omega; deviation, pairs


def _sph_mode_id(mode):
    if mode not in SPH_MODES:
        raise ValueError("the mode is one of %s: %r" % (', '.join(SPH_MODES), mode))
    return SPH_MODES.index(mode)


def _spha_column(slength, N=None):
    """A smoothing-length column, checked: ``N`` float32 or float64 values, converted to float64 exactly."""
    s = numpy.asarray(slength)
    if s.dtype not in (numpy.float32, numpy.float64) or (N is not None and s.size != N):
        raise ValueError("slength holds one float32 or float64 value per row of position")
    return s.reshape(-1).astype(numpy.float64)


def _spha_valid(h):
    """Is a smoothing length valid: ``h > 0.0 and h < +inf`` (a NaN is not)."""
    with numpy.errstate(invalid='ignore'):
        return (h > 0.0) & (h < numpy.inf)


def smoothing_range(slength, rows=None):
    """``(n, bad, h_min, h_max)`` of a smoothing-length column over a row list (``None``: every row): the entries, those
    whose ``h`` is not valid (``h > 0.0 and h < +inf``), and the smallest and the largest valid ``h`` as float64
    (``+inf`` and ``-inf`` without one).  A minimum and a maximum: no order enters.  What
    `pgsd.fl.PGSDFile.smoothing_range_device` equals exactly."""
    s = _spha_column(slength)
    if rows is not None:
        s = s[_list_rows(rows, s.shape[0])]
    ok = s[_spha_valid(s)]
    return (int(s.shape[0]), int(s.shape[0] - ok.shape[0]), float(ok.min()) if ok.size else float('inf'),
            float(ok.max()) if ok.size else float('-inf'))


def _spha_sigma_rows(kid, h, dimensions):
    """`sph_sigma` of every valid ``h`` of an array, in exactly that function's association; ``+0.0`` elsewhere."""
    h = numpy.where(_spha_valid(h), h, 1.0)
    if int(dimensions) == 3:
        return (21.0 / (16.0 * numpy.pi * (h * h * h))) if kid == 0 else (1.0 / (numpy.pi * (h * h * h)))
    return (7.0 / (4.0 * numpy.pi * (h * h))) if kid == 0 else (10.0 / (7.0 * numpy.pi * (h * h)))


class AdaptiveSums(object):
    """The SPH sums of a list in cell order with a per-particle smoothing length (`sph_adaptive_sums`).

    Attributes:
        h_max (float), kernel (str), mode (str), grid (``(cx, cy, cz)``), dimensions (int), surface_below (float or
            ``None``), volume (bool: was a ``density`` given): what was asked; ``h_max`` is the bound the grid was made
            for (the model: the largest valid ``h`` of the list; the GPU: the declared one).
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere).
        slength (float64), count (uint32), number, density, shepard, omega (float64): per entry, in list order: its
            ``h``, the contributing candidates (itself among them) and the sums; ``+0.0`` (``slength``: as stored) for an
            entry nowhere or with an invalid ``h``.  ``shepard`` is ``None`` without ``density``, ``omega`` in mean mode.
            Numpy arrays from the model; from the GPU ``None`` unless ``return_rows`` left them in GPU memory.
        n, nowhere, bad_h (int): the entries, those without a cell, and those that have a cell and an invalid ``h``.
        not_finite (int): the entries with a cell and a valid ``h`` (the *live* ones) whose ``density`` is NaN or infinite.
        surface (int or ``None``): the live entries with ``shepard < surface_below``.
        deviation, deviation_at, deviation_row: `KernelSums`' over the live entries.
        count_min, count_max, count_min_at: over the live entries; the smaller list position on a tie; ``None`` without one.
        pairs (int): the exact sum of ``count``.
        slength_min, slength_max, number_min, ..., omega_max (float): over the live entries, by strict compares from
            ``+inf`` / ``-inf`` (a NaN never replaces a value); ``shepard``'s ``None`` without ``density``, ``omega``'s
            ``None`` in mean mode.
    """

    __slots__ = ('h_max', 'kernel', 'mode', 'grid', 'dimensions', 'surface_below', 'volume', 'rows', 'cell', 'slength',
                 'count', 'number', 'density', 'shepard', 'omega', 'n', 'nowhere', 'bad_h', 'not_finite', 'surface',
                 'deviation', 'deviation_at', 'deviation_row', 'count_min', 'count_max', 'count_min_at', 'pairs',
                 'slength_min', 'slength_max', 'number_min', 'number_max', 'density_min', 'density_max', 'shepard_min',
                 'shepard_max', 'omega_min', 'omega_max', '_words')

    def __init__(self, h_max, kernel, mode, grid, dimensions, summary, volume, surface_below=None, rows=None, cell=None,
                 slength=None, count=None, number=None, density=None, shepard=None, omega=None):
        """``summary``: the 22 uint64 words of `pgsd_sph_adaptive_sums_device`."""
        s = numpy.ascontiguousarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _SPHA_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _SPHA_SUMMARY_WORDS)
        self._words = s.copy()
        _sph_kernel_id(kernel), _sph_mode_id(mode)
        self.h_max, self.kernel, self.mode = float(h_max), kernel, mode
        self.dimensions, self.volume = int(dimensions), bool(volume)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.surface_below = None if surface_below is None else float(surface_below)
        self.n, self.nowhere, self.bad_h, self.not_finite = int(s[0]), int(s[1]), int(s[2]), int(s[3])
        self.surface = int(s[4]) if self.volume and self.surface_below is not None else None
        found = self.volume and int(s[5]) != _NEIGHBOURS_NONE
        f = s[10:21].view(numpy.float64)
        self.deviation = float(f[10]) if found else None
        self.deviation_at, self.deviation_row = (int(s[5]), int(s[6])) if found else (None, None)
        some = int(s[9]) != _NEIGHBOURS_NONE
        self.count_min, self.count_max, self.count_min_at = (int(s[7]), int(s[8]), int(s[9])) if some else (None, None, None)
        self.pairs = int(s[21])
        self.slength_min, self.slength_max, self.number_min, self.number_max = (float(v) for v in f[:4])
        self.density_min, self.density_max = float(f[4]), float(f[5])
        self.shepard_min, self.shepard_max = (float(f[6]), float(f[7])) if self.volume else (None, None)
        self.omega_min, self.omega_max = (float(f[8]), float(f[9])) if mode == 'gather' else (None, None)
        self.rows, self.cell, self.slength, self.count = rows, cell, slength, count
        self.number, self.density, self.shepard, self.omega = number, density, shepard, omega

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return self._words.copy()

    def __repr__(self):
        return ("AdaptiveSums(h_max=%r, kernel=%r, mode=%r, grid=%r, n=%d, nowhere=%d, bad_h=%d, count=[%r, %r], "
                "density=[%r, %r])" % (self.h_max, self.kernel, self.mode, self.grid, self.n, self.nowhere, self.bad_h,
                                       self.count_min, self.count_max, self.density_min, self.density_max))


def _spha_summary(n, somewhere, live, rows_sorted, h, count, number, density, shepard, omega, rho, surface_below):
    """The 22 summary words from the per-entry results (``shepard``, ``rho`` None without a density, ``omega`` None in
    mean mode): no float is summed, so no order enters.  ``live``: the entries that have a cell and a valid ``h``."""
    words = numpy.zeros(_SPHA_SUMMARY_WORDS, dtype=numpy.uint64)
    f = words[10:21].view(numpy.float64)
    words[0], words[1], words[2] = n, n - somewhere, somewhere - int(numpy.count_nonzero(live))
    words[5] = words[6] = words[9] = _NEIGHBOURS_NONE
    f[0:10:2], f[1:10:2], f[10] = numpy.inf, -numpy.inf, 0.0
    words[21] = int(count.astype(numpy.uint64).sum())
    at = numpy.flatnonzero(live)
    if not at.size:
        return words
    with numpy.errstate(invalid='ignore', over='ignore'):
        for k, v in enumerate((h, number, density, shepard, omega)):
            if v is None:
                continue
            v = v[at]
            ok = v[v == v]
            if ok.size:
                f[2 * k], f[2 * k + 1] = min(numpy.inf, ok.min()), max(-numpy.inf, ok.max())
        words[3] = int(numpy.count_nonzero(~numpy.isfinite(density[at])))
        c = count[at]
        words[7], words[8], words[9] = int(c.min()), int(c.max()), int(at[int(numpy.argmin(c))])
        if shepard is not None:
            if surface_below is not None:
                words[4] = int(numpy.count_nonzero(shepard[at] < numpy.float64(surface_below)))
            dev = density[at] - rho[at]
            size = numpy.where(dev == dev, numpy.abs(dev), -1.0)
            k = int(numpy.argmax(size))                 # (the first position that attains the maximum)
            if size[k] >= 0.0:
                words[5], words[6], f[10] = at[k], rows_sorted[at[k]], dev[k]
    return words


def sph_adaptive_sums(position, box, slength, mass=None, density=None, rows=None, cells=None, dimensions=3,
                      kernel='wendland_c2', mode='gather', surface_below=None):
    """The SPH kernel sums of a row list whose smoothing length is stored per particle: per entry ``i`` the neighbour
    count inside its support, the number density, the summation density, the Shepard sum and -- in gather mode -- the
    grad-h factor ``Omega_i = 1 + (h_i / (D rho_i)) sum_j m_j dW_ij/dh_i`` (Springel & Hernquist; Price) every
    variable-``h`` momentum equation divides by.  The definition the GPU pass (`pgsd.fl.PGSDFile.sph_adaptive_sums_device`,
    `HOOMDTrajectory.frame_adaptive_sums_device`) equals exactly, the floats bit for bit.

    Args:
        position, box, mass, density, rows, cells, dimensions, kernel, surface_below: as `sph_kernel_sums` takes them.
        slength: ``N`` float32 or float64 values, converted to float64 exactly.  ``h`` is *valid* when ``h > 0.0 and h <
            +inf``; an entry with an invalid ``h`` is treated like an entry nowhere -- it contributes to nobody and
            every per-entry output of it is ``+0.0`` --, but it is counted in ``bad_h`` (if it has a cell), not in
            ``nowhere``.
        mode: ``'gather'`` (the support of a pair is ``2 h_i``) or ``'mean'`` (``h_i + h_j``, the pair-symmetric form).

    **The grid and the order.**  ``h_max`` is the largest valid ``h`` over the list (ValueError where a list that is not
    empty has none); the grid is that of `sph_kernel_sums` for ``h = h_max`` (``cells`` checked against the range ``2
    h_max``), and so are the cell order, the offsets and THE ORDER of the candidates.

    **One pair**, float64 without contraction; ``d2`` as `sph_kernel_sums`; ``i`` itself and coincident entries are
    candidates.  *gather*: once per entry ``s_i = 2.0*h_i``, ``r2_i = s_i*s_i``, ``inv_i = 1.0/h_i``; ``j`` contributes
    when ``d2 < r2_i``, strictly; ``q = sqrt(d2)*inv_i``, ``w = sph_weight(q)``, ``F = sph_gradient_factor(q)``; ``a_n +=
    w``, ``a_m += m_j*w``, ``a_v += V_j*w``, ``a_o += m_j*(D*w + (q*q)*F)`` with ``D`` 2.0 or 3.0, ``count_i += 1``.  After
    the last candidate ``number = sigma_i*a_n``, ``density = sigma_i*a_m``, ``shepard = sigma_i*a_v`` with ``sigma_i =
    sph_sigma(kernel, h_i, dimensions)`` and ``omega = 1.0 - a_o/(D*a_m)``.  *mean*: ``s = h_i + h_j``, ``hij = 0.5*s``,
    ``ih = 1.0/hij``; ``j`` contributes when ``d2 < s*s``; ``q = sqrt(d2)*ih``, ``w = sph_weight(q)``, ``p = ih*ih`` in 2-D
    and ``(ih*ih)*ih`` in 3-D, ``wp = w*p``; ``a_n += wp``, ``a_m += m_j*wp``, ``a_v += V_j*wp``; afterwards ``number =
    C*a_n`` and so on with ``C = sph_sigma(kernel, 1.0, dimensions)``; there is no ``omega``.

    Returns an `AdaptiveSums`.
    """
    dimensions = int(dimensions)
    kid, mid = _sph_kernel_id(kernel), _sph_mode_id(mode)
    if surface_below is not None:
        surface_below = float(surface_below)
        if surface_below != surface_below:
            raise ValueError("surface_below is a number or None")
    p = numpy.asarray(position)
    N = p.reshape(-1, 3).shape[0] if p.size else 0
    s = _spha_column(slength, N)
    listed, _, _, h_max = smoothing_range(s, rows)
    if listed and not h_max > 0.0:
        raise ValueError("no listed row has a valid smoothing length (finite and positive)")
    if listed:
        asked = _sph_asked(box, h_max, cells, dimensions, kernel)
    else:                                                # (a list of no entry: any grid serves, h_max stays -inf)
        asked = (dimensions, 1.0, kid, 2.0, (1, 1, 1) if cells is None else _order_cells(cells, dimensions))
    t = _sph_list(asked, position, box, rows, (('mass', mass, 1), ('density', density, 1), ('slength', s, 1)))
    grid = asked[4]
    n, rows_sorted, cell_sorted, somewhere = t.n, t.rows_sorted, t.cell_sorted, t.somewhere
    mass, density, h = t.columns
    m = numpy.ones(n, dtype=numpy.float64) if mass is None else mass
    rho = density
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        vol = None if rho is None else m / rho
    valid = _spha_valid(h)
    live = valid & (numpy.arange(n) < somewhere)
    t.xs = numpy.where(valid[:, None], t.xs, numpy.nan)  # an invalid h: no d2 of it passes a compare, in either role
    D = numpy.float64(3.0 if dimensions == 3 else 2.0)
    a_n, a_m = numpy.zeros(n, dtype=numpy.float64), numpy.zeros(n, dtype=numpy.float64)
    a_v = None if vol is None else numpy.zeros(n, dtype=numpy.float64)
    a_o = numpy.zeros(n, dtype=numpy.float64) if mid == 0 else None
    count = numpy.zeros(n, dtype=numpy.uint32)
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        hv = numpy.where(valid, h, 1.0)
        two_h = 2.0 * hv
        r2_i, inv_i = two_h * two_h, 1.0 / hv
        for i, j, d, d2 in _sph_near_pairs(t):
            if mid == 0:
                near = d2 < r2_i[i]
                i, j, d2 = i[near], j[near], d2[near]
                q = numpy.sqrt(d2) * inv_i[i]
                w = sph_weight(q, kernel)
                F = sph_gradient_factor(q, kernel)
                numpy.add.at(a_o, i, m[j] * (D * w + (q * q) * F))
            else:
                sij = hv[i] + hv[j]
                near = d2 < sij * sij
                i, j, d2, sij = i[near], j[near], d2[near], sij[near]
                ih = 1.0 / (0.5 * sij)
                w = sph_weight(numpy.sqrt(d2) * ih, kernel)
                w = w * ((ih * ih) * ih if dimensions == 3 else ih * ih)
            numpy.add.at(a_n, i, w)
            numpy.add.at(a_m, i, m[j] * w)
            if a_v is not None:
                numpy.add.at(a_v, i, vol[j] * w)
            count += numpy.bincount(i, minlength=n).astype(numpy.uint32)
        scale = _spha_sigma_rows(kid, h, dimensions) if mid == 0 else numpy.float64(sph_sigma(kernel, 1.0, dimensions))
        number, rho_sum = scale * a_n, scale * a_m
        shepard = None if a_v is None else scale * a_v
        omega = None if a_o is None else 1.0 - a_o / (D * a_m)
    for v in (number, rho_sum, shepard, omega):
        if v is not None:
            v[~live] = 0.0
    words = _spha_summary(n, somewhere, live, rows_sorted, h, count, number, rho_sum, shepard, omega, rho, surface_below)
    return AdaptiveSums(h_max, SPH_KERNELS[kid], SPH_MODES[mid], grid, dimensions, words, density is not None, surface_below,
                        rows_sorted, cell_sorted, h, count, number, rho_sum, shepard, omega)


def frame_adaptive_sums(frame_or_arrays, kernel='wendland_c2', mode='gather', cells=None, where=None, types=None, domain=None,
                        surface_below=None, box=None, dimensions=3):
    """`sph_adaptive_sums` of a frame's ``position``, ``slength``, ``mass`` and ``density`` over a selection: the host twin
    of `HOOMDTrajectory.frame_adaptive_sums_device`, which equals it exactly.  The selection is `frame_kernel_sums`' and
    is the list: both ``i`` and ``j`` come from it, and so does ``h_max``.  A ``slength`` stored nowhere is the schema
    default 1.0 in every row; position, mass and density as `frame_kernel_sums`.  Returns an `AdaptiveSums`."""
    arrays, position, box, dimensions, _, rows = _sph_frame_list(frame_or_arrays, 1.0, where, types, domain, box, dimensions)
    N = len(numpy.asarray(position).reshape(-1, 3)) if numpy.asarray(position).size else 0
    s = arrays.get('slength')
    if s is None or numpy.asarray(s).size == 0:
        s = numpy.full(N, _PARTICLE_FIELDS['slength'][2], dtype=numpy.float32)
    return sph_adaptive_sums(position, box, s, mass=arrays.get('mass'), density=arrays.get('density'), rows=rows, cells=cells,
                             dimensions=dimensions, kernel=kernel, mode=mode, surface_below=surface_below)


# ---- SPH kernel gradients: the definition the GPU pass (`pgsd.fl.PGSDFile.sph_gradients_device`) equals exactly
_SPHG_SUMMARY_WORDS = 13    # n, nowhere, not_finite, curl_at, curl_row, normal_at, normal_row, 2 x (min, max), curl2, normal2


def sph_gradient_factor(q, kernel='wendland_c2'):
    """``F(q) = (1/q) dw/dq`` of one pair, float64 without contraction, for ``q = |x_i - x_j| * (1/h)`` below 2, written
    so that only the spline's outer branch divides.  ``wendland_c2``: ``t = 1.0 - 0.5*q``, ``F = -5.0 * ((t*t)*t)``.
    ``cubic_spline``: where ``q < 1.0`` ``F = 2.25*q - 3.0``, otherwise ``u = 2.0 - q`` and ``F = (-0.75*(u*u)) / q``.
    The gradient of the kernel is ``grad_i W_ij = G * F * d`` with ``d = x_j - x_i`` and `sph_gradient_scale` ``G``."""
    q = numpy.asarray(q, dtype=numpy.float64)
    if _sph_kernel_id(kernel) == 0:
        t = 1.0 - 0.5 * q
        return -5.0 * ((t * t) * t)
    u = 2.0 - q
    with numpy.errstate(divide='ignore', invalid='ignore'):
        return numpy.where(q < 1.0, 2.25 * q - 3.0, (-0.75 * (u * u)) / q)


def sph_gradient_scale(kernel, h, dimensions=3):
    """``G = -((sigma*inv_h)*inv_h)`` with `sph_sigma` and ``inv_h = 1/h``, float64 on the host, formed once."""
    inv_h = numpy.float64(1.0) / numpy.float64(_sph_length(h))
    return float(-((numpy.float64(sph_sigma(kernel, h, dimensions)) * inv_h) * inv_h))


class KernelGradients(object):
    """The SPH kernel gradients of a list in cell order (`sph_kernel_gradients`).

    Attributes:
        h (float), kernel (str), grid (``(cx, cy, cz)``), dimensions (int), volume (bool: was a ``density`` given): what
            was asked; G (float): `sph_gradient_scale`.
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere).
        density_rate, divergence (float64, ``n``), curl, normal (float64, ``n x 3``): per entry, in list order, ``sum_j m_j
            (v_i - v_j) . grad_i W_ij``, ``sum_j V_j (v_j - v_i) . grad_i W_ij``, ``sum_j V_j (v_j - v_i) x grad_i W_ij``
            written as ``grad x u`` and the colour gradient ``sum_j V_j grad_i W_ij`` over the entries inside ``2h``;
            ``+0.0`` for an entry nowhere.  The last three are ``None`` without ``density``.  The six per-entry arrays are
            numpy arrays from the model; from the GPU they are ``None`` unless ``return_rows`` left them in GPU memory.
        n, nowhere (int): the entries, and those without a cell.
        not_finite (int): the entries that have a cell and whose ``density_rate`` is NaN or infinite.
        divergence_min, divergence_max, density_rate_min, density_rate_max (float): over the entries that have a cell, by
            strict compares from ``+inf`` / ``-inf`` (a NaN never replaces a value); the first two ``None`` without
            ``density``.
        curl2, curl_at, curl_row, normal2, normal_at, normal_row: the largest ``(c0*c0 + c1*c1) + c2*c2`` of the ``curl``
            and of the ``normal`` outputs over the entries that have a cell, its list position (the smaller one on a tie,
            a NaN never counts) and its row; all ``None`` without ``density`` or where no entry has a number for it.
    """

    __slots__ = ('h', 'kernel', 'grid', 'dimensions', 'volume', 'G', 'rows', 'cell', 'density_rate', 'divergence', 'curl',
                 'normal', 'n', 'nowhere', 'not_finite', 'divergence_min', 'divergence_max', 'density_rate_min',
                 'density_rate_max', 'curl2', 'curl_at', 'curl_row', 'normal2', 'normal_at', 'normal_row', '_words')

    def __init__(self, h, kernel, grid, dimensions, summary, volume, rows=None, cell=None, density_rate=None,
                 divergence=None, curl=None, normal=None):
        """``summary``: the 13 uint64 words of `pgsd_sph_gradients_device` -- n, nowhere, not_finite, curl_at, curl_row,
        normal_at, normal_row, then as float64 bit patterns the minimum and maximum of divergence and density_rate and
        the largest curl2 and normal2."""
        s = numpy.ascontiguousarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _SPHG_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _SPHG_SUMMARY_WORDS)
        self._words = s.copy()
        self.h, self.kernel, self.dimensions, self.volume = float(h), kernel, int(dimensions), bool(volume)
        self.G = sph_gradient_scale(kernel, h, dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.n, self.nowhere, self.not_finite = int(s[0]), int(s[1]), int(s[2])
        f = s[7:13].view(numpy.float64)
        self.divergence_min, self.divergence_max = (float(f[0]), float(f[1])) if self.volume else (None, None)
        self.density_rate_min, self.density_rate_max = float(f[2]), float(f[3])
        for k, name in enumerate(('curl', 'normal')):
            found = self.volume and int(s[3 + 2 * k]) != _NEIGHBOURS_NONE
            setattr(self, name + '2', float(f[4 + k]) if found else None)
            setattr(self, name + '_at', int(s[3 + 2 * k]) if found else None)
            setattr(self, name + '_row', int(s[4 + 2 * k]) if found else None)
        self.rows, self.cell, self.density_rate = rows, cell, density_rate
        self.divergence, self.curl, self.normal = divergence, curl, normal

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return self._words.copy()

    def __repr__(self):
        return "KernelGradients(h=%r, kernel=%r, grid=%r, n=%d, nowhere=%d, divergence=[%r, %r], density_rate=[%r, %r])" % (
            self.h, self.kernel, self.grid, self.n, self.nowhere, self.divergence_min, self.divergence_max,
            self.density_rate_min, self.density_rate_max)


def _sphg_summary(n, somewhere, rows_sorted, rate, divergence, curl, normal):
    """The summary words from the per-entry results (``divergence``, ``curl``, ``normal`` None without a density): no
    float is summed over the list, so no order enters."""
    words = numpy.zeros(_SPHG_SUMMARY_WORDS, dtype=numpy.uint64)
    f = words[7:13].view(numpy.float64)
    words[0], words[1] = n, n - somewhere
    words[3:7] = _NEIGHBOURS_NONE
    f[0:4:2], f[1:4:2], f[4:6] = numpy.inf, -numpy.inf, 0.0
    with numpy.errstate(invalid='ignore', over='ignore'):
        for k, v in enumerate((divergence, rate)):
            if v is None or not somewhere:
                continue
            v = v[:somewhere]
            ok = v[v == v]
            if ok.size:
                f[2 * k], f[2 * k + 1] = min(numpy.inf, ok.min()), max(-numpy.inf, ok.max())
        words[2] = int(numpy.count_nonzero(~numpy.isfinite(rate[:somewhere])))
        for k, v in enumerate((curl, normal)):
            if v is None or not somewhere:
                continue
            v = v[:somewhere]
            norm2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            size = numpy.where(norm2 == norm2, norm2, -1.0)
            at = int(numpy.argmax(size))                # (the first position that attains the maximum)
            if size[at] >= 0.0:
                words[3 + 2 * k], words[4 + 2 * k], f[4 + k] = at, rows_sorted[at], norm2[at]
    return words


def sph_kernel_gradients(position, velocity, box, h, mass=None, density=None, rows=None, cells=None, dimensions=3,
                         kernel='wendland_c2'):
    """The SPH kernel gradients of a row list: per entry ``i`` the density rate of the continuity equation ``sum_j m_j
    (v_i - v_j) . grad_i W_ij``, the velocity divergence ``sum_j V_j (v_j - v_i) . grad_i W_ij``, the curl (the
    vorticity) ``sum_j V_j grad_i W_ij x (v_j - v_i)`` and the colour gradient ``sum_j V_j grad_i W_ij`` (it points into
    the fluid at a free surface) over the entries ``j`` inside the kernel support ``2h``, and over the list the ranges of
    the two scalars and the largest curl and normal with their rows.  The definition the GPU pass
    (`pgsd.fl.PGSDFile.sph_gradients_device`, `HOOMDTrajectory.frame_kernel_gradients_device`) equals exactly, the floats
    bit for bit.

    Args:
        position: ``N x 3`` float32 or float64; velocity: ``N x 3`` float32 or float64, or ``None``: the zero vector.
        box, h, mass, density, rows, cells, dimensions, kernel: `sph_kernel_sums`'.  The grid, the support ``2h``, ``r2``,
            ``inv_h``, ``sigma``, the list in cell order, THE ORDER of the candidates and every refusal are its own.
            Without ``density`` only ``density_rate`` is formed.

    **One pair**, float64 throughout without contraction, float32 inputs converted exactly before any subtraction: ``d =
    pair_displacement(x_i, x_j)``, ``d2 = (dx*dx + dy*dy) + dz*dz``; ``j`` contributes when ``d2 < r2``, strictly; ``i``
    itself and coincident entries are candidates like any other (their ``d`` is zero and so are their terms); ``rr =
    sqrt(d2)``, ``q = rr * inv_h``, ``F = sph_gradient_factor(q)``; ``e_k = F * d_k`` -- the true gradient is ``grad_i W_ij =
    G * e`` with `sph_gradient_scale` ``G`` --; ``u_k = v_j[k] - v_i[k]``; ``dot = (u0*e0 + u1*e1) + u2*e2``; ``c0 = e1*u2 -
    e2*u1``, ``c1 = e2*u0 - e0*u2``, ``c2 = e0*u1 - e1*u0``; ``V_j = m_j / rho_j`` as in the sums.  Eight accumulators per
    entry start at ``+0.0`` and add in the defined order: ``a_r += m_j * dot``, ``a_d += V_j * dot``, ``a_w[k] += V_j *
    c_k``, ``a_c[k] += V_j * e_k``.  After the last candidate ``density_rate = -(G*a_r)``, ``divergence = G*a_d``,
    ``curl[k] = G*a_w[k]``, ``normal[k] = G*a_c[k]``.  In 2-D ``d_z`` is 0 and nothing else is special-cased.  An entry
    without a cell contributes to nobody and all its values are ``+0.0``.

    Returns a `KernelGradients`.
    """
    asked = _sph_asked(box, h, cells, dimensions, kernel)
    t = _sph_list(asked, position, box, rows, (('mass', mass, 1), ('density', density, 1), ('velocity', velocity, 3)))
    dimensions, h, kid, grid = asked[0], asked[1], asked[2], asked[4]
    n, somewhere = t.n, t.somewhere
    mass, rho, v = t.columns
    m = numpy.ones(n, dtype=numpy.float64) if mass is None else mass
    v = numpy.zeros((n, 3), dtype=numpy.float64) if v is None else v
    G = numpy.float64(-((t.sigma * t.inv_h) * t.inv_h))
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        vol = None if rho is None else m / rho
    a_r = numpy.zeros(n, dtype=numpy.float64)
    a_d = None if vol is None else numpy.zeros(n, dtype=numpy.float64)
    a_w = None if vol is None else [numpy.zeros(n, dtype=numpy.float64) for _ in range(3)]
    a_c = None if vol is None else [numpy.zeros(n, dtype=numpy.float64) for _ in range(3)]
    with numpy.errstate(invalid='ignore', over='ignore'):
        for i, j, d, d2 in _sph_near_pairs(t):
            F = sph_gradient_factor(numpy.sqrt(d2) * t.inv_h, kernel)
            e = [F * d[0], F * d[1], F * d[2]]
            u = [v[j, 0] - v[i, 0], v[j, 1] - v[i, 1], v[j, 2] - v[i, 2]]
            dot = (u[0] * e[0] + u[1] * e[1]) + u[2] * e[2]
            numpy.add.at(a_r, i, m[j] * dot)
            if vol is not None:
                V = vol[j]
                c = [e[1] * u[2] - e[2] * u[1], e[2] * u[0] - e[0] * u[2], e[0] * u[1] - e[1] * u[0]]
                numpy.add.at(a_d, i, V * dot)
                for k in range(3):
                    numpy.add.at(a_w[k], i, V * c[k])
                for k in range(3):
                    numpy.add.at(a_c[k], i, V * e[k])
        rate = -(G * a_r)
        divergence = None if vol is None else G * a_d
        curl = None if vol is None else numpy.stack([G * a for a in a_w], axis=1)
        normal = None if vol is None else numpy.stack([G * a for a in a_c], axis=1)
    for a in (rate, divergence, curl, normal):
        if a is not None:
            a[somewhere:] = 0.0
    words = _sphg_summary(n, somewhere, t.rows_sorted, rate, divergence, curl, normal)
    return KernelGradients(h, SPH_KERNELS[kid], grid, dimensions, words, rho is not None, t.rows_sorted, t.cell_sorted, rate,
                           divergence, curl, normal)


def frame_kernel_gradients(frame_or_arrays, h=None, kernel='wendland_c2', cells=None, where=None, types=None, domain=None,
                           box=None, dimensions=3):
    """`sph_kernel_gradients` of a frame's ``position``, ``velocity``, ``mass`` and ``density`` over a selection: the host
    twin of `HOOMDTrajectory.frame_kernel_gradients_device`, which equals it exactly.  The selection, the ``h=None`` rule,
    the refusals and the defaults are `frame_kernel_sums`'; a velocity that is stored nowhere is the zero vector.
    Returns a `KernelGradients`."""
    arrays, position, box, dimensions, h, rows = _sph_frame_list(frame_or_arrays, h, where, types, domain, box, dimensions)
    return sph_kernel_gradients(position, arrays.get('velocity'), box, h, mass=arrays.get('mass'),
                                density=arrays.get('density'), rows=rows, cells=cells, dimensions=dimensions, kernel=kernel)


# ---- SPH gradient tensors: the definition the GPU pass (`pgsd.fl.PGSDFile.sph_tensors_device`) equals exactly
_SPHT_SUMMARY_WORDS = 14    # n, nowhere, not_finite, uncorrected, det_at, det_row, shear_at, shear_row, det and trace (min, max), shear, 0


def _sph_det_min(det_min):
    """``det_min`` as a float, a number that is at least 0."""
    d = float(det_min)
    if not d >= 0.0:
        raise ValueError("det_min is a number, at least 0: %r" % (det_min,))
    return d


class KernelTensors(object):
    """The SPH gradient tensors of a list in cell order (`sph_gradient_tensors`).

    Attributes:
        h (float), kernel (str), grid (``(cx, cy, cz)``), dimensions (int), det_min (float): what was asked; G (float):
            `sph_gradient_scale`.
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere).
        correction (float64, ``n x 6``: xx, xy, xz, yy, yz, zz): the kernel-gradient correction matrix ``L_i``, the inverse
            of ``B_i = sum_j V_j d (x) grad_i W_ij``; the identity (2-D: ``diag(1, 1, 0)``) where the entry stayed
            uncorrected.
        determinant (float64, ``n``): ``det B_i`` (2-D: of its x-y block).
        velocity_gradient (float64, ``n x 9``, row-major ``dv_a/dx_b``): the corrected tensor ``D_i = R_i L_i``; the
            uncorrected ``R_i`` where the entry stayed uncorrected.
        shear_rate (float64, ``n``): ``sqrt(2 S:S)`` of the symmetric part of ``D_i``.  All four are ``+0.0`` for an entry
            nowhere; numpy arrays from the model, from the GPU ``None`` unless ``return_rows`` left them in GPU memory.
        n, nowhere (int): the entries, and those without a cell.
        not_finite (int): the entries that have a cell and whose ``shear_rate`` is NaN or infinite.
        uncorrected (int): the entries that have a cell and whose determinant is not inside ``(det_min, inf)``.
        determinant_min, determinant_max, trace_min, trace_max (float): over the entries that have a cell, by strict
            compares from ``+inf`` / ``-inf`` in which ``-0.0`` is below ``+0.0`` (a NaN never replaces a value); the
            trace is ``(D00 + D11) + D22``.
        det_at, det_row: the list position of the smallest determinant (a strict compare from ``+inf``, the smaller
            position on a tie, a NaN never counts) and its row; ``None`` without one.
        shear, shear_at, shear_row: the largest ``shear_rate`` over the entries that have a cell, its list position (the
            smaller one on a tie, a NaN never counts) and its row; ``None`` without one.
    """

    __slots__ = ('h', 'kernel', 'grid', 'dimensions', 'det_min', 'G', 'rows', 'cell', 'correction', 'determinant',
                 'velocity_gradient', 'shear_rate', 'n', 'nowhere', 'not_finite', 'uncorrected', 'determinant_min',
                 'determinant_max', 'trace_min', 'trace_max', 'det_at', 'det_row', 'shear', 'shear_at', 'shear_row', '_words')

    def __init__(self, h, kernel, grid, dimensions, summary, det_min=0.25, rows=None, cell=None, correction=None,
                 determinant=None, velocity_gradient=None, shear_rate=None):
        """``summary``: the 14 uint64 words of `pgsd_sph_tensors_device` -- n, nowhere, not_finite, uncorrected, det_at,
        det_row, shear_at, shear_row, then as float64 bit patterns the minimum and maximum of the determinant and of the
        trace and the largest shear rate, then 0."""
        s = numpy.ascontiguousarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _SPHT_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _SPHT_SUMMARY_WORDS)
        self._words = s.copy()
        self.h, self.kernel, self.dimensions, self.det_min = float(h), kernel, int(dimensions), _sph_det_min(det_min)
        self.G = sph_gradient_scale(kernel, h, dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.n, self.nowhere, self.not_finite, self.uncorrected = int(s[0]), int(s[1]), int(s[2]), int(s[3])
        f = s[8:13].view(numpy.float64)
        self.determinant_min, self.determinant_max, self.trace_min, self.trace_max = (float(v) for v in f[:4])
        found = int(s[4]) != _NEIGHBOURS_NONE
        self.det_at, self.det_row = (int(s[4]), int(s[5])) if found else (None, None)
        found = int(s[6]) != _NEIGHBOURS_NONE
        self.shear = float(f[4]) if found else None
        self.shear_at, self.shear_row = (int(s[6]), int(s[7])) if found else (None, None)
        self.rows, self.cell, self.correction, self.determinant = rows, cell, correction, determinant
        self.velocity_gradient, self.shear_rate = velocity_gradient, shear_rate

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return self._words.copy()

    def __repr__(self):
        return "KernelTensors(h=%r, kernel=%r, grid=%r, n=%d, nowhere=%d, uncorrected=%d, determinant=[%r, %r], shear=%r)" % (
            self.h, self.kernel, self.grid, self.n, self.nowhere, self.uncorrected, self.determinant_min,
            self.determinant_max, self.shear)


def _spht_summary(n, somewhere, rows_sorted, ok, det, trace, shear):
    """The summary words from the per-entry results: no float is summed over the list, so no order enters."""
    words = numpy.zeros(_SPHT_SUMMARY_WORDS, dtype=numpy.uint64)
    f = words[8:13].view(numpy.float64)
    words[0], words[1] = n, n - somewhere
    words[4:8] = _NEIGHBOURS_NONE
    f[0:4:2], f[1:4:2], f[4] = numpy.inf, -numpy.inf, 0.0
    if not somewhere:
        return words
    with numpy.errstate(invalid='ignore', over='ignore'):
        for k, v in enumerate((det, trace)):
            v = v[:somewhere]
            kept = v[v == v]
            if kept.size:
                # (-0.0 is below +0.0: both occur, and the bound of a parallel reduction must not depend on an order)
                zeros = numpy.signbit(kept[kept == 0.0])
                lo, hi = min(numpy.inf, kept.min()), max(-numpy.inf, kept.max())
                f[2 * k] = (-0.0 if zeros.any() else 0.0) if lo == 0.0 else lo
                f[2 * k + 1] = (0.0 if not zeros.all() else -0.0) if hi == 0.0 else hi
        words[2] = int(numpy.count_nonzero(~numpy.isfinite(shear[:somewhere])))
        words[3] = int(numpy.count_nonzero(~ok[:somewhere]))
        size = numpy.where(det[:somewhere] < numpy.inf, det[:somewhere], numpy.inf)
        at = int(numpy.argmin(size))                    # (the first position that attains the minimum)
        if size[at] < numpy.inf:
            words[4], words[5] = at, rows_sorted[at]
        s = shear[:somewhere]
        size = numpy.where(s == s, s, -numpy.inf)
        at = int(numpy.argmax(size))                    # (the first position that attains the maximum)
        if size[at] > -numpy.inf:
            words[6], words[7], f[4] = at, rows_sorted[at], s[at]
    return words


def _spht_epilogue(G, b, g, dimensions, det_min):
    """What follows the last candidate, for every entry at once: ``b`` the six and ``g`` the nine accumulators (lists of
    float64 arrays).  ``(ok, L (six arrays), det, D (nine arrays), trace, shear_rate)``, every product and sum in the
    association `sph_gradient_tensors` writes out, one rounding each."""
    B00, B01, B02, B11, B12, B22 = (G * a for a in b)
    R = [G * a for a in g]
    zero = numpy.zeros_like(B00)
    if dimensions == 3:
        c00 = B11 * B22 - B12 * B12
        c01 = B02 * B12 - B01 * B22
        c02 = B01 * B12 - B02 * B11
        c11 = B00 * B22 - B02 * B02
        c12 = B01 * B02 - B00 * B12
        c22 = B00 * B11 - B01 * B01
        det = (B00 * c00 + B01 * c01) + B02 * c02
    else:
        det = B00 * B11 - B01 * B01
        c00, c01, c11 = B11, -B01, B00
        c02 = c12 = c22 = zero
    ok = (det > numpy.float64(det_min)) & (det < numpy.inf)
    safe = numpy.where(ok, det, 1.0)                    # (what is not ok is written below, not computed)
    c = (c00, c01, c02, c11, c12, c22)
    identity = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0 if dimensions == 3 else 0.0)
    if dimensions == 3:
        L = [numpy.where(ok, c[k] / safe, identity[k]) for k in range(6)]
    else:
        L = [numpy.where(ok, c[k] / safe, identity[k]) if k in (0, 1, 3) else numpy.where(ok, 0.0, identity[k])
             for k in range(6)]
    Lm = ((L[0], L[1], L[2]), (L[1], L[3], L[4]), (L[2], L[4], L[5]))
    D = []
    for a in range(3):
        for col in range(3):
            if dimensions == 3:
                v = (R[3 * a] * Lm[0][col] + R[3 * a + 1] * Lm[1][col]) + R[3 * a + 2] * Lm[2][col]
            elif col < 2:
                v = R[3 * a] * Lm[0][col] + R[3 * a + 1] * Lm[1][col]
            else:
                v = zero
            D.append(numpy.where(ok, v, R[3 * a + col]))
    trace = (D[0] + D[4]) + D[8]
    s01, s02, s12 = 0.5 * (D[1] + D[3]), 0.5 * (D[2] + D[6]), 0.5 * (D[5] + D[7])
    ss = ((D[0] * D[0] + D[4] * D[4]) + D[8] * D[8]) + 2.0 * ((s01 * s01 + s02 * s02) + s12 * s12)
    return ok, L, det, D, trace, numpy.sqrt(2.0 * ss)


def sph_gradient_tensors(position, velocity, box, h, mass=None, density=None, rows=None, cells=None, dimensions=3,
                         kernel='wendland_c2', det_min=0.25):
    """The SPH gradient tensors of a row list: per entry ``i`` the kernel-gradient correction (renormalisation) matrix
    ``L_i``, the inverse of ``B_i = sum_j V_j d (x) grad_i W_ij``, its determinant, the corrected velocity-gradient tensor
    ``D_i = (sum_j V_j (v_j - v_i) (x) grad_i W_ij) L_i`` -- exact for a linear velocity field on any particle arrangement
    -- and the shear rate ``sqrt(2 S:S)`` of its symmetric part, over the entries ``j`` inside the kernel support ``2h``;
    over the list the entries that stayed uncorrected, the ranges of the determinant and of the trace and the largest
    shear rate with its row.  The definition the GPU pass (`pgsd.fl.PGSDFile.sph_tensors_device`,
    `HOOMDTrajectory.frame_gradient_tensors_device`) equals exactly, the floats bit for bit.

    Args:
        position, velocity, box, h, mass, rows, cells, dimensions, kernel: `sph_kernel_gradients`'.  The grid, the support
            ``2h``, ``r2``, ``inv_h``, ``sigma``, ``G``, the list in cell order, THE ORDER of the candidates and every
            refusal are its own.
        density: ``N`` float32 or float64 values, or ``None``: the schema's default, 0.0 in every row (the values that
            result may be infinite or NaN: that is defined behaviour).
        det_min (float): an entry is corrected where ``det_min < det < inf``; a number, at least 0.  The caller's knob,
            not a tuned figure: 0.25 is a convention, an interior particle has ``det`` near 1 and a flat free surface
            about one half.

    **One pair**, float64 throughout without contraction, float32 inputs converted exactly before any subtraction: ``d``,
    ``d2``, the strict test ``d2 < r2``, ``rr``, ``q``, ``F``, ``e_k = F * d_k`` and ``u_k = v_j[k] - v_i[k]`` as in
    `sph_kernel_gradients`; ``i`` itself and coincident entries are candidates like any other; ``V_j = m_j / rho_j``.
    Fifteen accumulators per entry start at ``+0.0`` and add in the defined order: ``b_ab += V_j * (d_a * e_b)`` for ``ab``
    in ``(00, 01, 02, 11, 12, 22)`` and ``g_ab += V_j * (u_a * e_b)`` for all nine ``ab``, row ``a`` the velocity component
    and column ``b`` the derivative direction.

    **After the last candidate**, every product and sum in the association shown: ``B_ab = G*b_ab``, ``R_ab = G*g_ab``
    (``R`` is the uncorrected ``dv_a/dx_b``).  In 3-D ``c00 = B11*B22 - B12*B12``, ``c01 = B02*B12 - B01*B22``, ``c02 =
    B01*B12 - B02*B11``, ``c11 = B00*B22 - B02*B02``, ``c12 = B01*B02 - B00*B12``, ``c22 = B00*B11 - B01*B01`` and ``det =
    (B00*c00 + B01*c01) + B02*c02``.  In 2-D (``d_z`` is 0, so the z row and column of ``B`` vanish) ``det = B00*B11 -
    B01*B01``, ``c00 = B11``, ``c01 = -B01``, ``c11 = B00`` and ``c02 = c12 = c22 = +0.0``.  ``ok = det > det_min and det <
    inf``; a NaN is never ``ok``.  Where ``ok``: ``L_ab = c_ab / det`` (2-D: the three z entries are ``+0.0``, written) and
    ``D_ab = (R_a0*L_0b + R_a1*L_1b) + R_a2*L_2b`` (2-D: ``D_ab = R_a0*L_0b + R_a1*L_1b`` for ``b < 2`` and ``D_a2 = +0.0``,
    written).  Where not ``ok``: ``L`` is the identity (2-D: ``diag(1, 1, 0)``) and ``D_ab = R_ab``, both written, not
    computed.  Then ``trace = (D00 + D11) + D22``, ``s01 = 0.5*(D01 + D10)``, ``s02 = 0.5*(D02 + D20)``, ``s12 = 0.5*(D12 +
    D21)``, ``ss = ((D00*D00 + D11*D11) + D22*D22) + 2.0*((s01*s01 + s02*s02) + s12*s12)`` and ``shear_rate =
    sqrt(2.0*ss)``.  An entry without a cell contributes to nobody and all its values are ``+0.0``, written.

    Returns a `KernelTensors`.
    """
    asked = _sph_asked(box, h, cells, dimensions, kernel)
    det_min = _sph_det_min(det_min)
    t = _sph_list(asked, position, box, rows, (('mass', mass, 1), ('density', density, 1), ('velocity', velocity, 3)))
    dimensions, h, kid, grid = asked[0], asked[1], asked[2], asked[4]
    n, somewhere = t.n, t.somewhere
    mass, rho, v = t.columns
    m = numpy.ones(n, dtype=numpy.float64) if mass is None else mass
    rho = numpy.zeros(n, dtype=numpy.float64) if rho is None else rho
    v = numpy.zeros((n, 3), dtype=numpy.float64) if v is None else v
    G = numpy.float64(-((t.sigma * t.inv_h) * t.inv_h))
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        vol = m / rho
    upper = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    b = [numpy.zeros(n, dtype=numpy.float64) for _ in range(6)]
    g = [numpy.zeros(n, dtype=numpy.float64) for _ in range(9)]
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i, j, d, d2 in _sph_near_pairs(t):
            F = sph_gradient_factor(numpy.sqrt(d2) * t.inv_h, kernel)
            e = [F * d[0], F * d[1], F * d[2]]
            u = [v[j, 0] - v[i, 0], v[j, 1] - v[i, 1], v[j, 2] - v[i, 2]]
            V = vol[j]
            for k, (r, c) in enumerate(upper):
                numpy.add.at(b[k], i, V * (d[r] * e[c]))
            for r in range(3):
                for c in range(3):
                    numpy.add.at(g[3 * r + c], i, V * (u[r] * e[c]))
        ok, L, det, D, trace, shear = _spht_epilogue(G, b, g, dimensions, det_min)
    correction, gradient = numpy.stack(L, axis=1), numpy.stack(D, axis=1)
    for a in (correction, det, gradient, trace, shear):
        a[somewhere:] = 0.0
    words = _spht_summary(n, somewhere, t.rows_sorted, ok, det, trace, shear)
    return KernelTensors(h, SPH_KERNELS[kid], grid, dimensions, words, det_min, t.rows_sorted, t.cell_sorted, correction, det,
                         gradient, shear)


def frame_gradient_tensors(frame_or_arrays, h=None, kernel='wendland_c2', det_min=0.25, cells=None, where=None, types=None,
                           domain=None, box=None, dimensions=3):
    """`sph_gradient_tensors` of a frame's ``position``, ``velocity``, ``mass`` and ``density`` over a selection: the host
    twin of `HOOMDTrajectory.frame_gradient_tensors_device`, which equals it exactly.  The selection, the ``h=None`` rule,
    the refusals and the defaults are `frame_kernel_gradients`'; a velocity that is stored nowhere is the zero vector, a
    mass 1.0 and a density the schema's 0.0.  Returns a `KernelTensors`."""
    arrays, position, box, dimensions, h, rows = _sph_frame_list(frame_or_arrays, h, where, types, domain, box, dimensions)
    return sph_gradient_tensors(position, arrays.get('velocity'), box, h, mass=arrays.get('mass'),
                                density=arrays.get('density'), rows=rows, cells=cells, dimensions=dimensions, kernel=kernel,
                                det_min=det_min)


# ---- SPH accelerations: the definition the GPU pass (`pgsd.fl.PGSDFile.sph_accelerations_device`) equals exactly
_SPHF_SUMMARY_WORDS = 12   # n, nowhere, not_finite, 3 x (at, row) of total, pressure, viscous, then total2, pressure2, viscous2
_SPHF_NORMS = ('total', 'pressure', 'viscous')


def _sph_viscosity(viscosity):
    """``mu`` as a float, finite and at least 0, or ``None``: no viscous term."""
    if viscosity is None:
        return None
    mu = float(viscosity)
    if not 0.0 <= mu < numpy.inf:
        raise ValueError("viscosity is a finite number, at least 0, or None: %r" % (viscosity,))
    return mu


def _sph_gravity(gravity):
    """``g`` as three finite floats; ``None``: ``(0.0, 0.0, 0.0)``."""
    g = numpy.array([0.0, 0.0, 0.0] if gravity is None else gravity, dtype=numpy.float64).reshape(-1)
    if g.shape[0] != 3 or not numpy.isfinite(g).all():
        raise ValueError("gravity holds three finite numbers, or is None")
    return tuple(float(c) for c in g)


class KernelAccelerations(object):
    """The SPH accelerations of a list in cell order (`sph_accelerations`).

    Attributes:
        h (float), kernel (str), grid (``(cx, cy, cz)``), dimensions (int), viscosity (float or ``None``), gravity (three
            floats): what was asked; G (float): `sph_gradient_scale`.
        rows, cell: the list in cell order and its cell ids (``n_cells``: nowhere).
        pressure_acc, viscous_acc, total (float64, ``n x 3``): per entry, in list order, ``-sum_j m_j (p_i/rho_i^2 +
            p_j/rho_j^2) grad_i W_ij``, Morris' laminar viscous acceleration and ``(pressure_acc + viscous_acc) + g``
            over the entries inside ``2h``; ``+0.0`` for an entry nowhere.  ``viscous_acc`` is ``None`` without a
            viscosity.  The three are numpy arrays from the model; from the GPU they are ``None`` unless ``return_rows``
            left them in GPU memory.
        n, nowhere (int): the entries, and those without a cell.
        not_finite (int): the entries that have a cell and whose ``total`` has a component that is NaN or infinite.
        total2, total_at, total_row, pressure2, pressure_at, pressure_row, viscous2, viscous_at, viscous_row: the largest
            ``(a0*a0 + a1*a1) + a2*a2`` of the ``total``, ``pressure_acc`` and ``viscous_acc`` outputs over the entries
            that have a cell, its list position (the smaller one on a tie, a NaN never counts) and its row; ``None``
            where no entry has a number for it (the last three always without a viscosity).
    """

    __slots__ = ('h', 'kernel', 'grid', 'dimensions', 'viscosity', 'gravity', 'G', 'rows', 'cell', 'pressure_acc', 'viscous_acc',
                 'total', 'n', 'nowhere', 'not_finite', 'total2', 'total_at', 'total_row', 'pressure2', 'pressure_at',
                 'pressure_row', 'viscous2', 'viscous_at', 'viscous_row', '_words')

    def __init__(self, h, kernel, grid, dimensions, summary, viscosity=None, gravity=None, rows=None, cell=None,
                 pressure_acc=None, viscous_acc=None, total=None):
        """``summary``: the 12 uint64 words of `pgsd_sph_accelerations_device` -- n, nowhere, not_finite, the list
        position and the row of the largest total, pressure and viscous acceleration, then as float64 bit patterns the
        three largest squared norms."""
        s = numpy.ascontiguousarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _SPHF_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _SPHF_SUMMARY_WORDS)
        self._words = s.copy()
        self.h, self.kernel, self.dimensions = float(h), kernel, int(dimensions)
        self.viscosity, self.gravity = _sph_viscosity(viscosity), _sph_gravity(gravity)
        self.G = sph_gradient_scale(kernel, h, dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.n, self.nowhere, self.not_finite = int(s[0]), int(s[1]), int(s[2])
        f = s[9:12].view(numpy.float64)
        for k, name in enumerate(_SPHF_NORMS):
            found = int(s[3 + 2 * k]) != _NEIGHBOURS_NONE and (name != 'viscous' or self.viscosity is not None)
            setattr(self, name + '2', float(f[k]) if found else None)
            setattr(self, name + '_at', int(s[3 + 2 * k]) if found else None)
            setattr(self, name + '_row', int(s[4 + 2 * k]) if found else None)
        self.rows, self.cell = rows, cell
        self.pressure_acc, self.viscous_acc, self.total = pressure_acc, viscous_acc, total

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return self._words.copy()

    def force_time_step(self, factor=0.25):
        """``factor * sqrt(h / sqrt(total2))``, the time step the largest acceleration allows; computed on the host from
        the summary; ``None`` without a ``total2`` (``inf`` where it is 0)."""
        if self.total2 is None:
            return None
        with numpy.errstate(divide='ignore'):
            return float(numpy.float64(factor) * numpy.sqrt(numpy.float64(self.h) / numpy.sqrt(numpy.float64(self.total2))))

    def __repr__(self):
        return "KernelAccelerations(h=%r, kernel=%r, grid=%r, n=%d, nowhere=%d, not_finite=%d, total2=%r, pressure2=%r, " \
            "viscous2=%r)" % (self.h, self.kernel, self.grid, self.n, self.nowhere, self.not_finite, self.total2,
                              self.pressure2, self.viscous2)


def _sphf_summary(n, somewhere, rows_sorted, total, pressure_acc, viscous_acc):
    """The summary words from the per-entry results (``viscous_acc`` None without a viscosity): no float is summed over
    the list, so no order enters."""
    words = numpy.zeros(_SPHF_SUMMARY_WORDS, dtype=numpy.uint64)
    f = words[9:12].view(numpy.float64)
    words[0], words[1] = n, n - somewhere
    words[3:9] = _NEIGHBOURS_NONE
    if not somewhere:
        return words
    with numpy.errstate(invalid='ignore', over='ignore'):
        words[2] = int(numpy.count_nonzero(~numpy.isfinite(total[:somewhere]).all(axis=1)))
        for k, v in enumerate((total, pressure_acc, viscous_acc)):
            if v is None:
                continue
            v = v[:somewhere]
            norm2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            size = numpy.where(norm2 == norm2, norm2, -1.0)
            at = int(numpy.argmax(size))                # (the first position that attains the maximum)
            if size[at] >= 0.0:
                words[3 + 2 * k], words[4 + 2 * k], f[k] = at, rows_sorted[at], norm2[at]
    return words


def sph_accelerations(position, velocity, box, h, mass=None, density=None, pressure=None, viscosity=None, gravity=None,
                      rows=None, cells=None, dimensions=3, kernel='wendland_c2'):
    """The SPH accelerations of a row list, the right-hand side of the momentum equation: per entry ``i`` the pressure
    acceleration ``-sum_j m_j (p_i/rho_i^2 + p_j/rho_j^2) grad_i W_ij``, Morris' laminar viscous acceleration for one
    constant ``mu``, ``(1/rho_i) sum_j V_j 2 mu (v_i - v_j) (d . grad_i W_ij) / (|d|^2 + eta^2)``, and their sum with
    gravity over the entries ``j`` inside the kernel support ``2h``, and over the list the largest of the three with
    their rows -- is the frame in equilibrium, where is the largest acceleration, what time step does it allow.  The
    definition the GPU pass (`pgsd.fl.PGSDFile.sph_accelerations_device`, `HOOMDTrajectory.frame_accelerations_device`)
    equals exactly, the floats bit for bit.

    Args:
        position, velocity, box, h, mass, rows, cells, dimensions, kernel: `sph_kernel_gradients`'.  The grid, the support
            ``2h``, ``r2``, ``inv_h``, ``sigma``, ``G``, the list in cell order, THE ORDER of the candidates and every
            refusal are its own.
        density, pressure: ``N`` float32 or float64 values, or ``None``: the schema's default, 0.0 in every row (the values
            that result may be infinite or NaN: that is defined behaviour).
        viscosity (float): the dynamic viscosity ``mu``, finite and at least 0; ``None``: no viscous term is formed and
            ``viscous_acc`` is ``None``.
        gravity: three finite floats; ``None``: ``(0, 0, 0)`` (the addition of ``+0.0`` is still performed).

    **Per entry**, float64, once, before the pair loop: ``A_k = p_k / (rho_k * rho_k)``, ``V_k = m_k / rho_k``.  On the
    host, once: ``eta2 = (0.01*h)*h`` and ``Gv = G * (2.0*mu)``.

    **One pair**, float64 throughout without contraction, float32 inputs converted exactly before any subtraction: ``d``,
    ``d2``, the strict test ``d2 < r2``, ``rr``, ``q`` and ``F`` as in `sph_kernel_gradients`; ``i`` itself and coincident
    entries are candidates like any other (their ``e`` is zero, so an infinite ``S`` gives a NaN there); ``e_k = F *
    d_k``, ``S = A_i + A_j``, ``a_p[k] += m_j * (S * e_k)``; with a viscosity ``K = (F * d2) / (d2 + eta2)``, ``u_k =
    v_j[k] - v_i[k]``, ``a_v[k] += V_j * (K * u_k)``.  After the last candidate ``pressure_acc[k] = -(G * a_p[k])``,
    ``viscous_acc[k] = (Gv * a_v[k]) / rho_i`` and ``total[k] = (pressure_acc[k] + viscous_acc[k]) + g[k]``, or
    ``pressure_acc[k] + g[k]`` without a viscosity.  In 2-D ``d_z`` is 0 and nothing else is special-cased.  An entry
    without a cell contributes to nobody and all its values are ``+0.0``.

    Returns a `KernelAccelerations`.
    """
    asked = _sph_asked(box, h, cells, dimensions, kernel)
    mu, g = _sph_viscosity(viscosity), _sph_gravity(gravity)
    t = _sph_list(asked, position, box, rows, (('mass', mass, 1), ('density', density, 1), ('velocity', velocity, 3),
                                               ('pressure', pressure, 1)))
    dimensions, h, kid, grid = asked[0], asked[1], asked[2], asked[4]
    n, somewhere = t.n, t.somewhere
    mass, rho, v, p = t.columns
    m = numpy.ones(n, dtype=numpy.float64) if mass is None else mass
    rho = numpy.zeros(n, dtype=numpy.float64) if rho is None else rho
    p = numpy.zeros(n, dtype=numpy.float64) if p is None else p
    v = numpy.zeros((n, 3), dtype=numpy.float64) if v is None else v
    G = numpy.float64(-((t.sigma * t.inv_h) * t.inv_h))
    eta2 = (numpy.float64(0.01) * numpy.float64(h)) * numpy.float64(h)
    Gv = None if mu is None else G * (numpy.float64(2.0) * numpy.float64(mu))
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        A, V = p / (rho * rho), m / rho
    a_p = [numpy.zeros(n, dtype=numpy.float64) for _ in range(3)]
    a_v = None if mu is None else [numpy.zeros(n, dtype=numpy.float64) for _ in range(3)]
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i, j, d, d2 in _sph_near_pairs(t):
            F = sph_gradient_factor(numpy.sqrt(d2) * t.inv_h, kernel)
            S, mj = A[i] + A[j], m[j]
            for k in range(3):
                numpy.add.at(a_p[k], i, mj * (S * (F * d[k])))
            if a_v is not None:
                K, Vj = (F * d2) / (d2 + eta2), V[j]
                for k in range(3):
                    numpy.add.at(a_v[k], i, Vj * (K * (v[j, k] - v[i, k])))
        pressure_acc = numpy.stack([-(G * a) for a in a_p], axis=1)
        viscous_acc = None if a_v is None else numpy.stack([(Gv * a) / rho for a in a_v], axis=1)
        total = (pressure_acc if viscous_acc is None else pressure_acc + viscous_acc) + numpy.array(g, dtype=numpy.float64)
    for a in (pressure_acc, viscous_acc, total):
        if a is not None:
            a[somewhere:] = 0.0
    words = _sphf_summary(n, somewhere, t.rows_sorted, total, pressure_acc, viscous_acc)
    return KernelAccelerations(h, SPH_KERNELS[kid], grid, dimensions, words, mu, g, t.rows_sorted, t.cell_sorted, pressure_acc,
                               viscous_acc, total)


def frame_accelerations(frame_or_arrays, h=None, kernel='wendland_c2', viscosity=None, gravity=None, cells=None, where=None,
                        types=None, domain=None, box=None, dimensions=3):
    """`sph_accelerations` of a frame's ``position``, ``velocity``, ``mass``, ``density`` and ``pressure`` over a selection:
    the host twin of `HOOMDTrajectory.frame_accelerations_device`, which equals it exactly.  The selection, the ``h=None``
    rule and the refusals are `frame_kernel_sums`'; a velocity that is stored nowhere is the zero vector, a mass 1.0, a
    density and a pressure the schema's 0.0.  Returns a `KernelAccelerations`."""
    arrays, position, box, dimensions, h, rows = _sph_frame_list(frame_or_arrays, h, where, types, domain, box, dimensions)
    return sph_accelerations(position, arrays.get('velocity'), box, h, mass=arrays.get('mass'), density=arrays.get('density'),
                             pressure=arrays.get('pressure'), viscosity=viscosity, gravity=gravity, rows=rows, cells=cells,
                             dimensions=dimensions, kernel=kernel)


# ---- SPH body forces: the definition the GPU pass (`pgsd.fl.PGSDFile.sph_body_force_device`) equals exactly
_SPHB_SUMMARY_WORDS = 22    # n_t, targets nowhere, n_s, sources nowhere, wetted, pairs, bad, largest (at, row, fp2), 12 sums
_SPHB_PARTS = ('force_pressure', 'force_viscous', 'torque_pressure', 'torque_viscous')


def _sph_about(about):
    """``about`` as three finite floats; ``None``: ``(0.0, 0.0, 0.0)``."""
    c = numpy.array([0.0, 0.0, 0.0] if about is None else about, dtype=numpy.float64).reshape(-1)
    if c.shape[0] != 3 or not numpy.isfinite(c).all():
        raise ValueError("about holds three finite numbers, or is None")
    return tuple(float(v) for v in c)


class KernelBodyForce(object):
    """The force and torque a fluid exerts on a body (`sph_body_force`): two lists in cell order on one grid, the
    *targets* (the body) and the *sources* (the fluid).

    Attributes:
        h (float), kernel (str), grid (``(cx, cy, cz)``), dimensions (int), viscosity (float or ``None``), about (three
            floats): what was asked; G (float): `sph_gradient_scale`.
        rows, cell: the targets in cell order and their cell ids (``n_cells``: nowhere).
        contacts (uint32, ``n``), pressure_acc, viscous_acc (float64, ``n x 3``): per target, in list order, the sources
            inside ``2h`` and the accelerations they cause; ``+0.0`` for a target nowhere.  ``viscous_acc`` is ``None``
            without a viscosity.  Numpy arrays from the model; from the GPU ``None`` unless ``return_rows`` left them in
            GPU memory.
        n, nowhere, n_sources, sources_nowhere (int): the targets and the sources, and those of each without a cell.
        wetted (int): the targets that have a cell and at least one contact; pairs (int): the sum of ``contacts``.
        bad (int): the targets that have a cell and one of whose force or torque terms is NaN or infinite; they count as
            ``+0.0`` in every sum.
        force_pressure, force_viscous, torque_pressure, torque_viscous (three floats each): the ordered sums of ``m_b *
            pressure_acc_b``, ``m_b * viscous_acc_b`` and of ``r_b x`` each over the targets, ``r_b`` the minimum-image
            arm from ``about``; the viscous parts are ``+0.0`` without a viscosity.
        force, torque (three floats each): the pressure part plus the viscous part per component.
        largest2, largest_at, largest_row: the largest ``(fp0*fp0 + fp1*fp1) + fp2*fp2`` of the pressure force of one
            target that has a cell and is not bad, its list position (the smaller one on a tie, a NaN never counts) and
            its row; ``None`` without such a target.
    """

    __slots__ = ('h', 'kernel', 'grid', 'dimensions', 'viscosity', 'about', 'G', 'rows', 'cell', 'contacts', 'pressure_acc',
                 'viscous_acc', 'n', 'nowhere', 'n_sources', 'sources_nowhere', 'wetted', 'pairs', 'bad', 'force_pressure',
                 'force_viscous', 'torque_pressure', 'torque_viscous', 'force', 'torque', 'largest2', 'largest_at',
                 'largest_row', '_words')

    def __init__(self, h, kernel, grid, dimensions, summary, viscosity=None, about=None, rows=None, cell=None, contacts=None,
                 pressure_acc=None, viscous_acc=None):
        """``summary``: the 22 uint64 words of `pgsd_sph_body_force_device` -- the targets, those nowhere, the sources,
        those nowhere, wetted, pairs, bad, the list position, the row and as a float64 bit pattern the squared norm of
        the largest pressure force, then as bit patterns the twelve sums."""
        s = numpy.ascontiguousarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _SPHB_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _SPHB_SUMMARY_WORDS)
        self._words = s.copy()
        self.h, self.kernel, self.dimensions = float(h), kernel, int(dimensions)
        self.viscosity, self.about = _sph_viscosity(viscosity), _sph_about(about)
        self.G = sph_gradient_scale(kernel, h, dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.n, self.nowhere, self.n_sources, self.sources_nowhere = int(s[0]), int(s[1]), int(s[2]), int(s[3])
        self.wetted, self.pairs, self.bad = int(s[4]), int(s[5]), int(s[6])
        found = int(s[7]) != _NEIGHBOURS_NONE
        self.largest_at = int(s[7]) if found else None
        self.largest_row = int(s[8]) if found else None
        self.largest2 = float(s[9:10].view(numpy.float64)[0]) if found else None
        f = s[10:22].view(numpy.float64)
        for k, name in enumerate(_SPHB_PARTS):
            setattr(self, name, tuple(float(v) for v in f[3 * k:3 * k + 3]))
        with numpy.errstate(invalid='ignore', over='ignore'):
            self.force = tuple(float(numpy.float64(a) + numpy.float64(b)) for a, b in zip(self.force_pressure, self.force_viscous))
            self.torque = tuple(float(numpy.float64(a) + numpy.float64(b))
                                for a, b in zip(self.torque_pressure, self.torque_viscous))
        self.rows, self.cell = rows, cell
        self.contacts, self.pressure_acc, self.viscous_acc = contacts, pressure_acc, viscous_acc

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return self._words.copy()

    def __repr__(self):
        return "KernelBodyForce(h=%r, kernel=%r, grid=%r, n=%d, nowhere=%d, n_sources=%d, wetted=%d, pairs=%d, bad=%d, " \
            "force=%r, torque=%r)" % (self.h, self.kernel, self.grid, self.n, self.nowhere, self.n_sources, self.wetted,
                                      self.pairs, self.bad, self.force, self.torque)


def _cross(r, f):
    """``r x f`` of two triples of float64 arrays, one rounding per operation."""
    return (r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0])


def sph_body_force(position, velocity, box, h, body_rows, fluid_rows, mass=None, density=None, pressure=None, viscosity=None,
                   about=None, cells=None, dimensions=3, kernel='wendland_c2'):
    """The force and the torque the fluid exerts on a body: a pair pass between two row lists of one frame on one grid --
    the *targets* ``b`` (``body_rows``) and the *sources* ``f`` (``fluid_rows``) -- with an ordered reduction over the
    targets on top: drag, lift, buoyancy, the load on a wall.  The definition the GPU pass
    (`pgsd.fl.PGSDFile.sph_body_force_device`, `HOOMDTrajectory.frame_body_force_device`) equals exactly, the floats bit for
    bit -- so the ORDER of every sum is part of it.

    Args:
        position, velocity, box, h, mass, density, pressure, viscosity, cells, dimensions, kernel: `sph_accelerations`'.
            The grid, the support ``2h``, ``r2``, ``inv_h``, ``sigma``, ``G``, ``eta2``, ``Gv``, the column defaults and
            every refusal are its own.
        body_rows, fluid_rows: the two lists (any order, repeats allowed), each put into cell order by `cell_order` with
            its own offsets; ``None`` is not accepted for either.  A row may occur in both lists: that is not detected,
            and such a pair is a candidate like any other.
        about: three finite floats, the point the torque is taken about; ``None``: ``(0, 0, 0)``.

    **Candidates** of target ``b``: the sources in the cells of the sums' order around the target's cell, looked up in
    the sources' offsets, inside a cell in ascending position in the sources' list; ``d = pair_displacement(x_b, x_f)`` and
    the test ``d2 < r2`` is strict.  Entries of either list that are nowhere take no part.

    **One pair** ``b <- f``: `sph_accelerations`' arithmetic with ``i = b`` and ``j = f`` -- ``A``, ``V``, ``rho``, ``v``
    and ``m`` of ``b`` from the targets' columns, those of ``f`` from the sources' --: ``contacts[b] += 1``, ``a_p[k] +=
    m_f * (S * e_k)`` with ``S = A_b + A_f`` and, with a viscosity, ``a_v[k] += V_f * (K * (v_f[k] - v_b[k]))``.  After
    the last candidate ``pressure_acc[k] = -(G * a_p[k])`` and ``viscous_acc[k] = (Gv * a_v[k]) / rho_b``; no gravity
    enters.  A target without a cell has every value ``+0.0``.

    **Per target**, float64, one rounding per operation: ``fp[k] = m_b * pressure_acc[k]``, ``fv[k] = m_b *
    viscous_acc[k]``, the arm ``r = pair_displacement(about, x_b)`` (in 2-D ``r_z = 0``), ``tp = (r1*fp2 - r2*fp1, r2*fp0
    - r0*fp2, r0*fp1 - r1*fp0)`` and ``tv`` likewise.  A target with a cell is *bad* if any of its six or twelve terms is
    NaN or infinite; all its terms then count as ``+0.0``.

    **Sums**: each of the twelve (six, and six ``+0.0``, without a viscosity) is `_ordered_sum` of its column over the
    targets' list positions, targets nowhere as ``+0.0``.  Without a target no source is looked at, and none counts as
    nowhere.

    Returns a `KernelBodyForce`.
    """
    asked = _sph_asked(box, h, cells, dimensions, kernel)
    mu, c = _sph_viscosity(viscosity), _sph_about(about)
    if body_rows is None or fluid_rows is None:
        raise ValueError("body_rows and fluid_rows are row lists: None is not accepted for either")
    columns = (('mass', mass, 1), ('density', density, 1), ('velocity', velocity, 3), ('pressure', pressure, 1))
    T = _sph_list(asked, position, box, body_rows, columns)
    S = _sph_list(asked, position, box, fluid_rows, columns)
    dimensions, h, kid, grid = asked[0], asked[1], asked[2], asked[4]

    def filled(t):
        mass, rho, v, p = t.columns
        m = numpy.ones(t.n, dtype=numpy.float64) if mass is None else mass
        rho = numpy.zeros(t.n, dtype=numpy.float64) if rho is None else rho
        p = numpy.zeros(t.n, dtype=numpy.float64) if p is None else p
        v = numpy.zeros((t.n, 3), dtype=numpy.float64) if v is None else v
        with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
            return m, rho, v, p / (rho * rho), m / rho

    m_b, rho_b, v_b, A_b, _ = filled(T)
    m_f, _, v_f, A_f, V_f = filled(S)
    n, somewhere = T.n, T.somewhere
    G = numpy.float64(-((T.sigma * T.inv_h) * T.inv_h))
    eta2 = (numpy.float64(0.01) * numpy.float64(h)) * numpy.float64(h)
    Gv = None if mu is None else G * (numpy.float64(2.0) * numpy.float64(mu))
    contacts = numpy.zeros(n, dtype=numpy.int64)
    a_p = [numpy.zeros(n, dtype=numpy.float64) for _ in range(3)]
    a_v = None if mu is None else [numpy.zeros(n, dtype=numpy.float64) for _ in range(3)]
    zero = numpy.zeros(n, dtype=numpy.float64)
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i, j, d, d2 in _sph_pairs_around(S, T.xs[:somewhere], T.cell_sorted[:somewhere]):
            F = sph_gradient_factor(numpy.sqrt(d2) * T.inv_h, kernel)
            numpy.add.at(contacts, i, 1)
            Sij, mj = A_b[i] + A_f[j], m_f[j]
            for k in range(3):
                numpy.add.at(a_p[k], i, mj * (Sij * (F * d[k])))
            if a_v is not None:
                K, Vj = (F * d2) / (d2 + eta2), V_f[j]
                for k in range(3):
                    numpy.add.at(a_v[k], i, Vj * (K * (v_f[j, k] - v_b[i, k])))
        pressure_acc = numpy.stack([-(G * a) for a in a_p], axis=1)
        viscous_acc = None if a_v is None else numpy.stack([(Gv * a) / rho_b for a in a_v], axis=1)
        for a in (pressure_acc, viscous_acc):
            if a is not None:
                a[somewhere:] = 0.0
        fp = [m_b * pressure_acc[:, k] for k in range(3)]
        r = pair_displacement(numpy.array(c, dtype=numpy.float64), T.xs, T.vectors, dimensions) if n else (zero, zero, zero)
        terms = fp + list(_cross(r, fp))
        if viscous_acc is not None:
            fv = [m_b * viscous_acc[:, k] for k in range(3)]
            terms = fp + fv + list(_cross(r, fp)) + list(_cross(r, fv))
        has = numpy.arange(n) < somewhere
        good = has.copy()
        for t in terms:
            good &= numpy.isfinite(t)
        norm2 = (fp[0] * fp[0] + fp[1] * fp[1]) + fp[2] * fp[2]
    words = numpy.zeros(_SPHB_SUMMARY_WORDS, dtype=numpy.uint64)
    f = words[9:22].view(numpy.float64)
    # (without a target no source is looked at: none counts as nowhere)
    words[0], words[1], words[2], words[3] = n, n - somewhere, S.n, S.n - S.somewhere if n else 0
    words[4] = int(numpy.count_nonzero(has & (contacts >= 1)))
    words[5] = int(contacts.sum())
    words[6] = int(numpy.count_nonzero(has & ~good))
    words[7] = words[8] = _NEIGHBOURS_NONE
    if good.any():
        size = numpy.where(good & (norm2 == norm2), norm2, -1.0)
        at = int(numpy.argmax(size))                    # (the first position that attains the maximum)
        if size[at] >= 0.0:
            words[7], words[8], f[0] = at, T.rows_sorted[at], norm2[at]
    for k, t in enumerate(terms):
        # (the twelve words are force_pressure, force_viscous, torque_pressure, torque_viscous; without a viscosity
        # `terms` holds the first and the third)
        slot = k if viscous_acc is not None else (k if k < 3 else k + 3)
        f[1 + slot] = _ordered_sum(numpy.where(good, t, 0.0))
    return KernelBodyForce(h, SPH_KERNELS[kid], grid, dimensions, words, mu, c, T.rows_sorted, T.cell_sorted,
                           contacts.astype(numpy.uint32), pressure_acc, viscous_acc)


def _sph_frame_arrays(frame_or_arrays, h, types, box, dimensions):
    """`_sph_frame_list` without a selection: ``(arrays, types, position, box, dimensions, h)``."""
    arrays, position, box, dimensions, h, _ = _sph_frame_list(frame_or_arrays, h, None, types, None, box, dimensions)
    if hasattr(frame_or_arrays, 'particles') and types is None:
        types = frame_or_arrays.particles.types
    return arrays, types, position, box, dimensions, h


def frame_body_force(frame_or_arrays, body, fluid, h=None, kernel='wendland_c2', viscosity=None, about=None, cells=None,
                     types=None, domain=None, box=None, dimensions=3):
    """`sph_body_force` of a frame's ``position``, ``velocity``, ``mass``, ``density`` and ``pressure`` over two selections:
    the host twin of `HOOMDTrajectory.frame_body_force_device`, which equals it exactly.  ``body`` and ``fluid`` are
    ``where`` dicts (`where_rows`), both required; with a ``domain`` each selection is intersected with its rows, as
    `frame_kernel_sums` forms its list.  The ``h=None`` rule, the column defaults and the refusals are
    `frame_accelerations`'.  Returns a `KernelBodyForce`."""
    if body is None or fluid is None:
        raise ValueError("body and fluid are where dicts: both are required")
    arrays, types, position, box, dimensions, h = _sph_frame_arrays(frame_or_arrays, h, types, box, dimensions)
    lists = []
    for where in (body, fluid):
        rows = where_rows(arrays, where, types)
        if domain is not None:
            if 'position' not in arrays:
                raise ValueError("a domain needs box and the 'position' array")
            rows = numpy.intersect1d(rows, domain_rows(arrays['position'], box, domain, dimensions))
        lists.append(rows)
    return sph_body_force(position, arrays.get('velocity'), box, h, lists[0], lists[1], mass=arrays.get('mass'),
                          density=arrays.get('density'), pressure=arrays.get('pressure'), viscosity=viscosity, about=about,
                          cells=cells, dimensions=dimensions, kernel=kernel)


# ---- SPH samples: the definition the GPU pass (`pgsd.fl.PGSDFile.sph_samples_device`) equals exactly
_SPHS_SUMMARY_WORDS = 11   # K, nowhere, outside, empty, not_finite, count_max, count_max_at, shepard min, max, density min, max
_SPHS_MAX_VALUES = 4        # value arrays of one call
_SPHS_MAX_WIDTH = 4         # columns of one value array
_SPHS_MAX_COLUMNS = 8       # columns of all of them together
_SPHS_COUNTERS = ('points', 'nowhere', 'outside', 'empty', 'not_finite', 'count_max')


def sample_grid(box, shape, dimensions=3, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0)):
    """The cell-centre points of an ``nx x ny x nz`` lattice over the fractional sub-box ``[lo, hi)`` of ``box``, as
    float64 real coordinates ``(nx*ny*nz) x 3``, x fastest, then y, then z: points for `sph_samples` and its GPU twin,
    which both receive them as plain data.

    The fraction on axis ``a`` is ``f_a = lo_a + (hi_a - lo_a) * ((i_a + 0.5) / n_a)``; the real coordinates come from
    the inverse of `domain_rows`' skew, box rounded to float32 as a file stores it: ``z = f_z*Lz - Lz/2``, ``y = (f_y*Ly -
    Ly/2) + yz*z``, ``x = (f_x*Lx - Lx/2) + ((xz - yz*xy)*z + xy*y)``.  With ``dimensions == 2`` ``nz`` is 1 and ``z`` is
    0."""
    dimensions = int(dimensions)
    if dimensions not in (2, 3):
        raise ValueError("dimensions must be 2 or 3")
    b = numpy.asarray(box, dtype=numpy.float32).reshape(-1)
    if b.shape[0] < 6:
        raise ValueError("box must hold 6 values")
    Lx, Ly, Lz, xy, xz, yz = (numpy.float64(v) for v in b[:6])
    n = tuple(int(v) for v in shape)
    if len(n) != 3 or any(v < 1 for v in n):
        raise ValueError("a sample grid takes three counts (nx, ny, nz), each at least 1: %r" % (shape,))
    if dimensions == 2 and n[2] != 1:
        raise ValueError("dimensions == 2 takes nz == 1: z is not looked at")
    lo = numpy.array(lo, dtype=numpy.float64).reshape(-1)
    hi = numpy.array(hi, dtype=numpy.float64).reshape(-1)
    if lo.shape[0] != 3 or hi.shape[0] != 3 or not (numpy.isfinite(lo).all() and numpy.isfinite(hi).all()):
        raise ValueError("lo and hi hold three finite fractions each")
    f = [lo[a] + (hi[a] - lo[a]) * ((numpy.arange(n[a], dtype=numpy.float64) + 0.5) / numpy.float64(n[a])) for a in range(3)]
    fz, fy, fx = numpy.meshgrid(f[2], f[1], f[0], indexing='ij')
    fx, fy, fz = fx.reshape(-1), fy.reshape(-1), fz.reshape(-1)
    z = numpy.zeros(fx.shape[0], dtype=numpy.float64) if dimensions == 2 else fz * Lz - Lz / 2
    y = (fy * Ly - Ly / 2) + yz * z
    x = (fx * Lx - Lx / 2) + ((xz - yz * xy) * z + xy * y)
    return numpy.stack([x, y, z], axis=1)


class KernelSamples(object):
    """The SPH interpolant of a list in cell order at probe points (`sph_samples`).

    Attributes:
        h (float), kernel (str), grid (``(cx, cy, cz)``: the search grid), dimensions (int), normalise (bool), columns
            (tuple: the width of every value array given): what was asked; sigma (float): `sph_sigma`.
        count (uint32, ``K``), density, shepard (float64, ``K``), values (float64, ``K x C``): per point, in the caller's
            order, the list entries strictly inside ``2h``, ``sigma * sum m_j w``, ``sigma * sum V_j w`` and per column
            ``sigma * sum V_j w f_j`` (with ``normalise``: ``sum V_j w f_j / sum V_j w``); 0 and ``+0.0`` at a point
            nowhere.  numpy arrays from the model, arrays in GPU memory from the GPU.
        points, nowhere, outside, empty, not_finite (int): the points; those with a NaN fraction; those that have a cell
            but whose unwrapped fraction is ``< 0`` or ``>= 1`` on an axis that takes part (the single-shift minimum image
            holds inside the box only: results not to trust); those that have a cell and no entry inside ``2h``; those
            that have a cell and whose ``density``, ``shepard`` or any value is NaN or infinite.
        count_max (int), count_max_at (int or ``None``): the largest ``count`` over the points that have a cell and its
            point, the smaller index on a tie; ``None`` where no point has a cell.
        shepard_min, shepard_max, density_min, density_max (float): over the points that have a cell, by strict compares
            from ``+inf`` / ``-inf`` (a NaN never replaces a value).
    """

    __slots__ = ('h', 'kernel', 'grid', 'dimensions', 'normalise', 'columns', 'sigma', 'count', 'density', 'shepard', 'values',
                 'points', 'nowhere', 'outside', 'empty', 'not_finite', 'count_max', 'count_max_at', 'shepard_min',
                 'shepard_max', 'density_min', 'density_max', '_words')

    def __init__(self, h, kernel, grid, dimensions, summary, normalise=False, columns=(), count=None, density=None,
                 shepard=None, values=None):
        """``summary``: the 11 uint64 words of `pgsd_sph_samples_device` -- K, nowhere, outside, empty, not_finite, the
        largest count and its point, then as float64 bit patterns the minimum and maximum of shepard and of density."""
        s = numpy.ascontiguousarray(summary, dtype=numpy.uint64).reshape(-1)
        if s.shape[0] != _SPHS_SUMMARY_WORDS:
            raise ValueError("the summary holds %d words" % _SPHS_SUMMARY_WORDS)
        self._words = s.copy()
        self.h, self.kernel, self.dimensions, self.normalise = float(h), kernel, int(dimensions), bool(normalise)
        self.sigma = sph_sigma(kernel, h, dimensions)
        self.grid = None if grid is None else tuple(int(v) for v in grid)
        self.columns = tuple(int(c) for c in columns)
        for k, name in enumerate(_SPHS_COUNTERS):
            setattr(self, name, int(s[k]))
        self.count_max_at = None if int(s[6]) == _NEIGHBOURS_NONE else int(s[6])
        f = s[7:11].view(numpy.float64)
        self.shepard_min, self.shepard_max, self.density_min, self.density_max = (float(v) for v in f)
        self.count, self.density, self.shepard, self.values = count, density, shepard, values

    @property
    def summary(self):
        """The uint64 words this was made from."""
        return self._words.copy()

    def field(self, k):
        """The ``K x M_k`` view of value array ``k`` inside ``values``."""
        k = int(k)
        if not 0 <= k < len(self.columns):
            raise ValueError("there are %d value arrays: no array %d" % (len(self.columns), k))
        if self.values is None:
            return None
        first, width, total = sum(self.columns[:k]), self.columns[k], sum(self.columns)
        v = self.values
        if fl is not None and isinstance(v, fl.DeviceBuffer):
            return v.view(shape=(int(v.shape[0]), width), strides=(8 * total, 8), offset_bytes=8 * first)
        return v[:, first:first + width]

    def as_grid(self, name_or_k, shape):
        """``count``, ``density`` or ``shepard`` (by name) or value array ``k`` of the points of `sample_grid` ``(box,
        shape)``, shaped ``(nz, ny, nx)`` (``(nz, ny, nx, M_k)`` for a value array)."""
        a = getattr(self, name_or_k) if name_or_k in ('count', 'density', 'shepard') else self.field(name_or_k)
        nx, ny, nz = (int(v) for v in shape)
        if a is None or nx * ny * nz != int(a.shape[0]):
            raise ValueError("as_grid needs the per-point arrays of %d x %d x %d points" % (nx, ny, nz))
        if fl is not None and isinstance(a, fl.DeviceBuffer):      # (no tensor library: the grid is shaped on the host)
            k = None if a.is_contiguous() else int(name_or_k)
            a = a.to_host() if k is None else self.values.to_host()[:, sum(self.columns[:k]):sum(self.columns[:k + 1])]
        return a.reshape((nz, ny, nx) + tuple(a.shape[1:]))

    def __repr__(self):
        return "KernelSamples(h=%r, kernel=%r, grid=%r, points=%d, nowhere=%d, outside=%d, empty=%d, shepard=[%r, %r])" % (
            self.h, self.kernel, self.grid, self.points, self.nowhere, self.outside, self.empty, self.shepard_min,
            self.shepard_max)


def _sphs_summary(has, outside, count, density, shepard, values):
    """The summary words from the per-point results: no float is summed over the points, so no order enters."""
    words = numpy.zeros(_SPHS_SUMMARY_WORDS, dtype=numpy.uint64)
    f = words[7:11].view(numpy.float64)
    f[0::2], f[1::2] = numpy.inf, -numpy.inf
    words[0], words[1], words[6] = has.shape[0], int(numpy.count_nonzero(~has)), _NEIGHBOURS_NONE
    if not has.any():
        return words
    words[2] = int(numpy.count_nonzero(outside & has))
    words[3] = int(numpy.count_nonzero(has & (count == 0)))
    finite = numpy.isfinite(density) & numpy.isfinite(shepard)
    if values.shape[1]:
        finite &= numpy.isfinite(values).all(axis=1)
    words[4] = int(numpy.count_nonzero(has & ~finite))
    size = numpy.where(has, count.astype(numpy.int64), -1)
    at = int(numpy.argmax(size))                        # (the first point that attains the maximum)
    words[5], words[6] = int(size[at]), at
    for k, v in enumerate((shepard, density)):
        ok = v[has & (v == v)]
        if ok.size:
            f[2 * k], f[2 * k + 1] = min(numpy.inf, ok.min()), max(-numpy.inf, ok.max())
    return words


def _sphs_points(points):
    x = numpy.asarray(points)
    if x.dtype not in (numpy.float32, numpy.float64) or (x.size and (x.ndim != 2 or x.shape[1] != 3)):
        raise ValueError("points holds K x 3 float32 or float64 values")
    return x.astype(numpy.float64).reshape(-1, 3)


def _sphs_values(values, N):
    """``values`` of `sph_samples`, checked: ``(float64 arrays N x M, widths)``."""
    values = tuple(values)
    if len(values) > _SPHS_MAX_VALUES:
        raise ValueError("values holds at most %d arrays: %d" % (_SPHS_MAX_VALUES, len(values)))
    given, widths = [], []
    for k, v in enumerate(values):
        v = numpy.asarray(v)
        width = 1 if v.ndim <= 1 else (int(v.shape[1]) if v.ndim == 2 else 0)
        if v.dtype not in (numpy.float32, numpy.float64) or not 1 <= width <= _SPHS_MAX_WIDTH or v.size != N * width:
            raise ValueError("value %d holds N x M float32 or float64 values, 1 <= M <= %d, one row per row of position"
                             % (k, _SPHS_MAX_WIDTH))
        given.append(v.astype(numpy.float64).reshape(-1, width))
        widths.append(width)
    if sum(widths) > _SPHS_MAX_COLUMNS:
        raise ValueError("the values hold at most %d columns together: %d" % (_SPHS_MAX_COLUMNS, sum(widths)))
    return given, tuple(widths)


def sph_samples(points, position, box, h, values=(), mass=None, density=None, rows=None, cells=None, dimensions=3,
                kernel='wendland_c2', normalise=False):
    """The SPH interpolant of a row list at points of the caller's choosing: per point ``p`` the entries ``j`` of the list
    strictly inside the kernel support ``2h`` of it, the density ``sigma * sum_j m_j W_pj``, the Shepard sum ``sigma *
    sum_j V_j W_pj`` and per value column ``sigma * sum_j V_j W_pj f_j`` (``V_j = m_j / rho_j``) -- the water height at a
    gauge, a pressure profile along a line, the velocity on a slice or a grid to render (`sample_grid`).  The definition
    the GPU pass (`pgsd.fl.PGSDFile.sph_samples_device`, `HOOMDTrajectory.frame_samples_device`) equals exactly, the floats
    bit for bit.

    Args:
        points: ``K x 3`` float32 or float64, converted exactly to float64; every per-point result is in their order.
        position, box, h, mass, rows, cells, dimensions, kernel: `sph_kernel_sums`'.  The grid, the support ``2h``, ``r2``,
            ``inv_h``, ``sigma``, the list in cell order and every refusal are its own.
        density: ``N`` float32 or float64 values, or ``None``: the schema's default, 0.0 in every row (the values that
            result may be infinite or NaN: that is defined behaviour).
        values: up to 4 arrays, each ``N x M`` with ``1 <= M <= 4``, float32 or float64, at most 8 columns together; their
            ``C`` columns are concatenated in the order given.
        normalise (bool): divide every value by the Shepard sum.

    **The point's cell** is ``cell_ids(points, box, grid, dimensions)``.  A point with a NaN fraction is nowhere: its
    ``count`` is 0 and every value ``+0.0``, whatever ``normalise`` says.

    **Candidates**: the cells of `sph_kernel_sums`' defined order around the point's cell (``oz``, inside it ``oy``, inside
    it ``ox``, the wrapped cell), inside a cell ascending list position; ``d = pair_displacement(x_p, x_j)`` and ``j``
    contributes when ``d2 < r2``, strictly.  Entries of the list that are nowhere contribute to no point.

    **One contributing pair**, float64 without contraction, one rounding per written operation: ``rr = sqrt(d2)``, ``q =
    rr * inv_h``, ``w = sph_weight(q)``; ``count += 1``, ``a_m += m_j * w``, ``vw = V_j * w``, ``a_v += vw``, ``a_f[c] +=
    vw * f_j[c]``.  After the last candidate ``density = sigma * a_m``, ``shepard = sigma * a_v`` and ``values[c] = sigma *
    a_f[c]``, or with ``normalise`` ``values[c] = a_f[c] / a_v`` -- what IEEE gives, so a point with no entry in reach is
    ``0/0``, a NaN: the blank value a renderer wants.

    Returns a `KernelSamples`.
    """
    asked = _sph_asked(box, h, cells, dimensions, kernel)
    xp = _sphs_points(points)
    t = _sph_list(asked, position, box, rows, (('mass', mass, 1), ('density', density, 1)))
    N = numpy.asarray(position).size // 3
    given, widths = _sphs_values(values, N)
    dimensions, h, kid, grid = asked[0], asked[1], asked[2], asked[4]
    n, sigma, K, C = t.n, t.sigma, xp.shape[0], sum(widths)
    at = t.rows_sorted.astype(numpy.int64)
    fs = numpy.concatenate([v[at] for v in given], axis=1) if given else numpy.zeros((n, 0), dtype=numpy.float64)
    mass, rho = t.columns
    m = numpy.ones(n, dtype=numpy.float64) if mass is None else mass
    rho = numpy.zeros(n, dtype=numpy.float64) if rho is None else rho
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        vol = m / rho
    n_cells = grid[0] * grid[1] * grid[2]
    ids = cell_ids(xp, box, grid, dimensions)
    has = ids < n_cells
    outside = numpy.zeros(K, dtype=bool)
    with numpy.errstate(invalid='ignore'):
        for s in _wrapped_fractions(xp, box, dimensions, unwrapped=True):
            outside |= (s < 0.0) | (s >= 1.0)
    where = numpy.flatnonzero(has)
    count = numpy.zeros(K, dtype=numpy.uint32)
    a_m, a_v = numpy.zeros(K, dtype=numpy.float64), numpy.zeros(K, dtype=numpy.float64)
    a_f = [numpy.zeros(K, dtype=numpy.float64) for _ in range(C)]
    with numpy.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i, j, d, d2 in _sph_pairs_around(t, xp[where], ids[where]):
            i = where[i]
            w = sph_weight(numpy.sqrt(d2) * t.inv_h, kernel)
            numpy.add.at(count, i, 1)
            numpy.add.at(a_m, i, m[j] * w)
            vw = vol[j] * w
            numpy.add.at(a_v, i, vw)
            for c in range(C):
                numpy.add.at(a_f[c], i, vw * fs[j, c])
        rho_sum, shepard = sigma * a_m, sigma * a_v
        out = numpy.zeros((K, C), dtype=numpy.float64)
        for c in range(C):
            out[:, c] = a_f[c] / a_v if normalise else sigma * a_f[c]
    rho_sum[~has], shepard[~has], out[~has] = 0.0, 0.0, 0.0
    words = _sphs_summary(has, outside, count, rho_sum, shepard, out)
    return KernelSamples(h, SPH_KERNELS[kid], grid, dimensions, words, normalise, widths, count, rho_sum, shepard, out)


def _sphs_fields(fields):
    """``fields`` of `frame_samples`, checked: the names of per-particle float fields of the schema, ``(name, width,
    default)`` each.  The default that stands for a field stored nowhere is one number per field."""
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    if len(names) > _SPHS_MAX_VALUES:
        raise ValueError("fields holds at most %d names: %d" % (_SPHS_MAX_VALUES, len(names)))
    out = []
    for name in names:
        if not isinstance(name, str) or name not in _PARTICLE_FIELDS:
            raise ValueError("%r is not a per-particle attribute of ParticleData" % (name,))
        dt, M, default, _ = _PARTICLE_FIELDS[name]
        default = numpy.asarray(default).reshape(-1)
        if numpy.dtype(dt) != numpy.float32 or (default != default[0]).any():
            raise ValueError("particles/%s is no float field with one default for its columns: it cannot be sampled" % name)
        out.append((name, int(M), float(default[0])))
    if sum(M for _, M, _ in out) > _SPHS_MAX_COLUMNS:
        raise ValueError("the fields hold at most %d columns together: %d" % (_SPHS_MAX_COLUMNS, sum(M for _, M, _ in out)))
    return out


def frame_samples(frame_or_arrays, points, fields=('velocity',), h=None, kernel='wendland_c2', normalise=False, cells=None,
                  where=None, types=None, domain=None, box=None, dimensions=3):
    """`sph_samples` of a frame's ``position``, ``mass``, ``density`` and the per-particle float ``fields`` over a
    selection: the host twin of `HOOMDTrajectory.frame_samples_device`, which equals it exactly.  The selection, the
    ``h=None`` rule and the refusals are `frame_kernel_sums`'; a field that is stored nowhere is its schema default in
    every row (a frame at rest has its velocity elided and samples as zeros), a mass 1.0, a density the schema's 0.0.
    Returns a `KernelSamples`."""
    asked = _sphs_fields(fields)
    arrays, position, box, dimensions, h, rows = _sph_frame_list(frame_or_arrays, h, where, types, domain, box, dimensions)
    N = numpy.asarray(position).size // 3
    values = []
    for name, M, default in asked:
        v = arrays.get(name)
        if v is None or numpy.asarray(v).size == 0 and N:
            v = numpy.full((N, M), default, dtype=numpy.float32)
        values.append(numpy.asarray(v).reshape(N, M))
    return sph_samples(points, position, box, h, values=values, mass=arrays.get('mass'), density=arrays.get('density'),
                       rows=rows, cells=cells, dimensions=dimensions, kernel=kernel, normalise=normalise)


def frame_moments(frame_or_arrays, by_type=True, centre=True, where=None, types=None, domain=None, box=None, dimensions=3):
    """`particle_moments` of a frame's ``mass``, ``velocity``, ``energy``, ``position`` and ``typeid`` over a selection:
    the host twin of `HOOMDTrajectory.frame_moments_device`, which equals it exactly.

    Args:
        frame_or_arrays: a `Frame` (``types``, ``box`` and ``dimensions`` default to its own) or a dict of attribute
            name -> ``N (x M)`` host array; an attribute that is missing is the schema's default.
        by_type (bool): one row per type of ``types``, computed in groups of four consecutive types; ``False``: one row
            for all entries, and no typeid is looked at.
        centre (bool): ``False`` leaves the position out: the first moment is that of the default row, zero.
        where, domain: the selection, as `frame_stats` takes it.

    ``position`` is used as stored, wrapped into the box: in a periodic box the centre of mass is that of the wrapped
    image, and the image flags are not applied.  Returns a `Moments`.

    ValueError: what `where_rows`, `domain_rows` and `particle_moments` refuse; ``by_type`` without ``types``; a domain
    without box or position.
    """
    if hasattr(frame_or_arrays, 'particles'):
        frame = frame_or_arrays
        arrays = _particle_arrays(frame.particles)
        types = frame.particles.types if types is None else types
        box = frame.configuration.box if box is None else box
        if frame.configuration.dimensions is not None:
            dimensions = int(frame.configuration.dimensions)
        N = int(frame.particles.N)
    else:
        arrays = dict((k, v) for k, v in frame_or_arrays.items() if v is not None)
        if not arrays:
            raise ValueError("arrays holds no per-particle array")
        N = len(next(iter(arrays.values())))
    rows = None
    if where is not None:
        rows = where_rows(arrays, where, types)
    if domain is not None:
        if box is None or 'position' not in arrays:
            raise ValueError("a domain needs box and the 'position' array")
        inside = domain_rows(arrays['position'], box, domain, dimensions)
        rows = inside if rows is None else numpy.intersect1d(rows, inside)
    inputs = dict(mass=arrays.get('mass'), velocity=arrays.get('velocity'), energy=arrays.get('energy'),
                  position=arrays.get('position') if centre else None, rows=rows, N=N)
    if not by_type:
        return particle_moments(**inputs)
    if types is None:
        raise ValueError("by_type needs the list of type names (types)")
    typeid = numpy.zeros(N, dtype=numpy.uint32) if arrays.get('typeid') is None else numpy.asarray(arrays['typeid'])
    n = N if rows is None else len(rows)
    parts = [particle_moments(typeid=typeid, type0=t0, n_types=min(_MOMENTS_MAX_TYPES, len(types) - t0), **inputs)
             for t0 in range(0, len(types), _MOMENTS_MAX_TYPES)]
    if not parts:
        return Moments.from_sums([], [], n, numpy.zeros((0, _MOMENTS_QUANTITIES)))
    return Moments.concatenate(parts, n)


# ---- frame displacements: the definition the GPU reduction (`pgsd.fl.PGSDFile.frame_displacements_device`) equals exactly
_DISPLACEMENT_VALUES = 5    # drift x 3, square, largest
_DISPLACEMENT_MAX_TYPES = 4


def box_vectors(box):
    """The six float64 values ``(Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz)`` of a box ``(Lx, Ly, Lz, xy, xz, yz)``: each value is
    converted to float64 first, then one float64 product each.  The unwrap and the fold of `particle_displacements`
    (and of the GPU kernel) take these as given, so the products are rounded once, here."""
    b = numpy.asarray(box, dtype=numpy.float64).reshape(-1)
    if b.shape[0] != 6:
        raise ValueError("a box holds six values (Lx, Ly, Lz, xy, xz, yz)")
    with numpy.errstate(over='ignore', invalid='ignore'):
        return numpy.array([b[0], b[1], b[2], b[3] * b[1], b[4] * b[2], b[5] * b[2]], dtype=numpy.float64)


class Displacements(object):
    """Displacements between two frames per particle type (`particle_displacements`): arrays of one entry (or one row)
    per type.

    Attributes:
        count, bad (int64, T): the entries of the type, and those of them at which a component of the displacement or
            its squared length is not finite.
        largest_entry (int64, T): the smallest entry that attains ``largest`` (a position in the row list when there is
            one, else a row); ``-1`` when the type has no entry whose squared length is a number.
        other (int): the entries of no type of the call.
        drift (float64, T x 3): ``sum d``.  square (float64, T): ``sum |d|^2``.
        largest (float64, T): the largest ``|d|^2`` (infinities included, NaN not); ``-inf`` when there is none.
        msd, mean_drift (properties): ``square / (count - bad)`` and ``drift / (count - bad)``, NaN where that is 0.
        largest_distance (property): ``sqrt(largest)``.

    Both sums are over the finite values only and in `column_stats`' order.
    """

    __slots__ = ('count', 'bad', 'largest_entry', 'other', 'drift', 'square', 'largest')

    def __init__(self, count, bad, largest_entry, other, drift, square, largest):
        self.count = numpy.asarray(count, dtype=numpy.int64).reshape(-1)
        T = self.count.shape[0]
        self.bad = numpy.asarray(bad, dtype=numpy.int64).reshape(T)
        self.largest_entry = numpy.asarray(largest_entry, dtype=numpy.int64).reshape(T)
        self.other = int(other)
        self.drift = numpy.asarray(drift, dtype=numpy.float64).reshape(T, 3)
        self.square = numpy.asarray(square, dtype=numpy.float64).reshape(T)
        self.largest = numpy.asarray(largest, dtype=numpy.float64).reshape(T)

    @classmethod
    def from_sums(cls, count, bad, largest_entry, other, sums):
        """From the ``T x 5`` table of values: drift x 3, square, largest."""
        s = numpy.asarray(sums, dtype=numpy.float64).reshape(-1, _DISPLACEMENT_VALUES)
        return cls(count, bad, largest_entry, other, s[:, 0:3].copy(), s[:, 3].copy(), s[:, 4].copy())

    @property
    def sums(self):
        """The ``T x 5`` table of values: drift x 3, square, largest."""
        return numpy.concatenate([self.drift, self.square[:, None], self.largest[:, None]], axis=1)

    def _per_entry(self, a):
        good = (self.count - self.bad).astype(numpy.float64)
        good = good if a.ndim == 1 else good[:, None]
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(good != 0, a / good, numpy.nan)

    @property
    def msd(self):
        return self._per_entry(self.square)

    @property
    def mean_drift(self):
        return self._per_entry(self.drift)

    @property
    def largest_distance(self):
        with numpy.errstate(invalid='ignore'):
            return numpy.sqrt(self.largest)

    def total(self):
        """All types as one: a `Displacements` of one row whose sums are the types' added in ascending type order by
        plain float64 additions, with the largest ``largest`` (on a tie the smaller entry); ``other`` stays."""
        s = self.sums
        acc = numpy.zeros(4, dtype=numpy.float64)
        best, entry = -numpy.inf, -1
        for t in range(s.shape[0]):
            acc = s[t, 0:4].copy() if t == 0 else acc + s[t, 0:4]
            e = int(self.largest_entry[t])
            if e >= 0 and (entry < 0 or s[t, 4] > best or (s[t, 4] == best and e < entry)):
                best, entry = s[t, 4], e
        return Displacements.from_sums([int(self.count.sum())], [int(self.bad.sum())], [entry], self.other,
                                       numpy.concatenate([acc, [best]]))

    @staticmethod
    def concatenate(parts, n_entries):
        """The `Displacements` of consecutive groups of types (each over the same ``n_entries`` entries) as one."""
        count = numpy.concatenate([p.count for p in parts])
        return Displacements.from_sums(count, numpy.concatenate([p.bad for p in parts]),
                                       numpy.concatenate([p.largest_entry for p in parts]),
                                       int(n_entries) - int(count.sum()), numpy.concatenate([p.sums for p in parts], axis=0))

    def __repr__(self):
        return "Displacements(%s)" % ', '.join(
            "%s=%r" % (name, getattr(self, name).tolist() if name != 'other' else self.other) for name in self.__slots__)


def _displacement_inputs(position_a, position_b, image_a, image_b, vectors_a, vectors_b, minimum_image, dimensions):
    """The inputs of `displacement_vectors`, checked: positions, images (or None), vectors (or None)."""
    pa, pb = numpy.asarray(position_a), numpy.asarray(position_b)
    for p in (pa, pb):
        if p.dtype.type not in (numpy.float32, numpy.float64):
            raise ValueError("displacements take float32 or float64 positions: %s" % p.dtype)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("a position is an N x 3 array")
    if pa.dtype != pb.dtype:
        raise ValueError("displacements take positions of one float type, not float32 and float64 mixed")
    if pa.shape[0] != pb.shape[0]:
        raise ValueError("the frames differ in their number of rows (%d and %d)" % (pa.shape[0], pb.shape[0]))
    images = []
    for im in (image_a, image_b):
        if im is not None:
            im = numpy.asarray(im)
            if im.dtype.type is not numpy.int32:
                raise ValueError("an image holds int32 elements: %s" % im.dtype)
            if im.ndim != 2 or im.shape[1] != 3:
                raise ValueError("an image is an N x 3 array")
            if im.shape[0] != pa.shape[0]:
                raise ValueError("the arrays differ in their number of rows (an image has %d)" % im.shape[0])
        images.append(im)
    if dimensions not in (2, 3):
        raise ValueError("dimensions is 2 or 3: %r" % (dimensions,))
    if minimum_image and (images[0] is not None or images[1] is not None):
        raise ValueError("the minimum image is taken without image flags: pass no image array")
    vectors = []
    for v, needed in ((vectors_a, images[0] is not None), (vectors_b, images[1] is not None or minimum_image)):
        if v is None:
            if needed:
                raise ValueError("an image array and the minimum image need the frame's box vectors (box_vectors)")
        else:
            v = numpy.asarray(v, dtype=numpy.float64).reshape(-1)
            if v.shape[0] != 6:
                raise ValueError("box vectors hold six values (box_vectors)")
        vectors.append(v)
    return pa, pb, images[0], images[1], vectors[0], vectors[1]


def _unwrapped(x, image, v):
    """The three float64 columns of ``x`` unwrapped through ``image`` and the box vectors ``v``."""
    x = [x[:, a].astype(numpy.float64) for a in range(3)]
    if image is None:
        return x
    i = [image[:, a].astype(numpy.float64) for a in range(3)]
    return [x[0] + ((i[0] * v[0] + i[1] * v[3]) + i[2] * v[4]),
            x[1] + (i[1] * v[1] + i[2] * v[5]),
            x[2] + i[2] * v[2]]


def displacement_vectors(position_a, position_b, image_a=None, image_b=None, vectors_a=None, vectors_b=None,
                         minimum_image=False, dimensions=3, rows=None):
    """The per-entry displacement ``d`` of `particle_displacements` as an ``n x 3`` float64 array: what the GPU pass
    stores per entry when it is given an output (``return_rows``), bit for bit."""
    pa, pb, ia, ib, va, vb = _displacement_inputs(position_a, position_b, image_a, image_b, vectors_a, vectors_b,
                                                  minimum_image, dimensions)
    if rows is not None:
        rows = _list_rows(rows, pa.shape[0])
        pa, pb = pa[rows], pb[rows]
        ia, ib = None if ia is None else ia[rows], None if ib is None else ib[rows]
    with numpy.errstate(over='ignore', invalid='ignore', under='ignore', divide='ignore'):
        ua, ub = _unwrapped(pa, ia, va), _unwrapped(pb, ib, vb)
        d = [ub[a] - ua[a] for a in range(3)]
        if minimum_image:
            Lx, Ly, Lz, xyLy, xzLz, yzLz = (numpy.float64(c) for c in vb)
            if dimensions == 3:
                n = numpy.rint(d[2] / Lz)
                d[2] = d[2] - n * Lz
                d[1] = d[1] - n * yzLz
                d[0] = d[0] - n * xzLz
            n = numpy.rint(d[1] / Ly)
            d[1] = d[1] - n * Ly
            d[0] = d[0] - n * xyLy
            n = numpy.rint(d[0] / Lx)
            d[0] = d[0] - n * Lx
    return numpy.stack(d, axis=1)


def particle_displacements(position_a, position_b, image_a=None, image_b=None, vectors_a=None, vectors_b=None,
                           minimum_image=False, dimensions=3, typeid=None, type0=0, n_types=1, rows=None):
    """Drift, squared displacement and the largest move between two frames per particle type: the definition the GPU
    reduction (`pgsd.fl.PGSDFile.frame_displacements_device`, `HOOMDTrajectory.frame_displacements_device`) equals
    exactly, the sums bit for bit.  Row ``k`` of frame a is the particle of row ``k`` of frame b.

    Args:
        position_a, position_b (N x 3): float32 or float64, both the same.
        image_a, image_b (N x 3): int32, or ``None``: the schema's default ``(0, 0, 0)`` in every row.
        vectors_a, vectors_b: `box_vectors` of each frame's box (needed with an image array; ``vectors_b`` with
            ``minimum_image``); the two frames may have different boxes.
        minimum_image (bool): fold the difference into frame b's box (HOOMD's ``minImage``: z, then y, then x; z not in
            two dimensions); allowed only without image arrays.
        typeid (N): uint32 or int32, or ``None``: one group, ``n_types`` is 1.
        type0, n_types, rows: as `particle_moments` takes them.

    Every element is converted to float64 first; no fused multiply-add, and the association is fixed.  With ``i`` the
    image as float64 and ``(Lx, Ly, Lz, xyLy, xzLz, yzLz)`` the frame's vectors::

        u[0] = x[0] + ((i[0]*Lx + i[1]*xyLy) + i[2]*xzLz)
        u[1] = x[1] + (i[1]*Ly + i[2]*yzLz)
        u[2] = x[2] + i[2]*Lz

    and ``u = x`` without an image array (no product is formed: an infinite box value creates no NaN).
    ``d = u_b - u_a``; with ``minimum_image`` and frame b's vectors ``n = rint(d[2] / Lz)``, ``d[2] -= n*Lz``,
    ``d[1] -= n*yzLz``, ``d[0] -= n*xzLz`` (three dimensions only), ``n = rint(d[1] / Ly)``, ``d[1] -= n*Ly``,
    ``d[0] -= n*xyLy``, ``n = rint(d[0] / Lx)``, ``d[0] -= n*Lx``; ``rint`` rounds half to even and every ``-=`` is one
    product and one subtraction.  ``s = (d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]``.

    Per type ``t`` the result (`Displacements`) holds the entries of the type, those of them where a ``d[a]`` or ``s``
    is not finite, the sums of ``d[a]`` and of ``s`` **in `column_stats`' order** over the sequence whose entry ``k`` is
    the value where ``typeid[k] == t`` and the value is finite and ``+0.0`` otherwise, the maximum of ``s`` over the
    entries of the type where ``s`` is no NaN (``-inf`` when there is none) and the smallest entry that attains it
    (``-1``).  ``other`` counts the entries of no type of the range; a negative int32 id is one.

    ValueError: other element types, mixed float types, wrong shapes or lengths, ``minimum_image`` with an image array,
    an image array or ``minimum_image`` without vectors, ``dimensions`` not 2 or 3, ``n_types`` of 0 or above 4, no
    typeid with ``n_types != 1``, what `column_stats` refuses for ``rows``.
    """
    if not isinstance(n_types, (int, numpy.integer)) or not 1 <= n_types <= _DISPLACEMENT_MAX_TYPES:
        raise ValueError("a call takes 1 to 4 types: %r" % (n_types,))
    if not isinstance(type0, (int, numpy.integer)) or not 0 <= type0 < 2 ** 32:
        raise ValueError("type0 is a type id: %r" % (type0,))
    d = displacement_vectors(position_a, position_b, image_a, image_b, vectors_a, vectors_b, minimum_image, dimensions,
                             rows)
    N = numpy.asarray(position_a).shape[0]
    if typeid is not None:
        typeid = numpy.asarray(typeid)
        if typeid.dtype.type not in (numpy.uint32, numpy.int32):
            raise ValueError("typeid holds uint32 or int32 elements: %s" % typeid.dtype)
        if typeid.ndim != 1:
            raise ValueError("typeid is an array of N values")
        if typeid.shape[0] != N:
            raise ValueError("the arrays differ in their number of rows (typeid has %d)" % typeid.shape[0])
    elif n_types != 1:
        raise ValueError("without a typeid there is one group: n_types must be 1")
    if rows is not None:
        rows = _list_rows(rows, N)
    n = d.shape[0]
    with numpy.errstate(over='ignore', invalid='ignore', under='ignore'):
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    values = [d[:, 0], d[:, 1], d[:, 2], s]
    finite = [numpy.isfinite(q) for q in values]
    all_finite = numpy.logical_and.reduce(finite) if n else numpy.zeros(0, dtype=bool)
    if typeid is None:
        group = numpy.zeros(n, dtype=numpy.int64)
    else:
        group = (typeid if rows is None else typeid[rows]).astype(numpy.int64) - int(type0)
    count, bad = numpy.zeros(n_types, numpy.int64), numpy.zeros(n_types, numpy.int64)
    entry = numpy.full(n_types, -1, numpy.int64)
    sums = numpy.zeros((n_types, _DISPLACEMENT_VALUES), dtype=numpy.float64)
    sums[:, 4] = -numpy.inf
    for t in range(n_types):
        mine = group == t
        count[t], bad[t] = mine.sum(), (mine & ~all_finite).sum()
        for q in range(4):
            sums[t, q] = _ordered_sum(numpy.where(mine & finite[q], values[q], 0.0))
        taking = numpy.flatnonzero(mine & ~numpy.isnan(s))
        if taking.size:
            sums[t, 4] = s[taking].max()
            entry[t] = taking[numpy.argmax(s[taking] == sums[t, 4])]
    return Displacements.from_sums(count, bad, entry, n - int(count.sum()), sums)


def _displacement_frame(frame_or_arrays, box):
    """``(arrays, types, box, dimensions, N)`` of one frame of `frame_displacements`."""
    if hasattr(frame_or_arrays, 'particles'):
        frame = frame_or_arrays
        dims = None if frame.configuration.dimensions is None else int(frame.configuration.dimensions)
        return (_particle_arrays(frame.particles), frame.particles.types,
                frame.configuration.box if box is None else box, dims, int(frame.particles.N))
    arrays = dict((k, v) for k, v in frame_or_arrays.items() if v is not None)
    if 'position' not in arrays:
        raise ValueError("arrays holds no 'position'")
    return arrays, None, box, None, len(arrays['position'])


def frame_displacements(frame_a, frame_b, by_type=True, images=True, minimum_image=False, where=None, types=None,
                        domain=None, box=None, dimensions=3):
    """`particle_displacements` from ``frame_a`` to ``frame_b`` over a selection: the host twin of
    `HOOMDTrajectory.frame_displacements_device`, which equals it exactly.

    Args:
        frame_a, frame_b: two `Frame` objects (``types``, the boxes and ``dimensions`` default to their own, frame b's
            where there is one of them) or two dicts of attribute name -> host array holding ``position`` and, where
            stored, ``image`` and ``typeid``.
        by_type (bool): one row per type of ``types``, computed in groups of four consecutive types, by frame b's
            ``typeid``; ``False``: one row for all entries.
        images (bool): ``False`` passes no image array: the difference of the wrapped positions.
        minimum_image (bool): fold the difference into frame b's box; needs ``images=False`` or frames without images.
        where, domain: the selection, as `frame_moments` takes it, evaluated on **frame b**.
        box: one box for both frames, or a pair ``(box_a, box_b)``; needed for dicts with images, the minimum image or
            a domain.

    ValueError: frames of different N; what `where_rows`, `domain_rows` and `particle_displacements` refuse;
    ``by_type`` without ``types``; a domain without box.
    """
    if box is not None and len(box) == 2 and numpy.ndim(box[0]) == 1:
        box_a, box_b = box
    else:
        box_a = box_b = box
    arrays_a, _, box_a, _, N_a = _displacement_frame(frame_a, box_a)
    arrays_b, types_b, box_b, dims_b, N_b = _displacement_frame(frame_b, box_b)
    if N_a != N_b:
        raise ValueError("the frames differ in their number of particles (%d and %d)" % (N_a, N_b))
    types = types_b if types is None else types
    dimensions = dims_b if dims_b is not None else dimensions
    N = N_b
    if 'position' not in arrays_a or 'position' not in arrays_b:
        raise ValueError("both frames need the 'position' array")
    rows = None
    if where is not None:
        rows = where_rows(arrays_b, where, types)
    if domain is not None:
        if box_b is None:
            raise ValueError("a domain needs box and the 'position' array")
        inside = domain_rows(arrays_b['position'], box_b, domain, dimensions)
        rows = inside if rows is None else numpy.intersect1d(rows, inside)
    image_a = arrays_a.get('image') if images else None
    image_b = arrays_b.get('image') if images else None
    inputs = dict(position_a=arrays_a['position'], position_b=arrays_b['position'], image_a=image_a, image_b=image_b,
                  vectors_a=None if box_a is None else box_vectors(box_a),
                  vectors_b=None if box_b is None else box_vectors(box_b),
                  minimum_image=minimum_image, dimensions=dimensions, rows=rows)
    if not by_type:
        return particle_displacements(**inputs)
    if types is None:
        raise ValueError("by_type needs the list of type names (types)")
    typeid = numpy.zeros(N, dtype=numpy.uint32) if arrays_b.get('typeid') is None else numpy.asarray(arrays_b['typeid'])
    n = N if rows is None else len(rows)
    parts = [particle_displacements(typeid=typeid, type0=t0, n_types=min(_DISPLACEMENT_MAX_TYPES, len(types) - t0), **inputs)
             for t0 in range(0, len(types), _DISPLACEMENT_MAX_TYPES)]
    if not parts:
        return Displacements.from_sums([], [], [], n, numpy.zeros((0, _DISPLACEMENT_VALUES)))
    return Displacements.concatenate(parts, n)


class Tracks(object):
    """What `HOOMDTrajectory.read_tracks` / `read_tracks_device` return: ``step`` (host, uint64, one entry per frame),
    ``rows`` (the K rows followed) and one ``F x K (x M)`` array per requested field, as an attribute and as
    ``tracks[name]``; ``fields`` lists the names."""

    def __init__(self, step, rows, fields):
        self.step = step
        self.rows = rows
        self.fields = tuple(fields)
        for name in self.fields:
            setattr(self, name, None)

    def __getitem__(self, name):
        if name not in self.fields:
            raise KeyError(name)
        return getattr(self, name)


class _FrameCursor(object):
    """What ``iter()`` hands out for a trajectory or a subset of one (the role of hoomd.py:471-488):
    it knows how many frames it covers (``len``), yields them in order, and asking it for an iterator
    again starts a fresh pass over the same frames -- so ``list(cursor)`` can be taken more than once."""

    def __init__(self, trajectory, indices):
        self._trajectory = trajectory
        self._indices = indices
        self._at = 0

    def __len__(self):
        return len(self._indices)

    def __iter__(self):
        return _FrameCursor(self._trajectory, self._indices)

    def __next__(self):
        if self._at >= len(self._indices):
            raise StopIteration
        i = self._indices[self._at]
        self._at += 1
        return self._trajectory[i]


class _FrameSubset(object):
    """The frames of a trajectory picked by a sequence of indices: what slicing a
    `HOOMDTrajectory` returns (the role of hoomd.py:491-512).  Supports ``len``, iteration,
    integer indexing and further slicing; frames are read when they are asked for."""

    def __init__(self, trajectory, indices):
        self._trajectory = trajectory
        self._indices = indices

    def __len__(self):
        return len(self._indices)

    def __iter__(self):
        return _FrameCursor(self._trajectory, self._indices)

    def __getitem__(self, key):
        picked = self._indices[key]
        if isinstance(key, slice):
            return _FrameSubset(self._trajectory, picked)
        return self._trajectory[picked]


def _equal(a, b):
    """`numpy.array_equal`, deciding from the first rows where it can: a 10^6-particle array that differs from
    frame 0 differs in its first rows, and comparing all of it costs as much as writing it."""
    if type(a) is not numpy.ndarray or type(b) is not numpy.ndarray:
        if isinstance(a, (int, float, numpy.number)) and isinstance(b, (int, float, numpy.number)):
            return bool(a == b)             # step, dimensions, N: no array is made of two scalars
        a, b = numpy.asarray(a), numpy.asarray(b)
    if a.shape != b.shape:
        return False
    if a.ndim >= 1 and a.shape[0] > 4096 and not (a[:1024] == b[:1024]).all():
        return False
    return bool((a == b).all())


_DEFAULT_AS = {}


def _equiv(a, default):
    """`numpy.array_equiv(a, default)` (default broadcast over the rows), first rows first.  The schema's defaults
    are Python lists and ints: compared as they are, a float32 array is promoted to float64 element by element
    (18 us for 1 024 positions); the default is therefore cast ONCE to the array's type -- when that is exact."""
    a = numpy.asarray(a)
    try:
        key = (a.dtype, default if not isinstance(default, list) else tuple(default))
        d = _DEFAULT_AS.get(key)
    except TypeError:                   # nested / unhashable default: compare the slow way
        key, d = None, None
    if d is None:
        d = numpy.asarray(default)
        if d.dtype.kind in 'biuf' and a.dtype.kind in 'biuf':
            with numpy.errstate(all='ignore'):
                cast = d.astype(a.dtype)
            if cast.shape == d.shape and (cast == d).all():
                d = cast
        if key is not None:
            _DEFAULT_AS[key] = d
    if d.ndim and a.shape[a.ndim - d.ndim:] != d.shape:
        return bool(numpy.array_equiv(a, d))        # not the scalar / one-row defaults of the schema: numpy decides
    # the first row first: an attribute that is set differs from its default there (and a row-broadcast compare of
    # a whole (N, 3) array costs 3-4x a dense one)
    if a.ndim > d.ndim and a.shape[0] > 1 and not (a[0] == d).all():
        return False
    return bool((a == d).all())


def _encode_strings(strings):
    """list[str] -> (n, wid) int8 array, NUL padded (hoomd.py:628-630)."""
    wid = max(len(w.encode('utf-8')) for w in strings) + 1
    b = numpy.array([w.encode('utf-8') for w in strings], dtype=numpy.dtype((bytes, wid)))
    return b.view(dtype=numpy.int8).reshape(len(b), wid)


def _decode_strings(tmp):
    """(n, wid) int8 array, NUL padded -> list[str]: the inverse of `_encode_strings` (hoomd.py:757-759)."""
    tmp = tmp.view(dtype=numpy.dtype((bytes, tmp.shape[1]))).reshape([tmp.shape[0]])
    return list(a.decode('UTF-8') for a in tmp)


def _shape_key(name, value):
    """(type, shape) of a replicated / state / log value as it will be written: what must agree between the ranks."""
    if isinstance(value, (list, tuple)) and name in ('types', 'type_shapes'):
        return ('strings', len(value), max([len(str(v).encode('utf-8')) for v in value] or [0]))
    a = numpy.asarray(value)
    return (a.dtype.str, a.shape)


class _AppendPlan(object):
    """One frame on its way through `HOOMDTrajectory.append`: `_plan_frame` fills it, `_agree` settles it over the
    ranks, `_write_frame` carries it out."""
    __slots__ = ('entries', 'dev', 'host_pp', 'replicated', 'at_count', 'n_local', 'part0', 'ticket', 'compared',
                 'frame0_equal', 'part_dist', 'n_global', 'declared')

    def __init__(self):
        self.entries = []       # [path, name, write?] per schema name, in the reference's chunk order
        self.dev = []           # GPU-resident per-particle attributes: (position in entries, chunk name, DeviceField)
        self.host_pp = []       # several ranks: per-particle HOST arrays that would be written: (position, chunk, array)
        self.replicated = []    # (chunk name, shape key) of the replicated values that are set on this rank
        self.at_count = None    # position of particles/N
        self.n_local = 0
        self.part0 = None       # the partition this rank's rows of frame 0 belong to (None: no such comparisons now)
        self.ticket = None      # staging ticket of the device arrays (None: they leave in fused launches)
        self.compared = []      # positions in `dev` that were compared with this rank's rows of frame 0 on the GPU
        self.frame0_equal = []  # positions in `entries` elided because they equal THIS rank's rows of frame 0
        self.part_dist = None
        self.n_global = 0
        self.declared = False


class HOOMDTrajectory(object):
    """Read and write hoomd pgsd files (hoomd.py:515-940).

    Args:
        file (`pgsd.fl.PGSDFile` or `pgsd.pypgsd.PGSDFile`): file to access.

    Attributes:
        device_elision: `append` applies the elision rule of hoomd.py:654-694 to GPU-resident per-particle arrays ON
            THE GPU.  True (default; ``'exact'`` is the same): every array that is set is compared in every frame --
            with this rank's rows of frame 0 where frame 0 holds the chunk, with the default value where it does
            not -- and the file is the one host arrays of the same values give, for every input (NaNs, signed zeros,
            arrays that return to frame 0's values, default-valued arrays); the price is one frame's worth of HBM for
            the rows of frame 0 and one comparison launch per frame.  False: GPU-resident arrays are always written.
            (Round 3's ``'once'`` shortcut -- stop comparing an array once it differed -- was removed in round 5: it
            wrote arrays that return to frame 0's values where the host path elides them.)

    Per-particle attributes of a `Frame` may be numpy arrays, torch GPU tensors or `pgsd.fl.DeviceField` views of
    GPU memory (a column range of a ``Scalar4`` array, a converted or bit-cast element type); `append` writes the
    GPU-resident ones through the fused pack kernel, `read_frame_device` restores a partition into GPU arrays.
    """

    def __init__(self, file):
        if file.mode == 'ab':
            raise ValueError('Append mode not yet supported')
        self._file = file
        self._initial_frame = None
        self._elision_ref = None       # what append compares against (frame 0; several ranks: its replicated part)
        self._elision_lazy = False     # one rank: per-particle arrays of frame 0 are read when first compared
        self._frame0_chunks = None
        #: compare GPU-resident per-particle arrays with frame 0 on the GPU and elide the equal ones, as hoomd.py:654-694
        #: does for host arrays (`append`); False: GPU-resident arrays are always written
        self.device_elision = True
        self._dev_ref = {}             # chunk -> GPU tensor: this rank's rows of frame 0 as the chunk stores them
        self._dev_ref_part = None      # the partition (every rank's row count) those rows belong to
        self._default_ref = {}         # (chunk, device) -> GPU tensor: rows of the default value as the chunk stores them
        self._dev_off = False          # the partition changed: frame 0's rows are other particles' from now on
        self._host_ref = {}            # several ranks: chunk -> this rank's rows of frame 0 (host arrays are compared too)
        self._prefix_names = {}        # reader: prefix -> (nnames when asked, matching chunk names)
        self._frame0_small_cache = {}  # device reader: small replicated chunks of frame 0, read once
        self._frame0_dev_part = None   # read_frame_device: the partition whose rows of frame 0 are kept in HBM ...
        self._frame0_dev_cache = {}    # ... chunk -> GPU tensor
        logger.info('opening HOOMDTrajectory: ' + str(self.file))
        if self.file.schema != 'hoomd':
            raise RuntimeError('PGSD file is not a hoomd schema file: ' + str(self.file))
        version = self.file.schema_version
        if not (version < (2, 0) and version >= (1, 0)):
            raise RuntimeError('Incompatible hoomd schema version ' + str(version) + ' in: ' + str(self.file))
        logger.info('found ' + str(len(self)) + ' frames')

    @property
    def file(self):
        """The file handle."""
        return self._file

    def __len__(self):
        """The number of frames in the trajectory."""
        return self.file.nframes

    # ------------------------------------------------------------------ writing
    def _comm(self):
        # the communicator the FILE was opened on (the process default unless `fl.open(..., comm=)` chose another)
        f = self.file
        if hasattr(f, 'nprocs'):
            return f.rank, f.nprocs
        return 0, 1                     # pgsd.pypgsd.PGSDFile: the pure-Python reader, one rank

    def append(self, frame, wait=True):
        """Append a frame (collective over the ranks of the file's communicator).

        ``wait=False`` seals the frame asynchronously (`pgsd.fl.PGSDFile.end_frame`): call
        ``trajectory.file.wait_packed()`` before changing GPU-resident arrays of the frame and
        ``trajectory.file.frame_sync()`` before relying on the file.

        The calls this makes are the ones the reference sketches (hoomd.py:569-642), pinned byte for
        byte against the oracle by ``tests/test_hoomd_append_oracle.py``:

        * order: ``configuration/{step, dimensions, box}``, then ``particles/*`` and ``constraints/*``
          in the order of their ``_default_value`` tables (hoomd.py:60-63, 167-184), then ``state/*``,
          then ``log/*``, then ``end_frame``;
        * ``box``, ``N`` (uint32, ``part_dist.sum()``), ``step`` (uint64), ``dimensions`` (uint8),
          ``types`` and ``type_shapes`` (int8 ``n x wid``, NUL padded, JSON for the shapes) are
          replicated small chunks: ``write_all=False, offset=None`` (hoomd.py:604-630);
        * per-particle arrays: ``write_all=True, offset=part_dist`` (hoomd.py:597-600);
        * ``state/*`` and ``log/*``: ``write_chunk(name, data)`` with default arguments (hoomd.py:634-640);
        * fields that are ``None`` are not written; fields that equal the initial frame, or the default value where
          frame 0 has no such chunk, are elided as hoomd.py:654-694 describes -- host arrays and GPU-resident arrays
          alike, by the same rule (``numpy.array_equal``'s equality: a NaN equals nothing, +0.0 equals -0.0).

        Three steps (`_plan_frame`, `_agree`, `_write_frame`): every rank decides what it would write, ONE allgather
        carries the ranks' row counts and votes, the chunks are written in the reference's order.

        Where the sketch cannot be followed literally:

        * ``constraints/*`` are replicated small chunks and ``constraints/N`` is the constraint count
          (the sketch would write the PARTICLE count as ``constraints/N`` and partition ``value`` /
          ``group`` by the particle distribution, hoomd.py:597-611: files its own reader rejects);
        * the write/skip decision of every chunk is agreed over the ranks (written if any rank needs
          it; a rank without a value contributes the default for its rows), because a chunk write is
          collective; ``particles/N`` is compared as the global count;
        * with several ranks a per-particle array is compared with THIS rank's rows of frame 0 (against the whole of
          frame 0, as the sketch compares, it could never be equal), while the partition is the one those rows were
          written with; after a change of the partition every per-particle array that is set is written;
        * GPU-resident per-particle arrays are compared ON THE GPU (`device_elision`): packed by one launch, their
          packed rows compared with this rank's rows of frame 0 (or with rows of the default value) in device memory;
        * replicated chunks, ``state/*`` and ``log/*`` must have the same shape on every rank (checked in the vote);
        * upstream HOOMD attributes (charge, diameter, moment_inertia, orientation, angmom) follow the
          SPH set in that order when they are set.
        """
        if logger.isEnabledFor(logging.DEBUG):
            logger.debug('Appending frame to hoomd trajectory: ' + str(self.file))
        frame.validate()
        rank, size = self._comm()
        self._elision_reference(frame, size)
        # From here on the frame costs ONE collective however many chunks of whatever kind it has: the allgather of
        # `_agree` (every rank's row count + its write/skip votes).  With the counts in hand the partition is DECLARED
        # to the library (pgsd_set_partition), which then places every chunk without an exchange of its own:
        # per-particle chunks by the declared rows (offset='auto'), everything else -- replicated small chunks,
        # state/* and log/* -- has the same size on every rank.  The file is byte-identical to the one the
        # exchanges would produce.  (One rank: nothing to exchange, the batched queue keeps the call pattern.)
        if size == 1 and getattr(self.file, 'frame_exchange', None) is False:
            self.file.frame_exchange = True
        plan = self._plan_frame(frame, rank, size)
        self._agree(plan, frame, rank, size)
        self._write_frame(plan, frame, rank, size, wait)

    # -- step 0 (once per trajectory): what the elision rule compares with
    def _elision_reference(self, frame, size):
        """The initial frame is the reference for elision (hoomd.py:654-694).  With several ranks only its REPLICATED
        part is read: a per-particle array of frame 0 holds all ranks' rows and can never equal this rank's share
        (round 2 had every rank read the whole global frame here -- 2.24 GB each at 8 x 10 M particles -- to find
        that out).  One rank: a per-particle array of frame 0 is read when (and if) a host array is to be compared with
        it -- reading all of frame 0 here cost the second append of a 10 M-particle trajectory 250 ms, for arrays that
        live on the GPU and are compared there never to be looked at.

        ... and so is the set of chunks frame 0 holds (hoomd.py:689-691).  Looked up ONCE, by every rank, for every
        name in the same order -- never from inside a comparison only some ranks make: a lookup flushes whatever is
        pending, which is collective (a rank whose velocities are all zero would ask alone)."""
        if len(self) == 0:
            return
        if self._elision_ref is None:
            if size == 1 and self._initial_frame is not None:
                self._elision_ref = self._initial_frame
            else:
                self._elision_ref = self._read_frame0_replicated()
                self._elision_lazy = size == 1
        if self._frame0_chunks is None:
            self._frame0_chunks = set()
            for path, names in _schema_names(frame):
                for name in names:
                    if self.file.chunk_exists(frame=0, name=path + '/' + name, write_all=False):
                        self._frame0_chunks.add(path + '/' + name)

    # -- step 1: this rank's decisions
    def _plan_frame(self, frame, rank, size):
        """What this rank would write: one entry per schema name, in the reference's order."""
        plan = _AppendPlan()
        entries = plan.entries
        dev, host_pp = plan.dev, plan.host_pp
        for path, names in _schema_names(frame):
            values = getattr(frame, path).__dict__
            particles = path == 'particles'
            for name in names:
                if particles and name == 'N':
                    # None = "as in frame 0": no count chunk; decided in `_agree` from the global count otherwise
                    plan.at_count = len(entries)
                    entries.append([path, name, frame.particles.N is not None])
                    continue
                value = values.get(name)
                if value is None and name == 'box':
                    value = values.get('_box')              # (the one attribute kept behind a property)
                if value is None:
                    entries.append([path, name, False])     # most of the schema, most of the time: not set
                    continue
                per_particle = particles and name in _PARTICLE_FIELDS
                if per_particle and _is_device(value):
                    dt = _PARTICLE_FIELDS[name][0]
                    field = value if isinstance(value, fl.DeviceField) else fl.DeviceField.from_device_array(value, out_dtype=dt)
                    dev.append((len(entries), path + '/' + name, field))
                    entries.append([path, name, True])
                    continue
                write = self._should_write(path, name, frame, None)
                if per_particle:
                    if write and size > 1:
                        host_pp.append((len(entries), path + '/' + name, value))
                else:
                    plan.replicated.append((path + '/' + name, _shape_key(name, value)))
                entries.append([path, name, write])
        plan.n_local = int(frame.particles.N) if frame.particles.N is not None else 0
        plan.part0 = self._frame0_partition(frame, dev or host_pp, rank, size, plan.n_local)
        self._host_row_votes(plan, rank)
        self._device_votes(plan, rank)
        return plan

    # -- step 2: the frame's ONE collective
    def _agree(self, plan, frame, rank, size):
        """One allgather carries every rank's particle count (-> part_dist, the MPI_Allgather of
        benchmark-write.cc:41), a digest of the shapes of its replicated / state / log chunks, and two bits per plan
        entry: "write" and "elided only because it equals THIS rank's rows of frame 0".  Everything decided from here
        on rests on replicated data, so every rank decides alike."""
        entries = plan.entries
        n_local = plan.n_local
        if frame.part_dist is not None:
            part_dist = numpy.asarray(frame.part_dist, dtype=numpy.uint64)
            if part_dist.shape[0] != size:
                raise ValueError("part_dist must have one entry per rank")
        else:
            part_dist = numpy.array([n_local], dtype=numpy.uint64)
        rows_equal = numpy.zeros(len(entries), dtype=bool)      # any rank: elided against its rows of frame 0
        for at in plan.frame0_equal:
            rows_equal[at] = True
        if size > 1:
            mine = numpy.zeros(16 + len(entries), dtype=numpy.uint8)
            mine[:8] = numpy.array([n_local], dtype=numpy.uint64).view(numpy.uint8)
            digest = hashlib.blake2b(repr(plan.replicated + [('state/' + k, _shape_key(k, v)) for k, v in frame.state.items()]
                                          + [('log/' + k, _shape_key(k, v)) for k, v in frame.log.items()]).encode(),
                                     digest_size=8).digest()
            mine[8:16] = numpy.frombuffer(digest, dtype=numpy.uint8)
            mine[16:] = [(1 if e[2] else 0) | (2 if rows_equal[at] else 0) for at, e in enumerate(entries)]
            allb = self.file.allgather(mine)
            if frame.part_dist is None:
                part_dist = numpy.ascontiguousarray(allb[:, :8]).view(numpy.uint64).reshape(size)
            if (allb[:, 8:16] != allb[0, 8:16]).any():
                # placed without an exchange (declared partition), such chunks would put different offsets into each
                # rank's replicated index: every rank sees the same vector, every rank stops here
                raise ValueError("replicated chunks (configuration/*, types, constraints/*, state/*, log/*) must be set "
                                 "on every rank with the same shape and type: the ranks differ")
            bits = allb[:, 16:]
            for e, w in zip(entries, (bits & 1).max(axis=0)):
                e[2] = bool(w)
            rows_equal = (bits & 2).max(axis=0).astype(bool)
        plan.part_dist = part_dist
        plan.n_global = int(part_dist.sum())
        if plan.at_count is not None and entries[plan.at_count][2]:
            entries[plan.at_count][2] = self._should_write('particles', 'N', frame, plan.n_global)
        self._partition_bookkeeping(plan, rows_equal, size)
        plan.declared = size > 1 and hasattr(self.file, 'set_partition')
        if plan.declared and int(part_dist[rank]) != n_local:
            raise ValueError("part_dist[%d] = %d but this rank holds %d particles" % (rank, int(part_dist[rank]), n_local))

    def _partition_bookkeeping(self, plan, rows_equal, size):
        """Comparisons with this rank's rows of frame 0 hold while the partition is the one those rows were written
        with.  Decided from the gathered partition and the gathered "equal to my rows of frame 0" bits alone --
        replicated data (the override used to hang on a rank-local condition, so that one rank placed a
        chunk the others did not)."""
        part = tuple(int(x) for x in plan.part_dist)
        n0 = self._elision_ref.particles.N if self._elision_ref is not None else None
        fits = len(self) == 0 or (n0 is not None and int(n0) == sum(part))     # frame 0 has that many particles
        if size == 1:
            # one rank: "my rows of frame 0" are the whole of frame 0 -- comparable whenever the counts agree, in
            # whatever frame (`_frame0_partition`), exactly as host arrays are compared (`_should_write`)
            if self._dev_ref_part is None and fits:
                self._dev_ref_part = part
        elif not self._dev_off:
            if self._dev_ref_part is None:
                # frame 0 being written, or the first frame appended to an existing file: the rows of frame 0 kept /
                # read from now on are those of THIS partition
                if fits:
                    self._dev_ref_part = part
                else:
                    self._dev_off = True
            elif part != self._dev_ref_part:
                # particles moved between the ranks (or their number changed): whatever was compared was compared
                # with other particles' rows.  Every per-particle array that some rank elided on those grounds is
                # written, and every array that is set from now on
                self._dev_off = True
                for at, e in enumerate(plan.entries):
                    if rows_equal[at]:
                        e[2] = True
        if self._dev_off:
            self._dev_ref.clear()
            self._host_ref.clear()
            return

    # -- step 3: the chunks, in the reference's order
    def _write_frame(self, plan, frame, rank, size, wait):
        debug = logger.isEnabledFor(logging.DEBUG)
        part_dist, n_local, n_global = plan.part_dist, plan.n_local, plan.n_global
        if plan.declared:
            self.file.set_partition(part_dist)
        particle_offset = 'auto' if plan.declared else part_dist
        ticket = plan.ticket
        if ticket is not None and len(self) == 0 and self._dev_ref_part is not None:
            # frame 0: the packed rows of what is written stay in HBM for the comparisons to come (a device-to-device
            # copy behind the pack)
            sizes = [int(f.N) * int(f.M) * f.out_dtype.itemsize if plan.entries[at][2] else None for at, _, f in plan.dev]
            for (_, chunk, _), ref in zip(plan.dev, self.file.copy_staged(ticket, 0, sizes)):
                if ref is not None:
                    self._dev_ref[chunk] = ref
        device_fields = []      # not staged: consecutive GPU-resident fields leave in one fused launch
        staged_run = []         # staged (one launch for the whole frame): consecutive chunk numbers of the ticket
        dev_at = dict((at, (k, field)) for k, (at, _, field) in enumerate(plan.dev)) if plan.dev else {}
        for at, (path, name, write) in enumerate(plan.entries):
            if not write:
                continue
            container = getattr(frame, path)
            data = getattr(container, name)
            chunk = path + '/' + name
            if debug:
                logger.debug('writing data chunk: ' + chunk)
            if path == 'particles' and name in _PARTICLE_FIELDS:
                dt, M, default, _ = _PARTICLE_FIELDS[name]
                if at in dev_at:
                    k, field = dev_at[at]
                    if ticket is None:
                        device_fields.append((chunk, field))
                    else:
                        if staged_run and staged_run[-1] + 1 != k:
                            self._flush_staged(ticket, staged_run, particle_offset, rank)
                        staged_run.append(k)
                    continue
                if data is None:
                    # another rank needs the chunk: contribute this rank's rows of the default
                    data = numpy.empty([n_local] + ([M] if M > 1 else []), dtype=dt)
                    data[...] = default
                self._flush_device_fields(device_fields, particle_offset, rank)
                self._flush_staged(ticket, staged_run, particle_offset, rank)
                self.file.write_chunk(chunk, data, particle_offset, rank, True)
                continue
            self._flush_device_fields(device_fields, particle_offset, rank)
            self._flush_staged(ticket, staged_run, particle_offset, rank)
            # replicated small chunks (hoomd.py:604-630)
            if name == 'N':
                count = n_global if path == 'particles' else int(container.N)
                data = numpy.array([count], dtype=numpy.uint32)
            elif name == 'step':
                data = numpy.array([data], dtype=numpy.uint64)
            elif name == 'dimensions':
                data = numpy.array([data], dtype=numpy.uint8)
            elif name in ('types', 'type_shapes'):
                if name == 'type_shapes':
                    data = [json.dumps(shape_dict) for shape_dict in data]
                data = _encode_strings(data)
            self.file.write_chunk(chunk, data, None, rank, False)
        self._flush_device_fields(device_fields, particle_offset, rank)
        self._flush_staged(ticket, staged_run, particle_offset, rank)

        # state and logged quantities: the sketch calls ``write_chunk(name, data)`` with the binding's
        # default arguments (hoomd.py:634-640; the state loop is commented out twice, upstream GSD
        # has it) -- write_all=True, no offset: every rank writes its (replicated) value at the same
        # place and the file advances by the ranks' sizes summed (pgsd.c:2240-2246)
        for state, data in frame.state.items():
            self.file.write_chunk('state/' + state, numpy.ascontiguousarray(data))
        for log, data in frame.log.items():
            self.file.write_chunk('log/' + log, data)

        self.file.end_frame(wait=wait)
        if plan.declared:
            self.file.set_partition(None)       # the declaration was this frame's

    def _flush_staged(self, ticket, run, part_dist, rank):
        if run:
            self.file.write_staged(ticket, run[0], len(run), offset=part_dist, rank=rank)
            del run[:]

    def _frame0_partition(self, frame, wanted, rank, size, n_local):
        """The partition (every rank's row count) for which this rank's rows of frame 0 are, or can be, at hand -- or
        None when per-particle arrays cannot be compared with frame 0's rows in this frame: nothing to compare, frame 0
        itself, the comparisons ended (`_dev_off`), a partition that differs from the one the rows were taken for,
        or one that is not known before the frame's exchange (no `Frame.part_dist`, several ranks, first frame
        appended to an existing file: the comparisons then start with the next frame)."""
        if not wanted or self._dev_off or len(self) == 0:
            return None
        given = None
        if frame.part_dist is not None:
            given = tuple(int(x) for x in numpy.asarray(frame.part_dist).reshape(-1))
        elif size == 1:
            given = (n_local,)
        part = self._dev_ref_part
        if part is None:
            n0 = self._elision_ref.particles.N if self._elision_ref is not None else None
            if given is None or n0 is None or int(n0) != sum(given):
                return None
            part = given
        elif given is not None and given != part:
            return None                     # (`_partition_bookkeeping` sees the change and ends the comparisons)
        if len(part) != size or part[rank] != n_local:
            return None
        return part

    def _read_frame0_rows(self, chunk, row0, n, device):
        """This rank's rows ``[row0, row0 + n)`` of a per-particle chunk of frame 0, as a numpy array or a GPU tensor.
        A LOCAL read (`PGSDFile.local_reads`, lookup included): these are rows this rank wrote itself in this session,
        or rows of a file that was complete when it was opened -- and which arrays a rank compares need not be the
        same on every rank, so the read must not be a collective."""
        f = self.file
        before = f.local_reads
        f.local_reads = True
        try:
            if device:
                return f.read_chunk_device(0, chunk, N=n, offset=row0)
            return f.read_rows(0, chunk, row0, n)
        finally:
            f.local_reads = before

    def _host_row_votes(self, plan, rank):
        """Several ranks: a per-particle HOST array is compared with THIS RANK'S rows of frame 0 (read from the file
        when first needed, ``numpy.array_equal`` as on one rank); equal rows vote "skip".  (Compared with the whole of
        frame 0 -- every rank's rows -- as the sketch has it, hoomd.py:673-687, an array could never be equal.)"""
        if not plan.host_pp or plan.part0 is None:
            return
        frame0 = self._frame0_chunks or ()
        row0 = sum(plan.part0[:rank])
        for at, chunk, data in plan.host_pp:
            if chunk not in frame0:
                continue
            ref = self._host_ref.get(chunk)
            if ref is None:
                ref = self._read_frame0_rows(chunk, row0, plan.n_local, False)
                self._host_ref[chunk] = ref
            if _equal(ref, data):
                logger.debug('skipping data chunk, this rank\'s rows match frame 0: ' + chunk)
                plan.entries[at][2] = False
                plan.frame0_equal.append(at)

    def _default_rows(self, chunk, field, device):
        """Rows of the schema's default value for ``chunk`` as the chunk stores them, in device memory: what "equals
        the default" is tested against (hoomd.py:692-693).  4096 rows stand for any number (the comparison lets a
        short reference repeat); fewer rows than that get exactly as many."""
        key = (chunk, device)
        ref = self._default_ref.get(key)
        if ref is None:
            row = numpy.empty((1, int(field.M)), dtype=field.out_dtype)
            row[...] = _PARTICLE_FIELDS[chunk.split('/', 1)[1]][2]
            # 4096 rows of the default value in the library's own device memory: ONE row repeated by the allocation
            ref = fl.DeviceBuffer((4096 * row.nbytes,), numpy.uint8, device, pattern=row)
            self._default_ref[key] = ref
        want = int(field.N) * int(field.M) * field.out_dtype.itemsize
        return ref if want >= ref.nbytes else ref.view(shape=(want,))

    def _device_votes(self, plan, rank):
        """The elision rule of hoomd.py:654-694 for GPU-resident per-particle arrays, decided on the GPU exactly as
        `_should_write` decides it for host arrays: a chunk frame 0 holds is compared with this rank's rows of frame 0
        (equal: skip), a chunk frame 0 does not hold -- or frame 0 itself -- with rows of the default value (equal:
        skip).  Equality is ``numpy.array_equal``'s (`PGSDFile.compare_staged`): the file is the one host arrays of
        the same values give.

        All of the frame's GPU-resident arrays are packed by ONE launch into staging (`stage_chunks`) and compared by
        one more (`compare_staged`: one stream wait).  Frame 0's rows come from the staging of frame 0 itself when
        this trajectory wrote it (`copy_staged` in `_write_frame`: a device-to-device copy), from the file otherwise
        (`read_chunk_device`, once per array).  ``device_elision = False``: no comparisons, every array that is set
        is written.  Everything the comparison keeps in HBM is the library's own memory (`pgsd.fl.DeviceBuffer`) on
        the GPU the file's pipeline runs on: no tensor library is involved, whatever kind of array the sources are."""
        f = self.file
        dev = plan.dev
        if not dev or not self.device_elision or not hasattr(f, 'compare_staged'):
            return
        frame0 = (self._frame0_chunks or ()) if len(self) > 0 else ()
        part0 = plan.part0
        refs = [None] * len(dev)
        kinds = [None] * len(dev)                   # 'rows': against frame 0's rows; 'default': against the default
        device = None
        for k, (_, chunk, field) in enumerate(dev):
            if chunk in frame0:
                if part0 is not None and not self._dev_off:
                    kinds[k] = 'rows'
            else:
                kinds[k] = 'default'
        if not any(kinds):
            return
        ticket = f.stage_chunks([(chunk, field) for _, chunk, field in dev])
        device = ticket[3]              # the GPU the file's pipeline runs on (the handle's own answer)
        row0 = sum(part0[:rank]) if part0 is not None else 0
        for k, (_, chunk, field) in enumerate(dev):
            if kinds[k] == 'default':
                refs[k] = self._default_rows(chunk, field, device)
            elif kinds[k] == 'rows':
                ref = self._dev_ref.get(chunk)
                if ref is None:
                    ref = self._read_frame0_rows(chunk, row0, plan.n_local, True)
                    self._dev_ref[chunk] = ref
                if ref.numel() * ref.element_size() == int(field.N) * int(field.M) * field.out_dtype.itemsize:
                    refs[k] = ref
        equal = f.compare_staged(ticket, 0, refs)
        for k, (at, chunk, _) in enumerate(dev):
            if refs[k] is None:
                continue
            if kinds[k] == 'rows':
                plan.compared.append(k)
            if equal[k]:
                plan.entries[at][2] = False
                if kinds[k] == 'rows':
                    plan.frame0_equal.append(at)
        plan.ticket = ticket

    def _flush_device_fields(self, device_fields, part_dist, rank):
        if device_fields:
            self.file.write_chunks(list(device_fields), offset=part_dist, rank=rank)
            del device_fields[:]

    def _should_write(self, path, name, frame, n_global):
        """False if the value is None, matches the initial frame, or matches the default and
        frame 0 has no such chunk (hoomd.py:654-694)."""
        container = getattr(frame, path)
        data = getattr(container, name, None)
        per_particle = path == 'particles' and name in _PARTICLE_FIELDS
        if name == 'N' and path == 'particles':
            data = n_global
        if data is None:
            return False
        if _is_device(data):
            return True
        if self._elision_ref is not None:
            initial_container = getattr(self._elision_ref, path)
            initial_data = getattr(initial_container, name, None)
            if (initial_data is None and self._elision_lazy and per_particle
                    and (path + '/' + name) in (self._frame0_chunks or ())):
                initial_data = self.file.read_chunk(frame=0, name=path + '/' + name, offset=numpy.uint32(0), r_all=False)
                initial_container.__dict__[name] = initial_data
            if initial_data is not None and _equal(initial_data, data):
                logger.debug('skipping data chunk, matches frame 0: ' + path + '/' + name)
                return False
        # a value that matches the default is elided -- unless frame 0 holds the chunk (a reader would take frame 0's
        # value for the default).  Most chunks that are written at all are in frame 0: the lookup comes first, the
        # comparison with the default (the dearer of the two) only when it can decide something
        if (path + '/' + name) in (self._frame0_chunks or ()):
            return True
        default = _PARTICLE_FIELDS[name][2] if per_particle else container._default_value.get(name)
        if name in ('types', 'type_shapes'):
            matches_default_value = data == default
        else:
            matches_default_value = _equiv(data, default)
        if matches_default_value:
            logger.debug('skipping data chunk, default value: ' + path + '/' + name)
            return False
        return True

    def _read_frame0_replicated(self):
        """Frame 0's replicated values -- configuration, particle count, types, type shapes, constraints -- for the
        elision test of `append` on several ranks; per-particle attributes stay None (never compared)."""
        f = self.file
        snap = Frame()
        self._read_scalar_any(0, 'configuration/step', snap.configuration, 'step')
        self._read_scalar_any(0, 'configuration/dimensions', snap.configuration, 'dimensions')
        snap.configuration.box = f.read_chunk(0, 'configuration/box') if f.chunk_exists(0, 'configuration/box') \
            else snap.configuration._default_value['box']
        for path in ('particles', 'constraints'):
            container = getattr(snap, path)
            container.N = int(f.read_chunk(0, path + '/N')[0]) if f.chunk_exists(0, path + '/N') else 0
        for name in ('types', 'type_shapes'):
            if f.chunk_exists(0, 'particles/' + name):
                tmp = _decode_strings(f.read_chunk(0, 'particles/' + name))
                if name == 'types':
                    snap.particles.types = tmp
                else:
                    snap.particles.type_shapes = list(json.loads(a) for a in tmp)
            else:
                setattr(snap.particles, name, snap.particles._default_value[name])
        for name in ('value', 'group'):
            if f.chunk_exists(0, 'constraints/' + name):
                setattr(snap.constraints, name, f.read_chunk(0, 'constraints/' + name))
        return snap

    def extend(self, iterable):
        """Append each item of the iterable to the file."""
        for item in iterable:
            self.append(item)

    def close(self):
        """Close the file."""
        self.file.close()
        del self._initial_frame
        self._elision_ref = None
        self._dev_ref = {}
        self._host_ref = {}
        self._frame0_dev_cache = {}

    def flush(self):
        """Flush all buffered frames to the file."""
        self._file.flush()

    # ------------------------------------------------------------------ reading
    def read_frame(self, idx):
        """Read the frame at the given index (deprecated alias of ``trajectory[idx]``)."""
        warnings.warn("Deprecated, trajectory[idx]", DeprecationWarning)
        return self._read_frame(idx)

    def _names_with_prefix(self, prefix):
        """`find_matching_chunk_names(prefix)`, asked again only when the file's name list has grown (names are never
        removed): the reader looks `log/` and `state/` up for every frame."""
        f = self.file
        n = getattr(f, 'nnames', None)
        if n is None:                       # pgsd.pypgsd.PGSDFile: the pure-Python reader keeps no count
            return f.find_matching_chunk_names(prefix, False)
        cached = self._prefix_names.get(prefix)
        if cached is None or cached[0] != n:
            cached = (n, f.find_matching_chunk_names(prefix, False))
            self._prefix_names[prefix] = cached
        return cached[1]

    def _read_scalar(self, idx, chunk, container, attr, fallback_path):
        if self.file.chunk_exists(frame=idx, name=chunk, write_all=False):
            arr = self.file.read_chunk(frame=idx, name=chunk, offset=numpy.uint32(0), r_all=False)
            setattr(container, attr, arr[0])
        elif self._initial_frame is not None:
            setattr(container, attr, getattr(getattr(self._initial_frame, fallback_path), attr))
        else:
            setattr(container, attr, container._default_value[attr])

    def _read_frame(self, idx):
        """Read one frame; chunks missing in the frame come from frame 0 (when N matches) or
        from the default values, returned read-only (hoomd.py:724-902)."""
        if idx >= len(self):
            raise IndexError
        if logger.isEnabledFor(logging.DEBUG):
            logger.debug('reading frame ' + str(idx) + ' from: ' + str(self.file))
        if self._initial_frame is None and idx != 0:
            self._read_frame(0)

        snap = Frame()
        self._read_scalar(idx, 'configuration/step', snap.configuration, 'step', 'configuration')
        self._read_scalar(idx, 'configuration/dimensions', snap.configuration, 'dimensions', 'configuration')
        if self.file.chunk_exists(frame=idx, name='configuration/box', write_all=False):
            snap.configuration.box = self.file.read_chunk(frame=idx, name='configuration/box',
                                                          offset=numpy.uint32(0), r_all=False)
        elif self._initial_frame is not None:
            snap.configuration.box = self._initial_frame.configuration.box
        else:
            snap.configuration.box = snap.configuration._default_value['box']

        for path in ('particles', 'constraints'):
            container = getattr(snap, path)
            initial = getattr(self._initial_frame, path) if self._initial_frame is not None else None

            container.N = 0
            if self.file.chunk_exists(frame=idx, name=path + '/N', write_all=False):
                container.N = self.file.read_chunk(frame=idx, name=path + '/N', offset=numpy.uint32(0),
                                                   r_all=False)[0]
            elif initial is not None:
                container.N = initial.N

            if 'types' in container._default_value:
                if self.file.chunk_exists(frame=idx, name=path + '/types', write_all=False):
                    tmp = self.file.read_chunk(frame=idx, name=path + '/types', offset=numpy.uint32(0), r_all=False)
                    container.types = _decode_strings(tmp)
                elif initial is not None:
                    container.types = initial.types
                else:
                    container.types = container._default_value['types']

            if 'type_shapes' in container._default_value and path == 'particles':
                if self.file.chunk_exists(frame=idx, name=path + '/type_shapes', write_all=False):
                    tmp = self.file.read_chunk(frame=idx, name=path + '/type_shapes', offset=numpy.uint32(0),
                                               r_all=False)
                    container.type_shapes = list(json.loads(s) for s in _decode_strings(tmp))
                elif initial is not None:
                    container.type_shapes = initial.type_shapes
                else:
                    container.type_shapes = container._default_value['type_shapes']

            for name, default, chunk, is_optional in _reader_fields(path, container):
                if self.file.chunk_exists(frame=idx, name=chunk, write_all=False):
                    container.__dict__[name] = self.file.read_chunk(frame=idx, name=chunk, offset=numpy.uint32(0),
                                                                    r_all=False)
                    continue
                if is_optional and (initial is None or initial.__dict__.get(name) is None):
                    continue  # upstream-only attribute that this file never stored
                if initial is not None and initial.N == container.N and initial.__dict__.get(name) is not None:
                    container.__dict__[name] = initial.__dict__[name]
                else:
                    tmp = numpy.array([default])
                    s = list(tmp.shape)
                    s[0] = container.N
                    container.__dict__[name] = numpy.empty(shape=s, dtype=tmp.dtype)
                    container.__dict__[name][:] = tmp
                container.__dict__[name].flags.writeable = False

        for log in self._names_with_prefix('log/'):
            if self.file.chunk_exists(frame=idx, name=log, write_all=False):
                snap.log[log[4:]] = self.file.read_chunk(frame=idx, name=log, offset=numpy.uint32(0), r_all=False)
            elif self._initial_frame is not None and log[4:] in self._initial_frame.log:
                snap.log[log[4:]] = self._initial_frame.log[log[4:]]

        # state chunks belong to the frame they were written in (no fall-back, as upstream GSD reads them)
        for state in self._names_with_prefix('state/'):
            if self.file.chunk_exists(frame=idx, name=state, write_all=False):
                snap.state[state[6:]] = self.file.read_chunk(frame=idx, name=state, offset=numpy.uint32(0), r_all=False)

        if self._initial_frame is None and idx == 0:
            self._initial_frame = snap
        return snap

    def read_frame_device(self, idx, part=None, scalar4=False, defaults=True, domain=None, where=None, ghost=None,
                          cell_order=None):
        """Read frame ``idx`` with the per-particle arrays of THIS rank's partition in GPU memory.

        Restart path (BASELINE config 5): each rank reads rows ``[row0, row0 + n)`` of every
        per-particle chunk through :meth:`pgsd.fl.PGSDFile.read_chunk_device` (pread -> pinned
        slabs -> HBM -> HIP unpack); configuration, types and log stay small host values.  Chunks
        missing in the frame come from frame 0 or from the defaults, like :meth:`_read_frame`.

        Args:
            idx (int): frame index.
            part (tuple): ``(row0, n)``; default: the particles split evenly over the ranks of the
                installed communicator.
            scalar4 (bool): also assemble HOOMD-style arrays on the device:
                ``frame.particles.pos4 = (x, y, z, typeid bits)`` and ``vel4 = (vx, vy, vz, mass)``.
            defaults (bool): attributes the file holds neither in this frame nor in frame 0 are filled with their
                default rows as the host reader fills them (hoomd.py:872-881) -- views of one small device copy per
                read, a third of a 1 024-particle frame's 90 us; False leaves them ``None``.
            domain (`Domain`): instead of a row slab, the particles whose position lies in this cell of a spatial
                domain decomposition (`domain_grid`), selected on the GPU from the frame's effective position and box
                exactly as `domain_rows` defines it; every per-particle array is gathered through that row list, and
                ``frame.tag`` holds it (file rows: the particle tags of a file written in tag order; int32, typed like
                `pgsd.fl.select_rows`).  Not together with ``part``.
            where (dict): instead of a row slab, the particles of a group: the rows that satisfy every term of this
                predicate over the frame's per-particle chunks -- ``{'type': ['fluid']}``, ``{'density': (1000.0,
                None)}``, ``{('velocity', 2): (None, 0.0), 'typeid': [0, 2]}`` --, selected on the GPU exactly as
                `where_rows` defines it; with ``domain`` the rows that also lie in that cell (one selection).  The
                result is a domain read's: ``frame.tag`` holds the selected file rows, ``frame.where`` the predicate.
                Not together with ``part``.
            ghost: with ``domain``, the cell plus the ghost layer its neighbours reach, as `halo_rows` defines it: the
                layer's width as a real distance (HOOMD's ``r_ghost``) or three fractions of the box.  Every
                per-particle array holds the owned rows first, then the ghost rows (each ascending);
                ``particles.N`` is their total, ``frame.n_owned`` the number of owned rows, ``frame.tag`` the file rows
                and ``frame.ghost_shift`` an ``n_ghost x 3`` int32 device array: the box vectors to add to each ghost's
                position so that it lies next to the cell (`halo_rows` gives the formula; positions are returned as
                stored).  Needs ``domain``; not together with ``part`` or ``where`` -- a ghost layer around a particle
                group is not provided.
            cell_order: with ``domain`` and / or ``where`` (and with ``ghost``), a tuple ``(cx, cy, cz)``: the selected row
                list is sorted by the cell of a uniform grid over the box its particles lie in -- on the GPU, between the
                selection and the gather, exactly as `cell_order` defines it (`cell_grid_for` gives the counts for an
                interaction range) --, and ``frame.tag``, every per-particle array, ``pos4`` / ``vel4`` follow that
                order: the particles of one cell are neighbours in memory, in ascending file-row order.  ``frame.cell``
                holds the sorted cell ids (int32, device; `cell_ids`), ``frame.cell_grid`` the counts.  With ``ghost``
                the owned and the ghost run are sorted separately: ``frame.n_owned`` is unchanged, the ghost run's ids
                ascend on their own and ``frame.ghost_shift`` is permuted with its ghosts.  A position that is stored
                nowhere puts every row at the origin: the order is unchanged and all rows share one id.  The other
                chunks are gathered through rows that are no longer ascending.  Not together with ``part``, and not
                without a selection: ValueError.

        Returns:
            `Frame` whose ``particles.N`` is this rank's count, ``particles.N_global`` the total.  The per-particle
            arrays are torch GPU tensors where torch is importable, `pgsd.fl.DeviceBuffer` objects (the library's own
            device memory, ``__cuda_array_interface__``) otherwise -- on the GPU the file's pipeline runs on.
        """
        if idx < 0:
            idx += len(self)
        if idx >= len(self) or idx < 0:
            raise IndexError()
        if ghost is not None and (domain is None or part is not None or where is not None):
            raise ValueError("ghost needs domain and goes with neither part nor where")
        if cell_order is not None:
            if part is not None or (domain is None and where is None):
                raise ValueError("cell_order needs domain or where and does not go with part")
            cell_order = _order_cells(cell_order, 3)
        f = self.file
        snap = Frame()
        self._read_scalar_any(idx, 'configuration/step', snap.configuration, 'step')
        self._read_scalar_any(idx, 'configuration/dimensions', snap.configuration, 'dimensions')
        box_frame = self._frame_of(idx, 'configuration/box')
        if box_frame is None:
            snap.configuration.box = snap.configuration._default_value['box']
        elif box_frame == 0:
            snap.configuration.box = self._frame0_small('configuration/box').copy()
        else:
            snap.configuration.box = f.read_chunk(box_frame, 'configuration/box')

        fn = self._frame_of(idx, 'particles/N')
        n_global = 0 if fn is None else int((self._frame0_small('particles/N') if fn == 0 else f.read_chunk(fn, 'particles/N'))[0])
        ft = self._frame_of(idx, 'particles/types')
        if ft is not None:
            snap.particles.types = _decode_strings(self._frame0_small('particles/types') if ft == 0
                                                   else f.read_chunk(ft, 'particles/types'))
        else:
            snap.particles.types = snap.particles._default_value['types']

        if where is not None:
            if part is not None:
                raise ValueError("part and where are mutually exclusive")
            self._read_where_device(idx, snap, where, domain, scalar4, defaults, n_global, cell_order)
            self._read_logs_device(idx, snap)
            return snap
        if domain is not None:
            if part is not None:
                raise ValueError("part and domain are mutually exclusive")
            self._read_domain_device(idx, snap, domain, scalar4, defaults, n_global, ghost, cell_order)
            self._read_logs_device(idx, snap)
            return snap
        if part is None:
            rank, size = self._comm()
            base, rem = divmod(n_global, size)
            n = base + (1 if rank < rem else 0)
            row0 = rank * base + min(rank, rem)
        else:
            row0, n = int(part[0]), int(part[1])
        snap.particles.N = n
        snap.particles.N_global = n_global
        snap.part = (row0, n)

        if self._frame0_dev_part != (row0, n):
            self._frame0_dev_part, self._frame0_dev_cache = (row0, n), {}     # rows of ONE partition are kept
        cache, fresh = self._frame0_dev_cache, []

        def slab(fr, chunk, attr, **kw):
            if fr == 0 and idx != 0 and not kw:
                # an array the frame does not hold because it equals frame 0's (elided by `append`): this partition's
                # rows of frame 0 are read from the file ONCE and handed out as device-to-device copies from then on
                # (a trajectory whose static arrays are elided would otherwise re-read them for every frame)
                cached = cache.get(chunk)
                if cached is not None:
                    return cached.clone()
                fresh.append((attr, chunk))
            return f.read_chunk_device(fr, chunk, N=n, offset=row0, wait=False, **kw)

        # everything is issued, then ONE wait
        self._read_particles_device(idx, snap, n, n_global, defaults, slab,
                                    [tuple(_PARTICLE_FIELDS) + (tuple(_SCALAR4) if scalar4 else ())])
        for name, chunk in fresh:
            cache[chunk] = getattr(snap.particles, name).clone()
        self._read_logs_device(idx, snap)
        return snap

    def _read_particles_device(self, idx, snap, n, n_global, defaults, read, groups):
        """The per-particle arrays of a device read, for slab and domain reads alike: which frame each chunk comes from
        (`_effective_frame`), the default rows of what is stored nowhere, and HOOMD's Scalar4 arrays.

        ``read(frame, chunk, attr, **kw)`` issues the read of the caller's ``n`` rows of one chunk without waiting --
        into ``out=`` and its ``columns=`` where given, else into a new array, which it returns; ``attr`` is the
        attribute of ``snap.particles`` the rows are for.  ``groups`` lists the attributes to read in the order of
        their reads, `_SCALAR4`'s names for the assembled arrays, as tuples that each share one ``wait_read``: what
        is in flight between two waits is what the HBM staging must hold."""
        f = self.file
        particles = snap.particles
        device = f.pipeline_device()
        frames = dict(('particles/' + name, self._effective_frame(idx, 'particles/' + name, n_global))
                      for name in _PARTICLE_FIELDS)
        missing = [name for name, field in _PARTICLE_FIELDS.items()
                   if defaults and not field[3] and frames['particles/' + name] is None]
        for group in groups:
            issued = False
            for attr in group:
                if attr in _SCALAR4:
                    # HOOMD's Scalar4 arrays, every row stored WHOLE by the unpack launch: the columns a missing chunk
                    # would have fed come from the `fill` of the chunk that is there (type id 0 as bits, mass 1.0,
                    # position / velocity 0) -- no memset of the arrays, no 12-byte stores at a 16-byte stride
                    xyz, w, w_bitcast, w_default = _SCALAR4[attr]
                    f_xyz, f_w = frames[xyz], frames[w]
                    if f_xyz is None and f_w is None:
                        # neither chunk anywhere: rows of (0, 0, 0, default w)
                        arr = fl._device_rows((n, 4), numpy.float32, device, [0.0, 0.0, 0.0, w_default])
                    else:
                        arr = fl._device_empty((n, 4), numpy.float32, device)
                        issued = True
                    if f_xyz is not None:
                        read(f_xyz, xyz, attr, out=arr, columns=(0, 3), fill=w_default if f_w is None else None)
                    if f_w is not None:
                        read(f_w, w, attr, out=arr, columns=(3, 4), bitcast=w_bitcast,
                             fill=0.0 if f_xyz is None else None)
                    setattr(particles, attr, arr)
                elif frames['particles/' + attr] is not None:
                    setattr(particles, attr, read(frames['particles/' + attr], 'particles/' + attr, attr))
                    issued = True
                elif missing:
                    # like the host reader (hoomd.py:872-881) a default is ONE row broadcast over the particles: no
                    # N-row allocation, no copy; `.contiguous()` / `.clone()` gives an array of its own.  The reference
                    # marks its defaults read-only; torch has no such flag, so every read gets its OWN copy of the rows
                    # (one clone of a 40-word template per frame, not one host->device copy per field): a write
                    # through a view changes this frame's view only, never a later frame's default.  All of the
                    # frame's default views are made here, at the first, behind the reads issued so far
                    words = self._default_rows_template(device).clone()
                    views = fl._device_row_views(words, [self._default_rows_layout[name] for name in missing], n)
                    for name, view in zip(missing, views):
                        setattr(particles, name, view)
                    missing = None
            if issued:
                f.wait_read()

    # ------------------------------------------------------------------ tracks: a few particles through many frames
    def _track_args(self, rows, frames, fields):
        """(rows on the host as int64, frame indices, field names) of a tracks read, checked: every frame must hold
        row max(rows) -- IndexError naming the first that does not, before anything is read."""
        n = len(self)
        if frames is None:
            idxs = list(range(n))
        elif isinstance(frames, slice):
            idxs = list(range(*frames.indices(n)))
        else:
            idxs = [int(i) + n if int(i) < 0 else int(i) for i in frames]
        for idx in idxs:
            if not 0 <= idx < n:
                raise IndexError("frame %d of %d" % (idx, n))
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        for name in fields:
            if name not in _PARTICLE_FIELDS:
                raise ValueError("'%s' is not a per-particle attribute of ParticleData" % name)
        if isinstance(rows, numpy.ndarray) or not _is_device(rows):
            host = numpy.asarray(rows)
        else:
            host = fl._device_to_host(rows)
        if host.size and host.dtype.kind not in 'iu':
            raise ValueError("rows must be integers")
        host = host.reshape(-1).astype(numpy.int64)
        if host.size and (host.min() < 0 or host.max() >= 1 << 32):
            raise ValueError("rows must be file rows, 0 <= row < 2^32")
        f = self.file
        counts = []
        for idx in idxs:
            if f.chunk_exists(frame=idx, name='particles/N', write_all=False):
                n_idx = int(f.read_chunk(frame=idx, name='particles/N', offset=numpy.uint32(0), r_all=False)[0])
            elif f.chunk_exists(frame=0, name='particles/N', write_all=False):
                n_idx = int(self._frame0_small('particles/N')[0])
            else:
                n_idx = 0
            if host.size and n_idx <= int(host.max()):
                raise IndexError("frame %d holds %d particles: row %d lies outside it" % (idx, n_idx, int(host.max())))
            counts.append(n_idx)
        return host, idxs, fields, counts

    def read_tracks(self, rows, frames=None, fields=('position',)):
        """A few particles through many frames, on the host: ``read_tracks(rows, frames, fields)[f][i]`` is
        ``trajectory[frames[i]].particles.<f>[rows]`` -- a plain loop over the frames that reads each field's effective
        chunk on the host and picks the rows; it is the model of `read_tracks_device`.

        Args:
            rows: K file rows (the tags of a file written in tag order): a host array, a GPU tensor or anything with
                ``__cuda_array_interface__``; any order, repeats allowed.
            frames: frame indices, a slice, or ``None`` for every frame.
            fields: names of per-particle attributes of `ParticleData`.

        Returns:
            `Tracks`: ``step`` (uint64, F entries), ``rows`` and per field an ``F x K (x M)`` numpy array of the chunk's
            dtype (also ``tracks[name]``).  Elided chunks come from frame 0 or the defaults exactly as the reader
            decides frame by frame.  A frame with ``N <= max(rows)`` raises IndexError before anything is read.
        """
        host, idxs, fields, counts = self._track_args(rows, frames, fields)
        f = self.file
        out = Tracks(numpy.zeros(len(idxs), dtype=numpy.uint64), host, fields)
        for i, idx in enumerate(idxs):
            step = ConfigurationData()
            self._read_scalar_any(idx, 'configuration/step', step, 'step')
            out.step[i] = step.step
            for name in fields:
                picked = self._read_particle_rows(idx, name, counts[i], host)
                if out[name] is None:
                    setattr(out, name, numpy.empty((len(idxs),) + picked.shape, dtype=picked.dtype))
                out[name][i] = picked
        for name in fields:
            if out[name] is None:       # no frames
                dt, M = _PARTICLE_FIELDS[name][:2]
                setattr(out, name, numpy.empty((0, host.size, M) if M > 1 else (0, host.size), dtype=dt))
        return out

    def _read_particle_rows(self, idx, name, n_global, rows):
        """``trajectory[idx].particles.<name>[rows]`` without reading the rest of the frame: the effective chunk's rows,
        or rows of the default value."""
        chunk = 'particles/' + name
        fr = self._effective_frame(idx, chunk, n_global)
        if fr is not None:
            return self.file.read_chunk(fr, chunk)[rows]
        if name not in ParticleData._default_value and not self.file.chunk_exists(0, chunk):
            raise ValueError("particles/%s is stored neither in frame %d nor in frame 0" % (name, idx))
        return numpy.repeat(numpy.array([_PARTICLE_FIELDS[name][2]]), len(rows), axis=0)

    def read_tracks_device(self, rows, frames=None, fields=('position',)):
        """`read_tracks` into GPU memory, reading only the file blocks the rows touch.

        One row plan (`pgsd.fl.PGSDFile.plan_rows`) per distinct particle count among the frames serves every chunk of
        every such frame; each frame's gather lands straight in its ``[i]`` slice of the result, and the reads of one
        frame share one ``wait_read`` (the HBM staging holds one frame's touched blocks).  Arguments as `read_tracks`.

        Returns:
            `Tracks` whose per-field ``F x K (x M)`` arrays (schema dtype) and ``rows`` (int32) live in GPU memory:
            torch tensors where torch is importable, `pgsd.fl.DeviceBuffer` objects otherwise; ``step`` stays a host
            array.
        """
        f = self.file
        host, idxs, fields, counts = self._track_args(rows, frames, fields)
        F, K = len(idxs), int(host.size)
        device = f.pipeline_device()
        rows_dev = fl._device_from_host(host.astype(numpy.uint32).view(numpy.int32), device)
        out = Tracks(numpy.zeros(F, dtype=numpy.uint64), rows_dev, fields)
        # which frame every (frame, field) reads, settled first: a field that some frame reads the default of is
        # allocated filled with it (such a frame keeps the fill), every other field uninitialised
        source = {}
        for i, idx in enumerate(idxs):
            for name in fields:
                chunk = 'particles/' + name
                source[i, name] = self._effective_frame(idx, chunk, counts[i])
                if source[i, name] is None and name not in ParticleData._default_value and not f.chunk_exists(0, chunk):
                    raise ValueError("particles/%s is stored neither in frame %d nor in frame 0" % (name, idx))
        for name in fields:
            dt, M, default, _ = _PARTICLE_FIELDS[name]
            shape = (F, K, M) if M > 1 else (F, K)
            if any(source[i, name] is None for i in range(F)):
                setattr(out, name, fl._device_rows(shape, dt, device, default))
            else:
                setattr(out, name, fl._device_empty(shape, dt, device))
        plans = {}
        for i, idx in enumerate(idxs):
            step = ConfigurationData()
            self._read_scalar_any(idx, 'configuration/step', step, 'step')
            out.step[i] = step.step
            if K == 0:
                continue
            n_idx = counts[i]
            for name in fields:
                if source[i, name] is None:
                    continue
                plan = plans.get(n_idx)
                if plan is None:
                    plan = plans[n_idx] = f.plan_rows(rows_dev, n_idx)
                f.read_chunk_device(source[i, name], 'particles/' + name, out=fl._device_at(out[name], i), rows=plan,
                                    wait=False)
            f.wait_read()
        out.plans = plans
        return out

    def _read_logs_device(self, idx, snap):
        f = self.file
        for log in self._names_with_prefix('log/'):
            fr = self._frame_of(idx, log)
            if fr is not None:
                snap.log[log[4:]] = f.read_chunk(fr, log)
        for state in self._names_with_prefix('state/'):
            if f.chunk_exists(idx, state):
                snap.state[state[6:]] = f.read_chunk(idx, state)

    def _read_domain_device(self, idx, snap, domain, scalar4, defaults, n_global, ghost=None, cell_order=None):
        """`read_frame_device(domain=...)`: select the domain's rows from the effective position chunk, then gather every
        per-particle array through them.  One `wait_read` per group of chunks that share destination rows, so the HBM
        staging holds one or two chunks at a time, never the frame; the position chunk the selection staged serves the
        position gather (same index entry, before the group's wait).  Frame 0's device cache of slab reads is not used.
        With ``ghost`` the row list is `halo_rows`' -- owned rows, then ghost rows -- and the gather is the same."""
        f = self.file
        if not isinstance(domain, Domain):
            domain = Domain(*domain)
        dims = int(snap.configuration.dimensions)
        box = snap.configuration.box
        f_pos = self._effective_frame(idx, 'particles/position', n_global)
        if ghost is not None:
            if f_pos is not None:
                rows, snap.n_owned, n_ghost, snap.ghost_shift = f.select_halo_device(f_pos, 'particles/position', box,
                                                                                      domain, ghost, dims)
            else:
                # no position anywhere: every particle sits at the origin, all of them owned, ghosts or neither
                owned, ghosts, shift = halo_rows(numpy.zeros((1, 3), numpy.float32), box, domain, ghost, dims)
                snap.n_owned, n_ghost = n_global * len(owned), n_global * len(ghosts)
                rows = fl._device_from_host(numpy.arange(snap.n_owned + n_ghost, dtype=numpy.int32), f.pipeline_device())
                snap.ghost_shift = fl._device_rows((n_ghost, 3), numpy.int32, f.pipeline_device(),
                                                   shift[0] if n_ghost else numpy.zeros(3, numpy.int32))
            count = snap.n_owned + n_ghost
        else:
            rows, count = self._domain_row_list(f_pos, box, dims, domain, n_global)
        snap.domain = domain
        if cell_order is not None:
            self._order_rows_device(snap, rows, count, cell_order, f_pos, snap.n_owned if ghost is not None else None)
        # group 1: position (the staged rows of the selection) and, with scalar4, (x, y, z, typeid bits)
        self._gather_rows_device(idx, snap, rows, count, scalar4, defaults, n_global,
                                 ('position', 'pos4') if scalar4 else ('position',))

    def _domain_row_list(self, f_pos, box, dims, domain, n_global):
        """The row list of a domain read without a ghost layer, ``(rows, count)`` in GPU memory: selected from the
        position chunk of frame ``f_pos``, which stays staged.  Shared by `read_frame_device` and `frame_stats_device`."""
        f = self.file
        if f_pos is not None:
            return f.select_domain_device(f_pos, 'particles/position', box, domain, dims)
        # no position anywhere: every particle sits at the origin, all of them or none are inside
        count = n_global if len(domain_rows(numpy.zeros((1, 3), numpy.float32), box, domain, dims)) else 0
        return fl._device_from_host(numpy.arange(count, dtype=numpy.int32), f.pipeline_device()), count

    def _order_rows_device(self, snap, rows, count, cells, f_pos, n_owned=None):
        """``read_frame_device(cell_order=...)``: sort the selection's row list (device, ``count`` entries) by cell in
        place, between the selection and the gather -- `pgsd.fl.PGSDFile.order_rows_by_cell_device` over the position
        chunk of frame ``f_pos``, which a selection by domain has left staged (a selection by ``where`` alone has not:
        the chunk is staged here and serves the position gather).  With ``n_owned`` the ghost run is sorted on its own
        and ``snap.ghost_shift`` follows it.  ``f_pos`` None: the position is stored nowhere, every row sits at the
        origin in one cell and the order stays."""
        f = self.file
        dims = int(snap.configuration.dimensions)
        box = snap.configuration.box
        cells = _order_cells(cells, dims)
        snap.cell_grid = cells
        if f_pos is not None:
            snap.cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, cells, rows, n=count, n_owned=n_owned,
                                                    shift=snap.ghost_shift if n_owned is not None else None,
                                                    dimensions=dims)
        else:
            one = cell_ids(numpy.zeros((1, 3), numpy.float32), box, cells, dims).astype(numpy.int32)
            snap.cell = fl._device_rows((count,), numpy.int32, f.pipeline_device(), one)

    def _gather_rows_device(self, idx, snap, rows, count, scalar4, defaults, n_global, staged):
        """The gather half of a domain or group read: every per-particle array of frame ``idx`` through the row list
        ``rows`` (device, ``count`` entries; ascending, or with a ghost layer two ascending runs -- the gather does not
        depend on the order), which becomes ``frame.tag``.  ``staged`` names the attributes
        whose chunks the selection has left staged whole: they are gathered first, in one group, from that staging."""
        f = self.file
        snap.particles.N = count
        snap.particles.N_global = n_global
        snap.part = None
        snap.tag = rows

        # The chunks gathered after the staged ones go through a row plan: in a file whose rows are spatially coherent
        # the selection's rows touch few blocks and only those are read; in a spatially random file every block is
        # touched and the plan hands the read to the whole-chunk route with the same rows.  (The staged attributes, and
        # the type id that shares the position's Scalar4 rows, gather from chunks that are staged whole anyway.)
        plan = []

        def gather(fr, chunk, attr, **kw):
            if attr in staged or count == 0:
                return f.read_chunk_device(fr, chunk, rows=rows, N=count, wait=False, **kw)
            if not plan:
                plan.append(f.plan_rows(rows, n_global))
            return f.read_chunk_device(fr, chunk, rows=plan[0], wait=False, **kw)

        # the staged group; then the Scalar4 arrays not in it; then every other per-particle array: one chunk, one wait
        groups = [tuple(staged)] if staged else []
        groups += [(name,) for name in (('pos4', 'vel4') if scalar4 else ()) if name not in staged]
        groups += [(name,) for name in _PARTICLE_FIELDS if name not in staged]
        self._read_particles_device(idx, snap, count, n_global, defaults, gather, groups)

    def _read_where_device(self, idx, snap, where, domain, scalar4, defaults, n_global, cell_order=None):
        """`read_frame_device(where=...)`: select the rows that satisfy `where_rows` (and lie in ``domain``, if given)
        on the GPU from the effective chunks of the terms' attributes, then gather every per-particle array through
        them.  A term whose attribute the file stores nowhere is decided on the host against the one default row."""
        dims = int(snap.configuration.dimensions)
        box = snap.configuration.box
        if domain is not None and not isinstance(domain, Domain):
            domain = Domain(*domain)
        rows, count, staged = self._where_row_list(idx, snap.particles.types, box, dims, where, domain, scalar4, n_global)
        snap.where = where
        if domain is not None:
            snap.domain = domain
        if cell_order is not None:
            f_pos = self._effective_frame(idx, 'particles/position', n_global)
            self._order_rows_device(snap, rows, count, cell_order, f_pos)
            if f_pos is not None and count > 0 and 'position' not in staged:
                staged[:0] = ['position', 'pos4'] if scalar4 else ['position']      # (staged by the ordering)
        self._gather_rows_device(idx, snap, rows, count, scalar4, defaults, n_global, tuple(staged))

    def _where_row_list(self, idx, types, box, dims, where, domain, scalar4, n_global):
        """The row list of a group read, ``(rows, count, staged)``: the rows in GPU memory, and the attributes whose
        chunks the selection has left staged whole.  Shared by `read_frame_device` and `frame_stats_device`."""
        f = self.file
        terms = _where_terms(where, types)
        all_pass, device_terms, staged = True, [], []
        for name, column, lo, hi, mask in terms:
            fr = self._effective_frame(idx, 'particles/' + name, n_global)
            if (lo is not None and lo != lo) or (hi is not None and hi != hi):
                all_pass = False            # a NaN bound: nothing is kept
            elif fr is None:
                if name not in ParticleData._default_value and not f.chunk_exists(0, 'particles/' + name):
                    raise ValueError("particles/%s is stored neither in frame %d nor in frame 0" % (name, idx))
                row = numpy.array([_PARTICLE_FIELDS[name][2]]).reshape(1, -1)
                all_pass = all_pass and bool(_where_term_keeps(row[:, column], lo, hi, mask)[0])
            else:
                device_terms.append((fr, 'particles/' + name, column, (lo, hi) if mask is None else mask))
                if name not in staged:
                    staged.append(name)
        dom = None
        if domain is not None:
            f_pos = self._effective_frame(idx, 'particles/position', n_global)
            if f_pos is not None:
                dom = (f_pos, 'particles/position', domain)
                staged = [n for n in staged if n != 'position']
                staged[:0] = ['position', 'pos4'] if scalar4 else ['position']
            else:
                # no position anywhere: every particle sits at the origin, all of them or none are inside
                all_pass = all_pass and len(domain_rows(numpy.zeros((1, 3), numpy.float32), box, domain, dims)) > 0
        if not all_pass:
            rows, count, staged = fl._device_from_host(numpy.zeros(0, dtype=numpy.int32), f.pipeline_device()), 0, []
        elif device_terms or dom is not None:
            rows, count = f.select_where_device(device_terms, domain=dom, box=box, dimensions=dims)
        else:
            rows, count = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device()), n_global
        return rows, count, staged

    def _census_frame(self, idx):
        """What a census of frame ``idx`` looks at: ``(box, dimensions, n_global, f_pos)`` -- the frame's configuration
        as a domain read takes it, and the frame whose position chunk it reads (`_effective_frame`; ``None``: stored
        nowhere, every particle sits on the default row)."""
        if idx < 0:
            idx += len(self)
        if idx >= len(self) or idx < 0:
            raise IndexError()
        f = self.file
        conf = ConfigurationData()
        self._read_scalar_any(idx, 'configuration/dimensions', conf, 'dimensions')
        box_frame = self._frame_of(idx, 'configuration/box')
        if box_frame is None:
            box = conf._default_value['box']
        elif box_frame == 0:
            box = self._frame0_small('configuration/box')
        else:
            box = f.read_chunk(box_frame, 'configuration/box')
        fn = self._frame_of(idx, 'particles/N')
        n_global = 0 if fn is None else int((self._frame0_small('particles/N') if fn == 0
                                             else f.read_chunk(fn, 'particles/N'))[0])
        return box, int(conf.dimensions), n_global, self._effective_frame(idx, 'particles/position', n_global)

    _DEFAULT_POSITION = numpy.zeros((1, 3), dtype=numpy.float32)

    def axis_histograms_device(self, idx, bins=1024):
        """`axis_histograms` of frame ``idx``, counted on the GPU from the frame's effective position chunk with the
        frame's box and dimensions: a ``(3, bins)`` int64 numpy array.  The position chunk is staged into HBM, binned
        there in one pass, and released; no per-particle data reaches the host.  A position stored nowhere is all
        defaults and is answered on the host from the one default row."""
        box, dims, n_global, f_pos = self._census_frame(idx)
        if f_pos is None:
            return axis_histograms(self._DEFAULT_POSITION, box, bins, dims) * n_global
        try:
            return self.file.domain_histogram_device(f_pos, 'particles/position', box, _census_bins(bins), dims)
        finally:
            self.file.wait_read()           # the staged chunk is released: a loop over frames piles nothing up in HBM

    def domain_counts_device(self, idx, nx, ny, nz, x_split=None, y_split=None, z_split=None):
        """`domain_counts` of frame ``idx``, counted on the GPU like `axis_histograms_device`: ``(counts, nowhere)``,
        the particle count of every cell of ``domain_grid(nx, ny, nz, x_split, y_split, z_split)`` in its rank order --
        what each rank's ``read_frame_device(idx, domain=...)`` will hold, known before any rank has read."""
        box, dims, n_global, f_pos = self._census_frame(idx)
        n = _census_cells(nx, ny, nz, dims)
        inner = _interior_bounds(grid_bounds(n[0], n[1], n[2], x_split, y_split, z_split))
        if f_pos is None:
            counts, nowhere = domain_counts(self._DEFAULT_POSITION, box, n[0], n[1], n[2], x_split, y_split, z_split, dims)
            return counts * n_global, nowhere * n_global
        try:
            return self.file.domain_counts_device(f_pos, 'particles/position', box, n, inner, dims)
        finally:
            self.file.wait_read()

    def balanced_grid_device(self, idx, nx, ny, nz, bins=1024, min_bins=1):
        """`balanced_grid` of frame ``idx`` on the GPU, with the outcome: ``(domains, splits, counts, nowhere)`` -- the
        decomposition and its split lists as `balanced_grid` returns them, and `domain_counts` of that decomposition.
        One histogram pass, `balanced_splits` on the host, one counting pass served from the rows the histogram left
        staged: the position chunk is read from the file once."""
        box, dims, n_global, f_pos = self._census_frame(idx)
        n = _census_cells(nx, ny, nz, dims)
        bins = _census_bins(bins)
        f = self.file
        try:
            if f_pos is None:
                hist = axis_histograms(self._DEFAULT_POSITION, box, bins, dims) * n_global
            else:
                hist = f.domain_histogram_device(f_pos, 'particles/position', box, bins, dims)
            splits = _balanced_axis_splits(hist, n, min_bins, dims)
            domains = domain_grid(n[0], n[1], n[2], *splits)
            if f_pos is None:
                counts, nowhere = domain_counts(self._DEFAULT_POSITION, box, n[0], n[1], n[2], *splits, dimensions=dims)
                return domains, splits, counts * n_global, nowhere * n_global
            inner = _interior_bounds(grid_bounds(n[0], n[1], n[2], *splits))
            counts, nowhere = f.domain_counts_device(f_pos, 'particles/position', box, n, inner, dims)
            return domains, splits, counts, nowhere
        finally:
            if f_pos is not None:
                f.wait_read()

    def frame_stats(self, idx, fields=_STATS_FIELDS, where=None, domain=None):
        """`frame_stats` of frame ``idx`` read through the host path: a dict from field name to `FieldStats`.  The
        definition of `frame_stats_device`."""
        return frame_stats(self[int(idx)], fields, where=where, domain=domain)

    def frame_stats_device(self, idx, fields=_STATS_FIELDS, where=None, domain=None):
        """`frame_stats` of frame ``idx``, reduced on the GPU: a dict from field name to `FieldStats` that equals
        ``frame_stats(idx, ...)`` exactly, the sums bit for bit.

        The selection is `read_frame_device`'s own -- ``where``, ``domain`` or both, selected on the GPU --; without one
        every row counts and no row list exists.  Each field's effective chunk (the frame's, else frame 0's) is staged
        into HBM -- a chunk the selection staged is not read again: those fields are reduced first --, reduced there in
        one pass (`pgsd.fl.PGSDFile.chunk_stats_device`) and released by one `wait_read`: a loop over fields or frames
        holds the selection's chunks or one field's in HBM, and no per-particle data reaches the host.  Float fields of three columns get the
        ``norm2`` column: ``stats['velocity'].max[3]`` is the square of the largest speed.  A field that is stored
        nowhere is all defaults and is answered on the host from the one default row.
        """
        idx = self._frame_index(idx)
        names = _stats_fields(fields)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        rows = None
        try:
            rows, count, staged = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
            # the fields whose chunks the selection left staged come first and share one wait: they are not read again
            first = [name for name in names if name in staged]
            out = {}
            for name in first + [name for name in names if name not in first]:
                dt, M, default, upstream = _PARTICLE_FIELDS[name]
                norm2 = _stats_norm2(dt, M)
                fr = self._effective_frame(idx, 'particles/' + name, n_global)
                if fr is None:
                    if upstream:
                        raise ValueError("arrays holds no '%s'" % name)
                    # stored nowhere: `count` copies of the default row, in the definition's order
                    row = numpy.ascontiguousarray(numpy.broadcast_to(numpy.asarray(default, dtype=dt), (M,)))
                    out[name] = column_stats(numpy.broadcast_to(row, (count, M)), norm2=norm2)
                    continue
                try:
                    out[name] = f.chunk_stats_device(fr, 'particles/' + name, rows=rows,
                                                     n=None if rows is None else count, norm2=norm2)
                finally:
                    if name not in first[:-1]:
                        f.wait_read()   # the staged chunk is released: a loop over fields piles nothing up in HBM
            return OrderedDict((name, out[name]) for name in names)
        finally:
            if rows is not None:
                f.wait_read()           # (a selection whose chunks no field used)

    def frame_moments(self, idx, by_type=True, centre=True, where=None, domain=None):
        """`frame_moments` of frame ``idx`` read through the host path: a `Moments`.  The definition of
        `frame_moments_device`."""
        return frame_moments(self[int(idx)], by_type=by_type, centre=centre, where=where, domain=domain)

    def frame_moments_device(self, idx, by_type=True, centre=True, where=None, domain=None):
        """`frame_moments` of frame ``idx``, reduced on the GPU: a `Moments` that equals ``frame_moments(idx, ...)``
        exactly, the sums bit for bit.

        The selection is `frame_stats_device`'s -- ``where``, ``domain`` or both, selected on the GPU --; without one
        every row counts and no row list exists.  The effective chunks (the frame's, else frame 0's) of ``typeid``,
        ``mass``, ``velocity``, ``energy`` and, with ``centre``, ``position`` are staged into HBM -- a chunk the selection
        staged is not read again -- and reduced there in one pass over all of them
        (`pgsd.fl.PGSDFile.frame_moments_device`); a chunk that is stored nowhere costs nothing: its schema default
        stands for every row and nothing is materialised.  More than four types take consecutive passes over the same
        staged chunks, so no file byte is read twice; one `wait_read` at the end releases them.  No per-particle data
        reaches the host.  ``position`` is used as stored: see `frame_moments`.
        """
        idx = self._frame_index(idx)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        types = self._types_of(idx)
        try:
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos, types)
            names = ['typeid' if by_type else None, 'mass', 'velocity', 'energy', 'position' if centre else None]
            chunks = []
            for name in names:
                fr = None if name is None else self._effective_frame(idx, 'particles/' + name, n_global)
                chunks.append(None if fr is None else (fr, 'particles/' + name))
            defaults = numpy.concatenate([numpy.broadcast_to(numpy.asarray(_PARTICLE_FIELDS[name][2], dtype=numpy.float32),
                                                             (M,)) for name, M, _ in _MOMENTS_INPUTS]).astype(numpy.float64)
            n = count if rows is not None or all(c is None for c in chunks) else None
            return self._grouped_by_type(
                lambda t0, n_types: f.frame_moments_device(chunks, defaults, type0=t0, n_types=n_types, rows=rows, n=n),
                Moments, lambda k: Moments.from_sums([0] * k, [0] * k, 0, numpy.zeros((k, _MOMENTS_QUANTITIES))),
                _MOMENTS_MAX_TYPES, len(types), by_type, chunks[0] is not None, count)
        finally:
            f.wait_read()

    def cell_moments(self, idx, cells, centre=True, where=None, domain=None):
        """`frame_cell_moments` of frame ``idx`` read through the host path: a `CellMoments`.  The definition of
        `cell_moments_device`."""
        return frame_cell_moments(self[int(idx)], cells, centre=centre, where=where, domain=domain)

    def cell_moments_device(self, idx, cells, centre=True, where=None, domain=None):
        """`frame_cell_moments` of frame ``idx``, reduced on the GPU: a `CellMoments` that equals
        ``cell_moments(idx, cells, ...)`` exactly, the sums bit for bit.

        The selection is `frame_moments_device`'s; without one the row list is every row in file order.  The list is
        sorted by cell over the staged position chunk (`pgsd.fl.PGSDFile.order_rows_by_cell_device`) and the effective
        chunks of ``mass``, ``velocity``, ``energy`` and, with ``centre``, ``position`` are reduced per cell in one
        segmented pass (`pgsd.fl.PGSDFile.cell_moments_device`); a chunk the selection or the ordering staged is not read
        again, a chunk that is stored nowhere costs nothing, and a position that is stored nowhere puts every row into
        the origin's cell.  One `wait_read` at the end releases the staged chunks.  No per-particle data reaches the host.
        """
        idx = self._frame_index(idx)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        grid = _order_cells(cells, dims)
        n_cells = grid[0] * grid[1] * grid[2]
        if n_cells > _CELLS_MAX_CELLS:
            raise ValueError("a grid holds at most 2^20 cells: %r" % (cells,))
        try:
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
            if rows is None:
                rows = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device())
            if f_pos is not None:
                cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows, n=count, dimensions=dims)
            else:
                one = cell_ids(numpy.zeros((1, 3), numpy.float32), box, grid, dims).astype(numpy.int32)
                cell = fl._device_rows((max(count, 1),), numpy.int32, f.pipeline_device(), one)
            chunks = []
            for name in ('mass', 'velocity', 'energy', 'position' if centre else None):
                fr = None if name is None else self._effective_frame(idx, 'particles/' + name, n_global)
                chunks.append(None if fr is None else (fr, 'particles/' + name))
            defaults = numpy.concatenate([numpy.broadcast_to(numpy.asarray(_PARTICLE_FIELDS[name][2], dtype=numpy.float32),
                                                             (M,)) for name, M, _ in _MOMENTS_INPUTS]).astype(numpy.float64)
            got = f.cell_moments_device(chunks, rows, cell, count, n_cells, defaults)
        finally:
            f.wait_read()
        b = numpy.asarray(box, dtype=numpy.float64).reshape(-1)
        got.grid = grid
        got.cell_volume = (b[0] * b[1] * (b[2] if dims == 3 else 1.0)) / n_cells
        return got

    def frame_neighbours(self, idx, r, bins=0, cells=None, where=None, domain=None):
        """`frame_neighbours` of frame ``idx`` read through the host path: a `Neighbours`.  The definition of
        `frame_neighbours_device`."""
        return frame_neighbours(self[int(idx)], r, bins=bins, cells=cells, where=where, domain=domain)

    def frame_neighbours_device(self, idx, r, bins=0, cells=None, where=None, domain=None, return_rows=False):
        """`frame_neighbours` of frame ``idx``, on the GPU: a `Neighbours` whose summary equals
        ``frame_neighbours(idx, r, ...)`` exactly -- every counter and index, ``closest2`` bit for bit.

        The selection is `frame_moments_device`'s and is the list both ``i`` and ``j`` come from; without one it is
        every row.  The list is sorted by cell over the staged position chunk
        (`pgsd.fl.PGSDFile.order_rows_by_cell_device`) with the grid `neighbour_grid_for` gives (or ``cells``, checked
        like the model's), and the pair pass (`pgsd.fl.PGSDFile.neighbours_device`) runs over the same staged chunk.
        ``return_rows=True`` leaves ``rows``, ``cell``, ``count``, ``nearest2`` and ``nearest`` in GPU memory on the
        result; otherwise they are ``None`` and no per-particle data is kept.  One `wait_read` at the end releases the
        staged chunk.  A frame whose position is stored nowhere has no chunk to search and raises ValueError.
        """
        idx = self._frame_index(idx)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        grid = _neighbour_grid(box, r, cells, dims)
        if int(bins):
            neighbour_edges2(r, bins)
        if f_pos is None:
            raise ValueError("frame_neighbours_device: the position is stored nowhere (every particle sits at the origin)")
        try:
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
            if rows is None:
                rows = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device())
            cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows, n=count, dimensions=dims)
            got = f.neighbours_device(f_pos, 'particles/position', box, r, grid, rows, cell, n=count, dimensions=dims,
                                      bins=bins, return_rows=return_rows)
        finally:
            f.wait_read()
        return got

    def frame_neighbour_list(self, idx, r, half=False, distances=False, cells=None, where=None, domain=None):
        """`frame_neighbour_list` of frame ``idx`` read through the host path: a `NeighbourList`.  The definition of
        `frame_neighbour_list_device`."""
        return frame_neighbour_list(self[int(idx)], r, half=half, distances=distances, cells=cells, where=where,
                                    domain=domain)

    def frame_neighbour_list_device(self, idx, r, half=False, distances=False, cells=None, where=None, domain=None):
        """`frame_neighbour_list` of frame ``idx``, on the GPU: a `NeighbourList` that equals
        ``frame_neighbour_list(idx, r, ...)`` exactly -- every offset and index, ``distance2`` bit for bit -- with
        ``rows``, ``cell``, ``offsets``, ``neighbours`` and ``distance2`` in GPU memory.

        The selection, the grid, the ordering over the staged position chunk and the one closing `wait_read` are
        `frame_neighbours_device`'s; the two passes (`pgsd.fl.PGSDFile.neighbour_list_device`) run over the same staged
        chunk.  Read with ``read_frame_device(idx, where=..., domain=..., cell_order=grid)`` for the same selection and
        grid, without a ghost layer, row ``k`` of the restarted arrays is list position ``k``: ``neighbours`` indexes
        them directly.  A frame whose position is stored nowhere has no chunk to search and raises ValueError.
        """
        idx = self._frame_index(idx)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        grid = _neighbour_grid(box, r, cells, dims)
        if f_pos is None:
            raise ValueError("frame_neighbour_list_device: the position is stored nowhere (every particle sits at the "
                             "origin)")
        try:
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
            if rows is None:
                rows = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device())
            cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows, n=count, dimensions=dims)
            got = f.neighbour_list_device(f_pos, 'particles/position', box, r, grid, rows, cell, n=count, dimensions=dims,
                                          half=half, distances=distances)
        finally:
            f.wait_read()
        return got

    def frame_components(self, idx, r, cells=None, where=None, domain=None):
        """`frame_components` of frame ``idx`` read through the host path: a `Components`.  The definition of
        `frame_components_device`."""
        return frame_components(self[int(idx)], r, cells=cells, where=where, domain=domain)

    def frame_components_device(self, idx, r, cells=None, where=None, domain=None):
        """`frame_components` of frame ``idx``, on the GPU: a `Components` that equals ``frame_components(idx, r, ...)``
        exactly -- every label, id, size and summary word -- with ``rows``, ``cell``, ``label``, ``component`` and
        ``sizes`` in GPU memory.

        The selection, the grid, the ordering over the staged position chunk and the one closing `wait_read` are
        `frame_neighbour_list_device`'s; the pass (`pgsd.fl.PGSDFile.components_device`) runs over the same staged chunk.
        Read with ``read_frame_device(idx, where=..., domain=..., cell_order=grid)`` for the same selection and grid,
        without a ghost layer, row ``k`` of the restarted arrays is list position ``k``: ``label`` indexes them directly
        and ``component[k]`` belongs to restarted row ``k``.  A frame whose position is stored nowhere has no chunk to
        search and raises ValueError.
        """
        idx = self._frame_index(idx)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        grid = _neighbour_grid(box, r, cells, dims)
        if f_pos is None:
            raise ValueError("frame_components_device: the position is stored nowhere (every particle sits at the "
                             "origin)")
        try:
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
            if rows is None:
                rows = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device())
            cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows, n=count, dimensions=dims)
            got = f.components_device(f_pos, 'particles/position', box, r, grid, rows, cell, n=count, dimensions=dims)
        finally:
            f.wait_read()
        return got

    def frame_component_moments(self, idx, r, cells=None, where=None, domain=None):
        """`frame_component_moments` of frame ``idx`` read through the host path: a `ComponentMoments`.  The definition
        of `frame_component_moments_device`."""
        return frame_component_moments(self[int(idx)], r, cells=cells, where=where, domain=domain)

    def frame_component_moments_device(self, idx, r, cells=None, where=None, domain=None):
        """`frame_component_moments` of frame ``idx``, on the GPU: a `ComponentMoments` that equals
        ``frame_component_moments(idx, r, ...)`` exactly -- every counter and flag, every float bit for bit -- with its
        tables, ``sizes`` and the arrays of ``components_of`` in GPU memory (``to_host()`` copies the tables).

        The selection, the grid and the ordering over the staged position chunk are `frame_components_device`'s; the
        components pass (`pgsd.fl.PGSDFile.components_device`) and then the moments
        (`pgsd.fl.PGSDFile.component_moments_device`) run over the same staged position chunk and the effective chunks of
        ``mass``, ``velocity`` and ``energy``; one that is stored nowhere costs nothing, its schema default stands for
        every row.  One `wait_read` at the end releases the staged chunks, on error paths too.  No per-particle array
        reaches the host.  A frame whose position is stored nowhere has no chunk to search and raises ValueError.
        """
        idx = self._frame_index(idx)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        grid = _neighbour_grid(box, r, cells, dims)
        if f_pos is None:
            raise ValueError("frame_component_moments_device: the position is stored nowhere (every particle sits at the "
                             "origin)")
        try:
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
            if rows is None:
                rows = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device())
            cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows, n=count, dimensions=dims)
            comps = f.components_device(f_pos, 'particles/position', box, r, grid, rows, cell, n=count, dimensions=dims)
            chunks = []
            for name in ('mass', 'velocity', 'energy'):
                fr = self._effective_frame(idx, 'particles/' + name, n_global)
                chunks.append(None if fr is None else (fr, 'particles/' + name))
            chunks.append((f_pos, 'particles/position'))
            defaults = numpy.concatenate([numpy.broadcast_to(numpy.asarray(_PARTICLE_FIELDS[name][2], dtype=numpy.float32),
                                                             (M,)) for name, M, _ in _MOMENTS_INPUTS]).astype(numpy.float64)
            got = f.component_moments_device(chunks, box, comps.rows, comps.label, comps.component, comps.n,
                                             comps.components, defaults=defaults, dimensions=dims)
        finally:
            f.wait_read()
        got.components_of, got.sizes = comps, comps.sizes
        return got

    def frame_kernel_sums(self, idx, h=None, kernel='wendland_c2', cells=None, where=None, domain=None, surface_below=None):
        """`frame_kernel_sums` of frame ``idx`` read through the host path: a `KernelSums`.  The definition of
        `frame_kernel_sums_device`."""
        return frame_kernel_sums(self[int(idx)], h, kernel=kernel, cells=cells, where=where, domain=domain,
                                 surface_below=surface_below)

    def frame_kernel_sums_device(self, idx, h=None, kernel='wendland_c2', cells=None, where=None, domain=None,
                                 surface_below=None, return_rows=False):
        """`frame_kernel_sums` of frame ``idx``, on the GPU: a `KernelSums` that equals ``frame_kernel_sums(idx, h,
        ...)`` exactly -- every counter and index, every float bit for bit.

        ``h=None`` takes the frame's ``slength`` if its smallest and largest value are equal
        (`pgsd.fl.PGSDFile.chunk_stats_device` of the whole chunk; stored nowhere: the schema default 1.0) and raises
        ValueError if they differ.  The selection is `frame_neighbours_device`'s and is the list both ``i`` and ``j``
        come from; without one it is every row.  The list is sorted by cell over the staged position chunk with the
        grid `neighbour_grid_for` gives for the support ``2h`` (or ``cells``, checked like the model's), and the pass
        (`pgsd.fl.PGSDFile.sph_sums_device`) runs over the same staged chunk and the effective ``mass`` and ``density``
        chunks; one that is stored nowhere costs nothing, its schema default stands for every row.
        ``return_rows=True`` leaves ``rows``, ``cell``, ``number``, ``density`` and ``shepard`` in GPU memory on the
        result; otherwise they are ``None`` and no per-particle data is kept.  One `wait_read` at the end releases the
        staged chunks.  A frame whose position is stored nowhere has no chunk to search and raises ValueError.
        """
        f = self.file
        try:
            f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults = self._sph_device_list(
                "frame_kernel_sums_device", idx, h, kernel, cells, where, domain, ('mass', 'density'))
            got = f.sph_sums_device(f_pos, 'particles/position', box, h, grid, rows, cell, n=count, mass=chunks[0],
                                    density=chunks[1], defaults=defaults, dimensions=dims, kernel=kernel,
                                    surface_below=surface_below, return_rows=return_rows)
        finally:
            f.wait_read()
        return got

    def _sph_device_list(self, who, idx, h, kernel, cells, where, domain, names, second=None):
        """What `frame_kernel_sums_device`, `frame_kernel_gradients_device`, `frame_gradient_tensors_device` and
        `frame_accelerations_device` share ahead of their pass: the ``h=None``
        rule, the grid for the support ``2h``, the selection as a row list sorted by cell on the GPU and, for each of
        ``names``, the effective chunk ``(frame, name)`` or ``None``.  ``(f_pos, box, dims, h, grid, rows, cell, count,
        chunks, [mass default, density default])``; the caller ends with `wait_read`, whatever is raised here.
        ``second``: one more ``where`` (`frame_body_force_device`), selected and ordered the same way on the same grid;
        its ``(rows, cell, count)`` is appended to the result."""
        idx = self._frame_index(idx)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        _sph_kernel_id(kernel)
        if h is None:
            f_h = self._effective_frame(idx, 'particles/slength', n_global)
            if f_h is None or n_global == 0:
                h = float(_PARTICLE_FIELDS['slength'][2])
            else:
                stats = f.chunk_stats_device(f_h, 'particles/slength')
                h = _uniform_slength(float(stats.min[0]), float(stats.max[0]))
        h = _sph_length(h)
        grid = _neighbour_grid(box, float(numpy.float64(2.0) * numpy.float64(h)), cells, dims)
        if f_pos is None:
            raise ValueError("%s: the position is stored nowhere (every particle sits at the origin)" % who)
        rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
        if rows is None:
            rows = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device())
        cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows, n=count, dimensions=dims)
        chunks = []
        for name in names:
            fr = self._effective_frame(idx, 'particles/' + name, n_global)
            chunks.append(None if fr is None else (fr, 'particles/' + name))
        defaults = [float(_PARTICLE_FIELDS[name][2]) for name in ('mass', 'density')]
        if second is not None:
            rows2, count2, _ = self._selection_row_list(idx, second, domain, box, dims, n_global, f_pos)
            cell2 = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows2, n=count2, dimensions=dims)
            return f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults, (rows2, cell2, count2)
        return f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults

    def frame_adaptive_sums(self, idx, kernel='wendland_c2', mode='gather', cells=None, where=None, domain=None,
                            surface_below=None):
        """`frame_adaptive_sums` of frame ``idx`` read through the host path: an `AdaptiveSums`.  The definition of
        `frame_adaptive_sums_device`."""
        return frame_adaptive_sums(self[int(idx)], kernel=kernel, mode=mode, cells=cells, where=where, domain=domain,
                                   surface_below=surface_below)

    def frame_adaptive_sums_device(self, idx, kernel='wendland_c2', mode='gather', cells=None, where=None, domain=None,
                                   surface_below=None, return_rows=False):
        """`frame_adaptive_sums` of frame ``idx``, on the GPU: an `AdaptiveSums` that equals ``frame_adaptive_sums(idx,
        ...)`` exactly -- every counter and index, every float bit for bit.

        The selection is `frame_kernel_sums_device`'s.  `pgsd.fl.PGSDFile.smoothing_range_device` reduces the effective
        ``slength`` chunk over it (stored nowhere: the schema default 1.0, nothing is read), the grid is
        `neighbour_grid_for` of ``2*h_max`` (or ``cells``, checked like the model's), the list is sorted by cell over the
        staged position chunk and the pass (`pgsd.fl.PGSDFile.sph_adaptive_sums_device`) runs over the staged chunks; no
        row is copied to the host.  ``return_rows=True`` leaves ``rows``, ``cell``, ``count``, ``number``, ``density``,
        ``shepard`` and ``omega`` in GPU memory on the result.  One `wait_read` at the end releases the staged chunks.
        A frame whose position is stored nowhere has no chunk to search and raises ValueError, and so does a selection
        that is not empty and holds no valid smoothing length.
        """
        f = self.file
        who = "frame_adaptive_sums_device"
        try:
            idx = self._frame_index(idx)
            box, dims, n_global, f_pos = self._census_frame(idx)
            _sph_kernel_id(kernel), _sph_mode_id(mode)
            if f_pos is None:
                raise ValueError("%s: the position is stored nowhere (every particle sits at the origin)" % who)
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos)
            if rows is None:
                rows = fl._device_from_host(numpy.arange(n_global, dtype=numpy.int32), f.pipeline_device())
            f_h = self._effective_frame(idx, 'particles/slength', n_global)
            slength = None if f_h is None else (f_h, 'particles/slength')
            defaults = [float(_PARTICLE_FIELDS[name][2]) for name in ('mass', 'density', 'slength')]
            listed, _, _, h_max = f.smoothing_range_device(slength, n_global, rows, n=count, default=defaults[2])
            if not listed:
                nothing = numpy.zeros(0, dtype=numpy.float64)
                words = _spha_summary(0, 0, numpy.zeros(0, dtype=bool), None, nothing, numpy.zeros(0, dtype=numpy.uint32),
                                      nothing, nothing, None, None, None, None)
                return AdaptiveSums(h_max, kernel, mode, (1, 1, 1) if cells is None else _order_cells(cells, dims), dims, words,
                                    True, surface_below)
            if not h_max > 0.0:
                raise ValueError("no listed row has a valid smoothing length (finite and positive)")
            grid = _neighbour_grid(box, float(numpy.float64(2.0) * numpy.float64(h_max)), cells, dims)
            cell = f.order_rows_by_cell_device(f_pos, 'particles/position', box, grid, rows, n=count, dimensions=dims)
            chunks = []
            for name in ('mass', 'density'):
                fr = self._effective_frame(idx, 'particles/' + name, n_global)
                chunks.append(None if fr is None else (fr, 'particles/' + name))
            got = f.sph_adaptive_sums_device(f_pos, 'particles/position', box, h_max, grid, rows, cell, n=count,
                                             slength=slength, mass=chunks[0], density=chunks[1], defaults=defaults,
                                             dimensions=dims, kernel=kernel, mode=mode, surface_below=surface_below,
                                             return_rows=return_rows)
        finally:
            f.wait_read()
        return got

    def frame_kernel_gradients(self, idx, h=None, kernel='wendland_c2', cells=None, where=None, domain=None):
        """`frame_kernel_gradients` of frame ``idx`` read through the host path: a `KernelGradients`.  The definition of
        `frame_kernel_gradients_device`."""
        return frame_kernel_gradients(self[int(idx)], h, kernel=kernel, cells=cells, where=where, domain=domain)

    def frame_kernel_gradients_device(self, idx, h=None, kernel='wendland_c2', cells=None, where=None, domain=None,
                                      return_rows=False):
        """`frame_kernel_gradients` of frame ``idx``, on the GPU: a `KernelGradients` that equals
        ``frame_kernel_gradients(idx, h, ...)`` exactly -- every counter and index, every float bit for bit.

        ``h=None``, the selection, the grid and the ordering are `frame_kernel_sums_device`'s; the pass
        (`pgsd.fl.PGSDFile.sph_gradients_device`) runs over the staged position chunk and the effective ``velocity``,
        ``mass`` and ``density`` chunks; one that is stored nowhere costs nothing: the zero vector and the schema defaults
        stand for every row.  ``return_rows=True`` leaves ``rows``, ``cell``, ``density_rate``, ``divergence``, ``curl``
        and ``normal`` in GPU memory on the result; otherwise they are ``None`` and no per-particle data is kept.  One
        `wait_read` at the end releases the staged chunks.  A frame whose position is stored nowhere has no chunk to
        search and raises ValueError.
        """
        f = self.file
        try:
            f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults = self._sph_device_list(
                "frame_kernel_gradients_device", idx, h, kernel, cells, where, domain, ('mass', 'density', 'velocity'))
            got = f.sph_gradients_device(f_pos, 'particles/position', box, h, grid, rows, cell, n=count, velocity=chunks[2],
                                         mass=chunks[0], density=chunks[1], defaults=defaults, dimensions=dims, kernel=kernel,
                                         return_rows=return_rows)
        finally:
            f.wait_read()
        return got

    def frame_gradient_tensors(self, idx, h=None, kernel='wendland_c2', det_min=0.25, cells=None, where=None, domain=None):
        """`frame_gradient_tensors` of frame ``idx`` read through the host path: a `KernelTensors`.  The definition of
        `frame_gradient_tensors_device`."""
        return frame_gradient_tensors(self[int(idx)], h, kernel=kernel, det_min=det_min, cells=cells, where=where,
                                      domain=domain)

    def frame_gradient_tensors_device(self, idx, h=None, kernel='wendland_c2', det_min=0.25, cells=None, where=None,
                                      domain=None, return_rows=False):
        """`frame_gradient_tensors` of frame ``idx``, on the GPU: a `KernelTensors` that equals
        ``frame_gradient_tensors(idx, h, ...)`` exactly -- every counter and index, every float bit for bit.

        ``h=None``, the selection, the grid and the ordering are `frame_kernel_sums_device`'s; the pass
        (`pgsd.fl.PGSDFile.sph_tensors_device`) runs over the staged position chunk and the effective ``velocity``,
        ``mass`` and ``density`` chunks; one that is stored nowhere costs nothing: the zero vector and the schema defaults
        1.0 and 0.0 stand for every row.  ``return_rows=True`` leaves ``rows``, ``cell``, ``correction``, ``determinant``,
        ``velocity_gradient`` and ``shear_rate`` in GPU memory on the result; otherwise they are ``None`` and no
        per-particle data is kept.  One `wait_read` at the end releases the staged chunks.  A frame whose position is
        stored nowhere has no chunk to search and raises ValueError.
        """
        f = self.file
        try:
            det_min = _sph_det_min(det_min)
            f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults = self._sph_device_list(
                "frame_gradient_tensors_device", idx, h, kernel, cells, where, domain, ('mass', 'density', 'velocity'))
            got = f.sph_tensors_device(f_pos, 'particles/position', box, h, grid, rows, cell, n=count, velocity=chunks[2],
                                       mass=chunks[0], density=chunks[1], defaults=defaults, dimensions=dims, kernel=kernel,
                                       det_min=det_min, return_rows=return_rows)
        finally:
            f.wait_read()
        return got

    def frame_accelerations(self, idx, h=None, kernel='wendland_c2', viscosity=None, gravity=None, cells=None, where=None,
                            domain=None):
        """`frame_accelerations` of frame ``idx`` read through the host path: a `KernelAccelerations`.  The definition of
        `frame_accelerations_device`."""
        return frame_accelerations(self[int(idx)], h, kernel=kernel, viscosity=viscosity, gravity=gravity, cells=cells,
                                   where=where, domain=domain)

    def frame_accelerations_device(self, idx, h=None, kernel='wendland_c2', viscosity=None, gravity=None, cells=None,
                                   where=None, domain=None, return_rows=False):
        """`frame_accelerations` of frame ``idx``, on the GPU: a `KernelAccelerations` that equals
        ``frame_accelerations(idx, h, ...)`` exactly -- every counter and index, every float bit for bit.

        ``h=None``, the selection, the grid and the ordering are `frame_kernel_sums_device`'s; the pass
        (`pgsd.fl.PGSDFile.sph_accelerations_device`) runs over the staged position chunk and the effective ``velocity``,
        ``mass``, ``density`` and ``pressure`` chunks; one that is stored nowhere costs nothing: the zero vector and the
        schema defaults 1.0, 0.0 and 0.0 stand for every row.  ``return_rows=True`` leaves ``rows``, ``cell``,
        ``pressure_acc``, ``viscous_acc`` and ``total`` in GPU memory on the result; otherwise they are ``None`` and no
        per-particle data is kept.  One `wait_read` at the end releases the staged chunks.  A frame whose position is
        stored nowhere has no chunk to search and raises ValueError.
        """
        f = self.file
        try:
            mu, g = _sph_viscosity(viscosity), _sph_gravity(gravity)
            f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults = self._sph_device_list(
                "frame_accelerations_device", idx, h, kernel, cells, where, domain, ('mass', 'density', 'velocity', 'pressure'))
            got = f.sph_accelerations_device(f_pos, 'particles/position', box, h, grid, rows, cell, n=count, velocity=chunks[2],
                                             mass=chunks[0], density=chunks[1], pressure=chunks[3],
                                             defaults=defaults + [float(_PARTICLE_FIELDS['pressure'][2])], viscosity=mu,
                                             gravity=g, dimensions=dims, kernel=kernel, return_rows=return_rows)
        finally:
            f.wait_read()
        return got

    def frame_body_force(self, idx, body, fluid, h=None, kernel='wendland_c2', viscosity=None, about=None, cells=None,
                         domain=None):
        """`frame_body_force` of frame ``idx`` read through the host path: a `KernelBodyForce`.  The definition of
        `frame_body_force_device`."""
        return frame_body_force(self[int(idx)], body, fluid, h, kernel=kernel, viscosity=viscosity, about=about, cells=cells,
                                domain=domain)

    def frame_body_force_device(self, idx, body, fluid, h=None, kernel='wendland_c2', viscosity=None, about=None, cells=None,
                                domain=None, return_rows=False):
        """`frame_body_force` of frame ``idx``, on the GPU: a `KernelBodyForce` that equals ``frame_body_force(idx, body,
        fluid, h, ...)`` exactly -- every counter and index, every float bit for bit.

        ``body`` and ``fluid`` are ``where`` dicts, both required; each is selected on the GPU (with ``domain``:
        intersected with it) and sorted by cell over the staged position chunk on one grid, `frame_kernel_sums_device`'s
        for the support ``2h``; ``h=None`` is its rule too.  One pass (`pgsd.fl.PGSDFile.sph_body_force_device`) runs over
        the staged position chunk and the effective ``velocity``, ``mass``, ``density`` and ``pressure`` chunks, which
        both lists read; one that is stored nowhere costs nothing.  ``return_rows=True`` leaves the targets' ``rows``,
        ``cell``, ``contacts``, ``pressure_acc`` and ``viscous_acc`` in GPU memory on the result; otherwise they are
        ``None``.  One `wait_read` at the end releases the staged chunks.  A frame whose position is stored nowhere has no
        chunk to search and raises ValueError.
        """
        f = self.file
        try:
            mu, c = _sph_viscosity(viscosity), _sph_about(about)
            if body is None or fluid is None:
                raise ValueError("body and fluid are where dicts: both are required")
            f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults, (rows2, cell2, count2) = self._sph_device_list(
                "frame_body_force_device", idx, h, kernel, cells, body, domain, ('mass', 'density', 'velocity', 'pressure'),
                second=fluid)
            got = f.sph_body_force_device(f_pos, 'particles/position', box, h, grid, rows, cell, rows2, cell2, n_body=count,
                                          n_fluid=count2, velocity=chunks[2], mass=chunks[0], density=chunks[1],
                                          pressure=chunks[3], defaults=defaults + [float(_PARTICLE_FIELDS['pressure'][2])],
                                          viscosity=mu, about=c, dimensions=dims, kernel=kernel, return_rows=return_rows)
        finally:
            f.wait_read()
        return got

    def frame_samples(self, idx, points, fields=('velocity',), h=None, kernel='wendland_c2', normalise=False, cells=None,
                      where=None, domain=None):
        """`frame_samples` of frame ``idx`` read through the host path: a `KernelSamples`.  The definition of
        `frame_samples_device`."""
        return frame_samples(self[int(idx)], points, fields=fields, h=h, kernel=kernel, normalise=normalise, cells=cells,
                             where=where, domain=domain)

    def frame_samples_device(self, idx, points, fields=('velocity',), h=None, kernel='wendland_c2', normalise=False,
                             cells=None, where=None, domain=None):
        """`frame_samples` of frame ``idx``, on the GPU: a `KernelSamples` that equals ``frame_samples(idx, points, ...)``
        exactly -- every counter and index, every float bit for bit -- with ``count``, ``density``, ``shepard`` and
        ``values`` in GPU memory.

        ``points`` is a numpy array (uploaded) or ``K x 3`` float64 values in GPU memory.  ``h=None``, the selection, the
        grid and the ordering are `frame_kernel_sums_device`'s; the pass (`pgsd.fl.PGSDFile.sph_samples_device`) runs
        over the staged position chunk and the effective ``mass`` and ``density`` chunks and those of ``fields``; one that
        is stored nowhere costs nothing: its schema default stands for every row.  One `wait_read` at the end releases the
        staged chunks.  A frame whose position is stored nowhere has no chunk to search and raises ValueError.
        """
        f = self.file
        try:
            asked = _sphs_fields(fields)
            f_pos, box, dims, h, grid, rows, cell, count, chunks, defaults = self._sph_device_list(
                "frame_samples_device", idx, h, kernel, cells, where, domain,
                ('mass', 'density') + tuple(name for name, _, _ in asked))
            values = [(chunk, M, default) for chunk, (_, M, default) in zip(chunks[2:], asked)]
            got = f.sph_samples_device(f_pos, 'particles/position', box, h, grid, rows, cell, points, n=count, values=values,
                                       mass=chunks[0], density=chunks[1], defaults=defaults, dimensions=dims, kernel=kernel,
                                       normalise=normalise)
        finally:
            f.wait_read()
        return got

    def _types_of(self, idx):
        """The type names frame ``idx`` reads: its own, else frame 0's, else the schema's default."""
        ft = self._frame_of(idx, 'particles/types')
        return ParticleData._default_value['types'] if ft is None else _decode_strings(
            self._frame0_small('particles/types') if ft == 0 else self.file.read_chunk(ft, 'particles/types'))

    def _selection_row_list(self, idx, where, domain, box, dims, n_global, f_pos, types=None):
        """``where``, ``domain`` or both, selected on the GPU in frame ``idx``: ``(rows, count, staged)`` -- the row list
        in GPU memory, its entries and the fields whose chunks the selection left staged --; without a selection every
        row counts and no row list exists: ``(None, n_global, [])``."""
        if domain is not None and not isinstance(domain, Domain):
            domain = Domain(*domain)
        if where is not None:
            return self._where_row_list(idx, self._types_of(idx) if types is None else types, box, dims, where, domain,
                                        False, n_global)
        if domain is not None:
            rows, count = self._domain_row_list(f_pos, box, dims, domain, n_global)
            return rows, count, ['position']
        return None, n_global, []

    @staticmethod
    def _grouped_by_type(launch, cls, nothing, group, T, by_type, has_typeid, count):
        """A grouped reduction's result (a ``cls``: `Moments`, `Displacements`) over ``T`` types and ``count`` entries.
        ``launch(type0, n_types)`` is one pass over the staged chunks for up to ``group`` consecutive types, ``nothing(k)``
        the result of ``k`` types that hold no entry.  More than ``group`` types take consecutive passes."""
        if by_type and T == 0:
            return cls.concatenate([nothing(0)], count)
        if not by_type or not has_typeid:
            # one group; by type without a stored typeid every particle is of type 0
            part = launch(0, 1)
            return part if not by_type or T == 1 else cls.concatenate([part, nothing(T - 1)], count)
        return cls.concatenate([launch(t0, min(group, T - t0)) for t0 in range(0, T, group)], count)

    def _frame_index(self, idx):
        idx = int(idx)
        if idx < 0:
            idx += len(self)
        if idx >= len(self) or idx < 0:
            raise IndexError()
        return idx

    def frame_displacements(self, idx, origin=0, by_type=True, images=True, minimum_image=False, where=None, domain=None,
                            return_rows=False):
        """`frame_displacements` from frame ``origin`` to frame ``idx``, both read through the host path: a
        `Displacements` (with ``return_rows`` also `displacement_vectors` of the selection, a host array).  The
        definition of `frame_displacements_device`.  An image that is stored nowhere is no array (``u = x``)."""
        idx, origin = self._frame_index(idx), self._frame_index(origin)
        snaps, arrays = [self[origin], self[idx]], []
        for at, snap in zip((origin, idx), snaps):
            a = _particle_arrays(snap.particles)
            if self._effective_frame(at, 'particles/image', int(snap.particles.N)) is None:
                a.pop('image', None)
            arrays.append(a)
        if int(snaps[0].particles.N) != int(snaps[1].particles.N):
            raise ValueError("the frames differ in their number of particles (%d and %d)"
                             % (snaps[0].particles.N, snaps[1].particles.N))
        boxes = (snaps[0].configuration.box, snaps[1].configuration.box)
        dims = int(snaps[1].configuration.dimensions)
        types = snaps[1].particles.types
        got = frame_displacements(arrays[0], arrays[1], by_type=by_type, images=images, minimum_image=minimum_image,
                                  where=where, types=types, domain=domain, box=boxes, dimensions=dims)
        if not return_rows:
            return got
        rows = None
        if where is not None:
            rows = where_rows(arrays[1], where, types)
        if domain is not None:
            inside = domain_rows(arrays[1]['position'], boxes[1], domain, dims)
            rows = inside if rows is None else numpy.intersect1d(rows, inside)
        d = displacement_vectors(arrays[0]['position'], arrays[1]['position'], arrays[0].get('image') if images else None,
                                 arrays[1].get('image') if images else None, box_vectors(boxes[0]), box_vectors(boxes[1]),
                                 minimum_image, dims, rows)
        return got, d

    def frame_displacements_device(self, idx, origin=0, by_type=True, images=True, minimum_image=False, where=None,
                                   domain=None, return_rows=False):
        """`frame_displacements` from frame ``origin`` to frame ``idx``, reduced on the GPU: a `Displacements` that
        equals ``frame_displacements(idx, origin, ...)`` exactly, the sums bit for bit.

        The selection is `frame_moments_device`'s own, on frame ``idx``; the types are frame ``idx``'s.  The effective
        chunks (each frame's own, else frame 0's) of both positions, with ``images`` of both images and with
        ``by_type`` of the typeid are staged into HBM -- a chunk the selection staged is not read again, and a chunk
        both frames read from frame 0 is staged once -- and reduced there in one pass
        (`pgsd.fl.PGSDFile.frame_displacements_device`); an image that is stored nowhere costs nothing.  More than four
        types take consecutive passes over the same staged chunks; one `wait_read` at the end releases them.  With
        ``return_rows`` the result is ``(displacements, d)``, ``d`` the ``count x 3`` float64 displacements of the
        selection's entries in GPU memory.  A position that neither frame nor frame 0 stores is answered on the host.

        ValueError: frames of different N (before anything is read); what `frame_displacements` refuses.
        """
        idx, origin = self._frame_index(idx), self._frame_index(origin)
        f = self.file
        box, dims, n_global, f_pos = self._census_frame(idx)
        box_o, _, n_origin, f_pos_o = self._census_frame(origin)
        if n_origin != n_global:
            raise ValueError("the frames differ in their number of particles (%d and %d)" % (n_origin, n_global))
        if f_pos is None or f_pos_o is None:
            # a degenerate file: no kernel path for a position that is all defaults
            got = self.frame_displacements(idx, origin, by_type, images, minimum_image, where, domain, return_rows)
            return (got[0], fl._device_from_host(got[1], f.pipeline_device())) if return_rows else got
        types = self._types_of(idx)
        try:
            rows, count, _ = self._selection_row_list(idx, where, domain, box, dims, n_global, f_pos, types)
            chunks = [(f_pos_o, 'particles/position'), None, (f_pos, 'particles/position'), None, None]
            for slot, at, name, wanted in ((1, origin, 'image', images), (3, idx, 'image', images), (4, idx, 'typeid', by_type)):
                fr = self._effective_frame(at, 'particles/' + name, n_global) if wanted else None
                chunks[slot] = None if fr is None else (fr, 'particles/' + name)
            if minimum_image and (chunks[1] is not None or chunks[3] is not None):
                raise ValueError("the minimum image is taken without image flags: pass no image array")
            out = result = None
            if return_rows:
                out = fl._device_empty((max(count, 1), 3), numpy.float64, f.pipeline_device())
                result = out if count > 0 else (out.view(shape=(0, 3)) if isinstance(out, fl.DeviceBuffer) else out[:0])
            common = dict(vectors_a=box_vectors(box_o), vectors_b=box_vectors(box), minimum_image=minimum_image,
                          dimensions=dims, rows=rows, n=None if rows is None else count)
            if by_type and len(types) == 0 and out is not None:
                f.frame_displacements_device(chunks[:4] + [None], out=out, **common)

            def nothing(k):
                values = numpy.zeros((k, _DISPLACEMENT_VALUES))
                values[:, 4] = -numpy.inf
                return Displacements.from_sums([0] * k, [0] * k, [-1] * k, 0, values)

            got = self._grouped_by_type(
                lambda t0, n_types: f.frame_displacements_device(chunks, type0=t0, n_types=n_types,
                                                                 out=out if t0 == 0 else None, **common),
                Displacements, nothing, _DISPLACEMENT_MAX_TYPES, len(types), by_type, chunks[4] is not None, count)
            return (got, result) if return_rows else got
        finally:
            f.wait_read()

    def _frame_of(self, idx, chunk):
        """The frame whose copy of a chunk that is NOT per-particle (box, N, types, log/*) frame ``idx`` reads: its
        own, else frame 0's, else ``None``."""
        f = self.file
        if f.chunk_exists(idx, chunk):
            return idx
        if f.chunk_exists(0, chunk):
            return 0
        return None

    def _effective_frame(self, idx, chunk, n_global):
        """The frame whose copy of a per-particle chunk frame ``idx`` (of ``n_global`` particles) reads: its own, else
        frame 0's while N is frame 0's, else ``None`` (the default value) -- the host reader's choice."""
        f = self.file
        if f.chunk_exists(idx, chunk):
            return idx
        if not f.chunk_exists(0, chunk):
            return None
        n_frame0 = int(self._frame0_small('particles/N')[0]) if f.chunk_exists(0, 'particles/N') else n_global
        return 0 if n_frame0 == n_global else None

    def _default_rows_template(self, device):
        """All default rows of the SPH schema as ONE int32 device array (every element type of the schema is four
        bytes wide), built once per trajectory and device; `_default_rows_layout[name]` = (first word, words, numpy
        dtype).  `_read_particles_device` clones it per read and hands out views of the clone."""
        cached = getattr(self, '_default_rows_cache', None)
        if cached is not None and cached[0] == device:
            return cached[1]
        words, layout = [], {}
        for name, (dt, M, default, upstream) in _PARTICLE_FIELDS.items():
            if not upstream:
                layout[name] = (len(words), M, numpy.dtype(dt))
                words += numpy.ascontiguousarray(numpy.broadcast_to(default, (M,))).view(numpy.int32).tolist()
        template = fl._device_from_host(numpy.array(words, dtype=numpy.int32), device)
        self._default_rows_layout = layout
        self._default_rows_cache = (device, template)
        return template

    def _frame0_small(self, chunk):
        """A small replicated chunk of frame 0 (box, counts, types ...), read once: frame 0 never changes, and a
        trajectory whose later frames fall back on it asked the file for it again for every frame read."""
        value = self._frame0_small_cache.get(chunk)
        if value is None:
            value = self.file.read_chunk(0, chunk)
            value.flags.writeable = False
            self._frame0_small_cache[chunk] = value
        return value

    def _read_scalar_any(self, idx, chunk, container, attr):
        f = self.file
        if f.chunk_exists(idx, chunk):
            setattr(container, attr, f.read_chunk(idx, chunk)[0])
        elif f.chunk_exists(0, chunk):
            setattr(container, attr, self._frame0_small(chunk)[0])
        else:
            setattr(container, attr, container._default_value[attr])

    def __getitem__(self, key):
        """``trajectory[i]`` reads one frame (negative ``i`` counts from the end), ``trajectory[a:b:c]``
        returns a lazy subset."""
        n = len(self)
        if isinstance(key, slice):
            return _FrameSubset(self, range(*key.indices(n)))
        if not isinstance(key, (int, numpy.integer)):
            raise TypeError
        idx = int(key)
        if idx < 0:
            idx += n
        if not 0 <= idx < n:
            raise IndexError()
        return self._read_frame(idx)

    def __iter__(self):
        return _FrameCursor(self, range(len(self)))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.file.close()


def open(name, mode='r'):
    """Open a hoomd schema PGSD file (hoomd.py:943-989).

    Valid modes: ``'r'``, ``'r+'``, ``'w'``, ``'x'``, ``'a'``.  Returns a `HOOMDTrajectory`.
    """
    if fl is None:
        raise RuntimeError("file layer module is not available")
    pgsdfileobj = fl.open(name=str(name), mode=mode, application='pgsd.hoomd ' + _pgsd_version,
                          schema='hoomd', schema_version=[1, 4])
    return HOOMDTrajectory(pgsdfileobj)


def read_log(name, scalar_only=False):
    """Read ``configuration/step`` and every ``log/*`` quantity into a dict of time-series arrays
    (hoomd.py:992-1075).  Quantities must keep their shape over the frames."""
    if fl is None:
        raise RuntimeError("file layer module is not available")
    with fl.open(name=str(name), mode='r', application='pgsd.hoomd ' + _pgsd_version, schema='hoomd',
                 schema_version=[1, 4]) as f:
        names = f.find_matching_chunk_names('log/')
        names.insert(0, 'configuration/step')
        if len(names) == 1:
            warnings.warn('No logged data in file: ' + str(name), RuntimeWarning)
        out = dict()
        nframes = f.nframes
        for log in names:
            exists0 = f.chunk_exists(frame=0, name=log, write_all=False)
            is_step = log == 'configuration/step'
            if exists0 or is_step:
                if is_step and not exists0:
                    tmp = numpy.array([0], dtype=numpy.uint64)
                else:
                    tmp = f.read_chunk(frame=0, name=log)
                if scalar_only and not tmp.shape[0] == 1:
                    continue
                if tmp.shape[0] == 1:
                    out[log] = numpy.full(fill_value=tmp[0], shape=(nframes,))
                else:
                    out[log] = numpy.tile(tmp, (nframes,) + tuple(1 for _ in tmp.shape))
        for idx in range(1, nframes):
            for log in out.keys():
                if not f.chunk_exists(frame=idx, name=log, write_all=False):
                    continue
                data = f.read_chunk(frame=idx, name=log)
                if len(out[log][idx].shape) == 0:
                    out[log][idx] = data[0]
                else:
                    out[log][idx] = data
    return out
