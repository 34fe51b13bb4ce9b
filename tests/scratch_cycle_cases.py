"""What the scratch life-cycle tests of the pair, cell and SPH passes share: the contents of one small file, the bytes every
family's launcher asks its `Scratch` for (restated from the layout comment above each `Scratch` definition and the
`LaunchScope` argument in csrc/), the steps of every sequence as data, and the host model of a step.
`test_scratch_cycle_cases.py` holds the sizes and the inputs against what the sequences need, without a GPU;
`test_gpu_scratch_cycle.py` runs the sequences, each in a fresh process.

The sizes are the smallest that can go wrong.  7 entries lie far below the 64 KiB floor in every family.  6001 float32
entries put the compacted positions alone (12 bytes per entry) past the floor in every pair family, the four n-word lists
in the component fields, and the cell fields pass it through a (10, 10, 10) table of 80 bytes per cell.  4097 entries on a
grid of no more cells lie inside the grown space with every part at another offset, and cross a tile of 4096 and a block
of 256 by one entry."""
import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import TRICLINIC, random_rows

BOX = TRICLINIC
HEIGHTS = (7, 4097, 6001)
TINY, MID, BIG = HEIGHTS
DTYPES = {'f32': np.float32, 'f64': np.float64}
R = 0.8                             # the range of the census and the lists; the support 2h of every SPH family
H = 0.4
R_LINK = 0.45                       # the linking length: one large component, some hundred small ones
FINE = (11, 9, 7)                   # neighbour_grid_for(BOX, R): the finest grid R allows
COARSE = (6, 5, 3)
CLUMP = 1100                        # rows 2000 .. 3099 of the two larger heights, inside one cell of every grid used
CLUMP_AT = np.array([0.336, 0.312, 0.18])      # fractions (0.53, 0.53, 0.53) of the box
VOID_AT = np.array([-2.0, -1.0, -1.5])         # no row within 1.0 of it: a probe point without a neighbour
POINTS = 300
FLOOR, FACTOR = 1 << 16, 1.25
KERNELS = hoomd.SPH_KERNELS
FAMILIES = ('cells', 'census', 'list', 'components', 'component_fields', 'sums', 'adaptive', 'gradients', 'tensors',
            'forces', 'body', 'samples')


# ---------------------------------------------------------------- the file
def positions(n):
    """n rows of the box as float64: uniform, none within 1.0 of VOID_AT, the clump, and a few rows that are nowhere."""
    p = random_rows(100 + n, n, BOX, np.float64)
    near = np.linalg.norm(p - VOID_AT, axis=1) < 1.0
    p[near, 0] += 2.5
    if n >= 2000 + CLUMP:
        p[2000:2000 + CLUMP] = CLUMP_AT + np.random.default_rng(n).uniform(-0.04, 0.04, size=(CLUMP, 3))
    p[5::97, 0] = np.nan            # (as sph_cases._with_lost_rows)
    p[11::97, 1] = np.inf
    return p


def arrays():
    """name -> array of everything the file holds: per height and element type the position ``x`` and the columns ``m``
    (mass), ``rho`` (density), ``v`` (velocity), ``e`` (energy), ``p`` (pressure), ``s`` (slength); per height ``tid``
    (typeid: 1 is the body, 0 the fluid); the probe points ``points``."""
    out = {}
    for n in HEIGHTS:
        rng = np.random.default_rng(7000 + n)
        x = positions(n)
        rho = 1000.0 + 50.0 * rng.standard_normal(n)
        columns = dict(x=x, m=rng.uniform(0.5, 2.0, size=n), rho=rho, v=rng.standard_normal((n, 3)),
                       e=rng.uniform(-1.0, 3.0, size=n) * 2.0 ** rng.integers(-4, 5, size=n),
                       p=1500.0 * (rho - 1000.0) + rng.standard_normal(n), s=rng.uniform(0.3, H, size=n))
        for key, dt in DTYPES.items():
            for c, a in columns.items():
                out['%s%d_%s' % (c, n, key)] = np.ascontiguousarray(a.astype(dt))
        out['tid%d' % n] = (np.arange(n) % 5 == 0).astype(np.uint32)
    points = random_rows(55, POINTS, BOX, np.float64)
    points[0], points[1], points[2] = VOID_AT, CLUMP_AT, np.nan
    out['points'] = points
    return out


def write_file(f, A):
    """Every array through the host path of an open `pgsd.fl` file, one frame."""
    for name, a in A.items():
        if name != 'points':
            f.write_chunk(name, a.reshape(len(a), -1))
    f.end_frame()


def col(A, c, step):
    return A['%s%d_%s' % (c, step['n'], step['key'])]


def name(c, step):
    return '%s%d_%s' % (c, step['n'], step['key'])


def body_fluid(A, n):
    tid = A['tid%d' % n]
    return np.flatnonzero(tid == 1), np.flatnonzero(tid == 0)


# ---------------------------------------------------------------- the bytes a call needs
def round16(b):
    return (b + 15) & ~15


def _blocks(n, per=256):
    return (n + per - 1) // per


def _pair_head(n, key, n_cells):
    """What every pair family begins with: the device flag word (16), the offsets (n_cells + 2 words), the compacted
    positions (n x 3 elements)."""
    return 16 + round16((n_cells + 2) * 4) + round16(n * 3 * (8 if key == 'f64' else 4))


def _col(n):
    return round16(n * 8)               # one double per entry


def n_cells_of(grid):
    return grid[0] * grid[1] * grid[2]


def need(family, n, key, grid, opts=None, components=1, n_body=0):
    """The bytes the launcher of ``family`` hands its LaunchScope for a list of ``n`` entries of a ``key`` position chunk
    on ``grid`` (the largest of the layouts where a step makes more than one call on the space)."""
    o = opts or {}
    C, nb = n_cells_of(grid), _blocks(n)
    head = _pair_head(n, key, C)
    if family == 'cells':
        # pgsd_cells.hip: CELLS_PIECE 1024 entries per slab; first[]: a word per slab; the table: CELLS_Q 9 doubles and a
        # 64-bit counter per cell; the partials: two slots of CELLS_SLOT_WORDS 10 words per slab.  (cell offsets: 16)
        slabs = _blocks(n, 1024)
        return 16 + round16((C + 2) * 4) + round16(slabs * 4) + C * 9 * 8 + C * 8 + slabs * 2 * 10 * 8
    if family == 'census':
        # pgsd_neighbours.hip: sizeof(NeighboursPartial) 24 per workgroup; bins + 1 edges; the summary of
        # NEIGHBOURS_HEAD_WORDS 8 + NEIGHBOURS_COUNT_BINS 257 + bins words and closest2 behind it
        bins = o.get('bins', 0)
        return head + round16(nb * 24) + round16((bins + 1) * 8) + (8 + 257 + bins + 1) * 8
    if family == 'list':
        # pgsd_neighbour_list.hip, the count pass: n counts, sums and bases (64 bits) and the longest (32 bits) per
        # workgroup, NLIST_SUMMARY_WORDS 4; the fill pass takes head + 8 (the mismatch word), which is less
        return head + round16(n * 4) + 2 * round16(nb * 8) + round16(nb * 4) + 4 * 8
    if family == 'components':
        # pgsd_components.hip: size_at (n words), root counts and bases per workgroup, COMP_WORDS 8
        return head + round16(n * 4) + 2 * round16(nb * 8) + 8 * 8
    if family == 'component_fields':
        # pgsd_component_moments.hip: CMOM_WORK_BYTES 48; four n-word lists; the digit table of SORT_RADIX 256 words per
        # SORT_TILE 4096 entries and 256 totals; components + 1 offsets; first[] per slab of 1024; two slots of
        # CMOM_SLOT_WORDS 16 words per slab
        slabs = _blocks(n, 1024)
        return (16 + 48 + 4 * round16(n * 4) + round16(256 * _blocks(n, 4096) * 4) + 256 * 4 + round16((components + 1) * 4)
                + round16(slabs * 4) + slabs * 2 * 16 * 8)
    if family == 'sums':
        # pgsd_sph.hip: masses and volumes; sizeof(SphPartial) 64; SPH_SUMMARY_WORDS 13
        return head + 2 * _col(n) + round16(nb * 64) + 13 * 8
    if family == 'adaptive':
        # pgsd_sph_adaptive.hip: masses, volumes, smoothing lengths; sizeof(SphaPartial) 104; SPHA_SUMMARY_WORDS 22.  (the
        # range call: 16 + sizeof(SphaRange) 24 per workgroup, at most SPHA_RANGE_BLOCKS 1024, + 4 words: less)
        return head + 3 * _col(n) + round16(nb * 104) + 22 * 8
    if family == 'gradients':
        # pgsd_sph_gradients.hip: masses, volumes, velocities (3 doubles); sizeof(SphgPartial) 56; SPHG_SUMMARY_WORDS 13
        return head + 2 * _col(n) + round16(n * 24) + round16(nb * 56) + 13 * 8
    if family == 'tensors':
        # pgsd_sph_tensors.hip: as the gradients; sizeof(SphtPartial) 56; SPHT_SUMMARY_WORDS 14
        return head + 2 * _col(n) + round16(n * 24) + round16(nb * 56) + 14 * 8
    if family == 'forces':
        # pgsd_sph_forces.hip: masses, A values, volumes, densities, velocities; sizeof(SphfPartial) 40; SPHF_SUMMARY_WORDS 12
        return head + 4 * _col(n) + round16(n * 24) + round16(nb * 40) + 12 * 8
    if family == 'body':
        # pgsd_sph_body.hip: two offset tables; per list positions, four columns and velocities; the table of 12 (viscous)
        # or 6 doubles per target; the sums per SPHB_TILE 4096 targets; sizeof(BodyPartial) 16; SPHB_SUMMARY_WORDS 22
        E, W, n_fluid = (8 if key == 'f64' else 4), (12 if o.get('viscosity') is not None else 6), n - n_body
        lists = sum(round16(k * 3 * E) + 4 * _col(k) + round16(k * 24) for k in (n_body, n_fluid))
        return (16 + 2 * round16((C + 2) * 4) + lists + round16(n_body * W * 8) + round16(_blocks(n_body, 4096) * W * 8)
                + round16(_blocks(n_body) * 16) + 22 * 8)
    if family == 'samples':
        # pgsd_sph_samples.hip: masses, volumes, the value table of samp_padded(C) in {0, 1, 4, 8} doubles per entry;
        # sizeof(SampPartial) 40 per workgroup of points; SPHS_SUMMARY_WORDS 11
        width = 3 * len(o.get('values', ()))
        padded = 0 if width == 0 else (1 if width == 1 else (4 if width <= 4 else 8))
        return head + 2 * _col(n) + round16(n * padded * 8) + round16(_blocks(POINTS) * 40) + 11 * 8
    raise KeyError(family)


def capacity(bytes_needed):
    """What a `Scratch` allocates for a need beyond what it holds (pgsd_scratch.cpp)."""
    return max(int(bytes_needed * FACTOR), FLOOR)


# ---------------------------------------------------------------- the sequences
def _steps(family, tiny, big, mid, wide, again, grids=((2, 2, 2), FINE, COARSE, FINE, (3, 3, 3))):
    """tiny float64, big float32 (growth), mid float32 on another grid with the options flipped (reuse at other
    offsets), 4097 float64 (fits or grows again: FOURTH), tiny float32."""
    shapes = ((TINY, 'f64'), (BIG, 'f32'), (MID, 'f32'), (MID, 'f64'), (TINY, 'f32'))
    return [dict(family=family, n=n, key=key, grid=grid, opts=opts)
            for (n, key), grid, opts in zip(shapes, grids, (tiny, big, mid, wide, again))]


_ALL = dict(mass=True, density=True)
_W, _S = KERNELS
SEQUENCES = {
    # the grid varies (8, 1000, 343, 27, 8 cells), not only the element type; absent: inputs stored nowhere
    'cells': _steps('cells', dict(absent=()), dict(absent=()), dict(absent=('velocity', 'energy')), dict(absent=('mass',)),
                    dict(absent=('position',)), grids=((2, 2, 2), (10, 10, 10), (7, 7, 7), (3, 3, 3), (2, 2, 2))),
    'census': _steps('census', dict(bins=0), dict(bins=64), dict(bins=0), dict(bins=64), dict(bins=64)),
    'list': _steps('list', dict(half=False, distances=True), dict(half=False, distances=True),
                   dict(half=True, distances=False), dict(half=True, distances=True), dict(half=False, distances=False)),
    'components': _steps('components', {}, {}, {}, {}, {}),
    'component_fields': _steps('component_fields', dict(absent=()), dict(absent=()), dict(absent=('velocity', 'energy')),
                               dict(absent=('mass',)), dict(absent=('mass', 'velocity', 'energy'))),
    'sums': _steps('sums', dict(_ALL, kernel=_W), dict(_ALL, kernel=_W), dict(mass=False, density=False, kernel=_S),
                   dict(mass=True, density=False, kernel=_S), dict(mass=False, density=True, kernel=_W)),
    'adaptive': _steps('adaptive', dict(_ALL, kernel=_W, mode='gather'), dict(_ALL, kernel=_W, mode='gather'),
                       dict(mass=False, density=False, kernel=_S, mode='mean'), dict(_ALL, kernel=_S, mode='gather'),
                       dict(mass=True, density=False, kernel=_W, mode='mean')),
    'gradients': _steps('gradients', dict(_ALL, kernel=_W), dict(_ALL, kernel=_W), dict(mass=False, density=False, kernel=_S),
                        dict(mass=False, density=True, kernel=_S), dict(_ALL, kernel=_S)),
    # (the tensors need a density: the mass, the kernel and det_min flip)
    'tensors': _steps('tensors', dict(mass=True, kernel=_W, det_min=0.25), dict(mass=True, kernel=_W, det_min=0.0),
                      dict(mass=False, kernel=_S, det_min=0.25), dict(mass=True, kernel=_S, det_min=0.0),
                      dict(mass=False, kernel=_W, det_min=0.0)),
    'forces': _steps('forces', dict(viscosity=0.001, gravity=(0.0, 0.0, -9.81), kernel=_W), dict(viscosity=0.001, kernel=_W),
                     dict(viscosity=None, kernel=_S), dict(viscosity=0.5, kernel=_S), dict(viscosity=None, kernel=_W)),
    'body': _steps('body', dict(viscosity=0.001, kernel=_W), dict(viscosity=0.001, kernel=_W), dict(viscosity=None, kernel=_S),
                   dict(viscosity=0.5, kernel=_S), dict(viscosity=None, kernel=_W)),
    'samples': _steps('samples', dict(values=('v',), kernel=_W, normalise=False), dict(values=('v',), kernel=_W, normalise=False),
                      dict(values=(), kernel=_S, normalise=False), dict(values=('v',), kernel=_S, normalise=True),
                      dict(values=(), kernel=_W, normalise=True)),
}
# what the fourth step (4097 float64) exercises after the growth of the second: it fits in 1.25 x need(big), or the space
# grows again.  test_scratch_cycle_cases.py holds this against the formulas.
FOURTH = {'cells': 'fits', 'census': 'grows', 'list': 'fits', 'components': 'fits', 'component_fields': 'fits',
          'sums': 'fits', 'adaptive': 'fits', 'gradients': 'fits', 'tensors': 'fits', 'forces': 'fits', 'body': 'fits',
          'samples': 'fits'}


def step_of(family, k):
    return SEQUENCES[family][k]


# one process, all twelve families in turn at mixed sizes, then the first four again at the other sizes; the child puts
# a call of an old family between them
INTERLEAVED = [step_of('census', 1), step_of('sums', 0), step_of('list', 3), step_of('components', 1),
               step_of('component_fields', 1), step_of('cells', 1), step_of('adaptive', 4), step_of('gradients', 2),
               step_of('tensors', 1), step_of('forces', 0), step_of('body', 1), step_of('samples', 2),
               step_of('census', 4), step_of('sums', 1), step_of('list', 0), step_of('components', 2)]


# ---------------------------------------------------------------- the truth of a step
_MODELS = {}


def _given(A, step, c, flag):
    return col(A, c, step) if step['opts'].get(flag, True) else None


def model(A, step):
    """The host model of a step (computed once): the result type of `pgsd.hoomd` the device call must equal; for the
    component fields ``(components, fields)``."""
    tag = (step['family'], step['n'], step['key'], step['grid'], repr(sorted(step['opts'].items())))
    if tag not in _MODELS:
        _MODELS[tag] = _model(A, step)
    return _MODELS[tag]


def _model(A, step):
    family, n, grid, o = step['family'], step['n'], step['grid'], step['opts']
    x = col(A, 'x', step)
    if family in ('cells', 'component_fields'):
        absent = o['absent']
        m, v, e, p = [None if k in absent else col(A, c, step)
                      for k, c in (('mass', 'm'), ('velocity', 'v'), ('energy', 'e'), ('position', 'x'))]
    if family == 'cells':
        rows, cell, _ = hoomd.cell_order(x, BOX, np.arange(n), grid)
        defaults = (1.0, [0.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0])        # the schema's row, where a chunk is stored nowhere
        given = [d if a is None else a for a, d in zip((m, v, e, p), defaults)]
        return hoomd.cell_moments(*given, cell=cell, n_cells=n_cells_of(grid), rows=rows, N=n)
    if family == 'census':
        return hoomd.particle_neighbours(x, BOX, R, cells=grid, bins=o['bins'])
    if family == 'list':
        return hoomd.neighbour_list(x, BOX, R, cells=grid, half=o['half'], distances=True)
    if family == 'components':
        return hoomd.neighbour_components(x, BOX, R_LINK, cells=grid)
    if family == 'component_fields':
        comps = hoomd.neighbour_components(x, BOX, R_LINK, cells=grid)
        return comps, hoomd.component_moments(m, v, e, x, BOX, comps.label, comps.component, rows=comps.rows)
    mass, density = _given(A, step, 'm', 'mass'), _given(A, step, 'rho', 'density')
    if family == 'sums':
        return hoomd.sph_kernel_sums(x, BOX, H, mass=mass, density=density, cells=grid, kernel=o['kernel'])
    if family == 'adaptive':
        return hoomd.sph_adaptive_sums(x, BOX, col(A, 's', step), mass=mass, density=density, cells=grid, kernel=o['kernel'],
                                       mode=o['mode'])
    v = col(A, 'v', step)
    if family == 'gradients':
        return hoomd.sph_kernel_gradients(x, v, BOX, H, mass=mass, density=density, cells=grid, kernel=o['kernel'])
    if family == 'tensors':
        return hoomd.sph_gradient_tensors(x, v, BOX, H, mass=mass, density=density, cells=grid, kernel=o['kernel'],
                                          det_min=o['det_min'])
    if family == 'forces':
        return hoomd.sph_accelerations(x, v, BOX, H, mass=mass, density=density, pressure=col(A, 'p', step),
                                       viscosity=o['viscosity'], gravity=o.get('gravity'), cells=grid, kernel=o['kernel'])
    if family == 'body':
        body, fluid = body_fluid(A, n)
        return hoomd.sph_body_force(x, v, BOX, H, body, fluid, mass=mass, density=density, pressure=col(A, 'p', step),
                                    viscosity=o['viscosity'], cells=grid, kernel=o['kernel'])
    if family == 'samples':
        return hoomd.sph_samples(A['points'], x, BOX, H, values=[col(A, c, step) for c in o['values']], mass=mass,
                                 density=density, cells=grid, kernel=o['kernel'], normalise=o['normalise'])
    raise KeyError(family)


def step_need(A, step):
    """`need` of a step, with the components and the body list its model has."""
    family = step['family']
    components = model(A, step)[0].components if family == 'component_fields' else 1
    n_body = len(body_fluid(A, step['n'])[0]) if family == 'body' else 0
    return need(family, step['n'], step['key'], step['grid'], step['opts'], components, n_body)


# ---------------------------------------------------------------- comparing a result with its model
# the per-entry (per-point, per-component) arrays of every result type; the summary words come on top
RESULT_ARRAYS = {
    'census': ('rows', 'cell', 'count', 'nearest', 'nearest2'),
    'list': ('rows', 'cell', 'offsets', 'neighbours', 'distance2'),
    'components': ('rows', 'cell', 'label', 'component', 'sizes'),
    'sums': ('rows', 'cell', 'number', 'density', 'shepard'),
    'adaptive': ('rows', 'cell', 'count', 'number', 'density', 'shepard', 'omega'),
    'gradients': ('rows', 'cell', 'density_rate', 'divergence', 'curl', 'normal'),
    'tensors': ('rows', 'cell', 'correction', 'determinant', 'velocity_gradient', 'shear_rate'),
    'forces': ('rows', 'cell', 'pressure_acc', 'viscous_acc', 'total'),
    'body': ('rows', 'cell', 'contacts', 'pressure_acc', 'viscous_acc'),
    'samples': ('count', 'density', 'shepard', 'values'),
}
CELL_FIELDS = ('count', 'bad', 'mass', 'momentum', 'kinetic', 'internal', 'first_moment')


def words_differ(got, want):
    """Two summaries as 64-bit words: the same bits, or a NaN in both where the word is a float."""
    g, w = np.asarray(got, np.uint64).ravel(), np.asarray(want, np.uint64).ravel()
    if g.shape != w.shape:
        return True
    gf, wf = g.view(np.float64), w.view(np.float64)
    return bool(((g != w) & ~((gf != gf) & (wf != wf))).any())


def arrays_differ(got, want):
    """Two arrays of one result attribute, the kernel's copied to the host: integers by value (a 32-bit array of the other
    signedness viewed as the model's), floats as float64 bit for bit, a NaN equal to a NaN."""
    if got is None or want is None:
        return (got is None) != (want is None)
    g, w = np.asarray(got), np.asarray(want)
    if g.shape != w.shape:
        return True
    if w.dtype.kind == 'f':
        if g.dtype != np.float64 or w.dtype != np.float64:
            return True
        return words_differ(g.view(np.uint64), w.view(np.uint64))
    if g.dtype.kind == 'f':
        return True
    if g.dtype != w.dtype and g.dtype.itemsize == w.dtype.itemsize:
        g = g.view(w.dtype)
    return not np.array_equal(g, w)
