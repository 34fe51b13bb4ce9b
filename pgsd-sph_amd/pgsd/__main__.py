"""Command line of the package: ``python -m pgsd <command>``.

``read``   the reference's one command (``__main__.py:52-87``): an interactive Python prompt with
           the file open as ``handle`` and, for the hoomd schema, the trajectory as ``traj``.
``info``   header, frame count and the chunks of one frame, printed and done (no prompt); ``--balance NX,NY,NZ``
           adds the split lists that balance the frame's particles over such a decomposition and the per-cell counts
           of the equal and of the balanced grid (the host models of ``pgsd.hoomd``: no GPU); ``--stats`` adds per
           field and column the count, the NaN and infinite entries, minimum, maximum and mean of one frame, and the
           largest norm of three-column float fields (``--fields``, ``--types``); ``--stats --all-frames`` prints one
           line per frame with the number of non-finite entries and the largest speed: the blow-up scan;
           ``--moments`` adds per particle type the count, mass, momentum, kinetic and internal energy and centre of
           mass of one frame and a total line (``--types``), ``--moments --all-frames`` one line per frame with the
           totals: the conservation table (``pgsd.hoomd.frame_moments`` on the host: no GPU);
           ``--displacement`` adds per particle type the count, mean drift, mean-squared displacement and the largest
           move with its row between frame ``--origin`` and the frame, unwrapped through the image flags
           (``--minimum-image``: the wrapped positions' difference folded into the box instead; ``--types``), and a
           total line; ``--displacement --all-frames`` one line per frame against the origin: the MSD curve
           (``pgsd.hoomd.frame_displacements`` on the host: no GPU);
           ``--cells CX,CY,CZ`` adds the occupied cells of such a grid, the smallest and largest count, the largest
           density and mean speed with their cell indices and the particles nowhere (``--types``;
           ``pgsd.hoomd.frame_cell_moments`` on the host: no GPU);
           ``--neighbours R`` adds the neighbour census inside the range R: the search grid, the entries and those
           nowhere, the mean, smallest and largest neighbour count, the isolated entries and the closest pair with its
           rows and distance, and with ``--bins B`` the g(r) table (``--types``; ``pgsd.hoomd.frame_neighbours`` on the
           host: no GPU);
           ``--neighbour-list R`` adds what a neighbour list inside the range R would hold: the search grid, the entries
           and those nowhere, the pairs, the longest segment and the bytes the list occupies, ``8 (n + 1) + 4 pairs`` and
           ``8 pairs`` more with distances -- what a restart budgets in HBM before it asks (``--half``: each pair once;
           ``--types``; ``pgsd.hoomd.frame_neighbour_list`` on the host: no GPU);
           ``--components R`` adds the connected components with the linking length R -- the pieces the fluid has broken
           into: their number, the singletons, the largest with its label and row, the entries nowhere, and with
           ``--min-size K`` how many components have at least K entries and the share of the entries they hold
           (``--types``; ``pgsd.hoomd.frame_components`` on the host: no GPU), and with ``--pieces [K]`` what the K
           heaviest pieces (default 10) are: size, mass, centre of mass, mean velocity, span and whether the piece is
           ``wide`` -- its extent reaches half a box length, so it percolates or nearly does and its centre and span are
           not meaningful --, then the number of wide pieces and of entries with a value that is not finite
           (``pgsd.hoomd.frame_component_moments`` on the host: no GPU);
           ``--sph [H]`` adds the SPH kernel sums for the smoothing length H (without H: the frame's ``slength``, which
           must be uniform): the search grid and the entries, the range of the summation density, its largest deviation
           from the stored density with the row, the range of the Shepard sum and -- with ``--surface S`` -- the entries
           whose Shepard sum is below S (``--kernel wendland_c2|cubic_spline``, ``--types``;
           ``pgsd.hoomd.frame_kernel_sums`` on the host: no GPU);
           ``--sph-gradients [H]`` adds the SPH kernel gradients for the smoothing length H (without H: the frame's
           uniform ``slength``): the search grid and the entries, the ranges of the velocity divergence and of the
           density rate of the continuity equation and the largest vorticity and surface normal, each with its row
           (``--kernel``, ``--types``; ``pgsd.hoomd.frame_kernel_gradients`` on the host: no GPU);
           ``--sph-adaptive`` adds the SPH sums with the frame's per-particle ``slength`` (``--mode gather|mean``): the
           search grid for ``2 h_max``, the range of the smoothing length and the entries without a valid one, the range
           of the neighbour count and the pairs, the range of the summation density and its largest deviation from the
           stored density and, in gather mode, the range of the grad-h factor ``omega`` (``--kernel``, ``--surface``,
           ``--types``; ``pgsd.hoomd.frame_adaptive_sums`` on the host: no GPU);
           ``--sph-tensors [H]`` adds the SPH gradient tensors for the smoothing length H (without H: the frame's uniform
           ``slength``): the search grid and the entries, those left uncorrected because the determinant of their
           correction matrix is not above ``--det-min D`` (default 0.25), the ranges of the determinant and of the trace
           of the corrected velocity gradient and the largest shear rate with its row (``--kernel``, ``--types``;
           ``pgsd.hoomd.frame_gradient_tensors`` on the host: no GPU);
           ``--sph-forces [H]`` adds the SPH accelerations for the smoothing length H (without H: the frame's uniform
           ``slength``): the search grid and the entries, the largest total, pressure and viscous acceleration, each with
           its row, the entries whose total is not finite and the force time step ``0.25 sqrt(h / |a|)``
           (``--viscosity MU``, ``--gravity GX,GY,GZ``, ``--kernel``, ``--types``; ``pgsd.hoomd.frame_accelerations`` on the
           host: no GPU);
           ``--sample NX,NY,NZ [H]`` adds the SPH interpolant on an NX x NY x NZ lattice of cell-centre points over the box
           (``pgsd.hoomd.sample_grid``) for the smoothing length H (without H: the frame's uniform ``slength``): the search
           grid, the points nowhere, outside, empty and not finite, the largest count, the ranges of the density and of
           the Shepard sum and per sampled column the smallest and largest value (``--fields a,b``: the per-particle
           fields sampled, default velocity; ``--normalise``: values divided by the Shepard sum; ``--kernel``,
           ``--types``; ``pgsd.hoomd.frame_samples`` on the host: no GPU);
           ``--body-force TYPE[,TYPE...] --fluid TYPE[,TYPE...] [H]`` adds the force and the torque the particles of the
           ``--fluid`` types exert on those of the ``--body-force`` types for the smoothing length H (without H: the
           frame's uniform ``slength``): the search grid, the counters, the pressure and the viscous force and torque and
           their sums and the largest pressure force on one particle with its row (``--viscosity MU``, ``--about X,Y,Z``:
           the point the torque is taken about, ``--kernel``; ``pgsd.hoomd.frame_body_force`` on the host: no GPU).
``vtu``    every frame as a VTK ``.vtu`` file plus a ``.pvd`` collection (``pgsd.vtu``); ``--types`` keeps the
           particles of the named types only.
"""
import argparse
import code
import sys

from .version import __version__

_MODES = ['rb', 'rb+', 'wb', 'wb+', 'xb', 'xb+', 'ab', 'w', 'r', 'r+', 'x', 'a']

_BANNER = """Python {python}
pgsd {version}

File: {name}
{extras}
Variables: "handle" is the open pgsd.fl.PGSDFile; with the hoomd schema "traj" is the
pgsd.hoomd.HOOMDTrajectory on top of it. The modules pgsd, pgsd.fl and pgsd.hoomd are imported.
help(handle) and help(traj) describe them."""


def _cmd_read(args):
    import pgsd
    from . import fl, hoomd
    ns = {'pgsd': pgsd, 'pgsd.fl': fl, 'pgsd.hoomd': hoomd}
    extras = []
    if args.schema == 'hoomd':
        traj = hoomd.open(args.file, mode=args.mode)
        ns['traj'] = traj
        ns['handle'] = traj.file
        extras.append("Number of frames: %d" % len(traj))
    else:
        if args.mode not in ('rb', 'rb+', 'ab', 'a', 'r', 'r+'):
            raise ValueError("Unsupported schema for creating a file.")
        ns['handle'] = fl.open(args.file, args.mode)
    code.interact(local=ns, banner=_BANNER.format(python=sys.version, version=__version__, name=args.file,
                                                  extras="\n".join(extras) + "\n"))


def _cmd_info(args):
    from . import fl
    with fl.open(args.file, 'r') as f:
        print("file:            %s" % args.file)
        print("application:     %s" % f.application)
        print("schema:          %s %d.%d" % ((f.schema,) + tuple(f.schema_version)))
        print("pgsd version:    %d.%d" % tuple(f.pgsd_version))
        print("frames:          %d" % f.nframes)
        print("chunk names:     %d" % f.nnames)
        if f.nframes == 0:
            return
        frame = args.frame if args.frame >= 0 else f.nframes + args.frame
        if not 0 <= frame < f.nframes:
            raise ValueError("frame %d is not in the file" % args.frame)
        print("chunks of frame %d:" % frame)
        for name in f.find_matching_chunk_names(''):
            if f.chunk_exists(frame, name):
                data = f.read_chunk(frame, name)
                print("  %-28s %-8s %s" % (name, data.dtype, 'x'.join(str(n) for n in data.shape)))
    if args.balance:
        _print_balance(args, frame)
    if args.stats:
        _print_stats(args, frame)
    if args.moments:
        _print_moments(args, frame)
    if args.displacement:
        _print_displacement(args, frame)
    if args.cells:
        _print_cells(args, frame)
    if args.neighbours is not None:
        _print_neighbours(args, frame)
    if args.neighbour_list is not None:
        _print_neighbour_list(args, frame)
    if args.components is not None:
        _print_components(args, frame)
    if args.sph is not None:
        _print_sph(args, frame)
    if args.sph_gradients is not None:
        _print_sph_gradients(args, frame)
    if args.sph_adaptive:
        _print_sph_adaptive(args, frame)
    if args.sph_tensors is not None:
        _print_sph_tensors(args, frame)
    if args.sph_forces is not None:
        _print_sph_forces(args, frame)
    if args.sample is not None:
        _print_sample(args, frame)
    if args.body_force is not None or args.fluid is not None:
        _print_body_force(args, frame)


def _print_body_force(args, frame):
    """``info --body-force``: `pgsd.hoomd.frame_body_force` of one frame, on the host."""
    from . import hoomd
    if args.body_force is None or args.fluid is None:
        raise ValueError("--body-force TYPE[,TYPE...] and --fluid TYPE[,TYPE...] [H] go together")
    try:
        h = float(args.fluid[1]) if len(args.fluid) > 1 else None
        if len(args.fluid) > 2:
            raise ValueError
    except ValueError:
        raise ValueError("--fluid takes TYPE[,TYPE...] [H]: %r" % ' '.join(args.fluid))
    about = None
    if args.about is not None:
        try:
            about = [float(v) for v in args.about.split(',')]
        except ValueError:
            raise ValueError("--about takes X,Y,Z: %r" % args.about)
    body = {'type': [t for t in args.body_force.split(',') if t]}
    fluid = {'type': [t for t in args.fluid[0].split(',') if t]}
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_body_force(traj[frame], body, fluid, h, kernel=args.kernel, viscosity=args.viscosity, about=about)
    print("SPH body force of frame %d with h = %r (%s) over %d x %d x %d cells (body %s, fluid %s):"
          % ((frame, m.h, m.kernel) + m.grid + (args.body_force, args.fluid[0])))
    print("  targets:      %d  nowhere: %d  wetted: %d  bad: %d" % (m.n, m.nowhere, m.wetted, m.bad))
    print("  sources:      %d  nowhere: %d  pairs: %d" % (m.n_sources, m.sources_nowhere, m.pairs))
    print("  viscosity:    %s  about: %r %r %r" % (("%r" % m.viscosity if m.viscosity is not None else "none",) + m.about))
    for label, v in (('force:', m.force), ('  pressure:', m.force_pressure), ('  viscous:', m.force_viscous),
                     ('torque:', m.torque), ('  pressure:', m.torque_pressure), ('  viscous:', m.torque_viscous)):
        print("  %-13s %r %r %r" % ((label,) + tuple(v)))
    if m.largest2 is not None:
        print("  largest:      %r at row %d (the pressure force on one particle)" % (m.largest2 ** 0.5, m.largest_row))


def _print_sample(args, frame):
    """``info --sample``: `pgsd.hoomd.frame_samples` of one frame on a `sample_grid` lattice, on the host."""
    import numpy
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    try:
        shape = tuple(int(v) for v in args.sample[0].split(','))
        h = float(args.sample[1]) if len(args.sample) > 1 else None
        if len(shape) != 3 or len(args.sample) > 2:
            raise ValueError
    except ValueError:
        raise ValueError("--sample takes NX,NY,NZ [H]: %r" % ' '.join(args.sample))
    fields = tuple(f for f in args.fields.split(',') if f) if args.fields else ('velocity',)
    with hoomd.open(args.file, 'r') as traj:
        fr = traj[frame]
        dims = int(fr.configuration.dimensions)
        points = hoomd.sample_grid(fr.configuration.box, shape, dims)
        m = hoomd.frame_samples(fr, points, fields=fields, h=h, kernel=args.kernel, normalise=args.normalise, where=where)
    print("SPH samples of frame %d with h = %r (%s) on %d x %d x %d points over %d x %d x %d cells%s:"
          % ((frame, m.h, m.kernel) + shape + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  points:       %d  nowhere: %d  outside: %d  empty: %d  not finite: %d"
          % (m.points, m.nowhere, m.outside, m.empty, m.not_finite))
    if m.count_max_at is not None:
        print("  count:        largest %d at point %d" % (m.count_max, m.count_max_at))
        print("  density:      smallest %r  largest %r" % (m.density_min, m.density_max))
        print("  shepard:      smallest %r  largest %r" % (m.shepard_min, m.shepard_max))
        for k, name in enumerate(fields):
            v = m.field(k)
            for c in range(v.shape[1]):
                ok = v[:, c][v[:, c] == v[:, c]]
                print("  %-13s smallest %r  largest %r%s"
                      % ("%s[%d]:" % (name, c), float(ok.min()) if ok.size else None, float(ok.max()) if ok.size else None,
                         "  (normalised)" if m.normalise else ""))


def _print_sph_forces(args, frame):
    """``info --sph-forces``: `pgsd.hoomd.frame_accelerations` of one frame, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    gravity = None
    if args.gravity is not None:
        try:
            gravity = [float(v) for v in args.gravity.split(',')]
        except ValueError:
            raise ValueError("--gravity takes GX,GY,GZ: %r" % args.gravity)
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_accelerations(traj[frame], None if args.sph_forces < 0 else args.sph_forces, kernel=args.kernel,
                                      viscosity=args.viscosity, gravity=gravity, where=where)
    print("SPH accelerations of frame %d with h = %r (%s) over %d x %d x %d cells%s:"
          % ((frame, m.h, m.kernel) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  entries:      %d  nowhere: %d" % (m.n, m.nowhere))
    print("  viscosity:    %s  gravity: %r %r %r" % (("%r" % m.viscosity if m.viscosity is not None else "none",) + m.gravity))
    if m.n > m.nowhere:
        for name, label in (('total', 'total:'), ('pressure', 'pressure:'), ('viscous', 'viscous:')):
            if getattr(m, name + '2') is not None:
                print("  %-13s largest %r at row %d" % (label, getattr(m, name + '2') ** 0.5, getattr(m, name + '_row')))
        print("  not finite:   %d" % m.not_finite)
        if m.total2 is not None:
            print("  time step:    %r (0.25 * sqrt(h / largest total))" % m.force_time_step())


def _print_sph_gradients(args, frame):
    """``info --sph-gradients``: `pgsd.hoomd.frame_kernel_gradients` of one frame, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_kernel_gradients(traj[frame], None if args.sph_gradients < 0 else args.sph_gradients,
                                         kernel=args.kernel, where=where)
    print("SPH gradients of frame %d with h = %r (%s) over %d x %d x %d cells%s:"
          % ((frame, m.h, m.kernel) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  entries:      %d  nowhere: %d" % (m.n, m.nowhere))
    if m.n > m.nowhere:
        if m.volume:
            print("  divergence:   smallest %r  largest %r" % (m.divergence_min, m.divergence_max))
        print("  density rate: smallest %r  largest %r  not finite: %d" % (m.density_rate_min, m.density_rate_max, m.not_finite))
        if m.curl2 is not None:
            print("  vorticity:    largest %r at row %d" % (m.curl2 ** 0.5, m.curl_row))
        if m.normal2 is not None:
            print("  normal:       largest %r at row %d" % (m.normal2 ** 0.5, m.normal_row))


def _print_sph_adaptive(args, frame):
    """``info --sph-adaptive``: `pgsd.hoomd.frame_adaptive_sums` of one frame, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_adaptive_sums(traj[frame], kernel=args.kernel, mode=args.mode, where=where, surface_below=args.surface)
    print("SPH sums of frame %d with the per-particle slength (%s, %s), h_max = %r, over %d x %d x %d cells%s:"
          % ((frame, m.kernel, m.mode, m.h_max) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  entries:      %d  nowhere: %d  bad_h: %d" % (m.n, m.nowhere, m.bad_h))
    if m.count_min is not None:
        print("  slength:      smallest %r  largest %r" % (m.slength_min, m.slength_max))
        print("  count:        smallest %d at entry %d  largest %d  pairs: %d" % (m.count_min, m.count_min_at, m.count_max, m.pairs))
        print("  density:      smallest %r  largest %r  not finite: %d" % (m.density_min, m.density_max, m.not_finite))
        if m.deviation is not None:
            print("  deviation:    %r at row %d" % (m.deviation, m.deviation_row))
        if m.surface is not None:
            print("  surface:      %d below %r" % (m.surface, m.surface_below))
        if m.omega_min is not None:
            print("  omega:        smallest %r  largest %r" % (m.omega_min, m.omega_max))


def _print_sph_tensors(args, frame):
    """``info --sph-tensors``: `pgsd.hoomd.frame_gradient_tensors` of one frame, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_gradient_tensors(traj[frame], None if args.sph_tensors < 0 else args.sph_tensors, kernel=args.kernel,
                                         det_min=args.det_min, where=where)
    print("SPH gradient tensors of frame %d with h = %r (%s), det_min = %r, over %d x %d x %d cells%s:"
          % ((frame, m.h, m.kernel, m.det_min) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  entries:      %d  nowhere: %d  uncorrected: %d" % (m.n, m.nowhere, m.uncorrected))
    if m.n > m.nowhere:
        print("  determinant:  smallest %r  largest %r" % (m.determinant_min, m.determinant_max))
        print("  trace:        smallest %r  largest %r" % (m.trace_min, m.trace_max))
        if m.shear is not None:
            print("  shear rate:   largest %r at row %d  not finite: %d" % (m.shear, m.shear_row, m.not_finite))
        else:
            print("  shear rate:   not finite: %d" % m.not_finite)


def _print_sph(args, frame):
    """``info --sph``: `pgsd.hoomd.frame_kernel_sums` of one frame, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_kernel_sums(traj[frame], None if args.sph < 0 else args.sph, kernel=args.kernel, where=where,
                                    surface_below=args.surface)
    print("SPH sums of frame %d with h = %r (%s) over %d x %d x %d cells%s:"
          % ((frame, m.h, m.kernel) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  entries:      %d  nowhere: %d" % (m.n, m.nowhere))
    if m.n > m.nowhere:
        print("  density:      smallest %r  largest %r  not finite: %d" % (m.density_min, m.density_max, m.not_finite))
        if m.deviation is not None:
            print("  deviation:    %r from the stored density at row %d" % (m.deviation, m.deviation_row))
        if m.volume:
            print("  shepard:      smallest %r  largest %r" % (m.shepard_min, m.shepard_max))
        if m.surface is not None:
            print("  surface:      %d entries below %r" % (m.surface, m.surface_below))


def _print_neighbour_list(args, frame):
    """``info --neighbour-list``: `pgsd.hoomd.frame_neighbour_list` of one frame inside the range R, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_neighbour_list(traj[frame], args.neighbour_list, half=args.half, where=where)
    print("neighbour list of frame %d inside %r over %d x %d x %d cells%s%s:"
          % ((frame, m.r) + m.grid + (" (half)" if m.half else "", " (types %s)" % args.types if args.types else "")))
    print("  entries:      %d  nowhere: %d" % (m.n, m.nowhere))
    print("  pairs:        %d  longest segment: %d" % (m.pairs, m.longest))
    print("  bytes:        %d  with distances: %d"
          % (hoomd.neighbour_list_bytes(m.n, m.pairs), hoomd.neighbour_list_bytes(m.n, m.pairs, True)))


def _print_components(args, frame):
    """``info --components``: `pgsd.hoomd.frame_components` of one frame with the linking length R, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_components(traj[frame], args.components, where=where)
    print("components of frame %d inside %r over %d x %d x %d cells%s:"
          % ((frame, m.r) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  entries:      %d  nowhere: %d" % (m.n, m.nowhere))
    print("  components:   %d  singletons: %d" % (m.components, m.singletons))
    if m.n:
        print("  largest:      %d entries, label %d, row %d" % (m.largest, m.largest_label, int(m.rows[m.largest_label])))
    if args.min_size is not None:
        kept = m.fragments(args.min_size)
        held = int(m.sizes[kept].sum())
        print("  at least %d:   %d components holding %d entries (%.2f %%)"
              % (args.min_size, len(kept), held, 100.0 * held / m.n if m.n else 0.0))
    if args.pieces is not None:
        with hoomd.open(args.file, 'r') as traj:
            p = hoomd.frame_component_moments(traj[frame], args.components, where=where)
        ids = p.heaviest(args.pieces)
        print("  the %d heaviest of %d pieces (centre, mean velocity and span per axis):" % (len(ids), p.components))
        triple = lambda v: "(%s)" % ", ".join("%.6g" % x for x in v)    # noqa: E731
        centre, velocity, span = p.centre_of_mass, p.mean_velocity, p.span
        for c in ids:
            print("    piece %d: %d entries, mass %.6g, centre %s, velocity %s, span %s%s"
                  % (c, int(p.sizes[c]), p.mass[c], triple(centre[c]), triple(velocity[c]), triple(span[c]),
                     "  WIDE" if p.wide[c] else ""))
        print("  wide pieces:  %d  (extent >= half a box length: centre and span are not meaningful)" % p.wide_components)
        print("  bad entries:  %d  (a value that is not finite; left out of the sums)" % p.bad_entries)


def _print_neighbours(args, frame):
    """``info --neighbours``: `pgsd.hoomd.frame_neighbours` of one frame inside the range R, on the host."""
    import numpy
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        snap = traj[frame]
        m = hoomd.frame_neighbours(snap, args.neighbours, bins=args.bins or 0, where=where)
    print("neighbours of frame %d inside %r over %d x %d x %d cells%s:"
          % ((frame, m.r) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  entries:      %d  nowhere: %d" % (m.n, m.nowhere))
    if m.n > m.nowhere:
        print("  count:        mean %r  smallest %d  largest %d" % (m.mean_count, m.count_min, m.count_max))
        print("  isolated:     %d" % m.isolated)
    if m.closest_rows is not None:
        print("  closest pair: rows %d and %d at distance %r" % (m.closest_rows + (m.closest_distance,)))
    if m.bins:
        b = numpy.asarray(snap.configuration.box, dtype=numpy.float64)
        mid, g = m.rdf(b[0] * b[1] * (b[2] if m.dimensions == 3 else 1.0))
        print("  g(r):")
        for k in range(m.bins):
            print("    %-12.6g %-12.6g %d" % (mid[k], g[k], m.pair_hist[k]))

def _print_cells(args, frame):
    """``info --cells``: `pgsd.hoomd.frame_cell_moments` of one frame over a CX x CY x CZ grid, on the host."""
    import numpy
    from . import hoomd
    try:
        cells = tuple(int(v) for v in args.cells.split(','))
        if len(cells) != 3:
            raise ValueError
    except ValueError:
        raise ValueError("--cells takes CX,CY,CZ: %r" % args.cells)
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        m = hoomd.frame_cell_moments(traj[frame], cells, where=where)
    cx, cy = m.grid[0], m.grid[1]

    def index(c):
        return "(%d, %d, %d)" % (c % cx, (c // cx) % cy, c // (cx * cy))

    occupied = numpy.nonzero(m.count > 0)[0]
    print("cell fields of frame %d over %d x %d x %d cells%s:" % ((frame,) + m.grid + (" (types %s)" % args.types if args.types else "",)))
    print("  occupied cells:  %d of %d" % (len(occupied), len(m.count)))
    if len(occupied):
        print("  count:           smallest %d  largest %d" % (m.count[occupied].min(), m.count[occupied].max()))
        c = int(numpy.argmax(m.density))
        print("  largest density: %r in cell %s" % (float(m.density[c]), index(c)))
        v = m.mean_velocity
        speed = numpy.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        if numpy.isfinite(speed).any():
            c = int(numpy.nanargmax(speed))
            print("  largest speed:   %r in cell %s" % (float(speed[c]), index(c)))
    if m.bad.sum():
        print("  entries with a value that is not finite: %d" % int(m.bad.sum()))
    print("  nowhere:         %d" % m.nowhere)


def _vector_text(v):
    return '(' + ', '.join(repr(float(c)) for c in v) + ')'


def _displacement_text(part, k):
    return ("count %d  bad %d  mean drift %s  msd %r  largest distance %r  row %d"
            % (part.count[k], part.bad[k], _vector_text(part.mean_drift[k]), float(part.msd[k]),
               float(part.largest_distance[k]), part.largest_entry[k]))


def _print_displacement(args, frame):
    """``info --displacement``: `pgsd.hoomd.frame_displacements` between the origin and one frame per type, or the
    totals of every frame against the origin in one line each, on the host.  With ``--types`` the row of the largest
    move is a position in the selection's ascending row list."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    options = dict(where=where, minimum_image=args.minimum_image, images=not args.minimum_image)
    with hoomd.open(args.file, 'r') as traj:
        origin = args.origin if args.origin >= 0 else len(traj) + args.origin
        if not 0 <= origin < len(traj):
            raise ValueError("frame %d is not in the file" % args.origin)
        note = "%s%s" % (" (types %s)" % args.types if args.types else "", " (minimum image)" if args.minimum_image else "")
        if args.all_frames:
            print("displacements per frame against frame %d%s:" % (origin, note))
            for i in range(len(traj)):
                step = int(traj[i].configuration.step)
                t = traj.frame_displacements(i, origin, **options).total()
                print("  frame %-6d step %-10d %s" % (i, step, _displacement_text(t, 0)))
            return
        m = traj.frame_displacements(frame, origin, **options)
        names = list(traj[frame].particles.types)
    print("displacements of frame %d against frame %d%s:" % (frame, origin, note))
    total = m.total()
    for name, part, k in [(names[k], m, k) for k in range(len(names))] + [('total', total, 0)]:
        print("  %-12s %s" % (name, _displacement_text(part, k)))
    if m.other:
        print("  %d particles of no listed type" % m.other)


def _print_moments(args, frame):
    """``info --moments``: `pgsd.hoomd.frame_moments` of one frame per type, or the totals of every frame in one line
    each, on the host."""
    from . import hoomd
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        if args.all_frames:
            print("conservation sums per frame%s:" % (" (types %s)" % args.types if args.types else ""))
            for i in range(len(traj)):
                snap = traj[i]
                t = hoomd.frame_moments(snap, where=where).total()
                print("  frame %-6d step %-10d count %-8d bad %-6d mass %r  momentum %s  kinetic %r  internal %r"
                      % (i, int(snap.configuration.step), t.count[0], t.bad[0], float(t.mass[0]),
                         _vector_text(t.momentum[0]), float(t.kinetic[0]), float(t.internal[0])))
            return
        snap = traj[frame]
        m = hoomd.frame_moments(snap, where=where)
        names = list(snap.particles.types)
    print("conservation sums of frame %d%s:" % (frame, " (types %s)" % args.types if args.types else ""))
    total = m.total()
    for name, part, k in [(names[k], m, k) for k in range(len(names))] + [('total', total, 0)]:
        print("  %-12s count %d  bad %d  mass %r  momentum %s  kinetic %r  internal %r  centre of mass %s"
              % (name, part.count[k], part.bad[k], float(part.mass[k]), _vector_text(part.momentum[k]),
                 float(part.kinetic[k]), float(part.internal[k]), _vector_text(part.centre_of_mass[k])))
    if m.other:
        print("  %d particles of no listed type" % m.other)


def _print_stats(args, frame):
    """``info --stats``: `pgsd.hoomd.frame_stats` of one frame, or of every frame in one line each, on the host."""
    from . import hoomd
    fields = [n for n in args.fields.split(',') if n] if args.fields else list(hoomd._STATS_FIELDS)
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    with hoomd.open(args.file, 'r') as traj:
        if args.all_frames:
            print("non-finite entries and largest speed per frame (%s):" % ', '.join(fields))
            for i in range(len(traj)):
                snap = traj[i]
                stats = hoomd.frame_stats(snap, fields, where=where)
                bad = sum(int(st.nan[:_stats_columns(hoomd, name)].sum() + st.inf[:_stats_columns(hoomd, name)].sum())
                          for name, st in stats.items())      # (the norm column is derived: its rows are counted already)
                speed = hoomd.frame_stats(snap, ['velocity'], where=where)['velocity'].max[3]
                print("  frame %-6d step %-10d non-finite %-8d max |velocity| %s"
                      % (i, int(snap.configuration.step), bad, _norm_text(speed)))
            return
        stats = hoomd.frame_stats(traj[frame], fields, where=where)
    print("statistics of frame %d%s:" % (frame, " (types %s)" % args.types if args.types else ""))
    for name, st in stats.items():
        M = _stats_columns(hoomd, name)
        mean = st.mean
        for c in range(M):
            print("  %-12s %d  count %d  nan %d  inf %d  min %r  max %r  mean %r"
                  % (name, c, st.count[c], st.nan[c], st.inf[c], float(st.min[c]), float(st.max[c]), float(mean[c])))
        if M < len(st.count):
            print("  %-12s max norm %s" % (name, _norm_text(st.max[M])))


def _stats_columns(hoomd, name):
    """The stored columns of a field: what `frame_stats` returns for it, without the norm column."""
    return hoomd._PARTICLE_FIELDS[name][1]


def _norm_text(norm2):
    """The largest norm from the largest squared norm (``-inf``: no row took part)."""
    import math
    return 'n/a' if norm2 == -math.inf else repr(math.sqrt(norm2))


def _print_balance(args, frame):
    """``info --balance``: `pgsd.hoomd.balanced_grid` of one frame on the host, beside the equal grid."""
    from . import hoomd
    try:
        nx, ny, nz = (int(v) for v in args.balance.split(','))
    except ValueError:
        raise ValueError("--balance takes NX,NY,NZ: %r" % args.balance)
    with hoomd.open(args.file, 'r') as traj:
        snap = traj[frame]
    position, box, dims = snap.particles.position, snap.configuration.box, int(snap.configuration.dimensions)
    bins = 1024 if args.bins is None else args.bins
    _, splits = hoomd.balanced_grid(position, box, nx, ny, nz, bins=bins, dimensions=dims)
    print("balance of frame %d over %d x %d x %d cells (%d bins):" % (frame, nx, ny, nz, bins))
    for axis, split in zip('xyz', splits):
        print("  %s_split:        %s" % (axis, 'None' if split is None else '[' + ', '.join(repr(w) for w in split) + ']'))
    for label, grid in (('equal', (None, None, None)), ('balanced', splits)):
        counts, nowhere = hoomd.domain_counts(position, box, nx, ny, nz, *grid, dimensions=dims)
        mean = counts.sum() / len(counts)
        print("  %s grid counts: %s" % (label, ' '.join(str(int(c)) for c in counts)))
        print("  %s grid max / mean: %s" % (label, "%.3f" % (counts.max() / mean) if mean > 0 else 'n/a'))
        if nowhere:
            print("  %s grid nowhere: %d" % (label, nowhere))


def _cmd_vtu(args):
    from . import vtu
    where = {'type': [t for t in args.types.split(',') if t]} if args.types else None
    for name in vtu.pgsd2vtu(args.file, args.output, where=where):
        print(name)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    parser = argparse.ArgumentParser(prog="pgsd", description="Readers and writers of the PGSD (GSD v2) file format.")
    parser.add_argument('--version', action='store_true', help="Display the version number and exit.")
    parser.add_argument('--debug', action='store_true', help="Show traceback on error for debugging.")
    sub = parser.add_subparsers()
    p = sub.add_parser('read', help="interactive prompt with the file open")
    p.add_argument('file', type=str, nargs='?', help="PGSD file to read.")
    p.add_argument('-s', '--schema', type=str, default='hoomd', choices=['hoomd', 'none'], help="The file schema.")
    p.add_argument('-m', '--mode', type=str, default='r', choices=_MODES, help="The file mode.")
    p.set_defaults(func=_cmd_read)
    p = sub.add_parser('info', help="print header and chunk list")
    p.add_argument('file', type=str)
    p.add_argument('-f', '--frame', type=int, default=-1, help="frame whose chunks are listed (default: last)")
    p.add_argument('--balance', type=str, default=None, metavar='NX,NY,NZ',
                   help="print the split lists that balance the frame over NX x NY x NZ cells, and the cell counts")
    p.add_argument('--bins', type=int, default=None, metavar='B',
                   help="histogram bins per axis for --balance (a power of two; default: 1024); with --neighbours the "
                        "g(r) table over B bins (1 to 1024; default: no table)")
    p.add_argument('--stats', action='store_true',
                   help="print count, nan, inf, min, max and mean per field and column of the frame")
    p.add_argument('--fields', type=str, default=None, metavar='NAME[,NAME...]',
                   help="the per-particle fields of --stats (default: position,velocity,density,pressure,energy) and the float "
                        "fields --sample interpolates (default: velocity)")
    p.add_argument('--types', type=str, default=None, metavar='NAME[,NAME...]',
                   help="--stats, --moments and --displacement over the particles of these types only")
    p.add_argument('--all-frames', action='store_true',
                   help="with --stats: one line per frame with the non-finite entries and the largest speed; "
                        "with --moments: one line per frame with the totals; "
                        "with --displacement: one line per frame against the origin")
    p.add_argument('--moments', action='store_true',
                   help="print count, mass, momentum, kinetic and internal energy and centre of mass per particle type")
    p.add_argument('--displacement', action='store_true',
                   help="print count, mean drift, mean-squared displacement and the largest move per particle type "
                        "between the origin and the frame")
    p.add_argument('--cells', type=str, default=None, metavar='CX,CY,CZ',
                   help="print the occupied cells, the smallest and largest count, the largest density and speed with "
                        "their cells and the particles nowhere, over a uniform CX x CY x CZ grid")
    p.add_argument('--neighbours', type=float, default=None, metavar='R',
                   help="print the neighbour census inside the range R: grid, entries, mean, smallest and largest count, "
                        "isolated entries and the closest pair")
    p.add_argument('--neighbour-list', type=float, default=None, metavar='R',
                   help="print what a neighbour list inside the range R holds: grid, entries, pairs, the longest segment "
                        "and the bytes it occupies, without and with distances")
    p.add_argument('--half', action='store_true', help="with --neighbour-list: each pair once (j > i by list position)")
    p.add_argument('--components', type=float, default=None, metavar='R',
                   help="print the connected components with the linking length R: their number, the singletons, the "
                        "largest with its label and row, the entries nowhere")
    p.add_argument('--pieces', type=int, nargs='?', const=10, default=None, metavar='K',
                   help="with --components: print the K heaviest pieces (default 10) -- size, mass, centre, mean velocity, "
                        "span, wide -- and the number of wide pieces and of bad entries")
    p.add_argument('--min-size', type=int, default=None, metavar='K',
                   help="with --components: how many components have at least K entries and their share of the entries")
    p.add_argument('--sph', type=float, nargs='?', const=-1.0, default=None, metavar='H',
                   help="print the SPH kernel sums for the smoothing length H (without H: the frame's uniform slength): "
                        "grid, entries, density range, largest deviation from the stored density, Shepard range")
    p.add_argument('--sph-gradients', type=float, nargs='?', const=-1.0, default=None, metavar='H',
                   help="print the SPH kernel gradients for the smoothing length H (without H: the frame's uniform "
                        "slength): grid, entries, divergence and density-rate ranges, largest vorticity and normal")
    p.add_argument('--sph-adaptive', action='store_true',
                   help="print the SPH sums with the frame's per-particle slength: grid, h range and bad_h, count range "
                        "and pairs, density range and deviation, omega range")
    p.add_argument('--mode', type=str, default='gather', choices=('gather', 'mean'),
                   help="with --sph-adaptive: the support of a pair, 2 h_i (gather) or h_i + h_j (mean) (default: gather)")
    p.add_argument('--sph-tensors', type=float, nargs='?', const=-1.0, default=None, metavar='H',
                   help="print the SPH gradient tensors for the smoothing length H (without H: the frame's uniform "
                        "slength): grid, entries, uncorrected entries, determinant and trace ranges, largest shear rate")
    p.add_argument('--det-min', type=float, default=0.25, metavar='D',
                   help="with --sph-tensors: an entry is corrected where its determinant is above D (default: 0.25)")
    p.add_argument('--sph-forces', type=float, nargs='?', const=-1.0, default=None, metavar='H',
                   help="print the SPH accelerations for the smoothing length H (without H: the frame's uniform slength): "
                        "grid, entries, the largest total, pressure and viscous acceleration and the force time step")
    p.add_argument('--viscosity', type=float, default=None, metavar='MU',
                   help="with --sph-forces and --body-force: the dynamic viscosity of the laminar viscous term (default: no "
                        "viscous term)")
    p.add_argument('--gravity', type=str, default=None, metavar='GX,GY,GZ',
                   help="with --sph-forces: the gravity (default: 0,0,0; write --gravity=-1,0,0 where GX is negative)")
    p.add_argument('--sample', type=str, nargs='+', default=None, metavar=('NX,NY,NZ', 'H'),
                   help="print the SPH interpolant on an NX x NY x NZ lattice of points over the box for the smoothing "
                        "length H (without H: the frame's uniform slength): the points nowhere, outside and empty, the "
                        "largest count and the ranges of density, Shepard sum and the sampled fields")
    p.add_argument('--normalise', action='store_true', help="with --sample: divide every value by the Shepard sum")
    p.add_argument('--body-force', type=str, default=None, metavar='TYPE[,TYPE...]',
                   help="with --fluid: print the force and the torque the fluid's particles exert on the particles of these "
                        "types: counters, pressure and viscous parts, their sums, the largest particle force")
    p.add_argument('--fluid', type=str, nargs='+', default=None, metavar=('TYPE[,TYPE...]', 'H'),
                   help="with --body-force: the types of the fluid and the smoothing length H (without H: the frame's "
                        "uniform slength)")
    p.add_argument('--about', type=str, default=None, metavar='X,Y,Z',
                   help="with --body-force: the point the torque is taken about (default: 0,0,0; write --about=-1,0,0 "
                        "where X is negative)")
    p.add_argument('--kernel', type=str, default='wendland_c2', choices=('wendland_c2', 'cubic_spline'),
                   help="the kernel of --sph, --sph-adaptive, --sph-gradients, --sph-tensors, --sph-forces, --sample and --body-force (default: wendland_c2)")
    p.add_argument('--surface', type=float, default=None, metavar='S',
                   help="with --sph and --sph-adaptive: count the entries whose Shepard sum is below S (the free surface)")
    p.add_argument('--origin', type=int, default=0, help="the frame --displacement measures from (default: 0)")
    p.add_argument('--minimum-image', action='store_true',
                   help="--displacement of the wrapped positions, folded into the box, instead of through the image flags")
    p.set_defaults(func=_cmd_info)
    p = sub.add_parser('vtu', help="convert the frames to VTK .vtu files")
    p.add_argument('file', type=str)
    p.add_argument('-o', '--output', type=str, default=None, help="output directory (default: next to the file)")
    p.add_argument('--types', type=str, default=None, metavar='NAME[,NAME...]',
                   help="write only the particles of these types")
    p.set_defaults(func=_cmd_vtu)

    if '--version' in argv:  # works without a subcommand, like the reference (__main__.py:139-145)
        print('pgsd', __version__)
        return 0
    args = parser.parse_args(argv)
    if not hasattr(args, 'func'):
        parser.print_usage()
        return 2
    try:
        args.func(args)
    except KeyboardInterrupt:
        print("\nInterrupted.", file=sys.stderr)
        if args.debug:
            raise
        return 1
    except Exception as error:  # noqa: BLE001 - the command line reports, --debug re-raises
        print('Error: {}'.format(error), file=sys.stderr)
        if args.debug:
            raise
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
