"""Interpolation used either side of the multigrid path -- the interface of ``emg3d.maps.interp3d``
(reference emg3d/maps.py:179-276), evaluated on the device through the C ABI (``emg3d_interp3d``) -- and regridding,
``grid2grid`` / ``volume_average`` (reference emg3d/maps.py:34-178, 453-576: ``emg3d_interp3d_grid``,
``emg3d_volume_average``)."""
import ctypes

import numpy as np

from . import _lib


_NPAD = 12      # scipy.ndimage pads 'nearest' inputs by 12 samples before the spline filter (_prepad_for_spline_filter)


def _index_coords(points, xi):
    """Coordinates -> index coordinates of the grid vectors, as the reference does it (maps.py:255-260: not-a-knot
    cubic interpolation of the index, extrapolated)."""
    from scipy import interpolate
    return [interpolate.interp1d(p, np.arange(p.size), kind='cubic', bounds_error=False,
                                 fill_value='extrapolate')(c) for p, c in zip(points, xi)]


def _wrap_coords(c, n):
    """scipy.ndimage's map_coordinate for mode 'wrap' (ni_interpolation.c, NI_EXTEND_WRAP): period n - 1, the integer part
    of the quotient truncated towards zero."""
    c = np.array(c, dtype=np.float64)
    sz = float(n - 1)
    lo = c < 0
    hi = c > n - 1
    c[lo] = c[lo] + sz * (np.trunc(-c[lo] / sz) + 1.0)
    c[hi] = c[hi] - sz * np.trunc(c[hi] / sz)
    return c


def _boundary_mode(pts, values, xi, mode):
    """Boundary modes of map_coordinates other than 'constant': index coordinates on the host (O(n) work), then the cubic
    spline of the (edge-padded) array on the device on INDEX coordinates.  ``xi``: one coordinate array per axis.  Returns
    ``(points, values, index coordinates, method code)`` for ``emg3d_interp3d`` / ``emg3d_interp3d_grid``."""
    co = _index_coords(pts, xi)
    if mode == 'nearest':       # edge-padded array, stencil at the shifted coordinate, indices clamped (code 3)
        values = np.pad(values, _NPAD, mode='edge')
        co = [c + _NPAD for c in co]
        code = 3
    elif mode == 'reflect':     # stencil at the coordinate, indices reflected, "reflect" prefilter (code 4)
        code = 4
    else:                       # stencil at the coordinate, indices mirrored (code 2)
        if mode == 'wrap':      # scipy's NI_EXTEND_WRAP: coordinates wrapped with period n - 1, then the mirror spline
            co = [_wrap_coords(c, m) for c, m in zip(co, values.shape)]
        code = 2
    return [np.arange(m, dtype=np.float64) for m in values.shape], values, co, code


def _check_interp_args(method, mode):
    if mode not in ('constant', 'nearest', 'mirror', 'reflect', 'wrap'):
        raise ValueError(f"emg3d_amd.maps.interp3d: unknown mode {mode!r} "
                         "('constant', 'nearest', 'mirror', 'reflect', 'wrap').")
    if method not in ('linear', 'cubic'):
        raise ValueError(f"`method` must be 'linear' or 'cubic'; provided: {method!r}.")


def _fill_of(fill_value):
    fill_c = None if fill_value is None else complex(np.asarray(fill_value).ravel()[0])
    if fill_c is not None and np.isnan(fill_c.real):
        fill_c = complex(np.nan, fill_c.imag)
    return fill_c


def interp3d(points, values, new_points, method, fill_value, mode, cval=0.0):
    """Interpolate ``values`` given on the regular grid ``points`` at ``new_points`` (reference
    emg3d/maps.py:179-276): ``method`` 'linear' (``RegularGridInterpolator``; ``fill_value=None``
    extrapolates) or 'cubic' (the SciPy spline arithmetic of the reference: not-a-knot index spline, cubic
    B-spline prefilter, 4x4x4 evaluation).  Fewer than four points along an axis force 'linear'.

    ``mode`` (cubic only, ``scipy.ndimage.map_coordinates``): 'constant' (points outside get ``cval``), 'nearest' (what
    ``fields.get_receiver(extrapolate=True)`` uses: the array is extended by its edge values), 'mirror', 'reflect' and 'wrap'
    (SciPy's legacy rule: coordinates wrapped with period n - 1, mirror spline) -- the prefilter and the evaluation over the
    whole array run in HBM, the boundary rule is applied to the O(n_points) index coordinates on the host."""
    _check_interp_args(method, mode)
    lib = _lib.load()
    values = np.asarray(values)
    dtype = np.dtype(np.complex128 if np.iscomplexobj(values) else np.float64)
    pts = [np.ascontiguousarray(p, dtype=np.float64) for p in points]
    if values.shape != tuple(p.size for p in pts):
        raise ValueError(f"There are {tuple(p.size for p in pts)} points and {values.shape} values.")
    xi = np.broadcast_arrays(*[np.asarray(c, dtype=np.float64) for c in new_points])
    shape = xi[0].shape
    n = int(xi[0].size)
    code = 0 if method == 'linear' else 1
    if code == 1 and mode != 'constant' and all(p.size >= 4 for p in pts):
        pts, values, xi, code = _boundary_mode(pts, values, [c.ravel() for c in xi], mode)
    vals = np.ascontiguousarray(values.astype(dtype, copy=False).ravel(order='F'))
    flat = np.ascontiguousarray(np.stack([np.asarray(c).ravel() for c in xi]))
    out = np.empty(max(n, 1), dtype=dtype)
    fill_c = _fill_of(fill_value)
    if n:
        _lib.check(lib.emg3d_interp3d(_lib.dtype_code(dtype), *(int(p.size) for p in pts), *(_lib.ptr(p) for p in pts),
                                      _lib.ptr(vals), n, _lib.ptr(flat), code,
                                      0 if fill_c is None else 1, 0.0 if fill_c is None else fill_c.real,
                                      float(cval), _lib.ptr(out)), "emg3d_interp3d")
    if code < 2 and fill_c is not None and dtype.kind == 'c' and np.isnan(fill_c.real) and np.isnan(fill_c.imag):
        # a complex NaN fill value (0j * nan = nan + nan j, what fields.get_receiver passes): both parts
        bad = np.isnan(out.real)
        out[bad] = complex(np.nan, np.nan)
    return out[:n].reshape(shape)


def interp3d_grid(points, values, new_axes, method, fill_value, mode, cval=0.0):
    """``interp3d`` on the tensor product of the coordinate vectors ``new_axes = (x, y, z)``: returns the F-ordered
    ``(x.size, y.size, z.size)`` array whose entry ``[i, j, k]`` is ``interp3d(points, values, (x[i], y[j], z[k]), ...)``
    bit for bit, without materialising the points (``emg3d_interp3d_grid``: index coordinates and intervals per axis)."""
    _check_interp_args(method, mode)
    lib = _lib.load()
    values = np.asarray(values)
    dtype = np.dtype(np.complex128 if np.iscomplexobj(values) else np.float64)
    pts = [np.ascontiguousarray(p, dtype=np.float64) for p in points]
    if values.shape != tuple(p.size for p in pts):
        raise ValueError(f"There are {tuple(p.size for p in pts)} points and {values.shape} values.")
    xi = [np.ascontiguousarray(np.ravel(c), dtype=np.float64) for c in new_axes]
    shape = tuple(c.size for c in xi)
    code = 0 if method == 'linear' else 1
    if code == 1 and mode != 'constant' and all(p.size >= 4 for p in pts):
        pts, values, xi, code = _boundary_mode(pts, values, xi, mode)
        xi = [np.ascontiguousarray(c, dtype=np.float64) for c in xi]
    vals = np.ascontiguousarray(values.astype(dtype, copy=False).ravel(order='F'))
    out = np.empty(shape, dtype=dtype, order='F')
    fill_c = _fill_of(fill_value)
    if out.size:
        _lib.check(lib.emg3d_interp3d_grid(_lib.dtype_code(dtype), *(int(p.size) for p in pts), *(_lib.ptr(p) for p in pts),
                                           _lib.ptr(vals), shape[0], _lib.ptr(xi[0]), shape[1], _lib.ptr(xi[1]), shape[2],
                                           _lib.ptr(xi[2]), code, 0 if fill_c is None else 1,
                                           0.0 if fill_c is None else fill_c.real, float(cval), _lib.ptr(out)),
                   "emg3d_interp3d_grid")
    if code < 2 and fill_c is not None and dtype.kind == 'c' and np.isnan(fill_c.real) and np.isnan(fill_c.imag):
        bad = np.isnan(out.real)            # a complex NaN fill value: both parts (as interp3d)
        out[bad] = complex(np.nan, np.nan)
    return out


def _volume_average_weights(x1, x2):
    """Weights and indices of volume averaging along one axis (reference emg3d/maps.py:526-576): the old edges ``x1`` and
    the new edges ``x2`` -> ``(hs, ix1, ix2)``: the length of every segment of the union of the edges that lies in the new
    grid, the old cell and the new cell holding it (``emg3d_volume_average_weights``, host work, no device)."""
    w, ix1, ix2, _ = _volume_average_segments(x1, x2)
    return w, ix1.astype(np.int32), ix2.astype(np.int32)


def _volume_average_segments(x1, x2):
    """``(w, ix1, ix2, ptr)``: ``_volume_average_weights`` plus the per-new-cell segment offsets (new cell ``o`` owns
    segments ``ptr[o]:ptr[o+1]``)."""
    lib = _lib.load()
    x1 = np.ascontiguousarray(x1, dtype=np.float64)
    x2 = np.ascontiguousarray(x2, dtype=np.float64)
    cap = max(x1.size + x2.size - 1, 1)
    w = np.empty(cap)
    ix1 = np.empty(cap, dtype=np.int64)
    ix2 = np.empty(cap, dtype=np.int64)
    ptr = np.empty(max(x2.size, 1), dtype=np.int64)
    ns = ctypes.c_int64(0)
    _lib.check(lib.emg3d_volume_average_weights(_lib.ptr(x1), x1.size, _lib.ptr(x2), x2.size, _lib.ptr(w), _lib.ptr(ix1),
                                                _lib.ptr(ix2), _lib.ptr(ptr), ctypes.byref(ns)),
               "emg3d_volume_average_weights")
    n = ns.value
    return w[:n], ix1[:n], ix2[:n], ptr


def volume_average(edges_x, edges_y, edges_z, values, new_edges_x, new_edges_y, new_edges_z, new_values, new_vol):
    """Volume averaging (reference emg3d/maps.py:453-523): the volume-weighted averages of ``values`` (on the grid of
    ``edges_*``) over the cells of the new grid are ADDED to ``new_values`` (in place), which is then divided by
    ``new_vol`` -- on the device (``emg3d_volume_average``: one thread per new cell, the reference's order of
    operations, bit for bit)."""
    lib = _lib.load()
    values = np.asarray(values)
    dtype = np.dtype(np.complex128 if np.iscomplexobj(values) or np.iscomplexobj(new_values) else np.float64)
    edges = [np.ascontiguousarray(e, dtype=np.float64) for e in (edges_x, edges_y, edges_z)]
    new_edges = [np.ascontiguousarray(e, dtype=np.float64) for e in (new_edges_x, new_edges_y, new_edges_z)]
    n = tuple(e.size - 1 for e in edges)
    m = tuple(e.size - 1 for e in new_edges)
    if values.shape != n or np.shape(new_values) != m or np.shape(new_vol) != m:
        raise ValueError(f"volume_average: values {values.shape} on a {n} grid, new_values {np.shape(new_values)} and "
                         f"new_vol {np.shape(new_vol)} on a {m} grid.")
    vals = values.astype(dtype, copy=False).ravel(order='F')            # a view when `values` is F-ordered already
    vals = np.ascontiguousarray(vals)
    out = np.ascontiguousarray(np.asarray(new_values, dtype=dtype).ravel(order='F'))
    vol = np.ascontiguousarray(np.asarray(new_vol, dtype=np.float64).ravel(order='F'))
    _lib.check(lib.emg3d_volume_average(_lib.dtype_code(dtype), *n, *(_lib.ptr(e) for e in edges), _lib.ptr(vals), *m,
                                        *(_lib.ptr(e) for e in new_edges), _lib.ptr(out), _lib.ptr(vol)),
               "emg3d_volume_average")
    new_values[...] = out.reshape(m, order='F')


def _volume_average_old_offsets(ix1, n):
    """The old-cell offsets of one axis' segments (``emg3d_volume_average_old_offsets``, host work, no device): ``ix1`` from
    ``_volume_average_weights`` is ascending, old cell ``i`` of ``n`` owns segments ``iptr[i]:iptr[i+1]`` -- what the transpose of
    volume averaging gathers with."""
    ix1 = np.ascontiguousarray(ix1, dtype=np.int64)
    iptr = np.empty(int(n) + 1, dtype=np.int64)
    _lib.check(_lib.load().emg3d_volume_average_old_offsets(_lib.ptr(ix1), ix1.size, int(n), _lib.ptr(iptr)),
               "emg3d_volume_average_old_offsets")
    return iptr


def volume_average_adjoint(edges_x, edges_y, edges_z, new_edges_x, new_edges_y, new_edges_z, y, new_vol):
    """The exact transpose of :func:`volume_average`: with ``A`` the matrix ``volume_average`` applies to a zero ``new_values``
    (``A[o, i]`` = the segment weights of new cell ``o`` that lie in old cell ``i``, over ``new_vol[o]``), returns ``A^T y`` --
    ``y`` and ``new_vol`` real, on the new grid, the result (float64, F-ordered) on the old grid; ``sum(A v * y) == sum(v *
    A^T y)``.  On the device (``emg3d_volume_average_adjoint``: one thread per old cell gathers ``y / new_vol`` over its
    segments in a fixed order; no atomics, results repeat bit for bit).  An old cell that no part of the new grid covers gets
    an exact 0.  The reference has no such function: it maps gradients to the model grid by cubic interpolation
    (``optimize.model_gradient``), which is not the derivative of what ``Model.interpolate2grid`` does."""
    lib = _lib.load()
    if np.iscomplexobj(y):
        raise TypeError("volume_average_adjoint: `y` must be real (gradients are real in both domains).")
    edges = [np.ascontiguousarray(e, dtype=np.float64) for e in (edges_x, edges_y, edges_z)]
    new_edges = [np.ascontiguousarray(e, dtype=np.float64) for e in (new_edges_x, new_edges_y, new_edges_z)]
    n = tuple(e.size - 1 for e in edges)
    m = tuple(e.size - 1 for e in new_edges)
    if np.shape(y) != m or np.shape(new_vol) != m:
        raise ValueError(f"volume_average_adjoint: y {np.shape(y)} and new_vol {np.shape(new_vol)} on a {m} grid.")
    yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel(order='F'))
    vol = np.ascontiguousarray(np.asarray(new_vol, dtype=np.float64).ravel(order='F'))
    out = np.empty(n, dtype=np.float64, order='F')
    _lib.check(lib.emg3d_volume_average_adjoint(*n, *(_lib.ptr(e) for e in edges), *m, *(_lib.ptr(e) for e in new_edges),
                                                _lib.ptr(yv), _lib.ptr(vol), _lib.ptr(out)), "emg3d_volume_average_adjoint")
    return out


def regrid_factors(model, sigma):
    """The diagonal factors of the Jacobian of ``model.interpolate2grid(model_grid, grid)`` followed by the property map, per
    direction: with ``A`` volume averaging from the model grid to the computational grid, ``d sigma_c / d p_m = F A Q``.
    ``model`` lives on the model grid, ``sigma = (sigma_x, sigma_y, sigma_z)`` are the conductivities on the computational grid
    as the device holds them (``DeviceMG.get_sigma``).  Returns ``(F, Q)``, 3-tuples of arrays (entries of directions that
    share the model's ``property_x`` are the same object).

    * logarithmic maps (regridded with ``log=False``): ``p_c = A p_m``; ``F = chain_factor(sigma_c)``, ``Q = 1``;
    * ``Conductivity`` / ``Resistivity`` (``log=True``): ``p_c = 10^(A log10 p_m)``, ``d p_c / d p_m = diag(p_c) A diag(1 / p_m)``:
      ``F = chain_factor(sigma_c) p_c`` -- ``sigma_c`` resp. ``-sigma_c`` --, ``Q = 1 / p_m``.

    Multiplications and one reciprocal of the model's own arrays only: no transcendental runs a second time."""
    fmap = model.map
    props = (model.property_x, model.property_y if model.case in (1, 3) else None,
             model.property_z if model.case in (2, 3) else None)
    F, Q = [], []
    for c in range(3):
        if c > 0 and props[c] is None:
            F.append(F[0]); Q.append(Q[0])
            continue
        s = np.asarray(sigma[c], dtype=np.float64)
        p = np.broadcast_to(np.asarray(props[c], dtype=np.float64), model.vnC)
        if fmap.log:
            F.append(fmap.chain_factor(s))
            Q.append(np.ones(p.shape))
        else:
            F.append(s.copy() if fmap.name == 'Conductivity' else -s)
            Q.append(1.0 / p)
    return tuple(F), tuple(Q)


def grid2grid(grid, values, new_grid, method='linear', extrapolate=True, log=False):
    """Interpolate ``values`` located on ``grid`` to ``new_grid`` (reference emg3d/maps.py:34-178).

    ``values``: model parameters on the cells, one field component (edges: cell centres and nodes per axis, chosen by the
    array's shape), or a :class:`emg3d_amd.fields.Field` (regridded per component; returns ``values.__class__(fx, fy,
    fz)``).  ``method``: 'linear', 'cubic' (fewer than four points along an axis: 'linear') or 'volume' (volume averaging,
    cells only).  ``extrapolate``: points outside ``grid`` take the nearest value ('cubic') or are extrapolated ('linear');
    ``False``: they are 0 ('volume' always takes the nearest cell).  ``log``: the same on ``log10(values)``, then ``10**``
    (both on the host).

    'volume' runs ``emg3d_volume_average``, 'linear' / 'cubic' run ``emg3d_interp3d_grid`` on the tensor product of the
    new grid's vectors: the reference's results bit for bit ('volume') or with its SciPy arithmetic ('linear', 'cubic')."""
    if hasattr(values, 'field') and np.ndim(values.field) == 1:
        fx, fy, fz = (grid2grid(grid, np.asarray(c), new_grid, method, extrapolate, log)
                      for c in (values.fx, values.fy, values.fz))
        return values.__class__(fx, fy, fz)
    values = np.asarray(values)
    if tuple(grid.vnC) != values.shape and method == 'volume':
        raise ValueError("``method='volume'`` not implemented for fields.")
    if method not in ('linear', 'cubic', 'volume'):
        raise ValueError(f"`method` must be 'linear', 'cubic' or 'volume'; provided: {method!r}.")
    if log:
        values = np.log10(values)
    if method == 'volume':
        new_values = np.zeros(new_grid.vnC, dtype=values.dtype, order='F')
        vol = new_grid.cell_volumes.reshape(new_grid.vnC, order='F')
        volume_average(grid.nodes_x, grid.nodes_y, grid.nodes_z, values, new_grid.nodes_x, new_grid.nodes_y,
                       new_grid.nodes_z, new_values, vol)
    else:
        points, new_points = [], []
        for i, c in enumerate('xyz'):
            kind = 'nodes_' if values.shape[i] == grid.shape_nodes[i] else 'cell_centers_'
            points.append(getattr(grid, kind + c))
            new_points.append(getattr(new_grid, kind + c))
        if extrapolate:
            new_values = interp3d_grid(points, values, new_points, method, None, 'nearest')
        else:
            new_values = interp3d_grid(points, values, new_points, method, 0.0, 'constant')
    return 10**new_values if log else new_values


def edges2cellaverages(ex, ey, ez, vol, out_x, out_y, out_z):
    """Interpolate fields defined on edges to volume-averaged cell values, ADDED into ``out_x/y/z`` in place --
    the interface of the reference's numba kernel ``maps.edges2cellaverages`` (emg3d/maps.py:578-630), evaluated on
    the device (``emg3d_edges2cellaverages``: one thread per cell, the reference's accumulation order)."""
    lib = _lib.load()
    dtype = np.dtype(np.complex128 if any(np.iscomplexobj(a) for a in (ex, ey, ez)) else np.float64)
    f = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=dtype).ravel(order='F') for a in (ex, ey, ez)]))
    nx, ny, nz = (int(v) for v in np.shape(vol))
    v = np.ascontiguousarray(np.asarray(vol, dtype=np.float64).ravel(order='F'))
    outs = [np.ascontiguousarray(np.asarray(o, dtype=dtype).ravel(order='F')) for o in (out_x, out_y, out_z)]
    _lib.check(lib.emg3d_edges2cellaverages(_lib.dtype_code(dtype), nx, ny, nz, _lib.ptr(f), _lib.ptr(v),
                                            *(_lib.ptr(o) for o in outs)), "emg3d_edges2cellaverages")
    for o, r in zip((out_x, out_y, out_z), outs):
        o[...] = r.reshape((nx, ny, nz), order='F') if np.iscomplexobj(o) or dtype == np.float64 else r.reshape((nx, ny, nz), order='F').real


def cellaverages2edges(vx, vy, vz, vol, out_x, out_y, out_z):
    """The exact transpose of :func:`edges2cellaverages`: cell values ``vx, vy, vz`` (shape ``vol.shape``; ``None`` skips a
    component) to the edges, ``out_c[edge] += sum vol * v_c / 4`` over the statements of ``edges2cellaverages`` that read the
    edge -- an interior edge takes its four cells once, a boundary edge its cells two or four times, as the reference's kernel
    (emg3d/maps.py:578-630) counts them.  ADDED into ``out_x/y/z`` (the components of a field: ``fx, fy, fz`` views) in place;
    ``sum(e2c(f) * v) == sum(f * c2e(v))``.  Evaluated on the device (``emg3d_cells2edges``: one thread per edge gathers its
    cells).  The reference has no such function (its adjoint does not need one); ``optimize.Jacobian.jvec`` builds its
    right-hand side with the same gather."""
    lib = _lib.load()
    arrs = [a for a in (vx, vy, vz, out_x, out_y, out_z) if a is not None]
    dtype = np.dtype(np.complex128 if any(np.iscomplexobj(a) for a in arrs) else np.float64)
    nx, ny, nz = (int(v) for v in np.shape(vol))
    shapes = ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))
    vl = np.ascontiguousarray(np.asarray(vol, dtype=np.float64).ravel(order='F'))
    vs, outs = [], []
    for v, o, shp in zip((vx, vy, vz), (out_x, out_y, out_z), shapes):
        if v is None:
            vs.append(None); outs.append(None)
            continue
        if np.shape(v) != (nx, ny, nz) or o is None or np.shape(o) != shp:
            raise ValueError(f"cellaverages2edges: cell arrays must have shape {(nx, ny, nz)}, the outputs {shapes}.")
        if dtype.kind == 'c' and not np.iscomplexobj(o):
            raise TypeError("cellaverages2edges: complex cell values need complex outputs.")
        vs.append(np.ascontiguousarray(np.asarray(v, dtype=dtype).ravel(order='F')))
        outs.append(np.ascontiguousarray(np.asarray(o, dtype=dtype).ravel(order='F')))
    none = ctypes.c_void_p(None)
    _lib.check(lib.emg3d_cells2edges(_lib.dtype_code(dtype), nx, ny, nz, *(none if v is None else _lib.ptr(v) for v in vs),
                                     _lib.ptr(vl), *(none if o is None else _lib.ptr(o) for o in outs)), "emg3d_cells2edges")
    for o, r, shp in zip((out_x, out_y, out_z), outs, shapes):
        if r is not None:
            o[...] = r.reshape(shp, order='F')


def _edges2cellaverages_host(comps, vol):
    """``edges2cellaverages`` in plain numpy, in the scalar type of its arguments (``np.longdouble`` included): the three cell
    arrays, returned.  Per cell the statements are added in the order of the device's ``e2c_component`` -- the cell's four edges
    of a component with the second transverse axis outermost, per edge the reference's four statements (m1, m2), (p1, m2), (m1,
    p2), (p1, p2) of which a boundary cell receives two or four -- each as one array operation (a statement that does not hit a
    cell adds an exact zero there)."""
    n = vol.shape
    J = np.ogrid[:n[0], :n[1], :n[2]]
    everywhere = np.ones((1, 1, 1), dtype=bool)
    out = []
    for c, f in enumerate(comps):
        t1, t2 = (1 if c == 0 else 0), (1 if c == 2 else 2)
        acc = np.zeros(n, dtype=np.result_type(f.dtype, vol.dtype))

        def hits(t, q):     # which cells edge j + q of axis t reaches through m = max(e - 1, 0) and through p = min(e, n - 1)
            return (everywhere if q else J[t] == 0), (J[t] == n[t] - 1 if q else everywhere)
        for q2 in (0, 1):
            m2, p2 = hits(t2, q2)
            for q1 in (0, 1):
                m1, p1 = hits(t1, q1)
                sl = [slice(None)] * 3
                sl[t1], sl[t2] = slice(q1, n[t1] + q1), slice(q2, n[t2] + q2)
                v = (vol * f[tuple(sl)]) / 4
                for a1, a2 in ((m1, m2), (p1, m2), (m1, p2), (p1, p2)):
                    acc = acc + np.where(a1 & a2, v, 0)
        out.append(acc)
    return out


def sensitivity_diagonal(grid, fwd, adj, smu0, weights, components=False, dtype=np.float64):
    """Host restatement (plain numpy) of what ``DeviceMG.sens_acc_add`` adds, from zero: ``sum over the pairs of weights[b_adj,
    b_fwd] * |c_x + c_y + c_z|^2`` with ``c_c = edges2cellaverages_c((adj[b_adj] * fwd[b_fwd]) * smu0)`` and the cell volumes
    ``(hx * hy) * hz`` of ``grid`` -- the diagonal of ``J^H W J`` when ``adj[b]`` is the field of receiver ``b``'s adjoint source
    and ``fwd[b]`` the forward field of source ``b`` (``optimize.SurveyJacobian.sensitivity_diagonal``).  ``fwd``: ``(n_fwd, nE)``,
    ``adj``: ``(n_adj, nE)`` fields ``[fx|fy|fz]`` (both real or complex), ``weights``: ``(n_adj, n_fwd)``, real; a pair with weight
    0 is skipped.  The pairs are added in the kernel's order (adjoint systems outer, forward systems inner, both ascending), the
    statements per cell in its order too.  ``dtype``: the real type everything is evaluated and accumulated in (``np.longdouble``:
    the yardstick of the tests).  ``components=True``: ``(W |c_x|^2, W |c_y|^2, W |c_z|^2)`` summed likewise.  Returns arrays of
    shape ``grid.vnC`` and type ``dtype``.  ``maps.edges2cellaverages`` runs on the device in float64, so the averaging is
    restated here (``_edges2cellaverages_host``)."""
    rtype = np.dtype(dtype)
    fwd, adj = np.atleast_2d(np.asarray(fwd)), np.atleast_2d(np.asarray(adj))
    cplx = np.iscomplexobj(fwd) or np.iscomplexobj(adj) or np.iscomplexobj(smu0)
    ftype = np.result_type(rtype, np.complex64) if cplx else rtype
    nx, ny, nz = (int(n) for n in grid.vnC)
    shapes = ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))
    off = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    weights = np.asarray(weights, dtype=np.float64)
    if fwd.shape[1] != off[3] or adj.shape[1] != off[3] or weights.shape != (adj.shape[0], fwd.shape[0]):
        raise ValueError(f"sensitivity_diagonal: fields of {off[3]} edges and weights of shape (n_adj, n_fwd) are needed; provided: "
                         f"{fwd.shape}, {adj.shape}, {weights.shape}.")
    hx, hy, hz = (np.asarray(h, dtype=np.float64).astype(rtype) for h in grid.h)
    vol = (hx[:, None, None] * hy[None, :, None]) * hz[None, None, :]
    s = ftype.type(smu0) if cplx else rtype.type(np.real(smu0))
    fwd, adj = fwd.astype(ftype), adj.astype(ftype)
    acc = [np.zeros((nx, ny, nz), dtype=rtype) for _ in range(3 if components else 1)]

    def abs2(c):
        return c.real * c.real + c.imag * c.imag if cplx else c * c
    for ba in range(adj.shape[0]):
        for bf in range(fwd.shape[0]):
            w = weights[ba, bf]
            if w == 0:
                continue
            prod = (adj[ba] * fwd[bf]) * s
            cc = _edges2cellaverages_host([prod[off[c]:off[c + 1]].reshape(shapes[c], order='F') for c in range(3)], vol)
            w = rtype.type(w)
            if components:
                acc = [a + w * abs2(c) for a, c in zip(acc, cc)]
            else:
                acc[0] = acc[0] + w * abs2((cc[0] + cc[1]) + cc[2])
    out = tuple(np.asfortranarray(a) for a in acc)
    return out if components else out[0]


def sensitivity_rows(grid, fwd, adj, smu0, components=False, dtype=np.float64):
    """Host restatement (plain numpy) of what ``DeviceMG.sens_rows`` returns: the rows whose weighted squares
    :func:`sensitivity_diagonal` sums.  Row ``p`` belongs to the pair ``(b_adj, b_fwd) = divmod(p, n_fwd)`` -- the kernel's order:
    adjoint systems outer, forward systems inner, both ascending -- and is ``(c_x + c_y) + c_z`` with ``c_c =
    edges2cellaverages_c((adj[b_adj] * fwd[b_fwd]) * smu0)`` and the cell volumes ``(hx * hy) * hz`` of ``grid``, the statements per
    cell in the kernel's order (``_edges2cellaverages_host``).  ``fwd``: ``(n_fwd, nE)``, ``adj``: ``(n_adj, nE)`` fields
    ``[fx|fy|fz]`` (both real or complex).  ``dtype``: the real type everything is evaluated in (``np.longdouble``: the yardstick of
    the tests); the rows are complex of that precision if a field or ``smu0`` is complex.  Returns an array of shape ``(n_adj *
    n_fwd, ndir) + grid.vnC``, ``ndir`` = 1, or 3 with ``components=True``: ``c_x, c_y, c_z`` apart."""
    rtype = np.dtype(dtype)
    fwd, adj = np.atleast_2d(np.asarray(fwd)), np.atleast_2d(np.asarray(adj))
    cplx = np.iscomplexobj(fwd) or np.iscomplexobj(adj) or np.iscomplexobj(smu0)
    ftype = np.result_type(rtype, np.complex64) if cplx else rtype
    nx, ny, nz = (int(n) for n in grid.vnC)
    shapes = ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))
    off = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    if fwd.shape[1] != off[3] or adj.shape[1] != off[3]:
        raise ValueError(f"sensitivity_rows: fields of {off[3]} edges are needed; provided: {fwd.shape}, {adj.shape}.")
    hx, hy, hz = (np.asarray(h, dtype=np.float64).astype(rtype) for h in grid.h)
    vol = (hx[:, None, None] * hy[None, :, None]) * hz[None, None, :]
    s = ftype.type(smu0) if cplx else rtype.type(np.real(smu0))
    fwd, adj = fwd.astype(ftype), adj.astype(ftype)
    ndir = 3 if components else 1
    rows = np.zeros((adj.shape[0] * fwd.shape[0], ndir, nz, ny, nx), dtype=ftype).transpose(0, 1, 4, 3, 2)      # every row F-ordered
    for ba in range(adj.shape[0]):
        for bf in range(fwd.shape[0]):
            prod = (adj[ba] * fwd[bf]) * s
            cc = _edges2cellaverages_host([prod[off[c]:off[c + 1]].reshape(shapes[c], order='F') for c in range(3)], vol)
            p = ba * fwd.shape[0] + bf
            if components:
                for c in range(3):
                    rows[p, c] = cc[c]
            else:
                rows[p, 0] = (cc[0] + cc[1]) + cc[2]
    return rows


# --------------------------------------------------------------------------
# Smoothing model covariance
# --------------------------------------------------------------------------
def smoothing_matrix(h, ell):
    """One axis of ``SmoothingCovariance``: the symmetric tridiagonal ``T = I + ell^2 H^-1/2 D^T diag(1/d) D H^-1/2`` of the cell
    widths ``h`` and the correlation length ``ell`` as ``(diag, off)``, float64 -- ``off[i] = -ell^2 / (d[i] sqrt(h[i] h[i+1]))``,
    ``diag[i] = 1 + ell^2 / (h[i] d[i-1]) + ell^2 / (h[i] d[i])`` with ``d[i] = (h[i] + h[i+1]) / 2`` and the term whose ``d``
    does not exist dropped (Neumann ends)."""
    h = np.asarray(h, dtype=np.float64)
    n = h.size
    ell = np.float64(ell)
    diag, off = np.ones(n), np.zeros(max(n - 1, 0))
    d = [(h[i] + h[i + 1]) / 2 for i in range(n - 1)]
    for i in range(n - 1):
        off[i] = -(ell * ell) / (d[i] * np.sqrt(h[i] * h[i + 1]))
    for i in range(n):
        t = np.float64(1.0)
        if i > 0:
            t = t + (ell * ell) / (h[i] * d[i - 1])
        if i < n - 1:
            t = t + (ell * ell) / (h[i] * d[i])
        diag[i] = t
    return diag, off


def smoothing_factors(h, ell):
    """The factors ``(lo, cp, inv)`` of ``smoothing_matrix(h, ell)`` for the line solve of ``SmoothingCovariance``, computed once, in
    NumPy float64 scalars, in this order: ``inv[0] = 1 / diag[0]``; ``lo[i] = off[i-1]``, ``inv[i] = 1 / (diag[i] - off[i-1]
    cp[i-1])`` for ``i >= 1``; ``cp[i] = off[i] inv[i]`` for ``i < n - 1``; ``lo[0] = cp[n-1] = 0``.  ``None`` where ``T = I``
    (one cell, or ``ell = 0``): the axis is skipped."""
    diag, off = smoothing_matrix(h, ell)
    n = diag.size
    if n == 1 or ell == 0:
        return None
    lo, cp, inv = np.zeros(n), np.zeros(n), np.zeros(n)
    inv[0] = 1 / diag[0]
    for i in range(n):
        if i >= 1:
            lo[i] = off[i - 1]
            inv[i] = 1 / (diag[i] - off[i - 1] * cp[i - 1])
        if i < n - 1:
            cp[i] = off[i] * inv[i]
    return lo, cp, inv


def smooth_lines_host(a, axis, factors, passes=1):
    """``passes`` line solves in a row along ``axis`` of the float64 array ``a``, IN PLACE: sequential Thomas, vectorised over the
    lines, every element through the same scalar operations, each rounded once -- ``a[0] *= inv[0]``; ``a[i] = (a[i] - lo[i]
    a[i-1]) inv[i]`` upwards; ``a[i] = a[i] - cp[i] a[i+1]`` downwards.  The reference the device equals bit for bit."""
    lo, cp, inv = factors
    v = np.moveaxis(a, axis, 0)
    n = v.shape[0]
    for _ in range(passes):
        v[0] = v[0] * inv[0]
        for i in range(1, n):
            v[i] = (v[i] - lo[i] * v[i - 1]) * inv[i]
        for i in range(n - 2, -1, -1):
            v[i] = v[i] - cp[i] * v[i + 1]
    return a


class SmoothingCovariance:
    """A smoothing model covariance ``C = L L^T`` on the cells of ``grid``, as tridiagonal line solves along x, y and z.

    Per axis ``S_axis = T^-1`` is one implicit diffusion step with the correlation length of that axis (``smoothing_matrix``:
    symmetric positive definite, smallest eigenvalue 1, on a uniform grid the discrete ``exp(-|x| / ell')`` family); the three act
    on different Kronecker factors, so ``S = S_z S_y S_x`` is symmetric.  With ``w`` the standard deviations per cell and ``p =
    passes``: ``L = diag(w) S^p``, ``L^T = S^p diag(w)``, ``C = diag(w) S^2p diag(w)``.

    ``lengths``: a scalar or ``(lx, ly, lz)`` in metres, ``>= 0``; ``std``: a scalar, an array of ``grid.vnC``, or a 3-tuple of
    those (one per direction, for the three planes of a ``components`` row store; there is no cross-direction covariance);
    ``passes``: an int ``>= 1``.  ``factors``: per axis ``(lo, cp, inv)`` (``smoothing_factors``), ``None`` for an axis that is
    skipped (one cell or length 0).

    ``sqrt_t(v)`` is ``L^T v``: ``w * v``, then for x, y, z in this order the solve ``passes`` times in a row on every line of the
    axis; ``sqrt(v)`` is ``L v``: the same sweeps, then ``w *``; ``apply(v) = sqrt(sqrt_t(v))`` is ``C v``.  ``v``: an array of
    ``grid.vnC``, or a 3-tuple of them.  They run on the device (``emg3d_smooth3d``, ``k_rows_smooth_*``); ``host=True`` runs the
    numpy loop ``smooth_lines_host`` instead, which the device equals bit for bit.  They are stateless: every plane is uploaded,
    smoothed and downloaded on its own, on ``device`` (the constructor's, default 0, or the method's ``device=``; a ``RowStore``
    made by ``with_covariance`` passes its store's device); the result does not depend on the device.  The order of the axes
    changes the last bits, so it is part of the contract."""

    def __init__(self, grid, lengths, std=1.0, passes=1, device=0):
        self.grid, self.device = grid, int(device)
        self.vnC = tuple(int(n) for n in grid.vnC)
        ln = np.asarray(lengths, dtype=np.float64)
        if ln.shape not in ((), (3,)) or not np.all(np.isfinite(ln)) or np.any(ln < 0):
            raise ValueError(f"`lengths` must be a scalar or (lx, ly, lz), finite and >= 0; provided: {lengths!r}.")
        self.lengths = tuple(float(x) for x in np.broadcast_to(ln, (3,)))
        if isinstance(passes, (bool, np.bool_)) or not isinstance(passes, (int, np.integer)) or passes < 1:
            raise ValueError(f"`passes` must be an int >= 1; provided: {passes!r}.")
        self.passes = int(passes)
        self.std = std
        if isinstance(std, (tuple, list)):
            if len(std) != 3:
                raise ValueError(f"`std` as a tuple must have three entries (one per direction); provided: {len(std)}.")
            self._w = tuple(self._std_plane(s) for s in std)
        else:
            self._w = self._std_plane(std)
        self.factors = tuple(smoothing_factors(h, ell) for h, ell in zip(grid.h, self.lengths))

    def _std_plane(self, s):
        """One plane of `std` as F-ordered doubles; None for the scalar 1 (a product with 1 is exact: the same bits)."""
        s = np.asarray(s, dtype=np.float64)
        if s.shape not in ((), self.vnC) or not np.all(np.isfinite(s)) or np.any(s < 0):
            raise ValueError(f"`std` must be a scalar or an array of shape {self.vnC} (or a 3-tuple of those), finite and >= 0; "
                             f"provided shape: {s.shape}.")
        if s.shape == () and s == 1.0:
            return None
        return np.ascontiguousarray(np.broadcast_to(s, self.vnC).ravel(order='F'))

    def scale(self, planes):
        """The standard deviations as the columns ``[plane][cell]`` (cells F-ordered) of a row of ``planes`` planes, or ``None``
        where they are all the scalar 1."""
        if isinstance(self._w, tuple):
            if planes != 3:
                raise ValueError("a `std` per direction (a 3-tuple) needs three planes: a 3-tuple `v`, a `components` row store.")
            w = self._w
        else:
            w = (self._w,) * planes
        if all(p is None for p in w):
            return None
        return np.concatenate([np.ones(int(np.prod(self.vnC))) if p is None else p for p in w])

    def diagonal(self):
        """``diag(C)``, the prior variances, as cells (an array of ``grid.vnC``; a 3-tuple of them where ``std`` is one, as
        ``scale``).  ``C = diag(w) S^2p diag(w)`` with ``S = S_z (x) S_y (x) S_x``, so ``diag(C) = w^2 (d_z (x) d_y (x) d_x)``
        with ``d_axis = diag(S_axis^2p)``: per axis the dense inverse of ``smoothing_matrix(h, ell)`` (a tridiagonal solve of the
        identity in ``np.longdouble``, on the host -- an axis has a few hundred cells at most), ``S_axis^p`` by repeated products
        and, ``S_axis`` being symmetric, the row sums of its squares: positive by construction.  A skipped axis (length 0, or
        one cell) contributes ones."""
        d = []
        for h, ell, f in zip(self.grid.h, self.lengths, self.factors):
            n = np.asarray(h).size
            if f is None:
                d.append(np.ones(n))
                continue
            dg, off = (a.astype(np.longdouble) for a in smoothing_matrix(h, ell))
            X = np.eye(n, dtype=np.longdouble)          # T X = I by elimination without pivoting (T is diagonally dominant)
            c = np.zeros(n, dtype=np.longdouble)
            for i in range(n):
                piv = dg[i] - off[i - 1] * c[i - 1] if i else dg[0]
                X[i] = (X[i] - off[i - 1] * X[i - 1]) / piv if i else X[0] / piv
                if i < n - 1:
                    c[i] = off[i] / piv
            for i in range(n - 2, -1, -1):
                X[i] = X[i] - c[i] * X[i + 1]
            Sp = X
            for _ in range(self.passes - 1):
                Sp = Sp @ X
            d.append(np.asarray((Sp * Sp).sum(axis=1), dtype=np.float64))
        kron = d[0][:, None, None] * d[1][None, :, None] * d[2][None, None, :]
        planes = [kron.copy() if w is None else (w * w).reshape(self.vnC, order='F') * kron
                  for w in (self._w if isinstance(self._w, tuple) else (self._w,))]
        return tuple(planes) if isinstance(self._w, tuple) else planes[0]

    def _run(self, v, scale_after, host, device=None):
        three = isinstance(v, (tuple, list))
        parts = list(v) if three else [v]
        if three and len(parts) != 3:
            raise ValueError(f"`v` as a tuple must have three entries; provided: {len(parts)}.")
        ncell = int(np.prod(self.vnC))
        cols = []
        for a in parts:
            a = np.asarray(a)
            if np.iscomplexobj(a):
                raise TypeError("`v` must be real.")
            if a.shape != self.vnC:
                raise ValueError(f"`v` must have shape {self.vnC} (or be a 3-tuple of such arrays); provided: {a.shape}.")
            cols.append(np.array(a, dtype=np.float64).ravel(order='F'))        # (a copy: the caller's array stays)
        w = self.scale(len(parts))
        out = []
        for q, a in enumerate(cols):
            wq = None if w is None else w[q * ncell:(q + 1) * ncell]
            if host:
                if wq is not None and not scale_after:
                    a = wq * a
                a3 = a.reshape(self.vnC, order='F')
                for axis, f in enumerate(self.factors):
                    if f is not None:
                        smooth_lines_host(a3, axis, f, self.passes)
                a = a3.ravel(order='F')
                if wq is not None and scale_after:
                    a = wq * a
            else:
                a = _lib.smooth3d(a.reshape(1, ncell), self.vnC, self.factors, self.passes, scale=wq, scale_after=scale_after,
                                  device=self.device if device is None else int(device))[0]
            out.append(a.reshape(self.vnC, order='F'))
        return tuple(out) if three else out[0]

    def sqrt_t(self, v, host=False, device=None):
        """``L^T v = S^p (w * v)``."""
        return self._run(v, False, host, device)

    def sqrt(self, v, host=False, device=None):
        """``L v = w * S^p v``."""
        return self._run(v, True, host, device)

    def apply(self, v, host=False, device=None):
        """``C v = L (L^T v)``."""
        return self.sqrt(self.sqrt_t(v, host=host, device=device), host=host, device=device)


# --------------------------------------------------------------------------
# Property maps
# --------------------------------------------------------------------------
class _Map:
    """A property map: the model's own parameter ``p`` against the conductivity ``sigma`` every computation uses (the six maps of
    the reference, emg3d/maps.py:284-448).  ``forward``: sigma -> p; ``backward``: p -> sigma; ``derivative_chain(gradient,
    mapped)``: a gradient with respect to sigma becomes one with respect to p, IN PLACE (``gradient *= d sigma / d p``).

    ``name`` is what ``Model(mapping=...)`` takes, ``code`` what the device takes (``emg3d_mg_create_vs``, ``emg3d_mg_set_model``:
    the handle forms ``backward(p)`` itself), ``log`` whether ``p`` is a logarithm (any sign is then a valid value)."""
    name = description = None
    code = None
    log = False

    def __repr__(self):
        return f"Map{self.name}: {self.description} <-> conductivity"

    def forward(self, conductivity):
        raise NotImplementedError

    def backward(self, mapped):
        raise NotImplementedError

    def derivative_chain(self, gradient, mapped):
        raise NotImplementedError

    def chain_factor(self, sigma):
        """``d sigma / d p`` from the conductivity itself, by multiplication only -- what the mapped Jacobian products use with
        the conductivity the device holds (``DeviceMG.get_sigma``), so that no transcendental is evaluated a second time."""
        raise NotImplementedError


class MapConductivity(_Map):
    """p = sigma."""
    name, description, code = 'Conductivity', 'conductivity', 0

    def forward(self, conductivity):
        return conductivity

    def backward(self, mapped):
        return mapped

    def derivative_chain(self, gradient, mapped):
        pass

    def chain_factor(self, sigma):
        return np.ones_like(sigma)


class MapResistivity(_Map):
    """p = rho = 1 / sigma; d sigma / d p = -1 / p^2 = -sigma^2."""
    name, description, code = 'Resistivity', 'resistivity', 1

    def forward(self, conductivity):
        return 1.0 / conductivity

    def backward(self, mapped):
        return 1.0 / mapped

    def derivative_chain(self, gradient, mapped):
        gradient *= -self.backward(mapped) ** 2

    def chain_factor(self, sigma):
        return -(sigma * sigma)


class MapLgConductivity(_Map):
    """p = log10(sigma); d sigma / d p = sigma ln 10."""
    name, description, code, log = 'LgConductivity', 'log_10(conductivity)', 2, True

    def forward(self, conductivity):
        return np.log10(conductivity)

    def backward(self, mapped):
        return 10 ** mapped

    def derivative_chain(self, gradient, mapped):
        gradient *= self.backward(mapped) * np.log(10)

    def chain_factor(self, sigma):
        return sigma * np.log(10)


class MapLnConductivity(_Map):
    """p = ln(sigma); d sigma / d p = sigma."""
    name, description, code, log = 'LnConductivity', 'log_e(conductivity)', 3, True

    def forward(self, conductivity):
        return np.log(conductivity)

    def backward(self, mapped):
        return np.exp(mapped)

    def derivative_chain(self, gradient, mapped):
        gradient *= self.backward(mapped)

    def chain_factor(self, sigma):
        return sigma.copy()


class MapLgResistivity(_Map):
    """p = log10(rho) = log10(1 / sigma); d sigma / d p = -sigma ln 10."""
    name, description, code, log = 'LgResistivity', 'log_10(resistivity)', 4, True

    def forward(self, conductivity):
        return np.log10(1.0 / conductivity)

    def backward(self, mapped):
        return 10 ** -mapped

    def derivative_chain(self, gradient, mapped):
        gradient *= -self.backward(mapped) * np.log(10)

    def chain_factor(self, sigma):
        return -sigma * np.log(10)


class MapLnResistivity(_Map):
    """p = ln(rho) = ln(1 / sigma); d sigma / d p = -sigma."""
    name, description, code, log = 'LnResistivity', 'log_e(resistivity)', 5, True

    def forward(self, conductivity):
        return np.log(1.0 / conductivity)

    def backward(self, mapped):
        return np.exp(-mapped)

    def derivative_chain(self, gradient, mapped):
        gradient *= -self.backward(mapped)

    def chain_factor(self, sigma):
        return -sigma


MAPS = {m.name: m for m in (MapConductivity, MapResistivity, MapLgConductivity, MapLnConductivity, MapLgResistivity,
                            MapLnResistivity)}
