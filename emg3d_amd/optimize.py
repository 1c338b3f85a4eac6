"""Misfit and adjoint-state gradient of ONE (source, frequency) pair on its computational grid -- what
``emg3d.optimize.misfit`` / ``gradient`` (reference emg3d/optimize.py:36-217) and ``Simulation._get_rfield`` /
``_get_bfields`` (emg3d/simulations.py:1131-1213) compute per pair, without the ``Simulation`` / ``Survey``
containers (xarray; out of scope).  Everything field-sized stays in HBM on ONE handle:

    source (built on the device) -> forward solve -> receiver responses (16 B each come back) -> residuals and
    misfit (host scalars) -> residual source (receivers as sources, built on the device) -> back-propagation solve
    -> gradient kernel (-Re(lambda E s mu_0), edges -> cells) -> nC doubles come back.

``Jacobian`` keeps that handle open and gives the two products with the sensitivity matrix ``J = d(data) / d(conductivity)``
of the pair, ``J v`` and ``J^T w``, one multigrid solve each on the operator the forward solve has set up (the reference
v0.17.0 has the gradient only).

``survey_gradient`` sums the gradient over the (source, frequency) pairs of a survey: batched forward and back-propagation solves
on one handle per dtype, the sum over the sources formed on the device (``DeviceMG.grad_acc_add``).  ``SurveyJacobian`` keeps those
handles and the forward fields of ALL pairs in HBM and gives ``J v``, ``J^T w`` and the Gauss-Newton product ``J^T W J v`` of the
survey, every solve batched over the sources.  ``model_gradient(...,
model_grid=)`` maps the gradient to the model grid as the reference does (``maps.grid2grid(grid, -grad, model_grid,
'cubic')``, optimize.py:201-211) and applies the chain rule there; ``method='transpose'`` and ``SurveyJacobian(model_grid=)`` give the
exact derivative with respect to the cells of a model grid instead (the transpose of ``Model.interpolate2grid``'s volume averaging,
applied to the accumulators in HBM).

An inversion keeps a ``Jacobian`` / ``SurveyJacobian`` (or the ``FrequencyHandles`` of ``survey_gradient(handles=)``) open for its
whole life: ``set_model`` presents the next model -- in any of the six property maps -- to the open handles, and ``mapped=True``
gives the products in the model's own parameter.

What the four entry points share is written once: the argument checks (``_check_arguments``), the receivers (``_receivers``), the
residual / adjoint source of one system (``_adjoint_source``, the reference's rule included), the flags of a short chunk
(``_first``) and, for the two Jacobians, ``_JacobianBase``; the per-dtype handles of the survey-level entry points, re-targeted
from frequency to frequency, are a ``solver.FrequencyHandles`` (``DeviceMG.retarget``) -- for ``SurveyJacobian`` one per distinct
computational grid, a ``solver.GridHandles``.
"""
import contextlib
import time

import numpy as np

from . import _lib, fields, maps, meshes, models, solver


def misfit(synthetic, observed, weights):
    """Weighted least-squares data misfit ``sum(w |syn - obs|^2) / 2`` and the residual (reference
    emg3d/optimize.py:100-111)."""
    residual = np.asarray(synthetic) - np.asarray(observed)
    # (the reference sums xarray DataArrays, which skip NaN entries -- receivers outside the grid or missing data)
    return float(np.nansum(weights * (residual.conj() * residual)).real / 2), residual


def _check_arguments(who, model, adjoint, electric=True, interpolation=None, krylov=None, count=None):
    """The argument checks of ``gradient`` / ``survey_gradient`` (``who='Gradient'``: isotropic models) and of the two Jacobians
    (``who='Jacobian'``: ``interpolation`` of the receivers; magnetic receivers with the exact adjoint only).  ``krylov``: the
    start of the message that refuses ``sslsolver`` (None: not asked for); ``count = (name, value)``: ``batch`` resp. ``nvec``."""
    if who == 'Jacobian' and interpolation not in ('linear', 'cubic'):
        raise ValueError(f"`receiver_interpolation` must be 'linear' or 'cubic'; provided: {interpolation!r}.")
    if adjoint not in ('reference', 'exact'):
        raise ValueError(f"`adjoint` must be 'reference' or 'exact'; provided: {adjoint!r}.")
    if who == 'Jacobian' and not electric and adjoint != 'exact':
        raise NotImplementedError(f"{who}: magnetic receivers are implemented with adjoint='exact' only (the reference's "
                                  "rule, loop sources, is not).")
    if who == 'Gradient' and getattr(model, 'case', 0) != 0:
        raise NotImplementedError(f"{who} only implemented for isotropic models.")
    if getattr(model, 'mu_r', None) is not None or getattr(model, 'epsilon_r', None) is not None:
        raise NotImplementedError(f"{who} not implemented for el. permittivity / magn. permeability.")
    if krylov:
        raise NotImplementedError(f"{krylov}; Krylov solvers are not implemented.")
    if count is not None and (int(count[1]) != count[1] or not 1 <= int(count[1]) <= 64):
        raise ValueError(f"`{count[0]}` must be an integer from 1 to 64; provided: {count[1]!r}.")


def _receivers(rec):
    """``(n_rec, rec)`` with the five entries of ``rec = (x, y, z, azimuth, dip)`` as float64 arrays broadcast to ``n_rec``."""
    n = fields._receiver_args(rec)[0]               # (refuses a `rec` of another form)
    return n, tuple(np.broadcast_to(np.asarray(c, dtype=np.float64), (n,)) for c in rec)


def _first(n, nb):
    """``nb`` int32 flags, the first ``n`` set: the systems of a chunk on a handle that carries ``nb``."""
    f = np.zeros(nb, dtype=np.int32)
    f[:n] = 1
    return f


def _each(got):
    """The arrays a ``DeviceMG.grad_acc_get*`` call returned: the one, or the three of ``components=True``."""
    return got if isinstance(got, tuple) else (got,)


def _adjoint_source(dev, rec, smu0, cw, *, method, exact, electric):
    """Residual / adjoint source of the selected system of ``dev`` from ``cw = conj(weights * residual)`` (resp. ``conj(w)``; NaN
    already replaced by 0), one value per receiver.  Returns whether a source was set -- if not, the source is left as it was.

    ``exact`` or ``method='linear'``: ``P^T cw`` with the exact transpose of the receiver operator the data came through (one
    ``set_receiver_adjoint``).  Otherwise the reference's rule (simulations.py:1181-1197): every receiver with a datum becomes a
    1 m dipole source of strength ``cw / s mu_0``; magnetic receivers: a loop source, ``/ s mu_0`` once more."""
    if exact or method == 'linear':
        if np.any(cw != 0):
            dev.set_receiver_adjoint(rec, cw, method=method, magnetic=not electric, smu0=smu0)
            return True
        return False
    done = False
    for k in range(len(cw)):
        strength = cw[k] / smu0 if electric else cw[k] / smu0 / smu0
        if strength == 0:
            continue
        dev.set_source([c[k] for c in rec], smu0, strength=strength, accumulate=done, electric=electric)
        done = True
    return done


def gradient(grid, model, src, freq, rec, observed, weights=None, strength=0, device=0, electric=True, adjoint='reference',
             **solver_opts):
    """Misfit and adjoint-state gradient with respect to conductivity for one source and frequency (isotropic
    models without ``epsilon_r`` / ``mu_r``: the reference's limitations, optimize.py:160-170).  ``electric=False``:
    magnetic receivers -- the data are responses of ``H = get_h_field(E)``, the residual sources magnetic point dipoles
    (square loops) with one more division by ``s mu_0`` (simulations.py:1190-1197).

    ``rec = (x, y, z, azimuth, dip)`` point receivers, ``observed`` their data, ``weights`` the data weights
    (default 1).  Returns ``(misfit, grad, info)``: ``grad`` has shape ``grid.vnC`` (Equation (10) of Plessix &
    Mulder 2008 on the computational grid, optimize.py:176-199; NaN receivers are skipped as in
    simulations.py:1181-1183), ``info`` holds the synthetic data and the two solver info dicts.

    SIGN AND CHAIN RULE: ``grad`` is the reference's ``gradient_model`` BEFORE its last two steps, i.e. the sum
    ``grad_x + grad_y + grad_z`` of optimize.py:199.  The reference then maps ``-grad`` to the model grid
    (``maps.grid2grid``, optimize.py:202-211) and applies the property map's ``derivative_chain`` (optimize.py:214):
    the derivative of the misfit with respect to CONDUCTIVITY on this grid is ``-grad`` (what the finite-difference check
    of tests/test_gpu_gradient.py compares with); for a model in another property (resistivity, log-conductivity) the
    caller applies that map's chain factor, as the reference does.  ``model_gradient()`` below returns that quantity.

    ``adjoint='reference'`` (default): the residual source follows the reference's rule, every receiver a 1 m dipole (or loop)
    SOURCE -- which is not the transpose of the cubic-spline interpolation the data come through, so ``-grad`` is the
    derivative of the misfit only approximately.  ``adjoint='exact'``: one ``DeviceMG.set_receiver_adjoint(rec, conj(weights *
    residual), method='cubic')`` builds ``P^T conj(W r)`` with the exact transpose of the receiver operator (electric or
    magnetic): ``-grad`` is then the derivative of the misfit to the accuracy of the two solves."""
    _check_arguments('Gradient', model, adjoint)
    observed = np.asarray(observed)
    n = observed.size
    weights = np.ones(n) if weights is None else np.broadcast_to(np.asarray(weights), (n,))
    sfield = fields.SourceField(grid, freq=freq)
    smu0 = sfield.smu0
    opts = dict(solver_opts)
    opts.pop('return_info', None)
    # (sigma, V) handle: eta with VolumeModel's rounding, i.e. the fields of solver.solve() bit for bit
    parts = models.model_parts(grid, model, raw=True)
    with solver.DeviceMG.from_model_parts(grid, *parts, smu0=smu0, device=device, map_code=parts.map_code) as dev:
        # forward field (stays on the device)
        _, finfo = solver.solve(grid, None, sfield, handle=dev, return_info=True, source=(src, strength),
                                download=False, **opts)
        synthetic = dev.get_receiver_response(rec) if electric else dev.get_receiver_response(rec, magnetic=True, smu0=smu0)
        phi, residual = misfit(synthetic, observed, weights)
        dev.vec_alloc(1)
        dev.vec_copy(0, dev.EFIELD)                         # keep the forward field
        # residual source (receivers without a datum, NaN, are skipped)
        rec = [np.broadcast_to(np.asarray(c, dtype=np.float64), (n,)) for c in rec]
        cw = np.conj(weights * residual)
        if not _adjoint_source(dev, rec, smu0, np.where(np.isnan(cw), 0, cw), method='cubic', exact=adjoint == 'exact',
                               electric=electric):
            return phi, np.zeros(grid.vnC, order='F'), dict(synthetic=synthetic, forward=finfo, backward=None)
        rfield = fields.SourceField(grid, freq=freq)
        _, binfo = solver.solve(grid, None, rfield, handle=dev, return_info=True, source='resident',
                                download=False, **opts)
        grad = dev.gradient(0, smu0).reshape(grid.vnC, order='F')
    return phi, grad, dict(synthetic=synthetic, forward=finfo, backward=binfo)


def _check_handles(handles, grid, nsys):
    """``survey_gradient(handles=)``: the caller's ``FrequencyHandles`` must be made for this grid, ``nsys`` systems and one
    batched vector."""
    if not isinstance(handles, solver.FrequencyHandles):
        raise TypeError(f"`handles` must be a solver.FrequencyHandles; provided: {type(handles).__name__}.")
    hg = handles.grid
    same = tuple(hg.vnC) == tuple(grid.vnC) and np.array_equal(hg.origin, grid.origin) and \
        all(np.array_equal(a, b) for a, b in zip(hg.h, grid.h))
    if not same:
        raise ValueError("survey_gradient: `handles` were made for another grid.")
    if handles.nsys != nsys or handles.bvecs != 1:
        raise ValueError(f"survey_gradient: `handles` must be made with nsys=min(batch, n_src)={nsys} and bvecs=1; "
                         f"they have nsys={handles.nsys}, bvecs={handles.bvecs}.")


def _sum_survey(partials, misfits, vnC):
    """The defined order of the survey sums: ``grad = ((0 + G_0) + G_1) + ...`` over the frequencies as given, ``phi`` the
    sequential sum of ``misfits[i_src, i_freq]`` with the frequency as the outer and the source as the inner loop."""
    grad = np.zeros(vnC, order='F')
    phi = 0.0
    misfits = np.asarray(misfits)
    for j, g in enumerate(partials):
        grad = grad + np.asarray(g).reshape(vnC, order='F')
        for i in range(misfits.shape[0]):
            phi = phi + float(misfits[i, j])
    return phi, grad


def survey_gradient(grid, model, sources, freqs, rec, observed, weights=None, strength=0, device=0, electric=True,
                    adjoint='reference', batch=8, handles=None, **solver_opts):
    """Misfit and adjoint-state gradient of a SURVEY -- every source of ``sources`` at every frequency of ``freqs`` -- on the
    computational grid: what the reference's ``simulation.gradient`` (emg3d/optimize.py:115-217) sums over its (source, frequency)
    pairs, i.e. the sum of ``gradient()`` over the pairs, without a handle, a hierarchy and an ``nC``-sized download per pair.

    ``observed[i_src, i_freq, i_rec]`` are the data (NaN: no datum), ``weights`` broadcastable to that shape (default 1);
    ``rec``, ``strength``, ``electric``, ``adjoint``, the model limits and the ``solver_opts`` (multigrid only) are those of
    ``gradient()``.  Frequencies < 0 are Laplace-domain values and may be mixed with frequencies; their data are real.

    One handle per dtype carries ``min(batch, n_src)`` systems and is re-targeted from frequency to frequency
    (``FrequencyHandles``).  Per frequency the sources go through in chunks of that size (a shorter last chunk with the surplus
    systems frozen): batched forward solve, data per system, ``misfit()`` per pair on the host, the forward fields parked with one
    ``bvec_copy``, the residual source of every system built as ``gradient()`` builds it, batched back-propagation solve, then ONE
    ``grad_acc_add`` adds the chunk's gradients on the device.  A pair without a usable datum gets no adjoint solve (its
    ``backward`` info is None).  Nothing field-sized crosses PCIe; one ``nC``-sized array comes back per frequency.

    SUMMATION ORDER (part of the contract): ``G_f``, the gradient of frequency ``f``, is the sequential sum over the sources in
    ascending order starting from zero, formed by the kernel; ``grad`` is the sequential sum of the ``G_f`` in the order of
    ``freqs`` starting from zeros, formed on the host; ``phi`` is the sum of the per-pair misfits in the same order (frequency
    outer, source inner).  The results do not depend on ``batch``, bit for bit.

    Returns ``(phi, grad, info)``: ``grad`` (shape ``grid.vnC``) is the sum over the pairs of ``gradient()``'s ``grad``, in its
    sign convention -- ``model_gradient(grid, model, grad, model_grid)`` maps it to the model grid unchanged.  ``info``:
    ``synthetic`` ``(n_src, n_freq, n_rec)``, ``misfit`` ``(n_src, n_freq)``, ``partial`` the ``G_f`` with shape ``(n_freq,) +
    vnC`` (F-ordered; the unit of exchange of ``shard.gather_survey_gradient``), ``forward[i][j]`` / ``backward[i][j]`` the solver
    info dicts, ``phases`` host seconds spent in the forward solves, the data, the adjoint sources, the backward solves and the
    accumulation.

    ``handles``: a ``solver.FrequencyHandles`` of the caller's, made on ``grid`` with ``nsys=min(batch, n_src)`` and ``bvecs=1``
    (``ValueError`` otherwise) -- it is used and left open, for the next call after a ``handles.set_model(...)``: the loop of an
    inversion then keeps hierarchies, work buffers and launch graphs.  The handles hold the model; ``model`` must be the one they
    were last given.  The results are those of a call without ``handles``, bit for bit."""
    _check_arguments('Gradient', model, adjoint, count=('batch', batch), krylov=solver_opts.get('sslsolver')
                     and "survey_gradient: resident sources are solved by multigrid only")
    nrec, rec = _receivers(rec)
    sources = list(sources)
    freqs = [float(f) for f in freqs]
    ns, nf = len(sources), len(freqs)
    if ns < 1:
        raise ValueError("survey_gradient: no sources.")
    observed = np.asarray(observed)
    if observed.shape != (ns, nf, nrec):
        raise ValueError(f"`observed` must have shape (n_src, n_freq, n_rec) = {(ns, nf, nrec)}; provided: {observed.shape}.")
    try:
        weights = np.ones(observed.shape) if weights is None else np.broadcast_to(np.asarray(weights), observed.shape)
    except ValueError:
        raise ValueError(f"`weights` must be broadcastable to the shape of `observed` {observed.shape}; "
                         f"provided: {np.shape(weights)}.") from None
    specs = [fields.FrequencySpec(f) for f in freqs]
    opts = {k: v for k, v in solver_opts.items() if k not in ('return_info', 'sslsolver')}
    vnC = tuple(int(n) for n in grid.vnC)
    nb = min(int(batch), ns)
    if handles is not None:
        _check_handles(handles, grid, nb)
    cplx = any(sp.dtype.kind == 'c' for sp in specs)
    synthetic = np.full((ns, nf, nrec), np.nan, dtype=np.complex128 if cplx else np.float64)
    misfits = np.zeros((ns, nf))
    partial = np.zeros((nf,) + vnC[::-1]).transpose(0, 3, 2, 1)         # (n_freq,) + vnC, every G_f F-ordered
    finfo = [[None] * nf for _ in range(ns)]
    binfo = [[None] * nf for _ in range(ns)]
    phases = dict(forward=0.0, data=0.0, adjoint_sources=0.0, backward=0.0, accumulate=0.0)

    def lap(name, t0):
        t1 = time.perf_counter()
        phases[name] += t1 - t0
        return t1

    if handles is None:
        own = handles = solver.FrequencyHandles(grid, models.model_parts(grid, model, raw=True), device, nsys=nb, bvecs=1)
    else:
        own = contextlib.nullcontext()
    with own:
        for j, spec in enumerate(specs):
            smu0 = spec.smu0
            dev = handles.target(spec)
            real = spec.dtype.kind != 'c'
            dev.grad_acc_reset()
            for i0 in range(0, ns, nb):
                n = min(nb, ns - i0)
                t = time.perf_counter()
                # 1. forward solve of the chunk's sources, built in HBM
                for b in range(n):
                    dev.select(b)
                    dev.set_source(sources[i0 + b], smu0, strength=strength)
                _, infos = solver.solve_sources(grid, None, None, freqs[j], handle=dev, resident=n, download=False, **opts)
                t = lap('forward', t)
                # 2. + 3. data and misfit per pair
                residuals = []
                for b in range(n):
                    finfo[i0 + b][j] = infos[b]
                    dev.select(b)
                    syn = dev.get_receiver_response(rec) if electric else dev.get_receiver_response(rec, magnetic=True, smu0=smu0)
                    obs = observed[i0 + b, j].real if real else observed[i0 + b, j]
                    synthetic[i0 + b, j] = syn
                    misfits[i0 + b, j], r = misfit(syn, obs, weights[i0 + b, j])
                    residuals.append(r)
                t = lap('data', t)
                # 4. park the forward fields of the chunk (the solve has left all but the last system to finish frozen)
                dev.set_mask(_first(n, nb))
                dev.bvec_copy(0, dev.EFIELD)
                # 5. residual sources, per system exactly as gradient() builds them
                use = _first(0, nb)
                for b in range(n):
                    dev.select(b)
                    cw = np.conj(weights[i0 + b, j] * residuals[b])
                    if _adjoint_source(dev, rec, smu0, np.where(np.isnan(cw), 0, cw), method='cubic', exact=adjoint == 'exact',
                                       electric=electric):
                        use[b] = 1
                    else:
                        dev.vec_scale(dev.SFIELD, 0.0)          # no usable datum: a zero source, frozen by the solve
                t = lap('adjoint_sources', t)
                if not use.any():
                    continue
                # 6. back-propagation solve of the chunk
                _, infos = solver.solve_sources(grid, None, None, freqs[j], handle=dev, resident=n, download=False, **opts)
                for b in range(n):
                    if use[b]:
                        binfo[i0 + b][j] = infos[b]
                t = lap('backward', t)
                # 7. G_f += the chunk's gradients, in system order
                dev.grad_acc_add(0, smu0, use)
                t = lap('accumulate', t)
            t = time.perf_counter()
            partial[j] = dev.grad_acc_get().reshape(vnC, order='F')
            lap('accumulate', t)
    phi, grad = _sum_survey(partial, misfits, vnC)
    return phi, grad, dict(synthetic=synthetic, misfit=misfits, partial=partial, forward=finfo, backward=binfo, phases=phases)


def model_gradient(grid, model, grad, model_grid=None, method='cubic'):
    """d(misfit) / d(model property) from ``gradient()``'s ``grad`` (on the computational grid ``grid``): the reference's
    last steps (optimize.py:201-214): the sign, the mapping to the model grid, then the chain rule of the model's property
    map -- conductivity: identity; resistivity rho: d sigma / d rho = -1 / rho^2; the four logarithmic maps: their
    ``derivative_chain`` (``maps.MapLgConductivity`` ...: ``sigma ln 10``, ``sigma``, ``-sigma ln 10``, ``-sigma`` with ``sigma =
    backward(p)`` on the host).

    ``model_grid=None``: ``model`` lives on ``grid`` (the reference's ``gridding='same'``), nothing is regridded.
    Otherwise ``model`` lives on ``model_grid``: ``-grad`` is mapped there with ``maps.grid2grid(grid, -grad, model_grid,
    method='cubic')`` and the chain rule takes the property on ``model_grid``.

    ``method='transpose'`` (needs ``model_grid``): the exact derivative with respect to the model cells instead, for a model that
    reaches ``grid`` through ``model.interpolate2grid(model_grid, grid)`` (volume averaging, in ``log10`` for ``Conductivity`` /
    ``Resistivity``): ``Q (.) A^T (F (.) -grad)`` with ``maps.volume_average_adjoint`` and ``maps.regrid_factors`` -- the
    transpose of what ``SurveyJacobian(model_grid=).jvec`` applies, which the cubic interpolation of the reference is not."""
    if method not in ('cubic', 'transpose'):
        raise ValueError(f"`method` must be 'cubic' or 'transpose'; provided: {method!r}.")
    if method == 'transpose':
        if model_grid is None:
            raise ValueError("model_gradient: method='transpose' needs `model_grid` (the grid `model` lives on).")
        if model.case != 0:
            raise NotImplementedError("model_gradient: `grad` is the sum over the directions; method='transpose' takes isotropic "
                                      "models (SurveyJacobian(model_grid=) gives the directions of an anisotropic one).")
        cmodel = model.interpolate2grid(model_grid, grid)
        F, Q = maps.regrid_factors(model, (cmodel.conductivity('property_x'),) * 3)
        vol = grid.cell_volumes.reshape(grid.vnC, order='F')
        y = F[0] * -np.asarray(grad, dtype=np.float64).reshape(grid.vnC, order='F')
        return Q[0] * maps.volume_average_adjoint(model_grid.nodes_x, model_grid.nodes_y, model_grid.nodes_z, grid.nodes_x,
                                                  grid.nodes_y, grid.nodes_z, y, vol)
    out = -np.asarray(grad)
    vnC = grid.vnC
    if model_grid is not None:
        out = maps.grid2grid(grid, out, model_grid, method='cubic')
        vnC = model_grid.vnC
    mapping = getattr(model, 'mapping', 'Resistivity')
    if mapping == 'Conductivity':
        return out
    if mapping == 'Resistivity':
        rho = np.asarray(model.property_x).reshape(vnC, order='F')
        return out * (-1.0 / rho ** 2)
    # the logarithmic maps: the reference's statement (optimize.py:214), the chain factor from the mapped values on the host
    out = np.array(out, dtype=np.float64, order='F')
    model.map.derivative_chain(out, np.broadcast_to(np.asarray(model.property_x), vnC))
    return out


def _mapped(mapped):
    if not isinstance(mapped, (bool, np.bool_)):
        raise TypeError(f"`mapped` must be True or False; provided: {mapped!r}.")
    return bool(mapped)


def _perturbations(v, vnC):
    """Conductivity perturbations on a grid of ``vnC`` cells, as ``Jacobian.jvec`` and ``SurveyJacobian.jvec`` take them
    -> (list of (vx, vy, vz) with F-raveled float64 arrays or None, single)"""
    dirs = list(v) if isinstance(v, (tuple, list)) and len(v) == 3 and not np.isscalar(v[0]) else None
    if isinstance(v, (tuple, list)) and dirs is None:
        raise ValueError("`v` must be an array of shape grid.vnC (or (k,) + grid.vnC), or a 3-tuple (v_x, v_y, v_z) of them.")
    same = dirs is None
    arrs = [np.asarray(v)] * 3 if same else [None if d is None else np.asarray(d) for d in dirs]
    if all(a is None for a in arrs):
        raise ValueError("`v`: at least one of (v_x, v_y, v_z) must be given.")
    nd = {a.ndim for a in arrs if a is not None}
    for a in arrs:
        if a is None:
            continue
        if np.iscomplexobj(a):
            raise TypeError("`v` must be real (a conductivity perturbation).")
        if a.ndim not in (3, 4) or a.shape[-3:] != vnC or len(nd) != 1:
            raise ValueError(f"`v` must have shape {vnC} or (k,) + {vnC}; provided: {a.shape}.")
    single = nd == {3}
    k = 1 if single else {a.shape[0] for a in arrs if a is not None}
    if not single:
        if len(k) != 1 or min(k) < 1:
            raise ValueError("`v`: (v_x, v_y, v_z) must hold the same number of vectors (at least one).")
        k = k.pop()

    def flat(a, i):
        return np.ascontiguousarray((a if single else a[i]).astype(np.float64, copy=False).ravel(order='F'))
    out = []
    for i in range(k):
        if same:
            f = flat(arrs[0], i)
            out.append((f, f, f))
        else:
            out.append(tuple(None if a is None else flat(a, i) for a in arrs))
    return out, single


def _parked_slots(grid_index, dtypes, n_chunks):
    """Where ``SurveyJacobian`` parks its forward fields.  A handle is a (distinct grid, dtype) pair, ``(grid_index[j],
    dtypes[j].str)`` for frequency ``j``; every frequency owns ``n_chunks`` consecutive batched vectors of its handle.  Returns
    ``(slot, nslots, first)``: ``slot[j]`` the first vector of frequency ``j``, numbered per handle in the order of the
    frequencies; ``nslots[handle]`` the vectors the handle needs; ``first[handle]`` the first frequency on it."""
    slot, nslots, first = {}, {}, {}
    for j, (k, dtype) in enumerate(zip(grid_index, dtypes)):
        key = (int(k), np.dtype(dtype).str)
        first.setdefault(key, j)
        slot[j] = nslots.get(key, 0)
        nslots[key] = slot[j] + int(n_chunks)
    return slot, nslots, first


def _parked_bytes(nslots, nb, nE):
    """The bytes of the parked forward fields: the sum over the handles of ``nslots`` (``_parked_slots``) of ``slots * nb *
    nE[k] * itemsize`` -- ``nb`` systems per batched vector, ``nE[k]`` the edges of distinct grid ``k``."""
    return sum(int(n) * int(nb) * int(nE[k]) * np.dtype(dtype).itemsize for (k, dtype), n in nslots.items())


class _JacobianBase:
    """What ``Jacobian`` and ``SurveyJacobian`` share: the ``with`` protocol, the test for the open state (``self._held``: the
    handle resp. the handles, None when closed) and the two steps every product is made of."""

    def __enter__(self):
        return self.open()

    def __exit__(self, *exc):
        self.close()

    def _require_open(self):
        if self._held is None:
            raise RuntimeError(self._closed)
        return self._held

    # ---- products in the model's own property (``mapped=True``) -----------------------------------------------------------
    # With sigma_c = backward(p_c) per component and D_c = d sigma_c / d p_c, the Jacobian with respect to p is J_m = J D: a
    # perturbation of p is multiplied by D_c before it becomes the right-hand side, the cell results of J^T are multiplied by
    # D_c on the way out (``components=False`` on an anisotropic model: the sum of the three D_c g_c).  D is formed on the host
    # from the conductivity the DEVICE holds (``DeviceMG.get_sigma``) by multiplication only (``maps._Map.chain_factor``): host
    # and device agree on sigma bit for bit, no transcendental runs a second time.  Formed at the first mapped product after
    # ``open()`` / ``set_model()``; ``mapped=False`` (default) never asks for it.
    _chain = None

    def _chain_factors(self):
        if self._chain is None:
            dev = next(iter(self._held)) if isinstance(self._held, solver.GridHandles) else self._held
            fmap = self.model.map
            dx = fmap.chain_factor(dev.get_sigma(0))
            dy = fmap.chain_factor(dev.get_sigma(1)) if self.model.case in (1, 3) else dx
            dz = fmap.chain_factor(dev.get_sigma(2)) if self.model.case in (2, 3) else dx
            self._chain = (dx, dy, dz)
        return self._chain

    def _to_sigma(self, vec):
        """(v_x, v_y, v_z), F-raveled perturbations of p (entries may be None) -> of sigma."""
        return tuple(None if v is None else v * d.ravel(order='F') for v, d in zip(vec, self._chain_factors()))

    def _from_sigma(self, g3, components):
        """The three terms (g_x, g_y, g_z) with respect to sigma -- or, for an isotropic model, their sum -> with respect to p."""
        d = self._chain_factors()
        if not isinstance(g3, tuple):
            return d[0] * g3
        out = tuple(dc * g for dc, g in zip(d, g3))
        return out if components else (out[0] + out[1]) + out[2]

    def _solve(self, dev, freq, n, grid=None):
        """Solve the systems 0 .. n-1 of the handle (at ``freq``) for the sources they hold; the fields stay in HBM.  ``grid``: the
        handle's own (default: ``self.grid``)."""
        _, infos = solver.solve_sources(self.grid if grid is None else grid, None, None, freq, handle=dev, resident=n,
                                        download=False, **self._opts)
        return infos

    def _data(self, dev, smu0):
        """Receiver responses of the selected system's field."""
        if self.electric:
            return dev.get_receiver_response(self.rec, method=self.receiver_interpolation)
        return dev.get_receiver_response(self.rec, magnetic=True, smu0=smu0, method=self.receiver_interpolation)


class Jacobian(_JacobianBase):
    """Products with the sensitivity matrix ``J = d(data) / d(conductivity)`` of ONE (source, frequency) pair on its
    computational grid, on one device handle::

        with Jacobian(grid, model, src, freq, rec, nvec=4, tol=1e-8, ...) as jac:
            jac.synthetic             # data of the forward field, (n_rec,)
            dd = jac.jvec(v)          # (nx, ny, nz) -> (n_rec,) complex;  (k, nx, ny, nz) -> (k, n_rec)
            g = jac.jtvec(w)          # (n_rec,) -> (nx, ny, nz) float64;  (k, n_rec) -> (k, nx, ny, nz)
            gx, gy, gz = jac.jtvec(w, components=True)

    The forward solve runs once at entry (source built in HBM), its field ``E`` is parked in a workspace vector; every product
    costs one more multigrid solve with the hierarchy, coarse models and line factorisations already there.  With the system
    ``A e = s`` of ``core.amat_x`` (the sigma-term of an edge is ``-1/4 (eta of its four cells) e``, ``eta = s mu_0 sigma V``):

    * ``jvec(v)``: ``A de = s mu_0 C(v) E``, ``C(v)`` on an edge = 1/4 of the sum of ``V_c v_c`` over its four cells (0 on the PEC
      boundary), then ``J v = P de`` with the receiver operator ``P``.  ``v`` is a conductivity perturbation on this grid: one
      array perturbs sigma_x = sigma_y = sigma_z together, a 3-tuple ``(v_x, v_y, v_z)`` (entries may be None) the directions
      separately -- for every model case, the operator always carries three eta.  ``mapped=True`` (both products): ``v`` and the
      result are in the model's own property instead (``Model(mapping=...)``: the chain factor per cell, ``_JacobianBase``).
      Regridding stays with the caller (``model_gradient`` shows how).
    * ``jtvec(w) = Re(J^H w)`` (so that ``sum(v * jtvec(w)) == Re sum(conj(w) * jvec(v))``): ``A lam = P^T conj(w)``, then
      ``-sum_c edges2cellaverages_c(-Re(s mu_0 lam E))`` -- the gradient kernel with the sign flipped; ``components=True`` keeps
      the terms of sigma_x, sigma_y, sigma_z apart.  The gradient of ``1/2 sum W |r|^2`` is ``jtvec(W r)``.

    ``receiver_interpolation='linear'`` (default): the data are trilinear interpolations on the trimmed points of
    ``get_receiver_response`` (NaN outside) times the rotation factors, and ``jtvec`` applies the exact transpose: ``jvec`` and
    ``jtvec`` are an adjoint pair to the accuracy of the solves.  NaN receivers are skipped in ``jtvec`` and stay NaN in
    ``jvec``.  ``'cubic'``: ``synthetic`` and ``jvec`` use the cubic-spline receivers of ``get_receiver_response`` (``jvec`` is the
    exact derivative of the data ``gradient()`` fits); see ``jtvec`` for what its transpose is then.

    ``nvec = k > 1``: the handle carries ``k`` systems (``DeviceMG.set_batch``); a product with up to ``k`` vectors runs them through
    the same cycles, each stopping by its own termination test (``solver.solve_sources``), more in groups of ``k`` -- the results
    equal those of one vector at a time bit for bit.  ``solver_opts`` go to the solver (``cycle, semicoarsening, linerelaxation,
    tol, maxit, ordering, verb, ...``; multigrid only).  Models without ``mu_r`` / ``epsilon_r``.

    ``adjoint='exact'``: with ``'cubic'`` receivers ``jtvec`` applies the exact transpose of the cubic-spline receiver operator
    (``DeviceMG.set_receiver_adjoint(method='cubic')``) instead of the reference's rule, and ``jvec`` / ``jtvec`` are an adjoint
    pair; ``'linear'`` is exact either way.  ``electric=False``: magnetic receivers -- the data and ``jvec`` are responses of
    ``H = get_h_field(E)``, the ``jtvec`` source is ``C^T P_faces^T conj(w)``; they need ``adjoint='exact'`` (the reference's
    rule for them, loop sources, is not implemented here), with ``'linear'`` or ``'cubic'`` receivers."""

    def __init__(self, grid, model, src, freq, rec, receiver_interpolation='linear', nvec=1, strength=0, device=0,
                 electric=True, adjoint='reference', **solver_opts):
        _check_arguments('Jacobian', model, adjoint, electric, receiver_interpolation, count=('nvec', nvec),
                         krylov=solver_opts.get('sslsolver') and "Jacobian: the products are multigrid solves")
        self.grid, self.model, self.src, self.freq = grid, model, src, freq
        self.n_rec, self.rec = _receivers(rec)
        self.receiver_interpolation = receiver_interpolation
        self.adjoint, self.electric = adjoint, bool(electric)
        self.nvec, self.strength, self.device = int(nvec), strength, device
        self._opts = {k: v for k, v in solver_opts.items() if k not in ('return_info', 'sslsolver')}
        self._spec = fields.FrequencySpec(freq)
        self._vnC = tuple(int(n) for n in grid.vnC)
        self._held = None
        self.synthetic = self.forward_info = self.info = None

    # ---- handle -------------------------------------------------------------------------------------------------------
    def open(self):
        """Create the handle, run the forward solve (system 0; the other systems of a batch frozen), extract the data and
        park the forward field."""
        if self._held is not None:
            return self
        smu0 = self._spec.smu0
        parts = models.model_parts(self.grid, self.model, raw=True)
        dev = solver.DeviceMG.from_model_parts(self.grid, *parts, smu0=smu0, device=self.device, map_code=parts.map_code)
        try:
            if self.nvec > 1:
                dev.set_batch(self.nvec)
            dev.vec_alloc(1)
            self._forward(dev)
        except BaseException:
            dev.close()
            raise
        self._held = dev
        return self

    def _forward(self, dev):
        smu0 = self._spec.smu0
        dev.select(0)
        dev.set_source(self.src, smu0, strength=self.strength)
        self.forward_info = self._solve(dev, self.freq, 1)[0]
        dev.select(0)
        self.synthetic = self._data(dev, smu0)
        dev.vec_copy(0, dev.EFIELD)                     # keep the forward field
        self.info = self._chain = None

    def set_model(self, model):
        """Another model on the same grid, in the same anisotropy case (any property map), on the open handle:
        ``DeviceMG.set_model``, the forward solve again into the parked vector, ``synthetic`` and ``forward_info`` anew -- then
        every product is bit for bit that of a new ``Jacobian`` on ``model``.  Nothing is allocated."""
        dev = self._require_open()
        _check_arguments('Jacobian', model, self.adjoint, self.electric, self.receiver_interpolation)
        dev.set_model(self.grid, model)
        self.model = model
        self._forward(dev)
        return self

    @property
    def device_bytes(self):
        """Device memory of the handle, the parked forward field included."""
        return self._require_open().device_bytes

    def close(self):
        if self._held is not None:
            self._held.close()
            self._held = None

    _closed = "Jacobian: the handle is closed (use it inside its `with` block, or call open())."

    # ---- J v ----------------------------------------------------------------------------------------------------------
    def jvec(self, v, mapped=False):
        """``J v``: the data change per unit of the conductivity perturbation ``v`` (see the class docstring); ``mapped=True``:
        per unit of a perturbation of the model's own property (``_JacobianBase``)."""
        mapped = _mapped(mapped)
        vecs, single = _perturbations(v, self._vnC)
        dev = self._require_open()
        if mapped:
            vecs = [self._to_sigma(vec) for vec in vecs]
        smu0 = self._spec.smu0
        out = np.empty((len(vecs), self.n_rec), dtype=self._spec.dtype)
        infos = []
        for g0 in range(0, len(vecs), self.nvec):
            group = vecs[g0:g0 + self.nvec]
            for b, (vx, vy, vz) in enumerate(group):
                dev.select(b)
                dev.jvec_source(0, smu0, vx, vy, vz)
            infos += self._solve(dev, self.freq, len(group))
            for b in range(len(group)):
                dev.select(b)
                out[g0 + b] = self._data(dev, smu0)
        self.info = infos[0] if single else infos
        return out[0] if single else out

    # ---- J^T w --------------------------------------------------------------------------------------------------------
    def _data_vectors(self, w):
        w = np.asarray(w)
        if w.ndim not in (1, 2) or w.shape[-1] != self.n_rec or w.size == 0:
            raise ValueError(f"`w` must have shape ({self.n_rec},) or (k, {self.n_rec}) -- one value per receiver; "
                             f"provided: {w.shape}.")
        if np.iscomplexobj(w) and self._spec.dtype.kind != 'c':
            raise TypeError("`w` must be real for a Laplace-domain Jacobian.")
        return np.atleast_2d(w).astype(self._spec.dtype), w.ndim == 1

    def _adjoint_source(self, dev, w):
        """Source of the selected system for ``jtvec``: NaN data (receivers outside, missing data) are skipped."""
        if not _adjoint_source(dev, self.rec, self._spec.smu0, np.where(np.isnan(w), 0, np.conj(w)),
                               method=self.receiver_interpolation, exact=self.adjoint == 'exact', electric=self.electric):
            dev.vec_scale(dev.SFIELD, 0.0)

    def jtvec(self, w, components=False, mapped=False):
        """``J^T w = Re(J^H w)``, a real cell array of shape ``grid.vnC`` (F-ordered); ``components=True``: the three terms
        ``(g_x, g_y, g_z)`` that belong to sigma_x, sigma_y, sigma_z (their sum is the default result).  ``mapped=True``: with
        respect to the model's own property (``_JacobianBase``).

        With ``receiver_interpolation='linear'``, or with ``adjoint='exact'``, this is the exact transpose of ``jvec`` (on the
        12 x 10 x 8 grid below the cubic pair then agrees as well as the linear one, to the accuracy of the solves; the gradient
        of ``1/2 sum W |r|^2`` is ``jtvec(W r) == -gradient(..., adjoint='exact')[1]``).  With ``'cubic'`` and the default
        ``adjoint='reference'`` the right-hand side follows the reference's rule -- every receiver becomes a 1 m dipole SOURCE (emg3d/simulations.py:1171-1213) --, so
        that ``jtvec(weights * residual) == -gradient(...)[1]``; that rule is not the transpose of the cubic-spline
        interpolation which ``jvec`` and the data use, and the two are NOT an adjoint pair: on the 12 x 10 x 8 grid of
        tests/golden/gradient.npz (1.5 Hz, random v and w) ``Re sum(conj(w) J v) = 0.4596`` against ``v . J^T w = 0.1202``, a
        relative gap of 0.74, where the linear pair agrees to 1.9e-8."""
        mapped = _mapped(mapped)
        ws, single = self._data_vectors(w)
        dev = self._require_open()
        smu0 = self._spec.smu0
        outs, infos = [], []
        keep, components = components, components or (mapped and self.model.case != 0)
        for g0 in range(0, len(ws), self.nvec):
            group = ws[g0:g0 + self.nvec]
            for b, wv in enumerate(group):
                dev.select(b)
                self._adjoint_source(dev, wv)
            infos += self._solve(dev, self.freq, len(group))
            for b in range(len(group)):
                dev.select(b)
                if components:
                    outs.append(tuple(-g.reshape(self._vnC, order='F') for g in dev.gradient(0, smu0, components=True)))
                else:
                    outs.append(-dev.gradient(0, smu0).reshape(self._vnC, order='F'))
        self.info = infos[0] if single else infos
        if mapped:
            outs = [self._from_sigma(o, keep) for o in outs]
            components = keep
        if single:
            return outs[0]
        if components:
            return tuple(np.stack([o[c] for o in outs]) for c in range(3))
        return np.stack(outs)


class SurveyJacobian(_JacobianBase):
    """Products with the sensitivity matrix of a SURVEY -- every source of ``sources`` at every entry of ``freqs`` (values < 0 are
    Laplace-domain, and may be mixed with frequencies) -- on the computational grid: the rows of ``Jacobian(src_i, freq_j)`` for all
    pairs ``(i, j)`` stacked, without a handle, a hierarchy, a forward solve and an ``nC``-sized download per pair::

        with SurveyJacobian(grid, model, sources, freqs, rec, batch=8, tol=1e-8, ...) as sj:
            sj.synthetic                      # (n_src, n_freq, n_rec)
            dd = sj.jvec(v)                   # v: vnC array or (v_x, v_y, v_z)  ->  (n_src, n_freq, n_rec)
            g = sj.jtvec(w)                   # w: (n_src, n_freq, n_rec) -> vnC;  components=True -> (g_x, g_y, g_z)
            hv = sj.gauss_newton(v, weights)  # == sj.jtvec(weights * sj.jvec(v)), bit for bit
            sj.partial                        # the last jtvec's per-frequency sums G_f

    One handle per dtype carries ``min(batch, n_src)`` systems and is re-targeted from entry to entry of ``freqs``
    (``FrequencyHandles``), as in ``survey_gradient``.  ``open()`` solves all pairs forward, the sources in chunks of that size
    (built in HBM), extracts the data and parks the forward fields of every (frequency, chunk) in a batched vector of its own:
    ``n_freq * n_chunks * min(batch, n_src) * nE`` field values stay in HBM (sized and allocated before the first solve; a
    workspace that does not fit raises ``HipLibraryError`` with the bytes needed and free) and never cross PCIe.

    * ``jvec(v)``: per frequency and chunk ONE ``jvec_source_b`` (``s mu_0 C(v) E_b`` for all systems of the chunk), one batched
      solve, the data per system.
    * ``jtvec(w)``: per frequency the accumulator is reset; per chunk ONE ``set_receiver_adjoint_b`` (``adjoint='reference'`` with
      cubic receivers: the per-system ``set_source`` loop of ``Jacobian``), one batched solve, ONE ``grad_acc_add`` (or
      ``grad_acc3_add``) with the chunk's parked fields.  NaN entries of ``w`` count as zero.  A pair whose row is all zero is
      not solved for: its system stays in the batch of its chunk with a zero source, which ``solve_sources`` freezes at entry
      (zero field, no cycle), it is not accumulated (``use = 0``) and its info is ``None``; a chunk whose rows are all zero is
      skipped altogether.  One ``nC``-sized array (three with ``components=True``) comes back per frequency.
    * ``gauss_newton(v, weights)``: both products chunk by chunk -- ``jvec_source_b``, solve, data, ``set_receiver_adjoint_b`` with
      ``conj(weights * data)``, solve, ``grad_acc_add`` -- so that every chunk's forward fields are visited once.  ``weights`` are
      real and broadcast to the data shape; a NaN in ``weights`` or in the data means "no datum".
    * ``sensitivity_diagonal``, ``sensitivity_rows``, ``park_rows``: ``diag(J^H W J)``, the rows of ``J`` on the host, and the same
      rows parked in HBM (a ``RowStore``: ``J C_m J^T``, ``C_m J^T y`` and ``J v`` on the device), from ``n_rec`` resp. ``2 n_rec``
      solves per frequency; see there.

    SUMMATION ORDER (part of the contract): ``G_f`` is the sequential sum of the pairs' gradients (``DeviceMG.gradient`` of the
    pair, i.e. ``-Jacobian.jtvec``) over the sources in ascending order starting from zero, formed by the kernel; the result is
    ``-(((0 + G_0) + G_1) + ...)`` in the order of ``freqs``, formed on the host (``_sum_survey``).  ``partial`` holds the ``G_f``
    with shape ``(n_freq,) + vnC`` (``(3, n_freq) + vnC`` with ``components=True``): what ``shard.combine_survey_gradient`` takes,
    whose result is then ``-jtvec``.  Every system goes through the arithmetic of a solve of its own: all results, cycle counts and
    norms are independent of ``batch``, bit for bit.

    Models, ``rec``, ``receiver_interpolation``, ``adjoint``, ``electric`` and the ``solver_opts`` (multigrid only) are those of
    ``Jacobian`` (tri-axial models included, without ``mu_r`` / ``epsilon_r``; ``electric=False`` needs ``adjoint='exact'``), with
    the defaults ``'cubic'`` and ``'exact'``: the pair ``jvec`` / ``jtvec`` is then an adjoint pair, and ``gauss_newton`` symmetric
    positive semi-definite, to the accuracy of the solves.  ``forward_info[i][j]`` and, after a product, ``info[i][j]`` (the last
    solve of the pair; ``jvec_info`` the J v solve of ``gauss_newton``) are the solver info dicts.

    ``model_grid`` (a ``TensorMesh``; default None: nothing changes): ``model`` lives on ``model_grid`` and ``grid`` is the
    computational grid.  ``open()`` and ``set_model(model_on_model_grid)`` regrid with ``model.interpolate2grid(model_grid, grid)``
    (volume averaging ``A``, in ``log10`` for ``'Conductivity'`` / ``'Resistivity'``); the products are with respect to the MODEL
    cells, in the model's own property: ``jvec(v, mapped=True) = J (F (.) A (Q (.) v))`` with ``v`` of shape ``model_grid.vnC``,
    ``jtvec(w, mapped=True) = Q (.) A^T (F (.) J^T w)`` of that shape (``maps.regrid_factors``; ``A^T`` applied to the accumulators
    on the device, ``DeviceMG.grad_acc_get_model``: one ``nM``-sized array per frequency and direction comes back), ``partial`` the
    per-frequency results on the model grid in the ``G_f`` sign convention.  The two are an adjoint pair as without a model grid.
    ``mapped=False`` (the default) raises ``ValueError`` there: the conductivity on the model grid is not what the solves see.

    A COMPUTATIONAL GRID PER FREQUENCY (the reference's ``gridding='dict'`` with the caller's grids, emg3d/simulations.py:92-117):
    with ``model_grid``, ``grid`` may be a list or tuple with one ``TensorMesh`` per entry of ``freqs``, repeats allowed
    (``ValueError`` without ``model_grid``, for another length or for an entry that is no mesh, before any device call).  Entries
    that are the same object or equal in every width and the origin are one grid (``meshes.same_grid``): ``grids`` holds the mesh
    of every entry, ``grid_index`` its position among the distinct grids in order of first appearance, ``grid`` what the caller
    passed.  There is one handle per distinct (grid, dtype), re-targeted among the entries it serves (``solver.GridHandles``);
    the model is regridded, the factors ``F`` are read back and a ``jvec`` right-hand side is formed once per distinct grid; the
    parked vectors are numbered per handle.  Every product of entry ``j`` is bit for bit that of ``SurveyJacobian(grids[j],
    model, sources, [freqs[j]], rec, model_grid=model_grid, ...)``, the sums over the frequencies are formed on the host in the
    order of ``freqs`` as always, and rows from any grid are model-grid sized: one ``RowStore`` holds them all.  A sequence that
    repeats one grid is the single-mesh call."""

    def __init__(self, grid, model, sources, freqs, rec, batch=8, receiver_interpolation='cubic', adjoint='exact', electric=True,
                 strength=0, device=0, model_grid=None, **solver_opts):
        _check_arguments('Jacobian', model, adjoint, electric, receiver_interpolation, count=('batch', batch),
                         krylov=solver_opts.get('sslsolver') and "SurveyJacobian: the products are multigrid solves")
        self.model_grid = model_grid
        self._check_model_grid(model)
        self.sources = list(sources)
        self.freqs = [float(f) for f in np.atleast_1d(freqs)]
        if len(self.sources) < 1 or len(self.freqs) < 1:
            raise ValueError("SurveyJacobian: no sources or no frequencies.")
        self.grid, self.model = grid, model
        self.n_src, self.n_freq = len(self.sources), len(self.freqs)
        self.grids = meshes.frequency_grids(grid, self.n_freq, model_grid, 'SurveyJacobian')
        self.grid_index = meshes.distinct_grids(self.grids)[1]
        self.n_rec, self.rec = _receivers(rec)
        self.receiver_interpolation = receiver_interpolation
        self.adjoint, self.electric = adjoint, bool(electric)
        self.batch, self.strength, self.device = int(batch), strength, device
        self._opts = {k: v for k, v in solver_opts.items() if k not in ('return_info', 'sslsolver')}
        self._specs = [fields.FrequencySpec(f) for f in self.freqs]
        self._vnC = tuple(int(n) for n in self.grids[0].vnC)    # (the cells of the one grid there is without `model_grid`)
        self._vnM = self._vnC if model_grid is None else tuple(int(n) for n in model_grid.vnC)     # the cells of `v` and `J^T w`
        self._nb = min(self.batch, self.n_src)
        self._chunks = [(i0, min(self._nb, self.n_src - i0)) for i0 in range(0, self.n_src, self._nb)]
        cplx = any(sp.dtype.kind == 'c' for sp in self._specs)
        self.dtype = np.dtype(np.complex128 if cplx else np.float64)
        self._held = None
        self._stores = []           # the row stores of park_rows, closed with the handles
        self.synthetic = self.forward_info = self.info = self.jvec_info = self.partial = None
        self.sensitivity_info = self.sensitivity_partial = self.rows_info = self.rows_info_imag = None

    # ---- the model grid ------------------------------------------------------------------------------------------------
    # With ``model_grid`` the model lives there and reaches ``grid`` through ``model.interpolate2grid(model_grid, grid)``: volume
    # averaging A, in log10 for the two linear maps.  Per direction d sigma_c / d p_m = F A Q with diagonal F (on ``grid``) and Q
    # (on ``model_grid``; ``maps.regrid_factors``), so J_m v = J (F (.) A (Q (.) v)) and J_m^T w = Q (.) A^T (F (.) J^T w).  ``jvec``
    # forms its right-hand side once per product with the device's volume averaging; ``jtvec`` reads the accumulators back through
    # ``grad_acc(3)_get_model`` (k_volume_average_adjoint on the resident tables and factors): model-grid-sized arrays only.
    _regrid_FQ = None
    _no_sigma = ("SurveyJacobian: on a model grid the products are defined in the model's own property only (the conductivity on "
                 "the model grid is not what the solves see); use mapped=True.")

    def _check_model_grid(self, model):
        if self.model_grid is not None and tuple(model.vnC) != tuple(int(n) for n in self.model_grid.vnC):
            raise ValueError(f"SurveyJacobian: `model` must live on `model_grid` {tuple(self.model_grid.vnC)}; it has "
                             f"{tuple(model.vnC)} cells.")

    # With a computational grid per frequency (``grid`` a sequence) all of this holds per DISTINCT grid: the model is regridded to
    # each (``GridHandles.on_grids``), F comes from a handle of that grid, Q from the model alone, and ``jvec`` forms one right-hand
    # side per distinct grid and product.  What comes back is model-grid sized whatever grid a frequency was solved on.

    def _refresh_factors(self, handles):
        """``_regrid_FQ[k]``: the factors of distinct grid ``k``, F from the conductivity one of its handles holds."""
        case = self.model.case
        self._regrid_FQ = []
        for k, member in enumerate(handles.members):
            dev = next(iter(member))
            sx = dev.get_sigma(0)
            sigma = (sx, dev.get_sigma(1) if case in (1, 3) else sx, dev.get_sigma(2) if case in (2, 3) else sx)
            self._regrid_FQ.append(maps.regrid_factors(self.model, sigma))
            handles.set_regrid_factors(k, *self._regrid_FQ[k])

    def _to_grid(self, vec, k):
        """(v_x, v_y, v_z), F-raveled perturbations of p on the model grid (entries may be None) -> of sigma on distinct grid
        ``k``; entries that are the same array with the same factors stay one array."""
        F, Q = self._regrid_FQ[k]
        grid = self._held.distinct[k]
        out, done = [], []
        for c, v in enumerate(vec):
            hit = [r for v0, c0, r in done if v0 is v and F[c0] is F[c] and Q[c0] is Q[c]]
            if v is None or hit:
                out.append(None if v is None else hit[0])
                continue
            vm = np.asfortranarray(Q[c] * v.reshape(self._vnM, order='F'))
            r = np.ascontiguousarray((F[c] * maps.grid2grid(self.model_grid, vm, grid, 'volume')).ravel(order='F'))
            done.append((v, c, r))
            out.append(r)
        return tuple(out)

    def _right_hand_sides(self, vec, mapped):
        """The perturbation of a product as the solves of every distinct grid take it, formed once per distinct grid: ``vecs[k]``
        for ``_sweep``."""
        if not mapped:
            return [vec]
        handles = self._require_open()
        if self.model_grid is None:
            return [self._to_sigma(vec)]
        return [self._to_grid(vec, k) for k in range(len(handles.distinct))]

    def _mapped_or_refuse(self, mapped):
        mapped = _mapped(mapped)
        if self.model_grid is not None and not mapped:
            raise ValueError(self._no_sigma)
        return mapped

    # ---- handles ------------------------------------------------------------------------------------------------------
    def open(self):
        """Create the handles, size and allocate the parked fields, solve all pairs forward (chunk by chunk), extract the data."""
        if self._held is not None:
            return self
        ns, nf, nb = self.n_src, self.n_freq, self._nb
        handles = solver.GridHandles(self.grids, self.model, self.device, nsys=nb, model_grid=self.model_grid)
        self._slot, nslots, first = _parked_slots(self.grid_index, [spec.dtype for spec in self._specs], len(self._chunks))
        try:
            devs = {key: handles.target(j, self._specs[j]) for key, j in first.items()}
            # the parked forward fields: one batched vector per (frequency, chunk), sized and allocated before the first solve
            need = _parked_bytes(nslots, nb, [g.nE for g in handles.distinct])
            mi = _lib.mem_info(self.device)
            free = mi['free'] + mi['pooled_on_device']
            if need >= 0.92 * free:
                raise _lib.HipLibraryError(
                    f"SurveyJacobian: the forward fields of {ns} sources x {nf} frequencies need {need} bytes of device memory, "
                    f"{free} bytes are free; use fewer sources or frequencies per SurveyJacobian (frequency shards).")
            for key, dev in devs.items():
                dev.bvec_alloc(nslots[key])
            if self.model_grid is not None:
                handles.set_model_grid(self.model_grid)
            self._forward(handles)
        except BaseException:
            handles.close()
            raise
        self._held = handles
        return self

    def _forward(self, handles):
        """Solve all pairs forward (chunk by chunk), extract the data, park the fields in their batched vectors."""
        ns, nf, nb = self.n_src, self.n_freq, self._nb
        self.synthetic = np.full((ns, nf, self.n_rec), np.nan, dtype=self.dtype)
        self.forward_info = [[None] * nf for _ in range(ns)]
        for j, spec in enumerate(self._specs):
            dev, smu0 = handles.target(j, spec), spec.smu0
            for c, (i0, n) in enumerate(self._chunks):
                for b in range(n):
                    dev.select(b)
                    dev.set_source(self.sources[i0 + b], smu0, strength=self.strength)
                infos = self._solve(dev, self.freqs[j], n, self.grids[j])
                for b in range(n):
                    self.forward_info[i0 + b][j] = infos[b]
                    dev.select(b)
                    self.synthetic[i0 + b, j] = self._data(dev, smu0)
                # park the chunk's forward fields (the solve has left all but the last system to finish frozen)
                dev.set_mask(_first(n, nb))
                dev.bvec_copy(self._slot[j] + c, dev.EFIELD)
        self.info = self.jvec_info = self.partial = self._chain = None
        self.sensitivity_info = self.sensitivity_partial = self.rows_info = self.rows_info_imag = None
        if self.model_grid is not None:
            self._refresh_factors(handles)

    def set_model(self, model):
        """Another model on the same grid, in the same anisotropy case (any property map), on the open handles -- what an
        inversion does every iteration and every trial step: ``GridHandles.set_model`` (the conductivities, eta, coarse
        models and line factorisations of every handle recomputed in HBM), all pairs solved forward again into the SAME parked
        vectors, ``synthetic`` and ``forward_info`` anew.  Every product is then bit for bit that of a new ``SurveyJacobian`` on
        ``model``; no handle, hierarchy, launch graph or parked vector is created (``device_bytes`` stays).  With ``model_grid``
        the model lives there: it is regridded as ``open()`` does and the regrid factors are refreshed in place."""
        handles = self._require_open()
        _check_arguments('Jacobian', model, self.adjoint, self.electric, self.receiver_interpolation)
        self._check_model_grid(model)
        handles.set_model(model)
        self.model = model
        self._forward(handles)
        return self

    def close(self):
        for store in self._stores:
            store.close()
        self._stores = []
        if self._held is not None:
            self._held.close()
            self._held = None

    _closed = "SurveyJacobian: the handles are closed (use it inside its `with` block, or call open())."

    @property
    def device_bytes(self):
        """Device memory of the handles, parked forward fields and accumulators included."""
        return sum(dev.device_bytes for dev in self._require_open())

    # ---- arguments ----------------------------------------------------------------------------------------------------
    def _perturbation(self, v):
        vecs, single = _perturbations(v, self._vnM)
        if not single:
            raise ValueError(f"`v` must have shape {self._vnM} (or be a 3-tuple of such arrays): one perturbation per product.")
        return vecs[0]

    def _data_array(self, w, name):
        shape = (self.n_src, self.n_freq, self.n_rec)
        w = np.asarray(w)
        if w.shape != shape:
            raise ValueError(f"`{name}` must have shape (n_src, n_freq, n_rec) = {shape}; provided: {w.shape}.")
        if np.iscomplexobj(w):
            for j, spec in enumerate(self._specs):
                if spec.dtype.kind != 'c' and np.any(np.nan_to_num(w[:, j].imag) != 0):
                    raise TypeError(f"`{name}` must be real for the Laplace-domain entries of `freqs`.")
        return w

    def _weights(self, weights):
        shape = (self.n_src, self.n_freq, self.n_rec)
        if weights is None:
            return np.ones(shape)
        if np.iscomplexobj(weights):
            raise TypeError("`weights` must be real.")
        try:
            return np.broadcast_to(np.asarray(weights, dtype=np.float64), shape)
        except ValueError:
            raise ValueError(f"`weights` must be broadcastable to the data shape {shape}; provided: {np.shape(weights)}.") from None

    # ---- the products -------------------------------------------------------------------------------------------------
    def _adjoint_sources(self, dev, smu0, cw, n):
        """Sources of the systems 0 .. n-1 <- P^T cw[b] (an all-zero row: a zero source)."""
        if self.receiver_interpolation == 'linear' or self.adjoint == 'exact':
            rows = np.zeros((self._nb, self.n_rec), dtype=dev.dtype)
            rows[:n] = cw
            dev.set_receiver_adjoint_b(self.rec, rows, _first(n, self._nb), method=self.receiver_interpolation,
                                       magnetic=not self.electric, smu0=smu0)
            return
        # 'cubic' receivers with the reference's rule: per system as Jacobian builds it
        for b in range(n):
            dev.select(b)
            if not _adjoint_source(dev, self.rec, smu0, cw[b], method='cubic', exact=False, electric=self.electric):
                dev.vec_scale(dev.SFIELD, 0.0)

    def _sweep(self, vecs, w, weights, components):
        """Frequency by frequency and chunk by chunk: [J v: source, solve, data] then [J^T w: source, solve, accumulate], the rows
        ``w`` given or ``weights * (J v)``.  ``vecs``: the perturbation per distinct grid (``_right_hand_sides``), or None."""
        handles = self._require_open()
        ns, nf, nb = self.n_src, self.n_freq, self._nb
        adj = w is not None or weights is not None
        dd = np.full((ns, nf, self.n_rec), np.nan, dtype=self.dtype) if vecs is not None else None
        jinfo = [[None] * nf for _ in range(ns)]
        binfo = [[None] * nf for _ in range(ns)]
        nacc = 3 if components else 1
        on_model = self.model_grid is not None          # read back through A^T: G_f on the model grid, factors applied
        partial = np.zeros((nacc, nf) + self._vnM[::-1]).transpose(0, 1, 4, 3, 2) if adj else None     # every G_f F-ordered
        for j, spec in enumerate(self._specs):
            dev, smu0 = handles.target(j, spec), spec.smu0
            real = dev.dtype.kind != 'c'
            vec = None if vecs is None else vecs[self.grid_index[j]]
            if adj:
                dev.grad_acc_reset(components)
            for c, (i0, n) in enumerate(self._chunks):
                slot = self._slot[j] + c
                if vec is not None:
                    dev.jvec_source_b(slot, smu0, *vec, _first(n, nb))
                    infos = self._solve(dev, self.freqs[j], n, self.grids[j])
                    for b in range(n):
                        jinfo[i0 + b][j] = infos[b]
                        dev.select(b)
                        dd[i0 + b, j] = self._data(dev, smu0)
                if not adj:
                    continue
                rows = w[i0:i0 + n, j] if w is not None else weights[i0:i0 + n, j] * dd[i0:i0 + n, j]
                if real:
                    rows = rows.real
                cw = np.where(np.isnan(rows), 0, np.conj(rows))         # NaN (no datum) counts as zero
                live = np.any(cw != 0, axis=1)
                if not live.any():
                    continue
                self._adjoint_sources(dev, smu0, cw, n)
                infos = self._solve(dev, self.freqs[j], n, self.grids[j])
                use = _first(0, nb)
                use[:n] = live
                for b in range(n):
                    if live[b]:
                        binfo[i0 + b][j] = infos[b]
                dev.grad_acc_add(slot, smu0, use, components)
            if adj:
                got = dev.grad_acc_get_model(components) if on_model else dev.grad_acc_get(components)
                for q, g in enumerate(_each(got)):
                    partial[q, j] = g.reshape(self._vnM, order='F')
        return dd, jinfo, partial, binfo

    def _result(self, partial, components):
        """``-(((0 + G_0) + G_1) + ...)`` per accumulator."""
        zeros = np.zeros((self.n_src, self.n_freq))
        out = tuple(-_sum_survey(p, zeros, self._vnM)[1] for p in partial)
        self.partial = partial if components else partial[0]
        return out if components else out[0]

    def _mapped_result(self, partial, components, mapped):
        """``_result`` -- for ``mapped`` products of the three accumulators, which an anisotropic model needs whatever
        ``components`` says, then times the chain factors (``_JacobianBase``).  ``partial`` stays what the device summed: the
        ``G_f`` with respect to conductivity."""
        if not mapped:
            return self._result(partial, components)
        three = components or self.model.case != 0
        if self.model_grid is not None:         # the device has applied F and Q: what is left is the sum of the directions
            out = self._result(partial, three)
            return out if components or not three else (out[0] + out[1]) + out[2]
        return self._from_sigma(self._result(partial, three), components)

    def jvec(self, v, mapped=False):
        """``J v`` for all pairs: ``(n_src, n_freq, n_rec)``; ``v`` as for ``Jacobian.jvec`` (one perturbation).  ``mapped=True``:
        ``v`` perturbs the model's own property."""
        mapped = self._mapped_or_refuse(mapped)
        vec = self._perturbation(v)
        dd, self.info, _, _ = self._sweep(self._right_hand_sides(vec, mapped), None, None, False)
        return dd

    def jtvec(self, w, components=False, mapped=False):
        """``J^T w = sum over the pairs of Jacobian.jtvec(w[i, j])`` in the defined order: a real cell array of shape ``grid.vnC``
        (F-ordered), or the three terms ``(g_x, g_y, g_z)`` of sigma_x, sigma_y, sigma_z with ``components=True``.
        ``mapped=True``: with respect to the model's own property, ``D_c g_c`` (``components=False`` on an anisotropic model:
        their sum)."""
        mapped = self._mapped_or_refuse(mapped)
        w = self._data_array(w, 'w')
        three = components or (mapped and self.model.case != 0)
        _, _, partial, self.info = self._sweep(None, w, None, three)
        return self._mapped_result(partial, components, mapped)

    def gauss_newton(self, v, weights=None, components=False, mapped=False):
        """``J^T W J v``, bit for bit ``jtvec(weights * jvec(v), components)``, the two products run chunk by chunk
        (``mapped=True``: of both mapped products)."""
        mapped = self._mapped_or_refuse(mapped)
        vec = self._perturbation(v)
        weights = self._weights(weights)
        three = components or (mapped and self.model.case != 0)
        _, self.jvec_info, partial, self.info = self._sweep(self._right_hand_sides(vec, mapped), None, weights, three)
        return self._mapped_result(partial, components, mapped)

    # ---- diag(J^H W J) ------------------------------------------------------------------------------------------------
    _no_diagonal_on_model_grid = (
        "SurveyJacobian.sensitivity_diagonal: not available with `model_grid`.  The diagonal on the model grid is not A^T of the "
        "diagonal on the computational grid: a row there is Q (.) A^T (F (.) row), whose squares mix the cells A averages over.")

    def sensitivity_diagonal(self, weights=None, components=False, mapped=False):
        """The diagonal of the Gauss-Newton Hessian ``J^H W J``, the cumulative sensitivity ``out[j] = sum over the data d = (i_src,
        i_freq, i_rec) of weights[d] |J_dj|^2``: a real array of shape ``grid.vnC`` (F-ordered).  ``J_dj = jtvec(e_d) + i
        jtvec(i e_d)`` is entry ``j`` of the complex row of datum ``d`` (Laplace-domain entries of ``freqs``: the real row
        ``jtvec(e_d)``).  ``components=True``: the three diagonals ``(d_x, d_y, d_z)`` with respect to sigma_x, sigma_y, sigma_z (of
        the rows ``jtvec(., components=True)``).  ``mapped=True``: of the rows with respect to the model's own property, i.e. times
        the square of the chain factor.  For an anisotropic model that holds per direction (``components=True``); the square of the
        mapped SUM ``|sum_c D_c J_c|^2`` needs the cross terms ``J_a conj(J_b)``, which no accumulator holds:
        ``NotImplementedError``.

        The operator is complex symmetric, so the row of (source s, receiver r) is the cell average of ``s mu_0 lambda_r E_s`` with
        ``lambda_r`` the field of receiver ``r``'s adjoint source alone: ``n_rec`` solves per frequency give every row (``2 n_src
        n_rec`` through ``jtvec``).  Per frequency the accumulator is reset; the receivers go in chunks of the handle's width
        ``min(batch, n_src)``, system ``b`` of a chunk with the unit row of receiver ``r0 + b`` (built as ``jtvec`` builds its
        sources, for every ``receiver_interpolation``, ``adjoint`` and ``electric``), one batched solve per chunk, then ONE
        ``DeviceMG.sens_acc_add`` per parked chunk of forward fields with that block of ``weights``; one ``nC``-sized array (three)
        comes back per frequency.  ``weights``: real, broadcast to ``(n_src, n_freq, n_rec)``, not negative (default 1); NaN: no
        datum.  A receiver without a datum at a frequency is not solved for (``sensitivity_info[i_freq][i_rec]`` is ``None``,
        otherwise the solver's info dict).  The result is ``((0 + P_0) + P_1) + ...`` over ``freqs`` on the host,
        ``sensitivity_partial`` the ``P_f`` -- ``(n_freq,) + vnC``, ``(3, n_freq) + vnC`` with ``components=True``, with respect to
        conductivity -- for frequency shards to add.  Deterministic for a given ``batch``; another ``batch`` adds the same
        non-negative terms in another order.  Nothing is allocated but the handle's weight table; works after ``set_model``.

        With ``model_grid`` it raises ``ValueError``: the diagonal on the model grid is not ``A^T`` of this one; there
        ``sensitivity_rows(i_freq, mapped=True)`` gives the rows on the model grid, and the diagonal is ``sum_d W_d |row_d|^2``."""
        mapped = _mapped(mapped)
        if self.model_grid is not None:
            raise ValueError(self._no_diagonal_on_model_grid)
        if mapped and not components and self.model.case != 0:
            raise NotImplementedError("SurveyJacobian.sensitivity_diagonal: mapped=True on an anisotropic model gives the diagonal per "
                                      "direction (components=True); the square of the mapped sum needs cross terms that are not "
                                      "accumulated.")
        weights = self._weights(weights)
        if np.any(np.nan_to_num(weights) < 0) or np.any(np.isinf(weights)):
            raise ValueError("`weights` must be finite and not negative (NaN: no datum).")
        weights = np.where(np.isnan(weights), 0.0, weights)
        handles = self._require_open()
        nf, nr, nb = self.n_freq, self.n_rec, self._nb
        nacc = 3 if components else 1
        partial = np.zeros((nacc, nf) + self._vnC[::-1]).transpose(0, 1, 4, 3, 2)       # every P_f F-ordered
        sinfo = [[None] * nr for _ in range(nf)]
        for j, spec in enumerate(self._specs):
            dev, smu0 = handles.target(j, spec), spec.smu0
            dev.grad_acc_reset(components)
            wanted = np.any(weights[:, j, :] != 0, axis=0)          # receivers with a datum at this frequency
            for r0 in range(0, nr, nb):
                n = min(nb, nr - r0)
                live = wanted[r0:r0 + n]
                if not live.any():
                    continue
                cw = np.zeros((n, nr), dtype=dev.dtype)
                for b in np.flatnonzero(live):
                    cw[b, r0 + b] = 1
                self._adjoint_sources(dev, smu0, cw, n)
                infos = self._solve(dev, self.freqs[j], n, self.grids[j])
                use_adj = _first(0, nb)
                use_adj[:n] = live
                for b in np.flatnonzero(live):
                    sinfo[j][r0 + b] = infos[b]
                for c, (i0, ns) in enumerate(self._chunks):
                    table = np.zeros((nb, nb))
                    table[:n, :ns] = weights[i0:i0 + ns, j, r0:r0 + n].T * live[:, None]
                    if np.any(table != 0):
                        dev.sens_acc_add(self._slot[j] + c, smu0, _first(ns, nb), use_adj, table, components=components)
            for q, g in enumerate(_each(dev.grad_acc_get(components))):
                partial[q, j] = g.reshape(self._vnC, order='F')
        self.sensitivity_info = sinfo
        self.sensitivity_partial = partial if components else partial[0]
        zeros = np.zeros((self.n_src, nf))
        out = tuple(_sum_survey(p, zeros, self._vnC)[1] for p in partial)
        if mapped:
            out = tuple(d * d * o for d, o in zip(self._chain_factors(), out))
        return out if components else out[0]

    # ---- the rows of J ------------------------------------------------------------------------------------------------
    @staticmethod
    def _solves(solves):
        """``solves`` of ``sensitivity_rows`` / ``park_rows`` after its check (no device call): 1 or 2."""
        if isinstance(solves, (bool, np.bool_)) or not isinstance(solves, (int, np.integer)) or solves not in (1, 2):
            raise ValueError(f"`solves` must be 2 (the imaginary parts from a second solve, for i e_d: the definition bit for bit) or 1 "
                             f"(both parts from the solve for e_d); provided: {solves!r}.")
        return int(solves)

    def _row_selection(self, i_freq, receivers):
        """``(i_freq, receiver indices)`` of ``sensitivity_rows`` after their checks (no device call)."""
        if isinstance(i_freq, (bool, np.bool_)) or not isinstance(i_freq, (int, np.integer)) or not 0 <= i_freq < self.n_freq:
            raise ValueError(f"`i_freq` must be an index into `freqs`, 0 .. {self.n_freq - 1}; provided: {i_freq!r}.")
        if receivers is None:
            return int(i_freq), list(range(self.n_rec))
        recs = np.asarray(receivers)
        if recs.ndim != 1 or recs.size < 1 or recs.dtype.kind not in 'iu' or recs.min() < 0 or recs.max() >= self.n_rec:
            raise ValueError(f"`receivers` must be a list of receiver indices, 0 .. {self.n_rec - 1} (at least one); provided: "
                             f"{receivers!r}.")
        return int(i_freq), [int(r) for r in recs]

    def sensitivity_rows(self, i_freq, receivers=None, components=False, mapped=False, solves=2):
        """The rows of ``J`` themselves, for all sources and the receivers ``receivers`` (a list of indices into ``rec``, any order,
        kept; default: all) at ``freqs[i_freq]``: an array ``rows[i_src, k] + cells``, ``k`` the position in ``receivers``, cells of
        shape ``grid.vnC`` (F-ordered) -- ``model_grid.vnC`` with ``model_grid`` --, ``complex128`` for a frequency and ``float64``
        for a Laplace-domain entry of ``freqs``.

        DEFINITION.  Row ``(s, r)`` is ``J_dj = jtvec(e_d) + i jtvec(i e_d)`` for the datum ``d = (s, i_freq, r)`` (``e_d``: one at
        ``d``, zero elsewhere; Laplace domain: ``jtvec(e_d)``) -- the row whose squares ``sensitivity_diagonal`` sums, and the
        derivative of datum ``d``: ``jvec(v)[s, i_freq, r] == sum_j rows[s, k][j] v[j]``.

        ``components``, ``mapped``, anisotropic models and ``model_grid`` follow ``jtvec``: ``components=True`` gives a tuple of three
        such arrays, the rows with respect to sigma_x, sigma_y, sigma_z; ``mapped=True`` multiplies every direction by its chain factor
        (and adds the three unless ``components``; all of this is linear, so an anisotropic model needs no cross terms); with
        ``model_grid``, ``mapped=False`` is refused as everywhere, and the device applies ``Q (.) A^T (F (.) .)`` to the real and
        the imaginary part of every row and direction, so that only model-grid-sized rows cross PCIe.

        The loop is that of ``sensitivity_diagonal``: the selected receivers in chunks of the handle's width ``min(batch, n_src)``,
        unit rows through the adjoint sources ``jtvec`` builds (every ``receiver_interpolation``, ``adjoint`` and ``electric``), one
        batched solve per chunk, then ONE ``DeviceMG.sens_rows`` per parked chunk of forward fields, whose real part is
        ``jtvec(e_d)`` for every source of the chunk, bit for bit.  For a frequency the chunk is then solved a second time with the
        rows ``i e_d`` -- the very solves of ``jtvec(i e_d)`` -- and the real part of that ``sens_rows`` is the imaginary part of
        the rows: the definition holds to the last bit, at ``2 n_rec`` solves for all ``n_src n_rec`` rows (``n_rec`` in the Laplace
        domain; ``2 n_src n_rec`` through ``jtvec``).  The imaginary part of the first solve's product is the same quantity, but
        not the same bits: the solve of a rotated right-hand side differs from the rotated solution by rounding that leaves the
        solver amplified (1e-14 .. 3e-13 of a row's largest magnitude at ``tol = 1e-8``), and it is not used.  ``rows_info[k]``
        is the solver's info dict of receiver ``receivers[k]``'s solve for ``e_d``, ``rows_info_imag[k]`` of that for ``i e_d``
        (``None`` in the Laplace domain).

        ``solves=1`` takes both parts from the solve for ``e_d``: one ``_adjoint_sources`` and one solve per chunk, and the real
        AND the imaginary planes of its ``DeviceMG.sens_rows``, each through the chain and sum operations as a real array of its
        own -- half the solves of a frequency.  The real parts are those of ``solves=2`` bit for bit; the imaginary parts equal
        ``jtvec(i e_d)`` to the rounding of the solves only (far below the ``tol`` to which either solve is accurate).
        ``rows_info_imag`` is ``None``.  A Laplace-domain entry is one solve and one part in both forms.  Any other ``solves``
        raises ``ValueError`` before any device call.

        The result is allocated before the first solve (``n_src * len(receivers)`` rows: 16 bytes per cell and row); the device
        keeps one chunk's rows
        (``min(batch, n_src)^2`` of them at most) in a buffer of the handle's own that grows to the largest call so far.  If that
        buffer does not fit, ``HipLibraryError`` names the bytes needed and free: use a smaller ``batch``, or fewer ``receivers`` per
        call.  Works after ``set_model``; deterministic."""
        mapped = self._mapped_or_refuse(mapped)
        solves = self._solves(solves)
        j, recs = self._row_selection(i_freq, receivers)
        handles = self._require_open()
        ns, nb, nk = self.n_src, self._nb, len(recs)
        spec = self._specs[j]
        three = components or (mapped and self.model.case != 0)
        on_model = self.model_grid is not None
        nout = 3 if components else 1
        out = [np.empty((ns, nk) + self._vnM[::-1], dtype=spec.dtype).transpose(0, 1, 4, 3, 2) for _ in range(nout)]    # rows F-ordered
        chain = self._chain_factors() if mapped and not on_model else None
        dev, smu0 = handles.target(j, spec), spec.smu0
        real = dev.dtype.kind != 'c'
        both = not real and solves == 1         # both parts from the solve for e_d
        infos = [[None] * nk for _ in range(1 if real else 2)]
        for k0 in range(0, nk, nb):
            n = min(nb, nk - k0)
            for part, unit in enumerate((1.0,) if real or both else (1.0, 1j)):     # e_d, then i e_d: jtvec's solves, jtvec's products
                w = np.zeros((n, self.n_rec), dtype=dev.dtype)
                for b in range(n):
                    w[b, recs[k0 + b]] = unit
                self._adjoint_sources(dev, smu0, np.conj(w), n)
                infos[part][k0:k0 + n] = self._solve(dev, self.freqs[j], n, self.grids[j])[:n]
                # (plane of the product, views into the rows it fills)
                dests = [('real', out if real else [(o.real, o.imag)[part] for o in out])]
                if both:
                    dests.append(('imag', [o.imag for o in out]))
                for c, (i0, nsrc) in enumerate(self._chunks):
                    got = dev.sens_rows(self._slot[j] + c, smu0, _first(nsrc, nb), _first(n, nb), components=three,
                                        model_grid=on_model)
                    for b in range(n):
                        for s in range(nsrc):
                            for plane, dest in dests:
                                parts = [getattr(g, plane) for g in got[b * nsrc + s]]      # pair p = b * nsrc + s: adjoint systems outer
                                if chain is not None:
                                    parts = [d * g for d, g in zip(chain, parts)]
                                if three and not components:
                                    parts = [(parts[0] + parts[1]) + parts[2]]
                                for q, g in enumerate(parts):
                                    dest[q][i0 + s, k0 + b] = g
        self.rows_info, self.rows_info_imag = infos[0], None if real or both else infos[1]
        return tuple(out) if components else out[0]

    def park_rows(self, data=None, components=False, mapped=False, solves=2):
        """The rows of ``sensitivity_rows`` for the selected data of the WHOLE survey, parked in HBM instead of returned: a
        ``RowStore`` whose ``gram``, ``matvec``, ``rmatvec`` and ``step`` run on the device, so that no row crosses PCIe.

        ``data``: a boolean array broadcast to ``(n_src, n_freq, n_rec)``, the data whose rows are kept (default: all).  A receiver
        with no selected datum at a frequency is not solved for.  The rows are REAL: a datum at a frequency gives two, the real and
        the imaginary part of its row of ``J`` (``part`` 0 and 1); a Laplace-domain datum gives one.  Their order is ``(i_freq,
        i_src, i_rec, part)`` ascending over the selected data, and ``store.index`` is the ``(n_rows, 4)`` table of it.

        The loop is that of ``sensitivity_rows``, frequency by frequency: the same chunks of receivers, the same adjoint sources,
        the same two solves per chunk (``e_d``, then ``i e_d``), the same parked forward fields, and ``DeviceMG.sens_rows_park``
        where that calls ``sens_rows`` -- the same launches into the handle's row buffer, then one that writes the real parts into
        their store rows with the chain factors and the sum of the directions applied in the order the host applies them:
        ``store.row(i)`` equals the matching real or imaginary part of ``sensitivity_rows(...)`` bit for bit.  ``components``,
        ``mapped``, anisotropic models and ``model_grid`` follow ``sensitivity_rows``, refusals included; the chain factors are
        uploaded once per call.  ``store.info[j][r]`` holds the solver info dicts ``(of e_d, of i e_d)`` of receiver ``r`` at
        ``freqs[j]`` (the second ``None`` in the Laplace domain), ``None`` for a receiver that was not solved for.

        ``solves=1`` is the one-solve form of ``sensitivity_rows(solves=1)``: at a frequency one solve per chunk of receivers, for
        ``e_d``, then ONE ``DeviceMG.sens_rows_fill`` per chunk of sources, which writes the real part of every pair into its
        ``part`` 0 row and the imaginary part into its ``part`` 1 row -- on the computational grid straight from the fields, with
        no row buffer on the handle and no parking launch.  ``store.row(i)`` equals the matching part of
        ``sensitivity_rows(..., solves=1)`` bit for bit, the ``part`` 0 rows those of ``solves=2`` too; ``store.info[j][r]`` is
        ``(info, None)``, and ``store.solves`` records the form.  Laplace-domain entries are parked as with ``solves=2``.

        The store is ONE block of ``n_rows * n_cols * 8`` bytes (``n_cols``: the cells of a row, times three with ``components``),
        checked against the free device memory before anything is solved: ``HipLibraryError`` names the bytes needed and free.
        It is a SNAPSHOT of the model at the time of the call: ``set_model`` leaves it valid as such -- it keeps returning the rows
        of the model it was parked for -- and a new ``park_rows`` gives those of the new model.  ``store.close()`` frees it; the
        ``SurveyJacobian`` closes its stores when it closes."""
        mapped = self._mapped_or_refuse(mapped)
        solves = self._solves(solves)
        handles = self._require_open()
        shape = (self.n_src, self.n_freq, self.n_rec)
        if data is None:
            sel = np.ones(shape, dtype=bool)
        else:
            data = np.asarray(data)
            if data.dtype != np.bool_:
                raise TypeError(f"`data` must be a boolean array; provided dtype: {data.dtype}.")
            try:
                sel = np.broadcast_to(data, shape)
            except ValueError:
                raise ValueError(f"`data` must be broadcastable to the data shape {shape}; provided: {data.shape}.") from None
        nb = self._nb
        three = components or (mapped and self.model.case != 0)
        on_model = self.model_grid is not None
        real = [spec.dtype.kind != 'c' for spec in self._specs]
        index = np.array([(j, s, r, part) for j in range(self.n_freq) for s in range(self.n_src) for r in range(self.n_rec)
                          if sel[s, j, r] for part in range(1 if real[j] else 2)], dtype=np.int64).reshape(-1, 4)
        if index.shape[0] < 1:
            raise ValueError("`data` selects no datum.")
        row_of = {tuple(int(x) for x in key): i for i, key in enumerate(index)}
        ncell = int(np.prod(self._vnM))
        store = RowStore(solver.DeviceRows(index.shape[0], (3 if components else 1) * ncell, device=self.device), index, shape,
                         self._vnM, bool(components), real, solves=solves)
        try:
            chain = mapped and not on_model
            if chain:
                store.rows.set_chain(self._chain_factors())
            for j, spec in enumerate(self._specs):
                recs = [r for r in range(self.n_rec) if sel[:, j, r].any()]
                if not recs:
                    continue
                dev, smu0 = handles.target(j, spec), spec.smu0
                got = {r: [None, None] for r in recs}
                both = not real[j] and solves == 1      # both parts from the solve for e_d, filled by the sensitivity kernel
                for k0 in range(0, len(recs), nb):
                    n = min(nb, len(recs) - k0)
                    for part, unit in enumerate((1.0,) if real[j] or both else (1.0, 1j)):     # e_d, then i e_d: sensitivity_rows' solves
                        w = np.zeros((n, self.n_rec), dtype=dev.dtype)
                        for b in range(n):
                            w[b, recs[k0 + b]] = unit
                        self._adjoint_sources(dev, smu0, np.conj(w), n)
                        infos = self._solve(dev, self.freqs[j], n, self.grids[j])
                        for b in range(n):
                            got[recs[k0 + b]][part] = infos[b]
                        for c, (i0, nsrc) in enumerate(self._chunks):
                            if both:
                                dre, dim = (np.array([row_of.get((j, i0 + s, recs[k0 + b], q), -1) for b in range(n)
                                                      for s in range(nsrc)], dtype=np.int32) for q in (0, 1))
                                if (dre >= 0).any():        # (a datum has both parts or neither)
                                    dev.sens_rows_fill(self._slot[j] + c, smu0, _first(nsrc, nb), _first(n, nb), store.rows, dre, dim,
                                                       components=three, model_grid=on_model, chain=chain,
                                                       sum3=three and not components)
                                continue
                            dest = np.array([row_of.get((j, i0 + s, recs[k0 + b], part), -1) for b in range(n) for s in range(nsrc)],
                                            dtype=np.int32)         # pair p = b * nsrc + s: adjoint systems outer
                            if (dest >= 0).any():
                                dev.sens_rows_park(self._slot[j] + c, smu0, _first(nsrc, nb), _first(n, nb), store.rows, dest,
                                                   components=three, model_grid=on_model, chain=chain,
                                                   sum3=three and not components)
                for r, pair in got.items():
                    store.info[j][r] = tuple(pair)
        except BaseException:
            store.close()
            raise
        self._stores.append(store)
        return store


class RowStore:
    """Rows of a survey's ``J`` parked on the device (``SurveyJacobian.park_rows``), and the products of a data-space method over
    them.  The rows are real and ordered as ``index`` says: ``index[i] = (i_freq, i_src, i_rec, part)``, ``part`` 0 the real and 1
    the imaginary part of the datum's row; ``n_rows`` of them.  ``info[j][r]``: the solver info dicts of receiver ``r`` at
    frequency ``j`` (``None``: not solved for).  A "stacked" vector has one real entry per row (``stack`` / ``data`` convert from
    and to complex data arrays); cells are arrays of the shape ``sensitivity_rows`` gives its rows, a tuple of three for a store
    parked with ``components=True``.  ``solves`` is the form it was parked in (``park_rows(solves=)``: 2 = the imaginary parts from
    solves of their own, 1 = both parts from the solve for ``e_d``); ``with_covariance`` and ``project`` carry it over.  A snapshot
    of the model it was parked for; a context manager, ``close()`` frees the device block."""

    def __init__(self, rows, index, shape, vnM, components, real, solves=2):
        self.rows, self.index, self.components = rows, index, components
        self.solves = solves        # park_rows(solves=): 2 = the imaginary parts from solves of their own, 1 = from the solve for e_d
        self.n_rows = index.shape[0]
        self._shape, self._vnM, self._real = shape, tuple(vnM), list(real)
        self._ncell = int(np.prod(vnM))
        self.info = [[None] * shape[2] for _ in range(shape[1])]
        self.cov = None             # with_covariance: the rows are those of B = J L

    def close(self):
        self.rows.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def device_bytes(self):
        return self.rows.device_bytes

    # ---- cells <-> the columns [dir][cell] of a store row ---------------------------------------------------------------------------
    def _columns(self, x, name):
        """Cells (an array of the rows' shape; with a ``components`` store a 3-tuple of them, ``None`` = zero, or one array for all
        three) -> ``n_cols`` doubles."""
        def flat(a):
            if a is None:
                return np.zeros(self._ncell)
            a = np.asarray(a)
            if np.iscomplexobj(a):
                raise TypeError(f"`{name}` must be real.")
            if a.shape != self._vnM:
                raise ValueError(f"`{name}` must have shape {self._vnM}; provided: {a.shape}.")
            return a.astype(np.float64, copy=False).ravel(order='F')
        if isinstance(x, (tuple, list)):
            if not self.components or len(x) != 3 or all(a is None for a in x):
                raise ValueError(f"`{name}`: a 3-tuple (x, y, z), not all None, needs a store parked with components=True.")
            return np.concatenate([flat(a) for a in x])
        return np.concatenate([flat(x)] * 3) if self.components else flat(x)

    def _cells(self, cols):
        parts = tuple(c.reshape(self._vnM, order='F') for c in cols.reshape(-1, self._ncell))
        return parts if self.components else parts[0]

    def _stacked(self, y, name):
        y = np.asarray(y)
        if y.shape == self._shape:
            return self.stack(y)
        if y.shape != (self.n_rows,) or np.iscomplexobj(y):
            raise ValueError(f"`{name}` must be a real vector of {self.n_rows} entries (one per row) or a data array of shape "
                             f"{self._shape}; provided: {y.shape}, {y.dtype}.")
        return np.ascontiguousarray(y, dtype=np.float64)

    # ---- stacked real vectors <-> complex data --------------------------------------------------------------------------------------
    def stack(self, d):
        """A data array ``(n_src, n_freq, n_rec)`` -> the stacked real vector: entry ``i`` is the real (``part`` 0) or imaginary
        (``part`` 1) part of the datum ``index[i]``; a real array gives its value to both parts (weights)."""
        d = np.asarray(d)
        if d.shape != self._shape:
            raise ValueError(f"the data must have shape (n_src, n_freq, n_rec) = {self._shape}; provided: {d.shape}.")
        j, s, r, part = self.index.T
        v = d[s, j, r]
        if not np.iscomplexobj(v):
            return np.ascontiguousarray(v, dtype=np.float64)
        return np.where(part == 0, v.real, v.imag)

    def data(self, y):
        """The inverse of ``stack``: a stacked real vector -> ``(n_src, n_freq, n_rec)`` complex data (NaN where no datum was
        selected; the imaginary part of a Laplace-domain datum is zero)."""
        y = np.asarray(y, dtype=np.float64)
        if y.shape != (self.n_rows,):
            raise ValueError(f"`y` must have {self.n_rows} entries (one per row); provided: {y.shape}.")
        out = np.full(self._shape, np.nan, dtype=np.complex128)
        j, s, r, part = self.index.T
        out[s, j, r] = 0.0
        np.add.at(out, (s, j, r), np.where(part == 0, y, 1j * y))
        return out

    # ---- rows and products ----------------------------------------------------------------------------------------------------------
    def row(self, i):
        """Row ``i`` on the host, cells shaped as the rows of ``sensitivity_rows`` (a tuple of three with ``components``)."""
        return self._cells(self.rows.get_row(i))

    def _refuse_cm(self, cm, what):
        if self.cov is not None and cm is not None:
            raise ValueError(f"RowStore.{what}: this store holds B = J L of a SmoothingCovariance (with_covariance), which is its model "
                             "covariance; a diagonal `cm` on top of it is not J C_m J^T -- use the store it was made from.")

    def gram(self, cm=None):
        """``J C_m J^T`` over the stacked rows, ``(n_rows, n_rows)``; ``cm``: the diagonal of ``C_m`` as cells (default: one).
        ``DeviceRows.gram``: deterministic and exactly symmetric.  On a store made by ``with_covariance``: ``J C J^T = B B^T``
        (``cm`` is refused)."""
        self._refuse_cm(cm, 'gram')
        return self.rows.gram(None if cm is None else self._columns(cm, 'cm'))

    def matvec(self, v):
        """``J v`` as a stacked real vector (``data`` folds it); ``v``: cells, as ``jvec`` takes them.  No solve."""
        if self.cov is not None:
            raise ValueError("RowStore.matvec: this store holds B = J L of a SmoothingCovariance (with_covariance), and B v is not "
                             "J v -- use the store it was made from.")
        return self.rows.matvec(self._columns(v, 'v'))

    def rmatvec(self, y, cm=None):
        """``C_m J^T y`` as cells; ``y``: a stacked real vector, or a data array (``stack``).  On a store made by
        ``with_covariance``: ``C J^T y = cov.sqrt(B^T y)``, on the store's device (``cm`` is refused)."""
        self._refuse_cm(cm, 'rmatvec')
        out = self._cells(self.rows.rmatvec(self._stacked(y, 'y'), None if cm is None else self._columns(cm, 'cm')))
        return out if self.cov is None else self.cov.sqrt(out, device=self.rows.device)

    def step(self, residual, weights, cm=None, damping=0.0):
        """The data-space Gauss-Newton step ``dm = C_m J^T (J C_m J^T + damping W^-1)^-1 r``, by definition
        ``rmatvec(np.linalg.solve(gram(cm) + damping * np.diag(1 / w), r), cm)`` with ``r`` and ``w`` the stacked ``residual`` and
        ``weights`` (stacked vectors or data arrays).  On a store made by ``with_covariance`` ``C_m`` is its covariance (``cm`` is
        refused)."""
        self._refuse_cm(cm, 'step')
        r, w = self._stacked(residual, 'residual'), self._stacked(weights, 'weights')
        return self.rmatvec(np.linalg.solve(self.gram(cm) + damping * np.diag(1 / w), r), cm)

    def project(self, M):
        """``M R`` as a ``solver.DeviceRows`` of ``m`` rows that the caller owns (a context manager; ``close()``); ``M``: ``(m,
        n_rows)`` real, ``R`` the stacked rows of this store, of any kind.  ``DeviceRows.project``: the product over the rows of
        the store on the f64 matrix cores, deterministic, every element one accumulation chain of its own.  With ``M =
        diag(lam_k^-1/2) U_k^T`` from ``np.linalg.eigh(gram())`` these are the principal rows of ``J`` (orthonormal: their
        ``gram()`` is the identity), a truncated-SVD basis or a compressed store.  The result carries this store's ``solves``."""
        out = self.rows.project(M)
        out.solves = self.solves        # (the form of the rows it combines)
        return out

    def _column_sums(self, weights, cm, damping, what):
        """``q[j] = (X^T A^-1 X)[j, j]`` over the columns of a store, ``A = gram(cm) + damping W^-1``: with ``A = K K^T`` and ``T =
        K^-1 R`` on the device, ``X = R`` and ``q = sum_k T[k, j]^2`` on a plain store, ``X = R L^T`` and ``q = sum_k (L t_k)[j]^2``
        on a ``with_covariance`` store.  The temporary store ``T`` is closed before this returns."""
        w = self._stacked(weights, 'weights')
        A = self.gram(cm) + damping * np.diag(1 / w)
        try:
            K = np.linalg.cholesky(A)
        except np.linalg.LinAlgError as exc:
            raise ValueError(f"RowStore.{what}: J C_m J^T + damping W^-1 is not positive definite with `damping` = {damping!r} "
                             "(dependent rows need a positive `damping`).") from exc
        P = np.linalg.solve(K, np.eye(self.n_rows))
        with self.project(P) as T:
            if self.cov is not None:
                planes = 3 if self.components else 1
                T.smooth(self._vnM, planes, self.cov.factors, self.cov.passes, scale=self.cov.scale(planes), after=True)
            return T.colsumsq()

    def resolution_diagonal(self, weights, cm=None, damping=0.0):
        """The diagonal of the model resolution matrix ``R_m = C_m J^T (J C_m J^T + damping W^-1)^-1 J`` as cells: how much of a
        unit change of a cell the data-space ``step`` with the same ``weights`` (stacked, or a data array), ``cm`` (cells, the
        diagonal of ``C_m``; default one) and ``damping`` gives back.  ``A = gram(cm) + damping * np.diag(1 / w)``, ``K =
        np.linalg.cholesky(A)``, ``T = project(K^-1)``, result ``cm * T.colsumsq()``; the temporary store (a second block of the
        store's size) is closed before the method returns.  Defined on a plain store only: under a smoothing covariance ``C = L
        L^T`` the matrix is ``L X L^-1`` with ``X = B^T A^-1 B``, and ``diag(L X L^-1)`` is not a column sum of anything the store
        holds -- a ``with_covariance`` store raises ``ValueError``; ``posterior_variance`` is defined there.  ``ValueError`` also
        where ``A`` is not positive definite (it names ``damping``)."""
        if self.cov is not None:
            raise ValueError("RowStore.resolution_diagonal: this store holds B = J L of a SmoothingCovariance (with_covariance); its "
                             "resolution matrix is L X L^-1, and diag(L X L^-1) is not a column sum of the rows -- use "
                             "posterior_variance, which is defined on this store, or the store it was made from.")
        c = None if cm is None else self._columns(cm, 'cm')
        q = self._column_sums(weights, cm, damping, 'resolution_diagonal')
        return self._cells(q if c is None else c * q)

    def posterior_variance(self, weights, cm=None, damping=0.0):
        """The diagonal of ``C - C J^T (J C J^T + damping W^-1)^-1 J C`` as cells: the posterior variance of every cell for the
        prior covariance ``C`` and the data covariance ``damping W^-1`` (``weights``: stacked, or a data array).  On a plain
        store ``C = diag(cm)`` (cells; default one) and the result is ``cm - cm^2 * q`` with ``q`` the column sums of
        ``resolution_diagonal``.  On a ``with_covariance`` store ``C`` is its covariance (``cm`` is refused): row ``k`` of ``T =
        K^-1 B`` becomes ``L t_k`` on the device (``DeviceRows.smooth(after=True)``) and the result is ``cov.diagonal() -
        T.colsumsq()``.  Returned as computed, a difference of two positive numbers: no clipping -- where the data fix a cell
        almost completely the value is small against the prior variance and carries its rounding error, and may be a few
        ``cond(A) eps`` of the prior variance below zero.  The temporary store is closed before the method returns."""
        self._refuse_cm(cm, 'posterior_variance')
        q = self._column_sums(weights, cm, damping, 'posterior_variance')
        if self.cov is not None:
            prior = self.cov.diagonal()
            prior = np.concatenate([p.ravel(order='F') for p in (prior if isinstance(prior, tuple) else (prior,) * (3 if self.components else 1))])
            return self._cells(prior - q)
        if cm is None:
            return self._cells(1.0 - q)
        c = self._columns(cm, 'cm')
        return self._cells(c - c * c * q)

    def with_covariance(self, cov, inplace=False):
        """A ``RowStore`` whose rows are ``B = J L`` for the smoothing covariance ``cov = L L^T`` (``maps.SmoothingCovariance``):
        row ``d`` of ``B`` is ``L^T j_d``, every row smoothed in place on the device (``DeviceRows.smooth``, ``k_rows_smooth_*``: per
        axis the store is read once and written once) and equal, bit for bit, to ``cov.sqrt_t(row, host=True)``.  On it ``gram()``
        is ``J C J^T = B B^T`` (the products without ``cm``, with their bitwise contracts), ``rmatvec(y)`` is ``C J^T y =
        cov.sqrt(B^T y)``, ``step`` the data-space step with ``C_m = C``, ``row(i)`` row ``i`` of ``B``; ``cm`` arguments,
        ``matvec`` and a second ``with_covariance`` are refused.  Same ``index`` and ``info``; the attribute ``cov``.

        ``inplace=False`` clones the store first (a second block of the same size, checked against the free memory): the original
        stays valid and the caller owns the new store (a context manager; ``close()``).  ``inplace=True`` converts this store, costs
        no second block and returns it.  ``cov``'s grid must have the shape of the store's rows (the model grid for a ``mapped``
        store of a ``model_grid``); every plane of a ``components`` store is smoothed on its own, with the matching entry of a
        3-tuple ``std``."""
        if self.cov is not None:
            raise ValueError("RowStore.with_covariance: this store already holds B = J L of a covariance; a second one would give "
                             "J L L' -- use the store it was made from.")
        if tuple(getattr(cov, 'vnC', ())) != self._vnM:
            raise ValueError(f"RowStore.with_covariance: `cov` must be a SmoothingCovariance on a grid of the rows' shape {self._vnM}; "
                             f"provided: {getattr(cov, 'vnC', None)}.")
        planes = 3 if self.components else 1
        scale = cov.scale(planes)
        if inplace:
            new = self
        else:
            new = RowStore(self.rows.clone(), self.index, self._shape, self._vnM, self.components, self._real, solves=self.solves)
            new.info = self.info
        try:
            new.rows.smooth(self._vnM, planes, cov.factors, cov.passes, scale=scale)
        except BaseException:
            if not inplace:
                new.close()
            raise
        new.cov = cov
        return new


def jvec(grid, model, src, freq, rec, v, **kwargs):
    """One-shot ``Jacobian(grid, model, src, freq, rec, **kwargs).jvec(v)``: open, one product, close."""
    with Jacobian(grid, model, src, freq, rec, **kwargs) as jac:
        return jac.jvec(v)


def jtvec(grid, model, src, freq, rec, w, components=False, **kwargs):
    """One-shot ``Jacobian(grid, model, src, freq, rec, **kwargs).jtvec(w, components)``: open, one product, close."""
    with Jacobian(grid, model, src, freq, rec, **kwargs) as jac:
        return jac.jtvec(w, components=components)
