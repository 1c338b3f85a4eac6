"""Host-side mirror of ``emg3d.solver`` for the multigrid hot path.

Same entry points, argument meaning, return values and error behaviour as the
reference (emg3d/solver.py): :func:`solve`, :func:`multigrid`, :func:`krylov`,
:func:`smoothing`, :func:`restriction`, :func:`prolongation`,
:func:`residual`, :class:`MGParameters` and the small helpers.  The numerics
run on the GPU through the C ABI (``include/emg3d_hip.h``):

* ``solve`` / ``multigrid`` / ``krylov`` keep grids, model, fields and the
  cached line factorisations device-resident in a :class:`DeviceMG` handle
  (tier 2); the host only sees one residual norm per cycle.
* the stand-alone sub-routines operate on host arrays (tier 1), like the
  reference's wrappers around ``emg3d.core``.

Build-specific keyword: ``ordering`` = ``'colour'`` (default; 4-/8-colour
Gauss-Seidel, the throughput mode) or ``'lex'`` (the reference's lexicographic
update order executed as hyperplane wavefronts; cycle-by-cycle parity).
"""
import ctypes
import itertools
import time
from dataclasses import dataclass
from datetime import datetime, timedelta

import warnings

import numpy as np
import scipy.sparse.linalg as ssl

from emg3d_amd import _lib, core, fields, meshes, models

__all__ = ['solve', 'multigrid', 'krylov', 'smoothing', 'restriction', 'prolongation',
           'residual', 'MGParameters', 'DeviceMG', 'FrequencyHandles', 'GridHandles']

ORDERINGS = {'lex': 0, 'colour': 1, 'color': 1}


# --------------------------------------------------------------------------
# Device handle
# --------------------------------------------------------------------------
def _cells(a, dtype=np.float64):
    """A cell array as the C ABI takes it: F-raveled, contiguous."""
    return np.ascontiguousarray(np.asarray(a, dtype=dtype).ravel(order='F'))


class DeviceMG:
    """Device-resident multigrid state (C-ABI tier 2, ``emg3d_mg_*``)."""

    def __init__(self, grid, vmodel, dtype, device=0):
        hx, hy, hz, origin = self._begin(grid, dtype, device)
        etx = _cells(vmodel.eta_x, self.dtype)
        ety = etx if vmodel.eta_y is vmodel.eta_x else _cells(vmodel.eta_y, self.dtype)
        etz = etx if vmodel.eta_z is vmodel.eta_x else _cells(vmodel.eta_z, self.dtype)
        zeta = _cells(vmodel.zeta)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.emg3d_mg_create(
            ctypes.byref(handle), _lib.dtype_code(self.dtype), *(int(n) for n in grid.vnC), _lib.ptr(hx), _lib.ptr(hy),
            _lib.ptr(hz), _lib.ptr(origin), _lib.ptr(etx), _lib.ptr(ety), _lib.ptr(etz),
            _lib.ptr(zeta), int(device)), "emg3d_mg_create")
        self._h = handle

    def _begin(self, grid, dtype, device, smu0=None, sval=None):
        """What the three constructors share: library, dtype, sizes, device and the frequency the handle stands at (``smu0``,
        ``sval``; None for a handle made from a given eta).  Returns the contiguous ``hx, hy, hz, origin``."""
        self._lib = _lib.load()
        self.dtype = np.dtype(dtype)
        self.nE = int(grid.nE)
        self.nC = int(grid.nC)
        self.device = int(device)
        self._smu0, self._sval, self._eps = smu0, sval, False
        self._vnC = tuple(int(n) for n in grid.vnC)
        self._alias = self._zeta = self._epsr = None        # (from_model_parts: what set_model compares a new model with)
        self._vnM = None                                    # (set_model_grid: the cells of the model grid)
        self._factors_shared = None                         # (set_regrid_factors: do the three directions share F and Q?)
        hx, hy, hz = (np.ascontiguousarray(h, dtype=np.float64) for h in grid.h)
        return hx, hy, hz, np.ascontiguousarray(grid.origin, dtype=np.float64)

    @classmethod
    def from_sigma_volume(cls, grid, sv_x, sv_y, sv_z, zeta, smu0, device=0):
        """Handle from the frequency-independent model (``models.sigma_volume``) and the scalar
        ``smu0 = s*mu_0``: ``eta = smu0 * sv`` is formed on the device (``emg3d_mg_create_sv``)."""
        self = cls.__new__(cls)
        hx, hy, hz, origin = self._begin(grid, np.complex128 if np.iscomplexobj(smu0) else np.float64, device, smu0)
        svx = _cells(sv_x)
        svy = svx if sv_y is sv_x else _cells(sv_y)
        svz = svx if sv_z is sv_x else _cells(sv_z)
        zt = _cells(zeta)
        handle = ctypes.c_void_p()
        a = complex(smu0)
        _lib.check(self._lib.emg3d_mg_create_sv(
            ctypes.byref(handle), _lib.dtype_code(self.dtype), *(int(n) for n in grid.vnC), _lib.ptr(hx),
            _lib.ptr(hy), _lib.ptr(hz), _lib.ptr(origin), _lib.ptr(svx), _lib.ptr(svy), _lib.ptr(svz),
            _lib.ptr(zt), a.real, a.imag, int(device)), "emg3d_mg_create_sv")
        self._h = handle
        return self

    @classmethod
    def from_model_parts(cls, grid, sigma_x, sigma_y, sigma_z, vol, zeta, resistivity=False, smu0=None, device=0,
                         epsilon_r=None, sval=None, map_code=None):
        """Handle from ``models.model_parts`` and ``smu0 = s*mu_0``: ``eta = (smu0 * vol) * sigma`` is formed on the device
        with VolumeModel's rounding (``emg3d_mg_create_vs``) -- bit for bit the reference's eta at this and, after
        ``set_smu0``, at every other frequency.  ``resistivity=True``: the three arrays hold resistivities
        (``models.model_parts(..., raw=True)``), the device takes the reciprocal; ``map_code`` (``parts.map_code``: 0 conductivity,
        1 resistivity, 2 / 3 log10 / ln conductivity, 4 / 5 log10 / ln resistivity) says the same for all six property maps and
        goes before ``resistivity``: the device forms ``sigma = backward(p)``.  ``epsilon_r`` (``parts.epsilon_r``) with
        ``sval = s``: ``eta = (smu0 vol) (sigma - s eps_0 eps_r)`` (``emg3d_mg_create_vse``, reference models.py:639-647)."""
        if smu0 is None:
            raise TypeError("from_model_parts: smu0 is required.")
        if epsilon_r is not None and sval is None:
            raise TypeError("from_model_parts: epsilon_r needs sval (s = 2 i pi f resp. the Laplace parameter).")
        self = cls.__new__(cls)
        hx, hy, hz, origin = self._begin(grid, np.complex128 if np.iscomplexobj(smu0) else np.float64, device, smu0, sval)
        sx = _cells(sigma_x)
        sy = sx if sigma_y is sigma_x else _cells(sigma_y)
        sz = sx if sigma_z is sigma_x else _cells(sigma_z)
        vl, zt = _cells(vol), _cells(zeta)
        handle = ctypes.c_void_p()
        a = complex(smu0)
        self._eps = epsilon_r is not None
        code = int(bool(resistivity)) if map_code is None else int(map_code)
        self._alias, self._zeta = (sy is sx, sz is sx), zt
        if self._eps:
            ep = self._epsr = _cells(epsilon_r)
            _lib.check(self._lib.emg3d_mg_create_vse(
                ctypes.byref(handle), _lib.dtype_code(self.dtype), *(int(n) for n in grid.vnC), _lib.ptr(hx),
                _lib.ptr(hy), _lib.ptr(hz), _lib.ptr(origin), _lib.ptr(sx), _lib.ptr(sy), _lib.ptr(sz), _lib.ptr(vl),
                _lib.ptr(zt), _lib.ptr(ep), a.real, a.imag, models.seps0_of(sval), code, int(device)),
                "emg3d_mg_create_vse")
        else:
            _lib.check(self._lib.emg3d_mg_create_vs(
                ctypes.byref(handle), _lib.dtype_code(self.dtype), *(int(n) for n in grid.vnC), _lib.ptr(hx),
                _lib.ptr(hy), _lib.ptr(hz), _lib.ptr(origin), _lib.ptr(sx), _lib.ptr(sy), _lib.ptr(sz), _lib.ptr(vl),
                _lib.ptr(zt), a.real, a.imag, code, int(device)), "emg3d_mg_create_vs")
        self._h = handle
        return self

    @classmethod
    def from_model(cls, grid, parts, spec, device=0):
        """``from_model_parts`` for ``parts = models.model_parts(grid, model, raw=True)`` and a field / frequency object
        ``spec`` (``smu0``, ``sval``): with or without ``epsilon_r``."""
        return cls.from_model_parts(grid, *parts, smu0=spec.smu0, device=device, epsilon_r=getattr(parts, 'epsilon_r', None),
                                    sval=spec.sval, map_code=getattr(parts, 'map_code', None))

    @classmethod
    def open(cls, grid, model, spec, device=0, parts=None):
        """A handle for (grid, model, frequency of the field / frequency object ``spec``): ``from_model`` where the device can
        form VolumeModel's eta bit for bit from sigma and V (``_exact_parts``; ``parts``: the caller's ``models.model_parts(grid,
        model, raw=True)``, computed once for several frequencies), else eta from ``models.VolumeModel`` on the host."""
        parts = _exact_parts(grid, model, spec.smu0) if parts is None else parts
        if parts is not None:
            return cls.from_model(grid, parts, spec, device=device)
        return cls(grid, models.VolumeModel(grid, model, spec), spec.dtype, device=device)

    def _model_arrays(self, grid, parts):
        """The checks of ``set_model`` -- all of them before anything is uploaded -- and the arrays it uploads."""
        if tuple(int(n) for n in grid.vnC) != self._vnC:
            raise ValueError(f"set_model: the handle has {self._vnC} cells, the model's grid {tuple(grid.vnC)}.")
        px, py, pz = parts[:3]
        if px.shape != self._vnC:
            raise ValueError(f"set_model: the handle has {self._vnC} cells, the model {px.shape}.")
        if self._alias is not None:         # (a handle of another kind: the library refuses it)
            if (py is px, pz is px) != self._alias:
                raise ValueError("set_model: the anisotropy case of a handle is fixed at creation; the model has another.")
            ep = getattr(parts, 'epsilon_r', None)
            if (ep is not None) != self._eps:
                raise ValueError("set_model: the handle was created " + ("with" if self._eps else "without") + " epsilon_r.")
            if not np.array_equal(_cells(parts[4]), self._zeta) or (self._eps and not np.array_equal(_cells(ep), self._epsr)):
                raise ValueError("set_model: mu_r and epsilon_r stay as the handle was created with them; the model's differ.")
        sx = _cells(px)
        return sx, (sx if py is px else _cells(py)), (sx if pz is px else _cells(pz))

    def set_model(self, grid, model):
        """Another model on the same grid (``emg3d_mg_set_model``; ``from_model`` / ``from_model_parts`` handles): its property
        arrays go to the device as they are, which forms the conductivities with the model's map and recomputes eta, the coarse
        models and every cached line factorisation at the frequency the handle stands at -- bit for bit a handle created from
        ``model``; hierarchies, work buffers, launch graphs, workspace vectors and accumulators stay, for any batch size.  The
        anisotropy case, ``mu_r`` and ``epsilon_r`` are those of the handle's first model (``ValueError`` otherwise, as for
        a grid of another size, before anything is uploaded); the map may change."""
        self._set_parts(grid, models.model_parts(grid, model, raw=True))

    def _set_parts(self, grid, parts):
        sx, sy, sz = self._model_arrays(grid, parts)
        _lib.check(self._lib.emg3d_mg_set_model(self._h, int(parts.map_code), _lib.ptr(sx), _lib.ptr(sy), _lib.ptr(sz)),
                   "emg3d_mg_set_model")

    def get_sigma(self, comp=0):
        """The conductivity of component ``comp`` (0, 1, 2) as the device holds it (``emg3d_mg_get_sigma``), shape ``vnC``,
        F-ordered: for the logarithmic maps the device's ``exp10`` / ``exp`` of the model's property."""
        out = np.empty(self.nC)
        _lib.check(self._lib.emg3d_mg_get_sigma(self._h, int(comp), _lib.ptr(out)), "emg3d_mg_get_sigma")
        return out.reshape(self._vnC, order='F')

    def set_smu0(self, smu0, sval=None):
        """Re-target a ``from_sigma_volume`` handle to another frequency (``emg3d_mg_set_smu0``): eta, the coarse models,
        every cached line factorisation are recomputed on the device as a fresh handle would; grids, work buffers and
        launch graphs stay.  Same dtype only (a Laplace-domain handle takes a real ``smu0``).  Handles with ``epsilon_r``
        need ``sval`` too (``emg3d_mg_set_smu0_eps``)."""
        a = complex(smu0)
        if self.dtype == np.float64 and a.imag != 0.0:
            raise ValueError("set_smu0: a float64 (Laplace-domain) handle takes a real s*mu_0.")
        if self.dtype == np.complex128 and not np.iscomplexobj(smu0):
            raise ValueError("set_smu0: a complex128 (frequency-domain) handle takes a complex s*mu_0.")
        if self._eps:
            if sval is None:
                raise TypeError("set_smu0: a handle with epsilon_r needs sval.")
            _lib.check(self._lib.emg3d_mg_set_smu0_eps(self._h, a.real, a.imag, models.seps0_of(sval)), "emg3d_mg_set_smu0_eps")
        else:
            _lib.check(self._lib.emg3d_mg_set_smu0(self._h, a.real, a.imag), "emg3d_mg_set_smu0")
        self._smu0, self._sval = smu0, sval

    def retarget(self, spec):
        """``set_smu0`` to the frequency of ``spec`` (a field or ``FrequencySpec``: ``smu0``, ``sval``) unless the handle stands
        at it already."""
        if self._smu0 != spec.smu0:
            self.set_smu0(spec.smu0, sval=spec.sval)

    def get_hfield(self, grid, smu0, mu_r=False):
        """``fields.get_h_field`` (reference fields.py:819-911) of the device-resident electric field:
        the curl runs on the device, only H crosses PCIe.  ``mu_r``: the model has ``mu_r``."""
        nx, ny, nz = (int(n) for n in grid.vnC)
        shapes = ((nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1))
        out = np.empty(sum(int(np.prod(sh)) for sh in shapes), dtype=self.dtype)
        a = complex(smu0)
        _lib.check(self._lib.emg3d_mg_get_hfield(self._h, int(bool(mu_r)), a.real, a.imag, _lib.ptr(out)),
                   "emg3d_mg_get_hfield")
        return fields._h_from_vector(out, shapes)

    def get_receiver_response(self, rec, magnetic=False, smu0=None, mu_r=False, method='cubic'):
        """``fields.get_receiver_response`` (reference fields.py:733-817) of the DEVICE-RESIDENT electric field
        (``magnetic=True``: of ``H = get_h_field(E)``, formed on the device; needs ``smu0``): spline
        prefilter and evaluation run on the device, 16 bytes per receiver cross PCIe.  ``method='linear'``:
        trilinear interpolation on the same trimmed points, NaN outside (``emg3d_mg_get_receiver_response_linear``,
        ``..._linear_h`` for magnetic receivers: models without ``mu_r``)."""
        if method not in ('cubic', 'linear'):
            raise ValueError(f"`method` must be 'cubic' or 'linear'; provided: {method!r}.")
        n, xyz, fac = fields._receiver_args(rec)
        out = np.empty(n, dtype=self.dtype)
        if magnetic and smu0 is None:
            raise ValueError("magnetic receivers need `smu0` (field.smu0).")
        a = complex(smu0) if smu0 is not None else 0j
        if method == 'linear':
            if magnetic:
                if mu_r:
                    raise NotImplementedError("Linear magnetic receivers are implemented for models without `mu_r`.")
                _lib.check(self._lib.emg3d_mg_get_receiver_response_linear_h(self._h, a.real, a.imag, n, _lib.ptr(xyz),
                                                                             _lib.ptr(fac), _lib.ptr(out)),
                           "emg3d_mg_get_receiver_response_linear_h")
                return out
            _lib.check(self._lib.emg3d_mg_get_receiver_response_linear(self._h, n, _lib.ptr(xyz), _lib.ptr(fac), _lib.ptr(out)),
                       "emg3d_mg_get_receiver_response_linear")
            return out
        _lib.check(self._lib.emg3d_mg_get_receiver_response(self._h, int(bool(magnetic)), int(bool(mu_r)), a.real,
                                                            a.imag, n, _lib.ptr(xyz), _lib.ptr(fac), _lib.ptr(out)),
                   "emg3d_mg_get_receiver_response")
        return out

    def gradient(self, efield_vec, smu0, components=False):
        """Adjoint-state gradient of one (source, frequency) pair on this grid (reference optimize.py:176-199):
        the handle's field = back-propagated field, workspace vector ``efield_vec`` = forward field.  ``components=True``:
        the three terms ``(grad_x, grad_y, grad_z)`` whose sum ``(grad_x + grad_y) + grad_z`` is the default result."""
        a = complex(smu0)
        if components:
            outs = [np.empty(self.nC, dtype=np.float64) for _ in range(3)]
            _lib.check(self._lib.emg3d_mg_gradient3(self._h, int(efield_vec), a.real, a.imag, *(_lib.ptr(o) for o in outs)),
                       "emg3d_mg_gradient3")
            return tuple(outs)
        out = np.empty(self.nC, dtype=np.float64)
        _lib.check(self._lib.emg3d_mg_gradient(self._h, int(efield_vec), a.real, a.imag, _lib.ptr(out)),
                   "emg3d_mg_gradient")
        return out

    # ---- per-cell accumulators of the handle: the gradients of all systems of a batch, summed on the device ----
    # Two independent blocks: one array of ``nC`` doubles (optimize.survey_gradient), and with ``components=True`` three, one per
    # direction (optimize.SurveyJacobian).  The C ABI has one entry point per form: name + '3'.
    def _acc_call(self, name, components, *args):
        name = f"emg3d_mg_grad_acc{'3' if components else ''}_{name}"
        return getattr(self._lib, name)(self._h, *args), name

    def _acc_out(self, n, components):
        """Where a ``get`` writes and what it returns: one array of ``n`` doubles, or the pointers and the tuple of three."""
        outs = [np.empty(n, dtype=np.float64) for _ in range(3 if components else 1)]
        return [_lib.ptr(o) for o in outs], (tuple(outs) if components else outs[0])

    def grad_acc_reset(self, components=False):
        """Zero the handle's gradient accumulator (``nC`` doubles of its own, allocated on first use; cycles, ``set_smu0`` and
        ``set_mask`` leave it alone).  ``components=True``: the three per-direction accumulators instead (``nC`` doubles each)."""
        _lib.check(*self._acc_call("reset", components))

    def grad_acc_add(self, fwd_bvec, smu0, use, components=False):
        """``acc = (((acc + g_0) + g_1) + ...)`` over the systems ``b`` with ``use[b] != 0`` in ascending order, in one launch:
        ``g_b`` is bit for bit ``gradient()`` of system ``b`` -- forward field = slice ``b`` of the batched vector ``fwd_bvec``
        (``bvec_copy(fwd_bvec, EFIELD)``; not the live field), back-propagated field = system ``b``'s field.  ``components=True``:
        ``acc_c = (((acc_c + g_c,0) + g_c,1) + ...)`` for ``c = x, y, z``, ``g_c,b`` bit for bit ``gradient(components=True)``."""
        a = complex(smu0)
        what = f"grad_acc{'3' if components else ''}_add"
        u = self._use_flags(use, what)
        st, name = self._acc_call("add", components, int(fwd_bvec), a.real, a.imag, _lib.ptr(u))
        self._check_bvec(st, name, f"{what}: batched vector {fwd_bvec} does not exist (the forward fields must be a saved copy).")

    def grad_acc_get(self, components=False):
        """The accumulator: ``nC`` doubles, F-ordered.  ``components=True``: the three ``(acc_x, acc_y, acc_z)``."""
        ptrs, out = self._acc_out(self.nC, components)
        _lib.check(*self._acc_call("get", components, *ptrs))
        return out

    def _use_flags(self, use, what):
        u = np.ascontiguousarray(use, dtype=np.int32)
        if u.size != self.nsys:
            raise ValueError(f"{what}: {u.size} flags for {self.nsys} systems.")
        return u

    def _check_bvec(self, st, name, message):
        """``_lib.check`` for the calls that read a batched vector: status -2 = that vector does not exist."""
        if st == -2:
            raise ValueError(message)
        _lib.check(st, name)

    # the per-direction form under its own names
    def grad_acc3_reset(self):
        self.grad_acc_reset(components=True)

    def grad_acc3_add(self, fwd_bvec, smu0, use):
        self.grad_acc_add(fwd_bvec, smu0, use, components=True)

    def grad_acc3_get(self):
        return self.grad_acc_get(components=True)

    def grad_acc3_get_model(self):
        return self.grad_acc_get_model(components=True)

    # ---- survey sensitivity diagonal: all pairs of adjoint and forward systems (optimize.SurveyJacobian.sensitivity_diagonal) ----
    def sens_acc_add(self, fwd_bvec, smu0, use_fwd, use_adj, weights, split=False, components=False):
        """``acc += weights[b_adj, b_fwd] * |(c_x + c_y) + c_z|^2`` over the pairs of an adjoint system ``b_adj`` (``use_adj[b_adj]
        != 0``; its field ``lambda`` = system ``b_adj``'s field) and a forward system ``b_fwd`` (``use_fwd[b_fwd] != 0``; ``E`` = slice
        ``b_fwd`` of the batched vector ``fwd_bvec``, a saved copy), ``c_c = edges2cellaverages_c(s mu_0 lambda E)``: one launch
        (``emg3d_mg_sens_acc_add``), adjoint systems ascending in the outer loop, forward systems ascending in the inner one, a
        pair with weight 0 skipped.  Into the accumulator of ``grad_acc_reset`` / ``grad_acc_get``; ``components=True`` (also spelled
        ``split=True``): ``W |c_x|^2, W |c_y|^2, W |c_z|^2`` into the three of ``grad_acc_reset(components=True)``.  The accumulator
        must have been reset once.  ``weights``: ``(nsys, nsys)`` finite doubles, uploaded into a table of the handle's own."""
        components = bool(components) or bool(split)
        a = complex(smu0)
        uf, ua = self._use_flags(use_fwd, "sens_acc_add"), self._use_flags(use_adj, "sens_acc_add")
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (self.nsys, self.nsys):
            raise ValueError(f"sens_acc_add: `weights` must have shape {(self.nsys, self.nsys)}; provided: {w.shape}.")
        if not np.isfinite(w).all():
            raise ValueError("sens_acc_add: `weights` must be finite.")
        st = self._lib.emg3d_mg_sens_acc_add(self._h, int(fwd_bvec), a.real, a.imag, _lib.ptr(uf), _lib.ptr(ua), _lib.ptr(w),
                                             int(components))
        self._check_bvec(st, "emg3d_mg_sens_acc_add",
                         f"sens_acc_add: batched vector {fwd_bvec} does not exist (the forward fields must be a saved copy), or the "
                         f"accumulator was never reset (grad_acc{'3' if components else ''}_reset).")

    # ---- explicit rows of J: what sens_acc_add squares, kept (optimize.SurveyJacobian.sensitivity_rows) ----
    def sens_rows(self, fwd_bvec, smu0, use_fwd, use_adj, components=False, model_grid=False):
        """The rows of all pairs of an adjoint system (``use_adj[b_adj] != 0``; ``lambda`` = system ``b_adj``'s field) and a forward
        system (``use_fwd[b_fwd] != 0``; ``E`` = slice ``b_fwd`` of the batched vector ``fwd_bvec``, a saved copy): an array of shape
        ``(n_pairs, ndir) + vnC``, ``complex128`` on a complex handle and ``float64`` otherwise, cells F-ordered.  Pair ``p`` is the
        ``p``-th in the order of ``sens_acc_add`` (adjoint systems ascending, outer; forward systems ascending, inner); ``ndir`` = 1:
        ``(c_x + c_y) + c_z``, ``components=True``: 3, the ``c_c = edges2cellaverages_c(s mu_0 lambda E)`` apart.  One launch
        (``emg3d_mg_sens_rows``), entry for entry the values whose squares ``sens_acc_add`` sums.  ``model_grid=True``: every real and
        imaginary part as ``Q_c (.) A^T (F_c (.) .)`` on the model grid of ``set_model_grid`` (shape ``(n_pairs, ndir) + vnM``),
        formed on the device so that only those cross PCIe; without ``components`` the three directions must share their factors.
        The device keeps the rows in a buffer of the handle's own that grows to the largest call so far (``device_bytes``); the real
        and imaginary planes it sends are combined here."""
        a = complex(smu0)
        uf, ua = self._use_flags(use_fwd, "sens_rows"), self._use_flags(use_adj, "sens_rows")
        pairs = int(self._lib.emg3d_mg_sens_rows_count(_lib.ptr(uf), _lib.ptr(ua), self.nsys))
        if pairs < 1:
            raise ValueError("sens_rows: `use_fwd` and `use_adj` must each name at least one system.")
        if model_grid and self._vnM is None:
            raise RuntimeError("sens_rows: the handle has no model grid or no regrid factors (set_model_grid, set_regrid_factors).")
        if model_grid and not components and self._factors_shared is False:
            raise ValueError("sens_rows: model_grid=True without components needs regrid factors that the three directions share "
                             "(set_regrid_factors with the same F and the same Q for x, y, z); ask for components=True and add.")
        cells = self._vnM if model_grid else self._vnC
        n = int(np.prod(cells))
        ndir, npart = (3 if components else 1), (2 if self.dtype == np.complex128 else 1)
        buf = np.empty((pairs, ndir, npart, n))
        before = self.device_bytes
        st = self._lib.emg3d_mg_sens_rows(self._h, int(fwd_bvec), a.real, a.imag, _lib.ptr(uf), _lib.ptr(ua), int(bool(components)),
                                          int(bool(model_grid)), _lib.ptr(buf))
        if st == 2:         # hipErrorOutOfMemory: a row buffer did not fit; the handle is still usable
            need = pairs * ndir * npart * 8 * (self.nC + (n if model_grid else 0))
            mi = _lib.mem_info(self.device)
            raise _lib.HipLibraryError(
                f"sens_rows: the rows of {pairs} pairs need up to {need} bytes of device memory beside the {before} the handle holds, "
                f"{mi['free'] + mi['pooled_on_device']} bytes are free; ask for fewer pairs per call (SurveyJacobian: a smaller "
                "`batch` or fewer `receivers`).")
        if st == -7:
            self._require_model_grid(st, "emg3d_mg_sens_rows")
        self._check_bvec(st, "emg3d_mg_sens_rows",
                         f"sens_rows: batched vector {fwd_bvec} does not exist (the forward fields must be a saved copy).")
        if npart == 2:
            out = np.empty((pairs, ndir, n), dtype=self.dtype)
            out.real, out.imag = buf[:, :, 0], buf[:, :, 1]
        else:
            out = buf.reshape(pairs, ndir, n)
        return out.reshape((pairs, ndir) + tuple(cells)[::-1]).transpose(0, 1, 4, 3, 2)         # every row F-ordered

    def sens_rows_park(self, fwd_bvec, smu0, use_fwd, use_adj, rows, dest, components=False, model_grid=False, chain=False,
                       sum3=False):
        """``sens_rows`` up to its copy to the host, the real part of pair ``p`` written into row ``dest[p]`` of the ``DeviceRows``
        ``rows`` instead (``emg3d_mg_sens_rows_park``; ``dest[p] < 0`` skips the pair): the same arguments, the same checks, the same
        launches into the handle's row buffers, then one launch that parks.  A store row's columns are ``[dir][cell]``;
        ``chain=True`` multiplies direction ``q`` by ``rows``' chain factor ``q`` (``DeviceRows.set_chain``), ``sum3=True`` (needs
        ``components``) writes the one plane ``(p0 + p1) + p2`` of the (scaled) directions -- the operations of
        ``SurveyJacobian.sensitivity_rows`` in their order, so that a parked row is that row bit for bit.  The handle's stream is
        synchronised before the call returns."""
        a = complex(smu0)
        uf, ua = self._use_flags(use_fwd, "sens_rows_park"), self._use_flags(use_adj, "sens_rows_park")
        pairs = int(self._lib.emg3d_mg_sens_rows_count(_lib.ptr(uf), _lib.ptr(ua), self.nsys))
        d = np.ascontiguousarray(dest, dtype=np.int32)
        if pairs < 1 or d.shape != (pairs,):
            raise ValueError(f"sens_rows_park: `use_fwd` and `use_adj` name {pairs} pairs (at least one is needed), `dest` has shape "
                             f"{d.shape}.")
        if model_grid and self._vnM is None:
            raise RuntimeError("sens_rows_park: the handle has no model grid or no regrid factors (set_model_grid, set_regrid_factors).")
        if model_grid and not components and self._factors_shared is False:
            raise ValueError("sens_rows_park: model_grid=True without components needs regrid factors that the three directions share.")
        before = self.device_bytes
        st = self._lib.emg3d_mg_sens_rows_park(self._h, int(fwd_bvec), a.real, a.imag, _lib.ptr(uf), _lib.ptr(ua), int(bool(components)),
                                               int(bool(model_grid)), rows._h, _lib.ptr(d), int(bool(chain)), int(bool(sum3)))
        if st == 2:         # hipErrorOutOfMemory: a row buffer did not fit; the handle is still usable
            n = int(np.prod(self._vnM if model_grid else self._vnC))
            need = pairs * (3 if components else 1) * (2 if self.dtype == np.complex128 else 1) * 8 * (self.nC + (n if model_grid else 0))
            mi = _lib.mem_info(self.device)
            raise _lib.HipLibraryError(
                f"sens_rows_park: the rows of {pairs} pairs need up to {need} bytes of device memory beside the {before} the handle "
                f"holds, {mi['free'] + mi['pooled_on_device']} bytes are free; ask for fewer pairs per call (SurveyJacobian: a smaller "
                "`batch`).")
        if st == -7:
            self._require_model_grid(st, "emg3d_mg_sens_rows_park")
        self._check_bvec(st, "emg3d_mg_sens_rows_park",
                         f"sens_rows_park: batched vector {fwd_bvec} does not exist (the forward fields must be a saved copy), or the "
                         "store does not fit the rows (its device, its columns, a destination row, its chain factors).")

    def sens_rows_fill(self, fwd_bvec, smu0, use_fwd, use_adj, rows, dest_re, dest_im=None, components=False, model_grid=False,
                       chain=False, sum3=False):
        """BOTH parts of the rows of ``sens_rows`` into the ``DeviceRows`` ``rows`` (``emg3d_mg_sens_rows_fill``): the real part of
        pair ``p`` into row ``dest_re[p]``, the imaginary part into row ``dest_im[p]`` (``None``: real parts only; a ``float64``
        handle has no other).  A negative entry skips that part; a pair with both negative is not computed; no row may be named
        twice and at least one must be named.  The arguments, the checks and the messages of ``sens_rows_park``, and its
        operations in its order: part 0 is what ``sens_rows_park`` parks and part 1 the imaginary plane of the same ``sens_rows``,
        bit for bit.  On the computational grid this is ONE launch from the fields into the store -- the handle's row buffer is
        neither allocated nor grown, ``device_bytes`` stays --; with ``model_grid=True`` the launches of ``sens_rows``, then one
        parking launch per part.  The handle's stream is synchronised before the call returns."""
        a = complex(smu0)
        uf, ua = self._use_flags(use_fwd, "sens_rows_fill"), self._use_flags(use_adj, "sens_rows_fill")
        pairs = int(self._lib.emg3d_mg_sens_rows_count(_lib.ptr(uf), _lib.ptr(ua), self.nsys))
        d = np.ascontiguousarray(dest_re, dtype=np.int32)
        di = None if dest_im is None else np.ascontiguousarray(dest_im, dtype=np.int32)
        if pairs < 1 or d.shape != (pairs,) or (di is not None and di.shape != (pairs,)):
            raise ValueError(f"sens_rows_fill: `use_fwd` and `use_adj` name {pairs} pairs (at least one is needed), `dest_re` has shape "
                             f"{d.shape}" + ("" if di is None else f", `dest_im` {di.shape}") + ".")
        if model_grid and self._vnM is None:
            raise RuntimeError("sens_rows_fill: the handle has no model grid or no regrid factors (set_model_grid, set_regrid_factors).")
        if model_grid and not components and self._factors_shared is False:
            raise ValueError("sens_rows_fill: model_grid=True without components needs regrid factors that the three directions share.")
        before = self.device_bytes
        st = self._lib.emg3d_mg_sens_rows_fill(self._h, int(fwd_bvec), a.real, a.imag, _lib.ptr(uf), _lib.ptr(ua), int(bool(components)),
                                               int(bool(model_grid)), rows._h, _lib.ptr(d), None if di is None else _lib.ptr(di),
                                               int(bool(chain)), int(bool(sum3)))
        if st == 2:         # hipErrorOutOfMemory: a row buffer of the model-grid path did not fit; the handle is still usable
            n = int(np.prod(self._vnM if model_grid else self._vnC))
            need = pairs * (3 if components else 1) * (2 if self.dtype == np.complex128 else 1) * 8 * (self.nC + (n if model_grid else 0))
            mi = _lib.mem_info(self.device)
            raise _lib.HipLibraryError(
                f"sens_rows_fill: the rows of {pairs} pairs need up to {need} bytes of device memory beside the {before} the handle "
                f"holds, {mi['free'] + mi['pooled_on_device']} bytes are free; ask for fewer pairs per call (SurveyJacobian: a smaller "
                "`batch`).")
        if st == -7:
            self._require_model_grid(st, "emg3d_mg_sens_rows_fill")
        self._check_bvec(st, "emg3d_mg_sens_rows_fill",
                         f"sens_rows_fill: batched vector {fwd_bvec} does not exist (the forward fields must be a saved copy), or the "
                         "store does not fit the rows (its device, its columns, a destination row, its chain factors), or the "
                         "destinations are refused (a row named twice, none named, imaginary parts of a real handle).")

    # ---- the accumulators on a model grid (optimize.SurveyJacobian(model_grid=)) ----
    def set_model_grid(self, model_grid):
        """Link the handle to the grid the model lives on (``emg3d_mg_set_model_grid``): the segment tables of volume averaging
        from ``model_grid`` to the handle's grid, built once and kept in HBM with the scratch of ``grad_acc(3)_get_model``
        (counted by ``device_bytes``).  Another model grid of the same size replaces the first in place."""
        edges = [np.ascontiguousarray(e, dtype=np.float64) for e in (model_grid.nodes_x, model_grid.nodes_y, model_grid.nodes_z)]
        vnM = tuple(int(n) for n in model_grid.vnC)
        st = self._lib.emg3d_mg_set_model_grid(self._h, *vnM, *(_lib.ptr(e) for e in edges))
        if st == -2:
            raise ValueError(f"set_model_grid: the handle is linked to a model grid of another size than {vnM}.")
        _lib.check(st, "emg3d_mg_set_model_grid")
        self._vnM = vnM

    def _require_model_grid(self, st, name):
        """``_lib.check`` for the model-grid calls: status -7 = no model grid, or no factors yet."""
        if st == -7:
            raise RuntimeError(f"{name}: the handle has no model grid or no regrid factors (set_model_grid, set_regrid_factors).")
        _lib.check(st, name)

    def set_regrid_factors(self, F, Q):
        """The diagonal factors of ``grad_acc(3)_get_model`` per direction (``emg3d_mg_set_regrid_factors``): ``F = (F_x, F_y,
        F_z)`` on the handle's grid, ``Q = (Q_x, Q_y, Q_z)`` on the model grid, resident; entries that are the same object as the
        first are uploaded once.  Later calls (another model) replace the values in place."""
        vnM = self._vnM
        if vnM is None:
            raise RuntimeError("set_regrid_factors: the handle has no model grid (set_model_grid).")
        if len(F) != 3 or len(Q) != 3:
            raise ValueError("set_regrid_factors: `F` and `Q` must be 3-tuples (x, y, z).")
        held = []
        for arrs, shape, name in ((F, self._vnC, 'F'), (Q, vnM, 'Q')):
            base = len(held)
            for c, a in enumerate(arrs):
                if c > 0 and a is arrs[0]:
                    held.append(held[base])
                    continue
                if np.shape(a) != shape:
                    raise ValueError(f"set_regrid_factors: `{name}[{c}]` must have shape {shape}; provided: {np.shape(a)}.")
                held.append(_cells(a))
        st = self._lib.emg3d_mg_set_regrid_factors(self._h, *(_lib.ptr(a) for a in held))
        if st == -2:
            raise ValueError("set_regrid_factors: the directions must share factors as in the handle's first call.")
        self._require_model_grid(st, "emg3d_mg_set_regrid_factors")
        self._factors_shared = all(a is arrs[0] for arrs in (F, Q) for a in arrs)

    def grad_acc_get_model(self, components=False):
        """``Q_x (.) A^T (F_x (.) acc)`` of the accumulator of ``grad_acc_add`` (``emg3d_mg_grad_acc_get_model``; ``A``: volume
        averaging from the model grid): ``nM`` doubles, F-ordered.  ``components=True``: ``Q_c (.) A^T (F_c (.) acc_c)`` of the three
        per-direction accumulators (``emg3d_mg_grad_acc3_get_model``), three such arrays.  The accumulators stay as they are."""
        ptrs, out = self._acc_out(int(np.prod(self._vnM or (1,))), components)
        self._require_model_grid(*self._acc_call("get_model", components, *ptrs))
        return out

    def _perturbation_ptrs(self, vs, what):
        held, ptrs = [], []
        for v in vs:
            if v is None:
                ptrs.append(ctypes.c_void_p(None))
                continue
            same = [h for src, h in held if src is v]
            arr = same[0] if same else np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel(order='F'))
            if arr.size != self.nC:
                raise ValueError(f"{what}: {arr.size} values for {self.nC} cells.")
            held.append((v, arr))
            ptrs.append(_lib.ptr(arr))
        return held, ptrs

    def jvec_source_b(self, fwd_bvec, smu0, vx, vy, vz, use):
        """Sources of the systems with ``use[b] != 0`` <- ``s mu_0 C(v) E_b`` in one launch (``emg3d_mg_jvec_source_b``): ``E_b`` =
        slice ``b`` of the batched vector ``fwd_bvec``, one perturbation ``vx, vy, vz`` (as ``jvec_source``) for all of them.  Per
        system bit for bit ``jvec_source``; the sources of the other systems are not touched."""
        a = complex(smu0)
        u = self._use_flags(use, "jvec_source_b")
        held, ptrs = self._perturbation_ptrs((vx, vy, vz), "jvec_source_b")
        st = self._lib.emg3d_mg_jvec_source_b(self._h, int(fwd_bvec), a.real, a.imag, *ptrs, _lib.ptr(u))
        self._check_bvec(st, "emg3d_mg_jvec_source_b", f"jvec_source_b: batched vector {fwd_bvec} does not exist (the forward "
                         "fields must be a saved copy), or a complex s*mu_0 on a float64 handle.")

    def _receiver_adjoint_args(self, rec, method, magnetic, smu0):
        """``(n, xyz, fac, s mu_0)`` of the two receiver-adjoint calls, after their argument checks."""
        if method not in ('cubic', 'linear'):
            raise ValueError(f"`method` must be 'cubic' or 'linear'; provided: {method!r}.")
        if magnetic and smu0 is None:
            raise ValueError("magnetic receivers need `smu0` (field.smu0).")
        return fields._receiver_args(rec) + (complex(smu0) if magnetic else 0j,)

    def set_receiver_adjoint_b(self, rec, w, use, accumulate=False, method='linear', magnetic=False, smu0=None):
        """``set_receiver_adjoint`` for the systems with ``use[b] != 0`` in one call (``emg3d_mg_set_receiver_adjoint_b``): ``w`` has
        shape ``(nsys, n_rec)``, row ``b`` belongs to system ``b``.  The tables that depend on grid and receivers are built once;
        per system bit for bit ``set_receiver_adjoint``; the sources of the other systems are not touched."""
        n, xyz, fac, a = self._receiver_adjoint_args(rec, method, magnetic, smu0)
        u = self._use_flags(use, "set_receiver_adjoint_b")
        wv = np.ascontiguousarray(np.broadcast_to(np.asarray(w), (self.nsys, n)), dtype=self.dtype)
        _lib.check(self._lib.emg3d_mg_set_receiver_adjoint_b(self._h, int(method == 'cubic'), int(bool(magnetic)), a.real, a.imag,
                                                             n, _lib.ptr(xyz), _lib.ptr(fac), _lib.ptr(wv), _lib.ptr(u),
                                                             int(bool(accumulate))), "emg3d_mg_set_receiver_adjoint_b")

    def jvec_source(self, efield_vec, smu0, vx, vy, vz):
        """Source of the selected system <- ``s mu_0 C(v) E`` (``emg3d_mg_jvec_source``): ``E`` = workspace vector
        ``efield_vec``, ``vx, vy, vz`` conductivity perturbations per direction (``nC`` values, F-ordered; ``None``: none)."""
        a = complex(smu0)
        held, ptrs = self._perturbation_ptrs((vx, vy, vz), "jvec_source")
        _lib.check(self._lib.emg3d_mg_jvec_source(self._h, int(efield_vec), a.real, a.imag, *ptrs), "emg3d_mg_jvec_source")

    def set_receiver_adjoint(self, rec, w, accumulate=False, method='linear', magnetic=False, smu0=None):
        """Source of the selected system (+)= ``P^T w``, ``P`` the receiver operator of ``get_receiver_response(rec, method=method,
        magnetic=magnetic, smu0=smu0)`` -- linear or cubic-spline receivers on the electric field or on ``H = get_h_field(E)``
        (without ``mu_r``; needs ``smu0``) -- applied on the device (``emg3d_mg_set_receiver_adjoint_ex``); ``w``: one value per
        receiver.  Receivers with a NaN datum contribute nothing; results repeat bit for bit."""
        n, xyz, fac, a = self._receiver_adjoint_args(rec, method, magnetic, smu0)
        wv = np.ascontiguousarray(np.broadcast_to(np.asarray(w), (n,)), dtype=self.dtype)
        _lib.check(self._lib.emg3d_mg_set_receiver_adjoint_ex(self._h, int(method == 'cubic'), int(bool(magnetic)), a.real, a.imag,
                                                              n, _lib.ptr(xyz), _lib.ptr(fac), _lib.ptr(wv),
                                                              int(bool(accumulate))), "emg3d_mg_set_receiver_adjoint_ex")

    def set_source(self, src, smu0, strength=0, length=1.0, decimals=6, accumulate=False, electric=True):
        """Build the source field ``s mu_0 J_s`` of an electric source IN HBM (``fields.get_source_field``,
        reference emg3d/fields.py:446-631): ``src`` = point dipole ``[x, y, z, azimuth, dip]``, finite dipole
        ``[x0, x1, y0, y1, z0, z1]`` or arbitrarily shaped ``[[x-coo], [y-coo], [z-coo]]``; ``electric=False``: a
        magnetic point dipole (a square loop of side ``length``, fields.py:1043-1049).  The edge
        distribution (``_finite_source_xyz``, fields.py:914-1010) runs on the device; six coordinates per
        segment cross PCIe instead of the nE-sized field.  Returns the moment (sum over segments)."""
        segs = fields._source_segments(src, strength, length, electric)
        a = complex(smu0) * fields._source_sign(src, electric)      # magnetic (loop) sources: the field is negated
        total = 0
        for k, (src6, moment) in enumerate(segs):
            sc = np.asarray(moment, dtype=np.complex128) * a
            scale = np.ascontiguousarray(np.stack([sc.real, sc.imag], axis=1).ravel())
            s6 = np.ascontiguousarray(src6, dtype=np.float64)
            sums = np.zeros(3)
            st = self._lib.emg3d_mg_set_sfield_dipole(self._h, _lib.ptr(s6), _lib.ptr(scale), int(decimals),
                                                      int(k > 0 or accumulate), _lib.ptr(sums))
            if st == -4:
                raise ValueError(f"Provided source outside grid: {np.round(s6, decimals)}.")
            _lib.check(st, "emg3d_mg_set_sfield_dipole")
            # "Ensure unity" (fields.py:1003-1010): the device has divided the weights by |sum|; the reference's
            # print + UserWarning are raised here, per component with a moment
            r6 = np.round(s6, decimals)
            for c in range(3):
                sum_s = abs(sums[c])
                if r6[2 * c + 1] != r6[2 * c] and abs(sum_s - 1) > 1e-6:
                    msg = f"Normalizing Source: {sum_s:.10f}."
                    print(f"* WARNING :: {msg}")
                    warnings.warn(msg, UserWarning)
            total = total + moment
        return total

    def set_sfield_vector(self, vector, smu0):
        """s = smu0 * vector with the real source vector (``SourceField.vector``), scaled on the device."""
        v = np.ascontiguousarray(np.asarray(vector), dtype=np.float64)
        a = complex(smu0)
        _lib.check(self._lib.emg3d_mg_set_sfield_vector(self._h, _lib.ptr(v), a.real, a.imag),
                   "emg3d_mg_set_sfield_vector")

    def close(self):
        if getattr(self, '_h', None):
            self._lib.emg3d_mg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_params(self, var, ordering=None):
        clevel = (ctypes.c_int * 4)(*[int(c) for c in var.clevel])
        order = ORDERINGS[var.ordering if ordering is None else ordering]
        cyc = ord(var.cycle) if var.cycle else ord('V')
        _lib.check(self._lib.emg3d_mg_set_params(self._h, cyc, int(var.nu_init), int(var.nu_pre),
                                                 int(var.nu_coarse), int(var.nu_post), clevel, order),
                   "emg3d_mg_set_params")

    def set_trace(self, on):
        """verb = 5: follow every smoothing call of every level with a residual norm (cycles then launch eagerly)."""
        _lib.check(self._lib.emg3d_mg_set_trace(self._h, int(bool(on))), "emg3d_mg_set_trace")

    def get_trace(self, max_recs=16384):
        """Records collected since the last call: [(it, level, cycmax, kind, (nx, ny, nz), norm)], kind 0 = coarsest level,
        1 = pre-, 2 = post-smoothing; it = -1 on level 0."""
        recs = np.zeros((max_recs, 7), dtype=np.int64)
        norms = np.zeros(max_recs, dtype=np.float64)
        n = ctypes.c_int(0)
        _lib.check(self._lib.emg3d_mg_get_trace(self._h, int(max_recs), _lib.ptr(recs), _lib.ptr(norms), ctypes.byref(n)),
                   "emg3d_mg_get_trace")
        return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), (int(r[4]), int(r[5]), int(r[6])), float(v))
                for r, v in zip(recs[:n.value], norms[:n.value])]

    def prepare(self, sc_dir, lr_dir):
        """Build everything loop invariant for cycles with this (sc_dir, lr_dir) without running one."""
        _lib.check(self._lib.emg3d_mg_prepare(self._h, int(sc_dir), int(lr_dir)), "emg3d_mg_prepare")

    def _field(self, f):
        return np.ascontiguousarray(np.asarray(f), dtype=self.dtype)

    def set_sfield(self, sfield):
        s = self._field(sfield)
        _lib.check(self._lib.emg3d_mg_set_sfield(self._h, _lib.ptr(s)), "emg3d_mg_set_sfield")

    def set_efield(self, efield=None):
        if efield is None:
            _lib.check(self._lib.emg3d_mg_set_efield(self._h, None), "emg3d_mg_set_efield")
        else:
            e = self._field(efield)
            _lib.check(self._lib.emg3d_mg_set_efield(self._h, _lib.ptr(e)), "emg3d_mg_set_efield")

    def get_efield(self, out=None):
        if out is None:
            out = np.empty(self.nE, dtype=self.dtype)
        buf = out if (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.dtype == self.dtype) \
            else np.empty(self.nE, dtype=self.dtype)
        _lib.check(self._lib.emg3d_mg_get_efield(self._h, _lib.ptr(buf)), "emg3d_mg_get_efield")
        if buf is not out:
            out[...] = buf
        return out

    def get_residual(self):
        out = np.empty(self.nE, dtype=self.dtype)
        _lib.check(self._lib.emg3d_mg_get_residual(self._h, _lib.ptr(out)), "emg3d_mg_get_residual")
        return out

    # ---- batched systems: several sources through the same launches (include/emg3d_hip.h) ----
    @property
    def nsys(self):
        return int(self._lib.emg3d_mg_get_batch(self._h))

    def set_batch(self, n):
        """Carry ``n`` systems (right-hand sides on this grid, model and frequency) through every launch of the
        cycle.  Before the first cycle only; zeroes the fields."""
        st = self._lib.emg3d_mg_set_batch(self._h, int(n))
        if st == -6:
            raise RuntimeError("set_batch: the handle has already run or prepared a cycle, or holds workspace vectors.")
        _lib.check(st, "emg3d_mg_set_batch")

    def select(self, b):
        """The system that set/get sfield/efield, set_source, get_hfield, get_receiver_response, get_residual,
        sfield_norm and gradient address from now on."""
        _lib.check(self._lib.emg3d_mg_select(self._h, int(b)), "emg3d_mg_select")

    def set_mask(self, active):
        """``active[b] == 0`` freezes system b: its cycles are skipped, its field stays as it is."""
        a = np.ascontiguousarray(active, dtype=np.int32)
        if a.size != self.nsys:
            raise ValueError(f"set_mask: {a.size} flags for {self.nsys} systems.")
        _lib.check(self._lib.emg3d_mg_set_mask(self._h, _lib.ptr(a)), "emg3d_mg_set_mask")

    def _norms(self, fn, name, *args):
        n = self.nsys
        out = np.empty(n, dtype=np.float64)
        _lib.check(fn(self._h, *args, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), name)
        return float(out[0]) if n == 1 else out

    def residual_norm(self):
        """||s - A e||_2 -- a float, or one value per system of a batch."""
        return self._norms(self._lib.emg3d_mg_residual_norm, "emg3d_mg_residual_norm")

    def sfield_norm(self):
        v = ctypes.c_double()
        _lib.check(self._lib.emg3d_mg_sfield_norm(self._h, ctypes.byref(v)), "emg3d_mg_sfield_norm")
        return v.value

    def smooth(self, nu, lr_dir):
        _lib.check(self._lib.emg3d_mg_smooth(self._h, int(nu), int(lr_dir)), "emg3d_mg_smooth")

    def begin(self, sc_dir):
        """Entry of ``solver.multigrid``: level 0's cycmax is fixed from the sc_dir of this moment, as the reference
        does (solver.py:480-485), for all cycles of the call."""
        _lib.check(self._lib.emg3d_mg_begin(self._h, int(sc_dir)), "emg3d_mg_begin")

    def cycle(self, sc_dir, lr_dir, nxt=None):
        """One multigrid cycle; returns the end-of-cycle residual norm (one per system of a batch).  ``nxt`` = the
        (sc_dir, lr_dir) of the NEXT cycle: its loop-invariant set-up then runs on the host while the device works."""
        if nxt is not None:
            return self._norms(self._lib.emg3d_mg_cycle_next, "emg3d_mg_cycle_next", int(sc_dir), int(lr_dir),
                               int(nxt[0]), int(nxt[1]))
        return self._norms(self._lib.emg3d_mg_cycle, "emg3d_mg_cycle", int(sc_dir), int(lr_dir))

    def cycles(self, n, sc_cycle, lr_cycle):
        """``n`` cycles back to back; norms of shape (n,), or (n, nsys) for a batch."""
        sc = np.ascontiguousarray(sc_cycle, dtype=np.int32)
        lr = np.ascontiguousarray(lr_cycle, dtype=np.int32)
        ns = self.nsys
        out = np.empty(n * ns, dtype=np.float64)
        _lib.check(self._lib.emg3d_mg_cycles(self._h, int(n), _lib.ptr(sc), sc.size, _lib.ptr(lr),
                                             lr.size, _lib.ptr(out)), "emg3d_mg_cycles")
        return out if ns == 1 else out.reshape(n, ns)

    def amatvec(self, x):
        x = self._field(x)
        y = np.empty(self.nE, dtype=self.dtype)
        _lib.check(self._lib.emg3d_mg_amatvec(self._h, _lib.ptr(x), _lib.ptr(y)), "emg3d_mg_amatvec")
        return y

    # ---- device-resident vector workspace (Krylov iteration) ----
    SFIELD, EFIELD = -1, -2      # vector ids of the level-0 source / field

    def vec_alloc(self, n):
        _lib.check(self._lib.emg3d_mg_vec_alloc(self._h, int(n)), "emg3d_mg_vec_alloc")

    def vec_set(self, i, x):
        x = self._field(x)
        _lib.check(self._lib.emg3d_mg_vec_set(self._h, int(i), _lib.ptr(x)), "emg3d_mg_vec_set")

    def vec_get(self, i):
        y = np.empty(self.nE, dtype=self.dtype)
        _lib.check(self._lib.emg3d_mg_vec_get(self._h, int(i), _lib.ptr(y)), "emg3d_mg_vec_get")
        return y

    def vec_copy(self, dst, src):
        _lib.check(self._lib.emg3d_mg_vec_copy(self._h, int(dst), int(src)), "emg3d_mg_vec_copy")

    def vec_axpy(self, y, alpha, x):
        """y += alpha * x"""
        a = complex(alpha)
        _lib.check(self._lib.emg3d_mg_vec_axpy(self._h, int(y), a.real, a.imag, int(x)), "emg3d_mg_vec_axpy")

    def vec_scale(self, y, alpha):
        a = complex(alpha)
        _lib.check(self._lib.emg3d_mg_vec_scale(self._h, int(y), a.real, a.imag), "emg3d_mg_vec_scale")

    def vec_dot(self, a, b):
        """numpy.vdot(a, b) (first argument conjugated) / numpy.dot for float64."""
        out = (ctypes.c_double * 2)()
        _lib.check(self._lib.emg3d_mg_vec_dot(self._h, int(a), int(b), out), "emg3d_mg_vec_dot")
        return complex(out[0], out[1]) if self.dtype.kind == 'c' else float(out[0])

    def vec_norm(self, a):
        return float(np.sqrt(abs(self.vec_dot(a, a))))

    def vec_amatvec(self, dst, src):
        _lib.check(self._lib.emg3d_mg_vec_amatvec(self._h, int(dst), int(src)), "emg3d_mg_vec_amatvec")

    # ---- batched vector workspace: vectors [nsys][nE]; every primitive acts on the systems that are not frozen ----
    # (ids 0..n-1; SFIELD / EFIELD = the whole level-0 source / field array; per system bit for bit the vec_* result)
    def bvec_alloc(self, n):
        _lib.check(self._lib.emg3d_mg_bvec_alloc(self._h, int(n)), "emg3d_mg_bvec_alloc")

    def _bcoef(self, alpha):
        c = np.broadcast_to(np.asarray(alpha, dtype=np.complex128), (self.nsys,))
        return np.ascontiguousarray(np.stack([c.real, c.imag], axis=1))

    def bvec_copy(self, dst, src):
        _lib.check(self._lib.emg3d_mg_bvec_copy(self._h, int(dst), int(src)), "emg3d_mg_bvec_copy")

    def bvec_zero(self, i):
        _lib.check(self._lib.emg3d_mg_bvec_zero(self._h, int(i)), "emg3d_mg_bvec_zero")

    def bvec_axpy(self, y, alpha, x):
        """y_b += alpha_b * x_b; ``alpha``: one value per system (or one for all)."""
        a = self._bcoef(alpha)
        _lib.check(self._lib.emg3d_mg_bvec_axpy(self._h, int(y), _lib.ptr(a), int(x)), "emg3d_mg_bvec_axpy")

    def bvec_scale(self, y, alpha):
        a = self._bcoef(alpha)
        _lib.check(self._lib.emg3d_mg_bvec_scale(self._h, int(y), _lib.ptr(a)), "emg3d_mg_bvec_scale")

    def bvec_dot(self, a, b, out=None):
        """``vec_dot`` per system in one call (one device-to-host copy); the entries of frozen systems keep what ``out``
        held (zero without ``out``)."""
        n = self.nsys
        if out is None:
            out = np.zeros(n, dtype=self.dtype)
        raw = np.zeros((n, 2))
        raw[:, 0] = out.real
        if self.dtype.kind == 'c':
            raw[:, 1] = out.imag
        _lib.check(self._lib.emg3d_mg_bvec_dot(self._h, int(a), int(b), _lib.ptr(raw)), "emg3d_mg_bvec_dot")
        out[...] = raw[:, 0] + 1j * raw[:, 1] if self.dtype.kind == 'c' else raw[:, 0]
        return out

    def bvec_amatvec(self, dst, src):
        _lib.check(self._lib.emg3d_mg_bvec_amatvec(self._h, int(dst), int(src)), "emg3d_mg_bvec_amatvec")

    def bvec_get(self, i, b):
        y = np.empty(self.nE, dtype=self.dtype)
        _lib.check(self._lib.emg3d_mg_bvec_get(self._h, int(i), int(b), _lib.ptr(y)), "emg3d_mg_bvec_get")
        return y

    def bvec_set(self, i, b, x):
        x = self._field(x)
        if x.size != self.nE:
            raise ValueError(f"bvec_set: {x.size} values for {self.nE} edges.")
        _lib.check(self._lib.emg3d_mg_bvec_set(self._h, int(i), int(b), _lib.ptr(x)), "emg3d_mg_bvec_set")

    def time_sweep(self, direction, reps=3):
        v = ctypes.c_float()
        _lib.check(self._lib.emg3d_mg_time_sweep(self._h, int(direction), int(reps), ctypes.byref(v)),
                   "emg3d_mg_time_sweep")
        return v.value

    def placement(self):
        """Record of the placement of level 0's working copies (``emg3d_mg_placement``): per working copy ('x': the transposed
        copy the x-line sweeps write, 'yz': the x-split copy of the y- / z-line sweeps) the candidates timed, the index of the one
        kept (0 = the block the handle had) and ms per sweep of every candidate; {} when nothing was placed (small levels,
        ``EMG3D_PLACE_TRIES=0``)."""
        out = {}
        for w, name in ((0, 'x'), (1, 'yz')):
            tries, kept = ctypes.c_int(0), ctypes.c_int(0)
            ms = (ctypes.c_float * 16)()
            _lib.check(self._lib.emg3d_mg_placement(self._h, w, ctypes.byref(tries), ctypes.byref(kept), ms), "emg3d_mg_placement")
            if kept.value < 0:
                out[name] = {"tries": 0, "kept": -1, "reused": True}        # (the block an earlier handle of the process had found)
            elif tries.value > 0:
                out[name] = {"tries": tries.value, "kept": kept.value, "first_ms": float(ms[0]), "kept_ms": float(ms[kept.value]),
                             "ms_per_sweep": [float(ms[k]) for k in range(tries.value)]}
        return out

    def last_sweep_kernel(self):
        """Name of the kernel instantiation the most recent line-sweep launch of this handle selected."""
        buf = ctypes.create_string_buffer(64)
        _lib.check(self._lib.emg3d_mg_last_sweep_kernel(self._h, buf), "emg3d_mg_last_sweep_kernel")
        return buf.value.decode()

    def last_residual_kernel(self):
        """Name of the kernel instantiation the most recent residual launch of this handle selected."""
        buf = ctypes.create_string_buffer(64)
        _lib.check(self._lib.emg3d_mg_last_residual_kernel(self._h, buf), "emg3d_mg_last_residual_kernel")
        return buf.value.decode()

    def time_residual(self, reps=3):
        v = ctypes.c_float()
        _lib.check(self._lib.emg3d_mg_time_residual(self._h, int(reps), ctypes.byref(v)),
                   "emg3d_mg_time_residual")
        return v.value

    @property
    def device_bytes(self):
        return int(self._lib.emg3d_mg_device_bytes(self._h))

    @property
    def efield_devptr(self):
        return self._lib.emg3d_mg_efield_devptr(self._h)

    @property
    def stream_ptr(self):
        """The handle's HIP stream (``hipStream_t`` as an integer) for ``torch.cuda.ExternalStream``."""
        return int(self._lib.emg3d_mg_stream(self._h) or 0)


class DeviceRows:
    """A row store on the device (``emg3d_rows_*``): ``n_rows`` x ``n_cols`` doubles, row-major, in ONE block of HBM of its own, and
    the dense products a data-space method takes from rows that stay there -- ``gram`` (``R diag(cm) R^T`` on the f64 matrix cores),
    ``matvec`` (``R v``) and ``rmatvec`` (``cm (.) R^T y``), and ``project`` (``M R`` into a second store) with ``colsumsq``.  It belongs to no ``DeviceMG``: the handles of a survey park into one
    store (``DeviceMG.sens_rows_park``); ``set_row`` fills it from the host.  Creating it checks its bytes against the device's free
    memory first: a store that cannot fit raises ``HipLibraryError`` with the bytes needed and free, and nothing was allocated.
    Every product is deterministic (no atomics; the column slabs follow from ``n_cols`` alone): see ``gram``.  A context manager;
    ``close()`` frees the block."""

    def __init__(self, n_rows, n_cols, device=0):
        self._lib = _lib.load()
        self._h = None
        self.n_rows, self.n_cols, self.device = int(n_rows), int(n_cols), int(device)
        if self.n_rows < 1 or self.n_cols < 1:
            raise ValueError(f"DeviceRows: `n_rows` and `n_cols` must be at least 1; provided: {n_rows!r}, {n_cols!r}.")
        h = ctypes.c_void_p()
        st = self._lib.emg3d_rows_create(self.device, self.n_rows, self.n_cols, ctypes.byref(h))
        if st == 2:         # hipErrorOutOfMemory, from the check before the allocation or from the allocation itself
            mi = _lib.mem_info(self.device)
            raise _lib.HipLibraryError(
                f"DeviceRows: {self.n_rows} rows of {self.n_cols} columns need {self.n_rows * self.n_cols * 8} bytes of device memory "
                f"in one block, {mi['free'] + mi['pooled_on_device']} bytes are free; park fewer data per store (SurveyJacobian."
                "park_rows: a `data` mask, or a `model_grid`).")
        _lib.check(st, "emg3d_rows_create")
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            self._lib.emg3d_rows_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _open(self):
        if not self._h:
            raise RuntimeError("DeviceRows: the store is closed.")
        return self._h

    def _vector(self, a, n, what):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (n,):
            raise ValueError(f"DeviceRows.{what} must have shape {(n,)}; provided: {a.shape}.")
        return a

    @property
    def device_bytes(self):
        """The bytes of the block (256-byte aligned); plus those of the chain factors once ``set_chain`` was called, and of the
        products' workspace (operands, slab partials, results), which grows to the largest product so far and is kept."""
        return int(self._lib.emg3d_rows_bytes(self._open()))

    def _row(self, i):
        if isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)) or not 0 <= i < self.n_rows:
            raise IndexError(f"DeviceRows: row {i!r} is outside 0 .. {self.n_rows - 1}.")
        return int(i)

    def set_row(self, i, row):
        """Row ``i`` <- ``row`` (``n_cols`` doubles of the host)."""
        r = self._vector(row, self.n_cols, "set_row: `row`")
        _lib.check(self._lib.emg3d_rows_set(self._open(), self._row(i), _lib.ptr(r)), "emg3d_rows_set")

    def get_row(self, i):
        """Row ``i`` on the host."""
        out = np.empty(self.n_cols)
        _lib.check(self._lib.emg3d_rows_get(self._open(), self._row(i), _lib.ptr(out)), "emg3d_rows_get")
        return out

    def set_chain(self, factors):
        """Three arrays of ``n`` doubles kept on the device for ``DeviceMG.sens_rows_park(chain=True)``; ``None`` frees them."""
        if factors is None:
            _lib.check(self._lib.emg3d_rows_set_chain(self._open(), 0, None, None, None), "emg3d_rows_set_chain")
            return
        f = [np.ascontiguousarray(np.asarray(a).ravel(order='F'), dtype=np.float64) for a in factors]
        if len(f) != 3 or any(a.shape != f[0].shape for a in f):
            raise ValueError("DeviceRows.set_chain: `factors` must be three arrays of one size.")
        _lib.check(self._lib.emg3d_rows_set_chain(self._open(), f[0].size, *(_lib.ptr(a) for a in f)), "emg3d_rows_set_chain")

    def gram(self, cm=None):
        """``G = R diag(cm) R^T``, ``(n_rows, n_rows)``: ``G[a, b] = sum_j R[a, j] cm[j] R[b, j]``; ``cm``: ``n_cols`` doubles, default
        all one.  ``k_rows_gram`` on ``v_mfma_f64_16x16x4_f64``, the partial sums of the column slabs added in ascending order by a
        second pass.  The same bits at every call; ``G == G.T`` exactly; without ``cm`` a store with its rows permuted gives the
        permuted ``G`` bit for bit (with ``cm`` the factor multiplies the row of the smaller index, which a permutation may change:
        then bit for bit only where the products ``cm[j] R[b, j]`` are exact, to rounding otherwise)."""
        c = None if cm is None else self._vector(cm, self.n_cols, "gram: `cm`")
        out = np.empty((self.n_rows, self.n_rows))
        _lib.check(self._lib.emg3d_rows_gram(self._open(), None if c is None else _lib.ptr(c), _lib.ptr(out)), "emg3d_rows_gram")
        return out

    def matvec(self, v):
        """``R v``, ``n_rows`` doubles: per row and column slab a fixed tree, the slabs added in ascending order (deterministic)."""
        v = self._vector(v, self.n_cols, "matvec: `v`")
        out = np.empty(self.n_rows)
        _lib.check(self._lib.emg3d_rows_matvec(self._open(), _lib.ptr(v), _lib.ptr(out)), "emg3d_rows_matvec")
        return out

    def rmatvec(self, y, cm=None):
        """``cm (.) R^T y``, ``n_cols`` doubles: per column ``acc = acc + y[i] * R[i, j]`` over the rows ascending, then
        ``cm[j] * acc`` (no ``cm``: ``acc``), every operation rounded once -- bit for bit that loop in numpy."""
        y = self._vector(y, self.n_rows, "rmatvec: `y`")
        c = None if cm is None else self._vector(cm, self.n_cols, "rmatvec: `cm`")
        out = np.empty(self.n_cols)
        _lib.check(self._lib.emg3d_rows_rmatvec(self._open(), _lib.ptr(y), None if c is None else _lib.ptr(c), _lib.ptr(out)),
                   "emg3d_rows_rmatvec")
        return out

    def clone(self):
        """A second store of the same size on the same device with the same rows (a device-to-device copy; chain factors are not
        copied).  The memory check of a new store: one that cannot fit raises ``HipLibraryError`` and nothing was allocated."""
        new = object.__new__(DeviceRows)
        new._lib, new._h = self._lib, None
        new.n_rows, new.n_cols, new.device = self.n_rows, self.n_cols, self.device
        h = ctypes.c_void_p()
        st = self._lib.emg3d_rows_clone(self._open(), ctypes.byref(h))
        if st == 2:
            mi = _lib.mem_info(self.device)
            raise _lib.HipLibraryError(
                f"DeviceRows.clone: a second store of {self.n_rows} rows of {self.n_cols} columns needs "
                f"{self.n_rows * self.n_cols * 8} bytes of device memory in one block, {mi['free'] + mi['pooled_on_device']} bytes "
                "are free; convert the store in place instead.")
        _lib.check(st, "emg3d_rows_clone")
        new._h = h
        return new

    def smooth(self, shape, planes, factors, passes, scale=None, after=False):
        """Every row <- ``L^T`` row of ``maps.SmoothingCovariance``, in place (``emg3d_rows_smooth``, ``k_rows_smooth_*``): a row is
        ``planes`` arrays of ``shape`` = ``(nx, ny, nz)``, x fastest, each smoothed on its own; ``factors``: per axis ``(lo, cp,
        inv)`` or ``None`` (skipped); ``scale``: ``n_cols`` doubles multiplied in first, or ``None``.  Bit for bit the numpy loop of
        ``SmoothingCovariance.sqrt_t(host=True)`` on every row.  ``after=True``: ``L`` row instead (``emg3d_rows_smooth_l``) -- the
        same sweeps, ``scale`` multiplied in last; bit for bit ``SmoothingCovariance.sqrt(host=True)``."""
        shape = tuple(int(n) for n in shape)
        if len(shape) != 3:
            raise ValueError(f"DeviceRows.smooth: `shape` must be (nx, ny, nz); provided: {shape}.")
        ptrs, keep = _lib.factor_ptrs(factors, shape)
        w = None if scale is None else self._vector(scale, self.n_cols, "smooth: `scale`")
        name = "emg3d_rows_smooth_l" if after else "emg3d_rows_smooth"
        st = getattr(self._lib, name)(self._open(), *shape, int(planes), None if w is None else _lib.ptr(w), *ptrs, int(passes))
        if st == -2:
            raise ValueError(f"DeviceRows.smooth: {planes} planes of shape {shape} are not the {self.n_cols} columns of a row, or "
                             f"`passes` = {passes!r} is less than 1 ({name}: -2).")
        _lib.check(st, name)

    def project(self, M, out=None):
        """``Y = M R`` as a ``DeviceRows`` of ``m`` rows, ``M``: ``(m, n_rows)`` real -- the product that contracts over the ROWS of
        the store (``emg3d_rows_project``, ``k_rows_project`` on ``v_mfma_f64_16x16x4_f64``); this store is not modified.  By
        default the result is a new store (the memory check of a new store: one that cannot fit raises ``HipLibraryError`` and
        nothing was allocated), which the caller owns; ``out=`` is a store of ``m`` rows and ``n_cols`` columns on the same device,
        not this one, that is overwritten and returned.  The same bits at every call.  ``Y[i, j]`` depends on row ``i`` of ``M``
        and column ``j`` of the store alone: one accumulation chain over the rows in groups of four, whatever ``m`` and ``n_cols``
        are -- rows of ``M`` permuted give the rows of ``Y`` permuted bit for bit.  The order inside a group of four is the
        hardware's: not bit for bit a numpy loop, but within ``gamma(n_rows + 2) |M| |R|`` of the exact product."""
        M = np.asarray(M)
        if np.iscomplexobj(M):
            raise TypeError("DeviceRows.project: `M` must be real.")
        if M.ndim != 2 or M.shape[0] < 1 or M.shape[1] != self.n_rows:
            raise ValueError(f"DeviceRows.project: `M` must have shape (m, {self.n_rows}), m >= 1; provided: {M.shape}.")
        M = np.ascontiguousarray(M, dtype=np.float64)
        m = M.shape[0]
        h = self._open()
        if out is None:
            dst = object.__new__(DeviceRows)
            dst._lib, dst._h = self._lib, None
            dst.n_rows, dst.n_cols, dst.device = m, self.n_cols, self.device
            hd = ctypes.c_void_p()
            st = self._lib.emg3d_rows_create(self.device, m, self.n_cols, ctypes.byref(hd))
            if st == 2:
                mi = _lib.mem_info(self.device)
                raise _lib.HipLibraryError(
                    f"DeviceRows.project: the result, a second block of {m} rows of {self.n_cols} columns, needs "
                    f"{m * self.n_cols * 8} bytes of device memory, {mi['free'] + mi['pooled_on_device']} bytes are free; project "
                    "onto fewer rows at a time.")
            _lib.check(st, "emg3d_rows_create")
            dst._h = hd
        else:
            dst = out
            if not isinstance(dst, DeviceRows) or dst is self or dst.n_rows != m or dst.n_cols != self.n_cols or dst.device != self.device:
                raise ValueError(f"DeviceRows.project: `out` must be another DeviceRows of {m} rows and {self.n_cols} columns on device "
                                 f"{self.device}.")
            dst._open()
        try:
            st = self._lib.emg3d_rows_project(h, _lib.ptr(M), m, dst._h)
            if st == -2:
                raise ValueError("DeviceRows.project: the stores do not fit each other (emg3d_rows_project: -2).")
            _lib.check(st, "emg3d_rows_project")
        except BaseException:
            if out is None:
                dst.close()
            raise
        return dst

    def colsumsq(self, s=None):
        """``sum_i s[i] R[i, j]^2``, ``n_cols`` doubles; ``s``: ``n_rows`` doubles, default all one.  One thread per column: ``acc =
        acc + s[i] * (R[i, j] * R[i, j])`` over the rows ascending (no ``s``: ``acc + R[i, j] * R[i, j]``), every operation
        rounded once -- bit for bit that loop in numpy."""
        s = None if s is None else self._vector(s, self.n_rows, "colsumsq: `s`")
        out = np.empty(self.n_cols)
        _lib.check(self._lib.emg3d_rows_colsumsq(self._open(), None if s is None else _lib.ptr(s), _lib.ptr(out)), "emg3d_rows_colsumsq")
        return out


class FrequencyHandles:
    """The handles of a loop over frequencies on one grid and model: one ``DeviceMG`` per dtype (and optional extra ``key``),
    created at the first frequency that asks for it -- ``DeviceMG.from_model`` on ``parts = models.model_parts(grid, model,
    raw=True)``, ``set_batch(nsys)`` if ``nsys > 1``, ``bvec_alloc(bvecs)`` if ``bvecs`` --, re-targeted at the later ones
    (``DeviceMG.retarget``: bit for bit a fresh handle), all closed on exit."""

    def __init__(self, grid, parts, device, nsys=1, bvecs=0):
        self.grid, self.parts, self.device, self.nsys, self.bvecs = grid, parts, device, int(nsys), int(bvecs)
        self._handles = {}
        self._model_grid = self._factors = None

    def target(self, spec, key=()):
        """The handle for ``spec`` (a field or ``FrequencySpec``: ``dtype``, ``smu0``, ``sval``), standing at its frequency."""
        key = (np.dtype(spec.dtype).str,) + tuple(key)
        dev = self._handles.get(key)
        if dev is not None:
            dev.retarget(spec)
            return dev
        dev = self._handles[key] = DeviceMG.from_model(self.grid, self.parts, spec, device=self.device)
        if self.nsys > 1:
            dev.set_batch(self.nsys)
        if self.bvecs:
            dev.bvec_alloc(self.bvecs)
        if self._model_grid is not None:
            dev.set_model_grid(self._model_grid)
            if self._factors is not None:
                dev.set_regrid_factors(*self._factors)
        return dev

    def set_model(self, model):
        """Re-target every handle to ``model`` (``DeviceMG.set_model``; checked against all of them before the first upload);
        handles created later are created from it."""
        parts = models.model_parts(self.grid, model, raw=True)
        for dev in self._handles.values():
            dev._model_arrays(self.grid, parts)
        for dev in self._handles.values():
            dev._set_parts(self.grid, parts)
        self.parts = parts

    def set_model_grid(self, model_grid):
        """Link every open handle, and the handles created later, to the grid the model lives on (``DeviceMG.set_model_grid``)."""
        for dev in self._handles.values():
            dev.set_model_grid(model_grid)
        self._model_grid = model_grid

    def set_regrid_factors(self, F, Q):
        """The factors of ``grad_acc(3)_get_model`` for every open handle and the handles created later
        (``DeviceMG.set_regrid_factors``)."""
        if self._model_grid is None:
            raise RuntimeError("set_regrid_factors: the handles have no model grid (set_model_grid).")
        for dev in self._handles.values():
            dev.set_regrid_factors(F, Q)
        self._factors = (tuple(F), tuple(Q))

    def __iter__(self):
        return iter(self._handles.values())

    def close(self):
        for dev in self._handles.values():
            dev.close()
        self._handles = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class GridHandles:
    """The handles of a loop over frequencies whose entries may each have a computational grid of their own: one
    ``FrequencyHandles`` per DISTINCT grid of ``grids`` (``meshes.distinct_grids``; one mesh per entry of the loop), hence one
    ``DeviceMG`` per distinct (grid, dtype) -- and optional extra ``key`` --, on which the entries of that grid are re-targeted
    exactly as on a ``FrequencyHandles`` of their own.  ``members[k]`` are the handles of ``distinct[k]``, ``index[j]`` the ``k``
    of entry ``j``.

    ``model_grid=None``: ``model`` lives on the (then one) grid.  Otherwise it lives on ``model_grid`` and reaches every distinct
    grid through ``model.interpolate2grid(model_grid, grid)``, once per distinct grid (``on_grids``)."""

    def __init__(self, grids, model, device, nsys=1, bvecs=0, model_grid=None):
        self.grids, self.device, self.model_grid = list(grids), device, model_grid
        self.distinct, self.index = meshes.distinct_grids(self.grids)
        self.members = [FrequencyHandles(g, models.model_parts(g, m, raw=True), device, nsys=nsys, bvecs=bvecs)
                        for g, m in zip(self.distinct, self.on_grids(model))]

    def on_grids(self, model):
        """``model`` on every distinct grid."""
        if self.model_grid is None:
            return [model] * len(self.distinct)
        return [model.interpolate2grid(self.model_grid, g) for g in self.distinct]

    def target(self, j, spec, key=()):
        """The handle of entry ``j`` for ``spec`` (``FrequencyHandles.target`` on the entry's grid), standing at its frequency."""
        return self.members[self.index[j]].target(spec, key)

    def set_model(self, model):
        """Re-target every handle to ``model`` (regridded once per distinct grid; checked against ALL handles of all grids before
        the first upload); handles created later are created from it."""
        parts = [models.model_parts(g, m, raw=True) for g, m in zip(self.distinct, self.on_grids(model))]
        for member, p in zip(self.members, parts):
            for dev in member:
                dev._model_arrays(member.grid, p)
        for member, p in zip(self.members, parts):
            for dev in member:
                dev._set_parts(member.grid, p)
            member.parts = p

    def set_model_grid(self, model_grid):
        """Link every open handle, and the handles created later, to the grid the model lives on."""
        for member in self.members:
            member.set_model_grid(model_grid)

    def set_regrid_factors(self, k, F, Q):
        """The factors of ``grad_acc(3)_get_model`` for the handles of ``distinct[k]``, open or created later (``F`` lives on that
        grid)."""
        self.members[k].set_regrid_factors(F, Q)

    def __iter__(self):
        return itertools.chain.from_iterable(self.members)

    def close(self):
        for member in self.members:
            member.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# --------------------------------------------------------------------------
# solve
# --------------------------------------------------------------------------
def solve(grid, model, sfield, efield=None, cycle='F', sslsolver=False, semicoarsening=False,
          linerelaxation=False, verb=1, **kwargs):
    """Solve Maxwell's equations with multigrid and/or a Krylov solver.

    Mirrors ``emg3d.solver.solve`` (reference emg3d/solver.py:35-430): same
    parameters (``tol, maxit, nu_init, nu_pre, nu_coarse, nu_post, clevel,
    return_info, log``), same return convention (``efield`` if none was
    provided, ``info_dict`` if ``return_info``), same ``info_dict`` keys and
    exit messages.  Extra keywords: ``ordering`` ('colour'|'lex'), ``device``,
    ``handle`` (an existing ``DeviceMG`` for this grid/model/frequency, e.g. from
    ``DeviceMG.from_sigma_volume``; it is used as is and not closed; ``model`` may then be None),
    ``source=(src, strength)`` (the source is built in HBM by ``DeviceMG.set_source`` -- ``sfield`` then only
    carries the frequency and is not uploaded; ``source='resident'``: the handle already holds it),
    ``download=False`` (multigrid only: the solution stays in HBM, the returned field is None).
    """
    device = kwargs.pop('device', 0)
    handle = kwargs.pop('handle', None)
    source = kwargs.pop('source', None)     # (src, strength): build the source in HBM instead of uploading `sfield`;
    #                                         'resident': the handle already holds the source
    download = kwargs.pop('download', True)  # False: leave the solution in HBM (returned efield is None)
    var = MGParameters(cycle=cycle, sslsolver=sslsolver, semicoarsening=semicoarsening,
                       linerelaxation=linerelaxation, vnC=grid.vnC, verb=verb, **kwargs)

    var.cprint(f"\n:: emg3d START :: {var.time.now} :: emg3d_amd (MI355X/HIP)\n", 2)
    var.cprint(var, 2)

    if sfield.freq is None:
        raise ValueError("Source field is missing frequency information;\n"
                         "Create it with `emg3d_amd.fields.get_source_field`, or\n"
                         "initiate it with `emg3d_amd.fields.SourceField`.")

    info = ""
    if handle is None:
        dev = DeviceMG.open(grid, model, sfield, device=device)
    else:
        dev = handle
        if dev.dtype != sfield.dtype:
            raise ValueError(f"`handle` is {dev.dtype}, the source field {sfield.dtype}.")
    try:
        dev.set_params(var)
        if isinstance(source, str) and source == 'resident':
            if var.sslsolver:
                sfield.field[:] = dev.vec_get(dev.SFIELD)
        elif source is not None:
            # the source field never exists on the host: six coordinates per dipole segment go up, the edge
            # distribution runs on the device (DeviceMG.set_source); `sfield` only carries the frequency
            dev.set_source(source[0], sfield.smu0, strength=source[1] if len(source) > 1 else 0,
                           electric=source[2] if len(source) > 2 else True)
            if var.sslsolver:               # the Krylov drivers take the right-hand side from the host object
                sfield.field[:] = dev.vec_get(dev.SFIELD)
        else:
            dev.set_sfield(sfield)
        # ||sfield||_2 (reference solver.py:305, scipy.linalg.norm) on the device, from the copy just uploaded.
        # Not numpy/BLAS on the host: the 64-128 worker threads a multi-threaded BLAS spins up for this one
        # norm stall the GPU queues of the process once, 30-50 ms later, for 60-80 ms (tools/idle_gap.py:
        # 128^3 solve 0.20 s with the host norm, 0.14 s without).
        var.l2_refe = dev.sfield_norm()
        var.error_at_cycle[0] = var.l2_refe

        if efield is None:
            efield = fields.Field(grid, dtype=sfield.dtype, freq=sfield._freq)
            var.do_return = True
            dev.set_efield(None)
        else:
            if sfield.dtype != efield.dtype:
                raise ValueError("Source field and electric field must have the\n same dtype; "
                                 "complex (f-domain) or real (s-domain).\n Provided:"
                                 f"sfield: {sfield.dtype}; efield: {efield.dtype}.")
            if efield.freq is None:
                efield._freq = sfield._freq
            var.do_return = False
            dev.set_efield(efield)
            var.l2 = dev.residual_norm()
            if var.l2 < var.tol * var.l2_refe:
                var.sslsolver = None
                var.cycle = None
                var.exit_message = "CONVERGED"
                info = "   > NOTHING DONE (provided efield already good enough)\n"

        if var.l2_refe < 100 * np.finfo(float).tiny:
            var.l2_refe = np.nan
            var.sslsolver = None
            var.cycle = None
            var.exit_message = "CONVERGED"
            info = "   > RETURN ZERO E-FIELD (provided sfield is zero)\n"
            efield = fields.Field(grid, dtype=sfield.dtype, freq=sfield._freq)

        header = f"   [hh:mm:ss]  {'rel. error':<22}"
        if var.sslsolver:
            header += f"{'solver':<20}"
            if var.cycle:
                header += f"{'MG':<11} l s"
            var.cprint(header + "\n", 3)
        elif var.cycle:
            var.cprint(header + f"{'[abs. error, last/prev]':>29}   l s\n", 3)

        if var.sslsolver:               # (model None: the handle holds eta and zeta, for SciPy's iterations on host vectors too)
            krylov(grid, None, sfield, efield, var, dev=dev)
        elif var.cycle:
            var._dev_efield_current = True
            multigrid(grid, None, sfield, efield if download else None, var, dev=dev)
            if not download and var.do_return:
                efield = None
    finally:
        if handle is None:
            dev.close()

    exit_status = int(var.exit_message != 'CONVERGED')

    if var.verb < 0 or var.verb == 2:
        var.one_liner(var.l2, True)
    elif var.verb > 2:
        if var.sslsolver:
            info = f"   > Solver steps     : {var._ssl_it}\n"
            if var.cycle:
                info += f"   > MG prec. steps   : {var.it}\n"
        elif var.cycle:
            info = f"   > MG cycles        : {var.it}\n"
        info += f"   > Final rel. error : {var.l2/var.l2_refe:.3e}\n\n"
        info += f":: emg3d END   :: {var.time.now} :: runtime = {var.time.runtime}\n"
        var.cprint(info, 2)
    elif var.verb == 1 and exit_status == 1:
        var.cprint(f"* WARNING :: {var.exit_message}", 0)

    if var.do_return and var.return_info:
        return efield, _info_dict(var)
    elif var.do_return:
        return efield
    elif var.return_info:
        return _info_dict(var)


def _info_dict(var):
    """The ``info_dict`` of a finished solve (reference solver.py:408-422)."""
    return {
        'exit': int(var.exit_message != 'CONVERGED'),
        'exit_message': var.exit_message,
        'abs_error': var.l2,
        'rel_error': var.l2 / var.l2_refe,
        'ref_error': var.l2_refe,
        'tol': var.tol,
        'it_mg': var.it,
        'it_ssl': var._ssl_it,
        'time': var.runtime_at_cycle[-1],
        'runtime_at_cycle': var.runtime_at_cycle,
        'error_at_cycle': var.error_at_cycle,
        'log': var.log_message,
    }


def _exact_parts(grid, model, smu0):
    """``models.model_parts`` where the device can form VolumeModel's eta from them: s*mu_0 purely imaginary (frequency
    domain) or real (Laplace domain); with or without epsilon_r."""
    if np.iscomplexobj(smu0) and np.real(smu0) != 0.0:
        return None
    return models.model_parts(grid, model, raw=True)


def _rotation_state(var):
    """Where ``var`` stands in the rotation of the semicoarsening / line-relaxation directions: the positions in the two
    lists (they advance by one per cycle the system has run) and the directions of the next cycle."""
    return (int(var.sc_dir), int(var.lr_dir), var.it % len(var._raw_sc_cycle) if var.sc_cycle else 0,
            var.it % len(var._raw_lr_cycle) if var.lr_cycle else 0)


def _rotation_partitions(states, active):
    """Groups of active systems (``active[b]`` != 0) with equal rotation ``states[b]``, in the order of their first members.
    The systems of a group can go through the same launches of a cycle; the groups run one after the other."""
    groups = {}
    for b, st in enumerate(states):
        if b < len(active) and active[b]:
            groups.setdefault(st, []).append(b)
    return list(groups.values())


def _batched_multigrid(dev, vars_, active, trace=False):
    """THE level-0 loop of the multigrid solver (reference emg3d/solver.py:434-607; ``multigrid`` runs it for one system), for the
    systems ``active[b]`` != 0 of the handle (mask already on the device), which stand at the same point of the direction rotation
    and start together: initial norm, optional initial smoothing, then cycles until every system has met one of its own
    termination tests (a finished system is frozen).  Returns the systems for which ``_terminate`` raised ``_ConvergenceError`` (a
    failing preconditioner) and the mask the device holds at the end.

    ``trace`` (``multigrid`` at verb = 5, one system; solver.py:498-515): also log the norm after every smoothing call of every
    level -- the device reports them."""
    active = np.array(active, dtype=np.int32)
    on_device = active.copy()
    idx = [b for b in range(len(vars_)) if active[b]]
    failed = []
    if not idx:
        return failed, on_device
    lead = vars_[idx[0]]
    maxc = lead._maxcycle
    dev.begin(lead.sc_dir)
    l2_last = np.atleast_1d(dev.residual_norm()).copy()
    l2_stag = {b: np.ones(maxc) * l2_last[b] for b in idx}
    if trace:
        cm0 = 1 if lead.clevel[lead.sc_dir] == 0 else lead.cycmax       # level 0's cycmax, fixed on entry (solver.py:480-485)
        lead.cprint("     it cycmax               error", 4)
        lead.cprint("      level [  dimension  ]            info\n", 4)
        lead.cprint(_print_gs_info(0, 0, cm0, lead.vnC, l2_last[0]) + "initial error", 4)
        dev.set_trace(True)
    if lead.nu_init > 0:
        dev.smooth(lead.nu_init, lead.lr_dir)
        if trace:
            lead.cprint(_print_gs_info(0, 0, cm0, lead.vnC, dev.residual_norm()) + "initial smoothing", 4)
    it = 0
    while active.any():
        live = [b for b in idx if active[b]]
        l2_prev = l2_last.copy()
        for b in idx:
            l2_stag[b][(it - 1) % maxc] = l2_last[b]
        # the rotation of the directions (solver.py:597-600) depends on the cycle count only: one state for the systems of the
        # group, each of which advances its own iterators (it may enter a later call in another group).  It is known before
        # the cycle: the handle prepares the next pair's hierarchy / factorisations / launch graph on the host meanwhile
        cur = (vars_[live[0]].sc_dir, vars_[live[0]].lr_dir)
        for b in live:
            v = vars_[b]
            nxt = (next(v.sc_cycle) if v.sc_cycle else v.sc_dir, next(v.lr_cycle) if v.lr_cycle else v.lr_dir)
        ahead = PREPARE_AHEAD and nxt != cur and it + 1 < lead.maxit
        norms = np.atleast_1d(dev.cycle(cur[0], cur[1], nxt=nxt if ahead else None))
        if trace:
            for rit, level, cm, kind, vnC, norm in dev.get_trace():
                lead.cprint(_print_gs_info(it if level == 0 else rit, level, cm, vnC, norm) +
                            ("coarsest level", "pre-smoothing", "post-smoothing")[kind], 4)
        it += 1
        changed = False
        for b in live:
            var = vars_[b]
            l2_last[b] = norms[b]
            var.it += 1
            _print_cycle_info(var, l2_last[b], l2_prev[b])
            var.sc_dir, var.lr_dir = nxt
            try:
                done = _terminate(var, l2_last[b], l2_stag[b][(it - 1) % maxc], it)
            except _ConvergenceError:
                failed.append(b)
                active[b] = 0
                changed = True
                continue
            if done:
                var.l2 = float(l2_last[b])
                active[b] = 0
                changed = True
        if changed and active.any():
            dev.set_mask(active)
            on_device = active.copy()
    return failed, on_device


def _krylov_sources(dev, vars_, active):
    """The Krylov part of ``solve_sources``: ``krylov`` for the systems ``active[b]`` != 0 of the batched handle ``dev`` (sources
    in place), all in lockstep (``_bicgstab_device_batched`` / ``_cgs_device_batched``), preconditioned -- if ``cycle`` -- by
    batched multigrid cycles.  The solutions end up in the level-0 field array of the handle."""
    n = len(vars_)
    nsys = dev.nsys
    live = [b for b in range(n) if active[b]]
    if not live:                    # zero sources only: zero fields
        return
    v0 = vars_[live[0]]
    name = v0.sslsolver
    if not _krylov_fits_device(dev, name, nsys=nsys):
        mi = _lib.mem_info(dev.device)
        raise _lib.HipLibraryError(
            f"solve_sources: the {name} workspace of {nsys} systems needs {_krylov_workspace_bytes(dev, name, nsys=nsys)} "
            f"bytes of device memory, {mi['free'] + mi['pooled_on_device']} bytes are free; use a smaller batch "
            f"(fewer sources per call, shard.solve_survey(batch=...)).")

    def psolve(src, dst, mask):
        """dst_b = M src_b for the systems of ``mask``: per system what ``mg_on_device`` + ``multigrid`` run for a single solve.
        The systems may stand at different points of the direction rotation (an inner call ends early for a system
        whose norm falls below tol * l2_refe): one batched pass per group of equal state, the others frozen.  The
        device's mask is ``mask`` on entry and on return."""
        dev.bvec_copy(dev.SFIELD, src)
        dev.bvec_zero(dev.EFIELD)
        failed, on_device = [], mask
        for group in _rotation_partitions([_rotation_state(v) for v in vars_], mask):
            gmask = np.zeros(nsys, dtype=np.int32)
            gmask[group] = 1
            if not np.array_equal(gmask, on_device):
                dev.set_mask(gmask)
            bad, on_device = _batched_multigrid(dev, vars_, gmask)
            failed += bad
        if not np.array_equal(mask, on_device):
            dev.set_mask(mask)
        dev.bvec_copy(dst, dev.EFIELD)
        return failed

    drive = {'bicgstab': _bicgstab_device_batched, 'cgs': _cgs_device_batched}[name]
    failed = []
    codes = drive(dev, n, rtol=v0.tol, maxiter=v0.ssl_maxit, atol=1e-30, psolve=psolve if v0.cycle else None,
                  callbacks=[lambda l2, var=var: _krylov_step(var, l2) for var in vars_], active=active, failed=failed)
    for b, var in enumerate(vars_):
        if active[b]:
            _krylov_exit_message(var, codes[b], b in failed)
    mask = np.zeros(nsys, dtype=np.int32)
    mask[:n] = active[:n]           # (a zero source's field was zeroed when it was set up)
    dev.set_mask(mask)
    dev.bvec_copy(dev.EFIELD, 0)    # the iterates (batched vector 0) -> the level-0 fields: receivers, download, reuse
    mask[:n] = 1
    dev.set_mask(mask)


def solve_sources(grid, model, sources, frequency, strength=0, cycle='F', semicoarsening=False,
                  linerelaxation=False, verb=1, rec=None, download=True, electric=True, resident=None, **kwargs):
    """``[solve(grid, model, get_source_field(grid, src, frequency, strength), ...) for src in sources]`` as ONE
    batched multigrid iteration: the sources of a survey share grid, model and frequency (the reference loops over
    them one solve at a time, simulations.py:916-1015), hence the operator, the coarse models and the cached
    line factorisations; the device carries all of them through every launch of the cycle (``DeviceMG.set_batch``).
    Every system goes through the arithmetic of a solve of its own and stops by its own termination tests
    (a finished system is frozen, ``DeviceMG.set_mask``): fields and ``info_dict`` equal those of separate solves.

    ``sources``: electric sources as ``DeviceMG.set_source`` takes them (built in HBM), or ``SourceField`` objects
    of frequency ``frequency`` (uploaded).  ``sslsolver=True | 'bicgstab' | 'cgs'``: the Krylov iteration of ``solve`` for all
    sources in lockstep on batched device vectors (``DeviceMG.bvec_*``), preconditioned by the batched cycles; every system
    keeps its own coefficients and stops by its own tests, as above.  The workspace (12 vectors per system) must fit
    in device memory (``HipLibraryError`` otherwise: use a smaller batch); ``'gcrotmk'`` is not batched.  ``rec``: receivers
    ``(x, y, z, azimuth, dip)`` -- the responses are extracted on the device.  ``download=False``: no fields
    returned.  Returns ``(efields | None, info_dicts)`` and the responses ``(n_sources, n_rec)`` if ``rec``.

    ``resident=n`` (with ``handle``; ``sources`` is ignored and may be None): the sources already sit in systems ``0 .. n-1`` of
    the handle (``DeviceMG.select`` + ``set_source`` / ``jvec_source`` / ``set_receiver_adjoint``); nothing is uploaded.  The
    handle may carry more systems than ``n``: the others are frozen for the call and keep their fields.  Multigrid only.
    """
    sslsolver = kwargs.pop('sslsolver', False)
    if sslsolver not in (False, None, True, 'bicgstab', 'cgs'):
        raise ValueError("solve_sources batches the Krylov solvers 'bicgstab' and 'cgs' (sslsolver=True: 'bicgstab'); "
                         f"use solve() per source for sslsolver={sslsolver!r}.")
    sslsolver = sslsolver or False
    if sslsolver and resident is not None:
        raise ValueError("solve_sources: `resident` sources are solved by multigrid only (sslsolver=False).")
    device = kwargs.pop('device', 0)
    handle = kwargs.pop('handle', None)       # an existing DeviceMG of this grid / model / frequency: used, not closed
    if resident is not None:
        if handle is None:
            raise ValueError("solve_sources: `resident` sources live on a `handle`.")
        sources = [None] * int(resident)
    n = len(sources)
    if n < 1:
        raise ValueError("solve_sources: no sources.")
    proto = fields.FrequencySpec(frequency)                 # dtype, smu0 of this frequency (no nE-sized array)
    host_fields = [s if hasattr(s, 'field') else None for s in sources]
    for sf in host_fields:
        if sf is not None and (sf.freq is None or sf._freq != proto._freq):
            raise ValueError("solve_sources: every source field must carry the frequency of the batch.")
    vars_ = [MGParameters(cycle=cycle, sslsolver=sslsolver, semicoarsening=semicoarsening,
                          linerelaxation=linerelaxation, vnC=grid.vnC, verb=verb, **kwargs) for _ in range(n)]
    v0 = vars_[0]
    if handle is not None:
        # the caller's handle, already on this frequency (DeviceMG.set_smu0) and fresh or batched for exactly n systems
        dev = handle
        if dev.dtype != proto.dtype:
            raise ValueError(f"solve_sources: `handle` is {dev.dtype}, the frequency needs {proto.dtype}.")
    else:
        dev = DeviceMG.open(grid, model, proto, device=device)
    try:
        dev.set_params(v0)
        if resident is not None and n > dev.nsys:
            raise ValueError(f"solve_sources: {n} resident sources on a handle of {dev.nsys} systems.")
        if resident is None and dev.nsys != n:
            dev.set_batch(n)
        active = np.ones(dev.nsys, dtype=np.int32)
        active[n:] = 0                  # (resident sources on a wider handle: the other systems stay frozen)
        if handle is not None:
            dev.set_mask(active)
        for b, (src, var) in enumerate(zip(sources, vars_)):
            dev.select(b)
            if handle is not None:
                dev.set_efield(None)
            if resident is not None:            # the system holds its source already
                pass
            elif host_fields[b] is not None:
                dev.set_sfield(host_fields[b])
            else:
                dev.set_source(src, proto.smu0, strength=strength, electric=electric)
            var.l2_refe = dev.sfield_norm()
            var.error_at_cycle[0] = var.l2_refe
            var.do_return = True
            if var.l2_refe < 100 * np.finfo(float).tiny:        # zero source: zero field (solver.py:330-337)
                var.l2_refe = np.nan
                var.exit_message = "CONVERGED"
                if sslsolver:           # (as solve(): neither solver runs, the error keeps its initial value)
                    var.sslsolver = None
                    var.cycle = None
                else:
                    var.l2 = 0.0
                active[b] = 0
        if sslsolver:
            _krylov_sources(dev, vars_, active)
        else:
            if not active.all():
                dev.set_mask(active)
            _batched_multigrid(dev, vars_, active)
        efields = [] if download else None
        resp = [] if rec is not None else None
        for b in range(n):
            dev.select(b)
            if rec is not None:
                resp.append(dev.get_receiver_response(rec))
            if download:
                e = fields.Field(grid, dtype=proto.dtype, freq=proto._freq)
                dev.get_efield(np.asarray(e.field))
                efields.append(e)
    finally:
        if handle is None:
            dev.close()
    infos = []
    for var in vars_:
        if var.verb == 1 and var.exit_message != 'CONVERGED':
            var.cprint(f"* WARNING :: {var.exit_message}", 0)
        infos.append(_info_dict(var))
    if rec is not None:
        return efields, infos, np.array(resp)
    return efields, infos


# --------------------------------------------------------------------------
# multigrid / krylov
# --------------------------------------------------------------------------
def multigrid(grid, model, sfield, efield, var, dev=None, **kwargs):
    """Level-0 loop of the multigrid solver (reference emg3d/solver.py:434-607).

    The coarse-level recursion (V/W/F scheduling, restriction, prolongation,
    smoothing) of one cycle runs inside ``emg3d_mg_cycle`` on the device; what
    the reference does once per cycle on the finest grid -- initial residual,
    optional initial smoothing, the end-of-cycle norm, sc_dir/lr_dir rotation,
    logging and the termination tests -- is ``_batched_multigrid``, the loop of
    ``solve_sources`` too, here with one system.  ``efield`` is updated in place.
    """
    if kwargs:
        raise TypeError("the coarse-level recursion lives on the device; `level`/`new_cycmax` "
                        "are not accepted here")
    own = dev is None
    if own:
        dev = DeviceMG(grid, model, sfield.dtype)
        dev.set_params(var)
        dev.set_sfield(sfield)
    trace = var.verb > 4 and dev.nsys == 1
    try:
        if own or not var._dev_efield_current:
            dev.set_efield(efield)
        if _batched_multigrid(dev, [var], [1], trace=trace)[0]:
            raise _ConvergenceError         # a failing preconditioner: var.l2 and the field stay as they are
        if efield is not None:          # None: the caller picks the field up on the device
            dev.get_efield(np.asarray(efield))
    finally:
        if own:
            dev.close()
        elif trace:
            dev.set_trace(False)


# BiCGSTAB with every vector resident on the device.  The reference hands this iteration to
# scipy.sparse.linalg.bicgstab (call site emg3d/solver.py:717-719; SciPy is a third-party
# dependency pinned only as scipy>=1.4.0, setup.py:39).  This is a restatement of that
# routine's published algorithm (SciPy 1.12+: scipy/sparse/linalg/_isolve/iterative.py,
# `bicgstab`: same order of operations, same breakdown tests rhotol = omegatol = eps**2, same
# exit codes 0 / maxiter / -10 / -11, atol = max(atol, rtol*||b||)), with numpy operations
# replaced by emg3d_mg_vec_* calls; pinned by the reference's `res>bicresult` and
# `lap>bicresult` goldens and by the host-SciPy path of this module (tests).
DEVICE_KRYLOV = True
# multigrid() / solve_sources(): set the next cycle's (sc_dir, lr_dir) pair up on the host while the device runs the
# current cycle (emg3d_mg_cycle_next); False: set-up on first use, as emg3d_mg_cycle does.  Same results either way.
PREPARE_AHEAD = True


class _Systems:
    """What the two backends of the Krylov bodies (``_bicgstab``, ``_cgs``) share: which systems still iterate and their
    return codes.  A backend adds the vector primitives the bodies are written on -- ``load``, ``start``, ``copy``,
    ``axpy``, ``scale``, ``dot``, ``norm`` (lists, one entry per system), ``amatvec``, ``psolve``, ``sync``."""

    def __init__(self, dev, psolve, nsys, n, active=None):
        self.dev, self._psolve, self.nsys = dev, psolve, nsys
        self.active = np.zeros(nsys, dtype=np.int32)
        self.active[:n] = 1 if active is None else np.asarray(active)[:n]
        self.codes = [0] * n

    def live(self):
        return [b for b in range(len(self.codes)) if self.active[b]]

    def finish(self, b, code):
        self.active[b] = 0
        self.codes[b] = code

    def finish_where(self, code, hit):
        for b in self.live():
            if hit(b):
                self.finish(b, code)

    def all_finished(self):
        """Freeze on the device what has finished since the last time; has every system?"""
        self.sync()
        return not self.live()

    def each(self, value):
        """[value(b)] for the systems that still iterate, None for the others."""
        return [value(b) if b < len(self.codes) and self.active[b] else None for b in range(self.nsys)]

    def coef(self, values, sign=1):
        """Per-system coefficients for axpy / scale (0 for frozen systems, which the kernels skip); sign -1: -v."""
        return [0.0 if (v is None or not self.active[k]) else (-v if sign < 0 else v) for k, v in enumerate(values)]


class _OneSystem(_Systems):
    """Backend of a single solve: the system the handle has selected, on ``vec_*`` one to one.  No mask, no ``bvec_*``;
    ``b`` and ``x0`` are host arrays, and a ``_ConvergenceError`` of ``psolve(src, dst)`` goes up to ``krylov()``."""
    lockstep = False

    def __init__(self, dev, psolve, b=None, x0=None):
        super().__init__(dev, psolve, 1, 1)
        self.copy, self.amatvec = dev.vec_copy, dev.vec_amatvec
        self.b, self.x0 = b, x0

    def load(self, nvec, X, B):
        self.dev.vec_alloc(nvec)
        self.dev.vec_set(B, self.b)
        self.dev.vec_set(X, self.x0)
        self.X = X

    def start(self, R, RT, B, TMP):
        """r = rt = b - A x0.  (A zero right-hand side has finished: nothing more is issued.)"""
        self.zero_rhs = not self.live()
        if self.zero_rhs:
            return
        if np.any(self.x0):
            _residual_into(self, R, self.X, B, TMP)
        else:
            self.copy(R, B)
        self.copy(RT, R)

    def sync(self, mask=None):
        pass

    def axpy(self, y, coefs, x):
        self.dev.vec_axpy(y, coefs[0] if isinstance(coefs, list) else coefs, x)

    def scale(self, y, coefs):
        self.dev.vec_scale(y, coefs[0])

    def dot(self, a, b):
        return [self.dev.vec_dot(a, b)]

    def norm(self, a):
        return [self.dev.vec_norm(a)]

    def psolve(self, src, dst):
        if self._psolve is None:
            self.copy(dst, src)
        else:
            self._psolve(src, dst)

    def solve(self, body, rtol, maxiter, atol, callback):
        code, = body(self, rtol, maxiter, atol, [callback] if callback else None)
        return (np.array(self.b) if self.zero_rhs else self.dev.vec_get(self.X)), code


class _Lockstep(_Systems):
    """Backend of a batched solve: the first ``n`` systems of a batched handle on ``bvec_*``.  All active systems execute
    iteration k together; a system that returns is frozen (``set_mask``) and its vectors stay as they are from then on.
    The right-hand sides are the level-0 sources in the handle, the start vector is zero."""
    lockstep = True

    def __init__(self, dev, n, active=None, psolve=None, failed=None):
        super().__init__(dev, psolve, dev.nsys, n, active)
        self.copy, self.amatvec, self.axpy, self.scale = dev.bvec_copy, dev.bvec_amatvec, dev.bvec_axpy, dev.bvec_scale
        self.failed = [] if failed is None else failed      # systems whose preconditioner failed (code -1, as krylov() sets it)
        self.cplx = np.dtype(dev.dtype).kind == 'c'
        self._on_device = None

    def load(self, nvec, X, B):
        self.dev.bvec_alloc(nvec)
        self.sync(self.only(range(len(self.codes))))
        self.dev.bvec_zero(X)
        self.sync()
        self.copy(B, self.dev.SFIELD)
        self.X = X

    def start(self, R, RT, B, TMP):
        self.sync()
        self.copy(R, B)
        self.copy(RT, R)

    def sync(self, mask=None):
        """The device's mask <- ``mask`` (default: the active systems), if it is another one."""
        mask = self.active if mask is None else mask
        if self._on_device is None or not np.array_equal(mask, self._on_device):
            self.dev.set_mask(mask)
            self._on_device = np.array(mask, dtype=np.int32)

    def only(self, systems):
        mask = np.zeros(self.nsys, dtype=np.int32)
        mask[list(systems)] = 1
        return mask

    def dot(self, a, b):
        """[vec_dot(a_b, b_b)] as Python scalars (what ``vec_dot`` gives a single solve), None for frozen systems."""
        d = self.dev.bvec_dot(a, b)
        return [(complex(d[k]) if self.cplx else float(d[k])) if k < len(self.codes) and self.active[k] else None
                for k in range(self.nsys)]

    def norm(self, a):
        return [None if v is None else float(np.sqrt(abs(v))) for v in self.dot(a, a)]

    def psolve(self, src, dst):
        """``psolve(src, dst, mask)`` applies the preconditioner to the systems of ``mask`` (the device's mask on entry, and
        again on return) and returns those for which it failed."""
        if self._psolve is None:
            self.copy(dst, src)
            return
        for b in self._psolve(src, dst, self.active.copy()):
            self.sync(self.only([b]))       # as a single solve ends there: the returned field is zero
            self.dev.bvec_zero(self.X)
            self.finish(b, -1)
            self.failed.append(b)
        self.sync()


def _residual_into(ops, dst, X, B, TMP):
    """dst = b - A x"""
    ops.amatvec(TMP, X)
    ops.copy(dst, B)
    ops.axpy(dst, -1.0, TMP)


def _krylov_start(ops, nvec, rtol, atol, X, R, RT, B, TMP):
    """x = x0, r = rt = b - A x0; a system with a zero right-hand side finishes with code 0.  Returns the absolute
    tolerance of every system, max(atol, rtol ||b||), and rhotol."""
    ops.load(nvec, X, B)
    bnrm2 = ops.norm(B)
    tol = [None if v is None else max(float(atol), float(rtol) * float(v)) for v in bnrm2]
    ops.finish_where(0, lambda b: bnrm2[b] == 0)
    ops.start(R, RT, B, TMP)
    return tol, np.finfo(np.dtype(ops.dev.dtype).char).eps ** 2


def _bicgstab(ops, rtol, maxiter, atol, callbacks):
    """The BiCGSTAB iteration (see above) of every system of the backend ``ops`` (``_OneSystem``, ``_Lockstep``).  Every
    system keeps its own rho, alpha, omega and atol and goes through exactly the operations of an iteration of its own;
    it ends with ``ops.finish(b, code)``: 0, maxiter, -10, -11 (-1: its preconditioner failed, the iterate is zero).
    ``callbacks[b]`` gets || s_b - A x_b || after every iteration of system b.  Returns the list of exit codes; the
    iterates are left in vector 0."""
    X, R, RT, P, V, S, T, PH, SH, B, TMP, RES = range(12)
    tol, rhotol = _krylov_start(ops, 12, rtol, atol, X, R, RT, B, TMP)
    omegatol = rhotol
    for iteration in range(maxiter):
        if not ops.live():
            break
        nr = ops.norm(R)
        ops.finish_where(0, lambda b: nr[b] < tol[b])
        if ops.all_finished():
            break
        rho = ops.dot(RT, R)
        ops.finish_where(-10, lambda b: abs(rho[b]) < rhotol)
        if iteration > 0:
            ops.finish_where(-11, lambda b: abs(omega[b]) < omegatol)
            if ops.all_finished():
                break
            beta = ops.each(lambda b: (rho[b] / rho_prev[b]) * (alpha[b] / omega[b]))
            ops.axpy(P, ops.coef(omega, -1), V)         # p -= omega*v
            ops.scale(P, ops.coef(beta))                # p *= beta
            ops.axpy(P, 1.0, R)                         # p += r
        else:
            if ops.all_finished():
                break
            ops.copy(P, R)
        ops.psolve(P, PH)
        if not ops.live():
            break
        ops.amatvec(V, PH)
        rv = ops.dot(RT, V)
        ops.finish_where(-11, lambda b: rv[b] == 0)
        if ops.all_finished():
            break
        alpha = ops.each(lambda b: rho[b] / rv[b])
        ops.axpy(R, ops.coef(alpha, -1), V)             # r -= alpha*v
        ops.copy(S, R)                                  # s = r
        ns = ops.norm(S)
        done = [b for b in ops.live() if ns[b] < tol[b]]
        # x += alpha*phat: the update of a system that converges here and the first of the two updates of the others
        # (nothing reads x in between: the same two operations on x in the same order either way).  In lockstep it is
        # issued once for all systems, before they part; a single solve that goes on issues it after omega, as SciPy.
        if ops.lockstep or done:
            ops.axpy(X, ops.coef(alpha), PH)
        for b in done:
            ops.finish(b, 0)
        if ops.all_finished():
            break
        ops.psolve(S, SH)
        if not ops.live():
            break
        ops.amatvec(T, SH)
        ts, tt = ops.dot(T, S), ops.dot(T, T)
        omega, rho_prev = ops.each(lambda b: ts[b] / tt[b]), rho
        if not ops.lockstep:
            ops.axpy(X, ops.coef(alpha), PH)
        ops.axpy(X, ops.coef(omega), SH)
        ops.axpy(R, ops.coef(omega, -1), T)
        if callbacks:
            _residual_into(ops, RES, X, B, TMP)         # the reference's callback: || sfield - A x ||
            res = ops.norm(RES)
            for b in ops.live():
                callbacks[b](res[b])
    for b in ops.live():
        ops.finish(b, maxiter)
    return ops.codes


def _cgs(ops, rtol, maxiter, atol, callbacks):
    """SciPy's ``cgs`` (the reference's call site emg3d/solver.py:717-719; SciPy >= 1.12 ``_isolve/iterative.py``)
    restated operation by operation on the primitives of the backend ``ops``, as ``_bicgstab`` is: every Krylov vector
    stays in HBM, the host sees two dot products and one norm per iteration.  Same breakdown tests and exit codes."""
    X, R, RT, P, U, Q, PH, VH, UQ, UH, B, TMP = range(12)
    tol, rhotol = _krylov_start(ops, 12, rtol, atol, X, R, RT, B, TMP)
    for iteration in range(maxiter):
        if not ops.live():
            break
        nr = ops.norm(R)
        ops.finish_where(0, lambda b: nr[b] < tol[b])
        if ops.all_finished():
            break
        rho = ops.dot(RT, R)
        ops.finish_where(-10, lambda b: abs(rho[b]) < rhotol)
        if ops.all_finished():
            break
        if iteration > 0:
            beta = ops.each(lambda b: rho[b] / rho_prev[b])
            ops.copy(U, R)                              # u = r + beta q
            ops.axpy(U, ops.coef(beta), Q)
            ops.scale(P, ops.coef(beta))                # p = u + beta (q + beta p)
            ops.axpy(P, 1.0, Q)
            ops.scale(P, ops.coef(beta))
            ops.axpy(P, 1.0, U)
        else:
            ops.copy(P, R)
            ops.copy(U, R)
        ops.psolve(P, PH)
        if not ops.live():
            break
        ops.amatvec(VH, PH)
        rv = ops.dot(RT, VH)
        ops.finish_where(-11, lambda b: rv[b] == 0)
        if ops.all_finished():
            break
        alpha, rho_prev = ops.each(lambda b: rho[b] / rv[b]), rho
        ops.copy(Q, U)                                  # q = u - alpha vhat
        ops.axpy(Q, ops.coef(alpha, -1), VH)
        ops.copy(UQ, U)                                 # uhat = M (u + q)
        ops.axpy(UQ, 1.0, Q)
        ops.psolve(UQ, UH)
        if not ops.live():
            break
        ops.axpy(X, ops.coef(alpha), UH)
        _residual_into(ops, R, X, B, TMP)               # the true residual, as SciPy computes it
        if callbacks:
            res = ops.norm(R)                           # the reference's callback: || sfield - A x ||
            for b in ops.live():
                callbacks[b](res[b])
    for b in ops.live():
        ops.finish(b, maxiter)
    return ops.codes


def _bicgstab_device(dev, b, x0, rtol, maxiter, atol, psolve, callback):
    """``_bicgstab`` for the system the handle has selected, from the host arrays ``b`` and ``x0``: (x, exit code)."""
    return _OneSystem(dev, psolve, b, x0).solve(_bicgstab, rtol, maxiter, atol, callback)


def _cgs_device(dev, b, x0, rtol, maxiter, atol, psolve, callback):
    return _OneSystem(dev, psolve, b, x0).solve(_cgs, rtol, maxiter, atol, callback)


def _bicgstab_device_batched(dev, n, rtol, maxiter, atol, psolve, callbacks, active=None, failed=None):
    """``_bicgstab`` for the first ``n`` systems of a batched handle in lockstep: per system what ``_bicgstab_device``
    gives it alone.  The right-hand sides are the level-0 sources in the handle, the start vector is zero; the iterates
    are left in batched vector 0.  ``psolve(src, dst, mask)``: see ``_Lockstep.psolve``; ``active``: flags, 0 leaves a
    system out from the start.  Returns the list of exit codes; the systems whose preconditioner failed are appended to
    ``failed`` (a code of -1 alone may also be ``maxiter``)."""
    return _bicgstab(_Lockstep(dev, n, active, psolve, failed), rtol, maxiter, atol, callbacks)


def _cgs_device_batched(dev, n, rtol, maxiter, atol, psolve, callbacks, active=None, failed=None):
    """``_cgs`` for the first ``n`` systems of a batched handle in lockstep (see ``_bicgstab_device_batched``)."""
    return _cgs(_Lockstep(dev, n, active, psolve, failed), rtol, maxiter, atol, callbacks)


def _krylov_fits_device(dev, name, m=20, nsys=1):
    """Do the Krylov vectors of the device-resident iteration fit next to the handle?  GCROT(m, k = m) keeps up to about
    5 + 2 (m + 1) + 2 m + 2 nE-sized vectors in HBM (~1.5 GB each at 256^3: ~130 GB), bicgstab / cgs 9 / 10.  When
    they do not fit, the caller runs SciPy's host iteration around the device preconditioner instead of failing in
    ``emg3d_mg_vec_alloc``.  ``nsys``: the batched workspace (``emg3d_mg_bvec_alloc``) holds every vector once per system."""
    need = _krylov_workspace_bytes(dev, name, m, nsys)
    try:
        # what is FREE now (other handles, torch allocations and other processes share the GPU), plus the DEVICE blocks this
        # process's own pool has parked for this device, which the vectors may take (not the blocks of other devices, not the
        # pinned host staging buffers)
        mi = _lib.mem_info(dev.device)
    except Exception:
        return True
    return need < 0.92 * (mi["free"] + mi["pooled_on_device"])


def _krylov_workspace_bytes(dev, name, m=20, nsys=1):
    nvec = {'bicgstab': 9, 'cgs': 10}.get(name, 5 + 2 * (m + 1) + 2 * m + 2)
    return nvec * dev.nE * dev.dtype.itemsize * int(nsys)


def _gcrotmk_device(dev, b, x0, rtol, maxiter, atol, psolve, callback, m=20, k=None):
    """SciPy's ``gcrotmk`` (GCROT(m,k) with its flexible inner GMRES ``_fgmres``; the reference's call site
    emg3d/solver.py:717-719 with SciPy's defaults m = 20, k = m, truncate = 'oldest', no recycled vectors;
    ``_isolve/_gcrotmk.py``) restated operation by operation on ``emg3d_mg_vec_*``: the Krylov, preconditioned and
    outer (C, U) vectors stay in HBM -- allocated as they are needed, recycled between outer iterations --, the host sees
    the dot products and keeps the small matrices (Hessenberg QR by ``scipy.linalg.qr_insert``, ``lstsq``) as SciPy does.
    Same breakdown tests and exit codes."""
    from scipy.linalg import qr_insert, lstsq
    if k is None:
        k = m
    dtype = dev.dtype
    free, top = [], [0]

    def new_vec():
        if free:
            return free.pop()
        top[0] += 1
        dev.vec_alloc(top[0])
        return top[0] - 1

    X, R, B, TMP, RT = new_vec(), new_vec(), new_vec(), new_vec(), new_vec()
    dev.vec_set(B, b)
    dev.vec_set(X, x0)
    ops = _OneSystem(dev, psolve)         # (its b - A x and its identity-or-preconditioner application)
    if np.any(x0):
        _residual_into(ops, R, X, B, TMP)
    else:
        dev.vec_copy(R, B)
    b_norm = dev.vec_norm(B)
    atol = max(float(atol), float(rtol) * float(b_norm))
    if b_norm == 0:
        return np.array(b), 0
    eps = np.finfo(dtype).eps
    CU = []                          # [(c, u)] vector ids, oldest first

    def fgmres(V0, ml, atol_in, cs):
        """_fgmres with right preconditioning; V0 is normalised.  Returns Q, R, B, vs, zs, y (ids in vs / zs)."""
        vs, zs = [V0], []
        Bm = np.zeros((len(cs), ml), dtype=dtype)
        Q = np.ones((1, 1), dtype=dtype)
        Rm = np.zeros((1, 0), dtype=dtype)
        breakdown = False
        j = 0
        for j in range(ml):
            z = new_vec()
            ops.psolve(vs[-1], z)
            w = new_vec()
            dev.vec_amatvec(w, z)
            w_norm = dev.vec_norm(w)
            for i, c in enumerate(cs):              # GCROT projection: orthogonalise against C
                alpha = dev.vec_dot(c, w)
                Bm[i, j] = alpha
                dev.vec_axpy(w, -alpha, c)
            hcur = np.zeros(j + 2, dtype=Q.dtype)
            for i, v in enumerate(vs):              # ... against V
                alpha = dev.vec_dot(v, w)
                hcur[i] = alpha
                dev.vec_axpy(w, -alpha, v)
            hcur[len(vs)] = dev.vec_norm(w)
            with np.errstate(over='ignore', divide='ignore'):
                alpha = 1 / hcur[-1]
            if np.isfinite(alpha):
                dev.vec_scale(w, alpha)
            if not (hcur[-1] > eps * w_norm):
                breakdown = True
            vs.append(w)
            zs.append(z)
            Q2 = np.zeros((j + 2, j + 2), dtype=Q.dtype, order='F')
            Q2[:j + 1, :j + 1] = Q
            Q2[j + 1, j + 1] = 1
            R2 = np.zeros((j + 2, j), dtype=Rm.dtype, order='F')
            R2[:j + 1, :] = Rm
            Q, Rm = qr_insert(Q2, R2, hcur, j, which='col', overwrite_qru=True, check_finite=False)
            res = abs(Q[0, -1])
            if res < atol_in or breakdown:
                break
        if not np.isfinite(Rm[j, j]):
            raise np.linalg.LinAlgError()
        y, _, _, _ = lstsq(Rm[:j + 1, :j + 1], Q[0, :j + 1].conj())
        return Q, Rm, Bm[:, :j + 1], vs, zs, y

    j_outer = -1
    for j_outer in range(maxiter):
        if callback is not None:
            _residual_into(ops, RT, X, B, TMP)
            callback(dev.vec_norm(RT))              # the reference's callback: || sfield - A x ||
        beta = dev.vec_norm(R)
        beta_tol = max(atol, rtol * b_norm)
        if beta <= beta_tol and (j_outer > 0 or CU):
            _residual_into(ops, R, X, B, TMP)       # recompute the residual to avoid rounding error
            beta = dev.vec_norm(R)
        if beta <= beta_tol:
            j_outer = -1
            break
        ml = m + max(k - len(CU), 0)
        cs = [c for c, u in CU]
        V0 = new_vec()
        dev.vec_copy(V0, R)
        dev.vec_scale(V0, 1 / beta)
        try:
            Q, Rm, Bm, vs, zs, y = fgmres(V0, ml, max(atol, rtol * b_norm) / beta, cs)
            y = y * beta
        except np.linalg.LinAlgError:
            break
        # ux := (Z - U B) y
        ux = new_vec()
        dev.vec_copy(ux, zs[0])
        dev.vec_scale(ux, y[0])
        for z, yc in zip(zs[1:], y[1:]):
            dev.vec_axpy(ux, yc, z)
        by = Bm.dot(y)
        for (c, u), byc in zip(CU, by):
            dev.vec_axpy(ux, -byc, u)
        # cx := V H y
        with np.errstate(invalid="ignore"):
            hy = Q.dot(Rm.dot(y))
        cx = new_vec()
        dev.vec_copy(cx, vs[0])
        dev.vec_scale(cx, hy[0])
        for v, hyc in zip(vs[1:], hy[1:]):
            dev.vec_axpy(cx, hyc, v)
        free.extend(vs)                             # the inner vectors are done with
        free.extend(zs)
        try:
            with np.errstate(divide='raise', invalid='raise'):
                alpha = 1 / dev.vec_norm(cx)
            if not np.isfinite(alpha):
                raise FloatingPointError()
        except (FloatingPointError, ZeroDivisionError):
            free.extend([cx, ux])
            continue
        dev.vec_scale(cx, alpha)
        dev.vec_scale(ux, alpha)
        gamma = dev.vec_dot(cx, R)
        dev.vec_axpy(R, -gamma, cx)
        dev.vec_axpy(X, gamma, ux)
        while len(CU) >= k and CU:                  # truncate = 'oldest'
            c, u = CU.pop(0)
            free.extend([c, u])
        CU.append((cx, ux))
    else:
        return dev.vec_get(X), maxiter
    return dev.vec_get(X), j_outer + 1


def _krylov_step(var, l2):
    """End of a Krylov iteration: bookkeeping and log line (solver.py:685-708).  ``l2``: || sfield - A x ||, or a function
    that computes it (after the time of the step is taken, as the reference does)."""
    var._ssl_it += 1
    var.runtime_at_cycle = np.r_[var.runtime_at_cycle, var.time.elapsed]
    var.l2 = l2() if callable(l2) else l2
    var.error_at_cycle = np.r_[var.error_at_cycle, var.l2]
    if var.verb > 3:
        log = f"   [{var.time.now}]   {var.l2/var.l2_refe:.3e} "
        log += f" after {var._ssl_it:3} {var.sslsolver}-cycles"
        if var._ssl_it == 1 and var.it == 0 and var.cycle is not None:
            log += "\n"
        var.cprint(log, 3)
    elif var.verb < 0:
        var.one_liner(var.l2)


def _krylov_exit_message(var, i, failed=False):
    """Exit message from the Krylov driver's return code ``i`` (solver.py:721-734); ``failed``: the preconditioner failed
    (``_ConvergenceError``) and ``i`` is -1."""
    if failed:
        var.exit_message += " (returned field is zero)"
    pre = "\n   > "
    if i < 0:
        if var.exit_message == '':
            var.exit_message = f"Error in {var.sslsolver} ({i})"
        pre = "\n* ERROR   :: "
    elif i > 0:
        var.exit_message = "MAX. ITERATION REACHED, NOT CONVERGED"
    else:
        var.exit_message = "CONVERGED"
    var.cprint(pre + var.exit_message, 2)


def krylov(grid, model, sfield, efield, var, dev=None):
    """Krylov solver preconditioned by multigrid (reference solver.py:610-734).

    ``bicgstab``, ``cgs`` and ``gcrotmk`` run device resident (``_bicgstab_device``, ``_cgs_device``, ``_gcrotmk_device``:
    SciPy's iterations restated on vectors in HBM; gcrotmk's Hessenberg QR / least-squares bookkeeping on small matrices
    stays host work, as in SciPy).  ``solver.DEVICE_KRYLOV = False`` selects SciPy's own iterations on host vectors with
    the operator A x (``core.amat_x``) and the preconditioner (multigrid cycles on a zero field) on the device: 2 x nE x
    16 B cross PCIe per operator or preconditioner application.
    """
    own = dev is None
    if own:
        dev = DeviceMG(grid, model, sfield.dtype)
        dev.set_params(var)
    freq = sfield._freq

    def amatvec(x):
        return dev.amatvec(np.asarray(x))

    A = ssl.LinearOperator(shape=(grid.nE, grid.nE), dtype=sfield.dtype, matvec=amatvec)

    def mg_matvec(b):
        bs = fields.Field(grid, np.ascontiguousarray(b, dtype=sfield.dtype), freq=freq)
        x = fields.Field(grid, dtype=sfield.dtype, freq=freq)
        dev.set_sfield(bs)
        dev.set_efield(None)
        var._dev_efield_current = True
        try:
            multigrid(grid, model, bs, x, var, dev=dev)
        finally:
            var._dev_efield_current = False
        return x

    M = None
    if var.cycle:
        M = ssl.LinearOperator(shape=(grid.nE, grid.nE), dtype=sfield.dtype, matvec=mg_matvec)

    def callback(x):
        if isinstance(x, float):        # device path: the norm of s - A x, computed on the device
            _krylov_step(var, x)
        else:
            _krylov_step(var, lambda: float(np.linalg.norm(np.asarray(sfield) - dev.amatvec(np.asarray(x)))))

    def mg_on_device(src, dst):
        """dst = M src with both vectors on the device (same cycles as mg_matvec)."""
        dev.vec_copy(dev.SFIELD, src)
        dev.set_efield(None)
        var._dev_efield_current = True
        try:
            multigrid(grid, model, None, None, var, dev=dev)
        finally:
            var._dev_efield_current = False
        dev.vec_copy(dst, dev.EFIELD)

    failed = False
    try:
        if var.sslsolver in ('bicgstab', 'cgs', 'gcrotmk') and DEVICE_KRYLOV and _krylov_fits_device(dev, var.sslsolver):
            drive = {'bicgstab': _bicgstab_device, 'cgs': _cgs_device, 'gcrotmk': _gcrotmk_device}[var.sslsolver]
            x, i = drive(dev, np.asarray(sfield), np.asarray(efield), rtol=var.tol, maxiter=var.ssl_maxit, atol=1e-30,
                         psolve=mg_on_device if var.cycle else None, callback=callback)
        else:
            x, i = getattr(ssl, var.sslsolver)(A, np.asarray(sfield), x0=np.array(efield), rtol=var.tol,
                                              maxiter=var.ssl_maxit, atol=1e-30, M=M, callback=callback)
        efield.field = x
    except _ConvergenceError:
        i, failed = -1, True
    finally:
        if own:
            dev.close()
    _krylov_exit_message(var, i, failed)


# --------------------------------------------------------------------------
# Stand-alone sub-routines on host arrays (tier 1)
# --------------------------------------------------------------------------
def smoothing(grid, model, sfield, efield, nu, lr_dir, ordering='lex'):
    """Gauss-Seidel smoothing, in place (reference emg3d/solver.py:738-799)."""
    inp = (sfield.fx, sfield.fy, sfield.fz, model.eta_x, model.eta_y, model.eta_z, model.zeta,
           grid.h[0], grid.h[1], grid.h[2], nu)
    lr_dir = _current_lr_dir(lr_dir, grid)
    order = ORDERINGS[ordering]
    if lr_dir == 0:
        core._gs(0, efield.fx, efield.fy, efield.fz, *inp, order=order)
    if lr_dir in [1, 5, 6, 7]:
        core._gs(1, efield.fx, efield.fy, efield.fz, *inp, order=order)
    if lr_dir in [2, 4, 6, 7]:
        core._gs(2, efield.fx, efield.fy, efield.fz, *inp, order=order)
    if lr_dir in [3, 4, 5, 7]:
        core._gs(3, efield.fx, efield.fy, efield.fz, *inp, order=order)


class _CoarseModel:
    """Coarse-grid VolumeModel stand-in (eta_x/y/z, zeta, case)."""

    def __init__(self, case):
        self.case = case


def _restrict_model_parameters(param, sc_dir):
    """Coarse model parameter = sum of the merged fine cells (solver.py:1747-1784)."""
    lib = _lib.load()
    param = np.asarray(param)
    is_c = int(param.dtype == np.complex128)
    dt = np.complex128 if is_c else np.float64
    p = np.ascontiguousarray(np.asarray(param, dtype=dt).ravel(order='F'))
    nx, ny, nz = param.shape
    cshape = (nx if sc_dir in [1, 5, 6] else nx // 2, ny if sc_dir in [2, 4, 6] else ny // 2,
              nz if sc_dir in [3, 4, 5] else nz // 2)
    out = np.empty(int(np.prod(cshape)), dtype=dt)
    _lib.check(lib.emg3d_restrict_model(is_c, nx, ny, nz, _lib.ptr(out), _lib.ptr(p), int(sc_dir)),
               "emg3d_restrict_model")
    return out.reshape(cshape, order='F')


def restriction(grid, model, sfield, residual, sc_dir):
    """Coarse grid, model and source from the fine ones (solver.py:802-901)."""
    rx = 1 if sc_dir in [1, 5, 6] else 2
    ry = 1 if sc_dir in [2, 4, 6] else 2
    rz = 1 if sc_dir in [3, 4, 5] else 2
    ch = [np.diff(grid.nodes_x[::rx]), np.diff(grid.nodes_y[::ry]), np.diff(grid.nodes_z[::rz])]
    cgrid = meshes.TensorMesh(ch, grid.origin)

    cmodel = _CoarseModel(model.case)
    cmodel.eta_x = _restrict_model_parameters(model.eta_x, sc_dir)
    cmodel.eta_y = _restrict_model_parameters(model.eta_y, sc_dir) if model.case in [1, 3] else cmodel.eta_x
    cmodel.eta_z = _restrict_model_parameters(model.eta_z, sc_dir) if model.case in [2, 3] else cmodel.eta_x
    cmodel.zeta = _restrict_model_parameters(model.zeta, sc_dir)

    wx, wy, wz = _get_restriction_weights(grid, cgrid, sc_dir)
    csfield = fields.Field(cgrid, dtype=sfield.dtype, freq=sfield._freq)
    core.restrict(csfield.fx, csfield.fy, csfield.fz, residual.fx, residual.fy, residual.fz,
                  wx, wy, wz, sc_dir)
    csfield.ensure_pec
    cefield = fields.Field(cgrid, dtype=sfield.dtype, freq=sfield._freq)
    return cgrid, cmodel, csfield, cefield


def prolongation(grid, efield, cgrid, cefield, sc_dir):
    """efield += P cefield, then PEC (reference emg3d/solver.py:904-977)."""
    lib = _lib.load()
    dt = _lib.dtype_code(efield.dtype)
    hx, hy, hz = (np.ascontiguousarray(h, dtype=np.float64) for h in grid.h)
    origin = np.ascontiguousarray(grid.origin, dtype=np.float64)
    e = np.ascontiguousarray(np.asarray(efield))
    ce = np.ascontiguousarray(np.asarray(cefield), dtype=e.dtype)
    _lib.check(lib.emg3d_prolongation(dt, *(int(n) for n in grid.vnC), _lib.ptr(hx), _lib.ptr(hy),
                                      _lib.ptr(hz), _lib.ptr(origin), _lib.ptr(e), _lib.ptr(ce),
                                      int(sc_dir)), "emg3d_prolongation")
    if e is not np.asarray(efield):
        efield.field = e
    else:
        np.asarray(efield)[...] = e


def residual(grid, model, sfield, efield, norm=False):
    """Residual field s - A e, or its l2-norm (reference solver.py:980-1039)."""
    rfield = sfield.copy()
    core.amat_x(rfield.fx, rfield.fy, rfield.fz, efield.fx, efield.fy, efield.fz, model.eta_x,
                model.eta_y, model.eta_z, model.zeta, grid.h[0], grid.h[1], grid.h[2])
    if norm:
        return float(np.linalg.norm(rfield))
    return rfield


# --------------------------------------------------------------------------
# Parameters
# --------------------------------------------------------------------------
class _Time:
    """Wall-clock helper with the reference's formatting (utils.py:604-634)."""

    def __init__(self):
        self._t0 = time.perf_counter()

    @property
    def now(self):
        return datetime.now().strftime("%H:%M:%S")

    @property
    def elapsed(self):
        return time.perf_counter() - self._t0

    @property
    def runtime(self):
        return str(timedelta(seconds=np.round(self.elapsed)))


@dataclass
class MGParameters:
    """Multigrid settings; mirrors emg3d/solver.py:1043-1364."""

    verb: int
    cycle: str
    sslsolver: str
    linerelaxation: int
    semicoarsening: int
    vnC: tuple

    tol: float = 1e-6
    maxit: int = 50
    nu_init: int = 0
    nu_pre: int = 2
    nu_coarse: int = 1
    nu_post: int = 2
    clevel: int = -1
    return_info: bool = False
    log: int = 1
    log_message: str = ''
    ordering: str = 'colour'

    def __post_init__(self):
        if self.ordering not in ORDERINGS:
            raise ValueError(f"`ordering` must be one of {list(ORDERINGS)}; provided: {self.ordering!r}.")
        self._first_cycle = True
        self._dev_efield_current = False
        self.it = 0
        self._ssl_it = 0
        self.l2 = 1.0
        self.l2_refe = 1.0
        self.exit_message = ''
        self.time = _Time()
        self.runtime_at_cycle = np.array([0.])
        self.error_at_cycle = np.array([0.])
        self.do_return = True
        self._semicoarsening()
        self._linerelaxation()
        self._solver_and_cycle()
        self.max_level

    def __repr__(self):
        n = self.vnC
        p = self.pclevel
        return (f"   MG-cycle       : {self.cycle!r:17}   sslsolver : {self.sslsolver!r}\n"
                f"   semicoarsening : {self._p_sc_dir:17}   tol       : {self.tol}\n"
                f"   linerelaxation : {self._p_lr_dir:17}   maxit     : {self._maxit}\n"
                f"   nu_{{i,1,c,2}}   : {self.nu_init}, {self.nu_pre}, {self.nu_coarse}, "
                f"{self.nu_post}          verb      : {self.verb}\n"
                f"   Original grid  : {n[0]:3} x {n[1]:3} x {n[2]:3}     => {n[0]*n[1]*n[2]:,} cells\n"
                f"   Coarsest grid  : {p['vnC'][0]:3} x {p['vnC'][1]:3} x {p['vnC'][2]:3}     "
                f"=> {p['nC']:,} cells\n"
                f"   Coarsest level : {p['clevel'][0]:3} ; {p['clevel'][1]:3} ;{p['clevel'][2]:4}   "
                f"{p['message']}\n"
                f"   ordering       : {self.ordering}\n")

    @staticmethod
    def _halvings(n):
        """How often ``n`` cells can be halved with at least two cells left: the trailing zero bits of ``n``, one fewer for a
        pure power of two (2^k stops at two cells)."""
        n = int(n)
        if n < 2:
            return 0
        tz = (n & -n).bit_length() - 1
        return tz - 1 if n >> tz == 1 else tz

    @property
    def max_level(self):
        """Coarsening depth per dimension, limited by the user's ``clevel``; sets ``clevel`` (the depth for sc_dir 0..3),
        ``pclevel`` (coarsest grid, for the log) and the "not optimal" note (behaviour of solver.py:1142-1206)."""
        asked = self.clevel
        cap = np.inf if asked < 0 else asked
        depth = np.array([self._halvings(n) for n in self.vnC], dtype=np.int_)
        if asked >= 0:
            depth = np.minimum(depth, asked).astype(np.int_)
        coarse = tuple(int(n) >> int(d) for n, d in zip(self.vnC, depth))
        # sc_dir d leaves dimension d alone: its depth is the deepest of the other two (sc_dir 0: of all three)
        self.clevel = np.array([depth.max()] + [max(depth[k] for k in range(3) if k != d) for d in range(3)])
        stuck_large = any(d < cap and c > 7 for d, c in zip(depth, coarse))      # stopped by an odd factor with > 7 cells left
        shallow = bool(np.any(depth < min(cap, 3)))                               # fewer than three halvings somewhere
        self.pclevel = {'nC': int(np.prod(coarse)), 'vnC': coarse, 'clevel': depth,
                        'message': "  :: Grid not optimal for MG solver ::" if (stuck_large or shallow) else ""}
        if min(self.vnC) < 2:
            raise ValueError("Nr. of cells must be at least two in each direction\n"
                             f"Provided shape: ({self.vnC[0]}, {self.vnC[1]}, {self.vnC[2]}).")

    def cprint(self, info, verbosity, **kwargs):
        """Print/log ``info`` if ``verb`` > ``verbosity`` (solver.py:1208-1229)."""
        if self.verb > verbosity:
            if self.log != 0:
                self.log_message += str(info) + '\n'
            if self.log >= 0:
                print(info, **kwargs)

    def one_liner(self, l2_last, last=False):
        info = f":: emg3d :: {l2_last/self.l2_refe:.1e}; "
        info += f"{self._ssl_it}({self.it}); " if self.sslsolver else f"{self.it}; "
        info += f"{self.time.runtime}"
        if last:
            self.cprint(info + f"; {self.exit_message}", -100)
        else:
            self.cprint(info, -100, end='\r')

    def _digits(self, value, true_cycle, nmax, name, allowed, combo):
        if value is True:
            raw = np.array(true_cycle)
            return itertools.cycle(raw), raw
        if value in np.arange(nmax):
            return False, np.array([int(value)])
        raw = np.array([int(x) for x in str(abs(value))])
        if np.any(raw < 0) or np.any(raw >= nmax):
            raise ValueError(f"`{name}` must be one of {allowed}.\n"
                             f"{' ':>13} Or a combination of {combo} to cycle, e.g. 1213.\n"
                             f"{'Provided:':>23} {name}={value}.")
        return itertools.cycle(raw), raw

    def _semicoarsening(self):
        self.sc_cycle, raw = self._digits(self.semicoarsening, [1, 2, 3], 4, 'semicoarsening',
                                          "(False, True, 0, 1, 2, 3)", "(0, 1, 2, 3)")
        self.sc_dir = next(self.sc_cycle) if self.sc_cycle else raw[0]
        self.semicoarsening = self.sc_dir != 0
        self._p_sc_dir = f"{self.semicoarsening} {raw}"
        self._raw_sc_cycle = raw

    def _linerelaxation(self):
        self.lr_cycle, raw = self._digits(self.linerelaxation, [4, 5, 6], 8, 'linerelaxation',
                                          "(False, True, 0, 1, 2, 3, 4, 5, 6, 7)", "(1, 2, 3, 4, 5, 6, 7)")
        self.lr_dir = next(self.lr_cycle) if self.lr_cycle else raw[0]
        self.linerelaxation = self.lr_dir != 0
        self._p_lr_dir = f"{self.linerelaxation} {raw}"
        self._raw_lr_cycle = raw

    def _solver_and_cycle(self):
        """Validate the (sslsolver, cycle) pair and derive cycmax / the iteration limits (behaviour of solver.py:1327-1364)."""
        known = ['bicgstab', 'cgs', 'gcrotmk']
        given = self.sslsolver
        if given is not True and given is not False and given not in known:
            raise ValueError(f"`sslsolver` must be True, False, or one of {known}.\n"
                             f"Provided: sslsolver={given!r}.")
        self.sslsolver = known[0] if given is True else given
        if self.cycle not in ('F', 'V', 'W', None):
            raise ValueError("`cycle` must be one of {'F', 'V', 'W', None}.\n"
                             f"Provided: cycle={self.cycle}.")
        if self.cycle is None and not self.sslsolver:
            raise ValueError("At least `cycle` or `sslsolver` is required.\nProvided"
                             f"input: cycle={self.cycle}; sslsolver={self.sslsolver}.")
        self.cycmax = {'F': 2, 'W': 2}.get(self.cycle, 1)
        # one multigrid iteration per entry of the longer of the two rotation lists when it preconditions a Krylov solver
        self._maxcycle = max(len(self._raw_sc_cycle), len(self._raw_lr_cycle))
        self._maxit = f"{self.maxit}"
        self.ssl_maxit = self.maxit if self.sslsolver else 0
        if self.sslsolver and self.cycle is not None:
            self.maxit = self._maxcycle
            self._maxit += f" ({self.maxit})"


# --------------------------------------------------------------------------
# Helpers
# --------------------------------------------------------------------------
class RegularGridProlongator:
    """Bilinear interpolation from a coarse tensor grid ``(x, y)`` to fixed points ``cxy``
    (interface and semantics of the reference's class, emg3d/solver.py:1368-1463: linear, no bounds
    error, linear EXTRApolation outside, cell index ``searchsorted - 1`` clipped to the last interval).

    The interval index and the four corner weights of every point are computed once; a call gathers the
    four corners of a 2-D value array and adds them in the order (0,0), (0,1), (1,0), (1,1) -- the
    arithmetic that the device kernel ``k_prolong`` reproduces (its weights come from the same rule,
    ``prolong_weights_host`` in csrc/mg.hpp).  Host-side: used by tests and by code written against
    the reference; the product path prolongates on the device.
    """

    def __init__(self, x, y, cxy):
        cxy = np.asarray(cxy, dtype=np.float64)
        self.size = cxy.shape[0]
        idx, frac = [], []
        for pts, nodes in zip(cxy.T, (np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))):
            i = np.clip(np.searchsorted(nodes, pts) - 1, 0, nodes.size - 2)
            idx.append(i)
            frac.append((pts - nodes[i]) / (nodes[i + 1] - nodes[i]))
        (ix, iy), (tx, ty) = idx, frac
        self._corners = ((ix, iy), (ix, iy + 1), (ix + 1, iy), (ix + 1, iy + 1))
        self.weight = np.array([(1 - tx) * (1 - ty), (1 - tx) * ty, tx * (1 - ty), tx * ty])

    def __call__(self, values):
        values = np.asarray(values)
        result = 0.
        for corner, w in zip(self._corners, self.weight):
            result = result + values[corner] * w
        return result


def _get_prolongation_coordinates(grid, d1, d2):
    """All (d1, d2) node coordinate pairs of ``grid``, d1 running fastest (reference
    emg3d/solver.py:1841-1845): the points at which a coarse field is evaluated for prolongation."""
    n1 = np.asarray(getattr(grid, 'nodes_' + d1), dtype=np.float64)
    n2 = np.asarray(getattr(grid, 'nodes_' + d2), dtype=np.float64)
    out = np.empty((n1.size * n2.size, 2))
    out[:, 0] = np.tile(n1, n2.size)
    out[:, 1] = np.repeat(n2, n1.size)
    return out


def _current_sc_dir(sc_dir, grid):
    """Actual coarsening code 0..6 for this grid (solver.py:1467-1514)."""
    n = grid.vnC
    xs = n[0] % 2 != 0 or n[0] < 3 or sc_dir == 1
    ys = n[1] % 2 != 0 or n[1] < 3 or sc_dir == 2
    zs = n[2] % 2 != 0 or n[2] < 3 or sc_dir == 3
    if xs:
        if ys:
            return 6
        return 5 if zs else 1
    if ys:
        return 4 if zs else 2
    return 3 if zs else 0


def _current_lr_dir(lr_dir, grid):
    """Drop line relaxation along 2-cell dimensions (solver.py:1517-1572)."""
    lr_dir = int(lr_dir)
    n = grid.vnC
    if n[0] == 2:
        lr_dir = {1: 0, 5: 3, 6: 2, 7: 4}.get(lr_dir, lr_dir)
    if n[1] == 2:
        lr_dir = {2: 0, 4: 3, 6: 1, 7: 5}.get(lr_dir, lr_dir)
    if n[2] == 2:
        lr_dir = {3: 0, 4: 2, 5: 1, 7: 6}.get(lr_dir, lr_dir)
    return lr_dir


def _first_cycle_levels(var):
    """The levels in the order ``solver.multigrid`` enters and re-enters them during the FIRST cycle (the reference
    records them for its cycle-QC figure, solver.py:494-496 and 565-567).  The recursion itself runs on the device
    (``MG<T>::mg_level``); this is the same V/W/F rule (solver.py:478-485, 519, 585-586) on level numbers only."""
    coarsest = int(var.clevel[var.sc_dir])
    seq = []

    def visit(level, new_cycmax):
        if level == coarsest:
            cycmax = 1
        elif new_cycmax == 0 or var.cycle != 'F':
            cycmax = var.cycmax
        else:
            cycmax = new_cycmax
        seq.append(level)
        it = cyc = 0
        while level == 0 or it < cycmax:
            if level != coarsest:
                visit(level + 1, cycmax - cyc)
                seq.append(level)
            it += 1
            if level == 0:
                break           # the figure is drawn at the end of the first level-0 iteration
            cyc += 1

    visit(0, 0)
    return seq


def _cycle_qc_figure(levels):
    """ASCII picture of one multigrid cycle, the format of the reference's log at verb > 3 (solver.py:1603-1632): one row
    per coarse level, a backslash where the cycle steps down into that level, a slash where it comes back up; at most
    70 steps."""
    lv = np.asarray(levels, dtype=np.int_)
    top = int(lv.max()) if lv.size else 0
    step = ((lv[1:] + lv[:-1]) // 2 + 1) * (lv[1:] - lv[:-1])      # +k: down into level k, -k: up out of it
    shown = step[:70]
    rows = ["       h_"]
    for k in range(1, top + 1):
        rows.append(f"   {2**k:4}h_ " + "".join("\\" if v == k else "/" if v == -k else " " for v in shown))
    out = "\n".join(rows) + ("\n\n" if top > 0 else "\n\n\n")
    if step.size > 70:
        out += f"  (Cycle-QC restricted to first 70 steps of {step.size} steps.)\n"
    return out


def _print_gs_info(it, level, cycmax, vnC, norm):
    """Info string logged after a smoothing call at verb = 5 (solver.py:1651-1680)."""
    return f"     {it:2} {level} {cycmax} [{vnC[0]:3}, {vnC[1]:3}, {vnC[2]:3}]: {norm:.3e} "


def _print_cycle_info(var, l2_last, l2_prev):
    """Bookkeeping + log line at the end of a cycle (solver.py:1575-1648), with the cycle-QC figure in front of the
    first cycle's line at verb > 3 and a blank line before and after the line at verb > 4."""
    var.runtime_at_cycle = np.r_[var.runtime_at_cycle, var.time.elapsed]
    var.error_at_cycle = np.r_[var.error_at_cycle, l2_last]
    if var.verb < 0:
        var.one_liner(l2_last)
        return
    elif var.verb < 4:
        return
    info = "\n" if var.verb > 4 else ""
    if var._first_cycle:
        info += _cycle_qc_figure(_first_cycle_levels(var))
        var._first_cycle = False
    info += f"   [{var.time.now}]   {l2_last/var.l2_refe:.3e}  "
    if var.sslsolver:
        info += f"after {19*' '} {var.it:3} {var.cycle}-cycles "
    else:
        info += f"after {var.it:3} {var.cycle}-cycles   "
        info += f"[{l2_last:.3e}, {l2_last/l2_prev:.3f}]"
    info += f"   {var.lr_dir} {var.sc_dir}"
    if var.verb > 4:
        info += "\n"
    var.cprint(info, 3)


def _terminate(var, l2_last, l2_stag, it):
    """End of an iteration: converged / diverged / stagnated / out of iterations, tested in that order (behaviour of
    solver.py:1682-1744).  A failing preconditioner aborts the Krylov solver through _ConvergenceError."""
    ref = var.l2_refe
    if l2_last < var.tol * ref:
        verdict, failed = "CONVERGED", False
    elif not np.isfinite(l2_last) or l2_last > 10 * ref:
        verdict, failed = "DIVERGED", True
    elif it > 2 and l2_last >= l2_stag:
        verdict, failed = "STAGNATED", True
    elif it == var.maxit:
        verdict, failed = (None if var.sslsolver else "MAX. ITERATION REACHED, NOT CONVERGED"), False
    else:
        return False
    if verdict is not None:
        var.exit_message = verdict
    if var.sslsolver:
        if failed:
            raise _ConvergenceError
    else:
        var.cprint(("\n" if var.verb < 5 else "") + "   > " + var.exit_message, 2)
    return True


def _get_restriction_weights(grid, cgrid, sc_dir):
    """Restriction weights per axis; dummies for non-coarsened axes
    (solver.py:1787-1838)."""
    out = []
    axes = (('x', [1, 5, 6]), ('y', [2, 4, 6]), ('z', [3, 4, 5]))
    for a, (c, skip) in enumerate(axes):
        if sc_dir not in skip:
            out.append(core.restrict_weights(
                getattr(grid, 'nodes_' + c), getattr(grid, 'cell_centers_' + c), grid.h[a],
                getattr(cgrid, 'nodes_' + c), getattr(cgrid, 'cell_centers_' + c), cgrid.h[a]))
        else:
            wlr = np.zeros(grid.vnN[a], dtype=np.float64)
            w0 = np.ones(grid.vnN[a], dtype=np.float64)
            out.append((wlr, w0, wlr))
    return out


class _ConvergenceError(Exception):
    """Raised inside the preconditioner to abort the SciPy solver."""
    pass
