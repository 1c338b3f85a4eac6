"""
Generate tests/golden/receiver_adjoint.npz by IMPORTING the reference (emg3d v0.17.0) at run time, exactly as make_golden.py
does (`_import_reference`: no-op numba stub; nothing of the reference is written into this repository: the fixture holds inputs
and expected outputs only).

The transposes of the receiver operators, from DENSE matrices that the reference's own functions fill column by column:

  P_e     (n_rec x nE)   fields.get_receiver_response of unit electric fields: the cubic-spline receivers
  P_f     (n_rec x nH)   the same of unit magnetic (face) fields
  P_fl    (n_rec x nH)   trilinear weights on the trimmed face points (the reference v0.17.0 has no linear receivers: own
                         restatement, asserted here against the reference's maps.interp3d(method='linear') on a random field)
  C       (nH x nE)      fields.get_h_field of unit electric fields (sparse), H = C e = -curl e / (s mu_0), frequency domain; the
                         Laplace-domain C is this one times smu0_c / smu0_r (the curl itself is real)

on two grids: A = the grid, receivers and frequency of gradient.npz (12 x 10 x 8, every component cubic) and B = 8 x 5 x 6 (the
y-component has three trimmed points along y and falls back to linear; several axes have exactly four trimmed points), six
receivers: interior, first intervals, on a node, NaN datum, far outside (not NaN: the index spline turns back), last intervals.
A receiver whose row is NaN contributes nothing: its row is zeroed before the transpose is applied.

  {A,B}_{hx,hy,hz,origin,rec,freq}, {A,B}_nan   inputs, and which receivers have a NaN datum (cubic electric / magnetic / linear
                                                magnetic: rows of a (3, n_rec) array)
  w_c, w_r                                      complex and real (Laplace domain) data-space vectors (the first n_rec are used)
  {A,B}_{el_cubic,mag_cubic,mag_linear}_{c,r}   P^T w on the edges ([fx|fy|fz]); magnetic: (P C)^T w
  smu0_c, smu0_r                                s mu_0 of +freq and -freq
  gap_cubic_ref, gap_mag_cubic_ref, gap_mag_linear_ref
        on A with the isotropic model, v and w of jacobian.npz, in the arithmetic of its adjoint_gap_ref:
        |Re sum conj(w) (P de) - v . J^T w| / |Re sum ...|, de and lam = A^-1 P^T conj(w) from reference solves at tol 1e-8

Run:  python tests/golden/make_receiver_adjoint_golden.py      (a few minutes without numba)
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

REC_B = np.array([[10., 5., -20., 30., 20.],          # interior
                  [-130., -45., -75., 0., 0.],        # first intervals
                  [-60., -30., -20., 110., -35.],     # exactly on a node
                  [-175., -70., -95., 0., 0.],        # NaN datum
                  [400., 0., 0., 0., 0.],             # far outside, not NaN
                  [120., 45., 50., -60., 15.]]).T     # last intervals


def face_shapes(vnC):
    nx, ny, nz = (int(n) for n in vnC)
    return ((nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1))


def edge_shapes(vnC):
    nx, ny, nz = (int(n) for n in vnC)
    return ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))


def linear_face_matrix(grid, rec, fac):
    """Dense trilinear receiver matrix on the trimmed face points (NaN row: a receiver outside them on an active component)."""
    shp = face_shapes(grid.vnC)
    off = np.cumsum([0] + [int(np.prod(s)) for s in shp])
    points = ((grid.nodes_x, grid.cell_centers_y, grid.cell_centers_z), (grid.cell_centers_x, grid.nodes_y, grid.cell_centers_z),
              (grid.cell_centers_x, grid.cell_centers_y, grid.nodes_z))
    nrec = fac.shape[1]
    P = np.zeros((nrec, off[-1]))
    for c in range(3):
        if not np.any(abs(fac[c]) > 1e-10):
            continue
        for r in range(nrec):
            idx, t = [], []
            for a in range(3):
                p = points[c][a][1:-1]
                x = rec[a][r]
                if not (p[0] <= x <= p[-1]):
                    P[r, :] = np.nan
                i = int(np.clip(np.searchsorted(p, x, side='left') - 1, 0, p.size - 2))
                idx.append(i + 1)
                t.append((x - p[i]) / (p[i + 1] - p[i]))
            for d0 in (0, 1):
                for d1 in (0, 1):
                    for d2 in (0, 1):
                        wgt = (t[0] if d0 else 1 - t[0]) * (t[1] if d1 else 1 - t[1]) * (t[2] if d2 else 1 - t[2])
                        lin = (idx[0] + d0) + shp[c][0] * ((idx[1] + d1) + shp[c][1] * (idx[2] + d2))
                        P[r, off[c] + lin] += fac[c][r] * wgt
    return P, points


def operators(emg3d, grid, rec, freq):
    """-> P_e, P_f, P_fl (dense, real, NaN rows kept) and C (sparse, complex)."""
    fields, models, maps = emg3d.fields, emg3d.models, emg3d.maps
    nrec = max(np.atleast_1d(c).size for c in rec)
    model = models.Model(grid, 1.0)
    nE = grid.nE
    eshp, fshp = edge_shapes(grid.vnC), face_shapes(grid.vnC)
    nH = sum(int(np.prod(s)) for s in fshp)
    foff = np.cumsum([0] + [int(np.prod(s)) for s in fshp])
    P_e = np.zeros((nrec, nE))
    cols, rows, vals = [], [], []
    unit = np.zeros(nE, dtype=complex)
    for j in range(nE):
        unit[j] = 1.0
        e = fields.Field(grid, unit, freq=freq)
        P_e[:, j] = np.real(fields.get_receiver_response(grid, e, rec))
        h = np.asarray(fields.get_h_field(grid, model, e))
        nz = np.flatnonzero(h)
        rows += list(nz); cols += [j] * nz.size; vals += list(h[nz])
        unit[j] = 0.0
    C = sp.csr_matrix((vals, (rows, cols)), shape=(nH, nE), dtype=complex)
    P_f = np.zeros((nrec, nH))
    unit = np.zeros(nH, dtype=complex)
    for j in range(nH):
        unit[j] = 1.0
        hf = fields.Field(*(unit[foff[c]:foff[c + 1]].reshape(fshp[c], order='F') for c in range(3)))
        assert not hf.is_electric
        P_f[:, j] = np.real(fields.get_receiver_response(grid, hf, rec))
        unit[j] = 0.0
    fac = np.array([np.broadcast_to(f, (nrec,)) for f in fields._rotation(*rec[3:])])
    P_fl, points = linear_face_matrix(grid, rec, fac)
    # the restatement against the reference's own linear interpolation, on a random face field
    rng = np.random.default_rng(3)
    hv = rng.standard_normal(nH)
    chk = np.zeros(nrec)
    for c in range(3):
        if np.any(abs(fac[c]) > 1e-10):
            comp = hv[foff[c]:foff[c + 1]].reshape(fshp[c], order='F')
            chk = chk + fac[c] * maps.interp3d(tuple(p[1:-1] for p in points[c]), comp[1:-1, 1:-1, 1:-1], tuple(rec[:3]),
                                               method='linear', fill_value=np.nan, mode='constant', cval=np.nan)
    ok = ~np.isnan(P_fl[:, 0])
    assert np.array_equal(np.isnan(chk), ~ok)
    assert np.abs(chk[ok] - P_fl[ok] @ hv).max() < 1e-13 * np.abs(chk[ok]).max()
    return P_e, P_f, P_fl, C


def zeroed(P):
    """(P with its NaN rows zeroed, which rows were NaN)"""
    nan = np.isnan(P).any(axis=1)
    Q = np.where(nan[:, None], 0.0, P)
    assert np.isfinite(Q).all()
    return Q, nan


def main():
    emg3d = _import_reference()
    from emg3d import fields, meshes, models, maps, solver
    g = np.load(os.path.join(HERE, 'gradient.npz'))
    j = np.load(os.path.join(HERE, 'jacobian.npz'))
    freq = float(g['freq'])
    grid_a = meshes.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    grid_b = meshes.TensorMesh([np.array([80., 60, 50, 50, 50, 55, 70, 90]), np.array([70., 50, 50, 60, 80]),
                                np.array([60., 40, 40, 45, 60, 90])], origin=np.array([-250., -150., -160.]))
    smu0_c = complex(fields.Field(grid_a, freq=freq).smu0)
    smu0_r = float(np.real(fields.Field(grid_a, freq=-freq).smu0))
    rng = np.random.default_rng(104)
    out = dict(smu0_c=np.array(smu0_c), smu0_r=np.array(smu0_r))
    w_c = rng.standard_normal(16) + 1j * rng.standard_normal(16)          # a grid with n receivers uses the first n
    w_r = rng.standard_normal(16)
    out.update(w_c=w_c, w_r=w_r)
    ops = {}
    for tag, grid, rec in (('A', grid_a, tuple(np.array(r, dtype=float) for r in g['rec'])), ('B', grid_b, tuple(REC_B))):
        nrec = rec[0].size
        assert nrec <= w_c.size
        P_e, P_f, P_fl, C = operators(emg3d, grid, rec, freq)
        (Q_e, nan_e), (Q_f, nan_f), (Q_fl, nan_fl) = zeroed(P_e), zeroed(P_f), zeroed(P_fl)
        print(f'{tag}: NaN receivers  cubic electric {np.flatnonzero(nan_e)}, cubic magnetic {np.flatnonzero(nan_f)}, '
              f'linear magnetic {np.flatnonzero(nan_fl)}')
        assert nan_e.sum() <= 1
        if tag == 'B':
            assert list(np.flatnonzero(nan_e)) == [3]
        out.update({f'{tag}_hx': grid.h[0], f'{tag}_hy': grid.h[1], f'{tag}_hz': grid.h[2], f'{tag}_origin': np.array(grid.origin),
                    f'{tag}_rec': np.array(rec), f'{tag}_freq': freq, f'{tag}_nan': np.array([nan_e, nan_f, nan_fl])})
        CT = C.T.tocsr()
        for sfx, w, scale in (('c', w_c[:nrec], 1.0), ('r', w_r[:nrec], smu0_c / smu0_r)):
            out[f'{tag}_el_cubic_{sfx}'] = Q_e.T @ w
            for key, Q in (('mag_cubic', Q_f), ('mag_linear', Q_fl)):
                val = scale * (CT @ (Q.T @ w).astype(complex))
                if sfx == 'r':
                    assert np.abs(val.imag).max() <= 1e-14 * np.abs(val).max()
                    val = val.real.copy()
                out[f'{tag}_{key}_{sfx}'] = val
        ops[tag] = (Q_e, Q_f, Q_fl, C)

    # ---- reference-side adjoint gaps of the three new pairs on A (arithmetic of make_jacobian_golden.py) -------------------
    grid = grid_a
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    sig = j['iso_sig_x']
    model = models.Model(grid, sig, mapping='Conductivity')
    opts = dict(cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-8, verb=1, maxit=100)
    e0 = fields.Field(grid, j['iso_efield'].copy(), freq=freq)
    v, w = j['iso_v'], j['iso_w']
    de = solver.solve(grid, model, fields.SourceField(grid, j['iso_full_src'].copy(), freq=freq), **opts)
    Q_e, Q_f, Q_fl, C = ops['A']
    PH, PHl = (C.T @ Q_f.T).T, (C.T @ Q_fl.T).T            # dense (n_rec x nE), complex
    for key, P in (('gap_cubic_ref', Q_e.astype(complex)), ('gap_mag_cubic_ref', PH), ('gap_mag_linear_ref', PHl)):
        jv = P @ np.array(de)
        jt_src = (P.T @ np.conj(w)).astype(complex)
        lam = solver.solve(grid, model, fields.SourceField(grid, jt_src, freq=freq), **opts)
        prod = fields.Field(grid, (-np.real(lam * e0 * e0.smu0)).astype(np.float64), freq=-1.)
        gx = np.zeros(grid.vnC, order='F'); gy = gx.copy(); gz = gx.copy()
        maps.edges2cellaverages(ex=prod.fx, ey=prod.fy, ez=prod.fz, vol=vol, out_x=gx, out_y=gy, out_z=gz)
        jt = -(gx + gy + gz)
        lhs = np.real(np.sum(np.conj(w) * jv))
        rhs = np.sum(jt.ravel('F') * v)
        gap = abs(lhs - rhs) / abs(lhs)
        print(f'{key}: Re sum conj(w) (J v) = {lhs:.10e}, v . J^T w = {rhs:.10e}, adjoint gap {gap:.3e}')
        assert gap < 1e-4       # (the error of two solves at tol 1e-8; the curl in the magnetic data amplifies it)
        out[key] = gap
    np.savez_compressed(os.path.join(HERE, 'receiver_adjoint.npz'), **out)
    print('wrote receiver_adjoint.npz', os.path.getsize(os.path.join(HERE, 'receiver_adjoint.npz')), 'bytes')


if __name__ == '__main__':
    main()
