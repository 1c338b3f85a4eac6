"""
Generate tests/golden/jacobian.npz by IMPORTING the reference (emg3d v0.17.0) at run time, exactly as make_golden.py does
(`_import_reference`: no-op numba stub; nothing of the reference is written into this repository: the fixture holds inputs
and expected outputs only).

The products J v and J^T w of the sensitivity matrix J = d(data) / d(conductivity) of ONE (source, frequency) pair,
composed from the reference's own functions on the grid, source, receivers and frequency of gradient.npz, with
LINEAR receivers (trilinear interpolation P on the trimmed staggered grids, times the rotation factors), for an
isotropic (`iso_*`) and a tri-axial (`tri_*`) conductivity model:

  sig_x/y/z       the conductivities; v a perturbation, w a data-space vector
  efield, d_lin   forward field (solver.solve, tol 1e-8, F-cycle, sc + lr) and its linear data P e
  {full,vz}_src   s mu_0 C(v) E: C = 1/4 sum of V_c v_c over the four cells of an edge, 0 on boundary edges;
                  `full` perturbs sigma_x = sigma_y = sigma_z by v, `vz` sigma_z alone
  {full,vz}_jv    P solve(src);   {full,vz}_jv_fd: central difference of the reference's forward data at step 1e-3
  jt_src, lam     P^T conj(w) and the solution of A lam = P^T conj(w)
  jt_gx/gy/gz     maps.edges2cellaverages of -Re(lam E s mu_0) per component (the reference's gradient arithmetic,
                  optimize.py:181-199); J^T w = -(jt_gx + jt_gy + jt_gz), for `vz`: -jt_gz
  fd_gap_ref      ||jv_fd - jv|| / ||jv||   (full);  adjoint_gap_ref  |Re sum conj(w) (J v) - v . J^T w| / |Re sum ...|

Run:  python tests/golden/make_jacobian_golden.py     (about two minutes per model without numba)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402


def edge_shapes(vnC):
    nx, ny, nz = (int(n) for n in vnC)
    return ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))


def cells2edges_pec(vnC, vol, v3):
    """C(v): per component 1/4 sum of V_c v_c over the four cells around an edge, boundary (PEC) edges 0."""
    nx, ny, nz = (int(n) for n in vnC)
    out = [np.zeros(s) for s in edge_shapes(vnC)]
    for c, v in enumerate(v3):
        if v is None:
            continue
        w = vol * np.asarray(v).reshape(vnC, order='F') / 4
        for a in (0, 1):
            for b in (0, 1):
                if c == 0:
                    out[0][:, a:ny + a, b:nz + b] += w
                elif c == 1:
                    out[1][a:nx + a, :, b:nz + b] += w
                else:
                    out[2][a:nx + a, b:ny + b, :] += w
    out[0][:, [0, -1], :] = 0; out[0][:, :, [0, -1]] = 0
    out[1][[0, -1], :, :] = 0; out[1][:, :, [0, -1]] = 0
    out[2][[0, -1], :, :] = 0; out[2][:, [0, -1], :] = 0
    return np.r_[out[0].ravel('F'), out[1].ravel('F'), out[2].ravel('F')]


def linear_receiver_matrix(grid, rec, fac):
    """Dense P (n_rec x nE): trilinear weights on the trimmed points of every component (first and last point per axis
    dropped, as fields.get_receiver_response), times the rotation factors; a component whose factors are all <= 1e-10
    is skipped (fields.py:812); a receiver outside the trimmed points of an active component gets a NaN row."""
    shp = edge_shapes(grid.vnC)
    off = np.cumsum([0] + [int(np.prod(s)) for s in shp])
    points = ((grid.cell_centers_x, grid.nodes_y, grid.nodes_z), (grid.nodes_x, grid.cell_centers_y, grid.nodes_z),
              (grid.nodes_x, grid.nodes_y, grid.cell_centers_z))
    nrec = fac.shape[1]
    P = np.zeros((nrec, grid.nE))
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
    return P


def main():
    _import_reference()
    from emg3d import fields, meshes, models, maps, solver
    g = np.load(os.path.join(HERE, 'gradient.npz'))
    grid = meshes.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    freq = float(g['freq'])
    src = g['src']
    rec = tuple(np.array(r, dtype=float) for r in g['rec'])
    nrec = rec[0].size
    fac = np.array(fields._rotation(*rec[3:]))
    P = linear_receiver_matrix(grid, rec, fac)
    assert np.isfinite(P).all()
    opts = dict(cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-8, verb=1, maxit=100)
    sfield = fields.get_source_field(grid, src, freq)
    points = ((grid.cell_centers_x, grid.nodes_y, grid.nodes_z), (grid.nodes_x, grid.cell_centers_y, grid.nodes_z),
              (grid.nodes_x, grid.nodes_y, grid.cell_centers_z))
    out = {}
    rng = np.random.default_rng(77)
    sig = 1.0 / g['res']
    cases = (('iso', (sig, sig, sig)),
             ('tri', (sig, sig * 10 ** rng.uniform(-0.3, 0.3, grid.nC), sig * 10 ** rng.uniform(-0.5, 0.2, grid.nC))))
    h = 1e-3
    for tag, s3 in cases:

        def forward(d3):
            m = models.Model(grid, s3[0] + d3[0], s3[1] + d3[1], s3[2] + d3[2], mapping='Conductivity')
            e = solver.solve(grid, m, sfield, **opts)
            return e, P @ np.array(e)

        model = models.Model(grid, *s3, mapping='Conductivity')
        e0, d_lin = forward((0., 0., 0.))
        # P against the reference's own linear interpolation on the trimmed grids
        chk = sum(fac[c] * maps.interp3d(tuple(p[1:-1] for p in points[c]), f[1:-1, 1:-1, 1:-1], rec[:3], method='linear',
                                         fill_value=0.0, mode='constant', cval=np.nan)
                  for c, f in enumerate((e0.fx, e0.fy, e0.fz)))
        assert np.abs(chk - d_lin).max() < 1e-13 * np.abs(d_lin).max()
        v = rng.standard_normal(grid.nC) * sig * 0.3
        w = (rng.standard_normal(nrec) + 1j * rng.standard_normal(nrec)) / np.abs(d_lin)
        out.update({f'{tag}_sig_x': s3[0], f'{tag}_sig_y': s3[1], f'{tag}_sig_z': s3[2], f'{tag}_v': v, f'{tag}_w': w,
                    f'{tag}_efield': np.array(e0), f'{tag}_d_lin': d_lin})
        jvs = {}
        for case, v3 in (('full', (v, v, v)), ('vz', (None, None, v))):
            vec = e0.smu0 * cells2edges_pec(grid.vnC, vol, v3) * np.array(e0)
            de = solver.solve(grid, model, fields.SourceField(grid, vec, freq=freq), **opts)
            jv = P @ np.array(de)
            d3 = tuple(0. if q is None else h * q for q in v3)
            _, dp = forward(d3)
            _, dm = forward(tuple(-q for q in d3))
            fd = (dp - dm) / (2 * h)
            gap = np.linalg.norm(fd - jv) / np.linalg.norm(jv)
            print(f'{tag} {case}: FD gap at step {h:g}: {gap:.3e}')
            assert gap < 1e-6
            jvs[case] = jv
            out.update({f'{tag}_{case}_src': vec, f'{tag}_{case}_jv': jv, f'{tag}_{case}_jv_fd': fd,
                        f'{tag}_{case}_fd_gap_ref': gap})
        # J^T w: exact transpose of the receiver operator as the source, the reference's gradient arithmetic
        jt_src = (P.T @ np.conj(w)).astype(complex)
        lam = solver.solve(grid, model, fields.SourceField(grid, jt_src, freq=freq), **opts)
        prod = fields.Field(grid, (-np.real(lam * e0 * e0.smu0)).astype(np.float64), freq=-1.)
        gx = np.zeros(grid.vnC, order='F'); gy = gx.copy(); gz = gx.copy()
        maps.edges2cellaverages(ex=prod.fx, ey=prod.fy, ez=prod.fz, vol=vol, out_x=gx, out_y=gy, out_z=gz)
        out.update({f'{tag}_jt_src': jt_src, f'{tag}_lam': np.array(lam), f'{tag}_jt_gx': gx, f'{tag}_jt_gy': gy,
                    f'{tag}_jt_gz': gz, f'{tag}_smu0': np.array(e0.smu0)})
        for case, jt in (('full', -(gx + gy + gz)), ('vz', -gz)):
            lhs = np.real(np.sum(np.conj(w) * jvs[case]))
            rhs = np.sum(jt.ravel('F') * v)
            gap = abs(lhs - rhs) / abs(lhs)
            print(f'{tag} {case}: Re sum conj(w) (J v) = {lhs:.10f}, v . J^T w = {rhs:.10f}, adjoint gap {gap:.3e}')
            assert gap < 1e-6
            out[f'{tag}_{case}_adjoint_gap_ref'] = gap
    out.update(fd_gap_ref=out['iso_full_fd_gap_ref'], adjoint_gap_ref=out['iso_full_adjoint_gap_ref'], fd_step=h)
    np.savez_compressed(os.path.join(HERE, 'jacobian.npz'), **out)
    print('wrote jacobian.npz', os.path.getsize(os.path.join(HERE, 'jacobian.npz')), 'bytes')


if __name__ == '__main__':
    main()
