"""
Generate tests/golden/survey_jacobian.npz by IMPORTING the reference (emg3d v0.17.0) at run time, exactly as make_golden.py does
(`_import_reference`: no-op numba stub; nothing of the reference is written into this repository: the fixture holds inputs
and expected outputs only).

The products J v and J^T w of the sensitivity matrix of a SURVEY, pair by pair, composed from the reference's own functions as
make_jacobian_golden.py composes them for one pair (its `linear_receiver_matrix` and `cells2edges_pec` are imported), on the
survey of survey_gradient.npz: the 12 x 10 x 8 grid of gradient.npz, 2 sources, the frequencies 1.5 and 0.7 Hz, 5 receivers,
solves at tol 1e-8 (F-cycle, sc + lr), for an isotropic (`iso_*`) and a tri-axial (`tri_*`) conductivity model, LINEAR receivers:

  hx, hy, hz, origin, sources (2, 5), freqs (2,), rec (5, 5)      the survey
  sig_x/y/z, v (nC), w [i_src, i_freq, i_rec]                    conductivities, ONE perturbation, a data-space vector per pair
  synthetic, jv  [i_src, i_freq, i_rec]                          P e of the forward field; P solve(s mu_0 C(v) E), v on all directions
  jt_pair [c, i_src, i_freq, nx, ny, nz]                         J^T w of the pair per component c = x, y, z:
                                                                 -edges2cellaverages_c(-Re(lam E s mu_0)), A lam = P^T conj(w)
  jt [c, nx, ny, nz]                                             the survey's J^T w per component in the defined order: per
                                                                 frequency the sequential sum over the sources from zeros, then
                                                                 the sequential sum of those over `freqs` from zeros
  adj_gap [i_src, i_freq]                                        |Re sum conj(w) (J v) - v . J^T w| / |Re sum ...| of those solves
  cubic_adj_gap [i_src, i_freq]                                  the same with the reference's cubic-spline receivers (dense P filled
                                                                 column by column by fields.get_receiver_response) in both products
  adj_gap_linear, adj_gap_cubic                                  the largest of the per-pair gaps over both models, per receiver kind

Run:  python tests/golden/make_survey_jacobian_golden.py     (about ten minutes without numba)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402
from make_jacobian_golden import cells2edges_pec, linear_receiver_matrix  # noqa: E402


def cubic_receiver_matrix(fields, grid, rec, freq):
    """Dense P (n_rec x nE) of the reference's cubic-spline receivers: fields.get_receiver_response of unit fields."""
    nrec = rec[0].size
    P = np.zeros((nrec, grid.nE))
    unit = np.zeros(grid.nE, dtype=complex)
    for k in range(grid.nE):
        unit[k] = 1.0
        P[:, k] = np.real(fields.get_receiver_response(grid, fields.Field(grid, unit, freq=freq), rec))
        unit[k] = 0.0
    assert np.isfinite(P).all()
    return P


def main():
    _import_reference()
    from emg3d import fields, meshes, models, maps, solver
    s = np.load(os.path.join(HERE, 'survey_gradient.npz'))
    grid = meshes.TensorMesh([s['hx'], s['hy'], s['hz']], origin=s['origin'])
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    vnC = tuple(int(n) for n in grid.vnC)
    sources, freqs = s['sources'], s['freqs']
    rec = tuple(np.array(r, dtype=float) for r in s['rec'])
    ns, nf, nrec = len(sources), len(freqs), rec[0].size
    fac = np.array(fields._rotation(*rec[3:]))
    P = linear_receiver_matrix(grid, rec, fac)
    assert np.isfinite(P).all()
    Pc = cubic_receiver_matrix(fields, grid, rec, float(freqs[0]))
    opts = dict(cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-8, verb=1, maxit=100)
    rng = np.random.default_rng(85)
    sig = 1.0 / s['res']
    cases = (('iso', (sig, sig, sig)),
             ('tri', (sig, sig * 10 ** rng.uniform(-0.3, 0.3, grid.nC), sig * 10 ** rng.uniform(-0.5, 0.2, grid.nC))))
    out = dict(hx=s['hx'], hy=s['hy'], hz=s['hz'], origin=s['origin'], sources=sources, freqs=freqs, rec=np.stack(rec))

    def jt_components(lam, e0):
        prod = fields.Field(grid, (-np.real(lam * e0 * e0.smu0)).astype(np.float64), freq=-1.)
        gx = np.zeros(grid.vnC, order='F'); gy = gx.copy(); gz = gx.copy()
        maps.edges2cellaverages(ex=prod.fx, ey=prod.fy, ez=prod.fz, vol=vol, out_x=gx, out_y=gy, out_z=gz)
        return -gx, -gy, -gz

    for tag, s3 in cases:
        model = models.Model(grid, *s3, mapping='Conductivity')
        v = rng.standard_normal(grid.nC) * sig * 0.3
        cv = cells2edges_pec(grid.vnC, vol, (v, v, v))
        w = np.zeros((ns, nf, nrec), dtype=complex)
        synthetic, jv = w.copy(), w.copy()
        jt_pair = np.zeros((3, ns, nf) + vnC)
        gap, gap_c = np.zeros((ns, nf)), np.zeros((ns, nf))
        for i, src in enumerate(sources):
            for j, freq in enumerate(freqs):
                freq = float(freq)
                e0 = solver.solve(grid, model, fields.get_source_field(grid, src, freq), **opts)
                synthetic[i, j] = P @ np.array(e0)
                w[i, j] = (rng.standard_normal(nrec) + 1j * rng.standard_normal(nrec)) / np.abs(synthetic[i, j])
                de = solver.solve(grid, model, fields.SourceField(grid, e0.smu0 * cv * np.array(e0), freq=freq), **opts)
                jv[i, j] = P @ np.array(de)
                for kind, Q in (('linear', P), ('cubic', Pc)):
                    lam = solver.solve(grid, model, fields.SourceField(grid, (Q.T @ np.conj(w[i, j])).astype(complex), freq=freq),
                                       **opts)
                    g3 = jt_components(lam, e0)
                    lhs = np.real(np.sum(np.conj(w[i, j]) * (Q @ np.array(de))))
                    rhs = np.sum(((g3[0] + g3[1]) + g3[2]).ravel('F') * v)
                    val = abs(lhs - rhs) / abs(lhs)
                    print(f'{tag} pair ({i}, {j}) {kind}: Re sum conj(w) (J v) = {lhs:.10e}, v . J^T w = {rhs:.10e}, gap {val:.3e}')
                    assert val < 1e-5
                    if kind == 'linear':
                        gap[i, j] = val
                        for c in range(3):
                            jt_pair[c, i, j] = g3[c]
                    else:
                        gap_c[i, j] = val
        jt = np.zeros((3,) + vnC)
        for c in range(3):
            for j in range(nf):
                gf = np.zeros(vnC)
                for i in range(ns):
                    gf = gf + jt_pair[c, i, j]
                jt[c] = jt[c] + gf
        out.update({f'{tag}_sig_x': s3[0], f'{tag}_sig_y': s3[1], f'{tag}_sig_z': s3[2], f'{tag}_v': v, f'{tag}_w': w,
                    f'{tag}_synthetic': synthetic, f'{tag}_jv': jv, f'{tag}_jt_pair': jt_pair, f'{tag}_jt': jt,
                    f'{tag}_adj_gap': gap, f'{tag}_cubic_adj_gap': gap_c})
    out['adj_gap_linear'] = np.array(max(out['iso_adj_gap'].max(), out['tri_adj_gap'].max()))
    out['adj_gap_cubic'] = np.array(max(out['iso_cubic_adj_gap'].max(), out['tri_cubic_adj_gap'].max()))
    path = os.path.join(HERE, 'survey_jacobian.npz')
    np.savez_compressed(path, **out)
    print('wrote survey_jacobian.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
