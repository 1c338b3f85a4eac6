"""
Generate tests/golden/survey_gradient.npz by IMPORTING the reference (emg3d v0.17.0) at run time, exactly as make_golden.py does
(`_import_reference`: no-op numba stub; nothing of the reference is written into this repository: the fixture holds inputs
and expected outputs only).

The survey gradient -- what the reference's `simulation.gradient` (optimize.py:115-217) sums over the (source, frequency)
pairs of a survey -- on the grid and model of gradient.npz (12 x 10 x 8; `gradient_fixture` of make_golden.py), with 2
point-dipole sources, the frequencies 1.5 and 0.7 Hz and the five receivers of gradient.npz.  Observed data come from the
perturbed model, weights are 1 / (0.05 |obs|)^2, ONE observed datum is NaN.  Per pair the reference's own functions are
composed exactly as `gradient_fixture` composes them; a NaN receiver is skipped in the residual source as in
simulations.py:1181-1183 and the misfit is the sum over the finite data.

  sources (2, 5), freqs (2,), rec (5, 5), res           the survey and the model (grid: hx, hy, hz, origin)
  observed, weights, synthetic   [i_src, i_freq, i_rec]
  misfit, grad_pair              [i_src, i_freq], [i_src, i_freq, nx, ny, nz]
  partial                        G_f = (0 + grad_pair[0, f]) + grad_pair[1, f]: sequential over the sources, ascending
  grad, phi                      (0 + G_0) + G_1 over the frequencies in the order of `freqs`; phi in the same (frequency outer,
                                 source inner) order

The generator asserts that no sum cancels badly: the norm of every G_f, and of the total, is at least 0.1 of the sum of
the norms of its terms (otherwise the tolerances of tests/test_gpu_survey_gradient.py would not follow from those of the pairs).

Run:  python tests/golden/make_survey_gradient_golden.py     (a few minutes without numba)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402


def main():
    _import_reference()
    from emg3d import fields, meshes, models, maps, solver
    g = np.load(os.path.join(HERE, 'gradient.npz'))
    hx, hy, hz, origin = g['hx'], g['hy'], g['hz'], g['origin']
    grid = meshes.TensorMesh([hx, hy, hz], origin=origin)
    vol = grid.cell_volumes.reshape(grid.vnC, order='F')
    res = g['res']
    model = models.Model(grid, res)
    res_true = res.copy().reshape(grid.vnC, order='F')
    res_true[5:9, 3:7, 2:5] *= 4.0                       # the "observed" data come from a perturbed model (gradient_fixture)
    model_true = models.Model(grid, res_true.ravel('F'))
    rec = tuple(np.array(r, dtype=float) for r in g['rec'])
    nrec = rec[0].size
    sources = np.array([g['src'], [140., -60., -25., -50., 20.]])
    freqs = np.array([1.5, 0.7])
    ns, nf = len(sources), len(freqs)
    opts = dict(cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-8, verb=1)

    observed = np.zeros((ns, nf, nrec), dtype=complex)
    synthetic = np.zeros((ns, nf, nrec), dtype=complex)
    efields = {}
    for i, src in enumerate(sources):
        for j, freq in enumerate(freqs):
            sfield = fields.get_source_field(grid, src, freq)
            efields[i, j] = solver.solve(grid, model, sfield, **opts)
            e_obs = solver.solve(grid, model_true, sfield, **opts)
            synthetic[i, j] = np.array(fields.get_receiver_response(grid, efields[i, j], rec))
            observed[i, j] = np.array(fields.get_receiver_response(grid, e_obs, rec))
    weights = 1.0 / (0.05 * np.abs(observed)) ** 2       # relative error 5 % (data weights = 1 / std^2)
    observed[1, 0, 2] = np.nan                           # one missing datum

    misfit = np.zeros((ns, nf))
    grad_pair = np.zeros((ns, nf) + tuple(grid.vnC))
    for i in range(ns):
        for j, freq in enumerate(freqs):
            efield = efields[i, j]
            residual = synthetic[i, j] - observed[i, j]
            ok = np.isfinite(residual)
            misfit[i, j] = np.sum(weights[i, j][ok] * (residual[ok].conj() * residual[ok])).real / 2    # optimize.py:110
            rfield = fields.SourceField(grid, freq=freq)                                # simulations.py:1171-1213
            for k in range(nrec):
                if np.isnan(residual[k]):
                    continue
                strength = residual[k].conj() * np.conj(weights[i, j, k]) / rfield.smu0
                rfield += fields.get_source_field(grid=grid, src=[r[k] for r in rec], freq=freq, strength=strength)
            bfield = solver.solve(grid, model, rfield, **opts)                          # simulations.py:1131-1143
            prod = -np.real(bfield * efield * efield.smu0)                              # optimize.py:181-184
            prod = fields.Field(grid, prod.astype(np.float64), freq=-1.)
            gx = np.zeros(grid.vnC, order='F'); gy = gx.copy(); gz = gx.copy()
            maps.edges2cellaverages(ex=prod.fx, ey=prod.fy, ez=prod.fz, vol=vol, out_x=gx, out_y=gy, out_z=gz)
            grad_pair[i, j] = gx + gy + gz
            print(f'pair ({i}, {j}): misfit {misfit[i, j]:.6f}, |grad| {np.linalg.norm(grad_pair[i, j]):.6e}')

    def norm(a):
        return float(np.linalg.norm(a))

    partial = np.zeros((nf,) + tuple(grid.vnC))
    grad = np.zeros(tuple(grid.vnC))
    phi = 0.0
    for j in range(nf):
        for i in range(ns):
            partial[j] = partial[j] + grad_pair[i, j]
            phi = phi + misfit[i, j]
        terms = sum(norm(grad_pair[i, j]) for i in range(ns))
        print(f'G_{j}: |G| {norm(partial[j]):.6e}, sum of |terms| {terms:.6e}')
        assert norm(partial[j]) >= 0.1 * terms, "G_f cancels badly: move a source"
        grad = grad + partial[j]
    terms = sum(norm(partial[j]) for j in range(nf))
    print(f'total: |grad| {norm(grad):.6e}, sum of |G_f| {terms:.6e}')
    assert norm(grad) >= 0.1 * terms, "the total cancels badly: move a source"

    out = dict(hx=hx, hy=hy, hz=hz, origin=origin, res=res, sources=sources, freqs=freqs, rec=np.stack(rec), observed=observed,
               weights=weights, synthetic=synthetic, misfit=misfit, grad_pair=grad_pair, partial=partial, grad=grad,
               phi=np.array(phi))
    path = os.path.join(HERE, 'survey_gradient.npz')
    np.savez_compressed(path, **out)
    print('wrote survey_gradient.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
