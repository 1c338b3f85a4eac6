"""
Generate tests/golden/grid2grid.npz by IMPORTING the reference (emg3d v0.17.0, read-only at /root/reference)
in the build container, exactly as make_golden.py does (no-op numba stub: the reference's volume averaging
runs as plain Python; nothing of the reference is written into this repository: the fixture holds inputs
and expected outputs only).

  w_<case>_{x1,x2,hs,ix1,ix2}     maps._volume_average_weights on one axis: identical edges, coarsening,
                                  refinement, shifted origins, a new grid sticking out on both sides, edges
                                  that coincide exactly or differ by ~1e-12, single-cell axes
  g1_*, g2_*, g3_*                three stretched grids (h and origin per axis)
  va_<dtype>_*                    maps.volume_average (g1 -> g2) onto a non-zero new_values, f64 and c128
  vol_<dtype>_log<0|1>            maps.grid2grid(g1, v, g2, 'volume', log=...), f64 and c128
  cc_<method>_ext<0|1>            maps.grid2grid of a cell array g1 -> g2, real (linear / cubic, extrapolate)
  fld_<method>_ext<0|1>_{x,y,z}   maps.grid2grid of a complex Field g1 -> g2, per component
  fb_<method>_ext<0|1>_{x,y,z}    the same g1 -> g3 (g3: two cells in z, i.e. fewer than four points: 'cubic' is 'linear')
  mdl_<case>_*                    Model.interpolate2grid g1 -> g2 (isotropic scalar, VTI, tri-axial with mu_r; one
                                  Conductivity model with non-default options)
  grad_*                          the gradient back-mapping of optimize.gradient (optimize.py:201-214): a stored `grad`
                                  on a computational grid, grid2grid(comp, -grad, model_grid, 'cubic') and
                                  MapResistivity.derivative_chain on the model grid

Run:  python tests/golden/make_grid2grid_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference, get_h  # noqa: E402


def weights_cases():
    """(name, x1, x2): old and new edges of one axis."""
    base = np.r_[0., np.cumsum(get_h(6, 3, 10., 1.3))]
    fine = np.linspace(-20., 80., 41)
    cases = [
        ('same', base, base.copy()),
        ('coarsen', fine, fine[::4].copy()),
        ('refine', fine[::5].copy(), np.linspace(-20., 80., 33)),
        ('shift', base, base[:-2] + 3.7),
        ('outside', np.linspace(0., 100., 11), np.r_[-30., -5., np.linspace(10., 90., 6), 125., 140.]),
        ('single_old', np.array([0., 10.]), np.array([-5., 3., 4.5, 12.])),
        ('single_new', base, np.array([2.5, 31.])),
        ('single_both', np.array([-1., 2.]), np.array([0.5, 7.])),
    ]
    x2 = base[::2].copy()
    x2[1] += 1e-12 * abs(x2[1])             # coinciding edges and edges about 1e-12 apart
    x2[3] -= 1e-12 * abs(x2[3])
    cases.append(('near', base, x2))
    return cases


def grids(meshes):
    g1 = dict(h=[get_h(6, 3, 20., 1.3), get_h(4, 3, 25., 1.2), get_h(4, 2, 30., 1.25)], origin=np.array([-150., -120., -110.]))
    g2 = dict(h=[get_h(5, 2, 31., 1.2), get_h(9, 1, 18., 1.5), get_h(3, 2, 40., 1.3)], origin=np.array([-140., -137., -96.]))
    g3 = dict(h=[get_h(4, 2, 33., 1.2), get_h(6, 1, 21., 1.3), np.array([70., 90.])], origin=np.array([-120., -95., -60.]))
    return [(g, meshes.TensorMesh(g['h'], origin=g['origin'])) for g in (g1, g2, g3)]


def main():
    _import_reference()
    from emg3d import fields, maps, meshes, models
    rng = np.random.default_rng(2024)
    out = {}
    for name, x1, x2 in weights_cases():
        hs, ix1, ix2 = maps._volume_average_weights(x1, x2)
        out.update({f'w_{name}_x1': x1, f'w_{name}_x2': x2, f'w_{name}_hs': hs, f'w_{name}_ix1': ix1, f'w_{name}_ix2': ix2})

    (d1, g1), (d2, g2), (d3, g3) = grids(meshes)
    for tag, d in (('g1', d1), ('g2', d2), ('g3', d3)):
        for i, c in enumerate('xyz'):
            out[f'{tag}_h{c}'] = d['h'][i]
        out[f'{tag}_origin'] = d['origin']

    # volume_average onto non-zero new values (the result is ADDED, then divided)
    vol2 = g2.cell_volumes.reshape(g2.vnC, order='F')
    for dt in ('f64', 'c128'):
        v = 10 ** rng.uniform(-1, 2, g1.vnC)
        nv = rng.uniform(-1, 1, g2.vnC)
        if dt == 'c128':
            v = v * np.exp(1j * rng.uniform(0, 2 * np.pi, g1.vnC))
            nv = nv + 1j * rng.uniform(-1, 1, g2.vnC)
        res = nv.copy()
        maps.volume_average(g1.nodes_x, g1.nodes_y, g1.nodes_z, v, g2.nodes_x, g2.nodes_y, g2.nodes_z, res, vol2)
        out.update({f'va_{dt}_in': v, f'va_{dt}_new_in': nv, f'va_{dt}_out': res})
        for log in (0, 1):
            out[f'vol_{dt}_log{log}'] = maps.grid2grid(g1, v, g2, 'volume', log=bool(log))

    # linear / cubic on a real cell array and on a complex Field (g2: regular, g3: two cells in z)
    cc = 10 ** rng.uniform(0, 2, g1.vnC)
    out['cc_in'] = cc
    fld = fields.Field(g1, rng.standard_normal(g1.nE) + 1j * rng.standard_normal(g1.nE))
    out['fld_in'] = np.array(fld)
    for method in ('linear', 'cubic'):
        for ext in (0, 1):
            out[f'cc_{method}_ext{ext}'] = maps.grid2grid(g1, cc, g2, method, extrapolate=bool(ext))
            out[f'cc_{method}_ext{ext}_log'] = maps.grid2grid(g1, cc, g2, method, extrapolate=bool(ext), log=True)
            for tag, g in (('fld', g2), ('fb', g3)):
                new = maps.grid2grid(g1, fld, g, method, extrapolate=bool(ext))
                for c in 'xyz':
                    out[f'{tag}_{method}_ext{ext}_{c}'] = np.asarray(getattr(new, 'f' + c))

    # Model.interpolate2grid
    n1 = g1.vnC

    def rand():
        return 10 ** rng.uniform(-1, 2, n1)
    cases = {
        'iso': dict(property_x=3.0),
        'vti': dict(property_x=rand(), property_z=rand()),
        'tri': dict(property_x=rand(), property_y=rand(), property_z=rand(), mu_r=1 + rng.uniform(0, 2, n1)),
        'cond': dict(property_x=rand(), property_y=rand(), epsilon_r=1 + rng.uniform(0, 5, n1), mapping='Conductivity'),
    }
    opts = {'cond': dict(method='cubic', extrapolate=False)}
    for case, kw in cases.items():
        m = models.Model(g1, **kw).interpolate2grid(g1, g2, **opts.get(case, {}))
        for name in ('property_x', 'property_y', 'property_z', 'mu_r', 'epsilon_r'):
            if name in kw:
                out[f'mdl_{case}_{name}_in'] = np.asarray(kw[name], dtype=np.float64)
                out[f'mdl_{case}_{name}'] = np.asarray(getattr(m, name))

    # gradient back-mapping (optimize.py:201-214) from a computational grid to a coarser model grid inside it
    comp = meshes.TensorMesh([get_h(8, 3, 50., 1.3), get_h(6, 3, 50., 1.3), get_h(6, 2, 50., 1.4)], origin=(-450., -400., -380.))
    mgrid = meshes.TensorMesh([np.full(6, 60.), np.full(5, 55.), np.full(4, 70.)], origin=(-180., -140., -150.))
    grad = rng.standard_normal(comp.vnC) * 1e-3
    res = 10 ** rng.uniform(-0.5, 1.5, mgrid.vnC)
    model = models.Model(mgrid, res.ravel('F'))
    grad_model = np.zeros(mgrid.vnC, order='F')
    grad_model += maps.grid2grid(comp, -grad, mgrid, method='cubic')
    mapped = grad_model.copy()
    model.map.derivative_chain(grad_model, model.property_x)
    for name, g in (('comp', comp), ('model', mgrid)):
        for i, c in enumerate('xyz'):
            out[f'grad_{name}_h{c}'] = g.h[i]
        out[f'grad_{name}_origin'] = np.asarray(g.origin, dtype=np.float64)
    out.update(grad_in=grad, grad_res=res, grad_mapped=mapped, grad_out=grad_model)

    np.savez_compressed(os.path.join(HERE, 'grid2grid.npz'), **out)
    print(f"wrote grid2grid.npz: {len(out)} arrays, {os.path.getsize(os.path.join(HERE, 'grid2grid.npz'))} bytes")


if __name__ == '__main__':
    main()
