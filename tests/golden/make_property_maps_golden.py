"""
Generate tests/golden/property_maps.npz by IMPORTING the reference (emg3d v0.17.0) at run time, exactly as make_golden.py does
(`_import_reference`; nothing of the reference is written into this repository: the fixture holds inputs and expected outputs
only).

The six property maps of the reference (emg3d/maps.py:284-448) and the places that apply them (models.py:390, 640-644), on the
12 x 10 x 8 grid of survey_jacobian.npz.  One tri-axial conductivity model, log10(sigma_c) uniform in [-3, 1], is stated in
each map M in ('Conductivity', 'Resistivity', 'LgConductivity', 'LnConductivity', 'LgResistivity', 'LnResistivity'):

  hx, hy, hz, origin                           the grid
  g2_hx, g2_hy, g2_hz, g2_origin               a second grid (other cell sizes, partly outside the first)
  grad (nx, ny, nz)                            a random gradient with respect to conductivity
  names                                        the six map names, in the order of their device codes 0..5 (see below)
  codes                                        the device code of each name
  M_p (3, nx, ny, nz)                          the mapped arrays p_c = forward(sigma_c) (LgConductivity: the drawn numbers)
  M_back (3, nx, ny, nz)                       backward(p_c): the conductivities every computation uses
  M_fwdback (nx, ny, nz)                       forward(backward(p_x))
  M_chain (nx, ny, nz)                         grad after derivative_chain(grad, p_x)
  M_eta_f (nx, ny, nz) complex                 VolumeModel(grid, Model(p_x, p_y, p_z, mapping=M), 1.5 Hz).eta_x
  M_eta_s (nx, ny, nz)                         the same at the Laplace value -1.5
  M_interp (3, ...)                            Model.interpolate2grid(grid, g2) of that model: property_x, _y, _z (defaults: volume
                                               averaging, of log10 of the values unless M is a logarithm already)

Run:  python tests/golden/make_property_maps_golden.py     (seconds)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

NAMES = ('Conductivity', 'Resistivity', 'LgConductivity', 'LnConductivity', 'LgResistivity', 'LnResistivity')


def main():
    _import_reference()
    from emg3d import fields, maps, meshes, models
    s = np.load(os.path.join(HERE, 'survey_jacobian.npz'))
    grid = meshes.TensorMesh([s['hx'], s['hy'], s['hz']], origin=s['origin'])
    vnC = tuple(int(n) for n in grid.vnC)
    rng = np.random.default_rng(20261018)
    lg = rng.uniform(-3, 1, (3,) + vnC)
    out = {k: s[k] for k in ('hx', 'hy', 'hz', 'origin')}
    # second grid: 9 x 7 x 5 cells of other sizes over the same region, pushed half a cell outside on the low side
    ext = [float(h.sum()) for h in grid.h]
    h2 = [np.full(n, e / (n - 0.5)) for n, e in zip((9, 7, 5), ext)]
    o2 = np.array([o - h[0] / 2 for o, h in zip(grid.origin, h2)])
    grid2 = meshes.TensorMesh(h2, origin=o2)
    out.update(g2_hx=h2[0], g2_hy=h2[1], g2_hz=h2[2], g2_origin=o2)
    grad = rng.standard_normal(vnC)
    out['grad'] = grad
    out['names'] = np.array(NAMES)
    out['codes'] = np.arange(6)
    sfield = fields.SourceField(grid, freq=1.5)
    lfield = fields.SourceField(grid, freq=-1.5)
    for name in NAMES:
        m = getattr(maps, 'Map' + name)()
        p = lg.copy() if name == 'LgConductivity' else np.array(m.forward(10 ** lg))
        back = np.array(m.backward(p))
        g = grad.copy()
        m.derivative_chain(g, p[0])
        model = models.Model(grid, p[0], p[1], p[2], mapping=name)
        new = model.interpolate2grid(grid, grid2)
        out.update({f'{name}_p': p, f'{name}_back': back, f'{name}_fwdback': np.array(m.forward(back[0])), f'{name}_chain': g,
                    f'{name}_eta_f': np.array(models.VolumeModel(grid, model, sfield).eta_x),
                    f'{name}_eta_s': np.array(models.VolumeModel(grid, model, lfield).eta_x),
                    f'{name}_interp': np.stack([new.property_x, new.property_y, new.property_z])})
    path = os.path.join(HERE, 'property_maps.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
