"""Host side of the survey gradient: argument checks that need no library, the fixture tests/golden/survey_gradient.npz
against the invariants of its generator, and the frequency-shard combination -- in process and over two gloo ranks."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT, load_golden


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup():
    import emg3d_amd as em
    g = load_golden("survey_gradient.npz")
    grid = em.TensorMesh([g['hx'], g['hy'], g['hz']], origin=g['origin'])
    return em, g, grid


def test_argument_checks_need_no_device():
    em, g, grid = _setup()
    rec = tuple(g['rec'])
    model = em.Model(grid, g['res'])
    args = (g['sources'], g['freqs'], rec, g['observed'])
    with pytest.raises(NotImplementedError):
        em.optimize.survey_gradient(grid, model, *args, sslsolver='bicgstab')
    with pytest.raises(NotImplementedError, match="isotropic"):
        em.optimize.survey_gradient(grid, em.Model(grid, g['res'], 2 * g['res']), *args)
    with pytest.raises(NotImplementedError, match="permeability"):
        em.optimize.survey_gradient(grid, em.Model(grid, g['res'], mu_r=np.full(grid.nC, 1.5)), *args)
    with pytest.raises(NotImplementedError, match="permittivity"):
        em.optimize.survey_gradient(grid, em.Model(grid, g['res'], epsilon_r=np.full(grid.nC, 5.)), *args)
    with pytest.raises(ValueError, match="adjoint"):
        em.optimize.survey_gradient(grid, model, *args, adjoint='nearly')
    for bad in (g['observed'][0], g['observed'][:, :1], g['observed'][:, :, :4], g['observed'].transpose(1, 0, 2)[:, :1]):
        with pytest.raises(ValueError, match="observed"):
            em.optimize.survey_gradient(grid, model, g['sources'], g['freqs'], rec, bad)
    with pytest.raises(ValueError, match="weights"):
        em.optimize.survey_gradient(grid, model, *args, weights=np.ones(4))
    with pytest.raises(ValueError, match="rec"):
        em.optimize.survey_gradient(grid, model, g['sources'], g['freqs'], rec[:4], g['observed'])
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="batch"):
            em.optimize.survey_gradient(grid, model, *args, batch=bad)
    with pytest.raises(ValueError, match="sources"):
        em.optimize.survey_gradient(grid, model, [], g['freqs'], rec, g['observed'][:0])


def test_fixture_invariants():
    """Shapes, the one NaN datum, and G_f / the total re-summed from the stored per-pair arrays in the defined order."""
    em, g, grid = _setup()
    ns, nf, nrec = 2, 2, 5
    vnC = tuple(grid.vnC)
    assert vnC == (12, 10, 8)
    assert g['sources'].shape == (ns, 5) and g['freqs'].tolist() == [1.5, 0.7] and g['rec'].shape == (5, nrec)
    for key in ('observed', 'weights', 'synthetic'):
        assert g[key].shape == (ns, nf, nrec), key
    assert g['misfit'].shape == (ns, nf) and g['grad_pair'].shape == (ns, nf) + vnC
    assert g['partial'].shape == (nf,) + vnC and g['grad'].shape == vnC
    assert np.isnan(g['observed']).sum() == 1 and np.isfinite(g['weights']).all() and np.isfinite(g['synthetic']).all()
    assert np.array_equal(g['weights'][np.isfinite(g['observed'])],
                          1.0 / (0.05 * np.abs(g['observed'][np.isfinite(g['observed'])])) ** 2)
    # the first pair is the pair of gradient.npz
    g0 = load_golden("gradient.npz")
    assert np.array_equal(g['sources'][0], g0['src']) and np.array_equal(g['grad_pair'][0, 0], g0['grad'])
    # misfit over the finite data
    for i in range(ns):
        for j in range(nf):
            r = g['synthetic'][i, j] - g['observed'][i, j]
            ok = np.isfinite(r)
            assert g['misfit'][i, j] == np.sum(g['weights'][i, j][ok] * (r[ok].conj() * r[ok])).real / 2
    grad, phi = np.zeros(vnC), 0.0
    for j in range(nf):
        gf = np.zeros(vnC)
        terms = 0.0
        for i in range(ns):
            gf = gf + g['grad_pair'][i, j]
            phi = phi + g['misfit'][i, j]
            terms += np.linalg.norm(g['grad_pair'][i, j])
        assert np.array_equal(gf, g['partial'][j])
        assert np.linalg.norm(gf) >= 0.1 * terms
        grad = grad + gf
    assert np.array_equal(grad, g['grad']) and phi == float(g['phi'])
    assert np.linalg.norm(grad) >= 0.1 * sum(np.linalg.norm(g['partial'][j]) for j in range(nf))
    # the package's own summation routine and the shard combination give the same, for one and for two ranks
    from emg3d_amd import optimize, shard
    p1, g1 = optimize._sum_survey(g['partial'], g['misfit'], vnC)
    assert p1 == phi and np.array_equal(g1, grad)
    p2, g2 = shard.combine_survey_gradient([(g['partial'][r::2], g['misfit'][:, r::2]) for r in range(2)], nf)
    assert p2 == phi and np.array_equal(g2, grad)
    p3, g3 = shard.gather_survey_gradient(g['partial'], g['misfit'], g['freqs'])
    assert p3 == phi and np.array_equal(g3, grad)
    with pytest.raises(ValueError):
        shard.combine_survey_gradient([(g['partial'][:1], g['misfit'][:, :1])], nf)


WORKER = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, {root!r})
    import torch.distributed as dist
    from emg3d_amd import shard
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    rank, world = dist.get_rank(), dist.get_world_size()
    freqs = {freqs!r}
    nf, ns, vnC = len(freqs), 3, (5, 4, 3)
    # synthetic per-frequency partials and per-pair misfits of widely different sizes, so that the order of a sum shows
    rng = np.random.default_rng(17)
    partial = rng.standard_normal((nf,) + vnC) * 10.0 ** rng.integers(-8, 8, (nf,) + vnC)
    misfit = rng.uniform(0, 1, (ns, nf)) * 10.0 ** rng.integers(-8, 8, (ns, nf))
    grad, phi = np.zeros(vnC), 0.0
    for j in range(nf):
        grad = grad + partial[j]
        for i in range(ns):
            phi = phi + misfit[i, j]
    got_phi, got_grad = shard.gather_survey_gradient(partial[rank::world], misfit[:, rank::world], freqs)
    assert got_grad.shape == vnC and isinstance(got_phi, float)
    assert got_phi == phi and np.array_equal(got_grad, grad)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok")
""")


@pytest.mark.parametrize("freqs", [[0.25, -0.5, 1.0], [1.0]])
def test_two_rank_gloo_survey_gradient(tmp_path, freqs):
    """3 frequencies on 2 ranks (counts 2 / 1) and ONE frequency on 2 ranks (rank 1 owns nothing): both ranks get exactly the
    single-process sums."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, freqs=freqs))
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o
