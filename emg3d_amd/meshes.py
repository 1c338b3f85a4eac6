"""Tensor mesh container (the attributes of ``emg3d.meshes._TensorMesh`` that
the multigrid path reads; reference emg3d/meshes.py:66-147).  Gridding helpers
of the reference (construct_mesh, skin depth, ...) are out of scope."""
import numpy as np


class TensorMesh:
    """Rectilinear mesh defined by cell widths ``h = [hx, hy, hz]`` and origin."""

    def __init__(self, h, origin=(0., 0., 0.)):
        self.h = [np.array(w, dtype=np.float64) for w in h]
        if len(self.h) != 3:
            raise ValueError("Provided grid must be a 3D grid.")
        self.origin = np.array(origin, dtype=np.float64)
        nodes = [np.r_[0., w.cumsum()] + o for w, o in zip(self.h, self.origin)]
        self.nodes_x, self.nodes_y, self.nodes_z = nodes
        cc = [(n[1:] + n[:-1]) / 2 for n in nodes]
        self.cell_centers_x, self.cell_centers_y, self.cell_centers_z = cc

        self.shape_cells = tuple(int(w.size) for w in self.h)
        self.shape_nodes = tuple(n + 1 for n in self.shape_cells)
        nx, ny, nz = self.shape_cells
        self.shape_edges_x = (nx, ny + 1, nz + 1)
        self.shape_edges_y = (nx + 1, ny, nz + 1)
        self.shape_edges_z = (nx + 1, ny + 1, nz)
        self.n_cells = nx * ny * nz
        self.n_nodes = int(np.prod(self.shape_nodes))
        self.n_edges_x = int(np.prod(self.shape_edges_x))
        self.n_edges_y = int(np.prod(self.shape_edges_y))
        self.n_edges_z = int(np.prod(self.shape_edges_z))
        self.n_edges_per_direction = (self.n_edges_x, self.n_edges_y, self.n_edges_z)
        self.n_edges = sum(self.n_edges_per_direction)

        # short aliases used throughout the reference
        self.x0 = self.origin
        self.vnC, self.nC = self.shape_cells, self.n_cells
        self.vnN, self.nN = self.shape_nodes, self.n_nodes
        self.vnEx, self.vnEy, self.vnEz = self.shape_edges_x, self.shape_edges_y, self.shape_edges_z
        self.nEx, self.nEy, self.nEz = self.n_edges_per_direction
        self.vnE, self.nE = self.n_edges_per_direction, self.n_edges
        self._vol = None

    def __repr__(self):
        nx, ny, nz = self.shape_cells
        return f"TensorMesh: {nx} x {ny} x {nz} ({self.n_cells:,})"

    @property
    def cell_volumes(self):
        """Cell volumes as 1-D array, x fastest (reference meshes.py:140-147)."""
        if self._vol is None:
            self._vol = (self.h[0][None, None, :] * self.h[1][None, :, None] *
                         self.h[2][:, None, None]).ravel()
        return self._vol


_TensorMesh = TensorMesh


def same_grid(a, b):
    """Whether two meshes are the same grid: the same object, or three width arrays and an origin that are equal element for
    element (a width that differs in its last bit makes another grid: results are compared bit for bit)."""
    if a is b:
        return True
    return all(np.array_equal(ha, hb) for ha, hb in zip(a.h, b.h)) and np.array_equal(a.origin, b.origin)


def distinct_grids(grids):
    """``(distinct, index)`` of a sequence of meshes: the distinct grids (``same_grid``) in order of first appearance -- the
    first object that stands for each --, and per entry the position of its grid among them."""
    distinct, index = [], []
    for g in grids:
        hit = [k for k, d in enumerate(distinct) if same_grid(d, g)]
        if not hit:
            distinct.append(g)
        index.append(hit[0] if hit else len(distinct) - 1)
    return distinct, index


def frequency_grids(grid, n_freq, model_grid, who):
    """The computational grid of every entry of a survey's ``freqs`` from the ``grid`` argument of ``who``: a mesh stands for all
    of them; a list or tuple holds one mesh per entry (repeats allowed) and needs ``model_grid``, the grid the model lives on --
    the cells of different computational grids have nothing else in common.  ``ValueError`` otherwise; no device call."""
    if not isinstance(grid, (list, tuple)):
        return [grid] * int(n_freq)
    bad = [type(g).__name__ for g in grid if not all(hasattr(g, a) for a in ('h', 'origin', 'vnC'))]
    if bad:
        raise ValueError(f"{who}: a sequence for `grid` must hold one TensorMesh per entry of `freqs`; it holds a {bad[0]}.")
    if len(grid) != int(n_freq):
        raise ValueError(f"{who}: a sequence for `grid` must hold one TensorMesh per entry of `freqs` ({int(n_freq)}); it holds "
                         f"{len(grid)}.")
    if model_grid is None:
        raise ValueError(f"{who}: a computational grid per frequency needs `model_grid`, the grid `model` lives on (the products of "
                         "different frequencies have no cells in common otherwise).")
    return list(grid)


def stretched_widths(ncore, npad, width, factor):
    """Widths [w f^npad .. w f, w x ncore, w f .. w f^npad] used by the synthetic
    benchmark grids."""
    pad = width * float(factor) ** np.arange(1, npad + 1)
    return np.r_[pad[::-1], np.full(ncore, float(width)), pad]
