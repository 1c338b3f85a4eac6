"""Frequency sharding across the GPUs of one node (reference counterpart:
``Simulation.compute`` fans (source, frequency) pairs out over a process pool,
emg3d/simulations.py:821-878).  Every (source, frequency) pair is an
independent linear system, so the path shards with NO data-path collective:
rank r solves the frequencies ``freqs[r::world]`` on GPU r; the only exchange
is ONE end-of-run gather of the fields (RCCL over xGMI when the backend is
"nccl"; gloo on CPU for the tests).
"""
import numpy as np


def my_frequencies(freqs, rank, world):
    """Round-robin assignment: rank r gets freqs[r], freqs[r+world], ..."""
    return [float(f) for f in list(freqs)[rank::world]]


def solve_frequencies(grid, model, src, freqs, device=0, strength=0, concurrent=1, rec=None, return_field=True,
                      **solver_opts):
    """Solve one source for several frequencies on ONE GPU from a shared, frequency-independent
    model: conductivities, cell volumes and ``zeta`` are computed and uploaded once (``models.model_parts``); per
    frequency only the scalar ``s*mu_0`` changes (``eta = (s mu_0 V) sigma`` -- VolumeModel's rounding, so every result is
    bit for bit that of ``solver.solve`` at this frequency -- and the source are formed on the device).  Reference counterpart: the per-frequency jobs of
    ``Simulation.compute`` (emg3d/simulations.py:840-867) with ``gridding='same'``.

    ``concurrent`` > 1 runs that many solves at the same time on the GPU (the ``max_workers`` of the
    reference's process pool, simulations.py:862-867, as host threads: every solve has its own handle
    and HIP stream, the library calls release the GIL).  The coarse levels of a cycle leave most
    SIMDs idle, so a second and third frequency fill them: measured 184 -> 233 -> 256 Mcells/s
    aggregate for 1 -> 2 -> 3 concurrent 128^3 F-cycles on one MI355X (``tools/multi_solve.py``).
    Results do not depend on ``concurrent`` (each solve is deterministic on its own stream).

    ``rec = (x, y, z, azimuth, dip)``: also extract the receiver responses of every solution
    (``fields.get_receiver_response``, reference fields.py:733-817) -- straight from the field in HBM
    (``DeviceMG.get_receiver_response``); with ``return_field=False`` the field itself is never downloaded,
    so a rank hands 16 bytes per receiver to the end-of-run gather instead of 102 MB per frequency (128^3).

    Returns ``[(efield, info), ...]`` in the order of ``freqs``; with ``rec``: ``[(efield | None, info,
    responses), ...]``."""
    from emg3d_amd import fields, models, solver
    freqs = [float(f) for f in freqs]
    if not freqs:
        return []
    parts = models.model_parts(grid, model, raw=True)        # (with or without epsilon_r)

    def one(f, handles=None):
        # the source is built in HBM per frequency (DeviceMG.set_source: the dipole's edge distribution runs on the
        # device, scaled by this frequency's s mu_0): no nE-sized array is formed or uploaded on the host
        # (with a Krylov solver the host object carries the right-hand side; otherwise only the frequency)
        sfield = fields.SourceField(grid, freq=f) if solver_opts.get('sslsolver') else fields.FrequencySpec(f)
        if handles is not None:
            dev = handles.target(sfield)
        else:
            dev = solver.DeviceMG.open(grid, model, sfield, device=device, parts=parts)
        try:
            # receivers only (multigrid path): the solution stays in HBM -- no nE-sized download that would be thrown away
            keep = not (rec is not None and not return_field and not solver_opts.get('sslsolver'))
            e, info = solver.solve(grid, None, sfield, handle=dev, return_info=True, source=(src, strength),
                                   download=keep, **solver_opts)
            if rec is None:
                return e, info
            if solver_opts.get('sslsolver'):       # the Krylov iterate lives in a workspace vector: use the host field
                resp = fields.get_receiver_response(grid, e, rec)
            else:
                resp = dev.get_receiver_response(rec)
            return (e if return_field else None), info, resp
        finally:
            if handles is None:
                dev.close()

    if int(concurrent) > 1 and len(freqs) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(int(concurrent), len(freqs))) as pool:
            return list(pool.map(one, freqs))
    # frequencies solved one after the other share ONE handle per dtype: only eta and what is derived from it
    # (coarse models, line factorisations) is recomputed (DeviceMG.retarget) -- the results are those of a fresh
    # handle bit for bit; hierarchy, buffers and launch graphs are not rebuilt (15-20 ms per frequency at 128^3)
    with solver.FrequencyHandles(grid, parts, device) as handles:
        return [one(f, handles) for f in freqs]


def solve_survey(grid, model, sources, freqs, rec, device=0, strength=0, batch=8, return_fields=False, model_grid=None,
                 **solver_opts):
    """A survey's forward modelling on ONE GPU: every source of ``sources`` at every frequency of ``freqs`` (the
    (source, frequency) loop of ``Simulation.compute``, emg3d/simulations.py:821-878, with ``gridding='same'``, or with
    ``model_grid`` its ``'single'`` and, for the caller's grids, ``'dict'``) and the responses at the receivers
    ``rec = (x, y, z, azimuth, dip)``.  Frequencies are independent handles
    (across GPUs: give every rank ``my_frequencies(freqs, rank, world)`` and gather the responses with
    ``gather_fields``); the sources of one frequency share its operator and go through the SAME launches, ``batch``
    at a time (``solver.solve_sources``: bit for bit the results of one solve per source).  Nothing nE-sized
    crosses PCIe unless ``return_fields``: sources are built and receivers evaluated in HBM.

    Returns ``(responses, infos)`` -- ``responses[i_src, i_freq, i_rec]`` complex (or float for Laplace-domain
    frequencies), ``infos[i_src][i_freq]`` the ``info_dict`` of that solve -- and the fields ``[i_src][i_freq]`` if
    ``return_fields``.

    ``model_grid`` (a ``TensorMesh``; default None: ``model`` lives on ``grid``): ``model`` lives on ``model_grid`` and reaches the
    computational grid through ``model.interpolate2grid(model_grid, grid)``.  ``grid`` may then be a list or tuple with one
    ``TensorMesh`` per entry of ``freqs``, repeats allowed (``ValueError`` without ``model_grid``, or for another length): the
    model is regridded once per distinct grid (``meshes.same_grid``), there is one handle per distinct (grid, dtype, systems per
    launch) (``solver.GridHandles``), and column ``j`` of every result is bit for bit that of ``solve_survey(grid[j],
    model.interpolate2grid(model_grid, grid[j]), sources, [freqs[j]], rec)``; ``return_fields`` gives every field on its own
    grid."""
    from emg3d_amd import fields, meshes, solver
    freqs = [float(f) for f in freqs]
    ns, nf = len(sources), len(freqs)
    grids = meshes.frequency_grids(grid, nf, model_grid, 'solve_survey')
    resp = None
    infos = [[None] * nf for _ in range(ns)]
    efs = [[None] * nf for _ in range(ns)] if return_fields else None
    # one handle per (dtype, systems per launch), re-targeted from frequency to frequency (DeviceMG.retarget: eta, coarse
    # models and line factorisations are recomputed in HBM, hierarchy / buffers / launch graphs stay); bit for bit the
    # results of solver.solve_sources with a handle of its own
    with solver.GridHandles(grids, model, device, model_grid=model_grid) as handles:
        for jf, f in enumerate(freqs):
            spec = fields.FrequencySpec(f)
            for i0 in range(0, ns, int(batch)):
                chunk = list(sources[i0:i0 + int(batch)])
                dev = handles.target(jf, spec, key=(len(chunk),))
                e, info, r = solver.solve_sources(grids[jf], None, chunk, f, strength=strength, rec=rec, device=device,
                                                  download=return_fields, handle=dev, **solver_opts)
                if resp is None:
                    resp = np.zeros((ns, nf, r.shape[1]), dtype=np.result_type(r.dtype, np.float64))
                if r.dtype.kind == 'c' and resp.dtype.kind != 'c':
                    resp = resp.astype(np.complex128)
                resp[i0:i0 + len(chunk), jf] = r
                for k in range(len(chunk)):
                    infos[i0 + k][jf] = info[k]
                    if return_fields:
                        efs[i0 + k][jf] = e[k]
    if resp is None:            # this rank owns no frequency
        resp = np.zeros((ns, 0, int(max(np.size(c) for c in rec[:3]))))
    return (resp, infos, efs) if return_fields else (resp, infos)


def gather_survey(resp_local, freqs, group=None):
    """End-of-run exchange of a sharded survey ("optionally only receiver responses"): every rank holds
    ``resp_local[i_src, j, i_rec]`` for ITS frequencies ``my_frequencies(freqs, rank, world)`` (the output of
    ``solve_survey``; a rank without frequencies passes shape ``(n_src, 0, n_rec)``) and gets back the full
    ``(n_src, len(freqs), n_rec)`` array in the order of ``freqs``.  One header and one payload collective
    (``gather_fields``): 16 bytes per source, frequency and receiver cross the links."""
    import torch.distributed as dist
    freqs = [float(f) for f in freqs]
    resp_local = np.asarray(resp_local)
    if not (dist.is_available() and dist.is_initialized()):
        return resp_local
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    n_mine = len(my_frequencies(freqs, rank, world))
    if resp_local.ndim != 3 or resp_local.shape[1] != n_mine:
        raise ValueError(f"gather_survey: rank {rank} owns {n_mine} frequencies, got an array of shape {resp_local.shape}.")
    ns, _, nr = resp_local.shape
    parts = gather_fields([np.ascontiguousarray(resp_local[:, j, :]).ravel() for j in range(n_mine)], group=group)
    cplx = any(np.iscomplexobj(a) for p in parts for a in p)
    out = np.zeros((ns, len(freqs), nr), dtype=np.complex128 if cplx else np.float64)
    for r in range(world):
        for j, a in enumerate(parts[r]):
            out[:, r + j * world, :] = a.reshape(ns, nr)          # my_frequencies(freqs, r, world) = freqs[r::world]
    return out


def combine_survey_gradient(per_rank, n_freq):
    """The sums of a frequency-sharded survey gradient: ``per_rank[r] = (partial_r, misfit_r)`` holds what
    ``optimize.survey_gradient`` returned on rank ``r`` for ``my_frequencies(freqs, r, world)`` -- ``info['partial']`` with shape
    ``(n_r,) + vnC`` and ``info['misfit']`` with shape ``(n_src, n_r)``.  The per-frequency partials ``G_f`` and the per-pair
    misfits are put back in the order of ``freqs`` (frequency ``r + j * world`` is rank ``r``'s ``j``-th) and summed in that
    order, exactly as ``survey_gradient`` sums them: ``(phi, grad)`` is bit for bit the single-process result for any world
    size."""
    from emg3d_amd import optimize
    world = len(per_rank)
    partials, misfits = [None] * int(n_freq), [None] * int(n_freq)
    vnC = None
    for r, (p, m) in enumerate(per_rank):
        p, m = np.asarray(p), np.asarray(m)
        if p.ndim != 4 or m.ndim != 2 or m.shape[1] != p.shape[0]:
            raise ValueError(f"combine_survey_gradient: rank {r}: partials of shape {p.shape}, misfits of shape {m.shape}.")
        vnC = tuple(p.shape[1:]) if vnC is None else vnC
        for j in range(p.shape[0]):
            if r + j * world >= n_freq:
                raise ValueError(f"combine_survey_gradient: rank {r} of {world} holds {p.shape[0]} of {n_freq} frequencies.")
            partials[r + j * world], misfits[r + j * world] = p[j], m[:, j]
    if any(p is None for p in partials):
        raise ValueError(f"combine_survey_gradient: the ranks hold {sum(p is not None for p in partials)} of {n_freq} frequencies.")
    if vnC is None:
        raise ValueError("combine_survey_gradient: no rank.")
    mis = np.stack(misfits, axis=1) if n_freq else np.zeros((np.asarray(per_rank[0][1]).shape[0], 0))
    return optimize._sum_survey(partials, mis, vnC)


def gather_survey_gradient(partial_local, misfit_local, freqs, group=None):
    """End-of-run exchange of a frequency-sharded survey gradient: every rank has run ``optimize.survey_gradient`` on ITS
    frequencies ``my_frequencies(freqs, rank, world)`` with its slice ``observed[:, rank::world, :]`` and passes
    ``info['partial']`` (``(n_mine,) + vnC``) and ``info['misfit']`` (``(n_src, n_mine)``; a rank without frequencies passes the
    empty arrays it got).  One header and one payload collective of host arrays (``gather_fields``): per frequency ``nC +
    n_src`` doubles.  Every rank then sums the partials and the misfits in the order of ``freqs``
    (``combine_survey_gradient``) and returns ``(phi, grad)`` -- identical on every rank and bit for bit the single-process
    result, whatever the world size: that is why the per-frequency partials, not per-rank sums, are exchanged.  Without an
    initialised process group the local arrays are summed.  No device collective."""
    import torch.distributed as dist
    freqs = [float(f) for f in freqs]
    partial_local, misfit_local = np.asarray(partial_local, dtype=np.float64), np.asarray(misfit_local, dtype=np.float64)
    if partial_local.ndim != 4 or misfit_local.ndim != 2 or misfit_local.shape[1] != partial_local.shape[0]:
        raise ValueError("gather_survey_gradient: `partial_local` must have shape (n_mine, nx, ny, nz) and `misfit_local` "
                         f"(n_src, n_mine); provided: {partial_local.shape}, {misfit_local.shape}.")
    if not (dist.is_available() and dist.is_initialized()):
        return combine_survey_gradient([(partial_local, misfit_local)], partial_local.shape[0])
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    n_mine = len(my_frequencies(freqs, rank, world))
    if partial_local.shape[0] != n_mine:
        raise ValueError(f"gather_survey_gradient: rank {rank} owns {n_mine} frequencies, got partials of shape "
                         f"{partial_local.shape}.")
    vnC, ns = tuple(partial_local.shape[1:]), misfit_local.shape[0]
    nC = int(np.prod(vnC))
    local = [np.concatenate([partial_local[j].ravel(order='F'), misfit_local[:, j]]) for j in range(n_mine)]
    got = gather_fields(local, group=group)
    per_rank = []
    for r in range(world):
        p = np.zeros((len(got[r]),) + vnC[::-1]).transpose(0, 3, 2, 1)
        m = np.zeros((ns, len(got[r])))
        for j, a in enumerate(got[r]):
            p[j] = a[:nC].reshape(vnC, order='F')
            m[:, j] = a[nC:]
        per_rank.append((p, m))
    return combine_survey_gradient(per_rank, len(freqs))


def gather_fields(local, group=None, device=None):
    """All-gather equally sized 1-D field arrays (complex128/float64).

    ``local``: list of NumPy arrays (this rank's fields, all the same length; may be EMPTY: a rank
    owns no frequency when there are fewer frequencies than ranks) or a single array.  Returns a list
    over ranks of lists of arrays.  Uses ``torch.distributed`` (nccl -> device tensors, gloo -> host
    tensors); with an un-initialised process group it degenerates to ``[local]``.

    The ranks first agree on (count, length, complex?) through a small header all_gather, so that a
    rank without fields takes part in the payload collective with a zero-filled buffer instead of
    raising before it (which would leave the other ranks blocked in the collective).

    ``device`` (nccl only): the GPU whose memory stages the collective -- this rank's own (``DeviceMG.device`` / LOCAL_RANK);
    default: the calling thread's current device (the library's stateless calls leave it unchanged).
    """
    import torch
    import torch.distributed as dist
    single = isinstance(local, np.ndarray)
    arrs = [local] if single else list(local)
    if not (dist.is_available() and dist.is_initialized()):
        return [arrs]
    world = dist.get_world_size(group)
    on_gpu = dist.get_backend(group) == "nccl"
    device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if on_gpu else torch.device("cpu")
    have = len(arrs) > 0
    head = torch.tensor([len(arrs), arrs[0].size if have else 0,
                         int(np.iscomplexobj(arrs[0])) if have else 0], dtype=torch.int64, device=device)
    heads = [torch.zeros_like(head) for _ in range(world)]
    dist.all_gather(heads, head, group=group)
    heads = [[int(v) for v in h_.tolist()] for h_ in heads]
    cnts = [h_[0] for h_ in heads]
    owners = [h_ for h_ in heads if h_[0] > 0]
    if not owners:
        return [[] for _ in range(world)]
    n, cplx = owners[0][1], bool(owners[0][2])
    if any(h_[1] != n or bool(h_[2]) != cplx for h_ in owners):
        raise ValueError(f"gather_fields: ranks disagree on field length / dtype: {heads}")
    per = n * (2 if cplx else 1)
    pad = torch.zeros(max(cnts) * per, dtype=torch.float64, device=device)
    if have:
        stack = np.stack([np.ascontiguousarray(a) for a in arrs])
        flat = torch.from_numpy(stack.view(np.float64).reshape(-1).copy())
        pad[:flat.numel()] = flat.to(device)
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    out = []
    for c, p in zip(cnts, parts):
        a = p[:c * per].cpu().numpy().reshape(c, per)
        a = a.view(np.complex128) if cplx else a
        out.append([a[i].copy() for i in range(c)])
    return out


class _DevArray:
    """A device buffer owned by a multigrid handle, seen through ``__cuda_array_interface__`` so that
    ``torch.as_tensor`` wraps it WITHOUT a copy (float64 view: complex128 = 2 doubles per entry)."""

    def __init__(self, ptr, n_doubles, owner):
        self.__cuda_array_interface__ = {"shape": (int(n_doubles),), "typestr": "<f8", "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner       # keeps the handle (and with it the memory) alive


def efield_tensor(dev):
    """The handle's level-0 electric field in HBM as a torch float64 tensor (zero copy; re/im
    interleaved for complex128 handles).  C ABI: ``emg3d_mg_efield_devptr`` / ``emg3d_mg_nE``.

    A SNAPSHOT: large levels keep the field in a parity-split working copy between cycles, and the call converts it back
    into the reference-layout buffer the tensor wraps (on the handle's stream; torch's CURRENT stream is made to wait for
    that stream before the tensor is returned, so torch work enqueued afterwards sees the converted field; consumers on
    other streams order themselves behind ``dev.stream_ptr``).  Valid until the next cycle / smoothing / solve call on the
    handle; call again afterwards instead of keeping the tensor, and do not write through it."""
    import torch
    from emg3d_amd._lib import HipLibraryError
    per = 2 if dev.dtype == np.complex128 else 1
    ptr = dev.efield_devptr         # (enqueues the conversion to the reference layout on the handle's stream)
    if not ptr:
        raise HipLibraryError("emg3d_mg_efield_devptr returned NULL: the handle is closed or a device call failed")
    t = torch.as_tensor(_DevArray(ptr, dev.nE * per, dev), device=torch.device("cuda", dev.device))
    # a torch consumer runs on torch's current stream: order it behind the handle's stream (no host synchronisation)
    torch.cuda.current_stream(t.device).wait_stream(torch.cuda.ExternalStream(dev.stream_ptr, device=t.device))
    return t


def gather_efield_device(dev, group=None):
    """Device-resident end-of-run gather: ONE ``all_gather_into_tensor`` of the handle's
    field straight out of its HBM buffer over RCCL/xGMI -- no host staging, no copy of the input.
    The collective is ordered behind the handle's own HIP stream (``emg3d_mg_stream``) by a stream wait, so no host
    synchronisation separates the last cycle from the gather.  Returns a (world, nE [*2]) float64
    device tensor (row r = rank r's field); ``.view(torch.complex128)`` rows for complex handles."""
    import torch
    import torch.distributed as dist
    src = efield_tensor(dev)
    if not (dist.is_available() and dist.is_initialized()):
        return src.clone().unsqueeze(0)
    world = dist.get_world_size(group)
    out = torch.empty((world, src.numel()), dtype=torch.float64, device=src.device)
    # The collective runs on torch's current stream, ordered behind the handle's stream by stream waits in both
    # directions (no host synchronisation).  It is NOT enqueued on the handle's stream itself: the process group's
    # watchdog thread keeps querying the events it records on the stream of a collective, and a later handle
    # whose stream the runtime gives the same address may be capturing a graph by then (hipErrorCapturedEvent).
    ext = torch.cuda.ExternalStream(dev.stream_ptr, device=src.device)
    cur = torch.cuda.current_stream(src.device)
    cur.wait_stream(ext)
    dist.all_gather_into_tensor(out.view(-1), src, group=group)    # flat output: the form every backend accepts
    ext.wait_stream(cur)        # later cycles of the handle do not overwrite the field under the collective
    return out
