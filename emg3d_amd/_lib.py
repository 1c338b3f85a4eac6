"""ctypes binding of ``libemg3d_hip.so`` (C ABI: ``include/emg3d_hip.h``).

The product path has NO CPU fallback: if the HIP library is missing or a call
fails, an exception is raised.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library.  EMG3D_HIP_LIB: another build of it (A/B runs in one gpurun call).
LIB_PATH = os.environ.get("EMG3D_HIP_LIB") or os.path.join(_HERE, "libemg3d_hip.so")
# The lab build (-DEMG3D_LAB): the same library plus the superseded kernel variants and one environment variable per
# tuning knob; only tests/test_gpu_variants.py and tools/ load it (`use(LAB_PATH)`).
LAB_PATH = os.path.join(_HERE, "libemg3d_hip_lab.so")

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_vp = ctypes.c_void_p
c_double = ctypes.c_double
c_dp = ctypes.POINTER(ctypes.c_double)

# include/emg3d_hip.h: EMG3D_HIP_ABI_VERSION -- a library built from another header version is refused at load
ABI_VERSION = 121

# name -> (restype, argtypes); mirrors include/emg3d_hip.h one to one.
SIGNATURES = {
    "emg3d_hip_version": (c_int, []),
    "emg3d_hip_device_count": (c_int, [ctypes.POINTER(c_int)]),
    "emg3d_hip_set_device": (c_int, [c_int]),
    "emg3d_hip_device_info": (c_int, [c_int, ctypes.c_char_p, ctypes.POINTER(c_i64), ctypes.POINTER(c_int)]),
    "emg3d_hip_mem_info": (c_int, [c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "emg3d_hip_release_cached": (c_i64, []),
    "emg3d_hip_cached_bytes": (c_i64, []),
    "emg3d_hip_cached_bytes_on": (c_i64, [c_int]),
    "emg3d_mg_placement": (c_int, [c_vp, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_float)]),
    "emg3d_amat_x": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "emg3d_get_h_field": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_double, c_double]),
    "emg3d_gauss_seidel": (c_int, [c_int, c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                   c_vp, c_vp, c_vp, c_int, c_int]),
    "emg3d_restrict": (c_int, [c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_int]),
    "emg3d_restrict_weights": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "emg3d_solve": (c_int, [c_int, c_vp, c_vp, c_i64]),
    "emg3d_blocks_to_amat": (c_int, [c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64]),
    "emg3d_prolongation": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int]),
    "emg3d_restrict_model": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_int]),
    "emg3d_sweep_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, ctypes.c_char_p, ctypes.POINTER(c_i64)]),
    "emg3d_sweep_scantab": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, ctypes.POINTER(c_i64)]),
    "emg3d_sweep_thm_zkeep": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, ctypes.POINTER(c_i64)]),
    "emg3d_sweep_fuse_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_i64, ctypes.POINTER(c_i64),
                                      ctypes.POINTER(c_i64), c_i64]),
    "emg3d_mg_create": (c_int, [ctypes.POINTER(c_vp), c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp,
                                c_vp, c_vp, c_vp, c_vp, c_int]),
    "emg3d_mg_destroy": (None, [c_vp]),
    "emg3d_mg_create_sv": (c_int, [ctypes.POINTER(c_vp), c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp,
                                   c_vp, c_vp, c_vp, c_vp, c_double, c_double, c_int]),
    "emg3d_mg_create_vs": (c_int, [ctypes.POINTER(c_vp), c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp,
                                   c_vp, c_vp, c_vp, c_vp, c_vp, c_double, c_double, c_int, c_int]),
    "emg3d_mg_create_vse": (c_int, [ctypes.POINTER(c_vp), c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp,
                                    c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_double, c_double, c_double, c_int, c_int]),
    "emg3d_mg_set_smu0_eps": (c_int, [c_vp, c_double, c_double, c_double]),
    "emg3d_mg_set_model": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp]),
    "emg3d_mg_get_sigma": (c_int, [c_vp, c_int, c_vp]),
    "emg3d_mg_set_sfield_vector": (c_int, [c_vp, c_vp, c_double, c_double]),
    "emg3d_mg_set_sfield_dipole": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_vp]),
    "emg3d_source_field": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    "emg3d_mg_prepare": (c_int, [c_vp, c_int, c_int]),
    "emg3d_mg_set_trace": (c_int, [c_vp, c_int]),
    "emg3d_mg_get_trace": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp]),
    "emg3d_mg_set_params": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int]),
    "emg3d_mg_set_sfield": (c_int, [c_vp, c_vp]),
    "emg3d_mg_set_efield": (c_int, [c_vp, c_vp]),
    "emg3d_mg_get_efield": (c_int, [c_vp, c_vp]),
    "emg3d_mg_get_residual": (c_int, [c_vp, c_vp]),
    "emg3d_mg_get_hfield": (c_int, [c_vp, c_int, c_double, c_double, c_vp]),
    "emg3d_interp3d": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_int, c_int, c_double,
                               c_double, c_vp]),
    "emg3d_get_receiver_response": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_i64,
                                            c_vp, c_vp, c_vp]),
    "emg3d_mg_get_receiver_response": (c_int, [c_vp, c_int, c_int, c_double, c_double, c_i64, c_vp, c_vp, c_vp]),
    "emg3d_edges2cellaverages": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "emg3d_mg_gradient": (c_int, [c_vp, c_int, c_double, c_double, c_vp]),
    "emg3d_mg_gradient3": (c_int, [c_vp, c_int, c_double, c_double, c_vp, c_vp, c_vp]),
    "emg3d_mg_grad_acc_reset": (c_int, [c_vp]),
    "emg3d_mg_grad_acc_add": (c_int, [c_vp, c_int, c_double, c_double, c_vp]),
    "emg3d_mg_grad_acc_get": (c_int, [c_vp, c_vp]),
    "emg3d_mg_grad_acc3_reset": (c_int, [c_vp]),
    "emg3d_mg_grad_acc3_add": (c_int, [c_vp, c_int, c_double, c_double, c_vp]),
    "emg3d_mg_grad_acc3_get": (c_int, [c_vp, c_vp, c_vp, c_vp]),
    "emg3d_mg_sens_acc_add": (c_int, [c_vp, c_int, c_double, c_double, c_vp, c_vp, c_vp, c_int]),
    "emg3d_mg_sens_rows_count": (c_i64, [c_vp, c_vp, c_int]),
    "emg3d_mg_sens_rows": (c_int, [c_vp, c_int, c_double, c_double, c_vp, c_vp, c_int, c_int, c_vp]),
    "emg3d_rows_create": (c_int, [c_int, c_i64, c_i64, ctypes.POINTER(c_vp)]),
    "emg3d_rows_destroy": (None, [c_vp]),
    "emg3d_rows_bytes": (c_i64, [c_vp]),
    "emg3d_rows_set": (c_int, [c_vp, c_i64, c_vp]),
    "emg3d_rows_get": (c_int, [c_vp, c_i64, c_vp]),
    "emg3d_rows_set_chain": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "emg3d_mg_sens_rows_park": (c_int, [c_vp, c_int, c_double, c_double, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_int, c_int]),
    "emg3d_mg_sens_rows_fill": (c_int, [c_vp, c_int, c_double, c_double, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int]),
    "emg3d_rows_gram": (c_int, [c_vp, c_vp, c_vp]),
    "emg3d_rows_matvec": (c_int, [c_vp, c_vp, c_vp]),
    "emg3d_rows_rmatvec": (c_int, [c_vp, c_vp, c_vp, c_vp]),
    "emg3d_rows_gram_plan": (c_int, [c_i64, c_i64, ctypes.POINTER(c_i64)]),
    "emg3d_rows_gram_job": (c_int, [c_i64, c_i64, ctypes.POINTER(c_i64)]),
    "emg3d_rows_gram_batch": (c_int, [c_i64, c_i64, ctypes.POINTER(c_i64)]),
    "emg3d_rows_smooth_plan": (c_int, [c_i64, c_i64, c_i64, c_int, ctypes.POINTER(c_i64)]),
    "emg3d_smooth3d": (c_int, [c_int, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int,
                               c_vp]),
    "emg3d_rows_smooth": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int]),
    "emg3d_rows_smooth_l": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int]),
    "emg3d_rows_clone": (c_int, [c_vp, ctypes.POINTER(c_vp)]),
    "emg3d_rows_project_plan": (c_int, [c_i64, c_i64, c_i64, ctypes.POINTER(c_i64)]),
    "emg3d_rows_project": (c_int, [c_vp, c_vp, c_i64, c_vp]),
    "emg3d_rows_colsumsq": (c_int, [c_vp, c_vp, c_vp]),
    "emg3d_cells2edges": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "emg3d_mg_jvec_source": (c_int, [c_vp, c_int, c_double, c_double, c_vp, c_vp, c_vp]),
    "emg3d_mg_jvec_source_b": (c_int, [c_vp, c_int, c_double, c_double, c_vp, c_vp, c_vp, c_vp]),
    "emg3d_mg_get_receiver_response_linear": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "emg3d_mg_set_receiver_adjoint": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_int]),
    "emg3d_mg_get_receiver_response_linear_h": (c_int, [c_vp, c_double, c_double, c_i64, c_vp, c_vp, c_vp]),
    "emg3d_mg_set_receiver_adjoint_ex": (c_int, [c_vp, c_int, c_int, c_double, c_double, c_i64, c_vp, c_vp, c_vp, c_int]),
    "emg3d_mg_set_receiver_adjoint_b": (c_int, [c_vp, c_int, c_int, c_double, c_double, c_i64, c_vp, c_vp, c_vp, c_vp, c_int]),
    "emg3d_receiver_adjoint": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_double, c_double,
                                       c_i64, c_vp, c_vp, c_vp, c_vp]),
    "emg3d_volume_average_weights": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "emg3d_volume_average": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp,
                                     c_vp, c_vp, c_vp]),
    "emg3d_volume_average_old_offsets": (c_int, [c_vp, c_i64, c_i64, c_vp]),
    "emg3d_volume_average_adjoint": (c_int, [c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp,
                                             c_vp, c_vp]),
    "emg3d_mg_set_model_grid": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp]),
    "emg3d_mg_set_regrid_factors": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "emg3d_mg_grad_acc_get_model": (c_int, [c_vp, c_vp]),
    "emg3d_mg_grad_acc3_get_model": (c_int, [c_vp, c_vp, c_vp, c_vp]),
    "emg3d_interp3d_grid": (c_int, [c_int, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64,
                                    c_vp, c_int, c_int, c_double, c_double, c_vp]),
    "emg3d_mg_set_batch": (c_int, [c_vp, c_int]),
    "emg3d_mg_get_batch": (c_int, [c_vp]),
    "emg3d_mg_select": (c_int, [c_vp, c_int]),
    "emg3d_mg_set_mask": (c_int, [c_vp, c_vp]),
    "emg3d_mg_residual_norm": (c_int, [c_vp, c_dp]),
    "emg3d_mg_sfield_norm": (c_int, [c_vp, c_dp]),
    "emg3d_mg_smooth": (c_int, [c_vp, c_int, c_int]),
    "emg3d_mg_begin": (c_int, [c_vp, c_int]),
    "emg3d_mg_set_smu0": (c_int, [c_vp, ctypes.c_double, ctypes.c_double]),
    "emg3d_mg_cycle": (c_int, [c_vp, c_int, c_int, c_dp]),
    "emg3d_mg_cycle_next": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_dp]),
    "emg3d_mg_cycles": (c_int, [c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp]),
    "emg3d_mg_efield_devptr": (c_vp, [c_vp]),
    "emg3d_mg_sfield_devptr": (c_vp, [c_vp]),
    "emg3d_mg_stream": (c_vp, [c_vp]),
    "emg3d_mg_nE": (c_i64, [c_vp]),
    "emg3d_mg_sync": (c_int, [c_vp]),
    "emg3d_mg_device_bytes": (c_i64, [c_vp]),
    "emg3d_mg_time_sweep": (c_int, [c_vp, c_int, c_int, ctypes.POINTER(ctypes.c_float)]),
    "emg3d_mg_last_sweep_kernel": (c_int, [c_vp, ctypes.c_char_p]),
    "emg3d_mg_time_residual": (c_int, [c_vp, c_int, ctypes.POINTER(ctypes.c_float)]),
    "emg3d_mg_last_residual_kernel": (c_int, [c_vp, ctypes.c_char_p]),
    "emg3d_mg_amatvec": (c_int, [c_vp, c_vp, c_vp]),
    "emg3d_mg_vec_alloc": (c_int, [c_vp, c_int]),
    "emg3d_mg_vec_set": (c_int, [c_vp, c_int, c_vp]),
    "emg3d_mg_vec_get": (c_int, [c_vp, c_int, c_vp]),
    "emg3d_mg_vec_copy": (c_int, [c_vp, c_int, c_int]),
    "emg3d_mg_vec_axpy": (c_int, [c_vp, c_int, c_double, c_double, c_int]),
    "emg3d_mg_vec_scale": (c_int, [c_vp, c_int, c_double, c_double]),
    "emg3d_mg_vec_dot": (c_int, [c_vp, c_int, c_int, c_dp]),
    "emg3d_mg_vec_amatvec": (c_int, [c_vp, c_int, c_int]),
    "emg3d_mg_bvec_alloc": (c_int, [c_vp, c_int]),
    "emg3d_mg_bvec_copy": (c_int, [c_vp, c_int, c_int]),
    "emg3d_mg_bvec_zero": (c_int, [c_vp, c_int]),
    "emg3d_mg_bvec_axpy": (c_int, [c_vp, c_int, c_vp, c_int]),
    "emg3d_mg_bvec_scale": (c_int, [c_vp, c_int, c_vp]),
    "emg3d_mg_bvec_dot": (c_int, [c_vp, c_int, c_int, c_vp]),
    "emg3d_mg_bvec_amatvec": (c_int, [c_vp, c_int, c_int]),
    "emg3d_mg_bvec_get": (c_int, [c_vp, c_int, c_int, c_vp]),
    "emg3d_mg_bvec_set": (c_int, [c_vp, c_int, c_int, c_vp]),
}

_lib = None
_path = None
_loaded = {}


class HipLibraryError(RuntimeError):
    """The HIP extension is missing or a device call failed."""


def _open(path):
    if path in _loaded:
        return _loaded[path]
    if not os.path.exists(path):
        raise HipLibraryError(
            f"{path} not found: the HIP extension is not built. Build it with\n"
            "  python -c 'import __graft_entry__ as g; g.build()'   (needs hipcc)\n"
            "emg3d_amd has no CPU fallback.")
    lib = ctypes.CDLL(path)
    try:
        lib.emg3d_hip_version.restype = c_int
        got = int(lib.emg3d_hip_version())
    except AttributeError:
        got = None
    if got != ABI_VERSION:
        raise HipLibraryError(
            f"{path} has ABI version {got}, this package needs {ABI_VERSION} (include/emg3d_hip.h: EMG3D_HIP_ABI_VERSION): "
            "a stale build. Rebuild it with\n  python -c 'import __graft_entry__ as g; g.build(force=True)'")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a symbol is missing
        fn.restype = res
        fn.argtypes = args
    _loaded[path] = lib
    return lib


def load():
    """The library of this process (loaded once; every prototype declared)."""
    global _lib, _path
    if _lib is None:
        _lib, _path = _open(LIB_PATH), LIB_PATH
    return _lib


def use(path=None):
    """Make another build of the library the one `load()` returns (None: back to LIB_PATH).  Objects created before
    keep the build they were created with.  Returns the previous path."""
    global _lib, _path
    prev = _path or LIB_PATH
    want = path or LIB_PATH
    _lib, _path = _open(want), want
    return prev


def check(status, what):
    if status != 0:
        raise HipLibraryError(f"{what} failed with status {status} "
                              f"({'invalid argument' if status < 0 else 'HIP error'})")


def dtype_code(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.complex128:
        return 1
    if dtype == np.float64:
        return 0
    raise TypeError(f"fields must be float64 or complex128, got {dtype}")


def ptr(a):
    return a.ctypes.data_as(c_vp)


def device_count():
    n = c_int(0)
    check(load().emg3d_hip_device_count(ctypes.byref(n)), "emg3d_hip_device_count")
    return n.value


def device_info(device=0):
    name = ctypes.create_string_buffer(256)
    mem = c_i64(0)
    cus = c_int(0)
    check(load().emg3d_hip_device_info(device, name, ctypes.byref(mem), ctypes.byref(cus)),
          "emg3d_hip_device_info")
    return {"name": name.value.decode(), "total_mem": mem.value, "cu_count": cus.value}


def mem_info(device=0):
    """(free, total) bytes of `device` as the driver reports them now, and what this process's own block pool holds (parked
    blocks count as used for the driver, but the next allocation of the process may take them)."""
    fr, tot = c_i64(0), c_i64(0)
    check(load().emg3d_hip_mem_info(device, ctypes.byref(fr), ctypes.byref(tot)), "emg3d_hip_mem_info")
    return {"free": fr.value, "total": tot.value, "pooled": int(load().emg3d_hip_cached_bytes()),
            "pooled_on_device": int(load().emg3d_hip_cached_bytes_on(device))}


def sweep_plan(vnC, direction, dtype=np.complex128, ordering='colour', nsys=1, cu_count=0):
    """The line-sweep kernel the library selects for a level of ``vnC`` cells along ``direction`` (1, 2, 3) on a device of
    ``cu_count`` compute units (0: the current device) -- ``emg3d_sweep_plan``: shape logic only, runs without a GPU when
    ``cu_count`` > 0.  Returns the instantiation's name and the launch shape."""
    name = ctypes.create_string_buffer(64)
    info, tab = (c_i64 * 6)(), (c_i64 * 4)()
    check(load().emg3d_sweep_scantab(dtype_code(dtype), int(vnC[0]), int(vnC[1]), int(vnC[2]), int(direction),
                                     1 if ordering == 'colour' else 0, int(nsys), int(cu_count), tab), "emg3d_sweep_scantab")
    check(load().emg3d_sweep_plan(dtype_code(dtype), int(vnC[0]), int(vnC[1]), int(vnC[2]), int(direction),
                                  1 if ordering == 'colour' else 0, int(nsys), int(cu_count), name, info), "emg3d_sweep_plan")
    return {"kernel": name.value.decode(), "lines_per_colour": info[0], "lines_per_wave": info[1], "rounds": info[2],
            "factor_kind": info[3], "split": bool(info[4]), "big_offsets": bool(info[5]), "scan_table": bool(tab[0]),
            "scan_table_bytes": tab[1]}


def sweep_thm_zkeep(vnC, direction, dtype=np.complex128, ordering='colour', nsys=1, cu_count=0):
    """How many forward steps per half of a line keep their intermediate result in LDS where ``k_line_sweep_thm`` serves a level of
    ``vnC`` cells along ``direction`` (1, 2, 3) -- ``emg3d_sweep_thm_zkeep``: shape logic only, runs without a GPU when
    ``cu_count`` > 0.  All zero where another kernel serves."""
    info = (c_i64 * 6)()
    check(load().emg3d_sweep_thm_zkeep(dtype_code(dtype), int(vnC[0]), int(vnC[1]), int(vnC[2]), int(direction),
                                       1 if ordering == 'colour' else 0, int(nsys), int(cu_count), info), "emg3d_sweep_thm_zkeep")
    return {"cap": info[0], "dyn_lds_bytes": info[1], "static_lds_bytes": info[2], "half": info[3], "kept": info[4],
            "lines_per_pair": info[5]}


def sweep_fuse_plan(vnC, direction, npass, dtype=np.complex128, ordering='colour', nsys=1, cu_count=0, own=0, max_seg=0, budget=0):
    """How the library issues a smoothing call of ``npass`` colour passes along ``direction`` (1, 2, 3) on a level of ``vnC`` cells
    -- ``emg3d_sweep_fuse_plan``: per-pass launches (``fused`` False) or all passes in one launch on private slab copies.  Shape
    logic only.  ``slabs``: per slab the own line nodes ``own`` = (x0, x1), the owned edge indices ``edges`` = (a, b), both half
    open, and per pass the live nodes (lo, hi), inclusive."""
    info = (c_i64 * 8)()
    cap = (4 + 2 * max(int(npass), 0)) * (max(vnC) + 1)
    ranges = (c_i64 * cap)()
    check(load().emg3d_sweep_fuse_plan(dtype_code(dtype), int(vnC[0]), int(vnC[1]), int(vnC[2]), int(direction),
                                       1 if ordering == 'colour' else 0, int(nsys), int(cu_count), int(npass), int(own), int(max_seg), int(budget),
                                       info, ranges, cap), "emg3d_sweep_fuse_plan")
    out = {"fused": bool(info[0]), "axis": info[1], "nX": info[2], "own": info[3], "nslabs": info[4], "npass": info[5],
           "waves": info[6], "scratch_bytes": info[7], "slabs": []}
    if out["fused"]:
        per = 4 + 2 * int(npass)
        for k in range(info[4]):
            r = ranges[per * k:per * (k + 1)]
            out["slabs"].append({"own": (r[0], r[1]), "edges": (r[2], r[3]),
                                 "live": [(r[4 + 2 * p], r[5 + 2 * p]) for p in range(int(npass))]})
    return out


def rows_gram_plan(n_rows, n_cols):
    """The geometry of the Gram launch of a row store of ``n_rows`` x ``n_cols`` (``emg3d_rows_gram_plan``): host arithmetic, runs
    without a GPU.  ``slab``, the columns of a K-slab, follows from ``n_cols`` alone; a workgroup owns one slab and one job, a pair
    of row blocks ``ba >= bb`` of ``block`` rows; ``jobs`` lists their rows ``(a0, a1, b0, b1)``, half open (``a0 == b0``: a diagonal
    job, which computes the 16 x 16 tile pairs ``ta >= tb`` of its block only).  The jobs run in their order in ``launches`` launches
    of ``jobs_per_launch`` (``emg3d_rows_gram_batch``, what ``emg3d_rows_gram`` itself runs): as many as fit ``scratch_bytes`` of
    slab partials, ``job_bytes`` each, and at least one."""
    info = (c_i64 * 8)()
    check(load().emg3d_rows_gram_plan(int(n_rows), int(n_cols), info), "emg3d_rows_gram_plan")
    batch = (c_i64 * 4)()
    check(load().emg3d_rows_gram_batch(int(n_rows), int(n_cols), batch), "emg3d_rows_gram_batch")
    out = {"block": info[0], "kstep": info[1], "slab": info[2], "nslab": info[3], "nblocks": info[4], "njobs": info[5],
           "grid": info[6], "lds_bytes": info[7], "tile": 16, "jobs_per_launch": batch[0], "launches": batch[1],
           "job_bytes": batch[2], "scratch_bytes": batch[3], "jobs": []}
    rect = (c_i64 * 4)()
    for job in range(info[5]):
        check(load().emg3d_rows_gram_job(int(n_rows), job, rect), "emg3d_rows_gram_job")
        out["jobs"].append(tuple(rect))
    return out


def rows_project_plan(n_rows, m, n_cols):
    """The geometry of ``emg3d_rows_project`` for ``Y[m x n_cols] = M[m x n_rows] R`` (``emg3d_rows_project_plan``): host arithmetic,
    runs without a GPU, and is what the launch itself calls.  A workgroup owns a panel of ``cols`` columns and a block of ``block``
    output rows and walks the source in steps of ``kstep`` rows; ``passes`` blocks, each one pass over the source; ``panels``
    follows from ``n_cols`` alone; ``last_rows``: the rows the last block's kernel covers (32, 64, 128 or ``block``)."""
    info = (c_i64 * 8)()
    check(load().emg3d_rows_project_plan(int(n_rows), int(m), int(n_cols), info), "emg3d_rows_project_plan")
    return {"block": info[0], "cols": info[1], "kstep": info[2], "passes": info[3], "grid": info[4], "lds_bytes": info[5],
            "panels": info[6], "last_rows": info[7], "tile": 16}


def rows_smooth_plan(shape, axis):
    """How the library smooths arrays of ``shape`` = ``(nx, ny, nz)`` along ``axis`` (0, 1, 2) -- ``emg3d_rows_smooth_plan``: host
    arithmetic, runs without a GPU.  ``path`` 0: a line stays in LDS between its sweeps and passes, 1: one thread per line through
    HBM; ``workgroups`` is per array (a launch over ``n`` arrays has ``n`` times as many)."""
    info = (c_i64 * 6)()
    check(load().emg3d_rows_smooth_plan(int(shape[0]), int(shape[1]), int(shape[2]), int(axis), info), "emg3d_rows_smooth_plan")
    return {"path": info[0], "lines_per_workgroup": info[1], "lds_bytes": info[2], "workgroups": info[3], "min_lines": info[4],
            "lines": info[5]}


def factor_ptrs(factors, shape):
    """The nine factor pointers of ``emg3d_smooth3d`` / ``emg3d_rows_smooth`` from ``factors`` = per axis ``(lo, cp, inv)`` or ``None``;
    -> (pointers, the arrays that must outlive the call)."""
    if len(factors) != 3:
        raise ValueError("`factors` must have one entry per axis: (lo, cp, inv) or None.")
    ptrs, keep = [], []
    for f, n in zip(factors, shape):
        if f is None:
            ptrs += [None, None, None]
            continue
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in f]
        if len(arrs) != 3 or any(a.shape != (int(n),) for a in arrs):
            raise ValueError(f"the factors of an axis must be three arrays (lo, cp, inv) of its {int(n)} cells.")
        keep += arrs
        ptrs += [ptr(a) for a in arrs]
    return ptrs, keep


def smooth3d(data, shape, factors, passes, scale=None, scale_after=False, device=0):
    """``emg3d_smooth3d`` on ``data``, ``(n_arrays, nx * ny * nz)`` doubles (each array x fastest), in place: ``L^T`` (``scale_after``
    False) or ``L`` of maps.SmoothingCovariance; ``scale``: ``nx * ny * nz`` doubles or None."""
    nx, ny, nz = (int(n) for n in shape)
    if data.dtype != np.float64 or not data.flags.c_contiguous or data.ndim != 2 or data.shape[1] != nx * ny * nz:
        raise ValueError(f"`data` must be C-contiguous float64 of shape (n_arrays, {nx * ny * nz}).")
    ptrs, keep = factor_ptrs(factors, (nx, ny, nz))
    w = None
    if scale is not None:
        w = np.ascontiguousarray(scale, dtype=np.float64)
        if w.shape != (nx * ny * nz,):
            raise ValueError(f"`scale` must have {nx * ny * nz} entries; provided: {w.shape}.")
    check(load().emg3d_smooth3d(int(device), data.shape[0], nx, ny, nz, None if w is None else ptr(w), *ptrs, int(passes),
                                1 if scale_after else 0, ptr(data)), "emg3d_smooth3d")
    return data
