// Translation unit of the two-sided chain kernel on the mirrored factorisation (smooth_thm.hpp): instantiations and launcher.
#include "sweep_launch.hpp"
// -DEMG3D_UNIT_T=0 | 1: only the float64 | complex128 instantiations (the build compiles the heavy families once per type)
#ifndef EMG3D_UNIT_T
#define EMG3D_UNIT_T 2
#endif
#include "smooth_thm.hpp"

template <class T, int ST, int LPW>
static void thm_launch_l(bool zsep, int kz, dim3 grid, hipStream_t st, const LineArgs<T>& a) {
    const size_t dyn = (size_t)kz * thm_keep_step_bytes<T, LPW>();
    if (zsep) hipLaunchKernelGGL((k_line_sweep_thm<T, ST, LPW, true>), grid, dim3(EMG_RP_BLOCK), dyn, st, a, kz);
    else hipLaunchKernelGGL((k_line_sweep_thm<T, ST, LPW, false>), grid, dim3(EMG_RP_BLOCK), dyn, st, a, kz);
}
template <class T, int ST>
static void thm_launch_s(int lpw, bool zsep, int kz, dim3 grid, hipStream_t st, const LineArgs<T>& a) {
    if (lpw == 4) thm_launch_l<T, ST, 4>(zsep, kz, grid, st, a);
    else if (lpw == 12) thm_launch_l<T, ST, 12>(zsep, kz, grid, st, a);
    else thm_launch_l<T, ST, 8>(zsep, kz, grid, st, a);
}
template <class T>
void thm_launch(int stages, int lpw, bool zsep, int kz, dim3 grid, hipStream_t st, const LineArgs<T>& a) {
    if (stages == 2) thm_launch_s<T, 2>(lpw, zsep, kz, grid, st, a);
    else thm_launch_s<T, 3>(lpw, zsep, kz, grid, st, a);
}
#if EMG3D_UNIT_T != 1
template void thm_launch<double>(int, int, bool, int, dim3, hipStream_t, const LineArgs<double>&);
#endif
#if EMG3D_UNIT_T != 0
template void thm_launch<c128>(int, int, bool, int, dim3, hipStream_t, const LineArgs<c128>&);
#endif

template <class T, int ST, int LPW>
static bool thm_attr(int lds_limit) {
    const int dyn = lds_limit - (int)thm_static_lds<T, LPW>();
    if (dyn < 0) return false;
    bool ok = true;
    auto dyn_lds = [&](const void* f) {
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, dyn) != hipSuccess) { (void)hipGetLastError(); ok = false; }
    };
    dyn_lds(reinterpret_cast<const void*>(&k_line_sweep_thm<T, ST, LPW, false>));
    dyn_lds(reinterpret_cast<const void*>(&k_line_sweep_thm<T, ST, LPW, true>));
    return ok;
}
template <class T>
bool thm_attrs(int lds_limit) {
    bool ok = thm_attr<T, 3, 4>(lds_limit);
    ok = thm_attr<T, 3, 8>(lds_limit) && ok;
    ok = thm_attr<T, 3, 12>(lds_limit) && ok;
    ok = thm_attr<T, 2, 4>(lds_limit) && ok;
    ok = thm_attr<T, 2, 8>(lds_limit) && ok;
    ok = thm_attr<T, 2, 12>(lds_limit) && ok;
    return ok;
}
#if EMG3D_UNIT_T != 1
template bool thm_attrs<double>(int);
#endif
#if EMG3D_UNIT_T != 0
template bool thm_attrs<c128>(int);
#endif
