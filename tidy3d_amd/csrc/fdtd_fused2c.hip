// Translation unit of the CLIPPED instantiations of the two-steps-per-sweep kernel (fdtd_kernels2.hpp, kF2Clip): the bulk
// launch of a step pair whose shell — CPML slabs and their collar, or the boundary planes of a z-slab rank — is advanced by
// single steps beside it (fdtd_capi.hip).  Own unit so that it compiles beside fdtd_fused2.hip; same flags (-fno-slp-vectorize).
#include "fdtd_static_kernels.hpp"
#include "fdtd_kernels2.hpp"

namespace fdtd {

FDTD_F2_LAUNCHER(launch_fused2_step_clip, FDTD_F2_LIST_CLIP)

}  // namespace fdtd
