// Translation unit of the instantiations of the two-steps-per-sweep kernel that advance DISPERSIVE cells inside the sweep
// (fdtd_kernels2.hpp, kF2Disp; round 6): materials + ADE, with / without the monitor table, whole grid (with / without absorber
// layers) or clipped to the bulk of a shell pair.  Always non-temporal stores; workgroups of up to 8 waves run under
// __launch_bounds__(512), larger ones under 1024.  Own unit so that it compiles beside the others; same flags (-fno-slp-vectorize).
#include "fdtd_static_kernels.hpp"
#include "fdtd_kernels2.hpp"

namespace fdtd {

FDTD_F2_LAUNCHER(launch_fused2_step_disp, FDTD_F2_LIST_DISP)

}  // namespace fdtd
