// Translation unit of the instantiations of the two-steps-per-sweep kernel that add PAGED SOURCE TERMS (fdtd_kernels2.hpp, kF2Src;
// round 6): step pairs while a TFSF box, a mode plane, a current sheet or any list of more than kMaxInj nodes injects.  Always with
// non-temporal stores and the monitor table (kF2NT, kF2Mon); with / without materials; whole grid (with / without absorber layers)
// or clipped to the bulk of a shell pair; the materials ones also with the dispersive cells' memory terms (kF2Disp).
// Workgroups of up to 8 waves run under __launch_bounds__(512), larger ones under 1024.  Own unit: compiles beside the others.
#include "fdtd_static_kernels.hpp"
#include "fdtd_kernels2.hpp"

namespace fdtd {

FDTD_F2_LAUNCHER(launch_fused2_step_src, FDTD_F2_LIST_SRC)

}  // namespace fdtd
