// Translation unit of the WHAT-IF and PREFETCH instantiations of the two-steps-per-sweep kernel (fdtd_kernels2.hpp, the kF2WhatifShift field of OPT;
// FDTD_OPT_WHATIF): measuring aids that skip part of the sweep's work — wrong results, meaningful times — switched inside one
// engine by scripts/probe_whatif.py.  Vacuum instantiation, 16-wave workgroups only.  Own unit: compiles beside the others.
#include "fdtd_static_kernels.hpp"
#include "fdtd_kernels2.hpp"

namespace fdtd {

FDTD_F2_LAUNCHER(launch_fused2_step_whatif, FDTD_F2_LIST_WHATIF)

}  // namespace fdtd
