// sbm_integrators.hpp -- ODE / forward-sensitivity integrators for gfx950 (CDNA4).
//
// Replaces the per-trajectory hot loop of the reference:
//   OdeModel.simulate       (model/ode_model.py:128-169)  -> state kernels
//   OdeModel.calc_jacobian  (model/ode_model.py:83-126)   -> sensitivity kernels
// which there is scipy.integrate.odeint (LSODA, Fortran) calling a Python RHS.
//
// Two mappings, chosen per kernel kind:
//
//  * sensitivity kernels: ONE TRAJECTORY PER WAVEFRONT.  The augmented state is
//    the n x (1+k) matrix Z = [ y | S ]; lane c of the wave owns column c
//    (lane 0 the state, lane 1+j the sensitivities w.r.t. parameter j) and keeps
//    all n rows of it, for every Runge-Kutta stage, in VGPRs.  A column evolves
//    as  z_c' = J_y(y) z_c + J_p[:, c]  and lane 0 as y' = f(y); y is broadcast
//    from lane 0 (v_readfirstlane -> SGPRs), J_y / J_p / f are evaluated once per
//    stage from scalar operands, and the sparse per-column product is unrolled
//    with static indices (SbmModel::apply_col).  No LDS, no HBM traffic inside
//    the step loop; step-size control is wave-uniform (no divergence).
//
//  * state-only kernels: ONE TRAJECTORY PER LANE (n is tiny; there is nothing to
//    spread over a wave).  Parameters are loaded coalesced and parked in LDS,
//    transposed to [param][lane] so that every access is conflict-free.
//
// The generated model header must define `struct SbmModel` (see
// sysbio_modeling_amd/symbolic/emit.py::emit_hip) and may use SBM_RCP.
//
// Which kernel a call runs, and which instantiations a plugin contains, is said in one place: sbm_kernel_choice.hpp
// (sbm_choose_kernel, sbm_kernel_built -- plain C++, checked on the host by tests/test_kernel_choice_cpu.py).
//
// This file is the umbrella the plugins and tests include; the code is in the headers below, by role, and they are
// included here only, in this order (none of them stands on its own).
#pragma once
#include <type_traits>

#include "sbm_plugin.h"
#include "sbm_wave.hpp"           // scalar helpers, SBM_* macros of the model headers, DPP reductions
#include "sbm_row_operands.hpp"   // the row-class contract: row table, operand exchange, row evaluation
#include "sbm_rk_drivers.hpp"     // tableaus, sbm_dopri45 / sbm_dop853 / sbm_rk4, kernel prologue / epilogue
#include "sbm_kernels_lane.hpp"   // SensSystem / StateSystem and their kernels
#include "sbm_kernels_rowlane.hpp"    // row-lane, state-rows and the two packed kernels
#include "sbm_kernels_rowgroup.hpp"   // row-group kernel
#include "sbm_implicit_midpoint.hpp"  // sbm_imid_kernel (includes sbm_implicit_stepper.hpp)
#include "sbm_implicit_adaptive.hpp"
#include "sbm_implicit_extrap.hpp"
#include "sbm_implicit_extrap_seq.hpp"
#include "sbm_sens_mfma.hpp"

// What the implicit kernels can hold: every lane keeps a whole column of S (NV values) and the solver's work vector
// in registers (4 NV VGPRs: beyond about 110 state variables the compiler spills), the error-controlled kernel parks two
// more copies of S in LDS.
template <class M>
struct SbmImplicitFits {
  static constexpr bool fixed = M::NV <= SBM_IMPLICIT_MAX_NV && sizeof(SbmImidShared<M>) <= 160u * 1024u;
  static constexpr bool adaptive = M::NV <= SBM_IMPLICIT_MAX_NV && sizeof(SbmImadShared<M>) <= 160u * 1024u;
};

// the host side: sbm_kernel_choice.hpp decides which of these kernels a call runs, sbm_launch_model launches it (used by
// sbm_plugin_main.hip)
#include "sbm_launch.hpp"
