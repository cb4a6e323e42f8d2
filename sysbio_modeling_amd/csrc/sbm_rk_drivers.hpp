// sbm_rk_drivers.hpp -- the explicit Runge-Kutta drivers (DOPRI45, DOP853, RK4) over a "System" policy, their tableaus
// and stage macros, and what every kernel does before and after its trajectory (grid window, status report).
#pragma once
// ---------------------------------------------------------------------------
// Dormand-Prince 5(4) tableau (Hairer, Norsett, Wanner, vol. I, table 5.2)
// ---------------------------------------------------------------------------
namespace dp {
constexpr double C2 = 1.0 / 5.0, C3 = 3.0 / 10.0, C4 = 4.0 / 5.0, C5 = 8.0 / 9.0;
constexpr double A21 = 1.0 / 5.0;
constexpr double A31 = 3.0 / 40.0, A32 = 9.0 / 40.0;
constexpr double A41 = 44.0 / 45.0, A42 = -56.0 / 15.0, A43 = 32.0 / 9.0;
constexpr double A51 = 19372.0 / 6561.0, A52 = -25360.0 / 2187.0, A53 = 64448.0 / 6561.0, A54 = -212.0 / 729.0;
constexpr double A61 = 9017.0 / 3168.0, A62 = -355.0 / 33.0, A63 = 46732.0 / 5247.0, A64 = 49.0 / 176.0,
                 A65 = -5103.0 / 18656.0;
constexpr double A71 = 35.0 / 384.0, A73 = 500.0 / 1113.0, A74 = 125.0 / 192.0, A75 = -2187.0 / 6784.0,
                 A76 = 11.0 / 84.0;
constexpr double E1 = 71.0 / 57600.0, E3 = -71.0 / 16695.0, E4 = 71.0 / 1920.0, E5 = -17253.0 / 339200.0,
                 E6 = 22.0 / 525.0, E7 = -1.0 / 40.0;
}  // namespace dp

// ---------------------------------------------------------------------------
// Dormand-Prince 8(5,3) tableau (Hairer, Norsett, Wanner, vol. I, section II.5: DOP853), 12 stages + FSAL;
// A<i>_<j> multiplies k_j in the argument of stage i (1-based), B<j> forms the 8th-order solution, E5_<j> / E3_<j>
// the two embedded error estimates the step controller combines.  Entries that are zero are left out.
// ---------------------------------------------------------------------------
namespace dp8 {
constexpr double C2 = 0.05260015195876773, C3 = 0.0789002279381516, C4 = 0.1183503419072274, C5 = 0.2816496580927726, C6 = 0.3333333333333333, C7 = 0.25, C8 = 0.3076923076923077, C9 = 0.6512820512820513, C10 = 0.6, C11 = 0.8571428571428571, C12 = 1.0;
constexpr double A2_1 = 0.05260015195876773;
constexpr double A3_1 = 0.0197250569845379, A3_2 = 0.0591751709536137;
constexpr double A4_1 = 0.02958758547680685, A4_3 = 0.08876275643042054;
constexpr double A5_1 = 0.2413651341592667, A5_3 = -0.8845494793282861, A5_4 = 0.924834003261792;
constexpr double A6_1 = 0.037037037037037035, A6_4 = 0.17082860872947386, A6_5 = 0.12546768756682242;
constexpr double A7_1 = 0.037109375, A7_4 = 0.17025221101954405, A7_5 = 0.06021653898045596, A7_6 = -0.017578125;
constexpr double A8_1 = 0.03709200011850479, A8_4 = 0.17038392571223998, A8_5 = 0.10726203044637328, A8_6 = -0.015319437748624402, A8_7 = 0.008273789163814023;
constexpr double A9_1 = 0.6241109587160757, A9_4 = -3.3608926294469414, A9_5 = -0.868219346841726, A9_6 = 27.59209969944671, A9_7 = 20.154067550477894, A9_8 = -43.48988418106996;
constexpr double A10_1 = 0.47766253643826434, A10_4 = -2.4881146199716677, A10_5 = -0.590290826836843, A10_6 = 21.230051448181193, A10_7 = 15.279233632882423, A10_8 = -33.28821096898486, A10_9 = -0.020331201708508627;
constexpr double A11_1 = -0.9371424300859873, A11_4 = 5.186372428844064, A11_5 = 1.0914373489967295, A11_6 = -8.149787010746927, A11_7 = -18.52006565999696, A11_8 = 22.739487099350505, A11_9 = 2.4936055526796523, A11_10 = -3.0467644718982196;
constexpr double A12_1 = 2.273310147516538, A12_4 = -10.53449546673725, A12_5 = -2.0008720582248625, A12_6 = -17.9589318631188, A12_7 = 27.94888452941996, A12_8 = -2.8589982771350235, A12_9 = -8.87285693353063, A12_10 = 12.360567175794303, A12_11 = 0.6433927460157636;
constexpr double B1 = 0.054293734116568765, B6 = 4.450312892752409, B7 = 1.8915178993145003, B8 = -5.801203960010585, B9 = 0.3111643669578199, B10 = -0.1521609496625161, B11 = 0.20136540080403034, B12 = 0.04471061572777259;
constexpr double E5_1 = 0.01312004499419488, E5_6 = -1.2251564463762044, E5_7 = -0.4957589496572502, E5_8 = 1.6643771824549864, E5_9 = -0.35032884874997366, E5_10 = 0.3341791187130175, E5_11 = 0.08192320648511571, E5_12 = -0.022355307863886294;
constexpr double E3_1 = -0.18980075407240762, E3_6 = 4.450312892752409, E3_7 = 1.8915178993145003, E3_8 = -5.801203960010585, E3_9 = -0.4226823213237919, E3_10 = -0.1521609496625161, E3_11 = 0.20136540080403034, E3_12 = 0.02265179219836082;
}  // namespace dp8

// every element a lane integrates: CPL columns of NV rows, plus NX extra scalars per lane
// (row-lane kernel: the lane's own state component)
#define SBM_ALL(c, i)                       \
  _Pragma("unroll") for (int c = 0; c < CPL; ++c) \
  _Pragma("unroll") for (int i = 0; i < NVX; ++i)
// the NV column rows / the NX extra elements (the stage STATE in the row-lane / row-group kernels)
#define SBM_MAIN(c, i)                      \
  _Pragma("unroll") for (int c = 0; c < CPL; ++c) \
  _Pragma("unroll") for (int i = 0; i < NV; ++i)
#define SBM_EXTRA(c, i)                     \
  _Pragma("unroll") for (int c = 0; c < CPL; ++c) \
  _Pragma("unroll") for (int i = NV; i < NVX; ++i)
// A stage runs in three phases:
//   issue  : form the extra elements, make them visible (LDS) and START fetching the row operands;
//   eval   : evaluate f / J_y / J_p of the lane's row, publish them; the extra elements of the
//            stage derivative (kout) are known from here on;
//   finish : form the column rows of the stage vector and their derivative.
// The state path (issue, eval) does not depend on the column rows, so the drivers software-pipeline
// it: stage s+1's issue is placed between eval and finish of stage s (SBM_STAGE_THEN's `next`),
// and the LDS round trip of its operands is covered by the column work of stage s.
// `stmt` forms element [c][i] of the stage vector zt (and may update running sums next to it); it is
// run once for the extra elements (issue) and once for the column rows (finish side).
#define SBM_ISSUE(tt, stmt)                 \
  {                                         \
    SBM_EXTRA(c, i) { stmt }                \
    pend_ = sys.issue((tt), zt);            \
  }
#define SBM_STAGE_THEN(tt, stmt, kout, next) \
  {                                         \
    auto tok_ = sys.eval(pend_, (tt));      \
    sys.extra_out(tok_, kout);              \
    next                                    \
    SBM_MAIN(c, i) { stmt }                 \
    sys.finish(tok_, (tt), zt, kout);       \
  }
#define SBM_STAGE(tt, stmt, kout) SBM_ISSUE(tt, stmt) SBM_STAGE_THEN(tt, stmt, kout, )
// The same with the stage's number s (sbm_dopri45: 2..7).  A System that has eval_stage<s> decides per stage how much
// of the hand-over eval starts (RowGroupSystem: whether the operand fetch of finish is issued there already); the
// token's type tells extra_out / finish what it carries.  Every other System is called through its one eval.
template <int S, class Sys, class P>
__device__ __forceinline__ auto sbm_stage_eval(const Sys& sys, const P& p, double t, int)
    -> decltype(sys.template eval_stage<S>(p, t)) {
  return sys.template eval_stage<S>(p, t);
}
template <int S, class Sys, class P>
__device__ __forceinline__ auto sbm_stage_eval(const Sys& sys, const P& p, double t, long) {
  return sys.eval(p, t);
}
#define SBM_STAGE_THEN_N(s, tt, stmt, kout, next)            \
  {                                                          \
    auto tok_ = sbm_stage_eval<s>(sys, pend_, (tt), 0);      \
    sys.extra_out(tok_, kout);                               \
    next                                                     \
    SBM_MAIN(c, i) { stmt }                                  \
    sys.finish(tok_, (tt), zt, kout);                        \
  }

// ---------------------------------------------------------------------------
// per-trajectory driver state shared by both integrators
// ---------------------------------------------------------------------------
struct SbmTrajOut {
  int32_t status;
  int32_t n_acc;
  int32_t n_rej;
};

// ---- what every kernel does before and after its trajectory ----
// the trajectory of workgroup / work item `block`: the caller's order (longest first) or the index itself; wave-uniform
template <class I>
__device__ __forceinline__ int sbm_traj_of(const sbm_kernel_args& a, I block) { return a.order ? a.order[block] : (int)block; }
// the trajectory's window of the shared time grid
struct SbmGridWindow {
  const double* t;
  int n;
};
__device__ __forceinline__ SbmGridWindow sbm_grid_window(const sbm_kernel_args& a, int traj) {
  const int goff = a.grid_off ? a.grid_off[traj] : 0;
  const int glen = a.grid_len ? a.grid_len[traj] : a.n_t;
  return SbmGridWindow{a.t_out + goff, glen};
}
// Called by the one lane that reports.  merge: several wavefronts (column chunks) share the trajectory -- worst status,
// most steps over the chunks (all non-negative; zeroed by the launcher).
__device__ __forceinline__ void sbm_report(const sbm_kernel_args& a, int traj, int status, int n_acc, int n_rej, bool merge) {
  if (merge) {
    if (a.status) atomicMax(a.status + traj, status);
    if (a.n_steps) atomicMax(a.n_steps + traj, n_acc);
    if (a.n_reject) atomicMax(a.n_reject + traj, n_rej);
  } else {
    if (a.status) a.status[traj] = status;
    if (a.n_steps) a.n_steps[traj] = n_acc;
    if (a.n_reject) a.n_reject[traj] = n_rej;
  }
}

// Whether sbm_dopri45 folds the step size into the tableau (products hs * a_ij formed per stage, see there): yes,
// except in the per-wave SensSystem of a model whose seven stage vectors do not fit the register file of a wave
// (7 vectors x 2 VGPRs x more than 36 elements per lane > 512; stiff50 has 50).  That kernel keeps its stage
// vectors in scratch as it is, and the compiler's report has MORE scratch instructions in its step loop with the
// products alive (1068) than without (1038), so it keeps the form that scales each finished sum.  The state and
// row-lane kernels of the same model go the other way (1362 -> 1262, 706 -> 543) and fold.
template <class Sys>
inline constexpr bool sbm_fold_step_size = true;

// Dormand-Prince 5(4) with FSAL, I-controller (safety 0.9, factor in [0.2, 10]),
// landing exactly on every output time (the reference samples the solution AT
// grid points, project/utils.py:18-21 -- no dense output, no interpolation).
// `Store` is called as store(io, z) once per output index.
template <class Sys, class Store>
__device__ __forceinline__ SbmTrajOut sbm_dopri45(const Sys& sys, double (&z)[Sys::CPL][Sys::NVX],
                                                   const double* __restrict__ t_out, int n_t,
                                                   const sbm_integrator_opts& o, Store&& store) {
  constexpr int NV = Sys::NV;
  constexpr int NVX = Sys::NVX;
  constexpr int CPL = Sys::CPL;
  using namespace dp;
  const double rtol = o.rtol, atol = o.atol;
  // max_steps < 0: a budget of |max_steps| attempts with an early exit -- a trajectory whose CURRENT step size
  // would need more than one and a half times what is LEFT of the budget for the rest of the time span gives up at
  // once (round 2: four whole budgets -- a trial point of a fit that was going to miss its budget by less than that
  // ran to the end of it, and one such trajectory sets the duration of the launch; checked every 256
  // attempts from the 512th on, when the controller has settled, and only while the step size has stopped growing
  // from one check to the next).  That is the explicit method on a stiff
  // system, its step size pinned by stability: method='auto' hands such trajectories to the implicit
  // integrator without first burning the whole budget on them.
  const bool early_exit = o.max_steps < 0;
  const int max_steps = o.max_steps > 0 ? o.max_steps : (o.max_steps < 0 ? -o.max_steps : 1000000);

  double k1[CPL][NVX], k2[CPL][NVX], k3[CPL][NVX], k4[CPL][NVX], k5[CPL][NVX], k6[CPL][NVX], zt[CPL][NVX];
  // defined values everywhere from the start: lanes / elements that carry no equation must hold
  // zeros, never whatever the previous kernel left in the register file
  SBM_ALL(c, i) { k1[c][i] = 0.0; k2[c][i] = 0.0; k3[c][i] = 0.0; k4[c][i] = 0.0; k5[c][i] = 0.0; k6[c][i] = 0.0; zt[c][i] = 0.0; }
  double t = o.t0;
  SbmTrajOut out{SBM_OK, 0, 0};
  if (n_t <= 0) return out;
  const double t_span = t_out[n_t - 1] - o.t0;

  sys.rhs(t, z, k1);

  // ---- initial step (Hairer's hinit) ----
  double h = o.h0;
  if (!(h > 0.0)) {
    double dnf = 0.0, dny = 0.0;
    SBM_ALL(c, i) {
      const double sk = atol + rtol * fabs(z[c][i]);
      const double a = k1[c][i] / sk, b = z[c][i] / sk;
      dnf = fma(a, a, dnf);
      dny = fma(b, b, dny);
    }
    dnf = sys.sum(dnf);
    dny = sys.sum(dny);
    h = (dnf <= 1e-10 || dny <= 1e-10) ? 1e-6 : sqrt(dny / dnf) * 0.01;
    h = fmin(h, t_span > 0.0 ? t_span : 1.0);
    SBM_ALL(c, i) zt[c][i] = fma(h, k1[c][i], z[c][i]);
    sys.rhs(t + h, zt, k2);
    double der2 = 0.0;
    SBM_ALL(c, i) {
      const double sk = atol + rtol * fabs(z[c][i]);
      const double a = (k2[c][i] - k1[c][i]) / sk;
      der2 = fma(a, a, der2);
    }
    der2 = sqrt(sys.sum(der2)) / h;
    const double der12 = fmax(fabs(der2), sqrt(dnf));
    const double h1 = (der12 <= 1e-15) ? fmax(1e-6, fabs(h) * 1e-3) : pow(0.01 / der12, 0.2);
    h = fmin(fmin(100.0 * h, h1), t_span > 0.0 ? t_span : 1.0);
    if (!(h > 0.0)) h = 1e-6;
  }

  int n_try = 0;
  bool failed = false;
  float h_mark = 0.f;          // step size at the previous early-exit check
  int rej_mark = 0;            // rejected attempts up to the previous check
  typename Sys::Pending pend_;
  for (int io = 0; io < n_t; ++io) {
    const double target = t_out[io];
    while (!failed && t < target) {
      if (n_try >= max_steps) { out.status = SBM_MAX_STEPS; failed = true; break; }
      if (early_exit && n_try >= 512 && (n_try & 255) == 0) {
        // A step size that is still GROWING (by half or more since the previous check) is not one pinned by stability:
        // a run that merely starts with small steps on a long horizon carries on.
        // and a controller that never rejects is limited by accuracy -- the transient of a long run -- not by stability:
        // there the step size sits on the stability boundary and about one attempt in 40 overshoots it (measured:
        // stiff50 497 rejections in 20 000 attempts, cascade20 beyond its transient 2.5 %, within it 0 of 978).
        const bool growing = (float)h > 1.5f * h_mark;
        const bool smooth = out.n_rej - rej_mark < 3;
        h_mark = (float)h;
        rej_mark = out.n_rej;
        // (the end of the time span is read again here, in the cold path, rather than kept alive across the step loop)
        if (!growing && !smooth && (t_out[n_t - 1] - t) > 1.5 * (double)(max_steps - n_try) * h) { out.status = SBM_MAX_STEPS; failed = true; break; }
      }
      ++n_try;
      // clip to land on the output time
      double hs = h;
      bool last = false;
      if (t + 1.01 * hs >= target) { hs = target - t; last = true; }

      // The step size is folded into the tableau: stage s is formed from the products hs * a_sj as one FMA chain
      // seeded with z, so no sum is opened by a multiply and none is scaled afterwards -- one VALU instruction
      // less per element in each of stages 3-7.  The products are formed from the CLIPPED step size hs, once per
      // attempted step (a rejection comes back through here with its new hs), and each right before the stage
      // that reads it first, NOT at the top of the step: there is no scalar fp64 ALU, so a product is a VGPR pair
      // for as long as it lives, and all 19 of them held for the whole step would be 38 VGPRs of a wave that
      // needs every register for its stage vectors.  Formed per stage they are transient: at most 11 are alive
      // at once (the three chains of stage 5: 22 VGPRs, where 6 of the 7 stage vectors are alive), 2-3 elsewhere.
      // They are wave-uniform: 19 v_mul_f64 per step against 5 instructions per ELEMENT saved.  The tableau
      // entries themselves stay compile-time constants (SGPR literals the compiler can rematerialise at will).
      //
      // Stages 2-4 combine the stored derivatives.  From stage 5 on every remaining linear
      // combination (the inputs of stages 6 and 7 and the error estimate) is carried as a RUNNING SUM
      // instead: when the input of stage 5 is formed, k2 / k3 / k4 are read one last time and their
      // registers take over U6 / U7 (the arguments of stages 6 and 7 short of their last term: z plus the
      // scaled terms known so far) and E (the error sum, unscaled by h: |hs| multiplies its norm once).
      // Each derivative is read once instead of up to four times and the live set peaks at 7 stage vectors
      // instead of 8 (z, k1, zt, U6, U7, E, k5), falling to 5 by stage 7 -- it is the v_accvgpr traffic of an
      // overflowing register file that this saves.
      //
      // kFold == false (the per-wave system of a large model, see sbm_fold_step_size) keeps the
      // earlier form: tableau literals inside the sums, each finished sum scaled by hs with one more FMA.
      constexpr bool kFold = sbm_fold_step_size<Sys>;
      const double ha21 = hs * A21;
      double ha31, ha32, ha41, ha42, ha43, ha51, ha52, ha53, ha54, ha61, ha62, ha63, ha64, ha71, ha73, ha74, ha65, ha75,
          ha76;
#define SBM_S2 zt[c][i] = fma(ha21, k1[c][i], z[c][i]);
#define SBM_S3                                                                                    \
  if constexpr (kFold) zt[c][i] = fma(ha32, k2[c][i], fma(ha31, k1[c][i], z[c][i]));              \
  else zt[c][i] = fma(hs, fma(A32, k2[c][i], A31 * k1[c][i]), z[c][i]);
#define SBM_S4                                                                                               \
  if constexpr (kFold) zt[c][i] = fma(ha43, k3[c][i], fma(ha42, k2[c][i], fma(ha41, k1[c][i], z[c][i])));    \
  else zt[c][i] = fma(hs, fma(A43, k3[c][i], fma(A42, k2[c][i], A41 * k1[c][i])), z[c][i]);
#define SBM_S5                                                                                    \
  const double a1_ = k1[c][i], a2_ = k2[c][i], a3_ = k3[c][i], a4_ = k4[c][i], z_ = z[c][i];      \
  if constexpr (kFold) {                                                                          \
    zt[c][i] = fma(ha54, a4_, fma(ha53, a3_, fma(ha52, a2_, fma(ha51, a1_, z_))));                \
    k2[c][i] = fma(ha64, a4_, fma(ha63, a3_, fma(ha62, a2_, fma(ha61, a1_, z_)))); /* U6 */       \
    k3[c][i] = fma(ha74, a4_, fma(ha73, a3_, fma(ha71, a1_, z_)));                 /* U7 */       \
  } else {                                                                                        \
    zt[c][i] = fma(hs, fma(A54, a4_, fma(A53, a3_, fma(A52, a2_, A51 * a1_))), z_);               \
    k2[c][i] = fma(A64, a4_, fma(A63, a3_, fma(A62, a2_, A61 * a1_)));                            \
    k3[c][i] = fma(A74, a4_, fma(A73, a3_, A71 * a1_));                                           \
  }                                                                                               \
  k4[c][i] = fma(E4, a4_, fma(E3, a3_, E1 * a1_));                                 /* E  */
#define SBM_S6                                                        \
  const double a5_ = k5[c][i];                                        \
  if constexpr (kFold) zt[c][i] = fma(ha65, a5_, k2[c][i]);           \
  else zt[c][i] = fma(hs, fma(A65, a5_, k2[c][i]), z[c][i]);          \
  if constexpr (kFold) k3[c][i] = fma(ha75, a5_, k3[c][i]);           \
  else k3[c][i] = fma(A75, a5_, k3[c][i]);                            \
  k4[c][i] = fma(E5, a5_, k4[c][i]);
#define SBM_S7                                                        \
  const double a6_ = k6[c][i];                                        \
  if constexpr (kFold) zt[c][i] = fma(ha76, a6_, k3[c][i]);           \
  else zt[c][i] = fma(hs, fma(A76, a6_, k3[c][i]), z[c][i]);          \
  k4[c][i] = fma(E6, a6_, k4[c][i]);
#define SBM_P3 if constexpr (kFold) { ha31 = hs * A31; ha32 = hs * A32; }
#define SBM_P4 if constexpr (kFold) { ha41 = hs * A41; ha42 = hs * A42; ha43 = hs * A43; }
#define SBM_P5                                                               \
  if constexpr (kFold) {                                                     \
    ha51 = hs * A51; ha52 = hs * A52; ha53 = hs * A53; ha54 = hs * A54;      \
    ha61 = hs * A61; ha62 = hs * A62; ha63 = hs * A63; ha64 = hs * A64;      \
    ha71 = hs * A71; ha73 = hs * A73; ha74 = hs * A74;                       \
  }
#define SBM_P6 if constexpr (kFold) { ha65 = hs * A65; ha75 = hs * A75; }
#define SBM_P7 if constexpr (kFold) { ha76 = hs * A76; }
      SBM_ISSUE(t + C2 * hs, SBM_S2)
      SBM_STAGE_THEN_N(2, t + C2 * hs, SBM_S2, k2, SBM_P3 SBM_ISSUE(t + C3 * hs, SBM_S3))
      SBM_STAGE_THEN_N(3, t + C3 * hs, SBM_S3, k3, SBM_P4 SBM_ISSUE(t + C4 * hs, SBM_S4))
      SBM_STAGE_THEN_N(4, t + C4 * hs, SBM_S4, k4, SBM_P5 SBM_ISSUE(t + C5 * hs, SBM_S5))
      SBM_STAGE_THEN_N(5, t + C5 * hs, SBM_S5, k5, SBM_P6 SBM_ISSUE(t + hs, SBM_S6))
      SBM_STAGE_THEN_N(6, t + hs, SBM_S6, k6, SBM_P7 SBM_ISSUE(t + hs, SBM_S7))
      // zt is the 5th-order solution now.  k1 was last read when the input of stage 5 was formed, so
      // k7 = f(z_new) goes straight into it: an accepted step continues with it (FSAL, no copy), a
      // rejected one -- rare -- re-evaluates f(z).  One stage vector fewer alive through stages 5-7.
      SBM_STAGE_THEN_N(7, t + hs, SBM_S7, k1, )
#undef SBM_S2
#undef SBM_S3
#undef SBM_S4
#undef SBM_S5
#undef SBM_S6
#undef SBM_S7
#undef SBM_P3
#undef SBM_P4
#undef SBM_P5
#undef SBM_P6
#undef SBM_P7

      // embedded error estimate h (E + e7 k7); ratios and norm in f32 (they only steer the controller).
      // The norm is homogeneous: |h| multiplies it once at the end instead of every element.
      // one sum of squares per column a lane holds (a lane of the row-group system holds the
      // rows of several columns next to each other inside one array: Sys::col_of maps them)
      float colsum[Sys::NCS];
#pragma unroll
      for (int c = 0; c < Sys::NCS; ++c) colsum[c] = 0.f;
      float xsum = 0.f;
      auto err_ratio = [&](int c, int i) {
        const double e = fma(E7, k1[c][i], k4[c][i]);
        const double sc = fma(rtol, sbm_max_abs(z[c][i], zt[c][i]), atol);
        return (float)e * __builtin_amdgcn_rcpf((float)sc);
      };
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const float r = err_ratio(c, i);
          colsum[Sys::col_of(c, i)] = fmaf(r, r, colsum[Sys::col_of(c, i)]);
        }
#pragma unroll
        for (int i = NV; i < NVX; ++i) {
          const float r = err_ratio(c, i);
          xsum = fmaf(r, r, xsum);
        }
      }
      const float err = fabsf((float)hs) * sys.norm(colsum, xsum);

      const bool finite = (err == err) && (err < 3.0e38f);
      const bool accept = finite && (err <= 1.0f);
      float fac;
      if (!finite) {
        fac = 0.2f;
      } else {
        // 0.9 * err^(-1/5), clipped
        fac = 0.9f * __builtin_amdgcn_exp2f(-0.2f * __builtin_amdgcn_logf(fmaxf(err, 1e-30f)));
        fac = fminf(10.f, fmaxf(0.2f, fac));
      }
      if (accept) {
        ++out.n_acc;
        t = last ? target : t + hs;
        SBM_ALL(c, i) z[c][i] = zt[c][i];
        const double hn = hs * (double)fac;
        // a step clipped to hit an output time says nothing against the unclipped proposal
        h = last ? fmax(hn, h) : hn;
      } else {
        ++out.n_rej;
        h = hs * (double)fminf(fac, 1.0f);
        if (!(h > 1e-14 * fmax(fabs(t), 1e-3))) {
          out.status = finite ? SBM_STEP_UNDERFLOW : SBM_NON_FINITE;
          failed = true;
        } else {
          sys.rhs(t, z, k1);   // k1 holds f(z_new) of the rejected attempt
        }
      }
    }
    if (failed) {
      SBM_ALL(c, i) z[c][i] = __builtin_nan("");
    }
    store(io, z);
  }
  return out;
}

// Dormand-Prince 8(5,3) (DOP853), for tight tolerances: twelve stages per step instead of six, one seventh of the
// steps at rtol 1e-9 (cascade20 with sensitivities: 123 steps where DOPRI45 takes 843 -- 3.4 times fewer evaluations
// of the right-hand side).  Same driver contract as sbm_dopri45: lands on every output time, error control on state and
// sensitivities with the system's norm, step budget with early exit.  Ten stage vectors are alive at the peak (k2's
// storage is taken over by k4, k3's by k6: the tableau never reads them later), with the state and the stage argument
// that is twelve vectors of a lane's elements -- the kernels give this method the whole register file (one wave per
// SIMD).  Error estimate and controller as in Hairer's code: err = |h| e5^2 / sqrt(e5^2 + 0.01 e3^2) with e5, e3 the
// norms of the fifth- and third-order embedded estimates, new step = h * min(6, max(1/3, 0.9 err^(-1/8))).
// f(y_new) is evaluated after acceptance only (it is the next step's k1).
template <class Sys, class Store>
__device__ __forceinline__ SbmTrajOut sbm_dop853(const Sys& sys, double (&z)[Sys::CPL][Sys::NVX],
                                                  const double* __restrict__ t_out, int n_t,
                                                  const sbm_integrator_opts& o, Store&& store) {
  constexpr int NV = Sys::NV;
  constexpr int NVX = Sys::NVX;
  constexpr int CPL = Sys::CPL;
  using namespace dp8;
  const double rtol = o.rtol, atol = o.atol;
  const bool early_exit = o.max_steps < 0;
  const int max_steps = o.max_steps > 0 ? o.max_steps : (o.max_steps < 0 ? -o.max_steps : 1000000);

  double k1[CPL][NVX], kx[CPL][NVX], ky[CPL][NVX], k5[CPL][NVX], k7[CPL][NVX], k8[CPL][NVX], k9[CPL][NVX],
      k10[CPL][NVX], k11[CPL][NVX], k12[CPL][NVX], zt[CPL][NVX];
  SBM_ALL(c, i) {
    k1[c][i] = 0.0; kx[c][i] = 0.0; ky[c][i] = 0.0; k5[c][i] = 0.0; k7[c][i] = 0.0; k8[c][i] = 0.0; k9[c][i] = 0.0;
    k10[c][i] = 0.0; k11[c][i] = 0.0; k12[c][i] = 0.0; zt[c][i] = 0.0;
  }
  double t = o.t0;
  SbmTrajOut out{SBM_OK, 0, 0};
  if (n_t <= 0) return out;
  const double t_span = t_out[n_t - 1] - o.t0;

  sys.rhs(t, z, k1);

  // ---- initial step (Hairer's hinit, order 8) ----
  double h = o.h0;
  if (!(h > 0.0)) {
    double dnf = 0.0, dny = 0.0;
    SBM_ALL(c, i) {
      const double sk = atol + rtol * fabs(z[c][i]);
      const double a = k1[c][i] / sk, b = z[c][i] / sk;
      dnf = fma(a, a, dnf);
      dny = fma(b, b, dny);
    }
    dnf = sys.sum(dnf);
    dny = sys.sum(dny);
    h = (dnf <= 1e-10 || dny <= 1e-10) ? 1e-6 : sqrt(dny / dnf) * 0.01;
    h = fmin(h, t_span > 0.0 ? t_span : 1.0);
    SBM_ALL(c, i) zt[c][i] = fma(h, k1[c][i], z[c][i]);
    sys.rhs(t + h, zt, kx);
    double der2 = 0.0;
    SBM_ALL(c, i) {
      const double sk = atol + rtol * fabs(z[c][i]);
      const double a = (kx[c][i] - k1[c][i]) / sk;
      der2 = fma(a, a, der2);
    }
    der2 = sqrt(sys.sum(der2)) / h;
    const double der12 = fmax(fabs(der2), sqrt(dnf));
    const double h1 = (der12 <= 1e-15) ? fmax(1e-6, fabs(h) * 1e-3) : pow(0.01 / der12, 0.125);
    h = fmin(fmin(100.0 * h, h1), t_span > 0.0 ? t_span : 1.0);
    if (!(h > 0.0)) h = 1e-6;
  }

  int n_try = 0;
  bool failed = false;
  float h_mark = 0.f;
  int rej_mark = 0;
  typename Sys::Pending pend_;
  for (int io = 0; io < n_t; ++io) {
    const double target = t_out[io];
    while (!failed && t < target) {
      if (n_try >= max_steps) { out.status = SBM_MAX_STEPS; failed = true; break; }
      if (early_exit && n_try >= 512 && (n_try & 255) == 0) {      // (see sbm_dopri45)
        const bool growing = (float)h > 1.5f * h_mark;
        const bool smooth = out.n_rej - rej_mark < 3;
        h_mark = (float)h;
        rej_mark = out.n_rej;
        if (!growing && !smooth && (t_out[n_t - 1] - t) > 1.5 * (double)(max_steps - n_try) * h) { out.status = SBM_MAX_STEPS; failed = true; break; }
      }
      ++n_try;
      double hs = h;
      bool last = false;
      if (t + 1.01 * hs >= target) { hs = target - t; last = true; }

      // The step size multiplies each finished sum once (tableau entries stay literals, as in sbm_dopri45).  Stages are
      // software-pipelined as there: stage s+1's state path (extra elements, LDS hand-off, operand fetch) is issued
      // between the row evaluation and the column work of stage s.
      const double ha21 = hs * A2_1;
#define SBM_D2 zt[c][i] = fma(ha21, k1[c][i], z[c][i]);
#define SBM_D3 zt[c][i] = fma(hs, fma(A3_2, kx[c][i], A3_1 * k1[c][i]), z[c][i]);
#define SBM_D4 zt[c][i] = fma(hs, fma(A4_3, ky[c][i], A4_1 * k1[c][i]), z[c][i]);
#define SBM_D5 zt[c][i] = fma(hs, fma(A5_4, kx[c][i], fma(A5_3, ky[c][i], A5_1 * k1[c][i])), z[c][i]);
#define SBM_D6 zt[c][i] = fma(hs, fma(A6_5, k5[c][i], fma(A6_4, kx[c][i], A6_1 * k1[c][i])), z[c][i]);
#define SBM_D7 zt[c][i] = fma(hs, fma(A7_6, ky[c][i], fma(A7_5, k5[c][i], fma(A7_4, kx[c][i], A7_1 * k1[c][i]))), z[c][i]);
#define SBM_D8                                                                                                      \
  zt[c][i] = fma(hs, fma(A8_7, k7[c][i], fma(A8_6, ky[c][i], fma(A8_5, k5[c][i], fma(A8_4, kx[c][i], A8_1 * k1[c][i])))), \
                 z[c][i]);
#define SBM_D9                                                                                                      \
  zt[c][i] = fma(hs, fma(A9_8, k8[c][i], fma(A9_7, k7[c][i], fma(A9_6, ky[c][i], fma(A9_5, k5[c][i],                 \
                 fma(A9_4, kx[c][i], A9_1 * k1[c][i]))))), z[c][i]);
#define SBM_D10                                                                                                     \
  zt[c][i] = fma(hs, fma(A10_9, k9[c][i], fma(A10_8, k8[c][i], fma(A10_7, k7[c][i], fma(A10_6, ky[c][i],             \
                 fma(A10_5, k5[c][i], fma(A10_4, kx[c][i], A10_1 * k1[c][i])))))), z[c][i]);
#define SBM_D11                                                                                                     \
  zt[c][i] = fma(hs, fma(A11_10, k10[c][i], fma(A11_9, k9[c][i], fma(A11_8, k8[c][i], fma(A11_7, k7[c][i],           \
                 fma(A11_6, ky[c][i], fma(A11_5, k5[c][i], fma(A11_4, kx[c][i], A11_1 * k1[c][i]))))))), z[c][i]);
#define SBM_D12                                                                                                     \
  zt[c][i] = fma(hs, fma(A12_11, k11[c][i], fma(A12_10, k10[c][i], fma(A12_9, k9[c][i], fma(A12_8, k8[c][i],         \
                 fma(A12_7, k7[c][i], fma(A12_6, ky[c][i], fma(A12_5, k5[c][i], fma(A12_4, kx[c][i],                 \
                 A12_1 * k1[c][i])))))))), z[c][i]);
      SBM_ISSUE(t + C2 * hs, SBM_D2)
      SBM_STAGE_THEN(t + C2 * hs, SBM_D2, kx, SBM_ISSUE(t + C3 * hs, SBM_D3))       // k2
      SBM_STAGE_THEN(t + C3 * hs, SBM_D3, ky, SBM_ISSUE(t + C4 * hs, SBM_D4))       // k3
      SBM_STAGE_THEN(t + C4 * hs, SBM_D4, kx, SBM_ISSUE(t + C5 * hs, SBM_D5))       // k4 takes k2's storage
      SBM_STAGE_THEN(t + C5 * hs, SBM_D5, k5, SBM_ISSUE(t + C6 * hs, SBM_D6))
      SBM_STAGE_THEN(t + C6 * hs, SBM_D6, ky, SBM_ISSUE(t + C7 * hs, SBM_D7))       // k6 takes k3's storage
      SBM_STAGE_THEN(t + C7 * hs, SBM_D7, k7, SBM_ISSUE(t + C8 * hs, SBM_D8))
      SBM_STAGE_THEN(t + C8 * hs, SBM_D8, k8, SBM_ISSUE(t + C9 * hs, SBM_D9))
      SBM_STAGE_THEN(t + C9 * hs, SBM_D9, k9, SBM_ISSUE(t + C10 * hs, SBM_D10))
      SBM_STAGE_THEN(t + C10 * hs, SBM_D10, k10, SBM_ISSUE(t + C11 * hs, SBM_D11))
      SBM_STAGE_THEN(t + C11 * hs, SBM_D11, k11, SBM_ISSUE(t + hs, SBM_D12))
      SBM_STAGE_THEN(t + hs, SBM_D12, k12, )
#undef SBM_D2
#undef SBM_D3
#undef SBM_D4
#undef SBM_D5
#undef SBM_D6
#undef SBM_D7
#undef SBM_D8
#undef SBM_D9
#undef SBM_D10
#undef SBM_D11
#undef SBM_D12

      // 8th-order solution into zt; the two error estimates, ratios and norms in f32 (they only steer the controller)
      float cs5[Sys::NCS], cs3[Sys::NCS];
#pragma unroll
      for (int c = 0; c < Sys::NCS; ++c) { cs5[c] = 0.f; cs3[c] = 0.f; }
      float xs5 = 0.f, xs3 = 0.f;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
#pragma unroll
        for (int i = 0; i < NVX; ++i) {
          const double a1 = k1[c][i], a6 = ky[c][i], a7 = k7[c][i], a8 = k8[c][i], a9 = k9[c][i], a10 = k10[c][i],
                       a11 = k11[c][i], a12 = k12[c][i];
          const double zn = fma(hs, fma(B12, a12, fma(B11, a11, fma(B10, a10, fma(B9, a9, fma(B8, a8, fma(B7, a7,
                                fma(B6, a6, B1 * a1))))))), z[c][i]);
          const double e5 = fma(E5_12, a12, fma(E5_11, a11, fma(E5_10, a10, fma(E5_9, a9, fma(E5_8, a8, fma(E5_7, a7,
                                fma(E5_6, a6, E5_1 * a1)))))));
          const double e3 = fma(E3_12, a12, fma(E3_11, a11, fma(E3_10, a10, fma(E3_9, a9, fma(E3_8, a8, fma(E3_7, a7,
                                fma(E3_6, a6, E3_1 * a1)))))));
          const float rsc = __builtin_amdgcn_rcpf((float)fma(rtol, fmax(fabs(z[c][i]), fabs(zn)), atol));
          const float r5 = (float)e5 * rsc, r3 = (float)e3 * rsc;
          zt[c][i] = zn;
          if (i < NV) {
            cs5[Sys::col_of(c, i)] = fmaf(r5, r5, cs5[Sys::col_of(c, i)]);
            cs3[Sys::col_of(c, i)] = fmaf(r3, r3, cs3[Sys::col_of(c, i)]);
          } else {
            xs5 = fmaf(r5, r5, xs5);
            xs3 = fmaf(r3, r3, xs3);
          }
        }
      }
      const float n5 = sys.norm(cs5, xs5), n3 = sys.norm(cs3, xs3);
      const float den = n5 * n5 + 0.01f * n3 * n3;
      const float err = fabsf((float)hs) * (den > 0.f ? n5 * n5 * __builtin_amdgcn_rsqf(den) : 0.f);

      const bool finite = (err == err) && (err < 3.0e38f) && (n3 == n3) && (n3 < 3.0e38f);
      const bool accept = finite && (err <= 1.0f);
      float fac;
      if (!finite) {
        fac = 1.0f / 3.0f;
      } else {
        fac = 0.9f * __builtin_amdgcn_exp2f(-0.125f * __builtin_amdgcn_logf(fmaxf(err, 1e-30f)));   // 0.9 err^(-1/8)
        fac = fminf(6.f, fmaxf(1.0f / 3.0f, fac));
      }
      if (accept) {
        ++out.n_acc;
        t = last ? target : t + hs;
        SBM_ALL(c, i) z[c][i] = zt[c][i];
        sys.rhs(t, z, k1);                       // FSAL: f(y_new) is the next step's k1
        const double hn = hs * (double)fac;
        h = last ? fmax(hn, h) : hn;
      } else {
        ++out.n_rej;
        h = hs * (double)fminf(fac, 1.0f);
        if (!(h > 1e-14 * fmax(fabs(t), 1e-3))) {
          out.status = finite ? SBM_STEP_UNDERFLOW : SBM_NON_FINITE;
          failed = true;
        }
      }
    }
    if (failed) {
      SBM_ALL(c, i) z[c][i] = __builtin_nan("");
    }
    store(io, z);
  }
  return out;
}

// one entry for the kernels: the driver of METHOD
template <int METHOD, class Sys, class Store>
__device__ __forceinline__ SbmTrajOut sbm_integrate(const Sys& sys, double (&z)[Sys::CPL][Sys::NVX],
                                                     const double* __restrict__ t_out, int n_t,
                                                     const sbm_integrator_opts& o, Store&& store) {
  if constexpr (METHOD == SBM_DOPRI45) return sbm_dopri45(sys, z, t_out, n_t, o, store);
  else if constexpr (METHOD == SBM_DOP853) return sbm_dop853(sys, z, t_out, n_t, o, store);
  else return sbm_rk4(sys, z, t_out, n_t, o, store);
}

// classic RK4, fixed step: every output interval is cut into ceil(dt / h0) equal steps
template <class Sys, class Store>
__device__ __forceinline__ SbmTrajOut sbm_rk4(const Sys& sys, double (&z)[Sys::CPL][Sys::NVX],
                                               const double* __restrict__ t_out, int n_t,
                                               const sbm_integrator_opts& o, Store&& store) {
  constexpr int NV = Sys::NV;
  constexpr int NVX = Sys::NVX;
  constexpr int CPL = Sys::CPL;
  double k[CPL][NVX], acc[CPL][NVX], zt[CPL][NVX];
  SBM_ALL(c, i) { k[c][i] = 0.0; acc[c][i] = 0.0; zt[c][i] = 0.0; }
  typename Sys::Pending pend_;
  SbmTrajOut out{SBM_OK, 0, 0};
  const double h0 = o.h0;
  const int max_steps = o.max_steps > 0 ? o.max_steps : 1000000000;
  double t = o.t0;
  bool failed = !(h0 > 0.0);
  if (failed) out.status = SBM_STEP_UNDERFLOW;
  for (int io = 0; io < n_t; ++io) {
    const double target = t_out[io];
    const double dt = target - t;
    if (!failed && dt > 0.0) {
      const double nd = ceil(dt / h0 - 1e-9) * (o.step_mult > 0 ? o.step_mult : 1);
      int ns = nd < 1.0 ? 1 : (nd > 2.0e9 ? 2000000000 : (int)nd);
      if (out.n_acc + ns > max_steps) { out.status = SBM_MAX_STEPS; failed = true; }
      if (!failed) {
        const double hs = dt / ns, hh = 0.5 * hs, h6 = hs * (1.0 / 6.0);
        const double t0 = t;
        for (int s = 0; s < ns; ++s) {
          const double ts = fma((double)s, hs, t0);
          sys.rhs(ts, z, k);
          SBM_ALL(c, i) acc[c][i] = k[c][i];
          SBM_STAGE(ts + hh, zt[c][i] = fma(hh, k[c][i], z[c][i]);, k)
          SBM_ALL(c, i) acc[c][i] = fma(2.0, k[c][i], acc[c][i]);
          SBM_STAGE(ts + hh, zt[c][i] = fma(hh, k[c][i], z[c][i]);, k)
          SBM_ALL(c, i) acc[c][i] = fma(2.0, k[c][i], acc[c][i]);
          SBM_STAGE(ts + hs, zt[c][i] = fma(hs, k[c][i], z[c][i]);, k)
          SBM_ALL(c, i) z[c][i] = fma(h6, acc[c][i] + k[c][i], z[c][i]);
        }
        out.n_acc += ns;
        t = target;
      }
    }
    if (failed) {
      SBM_ALL(c, i) z[c][i] = __builtin_nan("");
    }
    store(io, z);
  }
  // RK4 has no error estimate: flag non-finite end states
  bool bad = false;
  SBM_ALL(c, i) bad = bad || !(z[c][i] == z[c][i]);
  if (!failed && bad) out.status = SBM_NON_FINITE;
  return out;
}
