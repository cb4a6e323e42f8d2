// sbm_implicit_midpoint.hpp -- sbm_imid_kernel: implicit midpoint, fixed step, on SbmImplicitStepper.
#pragma once
// ===========================================================================
// Implicit midpoint for stiff systems (BASELINE configs[4]), state + forward sensitivities, FIXED step.
//
// The step itself (Newton on the midpoint, one linear solve per sensitivity column with the factored Newton matrix,
// the lane mapping, models with more than 64 state variables) is sbm_implicit_stepper.hpp.  A-stable and symmetric
// (second order, error expansion in h^2: the caller extrapolates two runs, or uses SBM_IMPLICIT_ADAPTIVE, which does
// that inside the kernel).  Fixed step h0 between output times like RK4; opts.rtol / atol are the Newton tolerances.
// More than 64 columns: blockIdx.y = chunk of 64 columns, each wavefront repeating the (identical, fixed-step)
// state iteration for its own columns; chunk 0 stores the state.
// ===========================================================================
#include "sbm_implicit_stepper.hpp"

template <class M>
struct SbmImidShared {
  // J_p reaches the columns through a compact per-row table (RL_MAXJP values, picked by column index) when rows have few
  // parameter entries -- round 2 kept the dense [row][64] image here (25.6 KB for 50 rows: five wavefronts per CU); with
  // the compact table and the fused Newton update (256 VGPRs) two wavefronts share a SIMD
  static constexpr bool A_SPARSE = (M::RL_MAXJP <= 4);
  static constexpr int NROW = 64 * ((M::NV + 63) / 64);
  static constexpr int A_SIZE = A_SPARSE ? (M::NV * M::RL_MAXJP + 2) : (M::NV * 64 + 2);
  double Y[NROW];               // iterate, one component per row lane (rows lane, lane + 64, ...)
  double G[NROW];               // Newton residual
  double JY[sbm_ijy_size<M>()]; // J_y non-zeros by entry index (+ spare slot): the redundant factorisation's input only
  double A[A_SIZE];             // A[i][c] = J_p[i][c] (+ spare slot)
  static constexpr int MF_SIZE = sbm_imf_size<M>(), RD_SIZE = sbm_ird_size<M>();
  __attribute__((aligned(16))) double MF[MF_SIZE];   // the factors (IM_TRI: reciprocal pivots and scaled entries; IM_DIST: dense rows)
  double RD[RD_SIZE];           // IM_DIST: reciprocal pivots
};

template <class M>
__global__ void __launch_bounds__(64) sbm_imid_kernel(sbm_kernel_args a) {
  constexpr int NV = M::NV, NK = M::NK;
  constexpr int NCH = (NK + 63) / 64;
  using Stepper = SbmImplicitStepper<M, SbmImidShared<M>>;
  constexpr int RPL = Stepper::RPL;
  __shared__ SbmImidShared<M> sh;
  if ((int)blockIdx.x >= a.n_traj) return;
  const int traj = sbm_traj_of(a, blockIdx.x);
  const int lane = threadIdx.x;
  const int chunk = NCH > 1 ? (int)blockIdx.y : 0;
  const int col = lane + 64 * chunk;       // this lane's column of S
  const bool has_col = col < NK;
  Stepper st;
  st.setup(&sh, lane, chunk, a.P + (size_t)traj * M::NP);
  __syncthreads();

  const auto [tg, glen] = sbm_grid_window(a, traj);
  const bool with_sens = a.S != nullptr;   // wave-uniform
  const bool graded = a.opts.method == SBM_IMPLICIT_MIDPOINT_GRADED;

  double z[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) z[i] = (a.s0 && has_col) ? a.s0[i * NK + col] : 0.0;
  double y[RPL], dy_prev[RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    y[r] = (a.y0 && st.has_row[r]) ? a.y0[lane + 64 * r] : 0.0;
    dy_prev[r] = 0.0;        // increment of the previous step (this lane's components)
  }

  double* Yt = a.Y ? a.Y + (size_t)traj * a.n_t * NV : nullptr;
  double* St = a.S ? a.S + (size_t)traj * a.n_t * NV * NK : nullptr;
  const double rtol = a.opts.rtol > 0.0 ? a.opts.rtol : 1e-10, atol = a.opts.atol > 0.0 ? a.opts.atol : 1e-12;
  const double h0 = a.opts.h0;
  const int max_steps = a.opts.max_steps > 0 ? a.opts.max_steps : 1000000000;
  int status = SBM_OK, n_acc = 0, n_newton = 0;
  double t = a.opts.t0;
  bool failed = !(h0 > 0.0);
  if (failed) status = SBM_STEP_UNDERFLOW;
  double hs_prev = 0.0;      // step size of the previous step

  for (int io = 0; io < glen; ++io) {
    const double target = tg[io];
    const double dt = target - t;
    if (!failed && dt > 0.0) {
      const double nd = ceil(dt / h0 - 1e-9) * (a.opts.step_mult > 0 ? a.opts.step_mult : 1);
      const int ns = nd < 1.0 ? 1 : (nd > 2.0e9 ? 2000000000 : (int)nd);
      if (n_acc + ns > max_steps) { status = SBM_MAX_STEPS; failed = true; }
      if (!failed) {
        const double hs = dt / ns;
        const double t0 = t;
        // Newton starts from the midpoint the previous step's increment predicts (free, and good for the
        // smooth solutions a fixed step resolves): 2.6 -> about 2 iterations per step on stiff50
        const double hsc = (hs_prev > 0.0) ? hs / hs_prev : 0.0;
#pragma unroll
        for (int r = 0; r < RPL; ++r) dy_prev[r] *= hsc;
        hs_prev = hs;
        for (int s = 0; s < ns && !failed; ++s) {
         // SBM_IMPLICIT_MIDPOINT_GRADED: the very first step of a trajectory is cut into GRADE + 1 midpoint
         // substeps of sizes hs * 2^-GRADE, 2^-GRADE, 2^-(GRADE-1), ..., 1/2 (they add up to hs).  An initial
         // condition off a fast manifold -- the reference always starts from y = 0 -- produces a layer far
         // thinner than any affordable fixed step; no one-step method integrates through it accurately
         // without resolving it (a backward-Euler start-up damps the layer but misses its area: measured 60x
         // WORSE than doing nothing).  The geometric grading resolves layers down to hs / 4096 for 12 extra
         // steps.  Richardson needs NESTED grids to keep the h^2 expansion (an irregular first step graded relative
         // to each run's own hs leaves an h^3 term: measured third-order convergence of the extrapolants): the
         // pattern belongs to the first BASE step (step_mult = 1), and a run with step_mult = m cuts every one
         // of its substeps into m equal parts -- m substeps of each size hs * 2^-k, covering the first m steps.
         constexpr int GRADE = 12;
         const int gm_ = a.opts.step_mult > 0 ? a.opts.step_mult : 1;
         const bool grade_now = graded && n_acc == 0;                  // wave-uniform
         const int nsub = grade_now ? (GRADE + 1) * gm_ : 1;
         double t_sub = fma((double)s, hs, t0);
         for (int sub = 0; sub < nsub && !failed; ++sub) {
          const int gj = sub / gm_;                                    // which size of the pattern
          const double hsub = nsub == 1 ? hs : ldexp(hs, -(gj == 0 ? GRADE : GRADE - gj + 1));
          const double hh = 0.5 * hsub;
          const double tm = t_sub + hh;
          t_sub += hsub;
          double yb[RPL];
#pragma unroll
          for (int r = 0; r < RPL; ++r) yb[r] = fma(0.5, dy_prev[r], y[r]);
          const int rc = st.template newton<12>(tm, hh, y, yb, rtol, atol, n_newton);
          if (rc != SBM_OK) { status = rc; failed = true; break; }
          // predictor for the next (sub)step: this increment, rescaled when the next substep is twice as long
          const double psc = (nsub > 1 && gj > 0 && sub % gm_ == gm_ - 1) ? 2.0 : 1.0;
#pragma unroll
          for (int r = 0; r < RPL; ++r) {
            dy_prev[r] = 2.0 * (yb[r] - y[r]) * psc;
            y[r] = fma(2.0, yb[r], -y[r]);
          }
          if (with_sens) st.sens(hh, z);
         }
          if (!failed) {
            // the graded block covered the first gm_ steps of this interval
            n_acc += grade_now ? gm_ : 1;
            if (grade_now) s += gm_ - 1;
          }
        }
        if (!failed) t = target;
      }
    }
    if (failed) {
#pragma unroll
      for (int i = 0; i < NV; ++i) z[i] = __builtin_nan("");
#pragma unroll
      for (int r = 0; r < RPL; ++r) y[r] = __builtin_nan("");
    }
    if (Yt && chunk == 0) {
#pragma unroll
      for (int r = 0; r < RPL; ++r)
        if (st.has_row[r]) Yt[(size_t)io * NV + lane + 64 * r] = y[r];
    }
    if (St && has_col) {
#pragma unroll
      for (int i = 0; i < NV; ++i) St[((size_t)io * NV + i) * NK + col] = z[i];
    }
  }
  if (lane == 0 && chunk == 0) {   // the state iteration, hence status and counts, is the same in every chunk
    if (a.status) a.status[traj] = status;
    if (a.n_steps) a.n_steps[traj] = n_acc;
    if (a.n_reject) a.n_reject[traj] = n_newton - n_acc;   // Newton iterations beyond one per step
  }
}
