// sbm_lm_geodesic.hpp -- the geodesic acceleration of the trust-region step (include/sbm.h: sbm_lm_geodesic), the second-order
// correction of Transtrum and Sethna ("Improvements to the Levenberg-Marquardt algorithm", 2012) for all starts in one
// launch.  The builder of the normal equations, the list of free columns and the factorisation are sbm_lm.hpp's; the host
// wrapper with the argument checks is in sbm_core.hip.
#ifndef SBM_LM_GEODESIC_HPP
#define SBM_LM_GEODESIC_HPP

#include "sbm_lm.hpp"

// ---------------------------------------------------------------------------------------------
// The step v that sbm_lm_trust_step_ex / _held just produced is taken as a velocity.  The second directional derivative of
// the residuals along it comes from one more residual evaluation (no second-order sensitivities),
//     r_vv = (2 / h) ((r(theta + h v) - r(theta)) / h - J v),
// the damped system the step came from is solved once more,
//     (J^T J + lambda D^2) a = -J^T r_vv,
// and the step becomes v + a / 2 where the acceleration is small beside the velocity: 2 ||D a|| / ||D v|| <= alpha.
// One 256-thread block per vector and one pass over J: the row tiles staged in LDS give J^T J, g = J^T r, (J v)_m, r_vv and
// J^T r_vv together (lm_normal_equations<., true>); one Cholesky factorisation; the quantities of the step TAKEN from the
// triangle in registers, as sbm_lm_trust_step_ex reports them for a clipped step.  Wherever the acceleration is not applied
// nothing but accel_status and ratio_out is written.
// ---------------------------------------------------------------------------------------------
struct LmGeodesicArgs {
  const double* J;              // [V][M][q]
  const double* r;              // [V][M]
  const double* r_base;         // [V][M]  residuals at theta from the probe's integration (nullable: r)
  const double* r_probe;        // [V][M]  residuals at theta + h delta
  const int32_t* status_base;   // [V]     nullable: integration status of the two ends of the difference
  const int32_t* status_probe;  // [V]     nullable
  const double* dscale;         // [V][q]  D as the trust step left it
  const double* lambda;         // [V]     the parameter the trust step found
  const double* row_scale;      // [M]     nullable
  const int32_t* skip;          // [V]     nullable
  const int32_t* step_status;   // [V]     the trust step's status
  const double* theta;          // [V][q]
  double* delta;                // [V][q]  in: v, out: v + a / 2 (clipped)      -- these five only where accel_status = 0
  double* trial;                // [V][q]  theta + delta
  double* pred;                 // [V]
  double* dxnorm;               // [V]
  double* gtx;                  // [V]
  int32_t* accel_status;        // [V]     out, always
  double* ratio_out;            // [V]     nullable: 2 ||D a|| / ||D v|| where it was computed, NaN elsewhere
  int32_t* n_accel;             // [V]     nullable: += 1 where accel_status = 0
  double h, alpha, max_step;
  int M, q, tile;
};

enum : int32_t { LM_GEO_APPLIED = 0, LM_GEO_NO_STEP = 1, LM_GEO_PROBE = 2, LM_GEO_SYSTEM = 3, LM_GEO_GATE = 4, LM_GEO_NO_DESCENT = 5 };

// Static LDS of the kernel (the list of free columns and the waves' counts, the staged rows' r_vv, the two flags, the
// reduction's four doubles: 576 bytes and their alignment), which the host wrapper takes off the limit it chooses the row
// tile for.
constexpr int LM_GEO_STATIC_LDS = 1024;

// HELD as in lm_trust_body: the free columns are compacted and the kernel is the HELD = false kernel on the q x q problem;
// the columns that are not free are neither read nor written (a = 0 there).
template <bool HELD>
__global__ void __launch_bounds__(256) k_lm_geodesic(LmGeodesicArgs a, const int32_t* held) {
  extern __shared__ __attribute__((aligned(16))) double lm_smem[];
  const int v = blockIdx.x, tid = threadIdx.x, qf = a.q, M = a.M, TILE = a.tile;
  const double nan = __builtin_nan("");
  auto not_applied = [&](int32_t status, double rho) {
    if (tid == 0) { a.accel_status[v] = status; if (a.ratio_out) a.ratio_out[v] = rho; }
  };
  // (uniform: per-vector values)
  if ((a.skip && a.skip[v]) || a.step_status[v] != 0) { not_applied(LM_GEO_NO_STEP, nan); return; }
  if ((a.status_base && a.status_base[v] != 0) || (a.status_probe && a.status_probe[v] != 0)) { not_applied(LM_GEO_PROBE, nan); return; }
  int q = qf;
  [[maybe_unused]] const short* idx = nullptr;
  __shared__ short s_idx[LM_MAX_Q];
  __shared__ int s_cnt[4];
  if constexpr (HELD) {
    q = lm_free_columns(tid < qf && held[(size_t)v * qf + tid] == 0, s_idx, s_cnt, tid);
    if (q == 0) { not_applied(LM_GEO_NO_STEP, nan); return; }
    __syncthreads();
    idx = s_idx;
  }
  auto col = [&](int c) -> int { if constexpr (HELD) return idx[c]; else return c; };
  const int ld = q + 1;
  double* A = lm_smem;                       // [q][ld]  the damped matrix / its Cholesky factor
  double* D = A + (size_t)q * ld;            // [q]      scaling
  double* g = D + q;                         // [q]      J^T r
  double* vv = g + q;                        // [q]      the trust step
  double* x = vv + q;                        // [q]      -J^T r_vv, the acceleration, then the step taken
  double* T = x + q;                         // [TILE][ld] row tile of J
  double* rt = T + (size_t)TILE * ld;        // [TILE]
  __shared__ double s_rvv[LM_TILE];
  __shared__ int s_bad, s_bad_probe;
  __shared__ double s_red[4];
  if (tid == 0) { s_bad = 0; s_bad_probe = 0; }
  if (tid < q) {
    vv[tid] = a.delta[(size_t)v * qf + col(tid)];
    D[tid] = a.dscale[(size_t)v * qf + col(tid)];
  }
  LmTriangle n;
  int n_own;
  double gacc;
  const double* rv = a.r + (size_t)v * M;
  LmSecondRhs second{vv, a.r_base ? a.r_base + (size_t)v * M : rv, a.r_probe + (size_t)v * M, s_rvv, &s_bad_probe, a.h, 0.0};
  lm_normal_equations<HELD, true>(n, n_own, gacc, a.J + (size_t)v * M * qf, rv, a.row_scale, M, q, TILE, T, rt, &s_bad, tid, qf, idx,
                                  &second);
  if (s_bad_probe != 0) { not_applied(LM_GEO_PROBE, nan); return; }
  const double lam = a.lambda[v];
  // the matrix the step came from, formed as lm_trust_body's solve_with forms it
  if (s_bad != 0 || !(lam >= 0.0)) { not_applied(LM_GEO_SYSTEM, nan); return; }
  for (int k = 0; k < n_own; ++k) {
    const int i = n.oi[k], j = n.oj[k];
    A[i * ld + j] = (i == j) ? fma(lam * D[i], D[i], n.acc[k]) : n.acc[k];
  }
  if (tid < q) { g[tid] = gacc; x[tid] = -second.acc; }
  __syncthreads();
  if (!lm_cholesky(A, q, ld, tid)) { not_applied(LM_GEO_SYSTEM, nan); return; }
  lm_forward(A, x, q, ld, tid);
  lm_backward(A, x, q, ld, tid);
  // the gate: the acceleration beside the velocity, in the trust region's norm
  double pa = 0.0, pv = 0.0;
  if (tid < q) { const double ta = D[tid] * x[tid], tv = D[tid] * vv[tid]; pa = ta * ta; pv = tv * tv; }
  const double dan = sqrt(block_sum(pa, s_red));
  const double dvn = sqrt(block_sum(pv, s_red));
  const double rho = 2.0 * dan / dvn;
  if (!(dan > 0.0) || !(rho <= a.alpha)) { not_applied(LM_GEO_GATE, rho); return; }
  // the step taken and its quantities, as the trust step's clipped branch reports them
  double xs = 0.0;
  if (tid < q) {
    xs = vv[tid] + 0.5 * x[tid];
    if (a.max_step > 0.0 && fabs(xs) > a.max_step) xs = copysign(a.max_step, xs);
  }
  if (tid < q) x[tid] = xs;                            // (x[tid] is read by its own thread alone until here)
  __syncthreads();
  const double gtx = block_sum(tid < q ? g[tid] * xs : 0.0, s_red);
  double p2 = 0.0;
  if (tid < q) { const double t = D[tid] * xs; p2 = t * t; }
  const double dxn = sqrt(block_sum(p2, s_red));
  double xhx = 0.0;                                    // x^T (J^T J) x from the lower triangle in registers
  for (int k = 0; k < n_own; ++k) xhx += (n.oi[k] == n.oj[k] ? 1.0 : 2.0) * n.acc[k] * x[n.oi[k]] * x[n.oj[k]];
  const double tot = -gtx - 0.5 * block_sum(xhx, s_red);
  if (!(gtx < 0.0 && tot > 0.0)) { not_applied(LM_GEO_NO_DESCENT, rho); return; }
  if (tid < q) {
    a.delta[(size_t)v * qf + col(tid)] = xs;
    a.trial[(size_t)v * qf + col(tid)] = a.theta[(size_t)v * qf + col(tid)] + xs;
  }
  if (tid == 0) {
    a.pred[v] = tot; a.dxnorm[v] = dxn; a.gtx[v] = gtx;
    a.accel_status[v] = LM_GEO_APPLIED;
    if (a.ratio_out) a.ratio_out[v] = rho;
    if (a.n_accel) a.n_accel[v] = a.n_accel[v] + 1;
  }
}

#endif  // SBM_LM_GEODESIC_HPP
