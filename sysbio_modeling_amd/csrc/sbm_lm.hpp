// sbm_lm.hpp -- kernels of the fitting loop (include/sbm.h: sbm_lm_step, sbm_lm_trust_step[_ex|_held|_bounded], sbm_lm_update,
// sbm_lm_accept).  The step kernels and the geodesic acceleration (sbm_lm_geodesic.hpp) share the builder of the normal
// equations (lm_normal_equations), the list of free columns (lm_free_columns) and the factorisation (lm_cholesky /
// lm_forward / lm_backward); the host wrappers with the argument checks are in sbm_core.hip.
#ifndef SBM_LM_HPP
#define SBM_LM_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbm_block_reduce.hpp"

constexpr int LM_MAX_Q = 128;  // the q x (q + 1) matrix lives in the LDS of one workgroup
constexpr int LM_TILE = 32;    // rows of J staged per pass (fewer when the q x q matrix leaves less room: lm_lds_bytes)
constexpr int LM_MAXOWN = (LM_MAX_Q * (LM_MAX_Q + 1) / 2 + 255) / 256;   // entries of the lower triangle per thread

// LDS of the normal-equation kernels: the q x (q + 1) matrix, `nvec` vectors of q, a row tile of J with the residuals
// beside it.  The tile shrinks (32, 16, 8 rows) until the total fits `limit`, what the device gives a workgroup; 0 = no fit.
// (The kernels' static LDS -- 48 bytes in k_lm_step, 304 in k_lm_trust -- is not counted: at q = 126 sbm_lm_step asks for
// 163 808 bytes with the 32-row tile, the launch helper's attribute call refuses them, and the call returns a HIP error.)
static inline size_t lm_lds_bytes(int q, int nvec, size_t limit, int* tile_out) {
  const size_t ld = (size_t)q + 1;
  for (int tile = LM_TILE; tile >= 8; tile /= 2) {
    const size_t b = sizeof(double) * ((size_t)q * ld + (size_t)nvec * q + (size_t)tile * ld + tile);
    if (b <= limit) { *tile_out = tile; return b; }
  }
  return 0;
}

// J^T J of one vector, spread over the threads of its block: thread tid owns the entries e = tid, tid + 256, ... of the
// lower triangle, acc[k] being entry (oi[k], oj[k]), oi >= oj.  The arrays are indexed in loops and live in scratch; the
// two scalars that go with them (n_own, and gacc: thread c < q owns g[c] of J^T r) are kept apart, in registers.
struct LmTriangle {
  double acc[LM_MAXOWN];
  int oi[LM_MAXOWN], oj[LM_MAXOWN];
};

// The normal equations of diag(row_scale) J (row_scale nullable) and r, accumulated from row tiles staged in LDS
// (T: [TILE][ld], rt: [TILE]).  *s_bad, in LDS and zeroed by the caller, is set on a non-finite entry; ends on a barrier.
// GATHER: the system is built from the q columns idx[0..q) (in LDS, written before the call) of a J with rows of qs entries
// -- column c of the tile is column idx[c] of J, everything after the staging is the same code on the same numbers.
// SECOND (sbm_lm_geodesic.hpp): a second right-hand side from the same pass, see LmSecondRhs; without it the code is the
// code it was.
struct LmSecondRhs {
  const double* vv;       // [q]    LDS, written before the call: the step v the second derivative is taken along
  const double* r_base;   // [M]    residuals at theta and at theta + h v, from one state-only integration
  const double* r_probe;  // [M]
  double* rvv;            // [TILE] LDS: the staged rows' r_vv = (2 / h) ((r_probe - r_base) / h - (J v)_m)
  int* s_bad;             // LDS, zeroed by the caller: set on a non-finite entry of r_base / r_probe
  double h;
  double acc;             // out: thread c < q owns (J^T r_vv)[c]
};
constexpr int LM_ROW_LANES = 8;   // threads that share one staged row's J v: 256 threads, LM_TILE rows
static_assert(LM_TILE * LM_ROW_LANES <= 256, "one lane group per staged row");

template <bool GATHER = false, bool SECOND = false>
__device__ __forceinline__ void lm_normal_equations(LmTriangle& n, int& n_own, double& gacc, const double* Jv, const double* rv,
                                                    const double* row_scale, int M, int q, int TILE, double* T, double* rt,
                                                    int* s_bad, int tid, int qs = 0, const short* idx = nullptr,
                                                    [[maybe_unused]] LmSecondRhs* second = nullptr) {
  const int ld = q + 1, n_low = q * (q + 1) / 2;
  n_own = 0;
  for (int e = tid; e < n_low; e += 256) {
    // row i with i(i+1)/2 <= e
    int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    while (i * (i + 1) / 2 > e) --i;
    n.oi[n_own] = i; n.oj[n_own] = e - i * (i + 1) / 2; n.acc[n_own] = 0.0; ++n_own;
  }
  gacc = 0.0;
  for (int m0 = 0; m0 < M; m0 += TILE) {
    const int rows = min(TILE, M - m0);
    __syncthreads();
    for (int e = tid; e < rows * q; e += 256) {
      const int rr = e / q, c = e - rr * q;
      double val = GATHER ? Jv[(size_t)(m0 + rr) * qs + idx[c]] : Jv[(size_t)(m0 + rr) * q + c];
      if (row_scale) val *= row_scale[m0 + rr];
      T[rr * ld + c] = val;
      if (!(fabs(val) < 1.0e300)) *s_bad = 1;
    }
    for (int e = tid; e < rows; e += 256) {
      const double val = rv[m0 + e];
      rt[e] = val;
      if (!(fabs(val) < 1.0e300)) *s_bad = 1;
    }
    __syncthreads();
    if constexpr (SECOND) {
      // (J v)_m of staged row m = tid / 8: eight strided fma chains over the columns, folded by a butterfly -- a shape that
      // depends on q alone, not on the tile
      const int rr = tid / LM_ROW_LANES, k = tid % LM_ROW_LANES;
      double w = 0.0;
      if (rr < rows)
        for (int c = k; c < q; c += LM_ROW_LANES) w = fma(T[rr * ld + c], second->vv[c], w);
#pragma unroll
      for (int off = 1; off < LM_ROW_LANES; off <<= 1) w += __shfl_xor(w, off, 64);
      if (rr < rows && k == 0) {
        const double rb = second->r_base[m0 + rr], rp = second->r_probe[m0 + rr];
        if (!(fabs(rb) < 1.0e300) || !(fabs(rp) < 1.0e300)) *second->s_bad = 1;
        second->rvv[rr] = (2.0 / second->h) * ((rp - rb) / second->h - w);
      }
      __syncthreads();
    }
    for (int k = 0; k < n_own; ++k) {
      double s = n.acc[k];
      for (int rr = 0; rr < rows; ++rr) s = fma(T[rr * ld + n.oi[k]], T[rr * ld + n.oj[k]], s);
      n.acc[k] = s;
    }
    if (tid < q) {
      double s = gacc;
      for (int rr = 0; rr < rows; ++rr) s = fma(T[rr * ld + tid], rt[rr], s);
      gacc = s;
      if constexpr (SECOND) {
        double s2 = second->acc;
        for (int rr = 0; rr < rows; ++rr) s2 = fma(T[rr * ld + tid], second->rvv[rr], s2);
        second->acc = s2;
      }
    }
  }
  __syncthreads();
}

// The free columns of a vector in ascending order (is_free: this thread's column, false for tid >= the column count): a
// ballot per wave (at most LM_MAX_Q = 128 columns: waves 0 and 1 have some), the waves' counts in LDS.  Writes
// s_idx[0..n) and returns n, the same on every thread; the caller's next barrier publishes s_idx.
__device__ __forceinline__ int lm_free_columns(bool is_free, short* s_idx, int* s_cnt /*[4]*/, int tid) {
  const unsigned long long m = __ballot(is_free);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_cnt[w];
  if (is_free) s_idx[base + __popcll(m & ((1ull << lane) - 1ull))] = (short)tid;
  return s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// in-place right-looking Cholesky of the lower triangle of A (q x q, leading dimension ld) by the whole block; false if
// a pivot is not positive (the decision is uniform: every thread reads the same pivot)
__device__ __forceinline__ bool lm_cholesky(double* A, int q, int ld, int tid) {
  for (int k = 0; k < q; ++k) {
    const double piv = A[k * ld + k];
    if (!(piv > 0.0) || !(piv < 1.0e300)) return false;
    const double rp = 1.0 / sqrt(piv);
    __syncthreads();
    if (tid == 0) A[k * ld + k] = sqrt(piv);
    for (int i = k + 1 + tid; i < q; i += 256) A[i * ld + k] *= rp;
    __syncthreads();
    // trailing update: entries (i, j), k < j <= i
    const int nt = q - k - 1;
    for (int e = tid; e < nt * nt; e += 256) {
      const int i = k + 1 + e / nt, j = k + 1 + e % nt;
      if (j <= i) A[i * ld + j] = fma(-A[i * ld + k], A[j * ld + k], A[i * ld + j]);
    }
    __syncthreads();
  }
  return true;
}
// x <- L^-1 x, column-oriented: one thread finishes x_i, all threads retire it from the remaining right-hand sides (two
// barriers per column instead of a serial O(q^2) chain on one thread)
__device__ __forceinline__ void lm_forward(const double* A, double* x, int q, int ld, int tid) {
  for (int i = 0; i < q; ++i) {
    if (tid == 0) x[i] /= A[i * ld + i];
    __syncthreads();
    const double xi = x[i];
    for (int j = i + 1 + tid; j < q; j += 256) x[j] = fma(-A[j * ld + i], xi, x[j]);
    __syncthreads();
  }
}
// x <- L^-T x
__device__ __forceinline__ void lm_backward(const double* A, double* x, int q, int ld, int tid) {
  for (int i = q - 1; i >= 0; --i) {
    if (tid == 0) x[i] /= A[i * ld + i];
    __syncthreads();
    const double xi = x[i];
    for (int j = tid; j < i; j += 256) x[j] = fma(-A[i * ld + j], xi, x[j]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Batched Levenberg-Marquardt step (the caller after the path: multi-start fitting).
// The reference fits with scipy.optimize.leastsq(project.residuals, x0, Dfun=project.calc_project_jacobian)
// (tests/test_Project.py:202-213, :352-357), one start at a time; here every parameter vector of an
// ensemble takes its own damped Gauss-Newton step:
//     (J^T J + lambda_v diag(J^T J)) delta_v = -J^T r_v          (Marquardt scaling)
// One 256-thread block per vector: J^T J and J^T r accumulated from row tiles staged in LDS,
// Cholesky and the two triangular solves in LDS.  q <= LM_MAX_Q.
// ---------------------------------------------------------------------------------------------
struct LmArgs {
  const double* J;       // [V][M][q]
  const double* r;       // [V][M]
  const double* lambda;  // [V]
  double* delta;         // [V][q]
  double* pred;          // [V] predicted decrease of 0.5 |r|^2: -g.delta - 0.5 delta^T (J^T J) delta
  int32_t* status;       // [V] 0 ok, 1 not positive definite / non-finite input (delta = 0)
  int M, q, tile;
};

__global__ void __launch_bounds__(256) k_lm_step(LmArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lm_smem[];
  const int v = blockIdx.x, tid = threadIdx.x, q = a.q, M = a.M;
  const int ld = q + 1;                      // padded leading dimension of the q x q matrices
  double* A = lm_smem;                       // [q][ld]  J^T J, then its Cholesky factor (lower)
  double* dg = A + (size_t)q * ld;           // [q]      diag(J^T J)
  double* g = dg + q;                        // [q]      J^T r
  double* x = g + q;                         // [q]      right-hand side, then the solution
  double* T = x + q;                         // [tile][ld] row tile of J
  double* rt = T + (size_t)a.tile * ld;      // [tile]
  __shared__ int s_bad;
  if (tid == 0) s_bad = 0;
  LmTriangle n;
  int n_own;
  double gacc;
  lm_normal_equations(n, n_own, gacc, a.J + (size_t)v * M * q, a.r + (size_t)v * M, nullptr, M, q, a.tile, T, rt, &s_bad, tid);
  for (int k = 0; k < n_own; ++k) A[n.oi[k] * ld + n.oj[k]] = n.acc[k];
  if (tid < q) g[tid] = gacc;
  __syncthreads();
  const double lam = a.lambda[v];
  if (tid < q) {
    const double d = A[tid * ld + tid];
    dg[tid] = d;
    // Marquardt scaling; a column J never touches (d = 0) gets a unit pivot: delta_c = 0
    A[tid * ld + tid] = d > 0.0 ? d * (1.0 + lam) : 1.0;
    x[tid] = -g[tid];
  }
  __syncthreads();
  // (uniform: s_bad and lam are the same for every thread, and so is what lm_cholesky decides)
  if (s_bad != 0 || !(lam >= 0.0) || !lm_cholesky(A, q, ld, tid)) {
    for (int c = tid; c < q; c += 256) a.delta[(size_t)v * q + c] = 0.0;
    if (tid == 0) { a.pred[v] = 0.0; a.status[v] = 1; }
    return;
  }
  lm_forward(A, x, q, ld, tid);              // L y = -g
  lm_backward(A, x, q, ld, tid);             // L^T x = y
  // predicted decrease of 0.5 |r|^2 under the Gauss-Newton model, H = J^T J:  -g.d - 0.5 d^T H d  with
  // (H + lambda D) d = -g  =>  d^T H d = -g.d - lambda sum D_i d_i^2   (D = diag(H), or 1 where it is 0)
  double part = 0.0;
  if (tid < q) {
    a.delta[(size_t)v * q + tid] = x[tid];
    const double Di = dg[tid] > 0.0 ? dg[tid] : 0.0;
    part = -0.5 * g[tid] * x[tid] + 0.5 * lam * Di * x[tid] * x[tid];
  }
  __shared__ double s_red[4];
  const double tot = block_sum(part, s_red);
  if (tid == 0) { a.pred[v] = tot; a.status[v] = 0; }
}

// ---------------------------------------------------------------------------------------------
// sbm_lm_trust_step: the Levenberg-Marquardt PARAMETER of a scaled trust region, per vector.
//
// What MINPACK's lmder does between two Jacobian evaluations (lmpar, More 1978), on the normal equations:
// given the scaling D (the largest column norm of J seen so far, kept by the caller from call to call) and a radius
// Delta, find lambda >= 0 with  (J^T J + lambda D^2) x = -J^T r  and  | ||D x|| - Delta | <= 0.1 Delta  (lambda = 0 if
// the Gauss-Newton step is already inside), by More's safeguarded Newton iteration on
// phi(lambda) = ||D x(lambda)|| - Delta:  lambda += (phi / Delta) / ||L^-1 D^2 x / ||D x||||^2  with L the Cholesky
// factor of the damped matrix, kept between the bounds the iteration itself produces.  At most 10 factorisations of a
// q x q matrix per call (two to three are the rule): microseconds, against the milliseconds of the integration that
// follows -- which is why the search for lambda happens here, in one launch, rather than as a sequence of trial
// INTEGRATIONS with lambda multiplied up and down (sbm_lm_step + project/fitting.py's 'marquardt' loop).
// One 256-thread block per vector; J^T J in registers (the lower triangle, spread over the threads), the matrix being
// factored in LDS.
// ---------------------------------------------------------------------------------------------
struct LmTrustArgs {
  const double* J;       // [V][M][q]
  const double* r;       // [V][M]
  double* dscale;        // [V][q]  in / out: D, made max(D, column norm of J) here (0 on the first call)
  const double* radius;  // [V]     Delta > 0
  double* lambda;        // [V]     in: the previous parameter (a starting guess), out: the one found
  double* delta;         // [V][q]  out: x
  double* pred;          // [V]     out: predicted decrease of 0.5 |r|^2 = -g.x - 0.5 x^T J^T J x
  double* dxnorm;        // [V]     out: ||D x||
  int32_t* status;       // [V]     out: 0, 1: non-finite input / no positive definite system found (x = 0), 2: skipped
  int M, q, tile;
  // extended entry point (sbm_lm_trust_step_ex); all nullable / 0
  const double* row_scale;   // [M]    J is used as diag(row_scale) J (reference_compat Jacobians: 1 / sigma)
  const int32_t* skip;       // [V]    != 0: leave the vector alone (x = 0, status 2)
  double max_step;           // > 0: every component of x is clipped to +-max_step; pred, dxnorm, gtx are those of the clipped step
  double* gtx;               // [V]    out: g . x (the directional derivative of 0.5 |r|^2 along the step)
  const double* theta;       // [V][q] with `trial`: trial = theta + x
  double* trial;             // [V][q]
};

// HELD = false is sbm_lm_trust_step[_ex]: qf = q, column c is column c.  HELD = true (sbm_lm_trust_step_held): the free
// columns of the vector, idx[0..q) in ascending order, are compacted -- J is gathered through idx when its tile is staged
// and from there on the kernel IS the HELD = false kernel on the q x q problem (leading dimension q + 1, thread t < q owns
// free column idx[t], the same sums in the same order: the same bits as sbm_lm_trust_step_ex on J with the held columns
// deleted), until the step is scattered back through idx.  A held column has no D, no g, no x: dscale = 0, delta = 0,
// trial = theta (a copy) are written for it before anything else, so every way out of the kernel leaves them.
// k_lm_update and k_lm_accept need no change for this: k_lm_update reads dscale only in ||D theta|| (exact zeros from
// the held columns: lmder's xnorm of the reduced problem) and everything else per start; k_lm_accept copies trial rows,
// whose held entries are theta's.
//
// BOUNDED (with HELD; sbm_lm_trust_step_bounded): an active-set step inside the box lower <= theta <= upper.  The mask the
// system is compacted by is chosen HERE, per call: a gradient pre-pass gives thread c < qf its g_c = sum_m rs_m J_mc r_m
// (one fma chain over the rows in ascending order -- the chain lm_normal_equations runs for the column afterwards, so the
// sign tested is the sign of the g the step uses), and a column that sits on a bound with the gradient pushing outward
// (theta <= lower and g > 0, theta >= upper and g < 0) joins the caller's held ones for this step; g == 0 leaves it free.
// From the ballot on, the kernel is the HELD kernel on that effective mask, with two additions after the max_step clip:
// the step is projected into the box (a component that would leave it ends ON the bound: trial gets the bound's bits, and
// the step counts as clipped, so pred, dxnorm and gtx are those of the step taken), and a projected step that is no
// descent step of the model any more (not gtx < 0 and pred > 0) is not taken (status 4: k_lm_update halves the radius).
// Nothing free although the caller has not held everything: a constrained stationary point, status 3.
struct LmBounds {
  const double* lower;   // [V][q]  -inf: no bound on that side
  const double* upper;   // [V][q]  +inf
  int32_t* active_out;   // [V][q]  nullable: 0 free, 1 held by the caller, 2 held at the lower bound, 3 at the upper
};

template <bool HELD, bool BOUNDED = false>
__device__ __forceinline__ void lm_trust_body(LmTrustArgs a, const int32_t* held, LmBounds b = LmBounds{}) {
  static_assert(HELD || !BOUNDED, "the bounded step compacts its system");
  extern __shared__ __attribute__((aligned(16))) double lm_smem[];
  const int v = blockIdx.x, tid = threadIdx.x, qf = a.q, M = a.M, TILE = a.tile;
  // no step: delta = 0, trial = theta.  Status 2: a skipped vector, or one with no free column; 1: no system solved;
  // 3, 4: see BOUNDED
  auto leave_alone = [&](int status) {
    for (int c = tid; c < qf; c += 256) {
      a.delta[(size_t)v * qf + c] = 0.0;
      if (a.trial && a.theta) a.trial[(size_t)v * qf + c] = a.theta[(size_t)v * qf + c];
    }
    if (tid == 0) { a.pred[v] = 0.0; a.dxnorm[v] = 0.0; a.status[v] = status; if (a.gtx) a.gtx[v] = 0.0; }
  };
  int q = qf;                                // columns of the system that is solved
  [[maybe_unused]] const short* idx = nullptr;
  if constexpr (HELD) {
    if (a.skip && a.skip[v]) { leave_alone(2); return; }
    // the free columns in ascending order (lm_free_columns)
    __shared__ short s_idx[LM_MAX_Q];
    __shared__ int s_cnt[4];
    [[maybe_unused]] int code = 0;           // BOUNDED: this thread's column as active_out names it
    bool is_free;
    if constexpr (BOUNDED) {
      if (tid < qf) {
        const size_t at = (size_t)v * qf + tid;
        if (held && held[at] != 0) {
          code = 1;
        } else {
          const double* Jc = a.J + (size_t)v * M * qf + tid;
          const double* rv = a.r + (size_t)v * M;
          // one chain of M dependent fmas; the loads of eight rows are issued together, ahead of their fmas (the order of the
          // chain, and so its bits, is the rows')
          double gc = 0.0;
          for (int m0 = 0; m0 < M; m0 += 8) {
            double val[8], rr[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int m = min(m0 + k, M - 1);
              val[k] = Jc[(size_t)m * qf];
              if (a.row_scale) val[k] *= a.row_scale[m];
              rr[k] = rv[m];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (m0 + k < M) gc = fma(val[k], rr[k], gc);
          }
          const double th = a.theta[at];
          if (th <= b.lower[at] && gc > 0.0) code = 2;
          else if (th >= b.upper[at] && gc < 0.0) code = 3;
        }
        if (b.active_out) b.active_out[at] = code;
      }
      is_free = tid < qf && code == 0;
    } else {
      is_free = tid < qf && held[(size_t)v * qf + tid] == 0;
    }
    q = lm_free_columns(is_free, s_idx, s_cnt, tid);
    if (tid < qf && !is_free) a.dscale[(size_t)v * qf + tid] = 0.0;
    if (q == 0) {                            // (uniform)
      if constexpr (BOUNDED) {
        if (__syncthreads_or(code >= 2)) { leave_alone(3); return; }      // bounds hold what the caller left free
      }
      leave_alone(2);
      return;
    }
    if (tid < qf && !is_free) {
      a.delta[(size_t)v * qf + tid] = 0.0;
      if (a.trial && a.theta) a.trial[(size_t)v * qf + tid] = a.theta[(size_t)v * qf + tid];
    }
    __syncthreads();
    idx = s_idx;
  }
  auto col = [&](int c) -> int { if constexpr (HELD) return idx[c]; else return c; };   // column of J / theta behind column c
  const int ld = q + 1;
  double* A = lm_smem;                       // [q][ld]  the damped matrix / its Cholesky factor
  double* D = A + (size_t)q * ld;            // [q]      scaling
  double* g = D + q;                         // [q]      J^T r
  double* x = g + q;                         // [q]      step
  double* w = x + q;                         // [q]      work vector of the Newton correction
  double* xg = w + q;                        // [q]      the last step that came out of a successful factorisation
  double* T = xg + q;                        // [TILE][ld] row tile of J
  double* rt = T + (size_t)TILE * ld;        // [TILE]
  __shared__ int s_bad;
  __shared__ double s_red[4];
  if constexpr (!HELD)
    if (a.skip && a.skip[v]) { leave_alone(2); return; }
  if (tid == 0) s_bad = 0;
  LmTriangle n;
  int n_own;
  double gacc;
  lm_normal_equations<HELD>(n, n_own, gacc, a.J + (size_t)v * M * qf, a.r + (size_t)v * M, a.row_scale, M, q, TILE, T, rt, &s_bad,
                            tid, qf, idx);
  const double Delta = a.radius[v];
  double lam = a.lambda[v];
  // scaling: the largest column norm seen so far (MINPACK mode 1); a column J never touches gets 1
  for (int k = 0; k < n_own; ++k)
    if (n.oi[k] == n.oj[k]) {
      const double cn = sqrt(fmax(n.acc[k], 0.0));
      double d = fmax(a.dscale[(size_t)v * qf + col(n.oi[k])], cn);
      if (!(d > 0.0)) d = 1.0;
      D[n.oi[k]] = d;
      a.dscale[(size_t)v * qf + col(n.oi[k])] = d;
    }
  if (tid < q) g[tid] = gacc;
  __syncthreads();
  bool bad = s_bad != 0 || !(Delta > 0.0) || !(lam >= 0.0);
  // paru = || D^-1 g || / Delta: with that much damping the step is inside the region
  double part = 0.0;
  if (tid < q) { const double t = g[tid] / D[tid]; part = t * t; }
  const double gnorm = sqrt(block_sum(part, s_red));
  double paru = gnorm / Delta;
  if (!(paru > 0.0)) paru = 2.2e-308 / fmin(Delta, 0.1);
  double parl = 0.0, fp = 0.0, dxn = 0.0;
  bool have = false;
  double lam_good = 0.0, dxn_good = 0.0;      // ... of the last successful factorisation (its step is parked in xg)

  auto solve_with = [&](double par) -> bool {          // A <- chol(J^T J + par D^2); x <- -A^-1 g; dxn, fp
    for (int k = 0; k < n_own; ++k) {
      const int i = n.oi[k], j = n.oj[k];
      A[i * ld + j] = (i == j) ? fma(par * D[i], D[i], n.acc[k]) : n.acc[k];
    }
    if (tid < q) x[tid] = -g[tid];
    __syncthreads();
    if (!lm_cholesky(A, q, ld, tid)) return false;
    lm_forward(A, x, q, ld, tid);
    lm_backward(A, x, q, ld, tid);
    double p2 = 0.0;
    if (tid < q) { const double t = D[tid] * x[tid]; p2 = t * t; xg[tid] = x[tid]; }
    dxn = sqrt(block_sum(p2, s_red));
    fp = dxn - Delta;
    lam_good = par;
    dxn_good = dxn;
    return true;
  };
  auto newton_denominator = [&]() -> double {           // || L^-1 (D^2 x / dxn) ||^2 with the current factor
    if (tid < q) w[tid] = D[tid] * D[tid] * x[tid] / dxn;
    __syncthreads();
    lm_forward(A, w, q, ld, tid);
    double p2 = 0.0;
    if (tid < q) p2 = w[tid] * w[tid];
    return block_sum(p2, s_red);
  };

  if (!bad) {
    // the Gauss-Newton step, if J has full rank numerically
    if (solve_with(0.0)) {
      if (fp <= 0.1 * Delta) { lam = 0.0; have = true; }
      else { const double den = newton_denominator(); if (den > 0.0) parl = (fp / Delta) / den; }
    }
    if (!have) {
      bool any = false;                                // a damped system has been solved
      lam = fmin(fmax(lam, parl), paru);
      if (lam == 0.0) lam = (dxn > 0.0) ? gnorm / dxn : 1.0e-3 * paru;
      for (int it = 0; it < 10; ++it) {
        if (lam == 0.0) lam = fmax(2.2e-308, 1.0e-3 * paru);
        const double fp_old = fp;
        if (!solve_with(lam)) {                        // rounding: not positive definite at this damping yet
          // A is half factored and x holds -g: what counts from here on is the last step that WAS solved for (xg)
          parl = fmax(parl, lam);
          lam = fmax(10.0 * lam, 1.0e-3 * paru);
          if (lam > 1.0e3 * paru) break;               // (only non-finite data gets here)
          continue;
        }
        any = true;
        if (fabs(fp) <= 0.1 * Delta || (parl == 0.0 && fp <= fp_old && fp_old < 0.0) || it == 9) break;
        const double den = newton_denominator();
        const double parc = den > 0.0 ? (fp / Delta) / den : 0.0;
        if (fp > 0.0) parl = fmax(parl, lam);
        if (fp < 0.0) paru = fmin(paru, lam);
        lam = fmax(parl, lam + parc);
      }
      // the answer is the last DAMPED system that factored -- never the right-hand side a failed factorisation left
      // in x, nor the undamped step that was outside the region
      have = any && lam_good > 0.0;
      if (have) { lam = lam_good; dxn = dxn_good; }
      __syncthreads();
      if (have && tid < q) x[tid] = xg[tid];
      __syncthreads();
    }
  }
  if (bad || !have) { leave_alone(1); return; }
  // a step bound per component (exp(theta) has to stay finite): clip, and report the quantities of the step TAKEN
  bool clipped = false;
  if (a.max_step > 0.0) {
    int cl = 0;
    if (tid < q && fabs(x[tid]) > a.max_step) { x[tid] = copysign(a.max_step, x[tid]); cl = 1; }
    clipped = __syncthreads_or(cl) != 0;
  }
  // BOUNDED: the projection into the box; a component that would leave it ends on the bound itself
  [[maybe_unused]] bool projected = false, on_bound = false;
  [[maybe_unused]] double t_bound = 0.0;
  if constexpr (BOUNDED) {
    if (tid < q) {
      const size_t at = (size_t)v * qf + col(tid);
      const double th = a.theta[at], s = th + x[tid];
      const double t = fmin(fmax(s, b.lower[at]), b.upper[at]);
      if (t != s) { x[tid] = t - th; t_bound = t; on_bound = true; }
    }
    projected = __syncthreads_or(on_bound ? 1 : 0) != 0;
    clipped = clipped || projected;
  }
  double gx = 0.0;
  if (tid < q) gx = g[tid] * x[tid];
  const double gtx = block_sum(gx, s_red);
  double tot;
  if (!clipped) {
    // predicted decrease of 0.5 |r|^2 under the Gauss-Newton model:  -g.x - 0.5 x^T H x  with  x^T H x = -g.x - lam dxn^2
    tot = -0.5 * gtx + 0.5 * lam * dxn * dxn;
  } else {
    double p2 = 0.0;
    if (tid < q) { const double t = D[tid] * x[tid]; p2 = t * t; }
    dxn = sqrt(block_sum(p2, s_red));
    double xhx = 0.0;                                  // x^T (J^T J) x from the lower triangle in registers
    for (int k = 0; k < n_own; ++k) xhx += (n.oi[k] == n.oj[k] ? 1.0 : 2.0) * n.acc[k] * x[n.oi[k]] * x[n.oj[k]];
    tot = -gtx - 0.5 * block_sum(xhx, s_red);
  }
  if constexpr (BOUNDED) {
    // (uniform: gtx and tot are block sums.)  lmder's radius formula wants g . x < 0; with the radius halved often enough
    // the step is a scaled gradient step, whose projection descends
    if (projected && !(gtx < 0.0 && tot > 0.0)) { leave_alone(4); return; }
  }
  if (tid < q) {
    a.delta[(size_t)v * qf + col(tid)] = x[tid];
    if (a.trial && a.theta)
      a.trial[(size_t)v * qf + col(tid)] = (BOUNDED && on_bound) ? t_bound : a.theta[(size_t)v * qf + col(tid)] + x[tid];
  }
  if (tid == 0) { a.pred[v] = tot; a.dxnorm[v] = dxn; a.lambda[v] = lam; a.status[v] = 0; if (a.gtx) a.gtx[v] = gtx; }
}

__global__ void __launch_bounds__(256) k_lm_trust(LmTrustArgs a) { lm_trust_body<false>(a, nullptr); }
// held [V][q]: != 0 = the column does not move.  Static LDS: k_lm_trust's 304 bytes + 256 of the index list + 16 of the
// waves' counts = LM_HELD_STATIC_LDS, which the host wrapper takes off the limit it chooses the row tile for.
constexpr int LM_HELD_STATIC_LDS = 576;
__global__ void __launch_bounds__(256) k_lm_trust_held(LmTrustArgs a, const int32_t* held) { lm_trust_body<true>(a, held); }
// held nullable here; theta, trial, lower, upper are not.  The same static LDS as k_lm_trust_held (the gradient pre-pass and
// the projection live in registers): LM_HELD_STATIC_LDS serves both.
__global__ void __launch_bounds__(256) k_lm_trust_bounded(LmTrustArgs a, const int32_t* held, LmBounds b) {
  lm_trust_body<true, true>(a, held, b);
}

// ---------------------------------------------------------------------------------------------
// sbm_lm_update / sbm_lm_accept: lmder's bookkeeping between two trust-region steps, for V starts in two launches
// (round 2 spelled it as ~70 tensor selects per iteration: 68 000 micro-launches in a 100-iteration fit).
// ---------------------------------------------------------------------------------------------
struct LmUpdateArgs {
  const double* cost;       // [V] 0.5 |r|^2 at the current point (inf: a start that cannot be integrated)
  const double* norms_t;    // [V] |r|^2 at the trial point
  const int32_t* status_t;  // [V] integration status of the trial point (non-zero: failed)
  const double* pred;       // [V] from sbm_lm_trust_step_ex
  const double* dxnorm;     // [V]
  const double* gtx;        // [V]
  const int32_t* st;        // [V] status of the trust step (0 ok, 1 no system solved, 2 skipped, 3 / 4: sbm_lm_trust_step_bounded)
  const double* theta;      // [V][q] current point (for ||D theta||)
  const double* dscale;     // [V][q]
  double* radius;           // [V] in / out
  double* lambda;           // [V] in / out
  int32_t* done;            // [V] in / out: 1 = converged (or never started)
  int32_t* accept;          // [V] out: 1 = take the trial point
  int32_t* n_iter;          // [V] in / out: iteration at which the start converged
  int32_t* counters;        // [2] out: starts still running, trial points accepted (zeroed by the caller's memset)
  double* ratio_out;        // [V] nullable: actual / predicted reduction (traces)
  double ftol, xtol;
  int V, q, iteration, first;
};

__global__ void __launch_bounds__(256) k_lm_update(LmUpdateArgs a) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= a.V) return;
  a.accept[v] = 0;
  if (a.done[v]) return;
  const double cost = a.cost[v];
  double cost_t = 0.5 * a.norms_t[v];
  if (!(cost_t < 1.0e300) || a.status_t[v] != 0) cost_t = __builtin_inf();
  const int st = a.st[v];
  double radius = a.radius[v], lam = a.lambda[v];
  const double dxn = a.dxnorm[v];
  if (a.first && st == 0) radius = fmin(radius, dxn);          // lmder: on the first iteration Delta = min(Delta, ||D p||)
  // lmder's quantities, relative to |r|^2 = 2 cost
  const double safe = cost > 0.0 ? cost : 1.0;
  const bool not_10x_worse = 0.1 * sqrt(cost_t) < sqrt(cost);   // (false for an infinite trial cost)
  const double actred = not_10x_worse ? 1.0 - cost_t / safe : -1.0;
  const double prered = a.pred[v] / safe;
  const double dirder = a.gtx[v] / (2.0 * safe);               // g . p / |r|^2 (= -(|J p|^2 + lam |D p|^2) / |r|^2 for an unclipped step)
  const double ratio = prered > 0.0 ? actred / prered : 0.0;
  if (a.ratio_out) a.ratio_out[v] = ratio;
  if (st == 3) {
    // sbm_lm_trust_step_bounded: every parameter the caller left free sits on a bound with the gradient pushing outward --
    // a constrained stationary point.  Converged where it stands; the radius is not touched
    a.done[v] = 1;
    a.n_iter[v] = a.iteration + 1;
    return;
  }
  if (st != 0) {
    // no system could be solved (1), or the projected step did not descend (4): halve the radius, keep the point
    a.radius[v] = 0.5 * radius;
    atomicAdd(a.counters, 1);
    return;
  }
  if (ratio <= 0.25) {
    double temp = actred >= 0.0 ? 0.5 : 0.5 * dirder / ((dirder + 0.5 * actred) != 0.0 ? dirder + 0.5 * actred : -1.0);
    if (!not_10x_worse || temp < 0.1 || !(temp == temp) || !(fabs(temp) < 1.0e300)) temp = 0.1;
    radius = temp * fmin(radius, dxn / 0.1);
    lam = lam / temp;
  } else if (lam == 0.0 || ratio >= 0.75) {
    radius = dxn / 0.5;
    lam = 0.5 * lam;
  }
  const bool ok = ratio >= 1.0e-4 && cost_t < 1.0e300;
  a.accept[v] = ok ? 1 : 0;
  // lmder's convergence tests (info 1, 2); ||D theta|| at the point the iteration started from (the current point, before
  // sbm_lm_accept moves it: lmder itself measures the point it ends on)
  double xn2 = 0.0;
  for (int c = 0; c < a.q; ++c) {
    const double t = a.dscale[(size_t)v * a.q + c] * a.theta[(size_t)v * a.q + c];
    xn2 = fma(t, t, xn2);
  }
  const bool conv_f = fabs(actred) <= a.ftol && prered <= a.ftol && 0.5 * ratio <= 1.0;
  const bool conv_x = radius <= a.xtol * sqrt(xn2);
  a.radius[v] = radius;
  a.lambda[v] = lam;
  if (conv_f || conv_x) {
    a.done[v] = 1;
    a.n_iter[v] = a.iteration + 1;
  } else {
    atomicAdd(a.counters, 1);
  }
  if (ok) atomicAdd(a.counters + 1, 1);
}

// accepted trial points become the current ones: theta, residuals, Jacobian (scaled by row_scale if given), cost
__global__ void __launch_bounds__(256) k_lm_accept(const int32_t* __restrict__ accept, int q, int M, const double* __restrict__ trial,
                                                   const double* __restrict__ r_t, const double* __restrict__ J_t,
                                                   const double* __restrict__ norms_t, double* __restrict__ theta,
                                                   double* __restrict__ r, double* __restrict__ J, double* __restrict__ cost) {
  const int v = blockIdx.x;
  if (!accept[v]) return;
  const size_t nJ = (size_t)M * q;
  const double2* src = reinterpret_cast<const double2*>(J_t + (size_t)v * nJ);
  double2* dst = reinterpret_cast<double2*>(J + (size_t)v * nJ);
  // 16-byte accesses only where both rows really are 16-byte aligned: an even row length and element offset say nothing
  // about the base pointers (a view that starts one double into an allocation is 8-byte aligned)
  if ((nJ & 1) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    for (size_t e = threadIdx.x + (size_t)blockIdx.y * blockDim.x; e < nJ / 2; e += (size_t)blockDim.x * gridDim.y) dst[e] = src[e];
  } else {
    for (size_t e = threadIdx.x + (size_t)blockIdx.y * blockDim.x; e < nJ; e += (size_t)blockDim.x * gridDim.y)
      J[(size_t)v * nJ + e] = J_t[(size_t)v * nJ + e];
  }
  if (blockIdx.y == 0) {
    for (int e = threadIdx.x; e < M; e += blockDim.x) r[(size_t)v * M + e] = r_t[(size_t)v * M + e];
    for (int e = threadIdx.x; e < q; e += blockDim.x) theta[(size_t)v * q + e] = trial[(size_t)v * q + e];
    if (threadIdx.x == 0) cost[v] = 0.5 * norms_t[v];
  }
}

#endif  // SBM_LM_HPP
