// sbm_sampling_axes.hpp -- kernel of sbm_sampling_axes (include/sbm.h): what the second algorithm of the reference's
// sampler (project/Ensembles.py:153-157, 200-258) needs per chain and step besides the integration and the
// Metropolis-Hastings rule (sbm_sampler.hpp) -- the eigen-decomposition of the Gauss-Newton Hessian at the trial point
// with SloppyCell's clipping recipe on top.
//
// k_sampling_axes: one 256-thread workgroup per chain, one launch for everything.
//   1. A = H / 2.  From a Jacobian: row tiles of J (times row_scale) go through LDS -- the tile borrows the space of V,
//      which is not needed yet -- and every thread adds the tile's contribution to its entries of A in LDS.  All q^2
//      entries are formed, not one triangle: fma(x_i, x_j, acc) does not depend on the order of the two factors, so the
//      two triangles come out equal bit for bit and no mirror pass is needed.  From a matrix: (H + H^T) / 4.
//   2. Cyclic Jacobi in the round-robin (parallel) ordering: with n = q rounded up to even, a sweep is n - 1 rounds of
//      n / 2 disjoint pairs (circle method: index n - 1 stays, the others rotate; a pair with the padding index of an odd q
//      is idle).  In a round thread k computes the rotation of pair k from the current A; then, with barriers between, a
//      column pass on A, and a row pass on A together with the column pass on V.  A pair is rotated unless
//      |a_pq| <= DBL_EPSILON sqrt(|a_pp|) sqrt(|a_qq|), and after every sweep all pairs are tested against the same bound
//      (both on the upper triangle, the one the rotations are computed from; the rotated entry is zeroed on both sides).
//      The bound is relative to the two diagonal entries, not to ||A||: a sloppy Hessian has eigenvalues many decades
//      below its largest, and the step lengths are 1 / sqrt of exactly those.  40 sweeps at most.
//   3. Rank sort of the signed eigenvalues (ascending, as eigh), absolute values, sign convention (the component of
//      largest magnitude of every eigenvector positive, lowest index on ties), the recipe, the outputs.
// LDS: A and V at leading dimension q + 1 -- the passes map consecutive lanes to consecutive columns, so the padding only
// matters to the sign scan down a column -- plus 5 q doubles and 2 q ints: 153 600 bytes at q = SBM_SAMPLING_AXES_MAX_Q = 96.
// No arrays in registers, no scratch.
// k_sampling_axes_held (sbm_sampling_axes_held) is the same body on the free columns of every chain: see sampling_axes_body.
#ifndef SBM_SAMPLING_AXES_HPP
#define SBM_SAMPLING_AXES_HPP

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "sbm_block_reduce.hpp"

#define SBM_AXES_MAX_SWEEPS 40

struct sbm_axes_args {
  const double* J;           // [C][M][q] or NULL
  const double* row_scale;   // [M] or NULL
  const double* H;           // [q][q] / [C][q][q] or NULL
  int per_chain_H, M, q;
  double cutoff, temperature, step_scale;
  double* eig;               // [C][q]      nullable
  double* V;                 // [C][q][q]   nullable
  double* s;                 // [C][q]      nullable
  double* samp;              // [C][q][q]   nullable
  int32_t* status;           // [C]
};

// bytes of dynamic LDS of k_sampling_axes
static inline size_t sbm_axes_lds_bytes(int q) {
  const size_t ld = (size_t)q + 1, np = ((size_t)q + 1) / 2;
  return sizeof(double) * (2 * (size_t)q * ld + 2 * np + 4 * (size_t)q) + sizeof(int) * (2 * np + (size_t)q);
}

// HELD = false is sbm_sampling_axes: q = qf, column c is column c.  HELD = true (sbm_sampling_axes_held): the free columns
// f_0 < ... < f_{q-1} of the chain (held[c][j] == 0) are listed in LDS by a ballot per wave, J's row tile (or H's rows and
// columns) is gathered through the list, and from there on the kernel IS the HELD = false kernel on the q x q problem
// (leading dimension q + 1, the same sums in the same order: the same bits as sbm_sampling_axes on the arrays with the
// held columns deleted; a held entry is never read), until the outputs are scattered back into the full qf layout:
// row f_k of V and samp holds row k of the reduced ones in its first q columns, everything else is 0, and eig = 0, s = 1
// from position q on -- axes along which sbm_mh_propose does not move and which add u = 0, log 1 = 0 to the candidate
// density of sbm_mh_accept_hastings.  Nothing free: status 0 with that padding alone.
constexpr int AXES_MAX_Q = 96;                 // SBM_SAMPLING_AXES_MAX_Q of include/sbm.h
template <bool HELD>
__device__ __forceinline__ void sampling_axes_body(sbm_axes_args a, const int32_t* held) {
  extern __shared__ __attribute__((aligned(16))) double ax_smem[];
  const int c = blockIdx.x, tid = threadIdx.x, qf = a.q;
  int q = qf;                                  // order of the system that is solved
  [[maybe_unused]] const short* idx = nullptr;
  if constexpr (HELD) {
    // the free columns in ascending order: a ballot per wave (qf <= 96: waves 0 and 1 have columns), the waves' counts in LDS
    __shared__ short s_idx[AXES_MAX_Q];
    __shared__ int s_cnt[4];
    const bool is_free = tid < qf && held[(size_t)c * qf + tid] == 0;
    const unsigned long long m = __ballot(is_free);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_cnt[w];
    q = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (is_free) s_idx[base + __popcll(m & ((1ull << lane) - 1ull))] = (short)tid;
    // the padding: held rows of V and samp, and the axes from q on
    for (int e = tid; e < qf * qf; e += 256) {
      if (held[(size_t)c * qf + e / qf] == 0) continue;
      if (a.V) a.V[(size_t)c * qf * qf + e] = 0.0;
      if (a.samp) a.samp[(size_t)c * qf * qf + e] = 0.0;
    }
    for (int i = q + tid; i < qf; i += 256) {
      if (a.eig) a.eig[(size_t)c * qf + i] = 0.0;
      if (a.s) a.s[(size_t)c * qf + i] = 1.0;
    }
    if (q == 0) {                              // (uniform)
      if (tid == 0) a.status[c] = 0;
      return;
    }
    __syncthreads();
    idx = s_idx;
  }
  auto col = [&](int k) -> int { if constexpr (HELD) return idx[k]; else return k; };   // column of J / H behind column k
  const int ld = q + 1;
  const int ne = (q + 1) & ~1, np = ne / 2, nr = ne - 1;      // players, pairs of a round, rounds of a sweep
  double* A = ax_smem;                         // [q][ld]
  double* Vm = A + (size_t)q * ld;             // [q][ld]  eigenvectors in the columns; before that the row tile of J
  double* rc = Vm + (size_t)q * ld;            // [np]     cosines of the round
  double* rs = rc + np;                        // [np]     sines
  double* ev = rs + np;                        // [q]      signed eigenvalues, by column of Vm
  double* av = ev + q;                         // [q]      |eigenvalue|, sorted
  double* sv = av + q;                         // [q]      step lengths, sorted
  double* sg = sv + q;                         // [q]      sign of the eigenvector, by column of Vm
  int* pp = (int*)(sg + q);                    // [np]     first index of the pair
  int* pq = pp + np;                           // [np]     second index (> first), -1: nothing to do
  int* perm = pq + np;                         // [q]      column of Vm that holds the k-th eigenvalue
  const int qq = q * q;
  int bad = 0;

  // ---- 1. A = H / 2
  if (a.J) {
    const int M = a.M, TILE = q < 32 ? q : 32;
    const double* Jc = a.J + (size_t)c * M * qf;
    double* T = Vm;
    for (int e = tid; e < qq; e += 256) A[(e / q) * ld + e % q] = 0.0;
    for (int m0 = 0; m0 < M; m0 += TILE) {
      const int rows = min(TILE, M - m0);
      __syncthreads();
      for (int e = tid; e < rows * q; e += 256) {
        const int rr = e / q, cc = e - rr * q;
        double val = Jc[(size_t)(m0 + rr) * qf + col(cc)];
        if (a.row_scale) val *= a.row_scale[m0 + rr];
        T[rr * ld + cc] = val;
        bad |= !is_finite(val);
      }
      __syncthreads();
      for (int e = tid; e < qq; e += 256) {
        const int i = e / q, j = e - i * q;
        double acc = A[i * ld + j];
        for (int rr = 0; rr < rows; ++rr) acc = fma(T[rr * ld + i], T[rr * ld + j], acc);
        A[i * ld + j] = acc;
      }
    }
    __syncthreads();
    for (int e = tid; e < qq; e += 256) {
      const int i = e / q, j = e - i * q;
      const double v = 0.5 * A[i * ld + j];
      A[i * ld + j] = v;
      bad |= !is_finite(v);
    }
  } else {
    const double* Hc = a.H + (a.per_chain_H ? (size_t)c * qf * qf : 0);
    for (int e = tid; e < qq; e += 256) {
      const int i = e / q, j = e - i * q;
      const double hij = Hc[(size_t)col(i) * qf + col(j)], hji = Hc[(size_t)col(j) * qf + col(i)];
      const double v = 0.5 * (0.5 * hij + 0.5 * hji);
      A[i * ld + j] = v;
      bad |= !is_finite(hij) || !is_finite(v);
    }
  }
  for (int e = tid; e < qq; e += 256) {
    const int i = e / q, j = e - i * q;
    Vm[i * ld + j] = i == j ? 1.0 : 0.0;
  }
  bad = __syncthreads_or(bad);

  // ---- 2. Jacobi
  int sweeps = 0;
  bool converged = false;
  while (!bad) {
    int open = 0;
    for (int e = tid; e < qq; e += 256) {
      const int i = e / q, j = e - i * q;
      if (i < j) open |= !(fabs(A[i * ld + j]) <= DBL_EPSILON * sqrt(fabs(A[i * ld + i])) * sqrt(fabs(A[j * ld + j])));
    }
    if (!__syncthreads_or(open)) { converged = true; break; }
    if (sweeps == SBM_AXES_MAX_SWEEPS) break;
    for (int r = 0; r < nr; ++r) {
      if (tid < np) {
        int p = tid == 0 ? nr : (r + tid) % nr;
        int s2 = tid == 0 ? r : (r - tid + nr) % nr;
        if (p > s2) { const int t = p; p = s2; s2 = t; }
        double cs = 1.0, sn = 0.0;
        int second = -1;
        if (s2 < q) {
          const double apq = A[p * ld + s2], app = A[p * ld + p], aqq = A[s2 * ld + s2];
          if (!(fabs(apq) <= DBL_EPSILON * sqrt(fabs(app)) * sqrt(fabs(aqq)))) {
            const double theta = (aqq - app) / (2.0 * apq);
            // the smaller root of t^2 + 2 theta t - 1 = 0; theta beyond the range of its square: t = 1 / (2 theta)
            const double t = fabs(theta) > 1.0e150 ? 0.5 / theta
                                                   : copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
            cs = 1.0 / sqrt(fma(t, t, 1.0));
            sn = t * cs;
            second = s2;
          }
        }
        pp[tid] = p;
        pq[tid] = second;
        rc[tid] = cs;
        rs[tid] = sn;
      }
      __syncthreads();
      // A <- A P: columns p and s2 of every row (consecutive lanes: consecutive pairs, i.e. consecutive columns)
      for (int e = tid; e < np * q; e += 256) {
        const int i = e / np, k = e - i * np;
        const int s2 = pq[k];
        if (s2 < 0) continue;
        const int p = pp[k];
        const double cs = rc[k], sn = rs[k];
        const double x = A[i * ld + p], y = A[i * ld + s2];
        A[i * ld + p] = fma(cs, x, -sn * y);
        A[i * ld + s2] = fma(sn, x, cs * y);
      }
      __syncthreads();
      // A <- P^T A: rows p and s2, the rotated entry set to zero on both sides; V <- V P
      for (int e = tid; e < 2 * np * q; e += 256) {
        const bool on_v = e >= np * q;
        const int f = on_v ? e - np * q : e;
        if (!on_v) {
          const int k = f / q, j = f - k * q;
          const int s2 = pq[k];
          if (s2 < 0) continue;
          const int p = pp[k];
          const double cs = rc[k], sn = rs[k];
          const double x = A[p * ld + j], y = A[s2 * ld + j];
          A[p * ld + j] = j == s2 ? 0.0 : fma(cs, x, -sn * y);
          A[s2 * ld + j] = j == p ? 0.0 : fma(sn, x, cs * y);
        } else {
          const int i = f / np, k = f - i * np;
          const int s2 = pq[k];
          if (s2 < 0) continue;
          const int p = pp[k];
          const double cs = rc[k], sn = rs[k];
          const double x = Vm[i * ld + p], y = Vm[i * ld + s2];
          Vm[i * ld + p] = fma(cs, x, -sn * y);
          Vm[i * ld + s2] = fma(sn, x, cs * y);
        }
      }
      __syncthreads();
    }
    ++sweeps;
  }

  if (!converged) {
    const double nan = __builtin_nan("");
    for (int e = tid; e < qf * qf; e += 256) {
      if (a.V) a.V[(size_t)c * qf * qf + e] = 0.0;
      if (a.samp) a.samp[(size_t)c * qf * qf + e] = 0.0;
    }
    for (int i = tid; i < qf; i += 256) {
      if (a.eig) a.eig[(size_t)c * qf + i] = nan;
      if (a.s) a.s[(size_t)c * qf + i] = nan;
    }
    if (tid == 0) a.status[c] = 1;
    return;
  }

  // ---- 3. order, signs, recipe
  for (int i = tid; i < q; i += 256) ev[i] = A[i * ld + i];
  __syncthreads();
  for (int i = tid; i < q; i += 256) {
    const double d = ev[i];
    int rank = 0;
    for (int j = 0; j < q; ++j) rank += (ev[j] < d) || (ev[j] == d && j < i);
    perm[rank] = i;
    av[rank] = fabs(d);
    double best = 0.0, val = 1.0;
    for (int r = 0; r < q; ++r) {
      const double x = Vm[r * ld + i];
      if (fabs(x) > best) { best = fabs(x); val = x; }
    }
    sg[i] = val < 0.0 ? -1.0 : 1.0;
  }
  __syncthreads();
  for (int k = tid; k < q; k += 256) {
    double amax = 0.0;
    for (int j = 0; j < q; ++j) amax = fmax(amax, av[j]);
    const double cut = a.cutoff * amax;
    double n_eff = (double)q;
    if (cut > 0.0) {
      n_eff = 0.0;
      for (int j = 0; j < q; ++j) n_eff += fmin(av[j] / cut, 1.0);
    }
    sv[k] = a.step_scale * sqrt(a.temperature / n_eff) / sqrt(fmax(av[k], fmax(cut, DBL_MIN)));
    if (a.eig) a.eig[(size_t)c * qf + k] = av[k];
    if (a.s) a.s[(size_t)c * qf + k] = sv[k];
  }
  __syncthreads();
  if constexpr (HELD) {
    // row f_r of the full layout: the reduced row in the first q columns, zeros behind it
    for (int e = tid; e < q * qf; e += 256) {
      const int r = e / qf, k = e - r * qf;
      const size_t at = ((size_t)c * qf + idx[r]) * qf + k;
      double v = 0.0, vs = 0.0;
      if (k < q) {
        const int from = perm[k];
        v = sg[from] * Vm[r * ld + from];
        vs = v * sv[k];
      }
      if (a.V) a.V[at] = v;
      if (a.samp) a.samp[at] = vs;
    }
  } else {
    for (int e = tid; e < qq; e += 256) {
      const int r = e / q, k = e - r * q;
      const int from = perm[k];
      const double v = sg[from] * Vm[r * ld + from];
      if (a.V) a.V[(size_t)c * qq + e] = v;
      if (a.samp) a.samp[(size_t)c * qq + e] = v * sv[k];
    }
  }
#ifdef SBM_AXES_STATUS_CARRIES_SWEEPS
  if (tid == 0) a.status[c] = sweeps << 8;      // developer builds only: the sweep count for the measurements of docs/history.md
#else
  if (tid == 0) a.status[c] = 0;
#endif
}

__global__ void __launch_bounds__(256) k_sampling_axes(sbm_axes_args a) { sampling_axes_body<false>(a, nullptr); }
// held [C][q]: != 0 = the column takes no part.  Static LDS: 192 bytes of the index list + 16 of the waves' counts, which
// the host wrapper adds to the dynamic block before it compares with the workgroup's limit.
__global__ void __launch_bounds__(256) k_sampling_axes_held(sbm_axes_args a, const int32_t* held) { sampling_axes_body<true>(a, held); }

#endif  // SBM_SAMPLING_AXES_HPP
