// sbm_ensemble_stats.hpp -- kernels of sbm_ensemble_stats (include/sbm.h): mean, standard deviation and interpolated order
// statistics over the member axis of values[V][L], members with a status or a non-finite entry left out.  What the
// reference does per trajectory set on the host (project/Ensembles.py:277-308 the NaN filter, :335-361 the statistics).
//
// Three steps, all on the context's stream:
//   k_ens_valid     one wavefront per member: status == 0 and every one of its L entries finite
//   k_ens_compact   one workgroup: the used members' indices in member order, their number n
//   k_ens_columns   the columns: the n values of a column go to LDS (+inf in the slots up to the next power of two), a
//                   bitonic network sorts them, then shifted two-pass mean / sd and the order statistics are read off
// The column kernel reads values[V][L] as it is: 8 bytes per member, L doubles apart (C x 8 bytes where columns are packed).
// Transposing chunks of columns into [columns][V] scratch first, so that a column is one contiguous run, was measured
// slower at the workload shape (12 800 x 4 000: 4.6 ms against 4.0 ms, docs/history.md) and is not kept.
//
// Work split of k_ens_columns.  A column takes P = next power of two >= V slots of 8 bytes.  P >= 2048: one column per
// workgroup of 1024 threads (P = 16384 = SBM_ENSEMBLE_MAX_MEMBERS is 128 KiB of the CU's 160 KiB).  P < 2048: C = min(32,
// 2048 / P) columns per workgroup of 256 threads, 256 / C lanes per column for the sums -- a 64-member ensemble sorts 32
// columns with every lane busy instead of one with 32 of 256.  Inside the kernel only the next power of two >= n is sorted.
//
// LDS banks (ds_read_b64: two groups of 32 lanes, bank = dword address mod 64, so 32 consecutive doubles are conflict
// free).  A compare-exchange stage with partner distance j gives lane i the pair (l, l + j), l = 2 i - (i mod j): for
// j >= 32 the 32 lanes of a group read 32 consecutive doubles twice -- no conflict; for j < 32 they read runs of j doubles
// with gaps of j, 64 doubles end to end: two-way.  Five of the log2(P) stages of every merge are of that kind
// (25 of 105 stages at P = 16384, where each costs a 2 x slower LDS pass).  Columns packed into one workgroup are laid
// out P + 1 doubles apart: LDS is filled column-fastest (what makes the global reads of packed columns contiguous), which
// with a stride of P would put the 32 columns of a member on one bank pair.
//
// Determinism: every sum has a fixed shape (lane-strided partial sums, xor butterfly, wavefront partials added in
// wavefront order), nothing is accumulated atomically.
#ifndef SBM_ENSEMBLE_STATS_HPP
#define SBM_ENSEMBLE_STATS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbm_block_reduce.hpp"

#define SBM_ENS_MAX_LEVELS 64           // quantile levels of one call (they travel as a kernel argument)
#define SBM_ENS_PACK_SLOTS 2048         // slots of a workgroup that packs columns
#define SBM_ENS_PACK_MAX_COLS 32

struct sbm_ens_levels {
  double q[SBM_ENS_MAX_LEVELS];
};

__global__ void __launch_bounds__(256) k_ens_valid(const double* __restrict__ values, const int32_t* __restrict__ status, int V,
                                                   int64_t L, int32_t* __restrict__ flag) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= V) return;
  const double* row = values + (size_t)v * (size_t)L;
  int bad = 0;
  for (int64_t j = lane; j < L; j += 64) bad |= !is_finite(row[j]);
  bad = __any(bad);
  if (lane == 0) flag[v] = (!bad && (status == nullptr || status[v] == 0)) ? 1 : 0;
}

// idx[0 .. n) = the used members in increasing order; thread t owns the members [t per, (t + 1) per)
__global__ void __launch_bounds__(1024) k_ens_compact(const int32_t* __restrict__ flag, int V, int32_t* __restrict__ idx,
                                                      int32_t* __restrict__ n_internal, int32_t* __restrict__ used_out,
                                                      int32_t* __restrict__ n_out) {
  __shared__ int32_t s_scan[1024];
  const int t = threadIdx.x;
  const int per = (V + 1023) / 1024;
  const int lo = t * per < V ? t * per : V, hi = lo + per < V ? lo + per : V;
  int32_t cnt = 0;
  for (int v = lo; v < hi; ++v) cnt += flag[v];
  s_scan[t] = cnt;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int32_t add = t >= off ? s_scan[t - off] : 0;
    __syncthreads();
    s_scan[t] += add;
    __syncthreads();
  }
  int32_t pos = s_scan[t] - cnt;
  for (int v = lo; v < hi; ++v) {
    const int32_t f = flag[v];
    if (f) idx[pos++] = v;
    if (used_out) used_out[v] = f;
  }
  if (t == 1023) {
    n_internal[0] = s_scan[1023];
    if (n_out) n_out[0] = s_scan[1023];
  }
}

struct sbm_ens_cols_args {
  const double* values;     // [V][L]
  const int32_t* idx;       // the used members, [n]
  const int32_t* n_ptr;
  int64_t L;                // columns: doubles between two members in values and between two levels in quant
  int64_t j0;               // first column of this launch
  int32_t n_cols;           // columns of this launch
  int32_t slots;            // P: LDS slots per column the launch was sized for
  int32_t cols_per_block;   // C, a power of two
  int32_t Q;
  double* mean;
  double* sd;
  double* quant;
};

template <int kThreads>
__global__ void __launch_bounds__(kThreads) k_ens_columns(sbm_ens_cols_args a, sbm_ens_levels lv) {
  extern __shared__ double s_col[];      // [C][P + 1] (C > 1) or [P], then [kThreads / 64] wavefront partials
  const int tid = threadIdx.x;
  const int C = a.cols_per_block;
  const int n = a.n_ptr[0] < a.slots ? a.n_ptr[0] : a.slots;      // (n <= V <= slots: the clamp only guards the LDS bounds)
  int P = 1;
  while (P < n) P <<= 1;                 // what is sorted
  const int ld = C > 1 ? a.slots + 1 : a.slots;
  double* red = s_col + (size_t)C * ld;
  const int64_t c_first = (int64_t)blockIdx.x * C;
  const int tpc = kThreads / C;          // lanes per column, a power of two >= 8
  const int my_c = tid / tpc, sub = tid % tpc;
  const bool my_col_live = c_first + my_c < a.n_cols;
  const double inf = __builtin_inf(), nan = __builtin_nan("");

  if (n <= 0) {
    if (sub == 0 && my_col_live) {
      const int64_t j = a.j0 + c_first + my_c;
      if (a.mean) a.mean[j] = nan;
      if (a.sd) a.sd[j] = nan;
    }
    for (int e = tid; e < C * a.Q; e += kThreads) {
      const int c = e % C, qi = e / C;
      if (c_first + c < a.n_cols) a.quant[(size_t)qi * (size_t)a.L + (size_t)(a.j0 + c_first + c)] = nan;
    }
    return;
  }

  // ---- load, column-fastest: neighbouring columns of a member are neighbours in memory
  const int total = C * P;
  for (int e = tid; e < total; e += kThreads) {
    const int c = e & (C - 1), k = e / C;
    double x = inf;
    if (k < n && c_first + c < a.n_cols) x = a.values[(size_t)a.idx[k] * (size_t)a.L + (size_t)(a.j0 + c_first + c)];
    s_col[c * ld + k] = x;
  }
  __syncthreads();

  // ---- bitonic sort of every column, ascending
  const int half = P >> 1;               // compare-exchanges per column and stage (0 for P = 1)
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < C * half; e += kThreads) {
        const int i = e & (half - 1), c = e / half;
        const int l = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        double* col = s_col + c * ld;
        const double x = col[l], y = col[l + j];
        const bool up = (l & k) == 0;
        if (up ? x > y : x < y) {
          col[l] = y;
          col[l + j] = x;
        }
      }
      __syncthreads();
    }
  }

  // ---- mean and sd, shifted by the column's lower median: d = x - shift is exact for a well-conditioned column
  //      (1e8 + 1e-3 noise) and zero for a constant one
  const double* col = s_col + my_c * ld;
  const double shift = col[(n - 1) >> 1];
  const int w = tpc < 64 ? tpc : 64;
  double s1 = 0.0;
  for (int k = sub; k < n; k += tpc) s1 += col[k] - shift;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    if (off < w) s1 += __shfl_xor(s1, off, 64);
  if (tpc > 64) {
    if ((tid & 63) == 0) red[tid >> 6] = s1;
    __syncthreads();
    s1 = 0.0;
    for (int i = 0; i < tpc / 64; ++i) s1 += red[my_c * (tpc / 64) + i];
    __syncthreads();
  }
  const double dm = s1 / (double)n;
  double s2 = 0.0;
  for (int k = sub; k < n; k += tpc) {
    const double d = (col[k] - shift) - dm;
    s2 = fma(d, d, s2);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    if (off < w) s2 += __shfl_xor(s2, off, 64);
  if (tpc > 64) {
    if ((tid & 63) == 0) red[tid >> 6] = s2;
    __syncthreads();
    s2 = 0.0;
    for (int i = 0; i < tpc / 64; ++i) s2 += red[my_c * (tpc / 64) + i];
  }
  if (sub == 0 && my_col_live) {
    const int64_t j = a.j0 + c_first + my_c;
    if (a.mean) a.mean[j] = shift + dm;
    if (a.sd) a.sd[j] = n > 1 ? sqrt(s2 / (double)n) : 0.0;
  }

  // ---- order statistics, numpy's 'linear' rule: idx = q (n - 1), x_(b) + (idx - b) (x_(a) - x_(b))
  for (int e = tid; e < C * a.Q; e += kThreads) {
    const int c = e % C, qi = e / C;
    if (c_first + c >= a.n_cols) continue;
    const double pos = lv.q[qi] * (double)(n - 1);
    const double fb = floor(pos), fa = ceil(pos);
    const double xb = s_col[c * ld + (int)fb];
    double r = xb;
    if (fa != fb) {
      const double xa = s_col[c * ld + (int)fa];
      r = xb + (pos - fb) * (xa - xb);
    }
    a.quant[(size_t)qi * (size_t)a.L + (size_t)(a.j0 + c_first + c)] = r;
  }
}

#endif  // SBM_ENSEMBLE_STATS_HPP
