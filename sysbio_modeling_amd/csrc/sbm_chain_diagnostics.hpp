// sbm_chain_diagnostics.hpp -- kernels of sbm_chain_autocorr and sbm_chain_summary (include/sbm.h): convergence
// diagnostics of the Metropolis record values[N][S] (steps slowest, S = C x q series) without reading it back.  What the
// reference's autocorrelation() does per series on the host with an FFT (project/Ensembles.py:14-29), plus the
// integrated autocorrelation time, the effective sample size and split-R-hat that users derive from it.
//
// Three kernels, all on the context's stream:
//   k_chain_autocorr  a series in LDS: constant test, shifted two-pass mean x_0 + mean(x - x_0), the deviations
//                     d = (x - x_0) - mean(x - x_0), half-chain moments, the lag
//                     sums r_k = sum_{i < N-k} d_i d_{i+k}, ac[k] = (r_k / (N-k)) / c_0 with c_0 = r_0 / N
//   k_chain_tau       one wavefront per series: Geyer's initial positive sequence on ac
//   k_chain_summary   one wavefront per parameter: split-R-hat over the 2C half-chains, ess = sum_c N / tau
//
// The normalisation is the reference's: de-meaned, zero-padded (no wrap-around), every lag divided by the number of its
// terms and by lag 0.  Lag 0 is the sum of squares the workgroup makes together; the lane of lag 0 takes that sum instead
// of its own, so ac[0] is (r_0 / N) / (r_0 / N) = 1 exactly.
//
// Work split of k_chain_autocorr.  N > 1024: one series per workgroup of 1024 threads (N = 16384 = SBM_CHAIN_MAX_STEPS
// is 128 KiB of the CU's 160 KiB).  N <= 1024: G = min(32, 2048 / N rounded down to a power of two) series per workgroup
// of 256 threads, tps = 256 / G threads per series (k_ens_columns packs columns the same way).  Inside a series a thread
// owns R = 5 consecutive lags k0 .. k0 + 4 (k0 = 5 kb, kb the lag block): it keeps the window d[i + k0 .. i + k0 + 4] in
// registers, and per step i reads d[i] (one address for the whole series: a broadcast) and ONE new window element
// d[i + k0 + 5] for five FMAs -- one lane per lag would read as often per FMA and leave the loop LDS-bound.  With KB =
// ceil(K / 5) lag blocks and LB = the power of two >= KB (at most tps), the tps threads are LB lag blocks x tps / LB
// slices of the i range; the slices of a lag block are added by a fixed tree through LDS (upper half onto lower half,
// log2 steps).  KB > tps: a thread takes the lag blocks kb, kb + tps, ... in turn.
// At K = 1024: 205 of 256 lag-block slots hold work (four fifths of the lanes).
//
// LDS layout (doubles): [G][ld] the series, ld = N + 10 (packed: rounded up to odd); the 10 slots behind a series are
// zero, so the window may run past the end: a product with a term beyond N - 1 is a product with 0, which is the zero
// padding.  Then [5][threads / 2] slices on their way through the tree, [threads / 64] wavefront partials.
//
// LDS banks (ds_read_b64: two groups of 32 lanes, bank = dword address mod 64, so 32 doubles whose indices differ mod 32
// are conflict free; sbm_ensemble_stats.hpp).  The window read of lane l is d[i + 5 (kb0 + l) + 5]: a stride of 5 doubles,
// odd, hence 32 different residues mod 32 -- no conflict.  That is why R is 5 and not 4 (stride 4: four-way) or 8.
// The passes before the lag sums read d[sub], d[sub + tps], ...: consecutive lanes, consecutive doubles.  Packed series
// are filled series-fastest (neighbouring series of a step are neighbours in memory, so the global reads are contiguous):
// with an even ld the G series of a step would fall on G / 2 ... 1 bank pairs, the odd ld spreads them.
//
// Determinism: every sum has a fixed shape (lane-strided partial sums, xor butterfly, wavefront partials in wavefront
// order; the slice tree), nothing is accumulated atomically: the same input gives the same bits.
//
// The compiler pairs the reads of neighbouring doubles into ds_read2_b64 (half the bytes per LDS cycle by the instruction
// table).  Ten single ds_read_b64 per block in an asm statement were measured against it at 4352 series x 16 384 steps:
// 4.92 / 4.95 ms against 4.90 / 4.97 ms at K = 1024, 28.2 against 28.3 ms at K = N -- no difference, so the loop is plain C++.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_chain_autocorr<1024> 56 VGPRs,
// k_chain_autocorr<256> 60 VGPRs, both 58 SGPRs, no scratch, no static LDS; dynamic LDS 151 760 bytes at N = 16384
// (16394 + 2560 + 16 doubles), 24 352 bytes at the most where series are packed (N = 64: 32 x 75 + 640 + 4 doubles).
//
// ess[j] = sum_c N / tau[c][j] adds the chains' effective sizes as if the chains sampled one distribution: it means
// something only where r_hat[j] is close to 1.
//
// The window rule (sbm_geyer_*) is plain C++ and also compiles for the host: tests/support/geyer_window_main.cpp.
#ifndef SBM_CHAIN_DIAGNOSTICS_HPP
#define SBM_CHAIN_DIAGNOSTICS_HPP

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBM_CHAIN_HD __host__ __device__
#else
#define SBM_CHAIN_HD
#endif

#define SBM_CHAIN_FLAG_CONSTANT 1       // min == max: ac and tau are NaN
#define SBM_CHAIN_FLAG_TRUNCATED 2      // no Gamma_m <= 0 within K lags: tau is a lower bound

// ---- Geyer's initial positive sequence: Gamma_m = ac[2m] + ac[2m + 1], M = the first m with Gamma_m <= 0,
//      tau = -1 + 2 sum_{m < M} Gamma_m.  An odd trailing lag is ignored.  No such m among the K / 2 complete pairs: the
//      sum over all of them, *truncated = 1.  A series whose ac is NaN (constant) gives NaN and is not "truncated".
SBM_CHAIN_HD inline double sbm_geyer_gamma(const double* ac, int m) { return ac[2 * m] + ac[2 * m + 1]; }
SBM_CHAIN_HD inline bool sbm_geyer_stops(double gamma) { return gamma <= 0.0; }

// the rule, one term after the other (k_chain_tau finds M by ballot and adds in its own fixed order)
SBM_CHAIN_HD inline double sbm_geyer_tau(const double* ac, int K, int* truncated) {
  const int pairs = K / 2;
  double sum = 0.0;
  int m = 0;
  for (; m < pairs; ++m) {
    const double g = sbm_geyer_gamma(ac, m);
    if (sbm_geyer_stops(g)) break;
    sum += g;
  }
  if (truncated) *truncated = (m == pairs && ac[0] == ac[0]) ? 1 : 0;
  return -1.0 + 2.0 * sum;
}

#if defined(__HIPCC__)

#include "sbm_block_reduce.hpp"

#define SBM_CHAIN_LAGS 5                // R: consecutive lags of a thread; odd (the bank argument above)
#define SBM_CHAIN_PAD (2 * SBM_CHAIN_LAGS)
#define SBM_CHAIN_PACK_SLOTS 2048       // steps of a workgroup that packs series
#define SBM_CHAIN_PACK_MAX 32
#define SBM_CHAIN_WIDE_FROM 1025        // N from which a series has a workgroup of 1024 threads to itself

struct sbm_chain_args {
  const double* values;     // first series of this launch; step i of series s at values[i * step_stride + s]
  int64_t step_stride;
  int32_t n_series;         // series of this launch
  int32_t N, K;
  int32_t G;                // series per workgroup, a power of two
  int32_t ld;               // LDS doubles per series, >= N + SBM_CHAIN_PAD
  double* ac;               // [n_series][K]
  double* moments;          // [n_series][4], nullable
  int32_t* flags;           // [n_series], nullable
};

// doubles of dynamic LDS of k_chain_autocorr<threads>
static inline size_t sbm_chain_lds_doubles(int threads, int G, int ld) {
  return (size_t)G * (size_t)ld + (size_t)SBM_CHAIN_LAGS * (size_t)(threads / 2) + (size_t)(threads / 64);
}

enum { SBM_CHAIN_SUM = 0, SBM_CHAIN_MIN = 1, SBM_CHAIN_MAX = 2 };

template <int kOp>
__device__ __forceinline__ double chain_combine(double v, double o) {
  if (kOp == SBM_CHAIN_SUM) return v + o;
  if (kOp == SBM_CHAIN_MIN) return (o < v || o != o) ? o : v;      // a NaN wins: such a series is not constant
  return (o > v || o != o) ? o : v;
}

// over the tps threads of series g (tps a power of two >= 8, the same for the whole workgroup), the same value on each of
// them: xor butterfly inside the wavefront, then the wavefront partials in wavefront order.  red: [blockDim.x / 64]
template <int kOp>
__device__ __forceinline__ double chain_reduce(double v, int tps, int g, double* red) {
  const int w = tps < 64 ? tps : 64;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    if (off < w) v = chain_combine<kOp>(v, __shfl_xor(v, off, 64));
  if (tps > 64) {
    const int nw = tps >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[g * nw];
    for (int i = 1; i < nw; ++i) v = chain_combine<kOp>(v, red[g * nw + i]);
  }
  return v;
}

template <int kThreads>
__global__ void __launch_bounds__(kThreads) k_chain_autocorr(sbm_chain_args a) {
  extern __shared__ __attribute__((aligned(16))) double s_chain[];
  constexpr int R = SBM_CHAIN_LAGS;
  const int tid = threadIdx.x;
  const int N = a.N, K = a.K, G = a.G, ld = a.ld;
  double* part = s_chain + (size_t)G * ld;           // [R][kThreads / 2]
  double* red = part + R * (kThreads / 2);           // [kThreads / 64]
  const int g_shift = __ffs(G) - 1;
  const int tps = kThreads >> g_shift;               // threads per series
  const int g = tid / tps, sub = tid & (tps - 1);
  const int64_t first = (int64_t)blockIdx.x * G;     // first series of this workgroup
  const bool live = first + g < a.n_series;
  const int64_t s = first + g;
  double* d = s_chain + g * ld;
  const double nan = __builtin_nan("");

  // ---- load, series-fastest; zeros behind every series (and in the series past the last one)
  for (int e = tid; e < G * N; e += kThreads) {
    const int gg = e & (G - 1), i = e >> g_shift;
    double x = 0.0;
    if (first + gg < a.n_series) x = a.values[(size_t)i * (size_t)a.step_stride + (size_t)(first + gg)];
    s_chain[gg * ld + i] = x;
  }
  const int pad = ld - N;
  for (int e = tid; e < G * pad; e += kThreads) s_chain[(e / pad) * ld + N + e % pad] = 0.0;
  __syncthreads();

  // ---- constant test on the values themselves, and the shifted mean m = x_0 + mean(x_i - x_0)
  const double x0 = d[0];
  double mn = x0, mx = x0, s1 = 0.0;
  for (int i = sub; i < N; i += tps) {
    const double x = d[i];
    mn = chain_combine<SBM_CHAIN_MIN>(mn, x);
    mx = chain_combine<SBM_CHAIN_MAX>(mx, x);
    s1 += x - x0;
  }
  mn = chain_reduce<SBM_CHAIN_MIN>(mn, tps, g, red);
  mx = chain_reduce<SBM_CHAIN_MAX>(mx, tps, g, red);
  s1 = chain_reduce<SBM_CHAIN_SUM>(s1, tps, g, red);
  const bool constant = mn == mx;
  // The mean is x_0 + dm0 and stays in these two parts: rounded into one double it would be off by up to half an ulp OF
  // THE MEAN (6e-11 at 1e6), far more than the N u max|x - x_0| of dm0; x_i - x_0 is exact for a series of unit spread
  const double dm0 = s1 / (double)N;
  __syncthreads();                                   // every thread has x_0 before d_0 takes its place
  double s2 = 0.0;
  for (int i = sub; i < N; i += tps) {
    const double di = (d[i] - x0) - dm0;
    d[i] = di;
    s2 = fma(di, di, s2);
  }
  __syncthreads();
  const double r0 = chain_reduce<SBM_CHAIN_SUM>(s2, tps, g, red);
  const double c0 = r0 / (double)N;
  if (sub == 0 && live && a.flags) a.flags[s] = constant ? SBM_CHAIN_FLAG_CONSTANT : 0;

  // ---- moments of the first and of the last n = N / 2 steps: mean x_0 + (dm0 + mean(d)), unbiased variance (n = 1: 0 / 0)
  if (a.moments) {
    const int n = N >> 1;
    for (int h = 0; h < 2; ++h) {
      const double* dh = d + (h ? N - n : 0);
      double sm = 0.0;
      for (int i = sub; i < n; i += tps) sm += dh[i];
      const double dm = chain_reduce<SBM_CHAIN_SUM>(sm, tps, g, red) / (double)n;
      double sv = 0.0;
      for (int i = sub; i < n; i += tps) {
        const double c = dh[i] - dm;
        sv = fma(c, c, sv);
      }
      sv = chain_reduce<SBM_CHAIN_SUM>(sv, tps, g, red);
      if (sub == 0 && live) {
        a.moments[(size_t)s * 4 + 2 * h] = x0 + (dm0 + dm);
        a.moments[(size_t)s * 4 + 2 * h + 1] = sv / (double)(n - 1);
      }
    }
  }

  // ---- lag sums: LB lag blocks x nsplit slices of i
  const int KB = (K + R - 1) / R;
  int LB = 1;
  while (LB < KB && LB < tps) LB <<= 1;
  const int nsplit = tps / LB;                       // a power of two; > 1 only where LB >= KB
  const int lb = sub & (LB - 1), sp = sub / LB;
  const int chunk = (((N + nsplit - 1) / nsplit + R - 1) / R) * R;      // steps of a slice, a multiple of R
  const int trips = nsplit > 1 ? 1 : (KB + LB - 1) / LB;
  for (int t = 0; t < trips; ++t) {
    const int kb = lb + t * LB;
    const bool active = kb < KB;
    const int k0 = kb * R;
    double acc[R];
#pragma unroll
    for (int b = 0; b < R; ++b) acc[b] = 0.0;
    if (active) {
      // i < N - k0 is every term of lag k0; the later lags of the block end sooner, on products with the zeros behind
      // the series.  A slice that ends inside the range ends on a multiple of R, so the R-step body never runs over
      // into the next slice; the one that ends the range runs over by at most R - 1 steps, all of them zeros.
      const int i0 = sp * chunk;
      const int i1 = i0 + chunk < N - k0 ? i0 + chunk : N - k0;
      if (i0 < i1) {
        double w[R];
#pragma unroll
        for (int b = 0; b < R; ++b) w[b] = d[i0 + k0 + b];
        for (int i = i0; i < i1; i += R) {
#pragma unroll
          for (int u = 0; u < R; ++u) {
            const double di = d[i + u];
#pragma unroll
            for (int b = 0; b < R; ++b) acc[b] = fma(di, w[(u + b) % R], acc[b]);
            w[u] = d[i + u + k0 + R];
          }
        }
      }
    }
    for (int h = nsplit >> 1; h >= 1; h >>= 1) {     // (nsplit is the same for the whole workgroup)
      __syncthreads();
      if (sp >= h && sp < 2 * h) {
#pragma unroll
        for (int b = 0; b < R; ++b) part[b * (kThreads / 2) + g * (tps / 2) + (sp - h) * LB + lb] = acc[b];
      }
      __syncthreads();
      if (sp < h) {
#pragma unroll
        for (int b = 0; b < R; ++b) acc[b] += part[b * (kThreads / 2) + g * (tps / 2) + sp * LB + lb];
      }
    }
    if (active && sp == 0 && live) {
#pragma unroll
      for (int b = 0; b < R; ++b) {
        const int k = k0 + b;
        if (k < K) {
          const double r = k == 0 ? r0 : acc[b];
          a.ac[(size_t)s * (size_t)K + (size_t)k] = constant ? nan : (r / (double)(N - k)) / c0;
        }
      }
    }
  }
}

// one wavefront per series
__global__ void __launch_bounds__(256) k_chain_tau(const double* __restrict__ ac, int32_t n_series, int K,
                                                   double* __restrict__ tau, int32_t* __restrict__ flags) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_series) return;
  const double* row = ac + (size_t)s * (size_t)K;
  const int pairs = K / 2;
  double sum = 0.0;
  bool stopped = false;
  for (int m0 = 0; m0 < pairs; m0 += 64) {           // (the same trips for the whole wavefront)
    const int m = m0 + lane;
    const bool in = m < pairs;
    const double gm = in ? sbm_geyer_gamma(row, m) : 0.0;
    const unsigned long long stop = __ballot(in && sbm_geyer_stops(gm));
    if (stop) {
      if (lane < __ffsll(stop) - 1) sum += gm;
      stopped = true;
      break;
    }
    sum += gm;
  }
  sum = wave_sum(sum);
  if (lane == 0) {
    tau[s] = -1.0 + 2.0 * sum;
    if (flags && !stopped && row[0] == row[0]) flags[s] |= SBM_CHAIN_FLAG_TRUNCATED;
  }
}

// one wavefront per parameter j; moments[C * q][4] and tau[C * q] with series s = c q + j
__global__ void __launch_bounds__(256) k_chain_summary(const double* __restrict__ moments, const double* __restrict__ tau, int N,
                                                       int C, int q, double* __restrict__ rhat, double* __restrict__ ess) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= q) return;
  const int n = N >> 1;
  const double H = 2.0 * (double)C;
  const double mu0 = moments[(size_t)j * 4];
  double sv = 0.0, sm = 0.0, se = 0.0;
  int cnt = 0;
  for (int c = lane; c < C; c += 64) {
    const double* mo = moments + ((size_t)c * (size_t)q + (size_t)j) * 4;
    sv += mo[1] + mo[3];
    sm += (mo[0] - mu0) + (mo[2] - mu0);
    const double t = tau[(size_t)c * (size_t)q + (size_t)j];
    if (t == t) {
      se += (double)N / t;
      ++cnt;
    }
  }
  const double W = wave_sum(sv) / H;
  const double dm = wave_sum(sm) / H;
  double sb = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double* mo = moments + ((size_t)c * (size_t)q + (size_t)j) * 4;
    const double e1 = (mo[0] - mu0) - dm, e2 = (mo[2] - mu0) - dm;
    sb = fma(e1, e1, sb);
    sb = fma(e2, e2, sb);
  }
  const double Bn = wave_sum(sb) / (H - 1.0);        // B / n: the variance of the 2C half-chain means
  se = wave_sum(se);
  cnt = __popcll(__ballot(cnt > 0));
  if (lane == 0) {
    const double nan = __builtin_nan("");
    rhat[j] = W == 0.0 ? nan : sqrt((((double)(n - 1) / (double)n) * W + Bn) / W);
    ess[j] = cnt > 0 ? se : nan;
  }
}

#endif  // __HIPCC__
#endif  // SBM_CHAIN_DIAGNOSTICS_HPP
