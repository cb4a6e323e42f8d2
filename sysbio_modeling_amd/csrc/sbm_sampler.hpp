// sbm_sampler.hpp -- kernels of the Metropolis sampler's step on the device (project/ensembles.py, sampler='device' and
// 'device_recalc'): scale-factor entropy of the trial simulations (sbm_project_sf_entropy; the quadrature rule itself is
// sbm_sf_quadrature.hpp, which is also compiled for the host), candidate move (sbm_mh_propose; inside a box and with held
// components: sbm_mh_propose_box), and the two acceptance rules (sbm_mh_accept[_ex], sbm_mh_accept_hastings[_ex]).  Between sbm_mh_propose, sbm_residuals_batch, sbm_project_sf_entropy
// and the acceptance no number goes through the host.  Parallel tempering adds one temperature per vector / chain to the
// entropy and to the Metropolis rule (sbm_project_sf_entropy_pt, sbm_mh_accept_pt: the same bodies, the temperature read
// from an array) and the replica-exchange step (sbm_pt_swap).  The host wrappers with the argument checks are in sbm_core.hip.
#ifndef SBM_SAMPLER_HPP
#define SBM_SAMPLER_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbm_block_reduce.hpp"
#include "sbm_sf_quadrature.hpp"

// One workgroup of four wavefronts per vector; wavefront w takes the groups w, w + 4, ...  For a group the rows go along
// the lanes (a = sum s^2 / sigma^2, b = sum s d / sigma^2 by a butterfly), then the panels of the quadrature rule
// (sbm_sf_quadrature.hpp) do: lane l integrates panels l and l + 64 and the wavefront combines the 64 partial
// log-sum-exps.  LDS: the G group values of the vector, summed in group order by one thread, so that the entropy does
// not depend on which wavefront finished first.
//
// Where the temperature of vector v comes from: one number for the launch (sbm_project_sf_entropy, whose wrapper has
// checked it) or one per vector (sbm_project_sf_entropy_pt: the rungs of a temperature ladder; an entry that is not
// positive gives the vector the entropy -inf, as a simulation that is not finite does).  The body below is written once.
struct sf_temperature_one {
  double T;
  __device__ __forceinline__ double of(int) const { return T; }
  __device__ __forceinline__ bool usable(double) const { return true; }
};
struct sf_temperature_each {
  const double* T;   // [V]
  __device__ __forceinline__ double of(int v) const { return T[v]; }
  __device__ __forceinline__ bool usable(double t) const { return t > 0.0 && is_finite(t); }
};

template <class Temperature>
__device__ __forceinline__ void sf_entropy_vector(const double* __restrict__ sims, int R, int G, const double* __restrict__ row_data,
                                                  const double* __restrict__ row_sigma, const int32_t* __restrict__ row_sf,
                                                  const double* __restrict__ sfg_mean, const double* __restrict__ sfg_sigma,
                                                  Temperature from, double* __restrict__ entropy, double* __restrict__ group_entropy,
                                                  double* s_group /* LDS [G] */) {
  const int v = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double temperature = from.of(v);
  const bool t_ok = from.usable(temperature);
  const double* sv = sims + (size_t)v * R;
  for (int k = wave; k < G; k += 4) {
    double a = 0.0, b = 0.0;
    int bad = 0;
    for (int r = lane; r < R; r += 64) {
      const double s = sv[r];
      bad |= !is_finite(s);       // any row of the vector, scale factor or not
      if (row_sf[r] == k) {
        const double w = 1.0 / (row_sigma[r] * row_sigma[r]);
        a = fma(s * s, w, a);
        b = fma(s * row_data[r], w, b);
      }
    }
    a = wave_sum(a);
    b = wave_sum(b);
    bad = __any(bad);
    double alpha = 0.0, c = 0.0, val = -__builtin_inf();
    if (!bad && t_ok && sbm_sfq_params(a, b, sfg_mean[k], temperature, &alpha, &c)) {
      sbm_sfq_plan q;
      sbm_sfq_make_plan(alpha, c, sfg_sigma[k], &q);         // (the same on every lane)
      double m = -__builtin_inf(), sum = 0.0;
      sbm_sfq_add_panel(q, lane, &m, &sum);
      sbm_sfq_add_panel(q, lane + 64, &m, &sum);
      const double mw = wave_max(m);
      const double tot = wave_sum(m > -__builtin_inf() ? sum * exp(m - mw) : 0.0);
      val = mw + log(tot);                                    // (no panel at all: -inf + log 0 = -inf)
    }
    if (lane == 0) {
      s_group[k] = val;
      if (group_entropy) group_entropy[(size_t)v * G + k] = val;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double e = 0.0;
    for (int k = 0; k < G; ++k) e += temperature * s_group[k];
    entropy[v] = (t_ok && e == e) ? e : -__builtin_inf();
  }
}

__global__ void __launch_bounds__(256) k_sf_entropy(const double* __restrict__ sims, int R, int G,
                                                    const double* __restrict__ row_data, const double* __restrict__ row_sigma,
                                                    const int32_t* __restrict__ row_sf, const double* __restrict__ sfg_mean,
                                                    const double* __restrict__ sfg_sigma, double temperature,
                                                    double* __restrict__ entropy, double* __restrict__ group_entropy) {
  extern __shared__ double s_group[];   // [G]
  sf_entropy_vector(sims, R, G, row_data, row_sigma, row_sf, sfg_mean, sfg_sigma, sf_temperature_one{temperature}, entropy,
                    group_entropy, s_group);
}

// The same with the temperature of vector v read from temperature[v] (sbm_project_sf_entropy_pt)
__global__ void __launch_bounds__(256) k_sf_entropy_pt(const double* __restrict__ sims, int R, int G,
                                                       const double* __restrict__ row_data, const double* __restrict__ row_sigma,
                                                       const int32_t* __restrict__ row_sf, const double* __restrict__ sfg_mean,
                                                       const double* __restrict__ sfg_sigma, const double* __restrict__ temperature,
                                                       double* __restrict__ entropy, double* __restrict__ group_entropy) {
  extern __shared__ double s_group[];   // [G]
  sf_entropy_vector(sims, R, G, row_data, row_sigma, row_sf, sfg_mean, sfg_sigma, sf_temperature_each{temperature}, entropy,
                    group_entropy, s_group);
}

// trial = curr + samp z: one thread per (chain, component); samp is one [q][q] matrix or one per chain
__global__ void __launch_bounds__(256) k_mh_propose(const double* __restrict__ curr, const double* __restrict__ samp, int per_chain,
                                                    const double* __restrict__ z, int C, int q, double* __restrict__ trial) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)C * q) return;
  const size_t c = idx / q;
  const int i = (int)(idx % q);
  const double* row = samp + (per_chain ? c * q * q : 0) + (size_t)i * q;
  const double* zc = z + c * q;
  double d = 0.0;
  for (int j = 0; j < q; ++j) d = fma(row[j], zc[j], d);
  trial[idx] = curr[idx] + d;
}

// The candidate move inside a box and with held components (sbm_mh_propose_box).  One wavefront per chain, four chains per
// workgroup; the lanes stride over the components.  A free component is curr_i + sum_j samp_ij z_j by k_mh_propose's chain
// of fmas in k_mh_propose's order (the same bits); a held one is curr_i, no arithmetic.  If any free component is not
// inside [lower, upper] -- a NaN is not -- the whole row becomes curr again, a point that is known to integrate, and
// outside[c] = 1 tells the acceptance kernel (veto) that the chain does not move.  A chain with nothing free has no
// candidate: outside[c] = 1 as well, so that it counts no accepted move.  held, lower / upper nullable.
__global__ void __launch_bounds__(256) k_mh_propose_box(const double* __restrict__ curr, const double* __restrict__ samp, int per_chain,
                                                        const double* __restrict__ z, int C, int q, const int32_t* __restrict__ held,
                                                        const double* __restrict__ lower, const double* __restrict__ upper,
                                                        double* __restrict__ trial, int32_t* __restrict__ outside) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const size_t o1 = (size_t)c * q;
  const double* sc = samp + (per_chain ? o1 * q : 0);
  const double* zc = z + o1;
  int out = 0, moves = 0;
  for (int i = lane; i < q; i += 64) {
    double t = curr[o1 + i];
    if (!(held && held[o1 + i] != 0)) {
      moves = 1;
      const double* row = sc + (size_t)i * q;
      double d = 0.0;
      for (int j = 0; j < q; ++j) d = fma(row[j], zc[j], d);
      t += d;
      const double lo = lower ? lower[o1 + i] : -__builtin_inf(), hi = upper ? upper[o1 + i] : __builtin_inf();
      out |= !(t >= lo && t <= hi);
    }
    trial[o1 + i] = t;
  }
  out = __any(out) || !__any(moves);
  if (out)
    for (int i = lane; i < q; i += 64) trial[o1 + i] = curr[o1 + i];
  if (lane == 0) outside[c] = out ? 1 : 0;
}

// What the two acceptance rules have in common: the chains' state and the trial points
struct sbm_mh_args {
  const double* norms_t;       // [C]
  const int32_t* status_t;     // [C]
  const double* entropy_t;     // [C] nullable
  const double* log_u;         // [C]
  double temperature;
  int C, q;
  const double* trial;         // [C][q]
  double* curr;                // [C][q]    in / out
  double* F_curr;              // [C]       in / out
  int32_t* n_accepted;         // [C]       in / out
  double* ens_slot;            // [C][q]    nullable
  double* ens_F_slot;          // [C]       nullable
  const int32_t* veto;         // [C]       nullable: != 0 = the chain stays, whatever its energy (sbm_mh_propose_box's outside)
};

// free energy of chain c's trial point; false if the chain cannot move there (integration failed, not finite, vetoed)
__device__ __forceinline__ bool mh_trial_energy(const sbm_mh_args& a, int c, double* Ft) {
  *Ft = 0.5 * a.norms_t[c] - (a.entropy_t ? a.entropy_t[c] : 0.0);
  return a.status_t[c] == 0 && is_finite(*Ft) && !(a.veto && a.veto[c] != 0);
}

// the decided move of chain c, by the `nt` threads t = 0 .. nt - 1 that serve the chain: they stride over the q
// components, thread 0 writes the scalars
__device__ __forceinline__ void mh_commit(const sbm_mh_args& a, int c, bool acc, double Ft, double Fc, int t, int nt) {
  for (int i = t; i < a.q; i += nt) {
    const size_t e = (size_t)c * a.q + i;
    const double x = acc ? a.trial[e] : a.curr[e];
    if (acc) a.curr[e] = x;
    if (a.ens_slot) a.ens_slot[e] = x;
  }
  if (t == 0) {
    if (acc) {
      a.F_curr[c] = Ft;
      a.n_accepted[c] += 1;
    }
    if (a.ens_F_slot) a.ens_F_slot[c] = acc ? Ft : Fc;
  }
}

// The Metropolis rule of chain c at the temperature T, by the 64 lanes of its wavefront
__device__ __forceinline__ void mh_metropolis(const sbm_mh_args& a, int c, double T, int lane) {
  const double Fc = a.F_curr[c];
  double Ft;
  const bool acc = mh_trial_energy(a, c, &Ft) && a.log_u[c] < -(Ft - Fc) / T;
  mh_commit(a, c, acc, Ft, Fc, lane, 64);
}

// The Metropolis rule.  One wavefront per chain: every lane reads the chain's scalars and takes the same decision.
__global__ void __launch_bounds__(256) k_mh_accept(sbm_mh_args a) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= a.C) return;
  mh_metropolis(a, c, a.temperature, lane);
}

// The same with one temperature per chain (sbm_mh_accept_pt; a.temperature is not read).  A device array cannot be checked
// by the wrapper, so the kernel does: a chain whose temperature is not positive and finite stays.
__global__ void __launch_bounds__(256) k_mh_accept_pt(sbm_mh_args a, const double* __restrict__ temperature) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= a.C) return;
  const double T = temperature[c];
  // (a NaN bound compares false: the chain stays and the record slots still get its point)
  mh_metropolis(a, c, T > 0.0 && is_finite(T) ? T : __builtin_nan(""), lane);
}

// One replica-exchange step of the temperature ladders (sbm_pt_swap; project/ensembles.py, `temperature=` a ladder with
// `swap_every=`).  The C chains are C / K ladders of K contiguous rungs; this step proposes the pairs (k, k + 1) with
// k % 2 == parity.  The launch shape of k_mh_accept: one wavefront per chain, four per workgroup.  The wavefront of a
// pair's lower chain i decides from the scalars -- every lane the same way -- and then exchanges the rows i and j = i + 1
// with its lanes striding over q; every other wavefront returns.  Pairs are disjoint, so no two wavefronts touch the same
// row, and a chain outside an exchanged pair keeps every bit (the rows move as they are: no arithmetic on them).
struct sbm_pt_swap_args {
  int C, q, K, parity;
  const double* temperature;   // [C]
  const double* F_cross;       // [C] nullable: the energy of chain c's point at its partner's temperature; NULL = F_curr
  const double* log_u;         // [C] read at the lower chain of a pair
  double* curr;                // [C][q]    in / out
  double* F_curr;              // [C]       in / out
  int32_t* n_swapped;          // [C]       in / out, counted at the lower chain
  double* ens_slot;            // [C][q]    nullable
  double* ens_F_slot;          // [C]       nullable
};

__global__ void __launch_bounds__(256) k_pt_swap(sbm_pt_swap_args a) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= a.C) return;
  const int k = i % a.K;
  if ((k & 1) != a.parity || k + 1 >= a.K) return;      // not the lower chain of a pair of this step
  const int j = i + 1;                                   // the same ladder: k + 1 < K and C % K == 0, so j < C
  const double Fi = a.F_curr[i], Fj = a.F_curr[j];
  const double Xi = a.F_cross ? a.F_cross[i] : Fi, Xj = a.F_cross ? a.F_cross[j] : Fj;
  const double bound = (Fi - Xj) / a.temperature[i] + (Fj - Xi) / a.temperature[j];
  if (!(is_finite(Xi) && is_finite(Xj) && a.log_u[i] < bound)) return;
  const size_t oi = (size_t)i * a.q, oj = (size_t)j * a.q;
  for (int e = lane; e < a.q; e += 64) {
    const double xi = a.curr[oi + e], xj = a.curr[oj + e];
    a.curr[oi + e] = xj;
    a.curr[oj + e] = xi;
    if (a.ens_slot) {
      a.ens_slot[oi + e] = xj;
      a.ens_slot[oj + e] = xi;
    }
  }
  if (lane == 0) {
    a.F_curr[i] = Xj;
    a.F_curr[j] = Xi;
    a.n_swapped[i] += 1;
    if (a.ens_F_slot) {
      a.ens_F_slot[i] = Xj;
      a.ens_F_slot[j] = Xi;
    }
  }
}

struct sbm_mh_hastings_args {
  sbm_mh_args mh;
  double *V_curr, *s_curr, *samp_curr;                     // [C][q][q], [C][q], [C][q][q]   in / out
  const double *V_trial, *s_trial, *samp_trial;
  const int32_t* axes_status_t;                            // [C]
};

// The Metropolis-Hastings rule of the sampler's second algorithm, with the candidate density at both ends of the move
// (axes: sbm_sampling_axes.hpp).  One workgroup per chain (there are q^2 axis entries to copy on acceptance); the two
// quadratic forms are strided over the threads and summed in a fixed shape, so every thread takes the same decision.
__global__ void __launch_bounds__(256) k_mh_accept_hastings(sbm_mh_hastings_args a) {
  extern __shared__ __attribute__((aligned(16))) double hs_d[];      // [q] the move
  __shared__ double s_red[4];
  const int c = blockIdx.x, tid = threadIdx.x, q = a.mh.q;
  const size_t o1 = (size_t)c * q, o2 = o1 * q;
  for (int i = tid; i < q; i += 256) hs_d[i] = a.mh.trial[o1 + i] - a.mh.curr[o1 + i];
  __syncthreads();
  // log q(d; V, s) = -0.5 |V^T d / s|^2 - sum log s: forward with the current axes, back (-d) with the trial point's
  double fwd = 0.0, back = 0.0;
  for (int i = tid; i < q; i += 256) {
    double uc = 0.0, ut = 0.0;
    for (int j = 0; j < q; ++j) {
      uc = fma(a.V_curr[o2 + (size_t)j * q + i], hs_d[j], uc);
      ut = fma(a.V_trial[o2 + (size_t)j * q + i], -hs_d[j], ut);
    }
    const double sc = a.s_curr[o1 + i], st = a.s_trial[o1 + i];
    uc /= sc;
    ut /= st;
    fwd += -0.5 * uc * uc - log(sc);
    back += -0.5 * ut * ut - log(st);
  }
  fwd = block_sum(fwd, s_red);
  back = block_sum(back, s_red);
  const double Fc = a.mh.F_curr[c];
  double Ft;
  const bool acc = mh_trial_energy(a.mh, c, &Ft) && a.axes_status_t[c] == 0 &&
                   a.mh.log_u[c] < -(Ft - Fc) / a.mh.temperature + back - fwd;
  __syncthreads();                // every thread has read F_curr and the current axes
  if (acc) {
    for (int i = tid; i < q; i += 256) a.s_curr[o1 + i] = a.s_trial[o1 + i];
    for (int e = tid; e < q * q; e += 256) {
      a.V_curr[o2 + e] = a.V_trial[o2 + e];
      a.samp_curr[o2 + e] = a.samp_trial[o2 + e];
    }
  }
  mh_commit(a.mh, c, acc, Ft, Fc, tid, 256);
}

#endif  // SBM_SAMPLER_HPP
