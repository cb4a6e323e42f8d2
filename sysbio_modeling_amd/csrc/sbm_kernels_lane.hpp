// sbm_kernels_lane.hpp -- the two mappings without a row phase: sbm_sens_kernel (one trajectory per wavefront, lane =
// column of [y | S]) and sbm_state_kernel (one trajectory per lane, state only).
#pragma once
// ---------------------------------------------------------------------------
// "System" policies: what differs between the two mappings
// ---------------------------------------------------------------------------
struct SbmLdsParams {  // [param][lane] image in LDS
  const double* base;
  __device__ __forceinline__ double operator[](int c) const { return base[c * 64]; }
};

// Systems WITHOUT a row phase (everything happens in rhs): the stage phases of the drivers collapse to finish = rhs.
template <class D>
struct SbmNoRowPhase {
  struct Pending {};
  template <class Z>
  __device__ __forceinline__ Pending issue(double, const Z&) const { return Pending{}; }
  __device__ __forceinline__ int eval(const Pending&, double) const { return 0; }
  template <class Z>
  __device__ __forceinline__ void extra_out(int, Z&) const {}
  template <class Z>
  __device__ __forceinline__ void finish(int, double t, const Z& z, Z& dz) const { static_cast<const D*>(this)->rhs(t, z, dz); }
};

// one trajectory per wave; lane = column of [y | S]
template <class M>
struct SensSystem : SbmNoRowPhase<SensSystem<M>> {
  static constexpr int NV = M::NV;
  static constexpr int NVX = M::NV;   // no extra per-lane elements
  static constexpr int NCOL = 1 + M::NK;
  static constexpr int CPL = (NCOL + 63) / 64;
  static constexpr int NCS = CPL;
  __device__ __forceinline__ static constexpr int col_of(int c, int) { return c; }
  static constexpr bool kUniform = true;
  const double* __restrict__ p;  // wave-uniform -> scalar loads
  int lane;

  __device__ __forceinline__ void rhs(double t, const double (&z)[CPL][NV], double (&dz)[CPL][NV]) const {
    double y[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) y[i] = sbm_bcast0(z[0][i]);
    if constexpr (CPL == 1) {
      // fused, row by row: J entries are consumed as they are produced
      M::eval_col(t, y, p, lane - 1, z[0], dz[0]);
    } else {
      double f[NV], jy[M::NJY], jp[M::NJP];
      M::eval_jac(t, y, p, f, jy, jp);
#pragma unroll
      for (int c = 0; c < CPL; ++c) M::apply_col(jy, jp, lane + 64 * c - 1, z[c], dz[c]);
      const bool state_lane = (lane == 0);
#pragma unroll
      for (int i = 0; i < NV; ++i) dz[0][i] = sbm_sel(state_lane, f[i], dz[0][i]);
    }
  }
  // error norm: max over columns of the column's RMS (every column, the state
  // included, individually meets the tolerance -- the CVODES-style sens. test)
  __device__ __forceinline__ float norm(const float (&colsum)[CPL], float /*xsum*/) const {
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) m = fmaxf(m, sbm_nan_to_inf(colsum[c]));
    return sqrtf(sbm_wave_max(m) * (1.0f / NV));   // +inf: the driver rejects the step
  }
  __device__ __forceinline__ double sum(double v) const { return sbm_wave_sum(v); }
};

// one trajectory per lane; state only
template <class M>
struct StateSystem : SbmNoRowPhase<StateSystem<M>> {
  static constexpr int NV = M::NV;
  static constexpr int NVX = M::NV;
  static constexpr int CPL = 1;
  static constexpr int NCS = 1;
  __device__ __forceinline__ static constexpr int col_of(int, int) { return 0; }
  static constexpr bool kUniform = false;
  SbmLdsParams p;

  __device__ __forceinline__ void rhs(double t, const double (&z)[1][NV], double (&dz)[1][NV]) const {
    M::eval_f(t, z[0], p, dz[0]);
  }
  __device__ __forceinline__ float norm(const float (&colsum)[1], float /*xsum*/) const {
    return sqrtf(colsum[0] * (1.0f / NV));
  }
  __device__ __forceinline__ double sum(double v) const { return v; }
};
// (the per-wave system of a large model does not fold the step size: see sbm_fold_step_size, sbm_rk_drivers.hpp)
template <class M>
inline constexpr bool sbm_fold_step_size<SensSystem<M>> = (SensSystem<M>::CPL * M::NV <= 36);

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// Sensitivity kernel.  grid = n_traj blocks of one wave; at ~1 wave per SIMD
// (the stage vectors fill most of the 512-VGPR budget) a CU holds 4 trajectories,
// the chip 1024, so a 4096-vector ensemble is 4 waves of work per SIMD.
template <class M, int METHOD>
__global__ void __launch_bounds__(64) sbm_sens_kernel(sbm_kernel_args a) {
  using Sys = SensSystem<M>;
  constexpr int NV = Sys::NV;
  constexpr int CPL = Sys::CPL;
  constexpr int NK = M::NK;
  if ((int)blockIdx.x >= a.n_traj) return;
  const int traj = sbm_traj_of(a, blockIdx.x);  // wave-uniform
  const int lane = threadIdx.x;

  Sys sys{{}, a.P + (size_t)traj * M::NP, lane};
  const auto [tg, glen] = sbm_grid_window(a, traj);

  double z[CPL][NV];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int col = lane + 64 * c;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double v = 0.0;
      if (col == 0) {
        if (a.y0) v = a.y0[i];
      } else if (col <= NK) {
        if (a.s0) v = a.s0[i * NK + (col - 1)];
      }
      z[c][i] = v;
    }
  }

  double* Yt = a.Y ? a.Y + (size_t)traj * a.n_t * NV : nullptr;
  double* St = a.S ? a.S + (size_t)traj * a.n_t * NV * NK : nullptr;
  auto store = [&](int io, const double (&zz)[CPL][NV]) {
    if (Yt && lane == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) Yt[(size_t)io * NV + i] = zz[0][i];
    }
    if (St) {
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int scol = lane + 64 * c - 1;
        if (scol >= 0 && scol < NK) {
#pragma unroll
          for (int i = 0; i < NV; ++i) St[((size_t)io * NV + i) * NK + scol] = zz[c][i];
        }
      }
    }
  };

  const SbmTrajOut r = sbm_integrate<METHOD>(sys, z, tg, glen, a.opts, store);
  if (lane == 0) sbm_report(a, traj, r.status, r.n_acc, r.n_rej, false);
}

// State-only kernel.  One trajectory per lane, 64 per block.
template <class M, int METHOD>
__global__ void __launch_bounds__(64) sbm_state_kernel(sbm_kernel_args a) {
  using Sys = StateSystem<M>;
  constexpr int NV = Sys::NV;
  constexpr int NP = M::NP;
  __shared__ double p_lds[NP * 64];
  const int lane = threadIdx.x;
  const int traj0 = blockIdx.x * 64;
  const int traj = traj0 + lane;
  const int n_here = min(64, a.n_traj - traj0);

  // coalesced read of the block's 64 x NP parameter slab, transposed into LDS
  const double* Pb = a.P + (size_t)traj0 * NP;
  for (int e = lane; e < n_here * NP; e += 64) {
    const int tl = e / NP, c = e - tl * NP;
    p_lds[c * 64 + tl] = Pb[e];
  }
  __syncthreads();
  if (traj >= a.n_traj) return;

  Sys sys{{}, SbmLdsParams{p_lds + lane}};
  // By hand, not sbm_grid_window / sbm_integrate / sbm_report: with them this kernel is scheduled differently in every
  // model, and for dense20_50 / DOPRI45 private_segment_fixed_size goes 340 -> 356 (vgpr_spill_count 98 -> 94).
  const int goff = a.grid_off ? a.grid_off[traj] : 0;
  const int glen = a.grid_len ? a.grid_len[traj] : a.n_t;
  const double* tg = a.t_out + goff;

  double z[1][NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) z[0][i] = a.y0 ? a.y0[i] : 0.0;

  double* Yt = a.Y + (size_t)traj * a.n_t * NV;
  auto store = [&](int io, const double (&zz)[1][NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) Yt[(size_t)io * NV + i] = zz[0][i];
  };

  SbmTrajOut r;
  if (METHOD == SBM_DOPRI45) r = sbm_dopri45(sys, z, tg, glen, a.opts, store);
  else r = sbm_rk4(sys, z, tg, glen, a.opts, store);

  if (a.status) a.status[traj] = r.status;
  if (a.n_steps) a.n_steps[traj] = r.n_acc;
  if (a.n_reject) a.n_reject[traj] = r.n_rej;
}
