// sbm_kernels_rowlane.hpp -- the kernels that evaluate the right-hand side by row class with ONE row per lane or segment
// lane: sbm_sens_rowlane_kernel, sbm_state_rows_kernel and the two packed kernels (several trajectories per wavefront).
#pragma once
// ===========================================================================
// Row-lane sensitivity kernel: SIMD across isomorphic equations.
//
// Still one trajectory per wavefront and one sensitivity column per lane (lane j owns column j
// of S, all NV rows, every Runge-Kutta stage in VGPRs).  What changes is who evaluates the part
// of the right-hand side that is identical for all columns.  The per-wave kernel (sbm_kernels_lane.hpp) computes
// f, J_y and J_p on all 64 lanes from broadcast operands, then every lane picks "its" J_p entry
// with v_cndmask chains: rocprofv3 shows it VALU-issue bound (one wave per SIMD issues one
// instruction per ~4 cycles whatever its type) with ~60 % of the instructions spent there.
// Here
//   * the state itself lives one component per lane (lane i integrates y_i as an extra
//     element next to its column), so publishing a stage state is ONE ds_write per lane;
//   * rows with the same kinetic form (emit_rowlane.py) are evaluated together, lane i
//     computing f_i and the J_y / J_p entries of row i from per-lane operands (its parameters
//     sit in registers for the whole kernel, its state operands come from LDS by index);
//   * each row lane drops its J_y entries into a list and its J_p entries into the additive
//     matrix A[NV][64] in LDS, and every column lane then evaluates the same
//     dz_i = sum_m J_y[i,m] z_m + A[i][lane]  -- J_y broadcast reads, A one column per lane
//     (conflict-free), no selects, no readfirstlane.
// Only wave-local ordering is needed (a 64-thread workgroup): no cross-wave barrier anywhere.
// ===========================================================================
template <class M>
struct SbmRowLaneShared {
  double Y[64];                 // stage state, one component per row lane
  double A[M::NV * 64 + 2];     // A[i][c] = J_p[i][c]; zero where J_p is structurally zero
};

template <class M>
struct RowLaneSystem {
  static constexpr int NV = M::NV;
  static constexpr int NVX = M::NV + 1;  // column rows + this lane's own state component
  static constexpr int CPL = 1;
  static constexpr int NCS = 1;
  __device__ __forceinline__ static constexpr int col_of(int, int) { return 0; }
  SbmRowLaneShared<M>* sh;
  int lane;
  SbmRowTable<M, 1> rows;        // this lane's row: class, operand indices, parameters
  int apos[M::RL_MAXJP];         // where this row's J_p entries go in A
  double sj[M::RL_NSTATIC > 0 ? M::RL_NSTATIC : 1];  // parameter-only J_y entries, wave-uniform

  // LDS traffic of ONE wave is processed in issue order, so a ds_read issued after a ds_write of
  // another lane sees that write: no barrier and no waitcnt is needed between the phases below,
  // only a compiler-level fence (SBM_LDS_FENCE) that keeps the memory operations in program order.
  struct Token {
    double f;                  // derivative of this lane's state component
    double jy[M::RL_MAXJY];    // J_y entries of this lane's row (read by the other lanes via v_readlane)
  };
  using Pending = typename SbmRowTable<M, 1>::Operands;   // the row's state operands, in flight from LDS
  // issue: publish this lane's stage state and start fetching the operands of the lane's row
  __device__ __forceinline__ Pending issue(double /*t*/, const double (&z)[1][NVX]) const {
    return rows.exchange(sh->Y, lane, &z[0][NV]);
  }
  // eval: evaluate the lane's row and publish its J_p entries
  __device__ __forceinline__ Token eval(const Pending& p, double t) const {
    Token k;
    double jp[M::RL_MAXJP];
    // Own copy of sbm_row_eval (jy lives in the token): with the shared one sbm_sens_rowlane_kernel<cascade20, DOP853>
    // goes from vgpr_spill_count 317 to 331 and private_segment_fixed_size 512 to 560.
    k.f = 0.0;
#pragma unroll
    for (int s = 0; s < M::RL_MAXJY; ++s) k.jy[s] = 0.0;
#pragma unroll
    for (int s = 0; s < M::RL_MAXJP; ++s) jp[s] = 0.0;
    M::class_dispatch(rows.cls[0], t, p.ys[0], rows.ps[0], k.f, k.jy, jp);
    k.f = rows.cls[0] >= 0 ? k.f : 0.0;   // lanes without a row come out of the select chain with the last class's value
    SBM_LDS_FENCE();
#pragma unroll
    for (int s = 0; s < M::RL_MAXJP; ++s) sh->A[apos[s]] = jp[s];
    SBM_LDS_FENCE();
    return k;
  }
  // phase 2: the lane's column, dz = J_y z + A[:, lane]
  __device__ __forceinline__ void finish(const Token& k, double /*t*/, const double (&z)[1][NVX],
                                         double (&dz)[1][NVX]) const {
    double zc[NV], dc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) zc[i] = z[0][i];
    // A[:, lane] is fetched here rather than in begin(): holding 2*NV more registers across the
    // column rows costs more (AGPR traffic) than the exposed LDS latency (measured 12.8 vs 13.3 ms)
    double acol[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acol[i] = sh->A[i * 64 + lane];
    SBM_LDS_FENCE();
    M::apply_rowlane(k.jy, sj, acol, zc, dc);
#pragma unroll
    for (int i = 0; i < NV; ++i) dz[0][i] = dc[i];
  }
  __device__ __forceinline__ void extra_out(const Token& k, double (&dz)[1][NVX]) const { dz[0][NV] = k.f; }
  __device__ __forceinline__ void rhs(double t, const double (&z)[1][NVX], double (&dz)[1][NVX]) const {
    const Token k = eval(issue(t, z), t);
    extra_out(k, dz);
    finish(k, t, z, dz);
  }
  // max( RMS of the state error, max over columns of the column RMS ): the same test as the
  // per-wave kernel, with the state spread over the lanes
  __device__ __forceinline__ float norm(const float (&colsum)[1], float xsum) const {
    // lanes without a column / without a row carry no equation: they must not steer the controller
    const float m = (lane < M::NK) ? sbm_nan_to_inf(colsum[0]) : 0.f;
    const float x = (lane < NV) ? sbm_nan_to_inf(xsum) : 0.f;
    const float mx = sbm_wave_max(m);
    const float xs = sbm_wave_sumf(x);
    return sqrtf(fmaxf(mx, xs) * (1.0f / NV));   // +inf: the driver rejects the step
  }
  __device__ __forceinline__ double sum(double v) const { return sbm_wave_sum(v); }
};

template <class M, int METHOD>
__global__ void __launch_bounds__(64) sbm_sens_rowlane_kernel(sbm_kernel_args a) {
  using Sys = RowLaneSystem<M>;
  constexpr int NV = M::NV;
  constexpr int NVX = NV + 1;
  constexpr int NK = M::NK;
  static_assert(NV <= 64 && NK <= 64, "row-lane kernel: one row and one column per lane");
  __shared__ SbmRowLaneShared<M> sh;
  if ((int)blockIdx.x >= a.n_traj) return;
  const int traj = sbm_traj_of(a, blockIdx.x);
  const int lane = threadIdx.x;

  for (int i = lane; i < NV * 64 + 2; i += 64) sh.A[i] = 0.0;
  sh.Y[lane] = 0.0;

  Sys sys;
  sys.sh = &sh;
  sys.lane = lane;
  const bool has_row = lane < NV;
  const int row = has_row ? lane : 0;
  SBM_ROW_TABLE_LOAD(M, sys.rows, 0, a.P + (size_t)traj * M::NP, row, has_row, 0)
#pragma unroll
  for (int s = 0; s < M::RL_MAXJP; ++s) sys.apos[s] = has_row ? M::rl_apos(s, row) : NV * 64 + 1;
  __syncthreads();
  {  // parameter-only J_y entries: evaluate the rows once (any state will do) and broadcast them
    double ys0[M::RL_MAXYS], f0, jy0[M::RL_MAXJY], jp0[M::RL_MAXJP];
#pragma unroll
    for (int s = 0; s < M::RL_MAXYS; ++s) ys0[s] = 0.0;
    sbm_row_eval<M, false>(sys.rows.cls[0], a.opts.t0, ys0, sys.rows.ps[0], f0, jy0, jp0);
    M::rl_static(jy0, sys.sj);
  }

  const auto [tg, glen] = sbm_grid_window(a, traj);

  double z[1][NVX];
#pragma unroll
  for (int i = 0; i < NV; ++i) z[0][i] = (a.s0 && lane < NK) ? a.s0[i * NK + lane] : 0.0;
  z[0][NV] = (a.y0 && has_row) ? a.y0[lane] : 0.0;

  double* Yt = a.Y ? a.Y + (size_t)traj * a.n_t * NV : nullptr;
  double* St = a.S ? a.S + (size_t)traj * a.n_t * NV * NK : nullptr;
  auto store = [&](int io, const double (&zz)[1][NVX]) {
    if (Yt && has_row) Yt[(size_t)io * NV + lane] = zz[0][NV];
    if (St && lane < NK) {
#pragma unroll
      for (int i = 0; i < NV; ++i) St[((size_t)io * NV + i) * NK + lane] = zz[0][i];
    }
  };

  const SbmTrajOut r = sbm_integrate<METHOD>(sys, z, tg, glen, a.opts, store);
  if (lane == 0) sbm_report(a, traj, r.status, r.n_acc, r.n_rej, false);
}

// ===========================================================================
// State-only kernel, one trajectory per wavefront: lane i integrates y_i and evaluates f_i with the
// class bodies of the row-lane form.  The lane-per-trajectory kernel (sbm_kernels_lane.hpp) needs 64 trajectories to
// fill ONE wave: an ensemble of 4096 is 64 waves on a chip with 1024 SIMDs, and the launch takes as
// long as one trajectory's serial chain of ~1400-instruction steps.  Here the same ensemble is 4096
// small waves (a handful of registers each, 8 per SIMD) of ~400-instruction steps.  Past ~64k
// trajectories the chip is full either way and the lane-per-trajectory kernel, which does no
// redundant work, wins again (launcher).
// ===========================================================================
template <class M>
struct StateRowSystem {
  static constexpr int NV = 0;           // no column rows: the lane's state components are the "extra" elements
  static constexpr int RPL = (M::NV + 63) / 64;   // state rows per lane: lane, lane + 64, ...
  static constexpr int NVX = RPL;
  static constexpr int CPL = 1;
  static constexpr int NCS = 1;
  static constexpr bool kUniform = true;
  __device__ __forceinline__ static constexpr int col_of(int, int) { return 0; }
  double* Y;                     // [64 * RPL] in LDS: stage state, one component per (lane, r)
  int lane;
  SbmRowTable<M, RPL> rows;

  using Pending = typename SbmRowTable<M, RPL>::Operands;
  struct Token { double f[RPL]; };
  __device__ __forceinline__ Pending issue(double, const double (&z)[1][NVX]) const { return rows.exchange(Y, lane, z[0]); }
  __device__ __forceinline__ Token eval(const Pending& p, double t) const {
    Token k;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      double jy[M::RL_MAXJY], jp[M::RL_MAXJP];   // dead: the compiler drops the Jacobian arithmetic
      // Own copy of sbm_row_eval: with the shared one sbm_state_rows_kernel<stiff50> comes out scheduled differently
      // (vgpr_count 46 -> 44 for RK4, 59 -> 57 for DOP853, 1230 -> 1231 instructions for DOPRI45; no spills either way).
      k.f[r] = 0.0;
#pragma unroll
      for (int s = 0; s < M::RL_MAXJY; ++s) jy[s] = 0.0;
#pragma unroll
      for (int s = 0; s < M::RL_MAXJP; ++s) jp[s] = 0.0;
      M::class_dispatch(rows.cls[r], t, p.ys[r], rows.ps[r], k.f[r], jy, jp);
      k.f[r] = rows.cls[r] >= 0 ? k.f[r] : 0.0;
    }
    return k;
  }
  __device__ __forceinline__ void extra_out(const Token& k, double (&dz)[1][NVX]) const {
#pragma unroll
    for (int r = 0; r < RPL; ++r) dz[0][r] = k.f[r];
  }
  __device__ __forceinline__ void finish(const Token&, double, const double (&)[1][NVX], double (&)[1][NVX]) const {}
  __device__ __forceinline__ void rhs(double t, const double (&z)[1][NVX], double (&dz)[1][NVX]) const {
    extra_out(eval(issue(t, z), t), dz);
  }
  __device__ __forceinline__ float norm(const float (&)[1], float xsum) const {
    const float x = (lane < M::NV) ? sbm_nan_to_inf(xsum) : 0.f;   // rows beyond NV hold zeros throughout
    return sqrtf(sbm_wave_sumf(x) * (1.0f / M::NV));
  }
  __device__ __forceinline__ double sum(double v) const { return sbm_wave_sum(v); }
};

template <class M, int METHOD>
__global__ void __launch_bounds__(64) sbm_state_rows_kernel(sbm_kernel_args a) {
  using Sys = StateRowSystem<M>;
  constexpr int RPL = Sys::RPL;
  __shared__ double Ysh[64 * RPL];
  if ((int)blockIdx.x >= a.n_traj) return;
  const int traj = blockIdx.x;
  const int lane = threadIdx.x;
  Sys sys;
  sys.Y = Ysh;
  sys.lane = lane;
  const double* P = a.P + (size_t)traj * M::NP;
  double z[1][RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    Ysh[lane + 64 * r] = 0.0;
    const bool has_row = lane + 64 * r < M::NV;
    const int row = has_row ? lane + 64 * r : 0;
    SBM_ROW_TABLE_LOAD(M, sys.rows, r, P, row, has_row, 0)
    z[0][r] = (a.y0 && has_row) ? a.y0[row] : 0.0;
  }
  __syncthreads();
  // By hand, not sbm_grid_window / sbm_report: with them this kernel is scheduled differently in every model, and for
  // dense20_50 and dstiff48 / DOPRI45 sgpr_spill_count goes 4 -> 6.
  const int goff = a.grid_off ? a.grid_off[traj] : 0;
  const int glen = a.grid_len ? a.grid_len[traj] : a.n_t;
  const double* tg = a.t_out + goff;
  double* Yt = a.Y + (size_t)traj * a.n_t * M::NV;
  auto store = [&](int io, const double (&zz)[1][RPL]) {
#pragma unroll
    for (int r = 0; r < RPL; ++r)
      if (lane + 64 * r < M::NV) Yt[(size_t)io * M::NV + lane + 64 * r] = zz[0][r];
  };
  const SbmTrajOut r = sbm_integrate<METHOD>(sys, z, tg, glen, a.opts, store);
  if (lane == 0) {
    if (a.status) a.status[traj] = r.status;
    if (a.n_steps) a.n_steps[traj] = r.n_acc;
    if (a.n_reject) a.n_reject[traj] = r.n_rej;
  }
}

// ===========================================================================
// Packed state-rows kernel: several trajectories per wavefront.
//
// A model with few state variables leaves most lanes of the state-rows kernel idle (cascade20: 20 of 64), and
// with thousands of trajectories the kernel is bound by instruction issue, not latency: every wavefront costs
// the same issue slots whether 20 or 60 of its lanes carry equations.  Here a wavefront is cut into 64 / SEG
// segments of SEG = 16 or 32 lanes, one trajectory each (lane i of a segment = state component i).  The
// segments share the instruction stream but not the control flow: each trajectory has its own time, step size
// and accept / reject decisions (per-lane values, uniform within a segment), so the wavefront runs until its
// slowest segment is done and a rejected step of one segment idles the others for one evaluation -- a few per
// cent.  Reductions stay inside a segment: DPP within rows of 16, one ds_bpermute across the two rows of a
// 32-lane segment (the fixed-step method reduces nothing and packs segments of any multiple of four lanes).  LDS exchange of the stage state is per segment (operand indices offset by the segment base).
// Used from 2048 trajectories on (below that the chip is not full and the unpacked kernel has the lower latency).
// ===========================================================================
// Sum over the lanes of a segment, the SAME BITS in every lane: the result steers the step size, and lanes of one
// trajectory that disagree in the last bit drift apart in time (measured: 3e-4 relative error with a rotation-based
// reduction whose lanes add the same numbers in different orders).  Every level is an exchange between two lanes that
// both form own + other -- commutative, hence identical: quad_perm (xor 1, xor 2), row_half_mirror (i <-> 7 - i),
// row_mirror (i <-> 15 - i) on DPP, the two rows of a 32-lane segment through ds_bpermute.
// (SEG 4 and 8 -- the levels guarded by SEG >= 8 / >= 16 -- serve sbm_sens_packed_kernel further down, next to sbm_seg_maxf_any)
template <int SEG>
__device__ __forceinline__ float sbm_seg_sumf_any(float v) {
  v += sbm_dpp<0xb1, 0xf>(v);                              // quad_perm:[1,0,3,2]
  v += sbm_dpp<0x4e, 0xf>(v);                              // quad_perm:[2,3,0,1]
  if constexpr (SEG >= 8) v += sbm_dpp<0x141, 0xf>(v);     // row_half_mirror
  if constexpr (SEG >= 16) v += sbm_dpp<0x140, 0xf>(v);    // row_mirror: every lane of the row of 16 holds the row's sum
  if constexpr (SEG == 32) v += __shfl_xor(v, 16, 64);
  return v;
}
template <int SEG>
__device__ __forceinline__ double sbm_seg_sum(double v) {
#pragma unroll
  for (int off = SEG / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);   // stays inside the aligned segment
  return v;
}

template <class M, int SEG>
struct PackedStateRowSystem {
  static constexpr int NV = 0;           // no column rows: the lane's state component is the "extra" element
  static constexpr int NVX = 1;
  static constexpr int CPL = 1;
  static constexpr int NCS = 1;
  static constexpr bool kUniform = false;
  __device__ __forceinline__ static constexpr int col_of(int, int) { return 0; }
  static constexpr bool kDpp = (SEG == 16 || SEG == 32);   // the widths the segment reductions exist for
  double* Y;                     // [64] in LDS: stage state, segment by segment
  int lane;
  bool has_row;
  SbmRowTable<M, 1> rows;

  using Pending = typename SbmRowTable<M, 1>::Operands;
  struct Token { double f; };
  __device__ __forceinline__ Pending issue(double, const double (&z)[1][1]) const { return rows.exchange(Y, lane, z[0]); }
  __device__ __forceinline__ Token eval(const Pending& p, double t) const {
    Token k;
    double jy[M::RL_MAXJY], jp[M::RL_MAXJP];   // dead: the compiler drops the Jacobian arithmetic
    // Own copy of sbm_row_eval: with the shared one sbm_state_packed_kernel<dense20_10 / dense20_25, DOPRI45 and DOP853>
    // is scheduled differently (1251 / 1537 and 1345 / 1669 instructions, all metadata unchanged).
    k.f = 0.0;
#pragma unroll
    for (int s = 0; s < M::RL_MAXJY; ++s) jy[s] = 0.0;
#pragma unroll
    for (int s = 0; s < M::RL_MAXJP; ++s) jp[s] = 0.0;
    M::class_dispatch(rows.cls[0], t, p.ys[0], rows.ps[0], k.f, jy, jp);
    k.f = rows.cls[0] >= 0 ? k.f : 0.0;
    return k;
  }
  __device__ __forceinline__ void extra_out(const Token& k, double (&dz)[1][1]) const { dz[0][0] = k.f; }
  __device__ __forceinline__ void finish(const Token&, double, const double (&)[1][1], double (&)[1][1]) const {}
  __device__ __forceinline__ void rhs(double t, const double (&z)[1][1], double (&dz)[1][1]) const {
    extra_out(eval(issue(t, z), t), dz);
  }
  // (only the adaptive driver reduces: fixed-step runs may use any segment width)
  __device__ __forceinline__ float norm(const float (&)[1], float xsum) const {
    static_assert(kDpp, "segment reductions: widths 16 and 32");
    const float x = has_row ? sbm_nan_to_inf(xsum) : 0.f;
    return sqrtf(sbm_seg_sumf_any<SEG>(x) * (1.0f / M::NV));
  }
  __device__ __forceinline__ double sum(double v) const {
    static_assert(kDpp, "segment reductions: widths 16 and 32");
    return sbm_seg_sum<SEG>(v);
  }
};

template <class M, int METHOD, int SEG>
__global__ void __launch_bounds__(64) sbm_state_packed_kernel(sbm_kernel_args a) {
  using Sys = PackedStateRowSystem<M, SEG>;
  static_assert(SEG >= 4 && SEG <= 32 && SEG % 4 == 0 && M::NV <= SEG, "one state component per lane of a segment");
  constexpr int TPW = 64 / SEG;          // trajectories per wavefront (lanes beyond TPW * SEG idle along with the last one)
  __shared__ double Ysh[64];
  const int lane = threadIdx.x;
  const int seg = lane / SEG < TPW ? lane / SEG : TPW - 1;
  const int li = lane - seg * SEG;               // >= SEG on the idle tail lanes
  const int traj_raw = (int)blockIdx.x * TPW + seg;
  const bool live = traj_raw < a.n_traj && li < SEG;   // segments beyond the batch integrate a copy of the last trajectory
  const int traj = traj_raw < a.n_traj ? traj_raw : a.n_traj - 1;
  Ysh[lane] = 0.0;
  Sys sys;
  sys.Y = Ysh;
  sys.lane = lane;
  sys.has_row = li < M::NV;
  const int row = sys.has_row ? li : 0;
  SBM_ROW_TABLE_LOAD(M, sys.rows, 0, a.P + (size_t)traj * M::NP, row, sys.has_row, seg * SEG)
  __syncthreads();
  const auto [tg, glen] = sbm_grid_window(a, traj);
  double z[1][1];
  z[0][0] = (a.y0 && sys.has_row) ? a.y0[li] : 0.0;
  double* Yt = a.Y + (size_t)traj * a.n_t * M::NV;
  auto store = [&](int io, const double (&zz)[1][1]) {
    if (sys.has_row && live) Yt[(size_t)io * M::NV + li] = zz[0][0];
  };
  const SbmTrajOut r = sbm_integrate<METHOD>(sys, z, tg, glen, a.opts, store);
  if (li == 0 && live) sbm_report(a, traj, r.status, r.n_acc, r.n_rej, false);
}

// ===========================================================================
// Packed row-lane sensitivity kernel: several trajectories per wavefront, for SMALL models.
//
// The reference's own fixtures have 1 - 2 state variables and 2 - 5 parameters: in the row-lane kernel 3 - 5 of the 64
// lanes carry equations and every trajectory costs a whole wavefront's issue slots.  Here a wavefront is cut into
// 64 / SEG segments of SEG = 4, 8, 16 or 32 lanes (SEG >= n_vars and >= n_sens), one trajectory each: lane li of a
// segment owns sensitivity column li (all NV rows) and state component li.  As in the packed state-only kernel the
// segments share the instruction stream but not the control flow: time, step size and accept / reject decisions are
// per-lane values, uniform within a segment; the controller's reductions stay inside a segment and return the same
// bits in every lane of it (exchange-symmetric DPP / butterfly levels).  A row lane hands its J_y entries to the
// segment's columns through a per-segment LDS table (a lane cannot name "its" row lane by a literal v_readlane index
// when the segment base varies) and its J_p entries through the segment's slice of A.  A trajectory's result does not
// depend on which trajectories share its wavefront (tested bitwise).  Used from 2048 trajectories on
// (SBM_VARIANT_PACKED forces it).
// ===========================================================================
template <int SEG>
__device__ __forceinline__ float sbm_seg_maxf_any(float v) {
  v = fmaxf(v, sbm_dpp<0xb1, 0xf>(v));
  v = fmaxf(v, sbm_dpp<0x4e, 0xf>(v));
  if constexpr (SEG >= 8) v = fmaxf(v, sbm_dpp<0x141, 0xf>(v));
  if constexpr (SEG >= 16) v = fmaxf(v, sbm_dpp<0x140, 0xf>(v));
  if constexpr (SEG == 32) v = fmaxf(v, __shfl_xor(v, 16, 64));
  return v;
}

template <class M, int SEG>
struct SbmPackedSensShared {
  static constexpr int TPW = 64 / SEG;
  double Y[64];                                   // stage state, segment by segment
  double JYL[TPW * M::NV * M::RL_MAXJY + 2];      // [segment][row][slot] (+ spare slot)
  double A[TPW * M::NV * SEG + 2];                // [segment][row][column of the segment] (+ spare slot)
};

template <class M, int SEG>
struct PackedRowLaneSystem {
  static constexpr int NV = M::NV;
  static constexpr int NVX = M::NV + 1;
  static constexpr int CPL = 1;
  static constexpr int NCS = 1;
  static constexpr bool kUniform = false;
  __device__ __forceinline__ static constexpr int col_of(int, int) { return 0; }
  SbmPackedSensShared<M, SEG>* sh;
  int lane, li;
  bool has_row, has_col;
  SbmRowTable<M, 1> rows;
  int jypos[M::RL_MAXJY], apos[M::RL_MAXJP];
  const double* jyl;        // this segment's J_y table
  const double* acolp;      // this lane's column of the segment's A: acolp[i * SEG]

  struct Token { double f; };
  using Pending = typename SbmRowTable<M, 1>::Operands;
  __device__ __forceinline__ Pending issue(double, const double (&z)[1][NVX]) const {
    return rows.exchange(sh->Y, lane, &z[0][NV]);
  }
  __device__ __forceinline__ Token eval(const Pending& p, double t) const {
    Token k;
    double jy[M::RL_MAXJY], jp[M::RL_MAXJP];
    rows.template eval<true>(0, t, p, k.f, jy, jp);
    SBM_LDS_FENCE();
#pragma unroll
    for (int s = 0; s < M::RL_MAXJP; ++s) sh->A[apos[s]] = jp[s];
#pragma unroll
    for (int s = 0; s < M::RL_MAXJY; ++s) sh->JYL[jypos[s]] = jy[s];
    SBM_LDS_FENCE();
    return k;
  }
  __device__ __forceinline__ void finish(const Token&, double, const double (&z)[1][NVX], double (&dz)[1][NVX]) const {
    double zc[NV], dc[NV], acol[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) { zc[i] = z[0][i]; acol[i] = acolp[i * SEG]; }
    SBM_LDS_FENCE();
    M::apply_lds(jyl, acol, zc, dc);
    SBM_LDS_FENCE();
#pragma unroll
    for (int i = 0; i < NV; ++i) dz[0][i] = dc[i];
  }
  __device__ __forceinline__ void extra_out(const Token& k, double (&dz)[1][NVX]) const { dz[0][NV] = k.f; }
  __device__ __forceinline__ void rhs(double t, const double (&z)[1][NVX], double (&dz)[1][NVX]) const {
    const Token k = eval(issue(t, z), t);
    extra_out(k, dz);
    finish(k, t, z, dz);
  }
  __device__ __forceinline__ float norm(const float (&colsum)[1], float xsum) const {
    const float m = has_col ? sbm_nan_to_inf(colsum[0]) : 0.f;
    const float x = has_row ? sbm_nan_to_inf(xsum) : 0.f;
    return sqrtf(fmaxf(sbm_seg_maxf_any<SEG>(m), sbm_seg_sumf_any<SEG>(x)) * (1.0f / NV));
  }
  __device__ __forceinline__ double sum(double v) const { return sbm_seg_sum<SEG>(v); }
};

template <class M, int METHOD, int SEG>
__global__ void __launch_bounds__(64) sbm_sens_packed_kernel(sbm_kernel_args a) {
  using Sys = PackedRowLaneSystem<M, SEG>;
  using Sh = SbmPackedSensShared<M, SEG>;
  constexpr int NV = M::NV, NVX = NV + 1, NK = M::NK, TPW = 64 / SEG;
  static_assert(SEG >= 4 && SEG <= 32 && (SEG & (SEG - 1)) == 0 && NV <= SEG && NK <= SEG, "packed sensitivity kernel: a row and a column per lane of a segment");
  __shared__ Sh sh;
  const int lane = threadIdx.x;
  const int seg = lane / SEG, li = lane - seg * SEG;
  const int traj_raw = (int)blockIdx.x * TPW + seg;
  const bool live = traj_raw < a.n_traj;            // segments beyond the batch integrate a copy of the last trajectory
  const int traj = live ? traj_raw : a.n_traj - 1;
  for (int i = lane; i < TPW * NV * M::RL_MAXJY + 2; i += 64) sh.JYL[i] = 0.0;
  for (int i = lane; i < TPW * NV * SEG + 2; i += 64) sh.A[i] = 0.0;
  sh.Y[lane] = 0.0;

  Sys sys;
  sys.sh = &sh;
  sys.lane = lane;
  sys.li = li;
  sys.has_row = li < NV;
  sys.has_col = li < NK;
  const int row = sys.has_row ? li : 0;
  SBM_ROW_TABLE_LOAD(M, sys.rows, 0, a.P + (size_t)traj * M::NP, row, sys.has_row, seg * SEG)
#pragma unroll
  for (int s = 0; s < M::RL_MAXJY; ++s)
    sys.jypos[s] = (sys.has_row && M::rl_jycol(s, row) >= 0) ? (seg * NV + row) * M::RL_MAXJY + s : TPW * NV * M::RL_MAXJY + 1;
#pragma unroll
  for (int s = 0; s < M::RL_MAXJP; ++s) {
    const int c = M::rl_jpcol(s, row);
    sys.apos[s] = (sys.has_row && c >= 0) ? (seg * NV + row) * SEG + c : TPW * NV * SEG + 1;
  }
  sys.jyl = sh.JYL + seg * NV * M::RL_MAXJY;
  sys.acolp = sh.A + seg * NV * SEG + li;
  __syncthreads();

  const auto [tg, glen] = sbm_grid_window(a, traj);

  double z[1][NVX];
#pragma unroll
  for (int i = 0; i < NV; ++i) z[0][i] = (a.s0 && sys.has_col) ? a.s0[i * NK + li] : 0.0;
  z[0][NV] = (a.y0 && sys.has_row) ? a.y0[li] : 0.0;

  double* Yt = a.Y ? a.Y + (size_t)traj * a.n_t * NV : nullptr;
  double* St = a.S ? a.S + (size_t)traj * a.n_t * NV * NK : nullptr;
  auto store = [&](int io, const double (&zz)[1][NVX]) {
    if (Yt && sys.has_row && live) Yt[(size_t)io * NV + li] = zz[0][NV];
    if (St && sys.has_col && live) {
#pragma unroll
      for (int i = 0; i < NV; ++i) St[((size_t)io * NV + i) * NK + li] = zz[0][i];
    }
  };
  SbmTrajOut r = sbm_integrate<METHOD>(sys, z, tg, glen, a.opts, store);
  if (li == 0 && live) sbm_report(a, traj, r.status, r.n_acc, r.n_rej, false);
}
