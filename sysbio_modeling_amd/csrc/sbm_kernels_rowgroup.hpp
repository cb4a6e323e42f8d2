// sbm_kernels_rowgroup.hpp -- sbm_sens_rowgroup_kernel: the row-lane kernel with the rows of a column split over G lanes.
#pragma once
// ===========================================================================
// Row-group sensitivity kernel: the row-lane kernel with the rows of a column split over G lanes.
//
// One trajectory per wavefront, as before; the state still lives one component per lane and the
// row lanes still evaluate f / J_y / J_p by class.  What changes is the distribution of S:
// lane (g, c') = g*C + c' owns rows [g*RPG, (g+1)*RPG) of the columns c', c'+C, ... (CPL of them),
// RPG*CPL elements instead of NV.  For the 20-state / 40-parameter cascade that is 14 elements
// on 60 lanes instead of 20 elements on 40 lanes: fewer instructions per step in proportion and a
// Runge-Kutta working set that (nearly) fits the 256 architectural VGPRs, so the v_accvgpr
// traffic of the row-lane kernel goes away.  Price: J_y coefficients are per-lane values now (LDS
// table JYL instead of v_readlane scalars) and terms that cross a group boundary go through an LDS
// halo (emit_rowgroup.py).  Still a 64-thread workgroup: wave-local LDS ordering, no barriers.
//
// Column chunks (L::RG_NCH > 1; L = the layout, M::RG0 or M::RG1): the columns of S are coupled only through the state, so a trajectory with
// more columns than one wavefront can hold in registers is cut into RG_NCH chunks of C*CPL columns;
// blockIdx.y = chunk, each chunk integrates (state, its columns) on its own -- own error norm, own step
// sequence, nothing exchanged.  Chunk 0 stores the state; status / step counts are combined with atomicMax
// (the launcher zeroes them first).
// ===========================================================================
#ifndef SBM_RG_LANE_SPARE
#define SBM_RG_LANE_SPARE 0
#endif
#if SBM_RG_LANE_SPARE
#define SBM_RG_SPARE(lane) (lane)
#else
#define SBM_RG_SPARE(lane) 1
#endif
template <class M, class L>
struct SbmRowGroupShared {
  // JYL rows: G groups of RPG (the last one padded), then one more all-padding group for the idle
  // lanes (>= G*C): nothing is ever written there, it stays zero
  static constexpr int NPAD = L::RG_G * L::RG_RPG;
  static constexpr int NROWS = NPAD + L::RG_RPG;
  static constexpr int LS = L::RG_LS;    // A / H are [local row][lane][cc]; element (i, j) at L::rg_pos(i, j)
  static constexpr int ZPOS = L::RG_RPG * LS;   // a slot of H that stays zero (absent halo terms)
  static constexpr int RPL = (M::NV + 63) / 64;   // state rows per lane (rows lane, lane + 64, ...)
  double Y[64 * RPL];                    // stage state, one component per (row lane, r)
  // (+ one spare slot PER LANE for the lanes without a row / the slots without an entry: 44 idle lanes storing to one
  //  address are a 16-way conflict on every store of the hand-over, round 4's PMC pass)
  alignas(16) double JYL[NROWS * L::RG_JYS + 64];  // J_y coefficients [row][term]
  alignas(16) double A[L::RG_RPG * LS + 64];       // J_p entries; idle / padded slots stay 0
  alignas(16) double H[L::RG_RPG * LS + 4];        // published rows of the stage vector (+ zero slot)
};

// Early hand-over: fetch the lane's A / J_y operands right after the row lanes published them (eval) instead of
// in finish, so that the column rows of the stage vector are formed while they are in flight.  The token carries
// them from eval to finish: 2*(NV + RPG*JYS) more live VGPRs across the stage argument.
//   EARLY         every stage, numbered or not (RK4: 18.0 vs 19.4 ms);
//   EARLY_STAGES  bit s set: stage s of a driver that numbers its stages (sbm_dopri45, 2..7) fetches early; the
//                 unnumbered eval / rhs (first evaluation, reject path) follow EARLY alone.  See SBM_RG_EARLY_STAGES.
#ifndef SBM_RG_KEEP_F_SELECT
#define SBM_RG_KEEP_F_SELECT 0
#endif
template <class M, class L, bool EARLY, unsigned EARLY_STAGES = 0u>
struct RowGroupSystem {
  static constexpr int G = L::RG_G, C = L::RG_C, RPG = L::RG_RPG;
  static constexpr int NV = L::RG_RPG * L::RG_CPL;   // elements of S this lane integrates
  static constexpr int RPL = (M::NV + 63) / 64;      // state rows this lane evaluates: lane, lane + 64, ...
  static constexpr int NVX = NV + RPL;               // + this lane's own state component(s)
  static constexpr int CPL = 1;
  static constexpr int NCS = L::RG_CPL;
  __device__ __forceinline__ static constexpr int col_of(int, int i) { return i / L::RG_RPG; }
  static constexpr int NH = L::RG_NHALO > 0 ? L::RG_NHALO : 1;
  // M::RL_F_ZERO_OFF_ROW (emit_rowlane.py): every class body gives f == 0 exactly, through finite intermediates, when
  // all its operands are 0.  Then a (lane, r) without a row is given ps = 0 and state operands that stay 0 by the
  // kernel, and eval_as needs no select to keep its f at zero (2 v_cndmask_b32 per row evaluation).
  // -DSBM_RG_KEEP_F_SELECT=1: the select everywhere, for A/B builds.
  static constexpr bool kZeroOffRow = M::RL_F_ZERO_OFF_ROW && !SBM_RG_KEEP_F_SELECT;
  SbmRowGroupShared<M, L>* sh;
  int lane, grp, cp;             // lane = grp*C + cp on the active lanes
  int cbase;                     // first column of this wavefront's chunk
  bool active;                   // lane < G*C
  SbmRowTable<M, RPL> rows;
  int jypos[RPL][M::RL_MAXJY];
  int apos[RPL][M::RL_MAXJP];
  const double* a_lane;
  const double* jy_lane;
  double* h_lane;
  int hoff[NH];

  template <bool E>
  struct TokenT {   // E: the operands travel with it
    static constexpr bool kEarly = E;
    double f[RPL];
    double acol[E ? NV : 1], coef[E ? RPG * L::RG_JYS : 1];
  };
  using Token = TokenT<EARLY>;
  using Pending = typename SbmRowTable<M, RPL>::Operands;
  __device__ __forceinline__ Pending issue(double /*t*/, const double (&z)[1][NVX]) const {
    return rows.exchange(sh->Y, lane, &z[0][NV]);
  }
  __device__ __forceinline__ Token eval(const Pending& p, double t) const { return eval_as<EARLY>(p, t); }
  template <int S>
  __device__ __forceinline__ TokenT<EARLY || ((EARLY_STAGES >> S) & 1u)> eval_stage(const Pending& p, double t) const {
    return eval_as<EARLY || ((EARLY_STAGES >> S) & 1u)>(p, t);
  }
  template <bool E>
  __device__ __forceinline__ TokenT<E> eval_as(const Pending& p, double t) const {
    TokenT<E> k;
    double jy[RPL][M::RL_MAXJY], jp[RPL][M::RL_MAXJP];
#pragma unroll
    // Own copy of sbm_row_eval: with the shared one five of cascade20's eight sbm_sens_rowgroup_kernel instantiations are
    // scheduled differently (RG2 / DOP853 3536 -> 3537 instructions; registers, spills and scratch unchanged).
    for (int r = 0; r < RPL; ++r) {
      k.f[r] = 0.0;
#pragma unroll
      for (int s = 0; s < M::RL_MAXJY; ++s) jy[r][s] = 0.0;
#pragma unroll
      for (int s = 0; s < M::RL_MAXJP; ++s) jp[r][s] = 0.0;
      M::class_dispatch(rows.cls[r], t, p.ys[r], rows.ps[r], k.f[r], jy[r], jp[r]);
      // lanes without a row come out of the select chain with the last class's value: zero it, unless the class bodies
      // do that themselves on the all-zero operands such lanes were given (kZeroOffRow)
      if constexpr (!kZeroOffRow) k.f[r] = rows.cls[r] >= 0 ? k.f[r] : 0.0;
    }
    SBM_LDS_FENCE();
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
#pragma unroll
      for (int s = 0; s < M::RL_MAXJP; ++s) sh->A[apos[r][s]] = jp[r][s];
#pragma unroll
      for (int s = 0; s < M::RL_MAXJY; ++s) sh->JYL[jypos[r][s]] = jy[r][s];
    }
    SBM_LDS_FENCE();
    if constexpr (E) {
      L::load_rowgroup(a_lane, jy_lane, k.acol, k.coef);
      SBM_LDS_FENCE();
    }
    return k;
  }
  template <class Tok>
  __device__ __forceinline__ void finish(const Tok& k, double /*t*/, const double (&z)[1][NVX],
                                         double (&dz)[1][NVX]) const {
    double zc[NV], dc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) zc[i] = z[0][i];
    L::publish_rowgroup(h_lane, zc);
    SBM_LDS_FENCE();
    if constexpr (Tok::kEarly) {
      L::apply_rowgroup(k.acol, k.coef, sh->H, hoff, zc, dc);
    } else {
      double acol[NV], coef[RPG * L::RG_JYS];
      L::load_rowgroup(a_lane, jy_lane, acol, coef);
      L::apply_rowgroup(acol, coef, sh->H, hoff, zc, dc);
    }
    SBM_LDS_FENCE();
#pragma unroll
    for (int i = 0; i < NV; ++i) dz[0][i] = dc[i];
  }
  template <class Tok>
  __device__ __forceinline__ void extra_out(const Tok& k, double (&dz)[1][NVX]) const {
#pragma unroll
    for (int r = 0; r < RPL; ++r) dz[0][NV + r] = k.f[r];
  }
  __device__ __forceinline__ void rhs(double t, const double (&z)[1][NVX], double (&dz)[1][NVX]) const {
    const Token k = eval(issue(t, z), t);
    extra_out(k, dz);
    finish(k, t, z, dz);
  }
  // max( RMS of the state error, max over columns of the column RMS ); a column's sum of squares
  // is spread over the G lanes cp, C + cp, ...
  __device__ __forceinline__ float norm(const float (&colsum)[NCS], float xsum) const {
    float m = 0.f;
#pragma unroll
    for (int cc = 0; cc < NCS; ++cc) {
      const float v = active ? sbm_nan_to_inf(colsum[cc]) : 0.f;
      float tot = v;
#pragma unroll
      for (int gg = 1; gg < G; ++gg) {
        int src = lane + gg * C;
        src = src >= G * C ? src - G * C : src;
        tot += __shfl(v, active ? src : lane, 64);
      }
      const bool has_col = active && ((L::RG_NCH > 1 ? cbase : 0) + cp + C * cc < M::NK);
      m = fmaxf(m, has_col ? tot : 0.f);
    }
    const float x = (lane < M::NV) ? sbm_nan_to_inf(xsum) : 0.f;
    const float mx = sbm_wave_max(m);
    const float xs = sbm_wave_sumf(x);
    return sqrtf(fmaxf(mx, xs) * (1.0f / M::NV));   // +inf: the driver rejects the step
  }
  __device__ __forceinline__ double sum(double v) const { return sbm_wave_sum(v); }
};

// the layouts whose DOPRI45 stages fetch early by default (derivation: at SBM_RG_EARLY_DEFAULT below)
template <class M, class L>
constexpr bool sbm_rg_early_fits() {
  constexpr int elems = L::RG_RPG * L::RG_CPL, rpl = (M::NV + 63) / 64;
  return rpl == 1 ? elems <= 14 : (rpl == 2 && elems <= 7);
}

template <class M, class L, int METHOD>
// Two waves per SIMD (256 registers each) when the lane's share of S is small enough for DOPRI45's seven
// stage vectors to fit: 2*(RPG*CPL + 1)*7 + operands <= 256 holds up to 15 elements (cascade20: 14 + 1).
// Larger shares get the whole register file (one wave per SIMD) rather than spill.
#ifndef SBM_RG_MIN_WAVES
#define SBM_RG_MIN_WAVES (METHOD == SBM_DOP853 ? ((L::RG_RPG * L::RG_CPL + (M::NV + 63) / 64 <= 8) ? 2 : 1) \
                          : ((L::RG_RPG * L::RG_CPL + (M::NV + 63) / 64 <= 15 || METHOD == SBM_RK4_FIXED) ? 2 : 1))
#endif
// Which stages of DOPRI45 (bit s = stage s, 2..7) fetch their operands early (RowGroupSystem::eval_stage).
// -DSBM_RG_EARLY_STAGES=<mask> sets it for every layout (0: every stage fetches in finish, the schedule before the
// switch existed); without it the default applies where the layout leaves room for the operands:
//   * Since the running-sum form of sbm_dopri45 seven stage vectors are alive at the peak and five by stage 7, and the
//     14 + 14 operands of cascade20 / RG0 (14 elements + 1 state row, 256 VGPRs, two waves) fit next to them: with
//     any mask the step loop stays free of scratch and vector memory, the loop body at 832 - 833 VALU instructions
//     (837 with mask 0), vgpr_spill_count 24 -> 32, all outside the loop.
//   * The default is stages 2, 3, 4 and 7, the ones with the smaller live set.  In stages 5 and 6 (six and seven
//     stage vectors alive) the compiler answers an early fetch by forming the stage argument ABOVE it, so nothing is
//     covered (VALU instructions between the last operand read and the wait that drains it, mask 0xFC against mask 0:
//     stage 5 4 / 11, stage 6 16 / 26; stages 2, 3, 4, 7 of the default 13 / 2, 7 / 5, 19 / 4, 69 / 4), and pinning
//     the order with __builtin_amdgcn_sched_barrier spills (126 VGPRs, 96 scratch instructions in the loop).
//     MI355X, 4096 vectors, ms per pass: mask 0 and the commit before 8.97 - 9.02, 0x9C 8.84 - 8.96, 0xFC 8.82 -
//     8.92: the two cannot be told apart, so the smaller one ships (docs/history.md, "Stage hand-over").
//   * Counted in the ISA of the zoo plugins and of cascade40 / cascade70 / stiff80 built with mask 0xFC: with ONE
//     state row per lane no layout gains scratch in its loop (cascade20 14 / 3 / 7 elements, cascade40 10 / 5 / 7,
//     stiff50 9 / 7).  With TWO state rows per lane (two row evaluations and their tables alive per stage) the
//     layouts of 6 and 7 elements stay clean (cascade70 / RG2, stiff80 / RG1) and those of 10 and 12 do not:
//     cascade70 / RG0 70 and RG1 39, stiff80 / RG0 34 scratch instructions inside the step loop, none before.
//   * Layouts of more than 14 elements (one wave per SIMD) have not been looked at: off.
#define SBM_RG_EARLY_DEFAULT 0x9Cu
#ifdef SBM_RG_EARLY_STAGES
#define SBM_RG_EARLY_MASK ((unsigned)(SBM_RG_EARLY_STAGES))
#else
#define SBM_RG_EARLY_MASK (sbm_rg_early_fits<M, L>() ? SBM_RG_EARLY_DEFAULT : 0u)
#endif
__global__ void __launch_bounds__(64, SBM_RG_MIN_WAVES) sbm_sens_rowgroup_kernel(sbm_kernel_args a) {
  using Sys = RowGroupSystem<M, L, METHOD == SBM_RK4_FIXED, METHOD == SBM_DOPRI45 ? SBM_RG_EARLY_MASK : 0u>;
  using Sh = SbmRowGroupShared<M, L>;
  constexpr int MNV = M::NV, NK = M::NK;
  constexpr int G = L::RG_G, C = L::RG_C, RPG = L::RG_RPG, CPL = L::RG_CPL;
  constexpr int NE = Sys::NV, NVX = Sys::NVX, NPAD = Sh::NPAD;
  constexpr int NCH = L::RG_NCH;
  constexpr int RPL = Sys::RPL;
  static_assert(G * C <= 64 && C * CPL * NCH >= NK && C * CPL * (NCH - 1) < NK && NPAD >= MNV, "row-group layout");
  __shared__ Sh sh;
  if ((int)blockIdx.x >= a.n_traj) return;
  const int traj = sbm_traj_of(a, blockIdx.x);
  const int lane = threadIdx.x;
  const int chunk = NCH > 1 ? (int)blockIdx.y : 0;
  const int cbase = chunk * (C * CPL);

  constexpr int NROWS = Sh::NROWS;
  constexpr int LS = Sh::LS;
  for (int i = lane; i < RPG * LS + 64; i += 64) sh.A[i] = 0.0;
  for (int i = lane; i < RPG * LS + 4; i += 64) sh.H[i] = 0.0;
  for (int i = lane; i < NROWS * L::RG_JYS + 64; i += 64) sh.JYL[i] = 0.0;
#pragma unroll
  for (int r = 0; r < RPL; ++r) sh.Y[lane + 64 * r] = 0.0;

  Sys sys;
  sys.sh = &sh;
  sys.lane = lane;
  sys.active = lane < G * C;
  sys.grp = sys.active ? lane / C : G;   // idle lanes form the all-padding group: zeros throughout
  sys.cp = lane - sys.grp * C;
  sys.cbase = cbase;
  const double* P = a.P + (size_t)traj * M::NP;
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    const bool has_row = lane + 64 * r < MNV;
    const int row = has_row ? lane + 64 * r : 0;
    SBM_ROW_TABLE_LOAD(M, sys.rows, r, P, row, has_row, 0)
    if constexpr (Sys::kZeroOffRow) {
      if (!has_row) sys.rows.zero_operands(r, lane + 64 * r);
    }
#pragma unroll
    for (int s = 0; s < M::RL_MAXJY; ++s) {
      const int jp_ = L::rg_jypos(s, row);
      sys.jypos[r][s] = (has_row && jp_ < NPAD * L::RG_JYS) ? jp_ : NROWS * L::RG_JYS + SBM_RG_SPARE(lane);   // else: spare slot
    }
#pragma unroll
    for (int s = 0; s < M::RL_MAXJP; ++s) {
      if constexpr (NCH == 1 && RPL == 1) {
        const int ap = M::rl_apos(s, row);                      // row*64 + column; unused slots carry MNV*64
        sys.apos[r][s] = (has_row && ap < MNV * 64) ? L::rg_pos(ap >> 6, ap & 63) : RPG * LS + SBM_RG_SPARE(lane);
      } else {
        const int lc = M::rl_jpcol(s, row) - cbase;             // column within this chunk (unused slots: -1)
        sys.apos[r][s] = (has_row && lc >= 0 && lc < C * CPL && lc + cbase < NK) ? L::rg_pos(row, lc) : RPG * LS + SBM_RG_SPARE(lane);
      }
    }
  }
  sys.a_lane = sh.A + CPL * lane;
  sys.jy_lane = sh.JYL + (sys.grp * RPG) * L::RG_JYS;
  sys.h_lane = sh.H + CPL * lane;
#pragma unroll
  for (int t = 0; t < Sys::NH; ++t) {
    const int src = (L::RG_NHALO > 0 && sys.active) ? L::rg_hsrc(t, sys.grp) : NPAD;   // NPAD: term absent
    sys.hoff[t] = src < NPAD ? L::rg_pos(src, sys.cp) : Sh::ZPOS;
  }
  __syncthreads();

  const auto [tg, glen] = sbm_grid_window(a, traj);

  // element (r, cc) of this lane = S[grp*RPG + r][cp + C*cc]
  double z[1][NVX];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc)
#pragma unroll
    for (int r = 0; r < RPG; ++r) {
      const int grow = sys.grp * RPG + r, col = cbase + sys.cp + C * cc;
      const bool valid = sys.active && grow < MNV && col < NK;
      z[0][r + RPG * cc] = (a.s0 && valid) ? a.s0[grow * NK + col] : 0.0;
    }
#pragma unroll
  for (int r = 0; r < RPL; ++r) z[0][NE + r] = (a.y0 && lane + 64 * r < MNV) ? a.y0[lane + 64 * r] : 0.0;

  double* Yt = a.Y ? a.Y + (size_t)traj * a.n_t * MNV : nullptr;
  double* St = a.S ? a.S + (size_t)traj * a.n_t * MNV * NK : nullptr;
  auto store = [&](int io, const double (&zz)[1][NVX]) {
    if (Yt && chunk == 0) {
#pragma unroll
      for (int r = 0; r < RPL; ++r)
        if (lane + 64 * r < MNV) Yt[(size_t)io * MNV + lane + 64 * r] = zz[0][NE + r];
    }
    if (St) {
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc)
#pragma unroll
        for (int r = 0; r < RPG; ++r) {
          const int grow = sys.grp * RPG + r, col = cbase + sys.cp + C * cc;
          if (sys.active && grow < MNV && col < NK) St[((size_t)io * MNV + grow) * NK + col] = zz[0][r + RPG * cc];
        }
    }
  };

  const SbmTrajOut r = sbm_integrate<METHOD>(sys, z, tg, glen, a.opts, store);
  if (lane == 0) sbm_report(a, traj, r.status, r.n_acc, r.n_rej, NCH > 1);
}
