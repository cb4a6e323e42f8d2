// sbm_row_operands.hpp -- the row-class contract of the kernels (symbolic/emit_rowlane.py), written once: the row table
// (class, operand indices, parameters of the RPL rows a lane owns; SBM_ROW_TABLE_LOAD), the operand exchange through Y in
// LDS (SbmRowTable::exchange) and the evaluation of one row (sbm_row_eval).  Where J_y / J_p go stays with each kernel.
// Needs the generated model (M) and SBM_LDS_FENCE only: compiles on the host (tests/test_row_operands_host.py).
// A kernel that keeps a copy of one of the pieces says so, with the figures (docs/history.md, "Row operands written once").
#pragma once

// f, jy[], jp[] of a row of class `cls` (-1: no row) from its state operands ys and parameters ps.  SELECT: a lane without
// a row leaves the class select chain with the last class's value; zero its f.  Off where such lanes get all-zero
// operands on which the class bodies vanish (RL_F_ZERO_OFF_ROW), or the caller masks with its own has_row.
template <class M, bool SELECT>
__device__ __forceinline__ void sbm_row_eval(int cls, double t, const double (&ys)[M::RL_MAXYS], const double (&ps)[M::RL_MAXPS],
                                             double& f, double (&jy)[M::RL_MAXJY], double (&jp)[M::RL_MAXJP]) {
  f = 0.0;
#pragma unroll
  for (int s = 0; s < M::RL_MAXJY; ++s) jy[s] = 0.0;
#pragma unroll
  for (int s = 0; s < M::RL_MAXJP; ++s) jp[s] = 0.0;
  M::class_dispatch(cls, t, ys, ps, f, jy, jp);
  if constexpr (SELECT) f = cls >= 0 ? f : 0.0;
}

template <class M, int RPL>
struct SbmRowTable {
  int cls[RPL];                    // class of the row, -1 without one
  int yidx[RPL][M::RL_MAXYS];      // which element of Y feeds operand slot s
  double ps[RPL][M::RL_MAXPS];     // the row's parameters
  struct Operands { double ys[RPL][M::RL_MAXYS]; };   // the rows' state operands (in flight from LDS)

  // RL_F_ZERO_OFF_ROW, a (lane, r) without a row: ps = 0 and every state operand read from `own`, the slot's own place in
  // Y, which only ever receives this slot's state component: 0 from the start, and its derivative is the f in question.
  __device__ __forceinline__ void zero_operands(int r, int own) {
#pragma unroll
    for (int s = 0; s < M::RL_MAXYS; ++s) yidx[r][s] = own;
#pragma unroll
    for (int s = 0; s < M::RL_MAXPS; ++s) ps[r][s] = 0.0;
  }
  // Publish own[r] as element lane + 64 r of Y and gather the operands of the lane's rows.  LDS traffic of ONE wave is
  // processed in issue order, so a ds_read issued after a ds_write of another lane sees that write: no barrier and no
  // waitcnt between the two, only a compiler-level fence that keeps the memory operations in program order.
  __device__ __forceinline__ Operands exchange(double* Y, int lane, const double* own) const {
    Operands p;
#pragma unroll
    for (int r = 0; r < RPL; ++r) Y[lane + 64 * r] = own[r];
    SBM_LDS_FENCE();
#pragma unroll
    for (int r = 0; r < RPL; ++r)
#pragma unroll
      for (int s = 0; s < M::RL_MAXYS; ++s) p.ys[r][s] = Y[yidx[r][s]];
    SBM_LDS_FENCE();
    return p;
  }
  template <bool SELECT>
  __device__ __forceinline__ void eval(int r, double t, const Operands& p, double& f, double (&jy)[M::RL_MAXJY],
                                       double (&jp)[M::RL_MAXJP]) const {
    sbm_row_eval<M, SELECT>(cls[r], t, p.ys[r], ps[r], f, jy, jp);
  }
};

// Row r of `tab` (SbmRowTable<M_, RPL>) := state row `row` of the trajectory with parameters P, if has_row (else the
// caller passes row 0: valid indices, class -1).  ybase: where the trajectory's state begins in Y (the packed kernels'
// segment base).  P is evaluated once, after the class was read.  A macro: as a forced-inline member the same text changes
// the code of every kernel it is used in (cascade20's row-lane kernel / DOP853: vgpr_spill_count 317 -> 325).
#define SBM_ROW_TABLE_LOAD(M_, tab, r, P, row, has_row, ybase)                                                       \
  {                                                                                                                  \
    (tab).cls[r] = (has_row) ? M_::rl_class(row) : -1;                                                               \
    const double* sbm_row_p_ = (P);                                                                                  \
    _Pragma("unroll") for (int s_ = 0; s_ < M_::RL_MAXYS; ++s_) (tab).yidx[r][s_] = M_::rl_ys(s_, row) + (ybase);    \
    _Pragma("unroll") for (int s_ = 0; s_ < M_::RL_MAXPS; ++s_) (tab).ps[r][s_] = sbm_row_p_[M_::rl_ps(s_, row)];    \
  }
