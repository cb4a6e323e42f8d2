// sbm_wave.hpp -- scalar helpers, the SBM_* macros of the generated model headers and the wave-wide primitives
// (broadcasts, DPP reductions, per-lane picks) every kernel of sbm_integrators.hpp builds on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---------------------------------------------------------------------------
// scalar helpers
// ---------------------------------------------------------------------------
// 1/x: v_rcp_f64 (~24 good bits on gfx950... refined by two Newton steps to < 1 ulp-ish).
// The IEEE division sequence (div_scale/div_fmas/div_fixup) costs about twice as much
// and the RHS of rate-law models is dominated by reciprocals.
#ifndef SBM_RCP_NR
#define SBM_RCP_NR 2
#endif
__device__ __forceinline__ double sbm_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
#pragma unroll
  for (int it = 0; it < SBM_RCP_NR; ++it) {
    const double e = fma(-x, r, 1.0);
    r = fma(e, r, r);
  }
  return r;
}
#define SBM_RCP(x) sbm_rcp(x)
// compiler-level ordering point for memory operations (no instruction): generated code uses it to bound
// how far loads are hoisted
#define SBM_LDS_FENCE() __atomic_signal_fence(__ATOMIC_SEQ_CST)

// J_p[row, scol] picked per lane.  Arguments BY VALUE: the candidates are computed
// unconditionally and this lowers to v_cndmask -- written as a ?: chain over array
// elements hipcc sinks the J_p arithmetic into exec-masked branches (one per non-zero).
__device__ __forceinline__ double sbm_pick(int scol, int c, double v, double otherwise) {
  return scol == c ? v : otherwise;
}
#define SBM_PICK(scol, c, v, otherwise) sbm_pick(scol, c, v, otherwise)
__device__ __forceinline__ double sbm_sel(bool c, double a, double b) { return c ? a : b; }
#define SBM_SEL(c, a, b) sbm_sel(c, a, b)
// max(|a|, |b|) of the DOPRI45 error norm's scale in ONE v_max_f64 with the absolute values as source modifiers.
// fmax(fabs(a), fabs(b)) compiles to two: where an operand is carried round the step loop the compiler first quiets a
// possible signalling NaN with v_max_f64 x, |a|, |a|.  With one NaN operand the instruction returns the other operand
// (a signalling NaN it returns quieted: IEEE mode is on in compute kernels); either way the error estimate of such an
// element is NaN itself and the step is rejected, which is all the controller needs.
__device__ __forceinline__ double sbm_max_abs(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  double m;
  asm("v_max_f64 %0, |%1|, |%2|" : "=v"(m) : "v"(a), "v"(b));
  return m;
#else
  return fmax(fabs(a), fabs(b));
#endif
}
// (col == c ? v : otherwise) for col = lane + 64 * chunk (chunk wave-uniform) and a literal c: the lane mask comes from
// scalar instructions (the inverse of a ballot: s_mov / s_cselect of the literal), the select is the v_cndmask pair alone
__device__ __forceinline__ double sbm_pick_col(int col, int c, double v, double otherwise) {
  const int chunk = __builtin_amdgcn_readfirstlane(col) >> 6;       // lane 0 holds 64 * chunk
  const unsigned long long mask = (c >> 6) == chunk ? (1ull << (c & 63)) : 0ull;
  return __builtin_amdgcn_inverse_ballot_w64(mask) ? v : otherwise;
}
#define SBM_PICK_COL(col, c, v, otherwise) sbm_pick_col(col, c, v, otherwise)
// value of `v` in lane `src` (compile-time constant) as a wave-uniform scalar: two v_readlane_b32
__device__ __forceinline__ double sbm_lane_bcast(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
#define SBM_LANE_BCAST(v, src) sbm_lane_bcast(v, src)

__device__ __forceinline__ double sbm_bcast0(double v) {
  int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float sbm_bcast0f(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
// Wave-wide reductions of the step controller, on DPP (data-parallel primitives: a VALU operand
// taken from another lane of the same row of 16, no LDS crossbar round trip).  The __shfl_xor
// butterflies they replace cost one ds_bpermute + s_waitcnt lgkmcnt(0) per level, ~20 dependent
// LDS round trips per step over the controller's reductions -- at one wave per SIMD nothing
// hides them.  Sequence as in rocPRIM's warp_reduce_dpp: two quad_perms and two row rotations leave
// every lane of a row with the row's result, row_bcast:15 / :31 fold the four rows into lane 63.
// Lanes of rows a row_mask disables read 0: fine for sums and for maxima of values >= 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float sbm_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float sbm_lane63f(float v) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// max over the wave of v >= 0 (NaN-free: callers map NaN to +inf first).  Non-negative floats order as their bit
// patterns do, and an integer max takes the DPP operand itself: one v_max_i32_dpp per level where fmaxf costs a
// v_mov_b32 for the fill, the DPP move, a canonicalising v_max_f32 and the max (6 instead of 30 instructions; the Newton
// loops of the implicit kernels reduce once per iteration).  INT_MIN is the identity the masked-off rows keep.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int sbm_dpp_smax(int x) {
  const int o = __builtin_amdgcn_update_dpp((int)0x80000000, x, CTRL, ROW_MASK, 0xf, false);
  return x > o ? x : o;
}
__device__ __forceinline__ float sbm_wave_max(float v) {
  int x = __float_as_int(v);
  x = sbm_dpp_smax<0xb1, 0xf>(x);    // quad_perm:[1,0,3,2]
  x = sbm_dpp_smax<0x4e, 0xf>(x);    // quad_perm:[2,3,0,1]
  x = sbm_dpp_smax<0x124, 0xf>(x);   // row_ror:4
  x = sbm_dpp_smax<0x128, 0xf>(x);   // row_ror:8
  x = sbm_dpp_smax<0x142, 0xa>(x);   // row_bcast:15 -> rows 1, 3
  x = sbm_dpp_smax<0x143, 0xc>(x);   // row_bcast:31 -> rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(x, 63));
}
__device__ __forceinline__ float sbm_wave_sumf(float v) {
  v += sbm_dpp<0xb1, 0xf>(v);
  v += sbm_dpp<0x4e, 0xf>(v);
  v += sbm_dpp<0x124, 0xf>(v);
  v += sbm_dpp<0x128, 0xf>(v);
  v += sbm_dpp<0x142, 0xa>(v);
  v += sbm_dpp<0x143, 0xc>(v);
  return sbm_lane63f(v);
}
// a failed evaluation (NaN) must surface as a failed step: +inf survives max and sum
__device__ __forceinline__ float sbm_nan_to_inf(float v) { return (v != v) ? __builtin_inff() : v; }
__device__ __forceinline__ double sbm_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return sbm_bcast0(v);
}

// v[lane] of a per-lane array held in registers: a binary select tree over the bits of `lane`.  The
// obvious chain of `lane == i` selects makes the compiler keep N loop-invariant 64-bit lane masks in
// SGPRs (100 of them for N = 50: it spilled them through v_writelane and AGPRs); the tree needs
// log2(N) masks for the same number of selects.
template <int N, int BIT = 0>
__device__ __forceinline__ double sbm_pick_tree(const double (&v)[N], int lane) {
  if constexpr (N == 1) {
    return v[0];
  } else {
    constexpr int H = (N + 1) / 2;
    double t[H];
    const bool odd = ((lane >> BIT) & 1) != 0;
#pragma unroll
    for (int j = 0; j < H; ++j) t[j] = (2 * j + 1 < N) ? sbm_sel(odd, v[2 * j + 1 < N ? 2 * j + 1 : 0], v[2 * j]) : v[2 * j];
    return sbm_pick_tree<H, BIT + 1>(t, lane);
  }
}
