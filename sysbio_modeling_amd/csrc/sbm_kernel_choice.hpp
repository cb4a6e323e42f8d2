// sbm_kernel_choice.hpp -- which integrator kernel of sbm_integrators.hpp a call runs, and which instantiations a plugin
// contains: plain C++17 on a literal description of the model (no HIP, no model header), so that the decision is checked
// on the host alone (tests/test_kernel_choice_cpu.py).  sbm_launch.hpp fills the description from the model
// (sbm_traits_of<M>) and switches on the answer.
#pragma once
#include "sbm_plugin.h"

// everything the launcher reads from a model M
struct SbmModelTraits {
  int NV, NK, NNZ_JY;
  bool RG_OK;          // M::RG0::RG_OK: the emitter found a split of the rows over lanes that cuts the elements per lane
  int RG_NCH[3];       // column chunks (wavefronts) per trajectory of M::RG0, RG1, RG2
  bool RG1_IS_RG0, RG2_IS_RG0, RG2_IS_RG1;   // layouts that are one type share their instantiations
  bool IMID_FITS, IMAD_FITS;                 // SbmImplicitFits<M>::fixed, ::adaptive
  bool IEX_FITS, IEX_SEQ_FITS;               // SbmIexFits<M>, SbmIexSeqFits<M>
  int IEX_SEQ_KMAX;                          // SbmIexSeqPlan<M>::KMAX
  bool IEX_SEQ_ROT_OK;                       // SbmIexSeqPlan<M>::ROT_OK
  int MFMA_NCH;                              // SbmMfmaPlan<M>::NCH
};

// the kernel family and, for the row-group kernel, its layout
enum SbmKernel {
  SBM_K_NONE = 0,        // no kernel takes the call: hipErrorInvalidConfiguration
  SBM_K_PER_WAVE,        // sbm_sens_kernel
  SBM_K_ROW_LANE,        // sbm_sens_rowlane_kernel
  SBM_K_ROW_GROUP_RG0,   // sbm_sens_rowgroup_kernel<M, M::RG0 / RG1 / RG2>
  SBM_K_ROW_GROUP_RG1,
  SBM_K_ROW_GROUP_RG2,
  SBM_K_MFMA,            // sbm_sens_mfma_kernel
  SBM_K_SENS_PACKED,     // sbm_sens_packed_kernel
  SBM_K_STATE_LANE,      // sbm_state_kernel
  SBM_K_STATE_ROWS,      // sbm_state_rows_kernel
  SBM_K_STATE_PACKED,    // sbm_state_packed_kernel
  SBM_K_IMID,            // sbm_imid_kernel
  SBM_K_IMAD,            // sbm_imid_adaptive_kernel
  SBM_K_IEX,             // sbm_iex_kernel
  SBM_K_IEX_SEQ,         // sbm_iex_seq_kernel<M, false>
  SBM_K_IEX_SEQ_ROT,     // sbm_iex_seq_kernel<M, true>
  SBM_K_COUNT
};
constexpr const char* sbm_kernel_name(int k) {
  constexpr const char* names[SBM_K_COUNT] = {"NONE", "PER_WAVE", "ROW_LANE", "ROW_GROUP_RG0", "ROW_GROUP_RG1", "ROW_GROUP_RG2",
                                              "MFMA", "SENS_PACKED", "STATE_LANE", "STATE_ROWS", "STATE_PACKED", "IMID",
                                              "IMAD", "IEX", "IEX_SEQ", "IEX_SEQ_ROT"};
  return k >= 0 && k < SBM_K_COUNT ? names[k] : "?";
}

struct SbmKernelChoice {
  int kernel;   // SbmKernel
  int method;   // the explicit method the kernel is instantiated for (anything but DOPRI45 / DOP853 runs as RK4); implicit
                // kernels: opts.method as it came
  int seg;      // packed kernels: lanes per trajectory; 0 elsewhere
  int nch;      // column chunks per trajectory: the grid's y extent; more than one: the report arrays are zeroed first
};

// lanes per trajectory of the packed kernels (template arguments of their instantiations)
constexpr int sbm_sens_packed_seg(const SbmModelTraits& t) {
  const int need = t.NV > t.NK ? t.NV : t.NK;
  return need <= 4 ? 4 : (need <= 8 ? 8 : (need <= 16 ? 16 : 32));
}
// DOPRI45 reduces its error norm inside a segment: widths 16 / 32 (DPP).  Segment sums through LDS for
// other widths were tried (20 lanes: three trajectories per wavefront): 0.53 against 0.49 ms -- the LDS
// round trip per step and a third trajectory to wait for cost more than the denser packing gains.
// RK4 reduces nothing: the width is the state variables rounded up to a multiple of four lanes.
constexpr int sbm_state_packed_seg(const SbmModelTraits& t, int method) {
  return method == SBM_RK4_FIXED ? (t.NV + 3) / 4 * 4 : (t.NV <= 16 ? 16 : 32);
}

// Which instantiations a plugin contains (the one place that says so: the launcher instantiates what is true here).
constexpr bool sbm_kernel_built(const SbmModelTraits& t, int kernel, int method) {
  const bool dop853 = method == SBM_DOP853;
  switch (kernel) {
    case SBM_K_PER_WAVE:
      // The per-wave kernel keeps all NV rows of ceil((NK+1)/64) columns on every lane: for a large model that is
      // minutes of compile time for a kernel whose stage vectors live in scratch.  Where the row-group form exists
      // it is not instantiated beyond 4096 sensitivity entries, and opts.variant becomes a no-op for that model.
      // (DOP853: twelve stage vectors, up to 64 elements per lane)
      return !(t.RG_OK && t.NV * (t.NK + 1) > 4096) && (!dop853 || t.NV * ((t.NK + 64) / 64) <= 64);
    case SBM_K_ROW_LANE:
      // one row + one column per lane.  DOP853: twelve stage vectors of NV rows per lane -- beyond ~16 state variables
      // they leave the register file and the kernel runs out of scratch (correct, slow); not built beyond 32
      return t.NV <= 64 && t.NK <= 64 && (!dop853 || t.NV <= 32);
    case SBM_K_ROW_GROUP_RG0:
      // any number of columns (chunks of them), up to four rows per lane.  DOP853: instantiated for its own split (RG2)
      // and the small-batch one (RG1) only
      return t.RG_OK && (!dop853 || t.RG1_IS_RG0 || t.RG2_IS_RG0);
    case SBM_K_ROW_GROUP_RG1:
    case SBM_K_ROW_GROUP_RG2:
      return t.RG_OK;
    case SBM_K_MFMA:          // one state row per lane
      return t.NV <= 64;
    case SBM_K_SENS_PACKED:   // small models: several trajectories per wavefront
      return t.NV <= 32 && t.NK <= 32 && t.NV * (t.NK + 1) <= 256;
    case SBM_K_STATE_LANE:
      // one trajectory per LANE keeps NV stage-vector rows per lane: beyond 64 rows only the rows kernel is built
      // (where there is one); never for the twelve stage vectors of DOP853
      return (t.NV <= 64 || !sbm_kernel_built(t, SBM_K_STATE_ROWS, method)) && !dop853;
    case SBM_K_STATE_ROWS:    // up to four state rows per lane
      return t.NV <= 256;
    case SBM_K_STATE_PACKED:  // several trajectories per wavefront: models of up to 32 state variables
      return t.NV <= 32 && t.NV >= 2;
    case SBM_K_IMID: return t.IMID_FITS;      // see SbmImplicitFits
    case SBM_K_IMAD: return t.IMAD_FITS;
    case SBM_K_IEX: return t.IEX_FITS;
    case SBM_K_IEX_SEQ: return t.IEX_FITS && t.IEX_SEQ_FITS;
    case SBM_K_IEX_SEQ_ROT: return t.IEX_FITS && t.IEX_SEQ_FITS && t.IEX_SEQ_ROT_OK;
    default: return false;
  }
}

// The kernel of a call: `kind` SBM_KIND_*, the caller's options, the size of the batch, whether the call wants
// sensitivities (args.S) and hands in initial ones (args.s0), and the developer switch SBM_IEX_SEQ.  SBM_K_NONE, or a
// kernel for which sbm_kernel_built is true.
constexpr SbmKernelChoice sbm_choose_kernel(const SbmModelTraits& t, int kind, const sbm_integrator_opts& o, int n_traj,
                                            bool has_S, bool has_s0, bool iex_seq_enabled) {
  const int variant = o.variant;
  auto pick = [&t](int kernel, int method, int seg, int nch) {
    return sbm_kernel_built(t, kernel, method) ? SbmKernelChoice{kernel, method, seg, nch} : SbmKernelChoice{SBM_K_NONE, method, 0, 1};
  };
  // ---- implicit methods: one trajectory per wavefront; with sensitivities one wavefront per chunk of 64 columns ----
  const int nch_implicit = has_S ? (t.NK + 63) / 64 : 1;
  if (o.method == SBM_IMPLICIT_EXTRAP) {
    // chain models, order <= 8: sequences side by side + persistent wavefronts (sbm_implicit_extrap_seq.hpp)
    int K = o.step_mult;
    const double rtol = o.rtol > 0.0 ? o.rtol : 1e-8;
    if (K <= 0) K = rtol >= 1e-4 ? 4 : (rtol >= 1e-6 ? 6 : 8);
    if (sbm_kernel_built(t, SBM_K_IEX_SEQ, o.method) && K <= t.IEX_SEQ_KMAX && iex_seq_enabled) {
      // columns held rotated (chain + one J_p entry per column: no select in the column step) unless the caller hands
      // in initial sensitivities, which need not respect the structure
      const bool rot = sbm_kernel_built(t, SBM_K_IEX_SEQ_ROT, o.method) && !has_s0;
      return pick(rot ? SBM_K_IEX_SEQ_ROT : SBM_K_IEX_SEQ, o.method, 0, nch_implicit);
    }
    return pick(SBM_K_IEX, o.method, 0, nch_implicit);
  }
  if (o.method == SBM_IMPLICIT_ADAPTIVE) return pick(SBM_K_IMAD, o.method, 0, nch_implicit);
  if (o.method == SBM_IMPLICIT_MIDPOINT || o.method == SBM_IMPLICIT_MIDPOINT_GRADED) return pick(SBM_K_IMID, o.method, 0, nch_implicit);

  // ---- explicit methods ----
  const int method = (o.method == SBM_DOPRI45 || o.method == SBM_DOP853) ? o.method : SBM_RK4_FIXED;
  const bool dop853 = method == SBM_DOP853;
  if (kind != SBM_KIND_SENS) {
    // Which state-only kernel (measured on cascade20, DOPRI45, scripts/dev_state_big.py): one trajectory per
    // wavefront up to 2047 trajectories (0.2 ms per 1024, lowest latency); several per wavefront from there
    // (0.14 ms per 1024: 0.56 ms at 4096, 3.3 ms at 32768); one trajectory per LANE costs 2.6 - 2.9 ms whatever
    // the batch up to 65536 (one serial chain per lane, 64 of them per wavefront) and wins from ~20000 on --
    // for small models only: beyond 32 state variables its stage vectors leave the register file.
    // (one trajectory per wave until the chip is full of lane-per-trajectory waves anyway)
    const int lane_from = (t.NV <= 32) ? 20480 : 65536;
    // several trajectories per wavefront once the chip is full
    if (sbm_kernel_built(t, SBM_K_STATE_PACKED, method) && n_traj >= 2048 && n_traj < lane_from && variant == SBM_VARIANT_AUTO)
      return pick(SBM_K_STATE_PACKED, method, sbm_state_packed_seg(t, method), 1);
    if (sbm_kernel_built(t, SBM_K_STATE_ROWS, method) &&
        (((n_traj < lane_from || variant == SBM_VARIANT_ROW_LANE || variant == SBM_VARIANT_ROW_GROUP) && variant != SBM_VARIANT_PER_WAVE) ||
         !sbm_kernel_built(t, SBM_K_STATE_LANE, SBM_RK4_FIXED) || dop853))
      return pick(SBM_K_STATE_ROWS, method, 0, 1);
    return pick(SBM_K_STATE_LANE, method, 0, 1);   // (DOP853 with more than 256 state variables: no kernel)
  }
  // J_y S on the matrix cores (sbm_sens_mfma.hpp) costs the same whatever the sparsity of J_y; the scalar kernels cost
  // 2 FMAs per non-zero and column.  Measured on 20-state networks, 4096 vectors, DOPRI45 (bench.py "dense",
  // profiles/r03, scalar / MFMA ms): 40 non-zeros (cascade20, twice the steps) 5.3 / 21.7; 60: 4.0 / 11.1; 120: 9.3 / 11.5;
  // 220: 25.7 / 12.1; 400 (dense): 67.1 / 13.4 -- the matrix cores win from about 35 % density (round 2, one wavefront per
  // SIMD: 45 %).  AUTO takes them from there (a static property of the model: a given model always runs the same
  // kernel); SBM_VARIANT_MFMA forces them.
  const bool mfma_pays = t.NV >= 16 && t.NV <= 64 && (long long)t.NNZ_JY * 100 >= 35LL * t.NV * t.NV;
  // (DOP853 keeps twelve stage vectors alive -- on the matrix-core kernel they leave the register file: built, so that a
  // forced variant answers, but AUTO keeps DOP853 on the row kernels.)  Models beyond one state row per lane fall
  // through to the scalar kernels.
  if ((variant == SBM_VARIANT_MFMA || (mfma_pays && !dop853 && (variant == SBM_VARIANT_AUTO || variant == SBM_VARIANT_SMALL_BATCH))) &&
      sbm_kernel_built(t, SBM_K_MFMA, method))
    return pick(SBM_K_MFMA, method, 0, t.MFMA_NCH);
  // AUTO: small models ALWAYS run packed (round 2 switched at 2048 trajectories: a vector's result then depended on
  // the size of the batch it travelled in -- the shard a rank owns, the subset a lazy-Jacobian fit re-integrates).  One
  // trajectory alone in its wavefront costs what it costs in the unpacked kernels; the single-vector methods of the
  // Python classes ask for SMALL_BATCH and keep the row kernels' lower latency.
  if ((variant == SBM_VARIANT_PACKED || variant == SBM_VARIANT_AUTO) && sbm_kernel_built(t, SBM_K_SENS_PACKED, method))
    return pick(SBM_K_SENS_PACKED, method, sbm_sens_packed_seg(t), 1);
  // the variants that leave the choice among the row kernels to the launcher (a forced MFMA / PACKED whose kernel
  // does not take the model ends up here too)
  const bool row_choice_free = variant == SBM_VARIANT_AUTO || variant == SBM_VARIANT_SMALL_BATCH ||
                               variant == SBM_VARIANT_MFMA || variant == SBM_VARIANT_PACKED;
  // row-group kernel: the row-lane kernel with the rows of a column split over several lanes, when the emitter found a
  // split that cuts the elements per lane; the only one where the per-wave kernel is not built
  if (t.RG_OK && (variant == SBM_VARIANT_ROW_GROUP || row_choice_free || !sbm_kernel_built(t, SBM_K_PER_WAVE, SBM_RK4_FIXED))) {
    // Two splits of the same form (emit_rowgroup.py): RG0 for throughput; RG1 -- more, smaller column chunks,
    // fewer elements per lane -- while all its wavefronts are resident at once (2048: two per SIMD; a wavefront of
    // this split issues ~40 % of the other's instructions per step, so two of them sharing a SIMD still finish a step
    // sooner than one of the other alone): a single parameter vector, a serial optimiser's call, is latency-bound.
    // Opt-in (SBM_VARIANT_SMALL_BATCH: what the single-vector methods of the Python classes ask for): the two
    // splits take different step sequences, and a batch call's rows must not depend on how many rows it has.
    const bool small_batch = !t.RG1_IS_RG0 && variant == SBM_VARIANT_SMALL_BATCH && (long long)n_traj * t.RG_NCH[1] <= 2048;
    // DOP853 keeps twelve stage vectors alive: its own split, planned for smaller shares per lane (RG2)
    const int layout = small_batch ? 1 : (dop853 ? 2 : 0);
    return pick(SBM_K_ROW_GROUP_RG0 + layout, method, 0, t.RG_NCH[layout]);
  }
  // row-lane kernel whenever the model fits one row + one column per lane.  Even when every row is a class of its own
  // it evaluates NCLASS <= NV row bodies per stage where the per-wave kernel evaluates all NV rows on every lane
  // (measured on random networks with 6 and 9 classes of 11 and 17 rows: 1.6x faster than per-wave).  DOP853, under its
  // own size limit: whatever the variant but PER_WAVE.
  const bool rowlane = dop853 ? variant != SBM_VARIANT_PER_WAVE : (variant == SBM_VARIANT_ROW_LANE || row_choice_free);
  if (rowlane && sbm_kernel_built(t, SBM_K_ROW_LANE, method)) return pick(SBM_K_ROW_LANE, method, 0, 1);
  return pick(SBM_K_PER_WAVE, method, 0, 1);
}
