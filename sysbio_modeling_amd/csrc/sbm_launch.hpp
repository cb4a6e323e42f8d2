// sbm_launch.hpp -- host side of a model plugin: which kernel of sbm_integrators.hpp a call runs, and how it is launched.
// Included last by sbm_integrators.hpp (never on its own).
#pragma once
#include <map>
#include <mutex>
#include <utility>
#include <stdlib.h>
#include <stdio.h>

template <class T>
struct SbmTypeTag { using type = T; };

// ---- scratch of the persistent kernels: one buffer per (device, stream), grown on demand, never shrunk.  Launches on
// one stream run one after the other, so they can share it; two contexts on two streams get one each. ----
struct SbmScratch {
  void* p = nullptr;
  size_t bytes = 0;
  int* counter = nullptr;      // the work counter of a persistent launch (zeroed on the stream before every launch)
};
static hipError_t sbm_scratch_for(hipStream_t stream, size_t need, SbmScratch** out) {
  static std::mutex mu;
  static std::map<std::pair<int, void*>, SbmScratch> table;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  SbmScratch& s = table[std::make_pair(dev, (void*)stream)];
  if (!s.counter) {
    e = hipMalloc((void**)&s.counter, 256);
    if (e != hipSuccess) { s.counter = nullptr; return e; }
  }
  if (s.bytes < need) {
    // work enqueued earlier on this stream may still read the old buffer
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    if (s.p) (void)hipFree(s.p);
    s.p = nullptr;
    s.bytes = 0;
    e = hipMalloc(&s.p, need);
    if (e != hipSuccess) { s.p = nullptr; return e; }
    // zeroed once, on the stream: a first launch sees the same bytes whatever the allocator hands out
    e = hipMemsetAsync(s.p, 0, need, stream);
    if (e != hipSuccess) { (void)hipFree(s.p); s.p = nullptr; return e; }
    s.bytes = need;
  }
  *out = &s;
  return hipSuccess;
}
// how many workgroups of `kernel` the device holds at once (cached per kernel and device)
static hipError_t sbm_resident_blocks(const void* kernel, int block, int* out) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> cache;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(std::make_pair(dev, kernel));
  if (it == cache.end()) {
    int per_cu = 0, cus = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    it = cache.emplace(std::make_pair(dev, kernel), per_cu * cus).first;
  }
  *out = it->second;
  return hipSuccess;
}
// developer A/B switch: SBM_IEX_SEQ=0 runs chain models through sbm_iex_kernel as round 3 did
static bool sbm_iex_seq_enabled() {
  static const bool on = [] { const char* v = getenv("SBM_IEX_SEQ"); return !(v && v[0] == '0'); }();
  return on;
}
// developer switch: SBM_DEBUG_LAUNCH prints the shape of every persistent launch, and names the matrix-core and packed
// sensitivity kernels with their compiled plan when a call runs them (a forced variant the launcher does not accept falls
// through to the row kernels without a word: tests/test_gpu_tile_edges.py reads these lines)
static bool sbm_debug_launch() {
  static const bool on = getenv("SBM_DEBUG_LAUNCH") != nullptr;
  return on;
}
// Column chunks of one trajectory combine status / counts with atomicMax (sbm_report): the arrays start from zero.
static hipError_t sbm_zero_report(const sbm_kernel_args& a, hipStream_t stream) {
  hipError_t e = hipSuccess;
  if (a.status) e = hipMemsetAsync(a.status, 0, sizeof(int32_t) * (size_t)a.n_traj, stream);
  if (e == hipSuccess && a.n_steps) e = hipMemsetAsync(a.n_steps, 0, sizeof(int32_t) * (size_t)a.n_traj, stream);
  if (e == hipSuccess && a.n_reject) e = hipMemsetAsync(a.n_reject, 0, sizeof(int32_t) * (size_t)a.n_traj, stream);
  return e;
}
// f(std::integral_constant<int, METHOD>) for the explicit method of a launch.  A kernel that is not built for a method
// says so with an `if constexpr` inside f.
template <class F>
static int sbm_with_method(int method, F&& f) {
  if (method == SBM_DOPRI45) return f(std::integral_constant<int, SBM_DOPRI45>{});
  if (method == SBM_DOP853) return f(std::integral_constant<int, SBM_DOP853>{});
  return f(std::integral_constant<int, SBM_RK4_FIXED>{});
}

template <class M>
static int sbm_launch_model(int kind, const sbm_kernel_args* args, hipStream_t stream) {
  const sbm_kernel_args a = *args;
  if (a.n_traj <= 0) return (int)hipSuccess;
  if (a.opts.method == SBM_IMPLICIT_EXTRAP) {
    if constexpr (SbmIexFits<M>::value) {
      const int nch = a.S ? (M::NK + 63) / 64 : 1;
      if (nch > 1) {
        const hipError_t e = sbm_zero_report(a, stream);
        if (e != hipSuccess) return (int)e;
      }
      if constexpr (SbmIexSeqFits<M>::value) {
        // chain models, order <= 8: sequences side by side + persistent wavefronts (sbm_implicit_extrap_seq.hpp)
        int K = a.opts.step_mult;
        const double rtol = a.opts.rtol > 0.0 ? a.opts.rtol : 1e-8;
        if (K <= 0) K = rtol >= 1e-4 ? 4 : (rtol >= 1e-6 ? 6 : 8);
        if (K <= SbmIexSeqPlan<M>::KMAX && sbm_iex_seq_enabled()) {
          const int n_work = a.n_traj * nch;
          int resident = 0;
          // columns held rotated (chain + one J_p entry per column: no select in the column step) unless the caller hands
          // in initial sensitivities, which need not respect the structure
          constexpr bool kRot = SbmIexSeqPlan<M>::ROT_OK;
          const bool rot = kRot && a.s0 == nullptr;
          const void* kfn = rot ? (const void*)sbm_iex_seq_kernel<M, kRot> : (const void*)sbm_iex_seq_kernel<M, false>;
          hipError_t e = sbm_resident_blocks(kfn, 64, &resident);
          if (e != hipSuccess) return (int)e;
          const int grid = n_work < resident ? n_work : resident;
          if (sbm_debug_launch()) fprintf(stderr, "sbm_iex_seq_kernel: %d pieces of work, %d resident workgroups, grid %d\n", n_work, resident, grid);
          SbmScratch* sc = nullptr;
          e = sbm_scratch_for(stream, (size_t)grid * SbmIexSeqPlan<M>::BLOCK_DOUBLES * sizeof(double), &sc);
          if (e != hipSuccess) return (int)e;
          e = hipMemsetAsync(sc->counter, 0, sizeof(int), stream);
          if (e != hipSuccess) return (int)e;
          if (rot) hipLaunchKernelGGL((sbm_iex_seq_kernel<M, kRot>), dim3(grid), dim3(64), 0, stream, a, (double*)sc->p, sc->counter, n_work, nch);
          else hipLaunchKernelGGL((sbm_iex_seq_kernel<M, false>), dim3(grid), dim3(64), 0, stream, a, (double*)sc->p, sc->counter, n_work, nch);
          return (int)hipGetLastError();
        }
      }
      hipLaunchKernelGGL((sbm_iex_kernel<M>), dim3(a.n_traj, nch), dim3(64), 0, stream, a);
      return (int)hipGetLastError();
    } else {
      return (int)hipErrorInvalidConfiguration;
    }
  }
  if (a.opts.method == SBM_IMPLICIT_ADAPTIVE) {
    if constexpr (SbmImplicitFits<M>::adaptive) {
      const int nch = a.S ? (M::NK + 63) / 64 : 1;
      if (nch > 1) {
        const hipError_t e = sbm_zero_report(a, stream);
        if (e != hipSuccess) return (int)e;
      }
      hipLaunchKernelGGL((sbm_imid_adaptive_kernel<M>), dim3(a.n_traj, nch), dim3(64), 0, stream, a);
      return (int)hipGetLastError();
    } else {
      return (int)hipErrorInvalidConfiguration;
    }
  }
  if (a.opts.method == SBM_IMPLICIT_MIDPOINT || a.opts.method == SBM_IMPLICIT_MIDPOINT_GRADED) {
    // one trajectory per wave for both kinds (state only: S == NULL skips the column work)
    if constexpr (SbmImplicitFits<M>::fixed) {
      // state only: one wavefront; with sensitivities: one per chunk of 64 columns
      const int nch = a.S ? (M::NK + 63) / 64 : 1;
      hipLaunchKernelGGL((sbm_imid_kernel<M>), dim3(a.n_traj, nch), dim3(64), 0, stream, a);
      return (int)hipGetLastError();
    } else {
      return (int)hipErrorInvalidConfiguration;   // see SbmImplicitFits
    }
  }
  // J_y S on the matrix cores (sbm_sens_mfma.hpp) costs the same whatever the sparsity of J_y; the scalar kernels cost
  // 2 FMAs per non-zero and column.  Measured on 20-state networks, 4096 vectors, DOPRI45 (bench.py "dense",
  // profiles/r03, scalar / MFMA ms): 40 non-zeros (cascade20, twice the steps) 5.3 / 21.7; 60: 4.0 / 11.1; 120: 9.3 / 11.5;
  // 220: 25.7 / 12.1; 400 (dense): 67.1 / 13.4 -- the matrix cores win from about 35 % density (round 2, one wavefront per
  // SIMD: 45 %).  AUTO takes them from there (a static property of the model: a given model always runs the same
  // kernel); SBM_VARIANT_MFMA forces them.
  constexpr bool kMfmaPays = M::NV >= 16 && M::NV <= 64 && (long long)M::NNZ_JY * 100 >= 35LL * M::NV * M::NV;
  // (DOP853 keeps twelve stage vectors alive -- on the matrix-core kernel they leave the register file: built, so that a
  // forced variant answers, but AUTO keeps DOP853 on the row kernels)
  if (kind == SBM_KIND_SENS && (a.opts.variant == SBM_VARIANT_MFMA ||
                                (kMfmaPays && a.opts.method != SBM_DOP853 &&
                                 (a.opts.variant == SBM_VARIANT_AUTO || a.opts.variant == SBM_VARIANT_SMALL_BATCH)))) {
    // models beyond one state row per lane fall through to the scalar kernels
    if constexpr (M::NV <= 64) {
      constexpr int nch = SbmMfmaPlan<M>::NCH;
      if (nch > 1) {
        const hipError_t e = sbm_zero_report(a, stream);
        if (e != hipSuccess) return (int)e;
      }
      if (sbm_debug_launch()) fprintf(stderr, "sbm_sens_mfma_kernel: RT %d CT %d NCH %d LDJ %d LDA %d, %d trajectories\n", SbmMfmaPlan<M>::RT, SbmMfmaPlan<M>::CT, nch, SbmMfmaShared<M, SbmMfmaPlan<M>::CT>::LDJ, SbmMfmaShared<M, SbmMfmaPlan<M>::CT>::LDA, a.n_traj);
      return sbm_with_method(a.opts.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_sens_mfma_kernel<M, decltype(m)::value>), dim3(a.n_traj, nch), dim3(64), 0, stream, a);
        return (int)hipGetLastError();
      });
    }
  }
  // small models: several trajectories per wavefront (sbm_sens_packed_kernel)
  if constexpr (M::NV <= 32 && M::NK <= 32 && M::NV * (M::NK + 1) <= 256) {
    constexpr int need = M::NV > M::NK ? M::NV : M::NK;
    constexpr int SEG = need <= 4 ? 4 : (need <= 8 ? 8 : (need <= 16 ? 16 : 32));
    // AUTO: small models ALWAYS run packed (round 2 switched at 2048 trajectories: a vector's result then depended on
    // the size of the batch it travelled in -- the shard a rank owns, the subset a lazy-Jacobian fit re-integrates).  One
    // trajectory alone in its wavefront costs what it costs in the unpacked kernels; the single-vector methods of the
    // Python classes ask for SMALL_BATCH and keep the row kernels' lower latency.
    if (kind == SBM_KIND_SENS && (a.opts.variant == SBM_VARIANT_PACKED || a.opts.variant == SBM_VARIANT_AUTO)) {
      if (sbm_debug_launch()) fprintf(stderr, "sbm_sens_packed_kernel: SEG %d, %d trajectories, grid %d\n", SEG, a.n_traj, (a.n_traj + 64 / SEG - 1) / (64 / SEG));
      return sbm_with_method(a.opts.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_sens_packed_kernel<M, decltype(m)::value, SEG>), dim3((a.n_traj + 64 / SEG - 1) / (64 / SEG)), dim3(64), 0, stream, a);
        return (int)hipGetLastError();
      });
    }
  }
  if (kind == SBM_KIND_SENS) {
    // row-lane / row-group kernels whenever the model fits one row + one column per lane.  Even when
    // every row is a class of its own they evaluate NCLASS <= NV row bodies per stage where the per-wave
    // kernel evaluates all NV rows on every lane (measured on random networks with 6 and 9 classes of 11
    // and 17 rows: 1.6x faster than per-wave)
    constexpr bool kRowLaneOk = (M::NV <= 64 && M::NK <= 64);
    constexpr bool kRowGroupOk = M::RG0::RG_OK;   // any number of columns (chunks of them), up to four rows per lane
    // The per-wave kernel keeps all NV rows of ceil((NK+1)/64) columns on every lane: for a large model that is
    // minutes of compile time for a kernel whose stage vectors live in scratch.  Where the row-group form exists
    // it is not instantiated beyond 4096 sensitivity entries, and opts.variant becomes a no-op for that model.
    constexpr bool kPerWaveBuilt = !(kRowGroupOk && M::NV * (M::NK + 1) > 4096);
    // the variants that leave the choice among the row kernels to the launcher (a forced MFMA / PACKED whose kernel
    // does not take the model ends up here too)
    const bool row_choice_free = a.opts.variant == SBM_VARIANT_AUTO || a.opts.variant == SBM_VARIANT_SMALL_BATCH ||
                                 a.opts.variant == SBM_VARIANT_MFMA || a.opts.variant == SBM_VARIANT_PACKED;
    const bool rowlane = a.opts.variant == SBM_VARIANT_ROW_LANE || (row_choice_free && kRowLaneOk);
    // row-group kernel: the row-lane kernel with the rows of a column split over several lanes,
    // when the emitter found a split that cuts the elements per lane (M::RG_OK)
    if constexpr (kRowGroupOk) {
      if (a.opts.variant == SBM_VARIANT_ROW_GROUP || row_choice_free || !kPerWaveBuilt) {
        // Two splits of the same form (emit_rowgroup.py): RG0 for throughput; RG1 -- more, smaller column chunks,
        // fewer elements per lane -- while all its wavefronts are resident at once (2048: two per SIMD; a wavefront of
        // this split issues ~40 % of the other's instructions per step, so two of them sharing a SIMD still finish a step
        // sooner than one of the other alone): a single parameter vector, a serial optimiser's call, is latency-bound.
        // Opt-in (SBM_VARIANT_SMALL_BATCH: what the single-vector methods of the Python classes ask for): the two
        // splits take different step sequences, and a batch call's rows must not depend on how many rows it has.
        const bool small_batch = !std::is_same<typename M::RG1, typename M::RG0>::value &&
                                 a.opts.variant == SBM_VARIANT_SMALL_BATCH && (long long)a.n_traj * M::RG1::RG_NCH <= 2048;
        auto go = [&](auto layout_tag) -> int {
          using L = typename decltype(layout_tag)::type;
          if constexpr (L::RG_NCH > 1) {
            const hipError_t e = sbm_zero_report(a, stream);
            if (e != hipSuccess) return (int)e;
          }
          return sbm_with_method(a.opts.method, [&](auto m) {
            constexpr int METHOD = decltype(m)::value;
            // (DOP853: instantiated for its own split and the small-batch one only)
            if constexpr (METHOD != SBM_DOP853 || std::is_same<L, typename M::RG2>::value || std::is_same<L, typename M::RG1>::value) {
              hipLaunchKernelGGL((sbm_sens_rowgroup_kernel<M, L, METHOD>), dim3(a.n_traj, L::RG_NCH), dim3(64), 0, stream, a);
              return (int)hipGetLastError();
            } else {
              return (int)hipErrorInvalidConfiguration;
            }
          });
        };
        // DOP853 keeps twelve stage vectors alive: its own split, planned for smaller shares per lane (RG2)
        if (a.opts.method == SBM_DOP853 && !small_batch) return go(SbmTypeTag<typename M::RG2>{});
        return small_batch ? go(SbmTypeTag<typename M::RG1>{}) : go(SbmTypeTag<typename M::RG0>{});
      }
    }
    if (a.opts.method == SBM_DOP853) {
      // beside the row-group form: the row-lane kernel (twelve stage vectors of NV rows per lane: beyond ~16 state
      // variables they leave the register file and the kernel runs out of scratch -- correct, slow), then the per-wave one
      if constexpr (kRowLaneOk && M::NV <= 32) {
        if (a.opts.variant != SBM_VARIANT_PER_WAVE) {
          hipLaunchKernelGGL((sbm_sens_rowlane_kernel<M, SBM_DOP853>), dim3(a.n_traj), dim3(64), 0, stream, a);
          return (int)hipGetLastError();
        }
      }
      if constexpr (kPerWaveBuilt && M::NV * ((M::NK + 64) / 64) <= 64) {
        hipLaunchKernelGGL((sbm_sens_kernel<M, SBM_DOP853>), dim3(a.n_traj), dim3(64), 0, stream, a);
        return (int)hipGetLastError();
      } else {
        return (int)hipErrorInvalidConfiguration;
      }
    }
    // (DOPRI45 and RK4 from here on: DOP853 has returned above, under its own size limits)
    if constexpr (kRowLaneOk) {
      if (rowlane) {
        return sbm_with_method(a.opts.method, [&](auto m) {
          constexpr int METHOD = decltype(m)::value;
          if constexpr (METHOD == SBM_DOP853) return (int)hipErrorInvalidConfiguration;
          else {
            hipLaunchKernelGGL((sbm_sens_rowlane_kernel<M, METHOD>), dim3(a.n_traj), dim3(64), 0, stream, a);
            return (int)hipGetLastError();
          }
        });
      }
    }
    if constexpr (kPerWaveBuilt) {
      // (as above: DOP853 cannot get here, its branch only keeps sbm_sens_kernel<DOP853> un-instantiated beyond the limit)
      return sbm_with_method(a.opts.method, [&](auto m) {
        constexpr int METHOD = decltype(m)::value;
        if constexpr (METHOD == SBM_DOP853) return (int)hipErrorInvalidConfiguration;
        else {
          hipLaunchKernelGGL((sbm_sens_kernel<M, METHOD>), dim3(a.n_traj), dim3(64), 0, stream, a);
          return (int)hipGetLastError();
        }
      });
    }
  } else {
    // one trajectory per wave until the chip is full of lane-per-trajectory waves anyway
    constexpr bool kRowsOk = (M::NV <= 256);   // up to four state rows per lane
    // one trajectory per LANE keeps NV stage-vector rows per lane: beyond 64 rows only the rows kernel is built
    constexpr bool kLaneBuilt = !(kRowsOk && M::NV > 64);
    // Which state-only kernel (measured on cascade20, DOPRI45, scripts/dev_state_big.py): one trajectory per
    // wavefront up to 2047 trajectories (0.2 ms per 1024, lowest latency); several per wavefront from there
    // (0.14 ms per 1024: 0.56 ms at 4096, 3.3 ms at 32768); one trajectory per LANE costs 2.6 - 2.9 ms whatever
    // the batch up to 65536 (one serial chain per lane, 64 of them per wavefront) and wins from ~20000 on --
    // for small models only: beyond 32 state variables its stage vectors leave the register file.
    constexpr int kLaneFrom = (M::NV <= 32) ? 20480 : 65536;
    // several trajectories per wavefront once the chip is full: models of up to 32 state variables
    if constexpr (M::NV <= 32 && M::NV >= 2) {
      if (a.n_traj >= 2048 && a.n_traj < kLaneFrom && a.opts.variant == SBM_VARIANT_AUTO) {
        // DOPRI45 reduces its error norm inside a segment: widths 16 / 32 (DPP).  Segment sums through LDS for
        // other widths were tried (20 lanes: three trajectories per wavefront): 0.53 against 0.49 ms -- the LDS
        // round trip per step and a third trajectory to wait for cost more than the denser packing gains.
        // RK4 reduces nothing: the width is the state variables rounded up to a multiple of four lanes.
        constexpr int SEG_A = M::NV <= 16 ? 16 : 32;
        constexpr int SEG_F = (M::NV + 3) / 4 * 4;
        return sbm_with_method(a.opts.method, [&](auto m) {
          constexpr int METHOD = decltype(m)::value;
          constexpr int SEG = METHOD == SBM_RK4_FIXED ? SEG_F : SEG_A;
          hipLaunchKernelGGL((sbm_state_packed_kernel<M, METHOD, SEG>), dim3((a.n_traj + 64 / SEG - 1) / (64 / SEG)), dim3(64), 0, stream, a);
          return (int)hipGetLastError();
        });
      }
    }
    if constexpr (kRowsOk) {
      if (((a.n_traj < kLaneFrom || a.opts.variant == SBM_VARIANT_ROW_LANE || a.opts.variant == SBM_VARIANT_ROW_GROUP) &&
           a.opts.variant != SBM_VARIANT_PER_WAVE) || !kLaneBuilt || a.opts.method == SBM_DOP853) {
        return sbm_with_method(a.opts.method, [&](auto m) {
          hipLaunchKernelGGL((sbm_state_rows_kernel<M, decltype(m)::value>), dim3(a.n_traj), dim3(64), 0, stream, a);
          return (int)hipGetLastError();
        });
      }
    }
    if constexpr (kLaneBuilt) {
      return sbm_with_method(a.opts.method, [&](auto m) {
        constexpr int METHOD = decltype(m)::value;
        // (DOP853 gets here only with more than 256 state variables -- up to 256, kRowsOk above takes every DOP853 call,
        // and !kLaneBuilt always takes the rows kernel: twelve stage vectors of NV rows per lane are not built)
        if constexpr (METHOD == SBM_DOP853) return (int)hipErrorInvalidConfiguration;
        else {
          hipLaunchKernelGGL((sbm_state_kernel<M, METHOD>), dim3((a.n_traj + 63) / 64), dim3(64), 0, stream, a);
          return (int)hipGetLastError();
        }
      });
    }
  }
  return (int)hipGetLastError();
}
