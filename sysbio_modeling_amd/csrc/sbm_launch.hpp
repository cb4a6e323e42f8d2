// sbm_launch.hpp -- host side of a model plugin: how the kernel of a call is launched.  Which kernel that is, and which
// kernels a plugin contains, is decided in sbm_kernel_choice.hpp (plain C++, checked on the host).
// Included last by sbm_integrators.hpp (never on its own).
#pragma once
#include <map>
#include <mutex>
#include <utility>
#include <stdlib.h>
#include <stdio.h>

#include "sbm_kernel_choice.hpp"

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
// developer switch: SBM_DEBUG_LAUNCH prints the choice of every launch ("launch choice: ..."), the shape of every
// persistent launch, and names the matrix-core and packed sensitivity kernels with their compiled plan when a call runs
// them (tests/test_gpu_tile_edges.py and tests/test_gpu_kernel_choice.py read these lines)
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

// the only place that reads M for dispatch
template <class M>
constexpr SbmModelTraits sbm_traits_of() {
  return SbmModelTraits{M::NV, M::NK, M::NNZ_JY, M::RG0::RG_OK, {M::RG0::RG_NCH, M::RG1::RG_NCH, M::RG2::RG_NCH},
                        std::is_same<typename M::RG1, typename M::RG0>::value, std::is_same<typename M::RG2, typename M::RG0>::value,
                        std::is_same<typename M::RG2, typename M::RG1>::value, SbmImplicitFits<M>::fixed, SbmImplicitFits<M>::adaptive,
                        SbmIexFits<M>::value, SbmIexSeqFits<M>::value, SbmIexSeqPlan<M>::KMAX, SbmIexSeqPlan<M>::ROT_OK,
                        SbmMfmaPlan<M>::NCH};
}
// launch(std::integral_constant<int, METHOD>) for the explicit method of a choice, where the plugin contains KERNEL for it
template <class M, int KERNEL, class F>
static int sbm_with_method(int method, F&& launch) {
  auto built = [&](auto m) {
    if constexpr (sbm_kernel_built(sbm_traits_of<M>(), KERNEL, decltype(m)::value)) {
      launch(m);
      return (int)hipGetLastError();
    } else {
      return (int)hipErrorInvalidConfiguration;
    }
  };
  if (method == SBM_DOPRI45) return built(std::integral_constant<int, SBM_DOPRI45>{});
  if (method == SBM_DOP853) return built(std::integral_constant<int, SBM_DOP853>{});
  return built(std::integral_constant<int, SBM_RK4_FIXED>{});
}
template <class M, class L, int KERNEL>
static int sbm_launch_rowgroup(int method, const sbm_kernel_args& a, hipStream_t stream) {
  return sbm_with_method<M, KERNEL>(method, [&](auto m) {
    hipLaunchKernelGGL((sbm_sens_rowgroup_kernel<M, L, decltype(m)::value>), dim3(a.n_traj, L::RG_NCH), dim3(64), 0, stream, a);
  });
}
// persistent wavefronts: as many workgroups as the device holds, each taking pieces of work from a counter
template <class M, bool ROT>
static int sbm_launch_iex_seq(const sbm_kernel_args& a, int nch, hipStream_t stream) {
  const int n_work = a.n_traj * nch;
  int resident = 0;
  hipError_t e = sbm_resident_blocks((const void*)sbm_iex_seq_kernel<M, ROT>, 64, &resident);
  if (e != hipSuccess) return (int)e;
  const int grid = n_work < resident ? n_work : resident;
  if (sbm_debug_launch()) fprintf(stderr, "sbm_iex_seq_kernel: %d pieces of work, %d resident workgroups, grid %d\n", n_work, resident, grid);
  SbmScratch* sc = nullptr;
  e = sbm_scratch_for(stream, (size_t)grid * SbmIexSeqPlan<M>::BLOCK_DOUBLES * sizeof(double), &sc);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(sc->counter, 0, sizeof(int), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((sbm_iex_seq_kernel<M, ROT>), dim3(grid), dim3(64), 0, stream, a, (double*)sc->p, sc->counter, n_work, nch);
  return (int)hipGetLastError();
}

template <class M>
static int sbm_launch_model(int kind, const sbm_kernel_args* args, hipStream_t stream) {
  const sbm_kernel_args a = *args;
  if (a.n_traj <= 0) return (int)hipSuccess;
  constexpr SbmModelTraits T = sbm_traits_of<M>();
  const SbmKernelChoice c = sbm_choose_kernel(T, kind, a.opts, a.n_traj, a.S != nullptr, a.s0 != nullptr, sbm_iex_seq_enabled());
  if (sbm_debug_launch())
    fprintf(stderr, "launch choice: %s method %d nch %d SEG %d, %d trajectories\n", sbm_kernel_name(c.kernel), c.method, c.nch, c.seg, a.n_traj);
  // (the chunks of sbm_imid_kernel repeat one fixed-step state: each stores the same report, nothing is combined)
  if (c.nch > 1 && c.kernel != SBM_K_IMID) {
    const hipError_t e = sbm_zero_report(a, stream);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 per_traj(a.n_traj, c.nch), block(64);
  // (The compiler emits the kernels into the code object in the order of the cases.  The implicit kernels come first, as
  // they did in the launcher before: tests/test_seq_kernel_isa.py reads sbm_iex_seq_kernel<M, true> up to the next symbol.)
  switch (c.kernel) {
    case SBM_K_IEX_SEQ_ROT:
      if constexpr (sbm_kernel_built(sbm_traits_of<M>(), SBM_K_IEX_SEQ_ROT, 0)) return sbm_launch_iex_seq<M, true>(a, c.nch, stream);
      break;
    case SBM_K_IEX_SEQ:
      if constexpr (sbm_kernel_built(sbm_traits_of<M>(), SBM_K_IEX_SEQ, 0)) return sbm_launch_iex_seq<M, false>(a, c.nch, stream);
      break;
    case SBM_K_IEX:
      if constexpr (sbm_kernel_built(sbm_traits_of<M>(), SBM_K_IEX, 0)) {
        hipLaunchKernelGGL((sbm_iex_kernel<M>), per_traj, block, 0, stream, a);
        return (int)hipGetLastError();
      }
      break;
    case SBM_K_IMAD:
      if constexpr (sbm_kernel_built(sbm_traits_of<M>(), SBM_K_IMAD, 0)) {
        hipLaunchKernelGGL((sbm_imid_adaptive_kernel<M>), per_traj, block, 0, stream, a);
        return (int)hipGetLastError();
      }
      break;
    case SBM_K_IMID:
      if constexpr (sbm_kernel_built(sbm_traits_of<M>(), SBM_K_IMID, 0)) {
        hipLaunchKernelGGL((sbm_imid_kernel<M>), per_traj, block, 0, stream, a);
        return (int)hipGetLastError();
      }
      break;
    case SBM_K_PER_WAVE:
      return sbm_with_method<M, SBM_K_PER_WAVE>(c.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_sens_kernel<M, decltype(m)::value>), per_traj, block, 0, stream, a);
      });
    case SBM_K_ROW_LANE:
      return sbm_with_method<M, SBM_K_ROW_LANE>(c.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_sens_rowlane_kernel<M, decltype(m)::value>), per_traj, block, 0, stream, a);
      });
    case SBM_K_ROW_GROUP_RG0: return sbm_launch_rowgroup<M, typename M::RG0, SBM_K_ROW_GROUP_RG0>(c.method, a, stream);
    case SBM_K_ROW_GROUP_RG1: return sbm_launch_rowgroup<M, typename M::RG1, SBM_K_ROW_GROUP_RG1>(c.method, a, stream);
    case SBM_K_ROW_GROUP_RG2: return sbm_launch_rowgroup<M, typename M::RG2, SBM_K_ROW_GROUP_RG2>(c.method, a, stream);
    case SBM_K_MFMA:
      if constexpr (sbm_kernel_built(sbm_traits_of<M>(), SBM_K_MFMA, SBM_RK4_FIXED)) {
        if (sbm_debug_launch()) fprintf(stderr, "sbm_sens_mfma_kernel: RT %d CT %d NCH %d LDJ %d LDA %d, %d trajectories\n", SbmMfmaPlan<M>::RT, SbmMfmaPlan<M>::CT, SbmMfmaPlan<M>::NCH, SbmMfmaShared<M, SbmMfmaPlan<M>::CT>::LDJ, SbmMfmaShared<M, SbmMfmaPlan<M>::CT>::LDA, a.n_traj);
      }
      return sbm_with_method<M, SBM_K_MFMA>(c.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_sens_mfma_kernel<M, decltype(m)::value>), per_traj, block, 0, stream, a);
      });
    case SBM_K_SENS_PACKED: {
      constexpr int SEG = sbm_sens_packed_seg(T);
      const int grid = (a.n_traj + 64 / SEG - 1) / (64 / SEG);
      if (sbm_debug_launch()) fprintf(stderr, "sbm_sens_packed_kernel: SEG %d, %d trajectories, grid %d\n", SEG, a.n_traj, grid);
      return sbm_with_method<M, SBM_K_SENS_PACKED>(c.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_sens_packed_kernel<M, decltype(m)::value, SEG>), dim3(grid), block, 0, stream, a);
      });
    }
    case SBM_K_STATE_LANE:
      return sbm_with_method<M, SBM_K_STATE_LANE>(c.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_state_kernel<M, decltype(m)::value>), dim3((a.n_traj + 63) / 64), block, 0, stream, a);
      });
    case SBM_K_STATE_ROWS:
      return sbm_with_method<M, SBM_K_STATE_ROWS>(c.method, [&](auto m) {
        hipLaunchKernelGGL((sbm_state_rows_kernel<M, decltype(m)::value>), per_traj, block, 0, stream, a);
      });
    case SBM_K_STATE_PACKED:
      return sbm_with_method<M, SBM_K_STATE_PACKED>(c.method, [&](auto m) {
        constexpr int SEG = sbm_state_packed_seg(sbm_traits_of<M>(), decltype(m)::value);
        hipLaunchKernelGGL((sbm_state_packed_kernel<M, decltype(m)::value, SEG>), dim3((a.n_traj + 64 / SEG - 1) / (64 / SEG)), block, 0, stream, a);
      });
    default: break;
  }
  return (int)hipErrorInvalidConfiguration;   // SBM_K_NONE: no kernel of this plugin takes the call
}
