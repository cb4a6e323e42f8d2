// sbm_core.hip -- libsbm_hip.so: the C ABI of include/sbm.h.
//
// Contexts, plugin loading, batched simulate / sensitivity entry points, and the host side -- argument checks, LDS
// sizes, launches (launch_lds) -- of the kernels kept in headers of their own:
//   sbm_assemble.hpp        k_gather_params, k_fill_grids, k_assemble: the model-independent Project kernels (theta ->
//                           per-experiment parameter vectors; fused measurement sampling + mapping + scale factors +
//                           weighted residuals + scaled Jacobian), with AssembleLds, the one layout of k_assemble's
//                           dynamic LDS that the kernel carves and launch_assemble sizes
//   sbm_observable_program.hpp  sbm_prog_eval, sbm_prog_check: interpreter and checker of the custom observables'
//                           postfix programs (plain C++, no HIP)
//   sbm_project_check.hpp   sbm_project_desc_check, sbm_loss_desc_check: everything sbm_project_load and
//                           sbm_loss_eval_host verify of a descriptor before they touch the device (plain C++, no HIP)
//   sbm_lm.hpp              k_lm_step, k_lm_trust[_held|_bounded], k_lm_update, k_lm_accept: the fitting loop (batched Levenberg-Marquardt
//                           step, lmder's trust-region step and bookkeeping)
//   sbm_lm_geodesic.hpp     k_lm_geodesic: the second-order (geodesic) correction of the trust-region step, on sbm_lm.hpp's
//                           builder of the normal equations and its factorisation
//   sbm_sampler.hpp         k_sf_entropy[_pt], k_mh_propose[_box], k_mh_accept[_pt], k_mh_accept_hastings, k_pt_swap: scale-factor entropy integrals
//                           (linear_scale_factor.py:63-81; the quadrature rule: sbm_sf_quadrature.hpp), candidate move and
//                           the two acceptance rules of the multi-chain sampler (project/Ensembles.py:193-198, 200-264)
//   sbm_sampling_axes.hpp   k_sampling_axes[_held]: per-chain Hessian axes (batched Jacobi eigensolver + SloppyCell's clipping
//                           recipe; project/Ensembles.py:153-157)
//   sbm_ensemble_stats.hpp  k_ens_*: statistics over the member axis of an ensemble of trajectories
//                           (project/Ensembles.py:277-308, 335-361)
//   sbm_chain_diagnostics.hpp  k_chain_*: autocorrelation, integrated autocorrelation time, effective sample size and
//                           split-R-hat of the samplers' record (project/Ensembles.py:14-29)
//   sbm_block_reduce.hpp    the wavefront / workgroup reductions that k_assemble, the fitting and the sampler kernels share
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sbm_plugin.h"
#include "sbm_assemble.hpp"
#include "sbm_block_reduce.hpp"
#include "sbm_chain_diagnostics.hpp"
#include "sbm_ensemble_stats.hpp"
#include "sbm_lm.hpp"
#include "sbm_lm_geodesic.hpp"
#include "sbm_project_check.hpp"
#include "sbm_sampler.hpp"
#include "sbm_sampling_axes.hpp"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

static int sbm_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define SBM_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return sbm_fail(-2, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

enum { SBM_E_HIP = -2, SBM_E_PLUGIN = -3 };   // SBM_E_ARG = -1: sbm_observable_program.hpp, with the checks that return it

// ---------------------------------------------------------------------------
// objects
// ---------------------------------------------------------------------------
struct sbm_model;

// A device array that grows on demand and is freed with its owner.  Whoever destroys one makes sure first that the
// device is current and that nothing on the stream still uses it.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int reserve(size_t want) {
    if (want <= n) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (hipMalloc((void**)&p, want * sizeof(T)) != hipSuccess) return -1;
    n = want;
    return 0;
  }
};

struct sbm_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  // sbm_ensemble_stats: validity flags [V], used members [V], their number [1]
  DevBuf<int32_t> ens_flag, ens_idx, ens_n;
};

struct sbm_model {
  sbm_ctx* ctx;
  void* dl;
  sbm_plugin_info_t info;
  sbm_plugin_launch_fn launch;
  // launch order of the sensitivity kernels (launch_sens): trajectories sorted by the cost of the
  // previous launch of the same size, most expensive first
  DevBuf<int32_t> order, cost_steps, cost_rej;
  int order_T = 0;   // number of trajectories `order` is a permutation of (0: none yet)
};

struct sbm_project {
  sbm_model* model;
  int E, q, R, G, NPR, NSP, compat, loss;
  int n_params, n_vars, n_sens;
  int n_t_max;  // longest per-experiment grid
  // static device data
  DevBuf<int32_t> pmap, sens_col, tgrid_off, grid_len, row_exp, row_tidx, row_var_off, row_vars, row_sf,
      prior_idx, inv_ptr, inv_m, sfp_group;
  DevBuf<double> pfixed, tgrid, row_data, row_sigma, prior_mean, prior_sigma, sfp_mean, sfp_sigma;
  // log prior of every scale-factor group, [G] (sbm_project_sf_entropy); sf_group_without_prior: first group that has none, or -1
  DevBuf<double> sfg_mean, sfg_sigma;
  int sf_group_without_prior = -1;
  // custom observables (postfix programs): see sbm_project_desc
  int n_programs = 0, n_custom_weights = 0;
  DevBuf<int32_t> row_prog, row_w0, prog_base, prog_sub_off, prog_code;
  DevBuf<double> prog_const, row_time;
  // per-call scratch, grown on demand
  DevBuf<double> P, Y, S, sims, sf;
  DevBuf<int32_t> traj_status, traj_steps, traj_rej, goff, glen;
  int scratch_V = 0;
  // Richardson extrapolation of the implicit-midpoint runs (sbm_project_set_extrapolation)
  int richardson = 0;
  DevBuf<double> Yx[2], Sx[2];
  DevBuf<int32_t> statx, stepsx;
};

extern "C" const char* sbm_last_error(void) { return g_err; }
extern "C" int sbm_abi_version(void) { return SBM_ABI_VERSION; }

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" int sbm_ctx_create(int device, void* stream, sbm_ctx** out) {
  if (!out) return sbm_fail(SBM_E_ARG, "sbm_ctx_create: out is NULL");
  int n = 0;
  SBM_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return sbm_fail(SBM_E_ARG, "sbm_ctx_create: device %d of %d", device, n);
  SBM_HIP(hipSetDevice(device));
  sbm_ctx* c = new sbm_ctx();
  c->device = device;
  // NULL = the device's default (null) stream, which is also what torch enqueues on
  // unless told otherwise: copies made by the caller and our kernels stay ordered
  c->stream = (hipStream_t)stream;
  c->own_stream = false;
  *out = c;
  return 0;
}

extern "C" int sbm_ctx_destroy(sbm_ctx* c) {
  if (!c) return 0;
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

extern "C" int sbm_ctx_synchronize(sbm_ctx* c) {
  if (!c) return sbm_fail(SBM_E_ARG, "sbm_ctx_synchronize: ctx is NULL");
  SBM_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int sbm_ctx_device(const sbm_ctx* c) { return c ? c->device : -1; }

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
extern "C" int sbm_model_load(sbm_ctx* ctx, const char* path, sbm_model** out) {
  if (!ctx || !path || !out) return sbm_fail(SBM_E_ARG, "sbm_model_load: NULL argument");
  SBM_HIP(hipSetDevice(ctx->device));
  void* dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!dl) return sbm_fail(SBM_E_PLUGIN, "dlopen(%s): %s", path, dlerror());
  auto info_fn = (sbm_plugin_info_fn)dlsym(dl, "sbm_plugin_info");
  auto launch_fn = (sbm_plugin_launch_fn)dlsym(dl, "sbm_plugin_launch");
  if (!info_fn || !launch_fn) {
    dlclose(dl);
    return sbm_fail(SBM_E_PLUGIN, "%s is not an sbm model plugin", path);
  }
  sbm_model* m = new sbm_model();
  m->ctx = ctx;
  m->dl = dl;
  m->launch = launch_fn;
  memset(&m->info, 0, sizeof(m->info));
  info_fn(&m->info);
  if (m->info.abi != SBM_PLUGIN_ABI) {
    int abi = m->info.abi;
    dlclose(dl);
    delete m;
    return sbm_fail(SBM_E_PLUGIN, "%s: plugin ABI %d, library expects %d", path, abi, SBM_PLUGIN_ABI);
  }
  *out = m;
  return 0;
}

extern "C" int sbm_model_unload(sbm_model* m) {
  if (!m) return 0;
  // the plugin's code object stays registered with the HIP runtime: do not dlclose
  (void)hipSetDevice(m->ctx->device);
  delete m;
  return 0;
}

extern "C" int sbm_model_info(const sbm_model* m, int32_t* n_vars, int32_t* n_params, int32_t* n_sens,
                              char* name_buf, int32_t name_buf_len) {
  if (!m) return sbm_fail(SBM_E_ARG, "sbm_model_info: model is NULL");
  if (n_vars) *n_vars = m->info.n_vars;
  if (n_params) *n_params = m->info.n_params;
  if (n_sens) *n_sens = m->info.n_sens;
  if (name_buf && name_buf_len > 0) {
    strncpy(name_buf, m->info.name, name_buf_len - 1);
    name_buf[name_buf_len - 1] = 0;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// batched integration
// ---------------------------------------------------------------------------
static int check_opts(const sbm_integrator_opts* o, const char* who) {
  if (!o) return sbm_fail(SBM_E_ARG, "%s: opts is NULL", who);
  if (o->method == SBM_RK4_FIXED) {
    if (!(o->h0 > 0.0)) return sbm_fail(SBM_E_ARG, "%s: RK4 needs h0 > 0", who);
  } else if (o->method == SBM_DOPRI45 || o->method == SBM_DOP853 || o->method == SBM_IMPLICIT_ADAPTIVE ||
             o->method == SBM_IMPLICIT_EXTRAP) {
    if (!(o->rtol > 0.0) || !(o->atol > 0.0)) return sbm_fail(SBM_E_ARG, "%s: adaptive methods need rtol, atol > 0", who);
  } else if (o->method == SBM_IMPLICIT_MIDPOINT || o->method == SBM_IMPLICIT_MIDPOINT_GRADED) {
    if (!(o->h0 > 0.0)) return sbm_fail(SBM_E_ARG, "%s: implicit midpoint needs h0 > 0", who);
  } else {
    return sbm_fail(SBM_E_ARG, "%s: unknown method %d", who, o->method);
  }
  if (o->step_mult < 0 || o->step_mult > 65536) return sbm_fail(SBM_E_ARG, "%s: step_mult %d", who, o->step_mult);
  if (o->variant < SBM_VARIANT_AUTO || o->variant > SBM_VARIANT_PACKED)
    return sbm_fail(SBM_E_ARG, "%s: unknown kernel variant %d", who, o->variant);
  return 0;
}

static int check_model_fits(const sbm_model* m, const sbm_integrator_opts& o, const char* who) {
  if ((o.method == SBM_IMPLICIT_MIDPOINT || o.method == SBM_IMPLICIT_MIDPOINT_GRADED || o.method == SBM_IMPLICIT_ADAPTIVE ||
       o.method == SBM_IMPLICIT_EXTRAP) && m->info.n_vars > SBM_IMPLICIT_MAX_NV)
    return sbm_fail(SBM_E_ARG, "%s: the implicit midpoint kernels hold a column of the sensitivity matrix per lane in "
                    "registers: n_vars <= %d (model '%s' has %d)", who, SBM_IMPLICIT_MAX_NV, m->info.name, m->info.n_vars);
  return 0;
}

static int launch_failed(sbm_model* m, const sbm_integrator_opts& o, int e, const char* who) {
  if (e == (int)hipErrorInvalidConfiguration &&
      (o.method == SBM_IMPLICIT_MIDPOINT || o.method == SBM_IMPLICIT_MIDPOINT_GRADED || o.method == SBM_IMPLICIT_ADAPTIVE ||
       o.method == SBM_IMPLICIT_EXTRAP))
    return sbm_fail(SBM_E_ARG, "%s: model '%s' (%d state variables, %d sensitivity columns) does not fit the implicit kernel "
                    "asked for: its tables need more than the 160 KB of LDS of a compute unit (the error-controlled kernel "
                    "parks two copies of a 64-column block of S there); the fixed-step method may still fit", who,
                    m->info.name, m->info.n_vars, m->info.n_sens);
  if (e == (int)hipErrorInvalidConfiguration && o.method == SBM_DOP853)
    return sbm_fail(SBM_E_ARG, "%s: DOP853 runs on the row-group sensitivity kernels and the state-rows kernels; model '%s' "
                    "has no row split (or more than 256 state variables): use DOPRI45", who, m->info.name);
  return sbm_fail(SBM_E_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
}

static int launch(sbm_model* m, int kind, const sbm_kernel_args& a, const char* who) {
  if (int rc = check_model_fits(m, a.opts, who)) return rc;
  SBM_HIP(hipSetDevice(m->ctx->device));
  int e = m->launch(kind, &a, (void*)m->ctx->stream);
  if (e != 0) return launch_failed(m, a.opts, e, who);
  return 0;
}

// ---- launch order of the sensitivity kernels ---------------------------------------------------
// An adaptive integrator takes a different number of steps for every parameter vector (configs[2]:
// 445 ... 574, mean 485).  One trajectory occupies one SIMD for its whole life, the hardware hands
// out workgroups in index order, and the kernel ends when the last trajectory does: in index order
// the chip idles for 5.8 % of the launch at 4 trajectories per SIMD (scripts/dev_balance.py).  A
// fitting loop integrates nearly the same ensemble again and again, so the step counts of the
// previous launch predict the next one: sort by them, longest first (LPT), 1.9 %.  The order only
// changes which workgroup integrates which trajectory, never a result.
__global__ void __launch_bounds__(1024) k_order(const int32_t* __restrict__ steps, const int32_t* __restrict__ rej, int T,
                                                int32_t* __restrict__ order) {
  constexpr int NB = 2048;
  __shared__ int hist[NB];
  __shared__ int smax;
  const int tid = threadIdx.x;
  for (int b = tid; b < NB; b += blockDim.x) hist[b] = 0;
  if (tid == 0) smax = 1;
  __syncthreads();
  int mx = 1;
  for (int i = tid; i < T; i += blockDim.x) mx = max(mx, steps[i] + rej[i]);
  atomicMax(&smax, mx);
  __syncthreads();
  const double scale = (double)(NB - 1) / (double)smax;
  // bin 0 = most expensive
  for (int i = tid; i < T; i += blockDim.x) {
    const int c = max(0, steps[i] + rej[i]);
    atomicAdd(&hist[NB - 1 - (int)(c * scale)], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int b = 0; b < NB; ++b) { const int h = hist[b]; hist[b] = run; run += h; }
  }
  __syncthreads();
  for (int i = tid; i < T; i += blockDim.x) {
    const int c = max(0, steps[i] + rej[i]);
    order[atomicAdd(&hist[NB - 1 - (int)(c * scale)], 1)] = i;
  }
}

static int launch_sens(sbm_model* m, sbm_kernel_args a, const char* who) {
  if (int rc = check_model_fits(m, a.opts, who)) return rc;
  SBM_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const int T = a.n_traj;
  // the order is only worth its bookkeeping when trajectories queue behind each other
  const bool use = T >= 2048;
  if (use) {
    if (m->order.reserve(T) || m->cost_steps.reserve(T) || m->cost_rej.reserve(T))
      return sbm_fail(SBM_E_HIP, "%s: out of device memory", who);
    if (m->order_T == T) a.order = m->order.p;
    if (!a.n_steps) a.n_steps = m->cost_steps.p;
    if (!a.n_reject) a.n_reject = m->cost_rej.p;
  }
  int e = m->launch(SBM_KIND_SENS, &a, (void*)s);
  if (e != 0) return launch_failed(m, a.opts, e, who);
  if (use) {
    hipLaunchKernelGGL(k_order, dim3(1), dim3(1024), 0, s, a.n_steps, a.n_reject, T, m->order.p);
    SBM_HIP(hipGetLastError());
    m->order_T = T;
  }
  return 0;
}

extern "C" int sbm_simulate_batch(sbm_model* m, const double* P, int32_t V, const double* t_out, int32_t n_t,
                                  const double* y0, const sbm_integrator_opts* opts, double* Y, int32_t* status,
                                  int32_t* n_steps, int32_t* n_reject) {
  if (!m || !P || !t_out || !Y) return sbm_fail(SBM_E_ARG, "sbm_simulate_batch: NULL argument");
  if (V < 0 || n_t < 0) return sbm_fail(SBM_E_ARG, "sbm_simulate_batch: negative size");
  int rc = check_opts(opts, "sbm_simulate_batch");
  if (rc) return rc;
  if (V == 0 || n_t == 0) return 0;
  sbm_kernel_args a;
  memset(&a, 0, sizeof(a));
  a.P = P; a.t_out = t_out; a.y0 = y0; a.Y = Y;
  a.status = status; a.n_steps = n_steps; a.n_reject = n_reject;
  a.n_traj = V; a.n_t = n_t; a.opts = *opts;
  return launch(m, SBM_KIND_STATE, a, "sbm_simulate_batch");
}

extern "C" int sbm_sens_batch(sbm_model* m, const double* P, int32_t V, const double* t_out, int32_t n_t,
                              const double* yS0, const sbm_integrator_opts* opts, double* Y, double* S,
                              int32_t* status, int32_t* n_steps, int32_t* n_reject) {
  if (!m || !P || !t_out || !S) return sbm_fail(SBM_E_ARG, "sbm_sens_batch: NULL argument");
  if (V < 0 || n_t < 0) return sbm_fail(SBM_E_ARG, "sbm_sens_batch: negative size");
  int rc = check_opts(opts, "sbm_sens_batch");
  if (rc) return rc;
  if (V == 0 || n_t == 0) return 0;
  sbm_kernel_args a;
  memset(&a, 0, sizeof(a));
  a.P = P; a.t_out = t_out;
  a.y0 = yS0; a.s0 = yS0 ? yS0 + m->info.n_vars : nullptr;
  a.Y = Y; a.S = S;
  a.status = status; a.n_steps = n_steps; a.n_reject = n_reject;
  a.n_traj = V; a.n_t = n_t; a.opts = *opts;
  return launch_sens(m, a, "sbm_sens_batch");
}

// ---- host-pointer variants -------------------------------------------------
namespace {
struct HostStage {
  std::vector<void*> allocs;
  ~HostStage() {
    for (void* p : allocs) (void)hipFree(p);
  }
  template <class T>
  T* up(const T* h, size_t n, hipStream_t s) {
    if (!h || n == 0) return nullptr;
    T* d = nullptr;
    if (hipMalloc((void**)&d, n * sizeof(T)) != hipSuccess) return nullptr;
    allocs.push_back(d);
    if (hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess) return nullptr;
    return d;
  }
  template <class T>
  T* dev(size_t n) {
    if (n == 0) return nullptr;
    T* d = nullptr;
    if (hipMalloc((void**)&d, n * sizeof(T)) != hipSuccess) return nullptr;
    allocs.push_back(d);
    return d;
  }
};
}  // namespace

#define SBM_NEED(ptr, what) \
  if (!(ptr)) return sbm_fail(SBM_E_HIP, "%s: device staging failed (out of memory?)", what)

extern "C" int sbm_simulate_batch_host(sbm_model* m, const double* P, int32_t V, const double* t_out, int32_t n_t,
                                       const double* y0, const sbm_integrator_opts* opts, double* Y,
                                       int32_t* status, int32_t* n_steps, int32_t* n_reject) {
  if (!m || !P || !t_out || !Y) return sbm_fail(SBM_E_ARG, "sbm_simulate_batch_host: NULL argument");
  if (V <= 0 || n_t <= 0) return V < 0 || n_t < 0 ? sbm_fail(SBM_E_ARG, "negative size") : 0;
  SBM_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const int nv = m->info.n_vars, np = m->info.n_params;
  HostStage st;
  double* dP = st.up(P, (size_t)V * np, s); SBM_NEED(dP, "simulate");
  double* dt = st.up(t_out, (size_t)n_t, s); SBM_NEED(dt, "simulate");
  double* dy0 = y0 ? st.up(y0, (size_t)nv, s) : nullptr;
  double* dY = st.dev<double>((size_t)V * n_t * nv); SBM_NEED(dY, "simulate");
  int32_t* dst = st.dev<int32_t>((size_t)V * 3); SBM_NEED(dst, "simulate");
  int rc = sbm_simulate_batch(m, dP, V, dt, n_t, dy0, opts, dY, dst, dst + V, dst + 2 * V);
  if (rc) return rc;
  SBM_HIP(hipMemcpyAsync(Y, dY, (size_t)V * n_t * nv * sizeof(double), hipMemcpyDeviceToHost, s));
  if (status) SBM_HIP(hipMemcpyAsync(status, dst, V * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (n_steps) SBM_HIP(hipMemcpyAsync(n_steps, dst + V, V * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (n_reject) SBM_HIP(hipMemcpyAsync(n_reject, dst + 2 * V, V * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SBM_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int sbm_sens_batch_host(sbm_model* m, const double* P, int32_t V, const double* t_out, int32_t n_t,
                                   const double* yS0, const sbm_integrator_opts* opts, double* Y, double* S,
                                   int32_t* status, int32_t* n_steps, int32_t* n_reject) {
  if (!m || !P || !t_out || !S) return sbm_fail(SBM_E_ARG, "sbm_sens_batch_host: NULL argument");
  if (V <= 0 || n_t <= 0) return V < 0 || n_t < 0 ? sbm_fail(SBM_E_ARG, "negative size") : 0;
  SBM_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const int nv = m->info.n_vars, np = m->info.n_params, nk = m->info.n_sens;
  HostStage st;
  double* dP = st.up(P, (size_t)V * np, s); SBM_NEED(dP, "sens");
  double* dt = st.up(t_out, (size_t)n_t, s); SBM_NEED(dt, "sens");
  double* d0 = yS0 ? st.up(yS0, (size_t)nv * (1 + nk), s) : nullptr;
  double* dY = st.dev<double>((size_t)V * n_t * nv); SBM_NEED(dY, "sens");
  double* dS = st.dev<double>((size_t)V * n_t * nv * nk); SBM_NEED(dS, "sens");
  int32_t* dst = st.dev<int32_t>((size_t)V * 3); SBM_NEED(dst, "sens");
  int rc = sbm_sens_batch(m, dP, V, dt, n_t, d0, opts, dY, dS, dst, dst + V, dst + 2 * V);
  if (rc) return rc;
  if (Y) SBM_HIP(hipMemcpyAsync(Y, dY, (size_t)V * n_t * nv * sizeof(double), hipMemcpyDeviceToHost, s));
  SBM_HIP(hipMemcpyAsync(S, dS, (size_t)V * n_t * nv * nk * sizeof(double), hipMemcpyDeviceToHost, s));
  if (status) SBM_HIP(hipMemcpyAsync(status, dst, V * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (n_steps) SBM_HIP(hipMemcpyAsync(n_steps, dst + V, V * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (n_reject) SBM_HIP(hipMemcpyAsync(n_reject, dst + 2 * V, V * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SBM_HIP(hipStreamSynchronize(s));
  return 0;
}

// ===========================================================================
// Project
// ===========================================================================
template <class T>
static int upload(DevBuf<T>& b, const T* h, size_t n, hipStream_t s) {
  if (n == 0) n = 1;  // keep pointers non-NULL
  if (b.reserve(n)) return -1;
  if (h && hipMemcpyAsync(b.p, h, (n) * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess) return -1;
  return 0;
}

extern "C" int sbm_project_load(sbm_model* m, const sbm_project_desc* d, sbm_project** out) {
  if (!m || !d || !out) return sbm_fail(SBM_E_ARG, "sbm_project_load: NULL argument");
  // validated on the host: the kernels index with these arrays and run the custom-observable programs unchecked
  sbm_project_tables t;
  if (int rc = sbm_project_desc_check(d, m->info.n_vars, m->info.n_params, m->info.n_sens, g_err, sizeof(g_err), &t)) return rc;
  const int E = d->n_experiments, q = d->n_project_params, R = d->n_rows, G = d->n_sf_groups,
            NPR = d->n_prior_rows, NSP = d->n_sf_prior_rows, NP = m->info.n_params, NPG = d->n_programs;

  SBM_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  sbm_project* p = new sbm_project();
  p->model = m;
  p->E = E; p->q = q; p->R = R; p->G = G; p->NPR = NPR; p->NSP = NSP; p->compat = d->reference_compat;
  p->loss = d->loss_type;
  p->n_params = NP; p->n_vars = m->info.n_vars; p->n_sens = m->info.n_sens; p->n_t_max = t.n_t_max;

  // inverse map: for experiment e and project column c, the model params that read it
  std::vector<int32_t> inv_ptr((size_t)E * (q + 1), 0), inv_m;
  for (int e = 0; e < E; ++e) {
    for (int c = 0; c < q; ++c) {
      inv_ptr[(size_t)e * (q + 1) + c] = (int32_t)inv_m.size();
      for (int k = 0; k < NP; ++k)
        if (d->pmap[e * NP + k] == c) inv_m.push_back(k);
    }
    inv_ptr[(size_t)e * (q + 1) + q] = (int32_t)inv_m.size();
  }
  std::vector<int32_t> glen(E);
  for (int e = 0; e < E; ++e) glen[e] = d->tgrid_off[e + 1] - d->tgrid_off[e];
  const int nvars_total = R ? d->row_var_off[R] : 0;
  int bad = 0;
  bad |= upload(p->pmap, d->pmap, (size_t)E * NP, s);
  bad |= upload(p->pfixed, d->pfixed, (size_t)E * NP, s);
  bad |= upload(p->sens_col, d->sens_col, (size_t)NP, s);
  bad |= upload(p->tgrid_off, d->tgrid_off, (size_t)E + 1, s);
  bad |= upload(p->tgrid, d->tgrid, (size_t)d->tgrid_off[E], s);
  bad |= upload(p->grid_len, glen.data(), (size_t)E, s);
  bad |= upload(p->row_exp, d->row_exp, (size_t)R, s);
  bad |= upload(p->row_tidx, d->row_tidx, (size_t)R, s);
  bad |= upload(p->row_var_off, d->row_var_off, (size_t)R + 1, s);
  bad |= upload(p->row_vars, d->row_vars, (size_t)nvars_total, s);
  bad |= upload(p->row_data, d->row_data, (size_t)R, s);
  bad |= upload(p->row_sigma, d->row_sigma, (size_t)R, s);
  bad |= upload(p->row_sf, d->row_sf, (size_t)R, s);
  bad |= upload(p->prior_idx, d->prior_idx, (size_t)NPR, s);
  bad |= upload(p->prior_mean, d->prior_mean, (size_t)NPR, s);
  bad |= upload(p->prior_sigma, d->prior_sigma, (size_t)NPR, s);
  bad |= upload(p->sfp_group, d->sf_prior_group, (size_t)NSP, s);
  bad |= upload(p->sfp_mean, d->sf_prior_mean, (size_t)NSP, s);
  bad |= upload(p->sfp_sigma, d->sf_prior_sigma, (size_t)NSP, s);
  std::vector<double> sfg_mean((size_t)(G > 0 ? G : 1), 0.0), sfg_sigma((size_t)(G > 0 ? G : 1), 0.0);
  for (int k = 0; k < NSP; ++k) {
    sfg_mean[d->sf_prior_group[k]] = d->sf_prior_mean[k];
    sfg_sigma[d->sf_prior_group[k]] = d->sf_prior_sigma[k];
  }
  for (int k = G - 1; k >= 0; --k)
    if (!(sfg_sigma[k] > 0.0)) p->sf_group_without_prior = k;
  bad |= upload(p->sfg_mean, sfg_mean.data(), (size_t)G, s);
  bad |= upload(p->sfg_sigma, sfg_sigma.data(), (size_t)G, s);
  bad |= upload(p->inv_ptr, inv_ptr.data(), inv_ptr.size(), s);
  bad |= upload(p->inv_m, inv_m.data(), inv_m.size(), s);
  p->n_programs = NPG;
  p->n_custom_weights = t.n_weights;
  if (NPG > 0) {
    bad |= upload(p->row_prog, d->row_prog, (size_t)R, s);
    bad |= upload(p->row_w0, t.row_w0.data(), (size_t)R, s);
    bad |= upload(p->prog_base, t.prog_base.data(), t.prog_base.size(), s);
    bad |= upload(p->prog_sub_off, d->prog_sub_off, (size_t)t.prog_base[NPG] + 1, s);
    bad |= upload(p->prog_code, d->prog_code, (size_t)d->n_prog_code, s);
    bad |= upload(p->prog_const, d->prog_const, (size_t)d->n_prog_const, s);
    bad |= upload(p->row_time, d->row_time, (size_t)R, s);
  }
  hipError_t e = hipStreamSynchronize(s);  // host vectors go out of scope
  if (bad || e != hipSuccess) {
    sbm_project_unload(p);
    return sbm_fail(SBM_E_HIP, "sbm_project_load: device upload failed");
  }
  *out = p;
  return 0;
}

extern "C" int sbm_project_unload(sbm_project* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->model->ctx->device);
  delete p;
  return 0;
}

extern "C" int64_t sbm_project_scratch_bytes(const sbm_project* p, int32_t V, int32_t with_sens) {
  if (!p || V < 0) return -1;
  const int64_t T = (int64_t)V * p->E;
  int64_t b = T * p->n_params * 8 + T * p->n_t_max * p->n_vars * 8 + T * 5 * 4 + (int64_t)V * (p->R + p->G) * 8;
  if (with_sens) b += T * p->n_t_max * p->n_vars * (int64_t)p->n_sens * 8;
  return b;
}

// Richardson combination of runs with step sizes h, h/2 (, h/4) of a symmetric one-step method (error
// expansion in h^2):  levels = 1: (4 b - a) / 3;  levels = 2: (16 (4 c - b)/3 - (4 b - a)/3) / 15.  In place in a.
__global__ void k_richardson(double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ c,
                             size_t n, int levels) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double t1 = (4.0 * b[i] - a[i]) * (1.0 / 3.0);
  if (levels == 1) { a[i] = t1; return; }
  const double t2 = (4.0 * c[i] - b[i]) * (1.0 / 3.0);
  a[i] = (16.0 * t2 - t1) * (1.0 / 15.0);
}
__global__ void k_merge_status(int32_t* __restrict__ st, int32_t* __restrict__ steps, const int32_t* __restrict__ st2,
                               const int32_t* __restrict__ steps2, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st[i] = max(st[i], st2[i]);
  steps[i] += steps2[i];
}

extern "C" int sbm_project_set_extrapolation(sbm_project* p, int32_t levels) {
  if (!p) return sbm_fail(SBM_E_ARG, "sbm_project_set_extrapolation: project is NULL");
  if (levels < 0 || levels > 2) return sbm_fail(SBM_E_ARG, "sbm_project_set_extrapolation: levels %d (0, 1 or 2)", levels);
  p->richardson = levels;
  return 0;
}

// accepted steps of every trajectory of the project's last evaluation, [V][E] (vector-major), device to device
extern "C" int sbm_project_trajectory_steps(sbm_project* p, int32_t V, int32_t* steps_dev) {
  if (!p || !steps_dev) return sbm_fail(SBM_E_ARG, "sbm_project_trajectory_steps: NULL argument");
  if (V < 0) return sbm_fail(SBM_E_ARG, "sbm_project_trajectory_steps: V < 0");
  const size_t T = (size_t)V * p->E;
  if (T == 0) return 0;
  // the counts of the LAST evaluation, whatever the buffer could hold: a V other than that evaluation's would hand back
  // stale or uninitialised counts with a success code (round 3 checked the capacity only)
  if (!p->traj_steps.p || p->traj_steps.n < T || p->scratch_V != V)
    return sbm_fail(SBM_E_ARG, "sbm_project_trajectory_steps: V = %d, but the project's last evaluation had %d vectors", V,
                    p->traj_steps.p ? p->scratch_V : 0);
  SBM_HIP(hipSetDevice(p->model->ctx->device));
  SBM_HIP(hipMemcpyAsync(steps_dev, p->traj_steps.p, T * sizeof(int32_t), hipMemcpyDeviceToDevice, p->model->ctx->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Kernels with dynamic LDS: what a workgroup may have, and the launch.
// ---------------------------------------------------------------------------------------------
static int lm_lds_limit(sbm_ctx* ctx) {
  int lim = 0;
  if (hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess || lim <= 0) lim = 64 * 1024;
  return lim;
}

// `kernel` on the context's device and stream with `lds` bytes of dynamic LDS; more than 64 KB have to be asked for
template <class... P, class... A>
static int launch_lds(sbm_ctx* ctx, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A&... args) {
  SBM_HIP(hipSetDevice(ctx->device));
  if (lds > 64 * 1024) SBM_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, args...);
  SBM_HIP(hipGetLastError());
  return 0;
}

// The dynamic block of k_assemble (AssembleLds) and the kernel's static LDS (s_bad, padded to the dynamic block's
// alignment: 16 bytes, read from the code object) have to fit the device's workgroup limit TOGETHER: compared alone with
// a literal 160 KB, a dynamic block within 16 bytes of the limit was accepted here and refused by the runtime at the launch.
//
// The instantiation is assemble_form's (sbm_assemble.hpp).  Developer switch, read at every launch:
// SBM_ASSEMBLE_ROWS_IN_REGS=0 takes the form through global memory (rows == 0) for every shape -- the reference the
// register-tile forms are compared with bit for bit (tests/test_gpu_assemble_one_trip.py), and the A/B timing.
// Under SBM_DEBUG_LAUNCH the launcher names the instantiation.
template <int K, bool PROG>
static int launch_assemble_as(sbm_ctx* ctx, const AssembleArgs& g, int V, size_t lds, bool log) {
  if (log) return launch_lds(ctx, k_assemble<K, PROG, true>, dim3(V), dim3(256), lds, g);
  return launch_lds(ctx, k_assemble<K, PROG, false>, dim3(V), dim3(256), lds, g);
}
template <int K>
static int launch_assemble_as(sbm_ctx* ctx, const AssembleArgs& g, int V, size_t lds, bool prog, bool log) {
  return prog ? launch_assemble_as<K, true>(ctx, g, V, lds, log) : launch_assemble_as<K, false>(ctx, g, V, lds, log);
}

static int launch_assemble(sbm_ctx* ctx, const AssembleArgs& g, int V, const char* who) {
  const size_t lds = AssembleLds(g.R, g.G, g.q, g.NW, 256).bytes();
  static const size_t stat = [] {   // asked once: the same on every device and in every instantiation (s_bad)
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, (const void*)k_assemble<0, false, false>) == hipSuccess ? (size_t)fa.sharedSizeBytes : (size_t)16;
  }();
  const size_t limit = (size_t)lm_lds_limit(ctx);
  if (lds + stat > limit)
    return sbm_fail(SBM_E_ARG, "%s: project too large for the assembly kernel (%zu B of LDS + %zu B static, the workgroup's limit is %zu B)",
                    who, lds, stat, limit);
  AssembleForm f = assemble_form(g.R, g.q, g.row_w0 != nullptr && !g.sims_in, g.loss, 256);
  const char* in_regs = getenv("SBM_ASSEMBLE_ROWS_IN_REGS");
  if (in_regs && in_regs[0] == '0' && !in_regs[1]) f.rows = 0;
  if (getenv("SBM_DEBUG_LAUNCH"))
    fprintf(stderr, "k_assemble<%d, %d, %d>: R %d q %d G %d, %d vectors, %zu B of LDS\n", f.rows, f.prog, f.log, g.R, g.q, g.G, V, lds);
  switch (f.rows) {
    case SBM_ASSEMBLE_TILE_LARGE: return launch_assemble_as<SBM_ASSEMBLE_TILE_LARGE>(ctx, g, V, lds, f.prog, f.log);
    case SBM_ASSEMBLE_TILE_SMALL: return launch_assemble_as<SBM_ASSEMBLE_TILE_SMALL>(ctx, g, V, lds, f.prog, f.log);
    default: return launch_assemble_as<0>(ctx, g, V, lds, f.prog, f.log);
  }
}

// the static part of the kernel's arguments: the project's tables
static AssembleArgs assemble_args(const sbm_project* p) {
  AssembleArgs g;
  memset(&g, 0, sizeof(g));
  g.E = p->E; g.q = p->q; g.R = p->R; g.G = p->G; g.NPR = p->NPR; g.NSP = p->NSP;
  g.NP = p->n_params; g.NV = p->n_vars; g.NK = p->n_sens; g.n_t = p->n_t_max;
  g.compat = p->compat;
  g.loss = p->loss;
  g.row_exp = p->row_exp.p; g.row_tidx = p->row_tidx.p; g.row_var_off = p->row_var_off.p; g.row_vars = p->row_vars.p;
  g.row_sf = p->row_sf.p; g.prior_idx = p->prior_idx.p; g.row_data = p->row_data.p; g.row_sigma = p->row_sigma.p;
  g.prior_mean = p->prior_mean.p; g.prior_sigma = p->prior_sigma.p;
  g.sfp_group = p->sfp_group.p; g.sfp_mean = p->sfp_mean.p; g.sfp_sigma = p->sfp_sigma.p; g.inv_ptr = p->inv_ptr.p; g.inv_m = p->inv_m.p;
  g.sens_col = p->sens_col.p;
  if (p->n_programs > 0) {
    g.NW = p->n_custom_weights;
    g.row_prog = p->row_prog.p; g.row_w0 = p->row_w0.p; g.prog_base = p->prog_base.p; g.prog_sub_off = p->prog_sub_off.p;
    g.prog_code = p->prog_code.p; g.prog_const = p->prog_const.p; g.row_time = p->row_time.p;
  }
  return g;
}

static int project_run(sbm_project* p, const double* Theta, int V, const sbm_integrator_opts* opts, bool sens,
                       double* sims, double* Rout, double* J, double* Jmodel, double* sf, double* sf_grad, double* norms,
                       double* grad, int32_t* status, int32_t* n_steps, const char* who) {
  if (!p || !Theta || !Rout) return sbm_fail(SBM_E_ARG, "%s: NULL argument", who);
  if (V < 0) return sbm_fail(SBM_E_ARG, "%s: V < 0", who);
  int rc = check_opts(opts, who);
  if (rc) return rc;
  if (V == 0) return 0;
  sbm_model* m = p->model;
  SBM_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const size_t T = (size_t)V * p->E;
  const int NV = p->n_vars, NK = p->n_sens, NP = p->n_params, nt = p->n_t_max;
  // scratch reallocation must not race with kernels of an earlier call still using it
  const bool grow = T * NP > p->P.n || T * nt * NV > p->Y.n || (sens && T * nt * NV * NK > p->S.n) ||
                    T > p->traj_status.n || (size_t)V * p->R > p->sims.n;
  if (grow) SBM_HIP(hipStreamSynchronize(s));
  if (p->P.reserve(T * NP) || p->Y.reserve(T * nt * NV) || (sens && p->S.reserve(T * nt * NV * NK)) ||
      p->traj_status.reserve(T) || p->traj_steps.reserve(T) || p->traj_rej.reserve(T) || p->goff.reserve(T) ||
      p->glen.reserve(T) || p->sims.reserve((size_t)V * (p->R > 0 ? p->R : 1)))
    return sbm_fail(SBM_E_HIP, "%s: out of device memory for %d vectors (%lld bytes of scratch)", who, V,
                    (long long)sbm_project_scratch_bytes(p, V, sens));
  if (p->scratch_V != V) {
    hipLaunchKernelGGL(k_fill_grids, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, p->tgrid_off.p, V, p->E,
                       p->goff.p, p->glen.p);
    p->scratch_V = V;
  }
  {
    const size_t total = T * NP;
    hipLaunchKernelGGL(k_gather_params, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Theta, p->pmap.p,
                       p->pfixed.p, V, p->E, NP, p->q, p->P.p);
  }
  sbm_kernel_args a;
  memset(&a, 0, sizeof(a));
  a.P = p->P.p; a.t_out = p->tgrid.p; a.grid_off = p->goff.p; a.grid_len = p->glen.p;
  a.Y = p->Y.p; a.S = sens ? p->S.p : nullptr;
  a.status = p->traj_status.p; a.n_steps = p->traj_steps.p; a.n_reject = p->traj_rej.p;
  a.n_traj = (int32_t)T; a.n_t = nt; a.opts = *opts;
  rc = sens ? launch_sens(m, a, who) : launch(m, SBM_KIND_STATE, a, who);
  if (rc) return rc;
  const int levels = (opts->method == SBM_IMPLICIT_MIDPOINT || opts->method == SBM_IMPLICIT_MIDPOINT_GRADED) ? p->richardson : 0;
  if (levels > 0) {
    // the same ensemble again with every step halved (and halved again), then the combination in place
    const size_t nY = T * nt * NV, nS = T * nt * NV * NK;
    const bool grow2 = nY > p->Yx[0].n || (levels > 1 && nY > p->Yx[1].n) || (sens && (nS > p->Sx[0].n || (levels > 1 && nS > p->Sx[1].n))) ||
                       T > p->statx.n;
    if (grow2) SBM_HIP(hipStreamSynchronize(s));
    if (p->statx.reserve(T) || p->stepsx.reserve(T)) return sbm_fail(SBM_E_HIP, "%s: out of device memory", who);
    const int mult0 = opts->step_mult > 0 ? opts->step_mult : 1;
    for (int l = 0; l < levels; ++l) {
      if (p->Yx[l].reserve(nY) || (sens && p->Sx[l].reserve(nS))) return sbm_fail(SBM_E_HIP, "%s: out of device memory", who);
      sbm_kernel_args b = a;
      b.Y = p->Yx[l].p; b.S = sens ? p->Sx[l].p : nullptr;
      b.status = p->statx.p; b.n_steps = p->stepsx.p; b.n_reject = nullptr;
      b.opts.step_mult = mult0 << (l + 1);
      rc = sens ? launch_sens(m, b, who) : launch(m, SBM_KIND_STATE, b, who);
      if (rc) return rc;
      hipLaunchKernelGGL(k_merge_status, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, p->traj_status.p,
                         p->traj_steps.p, p->statx.p, p->stepsx.p, (int)T);
    }
    hipLaunchKernelGGL(k_richardson, dim3((unsigned)((nY + 255) / 256)), dim3(256), 0, s, p->Y.p, p->Yx[0].p,
                       levels > 1 ? p->Yx[1].p : nullptr, nY, levels);
    if (sens)
      hipLaunchKernelGGL(k_richardson, dim3((unsigned)((nS + 255) / 256)), dim3(256), 0, s, p->S.p, p->Sx[0].p,
                         levels > 1 ? p->Sx[1].p : nullptr, nS, levels);
    SBM_HIP(hipGetLastError());
  }

  AssembleArgs g = assemble_args(p);
  g.Theta = Theta; g.Y = p->Y.p; g.S = sens ? p->S.p : nullptr;
  g.traj_status = p->traj_status.p; g.traj_steps = p->traj_steps.p;
  g.sims = sims ? sims : p->sims.p; g.Rout = Rout; g.sf = sf; g.norms = norms; g.status = status; g.n_steps = n_steps;
  g.J = sens ? J : nullptr; g.Jmodel = sens ? Jmodel : nullptr; g.grad = sens ? grad : nullptr;
  g.sf_grad = sens ? sf_grad : nullptr;
  return launch_assemble(m->ctx, g, V, who);
}

extern "C" int sbm_residuals_batch(sbm_project* p, const double* Theta, int32_t V, const sbm_integrator_opts* opts,
                                   double* sims, double* Rout, double* sf, double* norms, int32_t* status,
                                   int32_t* n_steps) {
  return project_run(p, Theta, V, opts, false, sims, Rout, nullptr, nullptr, sf, nullptr, norms, nullptr, status, n_steps,
                     "sbm_residuals_batch");
}

extern "C" int sbm_jacobian_batch(sbm_project* p, const double* Theta, int32_t V, const sbm_integrator_opts* opts,
                                  double* sims, double* Rout, double* J, double* Jmodel, double* sf, double* sf_grad,
                                  double* norms, double* grad, int32_t* status, int32_t* n_steps) {
  if (!J && !Jmodel) return sbm_fail(SBM_E_ARG, "sbm_jacobian_batch: J and Jmodel both NULL");
  if (grad && !J) return sbm_fail(SBM_E_ARG, "sbm_jacobian_batch: grad needs J");
  return project_run(p, Theta, V, opts, true, sims, Rout, J, Jmodel, sf, sf_grad, norms, grad, status, n_steps,
                     "sbm_jacobian_batch");
}

// ---------------------------------------------------------------------------------------------
// Loss functions on caller-supplied simulations (the reference's frame-level API, a13):
// the same assembly kernel, reading sims / the model Jacobian from the caller instead of Y / S.
// ---------------------------------------------------------------------------------------------
namespace {
struct LossFrames {   // device copies of one sbm_loss_eval_host call
  DevBuf<double> data, sigma, spm, sps, sims, Jm, R, J, sf, sfg, norms;
  DevBuf<int32_t> sfi, plain, spg, status;
};
}  // namespace

// uploads, the kernel and the copies back, all on the context's stream; returns at the first failure with whatever is
// already enqueued still running on `b`
static int loss_eval_enqueue(sbm_ctx* ctx, const sbm_loss_desc* d, int V, const double* sims, const double* Jm, double* Rout,
                             double* J, double* sf, double* sf_grad, double* norms, int32_t* status, LossFrames& b,
                             const char* who) {
  hipStream_t s = ctx->stream;
  const int R = d->n_rows, q = d->n_params, G = d->n_sf_groups, NSP = d->n_sf_prior_rows;
  const int RT = R + NSP, qq = q > 0 ? q : 1;
  int bad = 0;
  bad |= upload(b.data, d->row_data, (size_t)R, s);
  bad |= upload(b.sigma, d->row_sigma, (size_t)R, s);
  bad |= upload(b.sfi, d->row_sf, (size_t)R, s);
  if (d->row_plain) bad |= upload(b.plain, d->row_plain, (size_t)R, s);
  bad |= upload(b.spg, d->sf_prior_group, (size_t)NSP, s);
  bad |= upload(b.spm, d->sf_prior_mean, (size_t)NSP, s);
  bad |= upload(b.sps, d->sf_prior_sigma, (size_t)NSP, s);
  bad |= upload(b.sims, sims, (size_t)V * R, s);
  if (Jm) bad |= upload(b.Jm, Jm, (size_t)V * R * q, s);
  bad |= b.R.reserve((size_t)V * RT) | b.sf.reserve((size_t)V * (G ? G : 1)) | b.norms.reserve(V) | b.status.reserve(V);
  if (J) bad |= b.J.reserve((size_t)V * RT * qq);
  if (Jm) bad |= b.sfg.reserve((size_t)V * (G ? G : 1) * qq);
  if (bad) return sbm_fail(SBM_E_HIP, "%s: device allocation / upload failed", who);
  AssembleArgs g;
  memset(&g, 0, sizeof(g));
  g.E = 1; g.q = qq; g.R = R; g.G = G; g.NPR = 0; g.NSP = NSP;
  g.compat = d->reference_compat; g.loss = d->loss_type;
  g.row_sf = b.sfi.p; g.row_data = b.data.p; g.row_sigma = b.sigma.p; g.row_plain = d->row_plain ? b.plain.p : nullptr;
  g.sfp_group = b.spg.p; g.sfp_mean = b.spm.p; g.sfp_sigma = b.sps.p;
  g.sims_in = b.sims.p; g.Jm_in = Jm ? b.Jm.p : nullptr;
  g.Rout = b.R.p; g.sf = b.sf.p; g.norms = b.norms.p; g.status = b.status.p;
  g.J = J ? b.J.p : nullptr; g.sf_grad = Jm ? b.sfg.p : nullptr;
  if (int rc = launch_assemble(ctx, g, V, who)) return rc;
  hipError_t e = hipMemcpyAsync(Rout, b.R.p, (size_t)V * RT * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && J) e = hipMemcpyAsync(J, b.J.p, (size_t)V * RT * q * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && sf && G) e = hipMemcpyAsync(sf, b.sf.p, (size_t)V * G * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && sf_grad && G) e = hipMemcpyAsync(sf_grad, b.sfg.p, (size_t)V * G * q * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && norms) e = hipMemcpyAsync(norms, b.norms.p, (size_t)V * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && status) e = hipMemcpyAsync(status, b.status.p, (size_t)V * 4, hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) return sbm_fail(SBM_E_HIP, "%s: %s", who, hipGetErrorString(e));
  return 0;
}

extern "C" int sbm_loss_eval_host(sbm_ctx* ctx, const sbm_loss_desc* d, int32_t V, const double* sims, const double* Jm,
                                  double* Rout, double* J, double* sf, double* sf_grad, double* norms, int32_t* status) {
  const char* who = "sbm_loss_eval_host";
  if (!ctx || !d || !sims || !Rout) return sbm_fail(SBM_E_ARG, "%s: NULL argument", who);
  if (int rc = sbm_loss_desc_check(d, V, Jm != nullptr, J || sf_grad, who, g_err, sizeof(g_err))) return rc;
  if (V == 0) return 0;
  SBM_HIP(hipSetDevice(ctx->device));
  // The frames outlive everything enqueued on them: they are freed when this function returns, and however the
  // enqueueing ended, the one return below comes after the stream has drained.
  LossFrames b;
  const int rc = loss_eval_enqueue(ctx, d, V, sims, Jm, Rout, J, sf, sf_grad, norms, status, b, who);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (rc == 0 && e != hipSuccess) return sbm_fail(SBM_E_HIP, "%s: %s", who, hipGetErrorString(e));
  return rc;
}

// ---------------------------------------------------------------------------------------------
// The fitting loop (kernels: sbm_lm.hpp): the batched Levenberg-Marquardt step, the trust-region step with lmder's
// search for the Levenberg-Marquardt parameter, and lmder's bookkeeping between two steps.
// ---------------------------------------------------------------------------------------------
extern "C" int sbm_lm_step(sbm_ctx* ctx, const double* J, const double* r, const double* lambda, int32_t V, int32_t M,
                           int32_t q, double* delta, double* pred, int32_t* status) {
  if (!ctx || !J || !r || !lambda || !delta || !pred || !status) return sbm_fail(SBM_E_ARG, "sbm_lm_step: NULL argument");
  if (V < 0 || M <= 0 || q <= 0 || q > LM_MAX_Q) return sbm_fail(SBM_E_ARG, "sbm_lm_step: bad sizes V=%d M=%d q=%d (q <= %d)", V, M, q, LM_MAX_Q);
  if (V == 0) return 0;
  int tile = 0;
  const size_t lds = lm_lds_bytes(q, 3, (size_t)lm_lds_limit(ctx), &tile);
  if (!lds) return sbm_fail(SBM_E_ARG, "sbm_lm_step: q = %d does not fit the %d KB of LDS of a workgroup", q, lm_lds_limit(ctx) / 1024);
  LmArgs a{J, r, lambda, delta, pred, status, M, q, tile};
  return launch_lds(ctx, k_lm_step, dim3(V), dim3(256), lds, a);
}

// held = NULL: k_lm_trust, as before sbm_lm_trust_step_held existed (lm_lds_bytes does not count its 304 bytes of static
// LDS); otherwise k_lm_trust_held, whose whole static LDS (LM_HELD_STATIC_LDS = 576 bytes: the same 304 + the list of free
// columns and the waves' counts) is taken off the limit the row tile is chosen for, so that dynamic + static fit the
// workgroup at every q.  The tile decides how many rows are staged at once, not the order of any sum.
// bounds != NULL: k_lm_trust_bounded (held nullable, the same static LDS as k_lm_trust_held).
static int lm_trust_launch(sbm_ctx* ctx, const double* J, const double* r, double* dscale, const double* radius, double* lambda,
                           int32_t V, int32_t M, int32_t q, const double* row_scale, const int32_t* skip, double max_step,
                           const double* theta, double* trial, double* delta, double* pred, double* dxnorm, double* gtx,
                           int32_t* status, const int32_t* held, const LmBounds* bounds = nullptr) {
  if (!ctx || !J || !r || !dscale || !radius || !lambda || !delta || !pred || !dxnorm || !status)
    return sbm_fail(SBM_E_ARG, "sbm_lm_trust_step: NULL argument");
  if (V < 0 || M <= 0 || q <= 0 || q > LM_MAX_Q) return sbm_fail(SBM_E_ARG, "sbm_lm_trust_step: bad sizes V=%d M=%d q=%d (q <= %d)", V, M, q, LM_MAX_Q);
  if ((theta == nullptr) != (trial == nullptr)) return sbm_fail(SBM_E_ARG, "sbm_lm_trust_step_ex: theta and trial go together");
  if (V == 0) return 0;
  int tile = 0;
  const size_t lds = lm_lds_bytes(q, 5, (size_t)lm_lds_limit(ctx) - (held || bounds ? LM_HELD_STATIC_LDS : 0), &tile);
  if (!lds) return sbm_fail(SBM_E_ARG, "sbm_lm_trust_step: q = %d does not fit the %d KB of LDS of a workgroup", q, lm_lds_limit(ctx) / 1024);
  LmTrustArgs a{J, r, dscale, radius, lambda, delta, pred, dxnorm, status, M, q, tile, row_scale, skip, max_step, gtx, theta, trial};
  if (bounds) return launch_lds(ctx, k_lm_trust_bounded, dim3(V), dim3(256), lds, a, held, *bounds);
  if (held) return launch_lds(ctx, k_lm_trust_held, dim3(V), dim3(256), lds, a, held);
  return launch_lds(ctx, k_lm_trust, dim3(V), dim3(256), lds, a);
}

extern "C" int sbm_lm_trust_step_ex(sbm_ctx* ctx, const double* J, const double* r, double* dscale, const double* radius,
                                    double* lambda, int32_t V, int32_t M, int32_t q, const double* row_scale,
                                    const int32_t* skip, double max_step, const double* theta, double* trial, double* delta,
                                    double* pred, double* dxnorm, double* gtx, int32_t* status) {
  return lm_trust_launch(ctx, J, r, dscale, radius, lambda, V, M, q, row_scale, skip, max_step, theta, trial, delta, pred, dxnorm,
                         gtx, status, nullptr);
}

extern "C" int sbm_lm_trust_step_held(sbm_ctx* ctx, const double* J, const double* r, double* dscale, const double* radius,
                                      double* lambda, int32_t V, int32_t M, int32_t q, const double* row_scale,
                                      const int32_t* skip, double max_step, const double* theta, double* trial, double* delta,
                                      double* pred, double* dxnorm, double* gtx, int32_t* status, const int32_t* held) {
  return lm_trust_launch(ctx, J, r, dscale, radius, lambda, V, M, q, row_scale, skip, max_step, theta, trial, delta, pred, dxnorm,
                         gtx, status, held);
}

extern "C" int sbm_lm_trust_step_bounded(sbm_ctx* ctx, const double* J, const double* r, double* dscale, const double* radius,
                                         double* lambda, int32_t V, int32_t M, int32_t q, const double* row_scale,
                                         const int32_t* skip, double max_step, const double* theta, double* trial,
                                         double* delta, double* pred, double* dxnorm, double* gtx, int32_t* status,
                                         const int32_t* held, const double* lower, const double* upper, int32_t* active_out) {
  if (!theta || !trial || !lower || !upper)
    return sbm_fail(SBM_E_ARG, "sbm_lm_trust_step_bounded: theta, trial, lower and upper are needed");
  const LmBounds bounds{lower, upper, active_out};
  return lm_trust_launch(ctx, J, r, dscale, radius, lambda, V, M, q, row_scale, skip, max_step, theta, trial, delta, pred, dxnorm,
                         gtx, status, held, &bounds);
}

extern "C" int sbm_lm_trust_step(sbm_ctx* ctx, const double* J, const double* r, double* dscale, const double* radius,
                                 double* lambda, int32_t V, int32_t M, int32_t q, double* delta, double* pred,
                                 double* dxnorm, int32_t* status) {
  return sbm_lm_trust_step_ex(ctx, J, r, dscale, radius, lambda, V, M, q, nullptr, nullptr, 0.0, nullptr, nullptr, delta, pred,
                              dxnorm, nullptr, status);
}

// The geodesic acceleration of the step a trust-step call just produced (kernel: sbm_lm_geodesic.hpp).  held = NULL:
// k_lm_geodesic<false>, else the compacting instantiation.  The kernel's static LDS (LM_GEO_STATIC_LDS) is taken off the
// limit the row tile is chosen for, as for the held trust step.
extern "C" int sbm_lm_geodesic(sbm_ctx* ctx, const double* J, const double* r, const double* r_base, const double* r_probe,
                               const int32_t* status_base, const int32_t* status_probe, const double* dscale,
                               const double* lambda, int32_t V, int32_t M, int32_t q, const double* row_scale,
                               const int32_t* skip, const int32_t* step_status, const int32_t* held, double h, double alpha,
                               double max_step, const double* theta, double* delta, double* trial, double* pred,
                               double* dxnorm, double* gtx, int32_t* accel_status, double* ratio_out, int32_t* n_accel) {
  if (!ctx || !J || !r || !r_probe || !dscale || !lambda || !step_status || !theta || !delta || !trial || !pred || !dxnorm || !gtx ||
      !accel_status)
    return sbm_fail(SBM_E_ARG, "sbm_lm_geodesic: NULL argument");
  if (V < 0 || M <= 0 || q <= 0 || q > LM_MAX_Q) return sbm_fail(SBM_E_ARG, "sbm_lm_geodesic: bad sizes V=%d M=%d q=%d (q <= %d)", V, M, q, LM_MAX_Q);
  if (!(h > 0.0) || !(h < 1.0e300)) return sbm_fail(SBM_E_ARG, "sbm_lm_geodesic: the probe length h = %g has to be positive", h);
  if (!(alpha >= 0.0)) return sbm_fail(SBM_E_ARG, "sbm_lm_geodesic: the gate alpha = %g has to be >= 0", alpha);
  if (V == 0) return 0;
  int tile = 0;
  const size_t lds = lm_lds_bytes(q, 4, (size_t)lm_lds_limit(ctx) - LM_GEO_STATIC_LDS, &tile);
  if (!lds) return sbm_fail(SBM_E_ARG, "sbm_lm_geodesic: q = %d does not fit the %d KB of LDS of a workgroup", q, lm_lds_limit(ctx) / 1024);
  LmGeodesicArgs a{J, r, r_base, r_probe, status_base, status_probe, dscale, lambda, row_scale, skip, step_status, theta, delta, trial,
                   pred, dxnorm, gtx, accel_status, ratio_out, n_accel, h, alpha, max_step, M, q, tile};
  if (held) return launch_lds(ctx, k_lm_geodesic<true>, dim3(V), dim3(256), lds, a, held);
  return launch_lds(ctx, k_lm_geodesic<false>, dim3(V), dim3(256), lds, a, held);
}

extern "C" int sbm_lm_update(sbm_ctx* ctx, const double* cost, const double* norms_trial, const int32_t* status_trial,
                             const double* pred, const double* dxnorm, const double* gtx, const int32_t* step_status,
                             const double* theta, const double* dscale, int32_t V, int32_t q, double ftol, double xtol,
                             int32_t iteration, int32_t first, double* radius, double* lambda, int32_t* done, int32_t* accept,
                             int32_t* n_iter, int32_t* counters, double* ratio_out) {
  if (!ctx || !cost || !norms_trial || !status_trial || !pred || !dxnorm || !gtx || !step_status || !theta || !dscale ||
      !radius || !lambda || !done || !accept || !n_iter || !counters)
    return sbm_fail(SBM_E_ARG, "sbm_lm_update: NULL argument");
  if (V < 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_lm_update: bad sizes V=%d q=%d", V, q);
  SBM_HIP(hipSetDevice(ctx->device));
  SBM_HIP(hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), ctx->stream));
  if (V == 0) return 0;
  LmUpdateArgs a{cost, norms_trial, status_trial, pred, dxnorm, gtx, step_status, theta, dscale, radius, lambda, done, accept,
                 n_iter, counters, ratio_out, ftol, xtol, V, q, iteration, first};
  hipLaunchKernelGGL(k_lm_update, dim3((V + 255) / 256), dim3(256), 0, ctx->stream, a);
  SBM_HIP(hipGetLastError());
  return 0;
}

extern "C" int sbm_lm_accept(sbm_ctx* ctx, const int32_t* accept, int32_t V, int32_t M, int32_t q, const double* trial,
                             const double* r_trial, const double* J_trial, const double* norms_trial, double* theta,
                             double* r, double* J, double* cost) {
  if (!ctx || !accept || !trial || !r_trial || !J_trial || !norms_trial || !theta || !r || !J || !cost)
    return sbm_fail(SBM_E_ARG, "sbm_lm_accept: NULL argument");
  if (V < 0 || M <= 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_lm_accept: bad sizes V=%d M=%d q=%d", V, M, q);
  if (V == 0) return 0;
  SBM_HIP(hipSetDevice(ctx->device));
  const int ny = (int)(((size_t)M * q / 2 + 256 * 8 - 1) / (256 * 8));       // ~8 double2 per thread
  hipLaunchKernelGGL(k_lm_accept, dim3(V, ny < 1 ? 1 : (ny > 64 ? 64 : ny)), dim3(256), 0, ctx->stream, accept, q, M, trial, r_trial,
                     J_trial, norms_trial, theta, r, J, cost);
  SBM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The Metropolis sampler's step on the device (kernels: sbm_sampler.hpp, sbm_sampling_axes.hpp): scale-factor entropy
// of the trial simulations, candidate move, and the acceptance rules of its two algorithms -- Metropolis with fixed axes
// (project/ensembles.py, sampler='device'), and Hastings with axes of the candidate density from the Hessian at every
// chain's point (sampler='device_recalc').
// ---------------------------------------------------------------------------------------------
extern "C" int sbm_project_sf_entropy(sbm_project* p, const double* sims, int32_t V, double temperature, double* entropy,
                                      double* group_entropy) {
  if (!p || !sims || !entropy) return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy: NULL argument");
  if (V < 0) return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy: V < 0");
  if (!(temperature > 0.0)) return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy: temperature must be positive");
  if (p->G <= 0) return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy: the project has no scale factors");
  if (p->sf_group_without_prior >= 0)
    return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy: scale factor entropy needs a log prior on every scale factor (group %d has none)",
                    p->sf_group_without_prior);
  if (V == 0) return 0;
  return launch_lds(p->model->ctx, k_sf_entropy, dim3(V), dim3(256), sizeof(double) * (size_t)p->G, sims, p->R, p->G, p->row_data.p,
                    p->row_sigma.p, p->row_sf.p, p->sfg_mean.p, p->sfg_sigma.p, temperature, entropy, group_entropy);
}

extern "C" int sbm_project_sf_entropy_pt(sbm_project* p, const double* sims, int32_t V, const double* temperature, double* entropy,
                                         double* group_entropy) {
  if (!p || !sims || !temperature || !entropy) return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy_pt: NULL argument");
  if (V < 0) return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy_pt: V < 0");
  if (p->G <= 0) return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy_pt: the project has no scale factors");
  if (p->sf_group_without_prior >= 0)
    return sbm_fail(SBM_E_ARG, "sbm_project_sf_entropy_pt: scale factor entropy needs a log prior on every scale factor (group %d has none)",
                    p->sf_group_without_prior);
  if (V == 0) return 0;
  return launch_lds(p->model->ctx, k_sf_entropy_pt, dim3(V), dim3(256), sizeof(double) * (size_t)p->G, sims, p->R, p->G, p->row_data.p,
                    p->row_sigma.p, p->row_sf.p, p->sfg_mean.p, p->sfg_sigma.p, temperature, entropy, group_entropy);
}

extern "C" int sbm_mh_propose(sbm_ctx* ctx, const double* curr, const double* samp, int32_t per_chain, const double* z, int32_t C,
                              int32_t q, double* trial) {
  if (!ctx || !curr || !samp || !z || !trial) return sbm_fail(SBM_E_ARG, "sbm_mh_propose: NULL argument");
  if (C < 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_mh_propose: bad sizes C=%d q=%d", C, q);
  if (C == 0) return 0;
  SBM_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)C * q;
  hipLaunchKernelGGL(k_mh_propose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, curr, samp, per_chain, z, C, q, trial);
  SBM_HIP(hipGetLastError());
  return 0;
}

extern "C" int sbm_mh_propose_box(sbm_ctx* ctx, const double* curr, const double* samp, int32_t per_chain, const double* z, int32_t C,
                                  int32_t q, const int32_t* held, const double* lower, const double* upper, double* trial,
                                  int32_t* outside) {
  if (!ctx || !curr || !samp || !z || !trial || !outside) return sbm_fail(SBM_E_ARG, "sbm_mh_propose_box: NULL argument");
  if ((lower == nullptr) != (upper == nullptr)) return sbm_fail(SBM_E_ARG, "sbm_mh_propose_box: lower and upper go together");
  if (trial == curr) return sbm_fail(SBM_E_ARG, "sbm_mh_propose_box: trial must not be curr");
  if (C < 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_mh_propose_box: bad sizes C=%d q=%d", C, q);
  if (C == 0) return 0;
  SBM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_mh_propose_box, dim3((C + 3) / 4), dim3(256), 0, ctx->stream, curr, samp, per_chain, z, C, q, held, lower, upper,
                     trial, outside);
  SBM_HIP(hipGetLastError());
  return 0;
}

extern "C" int sbm_mh_accept_ex(sbm_ctx* ctx, const double* norms_trial, const int32_t* status_trial, const double* entropy_trial,
                                const double* log_u, double temperature, int32_t C, int32_t q, const double* trial, double* curr,
                                double* F_curr, int32_t* n_accepted, double* ens_slot, double* ens_F_slot, const int32_t* veto) {
  if (!ctx || !norms_trial || !status_trial || !log_u || !trial || !curr || !F_curr || !n_accepted)
    return sbm_fail(SBM_E_ARG, "sbm_mh_accept: NULL argument");
  if (C < 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_mh_accept: bad sizes C=%d q=%d", C, q);
  if (!(temperature > 0.0)) return sbm_fail(SBM_E_ARG, "sbm_mh_accept: temperature must be positive");
  if (C == 0) return 0;
  sbm_mh_args a{norms_trial, status_trial, entropy_trial, log_u, temperature, C, q, trial, curr, F_curr, n_accepted, ens_slot, ens_F_slot,
                veto};
  SBM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_mh_accept, dim3((C + 3) / 4), dim3(256), 0, ctx->stream, a);
  SBM_HIP(hipGetLastError());
  return 0;
}

extern "C" int sbm_mh_accept_pt(sbm_ctx* ctx, const double* norms_trial, const int32_t* status_trial, const double* entropy_trial,
                                const double* log_u, const double* temperature, int32_t C, int32_t q, const double* trial, double* curr,
                                double* F_curr, int32_t* n_accepted, double* ens_slot, double* ens_F_slot, const int32_t* veto) {
  if (!ctx || !norms_trial || !status_trial || !log_u || !temperature || !trial || !curr || !F_curr || !n_accepted)
    return sbm_fail(SBM_E_ARG, "sbm_mh_accept_pt: NULL argument");
  if (C < 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_mh_accept_pt: bad sizes C=%d q=%d", C, q);
  if (C == 0) return 0;
  sbm_mh_args a{norms_trial, status_trial, entropy_trial, log_u, 0.0, C, q, trial, curr, F_curr, n_accepted, ens_slot, ens_F_slot, veto};
  SBM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_mh_accept_pt, dim3((C + 3) / 4), dim3(256), 0, ctx->stream, a, temperature);
  SBM_HIP(hipGetLastError());
  return 0;
}

extern "C" int sbm_pt_swap(sbm_ctx* ctx, int32_t C, int32_t q, int32_t K, int32_t parity, const double* temperature,
                           const double* F_cross, const double* log_u, double* curr, double* F_curr, int32_t* n_swapped,
                           double* ens_slot, double* ens_F_slot) {
  if (!ctx || !temperature || !log_u || !curr || !F_curr || !n_swapped) return sbm_fail(SBM_E_ARG, "sbm_pt_swap: NULL argument");
  if (C < 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_pt_swap: bad sizes C=%d q=%d", C, q);
  if (K < 2 || C % K != 0) return sbm_fail(SBM_E_ARG, "sbm_pt_swap: C=%d chains are not ladders of K=%d >= 2 rungs", C, K);
  if (parity != 0 && parity != 1) return sbm_fail(SBM_E_ARG, "sbm_pt_swap: parity %d is neither 0 nor 1", parity);
  if (C == 0) return 0;
  sbm_pt_swap_args a{C, q, K, parity, temperature, F_cross, log_u, curr, F_curr, n_swapped, ens_slot, ens_F_slot};
  SBM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_pt_swap, dim3((C + 3) / 4), dim3(256), 0, ctx->stream, a);
  SBM_HIP(hipGetLastError());
  return 0;
}

extern "C" int sbm_mh_accept(sbm_ctx* ctx, const double* norms_trial, const int32_t* status_trial, const double* entropy_trial,
                             const double* log_u, double temperature, int32_t C, int32_t q, const double* trial, double* curr,
                             double* F_curr, int32_t* n_accepted, double* ens_slot, double* ens_F_slot) {
  return sbm_mh_accept_ex(ctx, norms_trial, status_trial, entropy_trial, log_u, temperature, C, q, trial, curr, F_curr, n_accepted,
                          ens_slot, ens_F_slot, nullptr);
}

// held = NULL: k_sampling_axes, as before sbm_sampling_axes_held existed; otherwise k_sampling_axes_held, whose static LDS
// (the list of free columns and the waves' counts, read from the code object) has to fit the workgroup together with the
// dynamic block: the same dynamic size, since the free columns are at most q.
static_assert(AXES_MAX_Q == SBM_SAMPLING_AXES_MAX_Q, "the index list of k_sampling_axes_held holds SBM_SAMPLING_AXES_MAX_Q columns");
extern "C" int sbm_sampling_axes_held(sbm_ctx* ctx, const double* J, const double* row_scale, const double* H, int32_t per_chain_H,
                                      int32_t C, int32_t M, int32_t q, double cutoff, double temperature, double step_scale,
                                      double* eig, double* V, double* s, double* samp, int32_t* status, const int32_t* held) {
  if (!ctx || !status) return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: NULL argument");
  if ((J == nullptr) == (H == nullptr)) return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: exactly one of J and H must be given");
  if (H && row_scale) return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: row_scale goes with J");
  if (C < 0 || q <= 0 || (J && M <= 0)) return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: bad sizes C=%d M=%d q=%d", C, M, q);
  if (q > SBM_SAMPLING_AXES_MAX_Q)
    return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: q = %d; two q x (q + 1) matrices are kept in the LDS of one workgroup, which holds "
                    "SBM_SAMPLING_AXES_MAX_Q = %d", q, SBM_SAMPLING_AXES_MAX_Q);
  if (!(cutoff >= 0.0) || !(temperature > 0.0) || !(step_scale > 0.0))
    return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: cutoff must be >= 0, temperature and step_scale positive");
  if (C == 0) return 0;
  const size_t lds = sbm_axes_lds_bytes(q);
  if (lds > (size_t)lm_lds_limit(ctx))
    return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: q = %d does not fit the %d KB of LDS of a workgroup", q, lm_lds_limit(ctx) / 1024);
  sbm_axes_args a{J, row_scale, H, per_chain_H, M, q, cutoff, temperature, step_scale, eig, V, s, samp, status};
  if (!held) return launch_lds(ctx, k_sampling_axes, dim3(C), dim3(256), lds, a);
  static const size_t stat = [] {   // asked once: the kernel is the same on every device
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, (const void*)k_sampling_axes_held) == hipSuccess ? (size_t)fa.sharedSizeBytes : (size_t)256;
  }();
  if (lds + stat > (size_t)lm_lds_limit(ctx))
    return sbm_fail(SBM_E_ARG, "sbm_sampling_axes: q = %d does not fit the %d KB of LDS of a workgroup (%zu B + %zu B static)", q,
                    lm_lds_limit(ctx) / 1024, lds, stat);
  return launch_lds(ctx, k_sampling_axes_held, dim3(C), dim3(256), lds, a, held);
}

extern "C" int sbm_sampling_axes(sbm_ctx* ctx, const double* J, const double* row_scale, const double* H, int32_t per_chain_H,
                                 int32_t C, int32_t M, int32_t q, double cutoff, double temperature, double step_scale,
                                 double* eig, double* V, double* s, double* samp, int32_t* status) {
  return sbm_sampling_axes_held(ctx, J, row_scale, H, per_chain_H, C, M, q, cutoff, temperature, step_scale, eig, V, s, samp, status,
                                nullptr);
}

extern "C" int sbm_mh_accept_hastings_ex(sbm_ctx* ctx, const double* norms_trial, const int32_t* status_trial,
                                         const double* entropy_trial, const double* log_u, double temperature, int32_t C, int32_t q,
                                         const double* trial, double* curr, double* F_curr, int32_t* n_accepted, double* ens_slot,
                                         double* ens_F_slot, double* V_curr, double* s_curr, double* samp_curr, const double* V_trial,
                                         const double* s_trial, const double* samp_trial, const int32_t* axes_status_trial,
                                         const int32_t* veto) {
  if (!ctx || !norms_trial || !status_trial || !log_u || !trial || !curr || !F_curr || !n_accepted || !V_curr || !s_curr ||
      !samp_curr || !V_trial || !s_trial || !samp_trial || !axes_status_trial)
    return sbm_fail(SBM_E_ARG, "sbm_mh_accept_hastings: NULL argument");
  if (C < 0 || q <= 0) return sbm_fail(SBM_E_ARG, "sbm_mh_accept_hastings: bad sizes C=%d q=%d", C, q);
  if (!(temperature > 0.0)) return sbm_fail(SBM_E_ARG, "sbm_mh_accept_hastings: temperature must be positive");
  if (C == 0) return 0;
  const size_t lds = sizeof(double) * (size_t)q;
  if (lds > (size_t)lm_lds_limit(ctx)) return sbm_fail(SBM_E_ARG, "sbm_mh_accept_hastings: q = %d does not fit the LDS of a workgroup", q);
  sbm_mh_hastings_args a{{norms_trial, status_trial, entropy_trial, log_u, temperature, C, q, trial, curr, F_curr, n_accepted,
                          ens_slot, ens_F_slot, veto}, V_curr, s_curr, samp_curr, V_trial, s_trial, samp_trial, axes_status_trial};
  return launch_lds(ctx, k_mh_accept_hastings, dim3(C), dim3(256), lds, a);
}

extern "C" int sbm_mh_accept_hastings(sbm_ctx* ctx, const double* norms_trial, const int32_t* status_trial,
                                      const double* entropy_trial, const double* log_u, double temperature, int32_t C, int32_t q,
                                      const double* trial, double* curr, double* F_curr, int32_t* n_accepted, double* ens_slot,
                                      double* ens_F_slot, double* V_curr, double* s_curr, double* samp_curr, const double* V_trial,
                                      const double* s_trial, const double* samp_trial, const int32_t* axes_status_trial) {
  return sbm_mh_accept_hastings_ex(ctx, norms_trial, status_trial, entropy_trial, log_u, temperature, C, q, trial, curr, F_curr,
                                   n_accepted, ens_slot, ens_F_slot, V_curr, s_curr, samp_curr, V_trial, s_trial, samp_trial,
                                   axes_status_trial, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Ensemble predictions: statistics over the member axis (kernels and the work split: sbm_ensemble_stats.hpp).
// ---------------------------------------------------------------------------------------------
extern "C" int sbm_ensemble_stats(sbm_ctx* ctx, const double* values, const int32_t* status, int32_t V, int64_t L,
                                  const double* levels, int32_t Q, double* mean, double* sd, double* quant, int32_t* used,
                                  int32_t* n_used) {
  if (!ctx || (!values && V > 0 && L > 0)) return sbm_fail(SBM_E_ARG, "sbm_ensemble_stats: NULL argument");
  if (V < 0 || L < 0 || Q < 0) return sbm_fail(SBM_E_ARG, "sbm_ensemble_stats: bad sizes V=%d L=%lld Q=%d", V, (long long)L, Q);
  if (V > SBM_ENSEMBLE_MAX_MEMBERS)
    return sbm_fail(SBM_E_ARG, "sbm_ensemble_stats: %d members; a column is sorted in the LDS of one workgroup, which holds "
                    "SBM_ENSEMBLE_MAX_MEMBERS = %d", V, SBM_ENSEMBLE_MAX_MEMBERS);
  if (Q > SBM_ENS_MAX_LEVELS) return sbm_fail(SBM_E_ARG, "sbm_ensemble_stats: %d quantile levels (at most %d per call)", Q, SBM_ENS_MAX_LEVELS);
  if (Q > 0 && (!levels || !quant)) return sbm_fail(SBM_E_ARG, "sbm_ensemble_stats: Q > 0 needs levels and quant");
  sbm_ens_levels lv;
  memset(&lv, 0, sizeof(lv));
  for (int i = 0; i < Q; ++i) {
    if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) return sbm_fail(SBM_E_ARG, "sbm_ensemble_stats: level %d = %g is not in [0, 1]", i, levels[i]);
    lv.q[i] = levels[i];
  }
  SBM_HIP(hipSetDevice(ctx->device));
  const size_t nv = (size_t)(V > 0 ? V : 1);
  if (ctx->ens_flag.reserve(nv) || ctx->ens_idx.reserve(nv) || ctx->ens_n.reserve(1))
    return sbm_fail(SBM_E_HIP, "sbm_ensemble_stats: out of device memory");
  hipStream_t s = ctx->stream;
  if (V > 0) hipLaunchKernelGGL(k_ens_valid, dim3((V + 3) / 4), dim3(256), 0, s, values, status, V, L, ctx->ens_flag.p);
  hipLaunchKernelGGL(k_ens_compact, dim3(1), dim3(1024), 0, s, ctx->ens_flag.p, V, ctx->ens_idx.p, ctx->ens_n.p, used, n_used);
  SBM_HIP(hipGetLastError());
  if (L == 0 || (!mean && !sd && Q == 0)) return 0;

  int slots = 1;
  while (slots < V) slots <<= 1;
  const bool wide = slots >= SBM_ENS_PACK_SLOTS;
  int C = 1;
  if (!wide) {
    C = SBM_ENS_PACK_SLOTS / slots;
    if (C > SBM_ENS_PACK_MAX_COLS) C = SBM_ENS_PACK_MAX_COLS;
  }
  const int threads = wide ? 1024 : 256;
  const size_t lds = sizeof(double) * ((size_t)C * (size_t)(C > 1 ? slots + 1 : slots) + (size_t)threads / 64);
  sbm_ens_cols_args a;
  a.n_ptr = ctx->ens_n.p;
  a.L = L;
  a.slots = slots;
  a.cols_per_block = C;
  a.Q = Q;
  a.mean = mean;
  a.sd = sd;
  a.quant = quant;
  a.values = values;
  a.idx = ctx->ens_idx.p;
  const int64_t chunk = (int64_t)C * 0x40000000ll;      // columns of one launch: the grid's x extent
  for (int64_t j0 = 0; j0 < L; j0 += chunk) {
    const int64_t nc = L - j0 < chunk ? L - j0 : chunk;
    a.j0 = j0;
    a.n_cols = (int32_t)nc;
    const unsigned blocks = (unsigned)((nc + C - 1) / C);
    if (int rc = wide ? launch_lds(ctx, k_ens_columns<1024>, dim3(blocks), dim3(1024), lds, a, lv)
                      : launch_lds(ctx, k_ens_columns<256>, dim3(blocks), dim3(256), lds, a, lv))
      return rc;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Chain diagnostics: autocorrelation, tau, half-chain moments; split-R-hat and ESS (kernels, the work split and the LDS
// layout: sbm_chain_diagnostics.hpp).
// ---------------------------------------------------------------------------------------------
extern "C" int sbm_chain_autocorr(sbm_ctx* ctx, const double* values, int32_t N, int64_t S, int64_t step_stride, int32_t K,
                                  double* ac, double* tau, double* moments, int32_t* flags) {
  if (!ctx || ((!values || !ac) && S > 0)) return sbm_fail(SBM_E_ARG, "sbm_chain_autocorr: NULL argument");
  if (S < 0) return sbm_fail(SBM_E_ARG, "sbm_chain_autocorr: bad sizes S=%lld", (long long)S);
  if (N < 2) return sbm_fail(SBM_E_ARG, "sbm_chain_autocorr: %d steps; a series needs N >= 2", N);
  if (N > SBM_CHAIN_MAX_STEPS)
    return sbm_fail(SBM_E_ARG, "sbm_chain_autocorr: %d steps; a series is kept in the LDS of one workgroup, which holds "
                    "SBM_CHAIN_MAX_STEPS = %d (thin the record with step_stride)", N, SBM_CHAIN_MAX_STEPS);
  if (K < 1 || K > N) return sbm_fail(SBM_E_ARG, "sbm_chain_autocorr: %d lags of %d steps (1 <= K <= N)", K, N);
  if (step_stride < S)
    return sbm_fail(SBM_E_ARG, "sbm_chain_autocorr: step_stride %lld < S = %lld", (long long)step_stride, (long long)S);
  if (S == 0) return 0;
  const bool wide = N >= SBM_CHAIN_WIDE_FROM;
  int G = 1;
  if (!wide) {
    while (2 * G <= SBM_CHAIN_PACK_SLOTS / N && 2 * G <= SBM_CHAIN_PACK_MAX) G *= 2;
  }
  const int threads = wide ? 1024 : 256;
  sbm_chain_args a;
  a.step_stride = step_stride;
  a.N = N;
  a.K = K;
  a.G = G;
  a.ld = wide ? N + SBM_CHAIN_PAD : ((N + SBM_CHAIN_PAD) | 1);
  const size_t lds = sizeof(double) * sbm_chain_lds_doubles(threads, G, a.ld);
  const int64_t chunk = (int64_t)G * 0x4000000ll;      // series of one launch: the grid's x extent, n_series in 32 bits
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t ns = S - s0 < chunk ? S - s0 : chunk;
    a.values = values + s0;
    a.n_series = (int32_t)ns;
    a.ac = ac + (size_t)s0 * (size_t)K;
    a.moments = moments ? moments + (size_t)s0 * 4 : nullptr;
    a.flags = flags ? flags + s0 : nullptr;
    const unsigned blocks = (unsigned)((ns + G - 1) / G);
    if (int rc = wide ? launch_lds(ctx, k_chain_autocorr<1024>, dim3(blocks), dim3(1024), lds, a)
                      : launch_lds(ctx, k_chain_autocorr<256>, dim3(blocks), dim3(256), lds, a))
      return rc;
    if (tau) {
      hipLaunchKernelGGL(k_chain_tau, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)a.ac, a.n_series, K,
                         tau + s0, a.flags);
      SBM_HIP(hipGetLastError());
    }
  }
  return 0;
}

extern "C" int sbm_chain_summary(sbm_ctx* ctx, const double* moments, const double* tau, int32_t N, int32_t C, int32_t q,
                                 double* rhat, double* ess) {
  if (!ctx || !moments || !tau || !rhat || !ess) return sbm_fail(SBM_E_ARG, "sbm_chain_summary: NULL argument");
  if (N < 2) return sbm_fail(SBM_E_ARG, "sbm_chain_summary: %d steps; a series needs N >= 2", N);
  if (C < 1 || q < 1) return sbm_fail(SBM_E_ARG, "sbm_chain_summary: bad sizes C=%d q=%d", C, q);
  SBM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_chain_summary, dim3((unsigned)((q + 3) / 4)), dim3(256), 0, ctx->stream, moments, tau, N, C, q, rhat, ess);
  SBM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The one collective of the path: all-gather of the per-vector residual norms.
// RCCL is resolved at run time from whatever instance the process already has loaded -- the one that
// created the caller's communicator -- so that libsbm_hip.so neither links RCCL nor brings a second copy
// into a process whose host framework ships its own.
// ---------------------------------------------------------------------------------------------
typedef int (*sbm_nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);

extern "C" int sbm_allgather_norms(sbm_ctx* ctx, void* nccl_comm, const double* send, int32_t count, double* recv) {
  if (!ctx || !nccl_comm || !send || !recv) return sbm_fail(SBM_E_ARG, "sbm_allgather_norms: NULL argument");
  if (count < 0) return sbm_fail(SBM_E_ARG, "sbm_allgather_norms: count < 0");
  if (count == 0) return 0;
  static sbm_nccl_allgather_fn fn = nullptr;
  if (!fn) {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);      // already in the process?
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);    // no: load the system one
    if (!h) return sbm_fail(SBM_E_PLUGIN, "sbm_allgather_norms: RCCL not found: %s", dlerror());
    fn = (sbm_nccl_allgather_fn)dlsym(h, "ncclAllGather");
    if (!fn) return sbm_fail(SBM_E_PLUGIN, "sbm_allgather_norms: ncclAllGather not found in RCCL");
  }
  SBM_HIP(hipSetDevice(ctx->device));
  const int nccl_double = 8;   // ncclFloat64 (rccl.h)
  const int rc = fn(send, recv, (size_t)count, nccl_double, nccl_comm, ctx->stream);
  if (rc != 0) return sbm_fail(SBM_E_HIP, "sbm_allgather_norms: ncclAllGather returned %d", rc);
  return 0;
}
