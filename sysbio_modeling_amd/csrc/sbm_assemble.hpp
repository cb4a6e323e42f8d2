// sbm_assemble.hpp -- the device half of the Project path (host side: sbm_core.hip):
//   k_gather_params   theta -> per-experiment parameter vectors
//                     (Project.get_experiment_parameters, project/base_project.py:343-363)
//   k_fill_grids      the output grid of every trajectory
//   k_assemble        fused measurement sampling + 'direct'/'sum'/custom mapping + linear scale factors + weighted
//                     residuals + log-parameter chain rule + scaled Jacobian (base_project.py:365-391,443-488;
//                     project/utils.py:10-89; loss_functions/squared_loss/squared_loss_function.py:27-80;
//                     linear_scale_factor.py:27-42)
// AssembleArgs and AssembleLds (the kernel's one description of its dynamic LDS, which the launcher sizes the block
// with) are plain C++ and compile for the host (tests/test_assemble_lds_cpu.py); the kernels need hipcc.
#ifndef SBM_ASSEMBLE_HPP
#define SBM_ASSEMBLE_HPP

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SBM_ASM_HD __host__ __device__
#else
#define SBM_ASM_HD
#endif

struct AssembleArgs {
  // static project data
  int E, q, R, G, NPR, NSP, NP, NV, NK, n_t, compat, loss;
  const int32_t *row_exp, *row_tidx, *row_var_off, *row_vars, *row_sf, *prior_idx, *sfp_group;
  const double *row_data, *row_sigma, *prior_mean, *prior_sigma, *sfp_mean, *sfp_sigma;
  const int32_t *inv_ptr, *inv_m;  // [E][q+1] CSR: model params mapped to project column c in experiment e
  const int32_t* sens_col;
  // per call
  const double* Theta;        // [V][q]
  const double* Y;            // [V*E][n_t][NV]
  const double* S;            // [V*E][n_t][NV][NK]   (nullable: residuals only)
  const int32_t* traj_status; // [V*E]
  const int32_t* traj_steps;  // [V*E]
  double* sims;               // [V][R]       (scratch or user)
  double* Rout;               // [V][R+NPR]
  double* sf;                 // [V][G]       nullable
  double* norms;              // [V]          nullable
  int32_t* status;            // [V]          nullable
  int32_t* n_steps;           // [V]          nullable: sum over the vector's trajectories
  double* J;                  // [V][R+NPR][q] nullable
  double* Jmodel;             // [V][R][q]     nullable
  double* grad;               // [V][q]        nullable
  double* sf_grad;            // [V][G][q]     nullable
  // direct mode (sbm_loss_eval): caller-supplied simulations / model Jacobian instead of Y / S
  const double* sims_in;      // [V][R]        nullable
  const double* Jm_in;        // [V][R][q]     nullable
  const int32_t* row_plain;   // [R] nullable: 1 = row keeps the plain (s - d)/sigma form under the log loss
  // custom observables: row_prog[r] = program or -1; row_w0[r] = first slot of the row's dg/dy weights in the LDS
  // table (or -1); prog_base[c] = first subprogram of program c in prog_sub_off
  int NW;                     // total weight slots (sum of the variable counts of the custom rows)
  const int32_t *row_prog, *row_w0, *prog_base, *prog_sub_off, *prog_code;
  const double *prog_const, *row_time;
};

// The dynamic LDS of k_assemble for a block of nthr threads: the byte offset of every region, in the order they lie.
// The kernel takes its pointers from it and launch_assemble the size of the block.
struct AssembleLds {
  int Gn;    // max(G, 1): the per-group regions are never empty
  int cw;    // columns handled side by side (consecutive threads -> consecutive columns)
  int rpp;   // row lanes
  size_t sim, res;            // double [R] each: simulations, weighted residuals
  size_t B, sde, sds;         // double [Gn] each: scale factors and the two sums they come from
  size_t red;                 // double [4]: one per wavefront (block_sum)
  // row tables staged once per block: every thread of pass A / B would otherwise chase them through global memory for
  // each of its elements (a chain of dependent loads per element: the kernel was bound by that latency, not by HBM)
  size_t d, sg;               // double [R] each: measurement, sigma
  size_t roff;                // int [R]: (e * n_t + tidx) * NV, the row's time point in the vector's Y block
  size_t rexp;                // int [R]: experiment
  size_t rv0, rnv;            // int [R] each: first entry of the row's variable list, its length
  size_t rvar;                // int [R]: first variable (the only one of a 'direct' mapping)
  size_t rsf;                 // int [R]: scale-factor group or -1
  size_t rw0;                 // int [R + (R & 1)]: first dg/dy weight slot of a custom row, -1 for plain rows
  size_t w;                   // double [NW]: dg/dy_k of the custom rows at this vector's sampled states
  size_t dB;                  // double [Gn][q]: dB_g / dtheta_c
  size_t part;                // double [2][Gn][rpp][q]: per-row-lane partial sums of pass A
  size_t end;

  SBM_ASM_HD AssembleLds(int R, int G, int q, int NW, int nthr) {
    Gn = G > 0 ? G : 1;
    cw = q < nthr ? q : nthr;
    rpp = nthr / cw;
    const size_t f8 = sizeof(double), i4 = sizeof(int);
    sim = 0;
    res = sim + f8 * R;
    B = res + f8 * R;
    sde = B + f8 * Gn;
    sds = sde + f8 * Gn;
    red = sds + f8 * Gn;
    d = red + f8 * 4;
    sg = d + f8 * R;
    roff = sg + f8 * R;
    rexp = roff + i4 * R;
    rv0 = rexp + i4 * R;
    rnv = rv0 + i4 * R;
    rvar = rnv + i4 * R;
    rsf = rvar + i4 * R;
    rw0 = rsf + i4 * R;
    w = rw0 + i4 * (R + (R & 1));   // 8-byte aligned again
    dB = w + f8 * NW;
    part = dB + f8 * Gn * q;
    // The size the launcher has always asked for counts 7 R + 2 ints of row tables where the regions above take
    // 7 R + (R & 1): kept, so that the shapes that fit a workgroup stay the same (4 or 8 bytes of slack behind `part`).
    end = part + f8 * 2 * Gn * rpp * q + i4 * (2 - (R & 1));
  }
  SBM_ASM_HD size_t bytes() const { return end; }
};

// The instantiation of k_assemble a launch takes: a pure function of the shape, so that it can be checked on the host
// (tests/test_assemble_tile_cpu.py).
//   rows   how many rows of J a thread of pass A keeps in registers between the model Jacobian and its scaling
//          (SBM_ASSEMBLE_TILE_*), or 0: the Jacobian makes the trip through global memory (pass A stores it, pass B
//          loads, scales and stores it again).  A thread's rows are r = row lane, + rpp, ...: ceil(R / rpp) of them.
//          0 for shapes beyond the largest tile and for q > nthr (several passes over the columns).
//   prog   the project has custom observables (row_w0 present): the postfix interpreter is compiled in
//   log    the logarithmic loss: log() and the plain-row table are compiled in
#define SBM_ASSEMBLE_TILE_SMALL 4
#define SBM_ASSEMBLE_TILE_LARGE 12
struct AssembleForm {
  int rows, prog, log;
};
SBM_ASM_HD inline AssembleForm assemble_form(int R, int q, int programs, int loss, int nthr) {
  AssembleForm f;
  f.prog = programs != 0;
  f.log = loss == 1;   // SBM_LOSS_LOG_SQUARE (include/sbm.h)
  f.rows = 0;
  if (R > 0 && q <= nthr) {
    const int rpp = nthr / (q > 0 ? q : 1);
    const int per_thread = (R + rpp - 1) / rpp;
    if (per_thread <= SBM_ASSEMBLE_TILE_SMALL) f.rows = SBM_ASSEMBLE_TILE_SMALL;
    else if (per_thread <= SBM_ASSEMBLE_TILE_LARGE) f.rows = SBM_ASSEMBLE_TILE_LARGE;
  }
  return f;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "sbm_block_reduce.hpp"
#include "sbm_observable_program.hpp"

// trajectory id = v * E + e

// theta -> P.  grid: ceil(V*E*NP / 256)
__global__ void k_gather_params(const double* __restrict__ Theta, const int32_t* __restrict__ pmap,
                                const double* __restrict__ pfixed, int V, int E, int NP, int q,
                                double* __restrict__ P) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)V * E * NP;
  if (idx >= total) return;
  const int m = (int)(idx % NP);
  const size_t ve = idx / NP;
  const int e = (int)(ve % E);
  const size_t v = ve / E;
  const int g = pmap[e * NP + m];
  P[idx] = (g >= 0) ? exp(Theta[v * q + g]) : pfixed[e * NP + m];
}

// per-trajectory grid descriptors (same for every vector): grid = ceil(V*E/256)
__global__ void k_fill_grids(const int32_t* __restrict__ tgrid_off, int V, int E, int32_t* __restrict__ goff,
                             int32_t* __restrict__ glen) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= V * E) return;
  const int e = idx % E;
  goff[idx] = tgrid_off[e];
  glen[idx] = tgrid_off[e + 1] - tgrid_off[e];
}

// ---------------------------------------------------------------------------------------------
// k_assemble: one block (256 threads) per parameter vector.  What follows are its steps, in the order the kernel
// calls them; each takes the arguments, the carved LDS block and the block's vector by reference.
// ---------------------------------------------------------------------------------------------
struct AssembleBlock {
  int v;                      // the block's parameter vector
  int Gn, cw, rpp;            // AssembleLds
  double *sim, *res, *B, *sde, *sds, *red, *d, *sg;
  int *roff, *rexp, *rv0, *rnv, *rvar, *rsf, *rw0;
  double *w, *dB, *part;
  int* bad;                   // static LDS: worst status seen by any thread
};

__device__ __forceinline__ void assemble_carve(AssembleBlock& s, const AssembleLds& l, char* smem, int* bad, int v) {
  s.v = v; s.Gn = l.Gn; s.cw = l.cw; s.rpp = l.rpp;
  s.sim = (double*)(smem + l.sim); s.res = (double*)(smem + l.res);
  s.B = (double*)(smem + l.B); s.sde = (double*)(smem + l.sde); s.sds = (double*)(smem + l.sds);
  s.red = (double*)(smem + l.red); s.d = (double*)(smem + l.d); s.sg = (double*)(smem + l.sg);
  s.roff = (int*)(smem + l.roff); s.rexp = (int*)(smem + l.rexp); s.rv0 = (int*)(smem + l.rv0);
  s.rnv = (int*)(smem + l.rnv); s.rvar = (int*)(smem + l.rvar); s.rsf = (int*)(smem + l.rsf);
  s.rw0 = (int*)(smem + l.rw0);
  s.w = (double*)(smem + l.w); s.dB = (double*)(smem + l.dB); s.part = (double*)(smem + l.part);
  s.bad = bad;
}

// The steps are templates over what the instantiation compiles in (AssembleForm): LOG the logarithmic loss (the
// launcher takes LOG == (a.loss == SBM_LOSS_LOG_SQUARE)), PROG the postfix interpreter of custom observables.
static_assert(SBM_LOSS_LOG_SQUARE == 1, "assemble_form() spells the logarithmic loss as 1");

// does row r take the logarithmic form of the residual?
template <bool LOG>
__device__ __forceinline__ bool assemble_log_row(const AssembleArgs& a, int r) {
  return LOG && !(a.row_plain && a.row_plain[r]);
}

__device__ __forceinline__ double* assemble_J(const AssembleArgs& a, int v) {
  return a.J ? a.J + (size_t)v * (a.R + a.NPR + a.NSP) * a.q : nullptr;
}

// the row tables into LDS
template <bool PROG>
__device__ __forceinline__ void assemble_stage_rows(const AssembleArgs& a, const AssembleBlock& s) {
  const int tid = threadIdx.x;
  if (tid == 0) *s.bad = 0;
  for (int r = tid; r < a.R; r += blockDim.x) {
    s.d[r] = a.row_data[r];
    s.sg[r] = a.row_sigma[r];
    s.rsf[r] = a.row_sf[r];
    s.rw0[r] = (PROG && a.row_w0 && !a.sims_in) ? a.row_w0[r] : -1;
    if (!a.sims_in) {
      const int e = a.row_exp[r], v0 = a.row_var_off[r];
      s.rexp[r] = e;
      s.roff[r] = (e * a.n_t + a.row_tidx[r]) * a.NV;
      s.rv0[r] = v0;
      s.rnv[r] = a.row_var_off[r + 1] - v0;
      s.rvar[r] = a.row_var_off[r + 1] > v0 ? a.row_vars[v0] : 0;
    } else {
      s.rexp[r] = 0; s.roff[r] = 0; s.rv0[r] = 0; s.rnv[r] = 0; s.rvar[r] = 0;
    }
  }
}

// status of the vector = worst status of its trajectories; its step count = their sum
__device__ __forceinline__ void assemble_status_and_steps(const AssembleArgs& a, const AssembleBlock& s) {
  const int tid = threadIdx.x, v = s.v, E = a.E;
  int st = 0, steps = 0;
  for (int e = tid; a.traj_status && e < E; e += blockDim.x) {
    st = max(st, a.traj_status[(size_t)v * E + e]);
    steps += a.traj_steps ? a.traj_steps[(size_t)v * E + e] : 0;
  }
  if (st != 0) atomicMax(s.bad, st);
  if (a.n_steps) {
    const double tot = block_sum((double)steps, s.red);
    if (tid == 0) a.n_steps[v] = (int32_t)tot;
  }
}

// sample + map: sims[r] = sum_{var in vars(r)} Y[traj][tidx][var], or the row's custom observable
template <bool PROG, bool LOG>
__device__ __forceinline__ void assemble_sample(const AssembleArgs& a, const AssembleBlock& s) {
  const int tid = threadIdx.x, v = s.v, R = a.R, E = a.E;
  for (int r = tid; r < R; r += blockDim.x) {
    double sv = 0.0;
    if (a.sims_in) {
      sv = a.sims_in[(size_t)v * R + r];
    } else {
      const double* Yb = a.Y + (size_t)v * E * a.n_t * a.NV + s.roff[r];
      if (PROG && s.rw0[r] >= 0) {
        // custom observable: value g(y), and dg/dy_k parked in LDS for the Jacobian pass
        const int32_t* sub = a.prog_sub_off + a.prog_base[a.row_prog[r]];
        const int32_t* vars = a.row_vars + s.rv0[r];
        const double tr = a.row_time[r];
        // (subprogram 0 is the value, 1 + k is dg/dy_k; one call site: the interpreter is inlined once)
        const int nsub = a.S ? 1 + s.rnv[r] : 1;
        for (int k = 0; k < nsub; ++k) {
          const double val = sbm_prog_eval(a.prog_code + sub[k], a.prog_const, Yb, vars, tr);
          if (k == 0) sv = val;
          else s.w[s.rw0[r] + k - 1] = val;
        }
      } else if (s.rnv[r] == 1) sv = Yb[s.rvar[r]];
      else for (int k = s.rv0[r]; k < s.rv0[r] + s.rnv[r]; ++k) sv += Yb[a.row_vars[k]];
    }
    s.sim[r] = sv;
    // NaN simulations -> inf rows; the log loss cannot take a non-positive simulation either
    const bool logrow = assemble_log_row<LOG>(a, r);
    if (!(sv == sv) || (logrow && !(sv > 0.0))) atomicMax(s.bad, (int)SBM_NON_FINITE);
  }
}

// a failed vector: NaN in simulations -> every residual / Jacobian entry is inf (squared_loss_function.py:28-32,46-50)
__device__ __forceinline__ void assemble_fill_failed(const AssembleArgs& a, const AssembleBlock& s) {
  const int tid = threadIdx.x, v = s.v, R = a.R, G = a.G, q = a.q;
  const int RT = R + a.NPR + a.NSP;
  const double inf = __builtin_inf();
  for (int r = tid; r < RT; r += blockDim.x) a.Rout[(size_t)v * RT + r] = inf;
  if (a.sims) for (int r = tid; r < R; r += blockDim.x) a.sims[(size_t)v * R + r] = s.sim[r];
  if (a.sf) for (int g = tid; g < G; g += blockDim.x) a.sf[(size_t)v * G + g] = __builtin_nan("");
  if (a.norms && tid == 0) a.norms[v] = inf;
  if (a.J) for (size_t i = tid; i < (size_t)RT * q; i += blockDim.x) a.J[(size_t)v * RT * q + i] = inf;
  if (a.Jmodel) for (size_t i = tid; i < (size_t)R * q; i += blockDim.x) a.Jmodel[(size_t)v * R * q + i] = inf;
  if (a.grad) for (int c = tid; c < q; c += blockDim.x) a.grad[(size_t)v * q + c] = inf;
  if (a.sf_grad) for (int i = tid; i < G * q; i += blockDim.x) a.sf_grad[(size_t)v * G * q + i] = __builtin_nan("");
}

// scale factors B_g = sum(s d / sigma^2) / sum(s^2 / sigma^2).  The 2 G sums are reduced side by side: every
// wavefront parks its 2 G butterfly results in LDS, one barrier, and the thread of group g adds the wavefront partials
// of its two sums in wavefront order from +0.0 -- the additions of block_sum, without its two barriers per sum.
// The partials lie in `part` ([2 G][wavefronts], at most 8 Gn doubles of its 2 Gn rpp q >= 256 Gn), which is zeroed
// only afterwards.  The caller's barrier publishes B, sde and sds.
template <bool LOG>
__device__ __forceinline__ void assemble_scale_factors(const AssembleArgs& a, const AssembleBlock& s) {
  const int tid = threadIdx.x, v = s.v, R = a.R, G = a.G;
  const int wf = tid >> 6, nwf = blockDim.x >> 6;
  double* wpart = s.part;
  for (int g = 0; g < G; ++g) {
    double sde = 0.0, sds = 0.0;
    for (int r = tid; r < R; r += blockDim.x) {
      if (s.rsf[r] == g) {
        if (LOG) {
          // log_scale_factor.py:17-28: weights 1/(sigma/d)^2; log B = sum(w (log d - log s)) / sum(w)
          const double w = (s.d[r] * s.d[r]) / (s.sg[r] * s.sg[r]);
          sde += (log(s.d[r]) - log(s.sim[r])) * w;
          sds += w;
        } else {
          const double w = 1.0 / (s.sg[r] * s.sg[r]);
          sde += s.sim[r] * s.d[r] * w;
          sds += s.sim[r] * s.sim[r] * w;
        }
      }
    }
    sde = wave_sum(sde);
    sds = wave_sum(sds);
    if ((tid & 63) == 0) {
      wpart[(2 * g + 0) * nwf + wf] = sde;
      wpart[(2 * g + 1) * nwf + wf] = sds;
    }
  }
  __syncthreads();
  for (int g = tid; g < G; g += blockDim.x) {
    double sde = 0.0, sds = 0.0;
    for (int i = 0; i < nwf; ++i) sde += wpart[(2 * g + 0) * nwf + i];
    for (int i = 0; i < nwf; ++i) sds += wpart[(2 * g + 1) * nwf + i];
    s.sde[g] = sde;
    s.sds[g] = sds;
    const double B = LOG ? exp(sde / sds) : sde / sds;
    s.B[g] = B;
    if (a.sf) a.sf[(size_t)v * G + g] = B;
  }
}

// residuals of the measurement, prior and scale-factor-prior rows, and their sum of squares
template <bool LOG>
__device__ __forceinline__ void assemble_residuals(const AssembleArgs& a, const AssembleBlock& s) {
  const int tid = threadIdx.x, v = s.v, R = a.R, q = a.q;
  const int RT = R + a.NPR + a.NSP;
  double nrm = 0.0;
  for (int r = tid; r < RT; r += blockDim.x) {
    double res;
    if (r < R) {
      const int g = s.rsf[r];
      const double B = g >= 0 ? s.B[g] : 1.0;
      const bool logrow = assemble_log_row<LOG>(a, r);
      res = logrow ? (log(B * s.sim[r]) - log(s.d[r])) / s.sg[r]
                   : (B * s.sim[r] - s.d[r]) / s.sg[r];
      s.res[r] = res;
    } else if (r < R + a.NPR) {
      const int k = r - R;
      res = (a.Theta[(size_t)v * q + a.prior_idx[k]] - a.prior_mean[k]) / a.prior_sigma[k];
    } else {
      const int k = r - R - a.NPR;  // (log B - prior)/sigma, linear_scale_factor.py:55-61
      res = (log(s.B[a.sfp_group[k]]) - a.sfp_mean[k]) / a.sfp_sigma[k];
    }
    a.Rout[(size_t)v * RT + r] = res;
    nrm += res * res;
  }
  nrm = block_sum(nrm, s.red);
  if (a.norms && tid == 0) a.norms[v] = nrm;
}

// Partial sums of pass A, owned by ONE thread each, [which][g][row lane][c]: no atomics, and the final reduction runs
// in a fixed order, so results are bitwise reproducible run to run.
__device__ __forceinline__ void assemble_zero_partials(const AssembleArgs& a, const AssembleBlock& s) {
  const int nthr = blockDim.x;
  for (int i = threadIdx.x; i < 2 * s.Gn * s.rpp * a.q; i += nthr) s.part[i] = 0.0;
}

// the (jde, jds) a thread has run up for group g, into its own partial sums
__device__ __forceinline__ void assemble_flush_partials(const AssembleBlock& s, int q, int g, int rl, int c, double jde,
                                                        double jds) {
  s.part[((size_t)(0 * s.Gn + g) * s.rpp + rl) * q + c] += jde;
  s.part[((size_t)(1 * s.Gn + g) * s.rpp + rl) * q + c] += jds;
}

// What a thread of pass A carries down its rows of one column: the group it is summing for and the two sums
// (the products J^T (d/sigma^2), J^T (s/sigma^2) of that group over the thread's rows so far).
struct AssembleRun {
  int gcur;
  double jde, jds;
};

// row r's entry jm of the model Jacobian into the thread's running sums
template <bool LOG>
__device__ __forceinline__ void assemble_accumulate(const AssembleBlock& s, AssembleRun& run, int q, int r, int rl, int c,
                                                    double jm) {
  const int g = s.rsf[r];
  if (g != run.gcur) {  // rows of one group are mostly consecutive: flush on change
    if (run.gcur >= 0) assemble_flush_partials(s, q, run.gcur, rl, c, run.jde, run.jds);
    run.gcur = g; run.jde = 0.0; run.jds = 0.0;
  }
  if (g >= 0) {
    if (LOG) {  // log_scale_factor.py:30-36: sum J / (s (sigma/d)^2)
      run.jde += jm * (s.d[r] * s.d[r]) / (s.sg[r] * s.sg[r] * s.sim[r]);
    } else {
      const double w = 1.0 / (s.sg[r] * s.sg[r]);
      run.jde += jm * s.d[r] * w;
      run.jds += jm * s.sim[r] * w;
    }
  }
}

// The model parameters of experiment e that read project column c: inv_m[k0 .. k1), and the sensitivity column of the
// only one (the common case), -1 where that parameter has no sensitivity column, -2 where the slot has none or several
struct AssembleReaders {
  int k0, k1, sc1;
};
__device__ __forceinline__ AssembleReaders assemble_readers(const AssembleArgs& a, int e, int c) {
  AssembleReaders m;
  m.k0 = a.inv_ptr[e * (a.q + 1) + c];
  m.k1 = a.inv_ptr[e * (a.q + 1) + c + 1];
  m.sc1 = (m.k1 - m.k0 == 1) ? a.sens_col[a.inv_m[m.k0]] : -2;
  return m;
}

// sum over the column's readers and the row's variables: every row kind that is not one variable read by one parameter
template <bool PROG>
__device__ __forceinline__ double assemble_row_sum(const AssembleArgs& a, const AssembleBlock& s, const double* Sb, int r,
                                                   int w0, const AssembleReaders& m) {
  double jm = 0.0;
  for (int k = m.k0; k < m.k1; ++k) {
    const int sc = a.sens_col[a.inv_m[k]];
    if (sc < 0) continue;
    if (!PROG || w0 < 0) {
      for (int kk = s.rv0[r]; kk < s.rv0[r] + s.rnv[r]; ++kk) jm += Sb[(size_t)a.row_vars[kk] * a.NK + sc];
    } else {   // custom observable: sum_k dg/dy_k * S[var_k][sc]
      for (int kk = 0; kk < s.rnv[r]; ++kk)
        jm = fma(s.w[w0 + kk], Sb[(size_t)a.row_vars[s.rv0[r] + kk] * a.NK + sc], jm);
    }
  }
  return jm;
}

// Pass A: model Jacobian with the log-parameter chain rule (base_project.py:450-455,482-485):
//   Jm[r][c] = exp(theta_c) * sum_{model params m of experiment e reading slot c} sum_{var in vars(r)} S[var][m]
// written to J / Jmodel; accumulated per SF group: the two products J^T (d/sigma^2), J^T (s/sigma^2)
// This is the form through global memory (AssembleForm::rows == 0): J holds the model Jacobian until pass B.
template <bool PROG, bool LOG>
__device__ __forceinline__ void assemble_model_jacobian(const AssembleArgs& a, const AssembleBlock& s) {
  const int tid = threadIdx.x, v = s.v, R = a.R, q = a.q, E = a.E;
  const int cw = s.cw, rpp = s.rpp;
  double* Jv = assemble_J(a, v);
  double* Jm = a.Jmodel ? a.Jmodel + (size_t)v * R * q : nullptr;
  const double* th = a.Theta + (size_t)v * q;
  const int cl = tid % cw, rl = tid / cw;
  for (int c0 = 0; c0 < q; c0 += cw) {
    const int c = c0 + cl;
    if (c >= q || rl >= rpp) continue;
    const double dth = a.Jm_in ? 1.0 : exp(th[c]);
    int e_cur = -1;
    AssembleReaders m = {0, 0, -1};
    AssembleRun run = {-1, 0.0, 0.0};
    for (int r = rl; r < R; r += rpp) {
      double jm = 0.0;
      if (a.Jm_in) {
        jm = a.Jm_in[((size_t)v * R + r) * q + c];
      } else {
        const int e = s.rexp[r];
        if (e != e_cur) {   // rows are sorted by experiment: the column's model parameters change rarely
          e_cur = e;
          m = assemble_readers(a, e, c);
        }
        const double* Sb = a.S + ((size_t)v * E * a.n_t * a.NV + s.roff[r]) * a.NK;
        const int w0 = PROG ? s.rw0[r] : -1;
        if (m.sc1 >= 0 && s.rnv[r] == 1 && w0 < 0) {
          jm = Sb[(size_t)s.rvar[r] * a.NK + m.sc1];   // the common case: one model parameter per slot
        } else if (m.sc1 != -1) {
          jm = assemble_row_sum<PROG>(a, s, Sb, r, w0, m);
        }
        jm *= dth;
      }
      if (Jm) Jm[(size_t)r * q + c] = jm;
      if (Jv) Jv[(size_t)r * q + c] = jm;
      assemble_accumulate<LOG>(s, run, q, r, rl, c, jm);
    }
    if (run.gcur >= 0) assemble_flush_partials(s, q, run.gcur, rl, c, run.jde, run.jds);
  }
}

// Pass A with the thread's K rows of the model Jacobian kept in registers (AssembleForm::rows == K; q <= blockDim.x:
// one pass over the columns, a thread is (row lane rl, column c) and owns rows rl, rl + rpp, ... < R, at most K).
// The loads of all K rows are issued before the first is used: a row that is not there or not of the common kind
// loads the vector's first entry instead, so that no load hangs on a branch.  The sums then run over the rows in
// the order of the form above.  J is not touched; Jmodel is stored here.
template <int K, bool PROG, bool LOG>
__device__ __forceinline__ void assemble_model_jacobian_tile(const AssembleArgs& a, const AssembleBlock& s, double (&jm)[K]) {
  const int tid = threadIdx.x, v = s.v, R = a.R, q = a.q;
  const int rpp = s.rpp;
  const int c = tid % s.cw, rl = tid / s.cw;
#pragma unroll
  for (int k = 0; k < K; ++k) jm[k] = 0.0;
  if (rl >= rpp) return;
  double* Jm = a.Jmodel ? a.Jmodel + (size_t)v * R * q : nullptr;
  if (a.Jm_in) {
    const double* Jin = a.Jm_in + (size_t)v * R * q + c;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int r = rl + k * rpp;
      jm[k] = Jin[(size_t)(r < R ? r : 0) * q];
    }
  } else {
    const double dth = exp(a.Theta[(size_t)v * q + c]);
    const double* Sv = a.S + (size_t)v * a.E * a.n_t * a.NV * a.NK;
    int e_cur = -1;
    AssembleReaders m = {0, 0, -1};
    unsigned other = 0;     // bit k: row k is there and takes assemble_row_sum (or is exactly zero: sc1 == -1)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int r = rl + k * rpp;
      const double* p = Sv;
      if (r < R) {
        const int e = s.rexp[r];
        if (e != e_cur) {
          e_cur = e;
          m = assemble_readers(a, e, c);
        }
        const int w0 = PROG ? s.rw0[r] : -1;
        if (m.sc1 >= 0 && s.rnv[r] == 1 && w0 < 0) p = Sv + ((size_t)s.roff[r] + s.rvar[r]) * a.NK + m.sc1;
        else other |= 1u << k;
      }
      jm[k] = *p;
    }
    if (other) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (other >> k & 1) {
          const int r = rl + k * rpp;
          const AssembleReaders mr = assemble_readers(a, s.rexp[r], c);
          jm[k] = 0.0;
          if (mr.sc1 != -1) jm[k] = assemble_row_sum<PROG>(a, s, Sv + (size_t)s.roff[r] * a.NK, r, PROG ? s.rw0[r] : -1, mr);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) jm[k] *= dth;
  }
  AssembleRun run = {-1, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int r = rl + k * rpp;
    if (r < R) {
      if (Jm) Jm[(size_t)r * q + c] = jm[k];
      assemble_accumulate<LOG>(s, run, q, r, rl, c, jm[k]);
    }
  }
  if (run.gcur >= 0) assemble_flush_partials(s, q, run.gcur, rl, c, run.jde, run.jds);
}

// dB_g/dtheta_c = jde/sds - 2 sde jds / sds^2   (linear_scale_factor.py:33-42)
template <bool LOG>
__device__ __forceinline__ void assemble_sf_gradient(const AssembleArgs& a, const AssembleBlock& s) {
  const int v = s.v, G = a.G, q = a.q, Gn = s.Gn, rpp = s.rpp;
  const int nthr = blockDim.x;
  for (int i = threadIdx.x; i < G * q; i += nthr) {
    const int g = i / q, c = i - g * q;
    double jde = 0.0, jds = 0.0;
    for (int l = 0; l < rpp; ++l) {
      jde += s.part[((size_t)(0 * Gn + g) * rpp + l) * q + c];
      jds += s.part[((size_t)(1 * Gn + g) * rpp + l) * q + c];
    }
    const double sds = s.sds[g], sde = s.sde[g];
    // square: dB = jde/sds - 2 sde jds/sds^2 ; log: dB = B * (-1/W) sum J/(s sigma'^2)
    const double db = LOG ? -s.B[g] * jde / sds : jde / sds - 2.0 * sde * jds / (sds * sds);
    s.dB[i] = db;
    if (a.sf_grad) a.sf_grad[(size_t)v * G * q + i] = db;
  }
}

// Pass B, a measurement row: J = B*Jm + sim (x) dB ; reference_compat: not divided by sigma
template <bool LOG>
__device__ __forceinline__ double assemble_scaled_entry(const AssembleArgs& a, const AssembleBlock& s, int r, int c, double val) {
  const int g = s.rsf[r], q = a.q;
  if (assemble_log_row<LOG>(a, r)) {
    // log_squared_loss_function.py:66-98: J/s (+ (dB/dtheta)/B for rows with a scale factor)
    val = val / s.sim[r];
    if (g >= 0) val += s.dB[g * q + c] / s.B[g];
  } else if (g >= 0) {
    val = s.B[g] * val + s.sim[r] * s.dB[g * q + c];
  }
  if (!a.compat) val /= s.sg[r];
  return val;
}

// Pass B, a prior row (r >= R); reference_compat: prior rows zero
__device__ __forceinline__ double assemble_prior_entry(const AssembleArgs& a, const AssembleBlock& s, int r, int c) {
  const int R = a.R, q = a.q;
  double val;
  if (r < R + a.NPR) {
    const int k = r - R;
    val = (!a.compat && a.prior_idx[k] == c) ? 1.0 / a.prior_sigma[k] : 0.0;
  } else {
    const int k = r - R - a.NPR;  // (dB/dtheta)/B, linear_scale_factor.py:44-53
    const int g = a.sfp_group[k];
    val = s.dB[g * q + c] / s.B[g];
    if (!a.compat) val /= a.sfp_sigma[k];
  }
  return val;
}

// Pass B through global memory: every entry of the model Jacobian pass A left in J, loaded, scaled and stored again
template <bool LOG>
__device__ __forceinline__ void assemble_scale_jacobian(const AssembleArgs& a, const AssembleBlock& s) {
  const int R = a.R, q = a.q;
  const int RT = R + a.NPR + a.NSP;
  double* Jv = assemble_J(a, s.v);
  if (!Jv) return;
  for (size_t i = threadIdx.x; i < (size_t)RT * q; i += blockDim.x) {
    const int r = (int)(i / q), c = (int)(i - (size_t)r * q);
    Jv[i] = r < R ? assemble_scaled_entry<LOG>(a, s, r, c, Jv[i]) : assemble_prior_entry(a, s, r, c);
  }
}

// Pass B on the rows pass A kept: J is stored once.  The prior rows keep the flat loop.
template <int K, bool LOG>
__device__ __forceinline__ void assemble_scale_jacobian_tile(const AssembleArgs& a, const AssembleBlock& s, const double (&jm)[K]) {
  const int R = a.R, q = a.q;
  const int RT = R + a.NPR + a.NSP;
  double* Jv = assemble_J(a, s.v);
  if (!Jv) return;
  const int c = threadIdx.x % s.cw, rl = threadIdx.x / s.cw;
  if (rl < s.rpp) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int r = rl + k * s.rpp;
      if (r < R) Jv[(size_t)r * q + c] = assemble_scaled_entry<LOG>(a, s, r, c, jm[k]);
    }
  }
  for (size_t i = (size_t)R * q + threadIdx.x; i < (size_t)RT * q; i += blockDim.x) {
    const int r = (int)(i / q), c2 = (int)(i - (size_t)r * q);
    Jv[i] = assemble_prior_entry(a, s, r, c2);
  }
}

// gradient of 0.5*sum r^2: (J^T r) with the Jacobian as returned (reference :803-805)
__device__ __forceinline__ void assemble_gradient(const AssembleArgs& a, const AssembleBlock& s) {
  const int v = s.v, q = a.q;
  const int RT = a.R + a.NPR + a.NSP;
  const double* Jv = assemble_J(a, v);
  for (int c = threadIdx.x; c < q; c += blockDim.x) {
    double gsum = 0.0;
    if (Jv) {
      for (int r = 0; r < RT; ++r) {
        const double res = a.Rout[(size_t)v * RT + r];
        gsum += Jv[(size_t)r * q + c] * res;
      }
    }
    a.grad[(size_t)v * q + c] = gsum;
  }
}

// K, PROG, LOG: the AssembleForm of the launch (assemble_form; launch_assemble picks the instantiation)
template <int K, bool PROG, bool LOG>
__global__ void __launch_bounds__(256) k_assemble(AssembleArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_bad;
  AssembleBlock s;
  assemble_carve(s, AssembleLds(a.R, a.G, a.q, a.NW, blockDim.x), (char*)smem, &s_bad, blockIdx.x);
  const int v = s.v, tid = threadIdx.x, R = a.R;

  assemble_stage_rows<PROG>(a, s);
  __syncthreads();
  assemble_status_and_steps(a, s);
  assemble_sample<PROG, LOG>(a, s);
  __syncthreads();
  const int bad = s_bad;
  if (a.status && tid == 0) a.status[v] = bad;
  if (bad) {
    assemble_fill_failed(a, s);
    return;
  }
  if (a.sims) for (int r = tid; r < R; r += blockDim.x) a.sims[(size_t)v * R + r] = s.sim[r];

  assemble_scale_factors<LOG>(a, s);
  __syncthreads();
  assemble_residuals<LOG>(a, s);
  if (!a.J && !a.Jmodel && !a.grad && !a.sf_grad) return;

  assemble_zero_partials(a, s);
  __syncthreads();
  if constexpr (K > 0) {
    double jm[K];
    assemble_model_jacobian_tile<K, PROG, LOG>(a, s, jm);      // pass A
    __syncthreads();
    assemble_sf_gradient<LOG>(a, s);
    __syncthreads();
    assemble_scale_jacobian_tile<K, LOG>(a, s, jm);            // pass B
  } else {
    assemble_model_jacobian<PROG, LOG>(a, s);                  // pass A
    __syncthreads();
    assemble_sf_gradient<LOG>(a, s);
    __syncthreads();
    assemble_scale_jacobian<LOG>(a, s);                        // pass B
  }
  if (a.grad) {
    __syncthreads();
    assemble_gradient(a, s);
  }
}
#endif  // __HIPCC__

#endif  // SBM_ASSEMBLE_HPP
