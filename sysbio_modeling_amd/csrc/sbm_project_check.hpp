// sbm_project_check.hpp -- what sbm_project_load and sbm_loss_eval_host verify of a descriptor before they first touch
// the device.  The kernels index with these arrays and run the custom-observable programs unchecked, so every refusal
// here is a memory-safety check.  Plain C++17 with no HIP include: tests/test_project_checks_cpu.py compiles the header
// with g++ and hands it one malformed descriptor per refusal.
#ifndef SBM_PROJECT_CHECK_HPP
#define SBM_PROJECT_CHECK_HPP

#include <vector>

#include "sbm_observable_program.hpp"

// what the check of a project descriptor works out on its way
struct sbm_project_tables {
  int n_t_max = 0;                  // longest per-experiment grid
  int n_weights = 0;                // dg/dy slots of the custom rows, all rows together
  std::vector<int32_t> prog_base;   // [n_programs + 1] first subprogram of every program in prog_sub_off
  std::vector<int32_t> row_w0;      // [max(R, 1)] first weight slot of a custom row, -1 for plain rows
};

// The descriptor of a project on a model with n_vars state variables, n_params parameters and n_sens sensitivity
// columns.  0 and the tables, or the refusal (message in msg).
inline int sbm_project_desc_check(const sbm_project_desc* d, int n_vars, int n_params, int n_sens, char* msg, size_t msg_len,
                                  sbm_project_tables* out) {
  const char* who = "sbm_project_load";
  const int E = d->n_experiments, q = d->n_project_params, R = d->n_rows, G = d->n_sf_groups,
            NPR = d->n_prior_rows, NSP = d->n_sf_prior_rows, NP = n_params;
  if (d->loss_type != SBM_LOSS_SQUARE && d->loss_type != SBM_LOSS_LOG_SQUARE)
    return sbm_refuse(msg, msg_len, "%s: unknown loss_type %d", who, d->loss_type);
  if (E <= 0 || q <= 0 || R < 0 || G < 0 || NPR < 0 || NSP < 0)
    return sbm_refuse(msg, msg_len, "%s: bad sizes E=%d q=%d R=%d G=%d", who, E, q, R, G);
  if (!d->pmap || !d->pfixed || !d->sens_col || !d->tgrid_off || !d->tgrid || (R && (!d->row_exp || !d->row_tidx ||
      !d->row_var_off || !d->row_vars || !d->row_data || !d->row_sigma || !d->row_sf)))
    return sbm_refuse(msg, msg_len, "%s: NULL array in descriptor", who);
  int n_t_max = 0;
  for (int e = 0; e < E; ++e) {
    const int len = d->tgrid_off[e + 1] - d->tgrid_off[e];
    if (len <= 0) return sbm_refuse(msg, msg_len, "%s: experiment %d has no output times", who, e);
    for (int k = d->tgrid_off[e] + 1; k < d->tgrid_off[e + 1]; ++k)
      if (!(d->tgrid[k] >= d->tgrid[k - 1])) return sbm_refuse(msg, msg_len, "%s: tgrid of experiment %d not sorted", who, e);
    if (d->tgrid[d->tgrid_off[e]] < 0.0) return sbm_refuse(msg, msg_len, "%s: negative output time", who);
    n_t_max = len > n_t_max ? len : n_t_max;
    for (int k = 0; k < NP; ++k) {
      const int g = d->pmap[e * NP + k];
      if (g >= q) return sbm_refuse(msg, msg_len, "%s: pmap[%d][%d]=%d >= q=%d", who, e, k, g, q);
    }
  }
  for (int k = 0; k < NP; ++k)
    if (d->sens_col[k] >= n_sens) return sbm_refuse(msg, msg_len, "%s: sens_col out of range", who);
  for (int r = 0; r < R; ++r) {
    const int e = d->row_exp[r];
    if (e < 0 || e >= E) return sbm_refuse(msg, msg_len, "%s: row %d experiment %d", who, r, e);
    const int len = d->tgrid_off[e + 1] - d->tgrid_off[e];
    if (d->row_tidx[r] < 0 || d->row_tidx[r] >= len) return sbm_refuse(msg, msg_len, "%s: row %d time index", who, r);
    if (d->row_var_off[r + 1] < d->row_var_off[r]) return sbm_refuse(msg, msg_len, "%s: row_var_off", who);
    for (int k = d->row_var_off[r]; k < d->row_var_off[r + 1]; ++k)
      if (d->row_vars[k] < 0 || d->row_vars[k] >= n_vars)
        return sbm_refuse(msg, msg_len, "%s: row %d maps to variable %d of %d", who, r, d->row_vars[k], n_vars);
    if (d->row_sf[r] >= G) return sbm_refuse(msg, msg_len, "%s: row %d sf group %d", who, r, d->row_sf[r]);
    if (d->row_sigma[r] == 0.0) return sbm_refuse(msg, msg_len, "%s: row %d has sigma 0", who, r);
    if (d->loss_type == SBM_LOSS_LOG_SQUARE && !(d->row_data[r] > 0.0))
      return sbm_refuse(msg, msg_len, "%s: LogSquare loss cannot handle measurements smaller or equal to zero (row %d)", who, r);
  }
  // custom observables: every program is checked here, once, so that the interpreter in the kernel can run unchecked
  const int NPG = d->n_programs;
  if (NPG < 0) return sbm_refuse(msg, msg_len, "%s: n_programs < 0", who);
  std::vector<int32_t> prog_base((size_t)NPG + 1, 0), row_w0((size_t)(R > 0 ? R : 1), -1);
  int n_weights = 0;
  if (NPG > 0) {
    if (!d->row_prog || !d->prog_nvars || !d->prog_sub_off || !d->prog_code || !d->row_time || d->n_prog_code <= 0 ||
        (d->n_prog_const > 0 && !d->prog_const))
      return sbm_refuse(msg, msg_len, "%s: NULL program table", who);
    for (int c = 0; c < NPG; ++c) {
      if (d->prog_nvars[c] < 0 || d->prog_nvars[c] > 64)
        return sbm_refuse(msg, msg_len, "%s: program %d lists %d variables", who, c, d->prog_nvars[c]);
      prog_base[c + 1] = prog_base[c] + 1 + d->prog_nvars[c];
    }
    for (int c = 0; c < NPG; ++c)
      for (int sidx = prog_base[c]; sidx < prog_base[c + 1]; ++sidx)
        if (int rc = sbm_prog_check(d->prog_code, d->n_prog_code, d->prog_sub_off[sidx], d->prog_sub_off[sidx + 1],
                                    d->prog_nvars[c], d->n_prog_const, who, c, msg, msg_len))
          return rc;
    for (int r = 0; r < R; ++r) {
      const int c = d->row_prog[r];
      if (c >= NPG) return sbm_refuse(msg, msg_len, "%s: row %d program %d of %d", who, r, c, NPG);
      if (c < 0) continue;
      if (d->row_var_off[r + 1] - d->row_var_off[r] != d->prog_nvars[c])
        return sbm_refuse(msg, msg_len, "%s: row %d lists %d variables, its program %d takes %d", who, r,
                          d->row_var_off[r + 1] - d->row_var_off[r], c, d->prog_nvars[c]);
      row_w0[r] = n_weights;
      n_weights += d->prog_nvars[c];
    }
  }
  for (int k = 0; k < NPR; ++k)
    if (d->prior_idx[k] < 0 || d->prior_idx[k] >= q) return sbm_refuse(msg, msg_len, "%s: prior index", who);
  for (int k = 0; k < NSP; ++k)
    if (d->sf_prior_group[k] < 0 || d->sf_prior_group[k] >= G) return sbm_refuse(msg, msg_len, "%s: sf prior group", who);
  out->n_t_max = n_t_max;
  out->n_weights = n_weights;
  out->prog_base.swap(prog_base);
  out->row_w0.swap(row_w0);
  return 0;
}

// The descriptor of sbm_loss_eval_host for V frames; have_Jm: the caller supplies a model Jacobian, want_J: it asks for
// J or sf_grad.  0, or the refusal (message in msg).
inline int sbm_loss_desc_check(const sbm_loss_desc* d, int V, bool have_Jm, bool want_J, const char* who, char* msg,
                               size_t msg_len) {
  const int R = d->n_rows, q = d->n_params, G = d->n_sf_groups, NSP = d->n_sf_prior_rows;
  if (V < 0 || R <= 0 || q < 0 || G < 0 || NSP < 0)
    return sbm_refuse(msg, msg_len, "%s: bad sizes V=%d R=%d q=%d G=%d", who, V, R, q, G);
  if (d->loss_type != SBM_LOSS_SQUARE && d->loss_type != SBM_LOSS_LOG_SQUARE)
    return sbm_refuse(msg, msg_len, "%s: unknown loss_type %d", who, d->loss_type);
  if (!d->row_data || !d->row_sigma || !d->row_sf) return sbm_refuse(msg, msg_len, "%s: NULL array in descriptor", who);
  if (want_J && (!have_Jm || q <= 0)) return sbm_refuse(msg, msg_len, "%s: J / sf_grad need the model Jacobian", who);
  if (NSP && (!d->sf_prior_group || !d->sf_prior_mean || !d->sf_prior_sigma))
    return sbm_refuse(msg, msg_len, "%s: NULL sf prior array", who);
  for (int r = 0; r < R; ++r) {
    if (d->row_sf[r] >= G) return sbm_refuse(msg, msg_len, "%s: row %d sf group %d", who, r, d->row_sf[r]);
    const bool plain = d->row_plain && d->row_plain[r];
    if (plain && d->row_sf[r] >= 0) return sbm_refuse(msg, msg_len, "%s: plain row %d cannot carry a scale factor", who, r);
    if (d->loss_type == SBM_LOSS_LOG_SQUARE && !plain && !(d->row_data[r] > 0.0))
      return sbm_refuse(msg, msg_len, "%s: LogSquare loss cannot handle measurements smaller or equal to zero (row %d)", who, r);
  }
  for (int k = 0; k < NSP; ++k)
    if (d->sf_prior_group[k] < 0 || d->sf_prior_group[k] >= G) return sbm_refuse(msg, msg_len, "%s: sf prior group", who);
  return 0;
}

#endif  // SBM_PROJECT_CHECK_HPP
