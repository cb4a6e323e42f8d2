// TEST INFRASTRUCTURE -- a stand-alone host program over csrc/sbm_observable_program.hpp and csrc/sbm_project_check.hpp
// (plain C++, no HIP, no GPU).  tests/test_project_checks_cpu.py compiles it with g++, once plainly and once with
// -fsanitize=address,undefined, and runs it as a child process on a file of cases:
//
//   case <name> <kind>          kind: project | loss | eval
//   int <field> <value>
//   ivec <field> <n> <v> ...    an int32 array of exactly n entries on the heap (what a sanitizer needs to see an overrun)
//   dvec <field> <n> <v> ...    a double array (values in C99 hex or decimal)
//   null <field>                the array pointer is NULL
//   end
//
// and prints one line per case: "<name>\t<rc>\t<message>" for the descriptor checks, "<name>\t0\t<value as %a>" for an
// evaluation (sbm_prog_eval of `code` on `consts`, `y`, `vars`, `t`).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "sbm_project_check.hpp"

struct Case {
  std::string name, kind;
  std::map<std::string, long> ints;
  // exactly-sized heap blocks: one past the end is a sanitizer error, not a neighbour's data
  std::map<std::string, std::unique_ptr<int32_t[]>> ivecs;
  std::map<std::string, std::unique_ptr<double[]>> dvecs;
  std::map<std::string, bool> nulls;

  int num(const char* f) const {
    auto it = ints.find(f);
    return it == ints.end() ? 0 : (int)it->second;
  }
  const int32_t* iv(const char* f) const {
    auto it = ivecs.find(f);
    return it == ivecs.end() || nulls.count(f) ? nullptr : it->second.get();
  }
  const double* dv(const char* f) const {
    auto it = dvecs.find(f);
    return it == dvecs.end() || nulls.count(f) ? nullptr : it->second.get();
  }
};

static void run(const Case& c) {
  char msg[1024] = "";
  if (c.kind == "project") {
    sbm_project_desc d;
    memset(&d, 0, sizeof(d));
    d.n_experiments = c.num("n_experiments"); d.n_project_params = c.num("n_project_params"); d.n_rows = c.num("n_rows");
    d.n_sf_groups = c.num("n_sf_groups"); d.n_prior_rows = c.num("n_prior_rows"); d.n_sf_prior_rows = c.num("n_sf_prior_rows");
    d.pmap = c.iv("pmap"); d.pfixed = c.dv("pfixed"); d.sens_col = c.iv("sens_col");
    d.tgrid_off = c.iv("tgrid_off"); d.tgrid = c.dv("tgrid");
    d.row_exp = c.iv("row_exp"); d.row_tidx = c.iv("row_tidx"); d.row_var_off = c.iv("row_var_off"); d.row_vars = c.iv("row_vars");
    d.row_data = c.dv("row_data"); d.row_sigma = c.dv("row_sigma"); d.row_sf = c.iv("row_sf");
    d.prior_idx = c.iv("prior_idx"); d.prior_mean = c.dv("prior_mean"); d.prior_sigma = c.dv("prior_sigma");
    d.sf_prior_group = c.iv("sf_prior_group"); d.sf_prior_mean = c.dv("sf_prior_mean"); d.sf_prior_sigma = c.dv("sf_prior_sigma");
    d.reference_compat = c.num("reference_compat"); d.loss_type = c.num("loss_type");
    d.n_programs = c.num("n_programs"); d.n_prog_code = c.num("n_prog_code"); d.n_prog_const = c.num("n_prog_const");
    d.row_prog = c.iv("row_prog"); d.prog_nvars = c.iv("prog_nvars"); d.prog_sub_off = c.iv("prog_sub_off");
    d.prog_code = c.iv("prog_code"); d.prog_const = c.dv("prog_const"); d.row_time = c.dv("row_time");
    sbm_project_tables t;
    const int rc = sbm_project_desc_check(&d, c.num("model_n_vars"), c.num("model_n_params"), c.num("model_n_sens"), msg,
                                          sizeof(msg), &t);
    if (rc == 0) {
      std::string s = "n_t_max=" + std::to_string(t.n_t_max) + " n_weights=" + std::to_string(t.n_weights) + " prog_base=";
      for (int32_t v : t.prog_base) s += std::to_string(v) + ",";
      s += " row_w0=";
      for (int32_t v : t.row_w0) s += std::to_string(v) + ",";
      snprintf(msg, sizeof(msg), "%s", s.c_str());
    }
    printf("%s\t%d\t%s\n", c.name.c_str(), rc, msg);
  } else if (c.kind == "loss") {
    sbm_loss_desc d;
    memset(&d, 0, sizeof(d));
    d.n_rows = c.num("n_rows"); d.n_params = c.num("n_params"); d.n_sf_groups = c.num("n_sf_groups");
    d.n_sf_prior_rows = c.num("n_sf_prior_rows"); d.loss_type = c.num("loss_type"); d.reference_compat = c.num("reference_compat");
    d.row_data = c.dv("row_data"); d.row_sigma = c.dv("row_sigma"); d.row_sf = c.iv("row_sf"); d.row_plain = c.iv("row_plain");
    d.sf_prior_group = c.iv("sf_prior_group"); d.sf_prior_mean = c.dv("sf_prior_mean"); d.sf_prior_sigma = c.dv("sf_prior_sigma");
    const int rc = sbm_loss_desc_check(&d, c.num("V"), c.num("have_Jm") != 0, c.num("want_J") != 0, "sbm_loss_eval_host", msg,
                                       sizeof(msg));
    printf("%s\t%d\t%s\n", c.name.c_str(), rc, msg);
  } else if (c.kind == "eval") {
    const double t = c.dv("t") ? c.dv("t")[0] : 0.0;
    const double r = sbm_prog_eval(c.iv("code"), c.dv("consts"), c.dv("y"), c.iv("vars"), t);
    printf("%s\t0\t%a\n", c.name.c_str(), r);
  } else {
    fprintf(stderr, "unknown kind %s\n", c.kind.c_str());
    exit(2);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  char word[64], a[128], b[128];
  Case c;
  int n_cases = 0;
  while (fscanf(f, "%63s", word) == 1) {
    const std::string w = word;
    if (w == "case") {
      if (fscanf(f, "%127s %127s", a, b) != 2) return 2;
      c = Case();
      c.name = a; c.kind = b;
    } else if (w == "int") {
      long v;
      if (fscanf(f, "%127s %ld", a, &v) != 2) return 2;
      c.ints[a] = v;
    } else if (w == "ivec" || w == "dvec") {
      long n;
      if (fscanf(f, "%127s %ld", a, &n) != 2 || n < 0) return 2;
      if (w == "ivec") {
        std::unique_ptr<int32_t[]> p(new int32_t[n]);
        for (long i = 0; i < n; ++i) { long v; if (fscanf(f, "%ld", &v) != 1) return 2; p[i] = (int32_t)v; }
        c.ivecs[a] = std::move(p);
      } else {
        std::unique_ptr<double[]> p(new double[n]);
        for (long i = 0; i < n; ++i) { if (fscanf(f, "%127s", b) != 1) return 2; p[i] = strtod(b, nullptr); }
        c.dvecs[a] = std::move(p);
      }
    } else if (w == "null") {
      if (fscanf(f, "%127s", a) != 1) return 2;
      c.nulls[a] = true;
    } else if (w == "end") {
      run(c);
      ++n_cases;
    } else {
      fprintf(stderr, "unknown word %s\n", word);
      return 2;
    }
  }
  fclose(f);
  fprintf(stderr, "%d cases\n", n_cases);
  return 0;
}
