// geyer_window_main.cpp -- the window rule of csrc/sbm_chain_diagnostics.hpp (sbm_geyer_tau) on the host, for
// tests/test_chain_diagnostics_cpu.py.  One case per input line: K hexadecimal doubles.  Each case is copied into a heap
// array of exactly K doubles, so that a read past the last lag is a read past the allocation.  One output line per case:
// tau as a hexadecimal double, a tab, the truncated flag.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sbm_chain_diagnostics.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  FILE* fh = fopen(argv[1], "r");
  if (!fh) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::string line;
  char buf[4096];
  while (fgets(buf, sizeof(buf), fh)) {
    line = buf;
    std::vector<double> vals;
    char* p = &line[0];
    for (char* tok = strtok(p, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) vals.push_back(strtod(tok, nullptr));
    if (vals.empty()) continue;
    const int K = (int)vals.size();
    double* ac = (double*)malloc(sizeof(double) * (size_t)K);
    memcpy(ac, vals.data(), sizeof(double) * (size_t)K);
    int truncated = -1;
    const double tau = sbm_geyer_tau(ac, K, &truncated);
    free(ac);
    printf("%a\t%d\n", tau, truncated);
  }
  fclose(fh);
  return 0;
}
