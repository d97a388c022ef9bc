// Stand-alone host driver of csrc/eelg_jacobi.h (built by tests/test_metrics.py with the address
// and undefined-behaviour sanitizers): reads "n" and n row-major 6x6 fp32 matrices from stdin,
// prints the six ascending eigenvalues of each, one matrix per line, with 9 significant digits
// (enough to restore the fp32 value).  argv[1]: the number of sweeps (default: the header's).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "eelg_jacobi.h"

int main(int argc, char** argv) {
  const int sweeps = argc > 1 ? atoi(argv[1]) : EELG_JACOBI_SWEEPS;
  int n = 0;
  if (scanf("%d", &n) != 1 || n < 0) return 2;
  std::vector<float> m((size_t)n * 36);
  for (size_t i = 0; i < m.size(); ++i)
    if (scanf("%f", &m[i]) != 1) return 2;
  for (int g = 0; g < n; ++g) {
    float e[6];
    eelg_jacobi6(m.data() + (size_t)g * 36, e, sweeps);
    printf("%.9g %.9g %.9g %.9g %.9g %.9g\n", e[0], e[1], e[2], e[3], e[4], e[5]);
  }
  return 0;
}
