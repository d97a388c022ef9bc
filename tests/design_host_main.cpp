// csrc/eelg_design.h on the host: the design step of one graph after another, read from standard
// input (or the file named by the first argument).  tests/test_design.py builds this with the
// address and undefined-behaviour sanitizers.
//
// input:  <graphs>, then per graph
//           <n> <e> <v0> <step_r> <step_pos> <beta> <r_min> <r_max> <move_limit> <keep_volume>
//           g_pos[3n] g_r[e] pos[3n] r[e] pos0[3n] m_pos[3n] m_r[e] partner[e] shifts[3e] send[e] recv[e]
//         (send / recv / partner local to the graph)
// output: per graph five lines: "<flag> <vol> <vol before the step>", pos, r, m_pos, m_r
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eelg_design.h"

static FILE* in = stdin;

static std::vector<float> floats(size_t n) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i)
    if (fscanf(in, "%f", &v[i]) != 1) exit(2);
  return v;
}

static std::vector<int> ints(size_t n) {
  std::vector<int> v(n);
  for (size_t i = 0; i < n; ++i)
    if (fscanf(in, "%d", &v[i]) != 1) exit(2);
  return v;
}

static void line(const std::vector<float>& v) {
  for (size_t i = 0; i < v.size(); ++i) printf(i ? " %.9g" : "%.9g", (double)v[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc > 1 && !(in = fopen(argv[1], "r"))) return 2;
  int graphs = 0;
  if (fscanf(in, "%d", &graphs) != 1) return 2;
  for (int g = 0; g < graphs; ++g) {
    int n = 0, e = 0, keep = 0;
    float v0 = 0.f;
    eelg_design_consts k;
    if (fscanf(in, "%d %d %f %f %f %f %f %f %f %d", &n, &e, &v0, &k.step_r, &k.step_pos, &k.beta, &k.r_min, &k.r_max,
               &k.move_limit, &keep) != 10 || n < 0 || e < 0)
      return 2;
    k.keep_volume = keep;
    const std::vector<float> g_pos = floats(3 * (size_t)n), g_r = floats(e);
    std::vector<float> pos = floats(3 * (size_t)n), r = floats(e);
    const std::vector<float> pos0 = floats(3 * (size_t)n);
    std::vector<float> m_pos = floats(3 * (size_t)n), m_r = floats(e);
    const std::vector<int> partner = ints(e);
    const std::vector<float> shifts = floats(3 * (size_t)e);
    const std::vector<int> send = ints(e), recv = ints(e);
    float before = NAN;
    bool inside = true;
    for (int i = 0; i < e; ++i) inside = inside && send[i] >= 0 && send[i] < n && recv[i] >= 0 && recv[i] < n;
    if (inside) before = eelg_design_graph_volume(pos.data(), r.data(), shifts.data(), send.data(), recv.data(), e);
    float vol = 0.f;
    const int flag = eelg_design_graph(g_pos.data(), g_r.data(), pos.data(), r.data(), pos0.data(), m_pos.data(),
                                       m_r.data(), partner.data(), shifts.data(), send.data(), recv.data(), n, e, v0, k,
                                       &vol);
    printf("%d %.9g %.9g\n", flag, (double)vol, (double)before);
    line(pos);
    line(r);
    line(m_pos);
    line(m_r);
  }
  if (in != stdin) fclose(in);
  return 0;
}
