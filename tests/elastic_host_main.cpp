// Stand-alone host driver of csrc/eelg_elastic.h (built by tests/test_elastic.py with the address
// and undefined-behaviour sanitizers).  It walks the directions and reduces over 64 "lanes" in the
// order of the kernels of csrc/eelg_elastic.hip, with the header's own arithmetic.
// Input (stdin, or the file named by argv[1]):
//   n P bwd                      graphs, directions, 1 if cotangents follow
//   n x 36                       row-major 6x6 fp32 matrices
//   P x 3                        unit directions
//   n x 12, n x P  (bwd only)    cotangents on the property rows and on e_dir
// Output, per graph: the 12 properties on one line, the P values of e_dir on the next (an empty
// line with P = 0) and, with bwd, the 36 entries of the gradient on a third; 9 significant digits
// (enough to restore the fp32 value).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "eelg_elastic.h"

namespace {

const int kLanes = 64;
const int kNoIndex = 0x7fffffff;

struct Extremes {
  float vmin[kLanes], vmax[kLanes];
  int imin[kLanes], imax[kLanes];
};

// per-lane first extremes of e[0 .. P), then the xor butterfly on (value, index) pairs
void extremes(const float* e, int P, Extremes& x) {
  for (int lane = 0; lane < kLanes; ++lane) {
    x.vmin[lane] = INFINITY;
    x.vmax[lane] = -INFINITY;
    x.imin[lane] = x.imax[lane] = kNoIndex;
    for (int k = lane; k < P; k += kLanes) {
      if (eelg_elastic_min_takes(x.vmin[lane], x.imin[lane], e[k], k)) { x.vmin[lane] = e[k]; x.imin[lane] = k; }
      if (eelg_elastic_max_takes(x.vmax[lane], x.imax[lane], e[k], k)) { x.vmax[lane] = e[k]; x.imax[lane] = k; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const Extremes o = x;
    for (int lane = 0; lane < kLanes; ++lane) {
      const int p = lane ^ off;
      if (eelg_elastic_min_takes(x.vmin[lane], x.imin[lane], o.vmin[p], o.imin[p])) {
        x.vmin[lane] = o.vmin[p];
        x.imin[lane] = o.imin[p];
      }
      if (eelg_elastic_max_takes(x.vmax[lane], x.imax[lane], o.vmax[p], o.imax[p])) {
        x.vmax[lane] = o.vmax[p];
        x.imax[lane] = o.imax[p];
      }
    }
  }
}

void forward(const float* c, const float* dirs, int P, float* props, float* e, float* s32) {
  double a[21], s[21], sc[9];
  const int spd = eelg_elastic_invert(c, a, s);
  eelg_elastic_scalars(a, s, spd, sc);
  std::vector<float> val((size_t)P);
  for (int k = 0; k < P; ++k) {
    val[k] = eelg_elastic_young(s, dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
    e[k] = spd ? val[k] : NAN;
  }
  Extremes x;
  extremes(val.data(), P, x);
  for (int i = 0; i < 9; ++i) props[i] = (float)sc[i];
  const bool have = spd && P > 0;
  props[EELG_EL_EMIN] = have ? x.vmin[0] : NAN;
  props[EELG_EL_EMAX] = have ? x.vmax[0] : NAN;
  props[EELG_EL_SPD] = spd ? 1.f : 0.f;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) s32[6 * i + j] = spd ? (float)s[eelg_el_tri(i, j)] : NAN;
}

void backward(const float* s32, const float* dirs, const float* e, const float* props, const float* g_props,
              const float* g_e, int P, float* g_c) {
  const int spd = props[EELG_EL_SPD] == 1.f;
  static double acc[kLanes][21], prev[kLanes][21];
  for (int lane = 0; lane < kLanes; ++lane)
    for (int i = 0; i < 21; ++i) acc[lane][i] = 0.0;
  if (spd && P > 0) {
    Extremes x;
    extremes(e, P, x);
    const double gmin = g_props[EELG_EL_EMIN], gmax = g_props[EELG_EL_EMAX];
    for (int lane = 0; lane < kLanes; ++lane)
      for (int k = lane; k < P; k += kLanes) {
        double w = g_e ? (double)g_e[k] : 0.0;
        if (k == x.imin[lane]) w += gmin;
        if (k == x.imax[lane]) w += gmax;
        const double ek = e[k];
        double m[6];
        eelg_elastic_mandel(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2], m);
        eelg_elastic_outer_acc(acc[lane], -(w * (ek * ek)), m);
      }
    for (int off = 32; off > 0; off >>= 1) {
      for (int lane = 0; lane < kLanes; ++lane)
        for (int i = 0; i < 21; ++i) prev[lane][i] = acc[lane][i];
      for (int lane = 0; lane < kLanes; ++lane)
        for (int i = 0; i < 21; ++i) acc[lane][i] = prev[lane][i] + prev[lane ^ off][i];
    }
  }
  double gs[3], gc[3];
  eelg_elastic_scalars_bwd(props, g_props, spd, gs, gc);
  eelg_elastic_grad_c(s32, acc[0], gs, gc, spd, g_c);
}

bool read_floats(FILE* f, std::vector<float>& v) {
  for (size_t i = 0; i < v.size(); ++i)
    if (fscanf(f, "%f", &v[i]) != 1) return false;
  return true;
}

void print_row(const float* v, int n) {
  for (int i = 0; i < n; ++i) printf(i ? " %.9g" : "%.9g", v[i]);
  printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  int n = 0, P = 0, bwd = 0;
  if (fscanf(f, "%d %d %d", &n, &P, &bwd) != 3 || n < 0 || P < 0) return 2;
  std::vector<float> c((size_t)n * 36), dirs((size_t)P * 3), gp, ge;
  if (!read_floats(f, c) || !read_floats(f, dirs)) return 2;
  if (bwd) {
    gp.resize((size_t)n * EELG_ELASTIC_COLS);
    ge.resize((size_t)n * P);
    if (!read_floats(f, gp) || !read_floats(f, ge)) return 2;
  }
  if (f != stdin) fclose(f);
  std::vector<float> e((size_t)P);
  for (int g = 0; g < n; ++g) {
    float props[EELG_ELASTIC_COLS], s32[36], g_c[36];
    forward(c.data() + (size_t)g * 36, dirs.data(), P, props, e.data(), s32);
    print_row(props, EELG_ELASTIC_COLS);
    print_row(e.data(), P);
    if (bwd) {
      backward(s32, dirs.data(), e.data(), props, gp.data() + (size_t)g * EELG_ELASTIC_COLS,
               ge.data() + (size_t)g * P, P, g_c);
      print_row(g_c, 36);
    }
  }
  return 0;
}
