// Stand-alone host driver of csrc/eelg_transverse.h (built by tests/test_transverse.py with the
// address and undefined-behaviour sanitizers).  It walks the directions and reduces over 64 "lanes"
// in the order of the kernels of csrc/eelg_transverse.hip, with the header's own arithmetic.
// Input (stdin, or the file named by argv[1]):
//   n P bwd                      graphs, directions, 1 if cotangents follow
//   n x 36                       row-major 6x6 fp32 matrices
//   P x 3                        unit directions
//   n x 7, n x P x 5 (bwd only)  cotangents on the property rows and on t_dir
// Output, per graph: the 7 properties, the P x 5 values of t_dir (an empty line with P = 0), the 6
// indices, the 4 x 3 transverse vectors and, with bwd, the 36 entries of the gradient, one line
// each; 9 significant digits (enough to restore the fp32 value).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "eelg_transverse.h"

namespace {

const int kLanes = 64;
const int kNoIndex = 0x7fffffff;

int source(int i) { return i < 4 ? i : EELG_TV_BETA; }

bool takes(int i, float v, int vi, float o, int oi) {
  return (i & 1) ? eelg_elastic_max_takes(v, vi, o, oi) : eelg_elastic_min_takes(v, vi, o, oi);
}

// first extreme of column i: per lane in direction order, then the xor butterfly on (value, index)
void extreme(const std::vector<float>& val, int P, int i, float& ext, int& idx) {
  float v[kLanes];
  int at[kLanes];
  for (int lane = 0; lane < kLanes; ++lane) {
    v[lane] = (i & 1) ? -INFINITY : INFINITY;
    at[lane] = kNoIndex;
    for (int k = lane; k < P; k += kLanes) {
      const float x = val[(size_t)k * EELG_TRANSVERSE_DIR_COLS + source(i)];
      if (takes(i, v[lane], at[lane], x, k)) { v[lane] = x; at[lane] = k; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    float ov[kLanes];
    int oa[kLanes];
    for (int lane = 0; lane < kLanes; ++lane) { ov[lane] = v[lane]; oa[lane] = at[lane]; }
    for (int lane = 0; lane < kLanes; ++lane)
      if (takes(i, v[lane], at[lane], ov[lane ^ off], oa[lane ^ off])) { v[lane] = ov[lane ^ off]; at[lane] = oa[lane ^ off]; }
  }
  ext = v[0];
  idx = at[0];
}

void forward(const float* c, const float* dirs, int P, float* props, float* t_dir, int* arg, float* n_ext, double* s) {
  double a[21];
  const int spd = eelg_elastic_invert(c, a, s);
  std::vector<float> val((size_t)P * EELG_TRANSVERSE_DIR_COLS);
  for (int k = 0; k < P; ++k) {
    eelg_tv_dir q;
    eelg_tv_direction(s, dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2], q);
    double v64[EELG_TRANSVERSE_DIR_COLS];
    eelg_tv_values(q, v64);
    for (int i = 0; i < EELG_TRANSVERSE_DIR_COLS; ++i) {
      val[(size_t)k * EELG_TRANSVERSE_DIR_COLS + i] = (float)v64[i];
      t_dir[(size_t)k * EELG_TRANSVERSE_DIR_COLS + i] = spd ? (float)v64[i] : NAN;
    }
  }
  for (int i = 0; i < 6; ++i) {
    float ext;
    int idx;
    extreme(val, P, i, ext, idx);
    const bool have = spd && idx >= 0 && idx < P;
    props[i] = have ? ext : NAN;
    arg[i] = have ? idx : -1;
    if (i < 4) {
      float n[3] = {NAN, NAN, NAN};
      if (have) {
        eelg_tv_dir q;
        eelg_tv_direction(s, dirs[3 * idx], dirs[3 * idx + 1], dirs[3 * idx + 2], q);
        eelg_tv_normal(q, i, n);
      }
      for (int j = 0; j < 3; ++j) n_ext[3 * i + j] = n[j];
    }
  }
  props[EELG_TV_SPD] = spd ? 1.f : 0.f;
}

void backward(const double* s, const float* dirs, const float* props, const int* arg, const float* g_props,
              const float* g_t_dir, int P, float* g_c) {
  for (int i = 0; i < 36; ++i) g_c[i] = 0.f;
  if (props[EELG_TV_SPD] != 1.f) return;
  static double acc[kLanes][21], prev[kLanes][21];
  double gx[6];
  for (int i = 0; i < 6; ++i) gx[i] = arg[i] >= 0 ? (double)g_props[i] : 0.0;
  for (int lane = 0; lane < kLanes; ++lane) {
    for (int i = 0; i < 21; ++i) acc[lane][i] = 0.0;
    for (int k = lane; k < P; k += kLanes) {
      double w[EELG_TRANSVERSE_DIR_COLS];
      for (int i = 0; i < EELG_TRANSVERSE_DIR_COLS; ++i)
        w[i] = g_t_dir ? (double)g_t_dir[(size_t)k * EELG_TRANSVERSE_DIR_COLS + i] : 0.0;
      for (int i = 0; i < 6; ++i)
        if (k == arg[i]) w[source(i)] += gx[i];
      eelg_tv_dir q;
      eelg_tv_direction(s, dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2], q);
      eelg_tv_direction_bwd(q, w, acc[lane]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    for (int lane = 0; lane < kLanes; ++lane)
      for (int i = 0; i < 21; ++i) prev[lane][i] = acc[lane][i];
    for (int lane = 0; lane < kLanes; ++lane)
      for (int i = 0; i < 21; ++i) acc[lane][i] = prev[lane][i] + prev[lane ^ off][i];
  }
  eelg_tv_grad_c(s, acc[0], g_c);
}

bool read_floats(FILE* f, std::vector<float>& v) {
  for (size_t i = 0; i < v.size(); ++i)
    if (fscanf(f, "%f", &v[i]) != 1) return false;
  return true;
}

void print_row(const float* v, size_t n) {
  for (size_t i = 0; i < n; ++i) printf(i ? " %.9g" : "%.9g", v[i]);
  printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  int n = 0, P = 0, bwd = 0;
  if (fscanf(f, "%d %d %d", &n, &P, &bwd) != 3 || n < 0 || P < 0) return 2;
  std::vector<float> c((size_t)n * 36), dirs((size_t)P * 3), gp, gt;
  if (!read_floats(f, c) || !read_floats(f, dirs)) return 2;
  if (bwd) {
    gp.resize((size_t)n * EELG_TRANSVERSE_COLS);
    gt.resize((size_t)n * P * EELG_TRANSVERSE_DIR_COLS);
    if (!read_floats(f, gp) || !read_floats(f, gt)) return 2;
  }
  if (f != stdin) fclose(f);
  const size_t row = (size_t)P * EELG_TRANSVERSE_DIR_COLS;
  std::vector<float> t_dir(row);
  for (int g = 0; g < n; ++g) {
    float props[EELG_TRANSVERSE_COLS], n_ext[12], g_c[36];
    int arg[6];
    double s[21];
    forward(c.data() + (size_t)g * 36, dirs.data(), P, props, t_dir.data(), arg, n_ext, s);
    print_row(props, EELG_TRANSVERSE_COLS);
    print_row(t_dir.data(), row);
    printf("%d %d %d %d %d %d\n", arg[0], arg[1], arg[2], arg[3], arg[4], arg[5]);
    print_row(n_ext, 12);
    if (bwd) {
      backward(s, dirs.data(), props, arg, gp.data() + (size_t)g * EELG_TRANSVERSE_COLS, gt.data() + (size_t)g * row, P,
               g_c);
      print_row(g_c, 36);
    }
  }
  return 0;
}
