// Stand-alone host driver of csrc/eelg_adamw.h (built by tests/test_flat_adamw.py with the address
// and undefined-behaviour sanitizers).  Two modes, chosen by the first token on stdin:
//
// "adamw n steps amsgrad lr beta1 beta2 eps weight_decay max_norm", then p[n], then steps x g[n]:
//   runs the flat step as csrc/eelg_optim.hip does (sum of squares -> norm -> clip coefficient ->
//   per-element update -> zeroed gradient; a norm that is not finite skips the step) and prints,
//   per step, the line "state <steps taken> <skipped> <norm> <coef>" and the four lines p, m, v,
//   vmax.
// "loss n_graphs n grad_scale", then pred[n_graphs * n], then target[n_graphs * n]:
//   prints the line "<loss> <stiffness_loss mean>" and one line of gradients per graph, with
//   eelg_loss_grad_coef.
// Floats are printed with 9 significant digits (enough to restore the fp32 value).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "eelg_adamw.h"

static bool read_floats(std::vector<float>& v) {
  for (size_t i = 0; i < v.size(); ++i)
    if (scanf("%f", &v[i]) != 1) return false;
  return true;
}

static void print_floats(const std::vector<float>& v) {
  for (size_t i = 0; i < v.size(); ++i) printf(i ? " %.9g" : "%.9g", v[i]);
  printf("\n");
}

static int run_adamw() {
  int n = 0, steps = 0, amsgrad = 0;
  double lr, beta1, beta2, eps, wd, max_norm;
  if (scanf("%d %d %d %lf %lf %lf %lf %lf %lf", &n, &steps, &amsgrad, &lr, &beta1, &beta2, &eps, &wd,
            &max_norm) != 9 || n < 1 || steps < 0)
    return 2;
  std::vector<float> p(n), m(n, 0.f), v(n, 0.f), vmax(n, 0.f), g(n);
  if (!read_floats(p)) return 2;
  int taken = 0, skipped = 0;
  for (int s = 0; s < steps; ++s) {
    if (!read_floats(g)) return 2;
    double sq = 0.0;
    for (int i = 0; i < n; ++i) sq += (double)(g[i] * g[i]);
    const double norm64 = sqrt(sq);
    const float norm = (float)norm64;
    float coef = 0.f;
    if (eelg_finite(norm)) {
      coef = eelg_clip_coef(norm64, max_norm);
      const eelg_adamw_consts k = eelg_adamw_prepare(lr, beta1, beta2, eps, wd, amsgrad, ++taken);
      for (int i = 0; i < n; ++i) eelg_adamw_update(k, g[i] * coef, &p[i], &m[i], &v[i], &vmax[i]);
    } else {
      ++skipped;
    }
    for (int i = 0; i < n; ++i) g[i] = 0.f;
    printf("state %d %d %.9g %.9g\n", taken, skipped, norm, coef);
    print_floats(p);
    print_floats(m);
    print_floats(v);
    print_floats(vmax);
  }
  return 0;
}

static int run_loss() {
  int nb = 0, n = 0;
  float grad_scale = 1.f;
  if (scanf("%d %d %f", &nb, &n, &grad_scale) != 3 || nb < 1 || n < 1) return 2;
  std::vector<float> pred((size_t)nb * n), target((size_t)nb * n), grad(n);
  if (!read_floats(pred) || !read_floats(target)) return 2;
  float ratio = 0.f, mse = 0.f;
  std::vector<std::vector<float>> rows;
  for (int b = 0; b < nb; ++b) {
    float d2 = 0.f, t2 = 0.f;
    for (int i = 0; i < n; ++i) {
      const float t = target[(size_t)b * n + i], d = pred[(size_t)b * n + i] - t;
      d2 += d * d;
      t2 += t * t;
    }
    const float mean_d2 = d2 / (float)n, mean_t2 = t2 / (float)n;
    ratio += mean_d2 / mean_t2;
    mse += mean_d2;
    const float c = eelg_loss_grad_coef(mean_t2, n, nb, grad_scale);
    for (int i = 0; i < n; ++i) grad[i] = c * (pred[(size_t)b * n + i] - target[(size_t)b * n + i]);
    rows.push_back(grad);
  }
  printf("%.9g %.9g\n", 100.f * (ratio / (float)nb), mse / (float)nb);
  for (const auto& r : rows) print_floats(r);
  return 0;
}

int main() {
  char mode[16] = {0};
  if (scanf("%15s", mode) != 1) return 2;
  if (!strcmp(mode, "adamw")) return run_adamw();
  if (!strcmp(mode, "loss")) return run_loss();
  return 2;
}
