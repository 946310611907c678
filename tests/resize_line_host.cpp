// Host program around csrc/resize_line.h for tests/test_resampling_cases_cpu.py: the header's arithmetic, line by line, printed as
// text.  Built with the address and undefined-behaviour sanitizers; reads a case file, writes a result file.
//   case   "S n_in n_out order v[0] .. v[n_in-1]"      -> "C ..." the prefilter coefficients (double, not rounded),
//                                                         "T o base ntaps idx.. w.." per output index, "R ..." the resized line
//          "L strict n lab[0..n) w[0..n)"              -> "V label"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "resize_line.h"

static std::vector<double> prefilter_line(const std::vector<double>& x) {
  const int n = (int)x.size();
  std::vector<double> c(x);
  if (n == 1) return c;
  std::vector<double> cp(n);
  cp[0] = mt_rs_causal_start(x[0]);
  for (int k = 1; k < n; ++k) cp[k] = 6.0 * x[k] + MT_RS_POLE * cp[k - 1];
  c[n - 1] = mt_rs_anticausal_start(cp[n - 1], x[n - 1]);
  for (int k = n - 2; k >= 0; --k) c[k] = MT_RS_POLE * (c[k + 1] - cp[k]);
  return c;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s cases.txt results.txt\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  char kind;
  while (fscanf(in, " %c", &kind) == 1) {
    if (kind == 'S') {
      int n_in, n_out, order;
      if (fscanf(in, "%d %d %d", &n_in, &n_out, &order) != 3 || n_in < 1 || n_out < 1) return 3;
      std::vector<double> x(n_in);
      for (int k = 0; k < n_in; ++k) if (fscanf(in, "%lf", &x[k]) != 1) return 3;
      const std::vector<double> c = (order == 3 && n_in != n_out) ? prefilter_line(x) : x;
      fprintf(out, "C");
      for (int k = 0; k < n_in; ++k) fprintf(out, " %.17g", c[k]);
      fprintf(out, "\n");
      std::vector<double> r(n_out);
      for (int o = 0; o < n_out; ++o) {
        int idx[4]; double w[4];
        const int nt = mt_rs_taps(order, o, n_in, n_out, idx, w);
        if (nt != mt_rs_ntaps(order, n_in, n_out)) return 4;
        fprintf(out, "T %d %d %d", o, order == 3 && n_in != n_out ? mt_rs_tap_base3(o, n_in, n_out) : 0, nt);
        double s = 0.0;
        for (int k = 0; k < nt; ++k) { fprintf(out, " %d", idx[k]); s += w[k] * c[(size_t)idx[k]]; }      // idx out of range: the sanitizer's
        for (int k = 0; k < nt; ++k) fprintf(out, " %.17g", w[k]);
        fprintf(out, "\n");
        r[o] = s;
      }
      fprintf(out, "R");
      for (int o = 0; o < n_out; ++o) fprintf(out, " %.17g", r[o]);
      fprintf(out, "\n");
      if (n_in > 1) fprintf(out, "E %.17g %.17g %.17g %.17g\n", mt_rs_extend(c[0], c[1], 1), mt_rs_extend(c[0], c[1], 2),
                            mt_rs_extend(c[n_in - 1], c[n_in - 2], 1), mt_rs_extend(c[n_in - 1], c[n_in - 2], 2));
    } else if (kind == 'L') {
      int strict, n;
      if (fscanf(in, "%d %d", &strict, &n) != 2 || n < 1 || n > 8) return 3;
      std::vector<float> lab(n); std::vector<double> w(n);
      for (int k = 0; k < n; ++k) if (fscanf(in, "%f", &lab[k]) != 1) return 3;
      for (int k = 0; k < n; ++k) if (fscanf(in, "%lf", &w[k]) != 1) return 3;
      fprintf(out, "V %.9g\n", (double)mt_rs_label_vote(lab.data(), w.data(), n, strict));
    } else return 3;
  }
  fclose(in);
  if (fclose(out) != 0) return 5;
  return 0;
}
