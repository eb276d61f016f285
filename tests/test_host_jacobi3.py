"""ai_jacobi3 (`csrc/ai_dense_sym.h`): the leading eigenpair of a symmetric 3 x 3 matrix, the one routine of that header that also runs on
the device (fk_pca_axis: the principal axis of a segment's points).  Compiled here with g++ and checked against cf_jacobi; no GPU."""
import os, subprocess, textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jacobi3_leading_pair_sign_and_degenerate_inputs(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(textwrap.dedent(r'''
        #include "ai_dense_sym.h"
        #include <cstdio>
        #include <random>
        static int check(const double a6[6], double* worst) {
          double e[3];
          const double lam = ai_jacobi3(a6, e);
          const double A[3][3] = {{a6[0], a6[1], a6[2]}, {a6[1], a6[3], a6[4]}, {a6[2], a6[4], a6[5]}};
          std::vector<double> a(9), ev, q;
          double scale = 0;
          for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { a[i * 3 + j] = A[i][j]; scale = std::max(scale, fabs(A[i][j])); }
          cf_jacobi(a, 3, ev, q);
          if (fabs(lam - ev[0]) > 1e-14 * std::max(scale, 1e-300)) return 1;
          if (fabs(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] - 1.0) > 1e-14) return 2;
          for (int i = 0; i < 3; ++i) {
            const double r = A[i][0] * e[0] + A[i][1] * e[1] + A[i][2] * e[2] - lam * e[i];
            *worst = std::max(*worst, fabs(r) / std::max(scale, 1e-300));
          }
          int big = 0;
          for (int k = 1; k < 3; ++k) if (fabs(e[k]) > fabs(e[big])) big = k;
          if (!(e[big] > 0.0)) return 3;    // the sign convention
          return 0;
        }
        int main() {
          std::mt19937_64 rng(3);
          std::normal_distribution<double> N(0, 1);
          double worst = 0;
          for (int rep = 0; rep < 2000; ++rep) {
            double p[4][3], a6[6] = {0, 0, 0, 0, 0, 0};
            const int rank = 1 + rep % 4;    // covariance of 1 .. 4 random points: rank 1, 2, 3, 3
            const double s = rep % 3 == 0 ? 1e-6 : rep % 3 == 1 ? 1.0 : 1e6;
            for (int k = 0; k < rank; ++k) for (int i = 0; i < 3; ++i) p[k][i] = s * N(rng);
            for (int k = 0; k < rank; ++k) {
              a6[0] += p[k][0] * p[k][0]; a6[1] += p[k][0] * p[k][1]; a6[2] += p[k][0] * p[k][2];
              a6[3] += p[k][1] * p[k][1]; a6[4] += p[k][1] * p[k][2]; a6[5] += p[k][2] * p[k][2];
            }
            if (int rc = check(a6, &worst)) return rc;
          }
          const double diag[6] = {1, 0, 0, 3, 0, 2}, zero[6] = {0, 0, 0, 0, 0, 0}, ball[6] = {2, 0, 0, 2, 0, 2};
          double e[3];
          if (ai_jacobi3(diag, e) != 3.0 || e[1] != 1.0) return 4;
          if (ai_jacobi3(zero, e) != 0.0 || e[0] != 1.0) return 5;     // every point the same: sigma = 0, the caller keeps the hash start
          if (ai_jacobi3(ball, e) != 2.0 || e[0] != 1.0) return 6;     // equal eigenvalues: the first in the order x, y, z
          printf("%.3e\n", worst);
          return worst < 1e-14 ? 0 : 8;
        }
    '''))
    exe = tmp_path / "t"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "autoinst_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
