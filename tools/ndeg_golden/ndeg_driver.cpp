/*
 * tools/ndeg_golden/ndeg_driver.cpp — TEST INFRASTRUCTURE, run by hand (see pack.py), never by the build or the tests.
 *
 * Calls the reference's host operators of the non-degenerate twisted-mass doublet (tm_ndeg_dslash, tm_ndeg_matpc,
 * tm_ndeg_mat) from the objects that `make -C oracle ref` leaves in oracle/_ref/, and writes inputs and outputs as raw
 * little-endian float64 files plus a manifest.  pack.py packs them into tests/golden/ndeg_*.npz.
 *
 * Seeding as oracle/ref_driver.cpp: srand(137), gauge field first, then the spinor.  Here the spinor has 2 V 24 reals
 * ("spinor2"); its first V 24 reals are the committed `spinor`, and the gauge field is the committed gauge0..3 (not written).
 *
 * Layout: a parity doublet is [flavour 1: Vh 24][flavour 2: Vh 24]; spinor2 = [even doublet][odd doublet].
 *   ndeg_dslash_<mpc>_d<dagger>_p<parity>   input: the even doublet of spinor2, output parity `parity`
 *   ndeg_matpc_<mpc>_d<dagger>              input: the doublet of the operator's parity
 *   ndeg_mat_d<dagger>                      input: spinor2, output [even doublet][odd doublet]
 *
 * usage: ndeg_driver <outdir> X Y Z T
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <quda.h>
#include <test_util.h>
#include <wilson_dslash_reference.h>

extern int V, Vh;

static std::string g_dir;
static FILE *g_manifest = nullptr;

static void dump(const std::string &name, const double *p, size_t n) {
  const std::string path = g_dir + "/" + name + ".f64";
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(double), n, f) != n) { fprintf(stderr, "write failed: %s\n", path.c_str()); exit(1); }
  fclose(f);
  fprintf(g_manifest, "%s %zu\n", name.c_str(), n);
}

static const char *mpc_name[4] = {"ee", "oo", "eeasym", "ooasym"};
static const QudaMatPCType mpc[4] = {QUDA_MATPC_EVEN_EVEN, QUDA_MATPC_ODD_ODD, QUDA_MATPC_EVEN_EVEN_ASYMMETRIC, QUDA_MATPC_ODD_ODD_ASYMMETRIC};

int main(int argc, char **argv) {
  if (argc < 6) return 1;
  g_dir = argv[1];
  QudaGaugeParam gp;
  memset(&gp, 0, sizeof(gp));
  for (int d = 0; d < 4; d++) gp.X[d] = atoi(argv[2 + d]);
  gp.anisotropy = 1.0;
  gp.type = QUDA_WILSON_LINKS;
  gp.gauge_order = QUDA_QDP_GAUGE_ORDER;
  gp.t_boundary = QUDA_ANTI_PERIODIC_T;
  gp.cpu_prec = QUDA_DOUBLE_PRECISION;
  gp.gauge_fix = QUDA_GAUGE_FIXED_NO;
  setDims(gp.X);
  setSpinorSiteSize(24);
  const QudaPrecision prec = QUDA_DOUBLE_PRECISION;
  const size_t nh = (size_t)Vh * 24, nd = 2 * nh, n2 = 2 * nd;   // one flavour of a parity, a parity doublet, the full doublet
  const double kappa = 0.12, mu = 0.3, epsilon = 0.2;

  srand(137);
  double *gauge[4];
  for (int d = 0; d < 4; d++) gauge[d] = (double *)malloc((size_t)V * 18 * sizeof(double));
  construct_gauge_field((void **)gauge, 1, prec, &gp);
  std::vector<double> spinor2(n2), in(n2), out(n2);
  for (size_t i = 0; i < n2; i++) spinor2[i] = rand() / (double)RAND_MAX;

  g_manifest = fopen((g_dir + "/manifest.txt").c_str(), "w");
  if (!g_manifest) return 1;
  fprintf(g_manifest, "# X %d %d %d %d kappa %.17g mu %.17g epsilon %.17g\n", gp.X[0], gp.X[1], gp.X[2], gp.X[3], kappa, mu, epsilon);
  for (int d = 0; d < 4; d++) dump("check_gauge" + std::to_string(d), gauge[d], (size_t)V * 18);   // compared with the committed links by pack.py, not packed
  dump("spinor2", spinor2.data(), n2);

  char nm[128];
  // the reference twists its input in place and back in the dagger-symmetric branches: a fresh copy per case
  for (int m = 0; m < 4; m++)
    for (int dg = 0; dg < 2; dg++) {
      for (int p = 0; p < 2; p++) {
        in = spinor2;
        tm_ndeg_dslash(out.data(), out.data() + nh, (void **)gauge, in.data(), in.data() + nh, kappa, mu, epsilon, p, dg, mpc[m], prec, gp);
        snprintf(nm, sizeof nm, "ndeg_dslash_%s_d%d_p%d", mpc_name[m], dg, p);
        dump(nm, out.data(), nd);
      }
      const int p0 = (m == 0 || m == 2) ? 0 : 1;
      in = spinor2;
      tm_ndeg_matpc(out.data(), out.data() + nh, (void **)gauge, in.data() + p0 * nd, in.data() + p0 * nd + nh, kappa, mu, epsilon, mpc[m], dg, prec, gp);
      snprintf(nm, sizeof nm, "ndeg_matpc_%s_d%d", mpc_name[m], dg);
      dump(nm, out.data(), nd);
    }
  for (int dg = 0; dg < 2; dg++) {
    in = spinor2;
    tm_ndeg_mat(out.data(), out.data() + nd, (void **)gauge, in.data(), in.data() + nd, kappa, mu, epsilon, dg, prec, gp);
    snprintf(nm, sizeof nm, "ndeg_mat_d%d", dg);
    dump(nm, out.data(), n2);
  }
  fclose(g_manifest);
  return 0;
}
