// loop_exact_driver.cpp — calcMG_loop_wOneD_TSM_wExact with exact deflation driven the way a QKXTM driver
// (qkxtm/CalcMG_Loops_w_oneD_TSM_wExact.cpp) drives it: one multigrid hierarchy, nEv = 12 eigenvectors of the full operator
// (nKv = 32, Chebyshev degree 20 on [0.2, 4.0], tolerance 1e-10), deflation steps {4, 12}, stochastic sources, the solution sink
// registered.  The sink appends every eigenvector ("eigvec") and every solution to <out>.sink, the eigenvalues go to <out>.evals;
// with output on the library writes <out>_loop_exact_NeV<n>_<type>.loop.<nT>_<r> and <out>_loop_stoch_NeV<n>_<type>.loop.<NNNN>.<nT>_<r>
// (or the families of the truncated solver method); tests/test_loop_exact_driver_gpu.py recomputes those files.
//
//   loop_exact_driver gauge.bin Lx Ly Lz Lt out_prefix output(0|1) tsm(0|1) bad(0 | 1: isFullOp = false | 2: deflStep = {13})
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <quda.h>
#include <quda_amd_ext.h>
#include <qudaQKXTM_Kepler.h>

static FILE *g_out = nullptr;
static void sink(void *, const char *kind, int index, int flavor, const double *h_source, const double *h_solution, size_t nreal) {
  char tag[16] = {0};
  strncpy(tag, kind, sizeof(tag) - 1);
  const int hdr[4] = {index, flavor, h_source ? 1 : 0, (int)nreal};
  fwrite(tag, 1, sizeof(tag), g_out);
  fwrite(hdr, sizeof(int), 4, g_out);
  if (h_source) fwrite(h_source, sizeof(double), nreal, g_out);
  fwrite(h_solution, sizeof(double), nreal, g_out);
}

int main(int argc, char **argv) {
  if (argc < 10) { fprintf(stderr, "usage: %s gauge.bin Lx Ly Lz Lt out_prefix output(0|1) tsm(0|1) bad(0|1|2)\n", argv[0]); return 2; }
  const std::string prefix = argv[6];
  const int output = atoi(argv[7]), tsm = atoi(argv[8]), bad = atoi(argv[9]), massnorm = 0;
  const int X[4] = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])};
  const size_t V = (size_t)X[0] * X[1] * X[2] * X[3];
  const double kappa = 0.124, mu = 0.005;
  std::vector<double> links[4];
  void *gauge[4];
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  for (int d = 0; d < 4; d++) { links[d].resize(V * 18); if (fread(links[d].data(), sizeof(double), V * 18, f) != V * 18) return 2; gauge[d] = links[d].data(); }
  fclose(f);
  g_out = fopen((prefix + ".sink").c_str(), "wb");
  if (!g_out) return 2;

  setVerbosityQuda(QUDA_SILENT, "", stdout);
  initQuda(0);
  QudaGaugeParam gp = newQudaGaugeParam();
  for (int d = 0; d < 4; d++) gp.X[d] = X[d];
  gp.anisotropy = 1.0; gp.type = QUDA_WILSON_LINKS; gp.gauge_order = QUDA_QDP_GAUGE_ORDER; gp.t_boundary = QUDA_PERIODIC_T;
  gp.cpu_prec = QUDA_DOUBLE_PRECISION; gp.cuda_prec = QUDA_DOUBLE_PRECISION; gp.reconstruct = QUDA_RECONSTRUCT_NO;
  gp.cuda_prec_sloppy = QUDA_SINGLE_PRECISION; gp.reconstruct_sloppy = QUDA_RECONSTRUCT_NO;
  gp.cuda_prec_precondition = QUDA_SINGLE_PRECISION; gp.reconstruct_precondition = QUDA_RECONSTRUCT_NO;
  gp.gauge_fix = QUDA_GAUGE_FIXED_NO; gp.ga_pad = 0;
  loadGaugeQuda((void *)gauge, &gp);

  QudaInvertParam ip = newQudaInvertParam();
  ip.dslash_type = QUDA_TWISTED_MASS_DSLASH; ip.kappa = kappa; ip.mu = mu; ip.epsilon = 0; ip.mass = 0.5 / kappa - 4.0;
  ip.twist_flavor = QUDA_TWIST_PLUS; ip.matpc_type = QUDA_MATPC_EVEN_EVEN; ip.dagger = QUDA_DAG_NO;
  ip.solution_type = QUDA_MAT_SOLUTION; ip.solve_type = QUDA_DIRECT_PC_SOLVE; ip.mass_normalization = massnorm ? QUDA_MASS_NORMALIZATION : QUDA_KAPPA_NORMALIZATION;
  ip.cpu_prec = QUDA_DOUBLE_PRECISION; ip.cuda_prec = QUDA_DOUBLE_PRECISION; ip.cuda_prec_sloppy = QUDA_SINGLE_PRECISION;
  ip.cuda_prec_precondition = QUDA_SINGLE_PRECISION;
  ip.gamma_basis = QUDA_UKQCD_GAMMA_BASIS; ip.dirac_order = QUDA_DIRAC_ORDER;
  ip.clover_cpu_prec = QUDA_DOUBLE_PRECISION; ip.clover_cuda_prec = QUDA_DOUBLE_PRECISION; ip.clover_cuda_prec_sloppy = QUDA_SINGLE_PRECISION;
  ip.clover_cuda_prec_precondition = QUDA_SINGLE_PRECISION; ip.clover_order = QUDA_PACKED_CLOVER_ORDER;
  ip.input_location = QUDA_CPU_FIELD_LOCATION; ip.output_location = QUDA_CPU_FIELD_LOCATION;
  ip.tune = QUDA_TUNE_NO; ip.sp_pad = 0; ip.cl_pad = 0; ip.verbosity = QUDA_SILENT;
  ip.inv_type = QUDA_GCR_INVERTER; ip.tol = 1e-10; ip.maxiter = 2000; ip.reliable_delta = 1e-4; ip.gcrNkrylov = 20;
  ip.use_init_guess = QUDA_USE_INIT_GUESS_NO; ip.preserve_source = QUDA_PRESERVE_SOURCE_YES; ip.residual_type = QUDA_L2_RELATIVE_RESIDUAL;

  // the hierarchy of the flavour the loops are computed for
  void *mg[1] = {nullptr};
  QudaInvertParam mg_ip[1];
  QudaMultigridParam mp[1];
  for (int fl = 0; fl < (bad ? 0 : 1); fl++) {   // the bad-parameter runs stop before any solve
    mg_ip[fl] = ip;
    mg_ip[fl].solve_type = QUDA_DIRECT_SOLVE;
    mg_ip[fl].twist_flavor = fl == 0 ? QUDA_TWIST_PLUS : QUDA_TWIST_MINUS;
    mp[fl] = newQudaMultigridParam();
    mp[fl].invert_param = &mg_ip[fl];
    mp[fl].n_level = 2;
    for (int l = 0; l < 2; l++) {
      for (int d = 0; d < 4; d++) mp[fl].geo_block_size[l][d] = 4;
      for (int d = 4; d < QUDA_MAX_DIM; d++) mp[fl].geo_block_size[l][d] = 1;
      mp[fl].spin_block_size[l] = l == 0 ? 2 : 1;
      mp[fl].n_vec[l] = 8; mp[fl].nu_pre[l] = 2; mp[fl].nu_post[l] = 2;
      mp[fl].cycle_type[l] = QUDA_MG_CYCLE_RECURSIVE; mp[fl].smoother[l] = QUDA_MR_INVERTER; mp[fl].smoother_tol[l] = 0.25;
      mp[fl].global_reduction[l] = QUDA_BOOLEAN_YES; mp[fl].smoother_solve_type[l] = QUDA_DIRECT_PC_SOLVE;
      mp[fl].coarse_grid_solution_type[l] = QUDA_MATPC_SOLUTION; mp[fl].omega[l] = 0.85; mp[fl].location[l] = QUDA_CUDA_FIELD_LOCATION;
    }
    mp[fl].setup_maxiter = 100; mp[fl].setup_tol = 1e-4;
    mp[fl].compute_null_vector = QUDA_COMPUTE_NULL_VECTOR_YES; mp[fl].generate_all_levels = QUDA_BOOLEAN_YES; mp[fl].run_verify = QUDA_BOOLEAN_NO;
    mg[fl] = newMultigridQuda(&mp[fl]);
  }
  ip.inv_type_precondition = QUDA_MG_INVERTER;
  ip.preconditioner = mg[0]; ip.preconditionerUP = mg[0]; ip.preconditionerDN = nullptr;
  ip.tol_precondition = 1e-1; ip.maxiter_precondition = 1; ip.precondition_cycle = 1; ip.omega = 1.0;

  qudaAmdSetSolutionSink(sink, nullptr);

  static quda::qudaQKXTMinfo_Kepler info;   // ~20 KB, passed by value as in the reference
  memset(&info, 0, sizeof(info));
  for (int d = 0; d < 4; d++) info.lL[d] = X[d];
  info.Precision = QUDA_DOUBLE_PRECISION; info.isEven = true; info.kappa = kappa; info.mu = mu; info.inv_tol = ip.tol;
  info.source_type = quda::RANDOM;
  info.Q_sq = 2;

  static quda::qudaQKXTM_loopInfo loop;
  memset(&loop, 0, sizeof(loop));
  static char names[6][16] = {"Scalar", "dOp", "Loops", "LoopsCv", "LpsDw", "LpsDwCv"};
  for (int i = 0; i < 6; i++) { loop.loop_type[i] = names[i]; loop.loop_oneD[i] = i >= 2; }
  snprintf(loop.loop_fname, sizeof(loop.loop_fname), "%s_loop", prefix.c_str());
  loop.seed = 4711; loop.FileFormat = quda::ASCII_FORM; loop.HighMomForm = false; loop.Qsq = info.Q_sq; loop.Nmoms = 0;
  loop.kappa = kappa; loop.mu = mu; loop.inv_tol = ip.tol;
  if (tsm) {
    loop.useTSM = true; loop.TSM_NLP = 4; loop.TSM_NdumpLP = 2; loop.TSM_NprintLP = 2; loop.TSM_NHP = 2; loop.TSM_NdumpHP = 1; loop.TSM_NprintHP = 2;
    loop.TSM_tol = 1e-3; loop.TSM_maxiter = 0;
  } else {
    loop.useTSM = false; loop.Nstoch = 4; loop.Ndump = 2; loop.Nprint = 2;
  }
  loop.nSteps_defl = 2; loop.deflStep[0] = 4; loop.deflStep[1] = 12;
  if (bad == 2) { loop.nSteps_defl = 1; loop.deflStep[0] = 13; }

  static quda::qudaQKXTM_arpackInfo arpack;
  memset(&arpack, 0, sizeof(arpack));
  arpack.PolyDeg = 20; arpack.nEv = 12; arpack.nKv = 32; arpack.spectrumPart = quda::SR; arpack.isACC = true;
  arpack.tolArpack = 1e-10; arpack.maxIterArpack = 100; arpack.amin = 0.2; arpack.amax = 4.0;
  arpack.isEven = true; arpack.isFullOp = bad != 1;
  QudaInvertParam evp = ip;   // the reference builds its deflation operator from a second parameter set with an asymmetric matpc_type
  evp.matpc_type = QUDA_MATPC_EVEN_EVEN_ASYMMETRIC;

  qudaAmdSetLoopOutput(output);
  calcMG_loop_wOneD_TSM_wExact(gauge, &evp, &ip, &gp, arpack, loop, info);
  printf("calcMG_loop_wOneD_TSM_wExact (loop output %s, %s): %d outer iterations, %.3f s\n", output ? "on" : "off", tsm ? "TSM" : "plain", ip.iter, ip.secs);
  qudaAmdSetLoopOutput(0);
  {
    double evals[12];
    const int n = qudaAmdLastEigenvalues(evals, 12);
    FILE *fe = fopen((prefix + ".evals").c_str(), "wb");
    if (!fe || n != 12) return 3;
    fwrite(evals, sizeof(double), 12, fe);
    fclose(fe);
  }

  fclose(g_out);
  if (mg[0]) destroyMultigridQuda(mg[0]);
  freeGaugeQuda();
  endQuda();
  return 0;
}
