// eigensolver.cpp — exact deflation of the quark loops: the lowest modes of A = M^dag M of the full twisted-mass / twisted-clover
// operator by a Chebyshev-accelerated thick-restart Lanczos process that lives on the device, the projector (1 - U U^+) and the
// exact part of the loops, sum_i L[v_i] / lambda_i.
//
// Reference: QKXTM_Deflation_Kepler (lib/qudaQKXTM_Deflation_Kepler.cpp: polynomialOperator :744-810, eigenSolver :815-1180 drives
// ARPACK's reverse-communication loop with a host round trip per operator application, projectVector / Loop_w_One_Der_FullOp_Exact
// in lib/qudaQKXTM_Loops_Kepler.cpp:178-281).  ARPACK is not a dependency here.  Differences, on purpose: the Krylov basis never
// leaves the device, the returned pairs are sorted by ascending eigenvalue (the first n vectors are the n lowest modes, so the
// deflation steps are nested), and there is no ARPACK log file.
//
// Lanczos on Op (= p(A) with the filter, = A without): nKv resident basis vectors; every new vector is orthogonalised against ALL
// previous ones by two passes of classical Gram-Schmidt (eigBlockDot / eigBlockAxpy, eig.hip); at nKv vectors the projected matrix
// (diagonal of the kept Ritz values, one arrow row of couplings, then tridiagonal) is diagonalised on the host (cyclic Jacobi below);
// a Ritz pair counts as converged when |beta_m s_{m,i}| <= tol |theta_i|; otherwise the basis is compressed to
// nEv + (nKv - nEv) / 2 Ritz vectors (eigRotate) plus the residual vector, and the iteration goes on.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "blas.h"
#include "eig.h"
#include "interface_internal.h"
#include "qkxtm_internal.h"
#include "quda_amd_ext.h"

namespace quda {

// ---- dense real symmetric eigenproblem on the host: cyclic Jacobi (Rutishauser's rotation formulas) ----
// a: n x n row-major (the upper triangle is read); w: ascending eigenvalues; q: n x n row-major, COLUMN i the eigenvector of w[i]
static void hostSymmetricEig(int n, const double *a_in, double *w, double *q) {
  std::vector<double> a(a_in, a_in + (size_t)n * n), b(n), z(n, 0.0), d(n), v((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < i; j++) a[(size_t)i * n + j] = a[(size_t)j * n + i];
    v[(size_t)i * n + i] = 1.0;
    b[i] = d[i] = a[(size_t)i * n + i];
  }
  for (int sweep = 0; sweep < 100; sweep++) {
    double sm = 0;
    for (int p = 0; p < n - 1; p++)
      for (int r = p + 1; r < n; r++) sm += fabs(a[(size_t)p * n + r]);
    if (sm == 0.0) break;
    for (int p = 0; p < n - 1; p++)
      for (int r = p + 1; r < n; r++) {
        double &apr = a[(size_t)p * n + r];
        const double g = 100.0 * fabs(apr);
        if (sweep > 3 && fabs(d[p]) + g == fabs(d[p]) && fabs(d[r]) + g == fabs(d[r])) { apr = 0.0; continue; }
        if (apr == 0.0) continue;
        const double h = d[r] - d[p];
        double t;
        if (fabs(h) + g == fabs(h)) t = apr / h;
        else {
          const double theta = 0.5 * h / apr;
          t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
          if (theta < 0.0) t = -t;
        }
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c), hh = t * apr;
        z[p] -= hh; z[r] += hh; d[p] -= hh; d[r] += hh;
        apr = 0.0;
        auto rot = [&](double &x, double &y) { const double gx = x, hy = y; x = gx - s * (hy + gx * tau); y = hy + s * (gx - hy * tau); };
        for (int j = 0; j < p; j++) rot(a[(size_t)j * n + p], a[(size_t)j * n + r]);
        for (int j = p + 1; j < r; j++) rot(a[(size_t)p * n + j], a[(size_t)j * n + r]);
        for (int j = r + 1; j < n; j++) rot(a[(size_t)p * n + j], a[(size_t)r * n + j]);
        for (int j = 0; j < n; j++) rot(v[(size_t)j * n + p], v[(size_t)j * n + r]);
      }
    for (int i = 0; i < n; i++) { b[i] += z[i]; d[i] = b[i]; z[i] = 0.0; }
  }
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return d[x] < d[y]; });
  for (int i = 0; i < n; i++) {
    w[i] = d[order[i]];
    for (int j = 0; j < n; j++) q[(size_t)j * n + i] = v[(size_t)j * n + order[i]];
  }
}

// ---- the deflation space ----
struct Deflation {
  QudaInvertParam param;
  QudaAmdEigParam eig;
  std::vector<ColorSpinorField *> U;   // nEv eigenvectors, ascending eigenvalue, device basis, normalisation of the solver's operator
  std::vector<double> evals, resid;
  int restarts = 0, matvecs = 0;
  double secs[4] = {0, 0, 0, 0};       // device-event seconds of the eigensolver: filter, dots, updates, rotations
  double **d_ptrs = nullptr;           // device table of the base pointers of U
  long segLen = 0, segStride = 0;
  PanelView view(int n) const { return PanelView{d_ptrs, n, segLen, segStride, 2}; }
  ~Deflation() {
    for (ColorSpinorField *f : U) delete f;
    if (d_ptrs) (void)hipFree(d_ptrs);
  }
};

// rank sum of the m complex coefficients; comm_allreduce takes at most 64 doubles at a time
static void sumOverRanks(double *c, int n) {
  for (int o = 0; o < n; o += 64) comm_allreduce(c + o, std::min(64, n - o));
}

static void uploadPointers(double **d_ptrs, const std::vector<ColorSpinorField *> &f) {
  std::vector<double *> h(f.size());
  for (size_t i = 0; i < f.size(); i++) h[i] = (double *)f[i]->V();
  HIP_CHECK(hipMemcpy(d_ptrs, h.data(), h.size() * sizeof(double *), hipMemcpyHostToDevice));
}

// Z4 noise keyed by the GLOBAL site index: a lattice split over ranks starts from the same vector
static void startVector(ColorSpinorField &v, const LatticeGeom &g) {
  const CommGrid &cg = commGrid();
  std::vector<double> h((size_t)g.V * 24);
  long G[4], o[4];
  for (int d = 0; d < 4; d++) { G[d] = (long)g.X[d] * cg.dims[d]; o[d] = (long)g.X[d] * cg.coords[d]; }
  for (long iv = 0; iv < g.V; iv++) {
    long l = iv;
    const long x = l % g.X[0] + o[0]; l /= g.X[0];
    const long y = l % g.X[1] + o[1]; l /= g.X[1];
    const long z = l % g.X[2] + o[2];
    const long t = l / g.X[2] + o[3];
    const unsigned long long site = (unsigned long long)(((t * G[2] + z) * G[1] + y) * G[0] + x);
    for (int c = 0; c < 12; c++) {
      const int r = z4Draw(0x5DEECE66DA3C91E7ull, site * 12 + c);
      h[(iv * 12 + c) * 2] = r == 0 ? 1.0 : (r == 1 ? -1.0 : 0.0);
      h[(iv * 12 + c) * 2 + 1] = r == 2 ? 1.0 : (r == 3 ? -1.0 : 0.0);
    }
  }
  lexToDevice(v, h.data(), g, false);
}

namespace {

struct Lanczos {
  const Dirac &dirac;
  const QudaAmdEigParam &ep;
  std::vector<ColorSpinorField *> V;   // nKv basis vectors + the residual vector
  ColorSpinorField *work[2];           // a Chebyshev iterate (the other one is the output) and A times the newer iterate
  double **d_ptrs;
  long segLen, segStride;
  int matvecs = 0;
  // QUDA_AMD_EIG_PANEL=0: blas::multiDot / multiCaxpy in chunks of 20 fields and the rotation as k multiCaxpy sweeps into k spare
  // fields instead of the panel kernels: what tools/eig_timing.py compares against
  bool panel = true;
  double secs[4] = {0, 0, 0, 0};
  hipEvent_t ev[2];

  PanelView view(int m) const { return PanelView{d_ptrs, m, segLen, segStride, 2}; }

  template <typename F> void timed(int phase, F f) {
    HIP_CHECK(hipEventRecord(ev[0], computeStream()));
    f();
    HIP_CHECK(hipEventRecord(ev[1], computeStream()));
    HIP_CHECK(hipEventSynchronize(ev[1]));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    secs[phase] += 1e-3 * ms;
  }

  void dots(double *c, int m, ColorSpinorField &w) {
    if (panel) { eigBlockDot(c, view(m), (const double *)w.V()); sumOverRanks(c, 2 * m); return; }
    for (int c0 = 0; c0 < m; c0 += 20) {
      const int kc = std::min(20, m - c0);
      std::vector<ColorSpinorField *> f(V.begin() + c0, V.begin() + c0 + kc);
      Complex beta[20], yr;
      double yn;
      blas::multiDot(beta, yr, yn, f, kc, w, w);
      for (int i = 0; i < kc; i++) { c[2 * (c0 + i)] = beta[i].real(); c[2 * (c0 + i) + 1] = beta[i].imag(); }
    }
  }
  void update(ColorSpinorField &w, const double *c, int m) {
    if (panel) { eigBlockAxpy((double *)w.V(), c, view(m)); return; }
    for (int c0 = 0; c0 < m; c0 += 20) {
      const int kc = std::min(20, m - c0);
      std::vector<ColorSpinorField *> f(V.begin() + c0, V.begin() + c0 + kc);
      Complex a[20];
      for (int i = 0; i < kc; i++) a[i] = -Complex(c[2 * (c0 + i)], c[2 * (c0 + i) + 1]);
      blas::multiCaxpy(a, f, kc, w);
    }
  }
  // V[:, 0..k) <- V[:, 0..m) Q
  void rotate(int m, int k, const double *Q) {
    if (panel) { eigRotate(view(m), k, Q); return; }
    std::vector<ColorSpinorField *> out(k);
    for (int c = 0; c < k; c++) {
      out[c] = new ColorSpinorField(*V[0]);
      blas::zero(*out[c]);
      for (int c0 = 0; c0 < m; c0 += 20) {
        const int kc = std::min(20, m - c0);
        std::vector<ColorSpinorField *> f(V.begin() + c0, V.begin() + c0 + kc);
        Complex a[20];
        for (int i = 0; i < kc; i++) a[i] = Complex(Q[(size_t)(c0 + i) * k + c], 0.0);
        blas::multiCaxpy(a, f, kc, *out[c]);
      }
    }
    for (int c = 0; c < k; c++) { delete V[c]; V[c] = out[c]; }
    std::vector<double *> h(V.size());
    for (size_t i = 0; i < V.size(); i++) h[i] = (double *)V[i]->V();
    HIP_CHECK(hipMemcpy(d_ptrs, h.data(), h.size() * sizeof(double *), hipMemcpyHostToDevice));
  }

  // out = Op in: the reference's polynomialOperator as a three-term recurrence on rotating field pointers, or A itself
  void op(ColorSpinorField &out, const ColorSpinorField &in) {
    if (!ep.isACC || ep.PolyDeg == 0) {
      if (ep.isACC) blas::copy(out, in); else { dirac.MdagM(out, in); matvecs++; }
      return;
    }
    const double delta = 0.5 * (ep.amax - ep.amin), theta = 0.5 * (ep.amax + ep.amin), sigma1 = -delta / theta;
    ColorSpinorField *At = work[1];
    // the results of the steps alternate between two fields; the last one lands in `out`
    ColorSpinorField *odd = (ep.PolyDeg & 1) ? &out : work[0], *even = (ep.PolyDeg & 1) ? work[0] : &out;
    auto step = [&](ColorSpinorField &res, const ColorSpinorField &tm1, const ColorSpinorField &tm2, double d3, double d2, double d1) {
      dirac.MdagM(*At, tm2);
      matvecs++;
      eigChebyUpdate((double *)res.V(), (const double *)tm1.V(), (const double *)tm2.V(), (const double *)At->V(), d3, d2, d1, segLen, segStride, 2);
    };
    step(*odd, in, in, 0.0, 1.0, sigma1 / delta);
    const ColorSpinorField *tm1 = &in, *tm2 = odd;
    double sigmaOld = sigma1;
    for (int i = 2; i <= ep.PolyDeg; i++) {
      const double sigma = 1.0 / (2.0 / sigma1 - sigmaOld);
      const double d1 = 2.0 * sigma / delta, d2 = -d1 * theta, d3 = -sigma * sigmaOld;
      // step 2 must not overwrite `in`; from step 3 on the result replaces tm1 in place
      ColorSpinorField *res = (i & 1) ? odd : even;
      step(*res, *tm1, *tm2, d3, d2, d1);
      tm1 = tm2; tm2 = res;
      sigmaOld = sigma;
    }
  }

  // w <- w - V_m (V_m^+ w), twice; returns the sum of the two coefficients on every vector
  void orthogonalise(ColorSpinorField &w, int m, std::vector<double> &c) {
    std::vector<double> c2(2 * m);
    c.assign(2 * m, 0.0);
    for (int pass = 0; pass < 2; pass++) {
      timed(1, [&] { dots(c2.data(), m, w); });
      timed(2, [&] { update(w, c2.data(), m); });
      for (int i = 0; i < 2 * m; i++) c[i] += c2[i];
    }
  }
};

}  // namespace

static Deflation *runEigensolver(QudaInvertParam *param, const QudaAmdEigParam *eig) {
  if (!gaugePrecise) errorQuda("eigensolver: Gauge field not allocated");
  if (param->dslash_type != QUDA_TWISTED_MASS_DSLASH && param->dslash_type != QUDA_TWISTED_CLOVER_DSLASH) errorQuda("eigensolver: twisted-mass / twisted-clover operators only");
  if (param->dslash_type == QUDA_TWISTED_CLOVER_DSLASH && !cloverPrecise) errorQuda("eigensolver: Clover field not allocated");
  if (param->cuda_prec != QUDA_DOUBLE_PRECISION) errorQuda("eigensolver: cuda_prec = %d, everything here is fp64", (int)param->cuda_prec);
  const int nEv = eig->nEv, nKv = eig->nKv;
  if (nEv < 1 || nKv <= nEv || nKv > kEigMaxVectors) errorQuda("eigensolver: nEv = %d, nKv = %d (0 < nEv < nKv <= %d)", nEv, nKv, kEigMaxVectors);
  if (eig->isACC && (eig->PolyDeg < 0 || !(eig->amin > 0) || !(eig->amax > eig->amin))) errorQuda("eigensolver: PolyDeg = %d, amin = %g, amax = %g", eig->PolyDeg, eig->amin, eig->amax);
  if (!(eig->tol > 0) || eig->maxRestarts < 0) errorQuda("eigensolver: tol = %g, maxRestarts = %d", eig->tol, eig->maxRestarts);

  const LatticeGeom &g = residentGeom();
  ColorSpinorParam cp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, param->twist_flavor);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  {
    // nKv + 4 full fields: the basis, the residual vector, two for the filter, the operator's own temporary
    size_t freeB = 0, totalB = 0;
    poolDeviceFlush();
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    const double one = (double)g.V * 24 * sizeof(double), need = (nKv + 4) * one;
    if (need > (double)freeB)
      errorQuda("eigensolver: nKv + 4 = %d full fp64 fields need %.3f GB of device memory, %.3f GB are free", nKv + 4, need / 1e9, (double)freeB / 1e9);
  }

  DiracParam dp;
  setDiracParam(dp, param, false);   // the full operator, in the normalisation of the operator the loop solutions invert
  Dirac *dirac = Dirac::create(dp);

  Deflation *D = new Deflation;
  D->param = *param;
  D->eig = *eig;
  Lanczos L{*dirac, D->eig};
  for (int i = 0; i <= nKv; i++) L.V.push_back(new ColorSpinorField(cp));
  for (int i = 0; i < 2; i++) L.work[i] = new ColorSpinorField(cp);
  HIP_CHECK(qaMalloc(&L.d_ptrs, (nKv + 1) * sizeof(double *)));
  uploadPointers(L.d_ptrs, L.V);
  { const char *e = getenv("QUDA_AMD_EIG_PANEL"); L.panel = e ? atoi(e) != 0 : true; }
  for (int i = 0; i < 2; i++) HIP_CHECK(hipEventCreate(&L.ev[i]));
  L.segLen = (long)L.V[0]->Stride() * 24;
  L.segStride = (long)parityDoubles(*L.V[0]);
  std::vector<ColorSpinorField *> &V = L.V;

  startVector(*V[0], g);
  blas::ax(1.0 / sqrt(blas::norm2(*V[0])), *V[0]);

  const int keep = nEv + (nKv - nEv) / 2;
  std::vector<double> T((size_t)nKv * nKv, 0.0), w(nKv), Y((size_t)nKv * nKv), c, Q;
  std::vector<int> idx(nKv);
  int first = 0, restarts = 0;
  double betaLast = 0;
  for (;;) {
    for (int j = first; j < nKv; j++) {
      L.timed(0, [&] { L.op(*V[j + 1], *V[j]); });
      L.orthogonalise(*V[j + 1], j + 1, c);
      T[(size_t)j * nKv + j] = c[2 * j];
      const double beta = sqrt(blas::norm2(*V[j + 1]));
      if (!(beta > 0) || !std::isfinite(beta)) errorQuda("eigensolver: the Lanczos process broke down at vector %d (beta = %g)", j + 1, beta);
      blas::ax(1.0 / beta, *V[j + 1]);
      if (j + 1 < nKv) T[(size_t)j * nKv + j + 1] = T[(size_t)(j + 1) * nKv + j] = beta;
      betaLast = beta;
    }
    hostSymmetricEig(nKv, T.data(), w.data(), Y.data());
    // the wanted end of the spectrum first: the largest values of the filtered operator, the smallest of A itself
    for (int i = 0; i < nKv; i++) idx[i] = D->eig.isACC ? nKv - 1 - i : i;
    int nconv = 0;
    double worst = 0;
    for (int i = 0; i < nEv; i++) {
      const double est = fabs(betaLast * Y[(size_t)(nKv - 1) * nKv + idx[i]]), rel = est / fabs(w[idx[i]]);
      if (est <= D->eig.tol * fabs(w[idx[i]])) nconv++;
      worst = std::max(worst, rel);
    }
    printfQuda("eigensolver: cycle %d, %d of %d Ritz pairs converged, largest relative residual estimate %.3e, %d applications of A\n", restarts, nconv, nEv, worst, L.matvecs);
    if (nconv == nEv || restarts == D->eig.maxRestarts) {
      if (nconv != nEv) warningQuda("eigensolver: %d of %d pairs converged after %d restarts (maxRestarts)", nconv, nEv, restarts);
      break;
    }
    // thick restart: V <- V Y[:, kept], then the residual vector; T <- diag(theta) with the arrow of couplings
    Q.assign((size_t)nKv * keep, 0.0);
    for (int j = 0; j < nKv; j++)
      for (int i = 0; i < keep; i++) Q[(size_t)j * keep + i] = Y[(size_t)j * nKv + idx[i]];
    L.timed(3, [&] { L.rotate(nKv, keep, Q.data()); });
    blas::copy(*V[keep], *V[nKv]);
    std::fill(T.begin(), T.end(), 0.0);
    for (int i = 0; i < keep; i++) {
      T[(size_t)i * nKv + i] = w[idx[i]];
      T[(size_t)i * nKv + keep] = T[(size_t)keep * nKv + i] = betaLast * Y[(size_t)(nKv - 1) * nKv + idx[i]];
    }
    first = keep;
    restarts++;
  }

  // the Ritz vectors of the wanted pairs, then (reference :1156-1178) lambda_i = Re (v_i, A v_i) and |A v_i - lambda_i v_i| with the true operator
  Q.assign((size_t)nKv * nEv, 0.0);
  for (int j = 0; j < nKv; j++)
    for (int i = 0; i < nEv; i++) Q[(size_t)j * nEv + i] = Y[(size_t)j * nKv + idx[i]];
  L.timed(3, [&] { L.rotate(nKv, nEv, Q.data()); });
  std::vector<double> lambda(nEv), res(nEv);
  ColorSpinorField &Av = *L.work[1];
  for (int i = 0; i < nEv; i++) {
    dirac->MdagM(Av, *V[i]);
    L.matvecs++;
    lambda[i] = blas::reDotProduct(*V[i], Av);
    res[i] = sqrt(blas::axpyNorm(-lambda[i], *V[i], Av));
  }
  std::vector<int> order(nEv);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lambda[a] < lambda[b]; });
  for (int i = 0; i < nEv; i++) {
    D->U.push_back(V[order[i]]);
    D->evals.push_back(lambda[order[i]]);
    D->resid.push_back(res[order[i]]);
    printfQuda("eigensolver: lambda[%d] = %.15e, |A v - lambda v| = %.3e\n", i, D->evals[i], D->resid[i]);
  }
  for (int i = nEv; i <= nKv; i++) delete V[i];
  for (int i = 0; i < 2; i++) delete L.work[i];
  (void)hipFree(L.d_ptrs);
  for (int i = 0; i < 2; i++) { (void)hipEventDestroy(L.ev[i]); }
  for (int i = 0; i < 4; i++) D->secs[i] = L.secs[i];
  printfQuda("eigensolver: %.4f s filter, %.4f s dots, %.4f s updates, %.4f s rotations (device events, %s)\n", L.secs[0], L.secs[1], L.secs[2], L.secs[3],
             L.panel ? "panel kernels" : "blas::multiDot / multiCaxpy in chunks of 20");
  delete dirac;
  poolDeviceFlush();
  HIP_CHECK(qaMalloc(&D->d_ptrs, nEv * sizeof(double *)));
  uploadPointers(D->d_ptrs, D->U);
  D->segLen = L.segLen; D->segStride = L.segStride;
  D->restarts = restarts; D->matvecs = L.matvecs;
  return D;
}

// ---- what the loop driver (qkxtm.hip) calls ----
Deflation *deflationCreate(QudaInvertParam *param, const QudaAmdEigParam *eig) { return runEigensolver(param, eig); }
void deflationDestroy(Deflation *d) { delete d; }
int deflationSize(const Deflation *d) { return (int)d->U.size(); }
const double *deflationEigenvalues(const Deflation *d) { return d->evals.data(); }
ColorSpinorField &deflationVector(Deflation *d, int i) {
  if (i < 0 || i >= (int)d->U.size()) errorQuda("deflation: vector %d of %d", i, (int)d->U.size());
  return *d->U[i];
}

// x <- (1 - U_n U_n^+) x on the device
void deflationProject(Deflation *d, int n, ColorSpinorField &x) {
  if (n < 0 || n > (int)d->U.size()) errorQuda("deflation: projection with %d of %d vectors", n, (int)d->U.size());
  if (n == 0) return;
  if (x.Precision() != QUDA_DOUBLE_PRECISION || x.SiteSubset() != QUDA_FULL_SITE_SUBSET || (long)x.Stride() * 24 != d->segLen || (long)parityDoubles(x) != d->segStride)
    errorQuda("deflation: the vector does not have the shape of the eigenvectors (full fp64 device field)");
  std::vector<double> c(2 * n);
  eigBlockDot(c.data(), d->view(n), (const double *)x.V());
  sumOverRanks(c.data(), 2 * n);
  eigBlockAxpy((double *)x.V(), c.data(), d->view(n));
}

// A += sum_{first <= i < last} L[v_i] / lambda_i
void deflationExactLoopAdd(Deflation *d, LoopAccum &A, int first, int last) {
  if (first < 0 || last > (int)d->U.size()) errorQuda("deflation: exact loop of the vectors %d .. %d of %d", first, last, (int)d->U.size());
  for (int i = first; i < last; i++) loopContractAdd(A, *d->U[i], &d->param, 1.0 / d->evals[i]);
}

}  // namespace quda

using namespace quda;

// ---- test hooks: m host vectors of V * 24 doubles as two segments with a gap, the way a full device field is walked ----
namespace {
struct HookPanel {
  double *buf = nullptr, **ptrs = nullptr;
  long n, half, gap = 64;
  int m;
  HookPanel(const void *h_V, int m_, const int X[4]) : m(m_) {
    if (!X || m < 1 || m > kEigMaxVectors) errorQuda("panel hook: m = %d (1 .. %d)", m, kEigMaxVectors);
    const long V = (long)X[0] * X[1] * X[2] * X[3];
    if (V < 2 || (V & 1)) errorQuda("panel hook: lattice of %ld sites (even, positive)", V);
    n = V * 24; half = n / 2;
    HIP_CHECK(qaMalloc(&buf, (size_t)m * (n + gap) * sizeof(double)));
    HIP_CHECK(hipMemset(buf, 0, (size_t)m * (n + gap) * sizeof(double)));
    HIP_CHECK(qaMalloc(&ptrs, m * sizeof(double *)));
    std::vector<double *> h(m);
    for (int j = 0; j < m; j++) h[j] = buf + (size_t)j * (n + gap);
    HIP_CHECK(hipMemcpy(ptrs, h.data(), m * sizeof(double *), hipMemcpyHostToDevice));
    for (int j = 0; j < m; j++) put(h[j], (const double *)h_V + (size_t)j * n);
  }
  ~HookPanel() { (void)hipFree(buf); (void)hipFree(ptrs); }
  void put(double *d, const double *h) const {
    HIP_CHECK(hipMemcpy(d, h, half * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d + half + gap, h + half, half * sizeof(double), hipMemcpyHostToDevice));
  }
  void get(double *h, const double *d) const {
    HIP_CHECK(hipMemcpy(h, d, half * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h + half, d + half + gap, half * sizeof(double), hipMemcpyDeviceToHost));
  }
  PanelView view() const { return PanelView{ptrs, m, half, half + gap, 2}; }
};
}  // namespace

extern "C" {

void qudaAmdHostSymmetricEig(int n, const double *a, double *w, double *q) {
  if (n < 1 || !a || !w || !q) errorQuda("qudaAmdHostSymmetricEig: n = %d or a NULL argument", n);
  hostSymmetricEig(n, a, w, q);
}

void *qudaAmdNewDeflation(QudaInvertParam *param, const QudaAmdEigParam *eig) {
  if (!param || !eig) errorQuda("qudaAmdNewDeflation: NULL argument");
  return runEigensolver(param, eig);
}

void qudaAmdDestroyDeflation(void *defl) { delete (Deflation *)defl; }

int qudaAmdDeflationInfo(void *defl, double *evals, double *residuals, int *restarts, int *matvecs) {
  Deflation *d = (Deflation *)defl;
  if (!d) errorQuda("qudaAmdDeflationInfo: NULL deflation object");
  const int n = (int)d->U.size();
  if (evals) memcpy(evals, d->evals.data(), n * sizeof(double));
  if (residuals) memcpy(residuals, d->resid.data(), n * sizeof(double));
  if (restarts) *restarts = d->restarts;
  if (matvecs) *matvecs = d->matvecs;
  return n;
}

void qudaAmdDeflationTimings(void *defl, double secs[4]) {
  Deflation *d = (Deflation *)defl;
  if (!d || !secs) errorQuda("qudaAmdDeflationTimings: NULL argument");
  for (int i = 0; i < 4; i++) secs[i] = d->secs[i];
}

void qudaAmdDeflationGetVector(void *defl, int i, void *h_vec) {
  Deflation *d = (Deflation *)defl;
  if (!d || !h_vec) errorQuda("qudaAmdDeflationGetVector: NULL argument");
  ColorSpinorParam cpuParam(h_vec, d->param, residentGeom().X, false);
  ColorSpinorField h(cpuParam);
  h = deflationVector(d, i);
}

void qudaAmdDeflationProject(void *defl, int n, void *h_out, const void *h_in) {
  Deflation *d = (Deflation *)defl;
  if (!d || !h_out || !h_in) errorQuda("qudaAmdDeflationProject: NULL argument");
  ColorSpinorParam cpuParam((void *)h_in, d->param, residentGeom().X, false);
  ColorSpinorField in_h(cpuParam);
  ColorSpinorParam cp = deviceSpinorParam(QUDA_DOUBLE_PRECISION, QUDA_FULL_SITE_SUBSET, d->param.twist_flavor);
  cp.create = QUDA_ZERO_FIELD_CREATE;
  ColorSpinorField x(cp);
  x = in_h;
  deflationProject(d, n, x);
  cpuParam.v = h_out;
  ColorSpinorField out_h(cpuParam);
  out_h = x;
}

void qudaAmdDeflationExactLoop(void *defl, int n, double *out, int Q_sq) {
  Deflation *d = (Deflation *)defl;
  if (!d || !out) errorQuda("qudaAmdDeflationExactLoop: NULL argument");
  LoopAccum *A = loopAccumCreate(Q_sq);
  deflationExactLoopAdd(d, *A, 0, n);
  A->get(out);
  delete A;
}

void qudaAmdRotateBasis(void *h_V, int m, int k, const double *Q, const int X[4]) {
  if (!h_V || !Q) errorQuda("qudaAmdRotateBasis: NULL argument");
  HookPanel P(h_V, m, X);
  eigRotate(P.view(), k, Q);
  for (int j = 0; j < m; j++) P.get((double *)h_V + (size_t)j * P.n, P.buf + (size_t)j * (P.n + P.gap));
}

void qudaAmdBlockDot(double *c, const void *h_V, int m, const void *h_w, const int X[4]) {
  if (!c || !h_V || !h_w) errorQuda("qudaAmdBlockDot: NULL argument");
  HookPanel P(h_V, m, X), W(h_w, 1, X);
  eigBlockDot(c, P.view(), W.buf);
}

void qudaAmdBlockAxpy(void *h_w, const double *c, const void *h_V, int m, const int X[4]) {
  if (!c || !h_V || !h_w) errorQuda("qudaAmdBlockAxpy: NULL argument");
  HookPanel P(h_V, m, X), W(h_w, 1, X);
  eigBlockAxpy(W.buf, c, P.view());
  W.get((double *)h_w, W.buf);
}

}  // extern "C"
