// qkxtm_internal.h — what the translation units of the QKXTM drivers (qkxtm.hip, contract.hip, loop.hip, threep.hip, momproj.hip) call across
// each other.  No .hip file declares another file's function itself.  The device code and the stencil argument that the contractions
// share are contract_stencil.h.
#pragma once

#include <functional>
#include <vector>

#include "interface_internal.h"
#include "qa_core.h"
#include "quda_amd_ext.h"

namespace quda {

// doubles between the even and the odd half of a full device spinor
inline size_t parityDoubles(const ColorSpinorField &f) { return (size_t)((const char *)f.Odd().V() - (const char *)f.Even().V()) / sizeof(double); }

// ---- fields.hip ----
void *stagingBuffer(size_t bytes);   // the library's one grow-only device buffer; valid until the next call

// ---- qkxtm.hip ----
void lexToDevice(ColorSpinorField &dst, const double *h_lex, const LatticeGeom &g, bool ukqcd);
void deviceLexToField(ColorSpinorField &dst, const double *d_lex, const LatticeGeom &g, bool ukqcd);   // the same from a device buffer
void deviceToLex(double *h_lex, const ColorSpinorField &src, const LatticeGeom &g, bool ukqcd, double scale);
GaugeField *loadLexGauge(void **gauge_lex, const LatticeGeom &g);
void gaussianSmear(ColorSpinorField &v, const GaugeField &U, double alpha, int nsmear);
void solveTwelveEach(QudaInvertParam *param, int flavorSign, ColorSpinorField *const sources[12], const char *fname,
                     void (*done)(void *ctx, int isc, ColorSpinorField &result, double scale), void *ctx);
// the counter-based generator of the noise vectors: draw number `counter` of the stream `key`, one of 0 .. 3 (1, -1, i, -i)
inline int z4Draw(unsigned long long key, unsigned long long counter) {
  unsigned long long z = key + counter * 0xBF58476D1CE4E5B9ull;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
  return (int)(z >> 62);
}

// ---- contract.hip: two-point functions ----
struct TwopProps;
bool twopOutputEnabled();
std::vector<int> twopMomenta(int Q_sq);
TwopProps *twopPropsCreate(const LatticeGeom &g);
void twopPropsDestroy(TwopProps *p);
double2 *twopPropsData(TwopProps &p, int fl);   // P[(mu * 4 + nu) * 9 + a * 3 + b][site] of flavour fl
void twopAbsorbColumn(TwopProps &props, int fl, int isc, ColorSpinorField &v, const LatticeGeom &g, const GaugeField *U, int nsmear, double alpha, bool deviceBasis, double scale);
void twopContract(TwopProps &props, const LatticeGeom &g, const int src[4], int Q_sq, double *h_mes, double *h_bar);
void twopWriteAscii(const char *fname_twop, const int src[4], int Q_sq, int T, const double *h_mes, const double *h_bar);

// ---- loop.hip: one-end-trick loops ----
struct MomAccum;
typedef MomAccum LoopAccum;   // [18][T_local][Nmoms][16], summed over the noise vectors
bool loopOutputEnabled();
std::vector<int> loopMomenta(const int L[3], int Q_sq);
LoopAccum *loopAccumCreate(int Q_sq);
void loopContractAdd(LoopAccum &A, ColorSpinorField &x, QudaInvertParam *param, double scale = 1.0);   // A += scale * (the 18 blocks of x)
void loopWriteAscii(const LoopAccum &A, const char *pref, const char *tsmTag, int nnnn);

// ---- eigensolver.cpp: exact deflation of the loops ----
struct Deflation;   // the lowest eigenpairs of M^dag M of the full operator, ascending, resident on the device
Deflation *deflationCreate(QudaInvertParam *param, const QudaAmdEigParam *eig);   // runs the eigensolver
void deflationDestroy(Deflation *d);
int deflationSize(const Deflation *d);
const double *deflationEigenvalues(const Deflation *d);
ColorSpinorField &deflationVector(Deflation *d, int i);
void deflationProject(Deflation *d, int n, ColorSpinorField &x);                  // x <- (1 - U_n U_n^+) x, the first n vectors
void deflationExactLoopAdd(Deflation *d, LoopAccum &A, int first, int last);      // A += sum_{first <= i < last} L[v_i] / lambda_i

// ---- threep.hip: three-point functions by the fixed-sink method ----
bool threepOutputEnabled();
int threepInsertedFlavor(int particle, int part);   // +1 up, -1 down
void threepToUkqcd(ColorSpinorField &ukqcd, const ColorSpinorField &dev, double scale);
void threepSeqSourceDevice(ColorSpinorField *const src[12], TwopProps &props, const GaugeField *Uape, const QudaAmdThreepParam *p);
void threepWriteAscii(const char *filename_out, const QudaAmdThreepParam *p, int T, const double *h_local, const double *h_noether, const double *h_oneD);
void threepSeqSource(double *h_out, const double *h_up, const double *h_dn, const GaugeField *Uape, const QudaAmdThreepParam *p);
void threepContract(double *h_local, double *h_noether, double *h_oneD, ColorSpinorField *const y[12], ColorSpinorField *const F[12], const GaugeField &U,
                    const QudaAmdThreepParam *p);

// ---- momproj.hip: the tail that the two-point, loop and three-point contractions share ----
// The momentum-space accumulator d[nblk][Lt][Nm][16] (complex, device, zero at first) of this rank's Lt time slices with its momentum
// list on the host and the device.
struct MomAccum {
  const int nblk, Lt, Nm;
  const std::vector<int> moms;   // [Nm][3]
  int *d_moms = nullptr;
  double2 *d = nullptr;
  MomAccum(int nblk, std::vector<int> moms);
  ~MomAccum();
  MomAccum(const MomAccum &) = delete;
  MomAccum &operator=(const MomAccum &) = delete;
  size_t per() const { return (size_t)Nm * 32; }   // doubles per (block, time slice)
  void zero();
  void get(double *out) const;   // gatherTimeBlocks: out[nblk][T global][Nm][16][re, im]
};
// A.d += the projection of the caller's blocks, staged chunk by chunk: stage(t0, nt, cs) launches the kernels that write
// cs[nblk][nt * Vs][16] for the local time slices [t0, t0 + nt).  A chunk holds as many slices as keep cs below 2 GiB, and at most
// maxSlicesPerChunk if that is positive.  gx as for momentumProject.  secs (may be NULL): the device-event seconds of the staging
// kernels and of the projections, summed over the chunks.  Synchronises the stream.
void stageAndProject(MomAccum &A, const int gx[3], int maxSlicesPerChunk, const std::function<void(int t0, int nt, double2 *cs)> &stage, double secs[2]);
double elapsedSecs(hipEvent_t a, hipEvent_t b);   // between two completed events
// Project the staged blocks cs[nblk][nt * Vs][16] (complex; Vs = X[0] X[1] X[2] sites per slice, x fastest) of the local time slices
// [t0, t0 + nt) onto the momenta d_moms[Nm][3] (device) and ADD the result into acc[nblk][Lt][Nm][16] (device):
//      acc[k][t0 + tl][m][e] += sum_s exp(-2 pi i sum_d n_d (x_d(s) + gx[d]) / L[d]) cs[k][tl * Vs + s][e],
// X the local spatial extents, gx the global coordinate of the local origin (of any sign: minus the source position for the two-point
// functions), L the global extents.  Part of the contract, so that results agree bit by bit whatever the launch: a slice is cut into
// NPART = 64 fixed shares [Vs p / 64, Vs (p + 1) / 64); a share is summed by NLANE = 16 site lanes (sites s0 + lane, s0 + lane + 16,
// ...), the lanes are added in order, then the 64 shares in order, then the old value of acc.  Asynchronous on the compute stream; the
// partial sums live in the staging buffer, so the caller synchronises before anything else stages through it.
void momentumProject(double2 *acc, const double2 *cs, int nblk, int t0, int nt, int Lt, const int *d_moms, int Nm, const int X[3], const int gx[3], const int L[3]);
// out[nblk][T][per] (host, T = Lt x ranks in t): this rank's d_loc[nblk][Lt][per] (device, doubles) placed at its time offset into
// zeros, ONE all-gather, the ranks added in rank order, so every rank holds the same bits.  Collective; synchronises the stream.
void gatherTimeBlocks(double *out, const double *d_loc, int nblk, int Lt, size_t per);
// the body of the extern "C" momentum queries: the number of momenta in m; copied to moms if that is not NULL and max_moms holds them
int copyMomenta(const std::vector<int> &m, int *moms, int max_moms, const char *fname);

}  // namespace quda
