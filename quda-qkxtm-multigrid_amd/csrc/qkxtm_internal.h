// qkxtm_internal.h — what the translation units of the QKXTM drivers (qkxtm.hip, contract.hip, loop.hip, momproj.hip) call across
// each other.  No .hip file declares another file's function itself.
#pragma once

#include <vector>

#include "interface_internal.h"
#include "qa_core.h"

namespace quda {

// doubles between the even and the odd half of a full device spinor
inline size_t parityDoubles(const ColorSpinorField &f) { return (size_t)((const char *)f.Odd().V() - (const char *)f.Even().V()) / sizeof(double); }

// ---- fields.hip ----
void *stagingBuffer(size_t bytes);   // the library's one grow-only device buffer; valid until the next call

// ---- qkxtm.hip ----
void lexToDevice(ColorSpinorField &dst, const double *h_lex, const LatticeGeom &g, bool ukqcd);
GaugeField *loadLexGauge(void **gauge_lex, const LatticeGeom &g);
void gaussianSmear(ColorSpinorField &v, const GaugeField &U, double alpha, int nsmear);

// ---- contract.hip: two-point functions ----
struct TwopProps;
bool twopOutputEnabled();
std::vector<int> twopMomenta(int Q_sq);
TwopProps *twopPropsCreate(const LatticeGeom &g);
void twopPropsDestroy(TwopProps *p);
void twopAbsorbColumn(TwopProps &props, int fl, int isc, ColorSpinorField &v, const LatticeGeom &g, const GaugeField *U, int nsmear, double alpha, bool deviceBasis, double scale);
void twopContract(TwopProps &props, const LatticeGeom &g, const int src[4], int Q_sq, double *h_mes, double *h_bar);
void twopWriteAscii(const char *fname_twop, const int src[4], int Q_sq, int T, const double *h_mes, const double *h_bar);

// ---- loop.hip: one-end-trick loops ----
struct LoopAccum;
bool loopOutputEnabled();
std::vector<int> loopMomenta(const int L[3], int Q_sq);
LoopAccum *loopAccumCreate(int Q_sq);
void loopAccumZero(LoopAccum &A);
void loopAccumDestroy(LoopAccum *A);
void loopContractAdd(LoopAccum &A, ColorSpinorField &x, QudaInvertParam *param);
void loopAccumGet(const LoopAccum &A, double *out);
void loopWriteAscii(const LoopAccum &A, const char *pref, const char *tsmTag, int nnnn);

// ---- momproj.hip: the tail both contractions share ----
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
