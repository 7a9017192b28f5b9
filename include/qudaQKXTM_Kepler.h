/*
 * qudaQKXTM_Kepler.h — the multigrid entry points of the QKXTM correlator drivers under the reference's names and signatures
 * (reference include/qudaQKXTM_Kepler.h:484-508; bodies lib/interface_quda.cpp:6018-6560, :8535-9300, :7093-8530).
 *
 * What this library runs is the SOLVE LOOP each of them opens with — sources, Dirac::prepare, even-odd GCR preconditioned by the
 * multigrid hierarchies in param->preconditioner[UP|DN], Dirac::reconstruct, normalisation.  Each finished solution is handed
 * to the sink registered with qudaAmdSetSolutionSink (quda_amd_ext.h).  With qudaAmdSetTwopOutput(1), calcMG_threepTwop_EvenOdd
 * also computes the two-point functions of every source on the device (meson and baryon contractions, momentum projection up to
 * info.Q_sq) and writes the reference's ASCII files named from filename_twop.  With qudaAmdSetThreepOutput(1) it also runs the
 * fixed-sink stage for every source with info.run3pt_src != 0: for every sink separation info.tsinkSource[its], projector
 * info.proj_list[its][ip] and part (1, 2) the sequential source, twelve solves with the twist opposite to the inserted flavour and
 * the contraction with the forward propagator (ultra-local and one-derivative operators, conserved current; links from `gauge` in the
 * QKXTM lexicographic layout with the boundary applied, or the resident precise links where it is NULL), and rank 0 writes
 * <filename_threep>_tsink<t>_proj<info.thrp_proj_type[P]>.<proton|neutron>.<up|down>.<ultra_local|noether|oneD>.SS.xx.yy.zz.tt.dat in the
 * line formats of writeThrp_ASCII.  With qudaAmdSetLoopOutput(1) calcMG_loop_wOneD_TSM_EvenOdd contracts and writes the quark loops.
 * HDF5 output, position-space correlators and the high-momenta form are not part of this library; gauge_param is accepted and ignored.
 */
#ifndef _QUDAQKXTM_KEPLER_H
#define _QUDAQKXTM_KEPLER_H

#include <quda.h>
#include <qudaQKXTM_Kepler_utils.h>

/* for every source position info.sourcePosition[0 .. Nsources-1]: 12 Gaussian-smeared point sources x (up, down):
 * sink("prop_up" | "prop_dn", index = 12 * isource + spin * 3 + colour, flavour +1 | -1, source = NULL, solution);
 * with the three-point output on, after the 24 solves of a source with run3pt_src != 0, for every (its, ip, part):
 * sink("seq_part1" | "seq_part2", index = ((isource * Ntsink + its) * Nproj[its] + ip) * 12 + column, flavour of the solve,
 * the smeared sequential source, solution), in the order its, ip, part, column.  Where Nproj differs between the sink
 * separations two (its, ip) pairs can share an index: tell them apart by the order of the calls. */
void calcMG_threepTwop_EvenOdd(void **gaugeSmeared, void **gauge, QudaGaugeParam *gauge_param, QudaInvertParam *param, quda::qudaQKXTMinfo_Kepler info,
                               char *filename_twop, char *filename_threep, quda::WHICHPARTICLE NUCLEON);

/* Nstoch Z4 noise sources (or, with the truncated solver method, TSM_NLP low-precision solves followed by TSM_NHP sources solved
 * both to the full and to the low precision):
 * sink("loop_stoch" | "loop_LP" | "loop_HP" | "loop_HP_LP", index = source number, flavour of param, source, solution) */
void calcMG_loop_wOneD_TSM_EvenOdd(void **gaugeToPlaquette, QudaInvertParam *param, QudaGaugeParam *gauge_param, quda::qudaQKXTM_loopInfo loopInfo,
                                   quda::qudaQKXTMinfo_Kepler info);

/* The same loop behind exact deflation.  The reference obtains the eigenvectors from ARPACK (not a dependency of this library):
 * arpackInfo.nEv must be 0 here, i.e. nothing is projected out and every source goes to the multigrid solver; nEv > 0 is an error. */
void calcMG_loop_wOneD_TSM_wExact(void **gaugeToPlaquette, QudaInvertParam *EVparam, QudaInvertParam *param, QudaGaugeParam *gauge_param,
                                  quda::qudaQKXTM_arpackInfo arpackInfo, quda::qudaQKXTM_loopInfo loopInfo, quda::qudaQKXTMinfo_Kepler info);

#endif /* _QUDAQKXTM_KEPLER_H */
