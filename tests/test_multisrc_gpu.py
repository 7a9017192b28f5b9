"""invertMultiSrcQuda (reference include/quda.h:647; lib/interface_quda.cpp:2546: declared, "cannot work" there): several sources through ONE
lockstep MG-GCR solve — outer GCR per source with a shared Krylov index, one multigrid cycle for all sources whose coarse levels run on block
fields through the multi-right-hand-side MFMA coarse operator (csrc/block_solver.cpp: the lockstep GCR; csrc/block_mg_cycle.cpp,
block_fine_smoother.cpp, block_coarse_cycle.cpp: its cycle).  Every column is a solution in its own right: host
residual with the oracle's tm_mat (as tests/multigrid_invert_test.cpp:529-577), agreement with the single-source invertQuda, the same
iteration count within one."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


from test_mg_gpu import _setup, _true_residual  # noqa: E402


@pytest.mark.parametrize("outer_pc", [False, True], ids=["full-system", "even-odd-outer"])
@pytest.mark.parametrize("X,levels,blocks,nvec,nsrc,mask", [((16, 8, 8, 16), 3, [(4, 4, 4, 4), (2, 2, 2, 2), (2, 2, 2, 2)], 8, 5, 0), ((16, 16, 16, 16), 3, [(4, 4, 4, 4), (2, 2, 2, 2), (2, 2, 2, 2)], 24, 12, 0),
                                                    ((16, 8, 8, 16), 2, (4, 4, 4, 4), 8, 3, 9), ((8, 8, 8, 16), 2, (4, 4, 4, 4), 8, 1, 0)],
                         ids=["5-sources-n16", "12-sources-n48", "3-sources-partitioned-xt", "a-single-source"])
def test_multi_source_mg_gcr_matches_single_source_solves(qa, oracle, X, levels, blocks, nvec, nsrc, mask, outer_pc):
    kappa, mu = 0.124, 0.005
    qa.lib().qudaAmdSetPartitionMask(mask)
    try:
        gauge, ip = _setup(qa, X, kappa, mu)
        mp = qa.multigrid_param(ip, n_level=levels, geo_block=blocks, n_vec=nvec, setup_maxiter=300, setup_tol=1e-5, smoother_pc=True, cycle=qa.QUDA_MG_CYCLE_VCYCLE)
        mg = qa.Multigrid(mp)
        try:
            V = int(np.prod(X))
            rng = np.random.default_rng(41)
            bs = [rng.random(V * 24) for _ in range(nsrc)]
            ip.inv_type_precondition, ip.preconditioner = qa.QUDA_MG_INVERTER, mg.h
            ip.tol_precondition, ip.maxiter_precondition, ip.precondition_cycle, ip.omega = 1e-1, 1, 1, 1.0
            if outer_pc:
                ip.solve_type = qa.QUDA_DIRECT_PC_SOLVE
            singles, iters = [], []
            for b in bs:
                singles.append(qa.invert(b, ip))
                iters.append(ip.iter)
            xs = qa.invert_multi_src(bs, ip)
            it_block = ip.iter
            assert abs(it_block - max(iters)) <= 1, (it_block, iters)
            for i in range(nsrc):
                res = _true_residual(oracle, gauge, X, kappa, mu, xs[i], bs[i])
                assert res < 1e-10, (i, res)
                assert np.linalg.norm(xs[i] - singles[i]) < 1e-7 * np.linalg.norm(singles[i]), i
            print("multi-source MG-GCR %s %d sources: %d lockstep iterations (single-source %s), worst residual reported %.2e" % (X, nsrc, it_block, iters, ip.true_res))
        finally:
            mg.free()
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)


@pytest.mark.parametrize("action,matpc,nu_pre,nsrc,mask,cycle", [("tm", "oo", 0, 9, 14, "V"), ("tmc", "ee", 2, 12, 0, "V"), ("tm", "ee", 2, 4, 15, "V"), ("tm", "eeasym", 2, 3, 0, "V"),
                                                                  ("tm", "ee", 2, 6, 0, "K")],
                         ids=["odd-odd-no-presmoothing-9-sources-yzt", "twisted-clover-12-sources", "4-sources-xyzt", "asymmetric-falls-back", "k-cycle"])
def test_fine_level_block_smoother(qa, oracle, action, matpc, nu_pre, nsrc, mask, cycle):
    """the fine-level smoothing of all sources on block fields (groups of 8 / 4 through the multi-right-hand-side stencil, MR sums in its epilogue,
    coefficient on the device): same outer iteration count and the same solutions as the single-source solves — odd-odd preconditioning, no
    pre-smoothing, twisted clover (dense site matrices), padded groups, partitioned dimensions; the asymmetric preconditioning is outside it
    and must run source by source; below a K-cycle the first coarse level is solved by a lockstep GCR around its block cycle, as the single-source coarse solver does per source"""
    X, kappa, mu = (16, 8, 8, 16), 0.124, 0.005
    qa.lib().qudaAmdSetPartitionMask(mask)
    try:
        gauge, ip = _setup(qa, X, kappa, mu)
        if action == "tmc":
            ip.dslash_type = qa.QUDA_TWISTED_CLOVER_DSLASH
            ip.clover_cpu_prec, ip.clover_cuda_prec, ip.clover_cuda_prec_sloppy, ip.clover_cuda_prec_precondition = 8, 8, 4, 4
            ip.clover_order = qa.QUDA_PACKED_CLOVER_ORDER
            ip.clover_coeff = kappa * 1.57551
            qa.load_clover(None, None, ip)
        ip.matpc_type = qa.MATPC[matpc]
        mp = qa.multigrid_param(ip, n_level=3, geo_block=[(4, 4, 4, 4), (2, 2, 2, 2), (2, 2, 2, 2)], n_vec=8, nu_pre=nu_pre, setup_maxiter=300, setup_tol=1e-5, smoother_pc=True,
                                cycle=qa.QUDA_MG_CYCLE_VCYCLE if cycle == "V" else qa.QUDA_MG_CYCLE_RECURSIVE)
        mg = qa.Multigrid(mp)
        try:
            rng = np.random.default_rng(47)
            bs = [rng.random(int(np.prod(X)) * 24) for _ in range(nsrc)]
            ip.inv_type_precondition, ip.preconditioner = qa.QUDA_MG_INVERTER, mg.h
            ip.tol_precondition, ip.maxiter_precondition, ip.precondition_cycle, ip.omega = 1e-1, 1, 1, 1.0
            ip.solve_type = qa.QUDA_DIRECT_PC_SOLVE
            singles, iters = [], []
            for b in bs:
                singles.append(qa.invert(b, ip))
                iters.append(ip.iter)
            s0 = qa.multi_src_stats()
            xs = qa.invert_multi_src(bs, ip)
            s1 = qa.multi_src_stats()
            assert abs(ip.iter - max(iters)) <= 1, (ip.iter, iters)
            cycles, smoothed = s1["block_cycles"] - s0["block_cycles"], s1["block_smoothed"] - s0["block_smoothed"]
            assert cycles >= ip.iter and smoothed == (0 if matpc == "eeasym" else cycles), (s0, s1)
            ip.solve_type = qa.QUDA_DIRECT_SOLVE
            for i in range(nsrc):
                assert np.linalg.norm(bs[i] - qa.mat(xs[i], ip)) < 1e-9 * np.linalg.norm(bs[i]), i
                if action == "tm":
                    assert _true_residual(oracle, gauge, X, kappa, mu, xs[i], bs[i]) < 1e-10, i
                assert np.linalg.norm(xs[i] - singles[i]) < 1e-7 * np.linalg.norm(singles[i]), i
            print("block smoother %s %s nu_pre %d, %d sources, mask %d: %d lockstep iterations (single-source %s), %s" % (action, matpc, nu_pre, nsrc, mask, ip.iter, iters, s1))
        finally:
            mg.free()
    finally:
        qa.lib().qudaAmdSetPartitionMask(0)
        qa.lib().freeCloverQuda()


def test_sources_of_different_kind_in_one_lockstep_solve(qa, oracle):
    """random sources next to sources whose solution is a constant spinor (almost in the coarse space) and a scaled, perturbed copy of one: every
    column is solved to its own relative tolerance and the smooth solution comes back to 1e-8.  (A source that converged earlier would stop
    being updated — its column turns to zeros in the block cycle; with this preconditioner all of them need the same 10 iterations, which the
    test reports.)"""
    X, kappa, mu = (16, 8, 8, 16), 0.124, 0.005
    gauge, ip = _setup(qa, X, kappa, mu)
    mp = qa.multigrid_param(ip, n_level=3, geo_block=[(4, 4, 4, 4), (2, 2, 2, 2), (2, 2, 2, 2)], n_vec=8, setup_maxiter=300, setup_tol=1e-5, smoother_pc=True, cycle=qa.QUDA_MG_CYCLE_VCYCLE)
    mg = qa.Multigrid(mp)
    try:
        V = int(np.prod(X))
        rng = np.random.default_rng(53)
        smooth = np.tile(rng.random(24), V)
        ip.inv_type_precondition = qa.QUDA_INVALID_ENUM
        b_smooth = qa.mat(smooth, ip)
        bs = [rng.random(V * 24), b_smooth, rng.random(V * 24), 3.0 * b_smooth + 1e-3 * rng.random(V * 24), rng.random(V * 24)]
        ip.inv_type_precondition, ip.preconditioner = qa.QUDA_MG_INVERTER, mg.h
        ip.tol_precondition, ip.maxiter_precondition, ip.precondition_cycle, ip.omega = 1e-1, 1, 1, 1.0
        ip.solve_type = qa.QUDA_DIRECT_PC_SOLVE
        iters = []
        for b in bs:
            qa.invert(b, ip)
            iters.append(ip.iter)
        xs = qa.invert_multi_src(bs, ip)
        assert abs(ip.iter - max(iters)) <= 1, (ip.iter, iters)
        for i in range(len(bs)):
            assert _true_residual(oracle, gauge, X, kappa, mu, xs[i], bs[i]) < 1e-10, (i, iters)
        assert np.linalg.norm(xs[1] - smooth) < 1e-8 * np.linalg.norm(smooth)
        print("sources of different difficulty: single-source iterations %s, lockstep %d" % (iters, ip.iter))
    finally:
        mg.free()


@pytest.mark.parametrize("cycle", ["V", "K"])
def test_a_source_that_converges_early_is_left_alone(qa, oracle, monkeypatch, cycle):
    """source 2 of 6 is given a tolerance 1e5 times looser (a test hook of the lockstep solver): it is finished after about half of the iterations,
    its column of every block field turns to zeros from then on (smoother groups, restrictor quads, coarse block cycle, lockstep coarsest GCR), and the
    other five still come out at 1e-10 in the usual number of iterations"""
    X, kappa, mu = (16, 8, 8, 16), 0.124, 0.005
    gauge, ip = _setup(qa, X, kappa, mu)
    mp = qa.multigrid_param(ip, n_level=3, geo_block=[(4, 4, 4, 4), (2, 2, 2, 2), (2, 2, 2, 2)], n_vec=8, setup_maxiter=300, setup_tol=1e-5, smoother_pc=True,
                            cycle=qa.QUDA_MG_CYCLE_VCYCLE if cycle == "V" else qa.QUDA_MG_CYCLE_RECURSIVE)
    mg = qa.Multigrid(mp)
    try:
        V = int(np.prod(X))
        rng = np.random.default_rng(59)
        bs = [rng.random(V * 24) for _ in range(6)]
        ip.inv_type_precondition, ip.preconditioner = qa.QUDA_MG_INVERTER, mg.h
        ip.tol_precondition, ip.maxiter_precondition, ip.precondition_cycle, ip.omega = 1e-1, 1, 1, 1.0
        ip.solve_type = qa.QUDA_DIRECT_PC_SOLVE
        ip.reliable_delta = 1e-6      # residual checks (and with them the decision that a source is finished) at every restart only otherwise
        qa.invert(bs[0], ip)
        it_single = ip.iter
        monkeypatch.setenv("QUDA_AMD_MULTISRC_TEST_LOOSE", "2:1e5")
        xs = qa.invert_multi_src(bs, ip)
        monkeypatch.delenv("QUDA_AMD_MULTISRC_TEST_LOOSE")
        assert abs(ip.iter - it_single) <= 1, (ip.iter, it_single)
        res = [_true_residual(oracle, gauge, X, kappa, mu, xs[i], bs[i]) for i in range(6)]
        print("early source (%s-cycle): residuals %s, %d iterations" % (cycle, ["%.1e" % r for r in res], ip.iter))
        assert all(r < 1e-10 for i, r in enumerate(res) if i != 2), res
        assert 1e-10 < res[2] < 1e-4, res      # stopped early, at its own tolerance
    finally:
        mg.free()


def test_multi_source_plain_gcr(qa, oracle):
    """without a preconditioner the lockstep solver is nsrc independent GCR(20) solves sharing their Krylov index"""
    X, kappa, mu = (8, 8, 8, 8), 0.124, 0.005
    gauge, ip = _setup(qa, X, kappa, mu)
    ip.inv_type_precondition = qa.QUDA_INVALID_ENUM
    rng = np.random.default_rng(43)
    bs = [rng.random(int(np.prod(X)) * 24) for _ in range(3)]
    xs = qa.invert_multi_src(bs, ip)
    for x, b in zip(xs, bs):
        assert _true_residual(oracle, gauge, X, kappa, mu, x, b) < 1e-10
