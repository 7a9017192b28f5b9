"""numpy restatements for the coarse-level transfer tests (tests/test_coarse_transfer_gpu.py, tests/test_transfer_ref.py): the aggregate
tables, R, P and the block orthonormalisation in a few lines of einsum / QR, a batched modified Gram-Schmidt in a chosen precision (the
reference-only figure behind the orthonormalisation bar), the rules by which csrc/transfer_setup.hip and csrc/transfer.hip pick the aggregate
shape and the kernel route, and a restrictor with the errors a lane-group kernel can make planted in it.

Fields are in the host order of the oracle (oracle/qo_mg.c): site = parity * Vh + x_cb, vectors (site, spin, colour), V (site, spin, colour, vector)."""
import numpy as np


def coords_eo(X):
    """(V, 4) coordinates x, y, z, t of every site of the even-odd host order"""
    X = [int(v) for v in X]
    V = int(np.prod(X))
    c = np.indices(X[::-1]).reshape(4, -1)[::-1]      # rows x, y, z, t of the lexicographic sites, x fastest
    eo = (c.sum(axis=0) & 1) * (V // 2) + np.arange(V) // 2
    out = np.empty((V, 4), dtype=np.int64)
    out[eo] = c.T
    return out


def aggregates(X, bs):
    """(nAgg, blockVol) fine sites of every aggregate: row = the coarse site in ITS even-odd order (createGeoMap), columns lexicographic in the block"""
    X, bs = np.array(X, dtype=np.int64), np.array(bs, dtype=np.int64)
    Xc = X // bs
    x = coords_eo(X)
    xc, y = x // bs, x % bs
    lexc = ((xc[:, 3] * Xc[2] + xc[:, 2]) * Xc[1] + xc[:, 1]) * Xc[0] + xc[:, 0]
    A = (xc.sum(axis=1) & 1) * (int(np.prod(Xc)) // 2) + lexc // 2
    b = ((y[:, 3] * bs[2] + y[:, 2]) * bs[1] + y[:, 1]) * bs[0] + y[:, 0]
    table = np.full((int(np.prod(Xc)), int(np.prod(bs))), -1, dtype=np.int64)
    table[A, b] = np.arange(len(x))
    assert table.min() == 0 and len(np.unique(table)) == len(x)
    return table


def restrict(phi, V, table, spin_bs=1):
    """out(A, chi, v) = sum over the sites of A, the spins of chi and colour of conj(V) phi"""
    nA, bv = table.shape
    Ns, Nc, Nv = V.shape[1:]
    W = V[table].reshape(nA, bv, Ns // spin_bs, spin_bs, Nc, Nv)
    return np.einsum("abxscv,abxsc->axv", W.conj(), phi[table].reshape(nA, bv, Ns // spin_bs, spin_bs, Nc))


def prolongate(eta, V, table, spin_bs=1):
    """out(x, s, c) = sum_v V(x, s, c, v) eta(A(x), chi(s), v)"""
    nA, bv = table.shape
    Ns, Nc, Nv = V.shape[1:]
    W = V[table].reshape(nA, bv, Ns // spin_bs, spin_bs, Nc, Nv)
    out = np.empty(V.shape[:3], dtype=np.result_type(V, eta))
    out[table] = np.einsum("abxscv,axv->abxsc", W, eta).reshape(nA, bv, Ns, Nc)
    return out


def block_matrices(F, table, spin_bs=1):
    """(nAgg * nChi, blockVol * spin_bs * Nc, Nvec): the tall matrix of every (aggregate, chirality) block of F (site, spin, colour, vector)"""
    nA, bv = table.shape
    Ns, Nc, Nv = F.shape[1:]
    M = F[table].reshape(nA, bv, Ns // spin_bs, spin_bs * Nc, Nv).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(M).reshape(nA * (Ns // spin_bs), bv * spin_bs * Nc, Nv)


def from_block_matrices(M, table, Ns, Nc, spin_bs=1):
    nA, bv = table.shape
    Nv = M.shape[-1]
    out = np.empty((table.size, Ns, Nc, Nv), dtype=M.dtype)
    out[table] = M.reshape(nA, Ns // spin_bs, bv, spin_bs * Nc, Nv).transpose(0, 2, 1, 3, 4).reshape(nA, bv, Ns, Nc, Nv)
    return out


def block_qr(B, table, spin_bs=1):
    """block orthonormalisation by Householder QR with the diagonal of R made positive: what Gram-Schmidt computes, by another algorithm"""
    M = block_matrices(B, table, spin_bs)
    Q, R = np.linalg.qr(M)
    d = np.diagonal(R, axis1=-2, axis2=-1)
    return from_block_matrices(Q * (d / np.abs(d))[:, None, :], table, B.shape[1], B.shape[2], spin_bs)


def gram_schmidt(M, dtype):
    """modified Gram-Schmidt over the columns of every matrix of the batch M (blocks, rows, Nvec) with every operation in `dtype`
    (oracle/qo_mg.c qo_mg_block_orthogonalize, reference lib/transfer_util.cu:328-363)"""
    M = np.array(M, dtype=dtype)
    real = np.zeros(1, dtype=dtype).real.dtype
    for j in range(M.shape[-1]):
        for i in range(j):
            dot = np.einsum("bm,bm->b", M[:, :, i].conj(), M[:, :, j]).astype(dtype)
            M[:, :, j] -= dot[:, None] * M[:, :, i]
        nrm2 = np.einsum("bm,bm->b", M[:, :, j].conj(), M[:, :, j]).real.astype(real)
        M[:, :, j] *= (real.type(1) / np.sqrt(nrm2))[:, None]
    return M


# ---- the rules of the library, restated ----
def blocks_after_fallback(Xf, bs):
    """Transfer::Transfer (reference lib/transfer.cpp:31-44): a block extent is halved until it divides the lattice into an EVEN number of
    blocks, and the x extent may not cover the whole lattice — no coarse lattice has an odd extent, 1 included"""
    out = []
    for d in range(4):
        b = int(bs[d])
        while b > 0:
            if d == 0 and Xf[0] == b:
                pass
            elif (Xf[d] // b) % 2 == 1:
                pass
            elif (Xf[d] // b) * b != Xf[d]:
                pass
            else:
                break
            b //= 2
        out.append(b)
    return out


def route(blockVol, nvec):
    """transfer.hip workGroup + the slot arithmetic of restrict_small_kernel (512 threads): (route, GS, slots, trips of the iteration loop)"""
    if blockVol > 32:
        return ("general", None, None, None)
    gs = 1
    while gs < blockVol:
        gs <<= 1
    slots = 8 * (64 // gs)
    return ("small", gs, slots, -(-nvec // slots))


# ---- the cases of tests/test_coarse_transfer_gpu.py: fine lattice, blocks asked for on level 1, Nvec of levels 0 and 1, set-up iterations, and
# what level 1 then is (blocks after the fallback, route, GS, slots, trips).  a-f are the lattices first proposed for these paths: the fallback above halves their
# level-1 blocks, so none of them reaches the aggregate it was meant for; A-F are the smallest lattices that do (every level-1 extent doubled).
CASES = {
    "a": ((8, 8, 8, 16), (2, 2, 2, 2), (24, 24), 50, ((1, 1, 1, 2), "small", 2, 256, 1)),
    "b": ((8, 8, 8, 16), (2, 2, 2, 2), (24, 32), 50, ((1, 1, 1, 2), "small", 2, 256, 1)),
    "c": ((8, 8, 8, 24), (2, 2, 2, 3), (32, 32), 50, ((1, 1, 1, 3), "small", 4, 128, 1)),
    "d": ((16, 8, 8, 16), (2, 2, 2, 2), (8, 4), 50, ((2, 1, 1, 2), "small", 4, 128, 1)),
    "e": ((8, 8, 16, 32), (2, 2, 4, 4), (8, 8), 50, ((1, 1, 2, 4), "small", 8, 64, 1)),
    "f": ((8, 8, 8, 32), (2, 2, 2, 4), (4, 4), 50, ((1, 1, 1, 4), "small", 4, 128, 1)),
    "A": ((16, 16, 16, 16), (2, 2, 2, 2), (24, 24), 10, ((2, 2, 2, 2), "small", 16, 32, 1)),
    "B": ((16, 16, 16, 16), (2, 2, 2, 2), (24, 32), 10, ((2, 2, 2, 2), "small", 16, 32, 1)),
    "C": ((16, 16, 16, 24), (2, 2, 2, 3), (32, 32), 10, ((2, 2, 2, 3), "small", 32, 16, 2)),
    "D": ((16, 16, 16, 16), (2, 2, 2, 2), (8, 4), 10, ((2, 2, 2, 2), "small", 16, 32, 1)),
    "E": ((16, 16, 32, 32), (2, 2, 4, 4), (8, 8), 10, ((2, 2, 4, 4), "general", None, None, None)),
    "F": ((16, 16, 16, 32), (2, 2, 2, 4), (4, 4), 10, ((2, 2, 2, 4), "small", 32, 16, 1)),
}


def case_id(name):
    X, req, nvec, _, (got, rt, gs, slots, trips) = CASES[name]
    tail = "general-NSF2" if rt == "general" else "small-GS%d-slots%d-trips%d" % (gs, slots, trips)
    return "%s-%s-ask%s-get%s-blockVol%d-%s-2x%dto%d" % (name, "x".join(map(str, X)), "x".join(map(str, req)), "x".join(map(str, got)), int(np.prod(got)), tail, nvec[0], nvec[1])


# ---- a restrictor built the way restrict_small_kernel is (component k = spin * Nc + colour, iteration it = chi * Nvec / 2 + vector pair on
# `nslots` lane groups), with one error planted ----
def restrict_planted(phi, V, table, nslots, error=None, spin_bs=1):
    nA, bv = table.shape
    Ns, Nc, Nv = V.shape[1:]
    K = Ns * Nc
    W, f = V[table].reshape(nA, bv, K, Nv), phi[table].reshape(nA, bv, K)
    k = np.arange(K)
    chi_of_k = (k // Nc) // (2 if error == "chirality" else spin_bs)   # planted: the fine level's spin blocking on a 2-spin level
    out = np.zeros((nA, 2, Nv), dtype=np.result_type(V, phi))
    for chi in range(2):
        sel = chi_of_k == chi
        out[:, chi] = np.einsum("abkv,abk->av", W[:, :, sel].conj(), f[:, :, sel])
    if error == "swap":      # the two vectors of a pair written to each other's place
        out = out.reshape(nA, 2, Nv // 2, 2)[..., ::-1].reshape(nA, 2, Nv)
    if error == "leak":      # a reduction one lane group too wide: the neighbour's sum arrives on top
        out = out.copy()
        out[0::2] += out[1::2]
    if error == "drop":      # the second trip of `for (it = slot; it < NIT; it += nslots)` never made
        it = np.arange(2)[:, None] * (Nv // 2) + np.arange(Nv)[None, :] // 2
        out = np.where(it[None] < nslots, out, 0)
    return out
