"""Self-test of tests/stored_ref.py on the CPU: the decoders against the matching encoders (which restate the loaders in numpy), every planted
error caught by the same checks the GPU test applies to the device's images, the stencil constants K16_PLAIN / K16_SITE and the 8-real constant
E8 measured, and the condition rs >= RS_MIN asserted on the seeded links of the two lattices of tests/test_stored_gpu.py.

Measured (pytest -s prints them):
    16-bit round trip   worst |dec - v| / (0.5 scale / 32767 + 3 2^-24 |v|) = 1.000 (spinors), within it for the clover term; links within
                        0.5 / 32767 + 2^-23 |v|
    fp64 decodes        12 reals: third row against the host matrix 3.85 * 2^-50 (the host fields are special-unitary to 3.4e-15)  ->  C12_FP64 = 2^-47
                        8 reals: worst |dec - U| rs / 2^-53 = 202 (12x6x10x4), 12.4 (2^4), but 5.5 in units of 2^-53 cond8, cond8 =
                        (1 + 1 / |U00| + 1 / |U20|) / rs  ->  C8_FP64 = 12
    stencil constants   worst |err| / (2^-24 T): 4.63 without, 3.85 with site matrices  ->  K16_PLAIN = 10, K16_SITE = 9 (caps 24 and 40)
    E8                  fp32 restatement of su3_reconstruct8 with sine / cosine off by 1e-6 against the fp64 decode, on the 16-bit and fp32
                        stored reals of both lattices: worst |dev| rs / 2^-24 = 56.6  ->  E8 = 128; smallest rs of the test fields 0.0429
                        (12x6x10x4, seed 37), 0.296 (2^4, seed 8)
    elimination         numpy fp64 Gauss-Jordan against the same in extended precision: worst error / (n eps |inv| |M| |inv|) = 0.515  ->  C_INV = 2.1
    recorded            smallest rs: golden files 3.5e-2, synth.make_gauge(8^4) 6.7e-3, synth.tiled_gauge(16^4) 4.7e-3, synth.smooth_gauge(16^4, 0.35) 4.1e-4"""
import os

import numpy as np
import pytest

import blas_ref as R
import fine_stencil_ref as F
import stored_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def fields(oracle, lat, anti):
    key = (lat, anti)
    if key not in _cache:
        X = S.LATTICES[lat]
        gauge, _, clover = oracle.make_fields(list(X), seed=S.SEEDS[lat], antiperiodic_t=anti, clover=True)
        for a in (gauge, clover):
            a.setflags(write=False)
        _cache[key] = (X, gauge, clover)
    return _cache[key]


# ---- round trips ----
@pytest.mark.parametrize("prec", [8, 4, 2])
@pytest.mark.parametrize("full", [False, True])
def test_spinor_round_trip(prec, full):
    """encode then decode: the identity for fp64 and fp32 (of the fp32 values); 16-bit within 0.5 scale / 32767 + 3 2^-24 |v|: with v' = fl(v),
    s = fl(32767 / m) and the product fl(v' s) each good to 2^-24 relative, the integer is v' s (1 + e1)(1 + e2) + d, |d| <= 0.5, and
    int m / 32767 = v (1 + e0)(1 + e1)(1 + e2) + d m / 32767.  Zero sites decode to zero with scale 0"""
    X = S.LATTICES["12x6x10x4"]
    v = S.operands(X, 0)
    vh = v.shape[1]
    host = v.reshape(-1) if full else v[0].reshape(-1)
    raw, nraw, info = S.encode_spinor(host, prec, full)
    for p in range(2 if full else 1):
        dec, scale = S.decode_spinor(raw, nraw, info, p)
        if prec == 8:
            assert np.array_equal(dec, v[p])
        elif prec == 4:
            assert np.array_equal(dec, v[p].astype(np.float32).astype(np.float64))
        else:
            assert np.array_equal(scale.astype(np.float32), np.max(np.abs(v[p].astype(np.float32)), axis=1))
            ratio = np.max(np.abs(dec - v[p]) / np.maximum(S.half_step_bound(v[p], scale[:, None]), 1e-300))
            print("16-bit spinor round trip: worst error / bound %.3f" % ratio)
            assert ratio <= 1.0
            zero = ~np.any(v[p], axis=1)
            assert np.sum(zero) == 1 and not np.any(dec[zero]) and not np.any(scale[zero])


@pytest.mark.parametrize("prec", [8, 4, 2])
def test_clover_round_trip(oracle, prec):
    X, _, clover = fields(oracle, "2^4", True)
    raw, nraw, info = S.encode_clover(clover, prec)
    dec, scales = S.decode_clover(raw, nraw, info)
    want = clover.reshape(2, -1, 2, 36)
    if prec == 8:
        assert np.array_equal(dec, want)
    elif prec == 4:
        assert np.array_equal(dec, want.astype(np.float32).astype(np.float64))
    else:
        sc = scales.transpose(0, 2, 1)[..., None]
        assert np.max(np.abs(dec - want) / S.half_step_bound(want, sc)) <= 1.0
    # the packed order is the oracle's: the Hermitian blocks are what apply_clover multiplies with
    m = S.clover_matrices(want[0])
    assert np.max(np.abs(m - F.dense_matrices(oracle, clover, X, 0, 0.0, False))) < 1e-14
    assert np.array_equal(S.pack_clover(m), want[0])


@pytest.mark.parametrize("lat", sorted(S.LATTICES))
@pytest.mark.parametrize("anti", [False, True])
@pytest.mark.parametrize("prec,recon", [(p, r) for p in (8, 4, 2) for r in (18, 12, 8)])
def test_link_round_trip(oracle, lat, anti, prec, recon):
    """the nine formats: the decode of the encoded field within check_links' bounds of the host blocks, negated boundary links included"""
    X, gauge, _ = fields(oracle, lat, anti)
    raw, info = S.encode_links(gauge, X, prec, recon)
    W, stored, rs = S.decode_links(raw, info, X, anti)
    res = S.check_links("%s %d/%d" % (lat, prec, recon), W, stored, rs, S.host_blocks(gauge, X), X, prec, recon, anti)
    print(res)
    if recon == 8:
        assert np.min(rs) >= S.RS_MIN


def test_negated_matrices_decode_through_the_sign():
    """12 and 8 reals of -V with sign -1 give -V back"""
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.standard_normal((50, 3, 3)) + 1j * rng.standard_normal((50, 3, 3)))
    v = q / np.linalg.det(q)[:, None, None] ** (1.0 / 3.0)
    for m, sign in ((v, 1.0), (-v, -1.0)):
        assert np.max(np.abs(S.third_row(m[:, :2], np.full(50, sign)) - m)) < 1e-14
        got, rs = S.reconstruct8(S.pack8(m, 1.0, np.float64), np.full(50, sign), 1.0)
        assert np.max(np.abs(got - m) / S.cond8(m)[:, None, None]) < S.C8_FP64 * 2.0 ** -53
    # the wrong sign is off by 2 |row 2|
    assert np.max(np.abs(S.third_row(-v[:, :2], np.ones(50)) + v)) > 0.5


# ---- planted errors ----
def _link_case(oracle, prec, recon, anti=True, lat="12x6x10x4"):
    X, gauge, _ = fields(oracle, lat, anti)
    raw, info = S.encode_links(gauge, X, prec, recon)
    return X, gauge, raw, info


@pytest.mark.parametrize("plant,prec,recon", [("no_boundary_sign", 4, 12), ("no_boundary_sign", 2, 8), ("sign_on_forward_t0", 8, 12), ("sign_on_forward_t0", 4, 8),
                                              ("tail_full_stride", 4, 18), ("tail_full_stride", 2, 18), ("tail_full_stride", 2, 12), ("phase_in_radians", 2, 8)])
def test_planted_decoder_errors_are_caught(oracle, plant, prec, recon):
    X, gauge, raw, info = _link_case(oracle, prec, recon)
    Wh = S.host_blocks(gauge, X)
    W, stored, rs = S.decode_links(raw, info, X, True)
    S.check_links("clean", W, stored, rs, Wh, X, prec, recon, True)
    W, stored, rs = S.decode_links(raw, info, X, True, plant=plant)
    with pytest.raises(R.Mismatch):
        S.check_links(plant, W, stored, rs, Wh, X, prec, recon, True)


@pytest.mark.parametrize("plant", ["backward_not_daggered", "backward_from_forward_neighbour"])
@pytest.mark.parametrize("prec,recon", [(8, 18), (2, 12), (4, 8)])
def test_planted_block_errors_are_caught(oracle, plant, prec, recon):
    """the expectation built wrongly is as good as the image built wrongly: the two disagree"""
    X, gauge, raw, info = _link_case(oracle, prec, recon)
    W, stored, rs = S.decode_links(raw, info, X, True)
    with pytest.raises(R.Mismatch) as e:
        S.check_links(plant, W, stored, rs, S.host_blocks(gauge, X, plant=plant), X, prec, recon, True)
    assert "block" in str(e.value)


def test_planted_scale_errors_are_caught(oracle):
    X = S.LATTICES["12x6x10x4"]
    v = S.operands(X, 0)
    raw, nraw, info = S.encode_spinor(v[0].reshape(-1), 2)
    dec, scale = S.decode_spinor(raw, nraw, info, 0, plant="spinor_scale_next_site")
    assert np.max(np.abs(dec - v[0]) / np.maximum(S.half_step_bound(v[0], scale[:, None]), 1e-300)) > 10.0
    _, _, clover = fields(oracle, "2^4", True)
    want = clover.reshape(2, -1, 2, 36)
    raw, nraw, info = S.encode_clover(clover, 2)
    dec, scales = S.decode_clover(raw, nraw, info, plant="clover_scale_other_block")
    assert np.max(np.abs(dec - want) / S.half_step_bound(want, scales.transpose(0, 2, 1)[..., None])) > 10.0


# ---- the reference of a launch ----
def test_hop_terms_on_blocks_and_dagger(oracle):
    X, gauge, _ = fields(oracle, "12x6x10x4", True)
    vh = int(np.prod(X)) // 2
    W = S.host_blocks(gauge, X)
    v = S.operands(X, 0)
    for parity in (0, 1):
        psi = F.to_complex(v[1 - parity].reshape(1, -1), vh)
        for dagger in (0, 1):
            want = oracle.wil_dslash(np.ascontiguousarray(gauge), np.ascontiguousarray(v[1 - parity].reshape(-1)), list(X), parity, dagger)
            for kw in (dict(blocks=W), dict()):
                got = F.to_real(F.hop_terms(gauge, X, parity, psi, dagger=bool(dagger), **kw))[0]
                assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want)), (parity, dagger, sorted(kw))


def _standin(oracle, X, links32, parity, inp32, x32, A32, Ainv32, arg):
    """one launch in fp32 with the oracle's fp32 variants (qo_wil_dslash_f, qo_apply_clover_f) standing in for the device, the epilogue as a
    sequential fp32 loop; operands float32"""
    f = np.float32
    g5 = np.tile(np.repeat(np.array([1, 1, -1, -1], dtype=f), 6), inp32.size // 24)
    swap = lambda v: np.stack([-v.reshape(-1, 2)[:, 1], v.reshape(-1, 2)[:, 0]], axis=1).reshape(-1)      # i v

    def twist(v, a):
        return (v + (f(a) * g5) * swap(v)).astype(f)

    def clov(c, v):
        return oracle.apply_clover(c, np.ascontiguousarray(v), list(X), parity)

    mode, a, b, k = arg["mode"], arg["a"], arg["b"], arg["k"]
    src = twist(inp32, a) if mode == "twist_inv_dslash" else inp32
    h = oracle.wil_dslash(links32, np.ascontiguousarray(src), list(X), parity, int(arg["dagger"]))
    if mode == "plain":
        return (x32 + f(k) * h).astype(f) if arg["xpay"] else h
    if mode in ("twist_inv", "twist_inv_dslash"):
        t = twist(h, a) if mode == "twist_inv" else h
        return (x32 + f(b) * t).astype(f) if arg["xpay"] else (f(b) * t).astype(f)
    if mode == "twist_xpay":
        return (f(k) * h + twist(x32, a)).astype(f)
    if mode == "clover_twist_inv":
        t = clov(Ainv32, (clov(A32, h) + (f(a) * g5) * swap(h)).astype(f))
        return (x32 + f(k) * t).astype(f) if arg["xpay"] else t
    return (f(k) * h + (clov(A32, x32) + (f(a) * g5) * swap(x32)).astype(f)).astype(f)


def test_stencil_constants(oracle):
    """K16_PLAIN and K16_SITE as fine_stencil_ref measures K_PLAIN: every launch of tests/test_stored_gpu.py with the oracle's fp32 variants
    standing in for the device, on operands a 16-bit device would hold (16-bit links of 18 reals, periodic and antiperiodic, the 16-bit spinors
    and clover blocks decoded and rounded to fp32); twice the worst |err| / (2^-24 T), rounded up, <= K <= the caps of fine_stencil_ref"""
    worst = {False: 0.0, True: 0.0}
    for anti in (False, True):
        X, gauge, clover = fields(oracle, "12x6x10x4", anti)
        vh = int(np.prod(X)) // 2
        raw, info = S.encode_links(gauge, X, 2, 18)
        W, _, _ = S.decode_links(raw, info, X, anti)
        links32 = S.blocks_to_qdp(W).astype(np.float32)
        W = S.host_blocks(links32.astype(np.float64), X)
        dec = lambda host: np.stack([S.decode_spinor(*S.encode_spinor(host[p].reshape(-1), 2), p * 0)[0] for p in (0, 1)]).astype(np.float32)
        inp, xop = dec(S.operands(X, 0)), dec(S.operands(X, 1))
        craw, cn, cinfo = S.encode_clover(clover, 2)
        A32 = S.decode_clover(craw, cn, cinfo)[0].astype(np.float32)
        Am = S.clover_matrices(A32.astype(np.float64))
        inv = np.linalg.inv(S.inverted_matrix(Am, (2 * S.KAPPA * S.MU) ** 2, True))
        Ainv32 = S.decode_clover(*S.encode_clover(S.pack_clover(inv).reshape(-1), 2))[0].astype(np.float32)
        Ainvm = S.clover_matrices(Ainv32.astype(np.float64))
        for c in S.launches():
            arg = S.kernel_args(c)
            for parity in (0, 1):
                got = _standin(oracle, X, links32, parity, inp[1 - parity].reshape(-1), xop[parity].reshape(-1), A32.reshape(-1), Ainv32.reshape(-1), arg)
                want, T, _ = S.launch(W, X, parity, inp[1 - parity].astype(np.float64), arg["mode"], arg["a"], arg["b"], arg["k"],
                                      x=xop[parity].astype(np.float64) if arg["xpay"] else None, dagger=arg["dagger"], A=Am[parity], Ainv=Ainvm[parity])
                assert np.all(T[np.any(inp[1 - parity], axis=1).nonzero()[0][:1]] > 0)
                ratio = float(np.max(np.abs(got.reshape(-1, 24) - want) / np.where(T > 0, S.EPS32 * T, 1.0)))
                assert ratio > 0.3, (S.launch_name(c), ratio)        # the stand-in does round: the measure is not vacuous
                site = S.uses_site_matrices(arg["mode"])
                worst[site] = max(worst[site], ratio)
    print("worst |err| / (2^-24 T): without site matrices %.2f, with %.2f" % (worst[False], worst[True]))
    assert int(np.ceil(2 * worst[False])) <= S.K16_PLAIN <= F.K_CAP_PLAIN
    assert int(np.ceil(2 * worst[True])) <= S.K16_SITE <= F.K_CAP_SITE


def test_launch_reference_is_the_oracle(oracle):
    """S.launch with the launcher's arguments on fp64 host fields is the oracle's operator: pins kernel_args and the epilogues"""
    X, gauge, clover = fields(oracle, "12x6x10x4", True)
    W = S.host_blocks(gauge, X)
    v, xo = S.operands(X, 0), S.operands(X, 1)
    mu2 = (2 * S.KAPPA * S.MU) ** 2
    Am = S.clover_matrices(clover.reshape(2, -1, 2, 36))
    Ainvm = np.linalg.inv(S.inverted_matrix(Am, mu2, True))
    cinv = oracle.clover_twisted_inverse(np.ascontiguousarray(clover), mu2)
    g, xl = np.ascontiguousarray(gauge), list(X)
    n = 0
    for c in S.launches():
        arg = S.kernel_args(c)
        if c["call"] == "M":
            full = np.ascontiguousarray(v.reshape(-1))
            ref = (oracle.tm_mat(g, full, xl, S.KAPPA, S.MU, c["flavor"], c["dagger"]) if c["op"] == "tm"
                   else oracle.tmc_mat(g, np.ascontiguousarray(clover), full, xl, S.KAPPA, S.MU, c["flavor"], c["dagger"])).reshape(2, -1, 24)
            for parity in (0, 1):
                want, _, _ = S.launch(W, X, parity, v[1 - parity], arg["mode"], arg["a"], arg["b"], arg["k"], x=v[parity], dagger=arg["dagger"], A=Am[parity], Ainv=Ainvm[parity])
                assert np.max(np.abs(want - ref[parity])) <= 1e-12 * np.max(np.abs(ref[parity])), S.launch_name(c)
                n += 1
        elif c["call"] == "dslash" and c["op"] != "wilson":
            for parity in (0, 1):
                src = np.ascontiguousarray(v[1 - parity].reshape(-1))
                matpc = {"ee": "ee", "eeasym": "eeasym"}[c["matpc"]]
                if c["op"] == "tm":
                    ref = oracle.tm_dslash(g, src, xl, S.KAPPA, S.MU, c["flavor"], parity, matpc, c["dagger"])
                elif arg["mode"] == "plain":
                    continue       # the clover-twist inverse is the caller's launch there
                elif c["dagger"]:  # the oracle's daggered dslash applies the inverse of the other parity first; the launch is the rest of it
                    ref = oracle.twist_clover_gamma5(oracle.wil_dslash(g, src, xl, parity, 1), np.ascontiguousarray(clover), cinv, xl, S.KAPPA, S.MU, c["flavor"], parity, 1, 1)
                else:
                    ref = oracle.tmc_dslash(g, src, np.ascontiguousarray(clover), cinv, xl, S.KAPPA, S.MU, c["flavor"], parity, matpc, c["dagger"])
                want, _, _ = S.launch(W, X, parity, v[1 - parity], arg["mode"], arg["a"], arg["b"], arg["k"], dagger=arg["dagger"], A=Am[parity], Ainv=Ainvm[parity])
                assert np.max(np.abs(want - ref.reshape(-1, 24))) <= 1e-12 * np.max(np.abs(ref)), S.launch_name(c)
                n += 1
    assert n >= 40


# ---- the 8-real format ----
def test_reconstruct8_in_fp32(oracle):
    """E8: su3_reconstruct8 restated in numpy float32 on the stored reals of the test fields (fp32 and 16-bit), sine and cosine off by the 1e-6
    csrc/device_io.h states for v_sin_f32 / v_cos_f32 in all four sign combinations; twice the worst element-wise deviation from the fp64
    decode times rs, in units of 2^-24, <= E8"""
    worst, rsmin = 0.0, {}
    for lat in sorted(S.LATTICES):
        for anti in (False, True):
            X, gauge, _ = fields(oracle, lat, anti)
            for prec in (4, 2):
                raw, info = S.encode_links(gauge, X, prec, 8)
                W, stored, rs = S.decode_links(raw, info, X, anti)
                sign = np.broadcast_to(S.boundary_sign(X, 8, anti)[None], rs.shape)
                unit = np.pi if prec == 2 else 1.0
                for ds in (-1e-6, 1e-6):
                    for dc in (-1e-6, 1e-6):
                        W32, _ = S.reconstruct8(stored, sign, unit, dtype=np.float32, ds=ds, dc=dc)
                        worst = max(worst, float(np.max(np.abs(W32 - W).real * rs[..., None, None])), float(np.max(np.abs((W32 - W).imag) * rs[..., None, None])))
                rsmin[lat] = min(rsmin.get(lat, 1.0), float(np.min(rs)))
    print("fp32 reconstruction: worst deviation rs / 2^-24 = %.2f; smallest rs %s" % (worst / S.EPS32, rsmin))
    assert 2.0 * worst / S.EPS32 <= S.E8


@pytest.mark.parametrize("lat", sorted(S.LATTICES))
@pytest.mark.parametrize("anti", [False, True])
def test_seeded_links_are_away_from_the_singular_set(oracle, lat, anti):
    X, gauge, _ = fields(oracle, lat, anti)
    W = S.host_blocks(gauge, X)
    rs = np.abs(W[..., 0, 1]) ** 2 + np.abs(W[..., 0, 2]) ** 2
    print("%s: smallest rs per block %s" % (lat, np.array2string(np.min(rs, axis=2), precision=3)))
    assert np.all(np.min(rs, axis=2) >= S.RS_MIN)


def test_record_rs_of_real_use():
    """record only: the smallest rs = |U01|^2 + |U02|^2 of the links real use stores in 8 reals: the golden files' links and the fields bench.py
    builds for its 8-real runs.  rs -> 0 (diagonal links, the unit gauge) is the singular set of the format"""
    import glob

    def smallest(u):
        return float(min((np.abs(u[..., 0, 1]) ** 2 + np.abs(u[..., 0, 2]) ** 2).min(), (np.abs(u[..., 1, 0]) ** 2 + np.abs(u[..., 2, 0]) ** 2).min()))

    rows = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_*.npz"))):
        data = np.load(path)
        rows.append((os.path.relpath(path, ROOT), smallest(S.to_matrix(np.stack([data["gauge%d" % mu] for mu in range(4)]).reshape(4, -1, 18)))))
    from synth import make_gauge, smooth_gauge, tiled_gauge       # bench.py: make_gauge / tiled_gauge for the stencil runs, smooth_gauge(., 0.35) for the solves
    for name, g in (("synth.make_gauge((8, 8, 8, 8))", make_gauge((8, 8, 8, 8))), ("synth.tiled_gauge((16, 16, 16, 16))", tiled_gauge((16, 16, 16, 16))),
                    ("synth.smooth_gauge((16, 16, 16, 16), 0.35)", smooth_gauge((16, 16, 16, 16), 0.35))):
        rows.append((name, smallest(S.to_matrix(np.asarray(g).reshape(4, -1, 18)))))
    for name, v in rows:
        print("smallest rs  %-60s %.3e" % (name, v))


def test_elimination_constant(oracle):
    """C_INV as tests/test_coarse_pc_gpu.py fixes its constant: four times the worst ratio of a numpy elimination in the kernel's precision (fp64,
    whatever the storage) to n eps |inv| |M| |inv|, on the matrices the GPU test inverts (A^2 + mu2 of the seeded clover term as an fp64, fp32
    and 16-bit field holds it), against the same elimination in extended precision"""
    mu2 = (2 * S.KAPPA * S.MU) ** 2
    worst = 0.0
    for lat in sorted(S.LATTICES):
        _, _, clover = fields(oracle, lat, True)
        for prec in (8, 4, 2):
            A = S.clover_matrices(S.decode_clover(*S.encode_clover(clover, prec), as_loaded=True)[0]).reshape(-1, 6, 6)
            M = S.inverted_matrix(A, mu2, True)
            got, tl = S.gauss_jordan(M, np.complex128)
            ref, _ = S.gauss_jordan(M.astype(np.clongdouble), np.clongdouble)
            assert np.max(np.abs(ref.astype(np.complex128) - np.linalg.inv(M))) < 1e-12 * np.max(np.abs(ref))
            assert np.max(np.abs(tl - np.linalg.slogdet(M)[1])) < 1e-13 * 6
            worst = max(worst, float(np.max(np.abs(got - ref).astype(np.float64) / S.inverse_bound(A, np.linalg.inv(M), mu2, True))))
    print("fp64 elimination: worst error / (n eps |inv| |M| |inv|) = %.3f" % worst)
    assert 4.0 * worst <= S.C_INV
