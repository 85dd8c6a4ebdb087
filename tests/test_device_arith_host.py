"""CPU-side half of the device-arithmetic checks (tests/devcheck.py): both compilations of the operation table build -- the gfx950 one
by cross-compilation -- and export what the Python side declares; the table entries no other host test pins get their residue
checks against Python integers here (tests/test_gpu_device_arith.py then compares the device build with this host build bit for
bit); and the comparators of the GPU tests reject what they must."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import devcheck as dc
from devcheck import FIELDS, LM, dc_dec, dc_host, dc_pools  # noqa: F401  (fixtures)


def test_both_libraries_build_and_export_the_table(dc_host, pkg):
    dc.build()
    want = "".join("%s:%d:%d;" % (k, v[0], v[1]) for k, v in dc.OPS.items())
    assert dc_host.dc_table().decode() == want
    cmd = dc.device_build_command()
    mk = open(os.path.join(dc.PRODUCT_CSRC, "Makefile")).read()
    assert "--offload-arch=gfx950" in cmd and "-O3" in cmd and all(f in mk for f in cmd[2:-4]), "the harness is built with the product's flags"
    dev = dc.device_lib()                               # loads without a GPU, like libtemsm.so
    assert dev.dc_table().decode() == want
    for name in list(dc.OPS) + ["%s_%d" % (k, n) for k in dc.DEVICE_ONLY for n in (9, 14)]:
        assert hasattr(dev, "dc_" + name), name
    blob = open(dc.DEV_SO, "rb").read()
    assert b"gfx950" in blob and b"k_reduce_tail" in blob and b"k_sum_groups_team" in blob
    # the table is HIP-free and includes the product's headers unchanged
    text = open(os.path.join(dc.CSRC, "devcheck_ops.hpp")).read()
    assert "hip/" not in text and "csrc/curve.hpp" in text and "csrc/scalar_form.hpp" in text


def test_pool_operands_are_what_they_are_named(dc_host, dc_pools, dc_dec, fpcheck, fq377check):
    """the accumulators the GPU tests feed decode to their model points; the O that came out of P + (-P) carries the representative p;
    records equal those of the older shims (fpc_prep_point / f377_prep_point), identities those of fpc_identity / f377_identity"""
    for N, pool in dc_pools.items():
        F = FIELDS[N]
        for i, acc in enumerate(pool.acc):
            dc_dec.check("pool", N, acc, pool.pts[i], "entry %d" % i)
        zp = pool.acc[pool.zero_p].reshape(4, N)
        assert F.val(zp[0]) == F.P and F.val(zp[3]) == F.P, "x and t of P + (-P) are the representative p of zero"
        ident = ctypes.create_string_buffer(16 * N)
        (fpcheck.fpc_identity if N == 9 else fq377check.f377_identity)(ident)
        assert ident.raw == pool.acc[pool.ident].tobytes()
        for j in (0, 3, len(pool.rec) - 1):
            x, y = pool.rec_pts[j]
            if N == 9:
                rec = ctypes.create_string_buffer(128)
                fpcheck.fpc_prep_point(x.to_bytes(32, "little") + y.to_bytes(32, "little"), rec)
                assert rec.raw[:108] == pool.rec[j].tobytes()
            else:
                rec = ctypes.create_string_buffer(224)
                fq377check.f377_prep_point(x.to_bytes(48, "little") + y.to_bytes(48, "little"), rec)
                assert rec.raw == pool.rec[j].tobytes()
    names = [c[0] for c in dc_pools[9].pair_cases()]
    assert {"O+O", "O+P", "P+O", "P+P", "P+(-P)", "P+Q", "O'+P", "P+T2", "T4+T4"} <= set(names)
    assert {"O+O", "O+P", "P+O", "P+P", "P+(-P)", "P+Q", "O'+P"} <= set(c[0] for c in dc_pools[14].pair_cases())


@pytest.mark.parametrize("N", (9, 14))
def test_residues_of_the_new_table_entries(N, dc_host, dc_pools):
    """mont_mul_x<M> (every chain its own product), fe_mul, fq_mul3, fe_norm, fe_sub<K>, fe_neg<K>, mask_select and pnt_cneg against
    Python integers, on the operands the device tests use"""
    F = FIELDS[N]
    P, val = F.P, F.val

    def product_ok(a, b, r):
        return val(r) % P == val(a) * val(b) * F.rinv % P and val(r) < val(a) * val(b) // F.R + P + 1 and all(int(x) <= LM for x in r[:N - 1])
    for name in ["mul_%d" % N] + ["mul_x%d_%d" % (M, N) for M in (2, 3, 4)]:
        inp = dc.table_inputs(name, dc_pools)
        out = dc.run_host(name, inp)
        M = inp.shape[1] // (2 * N)
        for e in range(len(inp)):
            for c in range(M):
                a, b = inp[e, 2 * N * c:2 * N * c + N], inp[e, 2 * N * c + N:2 * N * (c + 1)]
                assert product_ok(a, b, out[e, N * c:N * (c + 1)]), (name, e, c)
        if M > 1:                                                   # the chains do differ: a mix-up between them would show
            assert sum(1 for e in range(len(inp)) if len({out[e, N * c:N * (c + 1)].tobytes() for c in range(M)}) == M) > 0.7 * len(inp)
    for K in (2, 4, 16):
        inp = dc.table_inputs("sub%d_%d" % (K, N), dc_pools)
        out = dc.run_host("sub%d_%d" % (K, N), inp)
        for e in range(len(inp)):
            assert val(out[e]) == val(inp[e, :N]) - val(inp[e, N:]) + K * P, (K, e)
            assert list(out[e]) == [int(a) + o - int(b) for a, b, o in zip(inp[e, :N], inp[e, N:], F.offset(K))], "limb-wise, no carries"
    for K in (2, 4):
        inp = dc.table_inputs("neg%d_%d" % (K, N), dc_pools)
        out = dc.run_host("neg%d_%d" % (K, N), inp)
        for e in range(len(inp)):
            assert val(out[e]) == K * P - val(inp[e]) and all(int(x) < 1 << 31 for x in out[e]), (K, e)
    inp = dc.table_inputs("norm_%d" % N, dc_pools)
    out = dc.run_host("norm_%d" % N, inp)
    for e in range(len(inp)):
        assert val(out[e]) == val(inp[e]) and all(int(x) <= LM for x in out[e, :N - 1]), e
    if N == 14:
        inp = dc.table_inputs("mul3_14", dc_pools)
        out = dc.run_host("mul3_14", inp)
        assert all(val(out[e]) == 3 * val(inp[e]) and all(int(o) == 3 * int(i) for o, i in zip(out[e], inp[e])) for e in range(len(inp)))
    else:
        inp = dc.table_inputs("select", dc_pools)
        out = dc.run_host("select", inp)
        assert all(int(out[e, 0]) == (int(b) & int(mk)) | (int(a) & ~int(mk) & 0xFFFFFFFF) for e, (mk, b, a) in enumerate(inp))
        for name, mod in dc.SCALAR_MODULI.items():
            inp = dc.table_inputs(name, dc_pools)
            out = dc.run_host(name, inp)
            rinv = pow(dc.RA, -1, mod)
            w = lambda r: sum(int(x) << (32 * i) for i, x in enumerate(r))
            assert all(w(out[e]) == w(inp[e]) * rinv % mod for e in range(len(inp))), name
    # ete_add<N> on the synthetic limb-extreme accumulators (no curve points: the nine products, coordinate by coordinate)
    inp = dc.extreme_pairs(N)
    out = dc.run_host("add_%d" % N, inp)
    mm = lambda a, b: a * b * F.rinv % P
    for e in range(len(inp)):
        x1, y1, z1, t1, x2, y2, z2, t2 = (val(inp[e, N * c:N * (c + 1)]) for c in range(8))
        A, B, C, D = mm(y1 - x1, y2 - x2), mm(y1 + x1, y2 + x2), 2 * dc_pools[N].d * mm(t1, t2), 2 * mm(z1, z2)
        E, H, Fv, G = B - A, B + A, D - C, D + C
        assert [val(out[e, N * c:N * (c + 1)]) % P for c in range(4)] == [mm(E, Fv), mm(H, G), mm(Fv, G), mm(E, H)], e
        dc.check_contract("ete_add<%d>" % N, N, out[e])
    for name in ["cneg_%d" % N] + (["cneg_aff"] if N == 14 else []):
        inp = dc.table_inputs(name, dc_pools)
        out = dc.run_host(name, inp)
        for e in range(len(inp)):
            rec, sign = inp[e, :-1], int(inp[e, -1])
            hm, hp, dt, rest = rec[:N], rec[N:2 * N], rec[2 * N:3 * N], rec[3 * N:]
            if sign == 0:
                assert list(out[e]) == list(rec), (name, e)
            else:                                                   # -(x, y) = (-x, y): hm and hp change places, dt becomes 4p - dt, z stays
                assert list(out[e, :N]) == list(hp) and list(out[e, N:2 * N]) == list(hm) and list(out[e, 3 * N:]) == list(rest), (name, e)
                assert val(out[e, 2 * N:3 * N]) == 4 * P - val(dt) and all(int(x) < int(2 ** 30.6) for x in out[e, 2 * N:3 * N]), (name, e)


@pytest.mark.parametrize("N", (9, 14))
def test_point_formulas_of_the_table_against_the_model(N, dc_host, dc_pools, dc_dec):
    """ete_from_pnt, ete_from_pair, ete_madd for every record kind and ete_add<N> of the host build decode to the model's points on the
    exceptional operands the device tests use (the older host tests pin these formulas on their own, smaller sets)"""
    pool = dc_pools[N]
    kinds = [("%d" % N, pool.rec)] + ([("aff", pool.rec_aff)] if N == 14 else [])
    nr = len(pool.rec)
    sign = lambda r: pool.rec_pts[r] if r < nr else dc.mneg(N, pool.rec_pts[r - nr])
    for suffix, recs in kinds:
        cn = "cneg_aff" if suffix == "aff" else "cneg_%d" % N
        both = np.vstack([recs, dc.run_host(cn, np.hstack([recs, np.ones((nr, 1), dtype=np.uint32)]))])
        out = dc.run_host("from_pnt_" + suffix, both)
        for r in range(2 * nr):
            dc_dec.check("ete_from_pnt", N, out[r], sign(r), "record %d" % r)
        rnd = random.Random(7)
        idx = [(i, i) for i in range(nr)] + [(i, i + nr) for i in range(nr)] + [(rnd.randrange(2 * nr), rnd.randrange(2 * nr)) for _ in range(40)]
        out = dc.run_host("from_pair_" + suffix, np.array([np.concatenate([both[a], both[b]]) for a, b in idx], dtype=np.uint32))
        for e, (a, b) in enumerate(idx):
            dc_dec.check("ete_from_pair", N, out[e], dc.msum(N, [sign(a), sign(b)]), "records %d, %d" % (a, b))
        idx = [(rnd.randrange(len(pool.acc)), rnd.randrange(2 * nr)) for _ in range(60)] + [(0, 1), (1, 2), (2, nr), (2, 0)]
        out = dc.run_host("madd_" + suffix, np.array([np.concatenate([pool.acc[a], both[b]]) for a, b in idx], dtype=np.uint32))
        for e, (a, b) in enumerate(idx):
            dc_dec.check("ete_madd", N, out[e], dc.msum(N, [pool.pts[a], sign(b)]), "accumulator %d, record %d" % (a, b))
    cases = pool.pair_cases()
    out = dc.run_host("add_%d" % N, np.array([np.concatenate([pool.acc[a], pool.acc[b]]) for _, a, b in cases], dtype=np.uint32))
    for e, (name, a, b) in enumerate(cases):
        dc_dec.check("ete_add<%d>" % N, N, out[e], dc.msum(N, [pool.pts[a], pool.pts[b]]), name)


@pytest.mark.parametrize("N", (9, 14))
def test_the_comparators_bite(N, dc_host, dc_pools, dc_dec):
    """what the GPU tests would see from a wrong device build, made from host-build outputs: one limb bit flipped, T negated, a
    coordinate replaced by its residue + 2p, two chains of mont_mul_x exchanged -- each rejected, with the operation named"""
    F, pool = FIELDS[N], dc_pools[N]
    cases = pool.pair_cases()
    inp = np.array([np.concatenate([pool.acc[a], pool.acc[b]]) for _, a, b in cases], dtype=np.uint32)
    good = dc.run_host("add_%d" % N, inp)
    dc.compare_bits("add_%d" % N, good, good.copy(), inp)
    e = 10                                                          # P+Q
    want = dc.msum(N, [pool.pts[cases[e][1]], pool.pts[cases[e][2]]])
    dc_dec.check("ete_add_team<%d>" % N, N, good[e], want)
    # one bit of one limb
    for word, bit in ((0, 0), (N - 1, 3), (2 * N + 4, 28), (4 * N - 1, 0)):
        bad = good.copy()
        bad[e, word] ^= np.uint32(1 << bit)
        with pytest.raises(AssertionError, match=r"add_%d: element %d word %d" % (N, e, word)):
            dc.compare_bits("add_%d" % N, bad, good, inp)
        with pytest.raises(AssertionError, match=r"ete_add_team<%d>" % N):
            dc_dec.check("ete_add_team<%d>" % N, N, bad[e], want)
    # T negated: class N and below 1.1 p still, the point's x and y unchanged -- only T Z = X Y notices
    acc = good[e].copy().reshape(4, N)
    acc[3] = F.limbs(F.P - F.val(acc[3]) % F.P)
    with pytest.raises(AssertionError, match=r"k_reduce_tail<%d>" % N):
        dc_dec.check("k_reduce_tail<%d>" % N, N, acc.reshape(-1), want)
    # a coordinate outside the bound: the same residue, + 2p
    acc = good[e].copy().reshape(4, N)
    acc[1] = F.limbs(F.val(acc[1]) % F.P + 2 * F.P)
    with pytest.raises(AssertionError, match=r"block_sum_points<%d, true>: coordinate y is not below 1.1 p" % N):
        dc_dec.check("block_sum_points<%d, true>" % N, N, acc.reshape(-1), want)
    acc = good[e].copy().reshape(4, N)
    acc[0, 0] += np.uint32(1 << 29)                                  # the same value with limb 0 not carried
    acc[0, 1] -= np.uint32(1)
    with pytest.raises(AssertionError, match=r"k_sum_groups_team<%d>: coordinate x is not of limb class N" % N):
        dc_dec.check("k_sum_groups_team<%d>" % N, N, acc.reshape(-1), want)
    # the right point in the wrong place
    with pytest.raises(AssertionError, match=r"k_sum_groups<%d, true>: .* the model gives" % N):
        dc_dec.check("k_sum_groups<%d, true>" % N, N, good[e + 1], want, "output 3")
    # two interleaved chains exchanged
    for M in (2, 3, 4):
        name = "mul_x%d_%d" % (M, N)
        minp = dc.table_inputs(name, dc_pools)
        mgood = dc.run_host(name, minp)
        bad = mgood.copy()
        bad[:, :N], bad[:, N:2 * N] = mgood[:, N:2 * N], mgood[:, :N]
        with pytest.raises(AssertionError, match=name + ": element 0 word"):
            dc.compare_bits(name, bad, mgood, minp)


# ---- the second table: check.hip.hpp, from_x.hip.hpp, scalar_mul.hip.hpp ------------------------------------------------------------
def test_the_second_table_builds_and_exports(dc_host, pkg):
    dc.build()
    want = "".join("%s:%d:%d;" % (k, v[0], v[1]) for k, v in dc.OPS2.items())
    assert dc.host_lib2().dc_table().decode() == want
    cmd = dc.device_build_command(second=True)
    mk = open(os.path.join(dc.PRODUCT_CSRC, "Makefile")).read()
    assert "--offload-arch=gfx950" in cmd and "-O3" in cmd and all(f in mk for f in cmd[2:-4]), "built with the product's flags"
    assert cmd[2:-2] == dc.device_build_command()[2:-2], "both device libraries take the same flags"
    dev = dc.device_lib2()                              # loads without a GPU
    assert dev.dc_table().decode() == want
    assert all(hasattr(dev, "dc_" + name) for name in dc.OPS2)
    blob = open(dc.DEV2_SO, "rb").read()
    assert b"gfx950" in blob and b"k_dc_sqrt_ratio_9" in blob and b"k_dc_aff_group_377" in blob
    text = open(os.path.join(dc.CSRC, "devcheck_ops2.hpp")).read()
    assert "hip/" not in text and "csrc/scalar_mul.hip.hpp" in text
    assert not set(dc.OPS) & set(dc.OPS2)


@pytest.mark.parametrize("name", list(dc.OPS2))
def test_the_second_table_against_bigints(name, dc_host, dc_pools, dc_dec):
    """the host build of every operation of the second table on the operands the device test uses, pinned to Python integers and the
    bigint models (devcheck.check_table2): zero tests, canonical conversions, inverses, roots of every 2-adic order, word compares, the
    complete short-Weierstrass formulas with their exceptional pairs, the negating addition against ete_add<9> on (a, +-b), the order
    chain on the whole curve, the offset recoding, the affine groups with infinity in every position, and the verdicts"""
    inp = dc.table2_inputs(name)
    dc.check_table2(name, inp, dc.run_host(name, inp), dc_dec)


def test_the_second_table_comparators_bite(dc_host, dc_pools, dc_dec):
    """outputs a wrong build would give, made from the host build's: a wrong verdict word, the other root, a to_canon output left at
    value + modulus, a wrong digit, a finite point where infinity belongs, Y kept by the conditional negation -- each rejected by the
    bigint pin or, where both answers are valid roots, by the bit-for-bit comparison"""
    P = dc.FIELDS[9].P
    good = {}

    def outputs(name):
        if name not in good:
            inp = dc.table2_inputs(name)
            good[name] = (inp, dc.run_host(name, inp))
            dc.check_table2(name, inp, good[name][1], dc_dec)
        return good[name][0], good[name][1].copy()
    for name in ("is_zero_9", "is_zero_14", "words_lt_8", "words_lt_12", "check_form_te", "check_form_377_mont", "in_subgroup_te", "in_subgroup_377"):
        for e in {"in_subgroup_te": (3, 7), "in_subgroup_377": (6, 9)}.get(name, (0, 3)):   # (a subgroup verdict is pinned on curve points only)
            inp, bad = outputs(name)
            bad[e, 0] = (int(bad[e, 0]) + 1) % (3 if name.startswith("check_form") else 2)
            with pytest.raises(AssertionError, match=r"%s: element %d: " % (name, e)):
                dc.check_table2(name, inp, bad, dc_dec)
            with pytest.raises(AssertionError, match=r"%s: element %d word 0" % (name, e)):
                dc.compare_bits(name, bad, good[name][1], inp)
    # the other root: as good a root for the bigint pin -- only the comparison with the host build's words notices
    for name, N in (("sqrt_ratio_9", 9), ("sqrt_14", 14)):
        inp, bad = outputs(name)
        F = dc.FIELDS[N]
        e = 5
        assert dc.unmont(N, bad[e, 1:]) != 0
        bad[e, 1:] = F.limbs(F.P - F.val(bad[e, 1:]) % F.P)
        dc.check_table2(name, inp, bad, dc_dec)
        with pytest.raises(AssertionError, match=r"%s: element %d word 1" % (name, e)):
            dc.compare_bits(name, bad, good[name][1], inp)
        bad = good[name][1].copy()                                          # the flag of a non-square
        e = next(i for i in range(len(bad)) if bad[i, 0] == 0)
        bad[e, 0] = 1
        with pytest.raises(AssertionError, match=r"%s: element %d: flag 1" % (name, e)):
            dc.check_table2(name, inp, bad, dc_dec)
    # fe_to_canon without its conditional subtraction: value + modulus wherever the input was the larger representative
    for name, N, nw in (("to_canon_9", 9, 8), ("to_canon_14", 14, 12)):
        inp, bad = outputs(name)
        F = dc.FIELDS[N]
        e = next(i for i in range(len(inp)) if F.val(inp[i]) * F.rinv % F.P + F.P < 1 << (32 * nw))
        v = sum(int(x) << (32 * i) for i, x in enumerate(bad[e])) + F.P
        bad[e] = dc.words32(v, nw)
        with pytest.raises(AssertionError, match=r"%s: element %d: .*it is that \+ the modulus" % (name, e)):
            dc.check_table2(name, inp, bad, dc_dec)
    inp, bad = outputs("sm_digits")
    bad[7, 9 + 64] = np.uint32((int(bad[7, 9 + 64]) + 1) & 0xFFFFFFFF)
    with pytest.raises(AssertionError, match=r"sm_digits: element 7: "):
        dc.check_table2("sm_digits", inp, bad, dc_dec)
    inp, bad = outputs("aff_group_377")
    cases = dc.aff_cases(1)
    e = next(i for i, (slots, cnt) in enumerate(cases) if cnt == 8 and dc.sw_pool().pts[slots[0]] is None and dc.sw_pool().pts[slots[1]] is not None)
    bad[e, :24] = bad[e, 24:48]
    with pytest.raises(AssertionError, match=r"aff_group_377: element %d: cnt = 8, slot 0 \(infinity\)" % e):
        dc.check_table2("aff_group_377", inp, bad, dc_dec)
    inp, bad = outputs("sw_cneg")
    e = next(i for i in range(len(inp)) if inp[i, 42] == 1 and dc.sw_pool().pts[i // 4] is not None)
    bad[e] = inp[e, :42]
    with pytest.raises(AssertionError, match=r"sw_cneg: element %d: " % e):
        dc.check_table2("sw_cneg", inp, bad, dc_dec)
    inp, bad = outputs("add_cneg")
    bad[[2, 3]] = bad[[3, 2]]                                               # O + P and O - P exchanged: the sign ignored
    with pytest.raises(AssertionError, match=r"add_cneg: element [23]: "):
        dc.check_table2("add_cneg", inp, bad, dc_dec)
