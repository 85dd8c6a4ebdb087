"""The hand-written piece loops of points.hip, each run through more than one piece on the GPU: field inversion (field_on, pieces of
kFieldInvPiece elements over one slab), the NTT (ntt_on, pieces of the plan's piece_transforms over one tmp) and point checks over host
buffers (check_points_on, pieces of kCheckPiece points through one staging buffer).  Every piece is told apart from the others, so a loop
that skipped, repeated or misplaced a piece, or reported a piece's index without its offset, fails here.  Also: the NTT sizes 2^18 .. 2^23,
whose three passes are unbalanced, against the textbook transform and closed forms.

Every comparison is byte-exact.  Expected values are Python integers (tests/field_cases.py, tests/ntt_cases.py: pinned to the models by
tests/test_piece_cases_host.py), the textbook transform of the host shim, or closed forms -- never another kernel of the library.  The
piece sizes are read from points.hip and from the plan, and every test asserts that it really crosses one."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import field_cases as fc
import layout_cases as lc
import ntt_cases as nc
from test_point_checks_host import bls_bad_classes, te_bad_classes

pytestmark = pytest.mark.gpu

PAT = 0xAB
P = nc.P
EPOINT = -5
INV_PIECE = fc.piece_constant("kFieldInvPiece")
CHECK_PIECE = fc.piece_constant("kCheckPiece")
FORMS = [0, fc.MONTGOMERY]


@pytest.fixture(scope="module")
def L():
    return nc.shim()


@pytest.fixture(scope="module")
def one(pkg):
    with pkg.MsmContext((0,)) as c:
        yield c


def _sync():
    import torch
    torch.cuda.synchronize()


# =================================================================================================================================================
# A. field inversion across pieces
# =================================================================================================================================================
@pytest.fixture
def inv_group():
    """the chain length of the calls that follow (TE_MSM_FIELD_INV_GROUP, read by every call), put back afterwards"""
    keep = os.environ.get("TE_MSM_FIELD_INV_GROUP")

    def choose(g):
        os.environ["TE_MSM_FIELD_INV_GROUP"] = str(g)
    yield choose
    if keep is None:
        os.environ.pop("TE_MSM_FIELD_INV_GROUP", None)
    else:
        os.environ["TE_MSM_FIELD_INV_GROUP"] = keep


def _table(vals, eb):
    """TILE records of eb bytes on the device"""
    import torch
    return torch.frombuffer(bytearray(fc.pack(vals, eb)), dtype=torch.uint8).reshape(fc.TILE, eb).cuda()


def _tile(table, n):
    """v[i] = table[i mod TILE]: n records"""
    import torch
    return table.index_select(0, torch.arange(n, device="cuda") % fc.TILE)


def _inv(c, field, a, n, flags, out):
    _sync()
    return c._L.te_msm_field_op_device(c._h, field, fc.INV, a.data_ptr(), None, n, flags, out.data_ptr())


def _inversion_in_pieces(c, field, flags):
    """ZERO_OK: both sizes, out of place into a pattern and in place, compared in full with the tiled table of Python inverses"""
    import torch
    eb = fc.nbytes(field)
    tin, tout = _table(fc.tile_set(field), eb), _table(fc.tile_inverses(field, flags), eb)
    for n in (INV_PIECE + 1, 2 * INV_PIECE + 300):                  # a second piece of one element; three pieces, the last a partial tile
        assert n > INV_PIECE
        a, want = _tile(tin, n), _tile(tout, n)
        out = torch.full_like(a, PAT)
        assert _inv(c, field, a, n, flags | fc.ZERO_OK, out) == 0
        assert torch.equal(out, want), n
        assert torch.equal(a, _tile(tin, n)), n                    # the input is as it was
        assert _inv(c, field, a, n, flags | fc.ZERO_OK, a) == 0
        assert torch.equal(a, want), n
        del a, want, out


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_inversion_across_pieces(pkg, field, flags):
    with pkg.MsmContext((0,)) as c:
        _inversion_in_pieces(c, field, flags)


@pytest.mark.parametrize("group", [8, 64])
def test_inversion_across_pieces_other_chain_lengths(pkg, inv_group, group):
    inv_group(group)
    with pkg.MsmContext((0,)) as c:
        _inversion_in_pieces(c, fc.FIELD_P, 0)


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_strict_inversion_reports_the_lowest_zero_across_pieces(pkg, field, flags):
    import torch
    eb, p, n = fc.nbytes(field), fc.modulus(field), 2 * INV_PIECE + 300
    assert n > 2 * INV_PIECE
    tin, tout = _table(fc.tile_set(field, zeros=False), eb), _table(fc.tile_inverses(field, flags, zeros=False), eb)
    zero_records = [torch.frombuffer(bytearray(z.to_bytes(eb, "little")), dtype=torch.uint8).cuda() for z in (0, p, 2 * p)]
    with pkg.MsmContext((0,)) as c:
        a, want = _tile(tin, n), _tile(tout, n)
        out = torch.full_like(a, PAT)
        assert _inv(c, field, a, n, flags, out) == 0 and torch.equal(out, want)
        for k, where in enumerate(((INV_PIECE + 7,), (INV_PIECE - 1, INV_PIECE), (n - 1, INV_PIECE + 900))):
            bad = a.clone()
            for j, at in enumerate(where):
                bad[at] = zero_records[(k + j) % 3]
            out.fill_(PAT)
            assert _inv(c, field, bad, n, flags, out) == fc.EFIELD, where
            assert (c.get_option("bad_field_index"), c.get_option("bad_field_reason")) == (min(where), fc.ZERO), where
            assert bool((out == PAT).all()), where                  # nothing was written
            assert _inv(c, field, a, n, flags, out) == 0 and torch.equal(out, want), where      # the next call succeeds


def test_host_form_inversion_on_two_slices_of_two_pieces(pkg):
    field, eb, n = fc.FIELD_P, 32, 2 * INV_PIECE + 3
    assert n // 2 > INV_PIECE                                       # both slices run a second piece
    idx = np.arange(n) % fc.TILE
    a = np.frombuffer(fc.pack(fc.tile_set(field), eb), dtype=np.uint8).reshape(fc.TILE, eb)[idx]
    want = np.frombuffer(fc.pack(fc.tile_inverses(field, 0), eb), dtype=np.uint8).reshape(fc.TILE, eb)[idx]
    out = np.full_like(a, PAT)
    with pkg.MsmContext((0, 0)) as c:
        assert c._L.te_msm_field_op(c._h, field, fc.INV, a.ctypes.data, None, n, fc.ZERO_OK, out.ctypes.data) == 0
    assert np.array_equal(out, want)


# =================================================================================================================================================
# B. NTT batches across pieces
# =================================================================================================================================================
def _words(ints):
    """wire integers -> (len, 4) little-endian words of 64 bits on the device"""
    import torch
    return torch.from_numpy(np.frombuffer(nc.pack(ints, 32), dtype="<i8").reshape(-1, 4).copy()).cuda()


def _ntt(c, a, log_n, count, flags, shift, out):
    _sync()
    rec = None if shift is None else int(shift).to_bytes(32, "little")
    assert c._L.te_msm_ntt_device(c._h, a.data_ptr(), log_n, count, flags, rec, out.data_ptr()) == 0


def _pieces(L, log_n, count):
    """the plan's piece, and the first and the last transform of every piece of a batch that needs more than one"""
    piece = nc.plan_info(L, log_n)["piece"]
    assert piece == max(1, (1 << 24) >> log_n) and count > piece
    ends = set()
    for off in range(0, count, piece):
        ends |= {off, min(off + piece, count) - 1}
    return piece, sorted(ends)


def test_size_one_across_pieces(one, L):
    """2^24 + 5 transforms of one element: every direction and form is the identity on values below 2^252"""
    import torch
    count = (1 << 24) + 5
    piece, ends = _pieces(L, 0, count)
    assert ends == [0, piece - 1, piece, count - 1]
    g = torch.Generator(device="cuda")
    g.manual_seed(24)
    a = torch.randint(-(1 << 31), 1 << 31, (count, 4), dtype=torch.int64, device="cuda", generator=g)
    a <<= 32
    a |= torch.randint(0, 1 << 32, (count, 4), dtype=torch.int64, device="cuda", generator=g)      # every bit of the 64 is random
    a[:, 3] &= (1 << 60) - 1                                        # below 2^252: canonical for this p
    a[0], a[piece - 1], a[piece], a[count - 1] = _words([0, P - 1, (1 << 252) - 1, 1])
    out = torch.empty_like(a)
    for flags in (0, nc.INVERSE, nc.MONTGOMERY):
        out.fill_(-1)
        _ntt(one, a, 0, count, flags, None, out)
        assert torch.equal(out, a), flags


@pytest.mark.parametrize("log_n,count,passes", [(10, (1 << 14) + 3, 1), (11, (1 << 13) + 3, 2), (17, 131, 3)])
def test_constant_batches_across_pieces(one, L, log_n, count, passes):
    """transform t holds its own constant c_t = t + 1: all-c_t -> n c_t delta_0 -> (in place) all-c_t, and c_t delta_0 -> (inverse)
    c_t / n at every place -> (in place) c_t delta_0, each compared in full"""
    import torch
    n = 1 << log_n
    piece, _ = _pieces(L, log_n, count)
    assert nc.plan_info(L, log_n)["passes"] == passes and count % piece == 3
    cs = torch.arange(1, count + 1, dtype=torch.int64, device="cuda")
    x = torch.zeros((count, n, 4), dtype=torch.int64, device="cuda")
    y = torch.full((count, n, 4), -1, dtype=torch.int64, device="cuda")
    x[:, :, 0] = cs[:, None]
    _ntt(one, x, log_n, count, 0, None, y)
    x.zero_()
    x[:, 0, 0] = n * cs                                            # (= nc.const_forward, below 2^40: no reduction)
    assert nc.const_forward(log_n, count)[0] == n * count
    assert torch.equal(y, x)
    _ntt(one, y, log_n, count, nc.INVERSE, None, y)
    x.zero_()
    x[:, :, 0] = cs[:, None]
    assert torch.equal(y, x)
    x.zero_()
    x[:, 0, 0] = cs
    y.fill_(-1)
    _ntt(one, x, log_n, count, nc.INVERSE, None, y)
    each = _words([nc.delta0_inverse(log_n, t + 1) for t in range(count)])
    assert bool((y == each[:, None, :]).all())                      # one integer per transform, at every place
    _ntt(one, y, log_n, count, 0, None, y)
    assert torch.equal(y, x)


@pytest.mark.parametrize("log_n,count,flags,shift", [(11, (1 << 13) + 3, 0, None), (17, 131, nc.MONTGOMERY, 22)])
def test_delta_batches_across_pieces(one, L, log_n, count, flags, shift):
    """transform t is delta at k_t: output j is s^(k_t) w^(j k_t), sampled at the first and last transform of every piece, the tile corners
    and random pairs; the inverse call, in place, gives the deltas back in full"""
    import torch
    n = 1 << log_n
    piece, ends = _pieces(L, log_n, count)
    ts = torch.arange(count, dtype=torch.int64, device="cuda")
    at = ts * n + (2654435761 * (ts + 1)) % n
    assert int(at[count - 1]) == (count - 1) * n + nc.delta_place(log_n, count - 1)
    a = torch.zeros((count * n, 4), dtype=torch.int64, device="cuda")
    a[at] = _words(nc.encode([1], flags))
    y = torch.full_like(a, -1)
    _ntt(one, a, log_n, count, flags, shift, y)
    rnd = random.Random(log_n)
    corners = set(nc.tile_corners(L, log_n)) | {0, 1, n // 2, n - 1}
    pairs = {(t, j) for t in ends for j in corners} | {(rnd.randrange(count), rnd.choice(sorted(corners))) for _ in range(512)}
    while len(pairs) < 4096:
        pairs.add((rnd.randrange(count), rnd.randrange(n)))
    pairs = sorted(pairs)
    got = y[torch.tensor([t * n + j for t, j in pairs], device="cuda")].cpu().numpy().tobytes()
    assert got == nc.pack([nc.terms_forward(log_n, [(nc.delta_place(log_n, t), 1)], j, flags, shift) for t, j in pairs], 32)
    _ntt(one, y, log_n, count, flags | nc.INVERSE, shift, y)
    assert torch.equal(y, a)


# =================================================================================================================================================
# C. the sizes 2^18 .. 2^23: three passes of unequal digits, one transform each
# =================================================================================================================================================
@functools.lru_cache(maxsize=None)
def _values(log_n):
    return nc.values(1 << log_n, seed=log_n)


@pytest.mark.parametrize("step", [0, 1])
@pytest.mark.parametrize("log_n", [18, 19])
def test_sizes_18_and_19_match_the_textbook(one, L, log_n, step):
    import torch
    assert nc.plan_info(L, log_n)["r"] == {18: [6, 6, 6], 19: [7, 6, 6]}[log_n]
    flags, shift = nc.FLAGS[(log_n + step) % 4], nc.SHIFTS[(log_n + 2 * step) % 3]
    a = _values(log_n)
    want = nc.ref(L, a, log_n, 1, flags, shift)
    da = torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda()
    out = da if step else torch.full_like(da, PAT)                  # one combination in place, one out of place
    _ntt(one, da, log_n, 1, flags, shift, out)
    assert bytes(out.cpu().numpy()) == want


def _sampled(y, js):
    import torch
    return y[torch.tensor(js, device="cuda")].cpu().numpy().tobytes()


@pytest.mark.parametrize("log_n", [20, 21])
def test_sizes_20_and_21_geometric_sequence(one, L, log_n):
    """a_i = g^i -> (g^n - 1) / (g w^j - 1) at the sampled j; the inverse, in place, returns the input in full"""
    import torch
    assert nc.plan_info(L, log_n)["r"] == {20: [7, 7, 6], 21: [7, 7, 7]}[log_n]
    g = random.Random(log_n).randrange(2, P)
    a = _words(nc.geometric_input(log_n, g))
    y = torch.full_like(a, -1)
    _ntt(one, a, log_n, 1, 0, None, y)
    js = nc.sample_places(L, log_n, log_n)
    assert 4000 <= len(js) <= 4300
    assert _sampled(y, js) == nc.pack([nc.geometric_forward(log_n, g, j) for j in js], 32)
    _ntt(one, y, log_n, 1, nc.INVERSE, None, y)
    assert torch.equal(y, a)


@pytest.mark.parametrize("log_n,flags,shift", [(22, 0, 22), (23, nc.MONTGOMERY, None)])
def test_sizes_22_and_23_three_deltas(one, L, log_n, flags, shift):
    """three deltas with distinct coefficients at places whose plan digits are all non-zero and pairwise different"""
    import torch
    r = nc.plan_info(L, log_n)["r"]
    assert r == {22: [8, 7, 7], 23: [8, 8, 7]}[log_n]
    ks = nc.distinct_digit_places(log_n, r)
    terms = list(zip(ks, (1, P - 2, random.Random(log_n).randrange(P))))
    a = torch.zeros((1 << log_n, 4), dtype=torch.int64, device="cuda")
    a[torch.tensor(ks, device="cuda")] = _words(nc.encode([c for _, c in terms], flags))
    y = torch.full_like(a, -1)
    _ntt(one, a, log_n, 1, flags, shift, y)
    js = nc.sample_places(L, log_n, log_n)
    assert _sampled(y, js) == nc.pack([nc.terms_forward(log_n, terms, j, flags, shift) for j in js], 32)
    _ntt(one, y, log_n, 1, flags | nc.INVERSE, shift, y)
    assert torch.equal(y, a)


# =================================================================================================================================================
# D. point checks over host buffers in pieces
# =================================================================================================================================================
N_PTS = CHECK_PIECE + 3000
PB = {0: 64, 1: 96}


def _bad_points(curve):
    """one point of every reason: non-canonical (1), off the curve (2), outside the subgroup (3)"""
    classes = {name: (pt, reason) for name, pt, reason in (bls_bad_classes() if curve == 1 else te_bad_classes())}
    picks = (classes["x+q" if curve == 1 else "x+p"], classes["y+1"], classes["P+T2"])
    assert [reason for _, reason in picks] == [1, 2, 3]
    return picks


def _placements(r1, r2, r3):
    """[(index, point, reason), ..] per case, and what level 2 must report for it"""
    pc, n = CHECK_PIECE, N_PTS
    return [
        ([(pc + 900, r1), (pc + 7, r2), (n - 1, r3)], (pc + 7, 2)),                             # the second piece only
        ([(pc + 2, r1), (pc - 1, r2), (17 + pc // 2, r3), (n - 5, r1)], (17 + pc // 2, 3)),      # across pieces, the lowest in the first
        ([(pc - 1, r2), (pc, r1), (n - 1, r3)], (pc - 1, 2)),                                    # across the boundary
        ([(pc, r1), (n - 1, r2)], (pc, 1)),                                                     # the first point of the second piece
        ([(pc + 7, r3)], (pc + 7, 3)),                                                          # the subgroup alone: level 1 lets it pass
    ]


def _verdict(placed, level):
    """the lowest index among the points the level rejects, with its reason"""
    seen = [(at, reason) for at, (_, reason) in placed if reason < 3 or level == 2]
    return min(seen) if seen else None


def _with(buf, rec, placed, width):
    a = bytearray(buf)
    for at, (pt, _) in placed:
        assert 0 <= at < len(buf) // rec and len(pt) == width
        a[rec * at:rec * at + width] = pt
    return bytes(a)


@pytest.mark.parametrize("curve", [0, 1])
def test_host_point_checks_report_across_pieces(pkg, curve):
    """check_points, run and bind_points over a host buffer of more than one piece: the lowest bad index and its reason at both levels,
    the result buffer untouched, no handle, and the context usable afterwards; check_points_device (one launch) as the control"""
    import torch
    n, pb = N_PTS, PB[curve]
    assert n > CHECK_PIECE
    pts, sc = pkg.synth_inputs(0xD1CE + curve, n, curve=curve)
    lib = pkg.binding._lib()
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        want = c.run(pts, sc)                                       # unchecked
        assert c.check_points(pts, 1) is None and c.check_points(pts, 2) is None
        bound = c.get_option("bases_bound")
        for k, (placed, at_level_2) in enumerate(_placements(*_bad_points(curve))):
            bad = _with(pts, pb, placed, pb)
            assert _verdict(placed, 2) == at_level_2
            for level in (1, 2):
                v = _verdict(placed, level)
                assert c.check_points(bad, level) == v, (k, level)
                if level == 1 and v in (None, at_level_2):          # (run and bind at level 1 where its verdict is one of its own)
                    continue
                c.set_option("check_points", level)
                res = ctypes.create_string_buffer(b"\x5a" * 96, 96)
                assert lib.te_msm_run(c._h, bad, sc, n, res) == EPOINT, (k, level)
                assert res.raw == b"\x5a" * 96
                assert (c.get_option("bad_point_index"), c.get_option("bad_point_reason")) == v, (k, level)
                h = ctypes.c_void_p(1234)
                assert lib.te_msm_bind_points(c._h, bad, n, ctypes.byref(h)) == EPOINT and not h.value, (k, level)
                assert (c.get_option("bad_point_index"), c.get_option("bad_point_reason")) == v, (k, level)
                assert c.get_option("bases_bound") == bound
                assert c.run(pts, sc) == want, (k, level)           # the next clean run, checked, equals the unchecked result
                c.set_option("check_points", 0)
            if k == 0:
                dbad = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
                _sync()
                assert c.check_points_device(dbad.data_ptr(), n, 2) == at_level_2
                del dbad
        c.set_option("check_points", 2)
        c.release_points(c.bind_points(pts))                        # a clean set binds under the check


@functools.lru_cache(maxsize=None)
def _bls_points(pkg_name):
    """N_PTS valid BLS12-377 points, canonical and as Montgomery residues"""
    import importlib
    pts, _ = importlib.import_module(pkg_name).synth_inputs(0xD1CE + 1, N_PTS, scalars=False, curve=1)
    return pts, lc.to_montgomery_points(pts, 1)


@pytest.mark.parametrize("mont,stride,flag", [(1, 104, 1), (1, 0, 0), (0, 104, 1)])
def test_bls377_record_layouts_report_across_pieces(pkg, mont, stride, flag):
    """the same for a native prover's records (options "points_montgomery", "point_stride", "point_infinity_flag": te_msm_check_points
    and te_msm_bind_points read them): the piece offset in bytes follows the stride, and a flagged infinity record at the first place of
    the second piece passes"""
    n, rec = N_PTS, stride or 96
    canonical, residues = _bls_points(pkg.__name__)
    img = np.frombuffer(lc.at_stride(residues if mont else canonical, 96, rec), dtype=np.uint8).reshape(n, rec).copy()
    if flag:
        img[:, 96] = 0
        img[CHECK_PIECE, :96] = 0xFF                                # under the flag the coordinates are not read
        img[CHECK_PIECE, 96] = 1
    img = img.tobytes()
    r1, r2, r3 = _bad_points(1)
    if mont:                                                        # the same classes as stored residues
        good_x = int.from_bytes(residues[:48], "little")
        r1 = ((good_x + lc.Q_377).to_bytes(48, "little") + residues[48:96], 1)
        r2, r3 = (lc.to_montgomery_points(r2[0], 1), 2), (lc.to_montgomery_points(r3[0], 1), 3)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", 1)
        c.set_option("points_montgomery", mont)
        c.set_option("point_stride", stride)
        c.set_option("point_infinity_flag", flag)
        assert c.check_points(img, 1) is None and c.check_points(img, 2) is None
        bound = c.get_option("bases_bound")
        for k, (placed, at_level_2) in enumerate(_placements(r1, r2, r3)):
            if flag:                                                # keep the flagged record: a bad point beside it, not on it
                placed = [(at + 1 if at == CHECK_PIECE else at, pt) for at, pt in placed]
                at_level_2 = (at_level_2[0] + 1 if at_level_2[0] == CHECK_PIECE else at_level_2[0], at_level_2[1])
            bad = _with(img, rec, placed, 96)
            for level in (1, 2):
                v = _verdict(placed, level)
                assert level == 1 or v == at_level_2
                assert c.check_points(bad, level) == v, (k, level)
            c.set_option("check_points", 2)
            with pytest.raises(pkg.MsmError) as e:
                c.bind_points(bad)
            assert (e.value.code, e.value.index, e.value.reason) == (EPOINT,) + at_level_2, k
            assert c.get_option("bases_bound") == bound
            c.set_option("check_points", 0)
        if flag:                                                    # a flag byte that is neither 0 nor 1, in the second piece: non-canonical
            a = bytearray(img)
            a[rec * (CHECK_PIECE + 5) + 96] = 2
            assert c.check_points(bytes(a), 1) == (CHECK_PIECE + 5, pkg.POINT_NONCANONICAL)
        c.set_option("check_points", 2)
        c.release_points(c.bind_points(img))
