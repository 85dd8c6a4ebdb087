"""The expected values tests/test_gpu_piece_loops.py compares the GPU with, checked here against the models the rest of the suite trusts, at
sizes a model reaches: the tiled inversion table against fc.model_op, the NTT closed forms against nc.model, and the parser that reads the
piece constants out of points.hip.  A wrong reference fails here, not on the GPU."""
import pytest

import field_cases as fc
import ntt_cases as nc

P = nc.P


# ---- the piece constants ------------------------------------------------------------------------------------------------------------
def test_piece_constants_are_found():
    assert fc.piece_constant("kFieldInvPiece") == 1 << 20
    assert fc.piece_constant("kCheckPiece") == 1 << 18
    assert fc.piece_constant("kMulPiece") == 1 << 18
    with pytest.raises(AssertionError):
        fc.piece_constant("kNoSuchPiece")


# ---- the tiled inversion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, fc.MONTGOMERY])
@pytest.mark.parametrize("field", fc.FIELDS)
def test_tile_inverses_match_the_model(field, flags):
    p, eb = fc.modulus(field), fc.nbytes(field)
    for zeros in (True, False):
        vals = fc.tile_set(field, zeros)
        assert len(vals) == fc.TILE and all(0 <= x < 1 << (8 * eb) for x in vals)
        residues = {x % p for x in vals}
        assert (0 in residues) == zeros
        if zeros:
            assert {0, p, 2 * p} <= set(vals) and set(fc.extremes(field)) <= set(vals)
        want = fc.model_op(field, fc.INV, fc.pack(vals, eb), None, flags | (fc.ZERO_OK if zeros else 0))
        assert want[0] == 0 and fc.pack(fc.tile_inverses(field, flags, zeros), eb) == want[1]
    # the tiling: element i is entry i mod TILE on both sides, across more than two periods
    n = 2 * fc.TILE + 5
    a = fc.tiled([x.to_bytes(eb, "little") for x in fc.tile_set(field)], n)
    out = fc.tiled([x.to_bytes(eb, "little") for x in fc.tile_inverses(field, flags)], n)
    assert len(a) == n * eb and fc.model_op(field, fc.INV, a, None, flags | fc.ZERO_OK)[:2] == (0, out)


def test_strict_tile_set_fails_where_a_zero_is_planted():
    eb, p = 32, fc.modulus(fc.FIELD_P)
    v = list(fc.tile_set(fc.FIELD_P, zeros=False))
    v[77], v[11] = p, 0
    assert fc.model_op(fc.FIELD_P, fc.INV, fc.pack(v, eb))[::2] == (fc.EFIELD, 11)


# ---- the NTT closed forms --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    return nc.shim()


@pytest.mark.parametrize("log_n", [0, 6, 10])
def test_constant_and_delta0(log_n):
    n = 1 << log_n
    for c in (1, 2, 16387):
        assert nc.pack(nc.const_forward(log_n, c), 32) == nc.model(nc.pack([c] * n, 32), log_n)
        assert nc.pack([nc.delta0_inverse(log_n, c)] * n, 32) == nc.model(nc.pack([c] + [0] * (n - 1), 32), log_n, flags=nc.INVERSE)


@pytest.mark.parametrize("flags,shift", [(0, None), (nc.MONTGOMERY, 22), (0, 22), (nc.MONTGOMERY, None)])
@pytest.mark.parametrize("log_n", [6, 9])
def test_deltas_and_three_terms(log_n, flags, shift):
    n = 1 << log_n
    places = [nc.delta_place(log_n, t) for t in range(5)]
    assert len(set(places)) == 5 and all(0 <= k < n for k in places)
    for terms in ([(places[0], 1)], [(places[3], 1)], [(n - 1, 3), (n // 3, 5), (places[1], 7)]):
        a = nc.pack(nc.terms_input(log_n, terms, flags), 32)
        want = nc.model(a, log_n, 1, flags, shift)
        assert nc.pack([nc.terms_forward(log_n, terms, j, flags, shift) for j in range(n)], 32) == want
        assert nc.model(want, log_n, 1, flags | nc.INVERSE, shift) == a          # and the inverse call gives the input back


@pytest.mark.parametrize("log_n", [6, 10])
def test_geometric(log_n):
    n, g = 1 << log_n, 0x1234567 + log_n
    a = nc.geometric_input(log_n, g)
    assert a[:3] == [1, g, g * g % P] and len(a) == n
    assert nc.pack([nc.geometric_forward(log_n, g, j) for j in range(n)], 32) == nc.model(nc.pack(a, 32), log_n)


def test_plan_digits_and_places(L):
    assert nc.plan_digits([3, 2, 2], 0b1011001) == [0b101, 0b10, 0b01]
    for log_n, split in ((18, [6, 6, 6]), (19, [7, 6, 6]), (20, [7, 7, 6]), (21, [7, 7, 7]), (22, [8, 7, 7]), (23, [8, 8, 7])):
        r = nc.plan_info(L, log_n)["r"]
        assert r == split                                           # the unbalanced splits the GPU module is there for
        ks = nc.distinct_digit_places(log_n, r)
        assert len(set(ks)) == 3
        for k in ks:
            d = nc.plan_digits(r, k)
            assert all(d) and len(set(d)) == 3 and sum(x << s for x, s in zip(d, (r[1] + r[2], r[2], 0))) == k


def test_sample_places_hold_the_corners(L):
    for log_n in (3, 11, 17):
        js = nc.sample_places(L, log_n, 1)
        n = 1 << log_n
        assert set(nc.tile_corners(L, log_n)) <= set(js) and {0, n // 2, n - 1} <= set(js) and js == sorted(set(js)) and js[-1] < n
        assert len(js) >= min(n, 3900)                              # 4096 draws from 2^17 places: fewer than 200 can coincide
