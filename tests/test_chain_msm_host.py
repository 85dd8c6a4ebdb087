"""oracle/chain_msm.py, the closed-form reference of the large-n GPU tests (tests/test_gpu_large_n.py): equal to the bit-exact
oracles on chain inputs, blocked uint64 sums equal to plain Python-int sums on adversarial scalars, and check_chain() rejects a
point buffer that is not a chain.  CPU only."""
import numpy as np
import pytest

from oracle import chain_msm as cm
from oracle import model, model377, oracle, oracle377

ORA = {0: oracle, 1: oracle377}
SB = {0: 32, 1: 48}


def _python_sums(sc: bytes, sb: int, L: int):
    s0 = s1 = 0
    for i in range(L):
        v = int.from_bytes(sc[sb * i:sb * (i + 1)], "little")
        s0 += v
        s1 += i * v
    return s0, s1


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 4097])
def test_chain_msm_equals_the_oracle(pkg, curve, n):
    """synth_inputs' chain points (the GPU fixtures' generator) and the oracle's own: every prefix against the bit-exact oracle"""
    pts, sc = pkg.synth_inputs(0xC4A1 + n, n, curve=curve)
    cm.check_chain(curve, pts, cm.sample_indices(n, 8))
    lens = sorted({0, 1, n // 2, max(0, n - 1), n} | ({2, 3, 1000, 4096} if n > 4096 else set()))
    got = cm.chain_msms(curve, pts, sc, lens)
    for L, g in zip(lens, got):
        want = ORA[curve].msm(pts[:len(pts) // n * L], sc[:SB[curve] * L], threads=4)
        assert g == want, (curve, n, L)
    assert cm.chain_msm(curve, pts, sc) == got[-1]
    # the oracle's generator builds the same kind of chain
    opts, osc = ORA[curve].gen_points(77 + n, n), ORA[curve].gen_scalars(78 + n, n)
    assert cm.chain_msm(curve, opts, osc) == ORA[curve].msm(opts, osc, threads=4)


def test_empty_prefix_is_the_identity(pkg):
    pts, sc = pkg.synth_inputs(5, 3)
    assert cm.chain_msm(0, pts, sc, 0) == model.le32(0) + model.le32(1)
    pts, sc = pkg.synth_inputs(5, 3, curve=1)
    assert cm.chain_msm(1, pts, sc, 0) == bytes(96)


def _adversarial(curve: int, kind: str, n: int) -> bytes:
    sb = SB[curve]
    if kind == "ones":                                   # every bit set: the largest limbs the sums can see
        return b"\xff" * (sb * n)
    if kind == "p-1":
        top = model.P - 1 if curve == 0 else model377.R_ORDER - 1
        return top.to_bytes(sb, "little") * n
    rng = np.random.default_rng(n)                       # witness-like: mostly 0, 1, 2, 3 and 2^64 - 1, a few full-width values
    vals = rng.choice([0, 1, 2, 3, (1 << 64) - 1, -1], size=n, p=[0.4, 0.25, 0.1, 0.1, 0.1, 0.05])
    full = model.P - 1 if curve == 0 else model377.R_ORDER - 1
    return b"".join((full - int(rng.integers(1 << 62)) if v == -1 else int(v)).to_bytes(sb, "little") for v in vals)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("kind", ["ones", "p-1", "witness"])
def test_blocked_sums_equal_python_sums(curve, kind, monkeypatch):
    """a small BLOCK (many blocks, segments cut at block edges and at the requested lengths) and the real one at BLOCK + 5
    entries (the uint64 bound of the module at its worst case: every limb 0xffff)"""
    sb = SB[curve]
    n = 5003
    sc = _adversarial(curve, kind, n)
    lens = [n, 0, 1, 999, 1000, 1001, 2048, 4999, n]
    want = {L: _python_sums(sc, sb, L) for L in set(lens)}
    monkeypatch.setattr(cm, "BLOCK", 1000)
    assert cm.scalar_sums(curve, sc, lens) == want
    monkeypatch.setattr(cm, "BLOCK", 7)
    assert cm.scalar_sums(curve, sc, lens) == want
    monkeypatch.undo()
    big = cm.BLOCK + 5
    sc = _adversarial(curve, kind, big)
    lens = [big, cm.BLOCK, cm.BLOCK + 1, 3]
    if kind == "ones":                                   # closed forms: v = 2^(8 sb) - 1 everywhere
        v = (1 << (8 * sb)) - 1
        want = {L: (v * L, v * L * (L - 1) // 2) for L in lens}
    else:
        want = {L: _python_sums(sc, sb, L) for L in lens}
    assert cm.scalar_sums(curve, sc, lens) == want


@pytest.mark.parametrize("curve", [0, 1])
def test_check_chain_rejects_a_replaced_point(pkg, curve):
    n = 40
    pts, _ = pkg.synth_inputs(11, n, curve=curve)
    idx = cm.sample_indices(n, 12)
    assert n - 1 in idx and 0 in idx
    cm.check_chain(curve, pts, idx)
    pb = len(pts) // n
    other, _ = pkg.synth_inputs(12, n, curve=curve)          # a point of another chain
    for i in (n - 1, idx[len(idx) // 2]):
        bad = bytearray(pts)
        bad[pb * i:pb * (i + 1)] = other[pb * 3:pb * 4]
        with pytest.raises(AssertionError, match=f"point {i} "):
            cm.check_chain(curve, bytes(bad), idx)
