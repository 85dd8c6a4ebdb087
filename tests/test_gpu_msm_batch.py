"""GPU parity of BATCHED MSMs over prefixes of a bound point set (include/te_msm.h: te_msm_run_scalars_batch[_device]): every result is
compared bit for bit with the oracle over the prefix, the reference's own answers (the WASM goldens), or the existing paths (zero-padded
te_msm_run_scalars, te_msm_run on the point prefix).  Every test calls the new entry points.
One-GPU box: contexts of several "devices" name GPU 0 several times (every device holds its own copy of the records)."""
import ctypes
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle, oracle377
from oracle.gen_golden import make_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {0: (64, 32, 64), 1: (96, 48, 96)}          # point, scalar record, result bytes
ORA = {0: oracle, 1: oracle377}


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def identity(curve):
    return bytes(32) + (1).to_bytes(32, "little") if curve == 0 else bytes(96)


def scalars_for(curve, seed, n):
    return ORA[curve].gen_scalars(seed, n) if n else b""


def expect(curve, pts, sc, n):
    """the oracle's MSM over the first n points"""
    if n == 0:
        return identity(curve)
    pb, sb, _ = SIZES[curve]
    return ORA[curve].msm(pts[:pb * n], sc[:sb * n], threads=16)


def ragged_lens(n, seed, extra):
    r = random.Random(seed)
    base = [0, 1, 2, 3, 7, 8, 9, 255, 256, 257, n - 1, n, 3, 257, 0, n]
    return base + [r.randint(1, n) for _ in range(extra)] + [r.randint(1, 600) for _ in range(extra)]


def raw_batch(c, b, lens, scalars, out_len, device=False, lens_ptr=True, out_ptr=True):
    """the C call itself; returns (rc, out bytes) -- out is pre-filled with 0xAB to show what the call touched"""
    count = len(lens)
    lv = (ctypes.c_uint64 * max(1, count))(*lens)
    out = ctypes.create_string_buffer(b"\xab" * out_len, out_len)
    fn = c._L.te_msm_run_scalars_batch_device if device else c._L.te_msm_run_scalars_batch
    rc = fn(c._h, b._h if b is not None else None, count, lv if lens_ptr else None, scalars, out if out_ptr else None)
    return rc, out.raw


# ---- 1. both curves, ragged lengths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,logn", [(0, 16), (1, 14)])
def test_ragged_lengths_equal_the_oracle_over_the_prefix(pkg, curve, logn):
    n = 1 << logn
    pts = ORA[curve].gen_points(31 + curve, n)
    lens = ragged_lens(n, 5 + curve, 6)
    scs = [scalars_for(curve, 1000 + m, L) for m, L in enumerate(lens)]
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        b = c.bind_points(pts)
        got = c.run_scalars_batch(b, scs)
        seqs = c.get_option("batch_sequences")
        assert 1 <= seqs < len(lens)
        ds = _dev(b"".join(scs))
        _sync()
        got_dev = c.run_scalars_batch_device(b, ds.data_ptr(), lens)
        c.release_points(b)
    assert len(got) == len(lens)
    for m, L in enumerate(lens):
        assert got[m] == expect(curve, pts, scs[m], L), (m, L)
    assert got_dev == got


# ---- 2. the reference's own answers --------------------------------------------------------------------------------------------------
def test_wasm_goldens_as_the_first_msm_of_a_batch(pkg, wasm_golden, model):
    with pkg.MsmContext((0,)) as c:
        for g in wasm_golden:
            n = g["n"]
            pts, sc = make_inputs(g["seed"], n, g["mode"])
            b = c.bind_points(pts)
            pre = sorted({1, min(n, 4097), n // 3 if n <= (1 << 16) else 1000, max(1, n - 1)})
            got = c.run_scalars_batch(b, [sc] + [sc[:32 * k] for k in pre] + [b""])
            c.release_points(b)
            assert model.xy_from_bytes(got[0]) == (int(g["x"]), int(g["y"])), g["name"]
            for k, r in zip(pre, got[1:]):
                assert r == expect(0, pts, sc, k), (g["name"], k)
            assert got[-1] == identity(0)


# ---- 3. agreement with the existing paths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_equal_to_zero_padded_run_scalars_and_to_run_on_the_prefix(pkg, curve):
    n = 5000
    pb, sb, _ = SIZES[curve]
    pts = ORA[curve].gen_points(8, n)
    lens = [100, n, 3000, 1, 4096, 2500]
    scs = [scalars_for(curve, 70 + m, L) for m, L in enumerate(lens)]
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        b = c.bind_points(pts)
        got = c.run_scalars_batch(b, scs)
        for m, L in enumerate(lens):
            assert got[m] == c.run_scalars(b, scs[m] + bytes(sb * (n - L))), m
            assert got[m] == c.run(pts[:pb * L], scs[m]), m
        c.release_points(b)


# ---- 4. shared sequences and whole-MSM sequences in one call --------------------------------------------------------------------------
def test_small_msms_share_sequences_beside_large_ones(pkg):
    n = 1 << 20
    pts = oracle.gen_points(4, n)
    r = random.Random(9)
    small = [r.randint(1 << 8, 1 << 12) for _ in range(300)]
    lens = small[:150] + [1 << 18] + small[150:] + [1 << 20]
    scs = [oracle.gen_scalars(500 + m, L) for m, L in enumerate(lens)]
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts)
        got = c.run_scalars_batch(b, scs)
        seqs = c.get_option("batch_sequences")
        classes = len({L.bit_length() for L in small})
        assert seqs <= -(-300 // pkg.BATCH_SEQ_MAX) + classes + 2, seqs
        for m in (150, 301):
            assert got[m] == c.run_scalars(b, scs[m] + bytes(32 * (n - lens[m]))), m
        c.release_points(b)
    for m, L in enumerate(lens):
        if L <= 4096:
            assert got[m] == expect(0, pts, scs[m], L), (m, L)


# ---- 5. options and skewed scalars ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_options_and_skewed_scalars(pkg, curve):
    n = 4096
    pb, sb, _ = SIZES[curve]
    pts = ORA[curve].gen_points(12, n)
    k = (0xDEADBEEF12345).to_bytes(sb, "little")
    rng = np.random.default_rng(3)
    witness = b"".join(int(v).to_bytes(sb, "little") for v in rng.choice([0, 1, 2, 3, (1 << 64) - 1], size=n - 7))
    lens = [n, n - 7, 1000, 33, 1, 2048]
    scs = [k * n, witness, scalars_for(curve, 1, 1000), scalars_for(curve, 2, 33), k, scalars_for(curve, 3, 2048)]
    want = [expect(curve, pts, s, L) for s, L in zip(scs, lens)]
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        b = c.bind_points(pts)
        for signed in (1, 0):
            for wb in (0, 7):
                for seg in (0, 4):
                    c.set_option("signed_digits", signed)
                    c.set_option("window_bits", wb)
                    c.set_option("segment_len", seg)
                    assert c.run_scalars_batch(b, scs) == want, (signed, wb, seg)
        c.set_option("signed_digits", 1)
        c.set_option("window_bits", 0)
        c.set_option("segment_len", 0)
        c.set_option("batch_small_max", 0)                  # every MSM alone: the same results
        assert c.run_scalars_batch(b, scs) == want
        assert c.get_option("batch_sequences") == len(lens)
        c.release_points(b)


# ---- 6. device form, host form, several devices ---------------------------------------------------------------------------------------
def test_one_two_and_four_devices_give_identical_bytes(pkg):
    n = 1 << 14
    pts = oracle.gen_points(41, n)
    lens = ragged_lens(n, 17, 10) + [n] * 3
    scs = [oracle.gen_scalars(900 + m, L) for m, L in enumerate(lens)]
    ds = _dev(b"".join(scs))
    _sync()
    outs = []
    for ids in ((0,), (0, 0), (0, 0, 0, 0)):
        with pkg.MsmContext(ids) as c:
            b = c.bind_points(pts)
            outs.append(c.run_scalars_batch_device(b, ds.data_ptr(), lens))
            outs.append(c.run_scalars_batch(b, scs))
            c.release_points(b)
    assert all(o == outs[0] for o in outs)
    for m in (0, 4, 11, len(lens) - 1):
        assert outs[0][m] == expect(0, pts, scs[m], lens[m]), m


# ---- 7. fixed-base sets -------------------------------------------------------------------------------------------------------------
def test_fixed_base_set_gives_the_same_bytes(pkg):
    n = 1 << 13
    pts = oracle.gen_points(55, n)
    lens = [n, 1, 4000, 17, n - 1]
    scs = [oracle.gen_scalars(60 + m, L) for m, L in enumerate(lens)]
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts)
        plain = c.run_scalars_batch(b, scs)
        c.release_points(b)
        c.set_option("bind_fixed_base", 16)
        bf = c.bind_points(pts)
        c.set_option("bind_fixed_base", 0)
        assert c.run_scalars_batch(bf, scs) == plain
        c.release_points(bf)
    assert plain[0] == expect(0, pts, scs[0], n)


# ---- 8. errors leave out untouched ---------------------------------------------------------------------------------------------------
def test_errors_return_their_code_and_leave_out_untouched(pkg):
    n = 3000
    pts = oracle.gen_points(2, n)
    untouched = lambda out: out == b"\xab" * len(out)
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts)
        sc = oracle.gen_scalars(3, n)
        rc, out = raw_batch(c, b, [10, n + 1], sc + sc, 128)
        assert rc == -1 and untouched(out)                                   # longer than the set
        rc, out = raw_batch(c, b, [10], sc, 64, lens_ptr=False)
        assert rc == -1 and untouched(out)                                   # null lens
        rc, out = raw_batch(c, b, [10], None, 64)
        assert rc == -1 and untouched(out)                                   # null scalars
        assert raw_batch(c, b, [10], sc, 64, out_ptr=False)[0] == -1         # null out
        rc, out = raw_batch(c, b, [], sc, 64)
        assert rc == 0 and untouched(out)                                    # count 0 does nothing
        rc, out = raw_batch(c, b, [0, 0], None, 128)
        assert rc == 0 and out == identity(0) * 2                            # only empty MSMs: no scalars needed
        assert c._L.te_msm_set_window_shard(c._h, 0, 2) == 0
        rc, out = raw_batch(c, b, [10], sc, 64)
        assert rc == -1 and untouched(out)                                   # window shard set
        assert c._L.te_msm_set_window_shard(c._h, 0, 1) == 0
        c.set_option("curve", 1)
        rc, out = raw_batch(c, b, [10], sc, 96)
        assert rc == -1 and untouched(out)                                   # the set is of the other curve
        c.set_option("curve", 0)
        # a scalar that trips the final carry in MSM 17 of 40: the whole call fails, out untouched
        lens = [50 + 3 * m for m in range(40)]
        scs = [oracle.gen_scalars(200 + m, L) for m, L in enumerate(lens)]
        scs[17] = scs[17][:32 * 20] + b"\xff" * 32 + scs[17][32 * 21:]
        packed = b"".join(scs)
        rc, out = raw_batch(c, b, lens, packed, 64 * 40)
        assert rc == -3 and untouched(out)
        ds = _dev(packed)
        _sync()
        rc, out = raw_batch(c, b, lens, ctypes.c_void_p(ds.data_ptr()), 64 * 40, device=True)
        assert rc == -3 and untouched(out)
        c.set_option("signed_digits", 0)                                     # unsigned digits accept any 256-bit scalar
        got = c.run_scalars_batch(b, scs)
        assert got[17] == c.run_scalars(b, scs[17] + bytes(32 * (n - lens[17])))   # (the oracle decomposes with signed digits only)
        c.set_option("signed_digits", 1)
        c.release_points(b)                                                  # the set can be released afterwards
        rc, out = raw_batch(c, b, [10], sc, 64)
        assert rc == -1 and untouched(out)                                   # released
        with pytest.raises(pkg.MsmError):
            c.run_scalars_batch(b, [sc[:320]])
    with pkg.MsmContext((0,)) as c2, pkg.MsmContext((0,)) as c3:
        b3 = c3.bind_points(pts)
        rc, out = raw_batch(c2, b3, [10], sc, 64)
        assert rc == -1 and untouched(out)                                   # a set of another context
        c3.release_points(b3)


# ---- 9. Node ----------------------------------------------------------------------------------------------------------------------------
def test_node_msm_batch(pkg, tmp_path):
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists("/usr/include/node/node_api.h") and not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        pytest.skip("no N-API addon and no node headers to build it")
    subprocess.check_call(["make", "-C", js, "-s"])
    n = 3000
    pts = oracle.gen_points(71, n)
    lens = [n, 1, 0, 1500, 64, n - 1]
    (tmp_path / "p.bin").write_bytes(pts)
    for m, L in enumerate(lens):
        (tmp_path / ("s%d.bin" % m)).write_bytes(oracle.gen_scalars(80 + m, L))
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
(async () => {
  const pts = fs.readFileSync(process.argv[2]);
  const scs = process.argv.slice(3).map((f) => fs.readFileSync(f));
  const out = {};
  try { m.msmBatch(scs); out.unbound = 'returned'; } catch (e) { out.unbound = String(e.message); }
  m.setBases(pts);
  const got = m.msmBatch(scs);
  out.got = got.map((r) => [r.x.toString(), r.y.toString()]);
  out.want = [];
  for (const s of scs) {
    const r = await m.compute_msm(Buffer.from(pts.subarray(0, 64 * (s.length / 32))), s, false);
    out.want.push([r.x.toString(), r.y.toString()]);
  }
  m.setBases(null);
  console.log(JSON.stringify(out));
})();
"""
    files = [str(tmp_path / "p.bin")] + [str(tmp_path / ("s%d.bin" % m)) for m in range(len(lens))]
    r = subprocess.run([node, "-e", script, js] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert "te_msm error" in out["unbound"], out["unbound"]
    assert out["got"] == out["want"]
    for m, L in enumerate(lens):
        e = expect(0, pts, oracle.gen_scalars(80 + m, L) if L else b"", L)
        assert out["got"][m] == [str(int.from_bytes(e[:32], "little")), str(int.from_bytes(e[32:], "little"))], m
