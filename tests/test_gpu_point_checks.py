"""Input-point validation on the GPU (option "check_points", te_msm_check_points*; include/te_msm.h): valid inputs give the
unchecked result bit for bit, every class of bad point (tests/test_point_checks_host.py builds them from the bigint models) is
reported with its lowest index and reason through every checked entry point, and the context stays usable afterwards.
The bad points are data the check must reject; the MSM kernels never run over them while checking is on."""
import json
import os
import shutil
import subprocess

import pytest

from oracle import model as m
from oracle import oracle, oracle377
from oracle.gen_golden import make_inputs
from test_point_checks_host import bls_bad_classes, te_bad_classes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


CURVES = {
    0: dict(pb=64, gen=lambda s, n: oracle.gen_points(s, n), sc=lambda s, n: oracle.gen_scalars(s, n),
            msm=lambda p, s: oracle.msm(p, s, threads=8), bad=te_bad_classes),
    1: dict(pb=96, gen=lambda s, n: oracle377.gen_points(s, n), sc=lambda s, n: oracle377.gen_scalars(s, n),
            msm=lambda p, s: oracle377.msm(p, s, threads=8), bad=bls_bad_classes),
}


def _ctx(pkg, curve, level, ids=(0,)):
    c = pkg.MsmContext(ids)
    c.set_option("curve", curve)
    c.set_option("check_points", level)
    return c


def _with(pts, pb, at, pt):
    a = bytearray(pts)
    a[pb * at:pb * at + pb] = pt
    return bytes(a)


def _expect(err, index, reason):
    assert err.value.code == -5, err.value
    assert (err.value.index, err.value.reason) == (index, reason), err.value


def test_options_and_defaults(pkg):
    with pkg.MsmContext((0,)) as c:
        assert c.get_option("check_points") == 0
        assert c.get_option("bad_point_index") == -1 and c.get_option("bad_point_reason") == 0
        for v in (1, 2, 0):
            c.set_option("check_points", v)
            assert c.get_option("check_points") == v
        for v in (-1, 3):
            with pytest.raises(pkg.MsmError) as e:
                c.set_option("check_points", v)
            assert e.value.code == -1
        pts = oracle.gen_points(1, 10)
        assert c.check_points(pts, 1) is None and c.check_points(pts, 2) is None
        with pytest.raises(pkg.MsmError):
            c.check_points(pts, 0)
    assert pkg.EPOINT == -5 and (pkg.POINT_NONCANONICAL, pkg.POINT_OFF_CURVE, pkg.POINT_NOT_IN_SUBGROUP) == (1, 2, 3)


def test_valid_goldens_unchanged_te(pkg, wasm_golden, model):
    """levels 1 and 2 give the level-0 result bit for bit (the WASM goldens; n = 2^20 at level 1, n <= 2^16 at level 2)"""
    c0, c1, c2 = (_ctx(pkg, 0, lv) for lv in (0, 1, 2))
    try:
        big_done = False
        for g in wasm_golden:
            if g["n"] > 65536 and (g["n"] != 1 << 20 or big_done):
                continue
            pts, sc = make_inputs(g["seed"], g["n"], g["mode"])
            want = c0.run(pts, sc)
            assert model.xy_from_bytes(want) == (int(g["x"]), int(g["y"])), g["name"]
            assert c1.run(pts, sc) == want, g["name"]
            assert c1.check_points(pts, 1) is None
            if g["n"] <= 65536:
                assert c2.run(pts, sc) == want, g["name"]
                dp, ds = _dev(pts), _dev(sc)
                _sync()
                assert c2.run_device(dp.data_ptr(), ds.data_ptr(), g["n"]) == want, g["name"]
                if g["n"] == 65536:
                    assert c2.check_points_device(dp.data_ptr(), g["n"], 2) is None
            else:
                big_done = True
        assert big_done
        assert c1.get_option("bad_point_index") == -1 and c2.get_option("bad_point_index") == -1
    finally:
        for c in (c0, c1, c2):
            c.close()


def test_valid_bls377_unchanged(pkg):
    n = 1 << 16
    pts, sc = oracle377.gen_points(3, n), oracle377.gen_scalars(3, n)
    with _ctx(pkg, 1, 0) as c0, _ctx(pkg, 1, 2) as c2:
        want = c0.run(pts[:96 * 4096], sc[:48 * 4096])
        assert want == oracle377.msm(pts[:96 * 4096], sc[:48 * 4096], threads=8)
        assert c2.run(pts[:96 * 4096], sc[:48 * 4096]) == want
        c2.set_option("check_points", 1)
        assert c2.run(pts, sc) == c0.run(pts, sc)
        dp = _dev(pts)
        _sync()
        assert c2.check_points_device(dp.data_ptr(), n, 2) is None
        assert c2.check_points(pts, 2) is None


@pytest.mark.parametrize("curve", [0, 1])
def test_every_bad_class_first_middle_last(pkg, curve):
    """run (host) at level 2, each class at the first, a middle and the last index; level 1 lets the subgroup-only classes pass"""
    C = CURVES[curve]
    pts, sc = C["gen"](5, N), C["sc"](5, N)
    want = C["msm"](pts, sc)
    classes = C["bad"]()
    with _ctx(pkg, curve, 2) as c:
        for name, pt, reason in classes:
            for at in (0, N // 2, N - 1):
                bad = _with(pts, C["pb"], at, pt)
                with pytest.raises(pkg.MsmError) as e:
                    c.run(bad, sc)
                _expect(e, at, reason)
                assert (c.get_option("bad_point_index"), c.get_option("bad_point_reason")) == (at, reason), name
                assert c.check_points(bad, 2) == (at, reason), name
                assert c.check_points(bad, 1) == ((at, reason) if reason < 3 else None), name
            c.set_option("check_points", 1)
            if reason < 3:
                with pytest.raises(pkg.MsmError) as e:
                    c.run(_with(pts, C["pb"], 7, pt), sc)
                _expect(e, 7, reason)
            c.set_option("check_points", 2)
            assert c.run(pts, sc) == want                          # the context stays usable
        # two bad points: the lower index wins, whatever the reasons
        bad2 = _with(_with(pts, C["pb"], 200, classes[0][1]), C["pb"], 11, classes[-1][1])
        with pytest.raises(pkg.MsmError) as e:
            c.run(bad2, sc)
        _expect(e, 11, classes[-1][2])


@pytest.mark.parametrize("curve", [0, 1])
def test_every_path(pkg, curve):
    """run_device, submit (among good tickets in flight), submit_async, submit_device, bind_points[_device], the stand-alone checks"""
    C = CURVES[curve]
    pts, sc = C["gen"](6, N), C["sc"](6, N)
    want = C["msm"](pts, sc)
    classes = C["bad"]()
    picks = [classes[0], classes[2], classes[-1]]                  # one of each reason (1, 2, 3)
    with _ctx(pkg, curve, 2) as c:
        for name, pt, reason in picks:
            at = 123
            bad = _with(pts, C["pb"], at, pt)
            dbad, dgood, ds = _dev(bad), _dev(pts), _dev(sc)
            _sync()
            with pytest.raises(pkg.MsmError) as e:
                c.run_device(dbad.data_ptr(), ds.data_ptr(), N)
            _expect(e, at, reason)
            assert c.check_points_device(dbad.data_ptr(), N, 2) == (at, reason)
            # host tickets: the bad one among good ones in flight; only its collect fails
            for submit in (c.submit, c.submit_async):
                ts = [submit(pts, sc), submit(bad, sc), submit(pts, sc)]
                assert c.collect(ts[0]) == want
                with pytest.raises(pkg.MsmError) as e:
                    c.collect(ts[1])
                _expect(e, at, reason)
                assert c.collect(ts[2]) == want
            ts = [c.submit_device(dgood.data_ptr(), ds.data_ptr(), N), c.submit_device(dbad.data_ptr(), ds.data_ptr(), N)]
            with pytest.raises(pkg.MsmError) as e:
                c.collect(ts[1])
            _expect(e, at, reason)
            assert c.collect(ts[0]) == want
            assert c.get_option("in_flight") == 0
            # binds: no handle, no set
            before = c.get_option("bases_bound")
            with pytest.raises(pkg.MsmError) as e:
                c.bind_points(bad)
            _expect(e, at, reason)
            with pytest.raises(pkg.MsmError) as e:
                c.bind_points_device(dbad.data_ptr(), N)
            _expect(e, at, reason)
            assert c.get_option("bases_bound") == before
            # the next good MSM on the same context and work sets
            assert c.run(pts, sc) == want
            assert c.run_device(dgood.data_ptr(), ds.data_ptr(), N) == want
        bs = c.bind_points(pts)                                    # a good set binds, and its MSMs are not checked again
        assert c.run_scalars(bs, sc) == want
        c.release_points(bs)


def test_multi_device_reports_the_global_index(pkg):
    """a (0, 0, 0, 0) context: point slices of a host buffer and the window shards of device-resident inputs"""
    n = 40000
    pts, sc = oracle.gen_points(8, n), oracle.gen_scalars(8, n)
    name, pt, reason = te_bad_classes()[-1]
    at = n - 7                                                     # in the last of four slices
    bad = _with(pts, 64, at, pt)
    with _ctx(pkg, 0, 2, ids=(0, 0, 0, 0)) as c:
        with pytest.raises(pkg.MsmError) as e:
            c.run(bad, sc)
        _expect(e, at, reason)
        dbad, ds = _dev(bad), _dev(sc)
        _sync()
        with pytest.raises(pkg.MsmError) as e:
            c.run_device(dbad.data_ptr(), ds.data_ptr(), n)
        _expect(e, at, reason)
        with pytest.raises(pkg.MsmError) as e:
            c.bind_points(bad)
        _expect(e, at, reason)
        assert c.run(pts, sc) == oracle.msm(pts, sc, threads=8)


def test_partial_device_refused_while_checking(pkg):
    pts, sc = oracle.gen_points(9, 1000), oracle.gen_scalars(9, 1000)
    import torch
    with _ctx(pkg, 0, 1) as c:
        c_, w = c.plan(1000)
        dp, ds = _dev(pts), _dev(sc)
        rows = torch.zeros(w * pkg.PARTIAL_BYTES, dtype=torch.uint8, device="cuda")
        _sync()
        with pytest.raises(pkg.MsmError) as e:
            c.partial_device(dp.data_ptr(), ds.data_ptr(), 1000, rows.data_ptr())
        assert e.value.code == -1 and "te_msm_check_points_device" in str(e.value)
        with pytest.raises(pkg.MsmError) as e:
            c.partial_device_batch([dp.data_ptr()], [ds.data_ptr()], 1000, rows.data_ptr())
        assert e.value.code == -1


def test_default_is_unchanged_for_non_canonical_input(pkg):
    """check_points = 0: x + p at one index is reduced silently, exactly as before the option existed"""
    pts, sc = oracle.gen_points(10, N), oracle.gen_scalars(10, N)
    P = m.xy_from_bytes(pts[64 * 5:64 * 6])
    alt = _with(pts, 64, 5, (P[0] + m.P).to_bytes(32, "little") + P[1].to_bytes(32, "little"))
    with pkg.MsmContext((0,)) as c:
        assert c.run(alt, sc) == c.run(pts, sc) == oracle.msm(pts, sc, threads=8)


def test_node_rejects_bad_points(pkg, tmp_path):
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        subprocess.check_call(["make", "-C", js, "-s"])
    pts, sc = oracle.gen_points(12, N), oracle.gen_scalars(12, N)
    bad = _with(pts, 64, 42, te_bad_classes()[-1][1])
    (tmp_path / "p.bin").write_bytes(bad)
    (tmp_path / "g.bin").write_bytes(pts)
    (tmp_path / "s.bin").write_bytes(sc)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
const [bad, good, sc] = process.argv.slice(2).map((f) => fs.readFileSync(f));
(async () => {
  const out = {};
  m.setCheckPoints(2);
  try { await m.compute_msm(bad, sc, false); out.run = 'resolved'; } catch (e) { out.run = String(e.message); }
  try { m.setBases(bad); out.bases = 'bound'; } catch (e) { out.bases = String(e.message); }
  const r = await m.compute_msm(good, sc, false);
  out.x = r.x.toString(); out.y = r.y.toString();
  m.setCheckPoints(0);
  console.log(JSON.stringify(out));
})().catch((e) => { console.log(JSON.stringify({ fatal: String(e) })); });
"""
    r = subprocess.run([node, "-e", script, js, str(tmp_path / "p.bin"), str(tmp_path / "g.bin"), str(tmp_path / "s.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert "te_msm error -5" in out["run"] and "input point 42" in out["run"] and "subgroup" in out["run"], out
    assert "te_msm error -5" in out["bases"] and "input point 42" in out["bases"], out
    assert (int(out["x"]), int(out["y"])) == m.xy_from_bytes(oracle.msm(pts, sc, threads=8))
