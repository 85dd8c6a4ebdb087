"""GPU tests of the record conversion once per occupancy run of a shared slab (include/te_msm.h
te_msm_submit_device): whole-MSM calls in flight over one device-resident point buffer convert it once, while at least one of them
is in flight; a call that joins while that conversion may still be running converts as well; a run that ends forgets it.  Read-only
option "record_conversions" counts the conversions the MSM launch sequences enqueued.  Every result is checked against the oracle."""
import pytest

pytestmark = pytest.mark.gpu

N = 20000


def _dev(buf: bytes):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def data(ora):
    import torch
    pa, pb = ora.gen_points(5100, N), ora.gen_points(5101, N)
    scs = [ora.gen_scalars(5200 + i, N) for i in range(4)]
    d = {"pa": pa, "pb": pb, "scs": scs,
         "want_a": [ora.msm(pa, s, threads=8) for s in scs], "want_b": [ora.msm(pb, s, threads=8) for s in scs],
         "da": _dev(pa), "db": _dev(pb), "dsc": [_dev(s) for s in scs]}
    torch.cuda.synchronize()
    return d


def _conversions(c):
    return c.get_option("record_conversions")


def test_one_conversion_per_occupancy_run(pkg, data):
    """k tickets back to back over one buffer, 4 in flight, the run never empty: one conversion (the first ticket's, complete before
    the others are submitted); a synchronous call inside the run converts nothing either; results equal the oracle"""
    da, dsc, want = data["da"], data["dsc"], data["want_a"]
    with pkg.MsmContext((0,)) as c:
        assert c.get_option("share_records") == 1 and _conversions(c) == 0
        first = c.submit_device(da.data_ptr(), dsc[0].data_ptr(), N)
        c.ticket_wait(first)                                        # its conversion is over; the ticket stays in flight
        assert _conversions(c) == 1
        tickets, got = [(first, 0)], []
        for i in range(1, 16):
            tickets.append((c.submit_device(da.data_ptr(), dsc[i % 4].data_ptr(), N), i % 4))
            if len(tickets) >= 4:
                t, k = tickets.pop(0)
                got.append((c.collect(t), k))
            if i == 9:
                assert c.run_device(da.data_ptr(), dsc[1].data_ptr(), N) == want[1]
        while tickets:
            t, k = tickets.pop(0)
            got.append((c.collect(t), k))
        assert [g for g, _ in got] == [want[k] for _, k in got]
        assert _conversions(c) == 1
        # the run is over: the next ticket converts again
        assert c.collect(c.submit_device(da.data_ptr(), dsc[2].data_ptr(), N)) == want[2]
        assert _conversions(c) == 2


def test_joiners_right_behind_the_first_ticket(pkg, data):
    """tickets submitted back to back with nothing finished yet: each converts unless it finds the run's conversion complete --
    between 1 and k conversions, results equal the oracle; a second wave inside the same run converts nothing"""
    da, dsc, want = data["da"], data["dsc"], data["want_a"]
    with pkg.MsmContext((0,)) as c:
        ts = [c.submit_device(da.data_ptr(), d.data_ptr(), N) for d in dsc]
        first_wave = _conversions(c)
        assert 1 <= first_wave <= 4
        c.ticket_wait(ts[0])                                        # the run's first ticket: the conversion the run remembers
        ts.append(c.submit_device(da.data_ptr(), dsc[0].data_ptr(), N))     # the run is still open (nothing collected)
        assert _conversions(c) == first_wave
        assert [c.collect(t) for t in ts] == want + [want[0]]


def test_new_points_after_the_run_ends(pkg, data):
    """collect everything, overwrite the buffer, submit again: the new points' results, from a new conversion"""
    import torch
    dsc = data["dsc"]
    dx = data["da"].clone()
    torch.cuda.synchronize()
    with pkg.MsmContext((0,)) as c:
        t0 = c.submit_device(dx.data_ptr(), dsc[0].data_ptr(), N)
        c.ticket_wait(t0)
        ts = [t0] + [c.submit_device(dx.data_ptr(), d.data_ptr(), N) for d in dsc[1:]]
        assert [c.collect(t) for t in ts] == data["want_a"] and _conversions(c) == 1
        dx.copy_(data["db"])
        torch.cuda.synchronize()
        t0 = c.submit_device(dx.data_ptr(), dsc[0].data_ptr(), N)
        c.ticket_wait(t0)
        ts = [t0] + [c.submit_device(dx.data_ptr(), d.data_ptr(), N) for d in dsc[1:]]
        assert [c.collect(t) for t in ts] == data["want_b"] and _conversions(c) == 2
        # the same through a synchronous call alone: its run ends with it
        dx.copy_(data["da"])
        torch.cuda.synchronize()
        assert c.run_device(dx.data_ptr(), dsc[3].data_ptr(), N) == data["want_a"][3] and _conversions(c) == 3


def test_buffers_lengths_and_curves_convert_separately(pkg, ora, data):
    """two buffers interleaved, a shorter n over the first buffer's pointer and BLS12-377 tickets: a run (and one conversion) each,
    correct results"""
    import torch
    from oracle import oracle377 as o
    da, db, dsc = data["da"], data["db"], data["dsc"]
    h = N // 2
    want_h = ora.msm(data["pa"][:64 * h], data["scs"][1][:32 * h], threads=8)
    with pkg.MsmContext((0,)) as c:
        heads = [c.submit_device(da.data_ptr(), dsc[0].data_ptr(), N), c.submit_device(db.data_ptr(), dsc[0].data_ptr(), N),
                 c.submit_device(da.data_ptr(), dsc[1].data_ptr(), h)]
        for t in heads:
            c.ticket_wait(t)
        assert _conversions(c) == 3 and c.get_option("record_slabs") == 3
        more = [c.submit_device((da if i % 2 == 0 else db).data_ptr(), dsc[i].data_ptr(), N) for i in range(4)]
        more.append(c.submit_device(da.data_ptr(), dsc[1].data_ptr(), h))
        assert _conversions(c) == 3
        got = [c.collect(t) for t in heads + more]
        assert got[:3] == [data["want_a"][0], data["want_b"][0], want_h]
        assert got[3:7] == [data["want_a"][0], data["want_b"][1], data["want_a"][2], data["want_b"][3]] and got[7] == want_h
        m = 5000
        p3, s3 = o.gen_points(41, m), o.gen_scalars(41, m)
        d3, ds3 = _dev(p3), _dev(s3)
        torch.cuda.synchronize()
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        t0 = c.submit_device(d3.data_ptr(), ds3.data_ptr(), m)
        c.ticket_wait(t0)
        ts = [t0] + [c.submit_device(d3.data_ptr(), ds3.data_ptr(), m) for _ in range(3)]
        assert [c.collect(t) for t in ts] == [o.msm(p3, s3, threads=4)] * 4
        assert _conversions(c) == 4


def test_first_ticket_ends_in_a_scalar_error(pkg, model, data):
    """the run's first ticket ends in TE_MSM_ESCALAR (a scalar its 17 x 15-bit windows cannot hold): its conversion still ran, and
    the tickets that joined it gather from it -- correct results"""
    da, dsc, want = data["da"], data["dsc"], data["want_a"]
    bad = _dev(model.scalars_to_bytes([(1 << 254) + 12345] + [3] * (N - 1)))
    import torch
    torch.cuda.synchronize()
    with pkg.MsmContext((0,)) as c:
        c.set_option("window_bits", 15)
        base = _conversions(c)
        t0 = c.submit_device(da.data_ptr(), bad.data_ptr(), N)
        c.ticket_wait(t0)
        ts = [c.submit_device(da.data_ptr(), d.data_ptr(), N) for d in dsc[:3]]
        with pytest.raises(pkg.MsmError) as e:
            c.collect(t0)
        assert e.value.code == -3
        ts.append(c.submit_device(da.data_ptr(), dsc[3].data_ptr(), N))
        assert [c.collect(t) for t in ts] == want
        assert _conversions(c) == base + 1


def test_forms_that_convert_on_every_call(pkg, data):
    """"share_records" = 2 (the round-6 form), option "check_points" and the building block te_msm_partial_device convert on every
    call; a ticket that follows a building block over a buffer changed in between converts again"""
    import torch
    da, dsc, want = data["da"], data["dsc"], data["want_a"]
    with pkg.MsmContext((0,)) as c:
        for opt, val in (("share_records", 2), ("check_points", 1)):
            c.set_option(opt, val)
            base = _conversions(c)
            t0 = c.submit_device(da.data_ptr(), dsc[0].data_ptr(), N)
            c.ticket_wait(t0)
            ts = [t0] + [c.submit_device(da.data_ptr(), d.data_ptr(), N) for d in dsc[1:]]
            assert [c.collect(t) for t in ts] == want
            assert _conversions(c) == base + 4, opt
            c.set_option(opt, 1 if opt == "share_records" else 0)
        # a building block holds the slab of a buffer (its completion is not seen) while a ticket's run over it comes and goes
        dx = da.clone()
        cw, W = c.plan(N)
        part = torch.zeros(W * 720, dtype=torch.uint8, device="cuda")
        c.set_option("workset", 7)
        torch.cuda.synchronize()
        base = _conversions(c)
        c.partial_device(dx.data_ptr(), dsc[0].data_ptr(), N, part.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert c.finalize(part.cpu().numpy().tobytes(), cw, W) == want[0]
        assert c.collect(c.submit_device(dx.data_ptr(), dsc[1].data_ptr(), N)) == want[1]
        dx.copy_(data["db"])
        torch.cuda.synchronize()
        assert c.collect(c.submit_device(dx.data_ptr(), dsc[2].data_ptr(), N)) == data["want_b"][2]
        assert _conversions(c) == base + 3
