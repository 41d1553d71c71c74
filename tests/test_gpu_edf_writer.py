"""The EDF Writer / splitter and the osz_edf_encode kernel on the device.

Every comparison but the read-back is equality of bytes: against the files the reference wrote
(tests/golden/g22_edf_write.npz), against the source file's own records, and against
``encode_numpy`` of tests/test_edf_writer_host.py, which that file pins to the reference."""

import json
import os
import warnings
from functools import partial

import numpy as np
import pytest

from test_edf_writer_host import SYNTHETIC, encode_numpy, golden_cases

from openseize_amd import producer
from openseize_amd.core.producer import Producer

pytestmark = pytest.mark.gpu

SENTINEL = 1e200
KINDS = ("one", "ring2", "ring3", "host")


@pytest.fixture(scope="module")
def edf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd.file_io import edf as module
    return module


class Recycler(Producer):
    """Chunks of ``data`` along ``axis``, each written into a reused buffer and yielded (the
    source of tests/test_gpu_recycled.py); the buffer is overwritten once the stream has ended."""

    def __init__(self, data, chunksize, axis, kind):
        super().__init__(data, chunksize, axis)
        self.kind = kind

    @property
    def shape(self):
        return tuple(self.data.shape)

    def __iter__(self):
        import torch
        x, cs, axis = self.data, self.chunksize, self.axis
        n = x.shape[axis]
        dims = list(x.shape)
        if self.kind == "host":
            dims[axis] = cs
            buf = np.empty(dims)
            slots = [buf]
        else:
            ring = {"one": 1, "ring2": 2, "ring3": 3}[self.kind]
            dims[axis] = ring * cs
            buf = torch.empty(dims, dtype=torch.float64, device="cuda")
            slots = [buf.narrow(axis, r * cs, cs) for r in range(ring)]
        try:
            for k, start in enumerate(range(0, n, cs)):
                m = min(cs, n - start)
                slot = slots[k % len(slots)]
                if self.kind == "host":
                    idx = [slice(None)] * x.ndim
                    idx[axis] = slice(0, m)
                    src = list(idx)
                    src[axis] = slice(start, start + m)
                    dst = slot[tuple(idx)]
                    np.copyto(dst, x[tuple(src)])
                else:
                    dst = slot.narrow(axis, 0, m)
                    dst.copy_(x.narrow(axis, start, m))
                yield dst
        finally:
            if self.kind == "host":
                buf.fill(SENTINEL)
            else:
                buf.fill_(SENTINEL)


def make_header(spr, nrec, pmin, pmax):
    ns = len(spr)
    return {"version": "0", "patient": "p", "recording": "r", "start_date": "01.01.26",
            "start_time": "00.00.00", "header_bytes": 256 + 256 * ns, "reserved_0": "",
            "num_records": nrec, "record_duration": 1.0, "num_signals": ns,
            "names": [f"ch{i}" for i in range(ns)], "transducers": ["t"] * ns,
            "physical_dim": ["uV"] * ns, "physical_min": list(pmin), "physical_max": list(pmax),
            "digital_min": [-32768.0] * ns, "digital_max": [32767.0] * ns,
            "prefiltering": [""] * ns, "samples_per_record": list(spr), "reserved_1": [""] * ns}


def write(edf, path, header, data, channels):
    with edf.Writer(path) as writer:
        writer.write(header, data, channels, verbose=False)
    return np.fromfile(path, dtype=np.uint8)


def expected_file(edf, header, data, channels):
    """Header bytes + the restatement's records for (all channels, samples) host data."""
    plan = edf.record_plan(header, channels)
    recs, _, _ = encode_numpy([data[c] for c in channels], plan["spr"], plan["slope"], plan["offset"],
                              plan["nrec"])
    head = edf.header_bytes(edf.Header.from_dict(header).filter(channels))
    return np.concatenate([np.frombuffer(head, np.uint8), recs.view(np.uint8)])


# ------------------------------------------------------------------- against the reference's files
def test_golden_reader_and_array_cases(edf, golden, tmp_path):
    g = golden("g22_edf_write.npz")
    for name, hdr, chs, blob in golden_cases(g)[:3]:
        if name == "c2":
            got = write(edf, tmp_path / f"{name}.edf", hdr, g["c2_data"], chs)
        else:
            with edf.Reader(SYNTHETIC) as reader:
                got = write(edf, tmp_path / f"{name}.edf", hdr, reader, chs)
        assert np.array_equal(got, blob), name


def test_golden_splitter(edf, golden, tmp_path):
    g = golden("g22_edf_write.npz")
    before = np.fromfile(SYNTHETIC, dtype=np.uint8)
    edf.splitter(SYNTHETIC, {"left": [0, 1], "right.edf": [3, 2]}, outdir=tmp_path)
    assert sorted(os.listdir(tmp_path)) == ["left.edf", "right.edf"]
    for name in ("left", "right"):
        assert np.array_equal(np.fromfile(tmp_path / f"{name}.edf", dtype=np.uint8), g[f"c3_file_{name}"])
    assert np.array_equal(np.fromfile(SYNTHETIC, dtype=np.uint8), before)


def test_reader_to_writer_keeps_the_int16_values(edf, tmp_path):
    with edf.Reader(SYNTHETIC) as reader:
        reader.channels = [3, 0]
        got = write(edf, tmp_path / "all.edf", reader.header, reader, [0, 1, 2, 3])
        assert reader.channels == [3, 0]
        hdr = reader.header
    raw = np.fromfile(SYNTHETIC, "<i2", offset=hdr.header_bytes).reshape(hdr.num_records, -1)
    assert raw.shape[1] == 1780
    recs = got[256 + 256 * 4:].view("<i2").reshape(hdr.num_records, -1)
    assert np.array_equal(recs, raw[:, :1750])
    assert np.array_equal(got[:256 + 256 * 4], np.frombuffer(edf.header_bytes(hdr.filter([0, 1, 2, 3])), np.uint8))


# --------------------------------------------------------------- one file whatever the input kind
SPR, NREC = 300, 20
RANGE = ([-3276.8, -500.0, -1000.0, -200.0], [3276.7, 500.0, 1000.0, 250.0])


def stream_data(seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(lo, hi, SPR * NREC) for lo, hi in zip(*RANGE)])


@pytest.mark.parametrize("channels", ([0, 1, 2, 3], [0, 1, 3], [0, 2], [2], [3, 1]))
def test_array_tensor_and_producers_write_the_same_file(edf, tmp_path, channels, monkeypatch):
    import torch
    x = stream_data()
    hdr = make_header([SPR] * 4, NREC, *RANGE)
    want = expected_file(edf, hdr, x, channels)
    xd = torch.from_numpy(x).cuda()
    assert np.array_equal(write(edf, tmp_path / "a.edf", hdr, x, channels), want)
    assert np.array_equal(write(edf, tmp_path / "t.edf", hdr, xd, channels), want)
    reclen = SPR * len(channels)
    for group_bytes in (None, 2 * reclen * 3):           # one group; three records per launch
        if group_bytes:
            monkeypatch.setattr(edf, "GROUP_BYTES", group_bytes)
        assert np.array_equal(write(edf, tmp_path / "t.edf", hdr, xd, channels), want)
        for cs in (100, SPR, 301, 7000):                 # below a record, equal, coprime, > stream
            for data, axis in ((x, -1), (xd, -1), (np.ascontiguousarray(x.T), 0), (xd.T.contiguous(), 0)):
                got = write(edf, tmp_path / "p.edf", hdr, producer(data, cs, axis), channels)
                assert np.array_equal(got, want), (cs, axis, type(data).__name__, group_bytes)


def test_unequal_rates_in_several_groups(edf, golden, tmp_path, monkeypatch):
    """Arrays, tensors and a Reader with channels of different rates, three and seven records per
    launch: the same files as in one group."""
    import torch
    g = golden("g22_edf_write.npz")
    cases = golden_cases(g)
    for records in (3, 7):
        for name, hdr, chs, blob in cases:
            plan = edf.record_plan(hdr, chs)
            monkeypatch.setattr(edf, "GROUP_BYTES", 2 * plan["reclen"] * records)
            if name == "c2":
                assert np.array_equal(write(edf, tmp_path / "g.edf", hdr, g["c2_data"], chs), blob)
                data = torch.from_numpy(g["c2_data"]).cuda()
            else:
                data = edf.Reader(SYNTHETIC)
            assert np.array_equal(write(edf, tmp_path / "g.edf", hdr, data, chs), blob), (name, records)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("axis", (-1, 0))
def test_buffer_reusing_sources(edf, tmp_path, kind, axis):
    import torch
    x = stream_data(6)
    hdr = make_header([SPR] * 4, NREC, *RANGE)
    want = expected_file(edf, hdr, x, [0, 1, 3])
    xs = x if axis == -1 else np.ascontiguousarray(x.T)
    data = xs if kind == "host" else torch.from_numpy(xs).cuda()
    for cs in (77, SPR, 301, 1000):
        got = write(edf, tmp_path / "r.edf", hdr, Recycler(data, cs, axis % 2, kind), [0, 1, 3])
        assert np.array_equal(got, want), cs


def test_stream_that_does_not_match_its_shape(edf, tmp_path):
    x = stream_data()
    hdr = make_header([SPR] * 4, NREC, *RANGE)

    def gen(n):
        for s in range(0, n, 1000):
            yield x[:, s:min(s + 1000, n)]
    for n in (SPR * NREC - SPR, SPR * NREC - 1):           # ends early
        with pytest.raises(ValueError, match="does not describe"):
            write(edf, tmp_path / "s.edf", hdr, producer(partial(gen, n), 1000, -1, shape=x.shape), [0, 1])
    longer = np.concatenate([x, x[:, :SPR]], axis=1)       # goes on past num_records records

    def gen_long():
        yield longer
    with pytest.raises(ValueError, match="does not describe"):
        write(edf, tmp_path / "s.edf", hdr, producer(gen_long, 1000, -1, shape=x.shape), [0, 1])


# ------------------------------------------------------------------------------ the kernel alone
def run_kernel(rows, spr, slope, offset, nrec, pad=0, carried=0):
    """osz_edf_encode of the host rows: (records, saturated, NaN).  ``pad``: extra columns per
    row of x (ldx larger than the row), ``carried``: samples per row handed over as carry (at
    most the row's spr - 1).  Both buffers are filled with a sentinel where no sample lies, and
    the output is followed by guard values that must survive."""
    import torch
    from openseize_amd import _device as dev
    nch = len(rows)
    spr = np.asarray(spr, np.int64)
    h = np.minimum(carried, spr - 1).astype(np.int32)
    width = int(max(len(r) - hc for r, hc in zip(rows, h)))
    xh = np.full((nch, width + pad), SENTINEL)
    ch = np.full((nch, max(int(h.max()), 1)), SENTINEL)
    for c, r in enumerate(rows):
        ch[c, :h[c]] = r[:h[c]]
        xh[c, :len(r) - h[c]] = r[h[c]:]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    reclen = int(spr.sum())
    choff = np.cumsum(np.insert(spr, 0, 0))[:-1]
    n = nrec * reclen
    out = torch.full((n + 64,), 12345, dtype=torch.int16, device="cuda")
    counter = torch.zeros(2, dtype=torch.int64, device="cuda")
    x2d = up(xh)[:, :width] if pad else up(xh)
    dev.edf_encode(x2d, up(spr.astype(np.int32)), up(choff.astype(np.int32)), up(np.asarray(slope, float)),
                   up(np.asarray(offset, float)), reclen, nrec, out[:n], counter,
                   carry=up(ch) if carried else None, h=up(h) if carried else None)
    got = out.cpu().numpy()
    assert np.all(got[n:] == 12345)
    clipped, nans = counter.cpu().tolist()
    return got[:n], clipped, nans


GEOMETRIES = {
    "one channel": ([7], 5),
    "one record": ([5, 3, 1000, 4], 1),
    "300 channels": (list(np.random.default_rng(1).integers(1, 10, 300)), 3),
    # groups of four straddle several channels, choff takes every residue mod 4, reclen is odd
    "mixed": ([1, 3, 4, 5, 1000, 1, 1, 1, 1, 1, 3, 1000, 5, 4, 1, 1, 2, 1000, 1, 1, 1, 1, 1, 1, 1, 4], 7),
    "all ones": ([1] * 13, 9),
    "wide": ([1000, 999, 1001, 1024], 6),
    "grid wraps": ([100] * 256, 520),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_kernel_geometries(edf, name):
    spr, nrec = GEOMETRIES[name]
    if name == "mixed":
        choff = np.cumsum(np.insert(spr, 0, 0))[:-1]
        assert set(choff % 4) == {0, 1, 2, 3} and sum(spr) % 2 == 1
    rng = np.random.default_rng(len(spr) * 1000 + nrec)
    slope = rng.uniform(0.01, 2.0, len(spr))
    offset = rng.uniform(-50, 50, len(spr))
    rows = [o + s * rng.uniform(-32768, 32767, sp * nrec) for sp, s, o in zip(spr, slope, offset)]
    want, wc, wn = encode_numpy(rows, spr, slope, offset, nrec)
    variants = [(0, 0)] if name == "grid wraps" else [(0, 0), (5, 0), (0, 1), (3, 10 ** 6), (0, 2)]
    for pad, carried in variants:       # carry lengths 0, 1, spr - 1 (10 ** 6 is cut to it), 2
        got, clipped, nans = run_kernel(rows, spr, slope, offset, nrec, pad, carried)
        assert np.array_equal(got, want), (name, pad, carried)
        assert (clipped, nans) == (wc, wn)


def test_kernel_ties_round_half_to_even(edf):
    ks = np.arange(-32768, 32767, dtype=np.float64)
    rows = [ks + 0.5]
    got, clipped, nans = run_kernel(rows, [ks.size], [1.0], [0.0], 1)
    assert np.array_equal(got, np.rint(rows[0]).astype("<i2")) and (clipped, nans) == (0, 0)


def test_empty_launch(edf):
    import torch
    from openseize_amd import _device as dev
    z = lambda dt: torch.zeros(1, dtype=dt, device="cuda")
    out = torch.full((8,), 7, dtype=torch.int16, device="cuda")
    dev.edf_encode(None, z(torch.int32) + 4, z(torch.int32), z(torch.float64) + 1, z(torch.float64), 4, 0,
                   out, torch.zeros(2, dtype=torch.int64, device="cuda"))
    assert out.cpu().tolist() == [7] * 8


# ------------------------------------------------------------- out of range and non-finite input
def test_out_of_range_and_nonfinite(edf, tmp_path):
    x = stream_data(7)
    hdr = make_header([SPR] * 4, NREC, *RANGE)
    plan = edf.record_plan(hdr, [0, 1, 2, 3])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        clean = write(edf, tmp_path / "c.edf", hdr, x, [0, 1, 2, 3])
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)]
    bad = x.copy()
    bad[0, 3], bad[0, 4], bad[1, 10], bad[1, 11] = 4000.0, -4000.0, np.inf, -np.inf
    bad[2, 299], bad[3, 300], bad[3, 5999] = np.nan, np.nan, 1e300
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = write(edf, tmp_path / "b.edf", hdr, bad, [0, 1, 2, 3])
    caught = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(caught) == 1
    assert "5 values" in str(caught[0].message) and "2 values" in str(caught[0].message)
    recs = got[256 + 256 * 4:].view("<i2").reshape(NREC, 4, SPR)
    assert recs[0, 0, 3] == 32767 and recs[0, 0, 4] == -32768
    assert recs[0, 1, 10] == 32767 and recs[0, 1, 11] == -32768
    assert recs[0, 2, 299] == 0 and recs[1, 3, 0] == 0 and recs[19, 3, 299] == 32767
    same = np.ones(recs.shape, bool)
    for r, c, j in ((0, 0, 3), (0, 0, 4), (0, 1, 10), (0, 1, 11), (0, 2, 299), (1, 3, 0), (19, 3, 299)):
        same[r, c, j] = False
    assert np.array_equal(recs[same], clean[256 + 256 * 4:].view("<i2").reshape(NREC, 4, SPR)[same])
    # the kernel's counter alone, against the restatement
    want, wc, wn = encode_numpy(list(bad), plan["spr"], plan["slope"], plan["offset"], NREC)
    k, clipped, nans = run_kernel(list(bad), plan["spr"], plan["slope"], plan["offset"], NREC)
    assert (clipped, nans) == (wc, wn) == (5, 2) and np.array_equal(k, want)
    assert np.array_equal(k, recs.reshape(-1))


# ------------------------------------------------------------------------------------ a real chain
def test_reader_filter_downsample_writer_chain(edf, tmp_path):
    """producer(Reader, device=True) -> Kaiser low-pass -> downsample(M=5) -> Writer, against the
    restatement applied to the same chain's to_array() at the same chunksize."""
    from openseize_amd.filtering.fir import Kaiser
    from openseize_amd.resampling.resampling import downsample
    cs, chs = 1700, [0, 1, 3]

    def chain():
        reader = edf.Reader(SYNTHETIC)
        reader.channels = chs
        pro = producer(reader, cs, -1, device=True)
        low = Kaiser(fpass=40, fstop=50, fs=500)(pro, chunksize=cs, axis=-1)
        return downsample(low, M=5, fs=500, chunksize=cs, axis=-1)

    hdr = dict(edf.Header(SYNTHETIC).filter(chs))
    hdr["samples_per_record"] = [100] * 3
    out = chain()
    assert tuple(out.shape) == (3, 2000)
    got = write(edf, tmp_path / "chain.edf", hdr, out, [0, 1, 2])
    arr = chain().to_array()
    arr = arr.cpu().numpy() if hasattr(arr, "cpu") else np.asarray(arr)
    assert np.array_equal(got, expected_file(edf, hdr, arr, [0, 1, 2]))


# --------------------------------------------------------------------------------------- read back
def test_written_file_reads_back_within_one_step(edf, golden, tmp_path):
    """In-range samples come back from this package's Reader within one quantisation step
    slope[c]: rounding moves a value by at most half a step, the decode adds two roundings."""
    g = golden("g22_edf_write.npz")
    hdr, x = json.loads(str(g["c2_header"])), g["c2_data"]
    write(edf, tmp_path / "back.edf", hdr, x, [0, 1, 2])
    plan = edf.record_plan(hdr, [0, 1, 2])
    with edf.Reader(tmp_path / "back.edf") as reader:
        assert reader.header.samples_per_record == [100, 100, 50]
        back = reader.read(0)
    assert back.shape == (3, 1200)
    for c in range(3):
        n = int(plan["spr"][c]) * 12
        err = np.abs(back[c, :n] - x[c, :n]).max()
        print(f"channel {c}: max |read back - written| = {err:.6g}, step {plan['slope'][c]:.6g}")
        assert err <= plan["slope"][c]
        assert np.all(np.isnan(back[c, n:]))
