"""Reader.read and osz_edf_decode (file_io/edf.py, csrc/misc.hip) on the GPU against the restatement of
tests/edf_cells.py, which tests/test_edf_cells_host.py shows to be the reference Reader.  Every comparison is
bit for bit (edf_cells.same: NaN equals NaN): the decode is int16 -> float64, one multiply and one add.

* The tiny geometries: every cell of edf_cells.cells() -- all (start, stop) with 0 <= start <= max + 2 and
  stop in {None} u [start, max + 4], over all channels, each alone, reversed and one twice with padvalue NaN,
  and 0.0, -7.5 and inf over all channels.  The full grid is run, nothing is trimmed: 650 to 1650 reads per
  geometry (the time each takes is printed; on an MI355X the slowest, four_rates and annot_first, took
  0.25 s).
* The grid-stride loop (edf_decode_kernel: 256 threads, gridDim.x capped at 2048): a file of 1000 records of
  spr [600, 300, 1], width 600 000 > 2048 * 256 = 524 288, read whole, across the first index of the second
  trip (524 287 .. 524 290), from it to the end, and across the end of the 300-per-record channel.
* gridDim.y: 257 signals of spr 1 .. 3.
* A negative slope (physical_min > physical_max) with asymmetric digital limits.
* device=True: a CUDA tensor of the same bits; the chunks of a device producer over the large file for
  chunk sizes 599, 600 (= spr), 601 and 524 288 concatenate to read(0).
* A file cut short raises the host's ValueError before any launch; the same reader then reads the records
  that are whole."""

import time

import numpy as np
import pytest

import edf_cells as ec

pytestmark = pytest.mark.gpu

BIG_SPR, BIG_NREC = [600, 300, 1], 1000


@pytest.fixture(scope="module")
def Reader():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd.file_io.edf import Reader
    return Reader


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """(path, parsed file, read(0) restated) of the 1.8 MB file, written and restated once."""
    path = tmp_path_factory.mktemp("edf_big") / "big.edf"
    ec.write_edf(path, BIG_SPR, BIG_NREC, pmin=[-3276.8, 1000.0, -1.0], pmax=[3276.7, -1000.0, 1.0],
                 dmin=[-32768, -2048, -32768], dmax=[32767, 2047, 32767], seed=600)
    f = ec.parse_edf(path)
    whole = ec.edf_read(f, [0, 1, 2], 0)
    whole.setflags(write=False)
    return path, f, whole


@pytest.mark.parametrize("name", sorted(ec.GEOMETRIES))
def test_tiny_geometry_every_cell(Reader, tmp_path, name):
    path = tmp_path / (name + ".edf")
    ec.write_geometry(path, name)
    f = ec.parse_edf(path)
    ncell, t0 = 0, time.perf_counter()
    with Reader(path) as reader:
        for chans, pad, a, b in ec.cells(f):
            reader.channels = chans
            got = reader.read(a, b, padvalue=pad)
            assert ec.same(got, ec.edf_read(f, chans, a, b, padvalue=pad)), (chans, pad, a, b)
            ncell += 1
    print(f"{name}: {ncell} reads in {time.perf_counter() - t0:.2f} s")


def test_grid_stride_reads(Reader, big):
    path, f, whole = big
    full = ec.EDF_THREADS * ec.EDF_MAXBLK
    assert whole.shape == (3, 600_000) and ec.decode_trips(whole.shape[1]) == 2
    with Reader(path) as reader:
        assert ec.same(reader.read(0), whole)
        # the first index of the second trip, and one each side of it
        assert ec.same(reader.read(full - 1, full + 2), whole[:, full - 1:full + 2])
        got = reader.read(full)
        assert ec.same(got, whole[:, full:]) and ec.decode_trips(got.shape[1]) == 1
        # the 300-per-record channel ends at 300 000, inside the read; the 1-per-record one long before
        got = reader.read(299_999, 300_002)
        assert ec.same(got, ec.edf_read(f, [0, 1, 2], 299_999, 300_002))
        assert np.isnan(got[1]).tolist() == [False, True, True] and np.isnan(got[2]).all()
        # a pad value goes through the map of its channel: slope -1000 / 2047.5 on channel 1
        got = reader.read(299_999, 300_002, padvalue=np.inf)
        assert ec.same(got, ec.edf_read(f, [0, 1, 2], 299_999, 300_002, padvalue=np.inf))
        assert got[1, 1] == -np.inf and got[2, 0] == np.inf
        reader.channels = [2, 0, 2]
        assert ec.same(reader.read(0), whole[[2, 0, 2]])


def test_257_signals(Reader, tmp_path):
    """One block row of the grid per signal: 257 of them, spr 1, 2, 3, 1, ..."""
    spr = [1 + i % 3 for i in range(257)]
    path = tmp_path / "wide.edf"
    ec.write_edf(path, spr, 3, seed=257)
    f = ec.parse_edf(path)
    hc = list(range(257))
    with Reader(path) as reader:
        assert reader.shape == (257, 9)
        for chans in (hc, hc[::-1], [256], [255, 256, 0]):
            reader.channels = chans
            for a, b in ((0, None), (1, 5), (2, 3), (8, None), (9, None)):
                assert ec.same(reader.read(a, b), ec.edf_read(f, chans, a, b)), (chans[:3], a, b)


def test_negative_slope_and_asymmetric_digital_limits(Reader, tmp_path):
    path = tmp_path / "neg.edf"
    lim = dict(pmin=[1000.0, 250.5], pmax=[-1000.0, -100.25], dmin=[-2048, -100], dmax=[2047, 32767])
    ec.write_edf(path, [5, 3], 4, seed=5, **lim)
    f = ec.parse_edf(path)
    with Reader(path) as reader:
        assert np.all(reader.header.slopes < 0)
        for chans in ([0, 1], [1, 0], [1]):
            reader.channels = chans
            for a, b in ((0, None), (4, 6), (11, 13), (12, None), (3, 20)):
                for pad in (np.nan, np.inf, -7.5):
                    want = ec.edf_read(f, chans, a, b, padvalue=pad)
                    assert ec.same(reader.read(a, b, padvalue=pad), want), (chans, a, b, pad)
        reader.channels = [0, 1]
        got = reader.read(0)
        # the extreme int16 values through a negative slope: -32768 maps above physical_min
        assert got[0, 0] == -32768 * reader.header.slopes[0] + reader.header.offsets[0] > 1000.0


def test_device_reads_and_device_producer(Reader, big):
    import torch
    from openseize_amd import producer
    path, f, whole = big
    with Reader(path) as reader:
        x = reader.read(123, 4567, device=True)
        assert torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64
        assert ec.same(x.cpu().numpy(), whole[:, 123:4567])
        e = reader.read(600_000, device=True)
        assert torch.is_tensor(e) and e.is_cuda and tuple(e.shape) == (3, 0)
        assert tuple(reader.read(600_001, device=True).shape) == (3, 0)
    for cs in (599, 600, 601, ec.EDF_THREADS * ec.EDF_MAXBLK):
        chunks = list(producer(Reader(path), cs, axis=-1, device=True))
        assert all(torch.is_tensor(c) and c.is_cuda for c in chunks)
        assert [c.shape[-1] for c in chunks] == [min(cs, 600_000 - a) for a in range(0, 600_000, cs)]
        assert ec.same(torch.cat(chunks, -1).cpu().numpy(), whole), cs


@pytest.mark.parametrize("drop", [7, 20, 60], ids=["7_bytes", "one_record", "header_only"])
def test_truncated_file_raises_then_reads_whole_records(Reader, tmp_path, drop):
    """four_rates (3 records of 10 samples) cut short: the ValueError of the host test, with no launch; the
    same reader then reads what is whole."""
    path, full = tmp_path / "cut.edf", tmp_path / "full.edf"
    ec.write_geometry(path, "four_rates", drop=drop)
    ec.write_geometry(full, "four_rates")
    f = ec.parse_edf(full)
    whole = (60 - drop) // 20
    with Reader(path) as reader:
        for device in (False, True):
            with pytest.raises(ValueError, match=r"cut\.edf.* 30 samples .* {} of them".format((60 - drop) // 2)):
                reader.read(0, device=device)
        with pytest.raises(ValueError, match=r"cut\.edf"):
            reader.read(whole, whole + 1)
        if whole:
            assert ec.same(reader.read(0, whole), ec.edf_read(f, [0, 1, 2, 3], 0, whole))
            reader.channels = [2, 0]
            assert ec.same(reader.read(1, 3 * whole), ec.edf_read(f, [2, 0], 1, 3 * whole))
        assert reader.read(12).shape == (len(reader.channels), 0)
