"""The EDF cells of tests/edf_cells.py checked without a GPU: (1) the restatement edf_read is the reference
Reader -- on the recorded reads of tests/golden/g11_edf.npz / synthetic.edf and on every cell of the tiny
geometries that the reference itself can read (tests/golden/g11_edf_cells.npz, recipe
make_golden_edf_cells.py), bit for bit; (2) Reader.plan, the host half of the device decode, gives the
restatement's per-channel lengths and only indices inside the records Reader._records returns, and a NumPy
emulation of edf_decode_kernel's arithmetic on that plan gives the restatement's bits, on every cell --
the single-signal file and the channel behind a mid-file annotation signal included, which the reference
cannot read; (3) a file shorter than its header says raises ValueError from Reader.read before any device
is asked for, while reads of records that are wholly present plan and load as before; (4) the large file
of the GPU test sends the kernel's grid-stride loop (256 threads, at most 2048 blocks) round twice."""

import os

import numpy as np
import pytest

import edf_cells as ec
from openseize_amd.file_io.edf import Reader

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def emulate(reader, f, start, stop, padvalue):
    """Reader.read with edf_decode_kernel's arithmetic done in NumPy on Reader.plan's numbers; asserts on the
    way that the plan's lengths are the restatement's and every index formed lies inside the loaded records."""
    chans = list(reader.channels)
    span = ec.resolve(f, start, stop)
    if span is None:
        return np.empty((len(chans), 0))
    start, stop = span
    p = reader.plan(start, stop, reader.channels)
    raw = reader._records(p["rec0"], p["nrec"])
    assert raw.dtype == np.int16 and raw.size == p["nrec"] * p["reclen"]
    assert p["len"].tolist() == ec.channel_lengths(f, chans, start, stop), (chans, start, stop)
    assert p["width"] == max(p["len"]) and p["reclen"] == sum(f["spr"])
    idx = [reader.header.channels.index(c) for c in chans]
    slope, offset = reader.header.slopes[idx], reader.header.offsets[idx]
    out = np.empty((len(chans), p["width"]))
    i = np.arange(p["width"])
    for c in range(len(chans)):
        s = start + i[:p["len"][c]]
        spr = int(p["spr"][c])
        at = (s // spr - p["rec0"]) * p["reclen"] + int(p["choff"][c]) + s % spr
        assert at.size == 0 or (at.min() >= 0 and at.max() < raw.size), (chans, start, stop, c)
        d = np.full(p["width"], padvalue, dtype=np.float64)
        d[:at.size] = raw[at]
        with np.errstate(invalid="ignore"):
            out[c] = d * slope[c] + offset[c]
    return out


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """name -> (path, parsed file) of every tiny geometry, written once."""
    root = tmp_path_factory.mktemp("edf_cells")
    files = {}
    for name in ec.GEOMETRIES:
        path = root / (name + ".edf")
        recs = ec.write_geometry(path, name)
        f = ec.parse_edf(path)
        assert np.array_equal(f["recs"], recs) and recs.min() == -32768 and recs.max() == 32767
        files[name] = (path, f)
    return files


# ------------------------------------------------------------------ (1) the restatement is the reference
def test_restatement_reproduces_the_recorded_reads(golden):
    g = golden("g11_edf.npz")
    f = ec.parse_edf(os.path.join(GOLDEN, "synthetic.edf"))
    hc = ec.header_channels(f["names"])
    assert hc == g["channels"].tolist() and ec.longest(f) == g["shape"][1]
    assert ec.same(ec.edf_read(f, hc, 0), g["read_all"])
    assert ec.same(ec.edf_read(f, hc, 123, 4567), g["read_123_4567"])
    assert ec.same(ec.edf_read(f, hc, 4900, 5200), g["read_4900_5200"])
    assert ec.same(ec.edf_read(f, hc, 9990), g["read_9990_end"])
    assert ec.same(ec.edf_read(f, hc, 4000, 6000, padvalue=0.0), g["read_pad0"])
    assert ec.same(ec.edf_read(f, [0, 3], 250, 2750), g["read_ch03"])
    assert ec.same(ec.edf_read(f, [2], 100, 4000), g["read_ch2"])
    assert ec.same(ec.edf_read(f, hc, 300, 8000), g["pro2_cat"])
    assert np.isnan(g["read_4900_5200"]).any()              # the slow channel runs out inside a recorded read


@pytest.mark.parametrize("name", sorted(ec.GEOMETRIES))
def test_restatement_reproduces_the_reference_cells(golden, tiny, name):
    g = golden("g11_edf_cells.npz")
    _, f = tiny[name]
    ok, shapes, flat = g[name + "_ok"], g[name + "_shape"], g[name + "_flat"]
    cells = list(ec.cells(f))
    assert len(cells) == len(ok) == len(shapes)
    at = 0
    for (chans, pad, a, b), good, shape in zip(cells, ok, shapes):
        # what the reference cannot read (IndexError): a single-signal file, and any list with a channel
        # behind an annotation signal in mid-file -- unless the start lies past the end, which it answers
        # with (nch, 0) before it looks at the channels
        behind = ec.ANNOTATION in f["names"][1:-1] and max(chans) > f["names"].index(ec.ANNOTATION)
        readable = len(f["spr"]) > 1 and not behind
        assert good == (readable or (len(f["spr"]) > 1 and ec.resolve(f, a, b) is None)), (chans, a, b)
        if not good:
            continue
        want = flat[at:at + shape[0] * shape[1]].reshape(shape)
        at += want.size
        assert ec.same(ec.edf_read(f, chans, a, b, padvalue=pad), want), (chans, pad, a, b)
    assert at == flat.size
    assert ok.any() == (name != "single_signal")


# ------------------------------------------------------------------ (2) the plan
@pytest.mark.parametrize("name", sorted(ec.GEOMETRIES))
def test_plan_gives_the_restatement_on_every_cell(tiny, name):
    path, f = tiny[name]
    padded = 0
    with Reader(path) as reader:
        assert list(reader.header.channels) == ec.header_channels(f["names"])
        assert max(reader.header.samples) == ec.longest(f)
        for chans, pad, a, b in ec.cells(f):
            reader.channels = chans
            got, want = emulate(reader, f, a, b, pad), ec.edf_read(f, chans, a, b, padvalue=pad)
            assert ec.same(got, want), (chans, pad, a, b)
            padded += int(np.isnan(want).any())
    assert (padded > 0) == (len(set(f["spr"])) > 1)         # the sweep meets channels that run out


def test_pinned_behaviours(tiny):
    """Three behaviours that follow the reference (a sweep of this plan against the reference Reader found
    them equal; the recorded cells hold them too)."""
    path, f = tiny["four_rates"]
    top = ec.longest(f)
    assert top == 12
    hc = ec.header_channels(f["names"])
    # stop=0 means "to the end", as stop=None does: the reference tests the truth value of stop
    assert ec.same(ec.edf_read(f, hc, 0, 0), ec.edf_read(f, hc, 0, None))
    assert ec.edf_read(f, hc, 0, 0).shape == (4, top)
    # start == max(samples) is not "past the end": it is read, and gives (nch, 0); so does start > max
    assert ec.resolve(f, top, None) == (top, top) and ec.resolve(f, top + 1, None) is None
    assert ec.edf_read(f, hc, top).shape == (4, 0) and ec.edf_read(f, hc, top + 1).shape == (4, 0)
    with Reader(path) as reader:
        p = reader.plan(top, top, reader.channels)
        assert p["width"] == 0 and p["nrec"] == 0 and reader._records(p["rec0"], p["nrec"]).size == 0
        assert reader.read(top + 1).shape == (4, 0)
    # an annotation signal at index 0 stays an ordinary channel (Header.channels tests the index's truth
    # value), so this file has three channels and its longest is the annotation signal's
    path, f = tiny["annot_first"]
    with Reader(path) as reader:
        assert reader.header.annotated and reader.header.annotation == 0
        assert list(reader.channels) == [0, 1, 2] and reader.shape == (3, 12)
    assert ec.header_channels(f["names"]) == [0, 1, 2]
    for name, want in (("annot_last", [0, 1]), ("annot_middle", [0, 2])):
        with Reader(tiny[name][0]) as reader:
            assert list(reader.channels) == want and reader.shape == (2, 12)


# ------------------------------------------------------------------ (3) truncated files
@pytest.mark.parametrize("drop, whole", [(7, 2), (20, 2), (60, 0)], ids=["7_bytes", "one_record", "header_only"])
def test_truncated_file_raises_before_the_device(tmp_path, drop, whole):
    """four_rates: 3 records of 10 samples, 60 bytes.  ``whole`` records are left in the file.  Reader.read
    raises ValueError for a read that needs a missing record -- on a machine without a GPU too, so before
    the device is asked for -- and names the path and the sample counts."""
    path = tmp_path / "cut.edf"
    recs = ec.write_geometry(path, "four_rates", drop=drop)
    assert os.path.getsize(path) == 256 + 4 * 256 + 60 - drop
    full = tmp_path / "full.edf"
    ec.write_geometry(full, "four_rates")
    f = ec.parse_edf(full)
    with Reader(path) as reader:
        assert reader.header.num_records == 3                      # the header still announces them
        # the slowest channel (spr 1) needs record `whole` for sample `whole`: reads that stop there raise
        for a, b in ((0, None), (0, whole + 1), (whole, whole + 1), (11, 12)):
            p = reader.plan(a, b or 12, reader.channels)
            found = max(0, min(60 - drop - 20 * p["rec0"], 20 * p["nrec"])) // 2
            msg = r"cut\.edf.* {} samples .* {} of them".format(10 * p["nrec"], found)
            with pytest.raises(ValueError, match=msg):
                reader.read(a, b)
            with pytest.raises(ValueError, match=msg):
                reader._records(p["rec0"], p["nrec"])
        reader.channels = [0]                                      # spr 4: sample 4 * whole is in the hole
        with pytest.raises(ValueError, match=r"cut\.edf"):
            reader.read(4 * whole, 4 * whole + 1)
        # reads of records that are wholly present plan and load as before
        reader.channels = reader.header.channels
        for chans, a, b in (([0, 1, 2, 3], 0, whole), ([0], 0, 4 * whole), ([2, 0], 1, 3 * whole),
                            ([0, 1, 2, 3], 12, None)):
            if b is not None and b <= a:
                continue
            reader.channels = chans
            p = reader.plan(*ec.resolve(f, a, b), reader.channels)
            assert p["rec0"] + p["nrec"] <= whole or p["nrec"] == 0
            raw = reader._records(p["rec0"], p["nrec"])
            assert np.array_equal(raw, recs[p["rec0"]:p["rec0"] + p["nrec"]].reshape(-1))
            assert ec.same(emulate(reader, f, a, b, np.nan), ec.edf_read(f, chans, a, b))
        assert reader.read(13).shape == (len(reader.channels), 0)   # past the end: nothing is loaded


# ------------------------------------------------------------------ (4) the grid of the large file
def test_large_file_goes_round_the_grid_twice():
    full = ec.EDF_THREADS * ec.EDF_MAXBLK
    assert full == 524288
    assert ec.decode_blocks(full) == ec.EDF_MAXBLK and ec.decode_trips(full) == 1
    assert ec.decode_blocks(full - 256) == ec.EDF_MAXBLK - 1
    assert ec.decode_trips(full + 1) == 2 and ec.decode_trips(600 * 1000) == 2
    assert ec.decode_blocks(1) == 1 and ec.decode_blocks(257) == 2 and ec.decode_trips(0) == 0
