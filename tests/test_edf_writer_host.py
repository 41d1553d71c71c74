"""Host logic of the EDF Writer: header bytes, Header.from_dict, the record plan, the
errors raised before any device call -- and ``encode_numpy``, a NumPy restatement of the record
encode that is pinned here to the files the reference wrote (tests/golden/g22_edf_write.npz,
made by tests/golden/make_golden_edfwrite.py) and used by tests/test_gpu_edf_writer.py."""

import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTHETIC = os.path.join(ROOT, "tests", "golden", "synthetic.edf")


def encode_numpy(rows, spr, slope, offset, nrec):
    """EDF records of the 1-D float rows: (flat '<i2' array, saturated count, NaN count).
    Record r holds rint((rows[c][r spr[c]:(r + 1) spr[c]] - offset[c]) / slope[c]) channel after
    channel (the reference's _records / _encipher); outside int16, where the reference's cast is
    undefined, the value saturates and NaN becomes 0."""
    recs, clipped, nans = [], 0, 0
    with np.errstate(all="ignore"):
        for r in range(nrec):
            for c, x in enumerate(rows):
                part = np.asarray(x[r * spr[c]:(r + 1) * spr[c]], dtype=np.float64)
                d = np.rint((part - offset[c]) / slope[c])
                nans += int(np.isnan(d).sum())
                clipped += int(((d > 32767) | (d < -32768)).sum())
                recs.append(np.clip(np.nan_to_num(d, nan=0.0), -32768, 32767).astype("<i2"))
    return np.concatenate(recs), clipped, nans


def golden_cases(g):
    """(name, header dictionary, channels, file bytes) of every file in the fixture."""
    h1, h2 = json.loads(str(g["c1_header"])), json.loads(str(g["c2_header"]))
    cases = [("c1_023", h1, [0, 2, 3], g["c1_file_023"]), ("c1_1", h1, [1], g["c1_file_1"]),
             ("c2", h2, [0, 1, 2], g["c2_file"])]
    for name, chs in zip(g["c3_names"], g["c3_channels"]):
        cases.append((f"c3_{name}", h1, [int(c) for c in chs], g[f"c3_file_{name}"]))
    return cases


def test_header_bytes_match_reference(golden, tmp_path):
    from openseize_amd.file_io.edf import Header, header_bytes
    cases = golden_cases(golden("g22_edf_write.npz"))
    assert len(cases) == 5
    for name, hdr, chs, blob in cases:
        filtered = Header.from_dict(hdr).filter(chs)
        head = header_bytes(filtered)
        assert len(head) == filtered.header_bytes == 256 + 256 * len(chs)
        assert head == blob[:len(head)].tobytes(), name
        path = tmp_path / f"{name}.edf"
        path.write_bytes(head)
        assert dict(Header(path)) == dict(filtered), name
    # the fields the reference formats through str(): floats keep their '.0'
    head = header_bytes(Header.from_dict(cases[0][1]).filter([0, 2, 3]))
    assert head[184:192] == b"1024    " and head[236:256] == b"20      1.0     3   "
    assert head[256 + 3 * (16 + 80 + 8 + 8 + 8):][:8] == b"-32768.0"


def test_from_dict_needs_exactly_the_bytemap_keys():
    from openseize_amd.file_io.edf import Header
    full = dict(Header(SYNTHETIC))
    hdr = Header.from_dict(full)
    assert hdr.path is None and dict(hdr) == full and hdr.num_signals == 5
    assert hdr.count_signals() == 5 and hdr.channels == [0, 1, 2, 3]
    missing = {k: v for k, v in full.items() if k != "prefiltering"}
    with pytest.raises(ValueError):
        Header.from_dict(missing)
    with pytest.raises(ValueError):
        Header.from_dict(dict(full, sample_rate=500))


def test_record_plan():
    from openseize_amd.file_io.edf import Header, record_plan
    hdr = Header(SYNTHETIC)
    plan = record_plan(hdr, [0, 2, 3])
    assert plan["spr"].tolist() == [500, 250, 500] and plan["spr"].dtype == np.int32
    assert plan["choff"].tolist() == [0, 500, 750] and plan["choff"].dtype == np.int32
    assert plan["reclen"] == 1250 and plan["nrec"] == 20
    assert plan["group"] == 20                                     # the whole file fits one group
    assert record_plan(hdr, [0, 2, 3], group_bytes=3 * 2500)["group"] == 3
    assert record_plan(hdr, [0, 2, 3], group_bytes=100)["group"] == 1   # never less than a record
    idx = [0, 2, 3]
    assert np.array_equal(plan["slope"], hdr.slopes[idx])
    assert np.array_equal(plan["offset"], hdr.offsets[idx])


def test_write_errors_come_before_any_device_call(tmp_path, monkeypatch):
    from openseize_amd import _device as dev
    from openseize_amd import producer
    from openseize_amd.file_io.edf import Header, Writer

    def no_device(*a, **k):
        raise AssertionError("device call")
    monkeypatch.setattr(dev, "require_gpu", no_device)
    hdr = Header(SYNTHETIC)
    with Writer(tmp_path / "a.edf") as writer:
        with pytest.raises(ValueError, match="divisible"):
            writer.write(hdr, np.zeros((4, 10001)), [0, 1])
        with pytest.raises(ValueError, match="divisible"):
            writer.write(hdr, producer(np.zeros((4, 10001)), 1000, -1), [0, 1])
        with pytest.raises(ValueError, match="divisible"):
            writer.write(hdr, producer(np.zeros((10001, 4)), 1000, 0), [0, 1])
        with pytest.raises(ValueError, match="equal samples_per_record"):
            writer.write(hdr, producer(np.zeros((4, 10000)), 1000, -1), [0, 2, 3])
    assert os.path.getsize(tmp_path / "a.edf") == 0


def test_restatement_reproduces_reference_records(golden):
    """encode_numpy on the reference Reader's samples (g11) and on the case-2 array gives the
    records of the files the reference wrote, bit for bit."""
    from openseize_amd.file_io.edf import record_plan
    g, g11 = golden("g22_edf_write.npz"), golden("g11_edf.npz")
    cases = {name: (hdr, chs, blob) for name, hdr, chs, blob in golden_cases(g)}
    for name, (hdr, chs, blob) in cases.items():
        data = g["c2_data"] if name == "c2" else g11["read_all"]
        plan = record_plan(hdr, chs)
        rows = [data[c] for c in chs]
        recs, clipped, nans = encode_numpy(rows, plan["spr"], plan["slope"], plan["offset"], plan["nrec"])
        want = blob[256 + 256 * len(chs):].view("<i2")
        assert recs.size == plan["nrec"] * plan["reclen"] == want.size, name
        assert np.array_equal(recs, want), name
        assert clipped == 0 and nans == 0
    # the planted ties of case 2 round half to even, both signs
    rec0 = cases["c2"][2][256 + 256 * 3:].view("<i2")[100:116]
    assert rec0.tolist() == [0, 2, 2, 4, 100, 102, 32766, 32766, 0, -2, -2, -4, -100, -102, -32766, -32768]


def test_restatement_saturates_and_counts():
    x = np.array([40000.0, -40000.0, np.inf, -np.inf, np.nan, 32767.4, -32768.5, 1.5])
    recs, clipped, nans = encode_numpy([x], [8], [1.0], [0.0], 1)
    assert recs.tolist() == [32767, -32768, 32767, -32768, 0, 32767, -32768, 2]
    assert (clipped, nans) == (4, 1)
