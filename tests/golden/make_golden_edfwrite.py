"""Generate tests/golden/g22_edf_write.npz by RUNNING the reference EDF Writer / splitter.

Run with the reference openseize package importable (tests never import it):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<openseize checkout>/src \
        python3 tests/golden/make_golden_edfwrite.py

Only data is written: seeded inputs, the header dictionaries handed to the reference (as JSON
text: the fixture is loaded without pickling) and the bytes of the files the reference wrote.

  case 1  the reference Writer on the reference Reader of tests/golden/synthetic.edf
      c1_header           JSON of reader.header (shared by cases 1 and 3)
      c1_file_023         the file written for channels [0, 2, 3] (rates 500 / 250 / 500)
      c1_file_1           the file written for channels [1]
  case 2  the reference Writer on a float64 ndarray, 3 rows, spr 100 / 100 / 50, 12 records
      c2_header           JSON of the header dictionary
      c2_data             (3, 1200) float64; row 2 uses its first 600 samples.  Rows 0 and 2 are
                          uniform inside their physical range with physical_min / physical_max
                          planted; row 1 has physical == digital range (slope 1, offset 0) and
                          starts with the exact ties k + 0.5, k even and odd, both signs
      c2_file             the file written for channels [0, 1, 2]
  case 3  the reference splitter on synthetic.edf, mapping {"left": [0, 1], "right.edf": [3, 2]}
      c3_names, c3_channels   file stems and their channel lists (one row each)
      c3_file_left, c3_file_right

Every (x - offset) / slope fed to the reference lies in [-32768, 32767] and the reference raised
no warning (both asserted), so the fixture pins only behaviour the reference defines.
"""

import json
import os
import tempfile
import warnings

import numpy as np

from openseize.file_io import edf as ref_edf

OUT = os.path.dirname(os.path.abspath(__file__))
SYNTHETIC = os.path.join(OUT, "synthetic.edf")


def file_bytes(path):
    return np.fromfile(path, dtype=np.uint8)


def written(header, data, channels, tmp, name):
    path = os.path.join(tmp, name)
    with ref_edf.Writer(path) as writer:
        writer.write(header, data, channels, verbose=False)
    return file_bytes(path)


def case2():
    rng = np.random.default_rng(2201)
    nrec, spr = 12, [100, 100, 50]
    pmin, pmax = [-3276.8, -32768.0, -200.0], [3276.7, 32767.0, 250.0]
    header = {
        "version": "0", "patient": "golden patient", "recording": "golden recording",
        "start_date": "01.01.26", "start_time": "00.00.00", "header_bytes": 256 + 256 * 3,
        "reserved_0": "", "num_records": nrec, "record_duration": 1.0, "num_signals": 3,
        "names": ["EEG A", "EEG ties", "EMG slow"], "transducers": ["AgAgCl"] * 3,
        "physical_dim": ["uV"] * 3, "physical_min": pmin, "physical_max": pmax,
        "digital_min": [-32768.0] * 3, "digital_max": [32767.0] * 3,
        "prefiltering": ["HP:0.1Hz"] * 3, "samples_per_record": spr, "reserved_1": [""] * 3}
    x = np.stack([rng.uniform(lo, hi, size=nrec * 100) for lo, hi in zip(pmin, pmax)])
    x[0, [0, 5, 1199]] = [pmin[0], pmax[0], pmin[0]]
    x[2, [1, 7, 599]] = [pmax[2], pmin[2], pmax[2]]
    ks = np.array([0, 1, 2, 3, 100, 101, 32765, 32766, -1, -2, -3, -4, -101, -102, -32767, -32768])
    x[1, :ks.size] = ks + 0.5
    x[1, ks.size:ks.size + 2] = [pmin[1], pmax[1]]
    hdr = ref_edf.Header.from_dict(header)
    for c in range(3):
        d = (x[c, :spr[c] * nrec] - hdr.offsets[c]) / hdr.slopes[c]
        assert d.min() >= -32768 and d.max() <= 32767, (c, d.min(), d.max())
    assert hdr.slopes[1] == 1.0 and hdr.offsets[1] == 0.0
    return header, x


def main():
    out = {}
    with warnings.catch_warnings(), tempfile.TemporaryDirectory() as tmp:
        warnings.simplefilter("error")
        with ref_edf.Reader(SYNTHETIC) as reader:
            header = dict(reader.header)
            out["c1_header"] = np.array(json.dumps(header))
            out["c1_file_023"] = written(reader.header, reader, [0, 2, 3], tmp, "a.edf")
            out["c1_file_1"] = written(reader.header, reader, [1], tmp, "b.edf")
        # (checked where the fixture is made: the records are the source's own int16 columns)
        raw = np.fromfile(SYNTHETIC, "<i2", offset=header["header_bytes"]).reshape(20, -1)
        cols = np.r_[0:500, 1000:1250, 1250:1750]
        assert np.array_equal(out["c1_file_023"][1024:].view("<i2").reshape(20, -1), raw[:, cols])
        h2, x2 = case2()
        out["c2_header"] = np.array(json.dumps(h2))
        out["c2_data"] = x2
        out["c2_file"] = written(h2, x2, [0, 1, 2], tmp, "c.edf")
        mapping = {"left": [0, 1], "right.edf": [3, 2]}
        ref_edf.splitter(SYNTHETIC, mapping, outdir=tmp)
        out["c3_names"] = np.array(["left", "right"])
        out["c3_channels"] = np.array([[0, 1], [3, 2]])
        out["c3_file_left"] = file_bytes(os.path.join(tmp, "left.edf"))
        out["c3_file_right"] = file_bytes(os.path.join(tmp, "right.edf"))
    path = os.path.join(OUT, "g22_edf_write.npz")
    np.savez_compressed(path, **out)
    print(f"g22_edf_write.npz: {os.path.getsize(path) / 1e3:.0f} kB, {len(out)} arrays")


if __name__ == "__main__":
    main()
