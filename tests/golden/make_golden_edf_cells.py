"""Generate tests/golden/g11_edf_cells.npz by RUNNING the reference EDF Reader on the tiny files of
tests/edf_cells.py.

Run with the reference openseize package importable (tests never import it):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<openseize checkout>/src \
        python3 tests/golden/make_golden_edf_cells.py

Only results are written.  For every geometry <g> of edf_cells.GEOMETRIES the cells of
edf_cells.cells() -- (channels, padvalue, start, stop), in that generator's order -- are read with the
reference Reader from a file that edf_cells.write_geometry() writes to a temporary directory:

    <g>_ok      (ncells,) bool   True where the reference returned an array.  It raises IndexError on
                                 every read of a single-signal file and on a channel that follows an
                                 annotation signal in mid-file; those cells hold nothing
    <g>_shape   (ncells, 2) int  shape of each result, (0, 0) where not ok
    <g>_flat    float64          the results of the ok cells, flattened, one after the other
"""

import os
import sys
import tempfile

import numpy as np

from openseize.file_io import edf as ref_edf

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

import edf_cells as ec  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(ec.GEOMETRIES):
            path = os.path.join(tmp, name + ".edf")
            ec.write_geometry(path, name)
            f = ec.parse_edf(path)
            ok, shapes, flat = [], [], []
            with ref_edf.Reader(path) as reader:
                for chans, pad, a, b in ec.cells(f):
                    reader.channels = chans
                    try:
                        got = reader.read(a, b, padvalue=pad)
                    except IndexError:
                        ok.append(False)
                        shapes.append((0, 0))
                        continue
                    assert got.dtype == np.float64 and got.ndim == 2
                    ok.append(True)
                    shapes.append(got.shape)
                    flat.append(got.reshape(-1))
            out[name + "_ok"] = np.array(ok)
            out[name + "_shape"] = np.array(shapes, dtype=np.int64)
            out[name + "_flat"] = np.concatenate(flat) if flat else np.empty(0)
            print(f"{name}: {len(ok)} cells, {int(np.sum(ok))} read by the reference")
    path = os.path.join(OUT, "g11_edf_cells.npz")
    np.savez_compressed(path, **out)
    print(f"g11_edf_cells.npz: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
