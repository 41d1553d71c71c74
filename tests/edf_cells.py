"""The files, the cells and the restatement of the EDF Reader and its device decode (file_io/edf.py
Reader.plan / Reader.read, csrc/misc.hip osz_edf_decode), shared by tests/test_edf_cells_host.py,
tests/test_gpu_edf_cells.py and the fixture recipe tests/golden/make_golden_edf_cells.py.  NumPy only.

* write_edf: an EDF written byte by byte from the published layout (256-byte fixed header, 256 bytes per
  signal, little-endian int16 records), optionally cut short by a number of trailing bytes.
* parse_edf: the same layout read back, for the restatement only.
* edf_read: Reader.read restated from the layout.  Per channel its own samples [start, stop) are sliced out
  of the records; the channels that run out first are padded with padvalue BEFORE the map; the map is
  arr * slope followed by + offset, two roundings.
* GEOMETRIES / cells: the tiny files and the (channels, padvalue, start, stop) cells swept over them.  Every
  (start, stop) with 0 <= start <= max + 2 and stop in {None} u [start, max + 4] is a cell, max being the
  longest channel, so every record edge, the end of every channel and the first samples past the end are
  met with every offset in front of them.
* decode_blocks: gridDim.x of osz_edf_decode (256 threads, at most kEdfMaxBlk = 2048 blocks), restated so
  that the GPU test's large file can be shown to send the grid-stride loop round twice.
"""

import numpy as np

EDF_THREADS, EDF_MAXBLK = 256, 2048      # osz_edf_decode: threads per block, cap of gridDim.x
ANNOTATION = "EDF Annotations"


def decode_blocks(width):
    return min(-(-width // EDF_THREADS), EDF_MAXBLK)


def decode_trips(width):
    """The most trips a thread of edf_decode_kernel's grid-stride loop makes."""
    return -(-width // (decode_blocks(width) * EDF_THREADS)) if width else 0


# ------------------------------------------------------------------ writing and parsing the layout
def _field(val, width):
    text = str(val)
    assert len(text) <= width, (val, width)
    return text.ljust(width).encode("ascii")


def payload(spr, nrec, seed):
    """Seeded int16 records (nrec, sum(spr)) that hold -32768 and 32767."""
    rng = np.random.default_rng([seed, nrec] + list(spr))
    recs = rng.integers(-32768, 32768, size=(nrec, sum(spr)), dtype=np.int16)
    recs.flat[0], recs.flat[-1] = -32768, 32767
    if recs.size > 3:
        recs.flat[recs.size // 2], recs.flat[recs.size // 2 + 1] = 32767, -32768
    return recs


def write_edf(path, spr, nrec, names=None, pmin=None, pmax=None, dmin=None, dmax=None, seed=0, drop=0):
    """Writes the file and returns its records (nrec, sum(spr)) int16 as the header announces them; ``drop``
    trailing bytes are left out of the file (the header still says nrec)."""
    ns = len(spr)
    names = names or ["S%d" % i for i in range(ns)]
    pmin = pmin if pmin is not None else [-3276.8] * ns
    pmax = pmax if pmax is not None else [3276.7] * ns
    dmin = dmin if dmin is not None else [-32768] * ns
    dmax = dmax if dmax is not None else [32767] * ns
    assert all(len(v) == ns for v in (names, pmin, pmax, dmin, dmax))
    head = b"".join([
        _field("0", 8), _field("cells patient", 80), _field("cells recording", 80),
        _field("01.01.26", 8), _field("00.00.00", 8), _field(256 + 256 * ns, 8),
        _field("", 44), _field(nrec, 8), _field(1, 8), _field(ns, 4),
        b"".join(_field(n, 16) for n in names),
        b"".join(_field("AgAgCl", 80) for _ in names),
        b"".join(_field("uV", 8) for _ in names),
        b"".join(_field(v, 8) for v in pmin), b"".join(_field(v, 8) for v in pmax),
        b"".join(_field(v, 8) for v in dmin), b"".join(_field(v, 8) for v in dmax),
        b"".join(_field("HP:0.1Hz", 80) for _ in names),
        b"".join(_field(v, 8) for v in spr), b"".join(_field("", 32) for _ in names)])
    assert len(head) == 256 + 256 * ns
    recs = payload(spr, nrec, seed)
    body = recs.astype("<i2").tobytes()
    assert 0 <= drop <= len(body)
    with open(path, "wb") as fp:
        fp.write(head)
        fp.write(body[:len(body) - drop])
    return recs


def parse_edf(path):
    """The layout read back: a dict with names, spr, nrec, pmin, pmax, dmin, dmax (floats as written) and
    recs (nrec, sum(spr)) int16."""
    with open(path, "rb") as fp:
        blob = fp.read()
    nbytes, nrec, ns = int(blob[184:192]), int(blob[236:244]), int(blob[252:256])
    at = 256

    def per_signal(width, conv):
        nonlocal at
        vals = [conv(blob[at + i * width:at + (i + 1) * width].decode("ascii").strip()) for i in range(ns)]
        at += width * ns
        return vals

    names = per_signal(16, str)
    per_signal(80, str), per_signal(8, str)
    pmin, pmax, dmin, dmax = (per_signal(8, float) for _ in range(4))
    per_signal(80, str)
    spr = per_signal(8, int)
    assert nbytes == 256 + 256 * ns
    recs = np.frombuffer(blob, "<i2", nrec * sum(spr), offset=nbytes).reshape(nrec, sum(spr))
    return {"names": names, "spr": spr, "nrec": nrec, "pmin": pmin, "pmax": pmax, "dmin": dmin,
            "dmax": dmax, "recs": recs.astype(np.int16)}


# ------------------------------------------------------------------ the restatement
def header_channels(names):
    """Header.channels: every signal but the annotation signal -- which stays when it is signal 0, as in the
    reference (its test is the truth value of the index)."""
    sig = list(range(len(names)))
    if ANNOTATION in names and names.index(ANNOTATION):
        sig.pop(names.index(ANNOTATION))
    return sig


def longest(f):
    """max(Header.samples): the longest of the header's channels, whatever the reader's channel list."""
    return max(f["spr"][c] * f["nrec"] for c in header_channels(f["names"]))


def resolve(f, start, stop):
    """(start, stop) as Reader.read resolves them, None where it returns (nch, 0) at once: a start past the
    longest channel is empty, a stop of None or 0 means "to the end"."""
    if start > longest(f):
        return None
    if not stop:
        stop = longest(f)
    return int(start), int(stop)


def channel_lengths(f, channels, start, stop):
    """Samples each channel delivers for the resolved [start, stop)."""
    return [len(range(*slice(start, stop).indices(f["spr"][c] * f["nrec"]))) for c in channels]


def edf_read(f, channels, start, stop=None, padvalue=np.nan):
    """Reader.read(start, stop, padvalue) with reader.channels = channels, from the parsed file f."""
    span = resolve(f, start, stop)
    if span is None:
        return np.empty((len(channels), 0))
    start, stop = span
    choff = np.concatenate(([0], np.cumsum(f["spr"])))
    rows = []
    for c in channels:
        own = f["recs"][:, choff[c]:choff[c] + f["spr"][c]].reshape(-1)      # this channel's samples alone
        rows.append(own[start:stop].astype(np.float64))
    width = max(len(r) for r in rows)
    arr = np.full((len(channels), width), padvalue, dtype=np.float64)        # pad first ...
    for i, r in enumerate(rows):
        arr[i, :len(r)] = r
    pmin, pmax = np.array(f["pmin"], float)[channels], np.array(f["pmax"], float)[channels]
    dmin, dmax = np.array(f["dmin"], float)[channels], np.array(f["dmax"], float)[channels]
    slope = (pmax - pmin) / (dmax - dmin)
    offset = pmin - slope * dmin
    with np.errstate(invalid="ignore"):
        res = arr * slope[:, None]                                           # ... then the two roundings
        res += offset[:, None]
    return res


def same(a, b):
    """Bit for bit, as test_gpu_parity.py's same: equal shapes, equal values, NaN equal to NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------ the tiny files and their cells
# name -> (samples_per_record, nrec, names or None).  The physical and digital limits come from LIMITS by
# signal index: an ordinary signal, one with 12-bit asymmetric digital limits, one with a negative slope
# (physical_min > physical_max), one with an asymmetric physical range.
GEOMETRIES = {
    "four_rates": ([4, 2, 3, 1], 3, None),
    "single_signal": ([5], 2, None),
    "equal_rates": ([3, 3], 4, None),
    "annot_last": ([4, 2, 3], 3, ["S0", "S1", ANNOTATION]),
    "annot_middle": ([4, 2, 3], 3, ["S0", ANNOTATION, "S2"]),
    "annot_first": ([4, 2, 3], 3, [ANNOTATION, "S1", "S2"]),
}
LIMITS = {"pmin": [-3276.8, -500.0, 1000.0, -200.0], "pmax": [3276.7, 499.75, -1000.0, 250.0],
          "dmin": [-32768, -2048, -32768, -32767], "dmax": [32767, 2047, 32767, 32767]}
PADVALUES = (0.0, -7.5, np.inf)            # on the all-channels list; NaN everywhere


def write_geometry(path, name, drop=0):
    spr, nrec, names = GEOMETRIES[name]
    lim = {k: v[:len(spr)] for k, v in LIMITS.items()}
    return write_edf(path, spr, nrec, names=names, seed=sorted(GEOMETRIES).index(name), drop=drop, **lim)


def channel_lists(names):
    """All channels, each alone, reversed, one channel twice -- duplicates of these dropped."""
    hc = header_channels(names)
    lists = [hc] + [[c] for c in hc] + [hc[::-1], [hc[0], hc[-1], hc[0]]]
    out = []
    for lst in lists:
        if lst not in out:
            out.append(lst)
    return out


def spans(f):
    """Every (start, stop) of the sweep, stop None first."""
    top = longest(f)
    return [(a, b) for a in range(top + 3) for b in [None] + list(range(a, top + 5))]


def cells(f):
    """(channels, padvalue, start, stop) in the fixed order the fixture is stored in: NaN over every channel
    list, then the other pad values over the all-channels list."""
    lists = channel_lists(f["names"])
    for chans in lists:
        for a, b in spans(f):
            yield chans, np.nan, a, b
    for pad in PADVALUES:
        for a, b in spans(f):
            yield lists[0], pad, a, b


def edge_spans(f):
    """The spans whose start and stop both lie within one sample of a record edge of some signal (or are
    None): what a sweep is trimmed to where the full grid takes too long."""
    near = {0}
    for spr in f["spr"]:
        for r in range(f["nrec"] + 1):
            near.update((r * spr - 1, r * spr, r * spr + 1))
    return [(a, b) for a, b in spans(f) if a in near and (b is None or b in near)]
