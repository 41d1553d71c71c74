"""EDF reader and writer whose record decode and encode run on the device (SURVEY
section 8f rank 3).

Host side: header parsing and record location, same interface and semantics
as the reference's ``file_io/edf.py`` (``Header`` :111-314, ``Reader``
:317-586): ``Reader(path)``, ``.header``, ``.channels`` (settable), ``.shape``,
``.read(start, stop=None, padvalue=nan)``, ``open()`` / ``close()`` and context
management.  Device side: the little-endian int16 records are uploaded as they
are (2 B per sample over PCIe instead of 8) and de-interleaved + scaled by
``osz_edf_decode``.  ``read(..., device=True)`` returns a CUDA tensor so that a
``producer(reader, chunksize, axis=-1, device=True)`` chain never holds float64
samples on the host.

``Writer`` / ``splitter`` (reference :591-808) are the mirror image: physical float64
samples become the file's int16 records in ``osz_edf_encode`` and leave the device at 2 B
per sample.  ``Writer.write`` takes an ndarray, a CUDA tensor, this module's ``Reader`` or
a ``Producer``; ``header_bytes`` and ``record_plan`` are its host logic and need no GPU.
Annotation signals are not written (the reference does not write them either).
"""

import copy
import ctypes
import warnings
from pathlib import Path

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib


class Header(dict):
    """Dictionary of the EDF header fields with '.' access (reference
    file_io/bases.py:26-120, file_io/edf.py:111-314)."""

    def __init__(self, path):
        self.path = Path(path) if path else None
        dict.__init__(self)
        self.update(self.read())

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as exc:
            raise AttributeError(
                f"'{type(self).__name__}' object has no attribute '{name}'") from exc

    def bytemap(self, num_signals=None):
        """Field -> ([byte counts], type) of the EDF specification
        (edf.py:123-162)."""
        ns = self.count_signals() if num_signals is None else num_signals
        return {
            "version": ([8], str), "patient": ([80], str), "recording": ([80], str),
            "start_date": ([8], str), "start_time": ([8], str),
            "header_bytes": ([8], int), "reserved_0": ([44], str),
            "num_records": ([8], int), "record_duration": ([8], float),
            "num_signals": ([4], int),
            "names": ([16] * ns, str), "transducers": ([80] * ns, str),
            "physical_dim": ([8] * ns, str),
            "physical_min": ([8] * ns, float), "physical_max": ([8] * ns, float),
            "digital_min": ([8] * ns, float), "digital_max": ([8] * ns, float),
            "prefiltering": ([80] * ns, str),
            "samples_per_record": ([8] * ns, int), "reserved_1": ([32] * ns, str),
        }

    def count_signals(self):
        if not self.path:
            return int(self["num_signals"])
        with open(self.path, "rb") as fp:
            fp.seek(252)
            return int(fp.read(4).strip().decode())

    def read(self, encoding="ascii"):
        header = {}
        if not self.path:
            return header
        with open(self.path, "rb") as fp:
            for name, (nbytes, dtype) in self.bytemap().items():
                res = [dtype(fp.read(n).strip().decode(encoding=encoding))
                       for n in nbytes]
                # per-signal fields stay lists even for a single signal
                header[name] = res[0] if len(nbytes) == 1 and name not in _PER_SIGNAL else res
        return header

    @classmethod
    def from_dict(cls, dic):
        """A Header without a file that holds ``dic`` (edf.py:183-198); the keys must be
        exactly the bytemap's."""
        instance = cls(path=None)
        instance.update(dic)
        if set(dic) == set(instance.bytemap(1)):
            return instance
        raise ValueError("Missing keys required to create a header of type {}.".format(cls.__name__))

    # -- derived quantities (edf.py:200-300)
    @property
    def annotated(self):
        return "EDF Annotations" in self.names

    @property
    def annotation(self):
        return self.names.index("EDF Annotations") if self.annotated else None

    @property
    def channels(self):
        signals = list(range(self.num_signals))
        if self.annotation:
            signals.pop(self.annotation)
        return signals

    @property
    def samples(self):
        samples = np.array(self.samples_per_record) * self.num_records
        return [samples[ch] for ch in self.channels]

    @property
    def record_map(self):
        cum = np.cumsum(np.insert(self.samples_per_record, 0, 0))
        return [slice(a, b) for a, b in zip(cum, cum[1:])]

    @property
    def slopes(self):
        ch = self.channels
        pmax, pmin = np.array(self.physical_max)[ch], np.array(self.physical_min)[ch]
        dmax, dmin = np.array(self.digital_max)[ch], np.array(self.digital_min)[ch]
        return (pmax - pmin) / (dmax - dmin)

    @property
    def offsets(self):
        ch = self.channels
        pmin, dmin = np.array(self.physical_min)[ch], np.array(self.digital_min)[ch]
        return pmin - self.slopes * dmin

    def filter(self, indices):
        header = copy.deepcopy(self)
        for key, value in header.items():
            if isinstance(value, list):
                header[key] = [value[idx] for idx in indices]
        bytemap = self.bytemap(len(indices))
        header["header_bytes"] = sum(sum(tup[0]) for tup in bytemap.values())
        header["num_signals"] = len(indices)
        return header


_PER_SIGNAL = {"names", "transducers", "physical_dim", "physical_min", "physical_max",
               "digital_min", "digital_max", "prefiltering", "samples_per_record",
               "reserved_1"}


class Reader:
    """Reader of EDF / EDF+ data records (reference edf.py:317-586) with the
    decode on the device."""

    def __init__(self, path):
        self.path = Path(path)
        self.mode = "rb"
        self._fobj = open(self.path, self.mode)
        self.header = Header(path)
        self._channels = self.header.channels

    # -- file handle (file_io/bases.py Reader)
    def open(self):
        if self._fobj is None or self._fobj.closed:
            self._fobj = open(self.path, self.mode)

    def close(self):
        if self._fobj and not self._fobj.closed:
            self._fobj.close()

    def __enter__(self):
        return self

    # a reader travels between processes closed; it reopens on first use
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_fobj"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    def __exit__(self, exc_type, exc_value, traceback):
        self.close()

    @property
    def channels(self):
        return self._channels

    @channels.setter
    def channels(self, values):
        if not isinstance(values, (list, tuple, range)):
            raise ValueError("Channels must be type Sequence not {}".format(type(values)))
        self._channels = values

    @property
    def shape(self):
        return len(self.channels), max(self.header.samples)

    # -- record location (edf.py:421-483), pure host logic
    def plan(self, start, stop, channels):
        """Everything ``read`` needs besides the bytes: the union record range
        to load and, per channel, where its samples sit and how many it can
        deliver (a channel with a lower sample rate runs out first)."""
        hdr = self.header
        spr_all = np.array(hdr.samples_per_record)
        spr = spr_all[list(channels)]
        nrec = hdr.num_records
        r0 = start // spr
        r1 = np.minimum(np.ceil(stop / spr).astype(int), nrec)
        a = start - r0 * spr
        avail = np.maximum(r1 - r0, 0) * spr
        lens = np.maximum(np.minimum(a + (stop - start), avail) - a, 0)
        rec0 = int(min(r0.min(), nrec))
        rec1 = int(max(r1.max(), rec0))
        choff = np.cumsum(np.insert(spr_all, 0, 0))[list(channels)]
        return {"rec0": rec0, "nrec": rec1 - rec0, "reclen": int(spr_all.sum()),
                "spr": spr.astype(np.int32), "choff": choff.astype(np.int32),
                "len": lens.astype(np.int64), "width": int(lens.max()) if len(lens) else 0}

    def _records(self, a, cnt):
        """Raw int16 records [a, a + cnt) exactly as stored (edf.py:452-483)."""
        hdr = self.header
        reclen = sum(hdr.samples_per_record)
        offset = hdr.header_bytes + a * reclen * 2
        self._fobj.seek(0)
        raw = np.fromfile(self._fobj, "<i2", cnt * reclen, offset=offset)
        if raw.size != cnt * reclen:
            # a file shorter than its header says (an interrupted recording): the decode would
            # index past the end of what was read; the reference's reshape raises here too
            raise ValueError(
                "{}: records [{}, {}) hold {} samples according to the header, the file has {} "
                "of them".format(self.path, a, a + cnt, cnt * reclen, raw.size))
        return raw

    def read(self, start, stop=None, padvalue=np.nan, device=False):
        """Samples [start, stop) of this reader's channels as a float64
        (channels, samples) array (edf.py:558-586); ``device=True`` returns a
        CUDA tensor instead of an ndarray.  ValueError, before the device is
        touched, when the file ends before the records the read needs."""
        import torch
        nchan = len(self.channels)
        if start > max(self.header.samples):
            empty = np.empty((nchan, 0))
            return torch.from_numpy(empty).cuda() if device else empty
        if not stop:
            stop = max(self.header.samples)
        start, stop = int(start), int(stop)
        self.open()
        p = self.plan(start, stop, self.channels)
        records = self._records(p["rec0"], p["nrec"])      # raises on a truncated file
        lib = dev.require_gpu()
        if p["width"] == 0:        # nothing to decode, and an empty tensor has no address
            out = torch.empty((nchan, 0), dtype=torch.float64, device="cuda")
            return out if device else out.cpu().numpy()
        idx = [self.header.channels.index(c) for c in self.channels]
        raw = torch.from_numpy(records).cuda()
        t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        choff, spr, lens = t(p["choff"]), t(p["spr"]), t(p["len"])
        slope, offset = t(self.header.slopes[idx]), t(self.header.offsets[idx])
        out = torch.empty((nchan, p["width"]), dtype=torch.float64, device="cuda")
        _lib.check(lib.osz_edf_decode(
            dev.ptr(raw), p["reclen"], nchan, dev.ptr(choff), dev.ptr(spr),
            dev.ptr(slope), dev.ptr(offset), dev.ptr(lens), p["rec0"], start,
            p["width"], ctypes.c_double(padvalue), dev.ptr(out),
            max(out.stride(0), 1), dev.stream_ptr()))
        return out if device else out.cpu().numpy()


# ---------------------------------------------------------------------------
# writing (reference edf.py:591-808)
# ---------------------------------------------------------------------------
GROUP_BYTES = 32 << 20     # int16 bytes encoded per launch = size of each pinned buffer


def header_bytes(header):
    """The ASCII header section of the file a (filtered) ``Header`` describes, as the
    reference's ``Writer._write_header`` writes it (edf.py:619-641): ``str(item)`` of every
    value, left-justified to the width of its field.  (Fields are looked up by name; the
    reference pairs the dictionary's values with the bytemap by position.)"""
    parts = []
    for name, (nbytes, _) in header.bytemap(header["num_signals"]).items():
        items = header[name]
        items = items if isinstance(items, list) else [items]
        parts.extend(bytes(str(item), encoding="ascii").ljust(n) for item, n in zip(items, nbytes))
    return b"".join(parts)


def _plan_of(header, group_bytes=None):
    """The record plan of an already filtered header."""
    spr = np.array(header["samples_per_record"], dtype=np.int64).reshape(-1)
    if spr.size == 0 or spr.min() < 1:
        raise ValueError("every written signal needs samples_per_record >= 1")
    pmax, pmin = np.array(header["physical_max"], float), np.array(header["physical_min"], float)
    dmax, dmin = np.array(header["digital_max"], float), np.array(header["digital_min"], float)
    slope = (pmax - pmin) / (dmax - dmin)          # Header.slopes / .offsets over every signal
    offset = pmin - slope * dmin
    reclen, nrec = int(spr.sum()), int(header["num_records"])
    cap = GROUP_BYTES if group_bytes is None else group_bytes
    return {"spr": spr.astype(np.int32),
            "choff": np.cumsum(np.insert(spr, 0, 0))[:-1].astype(np.int32),
            "reclen": reclen, "nrec": nrec, "group": max(1, min(cap // (2 * reclen), nrec)),
            "slope": slope.reshape(-1), "offset": offset.reshape(-1)}


def record_plan(header, channels, group_bytes=None):
    """What the encode of ``channels`` of a file described by ``header`` (a mapping with the
    bytemap's keys) needs besides the samples: per written signal ``spr`` (samples per record),
    ``choff`` (offset inside an output record), ``slope`` and ``offset``; ``reclen`` = sum of
    spr, ``nrec``, and ``group``, the records encoded per launch (at most ``group_bytes`` of
    int16, default ``GROUP_BYTES``, so memory does not grow with the file).  Pure host logic."""
    return _plan_of(Header.from_dict(header).filter(list(channels)), group_bytes)


def _progression(channels):
    """(first, stop, step) when ``channels`` is an ascending arithmetic progression -- rows a
    view can select -- else None."""
    step = channels[1] - channels[0] if len(channels) > 1 else 1
    if step > 0 and list(channels) == list(range(channels[0], channels[-1] + 1, step)):
        return channels[0], channels[-1] + 1, step
    return None


class _Encoder:
    """Device side of one ``Writer.write``: encodes groups of whole records into an int16
    device buffer, copies each to one of two pinned host buffers on the current stream and
    writes the previous buffer to the file while the next group encodes."""

    def __init__(self, fobj, plan, progress):
        import torch
        dev.require_gpu()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.spr, self.choff = up(plan["spr"]), up(plan["choff"])
        self.slope, self.offset = up(plan["slope"]), up(plan["offset"])
        self.reclen, self.group, self.nrec = plan["reclen"], plan["group"], plan["nrec"]
        cap = self.group * self.reclen
        self.dout = torch.empty(cap, dtype=torch.int16, device="cuda")
        self.hbuf = [torch.empty(cap, dtype=torch.int16, pin_memory=True) for _ in range(2)]
        self.events = [torch.cuda.Event() for _ in range(2)]
        self.counter = dev.zeros(2, torch.int64)
        self.fobj, self.progress = fobj, progress
        self.pending, self.turn, self.done = None, 0, 0

    def encode(self, x2d, nrec, carry=None, h=None):
        """The next ``nrec`` (<= group) records from the rows ``carry[:, :h]`` + ``x2d``."""
        if self.done + nrec > self.nrec:
            raise ValueError("the data goes on past num_records records")
        slot, n = self.turn % 2, nrec * self.reclen
        self.turn += 1
        dev.edf_encode(x2d, self.spr, self.choff, self.slope, self.offset, self.reclen, nrec,
                       self.dout, self.counter, carry=carry, h=h)
        self.hbuf[slot][:n].copy_(self.dout[:n], non_blocking=True)
        self.events[slot].record()
        self._drain()                      # the previous group goes to the file meanwhile
        self.pending = (slot, n)
        self.done += nrec
        self.progress(self.done)

    def _drain(self):
        if self.pending is not None:
            slot, n = self.pending
            self.events[slot].synchronize()
            self.fobj.write(self.hbuf[slot][:n].numpy())
            self.pending = None

    def finish(self):
        """Writes what is still in flight; (saturated, NaN) counts of the whole write."""
        self._drain()
        clipped, nans = self.counter.cpu().tolist()
        return int(clipped), int(nans)


class Writer:
    """Writer of EDF files (reference edf.py:591-777, file_io/bases.py:228-270): a context
    manager that opens ``path`` in 'wb' on entry; the record encode runs on the device.
    Annotation signals are not written."""

    def __init__(self, path):
        self.path = Path(path)
        self.mode = "wb"
        self._fobj = None

    def __enter__(self):
        self._fobj = open(self.path, self.mode)
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        if self._fobj:
            self._fobj.close()
            self._fobj = None

    def _progress(self, done):
        msg = "Writing data: {:.1f}% complete"
        print(msg.format(done / self.header.num_records * 100), end="\r", flush=True)

    def write(self, header, data, channels, verbose=True):
        """Writes ``header`` filtered to ``channels`` and the records of those channels.

        ``data``: an ndarray or CUDA tensor (all channels, samples) -- row ``channels[i]`` is
        signal i, its first ``spr[i] * num_records`` samples are used --, this module's
        ``Reader``, or a 2-D ``Producer`` with samples along its axis whose written channels
        share one samples_per_record.  ValueError when the sample count is not divisible by
        ``num_records``, and when a producer's stream is not ``spr * num_records`` long.  One
        RuntimeWarning when values saturated at the int16 range or were NaN."""
        from openseize_amd.core.producer import Producer
        header = Header.from_dict(header).filter(list(channels))
        channels = list(channels)
        streamed = isinstance(data, Producer)
        nsamples = data.shape[data.axis] if streamed else data.shape[1]
        if nsamples % header.num_records != 0:
            raise ValueError("Number of data samples must be divisible by the number of records; "
                             "{} % {} != 0".format(nsamples, header.num_records))
        plan = _plan_of(header)
        if streamed and (len(data.shape) != 2 or len(set(plan["spr"].tolist())) > 1):
            raise ValueError("a Producer is written only as 2-D data whose channels all have equal "
                             "samples_per_record; got shape {} and samples_per_record {}".format(
                                 tuple(data.shape), plan["spr"].tolist()))
        if not streamed and not dev.is_arraylike(data) and not hasattr(data, "read"):
            raise TypeError("cannot write data of type {}".format(type(data)))
        self.header = header
        self._fobj.seek(0)
        self._fobj.write(header_bytes(header))
        self._fobj.seek(header.header_bytes)
        enc = _Encoder(self._fobj, plan, self._progress if verbose else (lambda done: None))
        if streamed:
            self._from_producer(enc, data, channels, plan)
        elif dev.is_arraylike(data):
            self._from_array(enc, data, channels, plan)
        else:
            self._from_reader(enc, data, channels, plan)
        clipped, nans = enc.finish()
        if clipped or nans:
            warnings.warn("EDF write: {} values lay outside the digital range and were written as "
                          "-32768 / 32767, {} values were NaN and were written as 0".format(clipped, nans),
                          RuntimeWarning, stacklevel=2)

    # -- sources
    @staticmethod
    def _from_array(enc, data, channels, plan):
        import torch
        spr, nrec = plan["spr"].astype(np.int64), plan["nrec"]
        if data.shape[1] < int(spr.max()) * nrec:
            raise ValueError("data holds {} samples per row, {} records of {} need {}".format(
                data.shape[1], nrec, int(spr.max()), int(spr.max()) * nrec))
        rows = _progression(channels)
        view = (rows is not None and dev.is_tensor(data) and data.is_cuda and spr.min() == spr.max()
                and data.dtype == torch.float64 and data.stride(1) == 1)
        for r0 in range(0, nrec, plan["group"]):
            r1 = min(r0 + plan["group"], nrec)
            if view:      # the group is a block of the resident tensor: nothing is copied
                x2d = data[rows[0]:rows[1]:rows[2], r0 * int(spr[0]):r1 * int(spr[0])]
            else:
                width = int(spr.max()) * (r1 - r0)
                if dev.is_tensor(data):
                    stage = torch.empty((len(channels), width), dtype=torch.float64, device=data.device)
                else:
                    stage = np.empty((len(channels), width))
                for i, ch in enumerate(channels):
                    stage[i, :(r1 - r0) * spr[i]] = data[ch, r0 * spr[i]:r1 * spr[i]]
                x2d = (stage if dev.is_tensor(stage) else torch.from_numpy(stage)).cuda()
            enc.encode(x2d, r1 - r0)

    @staticmethod
    def _from_reader(enc, reader, channels, plan):
        """Large spans per group of equal-rate channels, decoded and encoded on the device.  The
        reader's ``channels`` are the caller's again afterwards (the reference leaves the last
        written channel set, edf.py:673)."""
        import torch
        spr, nrec = plan["spr"].astype(np.int64), plan["nrec"]
        rates = sorted(set(spr.tolist()))
        keep = reader.channels
        try:
            for r0 in range(0, nrec, plan["group"]):
                r1 = min(r0 + plan["group"], nrec)
                if len(rates) == 1:
                    reader.channels = channels
                    x2d = reader.read(r0 * rates[0], r1 * rates[0], device=True)
                else:
                    x2d = torch.empty((len(channels), (r1 - r0) * rates[-1]), dtype=torch.float64,
                                      device="cuda")
                    for rate in rates:
                        rows = [i for i, s in enumerate(spr) if s == rate]
                        reader.channels = [channels[i] for i in rows]
                        x2d[rows, :(r1 - r0) * rate] = reader.read(r0 * rate, r1 * rate, device=True)
                enc.encode(x2d, r1 - r0)
        finally:
            reader.channels = keep

    @staticmethod
    def _from_producer(enc, pro, channels, plan):
        """Chunks do not end on record boundaries: what is left of a chunk (fewer than spr samples
        per row) is copied to a carry buffer that the next launch reads in front of the next chunk.
        Nothing of a chunk is referenced once the next one has been asked for."""
        import torch
        spr, nrec, axis = int(plan["spr"][0]), plan["nrec"], pro.axis % 2
        rows = _progression(channels)
        carry = torch.empty((len(channels), spr), dtype=torch.float64, device="cuda")
        hdev = torch.zeros(len(channels), dtype=torch.int32, device="cuda")
        h, total = 0, 0
        wrong = ("the producer's shape {} does not describe its stream: {{}} where {} records of {} "
                 "samples were announced").format(tuple(pro.shape), nrec, spr)
        for chunk in dev.pull_resident(pro, pro):
            if dev.is_tensor(chunk):
                t = chunk.movedim(axis, -1)
                t = t[rows[0]:rows[1]:rows[2]] if rows is not None else t[channels]
                t = t.to(device="cuda", dtype=torch.float64)
                x2d = t if t.shape[1] <= 1 or t.stride(1) == 1 else t.contiguous()
            else:
                picked = np.moveaxis(np.asarray(chunk), axis, -1)[channels]
                x2d = torch.from_numpy(np.ascontiguousarray(picked, dtype=np.float64)).cuda()
            m, at = x2d.shape[1], 0
            total += m
            if total > spr * nrec:
                raise ValueError(wrong.format("it goes on past them"))
            while h + m - at >= spr:
                k = min((h + m - at) // spr, enc.group)
                if h:
                    hdev.fill_(h)
                    enc.encode(x2d[:, at:], k, carry=carry, h=hdev)
                else:
                    enc.encode(x2d[:, at:], k)
                at += k * spr - h
                h = 0
            if m > at:                     # the remainder: a copy, the chunk itself is let go
                carry[:, h:h + m - at].copy_(x2d[:, at:])
                h += m - at
        if total != spr * nrec:
            raise ValueError(wrong.format("it ends after {} samples".format(total)))


def splitter(path, mapping, outdir=None):
    """Writes one EDF per entry ``filename: channel indices`` of ``mapping`` from the EDF at
    ``path`` (reference edf.py:780-808); the source file is left as it is."""
    reader = Reader(path)
    outdir = Path(outdir) if outdir else reader.path.parent
    try:
        for fname, indices in mapping.items():
            target = outdir.joinpath(Path(fname).with_suffix(".edf"))
            with Writer(target) as outfile:
                outfile.write(reader.header, reader, indices)
    finally:
        reader.close()
