"""Which sources hand on chunks that stay put: the one policy on the memory of a chunk.

A chunk handed on by a source may be rewritten once its consumer pulls the next chunk.  That is
the ordinary iterator contract, and the normal way to stream from a file, an acquisition device
or a decoder: fill one buffer, yield it, fill it again on the next ``next()``.  The stream code
joins neighbouring chunks into one launch, reads ahead, and keeps chunks by reference to read
them again when a non-finite sample turns up.  It may do so only for sources whose chunks are
known never to be rewritten, and ``stays_put`` is the one place that says which those are:

* an ``ArrayProducer`` (views of one array or tensor);
* a ``GenProducer``: it yields memory of its own (a copy of what its function yields, unless
  ``fresh_output`` says that is already new memory);
* a ``MaskedProducer`` (it gathers);
* a ``ReaderProducer`` over this library's EDF reader (every read is a new array).

Any other source is foreign, a user's ``Producer`` subclass included: each of its chunks is
pushed before the next one is pulled, and whatever must be kept is copied.
"""

_FRESH = set()      # generating functions of this library that write every chunk into new memory
_RELAY = set()      # generating functions of this library that hand on their source's own chunks


def fresh(fn):
    """Marks a generating function whose every yielded chunk is new memory (the computing
    generators: the filters, resampling, spectra, the arithmetic of protools)."""
    _FRESH.add(fn)
    return fn


def relay(fn):
    """Marks a generating function ``fn(pro, ...)`` that hands on chunks of its source ``pro``,
    or views of them (padding along the stream, squeeze, slicing)."""
    _RELAY.add(fn)
    return fn


def fresh_output(func):
    """Does the generating function ``func`` (bare, a ``functools.partial`` or a bound method)
    yield memory that nobody writes again: new memory, or the chunks of a source whose chunks
    stay put?"""
    fn = getattr(func, "func", func)
    fn = getattr(fn, "__func__", fn)
    if fn in _FRESH:
        return True
    if fn in _RELAY:
        args = getattr(func, "args", ())
        return bool(args) and stays_put(args[0])
    return False


def stays_put(pro):
    """Are the chunks ``pro`` hands on never written again, so that they may be joined, read
    ahead of their consumer and kept by reference?  Objects that pass another producer's chunks
    on unchanged name it in ``relays``."""
    from openseize_amd.core.producer import ArrayProducer, GenProducer, MaskedProducer, ReaderProducer
    while getattr(pro, "relays", None) is not None:
        pro = pro.relays
    if isinstance(pro, (ArrayProducer, GenProducer, MaskedProducer)):
        return True
    if isinstance(pro, ReaderProducer):
        from openseize_amd.file_io.edf import Reader
        return isinstance(pro.data, Reader)
    return False
