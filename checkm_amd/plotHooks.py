"""The names CheckM's plot modules import, answered by the library (checkm_amd.dropin.install binds them into checkm.plot.gcPlots,
gcBiasPlots, codingDensityPlots and tetraDistPlots; dist_plot runs through those three classes).

The plot classes compute inline -- `baseCount(seq[start:end])`, `prodigalParser.codingBases(seqId, start, end)`,
`genomicSig.seqSignature(seq[start:end])` per window -- so what can be replaced is what those expressions touch:

  readFasta                  returns {id: WindowSeq}: str subclasses that hold the real text (every other use of a sequence is unchanged)
  seq[start:end]             of a WindowSeq with two plain integers is a WindowToken (sequence, start, end): no text is copied
  baseCount                  a token on the window grid (start a multiple of w = end - start, end < len(seq): the windows the plot loops
  seqSignature               visit) is answered from a cache that ONE pass of SequenceWindows over the file fills per (file, w), made on
  codingBases                first use; the whole sequence (gc_bias_plot's baseCount(seq)) from the same pass

Anything else -- a plain str, a slice off the grid, a sequence with non-ASCII characters, 4-mer counts that do not fit the batch budget --
is computed by the ordinary implementation, and `fallbacks` counts those calls.
"""
import os

import numpy as np

from checkm_amd import genomicSignatures as _gs
from checkm_amd import prodigal as _pr
from checkm_amd.seqWindows import SequenceWindows, _base_count

fallbacks = 0          # calls answered by the ordinary implementation
library_calls = 0      # passes over a file
_cache = {}            # (file key, w) -> result of SequenceWindows._run
_open = {}             # file key -> the file as the library read it (_lib.NucSeqs), kept while its windows are cached
_last_file = None      # key of the file readFasta read last: codingBases(seqId, start, end) names no sequence object
_NO_WINDOWS = 2 ** 31 - 1


def _forget():
    _cache.clear()
    for seqs in _open.values():
        seqs.close()
    _open.clear()


def reset():
    global fallbacks, library_calls, _last_file
    fallbacks = library_calls = 0
    _last_file = None
    _forget()


class WindowToken(object):
    """seq[start:end] of a WindowSeq, not yet cut."""
    __slots__ = ('seq', 'start', 'end')

    def __init__(self, seq, start, end):
        self.seq, self.start, self.end = seq, start, end

    def text(self):
        return str.__getitem__(self.seq, slice(self.start, self.end))

    def __len__(self):
        return self.end - self.start

    def __str__(self):
        return self.text()

    def __eq__(self, other):
        return self.text() == (other.text() if isinstance(other, WindowToken) else other)

    def __hash__(self):
        return hash(self.text())

    def __getattr__(self, name):                          # any str method: on the text
        return getattr(self.text(), name)


class WindowSeq(str):
    """A sequence of readFasta: the text, and where it came from."""

    def __new__(cls, text, key, index):
        self = str.__new__(cls, text)
        self.key, self.index = key, index
        return self

    def __getitem__(self, k):
        if isinstance(k, slice) and k.step is None and type(k.start) is int and type(k.stop) is int and 0 <= k.start < k.stop <= len(self):
            return WindowToken(self, k.start, k.stop)
        return str.__getitem__(self, k)


def _file_key(path):
    st = os.stat(path)
    return (os.path.abspath(path), st.st_mtime_ns, st.st_size)


def _batch(key):
    from checkm_amd import _lib
    if key not in _open:
        _open[key] = _lib.NucSeqs([key[0]])
    return _open[key]


def readFasta(fastaFile, trimHeader=True):
    """{id: sequence} of checkm.util.seqUtils.readFasta, the sequences as WindowSeq.  The file is read once, by the library, and the
    batch stays open for the passes over its windows."""
    global _last_file
    if not trimHeader:
        raise ValueError('readFasta of the plot modules trims the header')
    key = _file_key(fastaFile)
    if _last_file is not None and key != _last_file:
        _forget()                                         # one file's windows at a time
    _last_file = key
    seqs = _batch(key)
    return {seqId: WindowSeq(seqs.seq(i).decode('utf-8'), key, i) for i, seqId in enumerate(seqs.ids())}


def _entry(key, w, gffFile=None):
    """The pass over file `key` with windows of w, made once; with a GFF file the coding bases per window are added to it."""
    global library_calls
    e = _cache.get((key, w))
    if e is None:
        e = SequenceWindows()._run(key[0], w, gffFile=gffFile, wantTetra=w != _NO_WINDOWS, seqs=_batch(key))
        e['index'] = {seqId: i for i, seqId in enumerate(e['ids'])}
        e['gff'] = gffFile
        library_calls += 1
        _cache[(key, w)] = e
    elif gffFile is not None and e['gff'] != gffFile:
        from checkm_amd import _lib
        e['coding'], e['gff'] = _lib.seq_windows_coding(_batch(key), [gffFile], w)[0], gffFile      # host code over the open batch
    return e


def _whole(key):
    """Any pass over file `key` (every pass carries the whole-sequence counts), else a pass without windows."""
    for (k, _w), e in _cache.items():
        if k == key:
            return e
    return _entry(key, _NO_WINDOWS)


def _slot(token):
    """(entry, window index) of a token on the grid of a sequence the device took, else None."""
    w = token.end - token.start
    if token.start % w or token.end >= len(token.seq) or w > _NO_WINDOWS:
        return None
    e = _entry(token.seq.key, w)
    if e['skipped'][token.seq.index]:
        return None
    return e, e['first'][token.seq.index] + token.start // w


def baseCount(seq):
    global fallbacks
    if isinstance(seq, WindowToken):
        at = _slot(seq)
        if at is not None:
            return tuple(int(x) for x in at[0]['base'][at[1]])
        seq = seq.text()
    elif isinstance(seq, WindowSeq):
        e = _whole(seq.key)
        if not e['skipped'][seq.index]:
            return tuple(int(x) for x in e['seq'][seq.index])
    fallbacks += 1
    return _base_count(seq)


class GenomicSignatures(_gs.GenomicSignatures):
    def seqSignature(self, seq):
        global fallbacks
        if isinstance(seq, WindowToken):
            at = _slot(seq) if self.K == 4 else None
            if at is not None and at[0]['tetra'] is not None:
                sig = np.array(at[0]['tetra'][at[1]], dtype=float)
                with np.errstate(invalid='ignore'):
                    sig /= np.sum(sig)
                return sig
            seq = seq.text()
        fallbacks += 1
        return _gs.GenomicSignatures.seqSignature(self, seq)


class ProdigalGeneFeatureParser(_pr.ProdigalGeneFeatureParser):
    """The window questions go to the library, which parses the GFF file itself; the Python parse of the base class is put off until
    something else is asked (the whole-sequence codingBases of BinTools.codingDensityDist, genes, translationTable, a fallback)."""

    def __init__(self, filename):
        if not os.path.exists(filename):
            _pr.ProdigalGeneFeatureParser.__init__(self, filename)          # the base class's error and exit
        self._gff = filename

    def __getattr__(self, name):                          # only reached for what the put-off parse would have set
        if name.startswith('__') or name == '_gff':
            raise AttributeError(name)
        _pr.ProdigalGeneFeatureParser.__init__(self, self._gff)
        return object.__getattribute__(self, name)

    def codingBases(self, seqId, start=0, end=None):
        global fallbacks
        if end is None:                                   # the whole sequence: BinTools.codingDensityDist, not a window
            return _pr.ProdigalGeneFeatureParser.codingBases(self, seqId, start, end)
        w = end - start
        if _last_file is not None and type(start) is int and type(end) is int and 0 < w <= _NO_WINDOWS and start % w == 0:
            e = _entry(_last_file, w, self._gff)
            s = e['index'].get(seqId)
            if s is not None and e['coding'] is not None and start // w < e['first'][s + 1] - e['first'][s]:
                return int(e['coding'][e['first'][s] + start // w])
        fallbacks += 1
        return _pr.ProdigalGeneFeatureParser.codingBases(self, seqId, start, end)
