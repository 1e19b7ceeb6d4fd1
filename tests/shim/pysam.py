"""TEST INFRASTRUCTURE -- a stand-in for the part of pysam that checkm/coverage.py touches, so that the REFERENCE's own Coverage can run
where pysam is not installed: tools/gen_coverage_golden.py binds `checkm.coverage.pysam` to this module, runs the reference on synthetic
BAM files and records what it writes (tests/golden/coverage_cases.json).  Never imported by checkm_amd.

A plain-Python BAM reader on gzip and struct.  What the reference relies on (checkm/coverage.py:131-133, 193-230):
  Samfile(path, 'rb'): .references, .lengths, .fetch(ref, 0, len), .close()
  read: is_unmapped, is_duplicate, is_secondary, is_supplementary, is_qcfail, is_proper_pair, mapping_quality, query_length,
        query_alignment_length, get_tag(tag)
pysam's semantics as written here are FROM MEMORY of pysam 0.2x (DESIGN section 15 marks each with [pysam-ext]):
  fetch(ref, 0, len) yields every record whose refID is ref, in file order, reads with the unmapped flag placed there included;
  query_length = l_seq;
  query_alignment_length = l_seq - leading soft clips - trailing soft clips (hard clips outside them skipped; the walk from the end
  stops before the first operation); with l_seq == 0 it is the sum of the M, I, = and X lengths and query_length is 0;
  get_tag raises KeyError("tag 'NM' not present") when the tag is absent."""
import gzip
import struct

_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
M, I, S, H, EQ, X = 0, 1, 4, 5, 7, 8


class AlignedSegment(object):
    def __init__(self, data, start, end, ordinal):
        (self.reference_id, self.reference_start, l_name, self.mapping_quality, _bin, n_cigar, self.flag, self.l_seq,
         _nref, _npos, _tlen) = struct.unpack_from("<iiBBHHHiiii", data, start)
        p = start + 32
        self.query_name = data[p:p + l_name - 1].decode("ascii", "replace")
        p += l_name
        self.cigar = [(v & 15, v >> 4) for v in struct.unpack_from("<%dI" % n_cigar, data, p)]
        p += 4 * n_cigar + (self.l_seq + 1) // 2 + self.l_seq
        self._data, self._aux, self._end = data, p, end
        self.ordinal, self.offset = ordinal, start - 4

    is_proper_pair = property(lambda s: bool(s.flag & 0x2))
    is_unmapped = property(lambda s: bool(s.flag & 0x4))
    is_secondary = property(lambda s: bool(s.flag & 0x100))
    is_qcfail = property(lambda s: bool(s.flag & 0x200))
    is_duplicate = property(lambda s: bool(s.flag & 0x400))
    is_supplementary = property(lambda s: bool(s.flag & 0x800))

    @property
    def query_length(self):
        return self.l_seq

    @property
    def query_alignment_length(self):
        c = self.cigar
        if self.l_seq == 0:
            return sum(n for op, n in c if op in (M, I, EQ, X))
        lead = 0
        for op, n in c:
            if op == S:
                lead += n
            elif op != H:
                break
        trail = 0
        for op, n in reversed(c[1:]):
            if op == S:
                trail += n
            elif op != H:
                break
        return self.l_seq - lead - trail

    def get_tag(self, tag):
        d, p, end = self._data, self._aux, self._end
        want = tag.encode("ascii")
        while p + 3 <= end:
            name, typ = d[p:p + 2], chr(d[p + 2])
            p += 3
            if typ in _SIZE:
                n = _SIZE[typ]
                if name == want:
                    return d[p:p + 1].decode("ascii") if typ == "A" else struct.unpack_from(_FMT[typ], d, p)[0]
            elif typ in "ZH":
                n = d.index(b"\0", p, end) - p + 1
                if name == want:
                    return d[p:p + n - 1].decode("ascii")
            elif typ == "B":
                sub = chr(d[p])
                cnt = struct.unpack_from("<i", d, p + 1)[0]
                n = 5 + cnt * _SIZE[sub]
                if name == want:
                    return list(struct.unpack_from("<%d%s" % (cnt, _FMT[sub][1]), d, p + 5))
            else:
                raise ValueError("auxiliary field of unknown type %r" % typ)
            p += n
        raise KeyError("tag '%s' not present" % tag)


class Samfile(object):
    def __init__(self, path, mode="rb"):
        assert mode == "rb"
        with gzip.open(path, "rb") as f:          # (a BGZF file is a series of gzip members)
            data = f.read()
        if data[:4] != b"BAM\1":
            raise ValueError("not a BAM file: " + path)
        l_text = struct.unpack_from("<i", data, 4)[0]
        p = 8 + l_text
        n_ref = struct.unpack_from("<i", data, p)[0]
        p += 4
        names, lengths = [], []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", data, p)[0]
            names.append(data[p + 4:p + 4 + l_name - 1].decode("utf-8"))
            lengths.append(struct.unpack_from("<i", data, p + 4 + l_name)[0])
            p += 8 + l_name
        self.references, self.lengths = tuple(names), tuple(lengths)
        self.header_bytes = p
        self._reads = []
        while p + 4 <= len(data):
            bs = struct.unpack_from("<i", data, p)[0]
            self._reads.append(AlignedSegment(data, p + 4, p + 4 + bs, len(self._reads)))
            p += 4 + bs
        self._by_ref = {}
        for r in self._reads:
            self._by_ref.setdefault(r.reference_id, []).append(r)

    def fetch(self, reference, start=None, end=None):
        return iter(self._by_ref.get(self.references.index(reference), []))

    def close(self):
        pass


AlignmentFile = Samfile
