"""A deterministic BAM writer for the tests of `checkm coverage`: records as plain dicts in, BGZF blocks out (fixed zlib level, so a
fixture materialises to the same bytes everywhere).  Written from the SAM/BAM specification (SAMv1, sections 4.1 and 4.2).

A record is a dict: ref (index into the references, -1: none), flag, mapq, l_seq, cigar ([(op letter, length)]), name, tags
([(two letters, type letter, value)]; type B takes (subtype letter, [values])), pos (default 0).  `l_seq` bases of 'A' with quality
0xff are written: the coverage pass reads neither.  `raw_tail` (bytes) is appended after the tags as it stands (damaged records)."""
import random
import struct
import zlib

CIGAR_OPS = "MIDNSHP=X"
FLAG_PAIRED, FLAG_PROPER, FLAG_UNMAPPED, FLAG_SECONDARY, FLAG_QCFAIL, FLAG_DUP, FLAG_SUPP = 0x1, 0x2, 0x4, 0x100, 0x200, 0x400, 0x800
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_FMT = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
LEVEL = 6


def tag_bytes(tag, typ, value):
    out = tag.encode("ascii") + typ.encode("ascii")
    if typ == "A":
        return out + value.encode("ascii")[:1]
    if typ in _FMT:
        return out + struct.pack(_FMT[typ], value)
    if typ in "ZH":
        return out + value.encode("ascii") + b"\0"
    if typ == "B":
        sub, vals = value
        return out + sub.encode("ascii") + struct.pack("<i", len(vals)) + b"".join(struct.pack(_FMT[sub], v) for v in vals)
    raise ValueError("tag type %r" % typ)


def record_bytes(r):
    name = r.get("name", "r").encode("ascii") + b"\0"
    cigar = r.get("cigar", [])
    l_seq = int(r.get("l_seq", 0))
    body = struct.pack("<iiBBHHHiiii", int(r.get("ref", -1)), int(r.get("pos", 0)), len(name), int(r.get("mapq", 0)), 4680, len(cigar),
                       int(r.get("flag", 0)), l_seq, -1, -1, 0)
    body += name
    body += b"".join(struct.pack("<I", (int(n) << 4) | CIGAR_OPS.index(op)) for op, n in cigar)
    body += b"\x11" * ((l_seq + 1) // 2) + b"\xff" * l_seq
    body += b"".join(tag_bytes(*t) for t in r.get("tags", []))
    body += r.get("raw_tail", b"")
    return struct.pack("<i", len(body)) + body


def header_bytes(refs, text=""):
    t = text.encode("ascii")
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode("utf-8") + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", int(length))
    return out


def bgzf_block(data):
    assert len(data) <= 0xff00
    co = zlib.compressobj(LEVEL, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    bsize = len(comp) + 25
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def bgzf(data, block_bytes=0xff00, empty_every=0, eof=True):
    """`data` cut into blocks of block_bytes inflated bytes (records may span blocks); empty_every = k puts an empty block in front of
    every k-th block."""
    out = []
    for k, a in enumerate(range(0, len(data), block_bytes)):
        if empty_every and k % empty_every == 0:
            out.append(bgzf_block(b""))
        out.append(bgzf_block(data[a:a + block_bytes]))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def bam_bytes(refs, records, text="@HD\tVN:1.6\tSO:coordinate\n", **kw):
    return bgzf(header_bytes(refs, text) + b"".join(record_bytes(r) for r in records), **kw)


def write_bam(path, refs, records, index=True, **kw):
    """Writes the BAM and, with index, an empty `.bai` beside it (CheckM only looks whether that file exists)."""
    with open(path, "wb") as f:
        f.write(bam_bytes(refs, records, **kw))
    if index:
        open(path + ".bai", "wb").close()
    return path


FLAG_CHOICES = (0x4 | 0x1, 0x400 | 0x3, 0x100 | 0x3, 0x800 | 0x3, 0x200 | 0x3)
NM_TYPES = "cCsSiI"


def synthetic(nrec, nref, seed, interleave=False, run_lengths=None):
    """(refs, records) for the structure tests: about an eighth of the reads in each class under PARAMS, reads sorted by reference (runs of
    random length, or of run_lengths), names of 1 to 9 characters, NM in all six types behind Z / H / B fields.  interleave: the same
    records dealt out so that neighbours have different references."""
    r = random.Random(seed)
    refs = [("contig_%04d" % k, 1000 + 37 * k) for k in range(nref)]
    recs = []
    if run_lengths is None:
        cuts = sorted(r.randrange(nrec + 1) for _ in range(nref - 1))
        run_lengths = [b - a for a, b in zip([0] + cuts, cuts + [nrec])]
    for ref, n in enumerate(run_lengths):
        for _ in range(n):
            cls = r.randrange(8)
            l_seq = r.choice((100, 150, 151, 250))
            flag, mapq, clip, nm = 0x3, 30, 0, r.randrange(0, 2)
            if cls in (0, 1, 2):
                flag = r.choice(FLAG_CHOICES[cls:cls + 1] if cls < 2 else FLAG_CHOICES[2:4])
            elif cls == 3:
                flag, mapq = r.choice(((0x203, 30), (0x3, 3)))
            elif cls == 4:
                clip = l_seq // 2
            elif cls == 5:
                nm = l_seq // 4
            elif cls == 6:
                flag = 0x1
            cigar = ([("H", 7)] if r.random() < 0.2 else []) + ([("S", clip)] if clip else []) + [("M", l_seq - clip - 3), ("I", 3)]
            tags = [("RG", "Z", "grp%d" % r.randrange(9)), ("XB", "B", ("S", [1, 2, 3][:r.randrange(4)])), ("XH", "H", "1AE3"), ("AS", "i", -r.randrange(90))]
            tags = tags[:r.randrange(5)] + [("NM", NM_TYPES[r.randrange(6)], nm)] + [("XS", "f", 0.5)]
            recs.append(dict(ref=ref, pos=len(recs), flag=flag, mapq=mapq, l_seq=l_seq, cigar=cigar, name="r" * r.randrange(1, 10), tags=tags))
    if interleave:
        by = {}
        for x in recs:
            by.setdefault(x["ref"], []).append(x)
        out, lists = [], [v for _k, v in sorted(by.items())]
        while lists:
            lists = [v for v in lists if v]
            for v in lists:
                out.append(v.pop())
        recs = out
    return refs, recs


PARAMS = (False, 0.98, 0.02, 15)
