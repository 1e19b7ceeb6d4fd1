"""The draws of the marker-set selection in plain Python: Philox4x32-10 and the draw rule of checkm_amd/csrc/select_dev.h, in numpy integer
arithmetic.  What MarkerSetBuilder.sampledGenomeChecks runs for a call the library refuses, and what the device is tested against; it
makes, word for word, the draws the kernel makes."""
import numpy as np

_MASK = np.uint64(0xffffffff)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32 = np.uint64(32)
STREAM_FRAC, STREAM_COMP, STREAM_CONT = 0, 1, 2


def philox4x32(counter, key):
    """Philox4x32-10: counter is four arrays (or numbers) of 32-bit words, key two; returns the four output arrays (uint64 holding 32 bits)."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _MASK for c in counter)
    k0, k1 = (np.uint64(int(k) & 0xffffffff) for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def words(seed, stream, genome, replicate, n):
    """The first n words of a stream of draw (genome, replicate): word k of index q is entry 4 * q + k."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    seed = int(seed) & 0xffffffffffffffff
    out = philox4x32((q, np.full_like(q, replicate), np.full_like(q, genome), np.full_like(q, stream)), (seed & 0xffffffff, seed >> 32))
    return np.stack(out, axis=1).reshape(-1)[:n]


def unit(a, b):
    """53 bits of two words times 2^-53, in [0, 1): random.random()'s formula."""
    return ((int(a) >> 5) * 67108864 + (int(b) >> 6)) / 9007199254740992.0


def plan(seed, genome, replicate, genomeLen, contigLen, compRange, contRange):
    """(nComp, nCont, trueComp, trueCont) of a draw: random.uniform's formula on two device fractions, then sampleGenome's counts."""
    f = [int(x) for x in words(seed, STREAM_FRAC, genome, replicate, 4)]
    testComp = compRange[0] + (compRange[1] - compRange[0]) * unit(f[0], f[1])
    testCont = contRange[0] + (contRange[1] - contRange[0]) * unit(f[2], f[3])
    contigsInGenome = genomeLen // contigLen
    nComp, nCont = int(contigsInGenome * testComp + 0.5), int(contigsInGenome * testCont + 0.5)
    return nComp, nCont, float(nComp) * contigLen * 100 / genomeLen, float(nCont) * contigLen * 100 / genomeLen


def draw(seed, genome, replicate, genomeLen, contigLen, compRange, contRange):
    """(trueComp, trueCont, multiplicity of every contig) of a draw.  Completeness: the nComp contigs with the smallest pairs (word, index),
    once each.  Contamination: draw j lands on contig (word * C) >> 32."""
    C = genomeLen // contigLen
    if not 0 <= C < (1 << 31):
        raise ValueError('%d contigs in a genome' % C)
    nComp, nCont, trueComp, trueCont = plan(seed, genome, replicate, genomeLen, contigLen, compRange, contRange)
    if nComp < 0 or nCont < 0 or nComp > C:
        raise ValueError('a draw of %d of %d contigs' % (nComp, C))
    mult = np.zeros(C, dtype=np.int64)
    pairs = (words(seed, STREAM_COMP, genome, replicate, C) << _S32) | np.arange(C, dtype=np.uint64)
    mult[np.argsort(pairs, kind='stable')[:nComp]] = 1
    if nCont:
        landing = (words(seed, STREAM_CONT, genome, replicate, nCont) * np.uint64(C)) >> _S32
        mult += np.bincount(landing.astype(np.int64), minlength=C)
    return trueComp, trueCont, mult


def contig_starts(mult, contigLen):
    """The sorted contig starts of a draw, as sampleGenome returns them: start c * contigLen once per time contig c was drawn."""
    return [int(c) * contigLen for c in np.repeat(np.arange(len(mult)), mult)]
