"""AminoAcidIdentity, API-compatible with checkm/aminoAcidIdentity.py:30-161: amino-acid identity between the copies of a
multi-copy marker (aligned to its model and masked to the match columns by HmmerAligner) and the strain-heterogeneity summary
`checkm qa` prints in its last column.

The alignment is libcheckm_hip's (ckm_align) and so is the comparison of all pairs of copies: `run` reads every
<bin>/<marker>.masked.faa, hands the rows of all groups of all bins to ONE ckm_aai_run call (checkm_amd/csrc/kernels_aai.hip: a
wavefront per pair) and builds the report, aaiRawScores, aaiHetero and aaiMeanBinHetero from the returned arrays.  A group the library
cannot take -- rows of unequal length, owners that differ, a non-ASCII character, rows of more than 4096 columns -- runs the host loop
of aai() at its place in the traversal, so the reference's AssertionError, its 'Bin ids do not match.' exit and the report written up
to that point are unchanged.  Without a visible device (CKM_ENODEV) `run` logs a warning and uses the host loop for every group, as
it did before the device pass existed; any other device error is raised.  `_run_host` is the whole run on the host loop, kept for
tools/aai_bench.py.  DESIGN section 20."""
from collections import defaultdict
import logging
import os
import sys
import time

from checkm_amd.common import getBinIdsFromOutDir
from checkm_amd.defaultValues import DefaultValues

MAX_COLUMNS = 4096          # ckm_aai_run refuses longer rows (the model limit of DESIGN section 8)


def _read_masked(path):
    """id -> sequence, ids cut at the first whitespace, blank lines skipped (checkm/util/seqUtils.py:180-211)."""
    seqs, cur = {}, None
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            if line[0] == '>':
                cur = line[1:].split(None, 1)[0]
                seqs[cur] = []
            else:
                seqs[cur].append(line.rstrip('\n'))
    return {k: ''.join(v) for k, v in seqs.items()}


class AminoAcidIdentity(object):
    def __init__(self):
        self.logger = logging.getLogger('timestamp')
        self.aaiRawScores = defaultdict(dict)
        self.aaiHetero = defaultdict(dict)
        self.aaiMeanBinHetero = {}
        self.last_timing = {}

    def run(self, aaiStrainThreshold, outDir, alignmentOutputFile):
        """AAI between all pairs of copies of every multi-copy marker of every bin (aminoAcidIdentity.py:39-98)."""
        self.logger.info('Calculating AAI between multi-copy marker genes.')
        t = dict(list=0.0, read=0.0, pack=0.0, copy_in=0.0, kernel=0.0, copy_out=0.0, python=0.0, groups=0, pairs=0, batches=0)
        self.last_timing = t
        t0 = time.perf_counter()
        report = open(alignmentOutputFile, 'w') if alignmentOutputFile else None
        groups = self._groups(outDir, t)
        done = False
        while not done:
            # the groups up to the end of the traversal, or up to one whose host loop ends the run: they go to the device together
            plan, last, failure = [], None, None
            try:
                for group in groups:
                    if self._ends_the_run(group):
                        last = group
                        break
                    plan.append(group)
                else:
                    done = True
            except Exception as e:                                # a file that cannot be read: what was read before it is still reported
                failure, done = e, True
            self._emit(plan, report, t)
            if last is not None:
                self._host_group(last, report)
            if failure is not None:
                raise failure
        if report:
            report.close()
        self.aaiHetero, self.aaiMeanBinHetero = self.strainHetero(self.aaiRawScores, aaiStrainThreshold)
        t['python'] = time.perf_counter() - t0 - sum(t[k] for k in ('list', 'read', 'pack', 'copy_in', 'kernel', 'copy_out'))

    def _groups(self, outDir, t=None):
        """(binId, marker, copies, owners) of every .masked.faa with at least two copies, in the reference's traversal: the order of
        getBinIdsFromOutDir, of os.listdir and of the ids in the file (a repeated id keeps its place and takes the later record)."""
        t = t if t is not None else dict(list=0.0, read=0.0)
        root = os.path.join(outDir, 'storage', 'aai_qa')
        sep = DefaultValues.SEQ_CONCAT_CHAR
        t0 = time.perf_counter()
        binIds = getBinIdsFromOutDir(outDir)
        t['list'] += time.perf_counter() - t0
        for binId in binIds:
            folder = os.path.join(root, binId)
            t0 = time.perf_counter()
            names = os.listdir(folder) if os.path.isdir(folder) else []
            t['list'] += time.perf_counter() - t0
            for name in names:
                if not name.endswith('.masked.faa'):
                    continue
                marker = name[:name.find('.')]                 # cut at the FIRST dot, as the reference does (PF00318.15 -> PF00318)
                t0 = time.perf_counter()
                copies = list(_read_masked(os.path.join(folder, name)).items())
                t['read'] += time.perf_counter() - t0
                if len(copies) < 2:
                    continue
                yield binId, marker, copies, [cid[:cid.find(sep)] for cid, _ in copies]

    @staticmethod
    def _ends_the_run(group):
        """A group whose host loop raises: owners that differ ('Bin ids do not match.') or rows of unequal length (aai()'s assertion)."""
        _binId, _marker, copies, owners = group
        return any(o != owners[0] for o in owners) or any(len(s) != len(copies[0][1]) for _cid, s in copies)

    @staticmethod
    def _device_takes(group):
        _binId, _marker, copies, _owners = group
        return len(copies[0][1]) <= MAX_COLUMNS and all(s.isascii() for _cid, s in copies)

    def _emit(self, plan, report, t):
        """The pairs of the groups of `plan`, in order: the groups the library takes in one call, the others on the host loop."""
        from checkm_amd import _lib
        t0 = time.perf_counter()
        slot, rows = {}, []
        for k, group in enumerate(plan):
            if self._device_takes(group):
                slot[k] = len(rows)
                rows.append([s.encode('ascii') for _cid, s in group[2]])
        t['pack'] += time.perf_counter() - t0
        r = None
        if rows:
            from checkm_amd import runtime
            try:
                ctx = runtime.get_ctx()
            except _lib.CkmError as e:
                if e.code != _lib.ENODEV:
                    raise
                # `run` worked on a host without a device before the device pass existed, and does so still: said aloud, never silently
                self.logger.warning('No usable MI355X (gfx950) device: the amino-acid identities are computed by the host loop.')
                for group in plan:
                    self._host_group(group, report)
                return
            t0 = time.perf_counter()
            r = _lib.aai_pairs(ctx, rows)
            # what the call spends outside the three device phases is packing: the offset tables, the joined text, the 16-byte stride
            t['pack'] += max(0.0, time.perf_counter() - t0 - (r['ms_upload'] + r['ms_kernel'] + r['ms_download']) / 1e3)
            t['copy_in'] += r['ms_upload'] / 1e3
            t['kernel'] += r['ms_kernel'] / 1e3
            t['copy_out'] += r['ms_download'] / 1e3
            t['groups'] += len(rows)
            t['pairs'] += int(r['npairs'])
            t['batches'] += int(r['nbatches'])
            scores = r['aai'].tolist()
            pair_off = r['pair_off'].tolist()
        for k, group in enumerate(plan):
            if k not in slot:
                self._host_group(group, report)
                continue
            binId, marker, copies, owners = group
            mine = scores[pair_off[slot[k]]:pair_off[slot[k] + 1]]
            if report:
                head, q = binId + ',' + marker + '\n', 0
                lines = [cid + '\t' + s + '\n' for cid, s in copies]
                for a in range(len(copies)):
                    for b in range(a + 1, len(copies)):
                        report.write(head + lines[a] + lines[b] + 'AAI: %.3f\n\n' % mine[q])
                        q += 1
            if owners[0] not in self.aaiRawScores:
                self.aaiRawScores[owners[0]] = defaultdict(list)
            self.aaiRawScores[owners[0]][marker].extend(mine)

    def _host_group(self, group, report):
        """The reference's pair loop over one group, one character at a time."""
        binId, marker, copies, owners = group
        for a in range(len(copies)):
            for b in range(a + 1, len(copies)):
                if owners[a] != owners[b]:
                    self.logger.error('Bin ids do not match.')
                    sys.exit(1)
                (ida, sa), (idb, sb) = copies[a], copies[b]
                score = self.aai(sa, sb)
                if report:
                    report.write('%s,%s\n%s\t%s\n%s\t%s\nAAI: %.3f\n\n' % (binId, marker, ida, sa, idb, sb, score))
                if owners[a] not in self.aaiRawScores:       # (a plain defaultdict(dict) on first touch would do; kept as the reference builds it)
                    self.aaiRawScores[owners[a]] = defaultdict(list)
                self.aaiRawScores[owners[a]][marker].append(score)

    def _run_host(self, aaiStrainThreshold, outDir, alignmentOutputFile):
        """`run` with every group on the host loop: what `run` was before the device pass.  tools/aai_bench.py times it."""
        self.logger.info('Calculating AAI between multi-copy marker genes.')
        report = open(alignmentOutputFile, 'w') if alignmentOutputFile else None
        for group in self._groups(outDir):
            self._host_group(group, report)
        if report:
            report.close()
        self.aaiHetero, self.aaiMeanBinHetero = self.strainHetero(self.aaiRawScores, aaiStrainThreshold)

    def strainHetero(self, aaiScores, aaiStrainThreshold):
        """Per marker: fraction of copy pairs above the threshold; per bin: percentage over all its pairs (:100-124)."""
        per_marker = defaultdict(dict)
        per_bin = {}
        for binId, markers in aaiScores.items():
            above_all = pairs_all = 0
            per_marker[binId] = {}
            for marker, scores in markers.items():
                above = sum(1 for sc in scores if sc > aaiStrainThreshold)
                per_marker[binId][marker] = float(above) / len(scores)
                above_all += above
                pairs_all += len(scores)
            per_bin[binId] = 100 * float(above_all) / pairs_all
        return per_marker, per_bin

    def aai(self, seq1, seq2):
        """Identity over the columns between the leading and trailing gap runs (:126-161): columns where both rows are gaps do not
        count, a gap against a residue is a mismatch.  The trailing scan never looks at column 0, as the reference's does not."""
        assert len(seq1) == len(seq2)
        gapped = [x == '-' or y == '-' for x, y in zip(seq1, seq2)]
        first = 0
        while first < len(gapped) and gapped[first]:
            first += 1
        last = len(gapped)
        while last > 1 and gapped[last - 1]:
            last -= 1
        compared = differing = 0
        for x, y in zip(seq1[first:last], seq2[first:last]):
            if x == '-' and y == '-':
                continue
            compared += 1
            differing += x != y
        return 1.0 - float(differing) / compared if compared else 0.0
