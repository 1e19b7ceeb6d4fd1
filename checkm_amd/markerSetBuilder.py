"""MarkerSetBuilder, with the results of scripts/genometreeworkflow/markerSetBuilder.py of the reference for markerGenes (:131-157),
colocatedGenes (:159-192), colocatedSets (:194-235), genomeCheck (:237-263), missingGenes (:486-510), duplicateGenes (:512-536),
buildMarkerGenes (:538-562) and buildMarkerSet (:564-574), and one method the reference lacks: buildMarkerSets answers a whole batch of
genome sets -- every node of a tree -- from ONE table resident on the device, with two device calls.

The counting loops run in libcheckm_hip (checkm_amd/csrc/kernels_markerset.hip): the marker pass gives one flag byte per (query,
family), the co-location pass the reported marker pairs of every query.  colocatedSets is a union-find on the host, genomeCheck host
float arithmetic in the reference's order.  What the library refuses -- a position that does not fit int32, a distThreshold that is
not an integer, a genome listed twice in a query -- runs this module's own plain loop at that place.  Without a device the device
methods raise: there is no other compute path.

The reference's lists came out in the order of Python 2's dicts.  Here they are defined: colocatedGenes returns its pair strings
sorted, colocatedSets its sets sorted by their smallest member.  Equality with the reference is equality of sets.  DESIGN section 21.

The simulation methods of the script (:265-369) are here as plain Python with the reference's results -- uniformity, sampleGenome,
sampleGenomeScaffoldsInvLength, sampleGenomeScaffoldsWithoutReplacement, containedMarkerGenes -- and genomeChecks scores every marker set
on every draw of a genome with one device call (kernels_sim.hip).

The scaffold simulation: markerGenesOnScaffolds (:371-378) is the reference's plain loop, scaffoldChecks scores every
marker set on every draw of scaffolds of a test genome and a contaminant with one device call (kernels_simscaf.hip).  The tree walk
(buildBinMarkerSet :587-634, buildDomainMarkerSet :636-687) runs over checkm_amd.treeParser's tree; its three data files are read by
readNodeMetadata, readDuplicateSeqs and readLineageSpecificGenesToRemove from paths the caller gives, or assigned as dicts.
buildBinMarkerSetsLOO answers the leave-one-out chains of many genomes from ONE buildMarkerSets call."""
from collections import defaultdict
import logging
import random
import time

import numpy as np

from checkm_amd.markerSets import BinMarkerSets, MarkerSet


def _pair_name(a, b):
    return a + '-' + b if a <= b else b + '-' + a


def _count_class(c):
    return 1 if c == 1 else 2 if c > 1 else 0


class _Resident(object):
    """The table as arrays: families sorted by name, genomes in the given order, count classes genome-major, and the copy positions of
    every (genome, family) cell.  `device()` is the library's copy of it, made on first use."""

    def __init__(self, genomeIds, countTable, positions=None, families=None):
        self.genomes = list(genomeIds)
        self.gidx = {g: k for k, g in enumerate(self.genomes)}
        self.families = sorted(countTable) if families is None else list(families)
        self.fidx = {f: k for k, f in enumerate(self.families)}
        G, C = len(self.genomes), len(self.families)
        self.cls = np.zeros((G, C), dtype=np.uint8)
        if countTable is not None:
            for f, fam in enumerate(self.families):
                for g, c in countTable[fam].items():
                    k = self.gidx.get(g)
                    if k is not None:
                        self.cls[k, f] = _count_class(c)
        ncopies = np.zeros((G, C), dtype=np.int64)
        starts = []
        for g, genome in enumerate(self.genomes):
            here = (positions or {}).get(genome) or {}
            mine = sorted((self.fidx[fam], copies) for fam, copies in here.items() if fam in self.fidx)
            for f, copies in mine:
                ncopies[g, f] = len(copies)
                starts.extend(p[0] for p in copies)
        self.pos_off = np.zeros(G * C + 1, dtype=np.uint64)
        np.cumsum(ncopies.reshape(-1), out=self.pos_off[1:])
        self.integral = all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) for s in starts)
        self.fits = self.integral and all(-(1 << 63) <= s < (1 << 63) for s in starts)
        self.pos = np.asarray(starts, dtype=np.int64) if self.fits else np.zeros(0, dtype=np.int64)
        self._table = None

    def refused(self, dist_threshold=0):
        """Why the library would not take this table (or this threshold), or None.  ckm_mset_check, no device."""
        from checkm_amd import _lib
        if not self.fits:
            return 'a position that is not an integer of 64 bits'
        try:
            _lib.mset_check(self.cls, self.pos_off, self.pos, dist_threshold=dist_threshold)
        except _lib.CkmError as e:
            return str(e)
        return None

    def device(self, timing=None):
        if self._table is None:
            from checkm_amd import _lib, runtime
            self._table = _lib.MsetTable(runtime.get_ctx(), self.cls, self.pos_off, self.pos)
            if timing is not None:
                timing['copy_in'] += self._table.ms_upload / 1e3
        return self._table

    def close(self):
        if self._table is not None:
            self._table.close()
            self._table = None


def _integral(x):
    try:
        return float(x) == int(x)
    except (TypeError, ValueError, OverflowError):
        return False


class MarkerSetBuilder(object):
    def __init__(self, img=None):
        self.logger = logging.getLogger('timestamp')
        self.img = img
        self.cachedGeneCountTable = None
        self.last_timing = {}
        self.last_sim_timing = {}
        self.last_scaffold_timing = {}
        self.last_select_timing = {}
        self.duplicateSeqs = {}                      # leaf label -> labels of the genomes dereplicated into it
        self.uniqueIdToLineageStatistics = {}        # node uid -> statistics of the node
        self.lineageSpecificGenesToRemove = {}       # node uid -> genes lost or duplicated in that lineage

    def precomputeGenomeFamilyScaffolds(self, genomeIds):
        self.img.precomputeGenomeFamilyScaffolds(genomeIds)

    def precomputeGenomeSeqLens(self, genomeIds):
        self.img.precomputeGenomeSeqLens(genomeIds)

    def precomputeGenomeFamilyPositions(self, genomeIds, spacingBetweenContigs):
        self.img.precomputeGenomeFamilyPositions(genomeIds, spacingBetweenContigs)

    # ---- the marker pass ------------------------------------------------------------------------------------------------------------
    def _ctx(self):
        from checkm_amd import runtime
        return runtime.get_ctx()

    @staticmethod
    def _walk(genomeIds, genomeCounts):
        """One family of one query on the host: ubiquity, single-copy and duplicate counts."""
        ubiquity = single = duplicate = 0
        for genomeId in genomeIds:
            c = genomeCounts.get(genomeId, 0)
            ubiquity += c > 0
            single += c == 1
            duplicate += c > 1
        return ubiquity, single, duplicate

    def _flags(self, genomeIds, countTable, tU, tS):
        """family -> flag byte of the marker pass for ONE query; the plain loop for a genome list the library does not take.  With a
        genome listed twice ubiquity can exceed len(genomeCounts), and only then does the reference's early `continue` decide."""
        genomeIds = list(genomeIds)
        if len(set(genomeIds)) != len(genomeIds):
            out = {}
            for fam, genomeCounts in countTable.items():
                u, s, d = self._walk(genomeIds, genomeCounts)
                out[fam] = (1 if len(genomeCounts) >= tU and u >= tU and s >= tS else 0) | (2 if len(genomeIds) - u >= tU else 0) | (4 if d >= tU else 0)
            return out
        from checkm_amd import _lib
        res = _Resident(genomeIds, countTable)
        try:
            r = _lib.mset_markers(self._ctx(), res.device(), [list(range(len(genomeIds)))], [tU], [tS])
        finally:
            res.close()
        return dict(zip(res.families, r['flag'][0].tolist()))

    def markerGenes(self, genomeIds, countTable, ubiquityThreshold, singleCopyThreshold):
        """Families present in at least ubiquityThreshold and single-copy in at least singleCopyThreshold of the genomes (both are
        numbers of genomes).  The reference's early `continue` on len(genomeCounts) is not reproduced: it never changes a result."""
        if ubiquityThreshold < 1 or singleCopyThreshold < 1:
            print('[Warning] Looks like degenerate threshold.')
        flags = self._flags(genomeIds, countTable, float(ubiquityThreshold), float(singleCopyThreshold))
        return set(fam for fam, f in flags.items() if f & 1)

    def _count_table(self, genomeIds):
        return self.cachedGeneCountTable if self.cachedGeneCountTable is not None else self.img.geneCountTable(genomeIds)

    def missingGenes(self, genomeIds, markerGenes, ubiquityThreshold):
        """Markers absent from at least ubiquityThreshold * len(genomeIds) of the genomes."""
        t = ubiquityThreshold * len(genomeIds)
        flags = self._flags(genomeIds, self._count_table(genomeIds), float(t), 0.0)
        return set(fam for fam, f in flags.items() if f & 2 and fam in markerGenes)

    def duplicateGenes(self, genomeIds, markerGenes, ubiquityThreshold):
        """Markers with more than one copy in at least ubiquityThreshold * len(genomeIds) of the genomes."""
        t = ubiquityThreshold * len(genomeIds)
        flags = self._flags(genomeIds, self._count_table(genomeIds), float(t), 0.0)
        return set(fam for fam, f in flags.items() if f & 4 and fam in markerGenes)

    def buildMarkerGenes(self, genomeIds, ubiquityThreshold, singleCopyThreshold):
        markers = self.markerGenes(genomeIds, self._count_table(genomeIds), ubiquityThreshold * len(genomeIds), singleCopyThreshold * len(genomeIds))
        return markers - self.img.identifyRedundantTIGRFAMs(markers)

    # ---- the co-location pass ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _colocated_host(geneDistTable, distThreshold, genomeThreshold):
        """The reference's loop, plainly: per genome every pair of its families, any two copies closer than the threshold."""
        seen = defaultdict(int)
        for locs in geneDistTable.values():
            ids = list(locs)
            for a in range(len(ids)):
                for b in range(a + 1, len(ids)):
                    if any(abs(p[0] - q[0]) < distThreshold for p in locs[ids[a]] for q in locs[ids[b]]):
                        seen[_pair_name(ids[a], ids[b])] += 1
        return sorted(name for name, count in seen.items() if float(count) / len(geneDistTable) > genomeThreshold)

    def colocatedGenes(self, geneDistTable, distThreshold=5000, genomeThreshold=0.95):
        """'A-B' (A <= B) for every pair of families with copies closer than distThreshold in more than genomeThreshold of the genomes
        of geneDistTable; sorted."""
        genomes = list(geneDistTable)
        families = sorted(set(fam for locs in geneDistTable.values() for fam in locs))
        if not genomes or len(families) < 2:
            return []
        res = None
        if _integral(distThreshold):
            res = _Resident(genomes, None, geneDistTable, families)
            if res.refused(int(distThreshold)) is not None:
                res = None
        if res is None:
            return self._colocated_host(geneDistTable, distThreshold, genomeThreshold)
        from checkm_amd import _lib
        try:
            r = _lib.mset_colocated(self._ctx(), res.device(), [list(range(len(genomes)))], [list(range(len(families)))], int(distThreshold), float(genomeThreshold))
        finally:
            res.close()
        return sorted(_pair_name(families[i], families[j]) for i, j in zip(r['i'].tolist(), r['j'].tolist()))

    def colocatedSets(self, colocatedGenes, markerGenes):
        """The connected groups of the pairs, and every marker outside them by itself; sorted by the smallest member."""
        parent = {}

        def root(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for cg in colocatedGenes:
            geneA, geneB = cg.split('-')
            ra, rb = root(parent.setdefault(geneA, geneA)), root(parent.setdefault(geneB, geneB))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        groups = defaultdict(set)
        for gene in parent:
            groups[root(gene)].add(gene)
        sets = list(groups.values()) + [set([m]) for m in markerGenes if m not in parent]
        return sorted(sets, key=min)

    def genomeCheck(self, colocatedSet, genomeId, countTable):
        """Completeness and contamination of one genome as fractions, and its missing and duplicated markers."""
        comp = cont = 0.0
        missingMarkers, duplicateMarkers = set(), set()
        if len(colocatedSet) == 0:
            return comp, cont, missingMarkers, duplicateMarkers
        for cs in colocatedSet:
            present = multiCopy = 0
            for marker in cs:
                count = countTable[marker].get(genomeId, 0)
                if count == 1:
                    present += 1
                elif count > 1:
                    present += 1
                    multiCopy += count - 1
                    duplicateMarkers.add(marker)
                elif count == 0:
                    missingMarkers.add(marker)
            comp += float(present) / len(cs)
            cont += float(multiCopy) / len(cs)
        return comp / len(colocatedSet), cont / len(colocatedSet), missingMarkers, duplicateMarkers

    # ---- whole marker sets ------------------------------------------------------------------------------------------------------------
    def buildMarkerSet(self, genomeIds, ubiquityThreshold, singleCopyThreshold, spacingBetweenContigs=5000):
        return self.buildMarkerSets([genomeIds], ubiquityThreshold, singleCopyThreshold, spacingBetweenContigs)[0]

    def _marker_set_host(self, genomeIds, table, positions, ubiquityThreshold, singleCopyThreshold):
        """One query entirely on the plain loops."""
        n = len(genomeIds)
        tU, tS = ubiquityThreshold * n, singleCopyThreshold * n
        markers = set()
        for fam, genomeCounts in table.items():
            u, s, _d = self._walk(genomeIds, genomeCounts)
            if len(genomeCounts) >= tU and u >= tU and s >= tS:
                markers.add(fam)
        markers -= self.img.identifyRedundantTIGRFAMs(markers)
        dist = {g: {m: positions[g][m] for m in markers if m in positions[g]} for g in genomeIds}
        return markers, self._colocated_host(dist, 5000, 0.95)

    def buildMarkerSets(self, listOfGenomeIdLists, ubiquityThreshold, singleCopyThreshold, spacingBetweenContigs=5000):
        """[buildMarkerSet(ids, ...) for ids in listOfGenomeIdLists] from one resident table: the marker pass over all lists in one
        device call, the TIGRFAM redundancy removal per list on the host, the co-location pass over all lists in a second call.  The
        gene count table is cachedGeneCountTable if set, else img.geneCountTable of the genomes of all lists together: a family
        absent from the genomes of a list has ubiquity 0 there, so with thresholds above zero the markers of a list are those of its
        own table."""
        t = dict(read=0.0, table=0.0, copy_in=0.0, markers=0.0, pack=0.0, count=0.0, scan=0.0, fill=0.0, copy_out=0.0, union_find=0.0, python=0.0,
                 queries=len(listOfGenomeIdLists), pairs=0, tests=0, rounds=0, batches=0)
        self.last_timing = t
        t_begin = time.perf_counter()
        lists = [list(ids) for ids in listOfGenomeIdLists]
        allGenomes = sorted(set(g for ids in lists for g in ids))
        t0 = time.perf_counter()
        table = self._count_table(allGenomes)
        positions = self.img.geneDistTable(allGenomes, list(table), spacingBetweenContigs)
        t['read'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        res = _Resident(allGenomes, table, positions)
        refused = res.refused(5000)
        t['table'] = time.perf_counter() - t0
        # the lists the library takes: no genome twice (the table itself may be refused as a whole)
        device = [k for k, ids in enumerate(lists) if refused is None and len(set(ids)) == len(ids)]
        markers, pairs = {}, {}
        try:
            self._device_passes(res, lists, device, ubiquityThreshold, singleCopyThreshold, markers, pairs, t)
        finally:
            res.close()
        out = []
        for k, ids in enumerate(lists):
            if ubiquityThreshold * len(ids) < 1 or singleCopyThreshold * len(ids) < 1:
                print('[Warning] Looks like degenerate threshold.')
            if k not in markers:
                markers[k], pairs[k] = self._marker_set_host(ids, table, positions, ubiquityThreshold, singleCopyThreshold)
            t0 = time.perf_counter()
            sets = self.colocatedSets(pairs[k], markers[k])
            t['union_find'] += time.perf_counter() - t0
            out.append(MarkerSet(0, 'NA', len(ids), sets))
        t['python'] = time.perf_counter() - t_begin - sum(t[k] for k in ('read', 'table', 'copy_in', 'markers', 'pack', 'count', 'scan', 'fill', 'copy_out', 'union_find'))
        return out

    def _device_passes(self, res, lists, device, ubiquityThreshold, singleCopyThreshold, markers, pairs, t):
        """The two device calls of buildMarkerSets over the lists numbered in `device`; fills markers[k] and pairs[k]."""
        from checkm_amd import _lib
        if device:
            ctx = self._ctx()
            dev = res.device(t)
            glists = [[res.gidx[g] for g in lists[k]] for k in device]
            r = _lib.mset_markers(ctx, dev, glists, [ubiquityThreshold * len(lists[k]) for k in device], [singleCopyThreshold * len(lists[k]) for k in device])
            t['copy_in'] += r['ms_upload'] / 1e3
            t['markers'] += r['ms_markers'] / 1e3
            t['copy_out'] += r['ms_download'] / 1e3
            fams = np.asarray(res.families, dtype=object)
            mlists = []
            for row, k in enumerate(device):
                found = set(fams[np.nonzero(r['flag'][row] & 1)[0]].tolist())
                found -= self.img.identifyRedundantTIGRFAMs(found)
                markers[k] = found
                mlists.append(sorted(res.fidx[m] for m in found))
            r = _lib.mset_colocated(ctx, dev, glists, mlists, 5000, 0.95)
            for name, key in (('copy_in', 'ms_upload'), ('pack', 'ms_pack'), ('count', 'ms_count'), ('scan', 'ms_scan'), ('fill', 'ms_fill'), ('copy_out', 'ms_download')):
                t[name] += r[key] / 1e3
            t['pairs'], t['tests'], t['rounds'], t['batches'] = int(r['npairs']), int(r['tests']), int(r['nrounds']), int(r['nbatches'])
            off, pi, pj = r['pair_off'].tolist(), r['i'].tolist(), r['j'].tolist()
            for row, k in enumerate(device):
                ml = mlists[row]
                pairs[k] = sorted(_pair_name(res.families[ml[pi[x]]], res.families[ml[pj[x]]]) for x in range(off[row], off[row + 1]))

    # ---- the simulation (markerSetBuilder.py:265-369) ---------------------------------------------------------------------------------------
    def uniformity(self, genomeSize, pts):
        """1 - sum |d - U| / sum max(d, U) over the gaps d of the sorted points, U the gap of len(pts) evenly spaced points."""
        U = float(genomeSize) / (len(pts) + 1)
        pts = sorted(pts)
        num = den = 0
        for a, b in zip(pts, pts[1:]):
            num += abs(b - a - U)
            den += max(b - a, U)
        return 1.0 - num / den

    def sampleGenome(self, genomeLen, percentComp, percentCont, contigLen):
        """A draw of fixed-length contigs: (true completeness, true contamination, sorted contig starts).  Completeness contigs come
        from random.sample, contamination contigs (with replacement) from numpy's legacy choice, in that order, so a caller that seeds
        both generators gets the reference's contigs.  contigsInGenome is the integer quotient of the reference's Python 2 text."""
        contigsInGenome = genomeLen // contigLen
        nComp = int(contigsInGenome * percentComp + 0.5)
        nCont = int(contigsInGenome * percentCont + 0.5)
        compContigs = random.sample(range(contigsInGenome), nComp)
        contContigs = np.random.choice(range(contigsInGenome), nCont, replace=True).tolist()
        contigStarts = sorted(c * contigLen for c in compContigs + contContigs)
        return float(nComp) * contigLen * 100 / genomeLen, float(nCont) * contigLen * 100 / genomeLen, contigStarts

    @staticmethod
    def _take_until(order, targetPer, seqLens, genomeSize):
        sampled, truePer = [], 0.0
        for seqId in order:
            sampled.append(seqId)
            truePer += float(seqLens[seqId]) / genomeSize
            if truePer >= targetPer:
                break
        return sampled, truePer * 100

    def sampleGenomeScaffoldsInvLength(self, targetPer, seqLens, genomeSize):
        """Sequences drawn without replacement with probability inversely proportional to their length, until they hold targetPer of
        the genome: (sequence ids, percentage held).  The probabilities are normalised with Python's own sum, as in the reference."""
        seqProb = np.array([1.0 / (float(seqLen) / genomeSize) for seqLen in seqLens.values()])
        seqProb /= sum(seqProb)
        return self._take_until(np.random.choice(list(seqLens.keys()), size=len(seqLens), replace=False, p=seqProb), targetPer, seqLens, genomeSize)

    def sampleGenomeScaffoldsWithoutReplacement(self, targetPer, seqLens, genomeSize):
        """Sequences drawn uniformly without replacement until they hold targetPer of the genome: (sequence ids, percentage held)."""
        return self._take_until(np.random.choice(list(seqLens.keys()), size=len(seqLens), replace=False), targetPer, seqLens, genomeSize)

    def containedMarkerGenes(self, markerGenes, clusterIdToGenomePositions, startPartialGenomeContigs, contigLen):
        """marker -> the contig starts s with 0 <= p[0] - s < contigLen, once per copy p and start s; markers without one are left out.
        The plain loop: what genomeChecks runs in place of the device for a call the library refuses, and what it is tested against."""
        contained = {}
        for markerGene in markerGenes:
            containedPos = [s for p in clusterIdToGenomePositions.get(markerGene, []) for s in startPartialGenomeContigs if 0 <= p[0] - s < contigLen]
            if containedPos:
                contained[markerGene] = containedPos
        return contained

    @staticmethod
    def _genome_check_host(ms, hits):
        """Both modes of MarkerSet.genomeCheck (checkm/markerSets.py:206-238) for one marker set on the host, in its operation order:
        (individual completeness, individual contamination, set completeness, set contamination)."""
        present = multiCopy = 0
        for marker in ms.getMarkerGenes():
            if marker in hits:
                present += 1
                multiCopy += len(hits[marker]) - 1
        numMarkers = ms.numMarkers()
        indComp, indCont = 100 * float(present) / numMarkers, 100 * float(multiCopy) / numMarkers
        comp = cont = 0.0
        for cs in ms.markerSet:
            present = multiCopy = 0
            for marker in cs:
                count = len(hits.get(marker, []))
                if count >= 1:
                    present += 1
                    multiCopy += count - 1
            comp += float(present) / len(cs)
            cont += float(multiCopy) / len(cs)
        return indComp, indCont, 100 * comp / len(ms.markerSet), 100 * cont / len(ms.markerSet)

    def _genome_checks_host(self, markerSets, genePositions, contigStartLists, contigLens):
        out = np.zeros((len(contigStartLists), len(markerSets), 4), dtype=np.float64)
        for r, (starts, contigLen) in enumerate(zip(contigStartLists, contigLens)):
            for s, ms in enumerate(markerSets):
                out[r, s] = self._genome_check_host(ms, self.containedMarkerGenes(ms.getMarkerGenes(), genePositions, starts, contigLen))
        return out

    @staticmethod
    def _sim_tables(markerSets, genePositions, contigStartLists, contigLens):
        """The arrays of one ckm_sim_run call (include/checkm_hip.h), or None where they cannot be said in int64: the distinct markers of
        all sets sorted by name, their copies' starts, the marker sets as lists of co-located sets, the draws with their starts sorted."""
        from checkm_amd import _lib
        markers = sorted(set(m for ms in markerSets for m in ms.getMarkerGenes()))
        midx = {m: k for k, m in enumerate(markers)}
        copies = [[p[0] for p in genePositions.get(m, [])] for m in markers]
        flat = [x for c in copies for x in c] + list(contigLens)
        if not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) and -(1 << 63) <= x < (1 << 63) for x in flat):
            return None
        starts = [np.asarray(s).reshape(-1) for s in contigStartLists]
        if not all(s.size == 0 or (s.dtype.kind in 'iu' and s.dtype.itemsize <= 8 and s.dtype != np.uint64) for s in starts):
            return None
        off = lambda lens: np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)])
        sets = [list(cs) for ms in markerSets for cs in ms.markerSet]
        return _lib.SimTables(off([len(c) for c in copies]), [x for c in copies for x in c], off([len(ms.markerSet) for ms in markerSets]), off([len(cs) for cs in sets]),
                              [midx[m] for cs in sets for m in cs], off([s.size for s in starts]),
                              np.concatenate([np.sort(s.astype(np.int64)) for s in starts]) if starts else [], list(contigLens))

    def genomeChecks(self, markerSets, genePositions, contigStartLists, contigLens):
        """out[replicate][markerSet] = (individual completeness, individual contamination, set completeness, set contamination): for
        every draw (contigStartLists[r], contigLens[r]) and marker set what containedMarkerGenes followed by MarkerSet.genomeCheck in
        both modes gives, from ONE device call.  genePositions is geneDistTable[genomeId].  A call the library refuses (a position
        beyond int32, a marker set without sets -- the reference's ZeroDivisionError) runs the plain loop."""
        markerSets = list(markerSets)
        if len(contigStartLists) != len(contigLens):
            raise ValueError('one contig length per draw')
        t = dict(pack=0.0, copy_in=0.0, kernel=0.0, copy_out=0.0, rounds=0, device=False)
        self.last_sim_timing = t
        from checkm_amd import _lib
        t0 = time.perf_counter()
        tables = self._sim_tables(markerSets, genePositions, contigStartLists, contigLens)
        if tables is not None:
            try:
                _lib.sim_check(tables)
            except _lib.CkmError:
                tables = None
        t['pack'] = time.perf_counter() - t0
        if tables is None:
            return self._genome_checks_host(markerSets, genePositions, contigStartLists, contigLens)
        r = _lib.sim_run(self._ctx(), tables)
        t.update(pack=t['pack'] + r['ms_pack'] / 1e3, copy_in=r['ms_upload'] / 1e3, kernel=r['ms_kernel'] / 1e3, copy_out=r['ms_download'] / 1e3, rounds=r['nrounds'], device=True)
        return r['out']

    # ---- sampled genomes drawn on the device (scripts/simInferBestMarkerSet.py:94-110) ------------------------------------
    @staticmethod
    def _select_tables(markerSets, genePositionsPerGenome, genomeSizes, numReplicates, contigLen, compRange, contRange, seed):
        """The arrays of one ckm_select_run call (include/checkm_hip.h), or None where they cannot be said in its number types: the
        distinct markers of all sets sorted by name, their copies' starts per test genome, the marker sets as lists of co-located sets."""
        from checkm_amd import _lib
        markers = sorted(set(m for ms in markerSets for m in ms.getMarkerGenes()))
        midx = {m: k for k, m in enumerate(markers)}
        copies = [[p[0] for p in positions.get(m, [])] for positions in genePositionsPerGenome for m in markers]
        flat = [x for c in copies for x in c] + list(genomeSizes) + [contigLen, numReplicates]
        if not isinstance(seed, (int, np.integer)) or not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) and -(1 << 63) <= x < (1 << 63) for x in flat):
            return None
        if not 0 <= numReplicates < (1 << 32) or not all(isinstance(x, (int, float)) for x in tuple(compRange) + tuple(contRange)):
            return None
        off = lambda lens: np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)])
        sets = [list(cs) for ms in markerSets for cs in ms.markerSet]
        return _lib.SelectTables(list(genomeSizes), len(markers), off([len(c) for c in copies]), [x for c in copies for x in c], off([len(ms.markerSet) for ms in markerSets]),
                                 off([len(cs) for cs in sets]), [midx[m] for cs in sets for m in cs], numReplicates, contigLen, compRange, contRange, seed)

    def _sampled_checks_host(self, markerSets, genePositionsPerGenome, genomeSizes, numReplicates, contigLen, compRange, contRange, seed):
        """The same draws in plain Python (checkm_amd.selectDraws), scored by the plain loop of genomeChecks."""
        from checkm_amd import selectDraws
        true = np.zeros((len(genomeSizes), numReplicates, 2), dtype=np.float64)
        out = np.zeros((len(genomeSizes), numReplicates, len(markerSets), 4), dtype=np.float64)
        mults = []
        for g, (positions, genomeSize) in enumerate(zip(genePositionsPerGenome, genomeSizes)):
            rows = np.zeros((numReplicates, max(genomeSize // contigLen, 0)), dtype=np.uint16)
            for r in range(numReplicates):
                true[g, r, 0], true[g, r, 1], mult = selectDraws.draw(seed, g, r, genomeSize, contigLen, compRange, contRange)
                rows[r] = np.minimum(mult, 65535)
                out[g, r] = self._genome_checks_host(markerSets, positions, [selectDraws.contig_starts(mult, contigLen)], [contigLen])[0]
            mults.append(rows)
        return true, out, mults

    def sampledGenomeChecks(self, markerSets, genePositionsPerGenome, genomeSizes, numReplicates, contigLen, compRange=(0.5, 1.0), contRange=(0.0, 0.2), seed=0,
                            withDraws=False):
        """(true[genome][replicate] = (true completeness, true contamination), out[genome][replicate][markerSet] = genomeChecks' four
        values) for numReplicates draws of sampleGenome per test genome, the target fractions uniform in compRange and contRange -- the
        replicate loop of scripts/simInferBestMarkerSet.py (:94-110) from ONE device call.  The draws are made on the device from a
        counter-based generator (Philox4x32-10 keyed by seed), so they are a function of the arguments alone and are not Python's.
        genePositionsPerGenome[g] is geneDistTable[genomeId] of test genome g.  withDraws: also, per genome, how often every contig was
        drawn, uint16 [replicate][contig], as the library returns it: min(multiplicity, 65535).  A call the library refuses (more contigs
        than a block keeps, a position beyond int32, ...) makes the same draws in plain Python and scores them with the plain loop."""
        markerSets, genePositionsPerGenome, genomeSizes = list(markerSets), list(genePositionsPerGenome), list(genomeSizes)
        if len(genePositionsPerGenome) != len(genomeSizes):
            raise ValueError('one genome size per test genome')
        t = dict(pack=0.0, copy_in=0.0, kernel=0.0, copy_out=0.0, rounds=0, device=False)
        self.last_select_timing = t
        from checkm_amd import _lib
        t0 = time.perf_counter()
        tables = self._select_tables(markerSets, genePositionsPerGenome, genomeSizes, numReplicates, contigLen, compRange, contRange, seed)
        if tables is not None:
            try:
                _lib.select_check(tables)
            except _lib.CkmError:
                tables = None
        t['pack'] = time.perf_counter() - t0
        if tables is None:
            true, out, mults = self._sampled_checks_host(markerSets, genePositionsPerGenome, genomeSizes, numReplicates, contigLen, compRange, contRange, seed)
            return (true, out, mults) if withDraws else (true, out)
        r = _lib.select_run(self._ctx(), tables, with_rows=withDraws)
        t.update(pack=t['pack'] + r['ms_pack'] / 1e3, copy_in=r['ms_upload'] / 1e3, kernel=r['ms_kernel'] / 1e3, copy_out=r['ms_download'] / 1e3, rounds=r['nrounds'], device=True)
        return (r['truth'], r['out'], r['rows']) if withDraws else (r['truth'], r['out'])

    # ---- the scaffold simulation (markerSetBuilder.py:371-378) -----------------------------------------------------------
    def markerGenesOnScaffolds(self, markerGenes, genomeId, scaffoldIds, containedMarkerGenes):
        """Appends to containedMarkerGenes[marker] the scaffold of every copy of the marker in genomeId that lies on one of scaffoldIds.
        The plain loop: what scaffoldChecks runs in place of the device for a call the library refuses, and what it is tested against."""
        scaffoldsOf = self.img.cachedGenomeFamilyScaffolds[genomeId]
        for markerGeneId in markerGenes:
            for scaffoldId in scaffoldsOf.get(markerGeneId, []):
                if scaffoldId in scaffoldIds:
                    containedMarkerGenes[markerGeneId] += [scaffoldId]

    def _scaffold_checks_host(self, markerSets, testGenomeId, draws):
        out = np.zeros((len(draws), len(markerSets), 4), dtype=np.float64)
        for r, (retainedTestSeqIds, contGenomeId, contSampledSeqIds) in enumerate(draws):
            for s, ms in enumerate(markerSets):
                contained = defaultdict(list)
                self.markerGenesOnScaffolds(ms.getMarkerGenes(), testGenomeId, retainedTestSeqIds, contained)
                if contGenomeId is not None:
                    self.markerGenesOnScaffolds(ms.getMarkerGenes(), contGenomeId, contSampledSeqIds, contained)
                out[r, s] = self._genome_check_host(ms, contained)
        return out

    def _scaffold_tables(self, markerSets, testGenomeId, draws):
        """The arrays of one ckm_simscaf_run call (include/checkm_hip.h): genome 0 is the test genome, the contaminants follow sorted;
        the distinct markers of all sets sorted by name; a genome's scaffolds are those that carry a copy of one of these markers,
        numbered as the copies meet them -- an id only the FASTA file knows has no copy and needs no bit, an id only the GFF file knows
        has a bit that no draw sets."""
        from checkm_amd import _lib
        cached = self.img.cachedGenomeFamilyScaffolds
        genomes = [testGenomeId] + sorted(set(d[1] for d in draws if d[1] is not None) - set([testGenomeId]))
        gidx = {g: k for k, g in enumerate(genomes)}
        markers = sorted(set(m for ms in markerSets for m in ms.getMarkerGenes()))
        midx = {m: k for k, m in enumerate(markers)}
        index, sc, lens = [], [], []
        for g in genomes:
            ids = {}
            for m in markers:
                copies = cached[g].get(m, [])
                sc.extend(ids.setdefault(s, len(ids)) for s in copies)
                lens.append(len(copies))
            index.append(ids)
        off = lambda n: np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(n, dtype=np.uint64)])
        words = [(len(ids) + 31) // 32 for ids in index]
        test, cont, rows, row_lens = [], [], [], []

        def row(g, seqIds):
            ids = index[g]
            at = np.fromiter((ids[s] for s in seqIds if s in ids), dtype=np.int64)
            w = np.zeros(words[g], dtype=np.uint32)
            np.bitwise_or.at(w, at >> 5, (np.uint32(1) << (at & 31).astype(np.uint32)))
            return w

        for retainedTestSeqIds, contGenomeId, contSampledSeqIds in draws:
            test.append(0)
            rows.append(row(0, retainedTestSeqIds))
            n = words[0]
            if contGenomeId is None:
                cont.append(_lib.SIMSCAF_NONE)
            else:
                cont.append(gidx[contGenomeId])
                rows.append(row(gidx[contGenomeId], contSampledSeqIds))
                n += words[gidx[contGenomeId]]
            row_lens.append(n)
        sets = [list(cs) for ms in markerSets for cs in ms.markerSet]
        return _lib.SimScafTables([len(ids) for ids in index], len(markers), off(lens), sc, off([len(ms.markerSet) for ms in markerSets]), off([len(cs) for cs in sets]),
                                  [midx[m] for cs in sets for m in cs], test, cont, off(row_lens), np.concatenate(rows) if rows else [])

    def scaffoldChecks(self, markerSets, testGenomeId, draws):
        """out[replicate][markerSet] = (individual completeness, individual contamination, set completeness, set contamination): for
        every draw (retainedTestSeqIds, contGenomeId or None, contSampledSeqIds) and marker set what markerGenesOnScaffolds over the
        test genome and over the contaminant followed by MarkerSet.genomeCheck in both modes gives, from ONE device call.  The scaffolds
        of the markers come from precomputeGenomeFamilyScaffolds.  A call the library refuses (a marker set without sets -- the
        reference's ZeroDivisionError) runs the plain loop."""
        markerSets, draws = list(markerSets), [tuple(d) for d in draws]
        t = dict(pack=0.0, copy_in=0.0, kernel=0.0, copy_out=0.0, rounds=0, device=False)
        self.last_scaffold_timing = t
        from checkm_amd import _lib
        t0 = time.perf_counter()
        tables = self._scaffold_tables(markerSets, testGenomeId, draws)
        try:
            _lib.simscaf_check(tables)
        except _lib.CkmError:
            tables = None
        t['pack'] = time.perf_counter() - t0
        if tables is None:
            return self._scaffold_checks_host(markerSets, testGenomeId, draws)
        r = _lib.simscaf_run(self._ctx(), tables)
        t.update(pack=t['pack'] + r['ms_pack'] / 1e3, copy_in=r['ms_upload'] / 1e3, kernel=r['ms_kernel'] / 1e3, copy_out=r['ms_download'] / 1e3, rounds=r['nrounds'], device=True)
        return r['out']

    # ---- the tree walk (markerSetBuilder.py:380-484, :576-687) --------------------------------------------------------------------------------
    def readDuplicateSeqs(self, path):
        """leaf label -> labels of the genomes whose alignments repeat it (the derep list: a label and its duplicates per line)."""
        self.duplicateSeqs = {}
        with open(path) as f:
            for line in f:
                fields = line.rstrip().split()
                if len(fields) > 1:
                    self.duplicateSeqs[fields[0]] = fields[1:]
        return self.duplicateSeqs

    def readNodeMetadata(self, path):
        """node uid -> statistics of the node (the node metadata table; the walk reads 'taxonomy')."""
        stats = {}
        with open(path) as f:
            f.readline()
            for line in f:
                fields = line.rstrip().split('\t')
                d = {'# genomes': int(fields[1]), 'taxonomy': fields[2]}
                try:
                    d['bootstrap'] = float(fields[3])
                except ValueError:
                    d['bootstrap'] = 'NA'
                d['gc mean'], d['gc std'] = float(fields[4]), float(fields[5])
                d['genome size mean'], d['genome size std'] = float(fields[6]) / 1e6, float(fields[7]) / 1e6
                d['gene count mean'], d['gene count std'] = float(fields[8]), float(fields[9])
                d['marker set'] = fields[10].rstrip()
                stats[fields[0]] = d
        self.uniqueIdToLineageStatistics = stats
        return stats

    def readLineageSpecificGenesToRemove(self, path):
        """node uid -> genes lost or duplicated in that lineage (uid, set literal of the missing, set literal of the duplicated)."""
        from checkm_amd.treeParser import parse_set_literal
        self.lineageSpecificGenesToRemove = {}
        with open(path) as f:
            for line in f:
                fields = line.rstrip('\n').split('\t')
                self.lineageSpecificGenesToRemove[fields[0]] = parse_set_literal(fields[1]) | parse_set_literal(fields[2])
        return self.lineageSpecificGenesToRemove

    def _next_named_node(self, node):
        """Taxonomy of the first labelled ancestor that has one, else 'root' (:421-436)."""
        p = node.parent
        while p is not None:
            if p.label:
                taxonomy = self.uniqueIdToLineageStatistics[p.label.split('|')[0]]['taxonomy']
                if taxonomy != '':
                    return taxonomy
            p = p.parent
        return 'root'

    @staticmethod
    def _without(markerSet, genesToRemove):
        """The marker set without those genes; a co-located set left empty is dropped (:461-484)."""
        kept = [cs - genesToRemove for cs in markerSet.markerSet]
        return MarkerSet(markerSet.UID, markerSet.lineageStr, markerSet.numGenomes, [cs for cs in kept if cs])

    def _chain_nodes(self, curNode, genomeIdsToRemove, domainOnly):
        """[(lineageStr, sorted genome ids)] of the nodes from curNode to the root that keep at least two genomes (:598-632): the leaves
        below the node and the genomes dereplicated into them, without genomeIdsToRemove."""
        out = []
        removed = set(genomeIdsToRemove) if genomeIdsToRemove is not None else set()
        while curNode is not None:
            uniqueId = curNode.label.split('|')[0]
            if not domainOnly or uniqueId in ('UID2', 'UID203'):
                taxonomyStr = self.uniqueIdToLineageStatistics[uniqueId]['taxonomy']
                if taxonomyStr == '':
                    taxonomyStr = self._next_named_node(curNode)
                genomeIds = set()
                for leaf in curNode.leaves():
                    genomeIds.add(leaf.taxon.replace('IMG_', ''))
                    genomeIds.update(dup.replace('IMG_', '') for dup in self.duplicateSeqs.get(leaf.taxon, []))
                genomeIds -= removed
                if len(genomeIds) >= 2:
                    out.append((uniqueId + ' | ' + taxonomyStr.split(';')[-1], sorted(genomeIds)))
            curNode = curNode.parent
        return out

    def _chains(self, starts, ubiquityThreshold, singleCopyThreshold, bMarkerSet, domainOnly=False):
        """[(binMarkerSets, refinedBinMarkerSet)] for every (node, genomeIdsToRemove) of starts.  The genome lists of all chains, each
        distinct list once, are answered by one buildMarkerSets call (bMarkerSet) or by buildMarkerGenes per list."""
        chains = [self._chain_nodes(node, remove, domainOnly) for node, remove in starts]
        lists = sorted(set(tuple(ids) for chain in chains for _, ids in chain))
        if bMarkerSet:
            built = self.buildMarkerSets([list(ids) for ids in lists], ubiquityThreshold, singleCopyThreshold) if lists else []
            sets = {ids: ms.markerSet for ids, ms in zip(lists, built)}
        else:
            sets = {ids: [self.buildMarkerGenes(list(ids), ubiquityThreshold, singleCopyThreshold)] for ids in lists}
        out = []
        for (node, _), chain in zip(starts, chains):
            refinement = self.lineageSpecificGenesToRemove[node.label.split('|')[0]]
            binMarkerSets, refined = BinMarkerSets(node.label, BinMarkerSets.TREE_MARKER_SET), BinMarkerSets(node.label, BinMarkerSets.TREE_MARKER_SET)
            for lineageStr, ids in chain:
                markerSet = MarkerSet(0, lineageStr, len(ids), [set(cs) for cs in sets[tuple(ids)]])
                binMarkerSets.addMarkerSet(markerSet)
                refined.addMarkerSet(self._without(markerSet, refinement))
            out.append((binMarkerSets, refined))
        return out

    def buildBinMarkerSet(self, tree, curNode, ubiquityThreshold, singleCopyThreshold, bMarkerSet=True, genomeIdsToRemove=None):
        """(binMarkerSets, refinedBinMarkerSet): the marker sets of every node from curNode to the root that keeps at least two genomes
        once genomeIdsToRemove are taken out, and the same without the genes lost or duplicated in curNode's lineage (:587-634)."""
        return self._chains([(curNode, genomeIdsToRemove)], ubiquityThreshold, singleCopyThreshold, bMarkerSet)[0]

    def buildDomainMarkerSet(self, tree, curNode, ubiquityThreshold, singleCopyThreshold, bMarkerSet=True, genomeIdsToRemove=None):
        """buildBinMarkerSet over the bacterial and archaeal nodes (UID2, UID203) alone (:636-687)."""
        return self._chains([(curNode, genomeIdsToRemove)], ubiquityThreshold, singleCopyThreshold, bMarkerSet, domainOnly=True)[0]

    def buildBinMarkerSetsLOO(self, tree, testGenomeIds, ubiquityThreshold, singleCopyThreshold, bMarkerSet=True):
        """genomeId -> buildBinMarkerSet(tree, parent of the leaf 'IMG_' + genomeId, ..., genomeIdsToRemove=[genomeId]), with the genome
        lists of every (genome, ancestor) pair answered by ONE buildMarkerSets call on the resident table."""
        testGenomeIds = list(testGenomeIds)
        starts = [(tree.find_leaf('IMG_' + g).parent, [g]) for g in testGenomeIds]
        return dict(zip(testGenomeIds, self._chains(starts, ubiquityThreshold, singleCopyThreshold, bMarkerSet)))
