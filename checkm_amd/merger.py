"""`checkm merge` (checkm/merger.py): bins whose marker genes complement each other.

The reference builds a merged hit dict for every pair of bins and calls geneCounts on it -- the one quadratic step of CheckM.  Only the
individual-marker estimate is used and the merged lists are only concatenated, so a pair needs nothing but integers: which genes of
the common marker gene set each bin has (a bit row), how many hits to them, and numMarkers() of bin J's set.  This class builds one bit
row per bin and hands them to the device (ckm_merge_run: count pass, scan, fill pass; checkm_amd/csrc/kernels_merge.hip); the lines
of merger.tsv are formatted by the library in the order of the reference's loop."""
import logging
import os
import sys
import time

import numpy as np

from checkm_amd import _lib, runtime
from checkm_amd.resultsParser import ResultsParser


def checkDirExists(inputDir):
    if not os.path.exists(inputDir):
        logging.getLogger('timestamp').error('Input directory does not exists: ' + inputDir + '\n')
        sys.exit(1)


HEADER = ('Bin Id 1\tBin Id 2'
          '\tBin 1 completeness\tBin 1 contamination'
          '\tBin 2 completeness\tBin 2 contamination'
          '\tDelta completeness\tDelta contamination\tMerger delta'
          '\tMerged completeness\tMerged contamination\n')


def bin_rows(results, binIds, binIdToBinMarkerSets, genes):
    """(member [nbins, len(genes)] bool, hit_sum [nbins] int64, n_markers [nbins] int32) of the bins in `binIds` order over the sorted
    gene list `genes`.  A bin whose hit dict has not been built is read from the key ids of its kept rows (as
    ResultsParser.batchedGeneCounts does); a bin whose dict exists is read from the dict, whatever its owner did to it: a key with an
    empty list is a member.  Raises where the reference's loop does: KeyError for a bin without marker sets, ZeroDivisionError for an
    empty marker set, at the first such bin in order."""
    index = {g: k for k, g in enumerate(genes)}
    member = np.zeros((len(binIds), len(genes)), dtype=bool)
    hit_sum = np.zeros(len(binIds), dtype=np.int64)
    n_markers = np.zeros(len(binIds), dtype=np.int32)
    gene_ids = {}                      # id(KeyTable) -> (KeyTable, key id of every gene, -1 where the reduction never saw it)
    for b, binId in enumerate(binIds):
        n = binIdToBinMarkerSets[binId].mostSpecificMarkerSet().numMarkers()
        if n == 0:
            raise ZeroDivisionError('float division by zero')
        n_markers[b] = n
        rm = results[binId]
        if rm._lazy is not None:
            res, lb, keys, _to_hit = rm._lazy
            ent = gene_ids.get(id(keys))
            if ent is None:
                ent = gene_ids[id(keys)] = (keys, np.asarray([keys.ids.get(g, -1) for g in genes], dtype=np.int64))
            gid = ent[1]
            o0, o1 = int(res.kept_bin_off[lb]), int(res.kept_bin_off[lb + 1])
            kc = np.bincount(res.kept_key[o0:o1], minlength=len(keys.names) + 1) if o1 > o0 else np.zeros(len(keys.names) + 1, dtype=np.int64)
            cnt = np.where(gid >= 0, kc[gid], 0)
            member[b] = cnt > 0
            hit_sum[b] = int(cnt.sum())
        else:
            total = 0
            for m, hits in rm.markerHits.items():
                k = index.get(m)
                if k is not None:
                    member[b, k] = True
                    total += len(hits)
            hit_sum[b] = total
    return member, hit_sum, n_markers


def pack_rows(member):
    """[nbins, ngenes] bool -> [nbins, (ngenes + 63) // 64] uint64, gene g at bit g % 64 of word g // 64."""
    nb, ng = member.shape
    nwords = max(1, (ng + 63) // 64)
    by = np.zeros((nb, nwords * 8), dtype=np.uint8)
    if ng:
        packed = np.packbits(member, axis=1, bitorder='little')
        by[:, :packed.shape[1]] = packed
    return np.ascontiguousarray(by).view('<u8').astype(np.uint64, copy=False)


class Merger():
    def __init__(self):
        self.logger = logging.getLogger('timestamp')
        self.last_timing = {}

    def run(self, binFiles, outDir, hmmTableFile,
                binIdToModels, binIdToBinMarkerSets,
                minDeltaComp, maxDeltaCont,
                minMergedComp, maxMergedCont):
        checkDirExists(outDir)

        self.logger.info('Comparing marker sets between all pairs of bins.')

        # ensure all bins are using the same marker set
        markerGenesI = binIdToBinMarkerSets[list(binIdToBinMarkerSets.keys())[0]].mostSpecificMarkerSet().getMarkerGenes()
        for binIdJ in binIdToBinMarkerSets:
            if markerGenesI != binIdToBinMarkerSets[binIdJ].mostSpecificMarkerSet().getMarkerGenes():
                self.logger.error('All bins must use the same marker set to assess potential mergers.')
                sys.exit(1)

        resultsParser = ResultsParser(binIdToModels)
        resultsParser.parseBinHits(outDir, hmmTableFile)
        resultsParser._localize_remote()          # bins another process reduced: the comparison needs their hits here

        outputFile = os.path.join(outDir, "merger.tsv")
        return self.compare(resultsParser.results, binIdToBinMarkerSets, markerGenesI, outputFile,
                            minDeltaComp, maxDeltaCont, minMergedComp, maxMergedCont)

    def compare(self, results, binIdToBinMarkerSets, markerGenes, outputFile, minDeltaComp, maxDeltaCont, minMergedComp, maxMergedCont,
                budget_bytes=0):
        """The loop of checkm/merger.py:56-110 over `results` ({binId: ResultsManager}): writes outputFile, returns its path."""
        t0 = time.perf_counter()
        fout = open(outputFile, 'w')
        encoding = fout.encoding
        fout.write(HEADER)
        fout.close()

        binIds = sorted(results.keys())
        genes = sorted(markerGenes)
        member, hit_sum, n_markers = bin_rows(results, binIds, binIdToBinMarkerSets, genes)
        bits = pack_rows(member)
        t1 = time.perf_counter()
        ids = [b.encode(encoding) for b in binIds]
        out = _lib.merge_pairs(runtime.get_ctx(), bits, hit_sum, n_markers, len(genes),
                               (minDeltaComp, maxDeltaCont, minMergedComp, maxMergedCont), bin_ids=ids, append_path=outputFile,
                               budget_bytes=budget_bytes, keep_columns=False) if binIds else dict(npairs=0, compared=0, nbatches=0)
        t2 = time.perf_counter()
        self.last_timing = dict(out, s_rows=t1 - t0, s_device_and_write=t2 - t1, s_total=t2 - t0, bins=len(binIds), genes=len(genes))
        return outputFile
