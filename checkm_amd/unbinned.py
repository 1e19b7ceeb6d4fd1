"""`checkm unbinned`: the contigs of an assembly that sit in no bin (checkm/unbinned.py:33-85), with the same two files, the same log
lines and the same failures.

The bin files are read for their ids and lengths only (ckm_fasta_ids_read: no sequence text is kept), the assembly with the rules of
CheckM's readFasta (ckm_nucseq_read), the selection is a hash set on the host (ckm_unbinned_select), baseCount of the kept contigs is
counted on the device (ckm_unbinned_count: only their tiles travel) and both files are written by the library from the reader's own
buffers (ckm_unbinned_write).  There is no CPU path for the device pass.

Declared difference: U+1E97 and U+1E9A, whose upper-casing yields a 'T' / an 'A' followed by a combining mark, do not count as T / A
(DESIGN §12, §19).
"""
import logging
import math
import os
import sys
import time

from checkm_amd import _lib


class Unbinned():
    def __init__(self):
        self.logger = logging.getLogger('timestamp')
        self.last_timing = {}

    def run(self, binFiles, seqFile, outSeqFile, outStatsFile, minSeqLen):
        if not os.path.exists(seqFile):                          # checkFileExists (checkm/common.py:106-111), with its line end
            self.logger.error('Input file does not exists: ' + seqFile + '\n')
            sys.exit(1)
        from checkm_amd import runtime
        try:
            ctx = runtime.get_ctx()
        except Exception as e:
            self.logger.error("No usable MI355X (gfx950) device for the base counts: %s" % e)
            sys.exit(1)
        t = dict(read_bins=0.0, read_assembly=0.0, select=0.0, stage=0.0, copy_in=0.0, kernel=0.0, copy_out=0.0, count=0.0, write=0.0)
        bins = seqs = None
        try:
            # get list of sequences in bins
            self.logger.info('Reading binned sequences.')
            t0 = time.perf_counter()
            bins = self._read(_lib.FastaIds, list(binFiles))
            _keep, tot = _lib.unbinned_select(bins, None, 0)
            t1 = time.perf_counter()
            self.logger.info('  Read %d (%.2f Mbp) binned sequences.' % (tot['binned_ids'], float(tot['binned_bases']) / 1e6))

            # get list of all sequences
            self.logger.info('Reading all sequences.')
            seqs = self._read(_lib.NucSeqs, [seqFile])
            t2 = time.perf_counter()
            keep, tot = _lib.unbinned_select(bins, seqs, math.ceil(minSeqLen))
            t3 = time.perf_counter()
            self.logger.info('  Read %d (%.2f Mbp) sequences.' % (tot['all_seqs'], float(tot['all_bases']) / 1e6))

            # write all unbinned sequences
            self.logger.info('Identifying unbinned sequences >= %d bp.' % minSeqLen)
            open(outSeqFile, 'w').close()                        # a path that cannot be written fails as the reference's open() does
            open(outStatsFile, 'w').close()
            r = _lib.unbinned_count(ctx, seqs, keep)
            t4 = time.perf_counter()
            zero = _lib.unbinned_write(seqs, keep, r['counts'], outSeqFile, outStatsFile)
            t5 = time.perf_counter()
            t.update(read_bins=t1 - t0, read_assembly=t2 - t1, select=t3 - t2, stage=r['ms_stage'] / 1e3, copy_in=r['ms_upload'] / 1e3,
                     kernel=(r['ms_count'] + r['ms_sum']) / 1e3, copy_out=r['ms_download'] / 1e3, count=t4 - t3, write=t5 - t4, bins=len(binFiles),
                     sequences=tot['all_seqs'], kept=int(r['kept']), tiles=int(r['tiles']), batches=int(r['batches']), bytes=int(r['bytes']))
            self.last_timing = t
            if zero >= 0:
                float(0) * 100 / 0                               # the reference's row of a kept sequence without A, C, G, T or U
        finally:
            for b in (bins, seqs):
                if b is not None:
                    b.close()

        self.logger.info('  Identified %d (%.2f Mbp) unbinned sequences.' % (tot['unbinned_seqs'], float(tot['unbinned_bases']) / 1e6))

        self.logger.info('Percentage of unbinned sequences: %.2f%%' % (tot['unbinned_seqs'] * 100.0 / tot['all_seqs']))
        self.logger.info('Percentage of unbinned bases: %.2f%%' % (tot['unbinned_bases'] * 100.0 / tot['all_bases']))

    def _read(self, reader, paths):
        try:
            return reader(paths)
        except _lib.CkmError as e:
            print(e)
            self.logger.error("Failed to process sequence file: %s" % e)
            sys.exit(1)
