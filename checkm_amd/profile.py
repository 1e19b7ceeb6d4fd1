"""`checkm profile` (checkm/profile.py): percentage of the mapped reads that belong to each bin, from a coverage file.

Host arithmetic on a small table; every division and product is evaluated in the reference's order so that str() of a value gives the
reference's digits.  The framed table of the non-tab mode is common.frame_table, which qa's table uses too."""
import logging
import sys

from checkm_amd.common import checkFileExists, frame_table
from checkm_amd.defaultValues import DefaultValues


class Profile():
    def __init__(self):
        self.logger = logging.getLogger('timestamp')

    def run(self, coverageFile, outFile, bTabTable):
        checkFileExists(coverageFile)

        self.logger.info('Determining number of reads mapped to each bin.')

        readsMappedToBin, binSize, totalMappedReads = {}, {}, {}
        with open(coverageFile) as f:
            next(f, None)
            for line in f:
                lineSplit = line.split('\t')
                binId = lineSplit[1]
                binSize[binId] = binSize.get(binId, 0) + int(lineSplit[2])
                perBam = readsMappedToBin.setdefault(binId, {})
                for i in range(3, len(lineSplit), 3):
                    bamId, mappedReads = lineSplit[i], int(lineSplit[i + 2])
                    totalMappedReads[bamId] = totalMappedReads.get(bamId, 0) + mappedReads
                    perBam[bamId] = perBam.get(bamId, 0) + mappedReads

        # share of the mapped reads per bin, and that share per base, normalised over the binned populations
        perMappedReads, normBinCoverage, sumNormBinCoverage = {}, {}, {}
        for binId, bamIds in readsMappedToBin.items():
            perMappedReads[binId], normBinCoverage[binId] = {}, {}
            for bamId in bamIds:
                perMR = float(bamIds[bamId]) / totalMappedReads[bamId]
                perMappedReads[binId][bamId] = perMR
                if binId == DefaultValues.UNBINNED:
                    continue
                normCoverage = perMR / binSize[binId]
                normBinCoverage[binId][bamId] = normCoverage
                sumNormBinCoverage[bamId] = sumNormBinCoverage.get(bamId, 0) + normCoverage
        for binId, bamIds in normBinCoverage.items():
            for bamId in bamIds:
                if sumNormBinCoverage[bamId] != 0:
                    bamIds[bamId] /= sumNormBinCoverage[bamId]
                else:
                    bamIds[bamId] = 0

        sortedBinIds = sorted(readsMappedToBin.keys())
        sortedBamIds = sorted(readsMappedToBin[sortedBinIds[0]].keys())
        header = ['Bin Id', 'Bin size (Mbp)']
        for bamId in sortedBamIds:
            header += [bamId + s for s in (': mapped reads', ': % mapped reads', ': % binned populations', ': % community')]

        rows = []
        unbinned = perMappedReads.get(DefaultValues.UNBINNED)
        for binId in sortedBinIds:
            row = [binId, float(binSize[binId]) / 1e6]
            for bamId in sortedBamIds:
                unbinnedPercentage = unbinned[bamId] if unbinned is not None else 0
                row += [readsMappedToBin[binId][bamId], perMappedReads[binId][bamId] * 100.0]
                if binId == DefaultValues.UNBINNED:
                    row += ['NA', unbinnedPercentage * 100.0]
                else:
                    row += [normBinCoverage[binId][bamId] * 100.0, normBinCoverage[binId][bamId] * 100.0 * (1.0 - unbinnedPercentage)]
            rows.append(row)

        if bTabTable:
            text = '\n'.join(['\t'.join(header)] + ['\t'.join(map(str, row)) for row in rows]) + '\n'
        else:
            text = frame_table(header, rows) + '\n'
        if outFile != '':
            try:
                fout = open(outFile, 'w')
            except Exception:
                self.logger.error("Error diverting stdout to file: " + outFile)
                sys.exit(1)
            with fout:
                fout.write(text)
        else:
            sys.stdout.write(text)
