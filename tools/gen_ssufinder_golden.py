#!/usr/bin/env python
"""Goldens of the SSU_Finder post-processing (tests/golden/ssufinder_cases.json).

Every case runs the reference's own SSU_Finder.run (checkm/ssuFinder.py:200-297) with its `_hmmSearch` replaced by a stand-in that logs
the three lines the original logs and writes, for the listed hits, reports of the shape the reference's `_readHits` parses (a '>>' line
per hit, two heading lines, the hit line with the E-value in field 3 and the alignment coordinates in fields 7 and 8, a blank line).
Everything after that -- _readHits, _addHit, _addDomainHit, the relabelling, the bin assignment and the two files -- runs unchanged.
Recorded: the inputs, ssu_summary.tsv, ssu.fna and the log lines (the output directory written as <out>).  This is the only place the
reference is read.  Runs only where a CheckM source tree is at hand; the tests read the JSON.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_ssufinder_golden.py"""
import gzip
import json
import logging
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ssufinder_synth as syn      # noqa: E402

LABELS = (('bacteria', 'Identifying bacterial 16S.'), ('archaea', 'Identifying archaeal 16S.'), ('euk', 'Identifying eukaryotic 18S.'))


def fasta(records):
    return ''.join('>%s\n%s\n' % (name, seq) for name, seq in records)


def cases():
    rng = np.random.default_rng(2024)
    contigs = [(name, syn.random_dna(rng, n)) for name, n in (('c1', 2400), ('c11', 2100), ('c2', 1900), ('scaffold_7 len=1800', 1800), ('x_y', 1700))]
    ids = [c[0].split()[0] for c in contigs]
    bins = [('binA.fna', fasta([contigs[0], contigs[2]])), ('binB.fa', fasta([contigs[1]]))]
    all_bins = bins + [('binC.fna', fasta(contigs[3:]))]

    def case(name, hits, evalue=1e-5, concatenate=200, contig_name='contigs.fna', bins_=None):
        full = {'bacteria': [], 'archaea': [], 'euk': []}
        full.update(hits)
        return dict(name=name, contig_name=contig_name, contig_text=fasta(contigs), bins=[list(b) for b in (bins if bins_ is None else bins_)], hits=full, evalue=evalue, concatenate=concatenate)

    return [
        case('concat_inside', {'bacteria': [[ids[0], '1e-50', 100, 600], [ids[0], '3e-40', 650, 1200], [ids[2], '2e-30', 900, 1500], [ids[2], '2e-20', 500, 760]]}),
        case('concat_outside', {'bacteria': [[ids[0], '1e-50', 100, 600], [ids[0], '3e-40', 1000, 1500], [ids[0], '3e-30', 800, 801]], 'euk': [[ids[1], '1e-9', 10, 900]]}, concatenate=199),
        case('numbered_names', {'archaea': [[ids[0], '1e-50', 100, 400], [ids[0], '1e-40', 900, 1200], [ids[0], '1e-30', 1700, 2000], [ids[0], '1e-20', 2100, 2300], [ids[0], '1e-10', 1300, 1400]],
                                'bacteria': [[ids[4], '1e-12', 200, 700], [ids[4], '1e-11', 1200, 1600]]}, concatenate=150, bins_=all_bins),
        case('substring_ids', {'archaea': [[ids[1], '1e-50', 100, 900]], 'bacteria': [[ids[0], '1e-40', 300, 800], [ids[1], '1e-30', 1200, 1300]], 'euk': [[ids[0], '1e-20', 1000, 2000], [ids[1], '1e-8', 50, 1000]]}),
        case('domain_longer_wins', {'archaea': [[ids[0], '1e-30', 200, 900], [ids[2], '1e-9', 100, 300]], 'bacteria': [[ids[0], '1e-50', 100, 1500]], 'euk': [[ids[2], '1e-7', 300, 1200]]}),
        case('domain_longer_loses', {'archaea': [[ids[0], '1e-50', 100, 1500]], 'bacteria': [[ids[0], '1e-30', 200, 900], [ids[0], '1e-20', 1500, 1900]], 'euk': [[ids[0], '1e-10', 100, 1500]]}),
        case('reverse_strand', {'bacteria': [[ids[0], '1e-50', 1600, 100], [ids[2], '1e-40', 900, 300], [ids[2], '1e-30', 1000, 1700]], 'archaea': [[ids[1], '2e-20', 2100, 1]]}),
        case('unbinned', {'bacteria': [[ids[3], '1e-50', 100, 1600], [ids[4], '1e-45', 5, 1500], [ids[0], '1e-40', 1, 2400]], 'euk': [[ids[3], '1e-12', 1650, 1790]]}),
        case('evalue_equal', {'bacteria': [[ids[0], '1e-05', 100, 1600], [ids[2], '1.1e-05', 100, 1600], [ids[1], '9.9e-06', 1500, 30]], 'archaea': [[ids[2], '1e-5', 200, 1000]]}, evalue=1e-5),
        case('gz_contigs', {'bacteria': [[ids[0], '1e-50', 100, 1600]], 'archaea': [[ids[3], '1e-30', 1700, 200]]}, contig_name='contigs.fna.gz', bins_=all_bins),
    ]


def report(hits):
    out = ['# stand-in report\n', '\n']
    for seqId, evalue, aliFrom, aliTo in hits:
        out.append('>> %s  \n' % seqId)
        out.append('    score  bias    Evalue   hmmfrom    hmm to     alifrom    ali to      envfrom    env to       sq len      acc\n')
        out.append('   ------ ----- ---------   -------   -------    --------- ---------    --------- ---------    ---------    ----\n')
        out.append(' !  100.0   1.0 %9s         1      1500 [] %9d %9d .. %9d %9d ..      3000    0.99\n' % (evalue, aliFrom, aliTo, aliFrom, aliTo))
        out.append('\n')
    return ''.join(out)


class Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def main():
    src = os.environ.get('CHECKM_SOURCE')
    if not src:
        sys.exit('set CHECKM_SOURCE to a CheckM source tree')
    sys.path.insert(0, src)
    from checkm.ssuFinder import SSU_Finder
    done = []
    for case in cases():
        with tempfile.TemporaryDirectory() as d:
            contig = os.path.join(d, case['contig_name'])
            with (gzip.open if contig.endswith('.gz') else open)(contig, 'wt') as f:
                f.write(case['contig_text'])
            binFiles = []
            for name, text in case['bins']:
                binFiles.append(os.path.join(d, name))
                with open(binFiles[-1], 'w') as f:
                    f.write(text)
            finder = SSU_Finder(1)

            def stand_in(seqFile, evalue, outputPrefix, finder=finder, case=case):
                for domain, line in LABELS:
                    finder.logger.info(line)
                    with open(outputPrefix + '.' + domain + '.txt', 'w') as f:
                        f.write(report(case['hits'][domain]))
            finder._hmmSearch = stand_in
            cap = Capture()
            finder.logger.addHandler(cap)
            finder.logger.setLevel(logging.INFO)
            out = os.path.join(d, 'out')
            finder.run(contig, binFiles, out, case['evalue'], case['concatenate'])
            finder.logger.removeHandler(cap)
            case['summary'] = open(os.path.join(out, 'ssu_summary.tsv')).read()
            case['fna'] = open(os.path.join(out, 'ssu.fna')).read()
            case['log'] = [ln.replace(out, '<out>') for ln in cap.lines]
            done.append(case)
    path = os.path.join(ROOT, 'tests', 'golden', 'ssufinder_cases.json')
    with open(path, 'w') as f:
        json.dump(done, f, indent=1)
        f.write('\n')
    print('wrote %s: %d cases' % (path, len(done)))


if __name__ == '__main__':
    main()
