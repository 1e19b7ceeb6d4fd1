"""IMG, the reader of per-genome annotation tables, with the results of checkm/util/img.py for the methods MarkerSetBuilder needs:
geneCountTable (:254-287), filterGeneCountTable (:289-309), familyIdToGeneId (:383-395), _genomeSeqLens (:397-406),
_genomeFamilyPositions (:420-490), the two precompute methods (:408-418, :492-499), geneDistTable (:501-530), the two redundancy
filters (:555-589), and for the scaffold simulation filterGenomeIds (:42-48), geneIdToScaffoldId (:50-65), _genomeIdToClusterScaffold
(:311-370) and precomputeGenomeFamilyScaffolds (:372-381), and for the genome tree genomeMetadata / genomeMetadataFromFile (:91-163).
Plain host code.

A genome <id> is a directory <genomeDir>/<id>/ with <id>.pfam.tab.txt (family in column 8), <id>.tigrfam.tab.txt (family in column
6), <id>.gff and <id>.fna.  As in the reference: the first line of an annotation table is a header; a column is taken as it stands
between two tabs (the last column of a line keeps its line end); a family is counted once per gene however many of the gene's rows
name it; a GFF line that starts with '#' or does not have nine fields is skipped; the gene id is what follows the first '=' of the
first ';'-separated part of field nine; a contig's offset grows by spacingBetweenContigs plus the length of the contig just left each
time field one changes; only genes with a GFF record have a position, and a family without one is absent from the result.

The order of the copies of a family is the order of the sorted gene ids here (the reference's is the iteration order of a set of
strings); nothing computed from them depends on it.  The genome directory is a constructor argument (the reference's is a class
attribute that holds a path of its authors' machine)."""
from collections import defaultdict
import logging
import os


class IMG(object):
    genomeDir = None
    pfamExtension = '.pfam.tab.txt'
    tigrExtension = '.tigrfam.tab.txt'

    def __init__(self, imgMetadataFile, redundantTIGRFAMsFile, genomeDir=None):
        self.logger = logging.getLogger()
        self.metadataFile = imgMetadataFile
        self.redundantTIGRFAMs = redundantTIGRFAMsFile
        if genomeDir is not None:
            self.genomeDir = genomeDir
        self.cachedGenomeSeqLens = None
        self.cachedGenomeFamilyPositions = None
        self.cachedGenomeFamilyScaffolds = None

    def _path(self, genomeId, suffix):
        return os.path.join(self.genomeDir, genomeId, genomeId + suffix)

    # ---- metadata -------------------------------------------------------------------------------------------------------------------
    def genomeMetadata(self):
        return self.genomeMetadataFromFile(self.metadataFile)

    def genomeMetadataFromFile(self, metadataFile):
        """genome -> its row of the metadata table (:91-163), in file order: 'status', 'taxonomy' (the seven ranks from Domain to
        Species), 'scaffold count', 'GC Count', 'GC %', 'genome size', 'gene count', 'coding base count', 'biotic relationships', 'N50'.
        Columns are found by their header; every field is stripped; a count that is no integer is 'NA', as in the reference."""
        def number(text, kind=int):
            try:
                return kind(text)
            except ValueError:
                return 'NA'

        metadata, col = {}, None
        ranks = ('Domain', 'Phylum', 'Class', 'Order', 'Family', 'Genus', 'Species')
        with open(metadataFile) as f:
            for line in f:
                fields = [x.strip() for x in line.split('\t')]
                if col is None:
                    col = {name: fields.index(name) for name in ('Status', 'Scaffold Count', 'GC Count', 'Genome Size', 'Gene Count', 'Coding Base Count',
                                                                 'Biotic Relationships', 'N50') + ranks}
                    continue
                gc, size = number(fields[col['GC Count']]), number(fields[col['Genome Size']])
                metadata[fields[0]] = {'status': fields[col['Status']], 'taxonomy': [fields[col[r]] for r in ranks], 'scaffold count': int(fields[col['Scaffold Count']]),
                                       'GC Count': gc if gc != 'NA' and size not in ('NA', 0) else 'NA',
                                       'GC %': float(fields[col['GC Count']]) / size if gc != 'NA' and size not in ('NA', 0) else 'NA',
                                       'genome size': size, 'gene count': number(fields[col['Gene Count']]), 'coding base count': number(fields[col['Coding Base Count']]),
                                       'biotic relationships': fields[col['Biotic Relationships']], 'N50': int(fields[col['N50']])}
        return metadata

    def filterGenomeIds(self, genomeIds, metadata, fieldToFilterOn, valueToRetain):
        return set(g for g in genomeIds if metadata[g][fieldToFilterOn] == valueToRetain)

    # ---- scaffolds ------------------------------------------------------------------------------------------------------------------
    def _gff_genes(self, genomeId):
        """(scaffold id, gene id, fields) of every GFF record, by this module's GFF rule."""
        with open(self._path(genomeId, '.gff')) as f:
            for line in f:
                if line[0] == '#':
                    continue
                fields = line.split('\t')
                if len(fields) != 9:
                    continue
                tag = fields[8].split(';')[0]
                yield fields[0], tag[tag.find('=') + 1:], fields

    def geneIdToScaffoldId(self, genomeId):
        """gene -> scaffold (:50-65).  The reference indexes field nine of every line and cuts the gene id at the first ';'; on records
        of nine fields with a ';' the two rules agree, and a line of fewer fields is skipped here where the reference fails."""
        return {geneId: scaffoldId for scaffoldId, geneId, _ in self._gff_genes(genomeId)}

    def _genomeIdToClusterScaffold(self, genomeId):
        """family -> [scaffold id, ...] of its genes that have a GFF record, one entry per gene (:311-370); a family none of whose
        genes has a record is absent.  The copies follow the sorted gene ids.  The reference keeps a TIGRFAM by the record of the gene
        its set of gene ids happens to yield last (:362 tests `scaffold`, not `scaffolds`), which is the Pfam rule whenever all genes of
        the family or none have a record; the Pfam rule is applied to both tables here."""
        where = self.geneIdToScaffoldId(genomeId)
        out = {}
        for extension, column in ((self.pfamExtension, 8), (self.tigrExtension, 6)):
            for familyId, geneIds in self.familyIdToGeneId(self._path(genomeId, extension), column).items():
                scaffolds = [where[g] for g in sorted(geneIds) if g in where]
                if scaffolds:
                    out[familyId] = scaffolds
        return out

    def precomputeGenomeFamilyScaffolds(self, genomeIds):
        self.cachedGenomeFamilyScaffolds = {g: self._genomeIdToClusterScaffold(g) for g in genomeIds}
        return self.cachedGenomeFamilyScaffolds

    # ---- counts ---------------------------------------------------------------------------------------------------------------------
    def _count_families(self, table, genomeIds, extension, column):
        for genomeId in genomeIds:
            genes = defaultdict(set)                    # family -> genes that carry it
            with open(self._path(genomeId, extension)) as f:
                f.readline()
                for line in f:
                    fields = line.split('\t')
                    genes[fields[column]].add(fields[0])
            for familyId, members in genes.items():
                table.setdefault(familyId, {})[genomeId] = len(members)

    def geneCountTable(self, genomeIds):
        """family -> genome -> genes annotated with it; the TIGRFAM table is read after the Pfam table."""
        table = {}
        self._count_families(table, genomeIds, self.pfamExtension, 8)
        self._count_families(table, genomeIds, self.tigrExtension, 6)
        return table

    def filterGeneCountTable(self, genomeIds, table, ubiquityThreshold=0.9, singleCopyThreshold=0.9):
        """Drops, in place, the families below either fraction; an empty genome list divides by zero as the reference does."""
        drop = []
        for familyId, counts in table.items():
            present = sum(1 for g in genomeIds if counts.get(g, 0) > 0)
            single = sum(1 for g in genomeIds if counts.get(g, 0) == 1)
            if float(present) / len(genomeIds) < ubiquityThreshold or float(single) / len(genomeIds) < singleCopyThreshold:
                drop.append(familyId)
        for familyId in drop:
            del table[familyId]
        return table

    def familyIdToGeneId(self, filename, clusterIdIndex):
        families = defaultdict(set)
        with open(filename) as f:
            f.readline()
            for line in f:
                fields = line.split('\t')
                families[fields[clusterIdIndex]].add(fields[0])
        return families

    # ---- positions ------------------------------------------------------------------------------------------------------------------
    def _genomeSeqLens(self, genomeId):
        """sequence id -> length, in the order of the FASTA file: numpy's choice in the scaffold samplers sees list(seqLens.keys())."""
        return {seqId: len(seq) for seqId, seq in _read_fna(self._path(genomeId, '.fna')).items()}

    def precomputeGenomeSeqLens(self, genomeIds):
        self.cachedGenomeSeqLens = {g: self._genomeSeqLens(g) for g in genomeIds}
        return self.cachedGenomeSeqLens

    def _genomeFamilyPositions(self, genomeId, seqLens, spacingBetweenContigs):
        """family -> [[start, end], ...] of its genes that have a GFF record, in whole-genome coordinates."""
        where = {}
        offset, contig = 0, None
        with open(self._path(genomeId, '.gff')) as f:
            for line in f:
                if line[0] == '#':
                    continue
                fields = line.split('\t')
                if len(fields) != 9:
                    continue
                if contig is None:
                    contig = fields[0]
                if fields[0] != contig:
                    offset += spacingBetweenContigs + seqLens[contig]
                    contig = fields[0]
                tag = fields[8].split(';')[0]
                where[tag[tag.find('=') + 1:]] = [offset + int(fields[3]), offset + int(fields[4])]
        out = {}
        for extension, column in ((self.pfamExtension, 8), (self.tigrExtension, 6)):
            for familyId, geneIds in self.familyIdToGeneId(self._path(genomeId, extension), column).items():
                copies = [where[g] for g in sorted(geneIds) if g in where]
                if copies:
                    out[familyId] = copies
        return out

    def precomputeGenomeFamilyPositions(self, genomeIds, spacingBetweenContigs):
        self.cachedGenomeFamilyPositions = {g: self._genomeFamilyPositions(g, self.cachedGenomeSeqLens[g], spacingBetweenContigs) for g in genomeIds}

    def geneDistTable(self, genomeIds, markerGenes, spacingBetweenContigs=0):
        """genome -> marker -> copies.  A cache that is not empty is used whatever spacing it was made with, as in the reference."""
        table = {}
        for genomeId in genomeIds:
            seqLens = self.cachedGenomeSeqLens[genomeId] if self.cachedGenomeSeqLens else self._genomeSeqLens(genomeId)
            if self.cachedGenomeFamilyPositions:
                positions = self.cachedGenomeFamilyPositions[genomeId]
            else:
                positions = self._genomeFamilyPositions(genomeId, seqLens, spacingBetweenContigs)
            table[genomeId] = {m: positions[m] for m in markerGenes if m in positions}
        return table

    # ---- redundancy between TIGRFAMs and Pfams -----------------------------------------------------------------------------------------
    def _redundant_pairs(self):
        pairs = []
        with open(self.redundantTIGRFAMs) as f:
            for line in f:
                fields = line.split('\t')
                pairs.append((fields[0], fields[1].rstrip()))
        return pairs

    def identifyRedundantPFAMs(self, markerGenes):
        return set(pfam for pfam, tigr in self._redundant_pairs() if pfam in markerGenes and tigr in markerGenes)

    def identifyRedundantTIGRFAMs(self, markerGenes):
        return set(tigr for pfam, tigr in self._redundant_pairs() if tigr in markerGenes and pfam in markerGenes)


def _read_fna(path):
    """id -> sequence as the reference's readFasta reads it (checkm/util/seqUtils.py:180-211): ids cut at the first whitespace, blank
    lines skipped, the last character of every sequence line dropped as its line end."""
    seqs, cur = {}, None
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            if line[0] == '>':
                cur = line[1:].split(None, 1)[0]
                seqs[cur] = []
            else:
                seqs[cur].append(line[:-1])
    return {k: ''.join(v) for k, v in seqs.items()}
