#!/usr/bin/env python
"""Goldens of MarkerSetBuilder: the reference's own checkm.util.img.IMG and the class of scripts/genometreeworkflow/markerSetBuilder.py over
small hand-made genome directories.  The script is Python 2 and does not compile as it stands; it is loaded in memory after four textual
substitutions (SUBSTITUTIONS below, each checked to hit) and never written to disk.  Its __init__ reads files of its authors' machine, so
the object is made without it and given an IMG whose class attribute genomeDir points at the case's temporary tree.  Per case: the texts
of the annotation files (a genome whose files repeat another's is stored as a reference to it), the parameters, the gene count
table, the markers before and after the TIGRFAM redundancy removal, geneDistTable,
the co-located pairs and sets, genomeCheck per genome (floats as float.hex()), missing and duplicate genes, buildMarkerSet, what was
printed, and a failure by type and args.  Lists whose order came from a dict or a set are stored sorted.  Runs only where a CheckM source
tree is at hand; the tests read the JSON.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_markerset_golden.py                  (writes tests/golden/markerset_cases.json)
       CHECKM_SOURCE=<checkm source> python tools/gen_markerset_golden.py --time --genomes N --markers M
                                      (times the reference's colocatedGenes on one core over a synthetic geneDistTable, writes
                                       profiles/r17_markerset_reference_cpu.json)"""
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (what, pattern, replacement): Python 2 -> 3, nothing else
SUBSTITUTIONS = [("dict.iteritems", r"\.iteritems\(\)", ".items()"),
                 ("xrange", r"\bxrange\(", "range("),
                 ("print statements", r"(?m)^(\s*)print (['\"].*?)\s*$", r"\1print(\2)"),
                 ("keys() sliced as a list", r"(clusterIds = )(\w+\.keys\(\))", r"\1list(\2)")]
EXPECTED_HITS = {"print statements": 2, "keys() sliced as a list": 1}


def load_builder(source):
    """The reference's MarkerSetBuilder class, compiled from the translated text in memory."""
    text = open(os.path.join(source, "scripts", "genometreeworkflow", "markerSetBuilder.py")).read()
    for what, pattern, repl in SUBSTITUTIONS:
        text, n = re.subn(pattern, repl, text)
        if n < 1 or n != EXPECTED_HITS.get(what, n):
            raise SystemExit("substitution '%s' hit %d times" % (what, n))
    ns = {"__name__": "reference_markerSetBuilder"}
    exec(compile(text, "<markerSetBuilder.py, translated in memory>", "exec"), ns)
    return ns["MarkerSetBuilder"]


# ---- the genome directories ------------------------------------------------------------------------------------------------------------
def genome(contigs, pfam_extra=(), tigr_extra=(), gff_extra=()):
    """contigs: [(contig id, length, [(gene id, start, end, [pfams], [tigrfams]), ...]), ...] -> the four file texts of a genome.
    pfam_extra / tigr_extra: further (gene, family) rows; gff_extra: raw lines put behind the first gene."""
    fna, gff, pfam, tigr = [], ["##gff-version 3\n"], ["gene_oid\tgene_length\tpercent_identity\tquery_start\tquery_end\tsubj_start\tsubj_end\tevalue\tpfam_id\tpfam_name\n"], \
        ["gene_oid\tgene_length\tpercent_identity\tquery_start\tquery_end\tevalue\ttigrfam_id\ttigrfam_name\n"]
    first = True
    for cid, length, genes in contigs:
        fna.append(">%s some description\n" % cid)
        seq = "ACGT" * (length // 4) + "A" * (length % 4)
        fna.extend(seq[k:k + 60] + "\n" for k in range(0, length, 60))
        for gid, start, end, pfams, tigrs in genes:
            gff.append("%s\timg\tCDS\t%d\t%d\t.\t+\t0\tID=%s;locus_tag=L_%s\n" % (cid, start, end, gid, gid))
            if first:
                gff.extend(gff_extra)
                first = False
            pfam.extend(pfam_row(gid, f) for f in pfams)
            tigr.extend(tigr_row(gid, f) for f in tigrs)
    pfam.extend(pfam_row(g, f) for g, f in pfam_extra)
    tigr.extend(tigr_row(g, f) for g, f in tigr_extra)
    return {".fna": "".join(fna), ".gff": "".join(gff), ".pfam.tab.txt": "".join(pfam), ".tigrfam.tab.txt": "".join(tigr)}


def pfam_row(gene, family):
    return "%s\t300\t55.0\t1\t100\t1\t100\t1e-20\t%s\tname of %s\n" % (gene, family, family)


def tigr_row(gene, family):
    return "%s\t300\t55.0\t1\t100\t1e-20\t%s\tname of %s\n" % (gene, family, family)


def tree(genomes):
    """genome id -> file texts  ->  (relative path -> text of the distinct genomes, genome id -> the genome whose files it repeats)"""
    files, same_as, first = {}, {}, {}
    for g in sorted(genomes):
        key = json.dumps(genomes[g], sort_keys=True)
        if key in first:
            same_as[g] = first[key]
        else:
            first[key] = g
            files.update(("%s/%s%s" % (g, g, ext), text) for ext, text in genomes[g].items())
    return files, same_as


def all_files(c):
    """relative path -> text of every genome of a case: the files written out, and the genomes that repeat another's under their own id"""
    out = dict(c["files"])
    for g, src in c["same_as"].items():
        out.update(("%s/%s%s" % (g, g, rel[len(src) * 2 + 1:]), text) for rel, text in c["files"].items() if rel.startswith(src + "/"))
    return out


def case(name, genomes, genomeIds=None, ubiquity=0.97, single=0.97, spacing=5000, redundant="", **extra):
    files, same_as = tree(genomes)
    return dict(dict(name=name, files=files, same_as=same_as, genomeIds=sorted(genomes) if genomeIds is None else genomeIds, ubiquity=ubiquity, single=single, spacing=spacing,
                     redundant=redundant, dist_threshold=5000, genome_threshold=0.95, missing_threshold=0.5, cache=False), **extra)


def simple(markers):
    """One contig, one gene per (family, start)."""
    return genome([("c1", 40, [("g%d" % k, s, s + 900, [f] if f.startswith("pfam") else [], [] if f.startswith("pfam") else [f]) for k, (f, s) in enumerate(markers)])])


def cases():
    c = []
    # families with 0, 1, 2 and 5 copies (pfam00005 and pfam00006 are near each other in G1 only through a later copy of each); a gene that
    # carries two families (distance 0); a family row repeated for one gene (counted once); a family whose only gene has no GFF record
    # (counted, no position); a GFF line of eight fields
    g1 = genome([("c1", 130, [("a1", 100, 1000, ["pfam00001", "pfam00002"], ["TIGR00001"]), ("a2", 3000, 3900, ["pfam00003"], []), ("a3", 9000, 9900, ["pfam00004"], []),
                              ("a4", 20000, 20900, ["pfam00005"], []), ("a5", 40000, 40900, ["pfam00005"], []), ("a6", 50000, 50900, ["pfam00006"], []),
                              ("a7", 44000, 44900, ["pfam00006"], []), ("a8", 54000, 54900, ["pfam00006"], []), ("a9", 56000, 56900, ["pfam00006"], []),
                              ("a10", 58000, 58900, ["pfam00006"], [])])],
                pfam_extra=[("a1", "pfam00001"), ("ghost", "pfam00007")], gff_extra=["c1\timg\tCRISPR\t500\t700\t.\t+\t0\n"])
    g2 = genome([("c1", 130, [("b1", 200, 1100, ["pfam00001", "pfam00002"], ["TIGR00001"]), ("b2", 3100, 3900, ["pfam00003"], []), ("b3", 9100, 9900, ["pfam00004"], []),
                              ("b4", 30000, 30900, ["pfam00005"], []), ("b5", 31000, 31900, ["pfam00006"], [])])], pfam_extra=[("ghost", "pfam00007")])
    c.append(case("copies", {"G1": g1, "G2": g2}, ubiquity=1.0, single=0.5))
    # markers on two contigs: with spacing 0 the second contig's gene is 130 + 100 - 50 away from the first's, with 5000 it is beyond the threshold
    two = lambda s: genome([("c1", 130, [("x1", 50, 120, ["pfam00010"], [])]), ("c2", 90, [("x2", 100, 160, ["pfam00011"], []), ("x3", 4000, 4100, ["pfam00012"], [])])])
    c.append(case("contigs_spacing_0", {"G1": two(0), "G2": two(0)}, spacing=0))
    c.append(case("contigs_spacing_5000", {"G1": two(0), "G2": two(0)}, spacing=5000))
    # distances of exactly 4999, 5000 and 5001 from pfam00020
    edge = simple([("pfam00020", 10000), ("pfam00021", 14999), ("pfam00022", 15000), ("pfam00023", 4999), ("pfam00024", 25000)])
    c.append(case("distance_edges", {"G1": edge, "G2": edge}))
    # counts exactly on the threshold: 19 of 20 is not above 0.95, 20 of 20 is; one genome without any marker still counts in the denominator
    near, far, none = simple([("pfam00030", 1000), ("pfam00031", 2000), ("pfam00032", 3000)]), simple([("pfam00030", 1000), ("pfam00031", 2000), ("pfam00032", 90000)]), \
        genome([("c1", 40, [("z1", 10, 20, ["pfam09999"], [])])])
    c.append(case("nineteen_of_twenty", dict([("G%02d" % k, near) for k in range(19)] + [("G19", far)]), ubiquity=0.9, single=0.9))
    c.append(case("empty_genome_in_denominator", dict([("G%02d" % k, near) for k in range(19)] + [("G19", none)]), ubiquity=0.9, single=0.9, genome_threshold=0.9))
    # 96 of 100 is above 0.95, 95 of 100 is not
    hundred = dict(("H%03d" % k, simple([("pfam00040", 1000), ("pfam00041", 2000 if k < 96 else 80000), ("pfam00042", 3000 if k < 95 else 70000)])) for k in range(100))
    c.append(case("ninetysix_of_hundred", hundred, ubiquity=0.97, single=0.97))
    # a TIGRFAM that is redundant with a Pfam marker is removed; one whose Pfam is no marker stays; chains of pairs join into one set
    red = simple([("pfam00050", 1000), ("TIGR00050", 1500), ("TIGR00051", 3000), ("pfam00052", 7000), ("pfam00053", 11000), ("pfam00054", 90000)])
    c.append(case("redundant_tigrfam", {"G1": red, "G2": red, "G3": red}, redundant="pfam00050\tTIGR00050\npfam77777\tTIGR00051\n"))
    # an empty genome list with a cached table: every family becomes a marker, the reference prints its warning
    c.append(case("empty_genome_list", {"G1": red, "G2": red}, genomeIds=[], cache=True))
    # the caches of IMG are used whatever spacing they were made with
    c.append(case("precomputed_caches", {"G1": two(0), "G2": two(0)}, spacing=5000, precompute_spacing=0))
    # failures: a contig of the GFF that the FASTA file lacks
    broken = genome([("c1", 130, [("x1", 50, 120, ["pfam00010"], [])]), ("c2", 90, [("x2", 100, 160, ["pfam00011"], [])])])
    broken[".fna"] = broken[".fna"].replace(">c1 ", ">other ")
    c.append(case("contig_without_sequence", {"G1": broken}, ubiquity=1.0, single=1.0))
    return c


def write_tree(d, c):
    for rel, text in all_files(c).items():
        p = os.path.join(d, *rel.split("/"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    open(os.path.join(d, "tigrfam2pfam.tsv"), "w").write(c["redundant"])
    return d


def plain_dist(table):
    return {g: {f: sorted(list(p) for p in copies) for f, copies in fams.items()} for g, fams in table.items()}


def run_case(Builder, IMG, c):
    d = write_tree(tempfile.mkdtemp(prefix="ckm_mset_golden_"), c)
    IMG.genomeDir = d + os.sep
    img = IMG(os.path.join(d, "img_metadata.tsv"), os.path.join(d, "tigrfam2pfam.tsv"))
    b = object.__new__(Builder)                     # the reference's __init__ reads files of its authors' machine
    b.img, b.cachedGeneCountTable = img, None
    ids, out, printed = c["genomeIds"], {}, io.StringIO()
    allIds = sorted(set(rel.split("/")[0] for rel in all_files(c)))
    try:
        with contextlib.redirect_stdout(printed):
            table = img.geneCountTable(allIds if c["cache"] else ids)
            out["count_table"] = table
            if c["cache"]:
                b.cachedGeneCountTable = table
            if "precompute_spacing" in c:
                img.precomputeGenomeSeqLens(ids)
                img.precomputeGenomeFamilyPositions(ids, c["precompute_spacing"])
                out["seq_lens"] = img.cachedGenomeSeqLens
            raw = b.markerGenes(ids, table, c["ubiquity"] * len(ids), c["single"] * len(ids))
            out["markers_raw"] = sorted(raw)
            out["tigr_removed"] = sorted(img.identifyRedundantTIGRFAMs(raw))
            out["pfam_redundant"] = sorted(img.identifyRedundantPFAMs(raw))
            markers = b.buildMarkerGenes(ids, c["ubiquity"], c["single"])
            out["markers"] = sorted(markers)
            dist = img.geneDistTable(ids, markers, c["spacing"])
            out["gene_dist_table"] = plain_dist(dist)
            pairs = b.colocatedGenes(dist, c["dist_threshold"], c["genome_threshold"])
            out["pairs"] = sorted(pairs)
            sets = b.colocatedSets(pairs, markers)
            out["sets"] = sorted(sorted(s) for s in sets)
            out["genome_check"] = {}
            for g in allIds:
                comp, cont, missing, dup = b.genomeCheck(sets, g, table)
                out["genome_check"][g] = [comp.hex(), cont.hex(), sorted(missing), sorted(dup)]
            b.cachedGeneCountTable = table
            out["missing"] = sorted(b.missingGenes(ids, markers, c["missing_threshold"]))
            out["duplicate"] = sorted(b.duplicateGenes(ids, markers, c["missing_threshold"]))
            if not c["cache"]:
                b.cachedGeneCountTable = None
            ms = b.buildMarkerSet(ids, c["ubiquity"], c["single"], c["spacing"])
            out["marker_set"] = dict(UID=ms.UID, lineageStr=ms.lineageStr, numGenomes=ms.numGenomes, sets=sorted(sorted(s) for s in ms.markerSet))
        error = None
    except (Exception, SystemExit) as e:
        error = dict(type=type(e).__name__, args=[repr(a) for a in e.args])
    return dict(c, out=out, printed=printed.getvalue(), error=error)


def main():
    source = os.environ.get("CHECKM_SOURCE", "")
    os.environ["CHECKM_DATA_PATH"] = tempfile.mkdtemp(prefix="ckm_mset_data_")      # the reference's import otherwise creates ~/.checkm
    sys.path.insert(0, source)
    from checkm.util.img import IMG
    Builder = load_builder(source)
    if "--time" in sys.argv:
        return time_reference(Builder)
    out = dict(generator="tools/gen_markerset_golden.py: checkm.util.img.IMG and the class of scripts/genometreeworkflow/markerSetBuilder.py of the reference, "
                         "the script loaded in memory after the four substitutions the tool lists",
               substitutions=[s[0] for s in SUBSTITUTIONS], cases=[run_case(Builder, IMG, c) for c in cases()])
    path = os.path.join(ROOT, "tests", "golden", "markerset_cases.json")
    head = json.dumps(dict(generator=out["generator"], substitutions=out["substitutions"]), sort_keys=True)
    lines = ",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in out["cases"])          # a case per line
    open(path, "w").write(head[:-1] + ', "cases": [\n' + lines + "\n]}\n")
    for c in out["cases"]:
        print(c["name"], c["error"], len(c["out"].get("markers", [])), c["out"].get("pairs"), repr(c["printed"]))
    print(os.path.getsize(path), "bytes")


def time_reference(Builder):
    from tools.markerset_bench import synth_dist_table
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    genomes, markers = arg("--genomes", 60), arg("--markers", 120)
    dist = synth_dist_table(genomes, markers, seed=17)
    b = object.__new__(Builder)
    t0 = time.perf_counter()
    pairs = b.colocatedGenes(dist)
    wall = time.perf_counter() - t0
    tests = genomes * (markers * (markers - 1) // 2)
    out = dict(what="reference colocatedGenes (translated in memory), one core, the synthetic geneDistTable of tools/markerset_bench.py", genomes=genomes, markers=markers,
               pair_tests=tests, reported=len(pairs), seconds=wall, pair_tests_per_second=tests / wall)
    open(os.path.join(ROOT, "profiles", "r17_markerset_reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
