"""BinTools without a device: modify / removeOutliers / unique and the numpy helpers against the reference's own output
(tests/golden/outliers_cases.json, tools/gen_outliers_golden.py), the two host readers of the outlier pass (ckm_seq_genes_read,
ckm_tetra_profile_read), the arithmetic of the kernels run by the host executor (tests/emu/outliers_emu.cpp) bit for bit against numpy,
and identifyOutliers() end to end with the two device passes replaced by their host executors."""
import hashlib
import json
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import binTools as bt
from checkm_amd import common
from checkm_amd import genomicSignatures as gs
from checkm_amd.defaultValues import DefaultValues
from checkm_amd.prodigal import ProdigalGeneFeatureParser
from tests.emu import nucstats as emu_ns
from tests.emu import outliers as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "outliers_cases.json")))
CASES = {c["name"]: c for c in GOLD["cases"]}
HEADER = "Sequence Id\t" + "\t".join(gs.GenomicSignatures(4, 1).canonicalKmerOrder()) + "\n"


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """== on the bit patterns, nan wherever the other is nan."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


@pytest.fixture
def data_root(tmp_path):
    """A data root holding the fixture's fabricated distributions; the previous one comes back afterwards."""
    before = DefaultValues.CHECKM_DATA_DIR
    root = tmp_path / "data"
    (root / "distributions").mkdir(parents=True)
    for name, text in GOLD["distributions"].items():
        (root / "distributions" / (name + ".txt")).write_text(text)
    DefaultValues.set_data_root(str(root))
    yield str(root)
    DefaultValues.set_data_root(before)


def read_fasta_text(text):
    """[(id, sequence)] of a fixture FASTA (plain: one header word, wrapped lines)."""
    recs = []
    for block in text.split(">")[1:]:
        lines = block.split("\n")
        recs.append((lines[0].split()[0], "".join(lines[1:])))
    return recs


def profile_text(case, tetra_of):
    """The tetranucleotide profile of a case as the generator built it: the writer's rows for profile_fasta, then the repeated ids.
    tetra_of(list of byte strings) -> [n, 136] counts."""
    recs = read_fasta_text(case["profile_fasta"])
    rows = gs.format_rows([i for i, _s in recs], tetra_of([s.encode() for _i, s in recs])).splitlines(True)
    by_id = dict((ln.split("\t", 1)[0], ln.split("\t", 1)[1]) for ln in rows)
    text = HEADER + "".join(rows) + "".join(seqId + "\t" + by_id[src] for seqId, src in case["repeat"])
    assert hashlib.sha256(text.encode()).hexdigest() == case["profile_sha256"], case["name"]
    return text


def emu_tetra(seqs):
    return emu_ns.nucstats(seqs, 4096)["tetra"]


def write_case(tmp, case, tetra_of=emu_tetra):
    """The case's bin files, bins/<name>/genes.gff and the profile under tmp; returns (bin paths, out dir, profile path)."""
    out = tmp / "out"
    paths = []
    for b in case["bins"]:
        p = tmp / (b["name"] + ".fna")
        p.write_text(b["fasta"])
        paths.append(str(p))
        if b["gff"] is not None:
            d = out / "bins" / b["name"]
            d.mkdir(parents=True, exist_ok=True)
            (d / "genes.gff").write_text(b["gff"])
    prof = tmp / "tetra.tsv"
    prof.write_text(profile_text(case, tetra_of))
    return paths, str(out), str(prof)


def restated_outliers(outDir, binFiles, tetraProfileFile, distribution, reportType, dists):
    """The file identifyOutliers writes, from BinTools' numpy helpers and plain Python: the statement the device path is held to."""
    gcB, cdB, tdB = dists
    tools = bt.BinTools()
    g = gs.GenomicSignatures(4, 1)
    sigs = g.read(tetraProfileFile)
    near = common.findNearest
    out = ['Bin Id\tSequence Id\tSequence length\tOutlying distributions',
           '\tSequence GC\tMean bin GC\tLower GC bound (%s%%)\tUpper GC bound (%s%%)' % (distribution, distribution),
           '\tSequence CD\tMean bin CD\tLower CD bound (%s%%)' % distribution, '\tSequence TD\tMean bin TD\tUpper TD bound (%s%%)\n' % distribution]
    for f in binFiles:
        binId = common.binIdFromFilename(f)
        seqs = bt._read_fasta(f)
        meanGC, dGC, GCs = tools.gcDist(seqs)
        binSig = tools.binTetraSig(seqs, sigs)
        meanTD, TDs = tools.tetraDiffDist(seqs, g, sigs, binSig)
        meanCD, dCD, CDs = tools.codingDensityDist(seqs, ProdigalGeneFeatureParser(os.path.join(outDir, 'bins', binId, 'genes.gff')))
        cg = near(np.array(list(gcB.keys())), meanGC)
        d = gcB[cg][list(gcB[cg].keys())[0]]
        kLo, kHi = near(list(d.keys()), (100 - distribution) / 2.0), near(list(d.keys()), (100 + distribution) / 2.0)
        cc = near(np.array(list(cdB.keys())), meanCD)
        d = cdB[cc][list(cdB[cc].keys())[0]]
        kCd = near(list(d.keys()), (100 - distribution) / 2.0)
        kTd = near(list(tdB[list(tdB.keys())[0]].keys()), distribution)
        for i, (seqId, seq) in enumerate(seqs.items()):
            n = len(seq)
            lo, hi = (gcB[cg][near(list(gcB[cg].keys()), n)][k] for k in (kLo, kHi))
            cdLo = cdB[cc][near(list(cdB[cc].keys()), n)][kCd]
            tdHi = tdB[near(list(tdB.keys()), n)][kTd]
            kinds = [name for name, isOut in (('GC', dGC[i] < lo or dGC[i] > hi), ('CD', dCD[i] < cdLo), ('TD', TDs[i] > tdHi)) if isOut]
            if (reportType == 'any' and kinds) or (reportType == 'all' and len(kinds) == 3):
                out.append('%s\t%s\t%d\t%s\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f\t%.1f\t%.3f\t%.3f\t%.3f\n' % (
                    binId, seqId, n, ','.join(kinds), GCs[i] * 100, meanGC * 100, (meanGC + lo) * 100, (meanGC + hi) * 100,
                    CDs[i] * 100, meanCD * 100, (meanCD + cdLo) * 100, TDs[i], meanTD, tdHi))
    return ''.join(out)


def fixture_dists():
    import ast
    return tuple(ast.literal_eval(GOLD["distributions"][k]) for k in ("gc_dist", "cd_dist", "td_dist"))


# ---- modify, removeOutliers, unique ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(GOLD["modify"])))
def test_modify_and_remove_outliers_write_the_reference_files(tmp_path, caplog, k):
    c = GOLD["modify"][k]
    (tmp_path / "binA.fna").write_text(c["bin"])
    out = str(tmp_path / "out.fna")
    tools = bt.BinTools()
    if c["kind"] == "removeOutliers":
        (tmp_path / "outliers.tsv").write_text(c["outliers"])
        tools.removeOutliers(str(tmp_path / "binA.fna"), str(tmp_path / "outliers.tsv"), out)
        assert open(out).read() == c["output"]
        return
    (tmp_path / "ref.fna").write_text(c["ref"])
    if c["error"] is None:
        tools.modify(str(tmp_path / "binA.fna"), str(tmp_path / "ref.fna"), c["add"], c["remove"], out)
        assert open(out).read() == c["output"]
    else:
        with caplog.at_level(logging.ERROR, logger="timestamp"), pytest.raises(SystemExit) as e:
            tools.modify(str(tmp_path / "binA.fna"), str(tmp_path / "ref.fna"), c["add"], c["remove"], out)
        assert e.value.code == c["error"]["code"]
        # the ids of the message are a set in the reference: same head, same ids
        want, got = c["error"]["log"][0], caplog.records[-1].getMessage()
        assert got.split(": ")[0] == want.split(": ")[0] and set(got.split(": ")[1].strip().split(", ")) == set(want.split(": ")[1].strip().split(", "))


def unique_blocks(text):
    """(warnings and other lines in order, {(pair line): set of ids})."""
    lines, pairs, cur = [], {}, None
    for ln in text.splitlines():
        if ln.startswith("  Sequences shared between"):
            cur = pairs.setdefault(ln, set())
            lines.append(ln)
        elif cur is not None and ln.startswith("    "):
            cur.add(ln)
        else:
            cur = None
            lines.append(ln)
    return lines, pairs


@pytest.mark.parametrize("k", range(len(GOLD["unique"])))
def test_unique_prints_what_the_reference_prints(tmp_path, capsys, k):
    c = GOLD["unique"][k]
    paths = []
    for name, text in c["files"]:
        (tmp_path / (name + ".fna")).write_text(text)
        paths.append(str(tmp_path / (name + ".fna")))
    bt.BinTools().unique(paths)
    got = capsys.readouterr().out
    assert unique_blocks(got) == unique_blocks(c["stdout"])
    assert got.count("\n") == c["stdout"].count("\n")


# ---- helpers -------------------------------------------------------------------------------------------------------------------------

def test_read_distribution_and_find_nearest(data_root):
    gcB = common.readDistribution("gc_dist")
    assert gcB == fixture_dists()[0] and list(gcB.keys())[0] == 0.5
    assert DefaultValues.DISTRIBUTION_DIR == os.path.join(data_root, "distributions")
    assert common.findNearest([200, 400, 700], 300) == 200 and common.findNearest([400, 200], 300) == 400      # the first of two equally near
    assert common.findNearest(np.array([0.5, 0.25, 0.75]), 0.375) == 0.5
    assert common.findNearest([0, 0.5, 2.5, 5, 50, 95, 97.5, 99.5, 100], (100 - 99) / 2.0) == 0.5


def test_read_distribution_without_the_file_exits(tmp_path):
    before = DefaultValues.CHECKM_DATA_DIR
    DefaultValues.set_data_root(str(tmp_path))
    try:
        with pytest.raises(SystemExit):
            common.readDistribution("gc_dist")
    finally:
        DefaultValues.set_data_root(before)


@pytest.mark.parametrize("run", range(len(CASES["three_bins"]["runs"])))
def test_numpy_helpers_restate_the_reference_file(tmp_path, run):
    case = CASES["three_bins"]
    paths, out, prof = write_case(tmp_path, case)
    r = case["runs"][run]
    with np.errstate(invalid="ignore"):
        assert restated_outliers(out, paths, prof, r["distribution"], r["reportType"], fixture_dists()) == r["output"]


# ---- the host readers --------------------------------------------------------------------------------------------------------------------

def test_seq_genes_is_coding_bases_per_sequence(tmp_path):
    case = CASES["three_bins"]
    paths, out, _ = write_case(tmp_path, case)
    gffs = [os.path.join(out, "bins", b["name"], "genes.gff") for b in case["bins"]]
    for g in gffs:
        open(os.path.join(os.path.dirname(g), "genes.faa"), "w").close()
    seqs = _lib.NucSeqs(paths)
    coding, missing = _lib.seq_genes(seqs, gffs)
    assert not missing.any()
    ids = seqs.ids()
    total = 0
    for f, g in enumerate(gffs):
        parser = ProdigalGeneFeatureParser(g)
        a, z = int(seqs.file_first[f]), int(seqs.file_first[f + 1])
        assert [int(x) for x in coding[a:z]] == [int(parser.codingBases(i)) for i in ids[a:z]]
        total += int(coding[a:z].sum())
    per_file = _lib.bin_genes(seqs, gffs, [os.path.join(os.path.dirname(g), "genes.faa") for g in gffs])
    assert [c for c, _t, _n in per_file] == [int(coding[int(seqs.file_first[f]):int(seqs.file_first[f + 1])].sum()) for f in range(len(gffs))]
    assert coding[ids.index("cd_only")] == 0 and total > 0
    # a missing file is reported per file, its sequences get -1
    coding, missing = _lib.seq_genes(seqs, [gffs[0], str(tmp_path / "nowhere.gff"), gffs[2]])
    a, z = int(seqs.file_first[1]), int(seqs.file_first[2])
    assert list(missing) == [False, True, False] and (coding[a:z] == -1).all() and (coding[:a] >= 0).all()
    seqs.close()


def test_profile_reader_is_genomic_signatures_read(tmp_path):
    case = CASES["three_bins"]
    _paths, _out, prof = write_case(tmp_path, case)
    want = gs.GenomicSignatures(4, 1).read(prof)
    p = _lib.TetraProfile(prof)
    ids, sig = p.ids(), p.sig()
    assert ids == list(want.keys()) and len(ids) == len(read_fasta_text(case["profile_fasta"]))          # repeated ids keep their place
    for i, k in enumerate(ids):
        assert same_bits(sig[i], want[k]), k
    assert np.isnan(sig[ids.index("nowin")]).all()
    rows = dict((ln.split("\t", 1)[0], ln) for ln in open(prof).read().splitlines()[1:])                # the later row of a repeated id won
    assert same_bits(sig[ids.index("m03")], [float(x) for x in rows["x_unbinned2"].split("\t")[1:]])
    # the gather by id
    paths, _, _ = write_case(tmp_path, case)
    seqs = _lib.NucSeqs(paths)
    got, missing = p.gather(seqs)
    assert missing == -1 and all(same_bits(got[s], want[i]) for s, i in enumerate(seqs.ids()))
    seqs.close()
    extra = tmp_path / "extra.fna"
    extra.write_text(">m00\nACGT\n>stranger\nACGT\n>stranger2\nAC\n")
    seqs = _lib.NucSeqs([str(extra)])
    assert p.gather(seqs)[1] == 1
    seqs.close()
    p.close()


def test_profile_reader_parses_every_float_as_python_does(tmp_path):
    rng = np.random.default_rng(99)
    vals = np.concatenate([rng.integers(0, 2 ** 63, size=6000, dtype=np.uint64).view(np.float64),            # every exponent, denormals, nan, inf
                           rng.integers(0, 2 ** 52, size=1500, dtype=np.uint64).view(np.float64),             # denormals
                           rng.random(2400) / 136, np.array([1e-300, 5e-324, 0.0, 1.7976931348623157e308])])
    vals = np.concatenate([vals, -vals[:100]])
    toks = [repr(float(v)) for v in vals] + ["nan", "1e-300", "0.007352941176470588", "2.2250738585072014e-308", "1E5", " 0.5 ", "inf", "-inf"]
    toks += toks[:(-len(toks)) % 136]
    assert len(toks) >= 10 ** 4 and len(toks) % 136 == 0
    nrows = len(toks) // 136
    with open(str(tmp_path / "p.tsv"), "w") as f:
        f.write(HEADER)
        for r in range(nrows):
            f.write("row%d\t" % r + "\t".join(toks[r * 136:(r + 1) * 136]) + ("\r\n" if r % 3 == 0 else "\n"))
    p = _lib.TetraProfile(str(tmp_path / "p.tsv"))
    sig = p.sig()
    want = np.array([float(t) for t in toks]).reshape(nrows, 136)
    assert p.n == nrows and same_bits(sig, want) and np.isnan(want).sum() >= 1 and (np.abs(want) < 2.3e-308).sum() > 1000
    p.close()
    with pytest.raises(_lib.CkmError) as e:
        _lib.TetraProfile(str(tmp_path / "missing.tsv"))
    assert e.value.code == -2


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("outliers_native") / "outliers_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "outliers_host_check.cpp"), os.path.join(CSRC, "outliers_host.cpp"), os.path.join(CSRC, "nucstats_host.cpp"), "-lz", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def run_checker(exe, *args):
    out = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    return out.stdout.splitlines()


def test_host_readers_under_sanitizers_take_malformed_files(checker, tmp_path):
    row = "\t".join(["0.25"] * 136)
    files = {
        "good": (HEADER + "a\t" + row + "\nb\t" + row + "\n", 0, 2),
        "no_trailing_newline": (HEADER + "a\t" + row + "\nb\t" + "\t".join(["nan"] * 136), 0, 2),
        "empty": ("", 0, 0),
        "header_only": (HEADER, 0, 0),
        "header_without_newline": (HEADER.rstrip("\n"), 0, 0),
        "short_row": (HEADER + "a\t" + row + "\nb\t0.5\t0.5\n", -3, 0),
        "id_only": (HEADER + "a\n", -3, 0),
        "cols_135": (HEADER + "a\t" + "\t".join(["0.25"] * 135) + "\n", -3, 0),
        "cols_137": (HEADER + "a\t" + "\t".join(["0.25"] * 137) + "\n", -3, 0),
        "not_a_float": (HEADER + "a\t" + "\t".join(["0.25"] * 135 + ["0x1p3"]) + "\n", -3, 0),
        "empty_field": (HEADER + "a\t" + "\t".join(["0.25"] * 135 + [""]) + "\n", -3, 0),
        "blank_line": (HEADER + "a\t" + row + "\n\nb\t" + row + "\n", -3, 0),
        "long_token": (HEADER + "a\t" + "\t".join(["0.25"] * 135 + ["1" * 5000]) + "\n", -3, 0),
        "repeated_id": (HEADER + "a\t" + row + "\nb\t" + row + "\na\t" + "\t".join(["0.5"] * 136) + "\n", 0, 2),
    }
    for name, (text, rc, n) in sorted(files.items()):
        p = tmp_path / (name + ".tsv")
        p.write_text(text)
        lines = run_checker(checker, "profile", str(p))
        assert lines[0] == "rc=%d n=%d" % (rc, n), (name, lines[:3])
    lines = run_checker(checker, "profile", str(tmp_path / "repeated_id.tsv"))
    assert lines[1].split() == ["a", "%016x" % int(bits(0.5)[0]), "%016x" % int(bits(0.5)[0])]
    # the genes of a sequence: the golden bin, a file with short rows, an empty file, no file
    b = CASES["three_bins"]["bins"][0]
    (tmp_path / "main.fna").write_text(b["fasta"])
    (tmp_path / "genes.gff").write_text(b["gff"])
    lines = run_checker(checker, "genes", str(tmp_path / "main.fna"), str(tmp_path / "genes.gff"))
    parser = ProdigalGeneFeatureParser(str(tmp_path / "genes.gff"))
    assert lines[0] == "rc=0 missing=0" and [ln.split() for ln in lines[1:]] == [[i, str(int(parser.codingBases(i)))] for i, _s in read_fasta_text(b["fasta"])]
    (tmp_path / "short.gff").write_text(b["gff"] + "m00\tx\tCDS\t5\n")
    assert run_checker(checker, "genes", str(tmp_path / "main.fna"), str(tmp_path / "short.gff"))[0].startswith("rc=-3")
    (tmp_path / "empty.gff").write_text("")
    lines = run_checker(checker, "genes", str(tmp_path / "main.fna"), str(tmp_path / "empty.gff"))
    assert lines[0] == "rc=0 missing=0" and all(ln.split()[1] == "0" for ln in lines[1:])
    assert run_checker(checker, "genes", str(tmp_path / "main.fna"), str(tmp_path / "none.gff"))[0] == "rc=0 missing=1"


# ---- the arithmetic of the kernels, host executor against numpy ---------------------------------------------------------------------------

def test_td_order_is_numpys_pairwise_sum():
    rng = np.random.default_rng(3)
    g = gs.GenomicSignatures(4, 1)
    for k in range(20000):
        a, b = rng.random(136) * 10.0 ** rng.integers(-6, 3), rng.random(136)
        if k % 1000 == 0:
            a[int(rng.integers(0, 136))] = np.nan
        want = g.distance(a, b)
        got = emu.td(a, b)
        assert (np.isnan(want) and np.isnan(got)) or bits(want)[0] == bits(got)[0], k
    A, B = rng.random((300, 136)), rng.random(136)
    assert np.array_equal(bits(np.abs(A - B).sum(axis=1)), bits([emu.td(A[i], B) for i in range(300)]))


def test_nearest_key_is_the_first_minimum():
    rng = np.random.default_rng(4)
    for _ in range(2000):
        keys = [int(x) for x in rng.integers(1, 6000, size=int(rng.integers(1, 12)))]
        n = int(rng.integers(1, 7000)) if rng.random() < .5 else (keys[0] + keys[-1]) // 2
        assert keys[emu.nearest_key(keys, n)] == common.findNearest(keys, n) and emu.nearest_key(keys, n) == int(np.abs(np.array(keys) - n).argmin())
    assert emu.nearest_key([400, 200], 300) == 0 and emu.nearest_key([200, 400], 300) == 0 and emu.nearest_key([0.5, 0.25], 0.375) == 0


class _Genes(object):
    def __init__(self, coding):
        self.coding = coding

    def codingBases(self, seqId):
        return self.coding[seqId]


def random_bins(rng, sizes):
    """Per bin a dict of sequences (lengths 4 .. 3000, a few without a 4-mer window when asked), coding bases, signature rows."""
    bins = []
    for b, n in enumerate(sizes):
        lens = rng.integers(4, 3000, size=n)
        seqs = {}
        for k, m in enumerate(lens):
            seqs["b%d_s%d" % (b, k)] = rng.choice(np.frombuffer(b"ACGTacgtNRu", dtype=np.uint8), size=int(m), p=[.22, .22, .22, .22, .02, .02, .02, .02, .02, .01, .01]).tobytes().decode()
        bins.append(seqs)
    return bins


def helper_columns(bins, tables, gcTab, cdTab, tdTab):
    """What the device pass returns, by BinTools' numpy helpers and numpy comparisons."""
    tools, g = bt.BinTools(), gs.GenomicSignatures(4, 1)
    out = {k: [] for k in ("gc", "delta_gc", "cd", "delta_cd", "td", "flags", "mean_gc", "mean_cd", "bin_sig")}
    for f, (seqs, coding, sigs) in enumerate(bins):
        mgc, dgc, gcs = tools.gcDist(seqs)
        mcd, dcd, cds = tools.codingDensityDist(seqs, _Genes(coding))
        with np.errstate(invalid="ignore"):
            binSig = tools.binTetraSig(seqs, {k: v.copy() for k, v in sigs.items()})
            _m, tds = tools.tetraDiffDist(seqs, g, sigs, binSig)
        off, key, lo, hi = tables
        for i, seq in enumerate(seqs.values()):
            kg, kc, kt = (off[t] + int(np.abs(np.array(key[off[t]:off[t + 1]]) - len(seq)).argmin()) for t in (gcTab[f], cdTab[f], tdTab))
            out["flags"].append((1 if dgc[i] < lo[kg] or dgc[i] > hi[kg] else 0) | (2 if dcd[i] < lo[kc] else 0) | (4 if tds[i] > hi[kt] else 0))
        for k, v in (("gc", gcs), ("delta_gc", dgc), ("cd", cds), ("delta_cd", dcd), ("td", tds)):
            out[k] += list(v)
        out["mean_gc"].append(mgc); out["mean_cd"].append(mcd); out["bin_sig"].append(binSig)
    return {k: np.array(v) for k, v in out.items()}


def counts_of(seqs):
    c = np.zeros((len(seqs), 8), dtype=np.uint64)
    for i, s in enumerate(seqs):
        u = s.upper()
        c[i] = [u.count("A"), u.count("C"), u.count("G"), u.count("T") + u.count("U"), s.count("N"), s.count("n"), len(s), len(s) - s.count("N")]
    return c


def random_tables(rng, ntab=5):
    off, key, lo, hi = [0], [], [], []
    for _ in range(ntab):
        n = int(rng.integers(1, 11))
        key += [float(x) for x in rng.integers(50, 4000, size=n)]
        lo += list(-rng.random(n) * 0.5)
        hi += list(rng.random(n) * 0.4 + 0.2)
        off.append(len(key))
    return off, key, lo, hi


def test_host_executor_matches_the_numpy_helpers_on_random_bins():
    rng = np.random.default_rng(8)
    g = gs.GenomicSignatures(4, 1)
    sizes = [1, 2, 7, 64, 65, 300, 5000, 1, 1023]
    raw = random_bins(rng, sizes)
    bins = []
    for seqs in raw:
        coding = {k: int(rng.integers(0, len(s) + 1)) for k, s in seqs.items()}
        # signatures as a profile holds them: counts over a total, with a nan row now and then in the small bins
        cnt = rng.integers(0, 40, size=(len(seqs), 136)).astype(np.float64)
        sig = cnt / cnt.sum(axis=1)[:, None]
        if len(seqs) in (7, 65):
            sig[len(seqs) // 2] = np.nan
        bins.append((seqs, coding, dict(zip(seqs.keys(), sig))))
    tables = random_tables(rng)
    gcTab, cdTab, tdTab = [int(x) for x in rng.integers(0, 5, size=len(bins))], [int(x) for x in rng.integers(0, 5, size=len(bins))], 2
    want = helper_columns(bins, tables, gcTab, cdTab, tdTab)
    flat = [s for seqs, _c, _s in bins for s in seqs.values()]
    first = np.cumsum([0] + sizes)
    got = emu.outliers(first, counts_of(flat), np.array([v for _s, _c, sg in bins for v in sg.values()]),
                       [c for _s, cd, _g in bins for c in cd.values()], tables[0], tables[1], tables[2], tables[3], gcTab, cdTab, tdTab)
    for k in ("gc", "delta_gc", "cd", "delta_cd", "td", "mean_gc", "mean_cd", "bin_sig"):
        assert same_bits(got[k], want[k]), k
    assert np.array_equal(got["flags"], want["flags"])
    assert np.isnan(got["td"]).sum() == 7 + 65
    for bit in (1, 2, 4):                                      # both outcomes of every comparison occur
        assert 0 < int((got["flags"] & bit != 0).sum()) < len(flat), bit
    assert g.distance(np.zeros(136), np.zeros(136)) == 0.0


# ---- identifyOutliers end to end, the device passes replaced by their host executors --------------------------------------------------------

@pytest.fixture
def host_executors(monkeypatch):
    from checkm_amd import runtime

    def nucstats(ctx, seqs, tetra=False, tile_bytes=0):
        r = emu_ns.nucstats([seqs.seq(i) for i in range(seqs.nseq)], 4096)
        r.update(ms_upload=0.0, ms_count=0.0, ms_fill=0.0, ms_total=0.0, bytes=0)
        return r

    def outliers(ctx, seqs, count, sig, coding, tab_off, key, lo, hi, gct, cdt, td_tab):
        o = emu.outliers(seqs.file_first, count, sig, coding, tab_off, key, lo, hi, gct, cdt, td_tab)
        o.update(ms_upload=0.0, ms_seq=0.0, ms_binsig=0.0, ms_td=0.0, ms_flags=0.0, ms_total=0.0)
        return o
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)
    monkeypatch.setattr(_lib, "nucstats", nucstats)
    monkeypatch.setattr(_lib, "outliers", outliers)


@pytest.mark.parametrize("run", range(len(CASES["three_bins"]["runs"])))
def test_identify_outliers_writes_the_reference_file(tmp_path, data_root, host_executors, run):
    case = CASES["three_bins"]
    paths, out, prof = write_case(tmp_path, case)
    r = case["runs"][run]
    tools = bt.BinTools()
    tools.identifyOutliers(out, paths, prof, r["distribution"], r["reportType"], str(tmp_path / "o.tsv"))
    assert open(str(tmp_path / "o.tsv")).read() == r["output"]
    assert tools.last_timing["sequences"] == 25 and tools.last_timing["flagged"] == r["output"].count("\n") - 1


def test_identify_outliers_fails_where_the_reference_fails(tmp_path, data_root, host_executors, caplog):
    for name, exc in (("missing_gff", SystemExit), ("missing_id", KeyError), ("zero_division", ZeroDivisionError)):
        case = CASES[name]
        d = tmp_path / name
        d.mkdir()
        paths, out, prof = write_case(d, case)
        want = case["runs"][0]["error"]
        assert want["type"] == exc.__name__
        with caplog.at_level(logging.ERROR, logger="timestamp"), pytest.raises(exc) as e:
            bt.BinTools().identifyOutliers(out, paths, prof, 95, "any", str(d / "o.tsv"))
        if exc is SystemExit:
            assert e.value.code == want["code"] and caplog.records[-1].getMessage() == want["log"][0]
        else:
            assert [str(a) for a in e.value.args] == want["args"]


def test_dropin_rebinds_bin_tools_when_present(tmp_path):
    import sys
    pkg = tmp_path / "stand_in" / "checkm"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_module_classes.json")))["classes"]
    for mod, classes in gold.items():
        (pkg / (mod.split(".")[1] + ".py")).write_text("".join("class %s(object):\n    pass\n\n\n" % c for c in classes))
    (pkg / "binTools.py").write_text("class BinTools(object):\n    pass\n")
    code = ("import checkm.binTools as b\nimport checkm_amd.dropin as d; d.install()\n"
            "assert b.BinTools.__module__ == 'checkm_amd.binTools', b.BinTools.__module__\nprint('ok')\n")
    env = dict(os.environ, PYTHONPATH=str(tmp_path / "stand_in") + os.pathsep + ROOT, CHECKM_DATA_PATH=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-1500:]
