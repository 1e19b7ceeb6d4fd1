"""TEST INFRASTRUCTURE shared by the `checkm merge` tests and tools/gen_merger_golden.py: the worlds of tests/golden/merger_cases.json laid
out on disk for a set of CheckM classes (the reference's or this package's), a numpy restatement of the reference's pair loop
(checkm/merger.py:64-106) and a plain-Python writer of merger.tsv.  Never imported by checkm_amd."""
import os

import numpy as np

TABLE = "hmmer.analyze.txt"
HEADER = ('Bin Id 1\tBin Id 2\tBin 1 completeness\tBin 1 contamination\tBin 2 completeness\tBin 2 contamination'
          '\tDelta completeness\tDelta contamination\tMerger delta\tMerged completeness\tMerged contamination\n')
COLUMNS = ("comp_i", "cont_i", "comp_j", "cont_j", "delta_comp", "delta_cont", "delta", "comp_merged", "cont_merged")


def reference_classes():
    from checkm.defaultValues import DefaultValues
    from checkm.hmmerModelParser import HmmModel
    from checkm.markerSets import BinMarkerSets, MarkerSet
    return dict(HmmModel=HmmModel, MarkerSet=MarkerSet, BinMarkerSets=BinMarkerSets, pfam=lambda d: DefaultValues.PFAM_CLAN_FILE)


def package_classes():
    from checkm_amd.defaultValues import DefaultValues
    from checkm_amd.hmmerModelParser import HmmModel
    from checkm_amd.markerSets import BinMarkerSets, MarkerSet

    def pfam(d):
        root = os.path.join(d, "data")
        os.makedirs(os.path.join(root, "pfam"), exist_ok=True)
        DefaultValues.set_data_root(root)
        return os.path.join(root, "pfam", "Pfam-A.hmm.dat")
    return dict(HmmModel=HmmModel, MarkerSet=MarkerSet, BinMarkerSets=BinMarkerSets, pfam=pfam)


def bin_table(world, case, b):
    """The domtblout text of bin b of a world: the kept rows of the case's table plus the bin's extra rows; None: no file."""
    if b["rows"] is None:
        return None
    lines = case["domtblout"].splitlines(True)
    keep = set(b["rows"])
    return "".join(ln for k, ln in enumerate(lines) if ln.startswith("#") or k in keep) + b["extra"]


def world_marker_sets(world, override=None):
    """{binId: [set structure, ...]}: the world's own assignment, or a failure case's."""
    if override is not None:
        return override
    return {b["id"]: [world["structures"][world["assign"][b["id"]]]] for b in world["bins"]}


def materialise(world, cases, d, classes, marker_sets=None, models_for=None):
    """Writes <d>/bins/<binId>/<TABLE> and the Pfam clan file; returns (binIdToModels, binIdToBinMarkerSets) of the given classes."""
    case = cases[world["reduce_case"]]
    with open(classes["pfam"](d), "w") as f:
        f.write(case["pfam_dat"])
    models = {}
    for m in case["models"]:
        hm = classes["HmmModel"]({"name": m["name"], "acc": m["acc"], "leng": m["leng"]})
        hm.ga = tuple(m["ga"]) if m["ga"] else None
        hm.tc = tuple(m["tc"]) if m["tc"] else None
        hm.nc = tuple(m["nc"]) if m["nc"] else None
        models[m["acc"]] = hm
    for b in world["bins"]:
        text = bin_table(world, case, b)
        os.makedirs(os.path.join(d, "bins", b["id"]), exist_ok=True)
        if text is not None:
            with open(os.path.join(d, "bins", b["id"], TABLE), "w") as f:
                f.write(text)
    bms = {}
    for binId, structures in world_marker_sets(world, marker_sets).items():
        s = classes["BinMarkerSets"](binId, classes["BinMarkerSets"].TAXONOMIC_MARKER_SET)
        for k, st in enumerate(structures):
            s.addMarkerSet(classes["MarkerSet"](k, "k__Bacteria", 100, [set(x) for x in st]))
        bms[binId] = s
    return {b["id"]: models for b in world["bins"]}, bms


def rows_from_hits(hits_by_bin, marker_sets_by_bin, genes):
    """(member [nbins, ngenes] bool, hit_sum, n_markers) over sorted bin ids from plain {binId: {marker: [hits]}} dicts."""
    ids = sorted(hits_by_bin)
    index = {g: k for k, g in enumerate(genes)}
    member = np.zeros((len(ids), len(genes)), dtype=bool)
    hit_sum = np.zeros(len(ids), dtype=np.int64)
    n_markers = np.zeros(len(ids), dtype=np.int32)
    for b, binId in enumerate(ids):
        for m, hits in hits_by_bin[binId].items():
            if m in index:
                member[b, index[m]] = True
                hit_sum[b] += len(hits)
        n_markers[b] = sum(len(s) for s in marker_sets_by_bin[binId][0])
    return ids, member, hit_sum, n_markers


def restate(member, hit_sum, n_markers, thr):
    """The reference's loop over all pairs i < j in numpy float64: 100*float(x) first, the division second.  Returns (i, j, {column: values})
    of the pairs it writes, in (i, j) order."""
    member = np.asarray(member, dtype=bool)
    nb = member.shape[0]
    c = member.sum(axis=1).astype(np.int64)
    s = np.asarray(hit_sum, dtype=np.int64)
    n = np.asarray(n_markers, dtype=np.int64).astype(np.float64)
    comp = 100 * c.astype(np.float64) / n
    cont = 100 * (s - c).astype(np.float64) / n
    m32 = member.astype(np.float32)
    inter = np.rint(m32 @ m32.T).astype(np.int64)                   # exact: counts far below 2^24
    i, j = np.triu_indices(nb, k=1)                                 # row-major: i ascending, then j ascending
    u = c[i] + c[j] - inter[i, j]
    comp_m = 100 * u.astype(np.float64) / n[j]
    cont_m = 100 * (s[i] + s[j] - u).astype(np.float64) / n[j]
    d_comp = comp_m - np.maximum(comp[i], comp[j])
    d_cont = cont_m - np.maximum(cont[i], cont[j])
    delta = d_comp - d_cont
    keep = (comp_m >= thr[2]) & (cont_m < thr[3]) & (d_comp >= thr[0]) & (d_cont < thr[1])
    cols = dict(comp_i=comp[i], cont_i=cont[i], comp_j=comp[j], cont_j=cont[j], delta_comp=d_comp, delta_cont=d_cont, delta=delta,
                comp_merged=comp_m, cont_merged=cont_m)
    return i[keep].astype(np.uint32), j[keep].astype(np.uint32), {f: v[keep] for f, v in cols.items()}


def write_lines(ids, i, j, cols):
    """The text after the header, as checkm/merger.py:101-106 formats it."""
    out = []
    fmt = '%s\t%s' + '\t%.2f' * 9 + '\n'
    vals = [cols[f].tolist() for f in COLUMNS]
    for k, (a, b) in enumerate(zip(i.tolist(), j.tolist())):
        out.append(fmt % ((ids[a], ids[b]) + tuple(v[k] for v in vals)))
    return "".join(out)


def pack(member):
    from checkm_amd.merger import pack_rows
    return pack_rows(np.asarray(member, dtype=bool))


def synthetic(nbins, ngenes, seed, lo=0.2, hi=0.98, dup=0.04):
    """A world of random bins: completeness spread between lo and hi, a few multi-copy genes, two values of n_markers."""
    r = np.random.RandomState(seed)
    frac = r.uniform(lo, hi, size=nbins)
    member = r.random_sample((nbins, ngenes)) < frac[:, None]
    copies = np.where(r.random_sample((nbins, ngenes)) < dup, r.randint(2, 8, size=(nbins, ngenes)), 1)
    hit_sum = (member * copies).sum(axis=1).astype(np.int64)
    n_markers = np.where(np.arange(nbins) % 5 == 0, ngenes + 7, ngenes).astype(np.int32)
    return member, hit_sum, n_markers
