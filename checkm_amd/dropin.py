"""Rebinds CheckM's stage classes to the MI355X implementations (option A)."""


def install():
    import checkm.hmmerModelParser
    import checkm.markerGeneFinder
    import checkm.markerSets
    import checkm.resultsParser
    from checkm_amd import hmmerModelParser as p
    from checkm_amd import markerGeneFinder as g
    from checkm_amd import markerSets as m
    from checkm_amd import resultsParser as r
    checkm.markerGeneFinder.MarkerGeneFinder = g.MarkerGeneFinder
    checkm.resultsParser.ResultsParser = r.ResultsParser
    checkm.resultsParser.ResultsManager = r.ResultsManager
    checkm.markerSets.MarkerSet = m.MarkerSet
    checkm.markerSets.BinMarkerSets = m.BinMarkerSets
    checkm.markerSets.MarkerSetParser = m.MarkerSetParser
    p.HmmModel.__module__ = 'checkm.hmmerModelParser'
    checkm.hmmerModelParser.HmmModel = p.HmmModel
    # every hmmalign call of CheckM (qa --aai_strain, qa -o 9, tree): the masked alignments come from ckm_align
    import checkm.aminoAcidIdentity
    import checkm.hmmerAligner
    from checkm_amd import aminoAcidIdentity as a
    from checkm_amd import hmmerAligner as h
    checkm.hmmerAligner.HmmerAligner = h.HmmerAligner
    checkm.aminoAcidIdentity.AminoAcidIdentity = a.AminoAcidIdentity
    # gene calling in front of the scan: the two translation tables of a bin side by side (same files, same table choice)
    import checkm.prodigal
    from checkm_amd import prodigal as pr
    checkm.prodigal.ProdigalRunner = pr.ProdigalRunner
    checkm.prodigal.ProdigalGeneFeatureParser = pr.ProdigalGeneFeatureParser
    # bin statistics (tree and analyze step: storage/bin_stats.*.tsv) and `checkm tetra`: the nucleotide pass on the device.  Guarded: a
    # CheckM package without these modules keeps what it has.
    try:
        import checkm.binStatistics
    except ImportError:
        pass
    else:
        from checkm_amd import binStatistics as bs
        checkm.binStatistics.BinStatistics = bs.BinStatistics
    try:
        import checkm.genomicSignatures
    except ImportError:
        pass
    else:
        from checkm_amd import genomicSignatures as gs
        checkm.genomicSignatures.GenomicSignatures = gs.GenomicSignatures
    # `checkm outliers`, `modify`, `unique`: per-sequence GC, coding density and tetranucleotide distance on the device
    try:
        import checkm.binTools
    except ImportError:
        pass
    else:
        from checkm_amd import binTools as bt
        checkm.binTools.BinTools = bt.BinTools
    # `checkm merge`: the all-pairs comparison of marker genes on the device
    try:
        import checkm.merger
    except ImportError:
        pass
    else:
        from checkm_amd import merger as mg
        checkm.merger.Merger = mg.Merger
    # `checkm coverage`, `checkm profile` and `qa --coverage_file`: BAM files read by the library (no pysam), the records on the device
    try:
        import checkm.coverage
        import checkm.profile
    except ImportError:
        pass
    else:
        from checkm_amd import coverage as cv
        from checkm_amd import profile as pf
        checkm.coverage.Coverage = cv.Coverage
        checkm.coverage.CoverageStruct = cv.CoverageStruct
        checkm.profile.Profile = pf.Profile
    # `checkm gc_bias_plot`: the per-window coverage of a BAM file on the device (the plot class stays the reference's)
    try:
        import checkm.coverageWindows
    except ImportError:
        pass
    else:
        from checkm_amd import coverageWindows as cw
        checkm.coverageWindows.CoverageWindows = cw.CoverageWindows
        checkm.coverageWindows.CoverageStruct = cw.CoverageStruct
    # `checkm gc_plot`, `coding_plot`, `tetra_plot`, `dist_plot` and the FASTA half of `gc_bias_plot`: the plot classes stay the reference's
    # and compute inline, so the names their modules imported are bound to the library's answers (checkm_amd/plotHooks.py)
    try:
        import checkm.plot.codingDensityPlots
        import checkm.plot.gcBiasPlots
        import checkm.plot.gcPlots
        import checkm.plot.tetraDistPlots
    except ImportError:
        pass
    else:
        from checkm_amd import plotHooks as ph
        for mod in (checkm.plot.gcPlots, checkm.plot.gcBiasPlots, checkm.plot.codingDensityPlots):
            mod.readFasta = ph.readFasta
            mod.baseCount = ph.baseCount
        checkm.plot.codingDensityPlots.ProdigalGeneFeatureParser = ph.ProdigalGeneFeatureParser
        checkm.plot.tetraDistPlots.readFasta = ph.readFasta
        checkm.plot.tetraDistPlots.GenomicSignatures = ph.GenomicSignatures
    # `checkm unbinned`: ids of the bins on the host, base counts of the kept contigs on the device, both files written by the library
    try:
        import checkm.unbinned
    except ImportError:
        pass
    else:
        from checkm_amd import unbinned as ub
        checkm.unbinned.Unbinned = ub.Unbinned
    # `checkm ssu_finder`: the three nucleotide models scanned on the device instead of three nhmmer runs
    try:
        import checkm.ssuFinder
    except ImportError:
        pass
    else:
        from checkm_amd import ssuFinder as sf
        checkm.ssuFinder.SSU_Finder = sf.SSU_Finder
