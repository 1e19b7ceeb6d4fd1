/* checkm_hip.h -- C ABI of libcheckm_hip.so, the MI355X (gfx950) marker-gene hot path of CheckM.
 *
 * The reference has no FFI: its seam is a shell command plus a text file.  Each entry point below
 * names the reference interface it replaces (paths relative to the CheckM source tree).
 *
 * Conventions
 *   - every function returns 0 on success or a negative CKM_E* code; ckm_last_error() returns a
 *     thread-local message for the last failure.  No C++ exception crosses this boundary.
 *   - the caller owns every input buffer; the library owns every output object and frees it in
 *     the matching *_free().  Column pointers returned by ckm_hits_columns()/ckm_qa_columns() stay
 *     valid until that object is freed.
 *   - a ckm_ctx runs ONE ckm_search / ckm_reduce / ckm_align at a time (not re-entrant); different ctxs are independent, also on
 *     one device: MarkerGeneFinder.find keeps up to three on a device, one batch of bins in flight on each.  A ctx owns its streams,
 *     tables and float workspace (budget: a quarter of the device memory free at creation, at most 96 GB); ckm_profiles, ckm_seqs
 *     and ckm_hits are plain device / host memory and may be used with ANY ctx of the device they were created on (the contexts of
 *     a device share one resident copy of a profile database; ckm_reduce may be called with another ctx than the one that searched).  ckm_seqs_pack / ckm_seqs_from_fasta use only the ctx's upload
 *     staging area and high-priority stream (serialised by a mutex of the ctx), ckm_hits_write_domtblout touches no state of the ctx: all
 *     three may run on other threads while a search is in flight (MarkerGeneFinder.find reads the next batch of bins and writes the previous batch's
 *     tables that way).  Searches of different ctxs of ONE device run concurrently but take their SSV phases one after the other
 *     (a device-wide baton inside the library).  The library never falls back to a CPU implementation: without a usable HIP
 *     device ckm_ctx_create() fails with CKM_ENODEV and nothing else can be called.
 */
#ifndef CHECKM_HIP_H
#define CHECKM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CKM_ABI_VERSION 12   /* the MarkerSetBuilder entries (ckm_mset_*) are additive: CKM_ABI_VERSION stays 12; so are ckm_sim_*, ckm_simscaf_*, ckm_place_*, ckm_nhmm_*, ckm_select_*, ckm_gtree_*, ckm_genetree_* and ckm_nearid_* */

enum {
  CKM_OK      =  0,
  CKM_EINVAL  = -1,   /* bad argument */
  CKM_EIO     = -2,   /* file could not be read/written */
  CKM_EFORMAT = -3,   /* malformed HMMER3 profile / input */
  CKM_ENODEV  = -4,   /* no usable HIP device */
  CKM_EHIP    = -5,   /* HIP runtime error */
  CKM_ENOMEM  = -6,
  CKM_ERANGE  = -7    /* size limit exceeded (see DESIGN.md limits) */
};

typedef struct ckm_ctx      ckm_ctx;
typedef struct ckm_profiles ckm_profiles;
typedef struct ckm_seqs     ckm_seqs;
typedef struct ckm_hits     ckm_hits;
typedef struct ckm_qa       ckm_qa;

const char *ckm_last_error(void);
int         ckm_abi_version(void);

/* Replaces the "is hmmsearch on PATH" probe, checkm/hmmer.py:131-137 (HMMERRunner.checkForHMMER). */
int ckm_device_count(int *n);
int ckm_ctx_create(int device, ckm_ctx **out);
void ckm_ctx_destroy(ckm_ctx *ctx);

/* ---- profiles ------------------------------------------------------------------------------
 * Replaces hmmsearch's reading of <hmmfile> (checkm/hmmer.py:70) and the header skim of
 * checkm/hmmerModelParser.py:54-83.  Parses a HMMER3/f ASCII file completely (headers, COMPO,
 * emissions, transitions, STATS LOCAL), configures the multihit-local search profiles and uploads
 * the score tables to HBM.  The header view is the RAW per-record view; the sticky ACC/GA/TC/NC
 * carry-over quirk of HmmModelParser.simpleParse is applied by the Python mirror, not here. */
typedef struct {
  const char *name;      /* NAME */
  const char *acc;       /* ACC or NULL */
  const char *desc;      /* DESC or NULL */
  int32_t     leng;      /* LENG */
  int32_t     has_ga, has_tc, has_nc;
  double      ga[2], tc[2], nc[2];   /* float64: CheckM compares them as Python floats with text scores */
  float       evparam[6];   /* MSV mu,lambda; VITERBI mu,lambda; FORWARD tau,lambda */
  int32_t     searchable;   /* 0: the model is longer than the kernels are instantiated for (LENG > 4096; models of 2049..4096 nodes are searched, through the exact MSV kernel instead of SSV): it keeps its place in the database, but a
                               ckm_search / ckm_align that selects it fails with CKM_ERANGE naming it */
} ckm_model_header;

int  ckm_profiles_load(ckm_ctx *ctx, const char *hmm_path, ckm_profiles **out);
int  ckm_profiles_count(const ckm_profiles *p, int32_t *n);
int  ckm_profiles_header(const ckm_profiles *p, int32_t i, ckm_model_header *out);
void ckm_profiles_free(ckm_profiles *p);

/* ---- target sequences ----------------------------------------------------------------------
 * Replaces hmmsearch's reading of <seqfile> (the genes.faa written at
 * checkm/markerGeneFinder.py:113-127).  `text` holds the residues of all sequences of all bins
 * back to back (no separators); sequence s is text[seq_off[s] .. seq_off[s+1]).  Bin b owns
 * sequences bin_off[b] .. bin_off[b+1]; Z of a bin = its sequence count, as one hmmsearch
 * run per bin has it.  names/descs (nseq entries, descs may be NULL) are copied. */
int  ckm_seqs_pack(ckm_ctx *ctx, const char *text, const uint64_t *seq_off, uint32_t nseq,
                   const uint32_t *bin_off, uint32_t nbins,
                   const char *const *names, const char *const *descs, ckm_seqs **out);
/* Same, reading the sequences itself: one protein FASTA file per bin (the bins/<binId>/genes.faa files of
 * checkm/markerGeneFinder.py:113-127; what hmmsearch does with <seqfile>).  Name = header up to the first
 * whitespace, description = the rest; residues are digitized on the fly.  Plain text files only. */
int  ckm_seqs_from_fasta(ckm_ctx *ctx, const char *const *paths, uint32_t nbins, ckm_seqs **out);
int  ckm_seqs_count(const ckm_seqs *s, uint32_t *nseq, uint32_t *nbins);
int  ckm_seqs_bin_offsets(const ckm_seqs *s, const uint32_t **bin_off);          /* [nbins+1], owned by s */
int  ckm_seqs_name(const ckm_seqs *s, uint32_t i, const char **name, const char **desc, int32_t *len);
int  ckm_seqs_residues(const ckm_seqs *s, uint64_t *total);
void ckm_seqs_free(ckm_seqs *s);

/* ---- the scan ------------------------------------------------------------------------------
 * Replaces one `hmmsearch --domtblout T --notextw -E <E> --domE <domE> --noali` process per bin
 * (checkm/markerGeneFinder.py:134-142 -> checkm/hmmer.py:61-74).
 * Bin b is searched with models model_idx[model_off[b] .. model_off[b+1]) in that order
 * (the order of the temporary HMM file of checkm/markerSets.py:326-343); model_off == NULL
 * means every model of `p`, in file order, for every bin. */
int  ckm_search(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s,
                const uint32_t *model_off, const uint32_t *model_idx,
                double E, double domE, ckm_hits **out);

/* One entry per reported domain = one domtblout row (column contract: checkm/hmmer.py:255-285). */
typedef struct {
  uint64_t        n;            /* rows */
  uint32_t        nbins;
  const uint64_t *bin_row_off;  /* [nbins+1] rows of bin b, already in domtblout order */
  const uint32_t *seq;          /* global sequence index (target_name / description / tlen) */
  const uint32_t *model;        /* profile index (query_name / accession / qlen) */
  const int32_t  *tlen, *qlen;
  const double   *full_evalue;  const float *full_score, *full_bias;
  const int32_t  *dom_idx, *ndom;
  const double   *c_evalue, *i_evalue; const float *dom_score, *dom_bias;
  const int32_t  *hmm_from, *hmm_to, *ali_from, *ali_to, *env_from, *env_to;
  const float    *acc;
  /* Only when the struct is INPUT to ckm_reduce (a table parsed from existing domtblout text):
   * target name of every row (prodigal `<contig>_<n>` form, resultsParser.py:410-422).  NULL in
   * the struct ckm_hits_columns() fills: those rows take their names from the ckm_seqs. */
  const char *const *target_name;
  /* INPUT only, optional: the two scores as float64 exactly as parsed from the text (Python floats in the
   * reference).  float32 cannot hold "25.3" exactly, and vetHit compares scores with cutoffs such as GA 25.30. */
  const double *full_score_d, *dom_score_d;
} ckm_hit_columns;

int  ckm_hits_columns(const ckm_hits *h, ckm_hit_columns *out);
void ckm_hits_free(ckm_hits *h);

/* Writes bin b's rows as hmmsearch --domtblout text, the file every later CheckM stage re-reads
 * (checkm/resultsParser.py:191-204; written today by hmmsearch itself, checkm/hmmer.py:70). */
int  ckm_hits_write_domtblout(const ckm_hits *h, const ckm_profiles *p, const ckm_seqs *s,
                              uint32_t bin, const char *path);

/* ---- per-stage counters of the last ckm_search on this ctx (bench.py) --- */
typedef struct {
  uint64_t pairs_ssv, pairs_msv_full, pairs_bias, pairs_vit, pairs_fwd, pairs_dom, envelopes;
  uint64_t regions_multi;       /* regions resolved by the stochastic trace ensemble */
  uint64_t pairs_vit_exact;     /* Viterbi pairs re-run by the exact kernel (bound failed F2 with the J flag set) */
  uint64_t cells_ssv;           /* sum over pairs of L*M: GCUPS denominator */
  uint64_t residue_hmm;         /* sum over pairs of L */
  double   ms_ssv, ms_filters, ms_fwdbwd, ms_domains, ms_host, ms_total;
  uint32_t ssv_launches;
  uint32_t cascade_fallback_lanes; /* lanes (length classes) of the last search that outgrew the device-side tables / workspace of the
                                      device-driven cascade and were run by the host-driven one instead (0 in the normal case) */
  uint64_t ws_cap_bytes, ws_used_bytes;  /* float workspace of the device-driven cascade: allocated, and the high-water mark the search asked for */
} ckm_search_stats;
/* Replaces the text `hmmsearch -o <hmmerOut>` leaves when CheckM keeps alignments (bKeepAlignment: checkm/markerGeneFinder.py:138-142
 * drops --noali): per query model the score table and, per reported domain, the alignment of the envelope's optimal-accuracy path
 * (model consensus / identity-or-'+' line / target with inserts in lower case / PP line: the posterior probability of every aligned
 * residue in the state that emits it, in hmmsearch's one-character code).  The `exp` column of hmmsearch's score table is not produced;
 * CheckM never reads this file back. */
int ckm_hits_write_alignments(ckm_ctx *ctx, const ckm_hits *h, const ckm_profiles *p, const ckm_seqs *s, uint32_t bin, const char *path);

int ckm_last_search_stats(const ckm_ctx *ctx, ckm_search_stats *out);

/* Starts allocating, on a background thread, the float workspace a search of `pairs` (ORF, model) pairs will ask for, so that the
 * allocation (tens of GB: seconds of hipMalloc) runs beside the caller's reading of FASTA files and profile databases instead of
 * inside the first ckm_search.  `cells` is what ckm_search sizes the workspace from: the sum, over the bins of the search and over the
 * models each bin is scanned against, of (Mp + 64) * Mp with Mp = 64 * ceil(M / 64) -- a marker model finds about one domain per bin
 * and a domain costs its envelope's matrices.  Returns at once; ckm_search / ckm_align / the diagnostics wait for it.  Replaces nothing
 * of the reference (one hmmsearch process per bin allocates per process, checkm/hmmer.py:70): it exists because one context serves a
 * whole batch of bins. */
int ckm_ctx_reserve(ckm_ctx *ctx, uint64_t pairs, double cells);

/* ---- the reduction --------------------------------------------------------------------------
 * Replaces ResultsParser.parseBinHits -> ResultsManager.{vetHit,addHit} -> PFAM.filterHitsFromSameClan
 * -> identifyAdjacentMarkerGenes -> geneCounts -> MarkerSet.genomeCheck
 * (checkm/resultsParser.py:76-119,340-537; checkm/util/pfam.py:86-147; checkm/markerSets.py:206-238).
 * Hits come either from ckm_search (h != NULL) or, for tables parsed from existing domtblout
 * text, through `ext` (same columns, text-rounded values).  */
typedef struct {
  /* per model (index = profile index, or caller's own model numbering when ext is used) */
  uint32_t        nmodels;
  const int32_t  *qlen;
  const uint8_t  *thr_kind;     /* 0 none, 1 NC(TIGR), 2 GA, 3 TC, 4 NC : the cascade of resultsParser.py:356-367, resolved by the caller from the (sticky) header view */
  const double   *thr_full, *thr_dom; /* Python floats in the reference: compared as float64 */
  const uint8_t  *is_pf;        /* marker id starts with 'PF' (pfam.py:97) */
  const int32_t  *clan;         /* clan id or -1 (pfam.py:116: None==None counts as same clan) */
  const uint32_t *nest_off, *nest_idx;   /* CSR: models nested with model m (pfam.py:135) */
  const uint32_t *key;          /* models sharing one accession share a key (markerHits dict key) */
} ckm_model_info;

typedef struct {
  int32_t ignore_thresholds, skip_pseudogene_correction, skip_adj_correction, individual_markers;
  double  evalue_threshold, length_threshold;
  const uint8_t *bin_select;    /* NULL = every bin; else only bins with a non-zero byte are reduced */
  /* Threshold VARIANTS: the reference resolves a model's GA/TC/NC from the header view of the BIN's own model file, and a sticky
   * header parse (hmmerModelParser.py:54-83) can give the same model different cutoffs in different subsets.  With nvariants > 1,
   * ckm_model_info.thr_kind / thr_full / thr_dom hold nvariants x nmodels entries (variant-major) and bin b uses variant
   * bin_variant[b]; nvariants <= 1 or bin_variant == NULL: one table for every bin. */
  uint32_t        nvariants;
  const uint32_t *bin_variant;  /* [nbins] or NULL */
} ckm_reduce_flags;

typedef struct {
  /* CSR over bins -> collocated sets -> marker keys */
  uint32_t        nbins;
  const uint32_t *set_off;      /* [nbins+1] */
  const uint32_t *marker_off;   /* [nsets+1] */
  const uint32_t *marker_key;   /* [nmarkers] key (see ckm_model_info.key) */
} ckm_marker_sets;

int  ckm_reduce(ckm_ctx *ctx, const ckm_hits *h, const ckm_hit_columns *ext, const ckm_seqs *s,
                const ckm_model_info *mi, const ckm_reduce_flags *fl, const ckm_marker_sets *ms, ckm_qa **out);

typedef struct {
  uint32_t        nbins;
  const int32_t  *hist;         /* [nbins*6] markers with 0,1,2,3,4,5+ hits (resultsParser.py:513-529) */
  const double   *completeness, *contamination;   /* markerSets.py:206-238 */
  const uint32_t *set_off;      /* [nbins+1] */
  const int32_t  *set_present, *set_multi;        /* per collocated set */
  /* surviving hits (ResultsManager.markerHits after all filters), grouped by bin then marker key in
   * the reference's dict/list order */
  uint64_t        nkept;
  const uint64_t *kept_bin_off; /* [nbins+1] */
  const uint32_t *kept_key;     /* marker key */
  const uint64_t *kept_row;     /* row index into the hit columns */
  const uint64_t *kept_row2;    /* second row when two adjacent ORFs were merged, else UINT64_MAX */
  const int32_t  *kept_tlen, *kept_hmm_from, *kept_hmm_to, *kept_ali_from, *kept_ali_to, *kept_env_from, *kept_env_to;
} ckm_qa_columns;

int  ckm_qa_columns_get(const ckm_qa *q, ckm_qa_columns *out);
void ckm_qa_free(ckm_qa *q);

/* The set-counting kernel alone: replaces the counting loops of MarkerSet.genomeCheck
 * (checkm/markerSets.py:206-238) and ResultsManager.geneCounts (checkm/resultsParser.py:513-529)
 * for caller-supplied copy numbers.  marker_count[i] = number of hits of marker i of the CSR
 * (i indexes ms->marker_key), marker_first[i] != 0 iff this is the first occurrence of that marker
 * within its bin.  Outputs: set_present/set_multi [nsets], hist [nbins*6], and per bin the
 * individual-marker totals present_total/multi_total [nbins].  The float64 division is left to the
 * caller, to be done in the reference's accumulation order. */
int  ckm_count_sets(ckm_ctx *ctx, const ckm_marker_sets *ms, const int32_t *marker_count, const uint8_t *marker_first,
                    int32_t *set_present, int32_t *set_multi, int32_t *hist, int32_t *present_total, int32_t *multi_total);

/* ---- alignment of marker genes to their models ---------------------------------------------------
 * Replaces `hmmalign --outformat Pfam <hmm> <seqs>` (checkm/hmmer.py:76-95, called from HmmerAligner._alignMarker,
 * checkm/hmmerAligner.py:275-302) as far as CheckM consumes it: _maskAlignment (hmmerAligner.py:325-352) keeps only the
 * match ('#=GC RF' x) columns, i.e. per model node the residue its match state emits on the optimal-accuracy path, or a gap.
 * Pair j aligns the WHOLE sequence seq[j] to model[j] (unihit local profile, length model of that sequence, Forward / Backward /
 * decoding / optimal accuracy -- hmmalign's own per-sequence computation).  node_residue[out_off[j] + k], k = 0..M-1, receives
 * the 1-based residue index emitted by match state k+1, or 0 (node deleted, or outside the local alignment).
 * out_off[j+1] - out_off[j] must equal the length of model[j].  A pair whose posterior decoding leaves the float range (the
 * eslERANGE case of HMMER's decoding: e.g. two strong copies of the domain in one sequence under this one-domain model) reports
 * no column at all (every entry 0). */
int  ckm_align(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s, const uint32_t *model, const uint32_t *seq, uint32_t n,
               const uint64_t *out_off, int32_t *node_residue);

/* ---- tables written by an earlier command -----------------------------------------------------
 * Replaces HMMERParser.readHitsDOM / HmmerHitDOM (checkm/hmmer.py:184-200, 255-285) and the serial per-bin loop around them
 * (checkm/resultsParser.py:94, 191-204): the domtblout text of all bins is parsed once, on a few threads, into the column form
 * ckm_reduce takes as `ext`.  No device is needed.  A path that cannot be opened gives an empty bin with bin_missing = 1
 * (the reference prints the IOError and goes on, resultsParser.py:200-204); a malformed row is CKM_EFORMAT. */
typedef struct ckm_tables ckm_tables;
typedef struct {
  ckm_hit_columns    cols;               /* numeric columns, target_name, full_score_d/dom_score_d; seq = row index;
                                            model = slot set by ckm_tables_assign_models (UINT32_MAX = not in the list) */
  const char *const *target_accession, *const *query_name, *const *query_accession /* '-' replaced by the name */, *const *description;
  const double      *full_bias_d, *dom_bias_d, *acc_d;      /* the remaining text floats as float64 (Python floats in HmmerHitDOM) */
  const uint8_t     *bin_missing;        /* [nbins] */
} ckm_table_columns;
int  ckm_tables_read(const char *const *paths, uint32_t nbins, ckm_tables **out);
/* model slot of every row = index of its query accession in keys[] (the markerHits keys of the caller's ckm_model_info) */
int  ckm_tables_assign_models(ckm_tables *t, const char *const *keys, uint32_t nkeys, uint64_t *unknown_rows);
int  ckm_tables_get(const ckm_tables *t, ckm_table_columns *out);
void ckm_tables_free(ckm_tables *t);

/* ---- gene calling, first slice ------------------------------------------------------
 * The deterministic front end of the gene finder CheckM runs before the scan -- `prodigal -p single -m -f gff -g <11|4>`, twice per bin,
 * checkm/prodigal.py:74,86-93,131-133: start / stop codon flags of all six frames and the start / stop NODES the gene finder's dynamic
 * program works on (Prodigal 2.6.3 node.c: add_nodes), for all contigs of a bin in two kernel launches.  `text` holds the contigs'
 * nucleotides (ASCII, any case; anything but ACGTU is "no base"), contig c = text[contig_off[c] .. contig_off[c+1]).  The rest of the gene
 * finder is ckm_genes_call below. */
typedef struct ckm_orf ckm_orf;
typedef struct {
  uint64_t        n;            /* nodes, sorted by (contig, position, strand [forward first: node.c compare_nodes], type, stop_val, edge) */
  const uint32_t *contig;
  const int32_t  *ndx;          /* position of the codon's first base on the FORWARD strand's coordinates (node.c: ndx) */
  const int32_t  *stop_val;     /* start node: the stop that closes its ORF; stop node: the previous stop of its frame (node.c: stop_val) */
  const uint8_t  *type;         /* 0 ATG, 1 GTG, 2 TTG, 3 stop */
  const uint8_t  *strand_rev;   /* 0 forward, 1 reverse */
  const uint8_t  *edge;         /* the ORF runs off an end of the contig */
  double          ms_flags, ms_chain;   /* kernel times of this call (HIP events): the streaming flag kernel, the per-frame chains */
  uint64_t        bases, padded_bytes;  /* nucleotides given; bytes the flag kernel read (= wrote) */
} ckm_orf_columns;
int  ckm_orf_scan(ckm_ctx *ctx, const char *text, const uint64_t *contig_off, uint32_t ncontigs, int trans_table, int closed_ends, ckm_orf **out);
int  ckm_orf_columns_get(const ckm_orf *o, ckm_orf_columns *out);
void ckm_orf_free(ckm_orf *o);
/* measurement hook (bench.py: gene_front_end): the streaming flag kernel over nbytes of device-generated nucleotides, average ms of reps launches */
int  ckm_debug_orf_flags(ckm_ctx *ctx, uint64_t nbytes, uint32_t reps, double *ms);

/* ---- gene calling, the body -----------------------------------------------------------
 * Replaces the two `prodigal -p single -q -m -f gff -g <table> -a genes.faa -i <bin>` processes per bin of checkm/prodigal.py:80-93
 * (ProdigalRunner.run) for a BATCH of bins and ONE translation table per call: training on each bin's own sequence (GC-frame bias, hexamer
 * coding statistics, start-site model), node scoring, the dynamic program over the nodes, gene records and their translations -- the
 * single-genome mode of Prodigal 2.6.3 as restated in oracle/gene_full.c (parity unpinned: no prodigal exists next to the reference).
 * NOT built: `-p meta` (checkm/prodigal.py:80-83 uses it below 100 kb; prodigal refuses to train below 20 kb): such a bin comes back with
 * bin_trained = 0 and no genes, and the caller decides (checkm_amd/prodigal.py falls back to an external binary or reports the bin).
 * text: all contigs' nucleotides (ASCII, any case; anything but ACGTU is an unknown base); contig c = text[contig_off[c] .. contig_off[c+1]);
 * bin b owns contigs bin_first[b] .. bin_first[b+1]-1.  mask_n_runs = prodigal's -m (runs of >= 50 unknown bases hide the genes crossing them). */
typedef struct ckm_genes ckm_genes;
typedef struct {
  uint64_t        n;                 /* genes, bin by bin, contig by contig, in order along the contig */
  const uint32_t *bin, *contig;      /* contig: index into the call's contig table */
  const int32_t  *begin, *end;       /* 1-based, inclusive, on the contig's forward strand (GFF columns 4 and 5) */
  const int8_t   *strand;            /* +1 / -1 */
  const uint8_t  *start_type;        /* 0 ATG, 1 GTG, 2 TTG, 3 Edge */
  const uint8_t  *partial_left, *partial_right;
  const int32_t  *rbs_bin;           /* Shine-Dalgarno bin 0..27 the start was credited with, or -1 (upstream motif / none) */
  const int32_t  *mot_len, *mot_ndx, *mot_spacer;   /* upstream motif of organisms without SD: length 3..6 (0 none), its base-4 index, spacer */
  const double   *gc_cont, *conf, *score, *cscore, *sscore, *rscore, *uscore, *tscore;
  const uint64_t *prot_off;          /* [n + 1] */
  const char     *prot;              /* translations, '*' for the stop of a complete gene */
  uint64_t        nbins;
  const uint8_t  *bin_trained, *bin_uses_sd;
  const double   *bin_gc;
  const uint64_t *bin_bases, *bin_coding, *bin_nodes;   /* nucleotides, bases inside genes (sum of gene lengths), start/stop nodes of the contigs */
  double          ms_nodes, ms_dp_train, ms_score, ms_dp_find, ms_total;   /* wall to the nodes; kernel times (HIP events) of both dynamic programs and of the per-node scores; wall of the call */
} ckm_genes_columns;
int  ckm_genes_call(ckm_ctx *ctx, const char *text, const uint64_t *contig_off, uint32_t ncontigs, const uint32_t *bin_first, uint32_t nbins,
                    int trans_table, int closed_ends, int mask_n_runs, ckm_genes **out);
int  ckm_genes_columns_get(const ckm_genes *g, ckm_genes_columns *out);
void ckm_genes_free(ckm_genes *g);
/* Several ckm_genes_call may run at once on one context (each takes a stream of its own): the gene finder is latency-bound, its
 * throughput comes from calls in flight.  closed_ends must be 0 (CheckM never passes prodigal's -c; ABI 6 refuses it).
 * ckm_genes_coding_union: bases of every bin covered by at least one gene -- ProdigalGeneFeatureParser.codingBases summed over the
 * bin's contigs (checkm/prodigal.py:246-274), the numerator of the coding density that picks the translation table (:117-133).
 * ckm_genes_write_bin: genes.faa / genes.gff (/ genes.fna when nt_path is not NULL) of one bin in prodigal's layout, the files
 * ProdigalRunner.run leaves in bins/<binId>/ (checkm/prodigal.py:86-93,136-153); contig_ids[c] = header of contig c up to the first
 * white space (checkm/util/seqUtils.py:180-211), text / contig_off / bin_first as passed to ckm_genes_call. */
int  ckm_genes_coding_union(const ckm_genes *g, uint64_t *bases /* [nbins] */);
int  ckm_genes_write_bin(const ckm_genes *g, uint32_t bin, int trans_table, const char *const *contig_ids, const char *text, const uint64_t *contig_off,
                         const uint32_t *bin_first, const char *aa_path, const char *gff_path, const char *nt_path);

/* ---- the nucleotide files of a batch of bins, laid out for ckm_genes_call / ckm_genes_write_bin (ABI 7) --------------------------------
 * What checkm/prodigal.py:86-93 hands to prodigal by path (`-i <bin>`): plain (uncompressed) nucleotide FASTA files, one per bin, read by
 * host threads (a file per thread) with the record rules of CheckM's own reader (checkm/util/seqUtils.py:180-211): a record begins with
 * '>' at the start of a line, text before the first one is skipped, the contig id is the header's first blank-delimited word, the
 * sequence is what follows up to the next record without '\n', '\r', ' ', '\t'.  The view's arrays are the arguments of ckm_genes_call
 * (text, contig_off, ncontigs, bin_first, nbins) and ckm_genes_write_bin (contig_ids) and live until ckm_nuc_batch_free. */
typedef struct ckm_nuc_batch ckm_nuc_batch;
typedef struct {
  const char        *text;          /* all contigs' nucleotides end to end */
  const uint64_t    *contig_off;    /* [ncontigs + 1] */
  const uint32_t    *bin_first;     /* [nbins + 1] */
  const char *const *contig_ids;    /* [ncontigs] */
  const uint64_t    *bin_bases;     /* [nbins]: nucleotides of each bin */
  uint32_t           ncontigs, nbins;
} ckm_nuc_batch_view;
int  ckm_nuc_batch_read(const char *const *paths, uint32_t nbins, ckm_nuc_batch **out);
int  ckm_nuc_batch_view_get(const ckm_nuc_batch *b, ckm_nuc_batch_view *out);
void ckm_nuc_batch_free(ckm_nuc_batch *b);

/* ---- bin statistics and tetranucleotide signatures (ABI 8) -----------------------------------------------------------------------------
 * ckm_nucseq_read replaces checkm/util/seqUtils.py:180-211 (readFasta) as BinStatistics._processBin (checkm/binStatistics.py:100-101) and
 * GenomicSignatures.calculate (checkm/genomicSignatures.py:157) call it, rule for rule: the file is read as UTF-8 text (invalid UTF-8 is
 * CKM_EFORMAT, as the reference fails on it), '.gz' names through zlib; "\n", "\r\n" and a lone "\r" end a line; a line of white space
 * only is skipped; a header's id is its first white-space delimited word; every other line loses exactly its last character
 * (line[0:-1]: the line end, or the last character of a file that does not end in one) and keeps blanks and tabs; a repeated id keeps
 * its first place and takes the later record's sequence.  Host threads, a file per thread.  ckm_nuc_batch_read is unchanged: its rules
 * are the gene caller's.  The view lives until ckm_nucseq_free; sequence s = text[seq_off[s] .. seq_off[s] + seq_bytes[s]) (UTF-8
 * bytes, 16-byte aligned), file f owns sequences file_first[f] .. file_first[f+1]-1 in the reference's dict order. */
typedef struct ckm_nucseq ckm_nucseq;
typedef struct {
  const char        *text;
  uint64_t           text_bytes;
  const uint64_t    *seq_off, *seq_bytes;   /* [nseq] */
  const uint32_t    *file_first;            /* [nfiles + 1] */
  const char *const *seq_ids;               /* [nseq] */
  uint32_t           nseq, nfiles;
} ckm_nucseq_view;
int  ckm_nucseq_read(const char *const *paths, uint32_t nfiles, ckm_nucseq **out);
int  ckm_nucseq_view_get(const ckm_nucseq *b, ckm_nucseq_view *out);
void ckm_nucseq_free(ckm_nucseq *b);

/* The device pass over a batch: replaces baseCount / calculateGC / calculateSeqStats (checkm/util/seqUtils.py:279-286,
 * checkm/binStatistics.py:173-234) and GenomicSignatures.seqSignature's counting loop (checkm/genomicSignatures.py:131-149).  Per sequence:
 * count[s*8 + k] = A, C, G, T+U (either case), 'N', 'n', code points (len(seq)), code points other than 'N'; the contig pieces
 * piece_len[piece_off[s] .. piece_off[s+1]) (scaffold.split('NNNNNNNNNN'), 'N' removed, empty pieces dropped); with tetra != 0 the 136
 * canonical 4-mer counts tetra[s*136 ..] in _makeKmerColNames order (windows of four A/C/G/T bytes, either case).  tile_bytes: bytes of
 * sequence per wavefront (0 = 4096; a multiple of 16, at most 1 MiB).  Integer results: identical from run to run. */
typedef struct ckm_nucstats ckm_nucstats;
typedef struct {
  uint32_t        nseq;
  const uint64_t *count;                    /* [nseq * 8] */
  const uint64_t *piece_off;                /* [nseq + 1] */
  const uint64_t *piece_len;
  const uint32_t *tetra;                    /* [nseq * 136] or NULL */
  uint64_t        bytes, tiles, run_starts; /* bytes uploaded, tiles, runs of >= 10 'N' */
  double          ms_upload, ms_count, ms_fill, ms_total;   /* HIP events: upload, count pass, fill pass; wall of the call */
} ckm_nucstats_columns;
int  ckm_nucstats_run(ckm_ctx *ctx, const ckm_nucseq *b, int tetra, uint32_t tile_bytes, ckm_nucstats **out);
int  ckm_nucstats_columns_get(const ckm_nucstats *r, ckm_nucstats_columns *out);
void ckm_nucstats_free(ckm_nucstats *r);

/* Replaces BinStatistics.calculateCodingDensity's file reading (checkm/binStatistics.py:236-253) for every file of a batch, on host threads:
 * gff_paths[f] / faa_paths[f] are bins/<binId>/genes.gff / genes.faa of file f.  coding[f] = bases of f's sequences inside the union of
 * their genes (ProdigalGeneFeatureParser.codingBases summed over the ids), trans_table[f] = the first '# Model Data' line's transl_table
 * (INT32_MIN: none), ngenes[f] = distinct records of genes.faa; all three -1 when the GFF does not exist.  No device needed. */
int  ckm_bin_genes_read(const char *const *gff_paths, const char *const *faa_paths, const ckm_nucseq *b, int64_t *coding, int32_t *trans_table, int64_t *ngenes);

/* ---- `checkm outliers`: per-sequence GC, coding density and tetranucleotide distance against the bin (ABI 9) ----------------------------
 * ckm_seq_genes_read replaces ProdigalGeneFeatureParser.codingBases(seqId) (checkm/prodigal.py:250-273) as
 * BinTools.codingDensityDist calls it (checkm/binTools.py:168-184): gff_paths[f] is bins/<binId>/genes.gff of file f of the batch;
 * coding_per_seq[s] = bases of sequence s inside the union of its genes, 0 for an id without genes.  The parsing is that of
 * ckm_bin_genes_read: the sum over a file's sequences is what that call returns.  missing[f] = 1 and coding_per_seq = -1 for the
 * sequences of a file whose GFF does not exist (the caller reports checkm/binTools.py:242-244).  Host threads, a file per thread. */
int  ckm_seq_genes_read(const char *const *gff_paths, const ckm_nucseq *b, int64_t *coding_per_seq /* [nseq] */, uint8_t *missing /* [nfiles] */);

/* ckm_tetra_profile_read replaces GenomicSignatures.read (checkm/genomicSignatures.py:192-200), which BinTools.identifyOutliers calls
 * once per bin (checkm/binTools.py:236-237): the file GenomicSignatures.calculate writes, read once, its lines split over host threads.
 * Every value equals Python's float(token) bit for bit (strtod is correctly rounded; 'nan' rows included); the first line is the header;
 * a later row of an id replaces the earlier one, as in the dict.  A row without exactly 136 frequencies, or with a token that is not a
 * float, is CKM_EFORMAT.  The view lives until ckm_tetra_profile_free.
 * ckm_tetra_profile_gather: sig[s*136 ..] = the row of sequence s of the batch, looked up by id (tetraSigs[seqId],
 * checkm/binTools.py:194,207); *first_missing = the first sequence whose id the profile does not hold (its row is zeros), or -1. */
typedef struct ckm_tetra_profile ckm_tetra_profile;
typedef struct {
  uint32_t           n;
  const char *const *ids;                   /* [n] */
  const double      *sig;                   /* [n * 136] */
} ckm_tetra_profile_view;
int  ckm_tetra_profile_read(const char *path, ckm_tetra_profile **out);
int  ckm_tetra_profile_view_get(const ckm_tetra_profile *p, ckm_tetra_profile_view *out);
int  ckm_tetra_profile_gather(const ckm_tetra_profile *p, const ckm_nucseq *b, double *sig /* [nseq * 136] */, int64_t *first_missing);
void ckm_tetra_profile_free(ckm_tetra_profile *p);

/* The device pass: replaces gcDist, codingDensityDist, binTetraSig, tetraDiffDist's distances and the comparisons of identifyOutliers
 * (checkm/binTools.py:148-209,263-286; GenomicSignatures.distance, checkm/genomicSignatures.py:189-190) for every bin (= file) of the
 * batch.  count = the counters of ckm_nucstats_run ([nseq * 8]), sig = the gathered profile rows, coding_per_seq = ckm_seq_genes_read.
 * Bounds: table t owns rows tab_off[t] .. tab_off[t+1]-1 of key / lo / hi, one row per sequence-length key in the distribution's dict
 * order; bin k uses table bin_gc_tab[k] (lo, hi: the two percentile bounds of delta GC), bin_cd_tab[k] (lo: the lower bound of delta CD)
 * and every bin table td_tab (hi: the bound of TD).  The caller picks the tables and percentile keys as checkm/binTools.py:249-261 does.
 * Results are float64 and equal the reference's bit for bit (evaluation orders: checkm_amd/csrc/outlier_dev.h); flags: bit 0 GC, 1 CD,
 * 2 TD.  A sequence without A, C, G, T, U (or a bin without sequences) is the reference's ZeroDivisionError: *zero_seq = its index and
 * the call fails with CKM_EINVAL; otherwise *zero_seq = -1. */
typedef struct {
  uint32_t        ntables;
  const uint32_t *tab_off;                  /* [ntables + 1] */
  const double   *key, *lo, *hi;            /* [tab_off[ntables]] */
  const uint32_t *bin_gc_tab, *bin_cd_tab;  /* [nfiles] */
  uint32_t        td_tab;
} ckm_outlier_bounds;
typedef struct ckm_outliers ckm_outliers;
typedef struct {
  uint32_t       nseq, nbins;
  const double  *gc, *delta_gc, *cd, *delta_cd, *td, *weight;   /* [nseq]; weight = len / bin length, the factor of binTetraSig */
  const uint8_t *flags;                                         /* [nseq] */
  const double  *mean_gc, *mean_cd;                             /* [nbins] */
  const double  *bin_sig;                                       /* [nbins * 136] */
  double         ms_upload, ms_seq, ms_binsig, ms_td, ms_flags, ms_total;   /* HIP events: upload and each kernel; wall of the call */
} ckm_outliers_columns;
int  ckm_outliers_run(ckm_ctx *ctx, const ckm_nucseq *b, const uint64_t *count, const double *sig, const int64_t *coding_per_seq,
                      const ckm_outlier_bounds *bounds, int64_t *zero_seq, ckm_outliers **out);
int  ckm_outliers_columns_get(const ckm_outliers *r, ckm_outliers_columns *out);
void ckm_outliers_free(ckm_outliers *r);

/* ---- `checkm merge`: the all-pairs comparison of marker genes (ABI 10) -------------------------------------------------------------------
 * Replaces the double loop of Merger.run (checkm/merger.py:64-106), which builds a merged hit dict and calls geneCounts for every pair
 * of bins.  A bin is: member_bits[b * nwords ..], nwords = (ngenes + 63) / 64, bit g set when marker gene g of the common gene set is a
 * key of the bin's hit dict (a key with an empty list counts); hit_sum[b] = hits to those genes; n_markers[b] = numMarkers() of the
 * bin's most specific marker set.  thr = {minDeltaComp, maxDeltaCont, minMergedComp, maxMergedCont}.  For every pair i < j, in (i, j)
 * order, the device applies merger.py:92 and :100 in float64 (evaluation order: checkm_amd/csrc/merge_dev.h; the merged pair is judged
 * by bin j's n_markers) and reports the pairs that pass, bit-equal to the reference.
 * append_path != NULL: the lines of the reported pairs ('%s\t%s' + 9 x '\t%.2f') are appended to that file, ids from bin_ids[nbins].
 * keep_columns != 0: the columns stay with the result (ckm_merge_columns_get); otherwise only the counts and timings do.
 * The output goes through the device in batches of whole rows of at most budget_bytes (0: CKM_MERGE_BATCH_MB, default 256, << 20);
 * the batches never change the result.  Refused with CKM_EINVAL, nothing computed: a NULL argument, ngenes == 0, n_markers[b] <= 0,
 * hit_sum[b] < 0, a member bit at or beyond ngenes.  ckm_merge_check applies the same tests and needs no device. */
typedef struct ckm_merge ckm_merge;
typedef struct {
  uint64_t        npairs;                   /* reported pairs */
  uint64_t        compared;                 /* nbins * (nbins - 1) / 2 */
  uint64_t        nbatches;                 /* output batches the fill pass ran in */
  int32_t         kept;                     /* 1: the columns below are there */
  const uint32_t *i, *j;                    /* [npairs] */
  const double   *col[9];                   /* [npairs] each: compI, contI, compJ, contJ, deltaComp, deltaCont, delta, compM, contM */
  double          ms_upload, ms_bins, ms_count, ms_scan, ms_fill, ms_download, ms_write, ms_total;   /* HIP events per phase (scan: with the host's row prefix); write and total: wall */
} ckm_merge_columns;
int  ckm_merge_check(uint32_t nbins, uint32_t ngenes, const uint64_t *member_bits, const int64_t *hit_sum, const int32_t *n_markers, const double *thr);
int  ckm_merge_run(ckm_ctx *ctx, uint32_t nbins, uint32_t ngenes, const uint64_t *member_bits, const int64_t *hit_sum, const int32_t *n_markers,
                   const double *thr /* [4] */, const char *const *bin_ids, const char *append_path, uint64_t budget_bytes, int keep_columns, ckm_merge **out);
int  ckm_merge_columns_get(const ckm_merge *r, ckm_merge_columns *out);
void ckm_merge_free(ckm_merge *r);

/* ---- `checkm coverage`: BAM records on the device (additions to ABI 12; no existing entry point changes) ---------------------------------
 * Replaces pysam and the per-read Python loop of Coverage.__workerThread (checkm/coverage.py:186-239).  ckm_bam_open walks the BGZF
 * blocks and parses the BAM header on the host; no device is needed for open / header / close.  ckm_coverage_run inflates the
 * file in batches of whole records (budget_bytes of inflated bytes, 0: CKM_COVERAGE_BATCH_MB, default 256, << 20; the batches never
 * change the result), classifies every record on the device by the chain of coverage.py:209-230 (checkm_amd/csrc/coverage_dev.h) and
 * adds it to its reference's row of out_counters[n_ref][9], all int64: reads, duplicates, secondary or supplementary, failed QC,
 * failed alignment length, failed edit distance, not properly paired, mapped, and the sum of query_alignment_length over the mapped
 * reads.  Records with refID -1 count nowhere.  A handle is read once: a second run on it sees no records.
 * Refused with CKM_EINVAL and a message that names the file and the record's ordinal: bad magic, a truncated block, a failed inflate,
 * a record shorter than its fixed part or running past its buffer, n_ref or a refID out of range, the placeholder of a long CIGAR
 * (real CIGAR in a CG tag: not supported), an auxiliary walk that leaves its record, and an NM tag that is needed and absent or not
 * an integer.  For the last group timing->error_reason is 1 (walk left the record), 2 (NM absent), 3 (NM not an integer) or 4
 * (unknown field type), error_record the ordinal and error_read the read's name.  ckm_coverage_check: the tests of the parameters
 * (no NaN), without a device. */
typedef struct ckm_bam ckm_bam;
typedef struct {
  uint32_t           n_ref;
  const char *const *names;                 /* [n_ref] */
  const int64_t     *lengths;               /* [n_ref] */
  uint64_t           header_bytes;          /* inflated bytes in front of the first record */
} ckm_bam_header_view;
typedef struct {
  double   min_align_per, max_edit_dist_per, min_qc;
  int32_t  all_reads;
  uint64_t budget_bytes;
} ckm_coverage_params;
typedef struct {
  uint64_t records, batches, blocks, inflated_bytes;
  uint32_t error_reason; uint64_t error_record; char error_read[256];
  double   ms_read, ms_inflate, ms_offsets, ms_upload, ms_kernel, ms_download, ms_total;   /* read, inflate, offsets, total: wall; the others: HIP events */
} ckm_coverage_timing;
int  ckm_bam_open(const char *path, ckm_bam **out);
int  ckm_bam_header(const ckm_bam *b, ckm_bam_header_view *out);
void ckm_bam_close(ckm_bam *b);
int  ckm_coverage_check(const ckm_coverage_params *params);
int  ckm_coverage_run(ckm_ctx *ctx, ckm_bam *b, const ckm_coverage_params *params, int64_t *out_counters, ckm_coverage_timing *timing);

/* ---- CoverageWindows of `checkm gc_bias_plot`: per-window read coverage of a BAM on the device (additions to ABI 12) ---------------------
 * Replaces pysam, the float64 depth array per reference and the per-read Python loop of checkm/coverageWindows.py.  The chain is that
 * file's (lines 55-79), NOT the one of ckm_coverage_run: unmapped, duplicate, secondary (0x100 only), QC-fail (0x200 only, no mapping
 * quality), alen < min_align_per * rlen, NM > max_edit_dist_per * rlen, not a proper pair, mapped -- with rlen = l_seq and alen = the
 * reference span of the CIGAR (M, D, N, = and X).  A mapped read adds 1 to the depth of [pos, min(pos + alen, L)).
 * With w = window_size a reference of length L > 0 has (L - 1) / w + 1 slots: window k = [k w, (k + 1) w) for every k with (k + 1) w < L --
 * the windows the reference reports -- and one last slot with the rest (a window that ends exactly at L is that last slot).
 * ckm_coverage_windows_layout: out_first[k] = the first slot of reference k, out_first[n_ref] = all slots (n_ref + 1 values); more than
 * 2^31 - 1 slots: CKM_EINVAL.  ckm_coverage_windows_run reads the file in the batches of ckm_coverage_run (same budget rule) and gives
 *   out_counters[n_ref][9]   reads, classes 1..7 by this chain, and the numerator: the bases covered by mapped reads after clipping
 *                            to [0, L), which is the sum of the reference's slots
 *   out_window_sums[slots]   the sum of the depth over each slot (int64; the caller divides by w, or the numerator by L)
 * A read costs O(1) memory operations whatever alen / w is (checkm_amd/csrc/covwin_dev.h); a scan after the last batch forms the sums.
 * Refusals as for ckm_coverage_run, with two more values of error_reason: 5 (a read without CIGAR reaches the alignment-length test: the
 * reference fails there with a TypeError) and 6 (a mapped read with pos < 0: numpy would wrap the slice; not imitated).
 * ckm_coverage_windows_check: no NaN fraction, 1 <= window_size <= 2^31 - 1; without a device.  A handle is read once. */
typedef struct {
  double   min_align_per, max_edit_dist_per;
  int32_t  all_reads;
  int64_t  window_size;
  uint64_t budget_bytes;
} ckm_coverage_windows_params;
typedef struct {
  uint64_t records, batches, blocks, inflated_bytes;
  uint32_t error_reason; uint64_t error_record; char error_read[256];
  double   ms_read, ms_inflate, ms_offsets, ms_upload, ms_kernel, ms_download, ms_total;   /* as ckm_coverage_timing */
  double   ms_scan;                         /* the scan over the slots (HIP events) */
  uint64_t slots;                           /* out_first[n_ref] */
} ckm_coverage_windows_timing;
int  ckm_coverage_windows_check(const ckm_coverage_windows_params *params);
int  ckm_coverage_windows_layout(const ckm_bam *b, int64_t window_size, int64_t *out_first);
int  ckm_coverage_windows_run(ckm_ctx *ctx, ckm_bam *b, const ckm_coverage_windows_params *params, int64_t *out_counters, int64_t *out_window_sums,
                              ckm_coverage_windows_timing *timing);

/* ---- SequenceWindows of the plot commands: per-window GC, coding density and tetranucleotide distance (additions to ABI 12) ------------
 * Replaces the per-window loops of checkm/plot/gcPlots.py:55-75, gcBiasPlots.py:51-66, codingDensityPlots.py:73-89 and
 * tetraDistPlots.py:63-79 over the sequences of a ckm_nucseq batch.  With w = window_size (1 .. 2^31 - 1), window k = [k w, (k + 1) w)
 * of a sequence of L code points exists while (k + 1) w < L: (L - 1) / w windows for L > 0, none that ends at L, no tail.
 * ckm_seq_windows_layout: out_first[s] = the first window of sequence s, out_first[nseq] = all windows (nseq + 1 values); more than
 * 2^31 - 1 windows: CKM_ERANGE.  No device needed.
 * ckm_seq_windows_run, on the device (checkm_amd/csrc/seqwin_dev.h, kernels_seqwin.hip):
 *   out_base_counts[nwin][4]  A, C, G, T+U of every window after upper-casing (baseCount)
 *   out_seq_counts[nseq][4]   the same over every whole sequence
 *   out_td[nwin]              tetra != 0 and bin_sig != NULL: np.sum(np.abs(sig - bin_sig[file])) with sig_i = count_i / total over the
 *                             136 canonical 4-mers whose four bytes lie inside the window (A/C/G/T either case; a 4-mer across a window
 *                             seam belongs to no window), in the summation order of ckm_outliers_run's TD; nan for a window without one.
 *                             bin_sig: [nfiles * 136], BinTools.binTetraSig of every file
 *   out_tetra_counts[nwin][136]  optional (tetra != 0): the counts themselves; CKM_ERANGE when they do not fit the budget
 *   out_skipped[nseq]         1: the sequence holds non-ASCII bytes (its bytes are not its code points) and was not sent to the device;
 *                             its rows are zero (nan) and the caller computes them
 * piece_bytes: bytes of a window per wavefront (0 = 4096; 16 .. 1 MiB).  budget_bytes: the 544-byte count rows of a batch of windows
 * (0: CKM_NUCSTATS_BATCH_MB, default 1024, << 20); the batches never change the result.  Integer counts, a fixed float64 order:
 * identical from run to run.
 * ckm_seq_windows_coding: out_coding[x] = np.sum(codingBaseMask[k w : (k + 1) w]) of window x (checkm/prodigal.py:250-273), from the
 * parsing of ckm_seq_genes_read: 0 for an id without genes, -1 (and missing[f] = 1) for the windows of a file whose GFF does not
 * exist.  Host threads, a file per thread; no device needed. */
typedef struct {
  uint64_t windows, pieces, batches, bytes, skipped_seqs;
  double   ms_upload, ms_count, ms_td, ms_download, ms_total;   /* HIP events: copies in, count kernel, td kernel, copies out; wall of the call */
} ckm_seq_windows_timing;
int  ckm_seq_windows_layout(const ckm_nucseq *b, int64_t window_size, int64_t *out_first /* [nseq + 1] */);
int  ckm_seq_windows_run(ckm_ctx *ctx, const ckm_nucseq *b, int64_t window_size, int tetra, const double *bin_sig, uint32_t piece_bytes, uint64_t budget_bytes,
                         uint32_t *out_base_counts, uint64_t *out_seq_counts, double *out_td, uint32_t *out_tetra_counts, uint8_t *out_skipped,
                         ckm_seq_windows_timing *timing);
int  ckm_seq_windows_coding(const char *const *gff_paths, const ckm_nucseq *b, int64_t window_size, int64_t *out_coding /* [nwin] */, uint8_t *missing /* [nfiles] */);

/* ---- ReferenceDistributions: the windows behind gc_dist / cd_dist / td_dist (additions to ABI 12) -----------------------------
 * Replaces the sampling loops of CheckM's scripts/distributionDeltaGC.py, distributionDeltaCodingDensity.py and
 * distributionDeltaTetraDiff.py.  The sequences of the batch are joined in file order with sep_len 'N' between them (GC 0, TD 4, CD 10)
 * into one scaffold of L bytes; window x is [starts[x], starts[x] + sizes[x]) of it, anywhere, overlapping freely.
 * stat: 0 gc, 1 cd (both: the two class counters), 2 td.  block: positions per prefix checkpoint (0 = 256; 16 .. 2^20); the result does
 * not depend on it.
 * ckm_refdist_check: CKM_EINVAL with a message for a stat, sep_len (> 1024) or block out of range and for a window with a size below 1
 * or not inside [0, scaffold_len]; CKM_ERANGE for a scaffold of 2^31 - 1 bytes or more and for more than 2^31 - 1 windows.  No device needed.
 * ckm_refdist_run, on the device (checkm_amd/csrc/refdist_dev.h, kernels_refdist.hip), after the same checks:
 *   out_counts[nwin][2]   stat 0 / 1: bytes of the window that are C or G, and that are A, T or U, after upper-casing
 *   out_td[nwin]          stat 2: np.sum(np.abs(genomeSig - sig)) with sig_i = count_i / total over the canonical 4-mers whose four bytes
 *                         lie inside the window (A/C/G/T either case), in the summation order of ckm_outliers_run's TD; nan without one
 *   out_totals[138]       the scaffold's gc, at (stat 0 / 1) and its 136 canonical 4-mer counts (stat 2: genomeSig_i = count_i / sum)
 * A sequence with non-ASCII bytes: CKM_EINVAL (the caller computes such a genome).  budget_bytes: the 544-byte count rows of a batch of
 * TD windows (0: CKM_NUCSTATS_BATCH_MB, default 1024, << 20); the batches never change the result.
 * ckm_refdist_coding: out_coding[x] = np.sum(codingBaseMask[starts[x] : starts[x] + sizes[x]]) of sequence seq_id of the GFF
 * (ProdigalGeneFeatureParser.codingBases(seqId, start, end), checkm/prodigal.py:250-273) and *out_total = codingBases(seqId), from the
 * parsing of ckm_seq_genes_read; 0 for an id without genes.  CKM_EIO when the file does not exist.  No device needed. */
typedef struct {
  uint64_t windows, blocks, batches, bytes;
  double   ms_scaffold, ms_upload, ms_blocks, ms_scan, ms_windows, ms_download, ms_total;   /* host join; HIP events; wall of the call */
} ckm_refdist_timing;
int  ckm_refdist_check(int stat, uint32_t sep_len, uint32_t block, uint64_t scaffold_len, const int64_t *starts, const int64_t *sizes, uint64_t nwin);
int  ckm_refdist_run(ckm_ctx *ctx, const ckm_nucseq *b, int stat, uint32_t sep_len, uint32_t block, const int64_t *starts, const int64_t *sizes, uint64_t nwin,
                     uint64_t budget_bytes, uint32_t *out_counts, double *out_td, uint64_t *out_totals, ckm_refdist_timing *timing);
int  ckm_refdist_coding(const char *gff_path, const char *seq_id, const int64_t *starts, const int64_t *sizes, uint64_t nwin, int64_t *out_coding /* [nwin] */,
                        int64_t *out_total);

/* ---- Unbinned: `checkm unbinned` (additions to ABI 12) -------------------------------------------------------------------------
 * Replaces Unbinned.run (checkm/unbinned.py:33-85): the contigs of an assembly that sit in no bin and have at least minSeqLen code points,
 * written with their length and GC.
 * ckm_fasta_ids_read: the ids, bytes and code points of every sequence of FASTA files by the rules of ckm_nucseq_read (a repeated id keeps
 * its place and takes the later record), a file per host thread; no sequence text is kept.  No device needed.
 * ckm_unbinned_select, on the host: keep[s] = 1 iff the id of assembly sequence s is the id of no sequence of `bins` (a hash set, ids
 * compared byte by byte) and its code points are >= min_len; and the totals Unbinned.run logs.  bins may be NULL (no bin files); assembly may be NULL
 * (only the bins' two totals are filled, keep is not touched).
 * ckm_unbinned_count, on the device (checkm_amd/csrc/unbinned_dev.h, kernels_unbinned.hip): counts[s] = A, C, G, T+U after upper-casing
 * and the code points of every sequence with keep[s] != 0, zeros for the others.  Only the tiles of kept sequences travel, in batches of
 * at most budget_bytes of text (0: CKM_NUCSTATS_BATCH_MB, default 1024, << 20).  tile_bytes: 0 = 4096, else a multiple of 1024 up to 1 MiB.
 * Neither changes the result.  A keep mask of zeros (or of empty sequences only) does not touch the device.  CKM_EINVAL for a NULL
 * argument or a bad tile_bytes, before any device call.
 * ckm_unbinned_write: the two files of Unbinned.run straight from the batch's buffers: '>' id '\n' sequence '\n' per kept sequence, and
 * "Sequence Id\tLength\tGC\n" with one "%s\t%d\t%.2f\n" row (id, code points, (double)(g + c) * 100 / (double)(a + c + g + t)) each.  A
 * kept sequence with a + c + g + t == 0 ends the writing after its FASTA record and before its row: *zero_seq = its index, else -1; both
 * files are closed either way and the call returns CKM_OK.  CKM_EINVAL when counts[s][4] of a kept sequence is not the reader's code
 * points; CKM_EIO when a file cannot be written. */
typedef struct ckm_fasta_ids ckm_fasta_ids;
typedef struct {
  const char *const *seq_ids;          /* [nseq], NUL terminated */
  const uint64_t *seq_bytes, *seq_cp;  /* [nseq] */
  const uint32_t *file_first;          /* [nfiles + 1] */
  uint32_t nseq, nfiles;
} ckm_fasta_ids_view;
typedef struct {
  uint64_t binned_ids, binned_bases;   /* len(binnedSeqs): distinct ids; totalBinnedBases: every bin file's own sequences */
  uint64_t all_seqs, all_bases;
  uint64_t unbinned_seqs, unbinned_bases;
} ckm_unbinned_totals;
typedef struct {
  uint64_t kept, tiles, batches, bytes;                        /* bytes: padded text of the kept tiles, what the kernel reads */
  double   ms_stage, ms_upload, ms_count, ms_sum, ms_download, ms_total;   /* host packing; HIP events; wall of the call */
} ckm_unbinned_timing;
int  ckm_fasta_ids_read(const char *const *paths, uint32_t nfiles, ckm_fasta_ids **out);
int  ckm_fasta_ids_view_get(const ckm_fasta_ids *b, ckm_fasta_ids_view *out);
void ckm_fasta_ids_free(ckm_fasta_ids *b);
int  ckm_unbinned_select(const ckm_fasta_ids *bins, const ckm_nucseq *assembly, int64_t min_len, uint8_t *keep /* [nseq] */, ckm_unbinned_totals *totals);
int  ckm_unbinned_count(ckm_ctx *ctx, const ckm_nucseq *assembly, const uint8_t *keep, uint32_t tile_bytes, uint64_t budget_bytes, uint64_t *counts /* [nseq][5] */,
                        ckm_unbinned_timing *timing);
int  ckm_unbinned_write(const ckm_nucseq *assembly, const uint8_t *keep, const uint64_t *counts /* [nseq][5] */, const char *seq_path, const char *stats_path,
                        int64_t *zero_seq);

/* ---- AminoAcidIdentity: all pairs of copies of every multi-copy marker (additions to ABI 12) -----------------------------------
 * Replaces the pair loop of AminoAcidIdentity.run and its aai() (checkm/aminoAcidIdentity.py:65-89, :127-161).  A group is one
 * <bin>/<marker>.masked.faa: rows group_row_off[g] .. group_row_off[g + 1] - 1, row r being bytes row_off[r] .. row_off[r + 1] - 1 of
 * `text` (rows back to back, no padding: the library packs them at its own 16-byte stride).  group_row_off holds ngroups + 1 entries,
 * row_off group_row_off[ngroups] + 1, text row_off[last] bytes; both tables start at 0 and never fall.  Rows are compared as bytes.
 * For every pair i < j of a group, i major and j minor, groups in the caller's order (pair_off[g] .. pair_off[g + 1] - 1 are the pairs of
 * group g; a group of fewer than two rows has none), the device computes (checkm_amd/csrc/aai_dev.h, kernels_aai.hip):
 *   start = the first column where neither row holds '-', or L; end = L lowered past the trailing columns where either row holds '-',
 *   never looking at column 0 (columns 1 .. L-1 all gapped: end = 1; L = 1: end = 1; L = 0: end = 0);
 *   over [start, end): mismatches = columns whose bytes differ (a residue against '-' and a case difference are mismatches), compared =
 *   columns that are not '-' in both rows; aai = 0.0 for compared == 0, else 1.0 - (double)mismatches / (double)compared in IEEE double.
 * The packed text and the outputs go through the device in batches of at most budget_bytes (0: CKM_AAI_BATCH_MB, default 64, << 20; a
 * batch holds at least one pair); the batches never change a result.  A call without a pair does not touch the device.
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, a table that does not start at 0 or falls, rows of unequal length in a
 * group; CKM_ERANGE for rows of more than 4096 bytes (the model limit of DESIGN §8) or more than 2^20 rows in a group.  ckm_aai_check
 * applies the same tests and needs no device. */
typedef struct ckm_aai ckm_aai;
typedef struct {
  uint64_t        ngroups, npairs;
  uint64_t        nbatches;                 /* batches the pairs ran in */
  uint64_t        bytes;                    /* packed text sent, over all batches */
  const uint64_t *pair_off;                 /* [ngroups + 1] */
  const int32_t  *mismatches, *compared;    /* [npairs] */
  const double   *aai;                      /* [npairs] */
  double          ms_pack, ms_upload, ms_kernel, ms_download, ms_total;   /* host packing; HIP events per phase; wall of the call */
} ckm_aai_columns;
int  ckm_aai_check(uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text);
int  ckm_aai_run(ckm_ctx *ctx, uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text, uint64_t budget_bytes, ckm_aai **out);
int  ckm_aai_columns_get(const ckm_aai *r, ckm_aai_columns *out);
void ckm_aai_free(ckm_aai *r);

/* ---- MarkerSetBuilder: marker genes and co-located marker pairs of a batch of genome sets (additions to ABI 12) --------------
 * Replaces the loops of scripts/genometreeworkflow/markerSetBuilder.py: markerGenes (:131-157), missingGenes (:486-510), duplicateGenes
 * (:512-536) and colocatedGenes (:159-192).  checkm_amd/csrc/markerset_dev.h, kernels_markerset.hip.
 *
 * The table, for ngenomes genomes and nfamilies families, genome-major: count_class[g * nfamilies + f] = 0, 1 or 2 (more than one) is the
 * class of geneCountTable[f].get(g, 0); the start positions of the copies of f in g (the first number of every entry of
 * IMG._genomeFamilyPositions(g)[f], checkm/util/img.py:420-490, contigs laid end to end) are pos[pos_off[g * nfamilies + f] ..
 * pos_off[g * nfamilies + f + 1] - 1]; pos_off holds ngenomes * nfamilies + 1 entries, starts at 0 and never falls.  Class and copies are
 * independent of each other.  ckm_mset_table_create copies the table to the device (positions as int32), where it stays until
 * ckm_mset_table_free; ms_upload (may be NULL) receives the milliseconds of the copy.
 *
 * A query is a list of genomes: qg[qg_off[q] .. qg_off[q + 1] - 1], indices into the table (qg_off holds nqueries + 1 entries from 0).
 *
 * ckm_mset_markers (markerGenes :138-155): per query and family, over the query's n genomes, ubiquity = genomes of class > 0, single =
 * genomes of class 1, duplicate = genomes of class 2, and one flag byte flag[q * nfamilies + f]:
 *   bit 0  (double)ubiquity >= ubiquity_threshold[q] && (double)single >= single_copy_threshold[q]      the family is a marker (:154)
 *   bit 1  (double)(n - ubiquity) >= ubiquity_threshold[q]                                                missingGenes (:507)
 *   bit 2  (double)duplicate >= ubiquity_threshold[q]                                                     duplicateGenes (:533)
 * The thresholds are the doubles the caller computed (ubiquityThreshold * len(genomeIds), ...).  want_counts != 0: counts[(q * nfamilies
 * + f) * 3 ..] = ubiquity, single, duplicate.  The reference's early `continue` (:141) never changes a result and is not reproduced
 * (DESIGN §21).  A genome listed twice in a query counts twice, as in the reference's loop.
 *
 * ckm_mset_colocated (colocatedGenes :163-190): a query also has a marker list qm[qm_off[q] .. qm_off[q + 1] - 1] of family indices.  For
 * every pair i < j of positions of that list, count = the query's genomes in which both families have a copy and some pair of copies has
 * |start1 - start2| < dist_threshold; the pair is reported when (double)count / (double)n > genome_threshold (:189; one IEEE division;
 * n = the genomes of the query, also those without any marker).  Reported pairs of query q are pair_off[q] .. pair_off[q + 1] - 1, in
 * ascending (i, j): i[], j[] are positions in the query's marker list, count[] the genomes.  A query without a genome or with fewer than
 * two markers reports nothing.  The pass runs in rounds of whole queries and its output in batches of whole rows, both within
 * budget_bytes (0: CKM_MSET_BATCH_MB, default 256, << 20; a round holds at least one query, a batch at least one row); neither changes
 * a result.  A call without a pair to test does not touch the device.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, an offset table that does not start at 0 or falls, a class above 2, an
 * index beyond the table, a dist_threshold that is not an integer; CKM_ERANGE for a position outside [0, 2^31), a dist_threshold outside
 * [0, 2^31), more than 2^31 - 1 positions, more than 2^24 genomes or families, more than 2^40 cells, more than 2^20 markers in a query.
 * ckm_mset_check applies the same tests (the query tables when qg_off is not NULL, the marker lists when qm_off is not NULL) and needs
 * no device: the caller then computes such a table or call with its own loop. */
typedef struct ckm_mset_table ckm_mset_table;
typedef struct ckm_mset_result ckm_mset_result;
typedef struct {
  uint64_t        nqueries, nfamilies;
  uint64_t        npairs, nbatches, nrounds;  /* reported pairs; output batches (marker pass: launches); rounds of the co-location pass */
  uint64_t        tests;                      /* (genome, pair) tests of the co-location pass: sum of n * m (m - 1) / 2 */
  const uint8_t  *flag;                       /* marker pass: [nqueries * nfamilies] */
  const uint32_t *counts;                     /* marker pass with want_counts: [nqueries * nfamilies * 3], else NULL */
  const uint64_t *pair_off;                   /* co-location pass: [nqueries + 1] */
  const uint32_t *i, *j, *count;              /* co-location pass: [npairs] */
  double          ms_upload, ms_markers, ms_pack, ms_count, ms_scan, ms_fill, ms_download, ms_total;   /* HIP events per phase; wall of the call */
} ckm_mset_columns;
int  ckm_mset_check(uint32_t ngenomes, uint32_t nfamilies, const uint8_t *count_class, const uint64_t *pos_off, const int64_t *pos, uint32_t nqueries,
                    const uint64_t *qg_off, const uint32_t *qg, const uint64_t *qm_off, const uint32_t *qm, double dist_threshold);
int  ckm_mset_table_create(ckm_ctx *ctx, uint32_t ngenomes, uint32_t nfamilies, const uint8_t *count_class, const uint64_t *pos_off, const int64_t *pos,
                           double *ms_upload, ckm_mset_table **out);
void ckm_mset_table_free(ckm_mset_table *t);
int  ckm_mset_markers(ckm_ctx *ctx, const ckm_mset_table *t, uint32_t nqueries, const uint64_t *qg_off, const uint32_t *qg, const double *ubiquity_threshold,
                      const double *single_copy_threshold, int want_counts, uint64_t budget_bytes, ckm_mset_result **out);
int  ckm_mset_colocated(ckm_ctx *ctx, const ckm_mset_table *t, uint32_t nqueries, const uint64_t *qg_off, const uint32_t *qg, const uint64_t *qm_off,
                        const uint32_t *qm, double dist_threshold, double genome_threshold, uint64_t budget_bytes, ckm_mset_result **out);
int  ckm_mset_columns_get(const ckm_mset_result *r, ckm_mset_columns *out);
void ckm_mset_result_free(ckm_mset_result *r);

/* ---- Simulation: marker sets scored on sampled genomes (additions to ABI 12) -------------------------------------------------
 * Replaces the loop nest of scripts/simulation.py's worker (:97-142): per draw of contigs MarkerSetBuilder.containedMarkerGenes
 * (scripts/genometreeworkflow/markerSetBuilder.py:353-369) and both modes of MarkerSet.genomeCheck (checkm/markerSets.py:206-238) for
 * every marker set.  checkm_amd/csrc/sim_dev.h, kernels_sim.hip.
 *
 * Keys: for the nmarkers distinct markers of all marker sets of the call, key[key_off[m] .. key_off[m + 1] - 1] are the start positions
 * p[0] of the copies of marker m in the test genome (nkeys entries in all; a marker without a copy has none).
 * Marker sets: marker set s holds the co-located sets ms_off[s] .. ms_off[s + 1] - 1; co-located set c holds the marker indices
 * cs_marker[cs_off[c] .. cs_off[c + 1] - 1] (ncs co-located sets, cs_off with ncs + 1 entries, nmembers entries of cs_marker).  A marker may
 * sit in two co-located sets of one marker set: numMarkers() counts it twice, the individual mode once, as in the reference.
 * Replicates: replicate r is the contig starts starts[rs_off[r] .. rs_off[r + 1] - 1], ascending, duplicates allowed, and contig_len[r].
 * Every offset table starts at 0 and never falls.
 *
 * A copy at p counts once for every start s with 0 <= p - s < contig_len; a marker's count is the sum over its copies.  out holds four
 * float64 per (replicate, marker set), out[(r * nsets + s) * 4 ..], in the reference's operation order:
 *   100 * float(present) / numMarkers, 100 * float(multiCopy) / numMarkers      genomeCheck(hits, bIndividualMarkers=True)
 *   100 * comp / nSets, 100 * cont / nSets                                      genomeCheck(hits, bIndividualMarkers=False)
 * One launch covers the replicates of a round; a call goes in rounds of whole replicates within budget_bytes (0: CKM_SIM_BATCH_MB,
 * default 256, << 20; a round holds at least one replicate), which never changes a result.  info may be NULL.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, an offset table that does not start at 0, falls or points beyond its table,
 * a marker index beyond the keys, starts that are not ascending within a replicate, a co-located set without a member, a marker set
 * without a co-located set (the reference divides by zero there); CKM_ERANGE for a key or a start outside [0, 2^31), a contig_len outside
 * [1, 2^31), more than 2^24 markers or replicates, more than 2^20 marker sets, copies of a marker times starts of a replicate beyond
 * 2^31 - 1.  ckm_sim_check applies the same tests and needs no device: the caller then computes such a call with its own loop. */
typedef struct {
  uint32_t        nmarkers;    const uint64_t *key_off;  const int64_t *key;        uint64_t nkeys;
  uint32_t        nsets;       const uint64_t *ms_off;   const uint64_t *cs_off;    uint64_t ncs;
  const uint32_t *cs_marker;   uint64_t        nmembers;
  uint32_t        nreplicates; const uint64_t *rs_off;   const int64_t *starts;     uint64_t nstarts;
  const int64_t  *contig_len;
} ckm_sim_args;
typedef struct {
  uint64_t nrounds;
  double   ms_pack, ms_upload, ms_kernel, ms_download, ms_total;   /* host packing; HIP events per phase; wall of the call */
} ckm_sim_info;
int  ckm_sim_check(const ckm_sim_args *a);
int  ckm_sim_run(ckm_ctx *ctx, const ckm_sim_args *a, uint64_t budget_bytes, double *out, ckm_sim_info *info);

/* ---- SimulationScaffolds: marker sets scored on genomes sampled by scaffold (additions to ABI 12) ----------------------------
 * Replaces the loop nest of the workers of scripts/simulationScaffoldsRandom.py and scripts/simulationScaffoldsByLength.py (:137-162): per
 * draw MarkerSetBuilder.markerGenesOnScaffolds (scripts/genometreeworkflow/markerSetBuilder.py:371-378) for the test genome and for the
 * contaminant, and both modes of MarkerSet.genomeCheck (checkm/markerSets.py:206-238) for every marker set.
 * checkm_amd/csrc/simscaf_dev.h, kernels_simscaf.hip.
 *
 * Resident: ngenomes genomes with nscaf[g] scaffolds each, and for the nmarkers distinct markers of all marker sets of the call the cells
 * (g, m) = g * nmarkers + m: sc[sc_off[cell] .. sc_off[cell + 1] - 1] are the scaffold indices (< nscaf[g]) of the copies of marker m in
 * genome g, one entry per copy (nsc entries in all).  The marker sets are ckm_sim_args' ms_off / cs_off / cs_marker.
 * Replicates: replicate r has the test genome test[r], the contaminant cont[r] (CKM_SIMSCAF_NONE: none; it may equal test[r]) and the words
 * bits[bit_off[r] .. bit_off[r + 1] - 1]: (nscaf[test[r]] + 31) / 32 words, bit i % 32 of word i / 32 set where scaffold i of the test genome
 * is kept, then (nscaf[cont[r]] + 31) / 32 words for the scaffolds of the contaminant that are sampled in (nwords words in all).
 * Every offset table starts at 0 and never falls.
 *
 * A marker's count is the number of its copies in the test genome on a kept scaffold plus the number of its copies in the contaminant on a
 * sampled scaffold.  out holds four float64 per (replicate, marker set), out[(r * nsets + s) * 4 ..], as ckm_sim_run's.
 * One launch covers the replicates of a round; a call goes in rounds of whole replicates within budget_bytes (0: CKM_SIMSCAF_BATCH_MB,
 * default 256, << 20; a round holds at least one replicate), which never changes a result.  info may be NULL.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, an offset table that does not start at 0, falls or points beyond its table,
 * a scaffold index >= nscaf[g], a genome index >= ngenomes, a marker index >= nmarkers, bit rows whose length is not that of the two genomes,
 * a bit set at or beyond nscaf, a co-located set without a member, a marker set without a co-located set; CKM_ERANGE for more than 2^24
 * genomes, markers or replicates, more than 2^20 marker sets, more than 2^28 cells, more than 2^30 scaffolds in a genome, more than
 * 2^31 - 1 copies, or a cell with 2^30 copies or more (a marker's copies in two genomes stay below 2^31).  ckm_simscaf_check applies the
 * same tests and needs no device: the caller then computes such a call with its own loop. */
#define CKM_SIMSCAF_NONE 0xffffffffu
typedef struct {
  uint32_t        ngenomes;    const uint32_t *nscaf;
  uint32_t        nmarkers;    const uint64_t *sc_off;   const uint32_t *sc;        uint64_t nsc;
  uint32_t        nsets;       const uint64_t *ms_off;   const uint64_t *cs_off;    uint64_t ncs;
  const uint32_t *cs_marker;   uint64_t        nmembers;
  uint32_t        nreplicates; const uint32_t *test;     const uint32_t *cont;
  const uint64_t *bit_off;     const uint32_t *bits;     uint64_t        nwords;
} ckm_simscaf_args;
typedef ckm_sim_info ckm_simscaf_info;
int  ckm_simscaf_check(const ckm_simscaf_args *a);
int  ckm_simscaf_run(ckm_ctx *ctx, const ckm_simscaf_args *a, uint64_t budget_bytes, double *out, ckm_simscaf_info *info);

/* ---- MarkerSetSelection: sampled genomes drawn and scored on the device (additions to ABI 12) ---------------------------------
 * Replaces the replicate loop of scripts/simInferBestMarkerSet.py (:94-110): per replicate two random.uniform, MarkerSetBuilder.sampleGenome
 * (scripts/genometreeworkflow/markerSetBuilder.py:265-289), containedMarkerGenes and both modes of MarkerSet.genomeCheck for every marker
 * set.  The draws come from a counter-based generator on the device.  checkm_amd/csrc/select_dev.h, kernels_select.hip.
 *
 * Genomes: ngenomes test genomes of genome_len[g] bases, C_g = genome_len[g] / contig_len contigs each.  Keys: for cell (g, m) =
 * g * nmarkers + m, key[key_off[cell] .. key_off[cell + 1] - 1] are the start positions p[0] of the copies of marker m in genome g (nkeys
 * entries in all).  The marker sets are ckm_sim_args' ms_off / cs_off / cs_marker.  Every offset table starts at 0 and never falls.
 *
 * Draw (g, r), r < nreplicates, from Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter (index, r, g, stream):
 * stream 0 gives the two fractions (u = 53 bits of two words * 2^-53; lo + (hi - lo) * u), nComp = (int)(C * testComp + 0.5), nCont
 * likewise, trueComp = (double)nComp * contig_len * 100 / genome_len; stream 1 gives contig i the word w_i, and the nComp contigs with the
 * smallest pairs (w_i, i) are taken once each; stream 2 gives contamination draw j the contig ((uint64)w_j * C) >> 32.  A copy at p counts
 * the multiplicity of contig p / contig_len where that is below C, else 0; a marker's count is the sum over its copies.
 *
 * out->truth holds trueComp and trueCont per draw, truth[(g * nreplicates + r) * 2 ..]; out->out four float64 per (draw, marker set),
 * out[((g * nreplicates + r) * nsets + s) * 4 ..], as ckm_sim_run's; out->rows, where not NULL, min(multiplicity, 65535) of every contig,
 * genome g's rows [nreplicates][C_g] behind those of the genomes before it.  One launch covers the draws of a round; a call goes in rounds
 * of whole draws within budget_bytes (0: CKM_SELECT_BATCH_MB, default 256, << 20; a round holds at least one draw), which never changes
 * a result.  info may be NULL.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, an offset table that does not start at 0, falls or points beyond its table, a
 * marker index beyond the markers, a co-located set without a member, a marker set without a co-located set; CKM_ERANGE for a key outside
 * [0, 2^31), a contig_len outside [1, 2^31), a genome with no contig (C = 0) or with more than 16384, a completeness range outside [0, 1]
 * or a contamination range outside [0, 8] (not finite, or lo > hi), more than 65535 contamination draws, copies of a marker times
 * (contamination draws + 1) beyond 2^32 - 1, more than 2^24 genomes, markers or replicates, more than 2^31 - 1 draws or cells, more than
 * 2^20 marker sets.  ckm_select_check applies the same tests and needs no device: the caller then computes such a call with its own loop. */
typedef struct {
  uint32_t        ngenomes;    const int64_t  *genome_len;
  uint32_t        nmarkers;    const uint64_t *key_off;  const int64_t *key;        uint64_t nkeys;
  uint32_t        nsets;       const uint64_t *ms_off;   const uint64_t *cs_off;    uint64_t ncs;
  const uint32_t *cs_marker;   uint64_t        nmembers;
  uint32_t        nreplicates; int64_t         contig_len;
  double          comp_lo, comp_hi, cont_lo, cont_hi;
  uint64_t        seed;
} ckm_select_args;
typedef struct { double *truth; double *out; uint16_t *rows; } ckm_select_out;
typedef ckm_sim_info ckm_select_info;
int  ckm_select_check(const ckm_select_args *a);
int  ckm_select_run(ckm_ctx *ctx, const ckm_select_args *a, uint64_t budget_bytes, const ckm_select_out *out, ckm_select_info *info);

/* ---- PplacerRunner: bins placed on the edges of the reference tree (additions to ABI 12) -------------------------------------
 * Replaces the pplacer call of checkm/pplacer.py:70-80 by a grid search on the device.  checkm_amd/csrc/place_dev.h, kernels_place.hip.
 *
 * Tree: nnodes nodes; node v has the children child[child_off[v] .. child_off[v + 1] - 1] (nchild entries in all), none (a leaf) or at
 * least two; the root, the one node nobody lists, has two or three.  length[v] is the length of the edge above v (the root's is not
 * read).  Edge numbers are node numbers.  Alignment: one row per leaf in ascending node order, rows[row_off[k] .. row_off[k + 1] - 1],
 * nsites characters each; queries likewise.  The 20 letters ARNDCQEGHILKMFPSTWYV are states, every other byte is "unknown".
 * Model: P(t)[i][j] = max(0, sum_k U[i][k] e_k Uinv[k][j]) with the caller's tables of e_k = exp(lambda_k * rate * t), 20 per entry:
 * exp_len[nnodes][nrates] (t = length), exp_half (length / 2), exp_dist[nnodes][nfrac][2][nrates] (f * length, (1 - f) * length),
 * exp_pend[1 + npend][nrates] (startPend, then the pendant grid); weights[nrates], pi[20].  No exp and no log runs in the library.
 *
 * Per query the max_pitches best edges of the scan (midpoint, startPend), larger first, ties to the lower edge number, each refined
 * over the grid (ties to the lower distal index, then the lower pendant index).  Outputs hold nqueries * max_pitches entries; entries
 * beyond the number of edges have top_edge -1.  A likelihood is m * 2^e with m in [0.5, 1) (or m = 0).  The sites go in chunks of a
 * multiple of 64 within budget_bytes (0: CKM_PLACE_BATCH_MB, default 2048, << 20; never fewer than 64 sites), which never changes a
 * result.  info may be NULL.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, offsets that do not start at 0, fall or point beyond their table, a child
 * listed twice, a node with one child, a root without two or three children, a cycle, a negative or non-finite length or table entry,
 * an alignment row or query whose length is not nsites, an empty grid; CKM_ERANGE for more than 8 rates, more than 32 grid values,
 * more than 2^22 nodes, sites or queries, max_pitches above 4096.  ckm_place_check applies the same tests and needs no device. */
typedef struct {
  uint32_t nnodes;    const uint64_t *child_off;  const uint32_t *child;   uint64_t nchild;       const double *length;
  uint32_t nsites;    uint32_t nrows;             const uint64_t *row_off; const uint8_t *rows;   uint64_t nrow_bytes;
  uint32_t nqueries;  const uint64_t *q_off;      const uint8_t *queries;  uint64_t nquery_bytes;
  uint32_t nrates;    const double *weights;      const double *U;         const double *Uinv;    const double *pi;
  const double *exp_len;  const double *exp_half;
  uint32_t nfrac;     const double *exp_dist;
  uint32_t npend;     const double *exp_pend;
  uint32_t max_pitches;
} ckm_place_args;
typedef struct {
  int32_t *top_edge;  double *scan_m;  int64_t *scan_e;  double *ref_m;  int64_t *ref_e;  int32_t *ref_f;  int32_t *ref_g;
} ckm_place_out;
typedef struct {
  uint64_t nchunks, chunk_sites, nlevels_up, nlevels_down;
  double   ms_pack, ms_upload, ms_matrices, ms_sweeps, ms_tables, ms_scan, ms_topk, ms_refine, ms_download, ms_total;
} ckm_place_info;
int  ckm_place_check(const ckm_place_args *a);
int  ckm_place_run(ckm_ctx *ctx, const ckm_place_args *a, uint64_t budget_bytes, const ckm_place_out *out, ckm_place_info *info);

/* ---- SSU_Finder: nucleotide models scanned over both strands of every contig (additions to ABI 12) --------------------------
 * Replaces the three nhmmer calls of checkm/ssuFinder.py:49-61 by a Viterbi scan of our own definition (checkm_amd/csrc/nhmm_dev.h states
 * it: int32 milli-bit scores, cells (score, start), unihit local, tiles of `stride` rows that start `overlap` rows early), on the device
 * in kernels_nhmm.hip.
 *
 * Model m has M[m] <= 2048 nodes; its tables start at node tab_off[m] of the call (tab_off[nmodels] == ntab): emis + 4 tab_off[m] is
 * [4][M] (A C G T/U), trans + 7 tab_off[m] is [7][M] in the order MM IM DM MI II MD DD, node k at index k - 1, the transitions into k
 * holding node k - 1's numbers of the file.  strands: 1 forward, 2 reverse complement, 3 both.  Every row i of a strand whose best cell
 * scores at least min_score[m] is reported, in (model, sequence, strand, row) order: row_pos = i and row_start in strand coordinates
 * (1-based).  Hits (nhmm_dev.h: groups by start, greedy by score) carry forward-strand coordinates hit_from <= hit_to.
 * budget_bytes (0: CKM_SSU_BATCH_MB, default 256, << 20) bounds the row buffer of a launch, 8 bytes per owned row, and changes no result.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, a model without nodes, a tab_off that does not step by M, strands outside
 * 1..3, a stride of 0, a sequence with a byte beyond ASCII (the message names it); CKM_ERANGE for M > 2048, a min_score below -2^20,
 * an emission outside [-2^21, 2048], a transition outside [-2^21, 0], stride + overlap above 2^17, a sequence of 2^31 - 1 bytes or more.
 * ckm_nhmm_check applies the tests of the arguments and needs no device. */
typedef struct {
  uint32_t nmodels;   const uint32_t *M;      const uint64_t *tab_off;   const int32_t *emis;   const int32_t *trans;   uint64_t ntab;
  const int32_t *min_score;
  uint32_t stride, overlap, strands;
} ckm_nhmm_args;
typedef struct ckm_nhmm_result ckm_nhmm_result;
typedef struct {
  uint64_t nrows;   const uint32_t *row_model, *row_seq, *row_strand, *row_pos, *row_start;   const int32_t *row_score;
  uint64_t nhits;   const uint32_t *hit_model, *hit_seq, *hit_strand, *hit_from, *hit_to;     const int32_t *hit_score;
} ckm_nhmm_columns;
typedef struct {
  uint64_t tiles, launches, cells, batches;
  double   ms_tables, ms_upload, ms_scan, ms_compact, ms_download, ms_hits, ms_total;
} ckm_nhmm_info;
int  ckm_nhmm_check(const ckm_nhmm_args *a);
int  ckm_nhmm_run(ckm_ctx *ctx, const ckm_nhmm_args *a, const ckm_nucseq *seqs, uint64_t budget_bytes, ckm_nhmm_result **out, ckm_nhmm_info *info);
int  ckm_nhmm_columns_get(const ckm_nhmm_result *r, ckm_nhmm_columns *out);
void ckm_nhmm_free(ckm_nhmm_result *r);

/* ---- GenomeTree: pair counts, corrected distances and neighbour joining (additions to ABI 12) --------------------------------
 * Replaces the FastTree calls of scripts/genometreeworkflow/inferGenomeTree.py and bootstrapTree.py by distances and neighbour joining
 * of our own definition (checkm_amd/csrc/gtree_dev.h states it), on the device in kernels_gtree.hip.
 *
 * Alignment: nrows rows of ncols bytes, row i at text + i * ncols (ntext_bytes = nrows * ncols).  The twenty letters
 * ARNDCQEGHILKMFPSTWYV in either case are residues, every other byte is "unknown".  Trees of a call: the alignment itself when base is 1,
 * then one per replicate r, whose column c is column cols[r * ncols + c] of the alignment.  With matrix set the text is not read and
 * tree t is joined from the nrows x nrows doubles at matrix + t * nrows * nrows (the upper triangle and the lower must agree).
 * model: 0 Kimura (-ln(1 - p - 0.2 p^2)), 1 Poisson (-ln(1 - p)), 2 p; a pair with nothing compared, a non-positive argument of the
 * logarithm or a value above max_dist takes max_dist.
 * Outputs, each may be NULL: compared, differ [nrows][nrows] uint32 and dist [nrows][nrows] of the alignment itself; merge_ij
 * [trees][nrows - 1][2] (the two slots of a join: a slot names the node last put there, slot i first being row i; the new node takes the
 * first slot) and merge_len [trees][nrows - 1][2] (the lengths of the edges above the two).  The last row is the root.
 * budget_bytes (0: CKM_GTREE_BATCH_MB, default 2048, << 20) bounds the trees resident at once (never fewer than one) and changes no
 * result.  info may be NULL.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, fewer than 2 rows, no column, an ntext_bytes that is not rows x columns, a
 * drawn column beyond the alignment, an unknown model, a max_dist that is not positive and finite, a distance that is not finite;
 * CKM_ERANGE for more than 2^14 rows, more than 2^20 columns, more than 2^15 - 1 replicates or 2^15 matrices, a byte beyond ASCII.
 * ckm_gtree_check applies the same tests and needs no device.  ckm_gtree_host is the host executor of gtree_dev.h behind the same
 * arguments: the same bits as ckm_gtree_run, no device, for checks and comparisons (the times of its info stay 0). */
typedef struct {
  uint32_t nrows, ncols;   const uint8_t *text;   uint64_t ntext_bytes;
  uint32_t nreps;          const uint32_t *cols;  uint32_t base;   int32_t model;   double max_dist;
  const double *matrix;    uint32_t nmatrices;
} ckm_gtree_args;
typedef struct { uint32_t *compared, *differ;   double *dist;   uint32_t *merge_ij;   double *merge_len; } ckm_gtree_out;
typedef struct {
  uint64_t nrounds, ntrees, launches;
  double   ms_upload, ms_gather, ms_counts, ms_dist, ms_joins, ms_download, ms_total;
} ckm_gtree_info;
int  ckm_gtree_check(const ckm_gtree_args *a);
int  ckm_gtree_host(const ckm_gtree_args *a, uint64_t budget_bytes, const ckm_gtree_out *out, ckm_gtree_info *info);
int  ckm_gtree_run(ckm_ctx *ctx, const ckm_gtree_args *a, uint64_t budget_bytes, const ckm_gtree_out *out, ckm_gtree_info *info);

/* ---- GeneTrees: the paralog and consistency tests of a forest of gene trees (additions to ABI 12) ---------------------------
 * Replaces the dendropy walks of scripts/genometreeworkflow/paralogTest.py and consistencyTest.py by integer problems over leaf ranges
 * (checkm_amd/csrc/genetree_dev.h states layout and arithmetic), on the device in kernels_genetree.hip.
 *
 * Forest: ntrees trees; the leaves of a tree are numbered in the order they are written.  Tree t has the nodes node_off[t] ..
 * node_off[t+1] in pre-order as written (node 0 the root): first, last (its subtree is the leaf range [first, last) of the tree), parent
 * (a node of the tree, 0xffffffff for the root), length (float64, the root's 0 when absent), internal (1: it has children); the leaves
 * leaf_off[t] .. leaf_off[t+1]: leaf_genome and leaf_species (dense per tree; species 0xffffffff: not counted) and leaf_class, rank-major
 * over all leaves of the call (leaf_class[r * nleaves + leaf]; r = 0 domain, 1 phylum, 2 class), dense per tree and rank; the classes
 * class_off[3t+r] .. class_off[3t+r+1] of rank r with class_total, the class's leaves in the tree; the groups group_off[t] ..
 * group_off[t+1], one per genome with several leaves, group g holding the leaf pairs gpair_off[g] .. gpair_off[g+1] (pair_a < pair_b,
 * positions in the tree).
 *
 * Outputs: consistency [classes] float64, the maximum over the internal nodes of k / (T + (n - k)) and (T - k) / (T + ((N - n) - (T - k)))
 * (one IEEE division each, start value 0); pair_flag [pairs], 1 when the patristic distance of the pair is > 0 (summed up the first side
 * to the common ancestor, the second side added onto it; two root distances, each summed from the leaf up, when the ancestor is the
 * root); group_node [groups], the node of the smallest subtree over every flagged leaf of the group (0xffffffff: no flagged pair), and
 * group_mixed [groups], 1 when the counted species in that subtree take more than one value.  Trees are processed in rounds of at most
 * budget_bytes (0: CKM_GENETREE_BATCH_MB, default 256) of resident arrays; no result depends on the budget.
 *
 * Refused, nothing computed: CKM_ERANGE for more than 2^14 leaves or 2^15 nodes in a tree, more than 65535 classes at a rank, more than
 * 2^20 trees; CKM_EINVAL for a NULL argument, offsets that descend, an empty tree, a length that is not finite, a leaf range outside the
 * tree, a parent that does not precede its child, children that do not tile their parent's range, a class index beyond the class count,
 * a class total that is not the count of its leaves, a pair that names a leaf beyond the tree, is not ascending or joins two genomes.
 * ckm_genetree_check applies the same tests and needs no device.  ckm_genetree_host is the host executor of genetree_dev.h behind the
 * same arguments: the same bits as ckm_genetree_run, no device (the times of its info stay 0). */
typedef struct {
  uint32_t ntrees;
  const uint32_t *node_off, *leaf_off, *class_off, *group_off, *gpair_off;
  const uint32_t *first, *last, *parent;   const double *length;   const uint8_t *internal;
  const uint32_t *leaf_genome, *leaf_species, *leaf_class;
  const uint32_t *class_total;
  const uint32_t *pair_a, *pair_b;
} ckm_genetree_args;
typedef struct { double *consistency;   uint8_t *pair_flag;   uint32_t *group_node;   uint8_t *group_mixed; } ckm_genetree_out;
typedef struct {
  uint64_t nrounds, ntrees, launches;
  double   ms_upload, ms_consistency, ms_flags, ms_conspecific, ms_download, ms_total;
} ckm_genetree_info;
int  ckm_genetree_check(const ckm_genetree_args *a);
int  ckm_genetree_host(const ckm_genetree_args *a, uint64_t budget_bytes, const ckm_genetree_out *out, ckm_genetree_info *info);
int  ckm_genetree_run(ckm_ctx *ctx, const ckm_genetree_args *a, uint64_t budget_bytes, const ckm_genetree_out *out, ckm_genetree_info *info);

/* ---- ReducedTree: which pairs of rows of an alignment are nearly identical (additions to ABI 12) ----------------------------
 * Replaces the all-pairs Python loop of scripts/genometreeworkflow/createSmallTree.py (__nearlyIdentical) by one pass over the upper
 * triangle (checkm_amd/csrc/nearid_dev.h states layout and arithmetic), on the device in kernels_nearid.hip.
 *
 * Text: n_rows rows of row_len raw bytes, row i at text + i * row_stride; row_stride >= row_len and a multiple of 16.  The bytes between
 * row_len and row_stride are never compared.  Every byte value counts as itself, gaps and 0x80 .. 0xFF included.  A pair (i, j > i) is
 * near iff the number of columns at which the two rows differ is below limit[i] (>= 1; the caller computes it with the reference's own
 * float expression, the library sees integers only).
 * Output: near [n_rows][ceil(n_rows / 64)] uint64, bit (j & 63) of word j / 64 of row i set iff j > i and the pair is near; every word
 * is written.  The text and the limits stay resident; the row tiles (64 rows) are cut into bands whose bit rows fit what budget_bytes
 * (0: CKM_NEARID_BATCH_MB, default 256, << 20) leaves beside them, never fewer than one row tile; no result depends on the budget.
 *
 * Refused, nothing computed: CKM_EINVAL for a NULL argument, n_rows == 0, row_len == 0, a limit of 0, a row_stride below row_len or not
 * a multiple of 16; CKM_ERANGE for more than 2^17 rows (the bit matrix stays at or below 2 GiB), a row_stride above 2^24, more than
 * 2^34 bytes of text (n_rows * row_stride).  ckm_nearid_check applies the same tests and needs no device.  ckm_nearid_host is the host
 * executor of nearid_dev.h behind the same arguments: the same bits as ckm_nearid_run, no device (the times of its info stay 0). */
typedef struct { const uint8_t *text; uint32_t n_rows, row_len, row_stride;   /* rows padded to a multiple of 16 */
                 const uint32_t *limit; } ckm_nearid_args;                   /* per row i: pairs (i, j > i) are near iff diffs < limit[i] */
typedef struct { uint64_t *near; } ckm_nearid_out;                            /* [n_rows][ceil(n_rows/64)] bit j of row i, only j > i set */
typedef struct {
  uint64_t nbands, npairs, launches, blocks;
  double   ms_upload, ms_kernel, ms_download, ms_total;
} ckm_nearid_info;
int  ckm_nearid_check(const ckm_nearid_args *a);
int  ckm_nearid_host(const ckm_nearid_args *a, uint64_t budget_bytes, const ckm_nearid_out *out, ckm_nearid_info *info);
int  ckm_nearid_run(ckm_ctx *ctx, const ckm_nearid_args *a, uint64_t budget_bytes, const ckm_nearid_out *out, ckm_nearid_info *info);

/* ---- diagnostics used by the parity tests: every stage of one (model, sequence) pair, no filtering */
typedef struct {
  int32_t msv_xJ;  float msv_sc, null_sc, bias_sc;
  int32_t vit_xC;  float vit_sc, fwd_sc, fwd_xC;  int32_t fwd_nscale;
  int32_t ssv_maxv;
  int32_t msvp_xJ; float msvp_sc;      /* the packed exact-MSV kernel the search uses (must equal msv_xJ / msv_sc) */
} ckm_stage_scores;
int ckm_debug_stages(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s,
                     const uint32_t *model, const uint32_t *seq, uint32_t npairs, ckm_stage_scores *out);
/* The SSV kernel as the search launches it (ABI 11): ONE model against seq[n] in the caller's order, cut into blocks of per_block sequences
 * (0: what the search uses for the model's launch class) whose tables are built as the search builds them.  lanes = 0: the launch class
 * the search picks; 8 or 16: that mapping's instance where the model has its image, else CKM_ERANGE.  Two launches: one stores Smax per
 * pair (smax[n], 0..256), one runs the fused finish of the MSV stage with tables sized for every pair: route[n] = 0 dropped, 1 survivor
 * (usc[n] = its score in nats, +inf on byte overflow), 2 handed to the exact MSV kernel.  info[4] (may be NULL) = launch class, threads per
 * block, sequences per block, blocks.  CKM_EINVAL: an empty sequence or one listed twice.  CKM_EHIP with a message naming the list
 * entry: the device reported a pair twice (or in both tables), a pair that was not listed, or no Smax for a pair. */
int ckm_debug_ssv(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s, uint32_t model, const uint32_t *seq, uint32_t n,
                  uint32_t per_block, int32_t lanes, uint16_t *smax, uint8_t *route, float *usc, int32_t *info);
/* The filter stages between MSV and Forward as the device-driven search runs them (ABI 12): the bias filter with its F1/F2 decisions, the
 * FAST Viterbi kernels (16 lanes per pair, four pairs per wavefront, for models of up to 512 nodes; a wavefront per pair beyond, and for
 * every model in the host-driven search) and the exact kernel with their F2 decisions, on n pairs (model[i], seq[i]) in the caller's
 * order; no sequence may be empty.  nblocks: workgroups of the FAST launches (0: what the search uses).
 *   CKM_FILTERS_VIT16            every pair's model must share ONE 16-lane class; candidate i = pair i with usc[i], filtersc[i]; the FAST queue
 *                                is the caller's order; then the exact kernel on whatever the FAST kernel queued for it
 *   CKM_FILTERS_WAVE_FAST        the same with the wave-per-pair FAST kernel (any model)
 *   CKM_FILTERS_WAVE_FAST_PLAIN  the wave-per-pair FAST kernel without decisions: vit_fast, vit_xC (32767 on overflow), vit_flag only
 *   CKM_FILTERS_CHAIN            the bias filter over the candidates (usc[i]; filtersc is ignored and may be NULL), then every Viterbi launch of the search
 * Per pair: bias_d, bias_e (CHAIN: the bias filter's d0 + d1 and power-of-two exponent), filtersc (CHAIN: the approximate null score the
 * device stored; else the caller's), route (0xff dead, 0 Viterbi skipped, 1 FAST kernel only, 2 exact kernel, | 0x10 exact kernel because the
 * NEED for the filter was within the margin), vit_fast / vit_exact (all bits set: not written), vit_flag, vit_xC (INT32_MAX where the mode
 * has none), and how often the pair appears in the FAST queues, the exact queues and as a Forward item.  *status = the cascade's status word.
 * CKM_EHIP with a message naming the pair: a queued pair that was not written, a pair reported twice, an entry that is no pair of the call. */
enum { CKM_FILTERS_VIT16 = 0, CKM_FILTERS_WAVE_FAST = 1, CKM_FILTERS_WAVE_FAST_PLAIN = 2, CKM_FILTERS_CHAIN = 3 };
typedef struct {
  float    bias_d, bias_e, filtersc;
  float    vit_fast, vit_exact;
  int32_t  vit_xC;
  uint32_t vit_flag, route;
  uint32_t n_vq, n_vxq, n_fwork;
} ckm_filter_result;
int ckm_debug_filters(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s, const uint32_t *model, const uint32_t *seq,
                      const float *usc, const float *filtersc, uint32_t n, int32_t mode, uint32_t nblocks,
                      ckm_filter_result *out, uint32_t *status);
typedef struct {
  float envsc, oasc, fwd_xC; int32_t nscale; float null2[20];
  int32_t hmm_from, hmm_to, ali_from, ali_to; int32_t ok;
} ckm_envelope_result;
int ckm_debug_envelopes(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s,
                        const uint32_t *model, const uint32_t *seq, const int32_t *ienv, const int32_t *jenv,
                        uint32_t n, ckm_envelope_result *out);
/* The same envelopes with their optimal-accuracy paths, as ckm_hits_write_alignments computes them: ok[n]; node_residue[out_off[i] ..
 * out_off[i + 1]) = int32[M], the envelope-local residue (1-based) emitted by every match node of item i, 0 = none; pp[pp_off[i] ..
 * pp_off[i + 1]) = float[Ld + 1], the posterior probability of every residue on the path in the state that emits it, 0 off the path.
 * Both stay zero where ok == 0.  Additive: CKM_ABI_VERSION stays 12. */
int ckm_debug_envelope_paths(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s,
                             const uint32_t *model, const uint32_t *seq, const int32_t *ienv, const int32_t *jenv,
                             uint32_t n, int32_t *ok, const uint64_t *out_off, int32_t *node_residue,
                             const uint64_t *pp_off, float *pp);

/* The trace ensemble of one multi-domain region ireg..jreg (1-based, inclusive) of sequence `seq`:
 * n2sum[jreg-ireg+1] = per residue, sum over the 200 traces of the null2 odds ratio; segs[200*cap*4] / nseg[200] = every
 * trace's sampled segments {sqfrom, sqto, hmmfrom, hmmto} in region-local coordinates, first domain first;
 * env[envcap*4] / *nenv = the clustered envelopes, sorted by start. */
int ckm_debug_region(ckm_ctx *ctx, const ckm_profiles *p, const ckm_seqs *s, uint32_t model, uint32_t seq,
                     int32_t ireg, int32_t jreg, float *n2sum, int32_t *segs, int32_t *nseg, int32_t cap,
                     int32_t *env, int32_t envcap, int32_t *nenv);

#ifdef __cplusplus
}
#endif
#endif
