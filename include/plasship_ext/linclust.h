/* plasship extension library: linclust's ungapped alignment step (libplasship_linclust.so)
 *
 * The functions below are exported by plass_amd/libplasship_linclust.so, which is linked against libplasship.so and libplasship_clust.so and
 * works on their contexts and handles (include/plasship.h, include/plasship_ext/clust.h): link all three, or dlopen this one after the
 * other two.  The exported sets of the other two libraries stay what their headers declare.  Conventions as there: 0 on success, a
 * negative code on failure, plasship_last_error() gives the message.
 */
#ifndef PLASSHIP_EXT_LINCLUST_H
#define PLASSHIP_EXT_LINCLUST_H
#include "clust.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- rescorediagonal --rescore-mode 2  (the best-scoring ungapped local segment on the candidate's diagonal: linclust's alignment step
 *      with --alignment-mode 4, mm/workflow/Linclust.cpp:86-129; doRescorediagonal for RESCORE_MODE_ALIGNMENT, mm/alignment/rescorediagonal.cpp:
 *      193-334 with DistanceCalculator::computeUngappedAlignment and computeSubstitutionStartEndDistance, DistanceCalculator.h:93-201).
 *      One DB is query and target.  `c` is any candidate list made on it (plasship_kmermatch, plasship_rescore_hamming, plasship_cands_filter,
 *      plasship_cands_read), with strands (prefScore < 0 scores the reverse complement of the query) or without.  Every +-65536 wrap of the
 *      16-bit diagonal is tried, a strictly greater score replaces the best; a pair on which nothing scores above 0 keeps score 0 and
 *      start = end = -1.  The result is an alignment list (dbtype 5, plasship_alns_write / plasship_alns_download / plasship_clust_greedy_alns):
 *      the pairs that pass canBeCovered and then coverage, --min-seq-id, --min-aln-len and -e, every identity pair, and — with --filter-hits —
 *      every pair whose score per diagonal column reaches score_per_col_thr, in the order of `c`.
 *      score_per_col_thr: the reference reads this threshold from a table in its binary (parsePrecisionLib) by --min-seq-id and -c; the table
 *      is not part of this library, the caller passes the value.  NaN: --filter-hits 0.  0: the reference's "no row found" case.
 *      A context with a communicator of more than one rank: PLASSHIP_ERR_UNSUPPORTED.
 *      stats: n_scored = pairs in `c`, n_accepted = records kept, overlap_residues = residues scored (overlap length x wraps tried). ---- */
typedef struct plasship_local_params {
    double  eval_thr;          /* -e                                      */
    float   seq_id_thr;        /* --min-seq-id                            */
    int32_t seq_id_mode;       /* --seq-id-mode                           */
    float   cov_thr;           /* -c                                      */
    int32_t cov_mode;          /* --cov-mode                              */
    int32_t min_aln_len;       /* --min-aln-len                           */
    int32_t add_backtrace;     /* -a: "<alnLen>M" as the eleventh column  */
    float   score_per_col_thr; /* --filter-hits 1: the threshold; NaN: off */
} plasship_local_params;
int plasship_rescore_local(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_local_params *par,
                           plasship_alns **out, plasship_rescore_stats *stats);
/* The same on the subset DB of cl's representatives without making that DB (linclust.sh:58-76 runs the alignment on input_step_redundancy):
 * `c` is plasship_cands_filter's list, `db` the whole DB, and the E-value's database size is the residue count of the representatives. */
int plasship_rescore_local_subset(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, const plasship_clusters *cl,
                                  const plasship_local_params *par, plasship_alns **out, plasship_rescore_stats *stats);

/* ---- mergeclusters with two clusterings  (mm/util/mergeclusters.cpp:28-145; the last call of linclust.sh, line 87).  `first` and `second`
 *      are clusterings of `db`; the second says how the first one's representatives are clustered again (what it says about other
 *      sequences is not read).  plasship_clust_greedy_alns on plasship_rescore_local_subset's list gives such a `second`; one made on a
 *      subset DB on disk comes in through plasship_clusters_read, which maps BY KEY (a sequence the DB does not list is its own cluster).
 *      The merged DB (dbtype 6): one entry per second-step representative R that is a first-step one — R's first-step list (own key first,
 *      the others ascending, as plasship_clusters_write lays it out), then the list of each other member of R in the second step, in that
 *      order; a sequence without a list gets NO entry (the reference's writer loop skips it).  The places are computed and the text is laid
 *      out on the device.  plasship_merged_download: db.n pairs (representative key, member key) in the merged DB's order.
 *      A context with a communicator of more than one rank: PLASSHIP_ERR_UNSUPPORTED. ---- */
typedef struct plasship_merged plasship_merged;
int plasship_clusters_merge(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_clusters *first, const plasship_clusters *second, plasship_merged **out);
int plasship_merged_count(const plasship_merged *m, uint64_t *n_members, uint64_t *n_clusters);
int plasship_merged_download(plasship_ctx *ctx, const plasship_merged *m, const plasship_seqdb *db, uint32_t *rep_key, uint32_t *member_key);
int plasship_merged_write(plasship_ctx *ctx, const plasship_merged *m, const plasship_seqdb *db, const char *db_path);
void plasship_merged_free(plasship_ctx *ctx, plasship_merged *m);
int plasship_clusters_read(plasship_ctx *ctx, const plasship_seqdb *db, const char *db_path, plasship_clusters **out);

#ifdef __cplusplus
}
#endif
#endif /* PLASSHIP_EXT_LINCLUST_H */
