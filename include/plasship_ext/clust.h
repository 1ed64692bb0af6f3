/* plasship extension library: linclust's greedy clustering and pre-cluster subset (libplasship_clust.so)
 *
 * The functions below are exported by plass_amd/libplasship_clust.so, which is linked against libplasship.so and works on its contexts and
 * handles (include/plasship.h): link both, or dlopen this one after libplasship.so.  libplasship.so's own set of exported functions is
 * what include/plasship.h, plasship_synth.h and plasship_rccl.h declare and stays as it is.  Conventions as there: 0 on success, a
 * negative code on failure, plasship_last_error() gives the message.
 */
#ifndef PLASSHIP_EXT_CLUST_H
#define PLASSHIP_EXT_CLUST_H
#include "../plasship.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct plasship_clusters plasship_clusters; /* clustering result (representative, member) in HBM */
#define PLASSHIP_DBTYPE_CLUSTER_RES 6               /* mm/commons/Parameters.h:65-84 */

/* ---- clust --cluster-mode 2 | 3  (greedy incremental clustering; replaces int clust(int, const char**, const Command&) for these modes:
 *      Clustering::run, mm/clustering/Clustering.cpp:32-114, with ClusteringAlgorithms::greedyIncrementalLowMem, ClusteringAlgorithms.cpp:271-332;
 *      the `clust` calls of mm/data/workflow/linclust.sh:35,82, which `penguin guided_nuclassemble` ends with).  Sequences are ranked by
 *      length descending, ties by key ascending (DBReader SORT_BY_LENGTH); every query lowers the assignment of itself and of every target it
 *      lists to its own rank, then a sequence that is named as a representative without being its own is made one.  The edges are the lines
 *      of a candidate list (plasship_kmermatch, plasship_rescore_hamming, plasship_cands_read: prefilter DBs, dbtype 7 and 14) or the accepted
 *      records of an alignment list (plasship_rescore, plasship_aln2nucl, plasship_alns_read: dbtype 5; identity pairs left as stubs are not
 *      scored for this); scores are not read.  The list must have been made on `db` and hold db's number of queries: PLASSHIP_ERR_ARG otherwise
 *      (the reference exits there too).  A context with a communicator of more than one rank: PLASSHIP_ERR_UNSUPPORTED.  Ids are 32-bit.
 *      Connected component (--cluster-mode 1) is in libplasship_cc.so (cc.h).  Set cover (--cluster-mode 0) stays with the reference: setCover is a
 *      bucket-queue greedy whose ties follow the history of swaps in decreaseClustersize, which no parallel form reproduces byte for byte.
 *      plasship_clusters_download: db.n pairs (representative key, member key), sorted by representative key, then member key.
 *      plasship_clusters_write: the DB Clustering::writeData writes (dbtype 6): one entry per representative under its key — its own key, then
 *      the other members' keys ascending, one per line — in one data file in key order; the text is laid out on the device. ---- */
typedef struct plasship_clust_stats {
    uint64_t n_sequences, n_edges;   /* edges: lines / record slots walked                                               */
    uint64_t n_clusters;
    uint64_t n_promoted;             /* sequences the correction pass made representatives                               */
    uint64_t n_long_queries;         /* queries whose list went to the workgroup kernel (more than 1024 lines)           */
    float ms_kernel;                 /* rank sort .. pair sort (HIP events on the context stream)                        */
} plasship_clust_stats;
int plasship_clust_greedy_cands(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, plasship_clusters **out, plasship_clust_stats *stats);
int plasship_clust_greedy_alns(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_alns *a, plasship_clusters **out, plasship_clust_stats *stats);
int plasship_clusters_count(const plasship_clusters *cl, uint64_t *n_members, uint64_t *n_clusters);
int plasship_clusters_download(plasship_ctx *ctx, const plasship_clusters *cl, const plasship_seqdb *db, uint32_t *rep_key, uint32_t *member_key);
int plasship_clusters_write(plasship_ctx *ctx, const plasship_clusters *cl, const plasship_seqdb *db, const char *db_path);
void plasship_clusters_free(plasship_ctx *ctx, plasship_clusters *cl);
/* What linclust.sh:39-56 leaves of `pref` (createsubdb --subdb-mode 1 with pre_clust's keys, then filterdb --filter-file with the same keys,
 * mm/util/filterdb.cpp:389-410: a positive filter on column 1): the entries whose query is a representative and, inside them, the lines whose
 * target is one, order, prefScore and diagonal unchanged.  plasship_cands_write writes the result with the representatives' entries only. */
int plasship_cands_filter(plasship_ctx *ctx, const plasship_cands *c, const plasship_clusters *cl, plasship_cands **out);

#ifdef __cplusplus
}
#endif
#endif /* PLASSHIP_EXT_CLUST_H */
