/* plasship extension library: linclust's connected-component clustering (libplasship_cc.so)
 *
 * The functions below are exported by plass_amd/libplasship_cc.so, which is linked against libplasship.so and libplasship_clust.so and works
 * on their contexts and handles (include/plasship.h, include/plasship_ext/clust.h): link all three, or dlopen this one after the other two.
 * The exported sets of the other libraries stay what their headers declare.  Conventions as there: 0 on success, a negative code on
 * failure, plasship_last_error() gives the message.
 */
#ifndef PLASSHIP_EXT_CC_H
#define PLASSHIP_EXT_CC_H
#include "clust.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- clust --cluster-mode 1  (connected component, "single linkage"; replaces int clust(int, const char**, const Command&) for this mode:
 *      Clustering::run, mm/clustering/Clustering.cpp:32-114, with ClusteringAlgorithms::execute(3), ClusteringAlgorithms.cpp:81-111, on the lists
 *      readInClusterData symmetrises, ClusteringAlgorithms.cpp:334-401 with AlignmentSymmetry.cpp:123-215).  The reference walks the sequences
 *      by (symmetric list size descending, id descending — ids of the sequence DB opened SORT_BY_LENGTH, Clustering.cpp:19: the longest sequence
 *      has id 0, ties by key ascending) and runs from every unassigned one a breadth-first search that expands nodes up to depth
 *      max_iterations and assigns their neighbours.  Wherever no node lies deeper than max_iterations + 1 below the first sequence of its
 *      component in that order, the result is the connected components of the list, each represented by that first sequence; that is what
 *      these functions compute.  Where a node would be reached at depth max_iterations + 2, the reference's answer depends on its visiting
 *      order: PLASSHIP_ERR_UNSUPPORTED, nothing is returned.
 *      The symmetric list size of a sequence: its lines (a line listed twice counts twice; an entry without lines counts 1, as the list of
 *      the sequence itself), plus one for every line of another sequence that names it and that it does not answer.
 *      Lists, edges, handles and refusals as for plasship_clust_greedy_* (clust.h); max_iterations is --max-iterations (the reference's
 *      default: 1000, mm/commons/Parameters.cpp:2171; it takes values >= 1 only, Parameters.cpp:91: a smaller one is PLASSHIP_ERR_ARG).
 *      The result is a plasship_clusters: plasship_clusters_write / _download / _count, plasship_cands_filter, plasship_clusters_merge and
 *      plasship_clusters_repseqs work on it unchanged.
 *      Set cover (--cluster-mode 0) is not implemented: see clust.h. ---- */
typedef struct plasship_cc_stats {
    uint64_t n_sequences, n_edges;   /* edges: lines / accepted records                                                  */
    uint64_t n_clusters;
    uint64_t n_missing_links;        /* lines whose reverse line is not listed (AlignmentSymmetry::findMissingLinks)     */
    uint32_t n_hook_rounds;          /* hook + pointer-jump rounds until no line joined two trees                        */
    uint32_t n_bfs_levels;           /* levels of the depth guard's breadth-first search                                 */
    float ms_kernel;                 /* line keys .. pair sort (HIP events on the context stream, the per-round reads included) */
} plasship_cc_stats;
int plasship_clust_connected_cands(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, int max_iterations, plasship_clusters **out, plasship_cc_stats *stats);
int plasship_clust_connected_alns(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_alns *a, int max_iterations, plasship_clusters **out, plasship_cc_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* PLASSHIP_EXT_CC_H */
