// plasship: what the clustering family shares — clust.hip, clust_cc.hip, merge_clusters.hip, repseqs.hip.  Internal; the definitions and their
// kernels are in clust.hip, that is in libplasship_clust.so, which the other three extension libraries link.
// what: the public call the error texts name.
#pragma once
#include "common.hpp"

namespace plasship {

#ifdef __HIPCC__
// a line of a list: the query and the target it names, false for a line that is none
__device__ __forceinline__ bool lineOf(const CandHit &r, uint32_t &q, uint32_t &t) { q = r.query; t = r.target; return true; }
__device__ __forceinline__ bool lineOf(const AlnRec &r, uint32_t &q, uint32_t &t) { q = r.query; t = r.target; return r.accepted != 0; }   // (a sparse list keeps rejected pairs as holes)
#endif

// ClusteringAlgorithms.cpp:20-23 ("Sequence db size != result db size"), and an alignment list's own DBs
int checkListOnDb(const char *what, const plasship_seqdb *db, const plasship_cands *c);
int checkListOnDb(const char *what, const plasship_seqdb *db, const plasship_alns *a);

// one device radix sort of n 64-bit keys, waited for
int sortKeysU64(plasship_ctx *ctx, const char *what, uint64_t *in, uint64_t *out, uint64_t n);
// SORT_BY_LENGTH (DBReader.cpp:298-315): sortedOut[r] names in its low word the id at place r of (length descending, id ascending); keysTmp: [db->n] too
int lengthRank(plasship_ctx *ctx, const char *what, const plasship_seqdb *db, uint64_t *keysTmp, uint64_t *sortedOut);

// ---- what a PairList's handle answers, whichever module made it ----
int pairListCount(const char *what, const PairList *list, uint64_t *nMembers, uint64_t *nClusters);
int pairListDownload(plasship_ctx *ctx, const char *what, const PairList *list, const plasship_seqdb *db, uint32_t *repKey, uint32_t *memberKey);
// The cluster DB: one entry per run of pairs with one representative, under the representative's key.  repFirst (Clustering::writeData): the
// representative's line first, then the other members' in pair order; without it (mergeclusters) every pair's member in pair order.
int pairListWrite(plasship_ctx *ctx, const char *what, const PairList *list, const plasship_seqdb *db, const char *dbPath, bool repFirst);

}  // namespace plasship
