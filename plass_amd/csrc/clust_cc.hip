// plasship: clust --cluster-mode 1 (connected component) on gfx950.
// Product code, built into the extension library libplasship_cc.so (include/plasship_ext/cc.h).  This is the `clust` call of
// lib/mmseqs/data/workflow/linclust.sh:35,82 when linclust runs with --cluster-mode 1 (single linkage).
//
// Reference behaviour reproduced (file:line in lib/mmseqs/src of the reference):
//   clustering/Clustering.cpp:18-19                    the sequence DB is opened SORT_BY_LENGTH: every "id" of ClusteringAlgorithms is the position in
//                                                      (length descending, key order ascending) — the LENGTH RANK below (lengthRank, clust_shared.hpp)
//   clustering/ClusteringAlgorithms.cpp:345-351        an entry without lines counts 1 ...
//   clustering/AlignmentSymmetry.cpp:45-47             ... and is read as the list of the sequence itself
//   clustering/AlignmentSymmetry.cpp:123-165           findMissingLinks: for every line (set, element) — a line listed twice is taken twice — whose
//                                                      reverse is not in the element's list as read, the element's list grows by one
//   clustering/AlignmentSymmetry.cpp:167-215           addMissingLinks appends exactly those (it looks for the reverse among the lines as read only)
//   clustering/ClusteringAlgorithms.cpp:391-396        clustersizes[] = the symmetric list sizes
//   clustering/ClusteringAlgorithms.cpp:148-180        initClustersizes: a counting sort by size, ids ascending inside a size ...
//   clustering/ClusteringAlgorithms.cpp:83-84          ... read from the back: (size descending, id descending) — the RANK below
//   clustering/ClusteringAlgorithms.cpp:85-110         from every unassigned sequence a breadth-first search: a node taken from the queue has its whole
//                                                      list assigned; a listed node is queued only if it was unassigned and the node's depth is below
//                                                      --max-iterations.  Nodes up to depth max-iterations are expanded, nodes up to max-iterations + 1 assigned
//   clustering/ClusteringAlgorithms.cpp:127-145        (key of the representative, key of the member), sorted as pairs
//
// THE ORDER-FREE STATEMENT.  The lists are symmetric when the search runs.  A later search can therefore take a node x from an earlier one only
// if x was never expanded: an expanded x has assigned all its neighbours, the later start among them.  Unexpanded assigned nodes lie at depth
// max-iterations + 1 exactly, and a node is left for a later search only behind them, at depth max-iterations + 2 or more.  So where the first
// sequence of a component in rank order has every node of the component within max-iterations + 1 steps, its search assigns the whole component
// and no later search starts in it or reaches it: the result is the components, each under its member of smallest rank.  The depth guard below
// checks exactly that condition from all those members at once; where it fails, the call is refused (the reference's answer then depends on the
// order in which its searches steal the nodes at the cut).
//
// Kernel design: everything is a lane per LINE over flat arrays, so a hub with thousands of lines is thousands of lanes like any other lines.
// The accepted lines become 64-bit keys (query id << 32 | target id) and are radix-sorted once; a line's reverse is then one binary search,
// and all later passes stream the sorted keys (8 bytes a line).  Rank: two radix sorts of n keys (lengthRank, then
// ~size << 32 | ~length rank).  Components: parent[] holds ranks; every line hooks the larger of its two roots under the smaller with
// atomicMin, a second kernel makes every parent a root (pointer jumping), and both repeat until no line joined two trees (one 4-byte read a
// round).  parent[] only ever decreases, so there are no cycles, a hook that an atomicMin of another line overwrote is found again in the next
// round, and the root of a finished component is its smallest rank: the representative.  Depth guard: a level-synchronous breadth-first search
// from all representatives, every line tried in both directions, one 8-byte read a level.
// Algorithmic bytes: per line 16 or 64 read once (the record) + 8 written, 16 per sort pass, 8 + a binary search (log2 lines probes of 8, the
// upper levels cached) for the reverse, and per hook round and BFS level 8 + two 4-byte rank reads + the parent / depth reads; per sequence
// 16 per sort pass of the two rank sorts and of the pair sort, 4 per round for the jump.  Unmeasured, see DESIGN.md row C4.
#include "clust_shared.hpp"
#include "../../include/plasship_ext/cc.h"
#include "device_utils.hpp"
#include "host_util.hpp"
#include <algorithm>
#include <cstring>
#include <memory>

namespace plasship {

constexpr uint32_t CC_UNSET = 0xFFFFFFFFu;
constexpr uint64_t CC_NO_LINE = ~0ull;            // a hole of a sparse alignment list: sorts behind every line (ids are below 2^32 - 1)

// stats: [0] lines, [1] lines that name an id outside the DB or lie outside their query's range, [2] missing links, [3] representatives
template <class Rec>
__global__ void ccLineKeyKernel(const uint64_t *__restrict__ qoff, const Rec *__restrict__ recs, uint64_t nRecs, uint32_t n, uint64_t *__restrict__ keys,
                                uint32_t *__restrict__ lines, unsigned long long *stats) {
    int good = 0, bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nRecs; i += (uint64_t) gridDim.x * blockDim.x) {
        uint32_t q, t; uint64_t key = CC_NO_LINE;
        if (lineOf(recs[i], q, t)) {
            if (q >= n || t >= n || i < qoff[q] || i >= qoff[q + 1]) bad++;      // (checked before anything is indexed with them)
            else { key = ((uint64_t) q << 32) | t; atomicAdd(&lines[q], 1u); good++; }
        }
        keys[i] = key;
    }
    good = waveReduceSum(good); bad = waveReduceSum(bad);
    if (laneId() == 0) { if (good) atomicAdd(&stats[0], (unsigned long long) good); if (bad) atomicAdd(&stats[1], (unsigned long long) bad); }
}

// findMissingLinks: line (q, t) without a line (t, q) lengthens t's list by one.  A line to itself is its own reverse.
__global__ void ccMissingKernel(const uint64_t *__restrict__ sorted, uint64_t nLines, uint32_t *__restrict__ missing, unsigned long long *stats) {
    int found = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nLines; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t q = (uint32_t) (sorted[i] >> 32), t = (uint32_t) sorted[i];
        if (q == t) continue;
        const uint64_t want = ((uint64_t) t << 32) | q;
        uint64_t lo = 0, hi = nLines;                     // first key >= want
        while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (sorted[mid] < want) lo = mid + 1; else hi = mid; }
        if (lo == nLines || sorted[lo] != want) { atomicAdd(&missing[t], 1u); found++; }
    }
    found = waveReduceSum(found);
    if (laneId() == 0 && found) atomicAdd(&stats[2], (unsigned long long) found);
}

// sortedLen[lr] names the id of length rank lr; the second key orders by (size descending, length rank descending)
__global__ void ccSizeKeyKernel(const uint64_t *__restrict__ sortedLen, const uint32_t *__restrict__ lines, const uint32_t *__restrict__ missing,
                                uint32_t *__restrict__ idOfLenRank, uint64_t *__restrict__ keys, uint32_t n) {
    for (uint32_t lr = blockIdx.x * blockDim.x + threadIdx.x; lr < n; lr += gridDim.x * blockDim.x) {
        const uint32_t id = (uint32_t) sortedLen[lr];
        const uint32_t size = (lines[id] ? lines[id] : 1u) + missing[id];       // (below 2^32: the lines are fewer than 2^31)
        idOfLenRank[lr] = id;
        keys[lr] = ((uint64_t) ~size << 32) | ~lr;
    }
}
__global__ void ccRankScatterKernel(const uint64_t *__restrict__ sorted, const uint32_t *__restrict__ idOfLenRank, uint32_t *__restrict__ rank,
                                    uint32_t *__restrict__ idOfRank, uint32_t *__restrict__ parent, uint32_t n) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t id = idOfLenRank[~(uint32_t) sorted[r]];
        rank[id] = r; idOfRank[r] = id; parent[r] = r;
    }
}

// parent[x] <= x always, and only ever lowered: every chain ends in a root
__device__ __forceinline__ uint32_t ccRoot(const uint32_t *parent, uint32_t x) {
    for (;;) { const uint32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED); if (p == x) return x; x = p; }
}
__global__ void ccHookKernel(const uint64_t *__restrict__ sorted, uint64_t nLines, const uint32_t *__restrict__ rank, uint32_t *parent, uint32_t *changed) {
    bool any = false;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nLines; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t q = (uint32_t) (sorted[i] >> 32), t = (uint32_t) sorted[i];
        if (q == t) continue;
        const uint32_t a = ccRoot(parent, rank[q]), b = ccRoot(parent, rank[t]);
        if (a != b) { atomicMin(&parent[a > b ? a : b], a > b ? b : a); any = true; }
    }
    if (any) *changed = 1u;                               // (every writer stores the same value)
}
__global__ void ccJumpKernel(uint32_t *parent, uint32_t n) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t root = ccRoot(parent, r);
        if (root != r) __atomic_store_n(&parent[r], root, __ATOMIC_RELAXED);      // (an ancestor of r, below what any hook of this round left here)
    }
}

// the depth guard: level d reaches every unset node next to a node of depth d; flags: [0] a node was reached, [1] one lies deeper than maxDepth
__global__ void ccDepthInitKernel(const uint32_t *__restrict__ parent, uint32_t *__restrict__ depth, uint32_t n) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) depth[r] = parent[r] == r ? 0u : CC_UNSET;
}
__global__ void ccLevelKernel(const uint64_t *__restrict__ sorted, uint64_t nLines, const uint32_t *__restrict__ rank, uint32_t *depth, uint32_t d, uint32_t maxDepth,
                              uint32_t *flags) {
    bool reached = false, deep = false;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nLines; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t q = (uint32_t) (sorted[i] >> 32), t = (uint32_t) sorted[i];
        if (q == t) continue;
        const uint32_t a = rank[q], b = rank[t];
        const uint32_t da = __atomic_load_n(&depth[a], __ATOMIC_RELAXED), db = __atomic_load_n(&depth[b], __ATOMIC_RELAXED);
        const bool toB = da == d && db == CC_UNSET, toA = db == d && da == CC_UNSET;
        if (!toA && !toB) continue;
        if (d >= maxDepth) { deep = true; continue; }
        __atomic_store_n(&depth[toB ? b : a], d + 1u, __ATOMIC_RELAXED);          // (every writer of this level stores d + 1)
        reached = true;
    }
    if (reached) flags[0] = 1u;
    if (deep) flags[1] = 1u;
}

__global__ void ccPairsKernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ idOfRank, uint32_t *__restrict__ repOf,
                              uint64_t *__restrict__ pairs, uint32_t n, unsigned long long *stats) {
    int reps = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t rep = idOfRank[parent[rank[i]]];       // (every parent is a root after the last jump)
        repOf[i] = rep; pairs[i] = ((uint64_t) rep << 32) | i;
        reps += rep == i;
    }
    reps = waveReduceSum(reps);
    if (laneId() == 0 && reps) atomicAdd(&stats[3], (unsigned long long) reps);
}

template <class Rec>
static int clustConnected(plasship_ctx *ctx, const plasship_seqdb *db, const uint64_t *dQoff, const Rec *dRecs, uint64_t nRecs, int maxIterations, plasship_clusters **out,
                          plasship_cc_stats *stats, const char *what) {
    PH_ENTER(ctx);
    if (const int rc = refuseWideIds(what, db)) return rc;
    if (nRecs >= 0x80000000ull) { setError(std::string(what) + ": list sizes are 32-bit (2^31 lines or more)"); return PLASSHIP_ERR_UNSUPPORTED; }
    const uint32_t n = (uint32_t) db->n;
    const uint64_t n1 = std::max<uint32_t>(n, 1), r1 = std::max<uint64_t>(nRecs, 1);
    const uint32_t maxDepth = (uint32_t) std::min<uint64_t>((uint64_t) maxIterations + 1, 0xFFFFFFFEull);
    std::unique_ptr<plasship_clusters> holder(new plasship_clusters());     // released to the caller on success only
    plasship_clusters *cl = holder.get();
    cl->n = n; cl->dbGen = db->gen;
    DevBuf dLineKeys, dLines, dCount, dMissing, dKeys, dSorted, dIdOfLenRank, dRank, dIdOfRank, dParent, dDepth, dFlags, dStats, dPairs;
    if (dLineKeys.alloc(r1 * 8) != hipSuccess || dLines.alloc(r1 * 8) != hipSuccess || dCount.alloc(n1 * 4) != hipSuccess || dMissing.alloc(n1 * 4) != hipSuccess ||
        dKeys.alloc(n1 * 8) != hipSuccess || dSorted.alloc(n1 * 8) != hipSuccess || dIdOfLenRank.alloc(n1 * 4) != hipSuccess || dRank.alloc(n1 * 4) != hipSuccess ||
        dIdOfRank.alloc(n1 * 4) != hipSuccess || dParent.alloc(n1 * 4) != hipSuccess || dDepth.alloc(n1 * 4) != hipSuccess || dFlags.alloc(8) != hipSuccess ||
        dStats.alloc(32) != hipSuccess || dPairs.alloc(n1 * 8) != hipSuccess || cl->d_pairs.alloc(n1 * 8) != hipSuccess || cl->d_repOf.alloc(n1 * 4) != hipSuccess) {
        setError(std::string(what) + ": out of device memory"); return PLASSHIP_ERR_DEVICE;
    }
    unsigned long long hs[4] = {0, 0, 0, 0};
    uint32_t hookRounds = 0, levels = 0;
    PH_CHECK(hipMemsetAsync(dStats.p, 0, 32, ctx->stream));
    PH_CHECK(hipMemsetAsync(dCount.p, 0, n1 * 4, ctx->stream));
    PH_CHECK(hipMemsetAsync(dMissing.p, 0, n1 * 4, ctx->stream));
    PH_CHECK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (n) {
        const unsigned g = flatGrid(n, ctx->numCU);
        uint64_t nLines = 0;
        const uint64_t *lines = dLines.as<uint64_t>();
        // the lines as sorted keys, and how many each sequence lists
        if (nRecs) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(ccLineKeyKernel<Rec>), dim3(flatGrid(nRecs, ctx->numCU)), dim3(256), 0, ctx->stream, dQoff, dRecs, nRecs, n, dLineKeys.as<uint64_t>(),
                               dCount.as<uint32_t>(), dStats.as<unsigned long long>());
            if (const int rc = sortKeysU64(ctx, what, dLineKeys.as<uint64_t>(), dLines.as<uint64_t>(), nRecs)) return rc;
            PH_COPY_SYNC(ctx->stream, hs, dStats.p, 32, hipMemcpyDeviceToHost);
            if (hs[1]) { setError(std::string(what) + ": the list names sequences that are not in the DB"); return PLASSHIP_ERR_ARG; }
            nLines = hs[0];                               // (the holes sorted behind them)
        }
        const unsigned gl = flatGrid(nLines, ctx->numCU);
        if (nLines) hipLaunchKernelGGL(ccMissingKernel, dim3(gl), dim3(256), 0, ctx->stream, lines, nLines, dMissing.as<uint32_t>(), dStats.as<unsigned long long>());
        // the rank: position in the order (symmetric list size descending, length rank descending)
        if (const int rc = lengthRank(ctx, what, db, dKeys.as<uint64_t>(), dSorted.as<uint64_t>())) return rc;
        hipLaunchKernelGGL(ccSizeKeyKernel, dim3(g), dim3(256), 0, ctx->stream, dSorted.as<uint64_t>(), dCount.as<uint32_t>(), dMissing.as<uint32_t>(), dIdOfLenRank.as<uint32_t>(),
                           dKeys.as<uint64_t>(), n);
        if (const int rc = sortKeysU64(ctx, what, dKeys.as<uint64_t>(), dSorted.as<uint64_t>(), n)) return rc;
        hipLaunchKernelGGL(ccRankScatterKernel, dim3(g), dim3(256), 0, ctx->stream, dSorted.as<uint64_t>(), dIdOfLenRank.as<uint32_t>(), dRank.as<uint32_t>(), dIdOfRank.as<uint32_t>(),
                           dParent.as<uint32_t>(), n);
        // the components: hook and jump until no line joined two trees
        for (uint32_t changed = nLines ? 1u : 0u; changed;) {
            PH_CHECK(hipMemsetAsync(dFlags.p, 0, 8, ctx->stream));
            hipLaunchKernelGGL(ccHookKernel, dim3(gl), dim3(256), 0, ctx->stream, lines, nLines, dRank.as<uint32_t>(), dParent.as<uint32_t>(), dFlags.as<uint32_t>());
            hipLaunchKernelGGL(ccJumpKernel, dim3(g), dim3(256), 0, ctx->stream, dParent.as<uint32_t>(), n);
            PH_COPY_SYNC(ctx->stream, &changed, dFlags.p, 4, hipMemcpyDeviceToHost);
            hookRounds++;
        }
        // the depth guard: no node deeper than max-iterations + 1 below its representative
        hipLaunchKernelGGL(ccDepthInitKernel, dim3(g), dim3(256), 0, ctx->stream, dParent.as<uint32_t>(), dDepth.as<uint32_t>(), n);
        for (uint32_t d = 0; nLines; d++) {
            uint32_t flags[2] = {0, 0};
            PH_CHECK(hipMemsetAsync(dFlags.p, 0, 8, ctx->stream));
            hipLaunchKernelGGL(ccLevelKernel, dim3(gl), dim3(256), 0, ctx->stream, lines, nLines, dRank.as<uint32_t>(), dDepth.as<uint32_t>(), d, maxDepth, dFlags.as<uint32_t>());
            PH_COPY_SYNC(ctx->stream, flags, dFlags.p, 8, hipMemcpyDeviceToHost);
            if (flags[1]) {
                setError(std::string(what) + ": a sequence lies more than --max-iterations + 1 = " + std::to_string(maxDepth) + " steps from the first sequence of its component: "
                         "the reference's answer depends on its visiting order there");
                return PLASSHIP_ERR_UNSUPPORTED;
            }
            if (!flags[0]) break;
            levels++;
        }
        hipLaunchKernelGGL(ccPairsKernel, dim3(g), dim3(256), 0, ctx->stream, dParent.as<uint32_t>(), dRank.as<uint32_t>(), dIdOfRank.as<uint32_t>(), cl->d_repOf.as<uint32_t>(),
                           dPairs.as<uint64_t>(), n, dStats.as<unsigned long long>());
        if (const int rc = sortKeysU64(ctx, what, dPairs.as<uint64_t>(), cl->d_pairs.as<uint64_t>(), n)) return rc;
    }
    PH_CHECK(hipEventRecord(ctx->ev[1], ctx->stream));
    PH_CHECK(hipMemcpyAsync(hs, dStats.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    PH_CHECK(plasship::streamSync(ctx->stream));
    PH_CHECK(hipGetLastError());
    cl->nClusters = hs[3];
    if (stats) {
        stats->n_sequences = n; stats->n_edges = hs[0]; stats->n_clusters = hs[3]; stats->n_missing_links = hs[2]; stats->n_hook_rounds = hookRounds; stats->n_bfs_levels = levels;
        float ms = 0; (void) hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); stats->ms_kernel = ms;
    }
    *out = holder.release();
    return PLASSHIP_OK;
}

}  // namespace plasship
using namespace plasship;

static int ccArgs(const plasship_ctx *ctx, int maxIterations, const char *what) {
    if (const int rc = refuseSharded(ctx, what)) return rc;
    // mm/commons/Parameters.cpp:91: --max-iterations matches ^[1-9]{1}[0-9]*$
    if (maxIterations < 1) { setError(std::string(what) + ": max_iterations must be at least 1"); return PLASSHIP_ERR_ARG; }
    return PLASSHIP_OK;
}

extern "C" int plasship_clust_connected_cands(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_cands *c, int max_iterations, plasship_clusters **out,
                                              plasship_cc_stats *stats) {
    const char *what = "plasship_clust_connected_cands";
    if (!ctx || !db || !c || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = ccArgs(ctx, max_iterations, what)) return rc;
    if (const int rc = checkListOnDb(what, db, c)) return rc;
    return clustConnected<CandHit>(ctx, db, c->d_qoff.as<uint64_t>(), c->d_hits.as<CandHit>(), c->nHits, max_iterations, out, stats, what);
}

extern "C" int plasship_clust_connected_alns(plasship_ctx *ctx, const plasship_seqdb *db, const plasship_alns *a, int max_iterations, plasship_clusters **out,
                                             plasship_cc_stats *stats) {
    const char *what = "plasship_clust_connected_alns";
    if (!ctx || !db || !a || !out) { setError(std::string(what) + ": bad argument"); return PLASSHIP_ERR_ARG; }
    if (const int rc = ccArgs(ctx, max_iterations, what)) return rc;
    if (const int rc = checkListOnDb(what, db, a)) return rc;
    return clustConnected<AlnRec>(ctx, db, a->d_qoff.as<uint64_t>(), a->d_recs.as<AlnRec>(), a->nSlots, max_iterations, out, stats, what);
}
